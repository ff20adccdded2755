"""azg_pv_replay_gather's argument checks (include/azg_pv.h), without a GPU: they run
before any device call, so a bad call returns nonzero with azg_pv_last_error() text
and never touches its pointers (the dummy addresses below are never dereferenced)."""
import pytest

import _native

P = 0x1000   # a non-null stand-in for a device pointer


def _call(lib, stones=P, pis=P, zs=P, cap_pos=4, head=0, count=2, nsym=8, ids=P, batch=16, x=P, pi_out=P, z_out=P):
    return lib.azg_pv_replay_gather(stones, pis, zs, cap_pos, head, count, nsym, ids, batch, x, pi_out, z_out, None)


@pytest.mark.parametrize("bad", [
    dict(stones=None), dict(pis=None), dict(zs=None), dict(ids=None), dict(x=None), dict(pi_out=None),
    dict(z_out=None), dict(nsym=3), dict(nsym=0), dict(batch=0), dict(batch=-1), dict(cap_pos=0),
    dict(count=0), dict(count=5), dict(head=4), dict(head=-1),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_replay_gather_rejects_bad_arguments(bad):
    lib = _native.load_library()
    assert _call(lib, **bad) != 0
    msg = lib.azg_pv_last_error()
    assert msg and b"azg_pv_replay_gather" in msg


def test_abi_version_unchanged():
    assert _native.load_library().azg_pv_abi_version() == 3 == _native.ABI_VERSION
    assert "azg_pv_replay_gather" in _native.EXPORTS
