"""The argument checks of the three weighted-sampling entry points (include/azg_pv.h
azg_pv_replay_surprise_weights, azg_pv_replay_prefix, azg_pv_replay_draw), without a GPU:
they run before any device call, so a bad call returns nonzero with the function named in
azg_pv_last_error() and never touches its pointers (the dummy addresses below are never
dereferenced).  Also the Python restatement's own self-checks, which the GPU tests rely on."""
import os
import re

import pytest

import _native
import replay_weights_reference as ref
from conftest import REPO

P = 0x1000   # a non-null stand-in for a device pointer
NAMES = ("azg_pv_replay_surprise_weights", "azg_pv_replay_prefix", "azg_pv_replay_draw")


def _weights(lib, surprise=P, stride=1, n=3, n_sum=3, mix=0.5, weights=P, cap_pos=4, at=0):
    return lib.azg_pv_replay_surprise_weights(surprise, stride, n, n_sum, mix, weights, cap_pos, at, None)


def _prefix(lib, weights=P, cap_pos=4, head=0, count=2, prefix=P):
    return lib.azg_pv_replay_prefix(weights, cap_pos, head, count, prefix, None)


def _draw(lib, prefix=P, count=2, nsym=8, rnd=P, batch=16, ids=P):
    return lib.azg_pv_replay_draw(prefix, count, nsym, rnd, batch, ids, None)


def _ids(d):
    return "-".join(f"{k}={v}" for k, v in d.items())


def _rejected(call, name, bad):
    lib = _native.load_library()
    assert call(lib, **bad) != 0
    msg = lib.azg_pv_last_error()
    assert msg and name.encode() in msg


@pytest.mark.parametrize("bad", [
    dict(surprise=None), dict(weights=None), dict(mix=-0.01), dict(mix=1.01), dict(mix=float("nan")),
    dict(stride=0), dict(stride=-8), dict(n=0), dict(n=-1), dict(n=5, n_sum=5), dict(n=3, n_sum=2),
    dict(cap_pos=0), dict(at=4), dict(at=-1),
], ids=_ids)
def test_surprise_weights_rejects_bad_arguments(bad):
    _rejected(_weights, NAMES[0], bad)


@pytest.mark.parametrize("bad", [
    dict(weights=None), dict(prefix=None), dict(cap_pos=0), dict(count=0), dict(count=5), dict(head=4),
    dict(head=-1),
], ids=_ids)
def test_prefix_rejects_bad_arguments(bad):
    _rejected(_prefix, NAMES[1], bad)


@pytest.mark.parametrize("bad", [
    dict(prefix=None), dict(rnd=None), dict(ids=None), dict(count=0), dict(count=-1), dict(nsym=0), dict(nsym=3),
    dict(batch=0), dict(batch=-1),
], ids=_ids)
def test_draw_rejects_bad_arguments(bad):
    _rejected(_draw, NAMES[2], bad)


def test_symbols_in_header_and_exports_and_abi_unchanged():
    lib = _native.load_library()
    with open(os.path.join(REPO, "include", "azg_pv.h")) as f:
        header = f.read()
    for name in NAMES:
        assert name in _native.EXPORTS and hasattr(lib, name)
        assert re.search(r"int32_t\s+" + name + r"\s*\(", header), name
    assert lib.azg_pv_abi_version() == 3 == _native.ABI_VERSION


def test_reference_self_checks():
    ref.self_check()
