"""The argument checks of the two position-averaging entry points (include/azg_pv.h
azg_pv_replay_canon_keys, azg_pv_replay_average), without a GPU: they run before any device
call, so a bad call returns nonzero with the function named in azg_pv_last_error() and never
touches its pointers (the dummy addresses below are never dereferenced)."""
import os
import re

import pytest

import _native
from conftest import REPO

P = 0x1000   # a non-null stand-in for a device pointer
NAMES = ("azg_pv_replay_canon_keys", "azg_pv_replay_average")


def _keys(lib, stones=P, cap_pos=4, head=0, count=2, nsym=8, keys_out=P, syms_out=P):
    return lib.azg_pv_replay_canon_keys(stones, cap_pos, head, count, nsym, keys_out, syms_out, None)


def _average(lib, stones=P, pis=P, zs=P, pw=P, cap_pos=4, head=0, count=2, keys_sorted=P, perm=P, syms=P, pi_avg=P,
             z_avg=P, pw_avg=P, group_first=P, group_size=P):
    return lib.azg_pv_replay_average(stones, pis, zs, pw, cap_pos, head, count, keys_sorted, perm, syms, pi_avg,
                                     z_avg, pw_avg, group_first, group_size, None)


def _ids(d):
    return "-".join(f"{k}={v}" for k, v in d.items())


def _rejected(call, name, bad):
    lib = _native.load_library()
    assert call(lib, **bad) != 0
    msg = lib.azg_pv_last_error()
    assert msg and name.encode() in msg


@pytest.mark.parametrize("bad", [
    dict(stones=None), dict(keys_out=None), dict(syms_out=None), dict(nsym=0), dict(nsym=2), dict(nsym=4),
    dict(nsym=9), dict(nsym=-8), dict(cap_pos=0), dict(count=0), dict(count=-1), dict(count=5), dict(head=4),
    dict(head=-1),
], ids=_ids)
def test_canon_keys_rejects_bad_arguments(bad):
    _rejected(_keys, NAMES[0], bad)


@pytest.mark.parametrize("bad", [
    dict(stones=None), dict(pis=None), dict(zs=None), dict(keys_sorted=None), dict(perm=None), dict(syms=None),
    dict(pi_avg=None), dict(z_avg=None), dict(group_first=None), dict(group_size=None),
    dict(pw=None), dict(pw_avg=None),          # exactly one of the pair
    dict(cap_pos=0), dict(count=0), dict(count=-1), dict(count=5), dict(head=4), dict(head=-1),
    dict(pw=None, pw_avg=None, count=0),       # both null is a valid pair: the next check still runs
], ids=_ids)
def test_average_rejects_bad_arguments(bad):
    _rejected(_average, NAMES[1], bad)


def test_symbols_in_header_and_exports_and_abi_unchanged():
    lib = _native.load_library()
    with open(os.path.join(REPO, "include", "azg_pv.h")) as f:
        header = f.read()
    for name in NAMES:
        assert name in _native.EXPORTS and hasattr(lib, name)
        assert re.search(r"int32_t\s+" + name + r"\s*\(", header), name
    assert lib.azg_pv_abi_version() == 3 == _native.ABI_VERSION
