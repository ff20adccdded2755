"""The entry points that per-example loss weights and playout cap randomization add, without
a GPU: include/azg_pv.h / include/azg_mcts.h, the libraries' exports and the bindings'
EXPORTS agree; the ABI version is still 3 (entry points were only added); bad arguments
return an error that names the function, before any device call (the dummy addresses below
are never dereferenced)."""
import ctypes
import os
import re

import pytest

import _native
import _native_mcts
from conftest import REPO

P = 0x1000   # a non-null stand-in for a device pointer
PV_NAMES = ("azg_pv_train_backward_weighted", "azg_pv_replay_gather_weight")
MCTS_NAMES = ("azg_mcts_set_budget",)


def _declared(header, prefix):
    with open(os.path.join(REPO, "include", header)) as f:
        txt = f.read()
    return set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\*?\s+\**(" + prefix + r"[a-z_0-9]+)\s*\(", txt, re.M))


def test_header_library_and_bindings_agree_for_both_libraries():
    for header, prefix, mod, names in (("azg_pv.h", "azg_pv_", _native, PV_NAMES),
                                       ("azg_mcts.h", "azg_mcts_", _native_mcts, MCTS_NAMES)):
        declared = _declared(header, prefix)
        assert declared == set(mod.EXPORTS)
        lib = mod.load_library()
        for name in declared:
            assert hasattr(lib, name), name
        for name in names:
            assert name in declared, name


def test_abi_version_is_still_3():
    assert _native.load_library().azg_pv_abi_version() == 3 == _native.ABI_VERSION


def _handle(lib):
    h = ctypes.c_void_p()
    _native.check(lib.azg_pv_create(ctypes.byref(_native.AzgConfig(1, 64, 15, 3)), ctypes.byref(h)), lib)
    return h


def test_train_backward_weighted_rejects_bad_arguments():
    lib = _native.load_library()
    name = b"azg_pv_train_backward_weighted"
    assert lib.azg_pv_train_backward_weighted(None, P, P, P, P, P, 8, P, None) != 0
    assert name in lib.azg_pv_last_error() and b"null handle" in lib.azg_pv_last_error()
    h = _handle(lib)
    try:
        for batch in (0, -3, 1):
            assert lib.azg_pv_train_backward_weighted(h, P, P, P, P, P, batch, P, None) != 0
            assert name in lib.azg_pv_last_error() and b"batch" in lib.azg_pv_last_error()
        for i in (1, 2, 3, 7):     # x, pis, zs, losses; the weights (4, 5) may be null
            a = [h, P, P, P, None, None, 8, P, None]
            a[i] = None
            assert lib.azg_pv_train_backward_weighted(*a) != 0
            assert name in lib.azg_pv_last_error() and b"null argument" in lib.azg_pv_last_error()
        # a handle nothing was bound to cannot train
        assert lib.azg_pv_train_backward_weighted(h, P, P, P, None, None, 8, P, None) != 0
        assert name in lib.azg_pv_last_error() and b"not bound" in lib.azg_pv_last_error()
    finally:
        lib.azg_pv_destroy(h)


@pytest.mark.parametrize("bad", [dict(vals=None), dict(ids=None), dict(out=None), dict(cap_pos=0), dict(head=4),
                                 dict(head=-1), dict(count=0), dict(count=5), dict(nsym=3), dict(nsym=0),
                                 dict(batch=0), dict(batch=-1)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_replay_gather_weight_rejects_bad_arguments(bad):
    lib = _native.load_library()
    a = dict(vals=P, cap_pos=4, head=0, count=2, nsym=8, ids=P, batch=1, out=P)
    a.update(bad)
    assert lib.azg_pv_replay_gather_weight(a["vals"], a["cap_pos"], a["head"], a["count"], a["nsym"], a["ids"],
                                           a["batch"], a["out"], None) != 0
    assert b"azg_pv_replay_gather_weight" in lib.azg_pv_last_error()


def test_set_budget_rejects_bad_arguments_and_keeps_the_config_layout():
    lib = _native_mcts.load_library()
    assert lib.azg_mcts_set_budget(None, 0, 4, 0) != 0
    assert b"azg_mcts_set_budget" in lib.azg_mcts_last_error()
    f = _native_mcts.SearchForest(2, 8)
    for g in (-1, 2):
        with pytest.raises(RuntimeError, match="azg_mcts_set_budget"):
            f.set_budget(g, 4, 0)
    f.set_budget(1, 4, 0)
    f.set_budget(1)          # back to the forest's own
    # azg_mcts_config: six int32 and three doubles, as before
    assert ctypes.sizeof(_native_mcts.MctsConfig) == 48
    assert [n for n, _ in _native_mcts.MctsConfig._fields_] == [
        "rules", "board", "n_simulations", "batch_size", "apply_dirichlet_n_first_moves", "add_dirichlet_noise",
        "cpuct", "dirichlet_alpha", "epsilon"]
