"""Symmetric leaf evaluation, the parts that need no GPU: the host symmetry helpers
against MCTS.symmetries, the new C-ABI entry point's export and argument checks (on a
created, unbound handle: nothing reaches the device), and the Python options' argument
errors."""
import ctypes

import numpy as np
import pytest

import _native
from mcts.new_mcts_alpha import MCTS
from network import (MEAN8_MAX_BOARDS, BoardEvaluator, PyTorchModel, SymmetricModel, apply_symmetry,
                     invert_symmetry, sym_table)

FN = b"azg_pv_forward_boards_sym"


def test_sym_table_is_the_permutation_of_mcts_symmetries():
    t = sym_table()
    assert t.shape == (8, 225) and t.dtype.kind == "i"
    idx = np.arange(225)
    images = MCTS.symmetries(None, idx.reshape(1, 15, 15).astype(np.float32), idx.astype(np.float64))
    assert len(images) == 8
    for s, (state, pi) in enumerate(images):
        assert np.array_equal(pi.astype(np.int64), t[s]), s
        assert np.array_equal(state.reshape(-1).astype(np.int64), t[s]), s
        assert np.array_equal(np.sort(t[s]), idx), s          # a permutation
        assert np.array_equal(apply_symmetry(idx, s), t[s]), s
    assert np.array_equal(t[0], idx)
    assert len({t[s].tobytes() for s in range(8)}) == 8


@pytest.mark.parametrize("s", range(8))
def test_invert_undoes_apply(s):
    rng = np.random.default_rng(s)
    a = rng.integers(0, 3, size=(6, 15, 15)).astype(np.int8)
    img = apply_symmetry(a, s)
    assert img.shape == a.shape and img.dtype == a.dtype
    k, flip = s >> 1, s & 1
    want = np.rot90(a, k, axes=(1, 2))
    want = np.flip(want, axis=2) if flip else want
    assert np.array_equal(img, want)
    assert np.array_equal(invert_symmetry(img, s), a)
    p = rng.random((6, 225)).astype(np.float32)
    assert np.array_equal(invert_symmetry(apply_symmetry(p, s), s), p)
    assert np.array_equal(apply_symmetry(invert_symmetry(p, s), s), p)
    # a result of the image at square j belongs to board square table[s, j]
    assert np.array_equal(invert_symmetry(p, s)[:, sym_table()[s]], p)


def test_helpers_reject_bad_symmetries():
    a = np.zeros((1, 225), np.int8)
    for bad in (-1, 8, 1.5, "mean8", None, True):
        with pytest.raises(ValueError):
            apply_symmetry(a, bad)
        with pytest.raises(ValueError):
            invert_symmetry(a, bad)


def test_entry_point_is_exported_and_abi_is_3():
    lib = _native.load_library()
    assert "azg_pv_forward_boards_sym" in _native.EXPORTS
    assert hasattr(lib, "azg_pv_forward_boards_sym")
    assert lib.azg_pv_abi_version() == 3 == _native.ABI_VERSION


@pytest.fixture()
def unbound():
    lib = _native.load_library()
    h = ctypes.c_void_p()
    _native.check(lib.azg_pv_create(ctypes.byref(_native.AzgConfig(2, 64, 15, 3)), ctypes.byref(h)), lib)
    yield lib, h
    lib.azg_pv_destroy(h)


def test_argument_errors_come_before_the_bound_check(unbound):
    lib, h = unbound
    i8 = (ctypes.c_int8 * 225)()
    f = (ctypes.c_float * 225)()
    p8, pf = ctypes.addressof(i8), ctypes.addressof(f)

    def call(handle=h, boards=p8, players=p8, syms=p8, mode=0, batch=1, probs=pf, values=pf, priors=pf):
        rc = lib.azg_pv_forward_boards_sym(handle, boards, players, syms, mode, batch, probs, values, priors, None)
        return rc, lib.azg_pv_last_error() or b""

    cases = {
        "null handle": (dict(handle=None), b"null handle"),
        "mode 2": (dict(mode=2), b"mode"),
        "mode -1": (dict(mode=-1), b"mode"),
        "mean8 2049": (dict(mode=1, batch=2049, syms=None), b"2048"),
        "negative batch": (dict(batch=-1), b"negative batch"),
        "null boards": (dict(boards=None), b"null"),
        "null players": (dict(players=None), b"null"),
        "null probs": (dict(probs=None), b"null"),
        "null values": (dict(values=None, mode=1), b"null"),
    }
    for name, (kw, text) in cases.items():
        rc, err = call(**kw)
        assert rc != 0, name
        assert FN in err and text in err, (name, err)
        assert b"not bound" not in err, (name, err)
    # a fully valid argument list (syms and priors are optional) reaches the bound check
    for kw in (dict(), dict(syms=None, priors=None), dict(mode=1, batch=2048, syms=None), dict(batch=0)):
        rc, err = call(**kw)
        assert rc != 0 and FN in err and b"not bound" in err, (kw, err)


class _NoDevice:
    """Stands where a PyTorchModel would: the argument checks come before any use of it."""
    engine = None


def test_python_argument_errors_need_no_device():
    with pytest.raises(ValueError, match="2048"):
        BoardEvaluator(_NoDevice(), 4096, symmetry="mean8")
    with pytest.raises(ValueError, match="2048"):
        BoardEvaluator(_NoDevice(), MEAN8_MAX_BOARDS + 1, symmetry="mean8")
    for bad in ("rot", 8, -1, 2.5):
        with pytest.raises(ValueError):
            BoardEvaluator(_NoDevice(), 8, symmetry=bad)
        with pytest.raises(ValueError):
            SymmetricModel(_NoDevice(), bad)
    with pytest.raises(ValueError):
        SymmetricModel(_NoDevice(), None)
    boards, players = np.zeros((3, 225), np.int8), np.ones(3, np.int8)
    for bad in ("random", 8, -1, np.array([0, 1]), np.array([0, 1, 8]), np.array([0.0, 1.0, 2.0])):
        with pytest.raises(ValueError):
            PyTorchModel.predict_boards(_NoDevice(), boards, players, symmetry=bad)


def test_proxy_delegates_and_numbers_its_evaluators():
    class Model:
        board_size, tag = 15, "m"
        made = []

        @staticmethod
        def make_batch_from_states(states):
            return np.stack(states).astype(np.float32)

        def predict_boards(self, boards, players, masked=True, symmetry=None):
            self.made.append((boards.copy(), players.copy(), masked, symmetry))
            return np.zeros((len(boards), 225), np.float32), np.zeros((len(boards), 1), np.float32)

    m = Model()
    proxy = SymmetricModel(m, "random", seed=3)
    assert proxy.board_size == 15 and proxy.tag == "m" and proxy.symmetry == "random"
    proxy.tag = "changed"                    # attributes the proxy does not own are the model's
    assert m.tag == "changed"
    x = np.zeros((4, 3, 15, 15), np.float32)
    x[:, 2] = 1.0
    x[0, 0, 1, 2] = 1.0                      # the side to move's stone -> 1
    x[1, 1, 3, 4] = 1.0                      # the opponent's -> 2
    state = np.random.get_state()[1].copy()
    proxy.predict(x)
    proxy.predict_batch(list(x))
    assert np.array_equal(np.random.get_state()[1], state)      # numpy's global RNG untouched
    (b0, p0, masked0, s0), (b1, _, _, s1) = m.made
    assert b0.dtype == np.int8 and b0.shape == (4, 225) and masked0 is False
    assert b0[0, 17] == 1 and b0[1, 49] == 2 and b0.sum() == 3 and np.array_equal(p0, np.ones(4, np.int8))
    assert s0.shape == (4,) and s0.min() >= 0 and s0.max() <= 7
    again = SymmetricModel(m, "random", seed=3)
    again.predict(x)
    again.predict(x)
    assert np.array_equal(m.made[2][3], s0) and np.array_equal(m.made[3][3], s1)   # seeded: the same draws
    SymmetricModel(m, "mean8").predict(x)
    SymmetricModel(m, 5).predict(x)
    assert m.made[4][3] == "mean8" and m.made[5][3] == 5
