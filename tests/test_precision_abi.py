"""azg_pv_set_eval_precision / azg_pv_get_eval_precision argument handling (no GPU: the
checks run before any device call; handles are created without a device as in test_abi.py)."""
import ctypes

import pytest

import _native

EXACT, FP16 = 0, 1


def _handle(lib, blocks, ch):
    h = ctypes.c_void_p()
    _native.check(lib.azg_pv_create(ctypes.byref(_native.AzgConfig(blocks, ch, 15, 3)), ctypes.byref(h)), lib)
    return h


@pytest.mark.parametrize("blocks,ch", [(6, 128), (1, 128)])
def test_precision_round_trip(blocks, ch):
    lib = _native.load_library()
    h = _handle(lib, blocks, ch)
    try:
        assert lib.azg_pv_get_eval_precision(h) == EXACT          # the default
        assert lib.azg_pv_set_eval_precision(h, FP16) == 0
        assert lib.azg_pv_get_eval_precision(h) == FP16
        assert lib.azg_pv_set_eval_precision(h, EXACT) == 0
        assert lib.azg_pv_get_eval_precision(h) == EXACT
    finally:
        lib.azg_pv_destroy(h)


def test_precision_is_per_handle():
    lib = _native.load_library()
    a, b = _handle(lib, 2, 128), _handle(lib, 2, 128)
    try:
        assert lib.azg_pv_set_eval_precision(b, FP16) == 0
        assert lib.azg_pv_get_eval_precision(a) == EXACT and lib.azg_pv_get_eval_precision(b) == FP16
    finally:
        lib.azg_pv_destroy(a)
        lib.azg_pv_destroy(b)


def test_null_handle_and_bad_value_are_rejected():
    lib = _native.load_library()
    assert lib.azg_pv_set_eval_precision(None, EXACT) != 0
    assert b"null handle" in lib.azg_pv_last_error()
    assert lib.azg_pv_get_eval_precision(None) == -1
    h = _handle(lib, 6, 128)
    try:
        for bad in (2, -1, 7):
            assert lib.azg_pv_set_eval_precision(h, bad) != 0
            assert b"unknown precision" in lib.azg_pv_last_error()
            assert lib.azg_pv_get_eval_precision(h) == EXACT      # unchanged
    finally:
        lib.azg_pv_destroy(h)


@pytest.mark.parametrize("blocks,ch", [(3, 64), (10, 256), (0, 128)])
def test_fp16_refused_where_there_is_no_kernel(blocks, ch):
    lib = _native.load_library()
    h = _handle(lib, blocks, ch)
    try:
        assert lib.azg_pv_set_eval_precision(h, FP16) != 0
        err = lib.azg_pv_last_error().decode()
        assert "128" in err and "256 and 64" in err, err          # says what is supported and what is out of scope
        assert lib.azg_pv_get_eval_precision(h) == EXACT
        assert lib.azg_pv_set_eval_precision(h, EXACT) == 0       # exact stays available
    finally:
        lib.azg_pv_destroy(h)


def test_model_rejects_unknown_precision_before_device_work():
    from network import PyTorchModel
    with pytest.raises(ValueError, match="exact.*fp16"):
        PyTorchModel(board_size=15, n_res_blocks=2, channels=128, eval_precision="nope")
