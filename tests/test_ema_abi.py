"""azg_pv_bind_ema / azg_pv_get_ema argument handling (no GPU: the function makes no device
call and checks its arguments first; handles are created without a device as in
test_precision_abi.py, and the "device" pointers are never dereferenced)."""
import ctypes
import math
import os

import pytest

import _native
from conftest import REPO

EMA_P, EMA_B, OTHER_P, OTHER_B = 0x1000, 0x2000, 0x3000, 0x4000   # stand-ins for device buffers


def _handle(lib, blocks=2, ch=64):
    h = ctypes.c_void_p()
    _native.check(lib.azg_pv_create(ctypes.byref(_native.AzgConfig(blocks, ch, 15, 3)), ctypes.byref(h)), lib)
    return h


def _state(lib, h):
    """(bound, ema_params, ema_bn, decay) as the handle holds them."""
    p, b, d = ctypes.c_void_p(0xdead), ctypes.c_void_p(0xdead), ctypes.c_float(-1.0)
    bound = lib.azg_pv_get_ema(h, ctypes.byref(p), ctypes.byref(b), ctypes.byref(d))
    return bound, p.value, b.value, d.value


OFF = (0, None, None, 0.0)


def test_exported_declared_and_abi_version_unchanged():
    lib = _native.load_library()
    for name in ("azg_pv_bind_ema", "azg_pv_get_ema"):
        assert name in _native.EXPORTS and hasattr(lib, name)
    assert lib.azg_pv_abi_version() == 3 == _native.ABI_VERSION
    with open(os.path.join(REPO, "include", "azg_pv.h")) as f:
        header = f.read()
    assert "int32_t azg_pv_bind_ema(azg_pv* h, float* ema_params, float* ema_bn, float decay);" in header
    assert "azg_pv_get_ema(const azg_pv* h" in header


def test_off_by_default_and_bind_unbind_bind():
    lib = _native.load_library()
    h = _handle(lib)
    try:
        assert _state(lib, h) == OFF
        assert lib.azg_pv_bind_ema(h, EMA_P, EMA_B, 0.9) == 0
        assert _state(lib, h) == (1, EMA_P, EMA_B, ctypes.c_float(0.9).value)
        assert lib.azg_pv_bind_ema(h, None, None, float("nan")) == 0      # unbind: decay is ignored
        assert _state(lib, h) == OFF
        assert lib.azg_pv_bind_ema(h, OTHER_P, OTHER_B, 0.0) == 0         # decay 0 is allowed: [0, 1)
        assert _state(lib, h) == (1, OTHER_P, OTHER_B, 0.0)
        assert lib.azg_pv_bind_ema(h, EMA_P, EMA_B, 0.999) == 0           # re-bind replaces
        assert _state(lib, h) == (1, EMA_P, EMA_B, ctypes.c_float(0.999).value)
        assert lib.azg_pv_get_ema(h, None, None, None) == 1               # every output is optional
    finally:
        lib.azg_pv_destroy(h)


BAD = [(EMA_P, None, 0.9), (None, EMA_B, 0.9), (EMA_P, EMA_B, 1.0), (EMA_P, EMA_B, 1.5), (EMA_P, EMA_B, -0.01),
       (EMA_P, EMA_B, float("nan")), (EMA_P, EMA_B, float("inf")), (EMA_P, EMA_B, -float("inf")),
       (EMA_P, None, float("nan"))]


@pytest.mark.parametrize("bound_first", [False, True])
def test_refused_calls_leave_the_state_unchanged(bound_first):
    lib = _native.load_library()
    h = _handle(lib, 1, 128)
    try:
        if bound_first:
            assert lib.azg_pv_bind_ema(h, OTHER_P, OTHER_B, 0.5) == 0
        before = _state(lib, h)
        assert before == ((1, OTHER_P, OTHER_B, 0.5) if bound_first else OFF)
        for p, b, d in BAD:
            assert lib.azg_pv_bind_ema(h, p, b, d) != 0, (p, b, d)
            err = lib.azg_pv_last_error().decode()
            assert err.startswith("azg_pv_bind_ema:"), err
            if p and b:
                assert "decay" in err and "[0, 1)" in err, err
            assert _state(lib, h) == before, (p, b, d)
    finally:
        lib.azg_pv_destroy(h)


def test_null_handle():
    lib = _native.load_library()
    assert lib.azg_pv_bind_ema(None, EMA_P, EMA_B, 0.9) != 0
    assert lib.azg_pv_last_error().decode() == "azg_pv_bind_ema: null handle"
    assert lib.azg_pv_bind_ema(None, None, None, 0.9) != 0                # unbinding nothing is refused too
    assert lib.azg_pv_get_ema(None, None, None, None) == -1


def test_binding_is_per_handle():
    lib = _native.load_library()
    a, b = _handle(lib), _handle(lib)
    try:
        assert lib.azg_pv_bind_ema(b, EMA_P, EMA_B, 0.75) == 0
        assert _state(lib, a) == OFF and _state(lib, b) == (1, EMA_P, EMA_B, 0.75)
    finally:
        lib.azg_pv_destroy(a)
        lib.azg_pv_destroy(b)


def test_model_rejects_a_bad_decay_before_device_work():
    from network import PyTorchModel
    for bad in (1.0, -0.5, math.nan):
        with pytest.raises(ValueError, match="ema_decay"):
            PyTorchModel(board_size=15, n_res_blocks=2, channels=64, ema_decay=bad)
