"""The low-range nets of tests/test_gpu_value_range.py are fair cases, and the activation
exponents folded at pack time repair the split-fp16 arithmetic on them (CPU only).

Fair: the fp32 oracle stays within 5e-6 of the fp64 oracle on probs and values, so a
kernel that misses 1e-5 on such a net has lost precision that plain fp32 keeps.  The
emulation (oracle.value_range.split_forward: operands rounded as the kernels round them,
fp64 accumulation) shows the split several times further from fp64 without the exponents
(past 1e-5 on most cases) and within 1e-5 with the ones oracle.value_range.act_exponents
picks."""
import numpy as np
import pytest
import torch

from conftest import golden_state, load_golden
from oracle.boards import encode_batch, synth_positions
from oracle.ref_net import state_to_numpy
from oracle.value_range import CASES, act_exponents, as_fp64, low_range_net, scale_bn, split_forward

FAIR = 5e-6
TOL = 1e-5
SHAPES = ((2, 128), (1, 256))
# (T, m_b) per case: k lifted back to the dead band's target, T capped by the trunk bound
WANT_EXPS = {("stem", 0): (0, 0), ("stem", 8): (8, 0), ("bn1", 10): (0, 10), ("trunk", 12): (12, 0)}


@pytest.fixture(scope="module")
def boards():
    b, p = synth_positions(16, seed=16)
    return encode_batch(b, p)


@pytest.mark.parametrize("which,k", CASES)
@pytest.mark.parametrize("blocks,ch", SHAPES)
def test_low_range_cases_are_fair_and_the_fold_repairs_the_split(blocks, ch, which, k, boards):
    torch.set_num_threads(8)
    ref = low_range_net(blocks, ch, which, k)
    st = state_to_numpy(ref.net)
    p32, v32 = ref.predict(boards)
    p64, v64 = as_fp64(ref).predict(boards)
    T, ms = act_exponents(st)
    pe, ve = split_forward(st, boards, (T, ms))
    p0, v0 = split_forward(st, boards)
    dev = lambda a, r: float(np.abs(a - r).max())
    print(f"{blocks}x{ch} {which} k={k} T={T} m={ms}: |cpu32-fp64| probs {dev(p32, p64):.2e} values {dev(v32, v64):.2e}; "
          f"emulated split probs {dev(p0, p64):.2e} values {dev(v0, v64):.2e}; "
          f"with the fold probs {dev(pe, p64):.2e} values {dev(ve, v64):.2e}")
    assert dev(p32, p64) <= FAIR and dev(v32, v64) <= FAIR
    assert dev(pe, p64) <= TOL and dev(ve, v64) <= TOL
    if (which, k) in WANT_EXPS:
        wt, wm = WANT_EXPS[(which, k)]
        assert T == wt and ms == [wm] * blocks
    else:   # stem k = 12: T is capped by the bound of the trunk sum, 4 (stem) + 4 per bn2
        assert (which, k) == ("stem", 12) and 0 < T < 12 and ms == [0] * blocks
    if k:   # the gap is real: the exponents lift the operands by >= 2^8, and lo's fixed
        # 2^-25 error falls with them until the fp32 steps of the epilogues are the floor
        assert max(dev(p0, p64), dev(v0, v64)) > 4 * max(dev(pe, p64), dev(ve, v64))
    else:
        assert np.array_equal(p0, pe) and np.array_equal(v0, ve)


def test_ordinary_nets_get_zero_exponents():
    """Seeded, calibrated, trained (the goldens) and overflowing nets are inside the dead
    band: their packed BN parameters, and so every bitwise fixture, stay as they were."""
    for tag in ("3x64", "6x128"):
        assert act_exponents(golden_state(load_golden(tag))) == (0, [0] * int(tag[0]))
    ref = low_range_net(2, 128, "stem", 0)
    assert act_exponents(state_to_numpy(ref.net)) == (0, [0, 0])
    scale_bn(ref.net, "stem", -17)             # gamma x 2^17: the overflow guard's side
    assert act_exponents(state_to_numpy(ref.net)) == (0, [0, 0])
    scale_bn(ref.net, "stem", 17 + 4)          # gamma = 2^-4: bound 0.25, still inside
    assert act_exponents(state_to_numpy(ref.net)) == (0, [0, 0])
    scale_bn(ref.net, "stem", 1)               # first net outside
    assert act_exponents(state_to_numpy(ref.net)) == (5, [0, 0])


def test_calib_bn_keeps_its_old_home():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(__file__), "test_gpu_forward.py")
    spec = importlib.util.spec_from_file_location("_tgf", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from oracle import value_range
    assert mod.calib_bn is value_range.calib_bn
