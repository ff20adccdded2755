"""Pins tests/fp16_emulation.py, the CPU emulation of the one-product fp16 eval precision
(no GPU): on the low-range nets of oracle/value_range.py it is a different arithmetic from
the exact forms (values at least 1e-4 from fp64, where every exact form holds 1e-5), and a
usable one (the masked-policy argmax is fp64's outside near-ties, and near-ties are rare)."""
import functools

import numpy as np
import pytest
import torch

from fp16_emulation import half_forward, near_tie_stats
from oracle.boards import encode_batch, synth_positions
from oracle.ref_net import state_to_numpy
from oracle.value_range import CASES, act_exponents, as_fp64, low_range_net, split_forward

NB = 37


@functools.lru_cache(maxsize=None)
def _case(which, k):
    torch.set_num_threads(8)
    ref = low_range_net(2, 128, which, k)
    boards, players = synth_positions(NB, seed=2 + 128)
    x = encode_batch(boards, players)
    p64, v64 = as_fp64(ref).predict(x)
    return state_to_numpy(ref.net), x, boards, p64, v64


@pytest.mark.parametrize("which,k", CASES)
def test_half_forward_is_a_different_usable_arithmetic(which, k):
    st, x, boards, p64, v64 = _case(which, k)
    pe, ve = half_forward(st, x)
    dp, dv = np.abs(pe - p64).max(), np.abs(ve - v64).max()
    bad, share = near_tie_stats(pe, p64, boards, dp)
    print(f"2x128 {which} k={k}: |emu16-fp64| probs {dp:.2e} values {dv:.2e}, near-tie share {share:.3f}")
    assert dv >= 1e-4, dv                 # not the exact forms' arithmetic (1e-5)
    assert dv <= 2e-2 and dp <= 2e-2      # and not garbage: fp16's 2^-11 through two blocks
    assert bad.size == 0, bad
    assert share <= 1 / 3, share


def test_half_forward_uses_the_activation_fold():
    """half_forward defaults to the library's activation exponents (the mode runs on the
    folded BN parameters): on the stem k = 12 net, whose trunk exponent is nonzero, that is
    the explicit fold and not the unfolded arithmetic, which rounds other operand bits."""
    st, x, _, p64, v64 = _case("stem", 12)
    T, ms = act_exponents(st)
    assert T > 0
    p_fold, v_fold = half_forward(st, x)
    p_exp, v_exp = half_forward(st, x, exps=(T, ms))
    assert np.array_equal(p_fold, p_exp) and np.array_equal(v_fold, v_exp)
    _, v_raw = half_forward(st, x, exps=(0, [0] * len(ms)))
    assert not np.array_equal(v_raw, v_fold)


def test_half_forward_is_split_forward_with_one_product():
    """Same structure as split_forward: they differ by the two correction products only, so
    the split emulation is much closer to fp64 on the same net."""
    st, x, _, p64, v64 = _case("stem", 0)
    _, vs = split_forward(st, x, act_exponents(st))
    _, vh = half_forward(st, x)
    assert np.abs(vs - v64).max() <= 1e-5 < 1e-4 <= np.abs(vh - v64).max()
