"""Per-example loss weights in the train step (azg_pv_train_backward_weighted,
train_batch(policy_weight=, value_weight=)):

    policy_loss = (1/B) sum_b wp_b KL_b,   value_loss = (1/B) sum_b wv_b (v_b - z_b)^2

Nets 1x64 and 2x128 at B = 5 and B = 37 (neither a multiple of the loss kernel's 4 boards
per workgroup: the last workgroup is partial) plus the golden 3x64 net.  The fp64 reference
is tests/weighted_loss_reference.py; the bars are test_gradients_match_oracle's.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import golden_state, has_gpu, load_golden
from _native import TUNE
from oracle.boards import encode_batch, synth_positions, synth_targets
from oracle.ref_net import RefModel, state_to_numpy
from test_gpu_train import _full_state, _overflow_model, gpu_masks, make_model
from weighted_loss_reference import POLICY_HEAD, VALUE_HEAD, seeded_weights, weighted_masked_grads_fp64

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

CASES = [(None, 1, 64, 5), (None, 1, 64, 37), (None, 2, 128, 5), (None, 2, 128, 37), ("3x64", 3, 64, 37)]
case = pytest.mark.parametrize("tag,blocks,ch,B", CASES)


@functools.lru_cache(maxsize=None)
def _data(tag, blocks, ch, B):
    """(state, x, pi, z, wp, wv) of a case: computed once, never written."""
    if tag is None:
        torch.manual_seed(blocks * 1000 + ch)
        st = state_to_numpy(RefModel(blocks, ch).net)
    else:
        st = golden_state(load_golden(tag))
    b, p = synth_positions(B, seed=177 + B)
    x = encode_batch(b, p)
    pi, z = synth_targets(B, seed=178 + B)
    wp, wv = seeded_weights(B, seed=179 + B + ch)
    for a in (x, pi, z, wp, wv):
        a.setflags(write=False)
    return st, x, pi, z, wp, wv


def _dev(m, a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float32)).to(m.engine.device)


def _backward(tag, blocks, ch, B, wp, wv, step=False, weighted=True):
    """One train_backward on a fresh model of the case; (model, grads {name: fp32 ndarray},
    losses [3]).  weighted=False: the plain entry point.  step: one hip_step after it, whose
    parameters come back as a fourth element."""
    st, x, pi, z, _, _ = _data(tag, blocks, ch, B)
    m = make_model(blocks, ch, st)
    eng = m.engine
    losses = torch.empty(3, device=eng.device)
    if weighted:
        eng.train_backward(_dev(m, x), _dev(m, pi), _dev(m, z), losses, _dev(m, wp), _dev(m, wv))
    else:
        eng.train_backward(_dev(m, x), _dev(m, pi), _dev(m, z), losses)
    torch.cuda.synchronize()
    eng.check_status()
    grads = {n: q.grad.detach().cpu().numpy().copy() for n, q in m.net.named_parameters()}
    out = (m, grads, losses.cpu().numpy().copy())
    if step:
        m.optimizer.hip_step(m.max_grad_norm)
        torch.cuda.synchronize()
        out += ([t.detach().cpu().clone() for t in m.net.state_dict().values()],)
    return out


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@case
def test_weighted_gradients_match_fp64(tag, blocks, ch, B):
    """Gradients and losses vs the fp64 weighted loss with the GPU's own ReLU masks:
    |g_gpu - g_64| <= 2e-5 max|g_64| + 1e-8 per tensor, losses rtol 1e-5 / atol 1e-7."""
    st, x, pi, z, wp, wv = _data(tag, blocks, ch, B)
    assert wp[0] == 0 and wv[0] == 0 and set(wp) == set(wv) == {0.0, 0.25, 1.0, 3.0} and not np.array_equal(wp, wv)
    m, grads, losses = _backward(tag, blocks, ch, B, wp, wv)
    mk = gpu_masks(m.engine, blocks, B)
    want, (pl, vl) = weighted_masked_grads_fp64(st, blocks, ch, x, pi, z, mk, wp, wv)
    print(f"losses gpu {losses.tolist()} fp64 {[pl, vl, pl + vl]}")
    bad = []
    for n, w in want.items():
        err, scale = np.abs(grads[n].astype(np.float64) - w).max(), np.abs(w).max()
        print(f"{tag} {blocks}x{ch} B={B} {n:28s} |gpu-64|={err:.2e} max|g|={scale:.2e} rel={err / (scale + 1e-30):.1e}")
        if err > 2e-5 * scale + 1e-8:
            bad.append(n)
    np.testing.assert_allclose(losses, [pl, vl, pl + vl], rtol=1e-5, atol=1e-7)
    assert not bad, bad


@case
def test_weights_of_one_are_the_unweighted_step_bitwise(tag, blocks, ch, B):
    """Ones passed explicitly -- for both heads, or for one with the other pointer NULL --
    give the unweighted call's gradients, losses and, after one hip_step, parameters and BN
    buffers, bit for bit."""
    ones = np.ones(B, np.float32)
    _, g0, l0, p0 = _backward(tag, blocks, ch, B, None, None, step=True, weighted=False)
    for wp, wv in ((ones, ones), (ones, None), (None, ones)):
        _, g, l, p = _backward(tag, blocks, ch, B, wp, wv, step=True)
        assert _bits_equal(l, l0), (l, l0)
        for n in g0:
            assert _bits_equal(g[n], g0[n]), n
        assert all(torch.equal(a, c) for a, c in zip(p, p0))


@case
def test_zero_weights_switch_one_head_off(tag, blocks, ch, B):
    """All policy weights 0: policy_loss == 0, the gradients of policy_fc, policy_conv and
    policy_bn are exactly zero, and the value-side head gradients are the unweighted step's
    bits.  The same with the two heads' roles swapped."""
    zeros = np.zeros(B, np.float32)
    _, g0, l0 = _backward(tag, blocks, ch, B, None, None, weighted=False)
    for wp, wv, off, on, li_off, li_on in ((zeros, None, POLICY_HEAD, VALUE_HEAD, 0, 1),
                                           (None, zeros, VALUE_HEAD, POLICY_HEAD, 1, 0)):
        _, g, l = _backward(tag, blocks, ch, B, wp, wv)
        assert l[li_off] == 0.0, l
        assert _bits_equal(l[li_on:li_on + 1], l0[li_on:li_on + 1]) and l[2] == l[li_on], (l, l0)
        seen_off = seen_on = 0
        for n in g0:
            if n.startswith(off):
                seen_off += 1
                assert not g[n].any(), (n, np.abs(g[n]).max())
            elif n.startswith(on):
                seen_on += 1
                assert _bits_equal(g[n], g0[n]), n
        assert seen_off >= 5 and seen_on >= 5, (seen_off, seen_on)


@case
def test_doubled_weights_double_every_gradient_bitwise(tag, blocks, ch, B):
    """Every weight of both heads times two: every gradient element with |g| >= 2^-100 is
    exactly twice what it was (a power of two scales the seeds exactly, and everything
    behind them is linear in them)."""
    _, _, _, _, wp, wv = _data(tag, blocks, ch, B)
    _, g1, l1 = _backward(tag, blocks, ch, B, wp, wv)
    _, g2, l2 = _backward(tag, blocks, ch, B, 2 * wp, 2 * wv)
    bad = {}
    for n, a in g1.items():
        big = np.abs(a) >= 2.0 ** -100
        ne = (2 * a != g2[n]) & big
        if ne.any():
            bad[n] = (int(ne.sum()), int(big.sum()))
    assert not bad, bad
    assert _bits_equal(2 * l1[:2], l2[:2]), (l1, l2)


def test_skipped_weighted_step_is_redone_with_its_weights():
    """test_train_h3_range_overflow_is_redone_in_fp32's setup with weights: the step
    train_batch_device redoes after the device skipped it is the key-49 = 0 WEIGHTED step,
    bitwise (params, moments, BN buffers, counters, Adam step), and not the unweighted one."""
    import _native
    lib = _native.load_library()
    b, p = synth_positions(32, seed=91)
    x = encode_batch(b, p)
    pi, z = synth_targets(32, seed=92)
    wp, wv = seeded_weights(32, seed=93)
    prev = lib.azg_pv_set_tuning(TUNE.TRAIN_ARITH, 2)
    try:
        m = _overflow_model()
        args = lambda mm: [_dev(mm, a) for a in (x, pi, z.reshape(-1, 1))]
        got = m.train_batch_device(*args(m), policy_weight=_dev(m, wp), value_weight=_dev(m, wv))
        assert all(np.isfinite(v) for v in got.values()), got
        assert m.engine.train_recoveries == 1 and m.engine.train_skips() == 1
        lib.azg_pv_set_tuning(TUNE.TRAIN_ARITH, 0)
        r = _overflow_model()
        want = r.train_batch_device(*args(r), policy_weight=_dev(r, wp), value_weight=_dev(r, wv))
        u = _overflow_model()
        plain = u.train_batch_device(*args(u))
        lib.azg_pv_set_tuning(TUNE.TRAIN_ARITH, 2)
        assert r.engine.train_recoveries == 0
        assert got == want, (got, want)
        assert got != plain, (got, plain)
        assert all(torch.equal(a, c) for a, c in zip(_full_state(m), _full_state(r))), "redo != key-49 = 0 weighted step"
        m.engine.clear_status()
    finally:
        lib.azg_pv_set_tuning(TUNE.TRAIN_ARITH, prev)


def test_train_batch_checks_host_weights_and_device_tensors():
    """Host arrays are validated (length, finite, >= 0); device tensors for dtype, shape and
    device only; train_batch with host weights equals train_batch_device with the same
    weights on the device."""
    tag, blocks, ch, B = CASES[0]
    st, x, pi, z, wp, wv = _data(tag, blocks, ch, B)
    m = make_model(blocks, ch, st)
    for bad in (np.ones(B + 1, np.float32), np.full(B, np.nan, np.float32), np.full(B, np.inf, np.float32),
                -np.ones(B, np.float32)):
        with pytest.raises(ValueError):
            m.train_batch(x, pi, z, policy_weight=bad)
        with pytest.raises(ValueError):
            m.train_batch(x, pi, z, value_weight=bad)
    dev = m.engine.device
    for bad in (torch.ones(B, dtype=torch.float64, device=dev), torch.ones(B + 1, device=dev),
                torch.ones((B, 2), device=dev)):
        with pytest.raises(ValueError):
            m.train_batch_device(_dev(m, x), _dev(m, pi), _dev(m, z), policy_weight=bad)
    before = _full_state(m)
    got = m.train_batch(x, pi, z, policy_weight=wp, value_weight=wv.reshape(B, 1))
    assert not all(torch.equal(a, c) for a, c in zip(before, _full_state(m)))
    r = make_model(blocks, ch, st)
    want = r.train_batch_device(_dev(r, x), _dev(r, pi), _dev(r, z), policy_weight=_dev(r, wp).reshape(B, 1),
                                value_weight=_dev(r, wv))
    assert got == want
    assert all(torch.equal(a, c) for a, c in zip(_full_state(m), _full_state(r)))
