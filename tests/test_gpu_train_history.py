"""A handle with a history: one model trains through eight steps of changing batch sizes,
and every step is checked.

The library keeps state from call to call that a fresh model per test never exercises:
  * the train workspace is sized by capacity (128 boards, doubling) and zero-filled once, so
    behind a larger batch every row at or beyond M = B x 225 holds another board's
    activations -- what a conv tile's last partial 128-row tile, a weight-grad chunk, a head
    partial or a BN partial sum reads if it forgets its mask;
  * azg_pv_train_apply re-packs the fp32 conv, dgrad, stem and FC packs and the eval BN fold
    behind Adam; the split-fp16 train packs follow through h3_dirty / h3_gen / wd16_gen and
    the one-product fp16 eval weights through h1_gen;
  * the loss weights of the previous call (LossWeights).

B runs 40, 160, 7, 2, 130, 3, 128, 5: 160 grows the capacity to 256; 7, 2, 3 and 5 run behind
larger batches; 130 and 128 straddle a tile boundary behind small ones.  Weighted and
unweighted calls alternate.  At every step a fresh model is built from a snapshot of the
long-lived one (parameters, BN buffers, counters, Adam moments, step number) and runs the
same call: gradients (with the skip word), losses and BN buffers must be bitwise equal, and
after hip_step on both so must parameters, moments and BN buffers (the step is deterministic
across handles: test_train_schedule_keys_bitwise relies on it).  Steps with B <= 40 are also
held to the fp64 masked reference (test_gpu_train_edges.compare_step, the small-batch rule);
at B >= 128 that reference costs too much CPU time for a test of a few seconds and the
bitwise comparison stands for it.  After steps 2, 5 and 8 the long-lived model, the step's
fresh model and a third model built from the parameters and BN buffers after the step (its
eval packs and BN fold have never been through azg_pv_train_apply: a re-pack that is
consistently one step stale on both trained handles would differ from it) evaluate 5 and
300 boards under key 19 = 0, 1 and 2 (2x128: also in eval_precision "fp16"): bitwise equal.

Five steps have B <= 40 (40, 7, 2, 3, 5), each with one fp64 and one fp32 reference run on
the CPU; the whole test took 2.9 s (2x128) and 0.4 s (1x64) on an MI355X host."""
import numpy as np
import pytest
import torch

from conftest import has_gpu
from _native import TUNE
from oracle.boards import encode_batch, synth_positions, synth_targets
from oracle.ref_net import RefModel, state_to_numpy
from test_gpu_train import make_model
from test_gpu_train_edges import compare_step
from weighted_loss_reference import seeded_weights

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

BATCHES = (40, 160, 7, 2, 130, 3, 128, 5)
EVAL_AFTER = (2, 5, 8)       # 1-based steps
FP64_MAX_B = 40


def _dev(m, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(m.engine.device)


def _backward(m, x, pi, z, wp, wv):
    """One train_backward on m; (losses [3], gradients with the skip word) as host clones."""
    eng = m.engine
    losses = torch.empty(3, device=eng.device)
    eng.train_backward(_dev(m, x), _dev(m, pi), _dev(m, z), losses, _dev(m, wp), _dev(m, wv))
    torch.cuda.synchronize()
    eng.check_status()
    assert eng.train_skips() == 0
    return losses.cpu().clone(), eng.flat_grads_ext.cpu().clone()


def _bn(m):
    return [m.engine.flat_bn.cpu().clone(), m.engine.flat_nbt.cpu().clone()]


def _after_step(m):
    torch.cuda.synchronize()
    return [m.engine.flat_params.cpu().clone(), m.optimizer.flat_exp_avg.cpu().clone(),
            m.optimizer.flat_exp_avg_sq.cpu().clone()] + _bn(m)


def _differing(a, b):
    """Indices at which two lists of host tensors are not bitwise equal (NaNs would count as
    unequal: there are none)."""
    return [i for i, (s, t) in enumerate(zip(a, b)) if not torch.equal(s, t)]


def _eval_all(lib, models, ch, step):
    """predict_boards on 5 and 300 boards under key 19 = 0, 1, 2 (and fp16 precision at
    C = 128) on every model of `models` (the long-lived one first): bitwise equal."""
    prev = lib.azg_pv_set_tuning(TUNE.EVAL_ARITH, 0)
    try:
        for n in (5, 300):
            boards, players = synth_positions(n, seed=500 + 10 * step + n)
            bi8, pl8 = np.asarray(boards, np.int8).reshape(n, 225), np.asarray(players, np.int8)
            modes = [("exact", a) for a in (0, 1, 2)] + ([("fp16", 2)] if ch == 128 else [])
            for prec, arith in modes:
                lib.azg_pv_set_tuning(TUNE.EVAL_ARITH, arith)
                out = []
                for mm in models:
                    mm.set_eval_precision(prec)
                    try:
                        out.append(mm.predict_boards(bi8, pl8))
                    finally:
                        mm.set_eval_precision("exact")
                    mm.engine.check_status()
                pa, va = out[0]
                assert np.all(np.isfinite(pa)) and np.all(np.isfinite(va))
                for k, (pb, vb) in enumerate(out[1:], start=1):
                    assert np.array_equal(pa, pb) and np.array_equal(va, vb), \
                        f"step {step}: eval of {n} boards, key 19 = {arith}, {prec}: the long-lived model differs from model {k}"
    finally:
        lib.azg_pv_set_tuning(TUNE.EVAL_ARITH, prev)


@pytest.mark.parametrize("blocks,ch", [(2, 128), (1, 64)])
def test_every_step_of_a_long_lived_model_is_a_fresh_models_step(blocks, ch):
    """2x128 trains in split-fp16 arithmetic (key 49 = 2, the default), 1x64 on BN = 64
    tiles in fp32.

    Measured on MI355X -- worst tensor of the fp64-checked steps, |g - g_64| / max|g_64|,
    GPU then the fp32 CPU run (bar 2e-5), and the tensors that needed the 2 e32 term:
      2x128  B = 40 (weighted) 2.3e-6 / 7.0e-6, B = 7 (weighted) 9.9e-7 / 5.5e-6, B = 2 1.5e-6 / 1.2e-6,
             B = 3 9.0e-7 / 4.9e-6, B = 5 9.7e-7 / 8.2e-6
      1x64   B = 40 (weighted) 7.9e-7 / 5.7e-6, B = 7 (weighted) 1.0e-6 / 4.3e-6, B = 2 9.9e-7 / 1.2e-6,
             B = 3 1.5e-6 / 6.1e-6, B = 5 1.2e-6 / 4.9e-6
      no tensor needed the 2 e32 term; every bitwise comparison held.
    """
    import _native
    lib = _native.load_library()
    torch.manual_seed(blocks * 1000 + ch + 3)
    m = make_model(blocks, ch, state_to_numpy(RefModel(blocks, ch).net))
    for step, B in enumerate(BATCHES, start=1):
        tag = f"history {blocks}x{ch} step {step} B={B}"
        b, p = synth_positions(B, seed=300 + step)
        x = encode_batch(b, p)
        pi, z = synth_targets(B, seed=400 + step)
        wp, wv = seeded_weights(B, seed=450 + step) if step % 2 == 1 else (None, None)
        # 1, 2: what the step starts from
        torch.cuda.synchronize()
        st = state_to_numpy(m.net)
        ea, es = m.optimizer.flat_exp_avg.clone(), m.optimizer.flat_exp_avg_sq.clone()
        n0 = m.optimizer.get_step()
        assert n0 == step - 1
        # 3: the long-lived model
        losses, grads = _backward(m, x, pi, z, wp, wv)
        bn = _bn(m)
        # 4: a fresh model from the snapshot
        f = make_model(blocks, ch, st)
        f.optimizer.set_step(n0)      # creates the optimizer state (zero moments) first
        with torch.no_grad():
            f.optimizer.flat_exp_avg.copy_(ea)
            f.optimizer.flat_exp_avg_sq.copy_(es)
        f_losses, f_grads = _backward(f, x, pi, z, wp, wv)
        diff = (grads != f_grads)
        print(f"{tag}: losses {losses.tolist()}, {int(diff.sum())} of {grads.numel()} gradient words differ from a fresh model's"
              + (f", max |d| {float((grads - f_grads).abs().max()):.3e}" if bool(diff.any()) else ""))
        assert torch.equal(grads, f_grads), f"{tag}: gradients differ from a fresh model's"
        assert torch.equal(losses, f_losses), (tag, losses, f_losses)
        assert not _differing(bn, _bn(f)), f"{tag}: BN buffers differ from a fresh model's"
        # 5: the fp64 reference under the GPU's masks
        if B <= FP64_MAX_B:
            compare_step(tag, m, st, blocks, ch, x, pi, z, losses.numpy(), wp, wv, small=True)
        # 6: clip + Adam and the re-pack behind it
        m.optimizer.hip_step(m.max_grad_norm)
        f.optimizer.hip_step(f.max_grad_norm)
        bad = _differing(_after_step(m), _after_step(f))
        assert not bad, f"{tag}: after hip_step, parts {bad} of (params, exp_avg, exp_avg_sq, bn, counters) differ"
        assert m.optimizer.get_step() == f.optimizer.get_step() == step
        if step in EVAL_AFTER:
            # f's eval packs and BN fold come from train_apply too: g, built from the
            # parameters and BN buffers after the step, packs them from scratch
            g = make_model(blocks, ch, state_to_numpy(m.net))
            _eval_all(lib, (m, f, g), ch, step)
            g.engine.close()
        f.engine.close()
    assert m.engine.train_recoveries == 0 and m.engine.train_skips() == 0
