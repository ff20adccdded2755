"""The train step at its smallest batches and the engine at the ends of its depth range,
against the fp64 references.

azg_pv_train_backward takes batch >= 2 and azg_pv_create 0..64 blocks; the other train tests
stop at B = 5 and use 1..10 blocks.  At B <= 3 every one of the 8 weight-grad splits has at
most 3 chunks of 32 pixels (pv_wgrad.h's two-chunks-ahead prologue and the partial last
chunk), M = B x 225 is below one 128-row conv tile at B = 2 and ends in a partial one at
every B here; 0 blocks take the towerless branches of the forward, of heads_bwd_fused and of
the stem backward; 33 blocks are one more than the persistent towers hold (kTowerMaxBlocks),
so every eval forward runs per-layer launches.

Train cases: test_gpu_train_edges.compare_step(small=True) -- per tensor
|g_gpu - g_64| <= max(2e-5 max|g_64| + 1e-8, 2 e32), e32 the error of the same masked
reference run in fp32 on the CPU; the second term for at most two tensors of a case and for
no 3x3 conv weight; losses at rtol 1e-5; the mask-flip rule.  Eval cases:
test_forward_matches_oracle's rule, e_gpu <= max(1e-5, 2 e_cpu32) on probs and values, and
logits_check."""
import functools

import numpy as np
import pytest
import torch

from conftest import has_gpu
from _native import TUNE
from oracle.boards import encode_batch, synth_positions, synth_targets
from oracle.ref_net import RefModel, state_to_numpy
from oracle.value_range import as_fp64, calib_bn
from test_gpu_forward import TOL, logits_check
from test_gpu_train import make_model
from test_gpu_train_edges import backward, check_step, seeded_state

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]


def _lib():
    import _native
    return _native.load_library()


def _train_case(blocks, ch, B):
    b, p = synth_positions(B, seed=277 + B)
    pi, z = synth_targets(B, seed=278 + B)
    return seeded_state(blocks, ch), encode_batch(b, p), pi, z


@pytest.mark.parametrize("blocks,ch,B", [(1, 64, 2), (1, 64, 3), (2, 128, 2), (2, 128, 3), (2, 128, 5), (2, 256, 2),
                                         (0, 64, 2), (0, 64, 16), (0, 128, 5)])
def test_tiny_batches_and_towerless_nets_match_fp64(blocks, ch, B):
    """One train_backward from a seeded init at default keys (split-fp16 forward convs at
    C = 128 / 256, fp32 at C = 64).

    Measured on MI355X -- worst tensor, |g - g_64| / max|g_64|, GPU then the fp32 CPU run
    (bar 2e-5), and the tensors that needed the 2 e32 term:
      1x64  B = 2    4.3e-6 (value_bn.weight)   1.0e-6    none
      1x64  B = 3    1.0e-6                     1.6e-6    none
      2x128 B = 2    1.6e-6                     2.4e-6    none
      2x128 B = 3    7.5e-6 (value_bn.weight)   3.5e-6    none
      2x128 B = 5    1.2e-6                     2.0e-6    none
      2x256 B = 2    1.7e-6                     1.4e-6    none
      0x64  B = 2    5.7e-7                     8.2e-7    none
      0x64  B = 16   7.4e-7                     2.1e-6    none
      0x128 B = 5    7.1e-7                     1.5e-6    none
    (the fp32 CPU run's worst tensor is the stem's conv.weight in most cases; with these
    positions and targets value_fc2.bias at 2x128 B = 3 is 1.5e-6 on the GPU and 2.9e-6 in
    the fp32 CPU run).
    """
    st, x, pi, z = _train_case(blocks, ch, B)
    check_step(f"small {blocks}x{ch} B={B}", st, blocks, ch, x, pi, z, small=True)


def test_33_blocks_train_step_matches_fp64():
    """33x64 at B = 4: one block more than the persistent towers hold; the train step has
    no such limit and runs its 66 convs as at any depth.

    Measured on MI355X -- worst tensor, |g - g_64| / max|g_64| (bar 2e-5):
      GPU 3.1e-4, fp32 CPU run 2.6e-4, both on value_fc2.bias (|g_gpu - g_64| = 1.90e-6,
      e32 = 1.58e-6, max|g_64| = 6.2e-3: a sum of four signed terms that cancel) -- the one
      tensor that needs the 2 e32 term.  Every other tensor: GPU <= 7.9e-6
      (res_blocks.27.bn1.weight), fp32 CPU run <= 7.6e-6; worst 3x3 conv weight 6.1e-6.
    """
    st, x, pi, z = _train_case(33, 64, 4)
    check_step("small 33x64 B=4", st, 33, 64, x, pi, z, small=True)


def test_split_override_shrinks_to_eight_at_two_boards():
    """Key 27 = 64 at 2x128, B = 2: M = 450 pixels are 15 chunks of 32, fewer than two per
    split at any count above 8, so wgrad_splits brings the override down to 8 (one or two
    chunks per split: the prologue's nch > 1 and nch > 2 branches both not taken / taken
    once) while the slabs stay sized for 64.  The step holds the case's tolerance, and its
    gradients (with the skip word) and losses are bitwise those of key 27 = 8 and of the
    automatic count (0: 8 at this shape as well): the slab stride does not enter the sums,
    while an override left at 64 splits over 15 chunks would add the chunks in another order.

    Measured on MI355X:
      worst tensor 1.6e-6 (policy_fc.weight), fp32 CPU run 2.4e-6; no tensor needs 2 e32.
    """
    lib = _lib()
    st, x, pi, z = _train_case(2, 128, 2)
    prev = lib.azg_pv_set_tuning(TUNE.WGRAD_SPLITS, 64)
    try:
        m, _, _, losses = check_step("small 2x128 B=2 key27=64", st, 2, 128, x, pi, z, small=True)
        grads = m.engine.flat_grads_ext.cpu().clone()
        assert bool(grads[:-1].abs().max() > 0)
        for splits in (8, 0):
            lib.azg_pv_set_tuning(TUNE.WGRAD_SPLITS, splits)
            r = make_model(2, 128, st)
            r_losses = backward(r, x, pi, z)
            r_grads = r.engine.flat_grads_ext.cpu().clone()
            nd = int((grads != r_grads).sum())
            print(f"key 27 = 64 against key 27 = {splits}: {nd} of {grads.numel()} gradient words differ")
            assert torch.equal(grads, r_grads), f"key 27 = 64 did not shrink to the 8 splits of key 27 = {splits}"
            assert np.array_equal(losses, r_losses), (losses, r_losses)
    finally:
        lib.azg_pv_set_tuning(TUNE.WGRAD_SPLITS, prev)


# ---------------------------------------------------------------- eval at the depth edges
EVAL_BATCHES = (4, 130)


@functools.lru_cache(maxsize=None)
def _eval_case(blocks, ch):
    """Calibrated seeded net and its fp32 / fp64 CPU forwards on the two batches: computed
    once per net, read only."""
    torch.set_num_threads(8)
    torch.manual_seed(blocks * 1000 + ch + 11)
    ref = RefModel(blocks, ch)
    calib_bn(ref, seed=blocks * 1000 + ch)
    r64 = as_fp64(ref)
    out = {"state": state_to_numpy(ref.net)}
    for B in EVAL_BATCHES:
        b, p = synth_positions(B, seed=B + ch + blocks)
        x = encode_batch(b, p)
        out[B] = (x, ref.predict(x, with_logits=True), r64.predict(x, with_logits=True))
    return out


@pytest.mark.parametrize("arith", [0, 2])
@pytest.mark.parametrize("blocks,ch", [(0, 64), (0, 128), (33, 64), (33, 128)])
def test_eval_forward_at_the_depth_edges(blocks, ch, arith):
    """0 blocks (the towerless forward: the heads read the stem output) and 33 (per-layer
    launches at every batch and key; under key 19 = 2 the 33x128 net cannot run the board
    tower and takes the per-layer split-fp16 convs) at B = 4 and B = 130 (one 128-row tile
    and two boards), under key 19 = 0 and 2."""
    lib = _lib()
    case = _eval_case(blocks, ch)
    m = make_model(blocks, ch, case["state"])
    prev = lib.azg_pv_set_tuning(TUNE.EVAL_ARITH, arith)
    try:
        for B in EVAL_BATCHES:
            x, (p32, v32, l32), (p64, v64, l64) = case[B]
            probs, values = m.predict(x)
            for name, got, r32, r_64 in (("probs", probs, p32, p64), ("values", values, v32, v64)):
                e_gpu, e_cpu = np.abs(got - r_64).max(), np.abs(r32 - r_64).max()
                print(f"{blocks}x{ch} key19={arith} B={B} {name}: |gpu-fp64|={e_gpu:.2e} |cpu32-fp64|={e_cpu:.2e}")
                assert np.all(np.isfinite(got))
                assert e_gpu <= max(TOL, 2 * e_cpu), (name, B, e_gpu, e_cpu)
            logits_check(m, x, l32, l64, f"{blocks}x{ch} key19={arith} B={B}")
        m.engine.check_status()
    finally:
        lib.azg_pv_set_tuning(TUNE.EVAL_ARITH, prev)


@pytest.mark.parametrize("blocks", [0, 33])
def test_fp16_precision_is_refused_beyond_the_board_tower(blocks):
    """eval_precision="fp16" needs the board16 tower (128 channels, 1..32 blocks): a 33x128
    or a 0x128 model refuses it with a ValueError, at construction and from the setter, and
    keeps evaluating in the exact precision."""
    from network import PyTorchModel
    case = _eval_case(blocks, 128)
    with pytest.raises(ValueError, match="not supported"):
        PyTorchModel(board_size=15, device="cuda", n_res_blocks=blocks, channels=128, eval_precision="fp16")
    m = make_model(blocks, 128, case["state"])
    x, _, (p64, v64, _) = case[4]
    p0, v0 = m.predict(x)
    with pytest.raises(ValueError, match="not supported"):
        m.set_eval_precision("fp16")
    assert m.eval_precision == "exact"
    p1, v1 = m.predict(x)
    assert np.array_equal(p0, p1) and np.array_equal(v0, v1)
    m.engine.check_status()
