"""The train step at the edges of its value range (azg_pv_train_backward at default keys).

heads_loss_kernel and the train BN have code for targets with zeros, rows that do not sum
to 1, logits far enough apart that expf underflows, a tanh of exactly +-1 and channels of
zero variance; the dense O(1) cases of tests/test_gpu_train.py reach none of it.
Reference and tolerances are that file's: fp64 autograd with the GPU's own ReLU masks
(oracle.masked_grads_fp64), |g_gpu - g_64| <= 2e-5 max|g_64| + 1e-8 per tensor, losses at
rtol 1e-5, every mask flip at |pre-activation| <= max(1e-6 x the layer's max, 2 x the GPU's
own error on the layer)."""
import numpy as np
import pytest
import torch

from conftest import has_gpu
from _native import TUNE
from oracle.boards import encode_batch, synth_positions, synth_targets, valid_mask
from oracle.ref_net import RefModel, masked_grads_fp64, state_to_numpy
from oracle.value_range import low_range_net
from test_gpu_train import gpu_masks, make_model, mask_flips
from weighted_loss_reference import weighted_masked_grads_fp64

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]


def seeded_state(blocks, ch):
    torch.manual_seed(blocks * 1000 + ch)
    return state_to_numpy(RefModel(blocks, ch).net)


def positions(B):
    b, p = synth_positions(B, seed=177 + B)
    return b, encode_batch(b, p)


def edge_targets(boards, seed=5):
    """Rows cycle through: one-hot; legal-mask style (zero on every stone, renormalised);
    all-zero; summing to 0.5.  z cycles through -1, 0, 1."""
    B = len(boards)
    rng = np.random.default_rng(seed)
    pi = np.zeros((B, 225), np.float32)
    for i, b in enumerate(boards):
        legal = valid_mask(b)
        kind = i % 4
        if kind == 0:
            pi[i, rng.choice(np.nonzero(legal)[0])] = 1.0
        elif kind == 1:
            r = rng.random(225).astype(np.float32) * legal
            pi[i] = r / r.sum()
        elif kind == 3:
            r = rng.random(225).astype(np.float32) * legal
            pi[i] = 0.5 * r / r.sum()
    z = (np.arange(B) % 3 - 1).astype(np.float32).reshape(B, 1)
    return pi, z


def backward(m, x, pi, z, wp=None, wv=None):
    """One azg_pv_train_backward (the weighted entry point with wp / wv, host arrays [B]);
    returns the losses (policy, value, total)."""
    eng = m.engine
    dev = eng.device
    losses = torch.empty(3, device=dev)
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    eng.train_backward(to(x), to(pi), to(z), losses, to(wp), to(wv))
    torch.cuda.synchronize()
    eng.check_status()
    assert eng.train_skips() == 0
    return losses.cpu().numpy()


def is_conv3x3(n):
    """True for the name of a 3x3 conv weight tensor (the stem's and the residual blocks')."""
    return n == "conv.weight" or (n.startswith("res_blocks.") and n.endswith(".weight") and ".conv" in n)


def compare_step(tag, m, st, blocks, ch, x, pi, z, losses, wp=None, wv=None, small=False):
    """The gradients m's last train_backward left (from state st, on x / pi / z and the loss
    weights wp / wv) against the fp64 masked reference, at the tolerances of
    test_gradients_match_oracle: per tensor |g_gpu - g_64| <= 2e-5 max|g_64| + 1e-8, losses
    at rtol 1e-5, every mask flip at |pre-activation| <= max(1e-6 x the layer's max, 2 x the
    GPU's own error on the layer).

    small (batches of a few boards, where a correct fp32 implementation cannot always hold
    the per-tensor bar: a scalar gradient is a sum of a few signed terms that cancel): the
    bound is max(2e-5 max|g_64| + 1e-8, 2 e32), e32 the error of the same reference run in
    fp32 on the CPU under the same masks -- for at most two tensors of the step and for no
    3x3 conv weight; the tensors that needed the second term are printed.

    Returns (GPU grads, fp64 grads, figures): figures = {"gpu": worst |g_gpu - g_64| /
    max|g_64| over the tensors, "cpu32": the same of the fp32 CPU run (small only),
    "needed": the tensors that needed 2 e32}."""
    torch.set_num_threads(8)
    B = len(x)
    eng = m.engine
    mk = gpu_masks(eng, blocks, B)
    if wp is None and wv is None:
        ref = lambda **kw: masked_grads_fp64(st, blocks, ch, x, pi, z, mk, **kw)
    else:
        ref = lambda **kw: weighted_masked_grads_fp64(st, blocks, ch, x, pi, z, mk, wp, wv, **kw)
    want, (pl, vl), pre = ref(return_pre=True)
    want32 = ref(dtype=torch.float32)[0] if small else None
    print(f"{tag}: losses gpu {losses.tolist()} fp64 {[pl, vl, pl + vl]}")
    assert np.all(np.isfinite(losses))
    nchw = lambda t: t.permute(0, 3, 1, 2).double().cpu().numpy()
    gpu_pre = {"a0": nchw(eng.debug_tensor("a0", B))}
    for i in range(blocks):
        gpu_pre[f"h{i}"] = nchw(eng.debug_tensor("h", B, i))
        gpu_pre[f"xo{i}"] = nchw(eng.debug_tensor("xo", B, i))
    for n_ in ("fp", "fv", "hv"):
        gpu_pre[n_] = eng.debug_tensor(n_, B).double().cpu().numpy()
    for k, (n, worst, mx) in mask_flips(mk, pre).items():
        err = float(np.abs(gpu_pre[k] - np.maximum(pre[k], 0)).max())
        if n:
            print(f"{tag}: mask flips {k}: {n} (worst |pre| {worst:.2e} = {worst / mx:.1e} x max), gpu max err {err:.2e}")
        assert worst <= max(1e-6 * mx, 2 * err), (k, n, worst, mx, err)
    got, bad, needed = {}, [], []   # every figure is printed before the first assertion on it
    fig = {"gpu": (0.0, None), "cpu32": (0.0, None)}
    for n, prm in m.net.named_parameters():
        gg = prm.grad.detach().cpu().numpy().astype(np.float64)
        got[n] = gg
        assert np.all(np.isfinite(gg)), n
        err, scale = np.abs(gg - want[n]).max(), np.abs(want[n]).max()
        e32 = float(np.abs(want32[n].astype(np.float64) - want[n]).max()) if small else 0.0
        rel, rel32 = err / (scale + 1e-30), e32 / (scale + 1e-30)
        print(f"{tag} {n:28s} |gpu-64|={err:.2e} max|g|={scale:.2e} rel={rel:.1e}"
              + (f" |cpu32-64|={e32:.2e} rel32={rel32:.1e}" if small else ""))
        if scale > 0 and rel > fig["gpu"][0]:
            fig["gpu"] = (float(rel), n)
        if scale > 0 and rel32 > fig["cpu32"][0]:
            fig["cpu32"] = (float(rel32), n)
        if err > 2e-5 * scale + 1e-8:
            if small and err <= 2 * e32:
                needed.append((n, float(err), float(e32), float(scale)))
            else:
                bad.append((n, float(err), float(e32), float(scale)))
    fig["needed"] = [t[0] for t in needed]
    print(f"{tag} SUMMARY worst gpu rel {fig['gpu'][0]:.1e} ({fig['gpu'][1]})"
          + (f", worst cpu32 rel {fig['cpu32'][0]:.1e} ({fig['cpu32'][1]}), needed 2 x e32: {needed}" if small else ""))
    np.testing.assert_allclose(losses, [pl, vl, pl + vl], rtol=1e-5, atol=1e-7)
    assert not bad, bad
    assert len(needed) <= 2, needed
    assert not [t for t in needed if is_conv3x3(t[0])], needed
    return got, want, fig


def check_step(tag, st, blocks, ch, x, pi, z, m=None, small=False):
    """train_backward on state st against the fp64 masked reference (compare_step).
    Returns (model, GPU grads, fp64 grads, GPU losses)."""
    m = m or make_model(blocks, ch, st)
    losses = backward(m, x, pi, z)
    got, want, _ = compare_step(tag, m, st, blocks, ch, x, pi, z, losses, small=small)
    return m, got, want, losses


POLICY_SIDE = ("policy_conv.weight", "policy_bn.weight", "policy_bn.bias", "policy_fc.weight", "policy_fc.bias")
VALUE_SIDE = ("value_conv.weight", "value_bn.weight", "value_bn.bias", "value_fc1.weight", "value_fc1.bias",
              "value_fc2.weight", "value_fc2.bias")


@pytest.mark.parametrize("B", [5, 37])
def test_sparse_and_unnormalised_targets(B):
    """One-hot, legal-mask, all-zero and half-mass pi rows in one batch (the tv > 0 guard
    of the KL term and the sum-of-targets factor of dlogits), z in {-1, 0, 1}; B = 5 and
    37 end in a partly filled four-boards-per-workgroup group of heads_loss_kernel."""
    boards, x = positions(B)
    pi, z = edge_targets(boards)
    assert (pi == 0).mean() > 0.5 and set(np.round(pi.sum(1), 3)) == {0.0, 0.5, 1.0}
    check_step(f"targets B={B}", seeded_state(1, 64), 1, 64, x, pi, z)


@pytest.mark.parametrize("B", [5, 37])
def test_all_zero_targets_give_exactly_zero_dlogits(B):
    """Every pi row zero: dlogits = (softmax x 0 - 0) / B is exactly 0 on every row, so the
    policy loss and every gradient of the policy head are exactly 0 (the trunk's gradients
    are the value head's alone, checked against the reference)."""
    boards, x = positions(B)
    _, z = edge_targets(boards)
    pi = np.zeros((B, 225), np.float32)
    _, got, _, losses = check_step(f"zero pi B={B}", seeded_state(1, 64), 1, 64, x, pi, z)
    assert losses[0] == 0.0
    for n in POLICY_SIDE:
        assert not got[n].any(), n


@pytest.mark.parametrize("B", [5, 37])
def test_peaked_logits(B):
    """policy_fc.weight scaled until the logit spread passes 100: expf(lg - max) underflows
    to 0 on most actions, the max-subtraction keeps the log-softmax finite."""
    st = seeded_state(1, 64)
    boards, x = positions(B)
    pi, z = synth_targets(B, seed=78 + B)
    ref = RefModel(1, 64)
    ref.net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    ref.net.train()
    with torch.no_grad():
        lg, _ = ref.net(torch.from_numpy(x))
    spread = float((lg.max(1).values - lg.min(1).values).min())
    st["policy_fc.weight"] = st["policy_fc.weight"] * np.float32(2.0 ** np.ceil(np.log2(150.0 / spread)))
    with torch.no_grad():
        ref.net.policy_fc.weight.copy_(torch.from_numpy(st["policy_fc.weight"]))
        lg, _ = ref.net(torch.from_numpy(x))
    assert float((lg.max(1).values - lg.min(1).values).min()) > 100.0
    check_step(f"peaked B={B}", st, 1, 64, x, pi, z)


def _value_pre(st, x):
    """fp32 oracle's train-mode value pre-activation (value_fc2's output, before tanh) per board."""
    ref = RefModel(1, 64)
    ref.net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in st.items()})
    ref.net.train()
    out = []
    hook = ref.net.value_fc2.register_forward_hook(lambda mod, a, r: out.append(r.detach().double().numpy().reshape(-1)))
    with torch.no_grad():
        ref.net(torch.from_numpy(x))
    hook.remove()
    return out[0]


@pytest.mark.parametrize("B", [5, 37])
def test_saturated_value_head(B):
    """value_fc2.weight scaled so tanhf returns +-1.0f exactly, z of the opposite sign.
    Mixed batch (most boards saturated): losses and gradients match the reference, whose
    1 - v^2 is below 1e-15 there.  Every board saturated: the value loss is exactly 4,
    dpre = 2 (v - z) / B x (1 - v^2) is exactly 0 on every row and with it every gradient
    of the value head."""
    st = seeded_state(1, 64)
    boards, x = positions(B)
    pi, _ = synth_targets(B, seed=78 + B)
    pre0 = np.abs(_value_pre(st, x))
    assert pre0.min() > 0
    w2 = st["value_fc2.weight"].copy()
    z = -np.sign(_value_pre(st, x)).astype(np.float32).reshape(B, 1)
    # tanhf(x) == 1.0f from |x| ~ 9.02; 20 leaves the reference's 1 - v^2 at 1.7e-17.
    # mixed: the upper three fifths of the boards (by |pre|) reach 20, the lowest stay live
    st["value_fc2.weight"] = w2 * np.float32(20.0 / np.sort(pre0)[2 * B // 5])
    pre = np.abs(_value_pre(st, x))
    assert (pre >= 19.9).sum() > B // 2 and (pre < 8).sum() >= 1, np.sort(pre)
    _, got, want, losses = check_step(f"saturated mixed B={B}", st, 1, 64, x, pi, z)
    assert np.abs(want["value_fc2.bias"]).max() > 0          # the live boards still train the head
    # all boards saturated
    st["value_fc2.weight"] = w2 * np.float32(20.0 / pre0.min())
    _, got, _, losses = check_step(f"saturated all B={B}", st, 1, 64, x, pi, z)
    assert np.isclose(losses[1], 4.0, rtol=1e-6, atol=0), losses
    for n in VALUE_SIDE:
        assert not got[n].any(), n


def test_zero_variance_channels():
    """Three conv1 output channels of block 0 and one stem output channel have all-zero
    weights: their conv outputs are 0 on every pixel, batch variance 0, invstd =
    1 / sqrt(eps) = 316, and the BN output is beta (+-0.25: the ReLU mask is unambiguous).
    Gradients of every tensor match the reference (these channels' conv-weight gradients
    carry the 316x factor); after one train_batch the channels' running stats follow the
    rule (mean 0.9 x 0 + 0.1 x 0, unbiased var 0.9 x 1 + 0.1 x 0); a second step leaves
    every parameter finite."""
    blocks, ch, B = 1, 64, 37
    st = seeded_state(blocks, ch)
    c1, betas = [3, 17, 40], np.array([0.25, -0.25, 0.25], np.float32)
    st["res_blocks.0.conv1.weight"][c1] = 0.0
    st["res_blocks.0.bn1.bias"][c1] = betas
    st["conv.weight"][9] = 0.0
    st["bn.bias"][9] = 0.25
    boards, x = positions(B)
    pi, z = synth_targets(B, seed=78 + B)
    m, got, want, _ = check_step("zero variance", st, blocks, ch, x, pi, z)
    # the zeroed channels are live in the backward: their weight gradients are not zero
    assert np.abs(want["res_blocks.0.conv1.weight"][c1[0]]).max() > 0 and np.abs(want["conv.weight"][9]).max() > 0
    m = make_model(blocks, ch, st)
    out = m.train_batch(x, pi, z)
    assert all(np.isfinite(v) for v in out.values()), out
    sd = {k: v.detach().cpu().numpy() for k, v in m.net.state_dict().items()}
    np.testing.assert_allclose(sd["res_blocks.0.bn1.running_var"][c1], 0.9, rtol=0, atol=1e-7)
    np.testing.assert_allclose(sd["res_blocks.0.bn1.running_mean"][c1], 0.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(sd["bn.running_var"][9], 0.9, rtol=0, atol=1e-7)
    np.testing.assert_allclose(sd["bn.running_mean"][9], 0.0, rtol=0, atol=1e-12)
    out = m.train_batch(x, pi, z)
    assert all(np.isfinite(v) for v in out.values()), out
    for k, v in m.net.state_dict().items():
        assert bool(torch.isfinite(v.float()).all()), k
    assert m.engine.train_recoveries == 0 and m.engine.train_skips() == 0


LOW_TRAIN = [("stem", 12), ("bn1", 10)]


# TRAIN_ARITH 2 misses the tolerances on these nets (figures in the docstring); selecting the
# fp32 forward for such a step from the eval fold's bound is not built yet
SPLIT = pytest.param(2, marks=pytest.mark.xfail(strict=True, reason="split-fp16 train forward loses the low range"))


@pytest.mark.parametrize("arith", [0, SPLIT])
@pytest.mark.parametrize("which,k", LOW_TRAIN)
def test_low_range_train_step(which, k, arith):
    """The stem k = 12 and bn1 k = 10 nets of tests/test_gpu_value_range.py in train mode
    (batch statistics: no calibration), 2x128 at B = 37, under the fp32 forward convs
    (TRAIN_ARITH 0) and the split-fp16 ones (2, the default).

    Measured on MI355X (worst tensor, |g_gpu - g_64| / max|g_64|; bar 2e-5):
      stem k = 12  TRAIN_ARITH 0: 1.7e-6, losses within 1e-6 relative
                   TRAIN_ARITH 2: 2.5e-4 (value_fc1.weight; 25 of 27 tensors miss), policy loss
                   0.6881311 against 0.6881390 (1.1e-5 relative; bar 1e-5)
      bn1 k = 10   TRAIN_ARITH 0: 1.3e-6
                   TRAIN_ARITH 2: 2.1e-5 (res_blocks.1.bn2.weight, the one tensor that misses)
    The split-fp16 train forward has no pack-time fold to carry activation exponents, and
    the fp32 forward is not yet selected for such nets: the TRAIN_ARITH 2 cases are strict
    expected failures until it is."""
    import _native
    lib = _native.load_library()
    blocks, ch, B = 2, 128, 37
    st = state_to_numpy(low_range_net(blocks, ch, which, k, calibrate=False).net)
    boards, x = positions(B)
    pi, z = synth_targets(B, seed=78 + B)
    prev = lib.azg_pv_set_tuning(TUNE.TRAIN_ARITH, arith)
    try:
        check_step(f"low range {which} k={k} TRAIN_ARITH={arith}", st, blocks, ch, x, pi, z)
    finally:
        lib.azg_pv_set_tuning(TUNE.TRAIN_ARITH, prev)
