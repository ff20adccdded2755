"""Oracle helpers for the low end of the activation range.  TEST INFRASTRUCTURE ONLY.

* ``scale_bn``      -- scale BN gamma / beta by 2^-k on a named set of BNs, so the
                       activations they produce sit 2^-k below O(1) (exact: powers of two).
* ``calib_bn``      -- give BN running stats the statistics of real activations.
* ``act_exponents`` -- the rule by which the library picks the power-of-two activation
                       exponents it folds into the eval BN parameters (``pv_pack.hip``
                       ``repack_all_kernel``), restated.
* ``split_forward`` -- CPU emulation of the split-fp16 eval forward: residual convs as
                       hi_a hi_w + lo_a hi_w + hi_a lo_w on operands rounded exactly as the
                       kernels round them, accumulated in fp64; stem and heads exact.  It
                       is a design aid (what a pack-time rule does to the operands' bits),
                       not a reference for GPU assertions: it has neither the fp32
                       accumulation order nor the MFMA's treatment of fp16 subnormals.
* ``sharpen_policy``, ``sharp_net``, ``sharp_case`` -- nets with peaked policy outputs
                       (policy_fc scaled by 2^k) and their CPU references: on a near-uniform
                       softmax an absolute bar on probabilities is a weak bar on the logits.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.boards import encode_batch, synth_positions

BN_EPS = 1e-5
DEAD_BAND = 0.25      # a BN whose bound is at least this keeps exponent 0
TRUNK_CAP = 12        # trunk bound * 2^T stays below 2^(TRUNK_CAP + 1)
MAX_EXP = 40


def calib_bn(ref, seed):
    """Give BN running stats the statistics of real activations (train-mode passes
    without optimizer steps), as a trained net has."""
    b, p = synth_positions(64, seed=seed)
    x = torch.from_numpy(encode_batch(b, p)).to(ref.dtype)
    ref.net.train()
    for mod in ref.net.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.momentum = None   # cumulative average
    with torch.no_grad():
        for _ in range(3):
            ref.net(x)
    for mod in ref.net.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.momentum = 0.1
    ref.net.eval()


def scale_bn(net, which: str, k: int) -> None:
    """gamma, beta *= 2^-k on: "stem" (the stem BN), "bn1" (every block's bn1), "trunk"
    (the stem BN's gamma and every bn2's gamma and beta: everything the trunk sums).
    Running stats are left alone: calibrate afterwards."""
    f = 2.0 ** -k
    with torch.no_grad():
        if which == "stem":
            net.bn.weight.mul_(f)
            net.bn.bias.mul_(f)
        elif which == "bn1":
            for blk in net.res_blocks:
                blk.bn1.weight.mul_(f)
                blk.bn1.bias.mul_(f)
        elif which == "trunk":
            net.bn.weight.mul_(f)
            for blk in net.res_blocks:
                blk.bn2.weight.mul_(f)
                blk.bn2.bias.mul_(f)
        else:
            raise ValueError(which)


def _bound(gamma, beta) -> np.float32:
    """max_c(|beta_c| + 4 |gamma_c|) in fp32: a 4-sigma bound on the BN's output."""
    g, b = np.asarray(gamma, np.float32), np.asarray(beta, np.float32)
    return np.float32(np.max(np.abs(b) + np.float32(4.0) * np.abs(g)))


def _ilogb(v) -> int:
    return math.frexp(float(v))[1] - 1


def _want(bound) -> int:
    """The exponent that lifts a bound below the dead band into [4, 8)."""
    if not (0.0 < float(bound) < DEAD_BAND):
        return 0
    return min(2 - _ilogb(bound), MAX_EXP)


def act_exponents(state: dict):
    """(T, [m_b]): the trunk activation is carried as 2^T x and block b's mid activation
    as 2^m_b x.  T lifts the stem BN's bound, capped so that the bound of the whole trunk
    sum (stem + every bn2) times 2^T stays below 2^13 (fp16 overflows at 2^16); m_b lifts
    bn1_b's bound.  Any bound of at least 0.25 (gamma >= 1/16) gives 0."""
    blocks = 0
    while f"res_blocks.{blocks}.bn1.weight" in state:
        blocks += 1
    a_s = _bound(state["bn.weight"], state["bn.bias"])
    u = a_s
    ms = []
    for i in range(blocks):
        p = f"res_blocks.{i}."
        ms.append(_want(_bound(state[p + "bn1.weight"], state[p + "bn1.bias"])))
        u = np.float32(u + _bound(state[p + "bn2.weight"], state[p + "bn2.bias"]))
    t = _want(a_s)
    if t:
        t = max(0, min(t, TRUNK_CAP - _ilogb(u)))
    return t, ms


def _fold(state, prefix):
    """Eval-mode BN fold in fp32, as fold_bn of pv_pack.hip."""
    g = np.asarray(state[prefix + ".weight"], np.float32)
    b = np.asarray(state[prefix + ".bias"], np.float32)
    mean = np.asarray(state[prefix + ".running_mean"], np.float32)
    var = np.asarray(state[prefix + ".running_var"], np.float32)
    alpha = (np.float32(1.0) / np.sqrt(var + np.float32(BN_EPS))) * g
    return alpha, b - mean * alpha


def _split16(a: np.ndarray):
    """hi = fp16(a), lo = fp16(a - hi) (round to nearest even, subnormals kept)."""
    a = np.asarray(a, np.float32)
    hi = a.astype(np.float16)
    lo = (a - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def _split_conv(a32: np.ndarray, w: np.ndarray):
    """3x3 conv of fp32 activations with fp32 weights by three split-fp16 products,
    fp64 accumulation; weights scaled by 2^e, e = 14 - floor(log2 max|w|) (h3_exp_of).
    Returns the accumulator (fp32, as the MFMA's) and e."""
    w = np.asarray(w, np.float32)
    m = float(np.abs(w).max())
    e = 14 - _ilogb(m) if m > 0 else 0
    wh, wl = _split16(np.ldexp(w, e))
    ah, al = _split16(a32)
    t = torch.from_numpy
    acc = (F.conv2d(t(al), t(wh), padding=1) + F.conv2d(t(ah), t(wl), padding=1)
           + F.conv2d(t(ah), t(wh), padding=1))
    return acc.numpy().astype(np.float32), e


def split_forward(state: dict, x: np.ndarray, exps=None):
    """(probs, values) in fp64 of the emulated split-fp16 eval forward.  exps: (T, [m_b])
    as act_exponents returns them (None: all zero, the arithmetic without the fold)."""
    blocks = 0
    while f"res_blocks.{blocks}.bn1.weight" in state:
        blocks += 1
    T, ms = exps if exps is not None else (0, [0] * blocks)
    d = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    bcast = lambda v: np.asarray(v, np.float64)[None, :, None, None]
    with torch.no_grad():
        sc, sh = _fold(state, "bn")
        z = F.conv2d(d(x), d(state["conv.weight"]), padding=1).numpy()
        h = np.maximum(z * bcast(np.ldexp(sc, T)) + bcast(np.ldexp(sh, T)), 0).astype(np.float32)
        for i in range(blocks):
            p = f"res_blocks.{i}."
            m = ms[i]
            sc, sh = _fold(state, p + "bn1")
            acc, e = _split_conv(h, state[p + "conv1.weight"])
            mid = acc.astype(np.float64) * bcast(np.ldexp(sc, m - T - e)) + bcast(np.ldexp(sh, m))
            mid = np.maximum(mid, 0).astype(np.float32)
            sc, sh = _fold(state, p + "bn2")
            acc, e = _split_conv(mid, state[p + "conv2.weight"])
            out = acc.astype(np.float64) * bcast(np.ldexp(sc, T - m - e)) + bcast(np.ldexp(sh, T)) + h
            h = np.maximum(out, 0).astype(np.float32)
        B = h.shape[0]
        ht = d(h)
        sc, sh = _fold(state, "policy_bn")
        pz = F.conv2d(ht, d(state["policy_conv.weight"])).numpy()
        pf = np.maximum(pz * bcast(np.ldexp(sc, -T)) + bcast(sh), 0).reshape(B, -1)
        logits = F.linear(d(pf), d(state["policy_fc.weight"]), d(state["policy_fc.bias"]))
        sc, sh = _fold(state, "value_bn")
        vz = F.conv2d(ht, d(state["value_conv.weight"])).numpy()
        vf = np.maximum(vz * bcast(np.ldexp(sc, -T)) + bcast(sh), 0).reshape(B, -1)
        hv = F.relu(F.linear(d(vf), d(state["value_fc1.weight"]), d(state["value_fc1.bias"])))
        value = torch.tanh(F.linear(hv, d(state["value_fc2.weight"]), d(state["value_fc2.bias"])))
        return F.softmax(logits, dim=1).numpy(), value.numpy()


# The low-range nets of tests/test_gpu_value_range.py: (BN set, k); k = 0 is the control.
CASES = (("stem", 0), ("stem", 8), ("stem", 12), ("bn1", 10), ("trunk", 12))


def low_range_net(blocks: int, ch: int, which: str, k: int, calibrate: bool = True):
    """A seeded RefModel whose named BNs are scaled by 2^-k and (calibrate) whose running
    stats are then calibrated; the seed depends on the shape only, so every case of one
    shape has the same conv and FC weights."""
    from oracle.ref_net import RefModel
    torch.manual_seed(blocks * 1000 + ch + 5)
    ref = RefModel(blocks, ch)
    scale_bn(ref.net, which, k)
    if calibrate:
        calib_bn(ref, seed=blocks * 1000 + ch)
    return ref


# The peaked-policy nets of tests/test_gpu_sharp_outputs.py: policy_fc scaled by 2^k; k = 0
# is the control.  At k = 4 rows saturate (top-2 gaps of 1e-8) and the softmax flattens again.
SHARP = (2, 3)


def sharpen_policy(net, k: int) -> None:
    """policy_fc.weight, policy_fc.bias *= 2^k: every logit scales by exactly 2^k (a power
    of two commutes with each rounding of the FC's products and sums), nothing else moves."""
    f = 2.0 ** int(k)
    with torch.no_grad():
        net.policy_fc.weight.mul_(f)
        net.policy_fc.bias.mul_(f)


def sharp_net(blocks: int, ch: int, k: int):
    """low_range_net's seeded, calibrated RefModel (its k = 0 control), policy sharpened by
    2^k.  Every k of one shape shares everything but policy_fc with the others."""
    ref = low_range_net(blocks, ch, "stem", 0)
    sharpen_policy(ref.net, k)
    return ref


# (boards, synth_positions seed) per shape; the GPU forms take prefixes of these sets.  The
# seeds are chosen so that the reference alone meets tests/test_oracle_sharp_outputs.py.
SHARP_BOARDS = {(2, 128): (258, 2 + 128), (1, 256): (20, 1 + 256), (2, 64): (37, 2 + 64)}
SHARP_PREFIXES = {(2, 128): (3, 37, 258), (1, 256): (20,), (2, 64): (37,)}
ARGMAX_GAP = 2e-5     # rows whose fp64 masked top-2 gap is below this are exempt from the argmax check


@functools.lru_cache(maxsize=None)
def sharp_case(blocks: int, ch: int, k: int) -> dict:
    """The sharpened net's state and its CPU references on the shape's board set, computed
    once and read only: x, boards, players, fp32 and fp64 probs / values / logits (p32, v32,
    l32, p64, v64, l64) and `exempt`, the rows whose fp64 masked top-2 gap is below ARGMAX_GAP."""
    from oracle.boards import valid_mask
    from oracle.ref_net import state_to_numpy
    torch.set_num_threads(8)
    n, seed = SHARP_BOARDS[(blocks, ch)]
    boards, players = synth_positions(n, seed=seed)
    x = encode_batch(boards, players)
    ref = sharp_net(blocks, ch, k)
    p32, v32, l32 = ref.predict(x, with_logits=True)
    p64, v64, l64 = as_fp64(ref).predict(x, with_logits=True)
    masks = np.stack([valid_mask(b) for b in boards])
    srt = np.sort(p64 * masks, axis=1)
    out = dict(state=state_to_numpy(ref.net), x=x, boards=np.asarray(boards), players=np.asarray(players), masks=masks,
               p32=p32, v32=v32, l32=l32, p64=p64, v64=v64, l64=l64, exempt=(srt[:, -1] - srt[:, -2]) < ARGMAX_GAP)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def as_fp64(ref):
    """The same weights in an fp64 RefModel."""
    from oracle.ref_net import RefModel
    r64 = RefModel(len(ref.net.res_blocks), ref.net.channels, dtype=torch.float64)
    r64.net.load_state_dict({k: (v.double() if v.dtype.is_floating_point else v)
                             for k, v in ref.net.state_dict().items()})
    return r64
