"""CPU emulation of the one-product fp16 eval precision (AZG_PV_EVAL_FP16).  Test helper.

``half_forward`` has ``oracle.value_range.split_forward``'s structure with one product per
conv: conv(fp16(a), fp16(w 2^e)), accumulated in fp64 and rounded to fp32 as the MFMA's
accumulator is stored; the activation-exponent fold, the stem, the residual add and the
heads are split_forward's (fp64 arithmetic, the trunk rounded to fp32 per block).  Unlike
the GPU it has neither the fp32 accumulation order nor the MFMA's subnormal handling, so a
GPU assertion against it needs a net on which those differences are bounded (see
tests/test_gpu_precision.py).

``near_tie_stats`` is the masked-argmax criterion the precision's tests share: boards whose
fp64 top-two gap is below ``4 x max|emu16 - fp64|`` on probs are near-ties; elsewhere the
argmax must agree with fp64's.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle.boards import valid_mask
from oracle.value_range import _fold, _ilogb, act_exponents  # noqa: F401  (act_exponents: re-exported for the tests)


def _half_conv(a32: np.ndarray, w: np.ndarray):
    """3x3 conv of fp32 activations with fp32 weights by ONE fp16 product, fp64 accumulation;
    weights scaled by 2^e, e = 14 - floor(log2 max|w|) (h3_exp_of).  Returns the accumulator
    (fp32, as the MFMA's) and e."""
    w = np.asarray(w, np.float32)
    m = float(np.abs(w).max())
    e = 14 - _ilogb(m) if m > 0 else 0
    wh = np.ldexp(w, e).astype(np.float16).astype(np.float64)
    ah = np.asarray(a32, np.float32).astype(np.float16).astype(np.float64)
    acc = F.conv2d(torch.from_numpy(ah), torch.from_numpy(wh), padding=1)
    return acc.numpy().astype(np.float32), e


def half_forward(state: dict, x: np.ndarray, exps=None):
    """(probs, values) in fp64 of the emulated one-product fp16 eval forward.  exps: (T, [m_b])
    as act_exponents returns them (None: act_exponents(state), the fold the library applies)."""
    blocks = 0
    while f"res_blocks.{blocks}.bn1.weight" in state:
        blocks += 1
    T, ms = exps if exps is not None else act_exponents(state)
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
            acc, e = _half_conv(h, state[p + "conv1.weight"])
            mid = acc.astype(np.float64) * bcast(np.ldexp(sc, m - T - e)) + bcast(np.ldexp(sh, m))
            mid = np.maximum(mid, 0).astype(np.float32)
            sc, sh = _fold(state, p + "bn2")
            acc, e = _half_conv(mid, state[p + "conv2.weight"])
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


def near_tie_stats(probs, probs64, boards, dev_probs):
    """(disagreements outside near-ties, near-tie share): a board is a near-tie when its
    fp64 masked top-two gap is below 4 x dev_probs (max|emu16 - fp64| on probs)."""
    masks = np.stack([valid_mask(b) for b in boards])
    a = np.argmax(np.asarray(probs, np.float64) * masks, axis=1)
    rm = np.asarray(probs64, np.float64) * masks
    r = np.argmax(rm, axis=1)
    srt = np.sort(rm, axis=1)
    near = (srt[:, -1] - srt[:, -2]) < 4.0 * float(dev_probs)
    return np.nonzero((a != r) & ~near)[0], float(near.mean())
