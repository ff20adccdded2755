"""The clip + Adam step (csrc/pv_train.hip adam_kernel, azg_pv_train_apply) in float64, and the
elementwise gate that holds a device's step against it.  TEST INFRASTRUCTURE ONLY; numpy only.

* ``adam_step_fp64``  -- torch's clip_grad_norm_ followed by single-tensor Adam with L2 weight
                         decay, in float64 on flat arrays.
* ``adam_constants``  -- the fp32 scalars the step is defined with (scalars are computed in
                         doubles and enter the tensor ops as fp32, torch's definition).
* ``adam_gate``       -- every output of one step against float64 from the step's OWN inputs,
                         with bounds counted from the roundings of the operation (below).
* ``emulate_fp32``    -- the same step with every operation rounded to fp32 in the kernel's
                         order; with ``mutant=`` one of MUTANTS it makes a subtly wrong step.
* ``CASES``, ``make_case`` -- the hyper-parameter / state cases the CPU and GPU tests share.

The gate, with u = 2^-24 (half an fp32 ulp, relative) and tiny = 2^-126 (so that an fp32
denormal flushed to zero, or rounded on the denormal grid, is not a failure):

  total_norm  |tn - sqrt(sum g^2)| <= 1.01 u tn64: ONE rounding of a float64 square root to
              fp32; the 1 % covers the float64 sum's own error.
  grads       bitwise fl32(g * coef), coef = min(fl32(fl32(max_norm) / fl32(tn + 1e-6f)), 1)
              from the returned tn: the clip is one IEEE multiply.
  gw          = g' + wd p, e_gw = u (2 |wd p| + |gw|): the product and the sum (0 for wd = 0).
  m           |m' - (m + b1w (gw - m))| <= 1.5 [u (|m'| + 2 b1w |gw - m|) + b1w e_gw] + tiny:
              the difference and the product (each u of b1w |gw - m|), the sum (u |m'|), and
              the inherited error of gw.
  v           |v' - (b2 v + w2 gw^2)| <= 1.5 [u (b2 v + 2 w2 gw^2 + v') + 2 w2 |gw| e_gw] + tiny:
              b2 v (one rounding), w2 gw gw (two), the sum (u v'), and gw's error through the
              square.
  p           from the device's own m', v': upd = lr_bc1 m' / (sqrt(v') / bc2s + eps),
              |p' - (p - upd)| <= 1.5 [u |p - upd| + 5 u |upd|] + tiny: sqrt, divide, add, divide
              and one spare on upd; the fused update itself rounds once.

The square brackets are first-order rounding counts; the factor 1.5 covers the second-order
terms (the bounds are written with computed values where exact ones belong)."""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
INF = float("inf")
F32 = np.float32

DEFAULTS = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=1e-4)

# name -> hyper-parameters (missing: DEFAULTS), step, max_norm and how make_case draws the data:
#   s      gradients ~ s N(0, 1)
#   norm   gradients rescaled in float64 so that their exact norm is this
#   zeros  a block of exactly-zero gradients (an eighth of the buffer, from n // 3)
#   spike  a block of gradients at 1e-20 and 16 elements at 1e15
# Moments are zero at step 1 and non-zero, of the scale of the gradients the step sees, above it.
CASES = {
    "defaults step 1": dict(step=1, s=1e-3, max_norm=3.0),
    "clipped hard step 7": dict(step=7, s=10.0, max_norm=3.0),
    # optimizer.step()'s path: no clip, the wd == 0 branch, bias corrections near 1
    "plain step 1000": dict(step=1000, s=1e-3, max_norm=INF, lr=3e-4, betas=(0.8, 0.99), eps=1e-6, wd=0.0),
    # a lerp weight above 1/2, where torch switches formula (the float64 gate is formula-agnostic)
    "lerp weight 0.6": dict(step=3, s=1e-3, max_norm=3.0, betas=(0.4, 0.999)),
    # L2 and decoupled weight decay differ by far more than the bound
    "wd 1e-2": dict(step=3, s=1e-3, max_norm=3.0, wd=1e-2),
    # clipping active, and the 1e-6 of the coefficient about 5 u of it
    "norm 3.2": dict(step=5, s=1e-3, norm=3.2, max_norm=3.0),
    # 3 ulps under max_norm: tn + 1e-6f lands one ulp above it, the coefficient one or two ulps under 1
    "norm just under": dict(step=2, s=1e-3, norm=3.0 * (1.0 - 2.0 ** -22), max_norm=3.0),
    # the coefficient is exactly 1: the grads come back bitwise
    "norm 1.5": dict(step=4, s=1e-3, norm=1.5, max_norm=3.0),
    "zeros": dict(step=1, s=1e-3, max_norm=3.0, wd=0.0, zeros=True),
    # wd = 0 and zero moments, or wd p and the moments would carry the small elements: the 16
    # large ones carry the norm (4e15) and squash every other clipped gradient to ~1e-18 and
    # ~1e-35; v' is an fp32 denormal or zero there and eps is the whole denominator
    "spike": dict(step=1, s=1e-3, max_norm=3.0, wd=0.0, spike=True),
}


def hyper_of(case: dict) -> dict:
    return {k: case.get(k, d) for k, d in DEFAULTS.items()}


def zero_block(n: int) -> slice:
    return slice(n // 3, n // 3 + n // 8)


def make_case(name: str, n: int, seed: int = 0):
    """-> (p, g, m, v) float32 arrays of n elements, hyper dict, step, max_norm."""
    c = CASES[name]
    rng = np.random.default_rng([seed, sorted(CASES).index(name), n])
    p = (0.05 * rng.standard_normal(n)).astype(F32)
    g = c["s"] * rng.standard_normal(n)
    if "norm" in c:
        g *= c["norm"] / math.sqrt(float(np.dot(g, g)))
    if c.get("zeros"):
        g[zero_block(n)] = 0.0
    if c.get("spike"):
        g[zero_block(n)] = 1e-20
        g[rng.choice(n, 16, replace=False)] = 1e15
    g = g.astype(F32)
    if c["step"] == 1:
        m, v = np.zeros(n, F32), np.zeros(n, F32)
    else:
        # the scale of the gradients after the clip
        gs = float(np.sqrt(np.mean(g.astype(np.float64) ** 2)))
        gs *= min(c["max_norm"] / (gs * math.sqrt(n)), 1.0)
        m = (0.5 * gs * rng.standard_normal(n)).astype(F32)
        v = ((gs * rng.standard_normal(n)) ** 2 * 0.7).astype(F32)
    return (p, g, m, v), hyper_of(c), c["step"], c["max_norm"]


def adam_step_fp64(p, g, m, v, step, lr, betas, eps, wd, max_norm):
    """clip_grad_norm_(max_norm) then torch.optim.Adam's single-tensor step (L2 weight decay, no
    amsgrad), everything in float64, hyper-parameters as given.  -> p', g', m', v', total_norm."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    tn = math.sqrt(float(np.dot(g, g)))
    coef = min(float(max_norm) / (tn + 1e-6), 1.0)
    g = g * coef
    gw = g + wd * p if wd != 0 else g
    w = 1.0 - b1
    m = m + w * (gw - m) if w < 0.5 else gw - (gw - m) * (1.0 - w)      # Tensor.lerp_
    v = v * b2 + (1.0 - b2) * gw * gw
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = np.sqrt(v) / math.sqrt(bc2) + eps
    p = p + (-(lr / bc1)) * (m / denom)
    return p, g, m, v, tn


def adam_constants(step, lr, betas, eps, wd) -> dict:
    """The fp32 scalars of step `step`: beta1 and beta2 are rounded to fp32 first and their
    powers taken in double."""
    b1, b2 = float(F32(betas[0])), float(F32(betas[1]))
    return dict(lr_bc1=F32(float(F32(lr)) / (1.0 - b1 ** step)), bc2s=F32(math.sqrt(1.0 - b2 ** step)),
                b1w=F32(1.0 - b1), b2=F32(b2), w2=F32(1.0 - b2), eps=F32(eps), wd=F32(wd))


def clip_coef(tn, max_norm) -> np.float32:
    """min(fl32(fl32(max_norm) / fl32(tn + 1e-6f)), 1) in fp32; 1 for an infinite max_norm."""
    with np.errstate(over="ignore"):
        coef = F32(max_norm) / (F32(tn) + F32(1e-6))
    return coef if coef < F32(1.0) else F32(1.0)


def _ratio(err, bound):
    r = err / bound
    return float(r.max()), int((err > bound).sum())


def adam_gate(before, after, step, hyper, max_norm) -> dict:
    """before = (p, g, m, v), after = (p', g', m', v', total_norm): a device's own float32 buffers
    around ONE step.  -> {"tn" | "g" | "m" | "v" | "p": (worst err / bound, violations)} over
    every element.  The clipped grads are required bitwise: their figure is the error in units of
    u |want| (at least 1 for any wrong bit) and their violations the elements that differ."""
    p, g, m, v = (np.asarray(a, np.float64) for a in before)
    p1, g1, m1, v1 = (np.asarray(a, np.float64) for a in after[:4])
    tn = F32(np.asarray(after[4]).reshape(-1)[0])
    k = {n: float(x) for n, x in adam_constants(step, **hyper).items()}
    out = {}

    tn64 = math.sqrt(float(np.dot(g, g)))
    e = abs(float(tn) - tn64)
    out["tn"] = (e / (1.01 * U * tn64), int(not e <= 1.01 * U * tn64))

    want = (np.asarray(before[1], F32) * clip_coef(tn, max_norm)).astype(F32)
    got = np.asarray(after[1], F32)
    e = np.abs(g1 - want.astype(np.float64))
    out["g"] = (float((e / np.maximum(U * np.abs(want.astype(np.float64)), TINY)).max()),
                int((got.view(np.uint32) != want.view(np.uint32)).sum()))

    wp = k["wd"] * p
    gw = g1 + wp
    e_gw = U * (2.0 * np.abs(wp) + np.abs(gw)) if k["wd"] != 0.0 else 0.0
    d = k["b1w"] * np.abs(gw - m)
    out["m"] = _ratio(np.abs(m1 - (m + k["b1w"] * (gw - m))),
                      1.5 * (U * (np.abs(m1) + 2.0 * d) + k["b1w"] * e_gw) + TINY)
    sq = k["w2"] * gw * gw
    out["v"] = _ratio(np.abs(v1 - (k["b2"] * v + sq)),
                      1.5 * (U * (k["b2"] * v + 2.0 * sq + v1) + 2.0 * k["w2"] * np.abs(gw) * e_gw) + TINY)
    upd = k["lr_bc1"] * m1 / (np.sqrt(v1) / k["bc2s"] + k["eps"])
    out["p"] = _ratio(np.abs(p1 - (p - upd)), 1.5 * (U * np.abs(p - upd) + 5.0 * U * np.abs(upd)) + TINY)
    return out


MUTANTS = ("bc_step_minus_1", "no_bc2", "eps_in_sqrt", "adamw", "unclipped_moments", "m_shift", "v_shift",
           "coef_no_1e-6")


def emulate_fp32(p, g, m, v, step, lr, betas, eps, wd, max_norm, mutant=None):
    """adam_kernel's step, every operation rounded to fp32 in the kernel's order (the norm: a
    float64 sum, its root rounded to fp32; the parameter update: one fused multiply-add).
    -> p', g', m', v', total_norm (float32).  mutant: None (faithful) or one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS, mutant
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    k = adam_constants(step - 1 if mutant == "bc_step_minus_1" else step, lr, betas, eps, wd)
    g64 = g.astype(np.float64)
    tn = F32(math.sqrt(float(np.dot(g64, g64))))
    if mutant == "coef_no_1e-6":
        with np.errstate(over="ignore"):
            coef = F32(max_norm) / tn
        coef = coef if coef < F32(1.0) else F32(1.0)
    else:
        coef = clip_coef(tn, max_norm)
    g1 = g * coef
    gi = g if mutant == "unclipped_moments" else g1
    if k["wd"] != 0 and mutant != "adamw":
        gi = gi + k["wd"] * p
    if mutant == "m_shift":
        m = np.roll(m, -1)
    if mutant == "v_shift":
        v = np.roll(v, -1)
    m1 = m + k["b1w"] * (gi - m)
    v1 = v * k["b2"]
    v1 = v1 + k["w2"] * gi * gi
    if mutant == "eps_in_sqrt":
        denom = np.sqrt(v1 + k["eps"]) / k["bc2s"]
    elif mutant == "no_bc2":
        denom = np.sqrt(v1) + k["eps"]
    else:
        denom = np.sqrt(v1) / k["bc2s"] + k["eps"]
    q = m1 / denom
    if mutant == "adamw":
        p = p * F32(1.0 - float(F32(lr)) * float(k["wd"]))
    # fmaf(-lr_bc1, q, p): the product of two fp32 values is exact in float64
    p1 = (p.astype(np.float64) - float(k["lr_bc1"]) * q.astype(np.float64)).astype(F32)
    assert all(a.dtype == F32 for a in (p1, g1, m1, v1))
    return p1, g1, m1, v1, tn
