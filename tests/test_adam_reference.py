"""oracle/adam_reference.py on the CPU: the float64 step is torch's, the gate passes a faithful
fp32 step and rejects subtly wrong ones.

The gate's bounds are derived (oracle/adam_reference.py's docstring); this module measures how
much of them a faithful fp32 step uses and by what factor each mutant exceeds them.  A mutant
counts only in the cases where it is observable, and the rule for that is stated beside it --
from the case's definition, never from the gate's verdict."""
import math

import numpy as np
import pytest
import torch

from oracle.adam_reference import (CASES, MUTANTS, adam_constants, adam_gate, adam_step_fp64, emulate_fp32, hyper_of,
                                   make_case, zero_block)

N = 65537            # odd; every case's data is drawn for this size
QUANTITIES = ("tn", "g", "m", "v", "p")


@pytest.mark.parametrize("name", list(CASES))
def test_fp64_step_is_torch(name):
    """adam_step_fp64 == clip_grad_norm_ + torch.optim.Adam on float64 tensors over five steps
    (the case's moments and step count loaded as optimizer state), rtol 1e-12."""
    (p, g, m, v), hyper, step, max_norm = make_case(name, 4099, seed=1)
    tp = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = torch.optim.Adam([tp], lr=hyper["lr"], betas=hyper["betas"], eps=hyper["eps"], weight_decay=hyper["wd"])
    opt.state[tp] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m.astype(np.float64)),
                     "exp_avg_sq": torch.from_numpy(v.astype(np.float64))}
    cur = [a.astype(np.float64) for a in (p, m, v)]
    rng = np.random.default_rng(5)
    for s in range(5):
        gs = g.astype(np.float64) * (1.0 + 0.25 * rng.standard_normal(g.size)) if s else g.astype(np.float64)
        tp.grad = torch.from_numpy(gs.copy())
        tn_t = torch.nn.utils.clip_grad_norm_([tp], max_norm)
        opt.step()
        p1, g1, m1, v1, tn = adam_step_fp64(cur[0], gs, cur[1], cur[2], step + s, hyper["lr"], hyper["betas"],
                                            hyper["eps"], hyper["wd"], max_norm)
        st = opt.state[tp]
        assert float(st["step"]) == step + s
        # rtol 1e-12 elementwise.  m' and p' are differences: where one cancels, two correct
        # float64 evaluations (torch's lerp is fused, numpy's is not) differ by a few 2^-53 of the
        # OPERANDS, which no relative bound on the result covers; that rounding of the reference's
        # own format is the only absolute term, and v', the grads and the norm have none.
        gw = g1 + hyper["wd"] * cur[0]
        eps64 = 8 * 2.0 ** -53
        for tag, got, want, operands in (("p", p1, tp.detach(), np.abs(cur[0]) + np.abs(p1 - cur[0])),
                                         ("g", g1, tp.grad, 0.0), ("m", m1, st["exp_avg"], np.abs(cur[1]) + np.abs(gw)),
                                         ("v", v1, st["exp_avg_sq"], 0.0), ("tn", np.array([tn]), tn_t.reshape(1), 0.0)):
            want = want.numpy()
            bad = np.abs(got - want) > 1e-12 * np.abs(want) + eps64 * operands
            assert not bad.any(), (name, step + s, tag, int(bad.sum()))
        cur = [p1, m1, v1]


def test_constants():
    k = adam_constants(7, 1e-3, (0.9, 0.999), 1e-8, 1e-4)
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    assert all(x.dtype == np.float32 for x in k.values())
    assert k["lr_bc1"] == np.float32(float(np.float32(1e-3)) / (1.0 - b1 ** 7))
    assert k["bc2s"] == np.float32(math.sqrt(1.0 - b2 ** 7))
    assert k["b1w"] == np.float32(1.0 - b1) and k["w2"] == np.float32(1.0 - b2) and k["b2"] == np.float32(0.999)
    assert k["eps"] == np.float32(1e-8) and k["wd"] == np.float32(1e-4)


def _gate(name, mutant=None):
    before, hyper, step, max_norm = make_case(name, N)
    after = emulate_fp32(*before, step, max_norm=max_norm, mutant=mutant, **hyper)
    return adam_gate(before, after, step, hyper, max_norm)


@pytest.mark.parametrize("name", list(CASES))
def test_faithful_emulation_passes(name):
    res = _gate(name)
    print(f"{name}: " + "  ".join(f"{q} {res[q][0]:.3f}" for q in QUANTITIES))
    for q in QUANTITIES:
        assert res[q][1] == 0, (name, q, res[q])
    assert res["g"][0] == 0.0            # the emulation's clip is the gate's, bitwise
    # first-order brackets (the gate is 1.5 x them): a faithful step stays inside them
    assert max(res[q][0] for q in "mvp") <= 1.0 / 1.5 + 0.01, res


def test_case_edges():
    """The cases are what their names say."""
    f = np.float32
    for name, want in (("norm 3.2", 3.2), ("norm just under", 3.0 * (1 - 2.0 ** -22)), ("norm 1.5", 1.5)):
        (p, g, m, v), hyper, step, max_norm = make_case(name, N)
        tn = math.sqrt(float(np.dot(g.astype(np.float64), g.astype(np.float64))))
        assert abs(tn - want) <= 1e-8 * want, (name, tn)
        coef = min(f(max_norm) / (f(tn) + f(1e-6)), f(1))
        if name == "norm 3.2":
            assert coef < 1 and abs(float(f(max_norm) / f(tn)) / float(coef) - 1.0) > 4 * 2.0 ** -24
        elif name == "norm just under":
            assert f(tn) < f(3.0) and f(1) - coef in (f(2.0 ** -24), f(2.0 ** -23)), coef
        else:
            assert coef == 1
    (p, g, m, v), hyper, step, max_norm = make_case("zeros", N)
    assert not g[zero_block(N)].any() and not m.any() and not v.any() and step == 1 and hyper["wd"] == 0
    p1, g1, m1, v1, tn = emulate_fp32(p, g, m, v, step, max_norm=max_norm, **hyper)
    z = zero_block(N)
    assert np.array_equal(p1[z], p[z]) and not m1[z].any() and not v1[z].any()
    (p, g, m, v), hyper, step, max_norm = make_case("spike", N)
    p1, g1, m1, v1, tn = emulate_fp32(p, g, m, v, step, max_norm=max_norm, **hyper)
    assert all(np.isfinite(a).all() for a in (p1, g1, m1, v1)) and np.isfinite(tn)
    small = (v1 > 0) & (v1 < f(2.0 ** -126))
    assert small.sum() > N // 2                                   # v' is an fp32 denormal on most elements
    assert (np.sqrt(v1[small]) / adam_constants(step, **hyper)["bc2s"] < 1e-6 * hyper["eps"]).all()
    assert (g == f(1e15)).sum() == 16 and abs(float(tn) / 4e15 - 1) < 1e-6
    assert CASES["lerp weight 0.6"]["betas"][0] < 0.5 and hyper_of(CASES["plain step 1000"])["wd"] == 0


def _observable(mutant, name):
    """Where a mutant changes the step by more than its roundings -- decided from the case's
    definition."""
    c, h = CASES[name], hyper_of(CASES[name])
    if mutant == "bc_step_minus_1":
        # bc(step - 1) and bc(step) differ by percents up to step 10.  At step 1000 (betas 0.8,
        # 0.99) the constants of steps 999 and 1000 differ by under 4 u, inside the p bound's own
        # 5 u of roundings: not observable there, and not counted (the last test of this module).
        # Step 1 has no step 0 (a division by zero).
        return 2 <= c["step"] <= 10
    if mutant == "no_bc2":
        return True                    # even at step 1000 bc2s = 1 - 2.2e-5 is 360 u from 1
    if mutant == "eps_in_sqrt":
        return True
    if mutant == "adamw":
        return h["wd"] != 0
    if mutant == "unclipped_moments":
        # the coefficient must be below 1 by much more than an ulp: not in "norm just under"
        return name in ("clipped hard step 7", "norm 3.2", "spike")
    if mutant in ("m_shift", "v_shift"):
        return c["step"] > 1                                                  # non-zero moments
    if mutant == "coef_no_1e-6":
        return name == "norm 3.2"      # elsewhere the term is below an ulp of the coefficient, or coef is 1
    raise KeyError(mutant)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutant_is_rejected(mutant):
    """Some quantity exceeds its bound, by a factor of at least 2, in every case where the
    mutant is observable."""
    factors = {}
    for name in CASES:
        if not _observable(mutant, name):
            continue
        res = _gate(name, mutant)
        assert sum(res[q][1] for q in QUANTITIES) > 0, (mutant, name, res)
        factors[name] = max(res[q][0] for q in QUANTITIES)
    assert factors, mutant
    worst = min(factors, key=factors.get)
    skipped = [n for n in CASES if n not in factors]
    print(f"mutant {mutant}: smallest rejection factor {factors[worst]:.3g} ({worst}); observable in "
          f"{len(factors)} of {len(CASES)} cases" + (f", not in: {', '.join(skipped)}" if skipped else ""))
    assert factors[worst] >= 2.0, (mutant, factors)


def test_bias_correction_off_by_one_is_invisible_at_step_1000():
    """Said, not pretended: at step 1000 of the plain case the constants of steps 999 and 1000
    together move the update by less than the 5 u its own roundings are allowed, so no
    elementwise gate can tell the two apart."""
    h = hyper_of(CASES["plain step 1000"])
    a, b = adam_constants(1000, **h), adam_constants(999, **h)
    shift = sum(abs(float(a[k]) - float(b[k])) / float(a[k]) for k in ("lr_bc1", "bc2s"))
    res = _gate("plain step 1000", "bc_step_minus_1")
    print(f"step 999 against 1000: constants {shift / 2.0 ** -24:.2f} u apart; gate " +
          "  ".join(f"{q} {res[q][0]:.3f}" for q in QUANTITIES))
    assert shift <= 5 * 2.0 ** -24
    assert max(res[q][0] for q in QUANTITIES) < 2.0
