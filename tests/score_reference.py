"""The score record's field table (include/azg_pv.h azg_pv_score_outputs) restated in
fp64 numpy, from logits, values and targets.  TEST INFRASTRUCTURE: what the GPU scoring
kernels are compared against; itself pinned against torch's KLDivLoss(batchmean) and
MSELoss, the reference's own calls (network.py:162-163,216-219), in test_score_reference."""
import numpy as np

FIELDS = ("kl", "sq", "entropy", "top1", "p_best", "v_agree", "decided", "target_mass")


def score_records(logits, values, pis, zs) -> np.ndarray:
    """[B,8] float64 records.  Inputs are taken as given (float32 inputs are widened
    exactly), so the GPU and this function see the same numbers."""
    l = np.asarray(logits, dtype=np.float64)
    t = np.asarray(pis, dtype=np.float64)
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    z = np.asarray(zs, dtype=np.float64).reshape(-1)
    B = l.shape[0]
    assert l.shape == t.shape == (B, 225) and v.shape == z.shape == (B,)
    sh = l - l.max(axis=1, keepdims=True)
    lp = sh - np.log(np.exp(sh).sum(axis=1, keepdims=True))
    p = np.exp(lp)
    pos = t > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = np.where(pos, t * (np.log(np.where(pos, t, 1.0)) - lp), 0.0).sum(axis=1)
    ent = -np.where(p > 0, p * lp, 0.0).sum(axis=1)
    jl = np.argmax(l, axis=1)            # numpy's argmax: the lowest index among equal maxima
    jt = np.argmax(t, axis=1)
    out = np.empty((B, 8), dtype=np.float64)
    out[:, 0] = kl
    out[:, 1] = (v - z) ** 2
    out[:, 2] = ent
    out[:, 3] = jl == jt
    out[:, 4] = p[np.arange(B), jt]
    out[:, 5] = v * z > 0
    out[:, 6] = z != 0
    out[:, 7] = t.sum(axis=1)
    return out


def summary_from_records(rec) -> dict:
    """engine.score_summary's dict from fp64 records (restated, not imported)."""
    rec = np.asarray(rec, dtype=np.float64)
    n = len(rec)
    s = rec.sum(axis=0)
    return {"policy_loss": s[0] / n, "value_loss": s[1] / n, "total_loss": s[0] / n + s[1] / n,
            "policy_entropy": s[2] / n, "policy_top1": s[3] / n, "target_move_prob": s[4] / n,
            "value_sign_agreement": s[5] / max(s[6], 1.0), "target_mass": s[7] / n, "n": n}


def planted_case(B, seed):
    """(logits, values, pis, zs) float32 for B boards: logits 3 * randn, softmax-of-randn
    targets, and the edge rows of the kernel test planted into every B that has room:
    row 0 a one-hot target; 1 a target with exact zeros; 2 a uniform target; 3 logits
    alternating +-80 (probabilities underflow to 0 in fp32); 4 the two largest logits equal
    and the two largest targets equal; and z in {-1, 0, 1} x v in {-1, 0, 1, 0.3, -0.3}
    cycled over all rows."""
    rng = np.random.default_rng(seed)
    l = (3.0 * rng.standard_normal((B, 225))).astype(np.float32)
    raw = rng.standard_normal((B, 225))
    t = np.exp(raw - raw.max(axis=1, keepdims=True))
    t = (t / t.sum(axis=1, keepdims=True)).astype(np.float32)
    vs = np.array([-1.0, 0.0, 1.0, 0.3, -0.3], dtype=np.float32)
    zs_ = np.array([-1.0, 0.0, 1.0], dtype=np.float32)
    v = vs[np.arange(B) % 5]
    z = zs_[(np.arange(B) // 5) % 3]     # 15 rows see every (z, v) pair
    if B >= 1:
        t[0] = 0.0
        t[0, 137] = 1.0
    if B >= 2:
        t[1, ::3] = 0.0
        t[1] /= t[1].sum(dtype=np.float64)
        assert (t[1] == 0).sum() == 75
    if B >= 3:
        t[2] = np.float32(1.0 / 225.0)
    if B >= 4:
        l[3] = np.where(np.arange(225) % 2 == 0, 80.0, -80.0).astype(np.float32)
    if B >= 5:
        top = np.float32(np.abs(l[4]).max() + 1.0)
        l[4, 200] = l[4, 17] = top           # argmax must be 17
        t[4, 201] = t[4, 17] = np.float32(t[4].max() * 2)   # argmax must be 17
    return l, v.copy(), t, z.copy()
