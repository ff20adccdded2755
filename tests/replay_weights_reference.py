"""Surprise-weighted replay sampling (include/azg_pv.h azg_pv_replay_surprise_weights,
azg_pv_replay_prefix, azg_pv_replay_draw) restated in numpy and Python integers.  Weights
are integers (65536 quanta per unit), so the running sums and the draw have exactly one
right answer and the kernels must give it; only the weight rule computes in floating
point, in fp64 with the operation order the header fixes, which numpy's fp64 follows
operation for operation (IEEE add, multiply and divide, round-to-even rint).

``python tests/replay_weights_reference.py`` runs the self-checks (no GPU)."""
from bisect import bisect_right

import numpy as np

QUANTA = 1 << 16
QMAX = (1 << 31) - 1


def sanitise(surprise) -> np.ndarray:
    """fp32 surprises as fp64: finite and > 0, else 0."""
    s = np.asarray(surprise, dtype=np.float32).astype(np.float64)
    return np.where(np.isfinite(s) & (s > 0), s, 0.0)


def fixed_order_sum(s: np.ndarray) -> float:
    """One workgroup's sum: thread i adds elements i, i + 256, ... in increasing order, then
    the 256 partials go through the tree part[i] += part[i + h], h = 128, 64, ..., 1."""
    s = np.asarray(s, dtype=np.float64)
    rows = -(-len(s) // 256)
    padded = np.zeros(rows * 256, dtype=np.float64)   # adding +0.0 changes no partial
    padded[:len(s)] = s
    part = np.zeros(256, dtype=np.float64)
    for row in padded.reshape(rows, 256):
        part = part + row
    h = 128
    while h:
        part = part[:h] + part[h:2 * h]
        h >>= 1
    return float(part[0])


def surprise_quanta(surprise, mix: float, keep=None) -> np.ndarray:
    """The quanta of the newest ``keep`` (default: all) of the records: w_i = (1 - mix) +
    mix * n * s_i / S over ALL n records, 1 when S == 0; min(2^31 - 1, rint(w_i * 65536))."""
    s = sanitise(surprise)
    n = len(s)
    S = fixed_order_sum(s)
    mix = float(mix)
    if S > 0.0:
        w = (1.0 - mix) + mix * float(n) * s / S    # ((mix * n) * s) / S, then the sum
    else:
        w = np.ones(n, dtype=np.float64)
    q = np.minimum(np.rint(w * float(QUANTA)), float(QMAX))
    q = np.maximum(q, 0.0).astype(np.uint32)
    return q if keep is None else q[n - keep:]


def ring_order(ring: np.ndarray, head: int, count: int) -> np.ndarray:
    return np.asarray(ring)[(head + np.arange(count)) % len(ring)]


def prefix_sums(ring, head: int, count: int) -> np.ndarray:
    """uint64 running sums of the ring's weights (by slot) in ring order."""
    return np.cumsum(ring_order(ring, head, count).astype(np.uint64), dtype=np.uint64)


def draw_ids(prefix, nsym: int, rnd) -> list:
    """Image ids of random words rnd [batch][2]: t = (r0 * total) >> 64 in Python integers,
    j = the first index with prefix[j] > t, id = j * nsym + (r1 & 7 if nsym == 8 else 0)."""
    pre = [int(v) for v in prefix]
    total = pre[-1]
    ids = []
    for r0, r1 in np.asarray(rnd, dtype=np.uint64).reshape(-1, 2).tolist():
        t = (int(r0) * total) >> 64
        j = min(bisect_right(pre, t), len(pre) - 1)   # the clamp acts only when total == 0
        ids.append(j * nsym + ((int(r1) & 7) if nsym == 8 else 0))
    return ids


def word_for(t: int, total: int) -> int:
    """The smallest random word r with (r * total) >> 64 == t (0 <= t < total < 2^64)."""
    r = -((-t << 64) // total)
    assert 0 <= r < 1 << 64 and (r * total) >> 64 == t
    return r


def self_check() -> None:
    # the fixed-order sum is a sum: exact on integers, and close to fsum otherwise
    ints = np.arange(1, 1000, dtype=np.float64)
    assert fixed_order_sum(ints) == 999 * 1000 / 2
    assert fixed_order_sum(np.zeros(0)) == 0.0
    # the weight rule: mean 1 over the records, uniform at mix 0, proportional at mix 1
    rng = np.random.default_rng(0)
    s = rng.random(37).astype(np.float32)
    s[[0, 5, 9, 11]] = [0.0, -2.0, np.nan, np.inf]
    assert np.array_equal(sanitise(s)[[0, 5, 9, 11]], np.zeros(4))
    assert (surprise_quanta(s, 0.0) == QUANTA).all()
    assert (surprise_quanta(np.zeros(5), 0.7) == QUANTA).all()
    q1 = surprise_quanta(s, 1.0)
    assert (q1[[0, 5, 9, 11]] == 0).all() and abs(int(q1.sum()) - 37 * QUANTA) <= 37
    assert np.allclose(q1 / q1.sum(), sanitise(s) / sanitise(s).sum(), atol=1e-5)
    q5 = surprise_quanta(s, 0.5)
    assert abs(int(q5.sum()) - 37 * QUANTA) <= 37 and q5.min() == QUANTA // 2
    assert np.array_equal(surprise_quanta(s, 0.5, keep=7), q5[-7:])
    assert surprise_quanta(np.r_[np.zeros(99999, np.float32), 1.0], 1.0)[-1] == QMAX   # the clamp
    # prefix sums in ring order, past 2^32
    ring = np.array([QMAX, 1, 2, QMAX, QMAX], dtype=np.uint32)
    assert prefix_sums(ring, 3, 4).tolist() == [QMAX, 2 * QMAX, 3 * QMAX, 3 * QMAX + 1]
    # the draw: exact proportionality on an equally spaced grid of words
    pre = np.cumsum(np.array([1, 2, 0, 5], dtype=np.uint64))
    rnd = [[k << 61, 0] for k in range(8)]
    assert np.bincount(draw_ids(pre, 1, rnd), minlength=4).tolist() == [1, 2, 0, 5]
    assert draw_ids(pre, 8, [[0, 13], [(1 << 64) - 1, 7]]) == [0 * 8 + 5, 3 * 8 + 7]
    for t in range(8):
        j = draw_ids(pre, 1, [[word_for(t, 8), 0]])[0]
        assert int(pre[j]) > t and (j == 0 or int(pre[j - 1]) <= t)
    assert draw_ids(np.zeros(3, dtype=np.uint64), 1, [[5, 0]]) == [2]


if __name__ == "__main__":
    self_check()
    print("replay_weights_reference: self-checks passed")
