"""Position averaging in the replay ring (include/azg_pv.h azg_pv_replay_canon_keys,
azg_pv_replay_average) restated in Python integers and numpy float64.  Keys are integers, and
the means are fp64 sums in member order, divided and rounded to fp32 once: numpy's fp64
follows the header operation for operation (IEEE add, multiply, divide; a product of two fp32
values is exact in fp64, so a fused multiply-add on the device cannot differ), so there is
exactly one right answer and the kernels must give it.

All arrays here are in RING ORDER (oldest position first); the device's by-slot arrays are
rolled by the caller.

``python tests/replay_average_reference.py`` runs the self-checks (no GPU)."""
import numpy as np

N = 15
PIX = N * N
MASK = (1 << 64) - 1


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def sym_src(y: int, x: int, s: int) -> int:
    """csrc/pv_common.h sym_src: the board square that image square (y, x) of symmetry s reads."""
    if s & 1:
        x = N - 1 - x
    k = s >> 1
    if k == 0:
        return y * N + x
    if k == 1:
        return x * N + (N - 1 - y)
    if k == 2:
        return (N - 1 - y) * N + (N - 1 - x)
    return (N - 1 - x) * N + y


SRC = np.array([[sym_src(j // N, j % N, s) for j in range(PIX)] for s in range(8)], dtype=np.int64)   # [8, 225]
ZT = np.zeros((PIX, 3), dtype=np.uint64)   # ZT[j, v]; v = 0 (empty) contributes nothing
for _j in range(PIX):
    for _v in (1, 2):
        ZT[_j, _v] = splitmix64(2 * _j + _v - 1)
_J = np.arange(PIX)


def image(row: np.ndarray, s: int) -> np.ndarray:
    """Image s of a [225] row (stones or pi): img[j] = row[sym_src(j, s)]."""
    return np.asarray(row)[SRC[s]]


def image_hash(stones_row: np.ndarray, s: int) -> int:
    img = image(stones_row, s).astype(np.int64)
    return int(np.bitwise_xor.reduce(ZT[_J, img]))


def canon_key(stones_row: np.ndarray, nsym: int):
    """(key, sym): the smallest image hash as unsigned and the smallest s attaining it."""
    hs = [image_hash(stones_row, s) for s in range(nsym)]
    key = min(hs)
    return key, hs.index(key)


def canon_keys(stones: np.ndarray, nsym: int):
    """keys uint64 [n], syms int8 [n] for stones int8 [n, 225]."""
    ks = [canon_key(row, nsym) for row in stones]
    return np.array([k for k, _ in ks], dtype=np.uint64), np.array([s for _, s in ks], dtype=np.int8)


def canon_board(stones_row: np.ndarray, sym: int) -> np.ndarray:
    return image(stones_row, int(sym))


def average(stones, pis, zs, pw, nsym: int, keys=None):
    """stones int8 [n,225], pis fp32 [n,225], zs fp32 [n], pw fp32 [n] or None, ring order.
    keys (uint64 [n], optional) replaces the canonical keys in the sort only (the syms stay
    canon_keys'): all-equal keys leave the grouping to the board comparison alone.
    Returns a dict of ring-order arrays: pi_avg fp32 [n,225], z_avg fp32 [n], pw_avg fp32 [n]
    (None when pw is None), group_first int32 [n], group_size int32 [n], and keys / syms."""
    stones = np.asarray(stones, dtype=np.int8)
    pis = np.asarray(pis, dtype=np.float32)
    zs = np.asarray(zs, dtype=np.float32)
    n = len(stones)
    ckeys, syms = canon_keys(stones, nsym)
    sort_keys = ckeys if keys is None else np.asarray(keys, dtype=np.uint64)
    perm = np.argsort(sort_keys, kind="stable")
    ks = sort_keys[perm]
    w32 = np.ones(n, dtype=np.float32) if pw is None else np.asarray(pw, dtype=np.float32)
    # group starts: place 0, another key, or another canonical board than the place before
    starts = []
    for k in range(n):
        if k == 0 or ks[k] != ks[k - 1] or not np.array_equal(canon_board(stones[perm[k]], syms[perm[k]]),
                                                               canon_board(stones[perm[k - 1]], syms[perm[k - 1]])):
            starts.append(k)
    starts.append(n)
    pi_avg = np.empty((n, PIX), dtype=np.float32)
    z_avg = np.empty(n, dtype=np.float32)
    pw_avg = np.empty(n, dtype=np.float32)
    group_first = np.empty(n, dtype=np.int32)
    group_size = np.empty(n, dtype=np.int32)
    for a, b in zip(starts[:-1], starts[1:]):
        members = [int(r) for r in perm[a:b]]          # ring order: the sort is stable
        W = np.float64(0.0)
        Zs = np.float64(0.0)
        A = np.zeros(PIX, dtype=np.float64)
        for r in members:
            w = np.float64(w32[r])
            W = W + w
            A = A + w * pis[r][SRC[syms[r]]].astype(np.float64)
            Zs = Zs + np.float64(zs[r])
        cnt = np.float64(len(members))
        for r in members:
            if W > 0:
                row = np.empty(PIX, dtype=np.float32)
                row[SRC[syms[r]]] = (A / W).astype(np.float32)
                pi_avg[r] = row
            else:
                pi_avg[r] = pis[r]
            z_avg[r] = np.float32(Zs / cnt)
            pw_avg[r] = np.float32(W / cnt)
            group_first[r] = members[0]
            group_size[r] = len(members)
    return {"pi_avg": pi_avg, "z_avg": z_avg, "pw_avg": None if pw is None else pw_avg, "group_first": group_first,
            "group_size": group_size, "keys": ckeys, "syms": syms}


def random_position(rng, stones_n: int) -> np.ndarray:
    """int8 [225] with stones_n stones, alternately 1 and 2, on distinct random squares."""
    row = np.zeros(PIX, dtype=np.int8)
    sq = rng.choice(PIX, size=stones_n, replace=False)
    row[sq] = 1 + (np.arange(stones_n) % 2)
    return row


def random_pi(rng, n: int) -> np.ndarray:
    p = rng.random((n, PIX)).astype(np.float32)
    return (p / p.sum(axis=1, keepdims=True)).astype(np.float32)


def self_check() -> None:
    # the published first output of splitmix64 seeded with 0
    assert splitmix64(0) == 0xE220A8397B1DCDAF
    # sym_src is np.rot90 by s // 2, then a column flip when s is odd (MCTS.symmetries' order)
    board = np.arange(PIX).reshape(N, N)
    for s in range(8):
        want = np.rot90(board, s >> 1)
        if s & 1:
            want = np.flip(want, axis=1)
        assert np.array_equal(image(board.reshape(-1), s), want.reshape(-1)), s
    rng = np.random.default_rng(1)
    # the 8 images of a position: one key, one canonical board
    for _ in range(20):
        row = random_position(rng, int(rng.integers(1, 30)))
        key, sym = canon_key(row, 8)
        canon = canon_board(row, sym)
        for s in range(8):
            k2, s2 = canon_key(image(row, s), 8)
            assert k2 == key and np.array_equal(canon_board(image(row, s), s2), canon)
    assert canon_key(np.zeros(PIX, np.int8), 8) == (0, 0) and canon_key(np.zeros(PIX, np.int8), 1) == (0, 0)
    # a singleton's mean is its own target: (p * w) / w rounds back to p
    stones = np.stack([random_position(rng, 5 + i) for i in range(6)])
    pis, zs = random_pi(rng, 6), rng.choice([-1.0, 0.0, 1.0], size=6).astype(np.float32)
    pw = np.array([0.25, 3.0, 1.0, 0.7, 1e-3, 2.5], dtype=np.float32)
    out = average(stones, pis, zs, pw, 8)
    assert np.array_equal(out["pi_avg"], pis) and np.array_equal(out["z_avg"], zs) and np.array_equal(out["pw_avg"], pw)
    assert np.array_equal(out["group_size"], np.ones(6, np.int32)) and np.array_equal(out["group_first"], np.arange(6))
    # two copies: the plain mean
    out = average(np.stack([stones[0], stones[0]]), pis[:2], np.array([1.0, -1.0], np.float32), None, 8)
    want = ((pis[0].astype(np.float64) + pis[1].astype(np.float64)) / 2.0).astype(np.float32)
    assert np.array_equal(out["pi_avg"][0], want) and np.array_equal(out["pi_avg"][1], want)
    assert np.array_equal(out["z_avg"], np.zeros(2, np.float32)) and out["pw_avg"] is None
    assert out["group_size"].tolist() == [2, 2] and out["group_first"].tolist() == [0, 0]


if __name__ == "__main__":
    self_check()
    print("replay_average_reference: self-checks pass")
