"""The Python restatement of position averaging (tests/replay_average_reference.py) checked
against its own definition, without a GPU: the GPU tests compare the kernels with it bit for
bit, so its invariants are pinned here.  Every comparison is exact."""
import numpy as np
import pytest

import replay_average_reference as ref


def _asymmetric(rng, stones_n):
    while True:
        row = ref.random_position(rng, stones_n)
        if len({ref.image(row, s).tobytes() for s in range(8)}) == 8:
            return row


def test_reference_self_checks():
    ref.self_check()


def test_eight_images_share_one_key_and_one_canonical_board():
    rng = np.random.default_rng(11)
    seen = {}
    for _ in range(200):
        row = ref.random_position(rng, int(rng.integers(1, 41)))
        key, sym = ref.canon_key(row, 8)
        canon = ref.canon_board(row, sym)
        for s in range(8):
            img = ref.image(row, s)
            k2, s2 = ref.canon_key(img, 8)
            assert k2 == key
            assert np.array_equal(ref.canon_board(img, s2), canon)
        assert seen.setdefault(key, canon.tobytes()) == canon.tobytes()   # no two boards under one key
    # a lone centre stone is its own 8 images: sym is the smallest s
    centre = np.zeros(ref.PIX, np.int8)
    centre[112] = 1
    assert ref.canon_key(centre, 8) == (int(ref.ZT[112, 1]), 0)


def test_single_images_merge_exact_repeats_only():
    rng = np.random.default_rng(12)
    row = _asymmetric(rng, 9)
    stones = np.stack([row, ref.image(row, 3), row])
    out = ref.average(stones, ref.random_pi(rng, 3), np.array([1, -1, -1], np.float32), None, 1)
    assert out["group_size"].tolist() == [2, 1, 2] and out["group_first"].tolist() == [0, 1, 0]
    assert out["syms"].tolist() == [0, 0, 0]
    out8 = ref.average(stones, ref.random_pi(rng, 3), np.array([1, -1, -1], np.float32), None, 8)
    assert out8["group_size"].tolist() == [3, 3, 3]


@pytest.mark.parametrize("weighted", [False, True])
def test_average_is_unchanged_when_members_are_replaced_by_their_images(weighted):
    """Three boards, 5 + 3 + 1 copies interleaved.  Replacing every member by a random image
    of itself (stones and pi alike) gives the same means, each in the member's new orientation."""
    rng = np.random.default_rng(13)
    boards = [_asymmetric(rng, n) for n in (7, 12, 20)]
    which = np.array([0, 1, 0, 0, 2, 1, 0, 1, 0])
    n = len(which)
    stones = np.stack([boards[b] for b in which])
    pis = ref.random_pi(rng, n)
    zs = rng.choice([-1.0, 1.0], size=n).astype(np.float32)
    pw = rng.choice([0.0, 0.25, 1.0, 3.0], size=n).astype(np.float32) if weighted else None
    base = ref.average(stones, pis, zs, pw, 8)
    assert sorted(set(base["group_size"].tolist())) == [1, 3, 5]
    ss = rng.integers(0, 8, size=n)
    stones2 = np.stack([ref.image(stones[i], ss[i]) for i in range(n)])
    pis2 = np.stack([ref.image(pis[i], ss[i]) for i in range(n)])
    moved = ref.average(stones2, pis2, zs, pw, 8)
    for i in range(n):
        assert np.array_equal(moved["pi_avg"][i], ref.image(base["pi_avg"][i], ss[i]))
    for k in ("z_avg", "group_first", "group_size", "keys"):
        assert np.array_equal(moved[k], base[k])
    if weighted:
        assert np.array_equal(moved["pw_avg"], base["pw_avg"])


def test_singletons_come_out_bit_equal():
    rng = np.random.default_rng(14)
    n = 40
    stones = np.stack([ref.random_position(rng, 3 + i) for i in range(n)])   # distinct stone counts: no duplicates
    pis = ref.random_pi(rng, n)
    pis[:, ::7] = 0.0
    zs = rng.choice([-1.0, 0.0, 1.0], size=n).astype(np.float32)
    pw = np.abs(rng.standard_normal(n)).astype(np.float32) + np.float32(1e-6)
    for w in (None, pw):
        for nsym in (1, 8):
            out = ref.average(stones, pis, zs, w, nsym)
            assert np.array_equal(out["pi_avg"].view(np.uint32), pis.view(np.uint32))
            assert np.array_equal(out["z_avg"].view(np.uint32), zs.view(np.uint32))
            assert out["group_size"].tolist() == [1] * n and out["group_first"].tolist() == list(range(n))
            if w is not None:
                assert np.array_equal(out["pw_avg"].view(np.uint32), pw.view(np.uint32))


def test_unit_weights_equal_the_unweighted_mean():
    rng = np.random.default_rng(15)
    boards = [_asymmetric(rng, n) for n in (4, 9)]
    which = [0, 1, 1, 0, 0, 1, 0]
    stones = np.stack([ref.image(boards[b], int(rng.integers(0, 8))) for b in which])
    pis = ref.random_pi(rng, len(which))
    zs = rng.choice([-1.0, 1.0], size=len(which)).astype(np.float32)
    a = ref.average(stones, pis, zs, None, 8)
    b = ref.average(stones, pis, zs, np.ones(len(which), np.float32), 8)
    assert a["pw_avg"] is None and np.array_equal(b["pw_avg"], np.ones(len(which), np.float32))
    for k in ("pi_avg", "z_avg", "group_first", "group_size"):
        assert np.array_equal(a[k], b[k])
    # and it IS the mean: member 0's group in member 0's orientation, summed in ring order
    members = [i for i, w in enumerate(which) if w == 0]
    acc = np.zeros(ref.PIX)
    for m in members:
        acc = acc + ref.image(pis[m], a["syms"][m]).astype(np.float64)
    want = np.empty(ref.PIX, np.float32)
    want[ref.SRC[a["syms"][0]]] = (acc / 4.0).astype(np.float32)
    assert np.array_equal(a["pi_avg"][0], want)


def test_group_of_zero_weights_keeps_its_rows():
    rng = np.random.default_rng(16)
    board, other = _asymmetric(rng, 6), _asymmetric(rng, 8)
    stones = np.stack([board, ref.image(board, 5), other, ref.image(board, 2), other])
    pis = ref.random_pi(rng, 5)
    zs = np.array([1, -1, 1, -1, -1], np.float32)
    pw = np.array([0.0, 0.0, 0.0, 0.0, 3.0], np.float32)
    out = ref.average(stones, pis, zs, pw, 8)
    for i in (0, 1, 3):   # no trusted policy target in the group: own rows, weight 0, z still averaged
        assert np.array_equal(out["pi_avg"][i], pis[i])
        assert out["pw_avg"][i] == 0.0 and out["z_avg"][i] == np.float32(-1.0 / 3.0) and out["group_size"][i] == 3
    # the other group: a zero-weight member takes no part in the mean and gets the trusted target
    assert np.array_equal(out["pi_avg"][4], pis[4])
    assert np.array_equal(ref.image(out["pi_avg"][2], out["syms"][2]), ref.image(pis[4], out["syms"][4]))
    assert out["pw_avg"][2] == out["pw_avg"][4] == np.float32(1.5) and out["z_avg"][2] == 0.0
