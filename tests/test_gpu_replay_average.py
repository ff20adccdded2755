"""Position averaging in the device replay ring (azg_pv_replay_canon_keys,
azg_pv_replay_average, DeviceReplayBuffer.set_target_averaging, train_alphazero(
average_duplicates=True)) on the GPU.  Keys are integers and the means are fp64 sums in ring
order rounded once, so every comparison with tests/replay_average_reference.py is bit for
bit; there is no tolerance anywhere.

The rings hold a mix of: the empty board, a lone centre stone (its own 8 images), an
asymmetric board stored as all eight of its images, exact repeats of another board, and
distinct positions -- 36 positions, in a fixed shuffled order, with random pi and z of mixed
sign inside every group."""
import io
import random
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import replay_average_reference as ref
import replay_weights_reference as wref
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

DEV = "cuda:0"
PIX = ref.PIX


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _examples(stones, pis, zs):
    """(state [3,15,15], pi [225], z) tuples of int8 stones [n,225]."""
    out = []
    for row, pi, z in zip(stones, pis, zs):
        b = row.reshape(15, 15)
        out.append((np.stack([b == 1, b == 2, np.ones_like(b, dtype=bool)]).astype(np.float32), pi, float(z)))
    return out


def _asymmetric(rng, stones_n):
    while True:
        row = ref.random_position(rng, stones_n)
        if len({ref.image(row, s).tobytes() for s in range(8)}) == 8:
            return row


def _mix(seed=5):
    """The 36 positions described above: stones int8 [36,225], pis, zs, and policy weights
    with 0.0, 0.25 and 3.0 among them and one group (the centre stones) all zero."""
    rng = np.random.default_rng(seed)
    empty = np.zeros(PIX, np.int8)
    centre = empty.copy()
    centre[112] = 1
    a, b = _asymmetric(rng, 7), _asymmetric(rng, 12)
    rows = [empty] * 3 + [centre] * 2 + [ref.image(a, s) for s in range(8)] + [b] * 3
    rows += [_asymmetric(rng, 3 + i) for i in range(20)]          # distinct stone counts: distinct boards
    kind = ["empty"] * 3 + ["centre"] * 2 + ["a"] * 8 + ["b"] * 3 + ["d"] * 20
    order = rng.permutation(len(rows))
    stones = np.stack([rows[i] for i in order])
    kind = [kind[i] for i in order]
    n = len(stones)
    pis = ref.random_pi(rng, n)
    zs = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)
    zs[rng.integers(0, n, size=4)] = 0.0
    pw = rng.choice(np.array([0.0, 0.25, 1.0, 3.0], np.float32), size=n)
    pw[[i for i, k in enumerate(kind) if k == "centre"]] = 0.0
    ia = [i for i, k in enumerate(kind) if k == "a"]
    pw[ia[0]], pw[ia[1]], pw[ia[2]] = 0.0, 0.25, 3.0
    assert {-1.0, 1.0} <= set(zs[ia].tolist())
    return stones, pis, zs, pw.astype(np.float32)


def _filler(n, seed=6):
    rng = np.random.default_rng(seed)
    stones = np.stack([_asymmetric(rng, 30 + i) for i in range(n)])
    return stones, ref.random_pi(rng, n), rng.choice([-1.0, 1.0], size=n).astype(np.float32)


# name -> (nsym, cap_pos, fillers added first, positions of the mix added)
CONFIGS = {"wrapped": (8, 40, 9, 36),      # 45 into 40: head = 5, the ring wraps, count == cap_pos
           "partial": (8, 64, 0, 36),      # count < cap_pos, head = 0
           "one": (8, 8, 0, 1),            # count == 1
           "single_images": (1, 40, 9, 36)}   # nsym = 1: images are not merged, exact repeats are
_cache = {}


def _ring(name, weighted):
    """(buffer with averaging on, ring-order host arrays (stones, pis, zs, pw or None))."""
    from replay import DeviceReplayBuffer
    nsym, cap_pos, n_fill, n_mix = CONFIGS[name]
    stones, pis, zs, pw = (v[:n_mix] for v in _mix())
    dev = DeviceReplayBuffer(cap_pos * nsym, DEV, symmetries=nsym == 8)
    if n_fill:
        fs, fp, fz = _filler(n_fill)
        dev.add_positions(_examples(fs, fp, fz))
        stones, pis, zs = np.concatenate([fs, stones]), np.concatenate([fp, pis]), np.concatenate([fz, zs])
        pw = np.concatenate([np.ones(n_fill, np.float32), pw])     # added without weights: 1.0
    dev.add_positions(_examples(stones[n_fill:], pis[n_fill:], zs[n_fill:]),
                      policy_weight=pw[n_fill:] if weighted else None)
    keep = slice(max(0, len(stones) - cap_pos), None)
    assert dev.count == min(cap_pos, len(stones)) and dev.head == (len(stones) - dev.count) % cap_pos
    dev.set_target_averaging(True)
    return dev, (stones[keep], pis[keep], zs[keep], pw[keep] if weighted else None)


def _reference(name, weighted):
    """Computed once per ring and shared; nobody writes to it."""
    key = (name, weighted)
    if key not in _cache:
        nsym = CONFIGS[name][0]
        stones, pis, zs, pw = (v[:CONFIGS[name][3]] for v in _mix())
        n_fill, cap_pos = CONFIGS[name][2], CONFIGS[name][1]
        if n_fill:
            fs, fp, fz = _filler(n_fill)
            stones, pis, zs = np.concatenate([fs, stones]), np.concatenate([fp, pis]), np.concatenate([fz, zs])
            pw = np.concatenate([np.ones(n_fill, np.float32), pw])
        keep = slice(max(0, len(stones) - cap_pos), None)
        out = ref.average(stones[keep], pis[keep], zs[keep], pw[keep] if weighted else None, nsym)
        for v in out.values():
            if v is not None:
                v.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _assert_equals_reference(got, want):
    assert np.array_equal(got["keys"], want["keys"])
    assert np.array_equal(got["syms"], want["syms"])
    assert np.array_equal(got["group_first"], want["group_first"])
    assert np.array_equal(got["group_size"], want["group_size"])
    assert np.array_equal(_bits(got["pi"]), _bits(want["pi_avg"]))
    assert np.array_equal(_bits(got["z"]), _bits(want["z_avg"]))
    if want["pw_avg"] is None:
        assert got["policy_weight"] is None
    else:
        assert np.array_equal(_bits(got["policy_weight"]), _bits(want["pw_avg"]))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_keys_and_syms_equal_the_reference(name):
    dev, (stones, _, _, _) = _ring(name, False)
    got, want = dev.get_averaged_targets(), _reference(name, False)
    assert got["keys"].dtype == np.uint64 and np.array_equal(got["keys"], want["keys"])
    assert got["syms"].dtype == np.int8 and np.array_equal(got["syms"], want["syms"])
    if name in ("wrapped", "partial"):     # the mix is what it claims to be
        empties = [i for i in range(len(stones)) if not stones[i].any()]
        assert len(empties) == 3 and all(got["keys"][i] == 0 and got["syms"][i] == 0 for i in empties)
        assert sorted(np.unique(want["group_size"]).tolist()) == [1, 2, 3, 8]
    if name == "single_images":
        assert not want["syms"].any() and sorted(np.unique(want["group_size"]).tolist()) == [1, 2, 3]


@pytest.mark.parametrize("weighted", [False, True], ids=["unit_weights", "policy_weights"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_averages_and_groups_equal_the_reference(name, weighted):
    dev, _ = _ring(name, weighted)
    want = _reference(name, weighted)
    _assert_equals_reference(dev.get_averaged_targets(), want)
    assert np.array_equal(dev.get_group_sizes(), want["group_size"])
    firsts = want["group_first"]
    assert dev.duplicate_stats() == {"positions": len(firsts), "largest": int(want["group_size"].max()),
                                     "groups": int((firsts == np.arange(len(firsts))).sum())}
    if weighted and name != "one":    # the all-zero group kept its own rows and has weight 0
        assert ((want["pw_avg"] == 0.0) & (want["group_size"] >= 2)).sum() >= 2


@pytest.mark.parametrize("n_empty,n_centre,n_other", [(64, 0, 0), (257, 256, 30)],
                         ids=["whole_ring_one_group", "groups_of_257_and_256"])
def test_long_groups(n_empty, n_centre, n_other):
    """Every position the empty board: one group spans the ring.  And groups longer than the
    256 members the averaging workgroup stages at a time, one of them ending on that boundary."""
    from replay import DeviceReplayBuffer
    rng = np.random.default_rng(21)
    centre = np.zeros(PIX, np.int8)
    centre[112] = 2
    rows = [np.zeros(PIX, np.int8)] * n_empty + [centre] * n_centre + [_asymmetric(rng, 4 + i) for i in range(n_other)]
    stones = np.stack([rows[i] for i in rng.permutation(len(rows))])
    n = len(stones)
    pis, zs = ref.random_pi(rng, n), rng.choice([-1.0, 0.0, 1.0], size=n).astype(np.float32)
    pw = rng.choice(np.array([0.0, 0.25, 1.0, 3.0], np.float32), size=n)
    dev = DeviceReplayBuffer(8 * n, DEV)
    dev.add_positions(_examples(stones, pis, zs), policy_weight=pw)
    dev.set_target_averaging(True)
    want = ref.average(stones, pis, zs, pw, 8)
    _assert_equals_reference(dev.get_averaged_targets(), want)
    assert dev.duplicate_stats()["largest"] == n_empty and dev.duplicate_stats()["groups"] == (n_centre > 0) + 1 + n_other


def test_equal_keys_leave_the_grouping_to_the_board_comparison():
    """azg_pv_replay_average at the C-ABI with keys_sorted all equal and perm the identity:
    groups are the runs of equal canonical boards in ring order, and unequal boards never merge."""
    from _native import check, load_library, ptr
    lib = load_library()
    rng = np.random.default_rng(31)
    a, b, c = _asymmetric(rng, 6), _asymmetric(rng, 6), _asymmetric(rng, 9)
    rows = [a, ref.image(a, 3), b, b, ref.image(b, 6), a, c, ref.image(c, 1), a, ref.image(a, 7)]
    stones = np.stack(rows * 4)[:37]
    n, cap_pos, head = len(stones), 41, 17
    pis, zs = ref.random_pi(rng, n), rng.choice([-1.0, 1.0], size=n).astype(np.float32)
    pw = rng.choice(np.array([0.0, 0.25, 3.0], np.float32), size=n)
    want = ref.average(stones, pis, zs, pw, 8, keys=np.zeros(n, np.uint64))
    assert want["group_size"][:10].tolist() == [2, 2, 3, 3, 3, 1, 2, 2, 4, 4]     # a a | b b b | a | c c | a a (a a ...)
    slots = (head + np.arange(n)) % cap_pos

    def by_slot(x, dtype):
        out = np.zeros((cap_pos,) + x.shape[1:], dtype)
        out[slots] = x
        return torch.from_numpy(out).to(DEV)

    d_st, d_pi, d_z, d_pw = by_slot(stones, np.int8), by_slot(pis, np.float32), by_slot(zs, np.float32), by_slot(pw, np.float32)
    d_keys = torch.zeros(n, dtype=torch.int64, device=DEV)
    d_syms = torch.zeros(n, dtype=torch.int8, device=DEV)
    with torch.cuda.device(DEV):
        st = torch.cuda.current_stream().cuda_stream
        check(lib.azg_pv_replay_canon_keys(ptr(d_st), cap_pos, head, n, 8, ptr(d_keys), ptr(d_syms), st), lib)
        assert np.array_equal(d_keys.cpu().numpy().view(np.uint64), want["keys"])
        assert np.array_equal(d_syms.cpu().numpy(), want["syms"])
        same = torch.zeros(n, dtype=torch.int64, device=DEV)
        perm = torch.arange(n, dtype=torch.int64, device=DEV)
        pi_avg = torch.full((cap_pos, PIX), -7.0, device=DEV)
        z_avg, pw_avg = torch.full((cap_pos,), -7.0, device=DEV), torch.full((cap_pos,), -7.0, device=DEV)
        first = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        size = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        check(lib.azg_pv_replay_average(ptr(d_st), ptr(d_pi), ptr(d_z), ptr(d_pw), cap_pos, head, n, ptr(same),
                                        ptr(perm), ptr(d_syms), ptr(pi_avg), ptr(z_avg), ptr(pw_avg), ptr(first),
                                        ptr(size), st), lib)
    assert np.array_equal(first.cpu().numpy(), want["group_first"])
    assert np.array_equal(size.cpu().numpy(), want["group_size"])
    assert np.array_equal(_bits(pi_avg.cpu().numpy()[slots]), _bits(want["pi_avg"]))
    assert np.array_equal(_bits(z_avg.cpu().numpy()[slots]), _bits(want["z_avg"]))
    assert np.array_equal(_bits(pw_avg.cpu().numpy()[slots]), _bits(want["pw_avg"]))
    free = np.setdiff1d(np.arange(cap_pos), slots)       # slots outside the ring are not written
    assert (pi_avg.cpu().numpy()[free] == -7.0).all() and (z_avg.cpu().numpy()[free] == -7.0).all()


def test_eight_images_with_eight_policies_gathered_under_every_symmetry():
    """One board stored as its 8 images, each with its own pi.  Every member's averaged row,
    gathered as image s, is the host's mean (formed in the board's own orientation with
    replay._images, summed in member order in fp64) under the member's and then the sampled
    symmetry."""
    from replay import DeviceReplayBuffer, _images
    rng = np.random.default_rng(41)
    board = _asymmetric(rng, 11)
    pis = ref.random_pi(rng, 8)
    stones = np.stack([ref.image(board, m) for m in range(8)])
    assert all(np.array_equal(stones[m].reshape(1, 15, 15),
                              _images(board.reshape(1, 1, 15, 15), board.reshape(1, 15, 15))[m][1].reshape(1, 15, 15))
               for m in range(8))
    # member m is image m of the board; image t of it that gives the board back undoes m
    back = []
    for m in range(8):
        imgs = _images(stones[m].reshape(1, 1, 15, 15), pis[m].reshape(1, 15, 15))
        t = [t for t in range(8) if np.array_equal(imgs[t][0].reshape(-1), board)]
        assert len(t) == 1
        back.append(imgs[t[0]][1].reshape(-1).astype(np.float64))
    acc = np.zeros(PIX)
    for m in range(8):
        acc = acc + back[m]
    mean = (acc / 8.0).astype(np.float32)
    dev = DeviceReplayBuffer(64, DEV)
    dev.add_positions(_examples(stones, pis, np.array([1, -1, 1, 1, -1, -1, 1, -1], np.float32)))
    dev.set_target_averaging(True)
    s, p, z = dev.sample(64, ids=list(range(64)))
    p = p.cpu().numpy()
    for m in range(8):
        own = _images(mean.reshape(1, 1, 15, 15), mean.reshape(1, 15, 15))[m][1]       # in member m's orientation
        want = _images(own.reshape(1, 1, 15, 15), own.reshape(1, 15, 15))
        for sym in range(8):
            assert np.array_equal(_bits(p[m * 8 + sym]), _bits(want[sym][1].reshape(-1))), (m, sym)
    assert np.array_equal(z.cpu().numpy(), np.zeros((64, 1), np.float32))
    assert dev.duplicate_stats() == {"positions": 8, "groups": 1, "largest": 8}


def _rnd(batch, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, size=(batch, 2), dtype=np.uint64)


def test_without_duplicates_sampling_is_bit_identical_on_and_off():
    from replay import DeviceReplayBuffer
    fs, fp, fz = _filler(12, seed=51)
    pw = np.array([0.0, 0.25, 3.0, 1.0] * 3, np.float32)
    dev = DeviceReplayBuffer(8 * 9, DEV)                 # 12 into 9: wrapped
    dev.add_positions(_examples(fs, fp, fz), policy_weight=pw)
    ids = np.random.default_rng(52).integers(0, 72, size=300).tolist()
    rnd = _rnd(300, 53)
    off = dev.sample(300, ids=ids, with_policy_weight=True) + dev.sample_weighted(300, rnd=rnd, with_policy_weight=True)
    assert dev._avg is None and not dev.target_averaging
    dev.set_target_averaging(True)
    assert dev.target_averaging
    on = dev.sample(300, ids=ids, with_policy_weight=True) + dev.sample_weighted(300, rnd=rnd, with_policy_weight=True)
    assert dev.duplicate_stats() == {"positions": 9, "groups": 9, "largest": 1}
    assert len(on) == len(off) == 8 and all(torch.equal(a, b) for a, b in zip(on, off))


@pytest.mark.parametrize("name", ["wrapped", "single_images"])
def test_with_duplicates_sampling_returns_the_averaged_rows(name):
    dev, (stones, pis, zs, pw) = _ring(name, True)
    want = _reference(name, True)
    nsym, count = dev.nsym, dev.count
    rng = np.random.default_rng(61)
    ids = np.concatenate([rng.permutation(count * nsym), rng.integers(0, count * nsym, size=40)])

    def expect(ids):
        pos, sym = np.asarray(ids) // nsym, np.asarray(ids) % nsym
        return (np.stack([ref.image(want["pi_avg"][i], s) for i, s in zip(pos, sym)]), want["z_avg"][pos].reshape(-1, 1),
                want["pw_avg"][pos], np.stack([ref.image(stones[i], s) for i, s in zip(pos, sym)]))

    s, p, z, w = dev.sample(len(ids), ids=ids.tolist(), with_policy_weight=True)
    ep, ez, ew, es = expect(ids)
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(ep)) and np.array_equal(_bits(z.cpu().numpy()), _bits(ez))
    assert np.array_equal(_bits(w.cpu().numpy()), _bits(ew))
    assert np.array_equal(s.cpu().numpy()[:, 0].reshape(len(ids), -1), (es == 1).astype(np.float32))
    s3, p3, z3 = dev.sample(len(ids), ids=ids.tolist())
    assert torch.equal(p3, p) and torch.equal(z3, z) and torch.equal(s3, s)
    # the weighted draw is untouched: the ids of the integer restatement, every weight 1.0
    rnd = _rnd(64, 62)
    wid = wref.draw_ids(np.arange(1, count + 1, dtype=np.uint64) * np.uint64(1 << 16), nsym, rnd)
    s, p, z, w = dev.sample_weighted(64, rnd=rnd, with_policy_weight=True)
    ep, ez, ew, es = expect(wid)
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(ep)) and np.array_equal(_bits(z.cpu().numpy()), _bits(ez))
    assert np.array_equal(_bits(w.cpu().numpy()), _bits(ew))
    assert np.array_equal(s.cpu().numpy()[:, 1].reshape(64, -1), (es == 2).astype(np.float32))
    # switching averaging off restores the raw sample bit for bit, and to_host never changed
    dev.set_target_averaging(False)
    s, p, z, w = dev.sample(len(ids), ids=ids.tolist(), with_policy_weight=True)
    pos, sym = ids // nsym, ids % nsym
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(np.stack([ref.image(pis[i], k) for i, k in zip(pos, sym)])))
    assert np.array_equal(_bits(z.cpu().numpy().reshape(-1)), _bits(zs[pos]))
    assert np.array_equal(_bits(w.cpu().numpy()), _bits(pw[pos]))


def test_to_host_is_unchanged_by_averaging():
    plain, _ = _ring("wrapped", True)
    plain.set_target_averaging(False)
    averaged, _ = _ring("wrapped", True)
    averaged.sample(8)      # refreshed
    ha, hb = list(averaged.to_host().buffer), list(plain.to_host().buffer)
    assert len(ha) == len(hb) == 320
    for ea, eb in zip(ha, hb):
        assert len(ea) == len(eb) == 3
        assert np.array_equal(ea[0], eb[0]) and np.array_equal(ea[1], eb[1]) and ea[2] == eb[2]
    assert np.array_equal(averaged.get_policy_weights(), plain.get_policy_weights())


def test_eviction_and_new_policy_weights_regroup_on_the_next_sample():
    """add_positions evicts part of a group (and adds to another); set_policy_weights changes
    the weights: the next sample reflects each, with no explicit refresh."""
    from replay import DeviceReplayBuffer
    stones, pis, zs, pw = _mix()
    cap_pos = 40
    dev = DeviceReplayBuffer(8 * cap_pos, DEV)
    dev.set_target_averaging(True)
    dev.add_positions(_examples(stones, pis, zs), policy_weight=pw)
    ids = list(range(8 * 36))
    dev.sample(len(ids), ids=ids)
    before = dev.get_averaged_targets()
    _assert_equals_reference(before, ref.average(stones, pis, zs, pw, 8))
    rng = np.random.default_rng(71)
    more = np.stack([np.zeros(PIX, np.int8)] * 2 + [_asymmetric(rng, 40 + i) for i in range(10)])
    mp, mz = ref.random_pi(rng, 12), rng.choice([-1.0, 1.0], size=12).astype(np.float32)
    dev.add_positions(_examples(more, mp, mz))           # 48 into 40: the 8 oldest leave; new ones count 1.0
    all_st, all_pi, all_z = np.concatenate([stones, more])[8:], np.concatenate([pis, mp])[8:], np.concatenate([zs, mz])[8:]
    all_pw = np.concatenate([pw, np.ones(12, np.float32)])[8:]
    want = ref.average(all_st, all_pi, all_z, all_pw, 8)
    assert not np.array_equal(np.sort(want["group_size"]), np.sort(before["group_size"]))
    ids = np.arange(8 * cap_pos)
    s, p, z, w = dev.sample(len(ids), ids=ids.tolist(), with_policy_weight=True)
    assert np.array_equal(_bits(p.cpu().numpy()[::8]), _bits(np.stack([ref.image(r, 0) for r in want["pi_avg"]])))
    assert np.array_equal(_bits(z.cpu().numpy()[::8, 0]), _bits(want["z_avg"]))
    assert np.array_equal(_bits(w.cpu().numpy()[::8]), _bits(want["pw_avg"]))
    _assert_equals_reference(dev.get_averaged_targets(), want)
    new_pw = np.roll(all_pw, 3)
    dev.set_policy_weights(new_pw)
    want = ref.average(all_st, all_pi, all_z, new_pw, 8)
    s, p, z, w = dev.sample(len(ids), ids=ids.tolist(), with_policy_weight=True)
    assert np.array_equal(_bits(p.cpu().numpy()[::8]), _bits(want["pi_avg"]))
    assert np.array_equal(_bits(w.cpu().numpy()[::8]), _bits(want["pw_avg"]))


def test_loop_iteration_reports_groups(tmp_path, monkeypatch):
    import _native
    import replay
    import train
    lib, calls = _native.load_library(), {}
    for name in ("azg_pv_replay_canon_keys", "azg_pv_replay_average"):     # counting wrappers
        calls[name] = 0

        def wrapper(*a, _fn=getattr(lib, name), _name=name):
            calls[_name] += 1
            return _fn(*a)

        monkeypatch.setattr(lib, name, wrapper)
    buffers = []
    new_buffer = replay.new_device_buffer
    monkeypatch.setattr(replay, "new_device_buffer", lambda *a: buffers.append(new_buffer(*a)) or buffers[-1])
    kw = dict(num_iterations=1, games_per_iteration=4, n_simulations=8, batch_size=16, epochs_per_iter=1, eval_games=2,
              eval_mcts_simulations=8, win_rate_threshold=0.0, n_res_blocks=2, channels=64, max_moves=6, device=DEV)
    out = {}
    for flag in (False, True):
        random.seed(3)
        np.random.seed(3)
        torch.manual_seed(3)
        history, log = [], io.StringIO()
        with redirect_stdout(log):
            train.train_alphazero(model_dir=str(tmp_path / f"avg{int(flag)}"), device_buffer=True, history=history,
                                  **({"average_duplicates": True} if flag else {}), **kw)
        assert "last_loss={" in log.getvalue() and len(history) == 1
        out[flag] = history[0]
        if not flag:     # the default: no new entry point is called, nothing is allocated
            assert calls == dict.fromkeys(calls, 0) and buffers[-1]._avg is None and not buffers[-1].target_averaging
    assert out[False]["buffer_groups"] is None
    assert calls["azg_pv_replay_canon_keys"] >= 1 and calls["azg_pv_replay_average"] == calls["azg_pv_replay_canon_keys"]
    g = out[True]["buffer_groups"]
    assert set(g) == {"positions", "groups", "largest"}
    assert g["positions"] == 24 and g["groups"] < g["positions"] and g["largest"] >= 4    # 4 games from the empty board
    # the buffer that iteration trained on: every position is in exactly one group
    dev = buffers[-1]
    sizes, firsts = dev.get_group_sizes(), dev.get_averaged_targets()["group_first"]
    assert dev.target_averaging and dev.nsym == 8 and dev.duplicate_stats() == g
    starts = np.flatnonzero(firsts == np.arange(len(firsts)))
    assert len(starts) == g["groups"] and int(sizes[starts].sum()) == g["positions"] == len(sizes)
    assert all(sizes[i] == sizes[firsts[i]] for i in range(len(sizes)))
    with pytest.raises(ValueError, match="device_buffer"):
        train.train_alphazero(model_dir=str(tmp_path / "bad"), average_duplicates=True, **kw)
