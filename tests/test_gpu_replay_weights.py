"""Surprise-weighted sampling from the device replay buffer on the GPU
(csrc/pv_replay_weights.hip, replay.DeviceReplayBuffer.sample_weighted,
train_alphazero(surprise_weight=...)).  Weights are integers (65536 quanta per unit), so
every comparison is exact: the quanta, the uint64 running sums and every drawn id equal
tests/replay_weights_reference.py's, and proportionality is checked by counting on an
equally spaced grid of random words, with no statistics and no tolerance."""
import os
import random

import numpy as np
import pytest
import torch

import replay_weights_reference as ref
from conftest import has_gpu
from replay_helpers import synthetic_positions

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

DEV = "cuda:0"
QUANTA, QMAX = ref.QUANTA, ref.QMAX
SENTINEL = 7   # in weight slots no call may write


def _lib():
    import _native
    return _native.load_library()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _dev_u(a, dtype):
    """A numpy unsigned array on the device, as the signed torch dtype of the same width."""
    signed = {np.uint32: (np.int32, torch.int32), np.uint64: (np.int64, torch.int64)}[dtype]
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).view(signed[0])).to(DEV)


def _host_u(t, dtype):
    return t.cpu().numpy().view(dtype)


# ------------------------------------------------------------------------------ weights
def _surprises(n, seed):
    rng = np.random.default_rng(seed)
    s = (rng.random(n) ** 4 * 3.0).astype(np.float32)      # a long tail, as KLs have
    for i, v in enumerate((0.0, -1.5, np.nan, np.inf, -np.inf, 1e-30)):
        if 2 * i + 1 < n:
            s[2 * i + 1] = v
    return s


def _run_weights(s, mix, cap_pos, at, keep=None, records=False):
    from _native import check, ptr
    n_sum = len(s)
    n = n_sum if keep is None else keep
    if records:   # [n,8] score records: field 0 is read, the others never
        host = np.full((n_sum, 8), np.nan, dtype=np.float32)
        host[:, 0] = s
    else:
        host = s
    d_s = torch.from_numpy(np.ascontiguousarray(host)).to(DEV)
    w = torch.full((cap_pos,), SENTINEL, dtype=torch.int32, device=DEV)
    check(_lib().azg_pv_replay_surprise_weights(ptr(d_s), 8 if records else 1, n, n_sum, mix, ptr(w), cap_pos, at,
                                                _stream()))
    got = _host_u(w, np.uint32)
    want = np.full(cap_pos, SENTINEL, dtype=np.uint32)
    want[(at + np.arange(n)) % cap_pos] = ref.surprise_quanta(s, mix, keep=n)
    return got, want


@pytest.mark.parametrize("mix", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("n", [1, 37, 1025])
def test_weights_equal_reference_quantum_for_quantum(n, mix):
    s = _surprises(n, seed=n)
    got, want = _run_weights(s, mix, cap_pos=n + 5, at=2, records=n == 37)
    assert np.array_equal(got, want)
    if mix == 0.0:
        assert (got[2:2 + n] == QUANTA).all()
    if n > 1 and mix == 1.0:
        assert (got[2:2 + n][[1, 3, 5, 7]] == 0).all()      # 0, negative, NaN, inf: no weight at all


def test_weights_edge_cases():
    # all-zero (and all unusable) surprises: every weight exactly 1.0, whatever the mix
    for s in (np.zeros(37, np.float32), np.array([np.nan, -1.0, np.inf, 0.0], np.float32), np.array([np.nan], np.float32)):
        got, want = _run_weights(s, 0.7, cap_pos=40, at=0)
        assert np.array_equal(got, want) and (got[:len(s)] == QUANTA).all()
    # a write that wraps the ring
    got, want = _run_weights(_surprises(37, seed=2), 0.5, cap_pos=50, at=47)
    assert np.array_equal(got, want)
    assert (got[[47, 48, 49, 0, 33]] != SENTINEL).all() and (got[34:47] == SENTINEL).all()
    # more records than the ring holds: the newest cap_pos are written, normalised over all
    s = _surprises(1025, seed=3)
    got, want = _run_weights(s, 0.5, cap_pos=1000, at=997, keep=1000)
    assert np.array_equal(got, want)
    assert np.array_equal(got[(997 + np.arange(1000)) % 1000], ref.surprise_quanta(s, 0.5)[25:])
    # one dominant surprise among many: the weight stops at 2^31 - 1 quanta
    s = np.zeros(70000, np.float32)
    s[-1] = 2.0
    got, want = _run_weights(s, 1.0, cap_pos=70000, at=0)
    assert np.array_equal(got, want) and got[-1] == QMAX and not got[:-1].any()


# ------------------------------------------------------------------------------- prefix
def _run_prefix(ring, head, count):
    from _native import check, ptr
    d_w = _dev_u(ring, np.uint32)
    pre = torch.full((len(ring),), -1, dtype=torch.int64, device=DEV)
    check(_lib().azg_pv_replay_prefix(ptr(d_w), len(ring), head, count, ptr(pre), _stream()))
    got = _host_u(pre, np.uint64)
    assert (got[count:] == np.uint64(2 ** 64 - 1)).all()      # nothing written past count
    return got[:count]


@pytest.fixture(scope="module")
def ring2050():
    rng = np.random.default_rng(11)
    ring = rng.integers(0, 1 << 18, size=2050, dtype=np.uint32)
    ring[rng.integers(0, 2050, size=200)] = 0
    ring[rng.integers(0, 2050, size=300)] = QMAX              # sums pass 2^32 within a few elements
    ring[[0, 1, 2, 2047, 2048, 2049]] = QMAX
    return ring


@pytest.mark.parametrize("head", [0, 2047])
@pytest.mark.parametrize("count", [1, 64, 65, 1024, 1025, 2050])
def test_prefix_equals_uint64_cumsum(ring2050, count, head):
    want = ref.prefix_sums(ring2050, head, count)
    assert count < 64 or int(want[-1]) > 1 << 32
    assert np.array_equal(_run_prefix(ring2050, head, count), want)


def test_prefix_more_tiles_than_one_round_of_totals():
    # 256 tiles of 1024 positions fill one round of the tile-total scan: 256 * 1024 + 5
    # positions need a second round with a carry (the path a ring of ~10^6 positions takes)
    n = 256 * 1024 + 5
    rng = np.random.default_rng(12)
    ring = rng.integers(0, QMAX, size=n + 3, dtype=np.uint32)
    assert np.array_equal(_run_prefix(ring, n - 1000, n), ref.prefix_sums(ring, n - 1000, n))


# --------------------------------------------------------------------------------- draw
def _run_draw(prefix, nsym, rnd):
    from _native import check, ptr
    rnd = np.asarray(rnd, dtype=np.uint64).reshape(-1, 2)
    d_pre, d_rnd = _dev_u(prefix, np.uint64), _dev_u(rnd, np.uint64)
    ids = torch.full((len(rnd),), -1, dtype=torch.int64, device=DEV)
    check(_lib().azg_pv_replay_draw(ptr(d_pre), len(prefix), nsym, ptr(d_rnd), len(rnd), ptr(ids), _stream()))
    return ids.cpu().numpy().tolist()


@pytest.mark.parametrize("nsym", [1, 8])
def test_draw_equals_reference_at_every_boundary(nsym):
    rng = np.random.default_rng(21)
    w = rng.integers(1, 1 << 20, size=301, dtype=np.uint64)
    w[[0, 7, 8, 9, 150, 299, 300]] = 0                        # zero weights, first and last included
    w[[40, 41]] = QMAX
    pre = np.cumsum(w, dtype=np.uint64)
    total = int(pre[-1])
    words = [0, 1, (1 << 64) - 1, (1 << 64) - 2, 1 << 63]
    targets = [int(pre[j]) - d for j in (1, 6, 10, 40, 41, 149, 151, 297) for d in (1, 0)]   # t on prefix[j] - 1
    for t in targets + [total - 1]:                                                          # and on prefix[j]
        words += [ref.word_for(t, total), max(0, ref.word_for(t, total) - 1)]
    words += [int(v) for v in rng.integers(0, 1 << 64, size=300, dtype=np.uint64)]
    rnd = [[r, int(s)] for r, s in zip(words, rng.integers(0, 1 << 64, size=len(words), dtype=np.uint64))]
    got = _run_draw(pre, nsym, rnd)
    assert got == ref.draw_ids(pre, nsym, rnd)
    chosen = np.array(got) // nsym
    assert w[chosen].all()                                    # a zero-weight position is never chosen
    assert chosen.min() == 1 and chosen.max() == 298          # words 0 and 2^64 - 1 skip the zero-weight ends
    if nsym == 8:
        assert len(set(np.array(got) % 8)) == 8


def test_draw_single_position_and_long_prefix():
    assert _run_draw(np.array([5], np.uint64), 8, [[0, 3], [(1 << 64) - 1, 12]]) == [3, 4]
    pre = np.cumsum(np.full(100003, QMAX, dtype=np.uint64))   # 17 search steps, total past 2^47
    rng = np.random.default_rng(22)
    rnd = rng.integers(0, 1 << 64, size=(257, 2), dtype=np.uint64)   # two workgroups of the draw
    assert _run_draw(pre, 1, rnd) == ref.draw_ids(pre, 1, rnd)


def test_draw_is_exactly_proportional():
    pre = np.cumsum(np.array([1, 2, 0, 5], dtype=np.uint64))
    rnd = [[k << 61, 0] for k in range(8)]
    assert np.bincount(_run_draw(pre, 1, rnd), minlength=4).tolist() == [1, 2, 0, 5]


# ---------------------------------------------------------------------- the buffer's API
@pytest.fixture(scope="module")
def positions():
    return synthetic_positions(12, seed=301)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_sample_weighted_equals_gather_of_reference_ids(positions):
    from replay import DeviceReplayBuffer
    dev = DeviceReplayBuffer(40, DEV)                         # a ring of 5 positions
    s = np.array([0.3, 0.0, 2.5, np.nan, 0.9, 0.05, 1.1], dtype=np.float32)
    dev.add_positions(positions[:7], surprise=s, mix=0.75)    # 7 into 5: head stays 0, the oldest 2 never enter
    dev.add_positions(positions[7:9])                         # wraps: head = 2; weight 1.0 each
    assert dev.head == 2 and dev.count == 5 and dev.weights.dtype == torch.uint32
    q = ref.surprise_quanta(s, 0.75)
    want_w = np.r_[q[4:7], QUANTA, QUANTA]
    assert np.array_equal(dev.get_weights(), want_w / QUANTA)
    pre = np.cumsum(want_w.astype(np.uint64))
    rnd = np.random.default_rng(31).integers(0, 1 << 64, size=(64, 2), dtype=np.uint64)
    got = dev.sample_weighted(64, rnd=rnd)
    assert _same(got, dev.sample(64, ids=ref.draw_ids(pre, 8, rnd)))
    # the default words come from `random`: same seed, same batch; and they are the reference's
    random.seed(5)
    a = dev.sample_weighted(32)
    random.seed(5)
    b = dev.sample_weighted(32)
    random.seed(5)
    words = np.array([random.getrandbits(64) for _ in range(64)], dtype=np.uint64).reshape(32, 2)
    assert _same(a, b) and _same(a, dev.sample(32, ids=ref.draw_ids(pre, 8, words)))
    assert not _same(a, dev.sample_weighted(32))
    ess = dev.effective_sample_size()
    assert ess == pytest.approx(want_w.sum() ** 2 / (want_w.astype(np.float64) ** 2).sum()) and 0 < ess <= 5
    for bad in (rnd[:5], rnd.astype(np.int64)):
        with pytest.raises(ValueError):
            dev.sample_weighted(64, rnd=bad)
    with pytest.raises(ValueError):
        dev.add_positions(positions[:2], surprise=np.ones(3, np.float32))
    with pytest.raises(ValueError):
        dev.add_positions(positions[:2], surprise=np.ones(2, np.float32), mix=1.5)
    assert dev.head == 2 and np.array_equal(dev.get_weights(), want_w / QUANTA)   # refused adds change nothing


def test_buffer_without_weights_draws_uniformly(positions):
    from replay import DeviceReplayBuffer
    dev = DeviceReplayBuffer(6, DEV, symmetries=False)
    dev.add_positions(positions[:4])
    dev.sample(3)
    dev.to_host()
    assert dev.weights is None and np.array_equal(dev.get_weights(), np.ones(4)) and dev.effective_sample_size() == 4.0
    assert DeviceReplayBuffer.from_host(dev.to_host(), DEV).weights is None
    rnd = np.array([[k << 62, 5] for k in range(4)], dtype=np.uint64)   # four equal weights: one word each
    got = dev.sample_weighted(4, rnd=rnd)
    assert _same(got, dev.sample(4, ids=[0, 1, 2, 3]))
    assert np.array_equal(dev.get_weights(), np.ones(4))


def test_set_weights_and_eviction_follow_a_host_model(positions):
    from replay import DeviceReplayBuffer
    dev = DeviceReplayBuffer(40, DEV)                         # 5 positions
    model = []                                                # the ring's weights in quanta, oldest first

    def add(examples, surprise=None, mix=0.5):
        dev.add_positions(examples, surprise=surprise, mix=mix)
        model.extend([QUANTA] * len(examples) if surprise is None else ref.surprise_quanta(surprise, mix).tolist())
        del model[:-5]
        if dev.weights is not None:
            assert np.array_equal(dev.get_weights(), np.array(model) / QUANTA)

    add(positions[:3])
    assert dev.weights is None
    dev.set_weights([0.25, 0.0, 3.0])
    model[:] = [QUANTA // 4, 0, 3 * QUANTA]
    add(positions[3:7], surprise=np.array([1.0, 0.2, 0.0, 4.0], np.float32), mix=1.0)      # first wrap
    add(positions[7:8])
    add(positions[8:12], surprise=np.array([0.5, 0.5, 3.0, 0.1], np.float32), mix=0.25)    # second wrap
    add(positions[0:2])
    assert dev.head == 4 and len(model) == 5
    w = np.array([0.0, 1.5, 2.0 ** -16, 32767.5, 0.3])
    dev.set_weights(w)                                        # written from head, around the wrap
    assert np.array_equal(dev.get_weights(), np.rint(w * QUANTA) / QUANTA)
    rnd = np.random.default_rng(41).integers(0, 1 << 64, size=(48, 2), dtype=np.uint64)
    pre = np.cumsum(np.rint(w * QUANTA).astype(np.uint64))
    assert _same(dev.sample_weighted(48, rnd=rnd), dev.sample(48, ids=ref.draw_ids(pre, 8, rnd)))
    for bad in ([1.0] * 4, [1, 1, 1, 1, np.nan], [1, 1, 1, 1, -0.5], [1, 1, 1, 1, 32768.0], [0.0] * 5, [1e-9] * 5):
        with pytest.raises(ValueError):
            dev.set_weights(bad)
    assert np.array_equal(dev.get_weights(), np.rint(w * QUANTA) / QUANTA)


def test_every_per_slot_array_wraps_at_the_same_place(positions):
    """One wrapped write, five per-slot arrays: position k of a batch of 4 added behind 3 in a ring of
    5 slots is in slot (3 + k) % 5 of stones, pis, zs, _wq and _pw alike, bit for bit."""
    from replay import DeviceReplayBuffer
    dev = DeviceReplayBuffer(40, DEV)
    assert dev.cap_pos == 5 and dev.nsym == 8
    dev.add_positions(positions[:3])
    new = positions[3:7]
    s = np.array([0.3, 0.0, 2.5, 0.9], dtype=np.float32)
    pw = np.array([1.0, 0.0, 0.5, 2.0], dtype=np.float32)
    dev.add_positions(new, surprise=s, mix=0.75, policy_weight=pw)
    assert dev.head == 2 and dev.count == 5
    q = ref.surprise_quanta(s, 0.75)
    stones, pis, zs, wq, pws = (t.cpu().numpy() for t in (dev.stones, dev.pis, dev.zs, dev._wq, dev._pw))
    for k, (state, pi, z) in enumerate(new):
        slot = (3 + k) % 5
        assert np.array_equal(stones[slot], (state[0] + 2 * state[1]).astype(np.int8).reshape(-1))
        assert np.array_equal(pis[slot].view(np.uint32), np.asarray(pi, dtype=np.float32).view(np.uint32))
        assert zs[slot:slot + 1].view(np.uint32)[0] == np.array([z], dtype=np.float32).view(np.uint32)[0]
        assert int(wq[slot]) == int(q[k])
        assert pws[slot:slot + 1].view(np.uint32)[0] == pw[k:k + 1].view(np.uint32)[0]
    assert int(wq[2]) == QUANTA and pws[2] == 1.0   # the survivor of the first three: slot 2, the new head


# ----------------------------------------------------------------------------- the loop
# the keywords of test_gpu_precision.py's test_selfplay_precision_in_the_training_loop at 64 channels; its
# selfplay_precision="fp16" exists for 128-channel nets only (engine.set_eval_precision), so LOOP_KW leaves it
# out and LOOP_KW_FP16 is that test's net and precision unchanged
LOOP_KW = dict(num_iterations=1, games_per_iteration=2, n_simulations=16, batch_size=16, epochs_per_iter=1,
               eval_games=2, eval_mcts_simulations=8, n_res_blocks=2, channels=64, max_moves=6, device=DEV)
LOOP_KW_FP16 = dict(LOOP_KW, channels=128, selfplay_precision="fp16")


def test_nothing_changes_when_the_feature_is_off(tmp_path, monkeypatch):
    import train
    lib = _lib()

    def refuse(*a):
        raise AssertionError("a weighted-sampling entry point was called with the feature off")

    for name in ("azg_pv_replay_surprise_weights", "azg_pv_replay_prefix", "azg_pv_replay_draw"):
        monkeypatch.setattr(lib, name, refuse)
    history = []
    train.train_alphazero(model_dir=str(tmp_path), device_buffer=True, history=history, **LOOP_KW)
    assert history[0]["last_train_loss"] is not None          # it trained, through sample()
    assert history[0]["surprise_weight"] is None and history[0]["buffer_ess"] is None
    assert not os.path.exists(tmp_path / "replay_weights_latest.npy")


def _weighted_iteration(tmp_path, monkeypatch, loop_kw):
    """One train_alphazero iteration with surprise_weight=0.5: (the buffers the loop makes from
    now on, the first one's weights)."""
    import replay
    import train
    buffers = []
    new_buffer = replay.new_device_buffer
    monkeypatch.setattr(replay, "new_device_buffer", lambda *a: buffers.append(new_buffer(*a)) or buffers[-1])
    history = []
    train.train_alphazero(model_dir=str(tmp_path), device_buffer=True, surprise_weight=0.5, history=history,
                          **loop_kw)
    buf = buffers[0]
    positions = buf.count
    assert positions == 2 * 6 and history[0]["last_train_loss"] is not None
    assert history[0]["surprise_weight"] == 0.5 and 0 < history[0]["buffer_ess"] <= positions
    w = buf.get_weights()
    assert abs(w.sum() - positions) <= positions * 2.0 ** -16   # mean weight 1: each quantum rounds by <= 2^-17
    assert w.min() >= 0.5 and len(set(w.tolist())) > 1          # the uniform share; and the KLs differ
    assert history[0]["buffer_ess"] == pytest.approx(w.sum() ** 2 / (w * w).sum())
    assert np.array_equal(np.load(tmp_path / "replay_weights_latest.npy"), w)
    return buffers, w


def test_loop_with_surprise_weighting_after_fp16_selfplay(tmp_path, monkeypatch):
    import train
    precisions = []
    score = train._score_surprise
    monkeypatch.setattr(train, "_score_surprise", lambda m, ex: precisions.append(m.eval_precision) or score(m, ex))
    _weighted_iteration(tmp_path, monkeypatch, LOOP_KW_FP16)
    assert precisions == ["exact"]                            # self-play in fp16, the surprise from exact forwards


def test_loop_with_surprise_weighting(tmp_path, monkeypatch):
    import replay
    import train
    buffers, w = _weighted_iteration(tmp_path, monkeypatch, LOOP_KW)
    side = tmp_path / "replay_weights_latest.npy"
    # a second run starts from the pickle and takes the sidecar's weights ...
    seen = []
    set_weights = replay.DeviceReplayBuffer.set_weights
    monkeypatch.setattr(replay.DeviceReplayBuffer, "set_weights",
                        lambda self, v: seen.append(np.array(v)) or set_weights(self, v))
    kw = dict(LOOP_KW, num_iterations=0)
    train.train_alphazero(model_dir=str(tmp_path), device_buffer=True, surprise_weight=0.5, **kw)
    assert len(seen) == 1 and np.array_equal(seen[0], w) and np.array_equal(buffers[1].get_weights(), w)
    # ... but not one of another length
    np.save(side, w[:-1])
    train.train_alphazero(model_dir=str(tmp_path), device_buffer=True, surprise_weight=0.5, **kw)
    assert len(seen) == 1 and buffers[2].weights is None
    for bad in (dict(device_buffer=False, surprise_weight=0.5), dict(device_buffer=True, surprise_weight=1.5),
                dict(device_buffer=True, surprise_weight=-0.1), dict(device_buffer=True, surprise_weight="0.5")):
        with pytest.raises(ValueError):
            train.train_alphazero(model_dir=str(tmp_path / "bad"), **dict(LOOP_KW, **bad))
