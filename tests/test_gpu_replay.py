"""The device-resident replay buffer (replay.DeviceReplayBuffer over
azg_pv_replay_gather) on the GPU.  Everything the gather writes is a copy or a 0/1
constant, so every comparison is bitwise: against the Python MCTS.symmetries images,
against the host ReplayBuffer under the same random.seed, and -- through the train step
and the whole train_alphazero loop -- against the host data path's model and pickle.
Boards are random (asymmetric) and pi is random, so a wrong rotation cannot pass."""
import io
import pickle
import random
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from conftest import has_gpu
from replay_helpers import synthetic_positions

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

DEV = "cuda:0"


def _positions(n, seed):
    """n canonical examples (state [3,15,15], pi [225], z) with pairwise distinct images."""
    return synthetic_positions(n, seed, distinct_images=True)


def _expand(examples):
    """The host buffer's content: every position's 8 images, as selfplay.play_game_gen forms them."""
    from mcts.new_mcts_alpha import MCTS
    return [(s_aug.astype(np.float32), pi_aug.astype(np.float32), z)
            for s, p, z in examples for s_aug, pi_aug in MCTS.symmetries(None, s, p)]


def _same_examples(a, b):
    assert len(a) == len(b)
    for (sa, pa, za), (sb, pb, zb) in zip(a, b):
        assert sa.dtype == sb.dtype == np.float32 and pa.dtype == pb.dtype == np.float32
        assert np.array_equal(sa, sb) and np.array_equal(pa, pb) and za == zb


def _same_samples(host, dev, seed, batch, rounds=10):
    random.seed(seed)
    want = [host.sample(batch) for _ in range(rounds)]
    random.seed(seed)
    got = [dev.sample(batch) for _ in range(rounds)]
    for (ws, wp, wz), (gs, gp, gz) in zip(want, got):
        assert np.array_equal(gs.cpu().numpy(), ws)
        assert np.array_equal(gp.cpu().numpy(), wp)
        assert np.array_equal(gz.cpu().numpy(), wz)


@pytest.fixture(scope="module")
def positions():
    return _positions(8, seed=101)


def test_gather_equals_numpy_symmetries(positions):
    from replay import DeviceReplayBuffer
    canon = positions[:5]
    images = _expand(canon)
    dev = DeviceReplayBuffer(40, DEV)
    dev.add_positions(canon)
    assert len(dev) == 40
    rng = np.random.default_rng(3)
    shuffled = rng.permutation(40)
    for ids in (shuffled[:1], shuffled, np.concatenate([shuffled, rng.integers(0, 40, size=90)])):
        s, p, z = dev.sample(len(ids), ids=ids.tolist())
        assert s.shape == (len(ids), 3, 15, 15) and p.shape == (len(ids), 225) and z.shape == (len(ids), 1)
        assert s.dtype == p.dtype == z.dtype == torch.float32 and s.is_cuda
        assert np.array_equal(s.cpu().numpy(), np.stack([images[i][0] for i in ids]))
        assert np.array_equal(p.cpu().numpy(), np.stack([images[i][1] for i in ids]))
        assert np.array_equal(z.cpu().numpy(), np.array([images[i][2] for i in ids], dtype=np.float32).reshape(-1, 1))


def test_equals_host_buffer_through_wrap_and_eviction(positions):
    from replay import DeviceReplayBuffer
    from selfplay import ReplayBuffer
    host, dev = ReplayBuffer(24), DeviceReplayBuffer(24, DEV)
    for k, chunk in enumerate((positions[:2], positions[2:5])):   # 2 + 3 positions in a ring of 3
        host.add(_expand(chunk))
        dev.add_positions(chunk)
        assert len(dev) == len(host) == (16, 24)[k]
        _same_examples(list(dev.to_host().buffer), list(host.buffer))
        _same_samples(host, dev, seed=7 + k, batch=16)
    assert dev.to_host().capacity == 24


def test_from_host_single_images_and_groups(positions):
    from replay import DeviceReplayBuffer
    from selfplay import ReplayBuffer
    # 24 images into a deque of 20: no whole groups -> every image its own entry
    host = ReplayBuffer(20)
    host.add(_expand(positions[:3]))
    assert len(host) == 20
    dev = DeviceReplayBuffer.from_host(host, DEV)
    assert dev.nsym == 1 and len(dev) == 20 and dev.capacity == 20
    _same_examples(list(dev.to_host().buffer), list(host.buffer))
    _same_samples(host, dev, seed=13, batch=16)
    # whole groups of 8 -> one stored position per group
    host = ReplayBuffer(24)
    host.add(_expand(positions[3:6]))
    dev = DeviceReplayBuffer.from_host(host, DEV)
    assert dev.nsym == 8 and dev.count == 3 and len(dev) == 24
    _same_examples(list(dev.to_host().buffer), list(host.buffer))
    _same_samples(host, dev, seed=14, batch=16)
    # aligned sizes, but one group is not the images of its first element
    ex = _expand(positions[3:6])
    ex[9], ex[10] = ex[10], ex[9]
    host = ReplayBuffer(24)
    host.add(ex)
    dev = DeviceReplayBuffer.from_host(host, DEV)
    assert dev.nsym == 1 and len(dev) == 24
    _same_examples(list(dev.to_host().buffer), list(host.buffer))
    _same_samples(host, dev, seed=15, batch=16)


def test_validation(positions):
    from replay import DeviceReplayBuffer
    with pytest.raises(ValueError):
        DeviceReplayBuffer(20, DEV, symmetries=True)
    with pytest.raises(ValueError):
        DeviceReplayBuffer(24, DEV, board_size=19)
    dev = DeviceReplayBuffer(24, DEV)
    s, p, z = positions[0]
    bad = s.copy()
    bad[2, 3, 4] = 0.0                      # plane 2 not constant
    with pytest.raises(ValueError):
        dev.add_positions([(bad, p, z)])
    bad = s.copy()
    bad[0] = bad[1] = 0.0
    bad[0, 1, 1] = bad[1, 1, 1] = 1.0       # both sides on one square
    with pytest.raises(ValueError):
        dev.add_positions([(bad, p, z)])
    bad = s.copy()
    bad[0, 0, 0] = 2.0
    with pytest.raises(ValueError):
        dev.add_positions([(bad, p, z)])
    assert len(dev) == 0                    # a refused add leaves the ring as it was
    dev.add_positions(positions[:2])
    for ids in ([0, 16], [-1, 0]):
        with pytest.raises(ValueError):
            dev.sample(2, ids=ids)
    dev.sample(2, ids=[0, 15])


def _model(seed):
    from network import PyTorchModel
    torch.manual_seed(seed)
    return PyTorchModel(board_size=15, device=DEV, n_res_blocks=1, channels=64)


def _float_state(m):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in m.net.state_dict().items()}


def test_train_steps_equal_host_path(positions):
    from replay import DeviceReplayBuffer
    from selfplay import ReplayBuffer
    host, dev = ReplayBuffer(64), DeviceReplayBuffer(64, DEV)
    host.add(_expand(positions))
    dev.add_positions(positions)
    ma, mb = _model(5), _model(5)
    random.seed(23)
    la = [ma.train_batch(*host.sample(16)) for _ in range(3)]
    random.seed(23)
    lb = [mb.train_batch_device(*dev.sample(16)) for _ in range(3)]
    assert la == lb
    sa, sb = _float_state(ma), _float_state(mb)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert any(not np.array_equal(v, w) for v, w in zip(sa.values(), _float_state(_model(5)).values()))   # it trained


@pytest.mark.timeout(600)
def test_train_alphazero_equal_with_device_buffer(tmp_path):
    import train
    out = {}
    for flag in (False, True):
        random.seed(3)
        np.random.seed(3)
        torch.manual_seed(3)
        d = tmp_path / ("dev" if flag else "host")
        log = io.StringIO()
        with redirect_stdout(log):
            best = train.train_alphazero(num_iterations=1, games_per_iteration=2, n_simulations=8, batch_size=16,
                                         epochs_per_iter=1, eval_games=2, eval_mcts_simulations=8,
                                         win_rate_threshold=0.0,   # the trained candidate is what comes back
                                         model_dir=str(d), n_res_blocks=1, channels=64, max_moves=6, device=DEV,
                                         device_buffer=flag)
        assert "last_loss={" in log.getvalue() and "evaluation failed" not in log.getvalue()   # it trained and gated
        with open(d / "replay_buffer_latest.pkl", "rb") as f:
            out[flag] = (_float_state(best), pickle.load(f))
    (sa, pa), (sb, pb) = out[False], out[True]
    for k in sa:
        if sa[k].dtype.kind == "f":
            assert np.array_equal(sa[k], sb[k]), k
    assert pa["capacity"] == pb["capacity"]
    assert len(pa["buffer"]) == 2 * 6 * 8
    _same_examples(pb["buffer"], pa["buffer"])
