"""train_alphazero(playout_cap_prob=, playout_cap_fast_sims=) end to end on the GPU: one
iteration of a 1x64 net, 2 games, 8 / 2 simulations.  The policy weights travel from the
self-play driver through the device ring into the weighted train step, are kept beside the
buffer pickle and restored; with the arguments left at None none of the new entry points
is called."""
import os
import pickle

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

DEV = "cuda:0"
LOOP_KW = dict(num_iterations=1, games_per_iteration=2, n_simulations=8, batch_size=16, epochs_per_iter=1,
               eval_games=2, eval_mcts_simulations=8, n_res_blocks=1, channels=64, max_moves=6, device=DEV)
PV_NEW = ("azg_pv_train_backward_weighted", "azg_pv_replay_gather_weight")
MCTS_NEW = ("azg_mcts_set_budget",)


def _count_calls(monkeypatch):
    """Counting wrappers around the new entry points of both libraries."""
    import _native
    import _native_mcts
    calls = {}
    for lib, names in ((_native.load_library(), PV_NEW), (_native_mcts.load_library(), MCTS_NEW)):
        for name in names:
            fn = getattr(lib, name)
            calls[name] = 0

            def wrapper(*a, _fn=fn, _name=name):
                calls[_name] += 1
                return _fn(*a)

            monkeypatch.setattr(lib, name, wrapper)
    return calls


def test_loop_with_playout_cap(tmp_path, monkeypatch):
    import replay
    import train
    np.random.seed(20)        # the games' seeds come from numpy's global stream
    calls = _count_calls(monkeypatch)
    buffers = []
    new_buffer = replay.new_device_buffer
    monkeypatch.setattr(replay, "new_device_buffer", lambda *a: buffers.append(new_buffer(*a)) or buffers[-1])
    side = tmp_path / "replay_policy_weights_latest.npy"

    # off: no new entry point is called, no sidecar, history says None
    h0 = []
    train.train_alphazero(model_dir=str(tmp_path / "off"), device_buffer=True, history=h0, **LOOP_KW)
    assert h0[-1]["playout_cap"] is None and h0[-1]["last_train_loss"] is not None
    assert calls == dict.fromkeys(PV_NEW + MCTS_NEW, 0), calls
    assert buffers[-1]._pw is None
    assert not os.path.exists(tmp_path / "off" / "replay_policy_weights_latest.npy")

    # on
    h = []
    train.train_alphazero(model_dir=str(tmp_path), device_buffer=True, playout_cap_prob=0.5,
                          playout_cap_fast_sims=2, history=h, **LOOP_KW)
    cap = h[-1]["playout_cap"]
    moves = 2 * 6
    assert cap["p_full"] == 0.5 and cap["fast_sims"] == 2 and cap["full_moves"] + cap["fast_moves"] == moves
    assert h[-1]["last_train_loss"] is not None and all(np.isfinite(v) for v in h[-1]["last_train_loss"].values())
    buf = buffers[-1]
    w = buf.get_policy_weights()
    assert buf.count == moves and w.shape == (moves,) and set(w.tolist()) <= {0.0, 1.0}
    assert int(w.sum()) == cap["full_moves"]
    n_batches = moves * 8 // 16
    assert calls["azg_mcts_set_budget"] == moves
    assert calls["azg_pv_replay_gather_weight"] == calls["azg_pv_train_backward_weighted"] == n_batches
    assert np.array_equal(np.load(side), w)
    with open(tmp_path / "replay_buffer_latest.pkl", "rb") as f:      # the reference pickle: 3-tuples
        saved = pickle.load(f)
    assert len(saved["buffer"]) == 8 * moves and all(len(e) == 3 for e in saved["buffer"])

    # a second call restores the sidecar ...
    kw = dict(LOOP_KW, num_iterations=0)
    train.train_alphazero(model_dir=str(tmp_path), device_buffer=True, playout_cap_prob=0.5,
                          playout_cap_fast_sims=2, **kw)
    assert buffers[-1] is not buf and np.array_equal(buffers[-1].get_policy_weights(), w)
    # ... but not one of another length: every position then counts 1.0
    np.save(side, w[:-1])
    train.train_alphazero(model_dir=str(tmp_path), device_buffer=True, playout_cap_prob=0.5,
                          playout_cap_fast_sims=2, **kw)
    assert buffers[-1]._pw is None and np.array_equal(buffers[-1].get_policy_weights(), np.ones(moves, np.float32))

    for bad in (dict(playout_cap_prob=0.5), dict(playout_cap_fast_sims=2),
                dict(playout_cap_prob=0.5, playout_cap_fast_sims=2, device_buffer=False),
                dict(playout_cap_prob=1.5, playout_cap_fast_sims=2), dict(playout_cap_prob=0.5, playout_cap_fast_sims=-1)):
        with pytest.raises(ValueError):
            train.train_alphazero(model_dir=str(tmp_path / "bad"), **dict(dict(LOOP_KW, device_buffer=True), **bad))


def test_loop_with_playout_cap_and_surprise_weighting(tmp_path, monkeypatch):
    """Both on: a fast position's surprise is set to 0, so it enters with the uniform share
    (1 - surprise_weight) of the sampling weight, and batches come from sample_weighted."""
    import replay
    import train
    np.random.seed(21)        # the games' seeds come from numpy's global stream
    buffers = []
    new_buffer = replay.new_device_buffer
    monkeypatch.setattr(replay, "new_device_buffer", lambda *a: buffers.append(new_buffer(*a)) or buffers[-1])
    h = []
    train.train_alphazero(model_dir=str(tmp_path), device_buffer=True, playout_cap_prob=0.5, playout_cap_fast_sims=2,
                          surprise_weight=0.5, history=h, **LOOP_KW)
    buf = buffers[-1]
    pw, sw = buf.get_policy_weights(), buf.get_weights()
    assert 0 < pw.sum() < len(pw), "the seeds of this run gave one kind of move only"
    assert (sw[pw == 0] == 0.5).all() and (sw[pw == 1] >= 0.5).all() and sw[pw == 1].max() > 0.5
    assert h[-1]["last_train_loss"] is not None and h[-1]["buffer_ess"] > 0
