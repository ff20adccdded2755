"""search="alphazero" on the GPU: the native value search fed by the HIP forward (int8
leaves, on-GPU encoding) equals the Python restatement of its rules
(tests/value_search_reference.py) fed by the same model's predict, bit for bit; the value
head changes the moves under "alphazero" and not under "reference"; one tiny training
iteration and a Player run with it.  No kernel is new: the search is host code over the
existing forward."""
import os
import sys

import numpy as np
import pytest

from conftest import has_gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

DEV = "cuda:0"
_MODELS = {}


def _model(blocks, ch):
    import torch
    from network import PyTorchModel
    if (blocks, ch) not in _MODELS:
        torch.manual_seed(100 * blocks + ch)
        m = PyTorchModel(board_size=15, device=DEV, n_res_blocks=blocks, channels=ch)
        m.net.eval()
        _MODELS[blocks, ch] = m
    return _MODELS[blocks, ch]


def _negated_value_head(m, blocks, ch):
    """A copy of m whose value is -m's: value_fc2 feeds tanh, which is odd."""
    from network import PyTorchModel
    sd = {k: v.clone() for k, v in m.net.state_dict().items()}
    sd["value_fc2.weight"] = -sd["value_fc2.weight"]
    sd["value_fc2.bias"] = -sd["value_fc2.bias"]
    m2 = PyTorchModel(board_size=15, device=DEV, n_res_blocks=blocks, channels=ch)
    m2.net.load_state_dict(sd)
    m2.net.eval()
    return m2


def same_examples(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]
                                    for x, y in zip(a, b))


NOISE = dict(dirichlet_alpha=0.3, epsilon=0.25, apply_dirichlet_n_first_moves=3)


@pytest.mark.parametrize("blocks,ch", [(2, 128), (1, 64)])
def test_native_on_hip_forward_equals_restatement(blocks, ch):
    """2 games, 48 simulations, 4 moves (3 noisy, tree reuse), exact precision."""
    import selfplay
    from games.gomoku import Gomoku
    from mcts.native_mcts import NativeSelfPlay
    from value_search_reference import ValueSearch
    m = _model(blocks, ch)
    seeds = [5, 6]
    temp = lambda n: 1.0 if n < 2 else 0.0
    kw = dict(cpuct=1.2, batch_size=8, **NOISE)
    sp = NativeSelfPlay(None, Gomoku, 2, 48, evaluator_factory=m.board_evaluator, groups=2, search="alphazero", **kw)
    got = sp.play(temp, max_moves=4, use_symmetries=False, seeds=seeds)
    assert sp.boards > 0 and all(len(ex) == 4 for ex, _ in got)
    assert sum(f.collisions(0) for f in sp.forests) > 0
    for g in range(2):
        ref = ValueSearch(Gomoku, 48, m, rng=np.random.RandomState(seeds[g]), **kw)
        ex, w = selfplay.play_game_and_collect(ref, Gomoku(15), temp, max_moves=4, use_symmetries=False)
        assert w == got[g][1]
        for t, (x, y) in enumerate(zip(ex, got[g][0])):
            assert np.array_equal(x[1], y[1]), f"game {g}: pi differs at move {t}"
        assert same_examples(ex, got[g][0])


def test_value_head_is_used_on_the_gpu():
    from games.gomoku import Gomoku
    from mcts.native_mcts import NativeMCTS
    m = _model(2, 128)
    m_neg = _negated_value_head(m, 2, 128)
    x = np.zeros((1, 3, 15, 15), np.float32)
    x[:, 2] = 1.0
    (p0, v0), (p1, v1) = m.predict(x), m_neg.predict(x)
    # (tanhf need not be odd to the last bit: 1e-6 is two float32 ulps at |v| <= 1)
    assert np.array_equal(p0, p1) and np.allclose(v0, -v1, rtol=0, atol=1e-6) and abs(v0.reshape(-1)[0]) > 1e-3
    pis = {}
    for search in ("alphazero", "reference"):
        for tag, model in (("plain", m), ("negated", m_neg)):
            mc = NativeMCTS(Gomoku, 48, model, cpuct=1.0, batch_size=8, add_dirichlet_noise=False, search=search)
            g, out = Gomoku(15), []
            for _ in range(3):
                pi = mc.run(g, len(g.move_history))
                out.append(pi)
                g.do_move(divmod(int(np.argmax(pi)), 15))
            pis[search, tag] = out
    assert not all(np.array_equal(a, b) for a, b in zip(pis["alphazero", "plain"], pis["alphazero", "negated"]))
    assert all(np.array_equal(a, b) for a, b in zip(pis["reference", "plain"], pis["reference", "negated"]))


@pytest.mark.parametrize("precision", [None, "fp16"])
def test_one_training_iteration_with_the_value_search(tmp_path, monkeypatch, precision):
    import replay
    import train
    np.random.seed(30)        # the games' seeds come from numpy's global stream
    buffers = []
    new_buffer = replay.new_device_buffer
    monkeypatch.setattr(replay, "new_device_buffer", lambda *a: buffers.append(new_buffer(*a)) or buffers[-1])
    h = []
    train.train_alphazero(model_dir=str(tmp_path), device_buffer=True, search="alphazero", history=h,
                          selfplay_precision=precision, num_iterations=1, games_per_iteration=2, n_simulations=16,
                          batch_size=16, epochs_per_iter=1, eval_games=2, eval_mcts_simulations=16, n_res_blocks=2,
                          channels=128, max_moves=6, device=DEV)
    assert h[-1]["search"] == "alphazero"
    assert h[-1]["last_train_loss"] is not None and all(np.isfinite(v) for v in h[-1]["last_train_loss"].values())
    assert buffers[-1].count == 2 * 6          # 2 games of max_moves positions each


def test_player_with_the_value_search():
    from players.player import Player
    p = Player("gomoku", 15, n_simulations=32, model_path=None, search="alphazero")
    assert p.mcts.forest.get_search_mode() == 1
    board = np.zeros((15, 15), dtype=int)
    board[7, 7] = 1
    r, c = p.play(board.tolist(), 1, (7, 7))
    assert 0 <= r < 15 and 0 <= c < 15 and board[r, c] == 0
    q, v_net, visits = p.mcts.root_value()
    assert visits == 31 and -1.0 <= q <= 1.0 and -1.0 <= v_net <= 1.0
