"""The opt-in AlphaZero search of the native engine (search="alphazero",
AZG_MCTS_SEARCH_VALUE in include/azg_mcts.h): the net's value is backed up under virtual
loss.  Bit-exact against the dict-based restatement of its rules
(tests/value_search_reference.py) and, at batch_size 1, against a separate textbook
recursive search; the value head changes the moves; invariants, independence of games and
threads, the self-play and evaluation drivers, API errors; and mode 0 set explicitly is
still the reference search of the goldens.  CPU only (the model is injected)."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fake_model import FakeBoardEvaluator, FakeModel  # noqa: E402
from value_search_reference import ValueSearch  # noqa: E402

import _native_mcts  # noqa: E402
import selfplay  # noqa: E402
from _native_mcts import DONE, NEED_EVAL, SearchForest  # noqa: E402
from games.gomoku import Gomoku  # noqa: E402
from games.pente import Pente  # noqa: E402
from mcts.native_mcts import NativeEval, NativeMCTS, NativeSelfPlay  # noqa: E402

NOISE = dict(dirichlet_alpha=0.3, epsilon=0.25, apply_dirichlet_n_first_moves=4)


class Recording:
    """A model that keeps every leaf batch it was asked for."""

    def __init__(self, model):
        self.model, self.batches = model, []

    def predict(self, X):
        self.batches.append(np.array(X, dtype=np.float32))
        return self.model.predict(X)


def same_examples(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]
                                    for x, y in zip(a, b))


def play_moves(search, cls, n_moves, root_value):
    """n_moves argmax moves from the empty board with tree reuse: per move pi and root value."""
    g = cls(15)
    pis, roots = [], []
    for _ in range(n_moves):
        pi = search.run(g, len(g.move_history))
        pis.append(pi)
        roots.append(root_value())
        g.do_move(divmod(int(np.argmax(pi)), 15))
    return pis, roots, search.tree_size()


# ------------------------------------------------------------ native == restatement
@pytest.mark.parametrize("cls", [Gomoku, Pente])
@pytest.mark.parametrize("bs", [1, 8, 32])
def test_native_equals_restatement(cls, bs):
    """64 simulations, 6 moves with tree reuse, noise on (noisy moves 0..3 re-mix an existing
    root, moves 4..5 drop the mix): pi, every leaf batch, tree size and root value."""
    ra, rb = Recording(FakeModel(seed=3)), Recording(FakeModel(seed=3))
    nat = NativeMCTS(cls, 64, ra, cpuct=1.3, batch_size=bs, rng=np.random.RandomState(17), search="alphazero",
                     **NOISE)
    ref = ValueSearch(cls, 64, rb, cpuct=1.3, batch_size=bs, rng=np.random.RandomState(17), **NOISE)
    pa, qa, na = play_moves(nat, cls, 6, nat.root_value)
    pb, qb, nb = play_moves(ref, cls, 6, ref.root_value)
    for m, (x, y) in enumerate(zip(pa, pb)):
        assert x.dtype == y.dtype == np.float32 and np.array_equal(x, y), f"pi differs at move {m}"
    assert len(ra.batches) == len(rb.batches)
    for i, (x, y) in enumerate(zip(ra.batches, rb.batches)):
        assert x.shape == y.shape and np.array_equal(x, y), f"leaf batch {i} differs"
    assert max(len(x) for x in ra.batches) <= bs
    assert na == nb
    assert qa == qb          # (q float64, v_net float32, visits) exactly
    if bs > 1:
        assert ref.collisions > 0 and nat.forest.collisions(0) == ref.collisions   # the suspended path ran


# ------------------------------------------------------------ batch size 1 == textbook
class Textbook:
    """AlphaZero's search as the paper has it: recursive, one evaluation per simulation, no
    queue, no virtual loss; vectorised float64 PUCT.  Shares no code with the restatement."""

    def __init__(self, model, n_simulations, cpuct, rng, dirichlet_alpha, epsilon, apply_dirichlet_n_first_moves):
        self.model, self.n, self.c, self.rng = model, n_simulations, float(cpuct), rng
        self.alpha, self.eps, self.first = dirichlet_alpha, epsilon, apply_dirichlet_n_first_moves
        self.P, self.N, self.W, self.valid, self.clean = {}, {}, {}, {}, {}

    @staticmethod
    def key(g):
        return g.board.tobytes() + bytes([g.current_player])

    def noise(self, k):
        d = self.rng.dirichlet([self.alpha] * 225)
        p = (1 - self.eps) * self.clean[k] + self.eps * d
        self.P[k] = p / np.sum(p)

    def run(self, game, move_number):
        root = self.key(game)
        self.noisy = move_number < self.first
        for k in self.P:                       # only the current root is ever mixed
            self.P[k] = self.clean[k].astype(np.float64)
        if self.noisy and root in self.P:
            self.noise(root)
        self.root = root
        for _ in range(self.n):
            self.search(game.clone())
        cnt = self.N[root].astype(np.float32)
        return cnt / np.sum(cnt)

    def search(self, g):
        if g.is_game_over():
            return np.float32(0.0 if g.get_winner() == 0 else -1.0)
        k = self.key(g)
        if k not in self.P:
            p, v = self.model.predict(g.get_encoded_state()[None].astype(np.float32))
            valid = g.get_valid_moves()
            p = p[0] * valid
            if np.sum(p) < 1e-8:
                p = valid / np.sum(valid)
            self.clean[k], self.P[k] = p, p.astype(np.float64)
            self.N[k], self.W[k], self.valid[k] = np.zeros(225, np.int64), np.zeros(225, np.float32), valid == 1
            if self.noisy and k == self.root:
                self.noise(k)
            return np.float32(np.asarray(v).reshape(-1)[0])
        n = self.N[k].astype(np.float64)
        q = np.divide(self.W[k].astype(np.float64), n, out=np.zeros(225), where=n > 0)
        u = self.c * self.P[k] * math.sqrt(1.0 + float(np.sum(self.N[k][self.valid[k]]))) / (1.0 + n)
        a = int(np.argmax(np.where(self.valid[k], q + u, -np.inf)))
        g.do_move(divmod(a, 15))
        v = np.float32(-self.search(g))
        self.W[k][a] += v
        self.N[k][a] += 1
        return v


@pytest.mark.parametrize("cls", [Gomoku, Pente])
def test_batch_size_one_equals_textbook_search(cls):
    nat = NativeMCTS(cls, 64, FakeModel(seed=5), cpuct=1.1, batch_size=1, rng=np.random.RandomState(23),
                     search="alphazero", **NOISE)
    book = Textbook(FakeModel(seed=5), 64, 1.1, np.random.RandomState(23), **NOISE)
    g = cls(15)
    for m in range(6):
        pa, pb = nat.run(g, len(g.move_history)), book.run(g, len(g.move_history))
        assert np.array_equal(pa, pb), f"pi differs at move {m}"
        g.do_move(divmod(int(np.argmax(pa)), 15))
    assert nat.tree_size() == len(book.P)


# ------------------------------------------------------------ the value is used
def _negated_value(seed):
    m = FakeModel(seed=seed)
    m.wv = -m.wv
    return m


def test_value_head_changes_alphazero_and_not_reference():
    pis = {}
    for search in ("alphazero", "reference"):
        for tag, model in (("plain", FakeModel(seed=7)), ("negated", _negated_value(7))):
            mc = NativeMCTS(Gomoku, 64, model, cpuct=1.0, batch_size=8, add_dirichlet_noise=False, search=search)
            pis[search, tag], _, _ = play_moves(mc, Gomoku, 3, mc.root_value)
    assert not all(np.array_equal(a, b) for a, b in zip(pis["alphazero", "plain"], pis["alphazero", "negated"]))
    assert all(np.array_equal(a, b) for a, b in zip(pis["reference", "plain"], pis["reference", "negated"]))


class FlatModel:
    """Uniform policy, value 0: nothing but the search's own terminal outcomes tells moves apart."""

    def predict(self, X):
        n = len(X)
        return np.full((n, 225), 1.0 / 225, np.float32), np.zeros((n, 1), np.float32)


@pytest.mark.parametrize("bs", [1, 8])
def test_win_in_one_gets_the_most_visits(bs):
    """Player 1 holds (7,3)..(7,6) with both ends open.  With equal priors the search tries the
    moves in index order; from the first visit of (7,2) on, that edge has q = 1 and every other
    q <= 0 + u with u < 1, so it takes all remaining simulations: 400 - ~108 of them."""
    g = Gomoku(15)
    for c in range(3, 7):
        g.do_move((7, c))
        g.do_move((12, 2 * c - 5))
    assert g.current_player == 1 and not g.is_game_over()
    mc = NativeMCTS(Gomoku, 400, FlatModel(), cpuct=1.0, batch_size=bs, add_dirichlet_noise=False,
                    search="alphazero")
    pi = mc.run(g, len(g.move_history))
    best = int(np.argmax(pi))
    assert best in (7 * 15 + 2, 7 * 15 + 7)
    assert pi[best] > 0.5
    q, v_net, visits = mc.root_value()
    assert q > 0.5 and v_net == 0.0 and visits == 399


# ------------------------------------------------------------ invariants
def test_inflight_zero_at_done_and_root_visits_grow_by_the_budget():
    sims, bs = 50, 8
    f = SearchForest(1, sims, cpuct=1.2, batch_size=bs, search="alphazero", **NOISE)
    assert f.get_search_mode() == 1
    model, rng = FakeModel(seed=9), np.random.RandomState(4)
    g = Gomoku(15)
    saw_inflight = False
    for move in range(5):
        f.set_root(0, g, move)
        try:
            before, existed = f.root_value(0)[2], True
        except RuntimeError:                      # the root has no node yet
            before, existed = 0, False
        assert existed == (move > 0)
        while True:
            p32 = f.noise_request(0)
            if p32 is not None:
                f.set_root_prior(0, (0.75 * p32 + 0.25 * rng.dirichlet([0.3] * 225)).astype(np.float64))
            n = f.advance()
            if f.status[0] != NEED_EVAL:
                break
            assert 1 <= n <= bs
            saw_inflight |= f.inflight(0) > 0
            f.feed(*model.predict(f.leaves[:n]))
        assert f.status[0] == DONE
        assert f.inflight(0) == 0
        q, v_net, visits = f.root_value(0)
        assert visits - before == sims - (0 if existed else 1)
        assert -1.0 <= q <= 1.0
        g.do_move(divmod(int(np.argmax(f.get_pi(0))), 15))
    assert saw_inflight


# ------------------------------------------------------------ independence
def test_forest_equals_games_alone_for_any_thread_count():
    G, sims = 6, 40
    seeds = [41 + i for i in range(G)]
    temp = lambda n: 1.0 if n < 6 else 0.0
    kw = dict(cpuct=1.0, batch_size=8, **NOISE)
    out = {}
    for threads in (1, 4):
        sp = NativeSelfPlay(FakeModel(seed=11).predict, Gomoku, G, sims, n_threads=threads, search="alphazero", **kw)
        out[threads] = sp.play(temp, max_moves=10, use_symmetries=False, seeds=seeds)
        assert sp.max_batch > 8
    for g in range(G):
        alone = NativeMCTS(Gomoku, sims, FakeModel(seed=11), rng=np.random.RandomState(seeds[g]),
                           search="alphazero", **kw)
        ex, w = selfplay.play_game_and_collect(alone, Gomoku(15), temp, max_moves=10, use_symmetries=False)
        for threads in (1, 4):
            assert w == out[threads][g][1] and same_examples(ex, out[threads][g][0])


# ------------------------------------------------------------ drivers
def test_selfplay_drivers_agree_and_equal_the_restatement():
    G, sims = 5, 36
    seeds = [61 + i for i in range(G)]
    temp = lambda n: 1.0 if n < 5 else 0.0
    kw = dict(cpuct=1.1, batch_size=8, **NOISE)
    sync = NativeSelfPlay(FakeModel(seed=12).predict, Gomoku, G, sims, search="alphazero", **kw)
    a = sync.play(temp, max_moves=10, seeds=seeds)
    m = FakeModel(seed=12)
    pipe = NativeSelfPlay(None, Gomoku, G, sims, evaluator_factory=lambda cap: FakeBoardEvaluator(m, cap), groups=2,
                          search="alphazero", **kw)
    b = pipe.play(temp, max_moves=10, seeds=seeds)
    assert len(pipe.forests) == 2
    capped = NativeSelfPlay(FakeModel(seed=12).predict, Gomoku, G, sims, search="alphazero", playout_cap=(1.0, 3),
                            **kw)
    c = capped.play(temp, max_moves=10, seeds=seeds)
    assert capped.fast_moves == 0
    for (ea, wa), (eb, wb), (ec, wc) in zip(a, b, c):
        assert wa == wb == wc and same_examples(ea, eb) and same_examples(ea, ec)
        assert all(e[3] == 1.0 for e in ec)
    # the driver's noise hand-off after set_root: a whole game equals the restatement's
    for g in (0, 3):
        ref = ValueSearch(Gomoku, sims, FakeModel(seed=12), rng=np.random.RandomState(seeds[g]), **kw)
        ex, w = selfplay.play_game_and_collect(ref, Gomoku(15), temp, max_moves=10)
        assert w == a[g][1] and same_examples(ex, a[g][0])


def _openings():
    gs = []
    for o in [(7, 7), (5, 9), (10, 3), (8, 8)]:
        g = Gomoku(15)
        g.do_move(o)
        gs.append(g)
    return gs


def test_native_eval_with_one_mode_per_tag():
    ma, mb = FakeModel(seed=21), FakeModel(seed=21)
    arena = NativeEval({"a": ma.predict, "b": mb.predict}, Gomoku, 4, 24, cpuct=1.3, batch_size=8,
                       search={"a": "alphazero", "b": "reference"})
    assert arena.forests["a"].get_search_mode() == 1 and arena.forests["b"].get_search_mode() == 0
    games = _openings()
    winners = arena.play(games, ["a", "b", "a", "b"])
    assert all(w in (0, 1, 2) for w in winners) and all(g.is_game_over() for g in games)
    assert all(arena.forests["a"].inflight(g) == 0 for g in range(4))
    # one mode for both, through the int8-board evaluators
    both = NativeEval(None, Gomoku, 4, 24, cpuct=1.3, batch_size=8, search="alphazero",
                      evaluator_factories={"a": lambda c: FakeBoardEvaluator(ma, c),
                                           "b": lambda c: FakeBoardEvaluator(mb, c)})
    assert all(w in (0, 1, 2) for w in both.play(_openings(), ["a", "b", "a", "b"]))
    with pytest.raises(ValueError):
        NativeEval({"a": ma.predict, "b": mb.predict}, Gomoku, 4, 24, search={"a": "alphazero"})


def test_evaluate_models_and_selfplay_games_take_the_keyword():
    import random

    import train
    random.seed(3)
    wins, rate, draws = train.evaluate_models(FakeModel(seed=1), FakeModel(seed=2), n_games=2, n_simulations=16,
                                              search={"new": "alphazero", "best": "reference"})
    assert 0 <= wins <= 2 and 0 <= draws <= 2
    ex, winners, drv = selfplay.selfplay_games(FakeModel(seed=1), Gomoku, 2, 16, 1.0, lambda n: 1.0, 0.3, 0.25, 4,
                                               max_moves=6, seeds=[1, 2], search="alphazero")
    assert drv.search == "alphazero" and all(f.get_search_mode() == 1 for f in drv.forests)
    assert len(ex) == 2 * 6 * 8 and sum(winners.values()) == 2


# ------------------------------------------------------------ API errors
def test_api_errors_are_loud():
    f = SearchForest(2, 8, batch_size=4, add_dirichlet_noise=False)
    assert f.get_search_mode() == 0 and f.search == "reference"
    with pytest.raises(RuntimeError, match="unknown mode"):
        f.set_search_mode(2)
    with pytest.raises(RuntimeError, match="unknown mode"):
        f.set_search_mode(-1)
    f.set_root(1, Gomoku(15), 0)
    with pytest.raises(RuntimeError, match="in progress"):
        f.set_search_mode(1)                   # a search is active in slot 1
    while True:
        n = f.advance()
        if f.status[1] != NEED_EVAL:
            break
        f.feed(*FakeModel().predict(f.leaves[:n]))
    assert f.status[1] == DONE
    with pytest.raises(RuntimeError, match="not empty"):
        f.set_search_mode(1)                   # slot 1's tree holds nodes
    assert f.get_search_mode() == 0
    f.clear(1)
    f.set_search_mode(1)
    assert f.get_search_mode() == 1 and f.inflight(0) == 0
    with pytest.raises(RuntimeError, match="root not in tree"):
        f.root_value(0)
    assert f.lib.azg_mcts_inflight(f.h, 2) == -1 and f.lib.azg_mcts_collisions(f.h, -1) == -1
    assert f.lib.azg_mcts_get_search_mode(None) == -1
    for bad in ("AlphaZero", "value", 1, None):
        with pytest.raises(ValueError):
            SearchForest(1, 8, search=bad)
    with pytest.raises(ValueError, match="native"):
        selfplay.selfplay_games(FakeModel(), Gomoku, 1, 8, 1.0, lambda n: 1.0, 0.3, 0.25, 4, native=False,
                                search="alphazero")
    import train
    with pytest.raises(ValueError, match="native"):
        train.evaluate_models(FakeModel(), FakeModel(), n_games=2, n_simulations=8, native=False,
                              search="alphazero")
    with pytest.raises(ValueError):
        train.train_alphazero(search="best", model_dir=os.devnull)


def test_player_takes_the_keyword_directly_and_through_mcts_kwargs():
    from players._alpha_base import AlphaPlayer
    from players.player import Player
    p = Player("gomoku", 15, n_simulations=32, model_path=None, nn_model=FakeModel, search="alphazero")
    q = AlphaPlayer("gomoku", 15, n_simulations=32, nn_model=FakeModel, mcts_kwargs=dict(search="alphazero"))
    r = Player("gomoku", 15, n_simulations=32, model_path=None, nn_model=FakeModel)
    assert p.mcts.forest.get_search_mode() == q.mcts.forest.get_search_mode() == 1
    assert r.mcts.forest.get_search_mode() == 0
    board = np.zeros((15, 15), dtype=int)
    board[7, 7] = 1
    mv = p.play(board.tolist(), 1, (7, 7))
    assert board[mv[0], mv[1]] == 0
    assert p.mcts.root_value()[2] == 31


# ------------------------------------------------------------ reference mode stays
def test_explicit_reference_mode_reproduces_the_goldens():
    with np.load(os.path.join(GOLDEN, "mcts_golden.npz"), allow_pickle=False) as z:
        gold = {k: z[k] for k in z.files}
    np.random.seed(123)
    model = FakeModel(seed=1)
    mcts = NativeMCTS(Gomoku, 60, model, cpuct=1.0, dirichlet_alpha=0.3, epsilon=0.25,
                      apply_dirichlet_n_first_moves=5, add_dirichlet_noise=True, search="reference")
    mcts.forest.set_search_mode(0)
    g = Gomoku(15)
    pis = []
    for _ in range(8):
        pi = mcts.run(g, len(g.move_history))
        pis.append(np.asarray(pi, dtype=np.float64))
        g.do_move(divmod(int(np.argmax(pi)), 15))
    assert np.array_equal(np.stack(pis), gold["noise/pis"])
    assert np.array_equal(np.array(model.calls), gold["noise/calls"])
    assert mcts.tree_size() == int(gold["noise/nkeys"])
    assert mcts.forest.inflight(0) == 0
    q, v_net, visits = mcts.root_value()      # works in reference mode: integer W
    assert visits > 0 and -1.0 <= q <= 1.0
