"""Playout cap randomization in the native search and self-play driver, on the CPU with the
fake model: azg_mcts_set_budget (per slot: simulations, root noise) and
NativeSelfPlay(playout_cap=(p_full, fast_sims)).  Every comparison is exact: games, moves,
policy targets and weights."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from fake_model import FakeBoardEvaluator, FakeModel  # noqa: E402

import _native_mcts  # noqa: E402
import selfplay  # noqa: E402
from games.gomoku import Gomoku  # noqa: E402
from mcts.native_mcts import NativeSelfPlay  # noqa: E402

G = 5
SEEDS = [71 + 13 * i for i in range(G)]
FULL, FAST = 16, 4
KW = dict(cpuct=1.1, dirichlet_alpha=0.3, epsilon=0.25, apply_dirichlet_n_first_moves=6)
MAX_MOVES = 12


def temp(n):
    return 1.0 if n < 5 else 0.0


def _play(n_sims, playout_cap=None, use_symmetries=False, seeds=SEEDS, **kw):
    args = dict(KW)
    args.update(kw)
    sp = NativeSelfPlay(FakeModel(seed=12).predict, Gomoku, len(seeds), n_sims, playout_cap=playout_cap, **args)
    return sp, sp.play(temp, max_moves=MAX_MOVES, use_symmetries=use_symmetries, seeds=seeds)


def _same(a, b, weight=None):
    """Results a (3-tuples) and b (3- or 4-tuples) hold the same games; weight: b's 4th field."""
    assert len(a) == len(b)
    for (ea, wa), (eb, wb) in zip(a, b):
        assert wa == wb and len(ea) == len(eb) and len(ea) > 0
        for x, y in zip(ea, eb):
            assert len(x) == 3 and len(y) == (3 if weight is None else 4)
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]
            assert x[1].dtype == y[1].dtype == np.float32
            if weight is not None:
                assert y[3] == weight and isinstance(y[3], float)


def _coins(seed, n, p_full):
    rs = np.random.RandomState((seed + 0x9E3779B1) % 2 ** 32)
    return [bool(rs.random_sample() < p_full) for _ in range(n)]


@pytest.mark.parametrize("sym", [False, True])
def test_cap_with_p_full_1_is_the_plain_driver(sym):
    plain_sp, plain = _play(FULL, use_symmetries=sym)
    cap_sp, cap = _play(FULL, playout_cap=(1.0, FAST), use_symmetries=sym)
    _same(plain, cap, weight=1.0)
    assert cap_sp.boards == plain_sp.boards and cap_sp.moves == plain_sp.moves
    assert cap_sp.full_moves == cap_sp.moves and cap_sp.fast_moves == 0
    assert plain_sp.full_moves == plain_sp.fast_moves == 0 and plain_sp.playout_cap is None


@pytest.mark.parametrize("sym", [False, True])
def test_cap_with_p_full_0_is_the_small_search_without_noise(sym):
    plain_sp, plain = _play(FAST, use_symmetries=sym, add_dirichlet_noise=False)
    cap_sp, cap = _play(FULL, playout_cap=(0.0, FAST), use_symmetries=sym)
    _same(plain, cap, weight=0.0)
    assert cap_sp.boards == plain_sp.boards and cap_sp.boards <= FAST * cap_sp.moves
    assert cap_sp.fast_moves == cap_sp.moves > 0 and cap_sp.full_moves == 0
    # and the noise matters in this setup: the noisy small search plays other games
    _, noisy = _play(FAST, use_symmetries=sym)
    assert any(wa != wb or len(ea) != len(eb) or any(not np.array_equal(x[1], y[1]) for x, y in zip(ea, eb))
               for (ea, wa), (eb, wb) in zip(plain, noisy))


def _flags(results):
    return [[e[3] == 1.0 for e in ex] for ex, _ in results]


def test_mixed_cap_follows_the_coin_stream_of_each_seed():
    sp, out = _play(FULL, playout_cap=(0.5, FAST))
    flags = _flags(out)
    for seed, f in zip(SEEDS, flags):
        assert f == _coins(seed, len(f), 0.5)
        assert all(e[3] in (0.0, 1.0) for ex, _ in out for e in ex)
    n_full = sum(sum(f) for f in flags)
    n_all = sum(len(f) for f in flags)
    assert sp.full_moves == n_full and sp.fast_moves == n_all - n_full and sp.moves == n_all
    assert 0 < n_full < n_all                       # both kinds occur
    # the images of a position share its weight
    _, sym = _play(FULL, playout_cap=(0.5, FAST), use_symmetries=True)
    for (ex, _), (ex8, _) in zip(out, sym):
        assert len(ex8) == 8 * len(ex)
        assert [e[3] for e in ex8] == [e[3] for e in ex for _ in range(8)]
        assert all(np.array_equal(ex8[8 * t][0], ex[t][0]) and np.array_equal(ex8[8 * t][1], ex[t][1])
                   for t in range(len(ex)))
    # a game's coins (and so its moves) do not depend on which games it is played beside
    _, alone = _play(FULL, playout_cap=(0.5, FAST), seeds=SEEDS[2:3])
    assert _flags(alone)[0] == flags[2]
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(alone[0][0], out[2][0]))


def _same4(a, b):
    assert len(a) == len(b)
    for (ea, wa), (eb, wb) in zip(a, b):
        assert wa == wb and len(ea) == len(eb)
        for x, y in zip(ea, eb):
            assert len(x) == len(y) == 4
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2:] == y[2:]


@pytest.mark.parametrize("groups,threads", [(1, 1), (2, 1), (1, 4), (2, 4)])
def test_mixed_cap_is_independent_of_grouping_and_threads(groups, threads):
    _, want = _play(FULL, playout_cap=(0.5, FAST), n_threads=1)
    m = FakeModel(seed=12)
    sp = NativeSelfPlay(None, Gomoku, G, FULL, evaluator_factory=lambda cap: FakeBoardEvaluator(m, cap),
                        groups=groups, n_threads=threads, playout_cap=(0.5, FAST), **KW)
    got = sp.play(temp, max_moves=MAX_MOVES, use_symmetries=False, seeds=SEEDS)
    assert len(sp.forests) == groups
    _same4(want, got)


def test_set_budget_takes_effect_at_the_next_root_and_survives_clear():
    """A slot's budget holds from its next set_root on.  With fewer simulations than the leaf
    queue holds (32) no simulation is ever suspended, so a search asks for at most one leaf
    per simulation."""
    model = FakeModel(seed=3)

    def search(f):
        n_leaves = 0
        f.set_root(0, Gomoku(15), 0)
        while True:
            n = f.advance()
            if f.status[0] != _native_mcts.NEED_EVAL:
                break
            n_leaves += n
            f.feed(*model.predict(f.leaves[:n]))
            assert f.noise_request(0) is None
        return n_leaves, f.get_pi(0)

    f = _native_mcts.SearchForest(1, 12, add_dirichlet_noise=False)
    n12, pi12 = search(f)
    f.clear(0)
    f.set_budget(0, 3, 0)
    f.clear(0)
    n3, pi3 = search(f)
    assert 0 < n3 <= 3 < n12 <= 12
    f.clear(0)
    f.set_budget(0)                       # back to the forest's own
    n12b, pi12b = search(f)
    assert n12b == n12 and np.array_equal(pi12b, pi12)
    # the noise switch: a forest with noise on, told "no noise" for the slot, asks for none
    f2 = _native_mcts.SearchForest(1, 4, add_dirichlet_noise=True, batch_size=1)
    f2.set_budget(0, -1, 0)
    search(f2)                            # asserts noise_request is None after every feed
    f2.clear(0)
    f2.set_budget(0, -1, -1)
    f2.set_root(0, Gomoku(15), 0)
    n = f2.advance()
    f2.feed(*model.predict(f2.leaves[:n]))
    assert f2.noise_request(0) is not None


def test_bad_caps_and_the_python_driver_are_refused():
    for bad in ((1.5, 4), (-0.1, 4), (0.5, -1), (0.5, 2.5)):
        with pytest.raises(ValueError):
            NativeSelfPlay(FakeModel().predict, Gomoku, 1, 8, playout_cap=bad)
    with pytest.raises(ValueError, match="native"):
        selfplay.selfplay_games(FakeModel(), Gomoku, 1, 8, 1.0, temp, 0.3, 0.25, 4, native=False,
                                playout_cap=(0.5, 2))
    ex, winners, drv = selfplay.selfplay_games(FakeModel(seed=12), Gomoku, 2, FULL, 1.1, temp, 0.3, 0.25, 6,
                                               max_moves=6, use_symmetries=False, seeds=SEEDS[:2],
                                               playout_cap=(0.5, FAST))
    assert len(ex) == 12 and all(len(e) == 4 for e in ex) and drv.full_moves + drv.fast_moves == 12
