"""bench.py's timed self-play on CPU (a test double stands in for the HIP model):
--steps K really plays K move rounds, whatever the games' lengths, with the same
results from run to run, and --dump-outputs writes the last round's examples of the
games that moved in it."""
import sys
import types

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
from fake_model import FakeBoardEvaluator, FakeModel  # noqa: E402

import bench  # noqa: E402
from games.gomoku import Gomoku  # noqa: E402

G, SIMS, MAX_MOVES = 6, 16, 12


class _Engine:
    """The engine calls selfplay_run makes around the games: nothing to profile here."""

    def tower_diag(self):
        return {k: 0 for k in ("waits_over_100us", "waits_over_1ms", "waits_over_10ms", "max_wait_us", "max_wall_us",
                               "waits_suspended", "timeouts", "recovered", "breaker_trips", "breaker_launches")}

    def profile_read(self):
        return {}

    profile_boards = profile_read

    def __getattr__(self, name):
        return lambda *a, **k: None


@pytest.fixture
def model(monkeypatch):
    monkeypatch.setattr(bench.torch.cuda, "synchronize", lambda *a, **k: None)
    fake = FakeModel(seed=3)
    return types.SimpleNamespace(engine=_Engine(), board_evaluator=lambda cap: FakeBoardEvaluator(fake, cap))


def run(model, steps):
    return bench.selfplay_run(model, Gomoku, G, SIMS, MAX_MOVES, list(range(G)), steps=steps)


@pytest.mark.parametrize("steps,generations", [(1, [1]), (7, [7]), (12, [12]), (30, [12, 12, 6])])
def test_steps_sets_the_rounds_played(model, steps, generations):
    """MAX_MOVES = 12 ends every generation after 12 rounds at the latest (no game of
    16-simulation searches wins sooner here): 30 steps are 12 + 12 + 6 rounds."""
    sp, _, _, _, results = run(model, steps)
    assert sp.rounds == steps and sp.last_rounds == generations[-1]
    assert sp.game_lengths == [n for n in generations for _ in range(G)]
    assert sp.moves == steps * G
    assert [len(ex) for ex, _ in results] == [8 * generations[-1]] * G


def test_without_steps_one_whole_generation(model):
    sp, _, _, _, results = run(model, None)
    assert sp.rounds == sp.last_rounds == MAX_MOVES and len(sp.game_lengths) == G


def test_dump_outputs_last_round_and_repeatable(model, tmp_path):
    outs = []
    for d in ("a", "b"):
        sp, _, _, _, results = run(model, 14)
        # a game that ended before the last round has nothing in it
        results[2] = (results[2][0][:8], results[2][1])
        bench.dump_outputs(str(tmp_path / d), results, sp.last_rounds)
        outs.append({n: np.load(tmp_path / d / f"{n}.npy") for n in ("game_index", "state", "pi", "z", "winner")})
    a, b = outs
    assert a["game_index"].tolist() == [0, 1, 3, 4, 5]
    assert a["state"].shape == (5, 8, 3, 15, 15) and a["pi"].shape == (5, 8, 225) and a["z"].shape == (5, 8)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    np.testing.assert_allclose(a["pi"].sum(-1), 1.0, atol=1e-6)
    # round 14 of the run is the 2nd of the second generation: one stone on the board before it
    assert (a["state"][:, :, :2].sum((2, 3, 4)) == 1).all()
    ex = results[0][0][-8:]
    assert np.array_equal(a["state"][0], np.stack([e[0] for e in ex]))
    assert np.array_equal(a["pi"][0], np.stack([e[1] for e in ex]))
    for n in a:
        assert np.array_equal(a[n], b[n]), n
