"""What the opt-in AlphaZero search (search="alphazero": the net's value backed up under
virtual loss) costs and buys beside the default reference search, in one process.

  1. Self-play throughput: 64 games at 400 simulations on a 6x128 net (bench.py's pretrained
     weights: throughput does not depend on what the net has learned), both modes, the same
     seeds, alternating windows: leaf boards/s, positions/s, forwards, mean leaves per game
     per advance, collisions per move.
  2. Strength: ONE net against itself under the two searches (NativeEval with one mode per
     tag), equal simulations, distinct openings, each opening played with both colours.  The
     net is trained here first, by train_alphazero itself (an untrained value head says
     nothing); the table states how.

    python scripts/bench_search_mode.py [--rounds 3] [--games 64] [--sims 400] [--moves 40]
        [--train-iters 40] [--train-games 64] [--train-sims 200] [--match-openings 64]
        [--match-sims 200] [--out profiles/search_mode_bench.md]

Writes the table to --out and prints one JSON line; every window is in both.  No threshold:
the numbers are reported as measured, whichever search they favour.
"""
import argparse
import glob
import json
import os
import random
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "alphazero-gomoku_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

MODES = ("reference", "alphazero")


def throughput(m, args):
    from games.gomoku import Gomoku
    from selfplay import selfplay_games
    temp_fn = lambda n: max(0.0, 1.0 - n / 8)
    # code objects and pinned pools, outside every window
    selfplay_games(m, Gomoku, 8, 64, 1.2, temp_fn, 0.05, 0.15, 10, max_moves=2, use_symmetries=False,
                   seeds=list(range(8)), search="alphazero")
    win = {k: [] for k in MODES}
    for r in range(args.rounds):
        for mode in MODES:
            seeds = [1000 * r + g for g in range(args.games)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ex, _, drv = selfplay_games(m, Gomoku, args.games, args.sims, 1.2, temp_fn, 0.05, 0.15, 10,
                                        max_moves=args.moves, use_symmetries=False, seeds=seeds, search=mode)
            dt = time.perf_counter() - t0
            coll = sum(f.collisions(i) for f in drv.forests for i in range(f.n_games))
            win[mode].append({"boards_per_s": round(drv.boards / dt, 1), "positions_per_s": round(len(ex) / dt, 2),
                              "forwards": drv.forwards, "leaves_per_game_per_advance": round(drv.boards / drv.emits, 3),
                              "collisions_per_move": round(coll / max(1, drv.moves), 3),
                              "boards_per_position": round(drv.boards / len(ex), 2), "positions": len(ex),
                              "search_seconds": round(drv.search_seconds, 3), "nn_seconds": round(drv.nn_seconds, 3),
                              "seconds": round(dt, 3)})
    return win


def train_net(args, model_dir):
    """A net trained by the loop itself, with the value search in self-play and gating."""
    import train
    random.seed(1)
    np.random.seed(1)
    torch.manual_seed(1)
    kw = dict(num_iterations=args.train_iters, games_per_iteration=args.train_games, n_simulations=args.train_sims,
              buffer_size=40000, batch_size=128, epochs_per_iter=2, temp_threshold=8, eval_games=8,
              eval_mcts_simulations=args.train_sims, win_rate_threshold=0.5, cpuct=1.2, dirichlet_alpha=0.05,
              dirichlet_epsilon=0.25, dirichlet_n_moves=10, n_res_blocks=args.train_blocks,
              channels=args.train_channels, max_moves=80, device_buffer=True, search="alphazero")
    hist = []
    t0 = time.perf_counter()
    best = train.train_alphazero(model_dir=model_dir, history=hist, device="cuda:0", **kw)
    best.net.eval()
    kw["seconds"] = round(time.perf_counter() - t0, 1)
    kw["last_train_loss"] = hist[-1]["last_train_loss"] if hist else None
    kw["snapshots"] = len(glob.glob(os.path.join(model_dir, "snapshot_iter*.pt")))
    return best, kw


def match(m, args):
    """One net, two searches: every opening twice, once with each search moving first."""
    from games.gomoku import Gomoku
    from mcts.native_mcts import NativeEval
    cells = [(r, c) for r in range(3, 12) for c in range(3, 12)]          # the centre 9x9, as gating opens
    rng = np.random.RandomState(7)
    openings = [cells[i] for i in rng.permutation(len(cells))[:args.match_openings]]
    games, first = [], []
    for o in openings:
        for tag in MODES:
            g = Gomoku(15)
            g.do_move(o)            # player 1's stone; `tag` plays player 1 from here on, so the other moves next
            games.append(g)
            first.append(tag)
    arena = NativeEval(None, Gomoku, len(games), args.match_sims, cpuct=1.2,
                       evaluator_factories={t: m.board_evaluator for t in MODES}, search={t: t for t in MODES})
    t0 = time.perf_counter()
    winners = arena.play(games, first)
    dt = time.perf_counter() - t0
    res = {"alphazero": 0, "reference": 0, "draws": 0, "as_second_mover": {"alphazero": 0, "reference": 0}}
    for w, tag in zip(winners, first):
        other = MODES[1 - MODES.index(tag)]
        if w == 0:
            res["draws"] += 1
        else:
            won = tag if w == 1 else other
            res[won] += 1
            if won != tag:       # the opening stone belongs to `tag`: the other side made the first free move
                res["as_second_mover"][won] += 1
    res.update(games=len(games), openings=len(openings), sims=args.match_sims, seconds=round(dt, 1),
               mean_length=round(float(np.mean([len(g.move_history) for g in games])), 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="alternating timed windows (>= 3)")
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--moves", type=int, default=40)
    ap.add_argument("--train-iters", type=int, default=40)
    ap.add_argument("--train-games", type=int, default=64)
    ap.add_argument("--train-sims", type=int, default=200)
    ap.add_argument("--train-blocks", type=int, default=3)
    ap.add_argument("--train-channels", type=int, default=64)
    ap.add_argument("--match-openings", type=int, default=64)
    ap.add_argument("--match-sims", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "search_mode_bench.md"))
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    import bench
    from network import PyTorchModel

    torch.manual_seed(0)
    m = PyTorchModel(board_size=15, device="cuda", n_res_blocks=6, channels=128)
    bench.pretrain(m, m.engine.device)
    m.net.eval()
    out = {"throughput": {"net": "6x128 pretrained (bench.py)", "games": args.games, "sims": args.sims,
                          "max_moves": args.moves, "rounds": args.rounds, **throughput(m, args)}}
    with tempfile.TemporaryDirectory() as d:
        net, how = train_net(args, d)
        out["training"] = how
        out["match"] = match(net, args)
    print(json.dumps(out))

    med = lambda v: float(np.median(v))
    fmt = lambda v: ", ".join(f"{t:.4g}" for t in v)
    tp = out["throughput"]
    lines = ["# Reference search and AlphaZero search (scripts/bench_search_mode.py)", "",
             "The default search (`search=\"reference\"`) never reads the value head; `search=\"alphazero\"` backs the "
             "net's value up under virtual loss.  Both are host C++ over the same HIP forward.  No threshold is set: "
             "the numbers are as measured.", "",
             "## Self-play throughput", "",
             f"MI355X, 6x128 pretrained (bench.py's weights), {args.games} games, {args.sims} simulations, at most "
             f"{args.moves} moves each; wall time of selfplay_games, the same seeds for both modes in each of "
             f"{args.rounds} alternating windows; medians, every window listed.", "",
             "| measured | reference | alphazero | reference windows | alphazero windows |", "|---|---|---|---|---|"]
    for key, label in (("boards_per_s", "leaf boards per second"), ("positions_per_s", "positions per second"),
                       ("forwards", "forwards"), ("leaves_per_game_per_advance", "mean leaves per game per advance"),
                       ("collisions_per_move", "collisions per move"),
                       ("boards_per_position", "leaf boards per position"),
                       ("search_seconds", "host search seconds"), ("nn_seconds", "seconds waiting for the forward")):
        u, c = [w[key] for w in tp["reference"]], [w[key] for w in tp["alphazero"]]
        lines.append(f"| {label} | {med(u):.4g} | {med(c):.4g} | {fmt(u)} | {fmt(c)} |")
    how, mt = out["training"], out["match"]
    lines += ["", "## Strength: one net, two searches", "",
              f"Weights: a {how['n_res_blocks']}x{how['channels']} net trained in this run by "
              f"`train_alphazero(search=\"alphazero\", device_buffer=True)` from the seeded init (seeds 1): "
              f"{how['num_iterations']} iterations of {how['games_per_iteration']} self-play games at "
              f"{how['n_simulations']} simulations (at most {how['max_moves']} moves, Dirichlet 0.05 / 0.25 for 10 "
              f"moves), batch {how['batch_size']}, {how['epochs_per_iter']} epochs per iteration, gating over "
              f"{how['eval_games']} games at threshold {how['win_rate_threshold']}; {how['seconds']} s in all; last "
              f"train loss {how['last_train_loss']}.  The weights are not kept.  This is a short run: the net is "
              f"weak, and the match says what the two searches make of THIS net, no more.", "",
              f"Match: NativeEval with search = {{\"alphazero\": \"alphazero\", \"reference\": \"reference\"}} over the "
              f"same weights, {mt['sims']} simulations a move for both, no noise, argmax moves, {mt['openings']} "
              f"distinct opening stones in the centre 9x9, each opening played twice with the searches swapped "
              f"({mt['games']} games, mean length {mt['mean_length']} moves, {mt['seconds']} s).", "",
              "| | alphazero | reference | draws |", "|---|---|---|---|",
              f"| games won | {mt['alphazero']} | {mt['reference']} | {mt['draws']} |",
              f"| of them without the opening stone | {mt['as_second_mover']['alphazero']} | "
              f"{mt['as_second_mover']['reference']} | |"]
    d = os.path.dirname(args.out)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
