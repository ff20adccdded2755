"""The one-product fp16 eval precision against the exact one, in one process, alternating.

Two models on the same 6x128 pretrained weights (bench.pretrain: what bench.py measures),
one "exact" and one "fp16" (PyTorchModel.set_eval_precision).  Per batch size the two
alternate over `rounds` windows:
  * the tower's device time per forward (the engine's AZG_PROF_BOARD16 event brackets, in
    windows of their own: the events cost time themselves),
  * whole-forward boards/s from int8 boards (one event pair around `steps` forwards).
Then a NativeSelfPlay leg (bench.py's driver and settings; the same games, sims, seeds and
move rounds for both) reporting leaf boards/s, and over one set of boards the deviation
between the two models: max |dprobs|, max |dvalues|, masked-argmax agreement and the share
of boards whose exact masked top-two gap is below 4 x max |dprobs| (the near-ties).

    python scripts/bench_precision.py [--steps 50] [--warmup 10] [--rounds 5]
                                      [--sp-games 64] [--sp-sims 100] [--sp-rounds 6]

Prints one JSON line; every window is in it, so the run-to-run spread is next to each ratio.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "alphazero-gomoku_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="alternating timed windows per model (medians are reported)")
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 85, 512, 3456])
    ap.add_argument("--sp-games", type=int, default=64)
    ap.add_argument("--sp-sims", type=int, default=100)
    ap.add_argument("--sp-rounds", type=int, default=6, help="move rounds per self-play window")
    ap.add_argument("--sp-windows", type=int, default=3)
    args = ap.parse_args()
    import bench
    from games.gomoku import Gomoku
    from network import PyTorchModel
    from oracle.boards import synth_positions, valid_mask

    models = {}
    for name in ("exact", "fp16"):
        torch.manual_seed(0)
        m = PyTorchModel(board_size=15, device="cuda", n_res_blocks=6, channels=128)
        bench.pretrain(m, m.engine.device)
        m.set_eval_precision(name)
        models[name] = m
    dev = models["exact"].engine.device
    bmax = max(args.batches)
    boards, players = synth_positions(bmax, seed=21)
    bi8 = np.ascontiguousarray(boards, np.int8).reshape(bmax, 225)
    d_boards = torch.from_numpy(bi8).to(dev)
    d_players = torch.from_numpy(np.ascontiguousarray(players, np.int8)).to(dev)
    probs = torch.empty((bmax, 225), dtype=torch.float32, device=dev)
    priors = torch.empty_like(probs)
    values = torch.empty((bmax, 1), dtype=torch.float32, device=dev)

    def forward(m, B):
        eng = m.engine
        return lambda: eng.forward_boards_into(d_boards[:B], d_players[:B], probs[:B], values[:B], priors[:B])

    def settle(m):
        torch.cuda.synchronize()
        m.engine.recover(m.engine.last_seq())
        m.engine.check_status()

    def wall_window(m, B):
        fn = forward(m, B)
        for _ in range(args.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        e1.synchronize()
        settle(m)
        return e0.elapsed_time(e1) / args.steps

    def tower_window(m, B):
        fn, eng = forward(m, B), m.engine
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        eng.profile_enable(True)
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        prof = eng.profile_read()
        eng.profile_enable(False)
        settle(m)
        return prof["board16"][0] / args.steps

    med = lambda v: float(np.median(v))
    out = {"net": "6x128 pretrained", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "forward": {}}
    for B in args.batches:
        w = {(k, n): [] for k in ("tower_ms", "forward_ms") for n in models}
        for _ in range(args.rounds):
            for n, m in models.items():
                w[("tower_ms", n)].append(tower_window(m, B))
            for n, m in models.items():
                w[("forward_ms", n)].append(wall_window(m, B))
        r = {}
        for k in ("tower_ms", "forward_ms"):
            for n in models:
                r[f"{k}_{n}"] = round(med(w[(k, n)]), 4)
                r[f"{k}_{n}_windows"] = [round(x, 4) for x in w[(k, n)]]
            r[f"{k}_exact_over_fp16"] = round(med(w[(k, "exact")]) / med(w[(k, "fp16")]), 3)
            # the ratio's spread: the extreme window pairings
            r[f"{k}_ratio_range"] = [round(min(w[(k, "exact")]) / max(w[(k, "fp16")]), 3),
                                     round(max(w[(k, "exact")]) / min(w[(k, "fp16")]), 3)]
        for n in models:
            r[f"boards_per_s_{n}"] = round(B / med(w[("forward_ms", n)]) * 1e3, 0)
        out["forward"][str(B)] = r

    # deviation between the two models over the same boards
    nb = min(bmax, 2048)
    pe, ve = models["exact"].predict_boards(bi8[:nb], np.asarray(players[:nb], np.int8), masked=False)
    ph, vh = models["fp16"].predict_boards(bi8[:nb], np.asarray(players[:nb], np.int8), masked=False)
    masks = np.stack([valid_mask(b) for b in boards[:nb]])
    dp = float(np.abs(ph - pe).max())
    srt = np.sort(pe * masks, axis=1)
    out["deviation"] = {"boards": nb, "max_dprobs": dp, "max_dvalues": float(np.abs(vh - ve).max()),
                        "masked_argmax_agreement": float((np.argmax(ph * masks, 1) == np.argmax(pe * masks, 1)).mean()),
                        "near_tie_share": float(((srt[:, -1] - srt[:, -2]) < 4 * dp).mean())}

    # self-play: bench.py's driver and settings, the same games / sims / seeds / move rounds
    G, S = args.sp_games, args.sp_sims
    if G > 0:
        sp_w = {n: [] for n in models}
        drivers = {}
        for n, m in models.items():
            m.net.eval()
            bench.selfplay_run(m, Gomoku, 8, 64, 2, [10_000 + i for i in range(8)], profile=False)
            bench.visit_buckets(m, (G + 1) // 2 * 32)
            drivers[n] = bench.selfplay_driver(m, Gomoku, G, S)
        for k in range(args.sp_windows):
            for n, m in models.items():
                sp, dt, _, _, _ = bench.selfplay_run(m, Gomoku, G, S, 225, [1000 * k + i for i in range(G)],
                                                     profile=False, steps=args.sp_rounds, sp=drivers[n])
                sp_w[n].append(sp.boards / dt)
        out["selfplay"] = {"games": G, "sims": S, "move_rounds": args.sp_rounds,
                           **{f"leaf_boards_per_s_{n}": round(med(v), 0) for n, v in sp_w.items()},
                           **{f"leaf_boards_per_s_{n}_windows": [round(x, 0) for x in v] for n, v in sp_w.items()},
                           "fp16_over_exact": round(med(sp_w["fp16"]) / med(sp_w["exact"]), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
