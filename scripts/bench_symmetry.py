"""Device time per board forward under symmetries (azg_pv_forward_boards_sym) against the
plain board forward, in one process: plain, mode 0 with a random symmetry per board, and
mode 1 (the mean over all 8 images), at 6x128 and B = 512 and 2048 boards (mode 1: B = 256
boards = 2048 images, to be read against the plain forward at 2048).  Every path is timed
with one event pair around `steps` back-to-back forwards on resident inputs; the paths
alternate over `rounds` windows and the medians are reported with every window, so the
spread of the plain path's own windows is visible next to the differences.  A last pass
with the engine's per-class event timing on shows the stem's and the heads' share.

    python scripts/bench_symmetry.py [--steps 200] [--warmup 20] [--rounds 5]

Prints one JSON line.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "alphazero-gomoku_amd")]

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5, help="alternating timed windows per path (medians are reported)")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--batches", type=int, nargs="+", default=[512, 2048])
    args = ap.parse_args()
    from network import PyTorchModel
    from oracle.boards import synth_positions

    torch.manual_seed(0)
    m = PyTorchModel(device="cuda", n_res_blocks=args.blocks, channels=args.channels)
    eng = m.engine
    dev = eng.device
    bmax = max(args.batches)
    boards, players = synth_positions(bmax, seed=21)
    d_boards = torch.from_numpy(np.ascontiguousarray(boards, np.int8).reshape(bmax, 225)).to(dev)
    d_players = torch.from_numpy(np.ascontiguousarray(players, np.int8)).to(dev)
    d_syms = torch.from_numpy(np.random.default_rng(3).integers(0, 8, bmax, dtype=np.int8)).to(dev)
    probs = torch.empty((bmax, 225), dtype=torch.float32, device=dev)
    priors = torch.empty_like(probs)
    values = torch.empty((bmax, 1), dtype=torch.float32, device=dev)

    def forward(kind, B):
        syms = d_syms[:B] if kind == "sym" else None
        return lambda: eng.forward_boards_into(d_boards[:B], d_players[:B], probs[:B], values[:B], priors[:B],
                                               syms=syms, mean8=kind == "mean8")

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        e1.synchronize()
        eng.recover(eng.last_seq())
        return e0.elapsed_time(e1) / args.steps

    paths = []
    for B in args.batches:
        paths += [(f"plain_B{B}", forward("plain", B)), (f"mode0_random_B{B}", forward("sym", B))]
        if B % 8 == 0:
            paths.append((f"mode1_mean8_B{B // 8}", forward("mean8", B // 8)))
    windows = {name: [] for name, _ in paths}
    for _ in range(args.rounds):
        for name, fn in paths:
            windows[name].append(timed(fn))
    out = {"net": f"{args.blocks}x{args.channels}", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "ms_per_forward": {k: round(float(np.median(v)), 4) for k, v in windows.items()},
           "windows_ms": {k: [round(x, 4) for x in v] for k, v in windows.items()}}
    for B in args.batches:
        pl, s0 = windows[f"plain_B{B}"], windows[f"mode0_random_B{B}"]
        out[f"plain_spread_B{B}_ms"] = round(max(pl) - min(pl), 4)
        out[f"mode0_minus_plain_B{B}_ms"] = round(float(np.median(s0) - np.median(pl)), 4)
        if B % 8 == 0:
            out[f"mode1_B{B // 8}_over_plain_B{B}"] = round(float(np.median(windows[f"mode1_mean8_B{B // 8}"]) /
                                                               np.median(pl)), 4)
    # where the time goes: per-class event timing (its own pass; the events cost time themselves)
    classes = {}
    for name, fn in paths:
        eng.profile_enable(True)
        for _ in range(min(args.steps, 50)):
            fn()
        torch.cuda.synchronize()
        prof = eng.profile_read()
        eng.profile_enable(False)
        n = min(args.steps, 50)
        classes[name] = {k: round(ms / n, 4) for k, (ms, _) in prof.items()}
    out["class_ms_per_forward"] = classes
    print(json.dumps(out))


if __name__ == "__main__":
    main()
