"""What per-example loss weights and playout cap randomization cost and buy, in one process.

  1. The loss launch: device time of heads_loss_weighted_kernel beside heads_loss_kernel
     (6x128, B = 128), read from torch.profiler's kernel records of the same train steps.
  2. The whole 6x128, B = 128 train step (bench.py's train leg: pretrained weights, pipelined
     train_batch_device(return_tensor=True)) with and without weights, in alternating
     windows of one model.
  3. Self-play with and without a cap of (0.25, n_simulations / 8), alternating: positions per
     second, leaf boards per position and the share of fully searched moves.

    python scripts/bench_playout_cap.py [--steps 50] [--warmup 10] [--rounds 5]
        [--games 64] [--sims 400] [--moves 40] [--out profiles/playout_cap_bench.md]

Writes the table to --out and prints one JSON line; every window is in both, so the spread
is next to each difference.  No threshold: the numbers are reported as measured.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "alphazero-gomoku_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def loss_kernel_times(step_plain, step_weighted, steps):
    """{kernel name: [device us per launch]} of the two loss kernels from torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    out = {}
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(steps):
                step_plain()
                step_weighted()
            torch.cuda.synchronize()
        for ev in prof.events():
            if "heads_loss" in ev.name:
                name = "heads_loss_weighted_kernel" if "weighted" in ev.name else "heads_loss_kernel"
                out.setdefault(name, []).append(float(ev.device_time))
    except Exception as e:   # no kernel records on this build: say so in the table
        out["error"] = repr(e)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="alternating timed windows (>= 3)")
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--moves", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "playout_cap_bench.md"))
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    import bench
    from games.gomoku import Gomoku
    from network import PyTorchModel
    from selfplay import selfplay_games
    from synth import synth_encoded

    torch.manual_seed(0)
    m = PyTorchModel(board_size=15, device="cuda", n_res_blocks=6, channels=128)
    bench.pretrain(m, m.engine.device)
    eng = m.engine
    dev = eng.device
    B = 128
    rng = np.random.default_rng(77)                       # bench.py train_leg's batch
    x = torch.from_numpy(synth_encoded(B, seed=77)).to(dev)
    pi = rng.random((B, 225)).astype(np.float32)
    pi /= pi.sum(1, keepdims=True)
    pi = torch.from_numpy(pi).to(dev)
    z = torch.from_numpy(rng.integers(-1, 2, (B, 1)).astype(np.float32)).to(dev)
    wp = torch.from_numpy((rng.random(B) < 0.25).astype(np.float32)).to(dev)     # a cap of 0.25: 1 in 4 trains the policy head

    plain = lambda: m.train_batch_device(x, pi, z, return_tensor=True)
    weighted = lambda: m.train_batch_device(x, pi, z, return_tensor=True, policy_weight=wp)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    out = {"net": "6x128 pretrained", "batch": B, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds}
    # 2. the step, alternating
    win = {"plain": [], "weighted": []}
    for _ in range(args.rounds):
        for name, fn in (("plain", plain), ("weighted", weighted)):
            win[name].append(timed(fn))
            assert eng.train_skips() == 0
    out["step_ms"] = {k: [round(v, 4) for v in w] for k, w in win.items()}
    # 1. the two loss kernels
    for _ in range(args.warmup):
        plain()
        weighted()
    torch.cuda.synchronize()
    kt = loss_kernel_times(plain, weighted, args.steps)
    out["loss_kernel_us"] = {k: ({"n": len(v), "median": round(float(np.median(v)), 3), "min": round(min(v), 3),
                                  "max": round(max(v), 3)} if isinstance(v, list) else v) for k, v in kt.items()}

    # 3. self-play, alternating
    m.net.eval()
    cap = (0.25, max(1, args.sims // 8))
    temp_fn = lambda n: max(0.0, 1.0 - n / 8)
    sp = {"plain": [], "cap": []}
    for r in range(args.rounds):
        for name, pc in (("plain", None), ("cap", cap)):
            seeds = [1000 * r + g for g in range(args.games)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ex, _, drv = selfplay_games(m, Gomoku, args.games, args.sims, 1.2, temp_fn, 0.05, 0.15, 10,
                                        max_moves=args.moves, use_symmetries=False, seeds=seeds, playout_cap=pc)
            dt = time.perf_counter() - t0
            sp[name].append({"positions_per_s": round(len(ex) / dt, 2), "boards_per_position": round(drv.boards / len(ex), 2),
                             "positions": len(ex), "full_share": round(drv.full_moves / len(ex), 3) if pc else 1.0,
                             "seconds": round(dt, 3)})
    out["selfplay"] = {"games": args.games, "sims": args.sims, "cap_setting": list(cap), "max_moves": args.moves, **sp}
    print(json.dumps(out))

    med = lambda v: float(np.median(v))
    fmt = lambda v: ", ".join(f"{t:.4g}" for t in v)
    a, b = win["plain"], win["weighted"]
    lines = ["# Per-example loss weights and playout cap randomization (scripts/bench_playout_cap.py)", "",
             f"MI355X, 6x128 pretrained, B = {B}; medians of {args.rounds} alternating windows of {args.steps} steps after "
             f"{args.warmup} warm-ups (hipEvent time per step); every window is listed.", "",
             "## Train step", "",
             "| measured | unweighted | weighted | weighted - unweighted | unweighted windows | weighted windows |",
             "|---|---|---|---|---|---|",
             f"| whole step (ms) | {med(a):.4f} | {med(b):.4f} | {med(b) - med(a):+.4f} | {fmt(a)} | {fmt(b)} |"]
    ku = out["loss_kernel_us"]
    if "heads_loss_kernel" in ku and "heads_loss_weighted_kernel" in ku:
        p, q = ku["heads_loss_kernel"], ku["heads_loss_weighted_kernel"]
        lines.append(f"| loss kernel alone (us, profiler records, n = {p['n']} / {q['n']}) | {p['median']:.3f} | {q['median']:.3f} | "
                     f"{q['median'] - p['median']:+.3f} | min {p['min']:.3f} max {p['max']:.3f} | min {q['min']:.3f} max {q['max']:.3f} |")
    else:
        lines.append(f"| loss kernel alone | not measured: the profiler gave no kernel records ({ku}) | | | | |")
    lines += ["", "## Self-play", "",
              f"{args.games} games, {args.sims} simulations, at most {args.moves} moves each, cap ({cap[0]}, {cap[1]}); wall time "
              f"of selfplay_games, the same seeds for both in each round.", "",
              "| measured | no cap | cap | no-cap windows | cap windows |", "|---|---|---|---|---|"]
    for key, label in (("positions_per_s", "positions per second"), ("boards_per_position", "leaf boards per position"),
                       ("full_share", "share of fully searched moves")):
        u, c = [w[key] for w in sp["plain"]], [w[key] for w in sp["cap"]]
        lines.append(f"| {label} | {med(u):.4g} | {med(c):.4g} | {fmt(u)} | {fmt(c)} |")
    d = os.path.dirname(args.out)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
