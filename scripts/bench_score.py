"""Device time of the scoring launches (azg_pv_score_outputs: score_heads + score_reduce)
beside the eval forward they follow, in one process.

One model on the 6x128 pretrained weights (bench.pretrain: what bench.py measures), exact
precision.  Per batch size, after `warmup` untimed rounds, `rounds` windows of `steps`
iterations of [forward with logits, scoring], each bracketed by hipEvents on the stream:
forward time = event 0 -> 1, scoring time = event 1 -> 2 (the scoring launches are queued
while the forward runs, so their bracket holds device time, not launch latency).  Reported:
the median window's per-iteration times and their ratio; every window is in the JSON line.

    python scripts/bench_score.py [--steps 50] [--warmup 10] [--rounds 5] [--batches 512 3456]
                                  [--out profiles/score_bench.md]

Prints one JSON line and writes the table to --out.  There is no pass / fail number.
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
    ap.add_argument("--rounds", type=int, default=5, help="timed windows (medians are reported)")
    ap.add_argument("--batches", type=int, nargs="+", default=[512, 3456])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "score_bench.md"))
    args = ap.parse_args()
    import bench
    from _native import check, ptr
    from network import PyTorchModel
    from oracle.boards import encode_batch, synth_positions, synth_targets

    torch.manual_seed(0)
    m = PyTorchModel(board_size=15, device="cuda", n_res_blocks=6, channels=128)
    bench.pretrain(m, m.engine.device)
    eng, dev = m.engine, m.engine.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    bmax = max(args.batches)
    boards, players = synth_positions(bmax, seed=21)
    x = torch.from_numpy(encode_batch(boards, players)).to(dev)
    pi, z = synth_targets(bmax, seed=22)
    pis, zs = torch.from_numpy(pi).to(dev), torch.from_numpy(z).to(dev)
    probs = torch.empty((bmax, 225), dtype=torch.float32, device=dev)
    logits = torch.empty_like(probs)
    values = torch.empty((bmax, 1), dtype=torch.float32, device=dev)
    records = torch.empty((bmax, 8), dtype=torch.float32, device=dev)
    sums = torch.empty(8, dtype=torch.float64, device=dev)

    def forward(B):
        eng.forward_into(x[:B], probs[:B], values[:B], logits[:B])

    def score(B):
        check(eng.lib.azg_pv_score_outputs(ptr(logits), ptr(values), ptr(pis), ptr(zs), B, ptr(records), ptr(sums),
                                           stream), eng.lib)

    def window(B):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
        for e0, e1, e2 in ev:
            e0.record()
            forward(B)
            e1.record()
            score(B)
            e2.record()
        torch.cuda.synchronize()
        eng.recover(eng.last_seq())
        eng.check_status()
        fwd = sum(e0.elapsed_time(e1) for e0, e1, _ in ev) / args.steps
        sc = sum(e1.elapsed_time(e2) for _, e1, e2 in ev) / args.steps
        return fwd, sc

    med = lambda v: float(np.median(v))
    out = {"net": "6x128 pretrained, exact", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "batches": {}}
    for B in args.batches:
        for _ in range(args.warmup):
            forward(B)
            score(B)
        torch.cuda.synchronize()
        w = [window(B) for _ in range(args.rounds)]
        fwd, sc = med([a for a, _ in w]), med([b for _, b in w])
        out["batches"][str(B)] = {"forward_ms": round(fwd, 5), "score_ms": round(sc, 5),
                                  "score_over_forward": round(sc / fwd, 5),
                                  "forward_ms_windows": [round(a, 5) for a, _ in w],
                                  "score_ms_windows": [round(b, 5) for _, b in w],
                                  "policy_loss": float(sums.cpu()[0]) / B}
    print(json.dumps(out))
    lines = ["# Scoring launches beside the eval forward (scripts/bench_score.py)", "",
             f"MI355X, {out['net']}; median of {args.rounds} windows of {args.steps} iterations after "
             f"{args.warmup} warm-ups; hipEvent device time per iteration.", "",
             "| batch | forward (ms) | score_heads + score_reduce (ms) | scoring / forward | scoring windows (ms) |",
             "|---|---|---|---|---|"]
    for B, r in out["batches"].items():
        lines.append(f"| {B} | {r['forward_ms']:.4f} | {r['score_ms']:.4f} | {100 * r['score_over_forward']:.2f} % | "
                     f"{', '.join(f'{v:.4f}' for v in r['score_ms_windows'])} |")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
