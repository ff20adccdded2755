"""Cost of surprise-weighted sampling from the device replay buffer (csrc/pv_replay_weights.hip,
replay.DeviceReplayBuffer.sample_weighted) beside the uniform sample() of the same ring, in
one process.

Per ring size (positions held; nsym = 8), with random weights in the ring:
  prefix        azg_pv_replay_prefix alone (runs once per buffer change, not per batch)
  weighted      sample_weighted(B): H2D of 2 B random words + draw + gather
  uniform       sample(B):          H2D of B ids + gather (the ids from random.sample)
for B = 128 and 512, and once:
  add           scoring 4,000 fresh positions (eval forward + score kernels, chunks of 4096,
                train._score_surprise) and add_positions(..., surprise=records), beside the
                plain add_positions of the same examples.
Each figure is taken twice: DEVICE time from hipEvents recorded on the stream around every
call, and HOST time per call from perf_counter over the window's enqueue loop (what the
training loop's thread spends: for the uniform path this holds random.sample, for the
weighted one 2 B random.getrandbits).  These calls take the host longer to enqueue than the
GPU to run, so on an idle stream an event bracket would hold the host's time again: every
window therefore first queues `--blocker` large fp32 matmuls (tens of ms), the window's calls
pile up behind them, and the brackets hold device time (copies and kernels back to back).
After `warmup` untimed calls, `rounds` windows of `steps` calls; the weighted and uniform
windows alternate; medians of the windows are reported and every window is in the JSON line.
`add` synchronises inside (the scoring sums go to the host), so it is reported as wall time
per call.

    python scripts/bench_replay_weighted.py [--steps 50] [--warmup 10] [--rounds 5]
        [--counts 7500 125000] [--batches 128 512] [--out profiles/replay_weighted_bench.md]

Prints one JSON line and writes the table to --out.  There is no pass / fail number.
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


def _examples(n, seed):
    from synth import synth_encoded
    rng = np.random.default_rng(seed)
    states = synth_encoded(n, seed=seed)
    pi = rng.random((n, 225)).astype(np.float32)
    pi /= pi.sum(1, keepdims=True)
    z = rng.integers(-1, 2, n).astype(np.float32)
    return [(states[i], pi[i], float(z[i])) for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per figure (medians are reported)")
    ap.add_argument("--counts", type=int, nargs="+", default=[7500, 125000])
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--fresh", type=int, default=4000, help="positions of the timed add_positions")
    ap.add_argument("--blocker", type=int, default=8, help="8192^2 fp32 matmuls queued in front of every window")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "replay_weighted_bench.md"))
    args = ap.parse_args()
    import train
    from _native import check, ptr
    from network import PyTorchModel
    from replay import DeviceReplayBuffer

    dev = torch.device("cuda:0")
    med = lambda v: float(np.median(v))
    r5 = lambda v: [round(x, 5) for x in v]

    blk_a = torch.randn((8192, 8192), dtype=torch.float32, device=dev)
    blk_c = torch.empty_like(blk_a)
    torch.mm(blk_a, blk_a, out=blk_c)
    torch.cuda.synchronize()
    b0, b1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b0.record()
    for _ in range(args.blocker):
        torch.mm(blk_a, blk_a, out=blk_c)
    b1.record()
    torch.cuda.synchronize()
    blocker_ms = b0.elapsed_time(b1)
    queued = []   # per window: did the last call's enqueue end before the blocker did?

    def window(fn):
        """(device ms, host ms) per call over one window of args.steps calls."""
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        done = torch.cuda.Event()
        torch.cuda.synchronize()
        for _ in range(args.blocker):
            torch.mm(blk_a, blk_a, out=blk_c)
        done.record()
        t0 = time.perf_counter()
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        host = (time.perf_counter() - t0) / args.steps * 1e3
        queued.append(not done.query())
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in ev) / args.steps, host

    fresh = _examples(args.fresh, seed=5)
    out = {"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "blocker_ms": round(blocker_ms, 2),
           "counts": {}}
    for count in args.counts:
        buf = DeviceReplayBuffer(count * 8, dev)
        for lo in range(0, count, 25000):                      # bounded host staging
            buf.add_positions(_examples(min(25000, count - lo), seed=100 + lo))
        rng = np.random.default_rng(count)
        buf.set_weights(0.5 + 0.5 * rng.gamma(0.5, 2.0, size=count).clip(0, 1000))   # the loop's shape at mix 0.5
        stream = torch.cuda.current_stream(dev).cuda_stream
        res = {"ess_positions": round(buf.effective_sample_size(), 1)}

        def prefix():
            check(buf.lib.azg_pv_replay_prefix(ptr(buf._wq), buf.cap_pos, buf.head, buf.count, ptr(buf._prefix),
                                               stream), buf.lib)

        for _ in range(args.warmup):
            prefix()
        w = [window(prefix) for _ in range(args.rounds)]
        res["prefix"] = {"device_ms": round(med([a for a, _ in w]), 5), "host_ms": round(med([b for _, b in w]), 5),
                         "device_ms_windows": r5([a for a, _ in w])}
        for B in args.batches:
            paths = {"weighted": lambda: buf.sample_weighted(B), "uniform": lambda: buf.sample(B)}
            for fn in paths.values():
                for _ in range(args.warmup):
                    fn()
            wins = {k: [] for k in paths}
            for _ in range(args.rounds):                        # the two paths alternate
                for k, fn in paths.items():
                    wins[k].append(window(fn))
            for k, w in wins.items():
                res[f"{k}_B{B}"] = {"device_ms": round(med([a for a, _ in w]), 5),
                                    "host_ms": round(med([b for _, b in w]), 5),
                                    "device_ms_windows": r5([a for a, _ in w]),
                                    "host_ms_windows": r5([b for _, b in w])}
        out["counts"][str(count)] = res
        del buf
        torch.cuda.empty_cache()

    # one iteration's hand-over: score the fresh positions, add them with their surprise
    torch.manual_seed(0)
    model = PyTorchModel(board_size=15, device=str(dev), n_res_blocks=6, channels=128)
    buf = DeviceReplayBuffer(max(args.counts) * 8, dev)
    buf.add_positions(fresh, surprise=train._score_surprise(model, fresh), mix=0.5)       # warm-up
    t_score, t_add, t_plain = [], [], []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec = train._score_surprise(model, fresh)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        buf.add_positions(fresh, surprise=rec, mix=0.5)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        buf.add_positions(fresh)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        t_score.append((t1 - t0) * 1e3)
        t_add.append((t2 - t1) * 1e3)
        t_plain.append((t3 - t2) * 1e3)
    out["add"] = {"positions": args.fresh, "net": "6x128, exact", "score_ms": round(med(t_score), 3),
                  "add_with_surprise_ms": round(med(t_add), 3), "add_plain_ms": round(med(t_plain), 3),
                  "score_ms_rounds": r5(t_score), "add_with_surprise_ms_rounds": r5(t_add),
                  "add_plain_ms_rounds": r5(t_plain)}
    out["windows_fully_queued_behind_blocker"] = f"{sum(queued)} of {len(queued)}"
    print(json.dumps(out))

    lines = ["# Surprise-weighted sampling from the device replay buffer (scripts/bench_replay_weighted.py)", "",
             f"MI355X, nsym = 8, random weights (0.5 + 0.5 gamma); median of {args.rounds} windows of {args.steps} "
             f"calls after {args.warmup} warm-ups, weighted and uniform windows alternating.  Device ms: hipEvents "
             f"around each call, every window queued behind {out['blocker_ms']:.0f} ms of matmuls so that the brackets "
             f"hold device work and not the host's enqueue time ({out['windows_fully_queued_behind_blocker']} windows "
             "were enqueued entirely before the matmuls ended); host ms: the calling thread's time per call (enqueue, "
             "the random draws included).", "",
             "| positions | call | device (ms) | host (ms) | device windows (ms) |", "|---|---|---|---|---|"]
    for count, res in out["counts"].items():
        for k, r in res.items():
            if isinstance(r, dict):
                lines.append(f"| {count} | {k} | {r['device_ms']:.4f} | {r['host_ms']:.4f} | "
                             f"{', '.join(f'{v:.4f}' for v in r['device_ms_windows'])} |")
    a = out["add"]
    lines += ["", f"One iteration's hand-over of {a['positions']} fresh positions ({a['net']}; wall ms, synchronised, "
              f"median of {args.rounds}): scoring forward + score kernels {a['score_ms']:.2f}; "
              f"add_positions with surprise {a['add_with_surprise_ms']:.2f}; plain add_positions of the same examples "
              f"{a['add_plain_ms']:.2f}.", "",
              "Effective sample size of the benchmark's weights: " +
              ", ".join(f"{r['ess_positions']:.0f} of {c} positions" for c, r in out["counts"].items()) + "."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
