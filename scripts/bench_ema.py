"""The cost of the weight average (EMA) in the train step: EMA on against EMA off, in one
process, alternating.

One 6x128 model on pretrained weights (bench.pretrain: what bench.py measures) runs bench.py's
train leg -- B = 128, pipelined steps (train_batch_device(return_tensor=True)), the same batch
-- with the average bound (enable_ema) and unbound (disable_ema) in alternating windows, so
both configurations see the same allocations.  Per round, after warm-up:
  * the whole step (one event pair around `steps` steps),
  * clip + Adam + repack alone, back to back (optimizer.hip_step on the gradients of the last
    step: the launches of azg_pv_train_apply, where the average is kept; the weights are put
    back afterwards),
  * the engine's kernel classes inside the step (azg_pv_profile_*: hipEvent brackets, in
    windows of their own because the events cost time; "train_other" holds the apply).
The expected cost is the Adam pass's extra load and store: 8 B per parameter.

    python scripts/bench_ema.py [--steps 50] [--warmup 10] [--rounds 5] [--out profiles/ema_bench.md]

Writes the table to --out and prints one JSON line; every window is in both, so the
run-to-run spread is next to each difference.
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
    ap.add_argument("--rounds", type=int, default=5, help="alternating timed windows per model (>= 5)")
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ema_bench.md"))
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("--rounds must be at least 5")
    import bench
    from network import PyTorchModel
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

    def select(name):                                     # outside every timed region
        torch.cuda.synchronize()
        if name == "on":
            m.enable_ema(args.decay)
        else:
            m.disable_ema()

    step = lambda: m.train_batch_device(x, pi, z, return_tensor=True)

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

    def class_window():
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        eng.profile_enable(True)
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        prof = eng.profile_read()
        eng.profile_enable(False)
        return {k: v[0] / args.steps for k, v in prof.items()}

    names = ("off", "on")
    keys = ["step_ms", "apply_ms"]
    w = {(k, n): [] for k in keys for n in names}
    for _ in range(args.rounds):
        for n in names:
            select(n)
            w[("step_ms", n)].append(timed(step))
            assert eng.train_skips() == 0
            if n == "on":
                torch.cuda.synchronize()
                assert not torch.equal(eng.flat_ema, eng.flat_params)   # the average was kept
        # the apply alone repeats one gradient: keep the weights it would walk away with out of the model
        opt = m.optimizer
        keep = [t.clone() for t in (eng.flat_params, opt.flat_exp_avg, opt.flat_exp_avg_sq)], opt.get_step()
        for n in names:
            select(n)
            w[("apply_ms", n)].append(timed(lambda: opt.hip_step(m.max_grad_norm)))
        torch.cuda.synchronize()
        with torch.no_grad():
            for t, saved in zip((eng.flat_params, opt.flat_exp_avg, opt.flat_exp_avg_sq), keep[0]):
                t.copy_(saved)
        opt.set_step(keep[1])
        eng.mark_dirty()
        for n in names:
            select(n)
            for cls, ms in class_window().items():
                w.setdefault((f"class_{cls}_ms", n), []).append(ms)
    keys += sorted({k for k, _ in w} - set(keys))
    select("off")
    med = lambda v: float(np.median(v))
    nparam = eng.nparam
    out = {"net": "6x128 pretrained", "batch": B, "params": nparam, "decay": args.decay, "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds, "extra_bytes_per_step": 8 * (nparam + eng.nbn)}
    rows = []
    for k in keys:
        off, on = w[(k, "off")], w[(k, "on")]
        out[k] = {"off": round(med(off), 4), "on": round(med(on), 4), "off_windows": [round(v, 4) for v in off],
                  "on_windows": [round(v, 4) for v in on], "on_minus_off": round(med(on) - med(off), 4),
                  "off_range": round(max(off) - min(off), 4), "on_range": round(max(on) - min(on), 4)}
        rows.append((k, out[k]))
    print(json.dumps(out))
    label = {"step_ms": "whole train step", "apply_ms": "clip + Adam + repack alone, back to back"}
    fmt = lambda v: ", ".join(f"{t:.4f}" for t in v)
    lines = ["# The weight average (EMA) in the train step (scripts/bench_ema.py)", "",
             f"MI355X, 6x128 pretrained ({nparam} parameters), B = {B}, pipelined steps, decay {args.decay}; one model "
             f"with the average bound and unbound in alternating windows; median of {args.rounds} windows of {args.steps} steps after "
             f"{args.warmup} warm-ups; hipEvent time per step.  The average adds "
             f"{8 * (nparam + eng.nbn) / 1e6:.2f} MB of traffic per step (8 B per parameter and running stat).", "",
             "| measured | EMA off (ms) | EMA on (ms) | on - off (ms) | off windows (ms) | on windows (ms) |",
             "|---|---|---|---|---|---|"]
    for k, r in rows:
        lines.append(f"| {label.get(k, k[6:-3] + ' kernels inside the step (event brackets)')} | {r['off']:.4f} | {r['on']:.4f} | {r['on_minus_off']:+.4f} | "
                     f"{fmt(r['off_windows'])} | {fmt(r['on_windows'])} |")
    d = os.path.dirname(args.out)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
