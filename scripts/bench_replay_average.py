"""Cost of position averaging in the device replay buffer (csrc/pv_replay_average.hip,
replay.DeviceReplayBuffer.set_target_averaging / refresh_averages), and how many duplicate
positions real self-play puts into the ring, in one process.

  duplicates    one iteration's self-play (--games games at --sims simulations on a fresh 6x128
                net, the loop's temperature and noise settings) added to a buffer:
                duplicate_stats() = positions, groups of equal boards, the largest group.
  refresh       the DEVICE time of one refresh_averages() at --count positions, and of its three
                parts alone (canonical keys; torch's stable sort; flags + averaging), for three
                rings: the self-play positions above, tiled to --count when there are fewer (the
                table says so: tiling makes every group count / positions times longer than
                self-play made it); all positions distinct; all positions the empty board (one
                group spans the ring: the longest walk there is).
  gather        sample(B) with averaging on and off on the first ring: the same launch on other
                pointers.
  yardsticks    what else runs once per buffer change at this size: azg_pv_replay_prefix, and
                scoring --fresh fresh positions (train._score_surprise, 6x128).
Device time is taken from hipEvents around every call, each window queued behind `--blocker`
large matmuls so that the brackets hold device work, not the host's enqueue time (see
scripts/bench_replay_weighted.py, whose window this is).  Medians of `rounds` windows; every
window is in the JSON line.  The refresh runs once per buffer change, not per batch.

    python scripts/bench_replay_average.py [--count 125000] [--games 64] [--sims 100]
        [--out profiles/replay_average_bench.md]

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


def _pi_z(n, rng):
    pi = rng.random((n, 225)).astype(np.float32)
    pi /= pi.sum(1, keepdims=True)
    return pi, rng.integers(-1, 2, n).astype(np.float32)


def _random_examples(n, seed):
    """n positions of 20..60 random stones: no two alike (the table shows groups == positions)."""
    rng = np.random.default_rng(seed)
    states = np.zeros((n, 3, 225), np.float32)
    states[:, 2] = 1.0
    for i in range(n):
        sq = rng.choice(225, size=int(rng.integers(20, 61)), replace=False)
        states[i, 0, sq[0::2]] = 1.0
        states[i, 1, sq[1::2]] = 1.0
    pi, z = _pi_z(n, rng)
    return [(states[i].reshape(3, 15, 15), pi[i], float(z[i])) for i in range(n)]


def _empty_examples(n, seed):
    rng = np.random.default_rng(seed)
    state = np.zeros((3, 15, 15), np.float32)
    state[2] = 1.0
    pi, z = _pi_z(n, rng)
    return [(state, pi[i], float(z[i])) for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=125000, help="positions in the timed rings")
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--max-moves", type=int, default=225)
    ap.add_argument("--steps", type=int, default=50, help="calls per window of the small calls")
    ap.add_argument("--refresh-steps", type=int, default=10, help="calls per window of the refresh and its parts")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per figure (medians are reported)")
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--fresh", type=int, default=4000, help="positions of the timed scoring")
    ap.add_argument("--blocker", type=int, default=8, help="8192^2 fp32 matmuls queued in front of every window")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "replay_average_bench.md"))
    args = ap.parse_args()
    import train
    from _native import check, ptr
    from games.gomoku import Gomoku
    from network import PyTorchModel
    from replay import DeviceReplayBuffer
    from selfplay import selfplay_games

    dev = torch.device("cuda:0")
    med = lambda v: float(np.median(v))
    r5 = lambda v: [round(x, 5) for x in v]

    blk_a = torch.randn((8192, 8192), dtype=torch.float32, device=dev)
    blk_c = torch.empty_like(blk_a)
    torch.mm(blk_a, blk_a, out=blk_c)
    torch.cuda.synchronize()
    queued = []   # per window: did the last call's enqueue end before the blocker did?

    def window(fn, steps):
        """Device ms per call over one window of `steps` calls."""
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        done = torch.cuda.Event()
        torch.cuda.synchronize()
        for _ in range(args.blocker):
            torch.mm(blk_a, blk_a, out=blk_c)
        done.record()
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        queued.append(not done.query())
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in ev) / steps

    def timed(fn, steps):
        for _ in range(args.warmup):
            fn()
        w = [window(fn, steps) for _ in range(args.rounds)]
        return {"device_ms": round(med(w), 5), "device_ms_windows": r5(w)}

    # ---- one iteration's real self-play
    torch.manual_seed(0)
    np.random.seed(0)
    model = PyTorchModel(board_size=15, device=str(dev), n_res_blocks=6, channels=128)
    t0 = time.perf_counter()
    real, winners, _ = selfplay_games(model, Gomoku, args.games, args.sims, 1.2, lambda n: max(0.0, 1.0 - n / 8),
                                      0.03, 0.25, 30, max_moves=args.max_moves, board_size=15, use_symmetries=False)
    t_sp = time.perf_counter() - t0
    one = DeviceReplayBuffer(8 * len(real), dev)
    one.set_target_averaging(True)
    one.add_positions(real)
    stats = one.duplicate_stats()
    sizes = one.get_group_sizes()
    out = {"selfplay": {"games": args.games, "sims": args.sims, "net": "6x128, fresh weights", "seconds": round(t_sp, 1),
                        "winners": {str(k): int(v) for k, v in winners.items()},
                        **stats, "groups_over_positions": round(stats["groups"] / stats["positions"], 4),
                        "positions_in_groups_of_2_or_more": int((sizes >= 2).sum())},
           "count": args.count, "steps": args.steps, "refresh_steps": args.refresh_steps, "rounds": args.rounds,
           "rings": {}}
    del one

    # ---- the three rings
    def fill(examples_of):
        buf = DeviceReplayBuffer(args.count * 8, dev)
        for lo in range(0, args.count, 25000):                     # bounded host staging
            buf.add_positions(examples_of(lo, min(25000, args.count - lo)))
        buf.set_target_averaging(True)
        return buf

    tiled = len(real) < args.count
    rings = {"selfplay": lambda lo, n: [real[(lo + i) % len(real)] for i in range(n)],
             "distinct": lambda lo, n: _random_examples(n, seed=100 + lo),
             "identical": lambda lo, n: _empty_examples(n, seed=200 + lo)}
    for name, examples_of in rings.items():
        buf = fill(examples_of)
        a_stats = buf.duplicate_stats()          # also the first refresh: everything is allocated
        a = buf._avg
        n, stream = buf.count, torch.cuda.current_stream(dev).cuda_stream
        keys_sorted, perm = torch.sort(a["keys"][:n], stable=True)

        def refresh():
            buf._avg_ok = False
            buf.refresh_averages()

        def keys():
            check(buf.lib.azg_pv_replay_canon_keys(ptr(buf.stones), buf.cap_pos, buf.head, n, buf.nsym, ptr(a["keys"]),
                                                   ptr(a["syms"]), stream), buf.lib)

        def sort():
            torch.sort(a["keys"][:n], stable=True)

        def average():
            check(buf.lib.azg_pv_replay_average(ptr(buf.stones), ptr(buf.pis), ptr(buf.zs), None, buf.cap_pos, buf.head,
                                                n, ptr(keys_sorted), ptr(perm), ptr(a["syms"]), ptr(a["pi_avg"]),
                                                ptr(a["z_avg"]), None, ptr(a["group_first"]), ptr(a["group_size"]),
                                                stream), buf.lib)

        res = {"stats": a_stats, "tiled_from": len(real) if name == "selfplay" and tiled else None}
        for k, fn in (("refresh", refresh), ("keys", keys), ("sort", sort), ("average", average)):
            res[k] = timed(fn, args.refresh_steps)
        if name == "selfplay":
            for B in args.batches:
                wins = {"on": [], "off": []}
                for on in (True, False):
                    buf.set_target_averaging(on)
                    for _ in range(args.warmup):
                        buf.sample(B)
                for _ in range(args.rounds):                       # the two settings alternate
                    for k, on in (("on", True), ("off", False)):
                        buf.set_target_averaging(on)
                        buf.refresh_averages()                      # outside the window
                        wins[k].append(window(lambda: buf.sample(B), args.steps))
                for k, w in wins.items():
                    res[f"sample_B{B}_averaging_{k}"] = {"device_ms": round(med(w), 5), "device_ms_windows": r5(w)}
            buf.sample_weighted(128)                               # gives the ring weights and a prefix array

            def prefix():
                check(buf.lib.azg_pv_replay_prefix(ptr(buf._wq), buf.cap_pos, buf.head, buf.count, ptr(buf._prefix),
                                                   stream), buf.lib)

            res["prefix"] = timed(prefix, args.steps)
        out["rings"][name] = res
        del buf, a, keys_sorted, perm
        torch.cuda.empty_cache()

    # ---- scoring an iteration's fresh positions (wall, synchronised: the sums go to the host)
    fresh = _random_examples(args.fresh, seed=5)
    train._score_surprise(model, fresh)
    t_score = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train._score_surprise(model, fresh)
        torch.cuda.synchronize()
        t_score.append((time.perf_counter() - t0) * 1e3)
    out["score"] = {"positions": args.fresh, "net": "6x128, exact", "wall_ms": round(med(t_score), 3),
                    "wall_ms_rounds": r5(t_score)}
    out["windows_fully_queued_behind_blocker"] = f"{sum(queued)} of {len(queued)}"
    print(json.dumps(out))

    sp = out["selfplay"]
    lines = ["# Position averaging in the device replay buffer (scripts/bench_replay_average.py)", "",
             "No effect of position averaging on playing strength has been measured; this file holds its cost and "
             "the share of duplicates in self-play data only.", "",
             "## Duplicates in one iteration's self-play", "",
             f"{sp['games']} games at {sp['sims']} simulations, {sp['net']} ({sp['seconds']:.0f} s of self-play): "
             f"{sp['positions']} positions in {sp['groups']} groups of equal boards up to symmetry "
             f"(groups / positions = {sp['groups_over_positions']:.4f}); the largest group has {sp['largest']} "
             f"positions; {sp['positions_in_groups_of_2_or_more']} positions share their board with another.", "",
             f"## One refresh at {args.count} positions", "",
             f"MI355X, nsym = 8, no policy weights; device ms from hipEvents around each call, median of {args.rounds} "
             f"windows of {args.refresh_steps} calls after {args.warmup} warm-ups, every window queued behind large "
             f"matmuls ({out['windows_fully_queued_behind_blocker']} windows were enqueued entirely before the "
             "matmuls ended).  refresh = keys + sort + average as refresh_averages() runs them; the parts were also "
             "timed alone.", "",
             "| ring | groups | largest | refresh (ms) | keys (ms) | sort (ms) | flags + average (ms) | refresh windows (ms) |",
             "|---|---|---|---|---|---|---|---|"]
    names = {"selfplay": "self-play" + (f" ({len(real)} positions tiled to {args.count})" if tiled else ""),
             "distinct": "all distinct", "identical": "all the empty board"}
    for name, r in out["rings"].items():
        lines.append(f"| {names[name]} | {r['stats']['groups']} | {r['stats']['largest']} | "
                     f"{r['refresh']['device_ms']:.4f} | {r['keys']['device_ms']:.4f} | {r['sort']['device_ms']:.4f} | "
                     f"{r['average']['device_ms']:.4f} | "
                     f"{', '.join(f'{v:.4f}' for v in r['refresh']['device_ms_windows'])} |")
    if tiled:
        lines += ["", f"The self-play ring is the {len(real)} positions above repeated until {args.count} are held, so "
                  f"each of its groups is about {args.count // len(real)} times as long as self-play made it."]
    r = out["rings"]["selfplay"]
    lines += ["", "## Beside it", "",
              f"Per batch, sample(B) on the self-play ring (device ms, median of {args.rounds} windows of {args.steps} "
              "calls, the two settings alternating):", "", "| call | averaging on | averaging off |", "|---|---|---|"]
    for B in args.batches:
        lines.append(f"| sample({B}) | {r[f'sample_B{B}_averaging_on']['device_ms']:.4f} | "
                     f"{r[f'sample_B{B}_averaging_off']['device_ms']:.4f} |")
    lines += ["", f"Once per buffer change at the same size: azg_pv_replay_prefix {r['prefix']['device_ms']:.4f} ms "
              f"(device); scoring {out['score']['positions']} fresh positions ({out['score']['net']}) "
              f"{out['score']['wall_ms']:.2f} ms (wall, synchronised, median of {args.rounds})."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
