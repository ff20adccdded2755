"""Train-step time with the batch's data path included: the host replay buffer
(ReplayBuffer.sample = random.sample + np.stack, then train_batch's three pageable
host-to-device copies) against the device-resident one (DeviceReplayBuffer.sample =
one gather kernel, then train_batch_device), in one process, on the same 60,000
images of synthetic positions, 6x128, B = 128 (the reference's batch_size,
train.py:849-889).  `floor_ms_per_step` is the same synchronous step on one fixed
resident batch (bench.py's train leg), i.e. what no data path can beat.

    python scripts/bench_replay.py [--steps 300] [--warmup 20] [--rounds 3] [--images 60000]

Prints one JSON line.
"""
import argparse
import json
import os
import random
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "alphazero-gomoku_amd")]

import numpy as np
import torch


def _timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternating timed windows per path (medians are reported)")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--images", type=int, default=60000, help="buffer size in images (a multiple of 8)")
    args = ap.parse_args()
    from network import PyTorchModel
    from replay import DeviceReplayBuffer
    from synth import synth_encoded

    B, n_pos = args.batch, args.images // 8
    rng = np.random.default_rng(0)
    states = synth_encoded(n_pos, seed=11)
    pi = rng.random((n_pos, 225)).astype(np.float32)
    pi /= pi.sum(1, keepdims=True)
    z = rng.integers(-1, 2, n_pos).astype(np.float32)
    dev = DeviceReplayBuffer(args.images, "cuda", symmetries=True)
    dev.add_positions([(states[i], pi[i], float(z[i])) for i in range(n_pos)])
    host = dev.to_host()                  # the same images as the deque of tuples the loop holds
    assert len(host) == len(dev) == args.images

    def model():
        torch.manual_seed(0)
        return PyTorchModel(device="cuda", n_res_blocks=args.blocks, channels=args.channels)

    m_host, m_dev, m_floor = model(), model(), model()
    fixed = dev.sample(B)
    # the three paths alternate over `rounds` windows of `steps` steps (the spread between
    # windows is printed); both buffer paths draw under one random state, so the two
    # models see the same batches
    r_host, r_dev = random.Random(1).getstate(), random.Random(1).getstate()
    floors, hosts, devs = [], [], []
    for _ in range(args.rounds):
        floors.append(_timed(lambda: m_floor.train_batch_device(*fixed), args.steps, args.warmup))
        random.setstate(r_host)
        hosts.append(_timed(lambda: m_host.train_batch(*host.sample(B)), args.steps, args.warmup))
        r_host = random.getstate()
        random.setstate(r_dev)
        devs.append(_timed(lambda: m_dev.train_batch_device(*dev.sample(B)), args.steps, args.warmup))
        r_dev = random.getstate()
    floor, t_host, t_dev = (float(np.median(v)) for v in (floors, hosts, devs))
    # the data paths alone (the device one synchronised per batch, so it is the gather's
    # latency, not its enqueue time)
    s_host = _timed(lambda: host.sample(B), args.steps, args.warmup)

    def dev_sample_sync():
        dev.sample(B)
        torch.cuda.synchronize()

    s_dev = _timed(dev_sample_sync, args.steps, args.warmup)
    s_dev_enq = _timed(lambda: dev.sample(B), args.steps, args.warmup)
    same = all(torch.equal(a, b) for a, b in zip(m_host.net.state_dict().values(), m_dev.net.state_dict().values()))
    print(json.dumps({
        "net": f"{args.blocks}x{args.channels}", "batch": B, "steps": args.steps, "warmup": args.warmup,
        "buffer_images": args.images, "buffer_positions": n_pos,
        "host_path_ms_per_step": round(t_host, 3), "device_path_ms_per_step": round(t_dev, 3),
        "floor_ms_per_step": round(floor, 3), "rounds": args.rounds,
        "host_path_rounds": [round(v, 3) for v in hosts], "device_path_rounds": [round(v, 3) for v in devs],
        "floor_rounds": [round(v, 3) for v in floors],
        "host_over_floor_ms": round(t_host - floor, 3), "device_over_floor_ms": round(t_dev - floor, 3),
        "speedup_device_vs_host": round(t_host / t_dev, 3),
        "host_sample_ms": round(s_host, 3), "device_sample_sync_ms": round(s_dev, 3),
        "device_sample_enqueue_ms": round(s_dev_enq, 3),
        "device_buffer_mb": round(n_pos * 1129 / 1e6, 2), "host_buffer_mb": round(args.images * 3604 / 1e6, 2),
        "models_bitwise_equal": bool(same)}))


if __name__ == "__main__":
    main()
