"""Golden outputs of the 16x16x32 board tower (csrc/pv_board16.hip, EVAL_ARITH = 2, C = 128)
for tests/test_gpu_board16_rows.py: which LDS row a lane reads for every (pixel, tap) pair
decides every output on dense random input, so the recorded probs and values pin the
kernel's A-row addressing bitwise.

The fixture holds the inputs (300 int8 boards, the side to move), the weight seeds and the
probs / values of the 1- and 2-block nets for the 300-board batch.  It was recorded on an
MI355X from the PRODUCT library of the commit before the A-row offsets moved into an LDS
table; re-record it only from a library whose arithmetic is the intended one, never to make
a failing test pass:
  AZG_PV_LIB=/path/to/libazg_pv.so PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_board16.py
While recording, every launch form the test runs (3 boards split, one workgroup per board
through predict and predict_boards, 258 boards unsplit, 300 boards with the split tail) is
checked to give the recording library the same rows, so one array per net covers them all.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
for _p in (REPO, os.path.join(REPO, "alphazero-gomoku_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PATH = os.path.join(HERE, "board16_rows.npz")
CH = 128
BLOCKS = (1, 2)
N_BOARDS = 300
BOARD_SEED = 1605
WEIGHT_SEED = {1: 71, 2: 72}


def seeded_state(net, seed: int) -> dict:
    """Every tensor of the net's state from numpy's generator (the same on every machine):
    fp32 conv / linear weights (He scale, off the fp16 grid), BN with scales in 0.5..1.5,
    nonzero shifts, nonzero running means and running variances in 0.5..1.5."""
    import torch
    rng = np.random.RandomState(seed)
    out = {}
    for k, v in net.state_dict().items():
        shape = tuple(v.shape)
        if not v.dtype.is_floating_point:
            out[k] = v.clone()
            continue
        if k.endswith("running_var") or (k.endswith("weight") and len(shape) == 1):
            a = rng.uniform(0.5, 1.5, shape)
        elif k.endswith("running_mean") or k.endswith("bias"):
            a = rng.normal(0.0, 0.1, shape)
        else:
            fan_in = int(np.prod(shape[1:]))
            a = rng.normal(0.0, np.sqrt(2.0 / fan_in), shape)
        out[k] = torch.from_numpy(a.astype(np.float32))
    return out


def make_model(blocks: int):
    from network import PyTorchModel
    m = PyTorchModel(board_size=15, device="cuda", n_res_blocks=blocks, channels=CH)
    m.net.load_state_dict(seeded_state(m.net, WEIGHT_SEED[blocks]))
    m.net.eval()
    return m


def inputs():
    from oracle.boards import synth_positions
    boards, players = synth_positions(N_BOARDS, seed=BOARD_SEED)
    return np.asarray(boards, np.int8).reshape(N_BOARDS, 225), np.asarray(players, np.int8)


def forms(m, lib, boards, players):
    """(name, probs, values) of every launch form the test runs, rows in board order."""
    from _native import TUNE
    from oracle.boards import encode_batch
    x = encode_batch(boards.reshape(-1, 15, 15), players)
    out = [("split3", *m.predict(x[:3])), ("tail300", *m.predict(x))]
    prev = lib.azg_pv_set_tuning(TUNE.BOARD16_SPLIT_MAX, 0)
    try:
        out.append(("one3", *m.predict(x[:3])))
        out.append(("fused3", *m.predict_boards(boards[:3], players[:3], masked=False)))
        out.append(("unsplit258", *m.predict(x[:258])))
    finally:
        lib.azg_pv_set_tuning(TUNE.BOARD16_SPLIT_MAX, prev)
    return out


if __name__ == "__main__":
    import _native
    lib = _native.load_library()
    boards, players = inputs()
    data = {"boards": boards, "players": players, "board_seed": np.int64(BOARD_SEED),
            "weight_seeds": np.asarray([WEIGHT_SEED[b] for b in BLOCKS], np.int64),
            "blocks": np.asarray(BLOCKS, np.int64)}
    for blocks in BLOCKS:
        m = make_model(blocks)
        res = {name: (p, v) for name, p, v in forms(m, lib, boards, players)}
        p300, v300 = res["tail300"]
        assert p300.dtype == np.float32 and p300.shape == (N_BOARDS, 225) and np.isfinite(p300).all()
        for name, (p, v) in res.items():
            assert np.array_equal(p, p300[:len(p)]) and np.array_equal(v, v300[:len(v)]), (blocks, name)
        data[f"probs_{blocks}"] = p300
        data[f"values_{blocks}"] = v300
        print(f"{blocks} block(s): {len(res)} forms agree; probs max {p300.max():.4f}, values "
              f"{v300.min():.4f} .. {v300.max():.4f}")
    np.savez_compressed(PATH, **data)
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes")
