"""Device time of the board16 tower per forward (hipEvent brackets, best of 4 x 10 forwards,
6x128 pretrained, key 19 = 2) at B = 512 and 3456, for the library AZG_PV_LIB names: one
library per process, so two builds are compared by alternating processes on one box.

    AZG_PV_LIB=/path/to/libazg_pv.so python scripts/board16_time.py [--abl N]
--abl N sets the study build's board ablation bits (key 51; 8: fixed A rows) for the timed
forwards.  Prints one JSON line {batch: ms}.
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "alphazero-gomoku_amd")]

import torch  # noqa: E402


def main():
    import _native
    import bench
    from network import PyTorchModel
    from synth import synth_encoded
    lib = _native.load_library()
    abl = int(sys.argv[sys.argv.index("--abl") + 1]) if "--abl" in sys.argv else 0
    torch.manual_seed(0)
    m = PyTorchModel(board_size=15, device="cuda", n_res_blocks=6, channels=128)
    bench.pretrain(m, m.engine.device)
    eng = m.engine
    out = {}
    for B in (512, 3456):
        x = torch.from_numpy(synth_encoded(B, seed=B)).cuda()
        for _ in range(3):
            eng.forward(x)
        torch.cuda.synchronize()
        if abl:
            lib.azg_pv_set_tuning(51, abl)
        best = 1e30
        for _ in range(4):
            eng.profile_enable(True)
            for _ in range(10):
                eng.forward(x)
            prof = eng.profile_read()
            eng.profile_enable(False)
            best = min(best, prof["board16"][0] / 10)
        if abl:
            lib.azg_pv_set_tuning(51, 0)
        out[B] = round(best, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
