"""The numbering of eval launches through the C-ABI (azg_pv_last_seq, azg_pv_status,
azg_pv_posted, azg_pv_recover, azg_pv_clear_status) over more forwards than the status
rings have slots, so every slot and launch record is reused.  Nothing is provoked: no wait
bound is lowered and no overflow forced, so no launch is ever posted.

A 1x128 net under the default tuning keys runs the board16 tower, where every forward is
numbered; batch 2 runs its split form."""
import numpy as np
import pytest
import torch

from conftest import has_gpu
from oracle.boards import synth_positions
from test_gpu_forward import make_model

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

FORWARDS = 300   # > kTowerRing = 256 (csrc/pv_posted.h)


def test_launch_numbers_over_more_forwards_than_ring_slots():
    import _native
    lib = _native.load_library()
    m = make_model(1, 128, seed=17)
    eng = m.engine
    dev = eng.device
    boards, players = synth_positions(2, seed=171)
    b = torch.from_numpy(np.ascontiguousarray(boards, np.int8).reshape(2, 225)).to(dev)
    pl = torch.from_numpy(np.ascontiguousarray(players, np.int8).reshape(-1)).to(dev)
    probs = torch.empty((2, 225), dtype=torch.float32, device=dev)
    values = torch.empty((2, 1), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev)
    first, prev = None, None
    for i in range(FORWARDS):
        eng.forward_boards_into(b, pl, probs, values)
        stream.synchronize()
        seq = eng.last_seq()
        assert seq != 0
        if prev is not None:
            assert seq == prev + 1, (i, prev, seq)
        prev = seq
        assert lib.azg_pv_status(eng.h) == 0 and lib.azg_pv_posted(eng.h, seq) == 0, (i, seq)
        if i == 0:
            first = (probs.cpu().numpy().copy(), values.cpu().numpy().copy())
    # an unposted launch: nothing to recover, and the numbering does not move
    assert eng.recover(prev) is False
    assert eng.last_seq() == prev
    stream.synchronize()
    assert np.array_equal(probs.cpu().numpy(), first[0]) and np.array_equal(values.cpu().numpy(), first[1])
    assert np.isfinite(first[0]).all() and abs(float(first[0].sum()) - 2.0) < 1e-3
    eng.clear_status()
    assert eng.train_skips() == 0
    assert lib.azg_pv_status(eng.h) == 0
