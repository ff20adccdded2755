"""Policy loss weights in the device replay ring (DeviceReplayBuffer.add_positions(...,
policy_weight=), sample(..., with_policy_weight=True), azg_pv_replay_gather_weight).  A ring
of 5 positions (capacity 40 images) takes 3 positions, then 4, so it wraps; the gather is a
copy, so every comparison is exact against a host model of the ring (a list, oldest first)."""
import random

import numpy as np
import pytest
import torch

from conftest import has_gpu
from test_gpu_replay import _positions

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

DEV = "cuda:0"
CAP_POS = 5


@pytest.fixture(scope="module")
def positions():
    return _positions(7, seed=211)


def _ring(positions, first_w, second_w):
    """The buffer after add 3, then 4, and the host model [(example, weight)] oldest first."""
    from replay import DeviceReplayBuffer
    dev = DeviceReplayBuffer(8 * CAP_POS, DEV)
    model = []
    for chunk, w in ((positions[:3], first_w), (positions[3:7], second_w)):
        dev.add_positions(chunk, policy_weight=w)
        model += list(zip(chunk, [1.0] * len(chunk) if w is None else list(w)))
        model = model[-CAP_POS:]
    return dev, model


def _all_ids():
    rng = np.random.default_rng(5)
    return np.concatenate([rng.permutation(8 * CAP_POS), rng.integers(0, 8 * CAP_POS, size=300)])


@pytest.mark.parametrize("first_w,second_w", [((0.0, 1.0, 0.25), (3.0, 0.0, 1.0, 0.5)),
                                              (None, (3.0, 0.0, 1.0, 0.5)),      # weights arrive late: old ones count 1.0
                                              ((0.0, 2.0, 0.25), None)])         # added without: 1.0, evicting old weights
def test_every_image_id_returns_its_positions_weight(positions, first_w, second_w):
    dev, model = _ring(positions, first_w, second_w)
    assert dev.count == CAP_POS and dev.head == 2 and dev._pw is not None and dev._pw.shape == (CAP_POS,)
    ids = _all_ids()     # 340 ids: more than one 256-thread workgroup of the weight gather
    s, p, z, w = dev.sample(len(ids), ids=ids.tolist(), with_policy_weight=True)
    assert w.shape == (len(ids),) and w.dtype == torch.float32 and w.is_cuda
    want = np.array([model[i // 8][1] for i in ids], dtype=np.float32)
    assert np.array_equal(w.cpu().numpy(), want)
    assert np.array_equal(z.cpu().numpy().reshape(-1), np.array([model[i // 8][0][2] for i in ids], np.float32))
    assert np.array_equal(dev.get_policy_weights(), np.array([mw for _, mw in model], np.float32))
    # the three tensors do not depend on the flag
    s2, p2, z2 = dev.sample(len(ids), ids=ids.tolist())
    assert torch.equal(s, s2) and torch.equal(p, p2) and torch.equal(z, z2)


def test_buffer_without_weights_returns_ones_and_allocates_nothing(positions):
    dev, model = _ring(positions, None, None)
    ids = _all_ids()
    s, p, z, w = dev.sample(len(ids), ids=ids.tolist(), with_policy_weight=True)
    assert torch.equal(w, torch.ones(len(ids), device=w.device))
    assert dev._pw is None and dev._wq is None
    assert np.array_equal(dev.get_policy_weights(), np.ones(CAP_POS, np.float32))
    s4, p4, z4, w4 = dev.sample_weighted(16, with_policy_weight=True)
    assert torch.equal(w4, torch.ones(16, device=w.device)) and dev._pw is None


def test_set_get_round_trip_and_validation(positions):
    dev, _ = _ring(positions, None, None)
    w = np.array([0.0, 0.5, 1.0, 7.25, 1e-3], np.float32)
    dev.set_policy_weights(w)
    assert np.array_equal(dev.get_policy_weights(), w)
    assert np.array_equal(dev._pw.cpu().numpy(), np.roll(w, dev.head))      # by slot: ring order starts at head
    s, p, z, got = dev.sample(40, ids=list(range(40)), with_policy_weight=True)
    assert np.array_equal(got.cpu().numpy(), np.repeat(w, 8))
    for bad in (w[:4], [np.nan] * 5, [-1.0] * 5, [np.inf] * 5):
        with pytest.raises(ValueError):
            dev.set_policy_weights(bad)
        with pytest.raises(ValueError):
            dev.add_positions(positions[:5], policy_weight=bad)
    assert np.array_equal(dev.get_policy_weights(), w) and dev.count == CAP_POS


def test_sample_without_the_flag_and_to_host_are_unchanged(positions):
    """sample() and sample_weighted() without the flag return the three tensors a buffer that
    never saw policy weights returns, bitwise, and to_host() is the same 3-tuples."""
    with_w, _ = _ring(positions, (0.0, 1.0, 0.25), (3.0, 0.0, 1.0, 0.5))
    plain, _ = _ring(positions, None, None)
    for seed in (1, 2):
        random.seed(seed)
        a = with_w.sample(24)
        random.seed(seed)
        b = plain.sample(24)
        assert len(a) == len(b) == 3 and all(torch.equal(u, v) for u, v in zip(a, b))
        random.seed(seed)
        a = with_w.sample_weighted(24)
        random.seed(seed)
        b = plain.sample_weighted(24)
        assert len(a) == len(b) == 3 and all(torch.equal(u, v) for u, v in zip(a, b))
        random.seed(seed)
        c = with_w.sample_weighted(24, with_policy_weight=True)
        assert len(c) == 4 and all(torch.equal(u, v) for u, v in zip(a, c))
    ha, hb = list(with_w.to_host().buffer), list(plain.to_host().buffer)
    assert len(ha) == len(hb) == 40
    for ea, eb in zip(ha, hb):
        assert len(ea) == len(eb) == 3
        assert np.array_equal(ea[0], eb[0]) and np.array_equal(ea[1], eb[1]) and ea[2] == eb[2]

