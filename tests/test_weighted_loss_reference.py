"""The float64 reference of the weighted train loss (tests/weighted_loss_reference.py) checked
on the CPU: against plain autograd of the same loss through the net's real ReLUs, and against
oracle.ref_net.masked_grads_fp64 (the unweighted reference) at weights of one."""
import numpy as np
import torch

import conftest  # noqa: F401  (paths)
from oracle.boards import encode_batch, synth_positions, synth_targets
from oracle.ref_net import RefModel, RefNet, load_numpy_state, masked_grads_fp64, state_to_numpy
from weighted_loss_reference import (own_masks_fp64, seeded_weights, weighted_loss,
                                     weighted_masked_grads_fp64)

BLOCKS, CH, B = 1, 64, 5


def _case():
    torch.manual_seed(11)
    st = state_to_numpy(RefModel(BLOCKS, CH).net)
    b, p = synth_positions(B, seed=3)
    x = encode_batch(b, p)
    pi, z = synth_targets(B, seed=4)
    return st, x, pi, z


def test_helper_matches_plain_autograd():
    """With the float64 net's own masks the masked forward IS the plain forward, so the
    helper's gradients are those of autograd through real ReLUs: float64 rounding apart."""
    st, x, pi, z = _case()
    wp, wv = seeded_weights(B, 5)
    assert wp[0] == 0 and wv[0] == 0 and set(wp) == set(wv) == {0.0, 0.25, 1.0, 3.0}
    got, (pl, vl) = weighted_masked_grads_fp64(st, BLOCKS, CH, x, pi, z, own_masks_fp64(st, BLOCKS, CH, x), wp, wv)
    net = RefNet(BLOCKS, CH).double()
    load_numpy_state(net, st)
    net.train()
    logits, value = net(torch.as_tensor(x, dtype=torch.float64))
    pl2, vl2 = weighted_loss(logits, value, pi, z, wp, wv)
    (pl2 + vl2).backward()
    np.testing.assert_allclose([pl, vl], [float(pl2.detach()), float(vl2.detach())], rtol=1e-13)
    for n, q in net.named_parameters():
        w = q.grad.numpy()
        assert np.abs(got[n] - w).max() <= 1e-12 * np.abs(w).max() + 1e-300, n
    # the loss by hand, per board, in numpy
    lg = logits.detach().numpy()
    lp = lg - lg.max(1, keepdims=True)
    lp = lp - np.log(np.exp(lp).sum(1, keepdims=True))
    t = pi.astype(np.float64)
    kl = np.where(t > 0, t * (np.log(np.where(t > 0, t, 1.0)) - lp), 0.0).sum(1)
    sq = (value.detach().numpy().reshape(-1) - z.reshape(-1).astype(np.float64)) ** 2
    np.testing.assert_allclose([pl, vl], [(wp * kl).sum() / B, (wv * sq).sum() / B], rtol=1e-12)


def test_helper_at_ones_is_the_unweighted_reference():
    st, x, pi, z = _case()
    mk = own_masks_fp64(st, BLOCKS, CH, x)
    want, (pl, vl) = masked_grads_fp64(st, BLOCKS, CH, x, pi, z, mk)
    ones = np.ones(B, np.float32)
    for wp, wv in ((None, None), (ones, ones), (ones, None), (None, ones)):
        got, (pl2, vl2) = weighted_masked_grads_fp64(st, BLOCKS, CH, x, pi, z, mk, wp, wv)
        np.testing.assert_allclose([pl2, vl2], [pl, vl], rtol=1e-13)
        for n, w in want.items():
            assert np.abs(got[n] - w).max() <= 1e-12 * np.abs(w).max() + 1e-300, n


def test_zero_weight_takes_a_board_out_of_its_head_only():
    """A board with policy weight 0 contributes nothing to the policy loss, yet still moves
    the gradients' BN statistics: the weighted loss is NOT the loss of the smaller batch."""
    st, x, pi, z = _case()
    mk = own_masks_fp64(st, BLOCKS, CH, x)
    wp = np.array([0, 1, 1, 1, 1], np.float32)
    _, (pl, vl) = weighted_masked_grads_fp64(st, BLOCKS, CH, x, pi, z, mk, wp, None)
    _, (pl1, vl1) = weighted_masked_grads_fp64(st, BLOCKS, CH, x, pi, z, mk, None, None)
    assert pl < pl1 and vl == vl1
