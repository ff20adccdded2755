"""The fp64 restatement of the score record (tests/score_reference.py) against torch's own
loss functions -- nn.KLDivLoss(reduction="batchmean") on F.log_softmax and nn.MSELoss, the
reference's calls (network.py:162-163,216-219) -- and engine.score_summary on hand-made
sums.  No GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from score_reference import FIELDS, planted_case, score_records, summary_from_records


@pytest.mark.parametrize("B", [1, 5, 37])
def test_kl_and_sq_means_are_torchs_losses(B):
    l, v, t, z = planted_case(B, seed=B)
    rec = score_records(l, v, t, z)
    l64, t64 = torch.from_numpy(l).double(), torch.from_numpy(t).double()
    v64, z64 = torch.from_numpy(v).double().reshape(-1, 1), torch.from_numpy(z).double().reshape(-1, 1)
    pl = float(nn.KLDivLoss(reduction="batchmean")(F.log_softmax(l64, dim=1), t64))
    vl = float(nn.MSELoss()(v64, z64))
    s = summary_from_records(rec)
    np.testing.assert_allclose(s["policy_loss"], pl, rtol=1e-12, atol=0)
    np.testing.assert_allclose(s["value_loss"], vl, rtol=1e-12, atol=0)
    assert np.isfinite(rec).all()


def test_fields_on_the_planted_rows():
    l, v, t, z = planted_case(20, seed=3)
    rec = dict(zip(FIELDS, score_records(l, v, t, z).T))
    # one-hot target: KL = -lp at the target square, p_best = exp(lp) there, mass 1
    lp0 = F.log_softmax(torch.from_numpy(l[0]).double(), dim=0).numpy()
    assert rec["kl"][0] == pytest.approx(-lp0[137], rel=1e-12)
    assert rec["p_best"][0] == pytest.approx(math.exp(lp0[137]), rel=1e-12)
    assert rec["target_mass"][0] == 1.0
    # alternating +-80: 113 squares share the mass, the entropy is log(113)
    assert rec["entropy"][3] == pytest.approx(math.log(113), rel=1e-12)
    assert np.isfinite(rec["kl"][3])
    # equal maxima: both argmaxes are the lower index, 17
    assert rec["top1"][4] == 1.0 and np.argmax(l[4]) == 17 and np.argmax(t[4]) == 17
    # value fields over every (z, v) pair
    want_agree = (v.astype(np.float64) * z > 0).astype(np.float64)
    assert np.array_equal(rec["v_agree"], want_agree) and np.array_equal(rec["decided"], (z != 0).astype(np.float64))
    assert {(float(a), float(b)) for a, b in zip(z[:15], v[:15])} == {(a, b) for a in (-1.0, 0.0, 1.0)
                                                                    for b in map(float, np.float32([-1, 0, 1, .3, -.3]))}


def test_score_summary_on_hand_made_sums():
    from engine import SCORE_FIELDS, score_summary
    assert SCORE_FIELDS == FIELDS
    s = score_summary([8.0, 2.0, 12.0, 3.0, 1.0, 2.0, 3.0, 4.0], 4)
    assert s == {"policy_loss": 2.0, "value_loss": 0.5, "total_loss": 2.5, "policy_entropy": 3.0,
                 "policy_top1": 0.75, "target_move_prob": 0.25, "value_sign_agreement": 2.0 / 3.0,
                 "target_mass": 1.0, "n": 4}
    assert list(s)[:3] == ["policy_loss", "value_loss", "total_loss"]     # train_batch's keys first
    # no decided board (S6 = 0): the agreement is 0, not a division by zero
    s = score_summary(np.array([1.0, 1.0, 1.0, 0.0, 0.5, 0.0, 0.0, 2.0]), 2)
    assert s["value_sign_agreement"] == 0.0 and s["n"] == 2 and s["target_mass"] == 1.0
    # fp64 throughout: a sum fp32 cannot hold survives
    s = score_summary(torch.tensor([2.0 ** 30 + 1.0] + [0.0] * 7, dtype=torch.float64), 1)
    assert s["policy_loss"] == 2.0 ** 30 + 1.0
    assert summary_from_records(np.array([[8.0, 2.0, 12.0, 3.0, 1.0, 2.0, 3.0, 4.0]])) == score_summary(
        [8.0, 2.0, 12.0, 3.0, 1.0, 2.0, 3.0, 4.0], 1)
    for bad in ([1.0] * 7, [1.0] * 9):
        with pytest.raises(ValueError):
            score_summary(bad, 1)
    with pytest.raises(ValueError):
        score_summary([1.0] * 8, 0)
