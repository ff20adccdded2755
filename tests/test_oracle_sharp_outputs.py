"""The peaked-policy nets of tests/test_gpu_sharp_outputs.py are fair cases (CPU only).

Every other parity net of the suite has a nearly uniform policy (largest probability of a
row about 0.04), where dp_i = p_i (dl_i - sum_j p_j dl_j) lets a logit error of 1e-3 pass
the absolute 1e-5 bar on probabilities.  oracle.value_range.sharp_net multiplies policy_fc
by 2^k (k in SHARP); these are the conditions the reference alone must meet, on exactly the
nets and board sets of the GPU test, for the unchanged 1e-5 bar to be fair there:

  * the fp32 logits at k are bitwise 2^k x the logits at 0 (so are the fp64 ones);
  * at least half of the rows of every board set have a probability in (0.1, 0.9);
  * |cpu32 - fp64| <= 5e-6 on probs and values;
  * the rows exempt from the argmax check (fp64 masked top-2 gap below 2e-5) are at most
    2 % of a board set (at most one row of a set smaller than 50);
  * the emulated split-fp16 arithmetic (split_forward with act_exponents; a design aid, not a
    GPU reference) stays within 1e-5 of fp64: the bar is reachable."""
import numpy as np
import pytest

from oracle.value_range import (ARGMAX_GAP, SHARP, SHARP_BOARDS, SHARP_PREFIXES, act_exponents, sharp_case, sharp_net,
                                split_forward)

FAIR = 5e-6
TOL = 1e-5


def test_sharp_constants():
    assert SHARP == (2, 3) and ARGMAX_GAP == 2 * TOL
    assert set(SHARP_BOARDS) == set(SHARP_PREFIXES)
    for shape, (n, _) in SHARP_BOARDS.items():
        assert max(SHARP_PREFIXES[shape]) == n


@pytest.mark.parametrize("blocks,ch", sorted(SHARP_BOARDS))
def test_only_policy_fc_changes_and_logits_scale_bitwise(blocks, ch):
    c0 = sharp_case(blocks, ch, 0)
    for k in SHARP:
        c = sharp_case(blocks, ch, k)
        f = np.float32(2.0 ** k)
        for name, w in c["state"].items():
            w0 = c0["state"][name]
            if name.startswith("policy_fc."):
                assert np.array_equal(w, w0 * f), name
            else:
                assert np.array_equal(w, w0), name
        assert np.array_equal(c["x"], c0["x"])
        assert c["l32"].dtype == np.float32 and np.array_equal(c["l32"], c0["l32"] * f)
        assert c["l64"].dtype == np.float64 and np.array_equal(c["l64"], c0["l64"] * 2.0 ** k)
        assert np.array_equal(c["v32"], c0["v32"]) and np.array_equal(c["v64"], c0["v64"])


def test_sharp_net_is_sharp_case_state():
    ref = sharp_net(2, 64, 3)
    st = sharp_case(2, 64, 3)["state"]
    for name, w in ref.net.state_dict().items():
        assert np.array_equal(w.numpy(), st[name]), name


@pytest.mark.parametrize("k", SHARP)
@pytest.mark.parametrize("blocks,ch", sorted(SHARP_BOARDS))
def test_sharp_cases_are_fair(blocks, ch, k):
    c = sharp_case(blocks, ch, k)
    pe, ve = split_forward(c["state"], c["x"], act_exponents(c["state"]))
    dev = lambda a, r: float(np.abs(a - r).max())
    top = c["p64"].max(axis=1)
    mid = ((c["p64"] > 0.1) & (c["p64"] < 0.9)).any(axis=1)
    for B in SHARP_PREFIXES[(blocks, ch)]:
        d32 = (dev(c["p32"][:B], c["p64"][:B]), dev(c["v32"][:B], c["v64"][:B]))
        dsp = (dev(pe[:B], c["p64"][:B]), dev(ve[:B], c["v64"][:B]))
        exempt = int(c["exempt"][:B].sum())
        print(f"{blocks}x{ch} k={k} B={B}: top-p q10/median/q90 {np.quantile(top[:B], [0.1, 0.5, 0.9]).round(3).tolist()} "
              f"rows with a p in (0.1, 0.9) {mid[:B].mean():.2f} exempt rows {exempt} | |cpu32-fp64| probs {d32[0]:.2e} "
              f"values {d32[1]:.2e} logits {dev(c['l32'][:B], c['l64'][:B]):.2e} | emulated split probs {dsp[0]:.2e} "
              f"values {dsp[1]:.2e}")
        assert mid[:B].mean() >= 0.5
        assert max(d32) <= FAIR, d32
        assert exempt <= (1 if B < 50 else int(0.02 * B)), (exempt, B)
        assert max(dsp) <= TOL, dsp
