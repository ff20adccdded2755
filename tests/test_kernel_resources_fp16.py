"""Register / scratch budgets of the one-product fp16 board16 tower, read from the built
code object (no GPU needed; tests/test_kernel_resources.py's reader).

board16_tower<0, false, 1> (one workgroup per board) keeps 12 waves per CU: <= 168 VGPRs +
AGPRs, and no more scratch than the exact form's budget; board16_tower<0, true, 1> (the
small-batch split form) has none.  Built figures:
168 VGPRs / 36 B (none of it in the K loop) and 144 VGPRs / 0 B."""
import re

from test_kernel_resources import SCRATCH_BUDGET, _kernels

ONE_WG = r"board16_towerILi0ELb0ELi1EE"
SPLIT = r"board16_towerILi0ELb1ELi1EE"


def _one(ks, pat):
    hits = [n for n in ks if re.search(pat, n)]
    assert len(hits) == 1, (pat, hits)
    return ks[hits[0]]


def test_fp16_tower_occupancy_and_scratch():
    ks = _kernels()
    exact_budget = dict(SCRATCH_BUDGET)[r"board16_towerILi0ELb0E"]
    k = _one(ks, ONE_WG)
    assert k.get("vgpr_count", 0) + k.get("agpr_count", 0) <= 168, k
    assert k.get("private_segment_fixed_size", 0) <= exact_budget, k


def test_fp16_split_tower_has_no_scratch():
    k = _one(_kernels(), SPLIT)
    assert k.get("private_segment_fixed_size", 0) == 0, k
    assert k.get("vgpr_count", 0) + k.get("agpr_count", 0) <= 168, k   # 8 waves: two per SIMD would allow 256
