"""The 16x16x32 board tower (csrc/pv_board16.hip) reads its A fragments' LDS rows through a
per-workgroup table of (pixel, tap) row offsets.  On dense random input a wrong entry for
any of the 240 x 9 pairs changes an output, so every launch form is pinned bitwise to
tests/golden/board16_rows.npz: probs and values recorded from the product library of the
commit before the table (tests/golden/make_golden_board16.py, which also checked that all
these forms gave that library the same rows).

Nets: C = 128 with 1 and 2 blocks (the non-residual, residual-to-LDS and last-conv
epilogues), seeded fp32 weights off the fp16 grid, BN with nonzero shifts and non-unit
running statistics."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, has_gpu
from _native import TUNE
from oracle.boards import encode_batch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

_spec = importlib.util.spec_from_file_location("make_golden_board16", os.path.join(GOLDEN, "make_golden_board16.py"))
gold = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gold)


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(GOLDEN, "board16_rows.npz"), allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    assert tuple(g["blocks"]) == gold.BLOCKS and int(g["board_seed"]) == gold.BOARD_SEED
    assert [int(s) for s in g["weight_seeds"]] == [gold.WEIGHT_SEED[b] for b in gold.BLOCKS]
    boards, players = gold.inputs()   # the recorded inputs are the seeded ones
    assert np.array_equal(boards, g["boards"]) and np.array_equal(players, g["players"])
    g["x"] = encode_batch(g["boards"].reshape(-1, 15, 15), g["players"])
    return g


@pytest.fixture(scope="module")
def models():
    return {b: gold.make_model(b) for b in gold.BLOCKS}


@pytest.fixture(scope="module")
def lib():
    import _native
    return _native.load_library()


def check(got, g, blocks):
    probs, values = got
    n = len(probs)
    assert probs.dtype == np.float32 and probs.shape == (n, 225) and values.shape == (n, 1)
    assert np.array_equal(probs, g[f"probs_{blocks}"][:n])
    assert np.array_equal(values, g[f"values_{blocks}"][:n])


@pytest.mark.parametrize("blocks", gold.BLOCKS)
def test_three_boards_every_form_bitwise(fixture, models, lib, blocks):
    """B = 3: split over three workgroups per board (the default), one workgroup per board
    (key BOARD16_SPLIT_MAX = 0) through predict and through predict_boards (int8 boards, the
    heads' projections fused after the last conv): the fixture's rows, and each other's."""
    g, m = fixture, models[blocks]
    split = m.predict(g["x"][:3])
    prev = lib.azg_pv_set_tuning(TUNE.BOARD16_SPLIT_MAX, 0)
    try:
        one = m.predict(g["x"][:3])
        fused = m.predict_boards(g["boards"][:3], g["players"][:3], masked=False)
    finally:
        lib.azg_pv_set_tuning(TUNE.BOARD16_SPLIT_MAX, prev)
    for got in (split, one, fused):
        check(got, g, blocks)
    for got in (one, fused):
        assert np.array_equal(got[0], split[0]) and np.array_equal(got[1], split[1])


@pytest.mark.parametrize("blocks", gold.BLOCKS)
def test_258_boards_unsplit_bitwise(fixture, models, lib, blocks):
    """B = 258 with the split off: two workgroups take a second board in turn (the table and
    the zero rows outlive a board, the heads' fp32 rows included)."""
    g, m = fixture, models[blocks]
    prev = lib.azg_pv_set_tuning(TUNE.BOARD16_SPLIT_MAX, 0)
    try:
        got = m.predict(g["x"][:258])
    finally:
        lib.azg_pv_set_tuning(TUNE.BOARD16_SPLIT_MAX, prev)
    check(got, g, blocks)
    three = m.predict(g["x"][:3])
    assert np.array_equal(got[0][:3], three[0]) and np.array_equal(got[1][:3], three[1])


@pytest.mark.parametrize("blocks", gold.BLOCKS)
def test_300_boards_with_split_tail_bitwise(fixture, models, blocks):
    """B = 300 at the defaults: one full round one workgroup per board, then the tail launch
    (the last 44 boards split)."""
    g, m = fixture, models[blocks]
    got = m.predict(g["x"])
    check(got, g, blocks)
    three = m.predict(g["x"][:3])
    assert np.array_equal(got[0][:3], three[0]) and np.array_equal(got[1][:3], three[1])
