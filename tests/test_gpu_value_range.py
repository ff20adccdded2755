"""The eval forward at the low end of the activation range.

The split-fp16 convs (EVAL_ARITH 1 and 2) stage every activation as hi = fp16(x),
lo = fp16(x - hi); below |x| ~ 2^-3 lo is subnormal and carries a fixed 2^-25 error that
the next BN scales back to O(1).  The nets here have BN gammas (and betas) scaled by 2^-k
on the stem, on every bn1, or on everything the trunk sums, then calibrated running
stats: the fp32 oracle stays within 5e-6 of fp64 on all of them
(tests/test_oracle_value_range.py), so they are fair cases for the 1e-5 bar.  Every eval
form that splits runs each net; the fp32 forward (EVAL_ARITH 0) runs beside it.

Gates, against the fp64 RefModel on the same weights (probs and values):
  * every form: |gpu - fp64| <= max(1e-5, 2 |cpu32 - fp64|) (test_forward_matches_oracle's);
  * split forms: also |split - fp32 GPU| <= 1e-5 (test_h3_matches_fp32_forward_and_oracle's);
  * masked-policy argmax; no overflow recompute (h3_overflows == 0) and status 0."""
import functools

import numpy as np
import pytest
import torch

from conftest import has_gpu
from _native import TUNE
from oracle.boards import encode_batch, synth_positions, valid_mask
from oracle.ref_net import state_to_numpy
from oracle.value_range import CASES, as_fp64, low_range_net

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

TOL = 1e-5
NBOARDS = {(2, 128): 258, (1, 256): 20}

# (name, channels, batch, input path, tuning keys, profile class that must have run)
K = TUNE
FORMS = (
    ("board16 B=3 split", 128, 3, "planes", {K.EVAL_ARITH: 2}, "board16"),
    ("board16 B=3 one workgroup", 128, 3, "planes", {K.EVAL_ARITH: 2, K.BOARD16_SPLIT_MAX: 0}, "board16"),
    ("board16 B=3 boards split", 128, 3, "boards", {K.EVAL_ARITH: 2}, "board16"),
    ("board16 B=3 boards fused heads", 128, 3, "boards", {K.EVAL_ARITH: 2, K.BOARD16_SPLIT_MAX: 0}, "board16"),
    ("board16 B=258 one workgroup", 128, 258, "planes", {K.EVAL_ARITH: 2, K.BOARD16_SPLIT_MAX: 0}, "board16"),
    ("tower 64x64 B=37", 128, 37, "planes", {K.EVAL_ARITH: 1, K.TOWER_MODE: 1, K.TOWER_SHAPE: 5}, "tower"),
    ("tower 128x64 B=37", 128, 37, "planes", {K.EVAL_ARITH: 1, K.TOWER_MODE: 1, K.TOWER_SHAPE: 8}, "tower"),
    ("per layer B=37", 128, 37, "planes", {K.EVAL_ARITH: 1, K.TOWER_MODE: 0}, "conv3x3"),
    ("h3_tile B=20", 256, 20, "planes", {K.EVAL_ARITH: 1, K.TOWER_MODE: 1, K.TOWER_SHAPE: 12}, "tower16"),
)


@functools.lru_cache(maxsize=None)
def _boards(blocks, ch):
    return synth_positions(NBOARDS[(blocks, ch)], seed=blocks + ch)


@functools.lru_cache(maxsize=None)
def _case(blocks, ch, which, k):
    """The net's state and its CPU references on every board (computed once, read only)."""
    torch.set_num_threads(8)
    ref = low_range_net(blocks, ch, which, k)
    b, p = _boards(blocks, ch)
    x = encode_batch(b, p)
    p32, v32 = ref.predict(x)
    p64, v64 = as_fp64(ref).predict(x)
    for a in (x, p32, v32, p64, v64):
        a.setflags(write=False)
    return state_to_numpy(ref.net), x, (p32, v32), (p64, v64)


def _argmax_check(probs, ref_probs, boards):
    masks = np.stack([valid_mask(b) for b in boards])
    a = np.argmax(probs * masks, axis=1)
    rm = ref_probs * masks
    r = np.argmax(rm, axis=1)
    srt = np.sort(rm, axis=1)
    bad = (a != r) & (srt[:, -1] - srt[:, -2] >= 2 * TOL)
    assert not bad.any(), np.nonzero(bad)


def _run(m, lib, keys, path, x, boards, players):
    """One forward under `keys` (restored afterwards): outputs, the profile classes that ran."""
    prev = {}
    try:
        for key, v in keys.items():
            prev[key] = lib.azg_pv_set_tuning(key, v)
        m.engine.profile_enable(True)
        if path == "boards":
            B = len(boards)
            probs, values = m.predict_boards(np.asarray(boards, np.int8).reshape(B, 225), np.asarray(players, np.int8),
                                             masked=False)
        else:
            probs, values = m.predict(x)
        ran = m.engine.profile_read()
        m.engine.profile_enable(False)
    finally:
        for key, v in prev.items():
            lib.azg_pv_set_tuning(key, v)
    return probs, values, ran


@pytest.mark.parametrize("which,k", CASES)
@pytest.mark.parametrize("blocks,ch", sorted(NBOARDS))
def test_low_range_forward_matches_oracle(blocks, ch, which, k):
    import _native
    from test_gpu_forward import make_model
    lib = _native.load_library()
    st, x_all, (p32_all, v32_all), (p64_all, v64_all) = _case(blocks, ch, which, k)
    boards_all, players_all = _boards(blocks, ch)
    m = make_model(blocks, ch, st)
    eng = m.engine
    stream = torch.cuda.current_stream().cuda_stream
    eng.tower_diag_clear()
    fp32_gpu = {}
    failures = []
    for name, fch, B, path, keys, cls in FORMS:
        if fch != ch:
            continue
        x, boards, players = x_all[:B], boards_all[:B], players_all[:B]
        if B not in fp32_gpu:
            pg, vg, _ = _run(m, lib, {K.EVAL_ARITH: 0}, "planes", x, boards, players)
            fp32_gpu[B] = (pg, vg)
            for what, got, r32, r64 in (("probs", pg, p32_all[:B], p64_all[:B]), ("values", vg, v32_all[:B], v64_all[:B])):
                e, e_cpu = np.abs(got - r64).max(), np.abs(r32 - r64).max()
                print(f"{blocks}x{ch} {which} k={k} | fp32 B={B} | {what}: |fp32 GPU-fp64|={e:.2e} |cpu32-fp64|={e_cpu:.2e}")
                if not e <= max(TOL, 2 * e_cpu):
                    failures.append((f"fp32 B={B}", what, float(e), float(e_cpu)))
        ps, vs, ran = _run(m, lib, keys, path, x, boards, players)
        assert cls in ran, (name, ran)
        status = (int(lib.azg_pv_tower_status(eng.h, stream)), int(lib.azg_pv_status(eng.h)))
        if status != (0, 0):
            failures.append((name, "status", status))
        for what, got, g32, r32, r64 in (("probs", ps, fp32_gpu[B][0], p32_all[:B], p64_all[:B]),
                                         ("values", vs, fp32_gpu[B][1], v32_all[:B], v64_all[:B])):
            e, e_cpu = np.abs(got - r64).max(), np.abs(r32 - r64).max()
            e_gpu, d = np.abs(g32 - r64).max(), np.abs(got - g32).max()
            print(f"{blocks}x{ch} {which} k={k} | {name} | {what}: |fp32 GPU-fp64|={e_gpu:.2e} |split-fp64|={e:.2e} "
                  f"|cpu32-fp64|={e_cpu:.2e} |split-fp32 GPU|={d:.2e}")
            if not (e <= max(TOL, 2 * e_cpu) and d <= TOL):
                failures.append((name, what, float(e), float(e_cpu), float(d)))
        _argmax_check(ps, p64_all[:B], boards)
    d = eng.tower_diag()
    assert d["h3_overflows"] == 0 and d["timeouts"] == 0 and eng.recoveries == 0, d
    assert not failures, failures
