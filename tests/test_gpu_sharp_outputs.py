"""The eval forward on nets with peaked policy outputs.

Every other parity net of the suite has a nearly uniform policy (largest probability of a
row about 0.04).  dp_i = p_i (dl_i - sum_j p_j dl_j), so there the absolute 1e-5 bar on
probabilities lets a logit error of 1e-3 pass; at p ~ 0.5 the same bar needs the logits
good to 2e-5.  The nets here are the seeded, calibrated nets of test_gpu_value_range.py
with policy_fc scaled by 2^k, k in oracle.value_range.SHARP (exact: every logit scales by
2^k), and k = 0 beside them as the control; tests/test_oracle_sharp_outputs.py shows on the
CPU that the reference alone is within 5e-6 of fp64 on them, so the unchanged bar is fair.

Gates, against the fp64 RefModel on the same weights:
  1. every eval form of test_gpu_value_range.FORMS, the fp32 forward, and 2x64 (fp32 only):
     |gpu - fp64| <= max(1e-5, 2 |cpu32 - fp64|) on probs and values; split forms also
     |split - fp32 GPU| <= 1e-5; masked argmax exact outside the rows the CPU test exempts;
     the expected profile class, statuses 0, no overflow recompute, no recovery;
  2. logits (planes path): bitwise 2^k x the same form's logits at k = 0 (pins a failure of 1
     to the softmax or the trunk); max|logit_gpu - logit_fp64| <= max(2e-5, 2 max|logit_cpu32 -
     logit_fp64|), where 2e-5 is the logit error that keeps every probability within 1e-5 at
     any sharpness (|dp| <= 2 p (1 - p) max|dl| <= 0.5 max|dl|);
  3. the softmax alone: GPU probs against an fp64 softmax of the GPU's own logits, within
     max(1e-7, 2 d), d the deviation of torch's fp32 CPU softmax of those logits from it (the
     floor is one fp32 ulp at p ~ 1);
  4. the one-product fp16 precision: |gpu16 - fp64| <= 2 |emu16 - fp64|, argmax outside
     near-ties, near-tie share <= 1/3 (test_fp16_forward_accuracy_on_low_range_nets's gates);
  5. score_batch on the k = 3 net against tests/score_reference.py.

Measured on MI355X (printed by every test): see DESIGN.md section 5."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import has_gpu
from _native import TUNE
from oracle.value_range import SHARP, SHARP_BOARDS, SHARP_PREFIXES, sharp_case, sharp_net
from test_gpu_value_range import FORMS, NBOARDS, _run

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

K = TUNE
TOL = 1e-5
LOGIT_TOL = 2e-5
SOFTMAX_FLOOR = 1e-7
KS = (0,) + SHARP
# 2x64 has no split form: the default form (whatever the tuner picks) and EVAL_ARITH 0 are fp32
FORMS_64 = (("default B=37", 64, 37, "planes", {}, ("tower", "conv3x3")),)
ALL_FORMS = tuple((n, c, B, path, keys, (cls,)) for n, c, B, path, keys, cls in FORMS) + FORMS_64
SHAPES = sorted(SHARP_BOARDS)


def test_board_sets_are_the_value_range_tests():
    for shape, n in NBOARDS.items():
        assert SHARP_BOARDS[shape] == (n, sum(shape))
    for name, ch, B, path, keys, cls in ALL_FORMS:
        shape = [s for s in SHAPES if s[1] == ch]
        assert len(shape) == 1 and B in SHARP_PREFIXES[shape[0]], name


@functools.lru_cache(maxsize=None)
def _model(blocks, ch, k, fp16=False):
    from test_gpu_forward import make_model
    m = make_model(blocks, ch, sharp_case(blocks, ch, k)["state"])
    if fp16:
        m.set_eval_precision("fp16")
        assert m.eval_precision == "fp16"
    return m


def _lib():
    import _native
    return _native.load_library()


def _dev(a, r):
    return float(np.abs(np.asarray(a, np.float64) - r).max())


def _argmax_failures(probs, c, B):
    """Rows, outside the exempt ones, whose masked argmax is not fp64's."""
    a = np.argmax(probs * c["masks"][:B], axis=1)
    r = np.argmax(c["p64"][:B] * c["masks"][:B], axis=1)
    return np.nonzero((a != r) & ~c["exempt"][:B])[0].tolist()


def forward_failures(blocks, ch, k, m):
    """Gate 1 for model m (the net of sharp_case(blocks, ch, k) on the GPU): every failure, so
    one run reports every form."""
    lib = _lib()
    c = sharp_case(blocks, ch, k)
    eng = m.engine
    stream = torch.cuda.current_stream().cuda_stream
    eng.tower_diag_clear()
    r0 = eng.recoveries
    fp32_gpu = {}
    failures = []
    tag = f"{blocks}x{ch} k={k}"
    for name, fch, B, path, keys, classes in ALL_FORMS:
        if fch != ch:
            continue
        x, boards, players = c["x"][:B], c["boards"][:B], c["players"][:B]
        refs = (("probs", c["p32"][:B], c["p64"][:B]), ("values", c["v32"][:B], c["v64"][:B]))
        if B not in fp32_gpu:
            pg, vg, _ = _run(m, lib, {K.EVAL_ARITH: 0}, "planes", x, boards, players)
            fp32_gpu[B] = (pg, vg)
            for (what, r32, r64), got in zip(refs, (pg, vg)):
                e, e_cpu = _dev(got, r64), _dev(r32, r64)
                print(f"{tag} | fp32 B={B} | {what}: |fp32 GPU-fp64|={e:.2e} |cpu32-fp64|={e_cpu:.2e}")
                if not e <= max(TOL, 2 * e_cpu):
                    failures.append((tag, f"fp32 B={B}", what, e, e_cpu))
            bad = _argmax_failures(pg, c, B)
            if bad:
                failures.append((tag, f"fp32 B={B}", "argmax", bad))
        ps, vs, ran = _run(m, lib, keys, path, x, boards, players)
        if not set(classes) & set(ran):
            failures.append((tag, name, "profile class", sorted(ran)))
        status = (int(lib.azg_pv_tower_status(eng.h, stream)), int(lib.azg_pv_status(eng.h)))
        if status != (0, 0):
            failures.append((tag, name, "status", status))
        for (what, r32, r64), got, g32 in zip(refs, (ps, vs), fp32_gpu[B]):
            e, e_cpu, d = _dev(got, r64), _dev(r32, r64), _dev(got, g32.astype(np.float64))
            print(f"{tag} | {name} | {what}: |gpu-fp64|={e:.2e} |cpu32-fp64|={e_cpu:.2e} |gpu-fp32 GPU|={d:.2e}")
            if not (e <= max(TOL, 2 * e_cpu) and d <= TOL):
                failures.append((tag, name, what, e, e_cpu, d))
        bad = _argmax_failures(ps, c, B)
        if bad:
            failures.append((tag, name, "argmax", bad))
    d = eng.tower_diag()
    if d["h3_overflows"] or d["timeouts"] or eng.recoveries != r0:
        failures.append((tag, "diag", d, eng.recoveries - r0))
    return failures


def _logit_forms(ch):
    """(name, B, keys): the fp32 form at every batch and each form the planes path reaches."""
    forms, seen = [], set()
    for name, fch, B, path, keys, _ in ALL_FORMS:
        if fch != ch or path != "planes":
            continue
        if B not in seen:
            seen.add(B)
            forms.append((f"fp32 B={B}", B, {K.EVAL_ARITH: 0}))
        forms.append((name, B, keys))
    return forms


def _forward_logits(m, keys, x):
    """(probs, values, logits) of the planes path under `keys` (restored afterwards)."""
    lib, prev = _lib(), {}
    try:
        for key, v in keys.items():
            prev[key] = lib.azg_pv_set_tuning(key, v)
        p, v, l = m.engine.forward(torch.from_numpy(np.ascontiguousarray(x)), want_logits=True)
        out = tuple(t.cpu().numpy() for t in (p, v, l))
    finally:
        for key, v in prev.items():
            lib.azg_pv_set_tuning(key, v)
    stream = torch.cuda.current_stream().cuda_stream
    return out, (int(lib.azg_pv_tower_status(m.engine.h, stream)), int(lib.azg_pv_status(m.engine.h)))


def logit_failures(blocks, ch, k, m, logits0):
    """Gates 2 and 3 for model m.  logits0: {form: GPU logits at k = 0} (filled in at k = 0)."""
    c = sharp_case(blocks, ch, k)
    failures = []
    tag = f"{blocks}x{ch} k={k}"
    for name, B, keys in _logit_forms(ch):
        (pg, vg, lg), status = _forward_logits(m, keys, c["x"][:B])
        if status != (0, 0):
            failures.append((tag, name, "status", status))
        if k == 0:
            logits0[name] = lg
        elif not np.array_equal(lg, logits0[name] * np.float32(2.0 ** k)):
            failures.append((tag, name, "logits are not 2^k x the logits at k = 0",
                             _dev(lg, logits0[name].astype(np.float64) * 2.0 ** k)))
        e, e_cpu = _dev(lg, c["l64"][:B]), _dev(c["l32"][:B], c["l64"][:B])
        soft64 = F.softmax(torch.from_numpy(lg).double(), dim=1).numpy()
        s = _dev(pg, soft64)
        d = _dev(F.softmax(torch.from_numpy(lg), dim=1).numpy(), soft64)
        print(f"{tag} | {name} | logits: |gpu-fp64|={e:.2e} |cpu32-fp64|={e_cpu:.2e} | softmax alone: "
              f"|gpu-fp64 softmax|={s:.2e} |torch fp32 softmax-fp64 softmax|={d:.2e}")
        if not e <= max(LOGIT_TOL, 2 * e_cpu):
            failures.append((tag, name, "logits", e, e_cpu))
        if not s <= max(SOFTMAX_FLOOR, 2 * d):
            failures.append((tag, name, "softmax", s, d))
    return failures


@pytest.mark.parametrize("blocks,ch", SHAPES)
def test_sharp_forward_matches_oracle(blocks, ch):
    failures = []
    for k in KS:
        failures += forward_failures(blocks, ch, k, _model(blocks, ch, k))
    assert not failures, failures


@pytest.mark.parametrize("blocks,ch", SHAPES)
def test_sharp_logits_scale_bitwise_and_the_softmax_is_fp32(blocks, ch):
    failures, logits0 = [], {}
    for k in KS:
        failures += logit_failures(blocks, ch, k, _model(blocks, ch, k), logits0)
    assert not failures, failures


@functools.lru_cache(maxsize=None)
def _emu16(k):
    from fp16_emulation import half_forward
    c = sharp_case(2, 128, k)
    pe, ve = half_forward(c["state"], c["x"])
    pe.setflags(write=False)
    ve.setflags(write=False)
    return pe, ve


def test_sharp_fp16_forward_accuracy():
    from fp16_emulation import near_tie_stats
    from test_gpu_precision import _i8, keys
    lib = _lib()
    stream = torch.cuda.current_stream().cuda_stream
    forms = [("B=3 split", 3, {}), ("B=3 one workgroup", 3, {K.BOARD16_SPLIT_MAX: 0}),
             ("B=258 one workgroup", 258, {K.BOARD16_SPLIT_MAX: 0})]
    failures = []
    for k in KS:
        c = sharp_case(2, 128, k)
        pe, ve = _emu16(k)
        m = _model(2, 128, k, fp16=True)
        eng = m.engine
        eng.tower_diag_clear()
        r0 = eng.recoveries
        for name, B, kv in forms:
            bi8, pl8 = _i8(c["boards"][:B], c["players"][:B])
            for path in ("planes", "boards"):
                with keys(lib, kv):
                    eng.profile_enable(True)
                    pg, vg = m.predict(c["x"][:B]) if path == "planes" else m.predict_boards(bi8, pl8, masked=False)
                    ran = eng.profile_read()
                    eng.profile_enable(False)
                if "board16" not in ran:
                    failures.append((k, name, path, "profile class", sorted(ran)))
                status = (int(lib.azg_pv_tower_status(eng.h, stream)), int(lib.azg_pv_status(eng.h)))
                if status != (0, 0):
                    failures.append((k, name, path, "status", status))
                for what, got, emu, r64 in (("probs", pg, pe[:B], c["p64"][:B]), ("values", vg, ve[:B], c["v64"][:B])):
                    d_emu, d_gpu = _dev(emu, r64), _dev(got, r64)
                    print(f"2x128 k={k} | fp16 {name} {path} | {what}: |gpu16-emu16|={_dev(got, emu):.2e} "
                          f"|gpu16-fp64|={d_gpu:.2e} |emu16-fp64|={d_emu:.2e}")
                    if not d_gpu <= 2 * d_emu:
                        failures.append((k, name, path, what, d_gpu, d_emu))
                bad, share = near_tie_stats(pg, c["p64"][:B], c["boards"][:B], _dev(pe[:B], c["p64"][:B]))
                print(f"2x128 k={k} | fp16 {name} {path} | near-tie share {share:.3f}")
                if bad.size:
                    failures.append((k, name, path, "argmax", bad.tolist()))
                if share > 1 / 3:
                    failures.append((k, name, path, "near-tie share", share))
        d = eng.tower_diag()
        if d["h3_overflows"] or d["timeouts"] or eng.recoveries != r0:
            failures.append((k, "diag", d, eng.recoveries - r0))
    assert not failures, failures


def test_sharp_score_batch_matches_the_oracle():
    """score_batch on the k = 3 2x128 net (peaked rows: what cross-entropy, entropy and top-1
    exist for).  Even rows' targets are the k = 0 net's own fp64 policy (same argmax, so top-1
    is live), odd rows' are synthetic; zs are synthetic.  The continuous keys are gated as in
    test_score_batch_matches_the_oracle; top-1 and the sign agreement equal fp64's exactly,
    given that no row's fp64 top-2 logit gap is within the logits gate of a tie (asserted)."""
    from oracle.boards import synth_targets
    from test_gpu_score import score_against_oracle
    B = 37
    c = sharp_case(2, 128, 3)
    pi, z = synth_targets(B, seed=B + 128 + 1)
    pi = pi.copy()
    pi[::2] = sharp_case(2, 128, 0)["p64"][:B:2].astype(np.float32)
    gpu, ref64, l64 = score_against_oracle(sharp_net(2, 128, 3), c["x"][:B], pi, z, "2x128 k=3")
    assert np.abs(l64 - c["l64"][:B]).max() < 1e-9       # the same fp64 forward, in another batch
    srt = np.sort(l64, axis=1)
    assert (srt[:, -1] - srt[:, -2]).min() > 1e-3        # 25 x the logits gate at k = 3
    assert np.abs(c["v64"][:B].ravel()[z.ravel() != 0]).min() > 1e-3   # no decided row's value is near a sign change
    print(f"2x128 k=3 policy_top1 {gpu['policy_top1']:.4f} (fp64 {ref64['policy_top1']:.4f}) "
          f"entropy {ref64['policy_entropy']:.4f} of ln 225 = {np.log(225):.4f}")
    assert 0.4 <= ref64["policy_top1"] <= 0.6            # the planted half agrees, the synthetic half does not
    assert gpu["policy_top1"] == ref64["policy_top1"]
    assert gpu["value_sign_agreement"] == ref64["value_sign_agreement"]
