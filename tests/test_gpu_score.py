"""Scoring without training (azg_pv_score_outputs, PyTorchModel.score_batch,
train.score_buffer, train_alphazero(score_new_games=True)) on the GPU.

  1. the kernels against the fp64 restatement (tests/score_reference.py) on synthetic
     outputs with planted edge rows; the sums' fixed order;
  2. a board's record depends on that board only (bitwise);
  3. end to end against the oracle: |gpu - ref64| within max(1e-5 |ref64| + 1e-7,
     2 |cpu32 - ref64|) per continuous summary key;
  4. host form == device form == chunked, bitwise records;
  5. nothing changes across a score_batch call;  6. the precision follows the handle;
  7. a posted forward is rescored;  8. buffer sweeps;  9. the training loop's report.

Measured on MI355X (test 3, printed): see DESIGN.md section 4g."""
import ast
import functools
import io
import re
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import has_gpu
from _native import TUNE
from oracle.boards import encode_batch, synth_positions, synth_targets
from oracle.ref_net import RefModel, state_to_numpy
from oracle.value_range import as_fp64, calib_bn
from score_reference import planted_case, score_records, summary_from_records
from test_gpu_forward import make_model

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

DEV = "cuda:0"
CONTINUOUS = (0, 1, 2, 4, 7)   # kl, sq, entropy, p_best, target_mass
EXACT = (3, 5, 6)              # top1, v_agree, decided
CONTINUOUS_KEYS = ("policy_loss", "value_loss", "total_loss", "policy_entropy", "target_move_prob", "target_mass")


class keys:
    """Tuning keys set for a block, restored afterwards."""

    def __init__(self, lib, kv):
        self.lib, self.kv, self.prev = lib, kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.prev[k] = self.lib.azg_pv_set_tuning(k, v)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.lib.azg_pv_set_tuning(k, v)


@functools.lru_cache(maxsize=None)
def _model_1x64():
    return make_model(1, 64, seed=11)


def _score_raw(eng, l, v, t, z):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    rec, sums = eng.score_outputs(d(l), d(v), d(t), d(z))
    return rec.cpu().numpy(), sums.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _batch300():
    boards, players = synth_positions(300, seed=300)
    x = encode_batch(boards, players)
    pi, z = synth_targets(300, seed=301)
    for a in (x, pi, z):
        a.setflags(write=False)
    return x, pi, z


# ---------------------------------------------------------------- 1. kernels vs fp64
@pytest.mark.parametrize("B", [1, 3, 5, 257])
def test_records_match_the_fp64_reference(B):
    eng = _model_1x64().engine
    l, v, t, z = planted_case(B, seed=100 + B)
    want = score_records(l, v, t, z)
    rec, sums = _score_raw(eng, l, v, t, z)
    assert rec.dtype == np.float32 and rec.shape == (B, 8) and sums.dtype == np.float64 and sums.shape == (8,)
    assert np.isfinite(rec).all() and np.isfinite(sums).all()
    for f in EXACT:
        assert np.array_equal(rec[:, f].astype(np.float64), want[:, f]), f
    for f in CONTINUOUS:
        err = np.abs(rec[:, f] - want[:, f])
        print(f"B={B} field {f}: max |gpu - fp64| = {err.max():.2e} (largest value {np.abs(want[:, f]).max():.3g})")
        np.testing.assert_allclose(rec[:, f], want[:, f], rtol=1e-5, atol=1e-6, err_msg=f"field {f}")
    np.testing.assert_allclose(sums, rec.astype(np.float64).sum(0), rtol=1e-12, atol=0)
    rec2, sums2 = _score_raw(eng, l, v, t, z)
    assert sums2.tobytes() == sums.tobytes() and rec2.tobytes() == rec.tobytes()
    # [B,1] values / zs are the same call
    rec3, sums3 = _score_raw(eng, l, v.reshape(-1, 1), t, z.reshape(-1, 1))
    assert rec3.tobytes() == rec.tobytes() and sums3.tobytes() == sums.tobytes()


def test_score_outputs_validates_its_arguments():
    eng = _model_1x64().engine
    l, v, t, z = (torch.from_numpy(a).to(DEV) for a in planted_case(6, seed=1))
    for bad in ((l[:, :200].contiguous(), v, t, z), (l, v[:5], t, z), (l, v, t[:5], z), (l, v, t, z[:5]),
                (l.double(), v, t, z), (l, v, t.half(), z), (l, v.cpu(), t, z), (l.cpu(), v.cpu(), t.cpu(), z.cpu()),
                (l, v, t.t().contiguous().t(), z), (l[:0], v[:0], t[:0], z[:0]), (l.cpu().numpy(), v, t, z)):
        with pytest.raises(ValueError):
            eng.score_outputs(*bad)
    eng.score_outputs(l, v, t, z)


# ---------------------------------------------------------------- 2. batch independence
def test_a_record_depends_on_its_board_only():
    eng = _model_1x64().engine
    l, v, t, z = planted_case(300, seed=9)
    rec, _ = _score_raw(eng, l, v, t, z)
    tail, _ = _score_raw(eng, l[256:300], v[256:300], t[256:300], z[256:300])
    one, _ = _score_raw(eng, l[:1], v[:1], t[:1], z[:1])
    assert tail.tobytes() == rec[256:300].tobytes()
    assert one.tobytes() == rec[:1].tobytes()


# ---------------------------------------------------------------- 3. end to end vs the oracle
@pytest.mark.parametrize("blocks,ch", [(2, 64), (1, 128)])
def test_score_batch_matches_the_oracle(blocks, ch):
    torch.set_num_threads(8)
    torch.manual_seed(blocks * 1000 + ch + 7)
    ref = RefModel(blocks, ch)
    calib_bn(ref, seed=blocks * 1000 + ch)
    B = 37
    boards, players = synth_positions(B, seed=B + ch)
    x = encode_batch(boards, players)
    pi, z = synth_targets(B, seed=B + ch + 1)
    score_against_oracle(ref, x, pi, z, f"{blocks}x{ch}")


def score_against_oracle(ref, x, pi, z, tag):
    """score_batch of a model with ref's weights against the fp64 restatement on the fp64
    oracle's outputs; the gate per continuous key is this file's item 3.  Returns (gpu
    summary, fp64 summary, fp64 logits) for further checks."""
    blocks, ch, B = len(ref.net.res_blocks), ref.net.channels, len(x)
    _, v64, l64 = as_fp64(ref).predict(x, with_logits=True)
    ref64 = summary_from_records(score_records(l64, v64, pi, z))
    # the fp32 CPU oracle through torch's own functions
    _, v32, l32 = ref.predict(x, with_logits=True)
    lt, tt = torch.from_numpy(l32), torch.from_numpy(pi)
    lp = F.log_softmax(lt, dim=1)
    pl = float(nn.KLDivLoss(reduction="batchmean")(lp, tt))
    vl = float(nn.MSELoss()(torch.from_numpy(v32), torch.from_numpy(z).reshape(-1, 1)))
    cpu32 = {"policy_loss": pl, "value_loss": vl, "total_loss": pl + vl,
             "policy_entropy": float(-(lp.exp() * lp).sum(1).mean()),
             "target_move_prob": float(lp.exp()[torch.arange(B), tt.argmax(1)].mean()),
             "target_mass": float(tt.sum(1).mean())}
    m = make_model(blocks, ch, state_to_numpy(ref.net))
    gpu = m.score_batch(x, pi, z)
    assert gpu["n"] == B and set(gpu) == set(ref64)
    failures = []
    for k in CONTINUOUS_KEYS:
        d_gpu, d_cpu = abs(gpu[k] - ref64[k]), abs(cpu32[k] - ref64[k])
        print(f"{tag} {k}: ref64={ref64[k]:.9g} |gpu-ref64|={d_gpu:.2e} |cpu32-ref64|={d_cpu:.2e} "
              f"|gpu-cpu32|={abs(gpu[k] - cpu32[k]):.2e}")
        if not d_gpu <= max(1e-5 * abs(ref64[k]) + 1e-7, 2 * d_cpu):
            failures.append((k, d_gpu, d_cpu))
    assert not failures, failures
    return gpu, ref64, l64


# ---------------------------------------------------------------- 4. host, device, chunked
def test_host_form_device_form_and_chunking_agree():
    m = _model_1x64()
    x, pi, z = _batch300()
    s_host, r_host = m.score_batch(x, pi, z, per_board=True)
    assert isinstance(r_host, np.ndarray) and r_host.shape == (300, 8) and r_host.dtype == np.float32
    d = lambda a: torch.from_numpy(a).to(DEV)
    s_dev, r_dev = m.score_batch_device(d(x), d(pi), d(z), per_board=True)
    assert r_dev.is_cuda and r_dev.cpu().numpy().tobytes() == r_host.tobytes()
    s_chunk, r_chunk = m.score_batch(x, pi, z, per_board=True, max_batch=128)
    assert r_chunk.tobytes() == r_host.tobytes()
    assert s_host == s_dev                                  # the same launches
    assert list(s_host) == list(s_chunk) and s_chunk["n"] == 300
    for k in s_host:
        np.testing.assert_allclose(s_chunk[k], s_host[k], rtol=1e-12, atol=0, err_msg=k)
    assert m.score_batch(x, pi, z) == s_host                 # without the records: the dict alone
    want = summary_from_records(r_host)
    for k in s_host:
        np.testing.assert_allclose(s_host[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    proxy = m.symmetric("mean8")                             # a SymmetricModel scores as its model
    assert proxy.score_batch(x, pi, z) == s_host
    with pytest.raises(ValueError):
        m.score_batch(x, pi[:299], z)
    with pytest.raises(ValueError):
        m.score_batch(x[:0], pi[:0], z[:0])


# ---------------------------------------------------------------- 5. no side effects
@pytest.mark.parametrize("training", [True, False])
def test_score_batch_changes_nothing(training):
    m = make_model(1, 64, seed=13)
    x, pi, z = (a[:48] for a in _batch300())
    m.train_batch(x[:16], pi[:16], z[:16])                  # grads, Adam moments and BN counters are live
    fixed = x[16:32]
    m.net.train(training)
    eng = m.engine

    def snapshot():
        torch.cuda.synchronize()
        opt = m.optimizer.state_dict()
        flat = [t.detach().cpu().numpy().tobytes() for t in (eng.flat_params, eng.flat_grads_ext, eng.flat_bn,
                                                             eng.flat_nbt, m.optimizer.flat_exp_avg,
                                                             m.optimizer.flat_exp_avg_sq)]
        state = [(i, k, v.detach().cpu().numpy().tobytes() if torch.is_tensor(v) else v)
                 for i, st in sorted(opt["state"].items()) for k, v in sorted(st.items())]
        nbt = [b.num_batches_tracked.item() for b in m.net.modules() if isinstance(b, nn.BatchNorm2d)]
        return flat, state, repr(opt["param_groups"]), nbt, m.optimizer.get_step()

    p0, v0 = m.predict(fixed)
    before = snapshot()
    assert before[3][0] == 1 and before[4] == 1
    s, rec = m.score_batch(x, pi, z, per_board=True)
    assert np.isfinite(rec).all() and s["n"] == 48
    assert m.net.training is training
    assert snapshot() == before
    p1, v1 = m.predict(fixed)
    assert p1.tobytes() == p0.tobytes() and v1.tobytes() == v0.tobytes()
    assert m.net.training is training


# ---------------------------------------------------------------- 6. precision follows the handle
@functools.lru_cache(maxsize=None)
def _models_2x128():
    exact = make_model(2, 128, seed=21)
    half = make_model(2, 128, state_to_numpy(exact.net))
    half.set_eval_precision("fp16")
    return exact, half


def test_scoring_runs_in_the_handles_precision():
    exact, half = _models_2x128()
    x, pi, z = (a[:37] for a in _batch300())
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    _, r_half = half.score_batch(x, pi, z, per_board=True)
    assert half.eval_precision == "fp16"
    xd = d(x)
    _, values, logits = half.engine.forward(xd, want_logits=True)
    rec, _ = half.engine.score_outputs(logits, values, d(pi), d(z))
    torch.cuda.synchronize()
    half.engine.recover(half.engine.last_seq())
    assert rec.cpu().numpy().tobytes() == r_half.tobytes()
    _, r_exact = exact.score_batch(x, pi, z, per_board=True)
    assert not np.array_equal(r_exact[:, 0], r_half[:, 0]) and not np.array_equal(r_exact[:, 1], r_half[:, 1])


# ---------------------------------------------------------------- 7. a posted forward is rescored
def test_a_timed_out_forward_is_rescored():
    """Key 14 = 0 makes the split form's exchange waits time out at once
    (test_gpu_precision's timed-out launch): the forward is posted with invalid logits,
    recover reruns it and score_batch scores the recomputed logits (run once)."""
    import _native
    lib = _native.load_library()
    _, half = _models_2x128()
    eng = half.engine
    x, pi, z = (a[:3] for a in _batch300())
    s0, r0 = half.score_batch(x, pi, z, per_board=True)
    eng.tower_diag_clear()
    n0 = eng.recoveries
    try:
        with keys(lib, {TUNE.TOWER_WAIT_US: 0}):
            s1, r1 = half.score_batch(x, pi, z, per_board=True)
        assert eng.recoveries == n0 + 1 and eng.tower_diag()["timeouts"] > 0
        assert r1.tobytes() == r0.tobytes() and s1 == s0
        eng.check_status()
    finally:
        eng.clear_status()
        eng.tower_diag_clear()


# ---------------------------------------------------------------- 8. buffer sweeps
def test_score_buffer_on_both_buffer_kinds():
    import train
    from replay import DeviceReplayBuffer
    m = _model_1x64()
    boards, players = synth_positions(55, seed=201)
    states = encode_batch(boards, players)
    pis, zs = synth_targets(55, seed=202)
    pos = [(states[i], pis[i], float(zs[i, 0])) for i in range(55)]   # canonical (state, pi, z) examples
    dev = DeviceReplayBuffer(320, DEV)                       # a ring of 40 positions, symmetries on
    dev.add_positions(pos[:30])
    dev.add_positions(pos[30:])                              # 55 > 40: wrapped once
    assert dev.count == 40 and dev.head == 15 and len(dev) == 320
    host = dev.to_host()
    assert len(host) == 320
    a = train.score_buffer(m, dev, batch_size=128)
    b = train.score_buffer(m, host, batch_size=128)
    assert a["n"] == b["n"] == 320 and list(a) == list(b)
    for k in a:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-12, atol=0, err_msg=k)
    # the first 100 images, whatever the batch size splits them into
    first = list(host.buffer)[:100]
    S = np.stack([e[0] for e in first])
    P = np.stack([e[1] for e in first])
    Z = np.array([e[2] for e in first], dtype=np.float32)
    want = m.score_batch(S, P, Z)
    for buf in (dev, host):
        got = train.score_buffer(m, buf, batch_size=64, max_examples=100)
        assert got["n"] == 100
        for k in want:
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    assert train.score_buffer(m, dev, max_examples=1000)["n"] == 320
    with pytest.raises(ValueError):
        train.score_buffer(m, DeviceReplayBuffer(8, DEV))


# ---------------------------------------------------------------- 9. the loop
@pytest.mark.parametrize("case", ["host", "device_buffer", "defaults"])
def test_the_training_loop_reports_new_game_scores(case, tmp_path, monkeypatch):
    import train
    from network import PyTorchModel
    calls = []
    score_batch = PyTorchModel.score_batch

    def recording_score_batch(self, states, *a, **kw):
        calls.append((self.eval_precision, len(states), self.net.training))
        return score_batch(self, states, *a, **kw)

    monkeypatch.setattr(PyTorchModel, "score_batch", recording_score_batch)
    h = []
    limit = 50
    kw = dict(num_iterations=1, games_per_iteration=2, n_simulations=16, batch_size=16, epochs_per_iter=1,
              eval_games=2, eval_mcts_simulations=8, n_res_blocks=2, channels=128, max_moves=6,
              selfplay_precision="fp16", model_dir=str(tmp_path), history=h)
    if case != "defaults":
        kw.update(score_new_games=True, score_max_examples=limit, device_buffer=case == "device_buffer")
    log = io.StringIO()
    with redirect_stdout(log):
        train.train_alphazero(**kw)
    out = log.getvalue()
    assert len(h) == 1 and h[0]["iteration"] == 1
    printed = ast.literal_eval(re.search(r"last_loss=(\{.*?\})", out).group(1))
    assert h[0]["last_train_loss"] == printed and set(printed) == {"policy_loss", "value_loss", "total_loss"}
    if case == "defaults":
        assert calls == [] and h[0]["new_games_before"] is None and h[0]["new_games_after"] is None
        assert "new games" not in out
        return
    # 2 games x 6 moves: 96 examples with host symmetries (the first 50 are scored), 12 canonical ones
    n = 12 if case == "device_buffer" else limit
    assert [c[:2] for c in calls] == [("exact", n), ("exact", n)]
    before, after = h[0]["new_games_before"], h[0]["new_games_after"]
    for d in (before, after):
        assert d["n"] == n and 0 < d["n"] <= limit
        assert all(np.isfinite(v) for v in d.values())
        assert d["total_loss"] == d["policy_loss"] + d["value_loss"] and 0.0 <= d["policy_top1"] <= 1.0
    assert before != after                                   # the net trained in between
    for tag, d in (("before training", before), ("after training", after)):
        line = re.search(rf"new games {tag}: (.*)", out).group(1)
        assert f"n={n} " in line and f"policy_loss={d['policy_loss']:.6f}" in line
        assert f"total_loss={d['total_loss']:.6f}" in line and f"policy_top1={d['policy_top1']:.4f}" in line
