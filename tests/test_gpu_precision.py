"""The opt-in one-product fp16 eval precision (azg_pv_set_eval_precision, AZG_PV_EVAL_FP16)
on the GPU: the board16 tower with one MFMA per product on operands rounded once to fp16.

  1. discriminating: on a net whose conv2 operand does not depend on conv1's accumulators the
     GPU is the CPU emulation (tests/fp16_emulation.py) to 1e-5, while the emulation is at
     least 1e-4 from fp64 -- a kernel that ran the three-product arithmetic fails by ~80x;
  2. accuracy: |gpu16 - fp64| <= 2 |emu16 - fp64| on the low-range nets, masked argmax
     fp64's outside near-ties, near-ties rare;
  3. bitwise inside the mode: batch independence, split == one workgroup, the tail path,
     boards == planes, symmetries == the host transform;
  4. isolation between handles and from the exact precision; the pack follows the weights;
  5. the range guard recomputes in fp32;  6. a timed-out split launch is rerun in fp16;
  7. the training loop's self-play phase and a Player run in it and leave the model exact.

Measured on MI355X (accuracy cases, printed by test 2): see DESIGN.md section 4f."""
import functools

import numpy as np
import pytest
import torch

from conftest import has_gpu
from _native import TUNE
from fp16_emulation import half_forward, near_tie_stats
from oracle.boards import encode_batch, synth_positions
from oracle.ref_net import RefModel, state_to_numpy
from oracle.value_range import CASES, as_fp64, calib_bn, low_range_net
from test_gpu_forward import make_model

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

K = TUNE
NB = 258


def _i8(boards, players):
    B = len(boards)
    return np.ascontiguousarray(boards, np.int8).reshape(B, 225), np.ascontiguousarray(players, np.int8)


def fp16_model(blocks, ch, state=None, seed=0):
    m = make_model(blocks, ch, state, seed)
    m.set_eval_precision("fp16")
    assert m.eval_precision == "fp16"
    return m


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


def _lib():
    import _native
    return _native.load_library()


# ---------------------------------------------------------------- 1. discriminating
@functools.lru_cache(maxsize=None)
def _beta_net():
    """1x128, bn1.weight = 0 and bn1.bias uniform in [0.5, 1.5) off the fp16 grid, running
    stats calibrated afterwards: conv2's operand is fp16(beta) whatever conv1 accumulated."""
    torch.set_num_threads(8)
    torch.manual_seed(1128)
    ref = RefModel(1, 128)
    g = torch.Generator().manual_seed(7)
    beta = (torch.rand(128, generator=g) + 0.5).float()
    on_grid = beta.half().float() == beta
    beta = torch.where(on_grid, beta + 2.0 ** -13, beta)
    assert not bool((beta.half().float() == beta).any())
    with torch.no_grad():
        ref.net.res_blocks[0].bn1.weight.zero_()
        ref.net.res_blocks[0].bn1.bias.copy_(beta)
    calib_bn(ref, seed=1128)
    boards, players = synth_positions(37, seed=11)
    x = encode_batch(boards, players)
    st = state_to_numpy(ref.net)
    p32, v32 = ref.predict(x)
    p64, v64 = as_fp64(ref).predict(x)
    pe, ve = half_forward(st, x)
    return st, boards, players, x, (p32, v32), (p64, v64), (pe, ve)


@pytest.mark.parametrize("B", [5, 37])
def test_fp16_forward_is_the_one_product_arithmetic(B):
    st, boards, players, x, (p32, v32), (p64, v64), (pe, ve) = _beta_net()
    dev_emu = np.abs(ve[:B] - v64[:B]).max()
    dev_32 = np.abs(v32[:B] - v64[:B]).max()
    print(f"beta net B={B}: |emu16-fp64| values {dev_emu:.2e}, |cpu32-fp64| {dev_32:.2e}")
    assert dev_emu >= 1e-4 and dev_32 <= 1e-5        # the precondition (CPU side)
    m = fp16_model(1, 128, st)
    pg, vg = m.predict(x[:B])
    dp, dv = np.abs(pg - pe[:B]).max(), np.abs(vg - ve[:B]).max()
    print(f"beta net B={B}: |gpu16-emu16| probs {dp:.2e} values {dv:.2e}; "
          f"|gpu16-fp64| values {np.abs(vg - v64[:B]).max():.2e}")
    assert dp <= 1e-5 and dv <= 1e-5, (dp, dv)
    m.set_eval_precision("exact")                     # and the exact form on the same handle is not it
    _, vx = m.predict(x[:B])
    assert np.abs(vx - v64[:B]).max() <= 1e-5 < np.abs(vx - ve[:B]).max()


# ---------------------------------------------------------------- 2. accuracy
@functools.lru_cache(maxsize=None)
def _case(which, k):
    torch.set_num_threads(8)
    ref = low_range_net(2, 128, which, k)
    boards, players = synth_positions(NB, seed=2 + 128)
    x = encode_batch(boards, players)
    st = state_to_numpy(ref.net)
    p64, v64 = as_fp64(ref).predict(x)
    pe, ve = half_forward(st, x)
    for a in (x, p64, v64, pe, ve):
        a.setflags(write=False)
    return st, boards, players, x, (p64, v64), (pe, ve)


@pytest.mark.parametrize("which,k", CASES)
def test_fp16_forward_accuracy_on_low_range_nets(which, k):
    lib = _lib()
    st, boards, players, x_all, (p64, v64), (pe, ve) = _case(which, k)
    big = 258 if (which, k) in (("stem", 0), ("stem", 12)) else 37
    forms = [("B=3 split", 3, {}), ("B=3 one workgroup", 3, {K.BOARD16_SPLIT_MAX: 0}),
             (f"B={big} one workgroup", big, {K.BOARD16_SPLIT_MAX: 0})]
    m = fp16_model(2, 128, st)
    eng = m.engine
    stream = torch.cuda.current_stream().cuda_stream
    eng.tower_diag_clear()
    failures = []
    for name, B, kv in forms:
        bi8, pl8 = _i8(boards[:B], players[:B])
        for path in ("planes", "boards"):
            with keys(lib, kv):
                eng.profile_enable(True)
                pg, vg = m.predict(x_all[:B]) if path == "planes" else m.predict_boards(bi8, pl8, masked=False)
                ran = eng.profile_read()
                eng.profile_enable(False)
            assert "board16" in ran, (name, ran)
            status = (int(lib.azg_pv_tower_status(eng.h, stream)), int(lib.azg_pv_status(eng.h)))
            if status != (0, 0):
                failures.append((name, path, "status", status))
            for what, got, emu, r64 in (("probs", pg, pe[:B], p64[:B]), ("values", vg, ve[:B], v64[:B])):
                d_emu, d_gpu = np.abs(emu - r64).max(), np.abs(got - r64).max()
                print(f"2x128 {which} k={k} | {name} {path} | {what}: |gpu16-emu16|={np.abs(got - emu).max():.2e} "
                      f"|gpu16-fp64|={d_gpu:.2e} |emu16-fp64|={d_emu:.2e}")
                if not d_gpu <= 2 * d_emu:
                    failures.append((name, path, what, float(d_gpu), float(d_emu)))
            bad, share = near_tie_stats(pg, p64[:B], boards[:B], np.abs(pe[:B] - p64[:B]).max())
            print(f"2x128 {which} k={k} | {name} {path} | near-tie share {share:.3f}")
            if bad.size:
                failures.append((name, path, "argmax", bad.tolist()))
            if share > 1 / 3:
                failures.append((name, path, "near-tie share", share))
    d = eng.tower_diag()
    assert d["h3_overflows"] == 0 and d["timeouts"] == 0 and eng.recoveries == 0, d
    assert not failures, failures


# ---------------------------------------------------------------- 3. bitwise inside the mode
@functools.lru_cache(maxsize=None)
def _mode_case():
    m = fp16_model(2, 128, seed=21)
    boards, players = synth_positions(300, seed=300)
    x = encode_batch(boards, players)
    p, v = m.predict(x)
    for a in (x, p, v):
        a.setflags(write=False)
    return m, boards, players, x, p, v


def test_fp16_rows_do_not_depend_on_the_batch():
    m, boards, players, x, p300, v300 = _mode_case()
    p1, v1 = m.predict(x[:1])
    p37, v37 = m.predict(x[100:137])
    assert np.array_equal(p1, p300[:1]) and np.array_equal(v1, v300[:1])
    assert np.array_equal(p37, p300[100:137]) and np.array_equal(v37, v300[100:137])
    perm = np.random.default_rng(3).permutation(300)
    pp, vp = m.predict(x[perm])
    assert np.array_equal(pp, p300[perm]) and np.array_equal(vp, v300[perm])


@pytest.mark.parametrize("B", [3, 85])
def test_fp16_split_is_bitwise_one_workgroup(B):
    lib = _lib()
    m, boards, players, x, p300, v300 = _mode_case()
    bi8, pl8 = _i8(boards[:B], players[:B])
    with keys(lib, {K.BOARD16_SPLIT_MAX: 0}):
        p0, v0 = m.predict(x[:B])
        q0, w0 = m.predict_boards(bi8, pl8, masked=False)
    with keys(lib, {K.BOARD16_SPLIT_MAX: 85}):
        p1, v1 = m.predict(x[:B])
        q1, w1 = m.predict_boards(bi8, pl8, masked=False)
    assert np.array_equal(p1, p0) and np.array_equal(v1, v0)
    assert np.array_equal(q1, q0) and np.array_equal(w1, w0)
    assert np.array_equal(p0, p300[:B]) and np.array_equal(q0, p0) and np.array_equal(w0, v0)   # boards == planes


def test_fp16_tail_path_is_bitwise_its_boards_alone():
    """B = 258 + 3: more boards than the launch grid (one workgroup per CU), so the last
    partial round runs split after the full rounds."""
    m, boards, players, x, p300, v300 = _mode_case()
    B = 258 + 3
    p, v = m.predict(x[:B])
    assert np.array_equal(p, p300[:B]) and np.array_equal(v, v300[:B])
    pt, vt = m.predict(x[256:B])
    assert np.array_equal(pt, p[256:]) and np.array_equal(vt, v[256:])
    bi8, pl8 = _i8(boards[:B], players[:B])
    q, w = m.predict_boards(bi8, pl8, masked=False)
    assert np.array_equal(q, p) and np.array_equal(w, v)


def test_fp16_symmetries_are_the_host_transform():
    from network import apply_symmetry, invert_symmetry
    from test_gpu_symmetry import positions, seq_mean8
    m = _mode_case()[0]
    b, p = positions(5, seed=17)
    P, V = [], []
    for s in range(8):
        probs, v = m.predict_boards(apply_symmetry(b, s), p, masked=False)
        P.append(invert_symmetry(probs, s))
        V.append(v)
    p3, v3 = m.predict_boards(b, p, masked=False, symmetry=3)
    assert np.array_equal(p3, P[3]) and np.array_equal(v3, V[3])
    pm, vm = m.predict_boards(b, p, masked=False, symmetry="mean8")
    assert np.array_equal(pm, seq_mean8(P)) and np.array_equal(vm, seq_mean8(V))


# ---------------------------------------------------------------- 4. isolation
def test_precision_is_isolated_between_models_and_follows_the_weights():
    from oracle.boards import synth_targets
    a = make_model(2, 128, seed=31)
    st = state_to_numpy(a.net)
    b = make_model(2, 128, st)
    boards, players = synth_positions(37, seed=37)
    x = encode_batch(boards, players)
    pa, va = a.predict(x)                                # exact, recorded first
    b.set_eval_precision("fp16")
    pb, vb = b.predict(x)
    assert a.eval_precision == "exact" and b.eval_precision == "fp16"
    assert not np.array_equal(vb, va)                    # b ran another arithmetic
    p, v = a.predict(x)
    assert np.array_equal(p, pa) and np.array_equal(v, va)
    a.set_eval_precision("fp16")
    p16, v16 = a.predict(x)
    assert np.array_equal(p16, pb) and np.array_equal(v16, vb)   # same weights, same mode: same bits
    a.set_eval_precision("exact")
    p, v = a.predict(x)
    assert np.array_equal(p, pa) and np.array_equal(v, va)
    # a parameter change through the train step: the fp16 pack follows
    pi, z = synth_targets(37, seed=38)
    b.train_batch(x, pi, z, epochs=1)
    b.net.eval()
    assert b.eval_precision == "fp16"
    pb2, vb2 = b.predict(x)
    assert not np.array_equal(pb2, pb)
    fresh = fp16_model(2, 128, state_to_numpy(b.net))
    pf, vf = fresh.predict(x)
    assert np.array_equal(pf, pb2) and np.array_equal(vf, vb2)


def test_checkpoints_do_not_carry_the_precision(tmp_path):
    """save / load keep the reference's dict format; load leaves the model's precision alone."""
    a = fp16_model(1, 128, seed=41)
    path = str(tmp_path / "m.pt")
    a.save(path)
    assert set(torch.load(path, map_location="cpu", weights_only=True)) == {"net", "opt", "board_size", "action_size"}
    b = make_model(1, 128, seed=42)
    b.load(path)
    assert b.eval_precision == "exact"
    b.set_eval_precision("fp16")
    b.load(path)
    assert b.eval_precision == "fp16"
    boards, players = synth_positions(5, seed=43)
    x = encode_batch(boards, players)
    pa, va = a.predict(x)
    pb, vb = b.predict(x)
    assert np.array_equal(pa, pb) and np.array_equal(va, vb)


# ---------------------------------------------------------------- 5. range guard
def test_fp16_range_guard_recomputes_in_fp32():
    """test_h3_range_guard_recomputes_in_fp32's construction: the stem BN gamma x 1e5 drives
    conv inputs past fp16's range; the launch is posted and recomputed with fp32 MFMA."""
    lib = _lib()
    m = make_model(3, 128, seed=8)
    with torch.no_grad():
        m.net.bn.weight.mul_(1e5)
    m.engine.mark_dirty()
    boards, players = synth_positions(64, seed=81)
    x = encode_batch(boards, players)
    bi8, pl8 = _i8(boards, players)
    with keys(lib, {K.EVAL_ARITH: 0}):
        p32, v32 = m.predict(x)
        pb32, vb32 = m.predict_boards(bi8, pl8)
    m.set_eval_precision("fp16")
    m.engine.tower_diag_clear()
    p, v = m.predict(x)
    pb, vb = m.predict_boards(bi8, pl8)
    d = m.engine.tower_diag()
    assert d["h3_overflows"] == 2, d
    assert np.array_equal(p, p32) and np.array_equal(v, v32)
    assert np.array_equal(pb, pb32) and np.array_equal(vb, vb32)
    assert lib.azg_pv_status(m.engine.h) == 0


# ---------------------------------------------------------------- 6. timed-out split launch
def test_fp16_timed_out_split_launch_is_rerun_in_fp16():
    """Key 14 = 0 makes the split form's exchange waits time out at once: the launch is
    posted and recover reruns it with one workgroup per board in fp16 (run once).  The recovery
    opens the breaker (key 18 = 30 s): with key 14 still 0 the next forward runs one workgroup
    per board in fp16 -- bitwise, no recovery, no new timeout, one breaker launch -- and after
    clear_status, with healthy waits, the forward is bitwise again and posts nothing."""
    lib = _lib()
    m, boards, players, x, p300, v300 = _mode_case()
    eng = m.engine
    bi8, pl8 = _i8(boards[:3], players[:3])
    with keys(lib, {K.BOARD16_SPLIT_MAX: 0}):
        p0, v0 = m.predict_boards(bi8, pl8)
    eng.clear_status()
    eng.tower_diag_clear()
    r0 = eng.recoveries
    try:
        with keys(lib, {K.BREAKER_SECONDS: 30}):
            with keys(lib, {K.TOWER_WAIT_US: 0}):
                p1, v1 = m.predict_boards(bi8, pl8)
                d = eng.tower_diag()
                assert eng.recoveries == r0 + 1 and d["timeouts"] > 0
                assert np.array_equal(p1, p0) and np.array_equal(v1, v0)
                eng.check_status()
                assert d["breaker_trips"] == 1 and d["breaker_launches"] == 0, d
                p2, v2 = m.predict_boards(bi8, pl8)
                d2 = eng.tower_diag()
                assert np.array_equal(p2, p0) and np.array_equal(v2, v0)
                assert eng.recoveries == r0 + 1, "the forward behind a recovered split launch ran split again"
                assert d2["timeouts"] == d["timeouts"] and d2["breaker_launches"] == 1, (d, d2)
                assert d2["breaker_trips"] == 1 and lib.azg_pv_status(eng.h) == 0
            eng.clear_status()
            p3, v3 = m.predict_boards(bi8, pl8)
            d3 = eng.tower_diag()
            assert np.array_equal(p3, p0) and np.array_equal(v3, v0)
            assert eng.recoveries == r0 + 1 and lib.azg_pv_status(eng.h) == 0
            assert d3["timeouts"] == d["timeouts"] and d3["breaker_launches"] == 1, (d, d3)
            eng.check_status()
    finally:
        eng.clear_status()
        eng.tower_diag_clear()


# ---------------------------------------------------------------- 7. the loop and a player
def test_selfplay_precision_in_the_training_loop(tmp_path, monkeypatch):
    import train
    models, seen, got = [], [], []
    new_model, play = train._new_model, train.selfplay_games

    def recording_new_model(*a, **kw):
        models.append(new_model(*a, **kw))
        return models[-1]

    def recording_selfplay(model, *a, **kw):
        seen.append(model.eval_precision)
        got.append(play(model, *a, **kw))
        return got[-1]

    monkeypatch.setattr(train, "_new_model", recording_new_model)
    monkeypatch.setattr(train, "selfplay_games", recording_selfplay)
    kw = dict(num_iterations=1, games_per_iteration=2, n_simulations=16, batch_size=16, epochs_per_iter=1,
              eval_games=2, eval_mcts_simulations=8, n_res_blocks=2, channels=128, max_moves=6,
              selfplay_precision="fp16")
    best = train.train_alphazero(model_dir=str(tmp_path / "a"), **kw)
    assert seen == ["fp16"]                               # self-play ran in fp16 ...
    examples = got[0][0]
    assert len(examples) > 0
    s, pi, z = examples[0]
    assert np.asarray(s).shape == (3, 15, 15) and np.asarray(pi).shape == (225,) and np.ndim(z) == 0
    assert best.eval_precision == "exact"
    assert [m.eval_precision for m in models] == ["exact"] * len(models)   # ... and every model is exact again

    def failing_selfplay(model, *a, **kw):
        seen.append(model.eval_precision)
        raise RuntimeError("injected self-play failure")

    del models[:]
    monkeypatch.setattr(train, "selfplay_games", failing_selfplay)
    with pytest.raises(RuntimeError, match="injected"):
        train.train_alphazero(model_dir=str(tmp_path / "b"), **kw)
    assert seen[-1] == "fp16" and len(models) == 2
    assert [m.eval_precision for m in models] == ["exact", "exact"]

    with pytest.raises(ValueError, match="selfplay_precision"):
        train.train_alphazero(model_dir=str(tmp_path / "c"), **dict(kw, selfplay_precision="bf16"))


def test_player_with_fp16_precision_plays_a_legal_move():
    from network import PyTorchModel
    from players.player_alpha import Player
    torch.manual_seed(5)
    net = lambda board_size: PyTorchModel(board_size=board_size, device="cuda", n_res_blocks=2, channels=128)
    pl = Player("gomoku", 15, n_simulations=32, model_path=None, nn_model=net, eval_precision="fp16")
    assert pl.net.eval_precision == "fp16"
    board = np.zeros((15, 15), dtype=int)
    board[7, 7] = 1
    r, c = pl.play(board.tolist(), 1, (7, 7))
    assert 0 <= r < 15 and 0 <= c < 15 and board[r, c] == 0
    with pytest.raises(ValueError, match="128 channels"):     # the default 3x64 net has no fp16 form
        Player("gomoku", 15, n_simulations=8, model_path=None, eval_precision="fp16")
