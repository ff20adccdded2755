"""The weight average (EMA) kept inside the Adam kernel (include/azg_pv.h azg_pv_bind_ema,
PyTorchModel(ema_decay=...), train_alphazero(ema_decay=...)).

Nets are 2x64 and 1x128 at B = 16: 1x128 has about 0.4 M parameters, more than the 262,144
threads of the Adam grid, so the kernel's grid-stride loop takes a second trip.

The update rule is checked step by step against the GPU's OWN previous average e and its own
new parameter or running stat p': want = e + w (p' - e) in float64 with w the fp32 weight, and
|e'_gpu - want| <= 2 * 2^-23 * max(|e|, |p'|) elementwise.  The bound is derived, not measured:
the update has at most three fp32 roundings -- the difference (<= 1/2 ulp of 2 max), the
product (of a value scaled by w <= 1/2 at the decays used) and the sum (<= 1/2 ulp of max) --
together <= 1.5 * 2^-23 * max, and with fmaf (one rounding for product and sum) less."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import PKG, REPO, has_gpu
from _native import TUNE
from oracle.boards import encode_batch, synth_positions, synth_targets

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

B, STEPS = 16, 6
NETS = {"2x64": (2, 64), "1x128": (1, 128)}


def _model(blocks, ch, seed=0, **kw):
    from network import PyTorchModel
    torch.manual_seed(seed)
    return PyTorchModel(board_size=15, device="cuda", n_res_blocks=blocks, channels=ch, **kw)


def _batch(step, n=B):
    b, p = synth_positions(n, seed=300 + step)
    pi, z = synth_targets(n, seed=400 + step)
    return encode_batch(b, p), pi, z


def _snap(m):
    eng = m.engine
    torch.cuda.synchronize()
    return {k: getattr(eng, "flat_" + k).cpu().numpy().copy() for k in ("params", "bn", "ema", "ema_bn")}


def _check_update(tag, e, x_new, e_new, w):
    """e_new against e + w (x_new - e) in float64; prints the worst error in units of the bound."""
    e64, x64 = e.astype(np.float64), x_new.astype(np.float64)
    want = e64 + float(w) * (x64 - e64)
    bound = 2.0 * 2.0 ** -23 * np.maximum(np.abs(e64), np.abs(x64))
    err = np.abs(e_new.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{tag}: worst |gpu - want| / bound = {worst:.3f} over {e.size} elements")
    assert (err <= bound).all(), (tag, worst, int((err > bound).sum()))


# ------------------------------------------------------------ 1. the update rule, step by step
@pytest.mark.parametrize("decay", [0.9, 0.999])
@pytest.mark.parametrize("net", list(NETS))
def test_update_rule_step_by_step(net, decay):
    m = _model(*NETS[net], seed=1, ema_decay=decay)
    eng = m.engine
    assert m.ema_decay == decay and eng.flat_ema.numel() == eng.nparam and eng.flat_ema_bn.numel() == eng.nbn
    w = np.float32(1.0 - float(np.float32(decay)))          # the library's (float)(1.0 - (double)decay)
    assert eng.ema_weight() == float(w)
    if net == "1x128":
        assert eng.nparam > 1024 * 256                       # a second trip of the grid-stride loop
    prev = _snap(m)
    assert np.array_equal(prev["ema"], prev["params"]) and np.array_equal(prev["ema_bn"], prev["bn"])
    start = prev
    for s in range(STEPS):
        m.train_batch(*_batch(s))
        cur = _snap(m)
        _check_update(f"{net} decay {decay} step {s} params", prev["ema"], cur["params"], cur["ema"], w)
        _check_update(f"{net} decay {decay} step {s} bn", prev["ema_bn"], cur["bn"], cur["ema_bn"], w)
        # it moved, and it is an average: not the parameters
        assert not np.array_equal(cur["ema"], prev["ema"]) and not np.array_equal(cur["ema_bn"], prev["ema_bn"])
        assert not np.array_equal(cur["ema"], cur["params"]) and not np.array_equal(cur["ema_bn"], cur["bn"])
        prev = cur
    assert not np.array_equal(prev["ema"], start["ema"])


# ------------------------------------------------------------ 2. EMA does not touch training
@pytest.mark.parametrize("net", list(NETS))
def test_ema_does_not_touch_training(net):
    def run(**kw):
        m = _model(*NETS[net], seed=2, **kw)
        losses = [m.train_batch(*_batch(s)) for s in range(STEPS)]
        torch.cuda.synchronize()
        eng, opt = m.engine, m.optimizer
        return losses, {"params": eng.flat_params.cpu(), "bn": eng.flat_bn.cpu(), "nbt": eng.flat_nbt.cpu(),
                        "m": opt.flat_exp_avg.cpu(), "v": opt.flat_exp_avg_sq.cpu(),
                        "step": torch.tensor([opt.get_step()])}
    l0, s0 = run()
    l1, s1 = run(ema_decay=0.9)
    assert l0 == l1, (l0, l1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    assert int(s0["step"][0]) == STEPS and int(s0["nbt"][0]) == STEPS


# ------------------------------------------------------------ 3. skipped steps
def test_skipped_step_does_not_move_the_average():
    """The recipe of test_gpu_train.test_train_h3_range_overflow_is_redone_in_fp32: stem BN
    gamma x 1e6, beta + 1e5 drives every staged activation of the first split-fp16 train conv
    (key 49 = 2) beyond fp16's range, so the device skips the step."""
    import _native
    lib = _native.load_library()
    b, p = synth_positions(32, seed=91)
    x = encode_batch(b, p)
    pi, z = synth_targets(32, seed=92)
    decay = 0.9
    w = np.float32(1.0 - float(np.float32(decay)))
    m = _model(2, 64, seed=5, ema_decay=decay)
    prev49 = lib.azg_pv_set_tuning(TUNE.TRAIN_ARITH, 2)
    try:
        with torch.no_grad():
            m.net.bn.weight.mul_(1e6)
            m.net.bn.bias.add_(1e5)
        m.engine.mark_dirty()
        m.reset_ema()                                       # weights changed through torch
        before = _snap(m)
        assert np.array_equal(before["ema"], before["params"]) and np.array_equal(before["ema_bn"], before["bn"])
        # a pipelined step the device skips: nobody waits for it, and the average stays bitwise
        dev = m.engine.device
        xd, pd, zd = (torch.from_numpy(np.asarray(a, np.float32)).to(dev) for a in (x, pi, z.reshape(-1, 1)))
        m.train_batch_device(xd, pd, zd, return_tensor=True)
        torch.cuda.synchronize()
        assert m.engine.train_skips() == 1
        m._settle_skips()
        after = _snap(m)
        for k in before:
            assert np.array_equal(before[k], after[k]), f"a skipped step changed {k}"
        # the synchronous step: skipped on the device, redone in fp32 -- ONE move of the average,
        # towards the committed parameters and stats
        got = m.train_batch(x, pi, z)
        assert all(np.isfinite(v) for v in got.values()), got
        assert m.engine.train_recoveries == 1 and m.engine.train_skips() == 2
        cur = _snap(m)
        assert not np.array_equal(cur["params"], before["params"])
        _check_update("redone step params", before["ema"], cur["params"], cur["ema"], w)
        _check_update("redone step bn", before["ema_bn"], cur["bn"], cur["ema_bn"], w)
        assert not np.array_equal(cur["ema"], before["ema"]) and not np.array_equal(cur["ema_bn"], before["ema_bn"])
    finally:
        m.engine.clear_status()
        lib.azg_pv_set_tuning(TUNE.TRAIN_ARITH, prev49)


# ------------------------------------------------------------ 4. reading the average
def test_reading_the_average():
    m = _model(1, 128, seed=3, ema_decay=0.9)
    for s in range(3):
        m.train_batch(*_batch(s))
    x = _batch(60, 8)[0]

    def fresh_prediction():
        f = _model(1, 128, seed=77)
        f.net.load_state_dict(m.ema_state_dict())
        return f.predict(x)

    sd, live = m.ema_state_dict(), m.net.state_dict()
    assert list(sd) == list(live)
    for k in live:
        assert sd[k].shape == live[k].shape and sd[k].dtype == live[k].dtype and sd[k].device == live[k].device, k
        assert sd[k].data_ptr() != live[k].data_ptr()                      # clones
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(live[k]) == 3, k                      # the live counters
    assert not torch.equal(sd["conv.weight"], live["conv.weight"])
    assert not torch.equal(sd["bn.running_mean"], live["bn.running_mean"])

    twin = m.ema_model()
    assert twin is not m and twin.ema_decay is None and twin.engine.flat_ema is None
    p_twin, v_twin = twin.predict(x)
    p_fresh, v_fresh = fresh_prediction()
    assert np.array_equal(p_twin, p_fresh) and np.array_equal(v_twin, v_fresh)
    p_live, v_live = m.predict(x)
    assert not np.array_equal(p_twin, p_live) and not np.array_equal(v_twin, v_live)

    for s in range(3, 5):                                                  # two more steps: a new average
        m.train_batch(*_batch(s))
    assert np.array_equal(twin.predict(x)[0], p_twin)                      # the twin moves only when asked
    twin2 = m.ema_model()
    assert twin2 is twin                                                   # cached, refreshed in place
    p2, v2 = twin2.predict(x)
    p2_fresh, v2_fresh = fresh_prediction()
    assert np.array_equal(p2, p2_fresh) and np.array_equal(v2, v2_fresh)
    assert not np.array_equal(p2, p_twin)

    # the twin's eval precision is its own
    assert m.eval_precision == "exact" and twin.eval_precision == "exact"
    m.set_eval_precision("fp16")
    assert m.ema_model().eval_precision == "exact"
    m.set_eval_precision("exact")
    twin.set_eval_precision("fp16")
    assert m.eval_precision == "exact" and m.ema_model().eval_precision == "fp16"
    twin.set_eval_precision("exact")

    off = _model(2, 64, seed=4)
    assert off.ema_decay is None and off.engine.flat_ema is None and off.engine.flat_ema_bn is None
    with pytest.raises(RuntimeError, match="EMA is off"):
        off.ema_state_dict()
    with pytest.raises(RuntimeError, match="EMA is off"):
        off.ema_model()
    # enable / disable on a live model
    off.enable_ema(0.5)
    assert off.ema_decay == 0.5 and torch.equal(off.engine.flat_ema, off.engine.flat_params)
    off.disable_ema()
    assert off.ema_decay is None and off.engine.flat_ema is None
    with pytest.raises(RuntimeError, match="EMA is off"):
        off.ema_state_dict()


# ------------------------------------------------------------ 5. checkpoints
def test_checkpoints(tmp_path):
    from oracle.ref_net import RefNet
    REF_KEYS = {"net", "opt", "board_size", "action_size"}
    m = _model(2, 64, seed=6, ema_decay=0.9)
    for s in range(2):
        m.train_batch(*_batch(s))
    ema_path, plain_path = str(tmp_path / "ema.pt"), str(tmp_path / "plain.pt")
    m.save(ema_path)
    state = torch.load(ema_path, map_location="cpu", weights_only=True)
    assert set(state) == REF_KEYS | {"ema"} and set(state["ema"]) == {"decay", "net"}
    assert state["ema"]["decay"] == 0.9 and list(state["ema"]["net"]) == list(state["net"])
    want = _snap(m)

    # round trip with EMA on: the average bitwise, the decay kept
    r = _model(2, 64, seed=7, ema_decay=0.9)
    r.train_batch(*_batch(9))                                # its own, different average first
    r.load(ema_path)
    got = _snap(r)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert r.ema_decay == 0.9
    assert not np.array_equal(got["ema"], got["params"])

    # an EMA checkpoint into a model without EMA: the key is ignored
    plain = _model(2, 64, seed=8)
    plain.load(ema_path)
    torch.cuda.synchronize()
    assert np.array_equal(plain.engine.flat_params.cpu().numpy(), want["params"])
    assert plain.ema_decay is None and plain.engine.flat_ema is None

    # EMA off: exactly the reference's four keys
    plain.save(plain_path)
    assert set(torch.load(plain_path, map_location="cpu", weights_only=True)) == REF_KEYS

    # a plain checkpoint into a model with EMA: the average resets to the loaded weights
    e = _model(2, 64, seed=9, ema_decay=0.99)
    e.train_batch(*_batch(10))
    e.load(plain_path)
    got = _snap(e)
    assert np.array_equal(got["params"], want["params"]) and np.array_equal(got["bn"], want["bn"])
    assert np.array_equal(got["ema"], got["params"]) and np.array_equal(got["ema_bn"], got["bn"])
    assert e.ema_decay == 0.99

    # the reference's loader reads state["net"] (and "opt") only
    ref = RefNet(2, 64)
    ref.load_state_dict(state["net"])
    assert np.array_equal(ref.conv.weight.detach().numpy().ravel(), want["params"][:64 * 27])


# ------------------------------------------------------------ 6. the loop
def test_ema_in_the_training_loop(tmp_path, monkeypatch):
    import train
    models, gated = [], []
    new_model = train._new_model

    def recording_new_model(*a, **kw):
        models.append(new_model(*a, **kw))
        return models[-1]

    def accepting_evaluate(model_new, model_best, game_name="gomoku", n_games=2, **kw):
        gated.append((model_new, model_best))
        return n_games, 1.0, 0

    monkeypatch.setattr(train, "_new_model", recording_new_model)
    monkeypatch.setattr(train, "evaluate_models", accepting_evaluate)
    kw = dict(num_iterations=1, games_per_iteration=2, n_simulations=16, batch_size=16, epochs_per_iter=1,
              eval_games=2, eval_mcts_simulations=8, n_res_blocks=2, channels=64, max_moves=6)
    hist = []
    best = train.train_alphazero(model_dir=str(tmp_path / "a"), ema_decay=0.9, history=hist, **kw)
    assert len(models) == 3 and best is models[0] and len(gated) == 1
    cand = models[1]                                         # the iteration's candidate
    assert cand.ema_decay == 0.9 and cand.optimizer.get_step() > 0
    assert gated[0][0] is cand.ema_model() and gated[0][0] is not cand and gated[0][1] is best
    want, live, got = cand.ema_state_dict(), cand.net.state_dict(), best.net.state_dict()
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k               # best took the averaged weights ...
    assert not torch.equal(got["conv.weight"], live["conv.weight"])   # ... not the raw ones
    assert best.optimizer.get_step() == cand.optimizer.get_step()     # with the candidate's optimiser state
    assert torch.equal(best.optimizer.flat_exp_avg, cand.optimizer.flat_exp_avg)
    assert best.ema_decay is None
    nxt = models[2]                                          # the next candidate: averaging from best's weights
    assert nxt.ema_decay == 0.9 and torch.equal(nxt.engine.flat_ema, nxt.engine.flat_params)
    assert torch.equal(nxt.engine.flat_params, best.engine.flat_params)
    assert [h["ema_decay"] for h in hist] == [0.9]

    del models[:], gated[:], hist[:]
    train.train_alphazero(model_dir=str(tmp_path / "b"), history=hist, **kw)
    assert len(models) == 3 and all(mm.engine.flat_ema is None and mm.ema_decay is None for mm in models)
    assert gated[0][0] is models[1]                          # without EMA the raw candidate is gated
    assert [h["ema_decay"] for h in hist] == [None]

    with pytest.raises(ValueError, match="ema_decay"):
        train.train_alphazero(model_dir=str(tmp_path / "c"), ema_decay=1.0, **kw)


# ------------------------------------------------------------ 7. data parallel
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_worker(rank, world, port, out_dir):
    import sys
    sys.path[:0] = [REPO, PKG]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    torch.set_num_threads(1)
    torch.distributed.init_process_group("gloo")
    import distributed as D
    from network import PyTorchModel
    torch.manual_seed(rank)                                  # replicas start different
    m = PyTorchModel(board_size=15, device="cuda:0", n_res_blocks=2, channels=64, ema_decay=0.9)
    if rank == 1:                                            # and rank 1's average has moved already
        m.train_batch(*_batch(70))
    out = {"pre_" + k: v for k, v in _snap(m).items()}
    D.broadcast_model(m, 0)
    out.update({"bc_" + k: v for k, v in _snap(m).items()})
    m.grad_hook = D.grad_hook()
    for s in range(4):
        m.train_batch(*_batch(100 + 10 * s + rank))          # rank-local batches
    out.update({"trained_" + k: v for k, v in _snap(m).items()})
    D.sync_bn_stats(m)
    out.update({"synced_" + k: v for k, v in _snap(m).items()})
    np.savez(os.path.join(out_dir, f"ema_rank{rank}.npz"), **out)
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
def test_dp_average_stays_equal_across_ranks(tmp_path):
    """World 2 over gloo, both ranks on this GPU (the pattern of test_gpu_distributed.py)."""
    port = _free_port()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (dict(np.load(tmp_path / f"ema_rank{r}.npz")) for r in range(2))
    # broadcast_model: a rank with a different average becomes rank 0
    assert not np.array_equal(r0["pre_ema"], r1["pre_ema"]) and not np.array_equal(r0["pre_ema_bn"], r1["pre_ema_bn"])
    for k in ("params", "bn", "ema", "ema_bn"):
        assert np.array_equal(r0["bc_" + k], r1["bc_" + k]), k
        assert np.array_equal(r0["bc_" + k], r0["pre_" + k]), k
    # after 4 DP steps the averaged parameters are bitwise equal without communication ...
    assert np.array_equal(r0["trained_params"], r1["trained_params"])
    assert np.array_equal(r0["trained_ema"], r1["trained_ema"])
    assert not np.array_equal(r0["trained_ema"], r0["trained_params"])
    # ... the averaged running stats are rank-local until sync_bn_stats mean-reduces them
    assert not np.array_equal(r0["trained_ema_bn"], r1["trained_ema_bn"])
    assert np.array_equal(r0["synced_ema_bn"], r1["synced_ema_bn"]) and np.array_equal(r0["synced_bn"], r1["synced_bn"])
    mean = (r0["trained_ema_bn"].astype(np.float64) + r1["trained_ema_bn"]) / 2
    assert np.abs(r0["synced_ema_bn"] - mean).max() <= 2.0 ** -23 * np.abs(mean).max()
    assert np.array_equal(r0["synced_ema"], r0["trained_ema"])
