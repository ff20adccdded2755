"""The clip + Adam step on the GPU (csrc/pv_train.hip adam_kernel through HipAdam.hip_step /
azg_pv_train_apply), gated element by element against float64 (oracle/adam_reference.py).

Known data goes straight into the bound flat buffers -- parameters, gradients, both moments --
the step runs once, and every output (total_norm, the clipped grads written back, m', v', p') is
held against float64 computed from the device's OWN inputs, within bounds counted from the
roundings of the operation (adam_gate; derived there, checked against a faithful fp32 emulation
and eight subtly wrong steps in tests/test_adam_reference.py).  Every element of every buffer is
gated; the worst err / bound per quantity is printed, and is a reported figure, not a threshold.

The kernel sees only nparam.  Its grid is at most 1024 workgroups of 256 threads:
  1x64   less than one grid pass, the last workgroup partial;
  1x128  a partial second trip of the grid-stride loop;
  2x256  about ten trips."""
import math

import numpy as np
import pytest
import torch

from conftest import has_gpu
from _native import TUNE
from oracle.adam_reference import CASES, adam_gate, make_case, zero_block
from oracle.boards import encode_batch, synth_positions, synth_targets

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

GRID = 1024 * 256
NETS = {"1x64": (1, 64), "1x128": (1, 128), "2x256": (2, 256)}
QUANTITIES = ("tn", "g", "m", "v", "p")
_models = {}


def _new_model(blocks, ch, seed=0):
    from network import PyTorchModel
    torch.manual_seed(seed)
    return PyTorchModel(board_size=15, device="cuda", n_res_blocks=blocks, channels=ch)


def _model(net):
    """One model per net for the cases that overwrite every buffer the step reads."""
    if net not in _models:
        _models[net] = _new_model(*NETS[net])
    m = _models[net]
    n = m.engine.nparam
    if net == "1x64":
        assert n < GRID and n % 256 != 0
    elif net == "1x128":
        assert GRID < n < 2 * GRID
    else:
        assert n > 4 * GRID
    return m


def _put(dst, a):
    dst.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dst.device))


def _inject(m, data, hyper, step):
    """The case's p, g, m, v into the flat buffers, its step count and hyper-parameters into the
    optimizer (state first: creating it zeroes the moments)."""
    eng, opt = m.engine, m.optimizer
    opt.set_step(step - 1)
    for dst, a in zip((eng.flat_params, eng.flat_grads, opt.flat_exp_avg, opt.flat_exp_avg_sq), data):
        _put(dst, a)
    g = opt.param_groups[0]
    g["lr"], g["betas"], g["eps"], g["weight_decay"] = hyper["lr"], tuple(hyper["betas"]), hyper["eps"], hyper["wd"]


def _snap(m):
    eng, opt = m.engine, m.optimizer
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().copy() for t in (eng.flat_params, eng.flat_grads, opt.flat_exp_avg,
                                                  opt.flat_exp_avg_sq))


def _hyper(opt):
    g = opt.param_groups[0]
    return dict(lr=g["lr"], betas=g["betas"], eps=g["eps"], wd=g["weight_decay"])


def _gated_step(tag, m, max_norm, plain=False):
    """One hip_step from the buffers as they are, gated.  -> (before, after)."""
    eng, opt = m.engine, m.optimizer
    assert float(eng.flat_grads_ext[-1]) == 0.0                 # the skip word: the step commits
    step = opt.get_step() + 1
    before = _snap(m)
    t = torch.full((1,), -1.0, dtype=torch.float32, device=eng.device)
    opt.hip_step(max_norm, total_norm=t)
    after = _snap(m) + (t.cpu().numpy(),)
    assert opt.get_step() == step
    assert all(np.isfinite(a).all() for a in after), tag
    res = adam_gate(before, after, step, _hyper(opt), max_norm)
    print(f"{tag} n={eng.nparam} step {step}: worst err/bound " + "  ".join(f"{q} {res[q][0]:.3f}" for q in QUANTITIES))
    for q in QUANTITIES:
        assert res[q][1] == 0, (tag, q, res[q])
    return before, after


# ------------------------------------------------------------ 1. the cases, on every net
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("net", list(NETS))
def test_step_against_fp64(net, name):
    m = _model(net)
    n = m.engine.nparam
    data, hyper, step, max_norm = make_case(name, n)
    _inject(m, data, hyper, step)
    before, after = _gated_step(f"{net} {name}", m, max_norm)
    for a, b in zip(before, data):
        assert np.array_equal(a, b)
    p, g, mm, v = before
    p1, g1, m1, v1, tn = after
    c = CASES[name]
    if math.isinf(max_norm) or name in ("defaults step 1", "norm 1.5"):
        assert np.array_equal(g1.view(np.uint32), g.view(np.uint32))       # coef is exactly 1
    if name in ("clipped hard step 7", "norm 3.2", "norm just under", "spike"):
        assert float(tn[0]) > max_norm or name == "norm just under"
        assert not np.array_equal(g1, g)                                   # the clip is active
    if "norm" in c:
        assert abs(float(tn[0]) - c["norm"]) <= 2.0 ** -23 * c["norm"]
    if name == "zeros":
        z = zero_block(n)
        assert np.array_equal(p1[z].view(np.uint32), p[z].view(np.uint32))
        assert not m1[z].any() and not v1[z].any() and not g1[z].any()
        assert not np.array_equal(p1, p)
    if name == "spike":
        z = zero_block(n)
        big = g == np.float32(1e15)
        assert big.sum() == 16 and abs(float(tn[0]) / 4e15 - 1.0) < 1e-6
        assert (np.abs(g1[~big]) < 1e-17).all() and (np.abs(g1[big]) > 0.7).all()
        assert (g1[z][~big[z]] > 0).all()                                  # 1e-20 clipped: ~7.5e-36, not flushed


def test_gate_rejects_the_device_step_under_wrong_constants():
    """Negative control on device data: the step the GPU took at step 7 with L2 weight decay
    does not pass as step 6, as a step without weight decay, or as a step clipped to another
    norm -- the gate tells these apart on the GPU's own buffers, not only on the emulation's."""
    m = _model("1x128")
    data, hyper, step, max_norm = make_case("clipped hard step 7", m.engine.nparam)
    _inject(m, data, hyper, step)
    before, after = _gated_step("1x128 negative control", m, max_norm)
    as_step_6 = adam_gate(before, after, step - 1, hyper, max_norm)
    assert as_step_6["p"][1] > 0 and as_step_6["p"][0] >= 2.0, as_step_6
    no_wd = adam_gate(before, after, step, dict(hyper, wd=0.0), max_norm)
    assert no_wd["m"][1] > 0 and no_wd["m"][0] >= 2.0, no_wd
    other_norm = adam_gate(before, after, step, hyper, max_norm * (1.0 + 2.0 ** -20))
    assert other_norm["g"][1] > 0, other_norm


# ------------------------------------------------------------ 2. several steps, lr changing
def test_six_steps_with_a_changing_lr():
    m = _new_model(*NETS["1x128"], seed=11)
    eng, opt = m.engine, m.optimizer
    assert eng.nparam > GRID
    rng = np.random.default_rng(21)
    assert opt.get_step() == 0
    lr0 = opt.param_groups[0]["lr"]
    first = None
    for s in range(1, 7):
        # fresh gradients: the first unclipped, then alternately clipped and not
        _put(eng.flat_grads, ((1e-3, 2e-2)[s % 2 == 0] * rng.standard_normal(eng.nparam)).astype(np.float32))
        before, after = _gated_step(f"1x128 run step {s}", m, 3.0)
        assert opt.get_step() == s
        if s > 1:                                       # the state the previous step left, bitwise
            assert all(np.array_equal(before[i], prev[j]) for i, j in ((0, 0), (2, 2), (3, 3)))
        first = first or before
        prev = after
        if s == 3:
            opt.param_groups[0]["lr"] = lr0 / 2         # as a scheduler would
    assert opt.param_groups[0]["lr"] == lr0 / 2 and not np.array_equal(prev[0], first[0])


# ------------------------------------------------------------ 3. torch-format optimizer state
def test_torch_format_state():
    m = _new_model(*NETS["1x128"], seed=12)
    eng, opt = m.engine, m.optimizer
    gen = torch.Generator().manual_seed(31)
    src_params = [torch.nn.Parameter(torch.zeros(p.shape)) for p in eng.params]
    src = torch.optim.Adam(src_params, lr=5e-4, weight_decay=1e-4)
    for p in src_params:
        src.state[p] = {"step": torch.tensor(57.0), "exp_avg": 1e-3 * torch.randn(p.shape, generator=gen),
                        "exp_avg_sq": 1e-6 * torch.rand(p.shape, generator=gen)}
    sd = src.state_dict()
    opt.load_state_dict(sd)
    assert opt.get_step() == 57 and opt.param_groups[0]["lr"] == 5e-4
    fm, fv = opt.flat_exp_avg.cpu(), opt.flat_exp_avg_sq.cpu()
    covered = 0
    for i, p in enumerate(eng.params):
        o, k = int(eng.param_views[i].storage_offset()), p.numel()
        assert torch.equal(fm[o:o + k], sd["state"][i]["exp_avg"].reshape(-1)), i
        assert torch.equal(fv[o:o + k], sd["state"][i]["exp_avg_sq"].reshape(-1)), i
        covered += k
    assert covered == eng.nparam
    _put(eng.flat_grads, (1e-3 * np.random.default_rng(32).standard_normal(eng.nparam)).astype(np.float32))
    _gated_step("1x128 loaded state", m, 3.0)
    out = opt.state_dict()
    fm, fv = opt.flat_exp_avg.cpu(), opt.flat_exp_avg_sq.cpu()
    assert len(out["state"]) == len(eng.params)
    for i, p in enumerate(eng.params):
        o, k = int(eng.param_views[i].storage_offset()), p.numel()
        st = out["state"][i]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert torch.equal(st["exp_avg"].cpu().reshape(-1), fm[o:o + k]), i
        assert torch.equal(st["exp_avg_sq"].cpu().reshape(-1), fv[o:o + k]), i
        assert float(st["step"]) == 58.0, i
        assert not torch.equal(st["exp_avg"].cpu(), sd["state"][i]["exp_avg"]), i     # the step moved it
    assert all(float(src.state[p]["step"]) == 57.0 for p in src_params)               # the source is untouched
    assert all(float(sd["state"][i]["step"]) == 57.0 for i in range(len(src_params)))


# ------------------------------------------------------------ 4. the repack behind Adam
@pytest.mark.parametrize("keys", [{}, {TUNE.EVAL_ARITH: 1, TUNE.TRAIN_ARITH: 0}], ids=["default keys", "eval 1 train 0"])
@pytest.mark.parametrize("net", ["2x64", "1x128"])
def test_packs_behind_adam_are_cold_packs(net, keys):
    """train_apply packs the next step's train weights and the eval BN fold right behind Adam.
    A fresh model that loads the stepped model's state_dict packs them cold: predictions, and
    the next train_backward's gradients, losses and running stats, must be bitwise the same."""
    import _native
    lib = _native.load_library()
    blocks, ch = {"2x64": (2, 64), "1x128": (1, 128)}[net]
    B = 16
    b, p = synth_positions(B, seed=500)
    x = encode_batch(b, p)
    pi, z = synth_targets(B, seed=501)
    xb = encode_batch(*synth_positions(37, seed=502))
    prev = {k: lib.azg_pv_set_tuning(k, v) for k, v in keys.items()}
    try:
        hot = _new_model(blocks, ch, seed=13)
        p0 = hot.engine.flat_params.cpu()
        got = hot.train_batch(x, pi, z)
        assert all(np.isfinite(v) for v in got.values()) and hot.engine.train_recoveries == 0
        assert not torch.equal(hot.engine.flat_params.cpu(), p0)
        cold = _new_model(blocks, ch, seed=14)
        cold.net.load_state_dict(hot.net.state_dict())
        for k in ("flat_params", "flat_bn", "flat_nbt"):
            assert torch.equal(getattr(hot.engine, k), getattr(cold.engine, k)), k
        ph, vh = hot.predict(xb)
        pc, vc = cold.predict(xb)
        assert np.array_equal(ph, pc) and np.array_equal(vh, vc)
        out = []
        for mdl in (hot, cold):
            eng = mdl.engine
            dev = eng.device
            losses = torch.empty(3, dtype=torch.float32, device=dev)
            eng.train_backward(torch.from_numpy(x).to(dev), torch.from_numpy(pi).to(dev),
                               torch.from_numpy(z.astype(np.float32).reshape(-1, 1)).to(dev), losses)
            torch.cuda.synchronize()
            out.append((eng.flat_grads_ext.cpu(), losses.cpu(), eng.flat_bn.cpu(), eng.flat_nbt.cpu()))
        assert float(out[0][0][-1]) == 0.0                       # no skipped step in the comparison
        assert out[0][0].abs().max() > 0 and torch.isfinite(out[0][1]).all()
        for a, c, what in zip(out[0], out[1], ("flat_grads", "losses", "flat_bn", "flat_nbt")):
            assert torch.equal(a, c), what
    finally:
        for k, v in prev.items():
            lib.azg_pv_set_tuning(k, v)
