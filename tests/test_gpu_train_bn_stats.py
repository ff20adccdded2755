"""The train step's BatchNorm running stats and counters (running_mean, running_var,
num_batches_tracked of every layer) against an fp64 reference.  They decide every eval
forward (pv_pack.hip folds 1/sqrt(running_var + eps) into the eval scale) and are written
at two sites: bn_fin_out<true> (pv_halo.h; trunk, fused or stand-alone finalize) and
head_stats_fin (pv_train_heads.hip; policy / value BN and every layer's counter).

Every model starts from oracle.randomized_bn_state: distinct non-default stats in every
channel of every layer and counters 3 + layer index, so an old value read at the wrong
channel, layer or offset shows.

Tolerance, per stored element (oracle.bn_stat_tolerance; tests/test_bn_stats_reference.py
shows on the CPU that it sees a biased variance, a shifted channel, a neighbouring layer's
stats and a swapped momentum at B <= 5):

    |gpu - want64| <= 2^-23 * |want64| + 4 * dev32

  * isolated (trunk layers): want64 = bn_update_fp64(the GPU's own raw conv output z, old
    stats), dev32 = the largest deviation over the tensor of torch's float32 mean /
    unbiased var / momentum on the same z.  The conv's rounding is out of the comparison:
    tile partials, fp64 combine, unbiased factor, momentum and indexing are what is left.
  * end to end (every layer): want64 = the buffers of the fp64 masked forward with the
    GPU's own ReLU masks, dev32 = the deviation of the float32 masked forward (same masks,
    inputs, old stats) from it.
  4x: the GPU's convs sum in another order and, under the default train arithmetic, as
  split-fp16 products; its fp64 finalize is otherwise at least as accurate as torch's
  fp32 one.  dev32 never comes from the GPU.  Counters, the restore after a skipped step
  and the eval fold are exact.

The raw conv outputs: the train workspace's z0 / z1[i] / z2[i] are separate allocations
written once per step by the forward conv that produces them (stem_stats, conv3x3_train's
`out`); the fused BN apply of the next conv's staging (key 23, C <= 128) and the separate
bn_apply passes (C = 256) write the activation buffers a0 / hh / xo, and the backward only
reads z.  So under the default schedule keys debug_tensor("z0" / "z1" / "z2") still holds
the pre-BN values when the step ends, and no key is set here.

Measured on an MI355X, default keys (train arithmetic 2), over all CASES, worst
|gpu - want64| / tolerance:
  * isolated 0.14 (1x64, B = 128; |gpu - want64| <= 7e-8 everywhere, dev32 3e-8 .. 1.4e-7 on
    stats of magnitude <= 1.5);
  * end to end 0.69 (policy_bn.running_mean at 1x64, B = 160: |gpu - want64| = 6.4e-9 with
    dev32 = 1.0e-9 on a value of 0.074, so the tolerance there is almost only its
    2^-23 |want64| term); every other tensor <= 0.33.
With q / (M - 1) changed to q / M in both update sites (a one-off build), running_var left
the gate in every case of both reference tests and in the several-steps test: by 115x ..
2000x at B = 2, 70x .. 140x (trunk) at B = 5, and still 1.5x .. 19x at B = 520; running_mean
stayed <= 0.24.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import has_gpu
from _native import TUNE
from oracle.boards import encode_batch, synth_positions, synth_targets
from oracle.ref_net import (RefModel, RefNet, bn_layer_names, bn_stat_tolerance, bn_update_fp64, load_numpy_state,
                            masked_forward_fp64, randomized_bn_state, state_to_numpy)
from test_gpu_train import _full_state, _overflow_model, gpu_masks, make_model, mask_flips

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

# (blocks, channels, B).  B: 2 the smallest batch azg_pv_train_backward accepts (450 rows = 3
# full 128-row tiles + one of 66); 5 a partial last tile; 37 odd; 128 exact tiles only (225);
# 160 the second 256-tile pass of bn_fin_accum with clamped loads; 520 above kHeadFoldMaxB
# (the unfolded head-BN path).  C = 256 finalizes with the two-group 16-wave form.  The
# 2-block case has z1[1], z2[1] and a second block's layer offsets.
CASES = [(1, 64, 2), (1, 64, 5), (1, 64, 37), (1, 64, 128), (1, 64, 160), (1, 64, 520),
         (1, 128, 2), (1, 128, 5), (1, 128, 37), (1, 128, 128),
         (1, 256, 2), (1, 256, 5), (1, 256, 37), (1, 256, 128),
         (2, 64, 37)]
STATS = ("running_mean", "running_var")


def start_state(blocks, ch, seed=None):
    torch.manual_seed(blocks * 1000 + ch)
    return randomized_bn_state(state_to_numpy(RefModel(blocks, ch).net), blocks, seed=blocks * 100 + ch
                               if seed is None else seed)


def batch(B):
    b, p = synth_positions(B, seed=77 + B)
    pi, z = synth_targets(B, seed=78 + B)
    return encode_batch(b, p), pi, z


def gpu_z(eng, blocks, B):
    """{BN layer: the GPU's raw conv output feeding it, [N, C] float32 rows} (trunk)."""
    rows = lambda t: t.reshape(-1, t.shape[-1]).cpu().numpy()
    out = {"bn": rows(eng.debug_tensor("z0", B))}
    for i in range(blocks):
        out[f"res_blocks.{i}.bn1"] = rows(eng.debug_tensor("z1", B, i))
        out[f"res_blocks.{i}.bn2"] = rows(eng.debug_tensor("z2", B, i))
    return out


def isolated_reference(z32, rm0, rv0):
    """(want64 mean, want64 var, dev32 mean, dev32 var) of one layer from the GPU's z."""
    wm, wv = bn_update_fp64(z32, rm0, rv0)
    zt = torch.from_numpy(z32)
    m32 = (1 - 0.1) * torch.from_numpy(np.asarray(rm0, np.float32)) + 0.1 * zt.mean(0)
    v32 = (1 - 0.1) * torch.from_numpy(np.asarray(rv0, np.float32)) + 0.1 * zt.var(0, unbiased=True)
    assert m32.dtype == torch.float32 and v32.dtype == torch.float32
    return wm, wv, float(np.abs(m32.double().numpy() - wm).max()), float(np.abs(v32.double().numpy() - wv).max())


def gpu_buffers(m):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().copy() for k, v in m.net.state_dict().items()
            if "running_" in k or "num_batches_tracked" in k}


def check_isolated(tag, got, old, z, blocks):
    """Every trunk layer's stats vs bn_update_fp64 of the GPU's own z and `old`; returns
    the worst |gpu - want64| / tolerance."""
    worst, bad = 0.0, []
    for n in bn_layer_names(blocks)[:-2]:
        ref = isolated_reference(z[n], old[f"{n}.running_mean"], old[f"{n}.running_var"])
        for s, want, dev32 in zip(STATS, ref[:2], ref[2:]):
            k = f"{n}.{s}"
            assert got[k].dtype == np.float32
            err = np.abs(got[k].astype(np.float64) - want)
            ratio = float((err / bn_stat_tolerance(want, dev32)).max())
            print(f"{tag} isolated {k:32s} |gpu-64|={err.max():.2e} dev32={dev32:.2e} max|want|={np.abs(want).max():.3f} "
                  f"|gpu-64|/tol={ratio:.2f}")
            worst = max(worst, ratio)
            if ratio > 1.0:
                bad.append((k, ratio))
    assert not bad, bad
    return worst


@functools.lru_cache(maxsize=None)
def one_step(blocks, ch, B):
    """One eng.train_backward from a randomized BN state, and everything the two reference
    comparisons need, reduced to stat-sized arrays (computed once per case, read-only)."""
    torch.set_num_threads(max(8, min(16, len(os.sched_getaffinity(0)))))
    st = start_state(blocks, ch)
    m = make_model(blocks, ch, st)
    x, pi, z = batch(B)
    eng = m.engine
    dev = eng.device
    losses = torch.empty(3, device=dev)
    eng.train_backward(torch.from_numpy(x).to(dev), torch.from_numpy(pi).to(dev), torch.from_numpy(z).to(dev), losses)
    torch.cuda.synchronize()
    eng.check_status()
    assert eng.train_skips() == 0
    got = gpu_buffers(m)
    zs = gpu_z(eng, blocks, B)
    mk = gpu_masks(eng, blocks, B)
    # fp64 and fp32 masked forwards with the GPU's masks
    bufs, pre = {}, None
    for dt in (torch.float64, torch.float32):
        net = RefNet(blocks, ch).to(dt)
        load_numpy_state(net, st)
        net.train()
        with torch.no_grad():
            _, _, p, bufs[dt] = masked_forward_fp64(net, x, mk, return_buffers=True, dtype=dt)
        if dt == torch.float64:
            pre = {k: v.numpy() for k, v in p.items()}
    # the mask-flip condition of test_gradients_match_oracle: a flip cannot explain a miss
    nchw = lambda t: t.permute(0, 3, 1, 2).double().cpu().numpy()
    gpu_act = {"a0": nchw(eng.debug_tensor("a0", B))}
    for i in range(blocks):
        gpu_act[f"h{i}"] = nchw(eng.debug_tensor("h", B, i))
        gpu_act[f"xo{i}"] = nchw(eng.debug_tensor("xo", B, i))
    for n_ in ("fp", "fv", "hv"):
        gpu_act[n_] = eng.debug_tensor(n_, B).double().cpu().numpy()
    flips = {}
    for k, (n, worst, mx) in mask_flips(mk, pre).items():
        err = float(np.abs(gpu_act[k] - np.maximum(pre[k], 0)).max())
        flips[k] = (n, worst, mx, err)
    return {"st": st, "got": got, "z": zs, "want64": bufs[torch.float64], "got32": bufs[torch.float32], "flips": flips}


@pytest.mark.parametrize("blocks,ch,B", CASES)
def test_running_stats_from_own_conv_outputs(blocks, ch, B):
    """Trunk BNs, layer-isolated: after one train_backward the stored stats equal
    bn_update_fp64(the GPU's own z of that layer, the old stats) within the isolated
    tolerance (module docstring; the z buffers hold the pre-BN values at the step's end
    under the default keys, so no key is set)."""
    r = one_step(blocks, ch, B)
    worst = check_isolated(f"{blocks}x{ch} B={B}", r["got"], r["st"], r["z"], blocks)
    print(f"{blocks}x{ch} B={B}: worst isolated |gpu-64|/tol = {worst:.2f}")


@pytest.mark.parametrize("blocks,ch,B", CASES)
def test_running_stats_match_fp64_forward(blocks, ch, B):
    """Every BN layer, heads included: the stored stats vs the buffers of the fp64 masked
    forward run with the GPU's own masks, within the end-to-end tolerance; every counter is
    its (per layer distinct) old value + 1.  Mask flips obey test_gradients_match_oracle's
    condition."""
    r = one_step(blocks, ch, B)
    for k, (n, worst, mx, err) in r["flips"].items():
        if n:
            print(f"mask flips {k}: {n} (worst |pre| {worst:.2e} = {worst / mx:.1e} x max), gpu max err {err:.2e}")
        assert worst <= max(1e-6 * mx, 2 * err), (k, n, worst, mx, err)
    got, want64, got32 = r["got"], r["want64"], r["got32"]
    bad, top = [], 0.0
    for i, n in enumerate(bn_layer_names(blocks)):
        k = f"{n}.num_batches_tracked"
        assert int(r["st"][k]) == 3 + i and int(want64[k]) == 4 + i
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want64[k]), (k, got[k], want64[k])
        for s in STATS:
            k = f"{n}.{s}"
            want = want64[k]
            assert want.dtype == np.float64 and got[k].dtype == np.float32 and got32[k].dtype == np.float32
            dev32 = float(np.abs(got32[k].astype(np.float64) - want).max())
            err = np.abs(got[k].astype(np.float64) - want)
            ratio = float((err / bn_stat_tolerance(want, dev32)).max())
            print(f"{blocks}x{ch} B={B} end-to-end {k:32s} |gpu-64|={err.max():.2e} dev32={dev32:.2e} "
                  f"max|want|={np.abs(want).max():.3f} |gpu-64|/tol={ratio:.2f}")
            top = max(top, ratio)
            if ratio > 1.0:
                bad.append((k, ratio))
    print(f"{blocks}x{ch} B={B}: worst end-to-end |gpu-64|/tol = {top:.2f}")
    assert not bad, bad


def test_running_stats_over_several_steps():
    """Three train_batch steps on one model at B = 5, 37, 5 (a change of batch size
    reallocates or regrows nothing that holds stats): after each, the trunk stats equal the
    recurrence bn_update_fp64(that step's GPU z, the GPU's stats before that step) within
    the isolated tolerance, and every counter is old + steps.  train_batch(epochs=3) on a
    second model is bitwise three train_batch calls (each checked the same way)."""
    blocks, ch = 1, 64
    names = bn_layer_names(blocks)
    st = start_state(blocks, ch, seed=11)

    def stepwise(batches):
        m = make_model(blocks, ch, st)
        for step, B in enumerate(batches, 1):
            x, pi, z = batch(B)
            old = gpu_buffers(m)
            m.train_batch(x, pi, z)
            got = gpu_buffers(m)
            check_isolated(f"step {step} B={B}", got, old, gpu_z(m.engine, blocks, B), blocks)
            for i, n in enumerate(names):
                assert int(got[f"{n}.num_batches_tracked"]) == 3 + i + step, (n, step)
            for n in names[-2:]:   # the head stats moved too
                assert not np.array_equal(got[f"{n}.running_var"], old[f"{n}.running_var"])
        return m

    stepwise((5, 37, 5))
    a = stepwise((5, 5, 5))
    b = make_model(blocks, ch, st)
    x, pi, z = batch(5)
    b.train_batch(x, pi, z, epochs=3)
    ga, gb = gpu_buffers(a), gpu_buffers(b)
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    for i, n in enumerate(names):
        assert int(gb[f"{n}.num_batches_tracked"]) == 3 + i + 3


def _set_by_load_state_dict(m, new_bn, new_nbt):
    sd = {k: v.detach().clone() for k, v in m.net.state_dict().items()}
    o = 0
    for i, n in enumerate(bn_layer_names(m.engine.blocks)):
        c = sd[f"{n}.running_mean"].numel()
        sd[f"{n}.running_mean"] = new_bn[o:o + c].clone()
        sd[f"{n}.running_var"] = new_bn[o + c:o + 2 * c].clone()
        sd[f"{n}.num_batches_tracked"] = new_nbt[i].clone()
        o += 2 * c
    m.net.load_state_dict(sd)


def _set_by_copy(m, new_bn, new_nbt):
    with torch.no_grad():
        m.engine.flat_bn.copy_(new_bn)


def _sync_bn_stats(m, new_bn, new_nbt):
    import distributed
    assert distributed.world() == 1
    distributed.sync_bn_stats(m)       # world size 1: touches nothing


def _set_counters_only(m, new_bn, new_nbt):
    bns = [b for b in m.net.modules() if isinstance(b, torch.nn.BatchNorm2d)]
    with torch.no_grad():
        for i, b in enumerate(bns):
            b.num_batches_tracked.fill_(int(new_nbt[i]))


@pytest.mark.parametrize("change,stats_move,counters_move",
                         [(_set_by_load_state_dict, True, True), (_set_by_copy, True, False),
                          (_sync_bn_stats, False, False), (_set_counters_only, False, True)],
                         ids=["load_state_dict", "copy_", "sync_bn_stats", "counters_only"])
def test_stats_changed_from_outside_are_the_ones_a_skipped_step_restores(change, stats_move, counters_move):
    """A skipped step restores the library's copy of the stats and counters (bn_bak /
    nbt_bak, refreshed by every committed step).  Stats set from outside AFTER a commit
    must be the ones it restores, bitwise -- not the commit's.

    The model is test_gpu_train._overflow_model (stem BN gamma x 1e6: the split-fp16 train
    forward skips the step on the device; the project's existing skip mechanism, nothing
    new).  The committed step before it runs on the same model with fp32 forward convs
    (train arithmetic key 49 = 0), under which the net does not leave any range: scaling
    gamma after a commit would itself be a parameter write that refreshes the copy, and the
    outside stat change would no longer be what the test is about.  Then key 49 = 2, the
    change, and the skipped step through train_batch_device as
    test_train_h3_range_overflow_is_redone_in_fp32 does.

    Ways of changing: load_state_dict (stats + counters); in-place copy_ into flat_bn;
    distributed.sync_bn_stats, which at world size 1 is a safe no-op (the restored stats are
    then the commit's own); and the counters alone through the modules'
    num_batches_tracked.  The last writes no flat_bn: engine.sync_dirty watches
    flat_nbt._version for it (it did not, and the skipped step then put the commit's
    counters back)."""
    import _native
    lib = _native.load_library()
    x, pi, z = batch(32)
    prev = lib.azg_pv_set_tuning(TUNE.TRAIN_ARITH, 0)
    try:
        m = _overflow_model()
        eng = m.engine
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            eng.flat_bn.copy_((torch.rand(eng.nbn, generator=g) + 0.5).to(eng.device))
            eng.flat_nbt.copy_((torch.arange(eng.flat_nbt.numel()) + 3).to(eng.device))
        got = m.train_batch(x, pi, z)                # committed, fp32 forward convs
        assert all(np.isfinite(v) for v in got.values()) and eng.train_skips() == 0 and eng.train_recoveries == 0
        committed = _full_state(m)
        lib.azg_pv_set_tuning(TUNE.TRAIN_ARITH, 2)
        new_bn = (torch.rand(eng.nbn, generator=g) + 0.25).to(eng.device)
        new_nbt = (torch.arange(eng.flat_nbt.numel()) * 7 + 100).to(eng.device)
        change(m, new_bn, new_nbt)
        before = _full_state(m)
        bn_c, nbt_c = eng.flat_bn.cpu().clone(), eng.flat_nbt.cpu().clone()
        assert torch.equal(bn_c, new_bn.cpu()) == stats_move
        assert torch.equal(nbt_c, new_nbt.cpu()) == counters_move
        assert all(torch.equal(a, c) for a, c in zip(committed, before)) == (not stats_move and not counters_move)
        dev = eng.device
        xd, pd, zd = (torch.from_numpy(np.asarray(a, np.float32)).to(dev) for a in (x, pi, z.reshape(-1, 1)))
        m.train_batch_device(xd, pd, zd, return_tensor=True)
        torch.cuda.synchronize()
        assert eng.train_skips() == 1
        m._settle_skips()
        after = _full_state(m)
        assert torch.equal(eng.flat_bn.cpu(), bn_c), "a skipped step restored other stats than the ones set from outside"
        assert torch.equal(eng.flat_nbt.cpu(), nbt_c), "a skipped step restored other counters than the ones set"
        assert all(torch.equal(a, c) for a, c in zip(before, after)), "a skipped step changed the model"
        eng.clear_status()
    finally:
        lib.azg_pv_set_tuning(TUNE.TRAIN_ARITH, prev)


def test_eval_reads_the_trained_stats():
    """After two train steps predict() is bitwise predict() of a fresh model that loads the
    trained state: the eval fold is redone from the new stats (no stale pack)."""
    blocks, ch = 1, 64
    m = make_model(blocks, ch, start_state(blocks, ch, seed=21))
    x, pi, z = batch(37)
    p0, v0 = m.predict(x)
    for _ in range(2):
        m.train_batch(x, pi, z)
    p1, v1 = m.predict(x)
    fresh = make_model(blocks, ch, state_to_numpy(m.net), seed=9)
    p2, v2 = fresh.predict(x)
    assert not np.array_equal(p0, p1)
    assert np.array_equal(p1, p2) and np.array_equal(v1, v2)
    # and the stats it folded are not the ones it started from
    old = start_state(blocks, ch, seed=21)
    assert not np.array_equal(gpu_buffers(m)["bn.running_var"], old["bn.running_var"])
