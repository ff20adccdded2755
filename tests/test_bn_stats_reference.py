"""The fp64 reference of the train step's BN running-stat update (oracle.bn_update_fp64,
masked_forward_fp64(return_buffers=True)) and the tolerance that tests/test_gpu_train_bn_stats.py
gates the GPU with, checked without a GPU:

  * bn_update_fp64 == torch.nn.BatchNorm2d in double, train mode, to 1e-14 relative;
  * the gate can see the bugs it is for.  Per stored element the gate is
        |got - want64| <= 2^-23 * |want64| + 4 * dev32
    with dev32 the largest deviation, over that tensor, of the float32 masked forward
    (same masks, inputs and old stats) from the fp64 one.  With the fp32 forward standing
    in for the GPU, the unmutated fp32 run stays inside it, and each mutant of the fp64
    reference leaves it in every BN layer it can differ in:
      (a) biased variance;  (b) old stats read one channel over;  (c) old stats of the
      neighbouring BN layer;  (d) momentum on the wrong term (0.9 / 0.1 swapped).
    (a) changes running_var only.  (b) is the identity on value_bn (one channel) and (c)
    needs a neighbour of the same channel count (the trunk layers), so those layers are
    not asserted for those mutants.

Every net starts from randomized_bn_state (distinct non-default stats and counters).
The mutant assertion stops at B = 5: the biased-variance shift is 0.1 * var / (N - 1),
about 15x the tolerance at B = 5 and only about 2.5x at B = 37.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.boards import encode_batch, synth_positions
from oracle.ref_net import (RefModel, RefNet, bn_layer_names, bn_stat_tolerance, bn_update_fp64, load_numpy_state,
                            masked_forward_fp64, randomized_bn_state, state_to_numpy)


@pytest.mark.parametrize("n,c,shape", [(450, 64, "nchw"), (8325, 128, "nchw"), (450, 3, "rows")])
def test_bn_update_matches_torch_double(n, c, shape):
    rng = np.random.default_rng(n + c)
    rm0, rv0 = rng.uniform(-0.5, 0.5, c), rng.uniform(0.5, 1.5, c)
    z = rng.normal(0.3, 1.7, (n // 225, c, 15, 15)) * rng.uniform(0.2, 3.0, (1, c, 1, 1))
    bn = torch.nn.BatchNorm2d(c).double().train()
    with torch.no_grad():
        bn.running_mean.copy_(torch.from_numpy(rm0))
        bn.running_var.copy_(torch.from_numpy(rv0))
        bn(torch.from_numpy(z))
    arg = z if shape == "nchw" else z.transpose(0, 2, 3, 1).reshape(-1, c)
    rm, rv = bn_update_fp64(arg, rm0, rv0)
    assert rm.dtype == np.float64 and rv.dtype == np.float64
    np.testing.assert_allclose(rm, bn.running_mean.numpy(), rtol=1e-14, atol=0)
    np.testing.assert_allclose(rv, bn.running_var.numpy(), rtol=1e-14, atol=0)


def test_randomized_bn_state_is_distinct_per_layer_and_channel():
    st = randomized_bn_state(state_to_numpy(RefNet(2, 64)), 2, seed=4)
    names = bn_layer_names(2)
    assert [n for n in names if f"{n}.running_mean" in st] == names and len(names) == 7
    for i, n in enumerate(names):
        rm, rv = st[f"{n}.running_mean"], st[f"{n}.running_var"]
        assert rm.dtype == np.float32 and rv.dtype == np.float32
        assert (np.abs(rm) < 0.5).all() and (rv > 0.5).all() and (rv < 1.5).all()
        assert len(np.unique(rm)) == rm.size and len(np.unique(rv)) == rv.size
        assert int(st[f"{n}.num_batches_tracked"]) == 3 + i
    assert not np.array_equal(st["bn.running_mean"], st["res_blocks.0.bn1.running_mean"])


def own_masks_fp64(state, blocks, ch, x):
    """The 0/1 ReLU masks of the plain fp64 train-mode forward (a scratch net)."""
    net = RefNet(blocks, ch).double()
    load_numpy_state(net, state)
    net.train()
    out = {}
    with torch.no_grad():
        h = F.relu(net.bn(net.conv(torch.from_numpy(x).double())))
        out["a0"] = h
        for i, blk in enumerate(net.res_blocks):
            hh = F.relu(blk.bn1(blk.conv1(h)))
            out[f"h{i}"] = hh
            h = F.relu(blk.bn2(blk.conv2(hh)) + h)
            out[f"xo{i}"] = h
        B = h.shape[0]
        p = F.relu(net.policy_bn(net.policy_conv(h))).reshape(B, -1)
        v = F.relu(net.value_bn(net.value_conv(h))).reshape(B, -1)
        out["fp"], out["fv"], out["hv"] = p, v, F.relu(net.value_fc1(v))
    return {k: (t > 0).double().numpy() for k, t in out.items()}


def masked_run(state, blocks, ch, x, masks, dtype):
    """(BN buffers after one masked train-mode forward in `dtype`, the pre-BN input of
    every BN layer as [N, C] rows)."""
    net = RefNet(blocks, ch).to(dtype)
    load_numpy_state(net, state)
    net.train()
    zin = {}
    hooks = [m.register_forward_pre_hook(
        lambda mod, args, n=n: zin.__setitem__(n, args[0].detach().double().permute(0, 2, 3, 1).reshape(
            -1, args[0].shape[1]).numpy().copy()))
        for n, m in net.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]
    with torch.no_grad():
        *_, buf = masked_forward_fp64(net, x, masks, return_buffers=True, dtype=dtype)
    for h in hooks:
        h.remove()
    return buf, zin


@pytest.mark.parametrize("blocks,ch,B", [(1, 64, 2), (1, 64, 5), (1, 256, 2)])
def test_gate_sees_the_mutants(blocks, ch, B):
    torch.manual_seed(blocks * 1000 + ch)
    st = randomized_bn_state(state_to_numpy(RefModel(blocks, ch).net), blocks, seed=ch + B)
    b, p = synth_positions(B, seed=77 + B)
    x = encode_batch(b, p)
    masks = own_masks_fp64(st, blocks, ch, x)
    want, z64 = masked_run(st, blocks, ch, x, masks, torch.float64)
    got32, _ = masked_run(st, blocks, ch, x, masks, torch.float32)
    names = bn_layer_names(blocks)
    trunk = names[:-2]
    old = {n: (st[f"{n}.running_mean"].astype(np.float64), st[f"{n}.running_var"].astype(np.float64)) for n in names}

    def biased(n):
        z = z64[n]
        return 0.9 * old[n][0] + 0.1 * z.mean(0), 0.9 * old[n][1] + 0.1 * z.var(0)

    def neighbour(n):
        i = trunk.index(n)
        return trunk[i + 1] if i + 1 < len(trunk) else trunk[i - 1]

    mutants = {
        "biased variance": (names, ("running_var",), biased),
        "old stats one channel over": (names[:-1], ("running_mean", "running_var"),
                                       lambda n: bn_update_fp64(z64[n], np.roll(old[n][0], 1), np.roll(old[n][1], 1))),
        "old stats of the neighbouring layer": (trunk, ("running_mean", "running_var"),
                                                lambda n: bn_update_fp64(z64[n], *old[neighbour(n)])),
        "momentum on the wrong term": (names, ("running_mean", "running_var"),
                                       lambda n: bn_update_fp64(z64[n], *old[n], momentum=0.9)),
    }
    tol = {}
    for i, n in enumerate(names):
        # the helper is the forward's own update, and the counters advance by one
        rm, rv = bn_update_fp64(z64[n], *old[n])
        np.testing.assert_allclose(rm, want[f"{n}.running_mean"], rtol=1e-13, atol=1e-16)
        np.testing.assert_allclose(rv, want[f"{n}.running_var"], rtol=1e-13, atol=0)
        assert int(want[f"{n}.num_batches_tracked"]) == 3 + i + 1 == int(got32[f"{n}.num_batches_tracked"])
        for s in ("running_mean", "running_var"):
            k = f"{n}.{s}"
            assert got32[k].dtype == np.float32 and want[k].dtype == np.float64
            dev = np.abs(got32[k].astype(np.float64) - want[k])
            tol[k] = bn_stat_tolerance(want[k], dev.max())
            print(f"{blocks}x{ch} B={B} {k:32s} dev32={dev.max():.2e} tol(min)={tol[k].min():.2e} "
                  f"max|want|={np.abs(want[k]).max():.3f}")
            assert (dev <= tol[k]).all(), k          # the unmutated fp32 run holds the gate
    for name, (layers, stats, fn) in mutants.items():
        for n in layers:
            mut = dict(zip(("running_mean", "running_var"), fn(n)))
            for s in stats:
                k = f"{n}.{s}"
                shift = np.abs(mut[s] - want[k])
                over = shift > tol[k]
                print(f"{name:36s} {k:32s} min shift/tol={np.min(shift / tol[k]):.1f} beyond: {over.sum()}/{over.size}")
                # one element beyond fails the gate; at these shapes every channel is beyond it
                # (the smallest: the biased variance's 0.1 * var / (N - 1), >= 15x at B = 5)
                assert over.all(), (name, k)
