"""float64 reference of the train step's WEIGHTED loss (include/azg_pv.h
azg_pv_train_backward_weighted):

    policy_loss = (1/B) sum_b wp_b KL_b,   value_loss = (1/B) sum_b wv_b (v_b - z_b)^2

with the divisor B, not the sum of the weights.  The forward is
oracle.ref_net.masked_forward_fp64, so every ReLU's 0/1 mask is the caller's (the GPU's
own forward): a pre-activation within fp32 rounding of zero then cannot make two correct
implementations disagree.  tests/test_weighted_loss_reference.py checks this helper against
plain autograd of the same loss and against oracle.ref_net.masked_grads_fp64 at weights 1.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle.ref_net import RefNet, load_numpy_state, masked_forward_fp64

# the head tensors of each side (named_parameters prefixes)
POLICY_HEAD = ("policy_conv.", "policy_bn.", "policy_fc.")
VALUE_HEAD = ("value_conv.", "value_bn.", "value_fc1.", "value_fc2.")


def weighted_loss(logits, value, pi, z, wp=None, wv=None):
    """(policy_loss, value_loss) of the weighted step as torch scalars; None = all ones."""
    B = logits.shape[0]
    dt = logits.dtype
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dt)
    pi, z = t(pi), t(z).reshape(B, 1)
    wp = torch.ones(B, dtype=dt) if wp is None else t(wp).reshape(B)
    wv = torch.ones(B, dtype=dt) if wv is None else t(wv).reshape(B)
    lp = F.log_softmax(logits, dim=1)
    kl = (torch.xlogy(pi, pi) - pi * lp).sum(dim=1)        # KLDivLoss' pointwise term, per board
    sq = ((value - z) ** 2).reshape(B)
    return (wp * kl).sum() / B, (wv * sq).sum() / B


def weighted_masked_grads_fp64(state: dict, blocks: int, channels: int, x, pi, z, masks: dict, wp=None, wv=None,
                               return_pre: bool = False, dtype=torch.float64):
    """(grads {name: ndarray}, (policy_loss, value_loss)) of the weighted loss with the
    caller's ReLU masks; with return_pre the pre-activations of every masked ReLU come third
    (as oracle.ref_net.masked_grads_fp64 returns them).  dtype: the arithmetic of the whole
    run; torch.float32 gives the fp32 run a tolerance is measured with."""
    net = RefNet(blocks, channels).to(dtype)
    load_numpy_state(net, state)
    net.train()
    logits, value, pre = masked_forward_fp64(net, x, masks, dtype=dtype)
    pl, vl = weighted_loss(logits, value, pi, z, wp, wv)
    (pl + vl).backward()
    out = ({n: q.grad.numpy() for n, q in net.named_parameters()}, (float(pl.detach()), float(vl.detach())))
    if return_pre:
        out += ({k: v.detach().numpy() for k, v in pre.items()},)
    return out


def own_masks_fp64(state: dict, blocks: int, channels: int, x) -> dict:
    """The ReLU masks of the float64 net's own train-mode forward (NCHW / [B, n])."""
    net = RefNet(blocks, channels).double()
    load_numpy_state(net, state)
    net.train()
    out = {}
    with torch.no_grad():
        h = F.relu(net.bn(net.conv(torch.as_tensor(np.asarray(x), dtype=torch.float64))))
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


def seeded_weights(B: int, seed: int):
    """(wp, wv) float32 [B]: 0, 0.25, 1 and 3 mixed independently for the two heads, every
    value present in both (B >= 5), and board 0 with both weights 0."""
    rng = np.random.RandomState(seed)
    vals = np.array([0.0, 0.25, 1.0, 3.0], dtype=np.float32)
    out = []
    for _ in range(2):
        w = vals[rng.randint(0, 4, size=B)]
        w[1:5] = vals[rng.permutation(4)]     # every value occurs
        w[0] = 0.0
        out.append(w)
    return out[0], out[1]
