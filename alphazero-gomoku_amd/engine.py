"""PolicyValueEngine: owns one libazg_pv handle and the torch-owned flat buffers
it computes on (parameters, gradients, Adam moments, BN running stats).

Layout contract (include/azg_pv.h): parameters / gradients / moments are flat
fp32 buffers in nn.Module.parameters() order with torch's per-tensor layout;
BN running stats are [mean(c) | var(c)] per BatchNorm layer in module order.
Each nn.Parameter / BN buffer of the module becomes a view into these buffers,
so state_dict(), load_state_dict() and torch.save() keep working unchanged.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.nn as nn

from _native import AzgConfig, check, load_library, ptr


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class TowerFault(RuntimeError):
    """A persistent-tower forward computed on stale inputs and could not be recomputed."""


# fields of a score record, in order (include/azg_pv.h AZG_PV_SCORE_*)
SCORE_FIELDS = ("kl", "sq", "entropy", "top1", "p_best", "v_agree", "decided", "target_mass")


def score_summary(sums, n) -> dict:
    """Means over n boards from the summed score records (PolicyValueEngine.score_outputs),
    in float64.  The first three keys are train_batch's: policy_loss is
    KLDivLoss(batchmean), value_loss MSELoss.  value_sign_agreement is taken over the
    decided boards (z != 0) only; with none it is 0."""
    s = [float(v) for v in sums]
    if len(s) != len(SCORE_FIELDS):
        raise ValueError(f"score_summary: {len(SCORE_FIELDS)} sums expected, got {len(s)}")
    n = int(n)
    if n < 1:
        raise ValueError(f"score_summary: n must be >= 1, got {n}")
    policy, value = s[0] / n, s[1] / n
    return {"policy_loss": policy, "value_loss": value, "total_loss": policy + value,
            "policy_entropy": s[2] / n, "policy_top1": s[3] / n, "target_move_prob": s[4] / n,
            "value_sign_agreement": s[5] / max(s[6], 1.0), "target_mass": s[7] / n, "n": n}


class PolicyValueEngine:
    MEAN8_MAX_BOARDS = 2048   # azg_pv_forward_boards_sym mode 1: boards per call (8 images each)

    def __init__(self, net: nn.Module, blocks: int, channels: int, board: int, device):
        if board != 15:
            raise ValueError("the gfx950 kernels are built for 15x15 boards only")
        self.lib = load_library()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("PolicyValueEngine needs a HIP (MI355X) device; there is no CPU path")
        cfg = AzgConfig(blocks, channels, board, 3)
        h = ctypes.c_void_p()
        check(self.lib.azg_pv_create(ctypes.byref(cfg), ctypes.byref(h)), self.lib)
        self.h = h
        self.net = net
        self.blocks, self.channels = blocks, channels
        n = self.lib.azg_pv_num_param_tensors(h)
        offs = (ctypes.c_int64 * n)()
        nums = (ctypes.c_int64 * n)()
        check(self.lib.azg_pv_param_layout(h, offs, nums), self.lib)
        params = list(net.parameters())
        if len(params) != n or any(p.numel() != nums[i] for i, p in enumerate(params)):
            raise RuntimeError("module parameters do not match the engine layout")
        self.nparam = int(self.lib.azg_pv_param_count(h))
        dev = self.device
        with torch.no_grad():
            self.flat_params = torch.empty(self.nparam, dtype=torch.float32, device=dev)
            # the gradients + ONE skip word (include/azg_pv.h azg_pv_bind, ABI 3): a DP
            # all-reduce of flat_grads_ext carries a rank's split-fp16 range overflow to
            # every rank, and train_apply commits the step only where the word is 0
            ng = int(self.lib.azg_pv_grad_count(h))
            if ng != self.nparam + 1:
                raise RuntimeError("libazg_pv: unexpected gradient buffer layout")
            self.flat_grads_ext = torch.zeros(ng, dtype=torch.float32, device=dev)
            self.flat_grads = self.flat_grads_ext[:self.nparam]
            self.param_views = []
            self.grad_views = []
            for i, p in enumerate(params):
                o, k = int(offs[i]), int(nums[i])
                v = self.flat_params[o:o + k].view_as(p)
                v.copy_(p.data.to(dev, torch.float32))
                p.data = v
                gv = self.flat_grads[o:o + k].view_as(p)
                p.grad = gv
                self.param_views.append(v)
                self.grad_views.append(gv)
            bns = [m for m in net.modules() if isinstance(m, nn.BatchNorm2d)]
            self.nbn = int(self.lib.azg_pv_bn_count(h))
            if sum(2 * b.num_features for b in bns) != self.nbn:
                raise RuntimeError("BatchNorm layers do not match the engine layout")
            self.flat_bn = torch.empty(self.nbn, dtype=torch.float32, device=dev)
            self.flat_nbt = torch.zeros(len(bns), dtype=torch.int64, device=dev)
            o = 0
            for i, b in enumerate(bns):
                c = b.num_features
                self.flat_bn[o:o + c].copy_(b.running_mean)
                self.flat_bn[o + c:o + 2 * c].copy_(b.running_var)
                self.flat_nbt[i].copy_(b.num_batches_tracked)
                b.running_mean = self.flat_bn[o:o + c]
                b.running_var = self.flat_bn[o + c:o + 2 * c]
                b.num_batches_tracked = self.flat_nbt[i]
                o += 2 * c
        self.params = params
        check(self.lib.azg_pv_bind(h, ptr(self.flat_params), ptr(self.flat_grads_ext), ptr(self.flat_bn)), self.lib)
        if self.lib.azg_pv_num_bn_layers(h) != len(bns):
            raise RuntimeError("BatchNorm layer count does not match the engine layout")
        # num_batches_tracked advances inside the train kernels (no extra launch)
        check(self.lib.azg_pv_bind_counters(h, ptr(self.flat_nbt)), self.lib)
        self._seen = self._versions()
        self._out_cache = {}
        self.recoveries = 0         # tower launches recomputed per layer (recover)
        self.train_recoveries = 0   # train steps skipped on the device and redone in fp32 (network.train_batch)
        self._unsettled = []        # launch numbers of forwards no host sync has settled yet (predict_device)
        # the running average of the weights (enable_ema): off, and nothing allocated, by default
        self.flat_ema = None        # [nparam], laid out like flat_params
        self.flat_ema_bn = None     # [nbn], laid out like flat_bn
        self.ema_decay = None

    # -- weight average (EMA) -----------------------------------------------
    def enable_ema(self, decay: float) -> None:
        """Keep e += (1 - decay) (x - e) of the parameters and the BN running stats, moved
        inside the Adam kernel by every train step that commits (include/azg_pv.h
        azg_pv_bind_ema; a step the device skips leaves it alone).  The average starts at
        the current weights, copied on the current stream.  Calling it again changes the
        decay and restarts the average."""
        d = float(decay)
        if not 0.0 <= d < 1.0:   # NaN fails too
            raise ValueError(f"ema_decay must be in [0, 1), got {decay!r}")
        with torch.no_grad():
            ema, ema_bn = self.flat_params.clone(), self.flat_bn.clone()
        check(self.lib.azg_pv_bind_ema(self.h, ptr(ema), ptr(ema_bn), d), self.lib)
        self.flat_ema, self.flat_ema_bn, self.ema_decay = ema, ema_bn, d

    def disable_ema(self) -> None:
        if self.flat_ema is not None:
            check(self.lib.azg_pv_bind_ema(self.h, None, None, 0.0), self.lib)
            self.flat_ema = self.flat_ema_bn = self.ema_decay = None

    def reset_ema(self) -> None:
        """The average back at the current weights (after loading weights through torch)."""
        if self.flat_ema is None:
            raise RuntimeError("reset_ema: EMA is off (enable_ema)")
        with torch.no_grad():
            self.flat_ema.copy_(self.flat_params)
            self.flat_ema_bn.copy_(self.flat_bn)

    def ema_weight(self) -> float:
        """The fp32 weight 1 - decay the kernel applies, as the library computes it."""
        return float(np.float32(1.0 - float(np.float32(self.ema_decay))))

    def ema_source(self, t: torch.Tensor):
        """For a tensor of net.state_dict() (a view of one of the flat buffers): the same
        elements of the average -- of flat_ema for a parameter, of flat_ema_bn for a running
        mean or variance -- or the tensor itself for a counter."""
        o, k = int(t.storage_offset()), t.numel()
        base = t.untyped_storage().data_ptr()
        if base == self.flat_params.untyped_storage().data_ptr():
            return self.flat_ema[o:o + k].view(t.shape)
        if base == self.flat_bn.untyped_storage().data_ptr():
            return self.flat_ema_bn[o:o + k].view(t.shape)
        if base == self.flat_nbt.untyped_storage().data_ptr():
            return t
        raise RuntimeError("a tensor of the module's state no longer lives in the engine's flat buffers")

    # -- housekeeping -------------------------------------------------------
    def _versions(self):
        # nn.Parameter keeps its own version counter after `p.data = view`, so sum them;
        # BN buffers ARE views of flat_bn and share its counter; the num_batches_tracked
        # buffers are views of flat_nbt (a counter written alone, e.g. bn.num_batches_tracked
        # .zero_(), must refresh the copy a skipped train step restores).
        return (self.flat_params._version, self.flat_bn._version, self.flat_nbt._version,
                sum(p._version for p in self.params))

    def sync_dirty(self):
        """Parameters or BN stats were modified in place through torch (load_state_dict,
        copy_, optimizer from outside): re-derive packed weights before the next call."""
        v = self._versions()
        if v != self._seen:
            check(self.lib.azg_pv_mark_dirty(self.h), self.lib)
            self._seen = v

    def mark_dirty(self):
        check(self.lib.azg_pv_mark_dirty(self.h), self.lib)

    def last_seq(self) -> int:
        """Launch number of the last forward if it ran the persistent tower, else 0
        (include/azg_pv.h azg_pv_last_seq)."""
        return int(self.lib.azg_pv_last_seq(self.h))

    def recover(self, seq: int) -> bool:
        """Call after synchronising with forward `seq`: if one of its tower waits timed
        out, recompute it with per-layer convs (bitwise what an undisturbed tower gives)
        into the same device outputs, stream-ordered, and return True.  The forward's
        input and output buffers must still be intact."""
        if not seq:
            return False
        if seq in self._unsettled:
            self._unsettled.remove(seq)
        done = ctypes.c_int32(0)
        check(self.lib.azg_pv_recover(self.h, int(seq), ctypes.byref(done), _stream(self.device)), self.lib)
        if done.value:
            self.recoveries += 1
        return bool(done.value)

    def track(self, seq: int) -> None:
        """Register a forward whose caller synchronises later without settling it
        (PyTorchModel.predict_device): the next settle point checks it."""
        if seq:
            self._unsettled.append(int(seq))
            del self._unsettled[:-1024]

    def check_orphans(self, upto: int = 0) -> None:
        """Settle point (the caller has synchronised this engine's stream): raise
        TowerFault if a tracked forward older than `upto` (0: every tracked one) timed out
        or met a split-fp16 range overflow -- its buffers may be gone, so it cannot be
        recomputed, and its outputs are invalid."""
        keep, bad = [], []
        for s in self._unsettled:
            if upto and s >= upto:
                keep.append(s)
            elif int(self.lib.azg_pv_posted(self.h, s)):
                bad.append(s)
        self._unsettled = keep
        if bad:
            raise TowerFault(f"libazg_pv: forward launch(es) {bad} timed out or left fp16's range and were never "
                             f"settled (predict_device outputs consumed without recover); their outputs are invalid "
                             f"({self.tower_diag()})")

    def check_status(self):
        """Raise TowerFault if an eval launch this handle ran timed out or met a split-fp16
        range overflow and was not recovered (azg_pv_status: a plain host load, complete
        for every forward the caller has synchronised with).  The product recovers every
        such launch at its host sync (recover), so this fires only for forwards nobody
        settled.  The posted launches stay until clear_status()."""
        s = int(self.lib.azg_pv_status(self.h))
        if s:
            d = self.tower_diag()
            raise TowerFault(f"libazg_pv: {s} eval launch(es) timed out or left fp16's range and were not "
                             f"recomputed; their outputs are invalid ({d})")

    def train_skips(self) -> int:
        """Train steps the Adam kernel skipped since clear_status (azg_pv_train_status: a
        plain host load, complete for every step the caller has synchronised with)."""
        return int(self.lib.azg_pv_train_status(self.h))

    def train_fp32_once(self):
        """The next train_backward runs its forward convs with fp32 MFMA (the redo of a
        skipped step)."""
        check(self.lib.azg_pv_train_fp32_once(self.h), self.lib)

    def clear_status(self):
        check(self.lib.azg_pv_clear_status(self.h), self.lib)

    def tower_diag(self) -> dict:
        """The tower's wait record since the last tower_diag_clear (include/azg_pv.h
        azg_pv_tower_diag): wait histogram, timeouts, and the first timed-out wait."""
        from _native import TowerDiag
        d = TowerDiag()
        check(self.lib.azg_pv_tower_diag_read(self.h, ctypes.byref(d), _stream(self.device)), self.lib)
        return d.as_dict()

    def tower_diag_clear(self):
        check(self.lib.azg_pv_tower_diag_clear(self.h, _stream(self.device)), self.lib)

    EVAL_PRECISIONS = ("exact", "fp16")   # AZG_PV_EVAL_EXACT, AZG_PV_EVAL_FP16 (include/azg_pv.h)

    @property
    def eval_precision(self) -> str:
        return self.EVAL_PRECISIONS[int(self.lib.azg_pv_get_eval_precision(self.h))]

    def set_eval_precision(self, precision: str) -> None:
        """"exact" (the default: 1e-5 fp32 parity) or "fp16" (one-product fp16 residual
        convs, for self-play leaf evaluation; C = 128 nets only).  Per handle: another model
        in the process keeps its own.  ValueError when the value is unknown or the engine
        has no fp16 form for this net."""
        if precision not in self.EVAL_PRECISIONS:
            raise ValueError(f"eval_precision must be one of {self.EVAL_PRECISIONS}, got {precision!r}")
        if self.lib.azg_pv_set_eval_precision(self.h, self.EVAL_PRECISIONS.index(precision)):
            err = self.lib.azg_pv_last_error()
            raise ValueError(f"eval_precision={precision!r} is not supported for a {self.blocks}x{self.channels} "
                             f"net (supported: 'exact' for every net, 'fp16' for 128 channels and 1..32 blocks): "
                             f"{err.decode() if err else ''}")

    def reattach_grads(self):
        for p, g in zip(self.params, self.grad_views):
            if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                p.grad = g

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.azg_pv_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- compute ------------------------------------------------------------
    def forward(self, x: torch.Tensor, want_logits: bool = False):
        """Eval-mode forward on device.  x: [B,3,15,15] fp32 (any device/dtype)."""
        x = x.to(self.device, torch.float32).contiguous()
        B = int(x.shape[0])
        probs = torch.empty((B, 225), dtype=torch.float32, device=self.device)
        values = torch.empty((B, 1), dtype=torch.float32, device=self.device)
        logits = torch.empty((B, 225), dtype=torch.float32, device=self.device) if want_logits else None
        self.forward_into(x, probs, values, logits)
        return probs, values, logits

    def forward_into(self, x, probs, values, logits=None):
        self.sync_dirty()
        check(self.lib.azg_pv_forward(self.h, ptr(x), int(x.shape[0]), ptr(probs), ptr(values), ptr(logits),
                                      _stream(self.device)), self.lib)

    def forward_boards_into(self, boards, players, probs, values, priors=None, syms=None, mean8=False):
        """Eval forward from device int8 boards [B,225] + players [B] (on-GPU encode);
        priors (optional) = probs * (board == 0).

        syms (device int8 [B], values 0..7): board b is evaluated as its image syms[b]
        (network.sym_table) and the results come back in the board's own coordinates.
        mean8: every board is evaluated as all 8 images and the results are their mean
        (B <= MEAN8_MAX_BOARDS).  Both run inside the stem and the heads' last kernel
        (include/azg_pv.h azg_pv_forward_boards_sym); syms must stay intact until the
        forward is settled, like boards.  With neither, the plain entry point runs."""
        self.sync_dirty()
        if syms is None and not mean8:
            check(self.lib.azg_pv_forward_boards(self.h, ptr(boards), ptr(players), int(boards.shape[0]), ptr(probs),
                                                 ptr(values), ptr(priors), _stream(self.device)), self.lib)
            return
        if syms is not None and not mean8:
            if syms.dtype != torch.int8 or syms.device != boards.device or syms.numel() != boards.shape[0] \
                    or not syms.is_contiguous():
                raise ValueError("syms must be a contiguous int8 tensor [B] on the boards' device")
        check(self.lib.azg_pv_forward_boards_sym(self.h, ptr(boards), ptr(players), None if mean8 else ptr(syms),
                                                 1 if mean8 else 0, int(boards.shape[0]), ptr(probs), ptr(values),
                                                 ptr(priors), _stream(self.device)), self.lib)

    def loss_weight(self, w, batch: int, name: str = "weight"):
        """A per-example loss weight as the device tensor train_backward takes: None stays
        None; a device tensor must be contiguous float32 [B] or [B,1] on this engine's device
        -- its VALUES are not checked (that would need a host sync): the caller passes finite
        weights >= 0; anything else is taken as a host array, which is checked (length,
        finite, >= 0) and copied over."""
        if w is None:
            return None
        if torch.is_tensor(w) and w.device.type == "cuda":
            if w.dtype != torch.float32 or tuple(w.shape) not in ((batch,), (batch, 1)) or not w.is_contiguous():
                raise ValueError(f"{name} must be a contiguous float32 tensor of shape [{batch}] or [{batch}, 1], "
                                 f"got {w.dtype} {tuple(w.shape)}")
            if self.device.index is not None and w.device != self.device:
                raise ValueError(f"{name} is on {w.device}, the engine on {self.device}")
            return w
        a = np.asarray(w.numpy() if torch.is_tensor(w) else w, dtype=np.float32)
        if a.shape not in ((batch,), (batch, 1)):
            raise ValueError(f"{name} must have shape [{batch}] or [{batch}, 1], got {a.shape}")
        if not np.isfinite(a).all() or (a < 0).any():
            raise ValueError(f"{name} must be finite and >= 0")
        return torch.from_numpy(np.ascontiguousarray(a.reshape(-1))).to(self.device)

    def train_backward(self, x, pis, zs, losses, policy_weight=None, value_weight=None):
        """One azg_pv_train_backward; with a weight (device float32 [B], see loss_weight) the
        weighted entry point: policy_loss = mean(wp KL), value_loss = mean(wv (v - z)^2)."""
        self.sync_dirty()
        if policy_weight is None and value_weight is None:
            check(self.lib.azg_pv_train_backward(self.h, ptr(x), ptr(pis), ptr(zs), int(x.shape[0]), ptr(losses),
                                                 _stream(self.device)), self.lib)
        else:
            check(self.lib.azg_pv_train_backward_weighted(self.h, ptr(x), ptr(pis), ptr(zs), ptr(policy_weight),
                                                          ptr(value_weight), int(x.shape[0]), ptr(losses),
                                                          _stream(self.device)), self.lib)
        self._seen = self._versions()
        self.reattach_grads()

    def train_apply(self, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, wd, max_norm, total_norm=None):
        check(self.lib.azg_pv_train_apply(self.h, ptr(exp_avg), ptr(exp_avg_sq), int(step), float(lr),
                                          float(beta1), float(beta2), float(eps), float(wd), float(max_norm),
                                          ptr(total_norm), _stream(self.device)), self.lib)

    def score_outputs(self, logits, values, pis, zs):
        """Score eval-forward outputs against targets on the device (include/azg_pv.h
        azg_pv_score_outputs; nothing but the results is written).  logits [B,225] as
        forward(want_logits=True) returns them, values [B] or [B,1], pis [B,225], zs [B] or
        [B,1]: contiguous float32 tensors on this engine's device.  Returns (per_board
        [B,8] float32 in SCORE_FIELDS order, sums [8] float64), device tensors, queued on
        the current stream.  Passing another model's probs and values as pis and zs gives
        the drift between two models.  ValueError on a wrong shape, dtype or device."""
        B = int(logits.shape[0]) if torch.is_tensor(logits) and logits.dim() == 2 else 0
        if B < 1:
            raise ValueError("score_outputs: logits must be a [B,225] tensor with B >= 1")
        for name, t, shapes in (("logits", logits, ((B, 225),)), ("values", values, ((B,), (B, 1))),
                                ("pis", pis, ((B, 225),)), ("zs", zs, ((B,), (B, 1)))):
            if not torch.is_tensor(t) or tuple(t.shape) not in shapes:
                raise ValueError(f"score_outputs: {name} must be a tensor of shape {' or '.join(map(str, shapes))}, "
                                 f"got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"score_outputs: {name} must be contiguous float32, got {t.dtype}")
            if t.device != logits.device or t.device.type != "cuda" or \
                    (self.device.index is not None and t.device != self.device):
                raise ValueError(f"score_outputs: {name} is on {t.device}, the engine on {self.device}")
        dev = logits.device
        per_board = torch.empty((B, len(SCORE_FIELDS)), dtype=torch.float32, device=dev)
        sums = torch.empty(len(SCORE_FIELDS), dtype=torch.float64, device=dev)
        check(self.lib.azg_pv_score_outputs(ptr(logits), ptr(values), ptr(pis), ptr(zs), B, ptr(per_board), ptr(sums),
                                            _stream(dev)), self.lib)
        return per_board, sums

    # -- instrumentation ----------------------------------------------------
    DEBUG_BUFFERS = {"z0": 0, "a0": 1, "z1": 2, "h": 3, "z2": 4, "xo": 5, "gX": 6, "DZ": 7, "DH": 8, "GR": 9, "snap": 10}

    HEAD_BUFFERS = {"fp": (11, 450), "fv": (12, 225), "hv": (13, 64)}

    def debug_tensor(self, name: str, batch: int, index: int = 0) -> torch.Tensor:
        """Interior [batch,15,15,C] of a train-workspace buffer from the last train step
        (head features fp/fv/hv: [batch, n])."""
        if name in self.HEAD_BUFFERS:
            which, n = self.HEAD_BUFFERS[name]
            out = torch.empty((batch, n), dtype=torch.float32, device=self.device)
            check(self.lib.azg_pv_debug_copy(self.h, which, 0, ptr(out), batch, _stream(self.device)), self.lib)
            return out
        out = torch.empty((batch, 15, 15, self.channels), dtype=torch.float32, device=self.device)
        check(self.lib.azg_pv_debug_copy(self.h, self.DEBUG_BUFFERS[name], index, ptr(out), batch,
                                         _stream(self.device)), self.lib)
        return out

    def profile_enable(self, on: bool = True):
        check(self.lib.azg_pv_profile_enable(self.h, 1 if on else 0), self.lib)

    def profile_read(self) -> dict:
        """{class: (ms_total, launches)} since the last profile_enable (synchronises)."""
        from _native import PROF_CLASSES
        k = len(PROF_CLASSES)
        ms = (ctypes.c_double * k)()
        n = (ctypes.c_int64 * k)()
        check(self.lib.azg_pv_profile_read(self.h, ms, n), self.lib)
        return {PROF_CLASSES[i]: (ms[i], int(n[i])) for i in range(k) if n[i]}

    def profile_boards(self) -> dict:
        """{class: boards processed} since the last profile_enable."""
        from _native import PROF_CLASSES
        k = len(PROF_CLASSES)
        b = (ctypes.c_int64 * k)()
        check(self.lib.azg_pv_profile_boards(self.h, b), self.lib)
        return {PROF_CLASSES[i]: int(b[i]) for i in range(k) if b[i]}
