"""Drop-in replacement for the reference ``network.py`` whose compute runs on
hand-written gfx950 HIP kernels (libazg_pv.so, include/azg_pv.h).

Same public surface as the reference (network.py:9-265):
  * ``ResidualBlock``, ``AlphaZeroNet`` -- same sub-module names, parameter order,
    state_dict keys and initialisation (so ``torch.manual_seed(s)`` + ctor gives the
    reference's weights bit for bit); ``forward`` runs the HIP eval path.
  * ``PyTorchModel(board_size, action_size, device, n_res_blocks=3, channels=64, lr,
    weight_decay)`` with ``predict``, ``predict_batch``, ``train_batch``, ``save``,
    ``load``, ``make_batch_from_states`` and the attributes ``.net``, ``.optimizer``,
    ``.board_size``, ``.action_size``, ``.device``; plus ``policy_value`` /
    ``train_step`` aliases named by the north star, and device-resident variants
    (``predict_device``) for the batched self-play driver, and ``score_batch`` /
    ``score_batch_device``: the train step's two losses and policy / value metrics of a
    batch from the eval forward, changing nothing; and, opt-in (``ema_decay``), an
    exponential moving average of the weights kept inside the train step's Adam kernel
    (``enable_ema``, ``ema_state_dict``, ``ema_model``).

Differences, by design: the device must be a HIP GPU (there is no CPU path: the
reference's CPU fallback, network.py:152, raises here) and the board must be 15x15.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from engine import PolicyValueEngine, score_summary

MEAN8_MAX_BOARDS = PolicyValueEngine.MEAN8_MAX_BOARDS   # boards per mean-of-8 forward (8 images each)
_N = 15


# ---------------- board symmetries (host helpers, numpy only) ----------------
def sym_table() -> np.ndarray:
    """[8, 225] int64: sym_table()[s, j] is the board square that image square j shows
    under symmetry s -- the one convention of MCTS.symmetries, azg_pv_replay_gather and
    azg_pv_forward_boards_sym (csrc/pv_common.h sym_src): np.rot90 by k = s >> 1
    (counter-clockwise), then a column flip when s is odd.  image.flat[j] =
    board.flat[table[s, j]]; a per-square result of the image at j belongs to board
    square table[s, j]."""
    n = _N
    y, x = np.divmod(np.arange(n * n, dtype=np.int64), n)
    t = np.empty((8, n * n), dtype=np.int64)
    for s in range(8):
        xs = n - 1 - x if s & 1 else x
        k = s >> 1
        t[s] = (y * n + xs if k == 0 else xs * n + (n - 1 - y) if k == 1
                else (n - 1 - y) * n + (n - 1 - xs) if k == 2 else (n - 1 - xs) * n + y)
    return t


_SYM_TABLE = sym_table()


def _check_sym(s) -> int:
    if isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) <= 7:
        raise ValueError(f"a symmetry is an int in 0..7, got {s!r}")
    return int(s)


def apply_symmetry(boards, s: int) -> np.ndarray:
    """Image s of boards [..., 15, 15] or [..., 225] (any dtype), same shape."""
    a = np.asarray(boards)
    flat = a.reshape(-1, _N * _N) if a.size else a.reshape(0, _N * _N)
    return flat[:, _SYM_TABLE[_check_sym(s)]].reshape(a.shape)


def invert_symmetry(per_square, s: int) -> np.ndarray:
    """Per-square results [..., 225] (or [..., 15, 15]) of image s back in the board's own
    coordinates: out[..., table[s, j]] = per_square[..., j]."""
    a = np.asarray(per_square)
    flat = a.reshape(-1, _N * _N) if a.size else a.reshape(0, _N * _N)
    out = np.empty_like(flat)
    out[:, _SYM_TABLE[_check_sym(s)]] = flat
    return out.reshape(a.shape)


def _parse_leaf_symmetry(symmetry):
    """Evaluator / proxy option -> None | int 0..7 | "random" | "mean8"."""
    if symmetry is None or (isinstance(symmetry, str) and symmetry in ("random", "mean8")):
        return symmetry
    if isinstance(symmetry, str):
        raise ValueError(f"symmetry must be None, an int 0..7, 'random' or 'mean8', got {symmetry!r}")
    return _check_sym(symmetry)


class ResidualBlock(nn.Module):
    """Parameter container of reference network.py:9-26 (compute: pv_conv.hip)."""

    def __init__(self, channels: int):
        super().__init__()
        self.conv1 = nn.Conv2d(channels, channels, kernel_size=3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(channels)
        self.conv2 = nn.Conv2d(channels, channels, kernel_size=3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(channels)


class AlphaZeroNet(nn.Module):
    """Reference network.py:29-117.  Parameters live in the engine's flat buffers
    once attached to a device (``attach``); forward() is the HIP eval path."""

    def __init__(self, in_channels: int = 3, board_size: int = 15, action_size: int = 15 * 15,
                 n_res_blocks: int = 6, channels: int = 128):
        super().__init__()
        self.board_size = board_size
        self.action_size = action_size
        self.channels = channels
        self.n_res_blocks = n_res_blocks
        self.conv = nn.Conv2d(in_channels, channels, kernel_size=3, padding=1, bias=False)
        self.bn = nn.BatchNorm2d(channels)
        self.res_blocks = nn.ModuleList([ResidualBlock(channels) for _ in range(n_res_blocks)])
        self.policy_conv = nn.Conv2d(channels, 2, kernel_size=1, bias=False)
        self.policy_bn = nn.BatchNorm2d(2)
        self.policy_fc = nn.Linear(2 * board_size * board_size, action_size)
        self.value_conv = nn.Conv2d(channels, 1, kernel_size=1, bias=False)
        self.value_bn = nn.BatchNorm2d(1)
        self.value_fc1 = nn.Linear(board_size * board_size, 64)
        self.value_fc2 = nn.Linear(64, 1)
        self._init_weights()
        self.engine: Optional[PolicyValueEngine] = None

    def _init_weights(self):
        # network.py:75-83 (same RNG consumption order)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
            elif isinstance(m, nn.Linear):
                nn.init.kaiming_uniform_(m.weight, nonlinearity="relu")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def attach(self, device) -> "AlphaZeroNet":
        """Move parameters into the engine's device buffers (once)."""
        if self.engine is None:
            self.engine = PolicyValueEngine(self, self.n_res_blocks, self.channels, self.board_size, device)
        return self

    def to(self, *args, **kwargs):  # keep `.to("cuda")` working like the reference
        dev = None
        if args and isinstance(args[0], (str, torch.device)):
            dev = torch.device(args[0])
        elif "device" in kwargs:
            dev = torch.device(kwargs["device"])
        if dev is not None and dev.type == "cuda":
            return self.attach(dev)
        if self.engine is not None:
            raise RuntimeError("AlphaZeroNet is bound to a HIP device; moving it is not supported")
        return super().to(*args, **kwargs)

    def mark_dirty(self):
        """Call after mutating parameters through ``.data`` (not tracked by autograd versions)."""
        if self.engine is not None:
            self.engine.mark_dirty()

    def forward(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(logits [B,225], value [B,1]) with BN running statistics (eval semantics).
        Train-mode BN runs only inside PyTorchModel.train_batch (fused with backward)."""
        if self.engine is None:
            raise RuntimeError("AlphaZeroNet.forward needs a HIP device: call .to('cuda') first")
        if self.training:
            raise RuntimeError("train-mode forward is fused into PyTorchModel.train_batch; "
                               "call .eval() for inference")
        eng = self.engine
        x = x.to(eng.device, torch.float32).contiguous()
        _, value, logits = eng.forward(x, want_logits=True)
        # a host-visible result, like the reference's: settle the launch now (x is alive)
        seq = eng.last_seq()
        if seq:
            torch.cuda.current_stream(eng.device).synchronize()
            eng.recover(seq)
            eng.check_orphans()
        return logits, value

    def predict(self, state):
        """network.py:119-129: single unbatched state -> (logits, value)."""
        st = torch.as_tensor(np.asarray(state), dtype=torch.float32).unsqueeze(0)
        return self(st)


class HipAdam(torch.optim.Adam):
    """torch.optim.Adam bookkeeping (param_groups, state_dict format: step /
    exp_avg / exp_avg_sq per parameter) whose moments live in flat device buffers
    updated by the fused clip+Adam kernel (azg_pv_train_apply)."""

    def __init__(self, net: AlphaZeroNet, lr: float = 1e-3, weight_decay: float = 1e-4):
        super().__init__(net.parameters(), lr=lr, weight_decay=weight_decay)
        self._net = net
        eng = net.engine
        self.flat_exp_avg = torch.zeros_like(eng.flat_params)
        self.flat_exp_avg_sq = torch.zeros_like(eng.flat_params)

    def get_step(self) -> int:
        self._ensure_state()
        return int(self.state[self._net.engine.params[0]]["step"].item())

    def set_step(self, step: int) -> None:
        self._ensure_state()
        for p in self._net.engine.params:
            self.state[p]["step"].fill_(float(step))

    def _views(self, p, i):
        eng = self._net.engine
        o = int(eng.param_views[i].storage_offset())
        return (self.flat_exp_avg[o:o + p.numel()].view_as(p), self.flat_exp_avg_sq[o:o + p.numel()].view_as(p))

    def _ensure_state(self):
        """Lazily create torch-format state (as torch does on the first step)."""
        for i, p in enumerate(self._net.engine.params):
            st = self.state[p]
            if "exp_avg" not in st:
                ea, es = self._views(p, i)
                ea.zero_()
                es.zero_()
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = ea
                st["exp_avg_sq"] = es

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        with torch.no_grad():
            for i, p in enumerate(self._net.engine.params):
                st = self.state.get(p)
                if not st or "exp_avg" not in st:
                    continue
                ea, es = self._views(p, i)
                ea.copy_(st["exp_avg"])
                es.copy_(st["exp_avg_sq"])
                st["exp_avg"], st["exp_avg_sq"] = ea, es
                # a private step counter: torch's load_state_dict hands back the SOURCE
                # step tensor, and hip_step's fill_ would otherwise advance the other
                # optimizer's step too (the moments above are private copies as well --
                # clean copy semantics; the reference aliases both, train.py:817,827)
                st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)

    def hip_step(self, max_norm: float = float("inf"), total_norm: Optional[torch.Tensor] = None):
        """One optimiser step on the bound flat grads: clip to max_norm, then Adam."""
        self._ensure_state()
        g = self.param_groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise NotImplementedError("amsgrad/maximize are not used by the reference")
        first = self.state[self._net.engine.params[0]]
        step = int(first["step"].item()) + 1
        b1, b2 = g["betas"]
        self._net.engine.train_apply(self.flat_exp_avg, self.flat_exp_avg_sq, step, g["lr"], b1, b2,
                                     g["eps"], g["weight_decay"], max_norm, total_norm)
        for p in self._net.engine.params:
            self.state[p]["step"].fill_(float(step))

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self.hip_step()
        return loss


class BoardEvaluator:
    """Asynchronous leaf evaluation for the native search: pinned host staging
    (the search writes int8 boards straight into it), non-blocking H2D, the
    board-input forward, non-blocking D2H of the masked priors and values, and an
    event to wait on.  Two evaluators let the host search one half of the games
    while the GPU evaluates the other.

    symmetry: None (the plain forward), an int 0..7 (every leaf as that image),
    "random" (a symmetry per leaf drawn from this evaluator's own Generator(seed) -- never
    numpy's global RNG, whose Dirichlet and move-sampling streams stay where they are --
    visible as ``syms[:n]`` after submit) or "mean8" (the mean over all 8 images, at most
    MEAN8_MAX_BOARDS leaves per batch).  The transform runs inside the forward's kernels;
    priors and values come back in the board's own coordinates."""

    def __init__(self, model: "PyTorchModel", capacity: int, symmetry=None, seed=None):
        self.symmetry = _parse_leaf_symmetry(symmetry)
        if self.symmetry == "mean8" and int(capacity) > MEAN8_MAX_BOARDS:
            raise ValueError(f"BoardEvaluator(symmetry='mean8'): capacity {int(capacity)} > {MEAN8_MAX_BOARDS}: a "
                             f"mean-of-8 batch runs 8 images per board in ONE forward, and the engine takes at "
                             f"most {MEAN8_MAX_BOARDS} boards (= {8 * MEAN8_MAX_BOARDS} images) per call")
        self.model = model
        dev = model.engine.device
        self.capacity = int(capacity)
        self.h_boards = torch.empty((capacity, 225), dtype=torch.int8).pin_memory()
        self.h_players = torch.empty((capacity,), dtype=torch.int8).pin_memory()
        self.h_priors = torch.empty((capacity, 225), dtype=torch.float32).pin_memory()
        self.h_values = torch.empty((capacity, 1), dtype=torch.float32).pin_memory()
        self.d_boards = torch.empty((capacity, 225), dtype=torch.int8, device=dev)
        self.d_players = torch.empty((capacity,), dtype=torch.int8, device=dev)
        self.d_probs = torch.empty((capacity, 225), dtype=torch.float32, device=dev)
        self.d_priors = torch.empty((capacity, 225), dtype=torch.float32, device=dev)
        self.d_values = torch.empty((capacity, 1), dtype=torch.float32, device=dev)
        self.boards = self.h_boards.numpy()      # views the search writes into
        self.players = self.h_players.numpy()
        self.event = torch.cuda.Event()
        self.n = 0
        self.seq = 0                             # tower launch number of the batch in flight
        self.h_syms = self.d_syms = self.syms = self.rng = None
        if self.symmetry is not None and self.symmetry != "mean8":
            self.h_syms = torch.zeros((capacity,), dtype=torch.int8).pin_memory()
            self.d_syms = torch.zeros((capacity,), dtype=torch.int8, device=dev)
            self.syms = self.h_syms.numpy()      # the symmetries of the batch in flight
            if self.symmetry == "random":
                self.rng = np.random.Generator(np.random.PCG64(seed))
            else:                                # a fixed image: set once
                self.syms[:] = self.symmetry
                self.d_syms.fill_(self.symmetry)

    def submit(self, n: int) -> None:
        self.n = n
        if n == 0:
            return
        self.d_boards[:n].copy_(self.h_boards[:n], non_blocking=True)
        self.d_players[:n].copy_(self.h_players[:n], non_blocking=True)
        eng = self.model.engine
        if self.symmetry is not None:
            if self.rng is not None:
                self.syms[:n] = self.rng.integers(0, 8, size=n, dtype=np.int8)
                self.d_syms[:n].copy_(self.h_syms[:n], non_blocking=True)
            eng.forward_boards_into(self.d_boards[:n], self.d_players[:n], self.d_probs[:n], self.d_values[:n],
                                    self.d_priors[:n], syms=None if self.d_syms is None else self.d_syms[:n],
                                    mean8=self.symmetry == "mean8")
        else:
            eng.forward_boards_into(self.d_boards[:n], self.d_players[:n], self.d_probs[:n],
                                    self.d_values[:n], self.d_priors[:n])
        self.seq = eng.last_seq()
        self.h_priors[:n].copy_(self.d_priors[:n], non_blocking=True)
        self.h_values[:n].copy_(self.d_values[:n], non_blocking=True)
        self.event.record()

    def wait(self):
        """-> (priors [n,225], values [n,1]) numpy views of the pinned buffers.  A batch
        whose persistent-tower forward timed out is recomputed per layer here (the device
        inputs and outputs of this evaluator are intact until its next submit)."""
        if self.n:
            self.event.synchronize()
            eng = self.model.engine
            if eng.recover(self.seq):
                n = self.n
                self.h_priors[:n].copy_(self.d_priors[:n], non_blocking=True)
                self.h_values[:n].copy_(self.d_values[:n], non_blocking=True)
                self.event.record()
                self.event.synchronize()
            eng.check_orphans(self.seq)
        return self.h_priors.numpy()[:self.n], self.h_values.numpy()[:self.n]


class PyTorchModel:
    """Reference network.py:132-265 surface over the HIP engine."""

    def __init__(self,
                 board_size: int = 15,
                 action_size: Optional[int] = None,
                 device: Optional[str] = None,
                 n_res_blocks: int = 3,
                 channels: int = 64,
                 lr: float = 1e-3,
                 weight_decay: float = 1e-4,
                 eval_precision: str = "exact",
                 ema_decay: Optional[float] = None):
        # "exact": every eval forward holds 1e-5 fp32 parity; "fp16": one-product fp16
        # residual convs (self-play leaf evaluation; 128-channel nets).  Checked before any
        # device work; never written to checkpoints (save / load keep the reference's format)
        if eval_precision not in PolicyValueEngine.EVAL_PRECISIONS:
            raise ValueError(f"eval_precision must be one of {PolicyValueEngine.EVAL_PRECISIONS}, "
                             f"got {eval_precision!r}")
        # ema_decay (None: off, nothing allocated): enable_ema(ema_decay) once the net is built
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be None or in [0, 1), got {ema_decay!r}")
        self.board_size = board_size
        self.action_size = action_size if action_size is not None else board_size * board_size
        self.device = device or ("cuda" if torch.cuda.is_available() else "cpu")
        if not str(self.device).startswith("cuda"):
            raise RuntimeError(
                f"PyTorchModel(device={self.device!r}): this build computes only on HIP devices "
                "(MI355X, gfx950); there is no CPU fallback")
        self.net = AlphaZeroNet(in_channels=3, board_size=board_size, action_size=self.action_size,
                                n_res_blocks=n_res_blocks, channels=channels).attach(self.device)
        self.optimizer = HipAdam(self.net, lr=lr, weight_decay=weight_decay)
        self.value_loss_fn = nn.MSELoss()
        self.policy_loss_fn = nn.KLDivLoss(reduction="batchmean")
        self.max_grad_norm = 3.0                        # network.py:223
        self.grad_hook = None                           # DP: all-reduce of the flat grads (+ skip word)
        self._losses = None
        self._skips_seen = 0                            # device-skipped steps already accounted for
        self._ctor = dict(board_size=board_size, action_size=self.action_size, device=self.device,
                          n_res_blocks=n_res_blocks, channels=channels)   # ema_model builds its twin from it
        self._ema_twin = None
        if eval_precision != "exact":
            self.set_eval_precision(eval_precision)
        if ema_decay is not None:
            self.enable_ema(ema_decay)

    @property
    def engine(self) -> PolicyValueEngine:
        return self.net.engine

    # ---------------- weight average (EMA) ----------------
    @property
    def ema_decay(self) -> Optional[float]:
        return self.engine.ema_decay

    def enable_ema(self, decay: float) -> None:
        """Keep an exponential moving average of the weights while the raw weights train:
        after every train step that commits, e += (1 - decay) (x - e) for every parameter
        and every BN running mean and variance, inside the step's Adam kernel (no second
        pass, and a step the device skips does not move it).  The average starts at the
        current weights.  Read it with ema_state_dict() or ema_model()."""
        self.engine.enable_ema(decay)

    def disable_ema(self) -> None:
        """Stop averaging and free the average (and ema_model's twin)."""
        self.engine.disable_ema()
        self._ema_twin = None

    def reset_ema(self) -> None:
        """Set the average back to the current weights: call it after loading weights
        through torch (net.load_state_dict), which the average does not see."""
        self.engine.reset_ema()

    def ema_state_dict(self) -> dict:
        """The average as clones shaped and keyed exactly like net.state_dict(): parameters
        and BN running means / variances from the average, num_batches_tracked from the
        live counters.  RuntimeError when EMA is off."""
        eng = self.engine
        if eng.flat_ema is None:
            raise RuntimeError("ema_state_dict: EMA is off (PyTorchModel(ema_decay=...) or enable_ema)")
        return {k: eng.ema_source(v).detach().clone() for k, v in self.net.state_dict().items()}

    def _load_ema_state(self, sd: dict) -> None:
        eng = self.engine
        with torch.no_grad():
            for k, v in self.net.state_dict().items():
                dst = eng.ema_source(v)
                if dst is not v:   # the counters are the live ones
                    dst.copy_(sd[k])

    def ema_model(self) -> "PyTorchModel":
        """A second PyTorchModel of the same shape on the same device that holds the
        average: created on the first call, and on every call refreshed from the average
        by device-to-device copies on the current stream (counters: the live ones).  It has
        its own eval precision ("exact" unless set on it), its own board evaluators and no
        EMA of its own; hand it to self-play or gating like any model."""
        eng = self.engine
        if eng.flat_ema is None:
            raise RuntimeError("ema_model: EMA is off (PyTorchModel(ema_decay=...) or enable_ema)")
        if self._ema_twin is None:
            with torch.random.fork_rng(devices=[]):   # the twin's weight init draws nothing from the caller's RNG
                self._ema_twin = PyTorchModel(**self._ctor)
            self._ema_twin.net.train(self.net.training)
        t = self._ema_twin.engine
        with torch.no_grad():
            t.flat_params.copy_(eng.flat_ema)
            t.flat_bn.copy_(eng.flat_ema_bn)
            t.flat_nbt.copy_(eng.flat_nbt)
        t.mark_dirty()
        return self._ema_twin

    @property
    def eval_precision(self) -> str:
        return self.engine.eval_precision

    def set_eval_precision(self, precision: str) -> None:
        """The precision of this model's eval forwards (predict, predict_boards, its board
        evaluators): "exact" or "fp16".  Another model in the process keeps its own; the train
        step is not affected.  ValueError names what is supported when the engine refuses."""
        self.engine.set_eval_precision(precision)

    # ---------------- inference ----------------
    def predict(self, encoded_states: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """network.py:168-183: (probs [B,225] float32, values [B,1] float32) with BN
        running stats; the module's train/eval flag is left as it was."""
        eng = self.engine
        x = torch.from_numpy(np.ascontiguousarray(encoded_states, dtype=np.float32)).to(eng.device)
        probs, values = self.predict_device(x)
        seq = eng.last_seq()
        out = probs.cpu().numpy(), values.cpu().numpy()
        if eng.recover(seq):   # a timed-out tower wait: recomputed per layer in place
            out = probs.cpu().numpy(), values.cpu().numpy()
        eng.check_orphans()
        return out

    def predict_device(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Device-resident predict: x [B,3,15,15] -> (probs, values) on the GPU.
        Asynchronous: a caller that synchronises should settle the forward with
        engine.recover(engine.last_seq()) (x must still be intact), as predict does;
        a forward nobody settles is checked at the engine's next settle point
        (check_orphans: a posted one raises TowerFault there)."""
        eng = self.engine
        probs, values, _ = eng.forward(x)
        eng.track(eng.last_seq())
        return probs, values

    policy_value = predict

    def predict_boards(self, boards: np.ndarray, players: np.ndarray, masked: bool = True, symmetry=None):
        """Leaf evaluation from int8 boards [B,15,15] or [B,225] and the side to move
        [B]: the encoding (games/gomoku.py:130-150) runs inside the stem kernel.
        Returns (priors = probs * valid if masked else probs, values [B,1]) as numpy.

        symmetry: None; an int 0..7 or an int array [B] (board b is evaluated as its image
        symmetry[b], sym_table()); or "mean8" (the mean over all 8 images, summed in image
        order; batches above MEAN8_MAX_BOARDS boards run as successive calls).  The
        transform runs on the GPU and the results are in the board's own coordinates:
        bitwise apply_symmetry -> plain predict_boards -> invert_symmetry."""
        n_boards = len(boards)
        syms_np = None
        if symmetry is not None and not (isinstance(symmetry, str) and symmetry == "mean8"):
            if isinstance(symmetry, str):
                raise ValueError(f"symmetry must be None, an int 0..7, an int array [B] or 'mean8', got {symmetry!r}")
            if np.ndim(symmetry) == 0:
                syms_np = np.full(n_boards, _check_sym(symmetry if not isinstance(symmetry, np.ndarray)
                                                       else symmetry.item()), dtype=np.int8)
            else:
                a = np.asarray(symmetry)
                if a.dtype.kind not in "iu" or a.shape != (n_boards,):
                    raise ValueError(f"symmetry array must be integers of shape [{n_boards}], got "
                                     f"{a.dtype} {a.shape}")
                if a.size and (a.min() < 0 or a.max() > 7):
                    raise ValueError("symmetry array values must be in 0..7")
                syms_np = np.ascontiguousarray(a, dtype=np.int8)
        mean8 = symmetry is not None and syms_np is None
        eng = self.engine
        b = torch.from_numpy(np.ascontiguousarray(boards, dtype=np.int8).reshape(len(boards), 225)).to(eng.device)
        pl = torch.from_numpy(np.ascontiguousarray(players, dtype=np.int8).reshape(-1)).to(eng.device)
        B = int(b.shape[0])
        probs = torch.empty((B, 225), dtype=torch.float32, device=eng.device)
        values = torch.empty((B, 1), dtype=torch.float32, device=eng.device)
        priors = torch.empty_like(probs) if masked else None
        if symmetry is None:
            eng.forward_boards_into(b, pl, probs, values, priors)
            seq = eng.last_seq()
            out = (priors if masked else probs).cpu().numpy(), values.cpu().numpy()
            if eng.recover(seq):
                out = (priors if masked else probs).cpu().numpy(), values.cpu().numpy()
            eng.check_orphans()
            return out
        sy = None if mean8 else torch.from_numpy(syms_np).to(eng.device)
        step = MEAN8_MAX_BOARDS if mean8 else max(B, 1)
        for lo in range(0, B, step):   # each call is settled before the next reuses the workspace
            hi = min(B, lo + step)
            eng.forward_boards_into(b[lo:hi], pl[lo:hi], probs[lo:hi], values[lo:hi],
                                    None if priors is None else priors[lo:hi],
                                    syms=None if mean8 else sy[lo:hi], mean8=mean8)
            seq = eng.last_seq()
            torch.cuda.current_stream(eng.device).synchronize()
            eng.recover(seq)
        out = (priors if masked else probs).cpu().numpy(), values.cpu().numpy()
        eng.check_orphans()
        return out

    def board_evaluator(self, capacity: int, symmetry=None, seed=None) -> "BoardEvaluator":
        return BoardEvaluator(self, capacity, symmetry=symmetry, seed=seed)

    def symmetric(self, symmetry, seed=None) -> "SymmetricModel":
        """This model with leaf evaluation under board symmetries (SymmetricModel)."""
        return SymmetricModel(self, symmetry, seed=seed)

    def predict_batch(self, states_list: list) -> Tuple[np.ndarray, np.ndarray]:
        return self.predict(self.make_batch_from_states(states_list))

    # ---------------- training ----------------
    def train_batch(self, states: np.ndarray, target_pis: np.ndarray, target_vs: np.ndarray,
                    epochs: int = 1, policy_weight=None, value_weight=None) -> dict:
        """network.py:199-235: per epoch zero_grad, train-mode forward, KLDiv(batchmean)
        + MSE, backward, clip_grad_norm_(3.0), Adam step.  Leaves the net in train mode.

        policy_weight / value_weight (optional host arrays [B] or [B,1], finite, >= 0):
        per-example loss weights, policy_loss = mean_b(wp_b KL_b) and value_loss =
        mean_b(wv_b (v_b - z_b)^2) -- the divisor stays B.  A weight of 0 takes an example
        out of that head's loss; it still passes through the forward and BatchNorm."""
        self.net.train()
        dev = self.engine.device
        B = len(states)
        policy_weight = self.engine.loss_weight(policy_weight, B, "policy_weight")
        value_weight = self.engine.loss_weight(value_weight, B, "value_weight")
        s = torch.from_numpy(np.ascontiguousarray(states, dtype=np.float32)).to(dev)
        t = torch.from_numpy(np.ascontiguousarray(target_pis, dtype=np.float32)).to(dev)
        z = torch.from_numpy(np.ascontiguousarray(target_vs, dtype=np.float32).reshape(-1, 1)).to(dev)
        return self.train_batch_device(s, t, z, epochs, policy_weight=policy_weight, value_weight=value_weight)

    def train_batch_device(self, s: torch.Tensor, t: torch.Tensor, z: torch.Tensor, epochs: int = 1,
                           return_tensor: bool = False, policy_weight=None, value_weight=None):
        """train_batch on device-resident tensors.  return_tensor=True returns the
        mean losses as a float32 [3] device tensor (policy, value, total) without a
        host sync, so consecutive steps pipeline on the stream.

        policy_weight / value_weight: train_batch's loss weights as contiguous float32
        device tensors [B] or [B,1].  Their dtype, shape and device are checked; their
        VALUES are not -- that would need a host sync -- so the caller passes finite
        weights >= 0.  (Host arrays are accepted too and are checked in full.)

        A step whose split-fp16 forward (tuning key 49) met an activation beyond fp16's
        range on any rank does not commit on the device (include/azg_pv.h
        azg_pv_train_apply: params, moments and BN buffers keep the values it started
        from).  Synchronous callers (return_tensor=False) see it with the losses and redo
        the step with fp32 forward convs on every rank -- the result is the key-49 = 0
        step, bitwise.  Pipelined callers (return_tensor=True) do not wait for it: the
        skipped step's batch is dropped, its Adam step number is given back at the next
        call (steps already queued behind it used numbers one higher), and
        engine.train_skips() counts it."""
        self.net.train()
        eng = self.engine
        self._settle_skips()
        B = int(s.shape[0])
        wp = eng.loss_weight(policy_weight, B, "policy_weight")
        wv = eng.loss_weight(value_weight, B, "value_weight")
        losses = torch.empty(3, dtype=torch.float32, device=eng.device)
        acc = None
        vals = None
        for _ in range(epochs):
            step0 = self.optimizer.get_step()
            self._one_step(s, t, z, losses, wp, wv)
            if not return_tensor:
                # one host sync per step (the reference reads its losses per step too)
                v = torch.cat((losses, eng.flat_grads_ext[-1:])).double().tolist()
                if v[3] != 0.0:
                    # skipped on the device on every rank (the all-reduced skip word): redo in fp32
                    self.optimizer.set_step(step0)
                    eng.train_recoveries += 1
                    self._skips_seen += 1
                    eng.train_fp32_once()
                    self._one_step(s, t, z, losses, wp, wv)
                    v = losses.double().tolist()
                vals = v[:3] if vals is None else [a + b for a, b in zip(vals, v[:3])]
            elif epochs > 1:
                acc = losses.double() if acc is None else acc + losses
        if return_tensor:
            return losses if epochs == 1 else (acc / float(epochs)).float()
        vals = [a / float(epochs) for a in vals]
        return {"policy_loss": vals[0], "value_loss": vals[1], "total_loss": vals[2]}

    def _one_step(self, s, t, z, losses, wp=None, wv=None):
        eng = self.engine
        eng.train_backward(s, t, z, losses, wp, wv)
        if self.grad_hook is not None:
            self.grad_hook(eng.flat_grads_ext)   # the gradients AND the step's skip word
        self.optimizer.hip_step(self.max_grad_norm)

    def _settle_skips(self):
        """Give back the Adam step numbers of pipelined steps the device skipped."""
        n = self.engine.train_skips()
        if n < self._skips_seen:       # clear_status reset the count
            self._skips_seen = n
        elif n > self._skips_seen:
            self.optimizer.set_step(self.optimizer.get_step() - (n - self._skips_seen))
            self._skips_seen = n

    train_step = train_batch

    # ---------------- scoring (no training) ----------------
    def score_batch(self, states: np.ndarray, target_pis: np.ndarray, target_vs: np.ndarray,
                    per_board: bool = False, max_batch: int = 4096):
        """Held-out loss and policy / value metrics of a batch, changing nothing: the host-
        array form of score_batch_device (arrays as train_batch takes them).  With
        per_board=True the records come back as a numpy [B,8] array."""
        sums, records = self.score_sums(states, target_pis, target_vs, per_board=per_board, max_batch=max_batch)
        summary = score_summary(sums, len(states))
        return (summary, records) if per_board else summary

    def score_sums(self, states, target_pis, target_vs, per_board: bool = False, max_batch: int = 4096):
        """score_sums_device on host arrays (the records, if asked for, as numpy)."""
        dev = self.engine.device
        s = torch.from_numpy(np.ascontiguousarray(states, dtype=np.float32)).to(dev)
        t = torch.from_numpy(np.ascontiguousarray(target_pis, dtype=np.float32)).to(dev)
        z = torch.from_numpy(np.ascontiguousarray(target_vs, dtype=np.float32).reshape(-1, 1)).to(dev)
        sums, records = self.score_sums_device(s, t, z, per_board=per_board, max_batch=max_batch)
        return sums, (records.cpu().numpy() if per_board else None)

    def score_batch_device(self, s: torch.Tensor, t: torch.Tensor, z: torch.Tensor, per_board: bool = False,
                           max_batch: int = 4096):
        """Score s [B,3,15,15] against targets t [B,225], z [B] or [B,1] (device tensors):
        the eval forward (BN running stats, this model's eval precision) with logits, then
        the scoring kernels (engine.score_outputs), in chunks of at most max_batch boards.
        Returns engine.score_summary's dict -- policy_loss (KLDiv batchmean), value_loss
        (MSE) and total_loss as train_batch names them, policy_entropy, policy_top1,
        target_move_prob, value_sign_agreement, target_mass, n -- and with per_board=True
        also the [B,8] records (engine.SCORE_FIELDS) as a device tensor.

        Only the sums reach the host (one copy per chunk, added in float64 in chunk order).
        The module's train / eval flag, parameters, gradients, BN statistics and counters
        and the optimizer are untouched.  Each chunk is settled as predict settles its
        forward: a posted launch is recomputed and its chunk scored again.
        A SymmetricModel forwards both score methods to its model unchanged: scoring is not
        leaf evaluation and applies no symmetry."""
        sums, records = self.score_sums_device(s, t, z, per_board=per_board, max_batch=max_batch)
        summary = score_summary(sums, int(s.shape[0]))
        return (summary, records) if per_board else summary

    def score_sums_device(self, s: torch.Tensor, t: torch.Tensor, z: torch.Tensor, per_board: bool = False,
                          max_batch: int = 4096):
        """score_batch_device's raw result, for callers that add up several calls
        (train.score_buffer): (the 8 field sums as a float64 numpy array, the [B,8] device
        records or None)."""
        eng = self.engine
        if max_batch < 1:
            raise ValueError(f"max_batch must be >= 1, got {max_batch}")
        s = s.to(eng.device, torch.float32).contiguous()   # alive until every chunk is settled
        t = t.to(eng.device, torch.float32).contiguous()
        z = z.to(eng.device, torch.float32).contiguous().reshape(-1)
        B = int(s.shape[0])
        if B < 1 or tuple(s.shape[1:]) != (3, _N, _N) or tuple(t.shape) != (B, _N * _N) or z.numel() != B:
            raise ValueError(f"score: states [B,3,{_N},{_N}], pis [B,{_N * _N}] and zs [B] with B >= 1 expected, got "
                             f"{tuple(s.shape)}, {tuple(t.shape)}, {tuple(z.shape)}")
        total = np.zeros(8, dtype=np.float64)
        records = []
        for lo in range(0, B, max_batch):
            hi = min(B, lo + max_batch)
            x = s[lo:hi]
            _, values, logits = eng.forward(x, want_logits=True)
            seq = eng.last_seq()
            rec, sums = eng.score_outputs(logits, values, t[lo:hi], z[lo:hi])
            host = sums.cpu().numpy()
            if eng.recover(seq):   # a posted forward left invalid logits: recomputed in place, scored again
                rec, sums = eng.score_outputs(logits, values, t[lo:hi], z[lo:hi])
                host = sums.cpu().numpy()
            eng.check_orphans()
            total += host
            if per_board:
                records.append(rec)
        if not per_board:
            return total, None
        return total, records[0] if len(records) == 1 else torch.cat(records)

    # ---------------- checkpoints ----------------
    def save(self, path: str) -> None:
        """network.py:240-248 format: {"net", "opt", "board_size", "action_size"}; with EMA
        on, one more key, "ema": {"decay", "net": ema_state_dict()} (the reference's loader
        reads "net" and "opt" only)."""
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        torch.cuda.current_stream(self.engine.device).synchronize()
        self._settle_skips()
        net_sd = {k: v.detach().clone() for k, v in self.net.state_dict().items()}
        opt_sd = self.optimizer.state_dict()
        opt_sd = {"state": {i: {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in st.items()}
                            for i, st in opt_sd["state"].items()},
                  "param_groups": opt_sd["param_groups"]}
        state = {"net": net_sd, "opt": opt_sd, "board_size": self.board_size, "action_size": self.action_size}
        if self.ema_decay is not None:
            state["ema"] = {"decay": self.ema_decay, "net": self.ema_state_dict()}
        torch.save(state, path)

    def load(self, path: str, map_location: Optional[str] = None) -> None:
        """network.py:250-258; optimizer-state errors are ignored as in the reference.
        With EMA on, the average is restored from the file's "ema" key (this model keeps its
        own decay), or reset to the loaded weights when the file has none; with EMA off the
        key is ignored."""
        map_location = map_location or self.device
        state = torch.load(path, map_location=map_location, weights_only=True)
        self.net.load_state_dict(state["net"])
        if self.ema_decay is not None:
            if state.get("ema") is not None:
                self._load_ema_state(state["ema"]["net"])
            else:
                self.reset_ema()
        if "opt" in state and state["opt"] is not None:
            try:
                self.optimizer.load_state_dict(state["opt"])
            except Exception:
                pass

    @staticmethod
    def make_batch_from_states(list_of_encoded_states: list) -> np.ndarray:
        return np.stack(list_of_encoded_states, axis=0).astype(np.float32)


class SymmetricModel:
    """A light proxy of a PyTorchModel whose leaf evaluations run under board symmetries:
    ``symmetry`` is an int 0..7, "random" (a symmetry per leaf, AlphaGo Zero's leaf
    evaluation) or "mean8" (the mean over all 8 images: exactly equivariant, 8x the cost).
    Self-play, gating and the players only call ``board_evaluator`` / ``predict``, so the
    proxy drops into selfplay_games, NativeSelfPlay, NativeEval, evaluate_models and
    NativeMCTS unchanged; everything else (net, engine, save, ...) is the model's --
    score_batch and score_batch_device among them: scoring applies no symmetry.

    seed: evaluator number k of a seeded proxy draws from Generator([seed, k]); predict
    draws from Generator(seed).  A position is evaluated once per tree node, so its
    symmetry is drawn once."""

    def __init__(self, model: PyTorchModel, symmetry, seed=None):
        sym = _parse_leaf_symmetry(symmetry)
        if sym is None:
            raise ValueError("SymmetricModel needs a symmetry: an int 0..7, 'random' or 'mean8'")
        self.__dict__.update(_model=model, symmetry=sym, seed=seed, _evaluators=0,
                             rng=np.random.Generator(np.random.PCG64(seed)) if sym == "random" else None)

    def __getattr__(self, name):          # everything not defined here: the model's
        return getattr(self._model, name)

    def __setattr__(self, name, value):
        if name in self.__dict__:
            self.__dict__[name] = value
        else:
            setattr(self._model, name, value)

    def board_evaluator(self, capacity: int) -> BoardEvaluator:
        k = self._evaluators
        self._evaluators = k + 1
        seed = None if self.seed is None else [self.seed, k]
        return BoardEvaluator(self._model, capacity, symmetry=self.symmetry, seed=seed)

    def predict(self, encoded_states: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """PyTorchModel.predict on float planes [B,3,15,15] (plane 0: the side to move's
        stones, plane 1: the opponent's): the planes become int8 stones (plane0 + 2 plane1,
        player 1) and the board forward applies the symmetry on the GPU."""
        x = np.asarray(encoded_states, dtype=np.float32)
        stones = (x[:, 0] + 2.0 * x[:, 1]).astype(np.int8).reshape(len(x), 225)
        players = np.ones(len(x), dtype=np.int8)
        sym = self.symmetry
        if sym == "random":
            sym = self.rng.integers(0, 8, size=len(x), dtype=np.int8)
        return self._model.predict_boards(stones, players, masked=False, symmetry=sym)

    policy_value = predict

    def predict_batch(self, states_list: list) -> Tuple[np.ndarray, np.ndarray]:
        return self.predict(self._model.make_batch_from_states(states_list))
