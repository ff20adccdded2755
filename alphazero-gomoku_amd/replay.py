"""Device-resident replay buffer with on-GPU symmetry sampling.

``DeviceReplayBuffer`` is a drop-in for selfplay.ReplayBuffer (reference
train.py:272-297) whose storage lives on the GPU.  The host buffer keeps every
position eight times (its dihedral images, 3,604 B of fp32 each) in a deque of
tuples and forms a batch with random.sample + np.stack + three pageable copies.
This one keeps every position ONCE, compactly -- int8 stones (0 empty, 1 side to
move, 2 opponent: plane 2 of the encoding is constant ones), fp32 pi, fp32 z =
1,129 B -- in a preallocated ring, and a HIP kernel (csrc/pv_replay.hip,
azg_pv_replay_gather) forms the batch: the reference's encoding
(games/gomoku.py:130-150) and the image's rotation / flip (MCTS.symmetries,
mcts/new_mcts_alpha.py) on the fly.

Image numbering makes the two buffers interchangeable: image i of this buffer is
element i of the host deque (position i // 8 in ring order, symmetry i % 8), and
random.sample picks by index from (len, k) alone, so under the same random.seed
``sample`` returns the host buffer's batch bit for bit.  Every per-slot array is written
through ``ring_spans`` (a write splits where the ring wraps) and read in ``_order()``.

Opt-in, the ring also carries one WEIGHT per position (``add_positions(...,
surprise=...)``, ``set_weights``) and ``sample_weighted`` draws positions in proportion to
it on the device (csrc/pv_replay_weights.hip): weights are integers, 2**16 quanta per unit
of weight, so their running sums are exact and the draw is an integer function of the
random words -- tests/replay_weights_reference.py reproduces every id in Python integers.
A buffer that never sees a weighted call allocates and does nothing new.

Also opt-in, and independent of the sampling weight: one POLICY LOSS WEIGHT per position
(``add_positions(..., policy_weight=...)``, ``set_policy_weights``), fp32, which
``sample(..., with_policy_weight=True)`` gathers for the batch on the device
(azg_pv_replay_gather_weight) for ``train_batch_device(policy_weight=...)`` -- playout cap
randomization stores 0.0 for positions searched at the small budget.  It does not exist
until the first call that passes weights; ``to_host`` and the pickle never carry it.

Also opt-in: POSITION AVERAGING (``set_target_averaging(True)``).  The ring holds the same
board many times -- the empty board once per game, openings that differ by a rotation or a
flip, transpositions -- each copy with its own noisy search policy and its own +-1 outcome.
With averaging on, ``refresh_averages`` (csrc/pv_replay_average.hip: a canonical 64-bit key per
position, torch's stable sort, an exact board comparison and an fp64 mean per group) derives
pi_avg / z_avg / pw_avg once per buffer change, and the unchanged gather reads those arrays in
place of the raw ones: no launch is added per batch, and which positions are drawn is not
touched.  The raw targets stay what ``to_host``, the pickle and the sidecars carry.
"""
from __future__ import annotations

import random
from typing import Optional

import numpy as np
import torch

from _native import check, load_library, ptr
from selfplay import ReplayBuffer

_N = 15
_PIX = _N * _N
QUANTA = 1 << 16          # quanta per unit of weight (include/azg_pv.h)
MAX_WEIGHT = 1 << 15      # set_weights' bound: below 2**31 quanta


def _images(S: np.ndarray, P: np.ndarray):
    """The 8 dihedral images of S [T,C,n,n] / P [T,n,n] in MCTS.symmetries' order
    (rotation k, then its column flip), formed for all T at once as
    NativeSelfPlay._finish does."""
    T = len(S)
    out = []
    for k in range(4):
        s_k = np.rot90(S, k, axes=(2, 3))
        p_k = np.rot90(P, k, axes=(1, 2))
        out.append((np.ascontiguousarray(s_k), np.ascontiguousarray(p_k).reshape(T, -1)))
        out.append((np.ascontiguousarray(np.flip(s_k, axis=3)),
                    np.ascontiguousarray(np.flip(p_k, axis=2)).reshape(T, -1)))
    return out


def ring_spans(at: int, n: int, cap: int):
    """A write of n <= cap items from slot ``at`` splits where it wraps: [(lo, hi, dst)], items [lo, hi) to slots dst..."""
    first = min(n, cap - at)
    return [(lo, hi, dst) for lo, hi, dst in ((0, first, at), (first, n, 0)) if hi > lo]


def _pinned(values: np.ndarray, dtype) -> torch.Tensor:
    """A pinned host copy; torch's host allocator keeps it alive until the copies queued from it have run."""
    stage = torch.empty(values.shape, dtype=dtype, pin_memory=True)
    stage.numpy()[...] = values
    return stage


def _stack(examples):
    S = np.stack([np.asarray(e[0]) for e in examples]).astype(np.float32, copy=False)
    P = np.stack([np.asarray(e[1]) for e in examples]).astype(np.float32, copy=False)
    Z = np.array([e[2] for e in examples], dtype=np.float32)
    if S.shape[1:] != (3, _N, _N) or P.shape[1:] != (_PIX,):
        raise ValueError(f"examples must be (state [3,{_N},{_N}], pi [{_PIX}], z), got {S.shape[1:]} / {P.shape[1:]}")
    return S, P, Z


class DeviceReplayBuffer:
    """``capacity`` counts images like the reference's deque(maxlen=capacity); the ring
    holds capacity // nsym positions, nsym = 8 if ``symmetries`` else 1."""

    def __init__(self, capacity: int, device, symmetries: bool = True, board_size: int = 15):
        self.nsym = 8 if symmetries else 1
        if board_size != _N:
            raise ValueError("the replay gather is built for 15x15 boards only")
        if capacity < self.nsym or capacity % self.nsym != 0:
            raise ValueError(f"capacity ({capacity}) must be a positive multiple of {self.nsym}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceReplayBuffer needs a HIP (MI355X) device; the host buffer is selfplay.ReplayBuffer")
        self.lib = load_library()
        self.capacity = capacity
        self.cap_pos = capacity // self.nsym
        self.stones = torch.zeros((self.cap_pos, _PIX), dtype=torch.int8, device=self.device)
        self.pis = torch.zeros((self.cap_pos, _PIX), dtype=torch.float32, device=self.device)
        self.zs = torch.zeros(self.cap_pos, dtype=torch.float32, device=self.device)
        self.head = 0     # slot of the oldest position
        self.count = 0    # positions held
        # surprise weighting: nothing of it exists until the first weighted call
        self.weights = None        # [cap_pos] uint32 quanta, by slot (a view of _wq)
        self._wq = None            # the same memory as int32 (quanta < 2**31), for torch's copies and fills
        self._prefix = None        # [cap_pos] running sums of the weights in ring order (uint64 bits in int64)
        self._prefix_ok = False    # False whenever the weights or the ring have moved since the last scan
        # policy loss weights: [cap_pos] float32 by slot, nothing until the first call that passes them
        self._pw = None
        # position averaging: nothing of it exists until set_target_averaging(True)
        self._avg_on = False
        self._avg = None           # dict of device arrays (see _ensure_averages)
        self._avg_ok = False       # False whenever the ring, the policy weights or the setting moved since the last refresh
        self._avg_pw = False       # whether the last refresh wrote pw_avg

    def __len__(self) -> int:
        return self.count * self.nsym

    def _ring(self):   # the (cap_pos, head, count) run of the native calls
        return self.cap_pos, self.head, self.count

    def _order(self) -> torch.Tensor:   # the slots in ring order (oldest first), a device index tensor [count]
        return (self.head + torch.arange(self.count, device=self.device)) % self.cap_pos

    def _write(self, dst, src, at: int) -> None:   # pinned host rows src into the per-slot array dst, from slot at on
        for lo, hi, d in ring_spans(at, len(src), self.cap_pos):
            dst[d:d + hi - lo].copy_(src[lo:hi], non_blocking=True)

    def _fill(self, dst, at: int, n: int, value) -> None:   # value into n slots of the per-slot array dst, from slot at on
        for lo, hi, d in ring_spans(at, n, self.cap_pos):
            dst[d:d + hi - lo].fill_(value)

    def _ring_moved(self) -> None:   # positions came or went: the prefix sums and the averages are stale
        self._prefix_ok = self._avg_ok = False

    def _weights_moved(self) -> None:   # the sampling weights changed: the prefix sums
        self._prefix_ok = False

    def _averaging_inputs_moved(self) -> None:   # the policy weights or the setting changed: the averages
        self._avg_ok = False

    # ---------------------------------------------------------------- writing
    def add_positions(self, examples, surprise=None, mix: float = 0.5, policy_weight=None) -> None:
        """Canonical (state [3,15,15], pi [225], z) tuples, as
        selfplay_games(use_symmetries=False) returns them; the oldest positions are
        overwritten (= the deque's eviction of whole groups of nsym images).

        surprise (optional; one value per example: a device fp32 tensor [n] or [n,8] -- score
        records, field 0 = the policy KL, used in place -- or a host array [n]) gives the new
        positions the weights  (1 - mix) + mix * n * s_i / sum(s)  (azg_pv_replay_surprise_weights:
        non-finite and non-positive surprises count as 0; all of them 0: every weight 1), in
        quanta of 2**-16; the sum runs over all n examples passed even where only the newest
        cap_pos survive.  Without it the new positions weigh 1.0 once the buffer has weights.

        policy_weight (optional host float array [n], finite, >= 0): the positions' policy
        loss weights (sample(with_policy_weight=True)).  Without it the new positions count
        1.0 once the buffer has policy weights.  Examples may be 4-tuples (playout-cap
        self-play); their 4th field is NOT read here -- pass it as policy_weight."""
        examples = list(examples)
        if not examples:
            return
        S, P, Z = _stack(examples)
        n_all = len(S)
        if policy_weight is not None:
            policy_weight = np.asarray(policy_weight, dtype=np.float32).reshape(-1)
            if len(policy_weight) != n_all:
                raise ValueError(f"{len(policy_weight)} policy weights for {n_all} examples")
            if not np.isfinite(policy_weight).all() or (policy_weight < 0).any():
                raise ValueError("policy_weight must be finite and >= 0")
        if surprise is not None:
            if not 0.0 <= float(mix) <= 1.0:
                raise ValueError(f"mix must be in [0, 1], got {mix!r}")
            if not torch.is_tensor(surprise):
                surprise = torch.from_numpy(np.ascontiguousarray(surprise, dtype=np.float32))
            if tuple(surprise.shape) not in ((n_all,), (n_all, 8)) or surprise.dtype != torch.float32:
                raise ValueError(f"surprise must be float32 of shape [{n_all}] or [{n_all}, 8], got "
                                 f"{surprise.dtype} {tuple(surprise.shape)}")
            surprise = surprise.to(self.device).contiguous()
        p0, p1 = S[:, 0], S[:, 1]
        if not (((p0 == 0) | (p0 == 1)).all() and ((p1 == 0) | (p1 == 1)).all()):
            raise ValueError("state planes 0 / 1 must hold 0 or 1")
        if (p0 * p1).any():
            raise ValueError("state planes 0 and 1 must be disjoint")
        if not (S[:, 2] == 1).all():
            raise ValueError("state plane 2 must be all ones (games/gomoku.py:146-150)")
        stones = (p0 + 2 * p1).astype(np.int8).reshape(len(S), _PIX)
        if len(S) > self.cap_pos:     # only the newest cap_pos survive, as in the deque
            stones, P, Z = stones[-self.cap_pos:], P[-self.cap_pos:], Z[-self.cap_pos:]
            if policy_weight is not None:
                policy_weight = policy_weight[-self.cap_pos:]
        n = len(stones)
        # one pinned staging buffer [pis | zs | stones], alive like _pinned's until its copies have run
        stage = torch.empty(n * (_PIX * 4 + 4 + _PIX), dtype=torch.uint8, pin_memory=True)
        o1, o2 = n * _PIX * 4, n * _PIX * 4 + n * 4
        h_pi = stage[:o1].view(torch.float32).view(n, _PIX)
        h_z = stage[o1:o2].view(torch.float32)
        h_st = stage[o2:].view(torch.int8).view(n, _PIX)
        tail = (self.head + self.count) % self.cap_pos
        for dst, host, values in ((self.pis, h_pi, P), (self.zs, h_z, Z), (self.stones, h_st, stones)):
            host.numpy()[...] = values
            self._write(dst, host, tail)
        if surprise is not None:
            self._ensure_weights()
            with torch.cuda.device(self.device):
                check(self.lib.azg_pv_replay_surprise_weights(
                    ptr(surprise), 8 if surprise.dim() == 2 else 1, n, n_all, float(mix), ptr(self._wq), self.cap_pos,
                    tail, torch.cuda.current_stream(self.device).cuda_stream), self.lib)
        elif self._wq is not None:     # eviction takes the old weights with the old positions
            self._fill(self._wq, tail, n, QUANTA)
        if policy_weight is not None:
            self._ensure_policy_weights()
            self._write(self._pw, _pinned(policy_weight, torch.float32), tail)
        elif self._pw is not None:     # eviction takes the old weights with the old positions
            self._fill(self._pw, tail, n, 1.0)
        self._ring_moved()
        over = self.count + n - self.cap_pos
        if over > 0:
            self.head = (self.head + over) % self.cap_pos
        self.count = min(self.count + n, self.cap_pos)

    # ---------------------------------------------------------------- weights
    def _ensure_weights(self) -> None:
        if self._wq is None:   # every position held so far weighs 1.0
            self._wq = torch.full((self.cap_pos,), QUANTA, dtype=torch.int32, device=self.device)
            self.weights = self._wq.view(torch.uint32)
            self._prefix = torch.zeros(self.cap_pos, dtype=torch.int64, device=self.device)   # not yet scanned

    def set_weights(self, w) -> None:
        """Weights of the positions held, a host float array [count] in ring order (oldest
        first): finite, >= 0, each < 32768, sum > 0; stored rounded to quanta of 2**-16."""
        w = np.asarray(w, dtype=np.float64).reshape(-1)
        if len(w) != self.count or self.count < 1:
            raise ValueError(f"{len(w)} weights for {self.count} positions")
        if not np.isfinite(w).all() or (w < 0).any() or (w >= MAX_WEIGHT).any() or not w.sum() > 0:
            raise ValueError(f"weights must be finite, in [0, {MAX_WEIGHT}) and not all zero")
        q = np.rint(w * QUANTA).astype(np.int64)
        if not q.sum() > 0:
            raise ValueError("every weight rounds to zero quanta (one quantum is 2**-16)")
        self._ensure_weights()
        self._write(self._wq, _pinned(q, torch.int32), self.head)
        self._weights_moved()

    def get_weights(self) -> np.ndarray:
        """The weights of the positions held, float64 [count] in ring order (all 1.0 for a
        buffer without weights).  Synchronises."""
        if self._wq is None:
            return np.ones(self.count, dtype=np.float64)
        return self._wq[self._order()].cpu().numpy().astype(np.float64) / QUANTA

    def effective_sample_size(self) -> float:
        """(sum w)^2 / sum w^2 over the positions held: how many equally weighted positions
        the weighted draw is worth.  Synchronises: for logging."""
        w = self.get_weights()
        return float(w.sum() ** 2 / (w * w).sum()) if len(w) and w.any() else 0.0

    # ----------------------------------------------------- policy loss weights
    def _ensure_policy_weights(self) -> None:
        if self._pw is None:   # every position held so far counts 1.0
            self._pw = torch.ones(self.cap_pos, dtype=torch.float32, device=self.device)

    def set_policy_weights(self, w) -> None:
        """Policy loss weights of the positions held, a host float array [count] in ring
        order (oldest first): finite, >= 0."""
        w = np.asarray(w, dtype=np.float32).reshape(-1)
        if len(w) != self.count or self.count < 1:
            raise ValueError(f"{len(w)} policy weights for {self.count} positions")
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError("policy weights must be finite and >= 0")
        self._ensure_policy_weights()
        self._write(self._pw, _pinned(w, torch.float32), self.head)
        self._averaging_inputs_moved()

    def get_policy_weights(self) -> np.ndarray:
        """The policy loss weights of the positions held, float32 [count] in ring order (all
        1.0 for a buffer without them).  Synchronises."""
        if self._pw is None:
            return np.ones(self.count, dtype=np.float32)
        return self._pw[self._order()].cpu().numpy()

    def _gather_policy_weight(self, d_ids, batch_size: int, st) -> torch.Tensor:
        """[B] float32: the policy weight of each image id's position, on the device (ones,
        without a launch or an allocation of the ring's array, for a buffer without them)."""
        if self._pw is None:
            return torch.ones(batch_size, dtype=torch.float32, device=self.device)
        vals = self._avg["pw_avg"] if self._avg_on else self._pw   # refreshed by the caller's _targets()
        w = torch.empty(batch_size, dtype=torch.float32, device=self.device)
        check(self.lib.azg_pv_replay_gather_weight(ptr(vals), *self._ring(), self.nsym, ptr(d_ids), batch_size, ptr(w),
                                                   st), self.lib)
        return w

    # ------------------------------------------------------ position averaging
    @property
    def target_averaging(self) -> bool:
        return self._avg_on

    def set_target_averaging(self, on: bool) -> None:
        """Train on the mean targets of positions with the same board (nsym = 8: up to a
        rotation or a flip; nsym = 1: exact repeats).  Off, the default, samples the raw
        targets bit for bit and makes no new call."""
        on = bool(on)
        if on != self._avg_on:
            self._avg_on = on
            self._averaging_inputs_moved()

    def _ensure_averages(self) -> None:
        if self._avg is None:
            dev, c = self.device, self.cap_pos
            self._avg = {"keys": torch.zeros(c, dtype=torch.int64, device=dev),       # by ring index
                         "syms": torch.zeros(c, dtype=torch.int8, device=dev),        # by ring index
                         "pi_avg": torch.zeros((c, _PIX), dtype=torch.float32, device=dev),   # by slot, like pis
                         "z_avg": torch.zeros(c, dtype=torch.float32, device=dev),    # by slot
                         "pw_avg": None,                                              # by slot, with _pw
                         "group_first": torch.zeros(c, dtype=torch.int32, device=dev),   # by ring index
                         "group_size": torch.zeros(c, dtype=torch.int32, device=dev)}    # by ring index

    def refresh_averages(self) -> None:
        """Recompute the averaged targets if the ring, the policy weights or the setting
        changed since they were last computed (sample and sample_weighted call this).  Two
        kernels around torch's stable sort; no host sync."""
        if not self._avg_on or self._avg_ok or self.count < 1:
            return
        self._ensure_averages()
        a = self._avg
        if self._pw is not None and a["pw_avg"] is None:
            a["pw_avg"] = torch.ones(self.cap_pos, dtype=torch.float32, device=self.device)
        n = self.count
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device).cuda_stream
            check(self.lib.azg_pv_replay_canon_keys(ptr(self.stones), *self._ring(), self.nsym, ptr(a["keys"]),
                                                    ptr(a["syms"]), st), self.lib)
            keys_sorted, perm = torch.sort(a["keys"][:n], stable=True)   # equal keys adjacent, in ring order
            check(self.lib.azg_pv_replay_average(
                ptr(self.stones), ptr(self.pis), ptr(self.zs), ptr(self._pw), *self._ring(),
                ptr(keys_sorted), ptr(perm), ptr(a["syms"]), ptr(a["pi_avg"]), ptr(a["z_avg"]),
                ptr(a["pw_avg"]) if self._pw is not None else None, ptr(a["group_first"]), ptr(a["group_size"]), st),
                self.lib)
            # the caching allocator hands keys_sorted / perm back only to work queued later on
            # this stream, so they may go out of scope here
        self._avg_pw = self._pw is not None
        self._avg_ok = True

    def _targets(self):
        """(pis, zs) the gather reads: the averaged arrays, refreshed if stale, while
        averaging is on."""
        if not self._avg_on:
            return self.pis, self.zs
        self.refresh_averages()
        return self._avg["pi_avg"], self._avg["z_avg"]

    def duplicate_stats(self) -> dict:
        """{"positions", "groups", "largest"}: positions held, groups of equal boards among
        them, and the largest group's size (needs averaging on).  Synchronises: for logging."""
        sizes = self.get_group_sizes()
        firsts = self._ring_order_int("group_first")
        groups = int((firsts == np.arange(len(firsts))).sum())
        return {"positions": int(self.count), "groups": groups, "largest": int(sizes.max()) if len(sizes) else 0}

    def _ring_order_int(self, name: str) -> np.ndarray:
        if not self._avg_on:
            raise RuntimeError("position averaging is off: call set_target_averaging(True) first")
        if self.count < 1:
            return np.zeros(0, dtype=np.int32)
        self.refresh_averages()
        return self._avg[name][:self.count].cpu().numpy()

    def get_group_sizes(self) -> np.ndarray:
        """int32 [count] in ring order: the size of each position's group.  Synchronises."""
        return self._ring_order_int("group_size")

    def get_averaged_targets(self) -> dict:
        """Host arrays in ring order: "pi" [count,225], "z" [count], "policy_weight" [count]
        (None for a buffer without policy weights), "group_first", "group_size", "keys"
        (uint64), "syms".  Synchronises: for tests and inspection."""
        first = self._ring_order_int("group_first")
        a, n, order = self._avg, self.count, self._order()
        return {"pi": a["pi_avg"][order].cpu().numpy(), "z": a["z_avg"][order].cpu().numpy(),
                "policy_weight": a["pw_avg"][order].cpu().numpy() if self._avg_pw else None,
                "group_first": first, "group_size": a["group_size"][:n].cpu().numpy(),
                "keys": a["keys"][:n].cpu().numpy().view(np.uint64), "syms": a["syms"][:n].cpu().numpy()}

    # --------------------------------------------------------------- sampling
    def draw_ids(self, batch_size: int) -> list:
        """The indices a seeded random.sample(deque, batch_size) picks on the host buffer."""
        return random.sample(range(len(self)), batch_size)

    def sample(self, batch_size: int, ids=None, with_policy_weight: bool = False):
        """Device tensors (s [B,3,15,15], p [B,225], z [B,1]); no host sync.
        with_policy_weight: a fourth tensor [B], the positions' policy loss weights."""
        ids = np.asarray(self.draw_ids(batch_size) if ids is None else ids, dtype=np.int64).reshape(-1)
        if len(ids) != batch_size or batch_size < 1:
            raise ValueError(f"{len(ids)} ids for a batch of {batch_size}")
        if int(ids.min()) < 0 or int(ids.max()) >= len(self):
            raise ValueError(f"image id outside [0, {len(self)})")
        dev = self.device
        with torch.cuda.device(dev):
            d_ids = _pinned(ids, torch.int64).to(dev, non_blocking=True)
            return self._gather_batch(d_ids, batch_size, with_policy_weight, torch.cuda.current_stream(dev).cuda_stream)

    def _gather_batch(self, d_ids, batch_size: int, with_policy_weight: bool, st):
        """sample's and sample_weighted's tail: the batch of the device image ids d_ids, on stream st."""
        dev = self.device
        s = torch.empty((batch_size, 3, _N, _N), dtype=torch.float32, device=dev)
        p = torch.empty((batch_size, _PIX), dtype=torch.float32, device=dev)
        z = torch.empty((batch_size, 1), dtype=torch.float32, device=dev)
        pis, zs = self._targets()
        check(self.lib.azg_pv_replay_gather(ptr(self.stones), ptr(pis), ptr(zs), *self._ring(), self.nsym, ptr(d_ids),
                                            batch_size, ptr(s), ptr(p), ptr(z), st), self.lib)
        if with_policy_weight:
            return s, p, z, self._gather_policy_weight(d_ids, batch_size, st)
        return s, p, z

    def draw_words(self, batch_size: int) -> np.ndarray:
        """sample_weighted's default random words, uint64 [batch, 2]: two
        random.getrandbits(64) per element in element order, so random.seed governs them
        as it governs draw_ids."""
        return np.array([random.getrandbits(64) for _ in range(2 * batch_size)], dtype=np.uint64).reshape(batch_size, 2)

    def sample_weighted(self, batch_size: int, rnd=None, with_policy_weight: bool = False):
        """``sample``'s tensors for a batch drawn WITH replacement, each position in proportion
        to its weight and, with nsym = 8, one of its 8 images uniformly; no host sync and no
        host copy of the weights.  rnd (optional uint64 [batch, 2]): word 0 of an element
        picks the position (azg_pv_replay_draw), the low 3 bits of word 1 the image.  A
        buffer without weights draws as if every weight were 1.0 (and has weights from then
        on).  The running sums are scanned again only after the weights or the ring moved.
        with_policy_weight: a fourth tensor [B], the positions' policy loss weights."""
        if batch_size < 1 or self.count < 1:
            raise ValueError(f"a batch of {batch_size} from {self.count} positions")
        rnd = self.draw_words(batch_size) if rnd is None else np.asarray(rnd)
        if rnd.dtype != np.uint64 or rnd.shape != (batch_size, 2):
            raise ValueError(f"rnd must be uint64 [{batch_size}, 2], got {rnd.dtype} {rnd.shape}")
        self._ensure_weights()
        dev, h_rnd = self.device, _pinned(rnd.view(np.int64), torch.int64)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            if not self._prefix_ok:
                check(self.lib.azg_pv_replay_prefix(ptr(self._wq), *self._ring(), ptr(self._prefix), st), self.lib)
                self._prefix_ok = True
            d_rnd = h_rnd.to(dev, non_blocking=True)
            d_ids = torch.empty(batch_size, dtype=torch.int64, device=dev)
            check(self.lib.azg_pv_replay_draw(ptr(self._prefix), self.count, self.nsym, ptr(d_rnd), batch_size,
                                              ptr(d_ids), st), self.lib)
            return self._gather_batch(d_ids, batch_size, with_policy_weight, st)

    # ------------------------------------------------------------ host format
    def to_host(self) -> ReplayBuffer:
        """A ReplayBuffer whose deque holds the reference-format examples in deque order
        (nsym = 8: each position's 8 images in MCTS.symmetries' order), so
        save_replay_buffer keeps writing the reference pickle."""
        out = ReplayBuffer(capacity=self.capacity)
        if not self.count:
            return out
        order = self._order()
        st = self.stones[order].cpu().numpy().reshape(self.count, _N, _N)
        P = self.pis[order].cpu().numpy()
        zs = [float(v) for v in self.zs[order].cpu().numpy()]
        S = np.empty((self.count, 3, _N, _N), dtype=np.float32)
        S[:, 0] = st == 1
        S[:, 1] = st == 2
        S[:, 2] = 1.0
        if self.nsym == 1:
            out.add([(S[t], P[t], zs[t]) for t in range(self.count)])
        else:
            imgs = _images(S, P.reshape(self.count, _N, _N))
            out.add([(si[t], pi[t], zs[t]) for t in range(self.count) for si, pi in imgs])
        return out

    @classmethod
    def from_host(cls, buffer: ReplayBuffer, device) -> "DeviceReplayBuffer":
        """nsym = 8 from every eighth example when the host buffer is whole groups of 8
        dihedral images (capacity and length multiples of 8, every aligned group the
        images of its first element with one z); otherwise nsym = 1 with each example
        as its own entry."""
        examples = list(buffer.buffer)
        grouped = buffer.capacity % 8 == 0 and len(examples) % 8 == 0
        if grouped and examples:
            try:
                S, P, Z = _stack(examples)
            except ValueError:
                grouped = False
            else:
                G = len(S) // 8
                S8, P8, Z8 = S.reshape(G, 8, 3, _N, _N), P.reshape(G, 8, _PIX), Z.reshape(G, 8)
                grouped = bool((Z8 == Z8[:, :1]).all())
                if grouped:
                    for s, (si, pi) in enumerate(_images(S8[:, 0], P8[:, 0].reshape(G, _N, _N))):
                        if not (np.array_equal(si, S8[:, s]) and np.array_equal(pi, P8[:, s])):
                            grouped = False
                            break
        out = cls(buffer.capacity, device, symmetries=grouped)
        out.add_positions(examples[::8] if grouped else examples)
        return out


def new_device_buffer(loaded: Optional[ReplayBuffer], capacity: int, device) -> DeviceReplayBuffer:
    """The loop's buffer: a loaded host buffer moved to the device, or an empty one
    (nsym = 8 unless ``capacity`` is no multiple of 8, where only single images
    reproduce the deque's eviction)."""
    if loaded is not None:
        return DeviceReplayBuffer.from_host(loaded, device)
    return DeviceReplayBuffer(capacity, device, symmetries=capacity % 8 == 0)
