"""Self-play -> train -> evaluate loop with the reference's entry point and
semantics (reference train.py:575-845), running on the HIP engine:

  * ``train_alphazero(**kwargs)`` takes every reference keyword (worker / device
    keywords are accepted and ignored: self-play and evaluation run as batched
    concurrent games on the GPU instead of CPU process pools) plus
    ``n_res_blocks`` / ``channels`` (reference default net 3x64, network.py:145-146);
  * candidate self-play (train.py:656-751), ``len(buffer)//batch_size`` train
    steps per epoch (train.py:754-765), gating by win rate (train.py:767-827) with
    the reference's optimiser-state hand-over, per-iteration snapshot + buffer
    pickle (train.py:829-840);
  * under torchrun (one process per GPU): games shard across ranks, the train
    step is data-parallel with one RCCL all-reduce of the flat gradient,
    evaluation wins are summed across ranks, BN stats averaged per iteration;
  * beyond the reference: ``score_buffer`` and ``train_alphazero(score_new_games=True,
    history=[...])`` report eval-mode losses and policy metrics of a buffer / of the
    iteration's fresh games without training on them (PyTorchModel.score_batch).
"""
from __future__ import annotations

import os
import random
import time
from datetime import datetime
from typing import Optional, Tuple

import numpy as np
import torch

import distributed as D
from games.gomoku import Gomoku as GameClass
from mcts.new_mcts_alpha import MCTS
from engine import TowerFault, score_summary
from network import PyTorchModel
from selfplay import (BatchedSelfPlay, ReplayBuffer, load_replay_buffer, play_game_and_collect,  # noqa: F401
                      sample_action_from_pi, save_replay_buffer, selfplay_games, softmax_temperature)


def _tagged(gen, tag):
    """Re-label a search generator's leaf requests as (tag, X)."""
    try:
        req = next(gen)
        while True:
            req = gen.send((yield (tag, req)))
    except StopIteration as stop:
        return stop.value


def eval_game_gen(mcts_new, mcts_best, game, new_starts: bool):
    """train.py:165-245 / :418-487 game body: alternate the two searches, argmax moves."""
    move_number = 1
    while not game.is_game_over():
        if (game.current_player == 1 and new_starts) or (game.current_player == 2 and not new_starts):
            pi = yield from _tagged(mcts_new.run_gen(game, len(game.move_history)), "new")
        else:
            pi = yield from _tagged(mcts_best.run_gen(game, len(game.move_history)), "best")
        action = int(np.argmax(pi))
        game.do_move(divmod(action, game.size))
        move_number += 1
        if move_number > game.size * game.size:
            break
    return game.get_winner()


def evaluate_models(model_new: PyTorchModel, model_best: PyTorchModel, game_name: str = "gomoku",
                    n_games: int = 20, n_simulations: int = 100, cpuct: float = 1.0,
                    native: bool = True, record: Optional[list] = None,
                    search="reference") -> Tuple[int, float, int]:
    """(new_wins, win_rate, draws) over n_games (sharded across ranks), each opened
    by one random move in the centre 9x9 (train.py:440-445), new model first on
    even game indices.  native=True: both searches in C++ (mcts/native_mcts.NativeEval);
    native=False: Python searches under BatchedSelfPlay.  ``record`` (optional list)
    receives this rank's finished games.  ``search``: "reference", "alphazero" or
    {"new": mode, "best": mode} (NativeEval); the Python searches are the reference search only."""
    from _native_mcts import search_mode
    modes = search if isinstance(search, dict) else {"new": search, "best": search}
    if set(modes) != {"new", "best"}:
        raise ValueError(f'search must be a mode or {{"new": mode, "best": mode}}, got {search!r}')
    if any([search_mode(m) for m in modes.values()]) and not native:
        raise ValueError('search="alphazero" needs the native evaluation driver (native=True): the Python '
                         "generator search is the reference search only")
    size = model_new.board_size
    center, radius = size // 2, 4
    games, starts, winners, failure = [], [], [], None
    for i in D.shard(n_games):
        game = GameClass(size=size)
        game.do_move((random.randint(center - radius, center + radius), random.randint(center - radius, center + radius)))
        games.append(game)
        starts.append(i % 2 == 0)
    try:
        winners = _play_eval_games(model_new, model_best, games, starts, n_simulations, cpuct, native, modes)
    except Exception as e:   # every rank must still reach the collective below
        failure, winners = e, []
    fault = isinstance(failure, TowerFault)
    if record is not None:
        record.extend(games)
    new_wins = sum(1 for w, s in zip(winners, starts) if (w == 1 and s) or (w == 2 and not s))
    draws = sum(1 for w in winners if w == 0)
    eng = getattr(model_new, "engine", None)
    dev = eng.device if eng is not None else "cpu"
    tot = torch.tensor([new_wins, draws, int(failure is not None), int(fault)], dtype=torch.int64, device=dev)
    D.allreduce_sum_(tot)
    new_wins, draws, failed, faults = (int(v) for v in tot.tolist())
    if faults:   # an engine fault is never a lost game: every rank re-raises it
        raise TowerFault(f"evaluation: engine fault on {faults} rank(s)" + (f": {failure}" if failure else ""))
    if failed:   # all ranks agree; the caller counts it as a loss (reference train.py:803-805)
        raise RuntimeError(f"evaluation failed on {failed} rank(s)" + (f": {failure}" if failure else ""))
    return new_wins, new_wins / float(n_games), draws


def _play_eval_games(model_new, model_best, games, starts, n_simulations, cpuct, native, search="reference"):
    if not games:
        winners = []
    elif native:
        from mcts.native_mcts import NativeEval
        if hasattr(model_new, "board_evaluator") and hasattr(model_best, "board_evaluator"):
            # HIP models: int8 leaves, on-GPU encoding, both networks' batches in flight
            arena = NativeEval(None, GameClass, len(games), n_simulations, cpuct=cpuct,
                               evaluator_factories={"new": model_new.board_evaluator,
                                                    "best": model_best.board_evaluator}, search=search)
        else:
            arena = NativeEval({"new": model_new.predict, "best": model_best.predict}, GameClass, len(games),
                               n_simulations, cpuct=cpuct, search=search)
        winners = arena.play(games, ["new" if s else "best" for s in starts])
    else:
        gens = []
        for game, new_starts in zip(games, starts):
            mn = MCTS(GameClass, n_simulations, model_new, cpuct=cpuct, add_dirichlet_noise=False)
            mb = MCTS(GameClass, n_simulations, model_best, cpuct=cpuct, add_dirichlet_noise=False)
            gens.append(eval_game_gen(mn, mb, game, new_starts))
        winners = BatchedSelfPlay({"new": model_new, "best": model_best}).run(gens)
    return winners


def evaluate_models_mp(model_new, model_best, board_size, action_size, n_games, n_simulations, cpuct, **_ignored):
    """Reference train.py:492-569 signature; runs the batched GPU evaluation."""
    return evaluate_models(model_new, model_best, "gomoku", n_games=n_games, n_simulations=n_simulations, cpuct=cpuct)


def _new_model(board_size, action_size, device, blocks, channels, like: Optional[PyTorchModel] = None,
               with_opt: bool = False) -> PyTorchModel:
    m = PyTorchModel(board_size=board_size, action_size=action_size, device=device, n_res_blocks=blocks,
                     channels=channels)
    if like is not None:
        m.net.load_state_dict(like.net.state_dict())
        if with_opt:
            m.optimizer.load_state_dict(like.optimizer.state_dict())
    if D.world() > 1:
        m.grad_hook = D.grad_hook()
    return m


def _stack_examples(examples):
    states, pis, zs = zip(*examples)
    return (np.stack(states, axis=0).astype(np.float32), np.stack(pis, axis=0).astype(np.float32),
            np.array(zs, dtype=np.float32).reshape(-1, 1))


def score_buffer(model, buffer, batch_size: int = 512, max_examples: Optional[int] = None) -> dict:
    """Eval-mode loss and policy / value metrics (PyTorchModel.score_batch's dict) of a
    whole replay buffer, or of its first max_examples examples, training nothing.  A
    replay.DeviceReplayBuffer is swept in image-id order through its gather kernel and
    score_batch_device: nothing goes to the host but the sums.  A host ReplayBuffer is
    swept in deque order.  Both orders are the same examples (image i of the device
    buffer is element i of the deque), the batches' sums are added in float64 in sweep
    order, and no RNG is consumed."""
    n = len(buffer) if max_examples is None else min(len(buffer), int(max_examples))
    if n < 1 or batch_size < 1:
        raise ValueError(f"score_buffer: nothing to score (examples={n}, batch_size={batch_size})")
    total = np.zeros(8, dtype=np.float64)
    on_device = hasattr(buffer, "add_positions")   # replay.DeviceReplayBuffer
    examples = None if on_device else iter(buffer.buffer)
    for lo in range(0, n, batch_size):
        hi = min(n, lo + batch_size)
        if on_device:
            s, p, z = buffer.sample(hi - lo, ids=range(lo, hi))
            sums, _ = model.score_sums_device(s, p, z, max_batch=batch_size)
        else:
            s, p, z = _stack_examples([next(examples) for _ in range(hi - lo)])
            sums, _ = model.score_sums(s, p, z, max_batch=batch_size)
        total += sums
    return score_summary(total, n)


def _score_new_games(model, examples, limit: int) -> Optional[dict]:
    examples = examples[:max(0, int(limit))]
    return model.score_batch(*_stack_examples(examples)) if examples else None


def _score_surprise(model, examples) -> torch.Tensor:
    """The [n,8] device score records of ALL of examples under the model as it is now (field 0:
    the KL between the search's policy target and the net's policy), scored as
    _score_new_games scores but kept on the device."""
    s, t, z = _stack_examples(examples)
    dev = model.engine.device
    _, records = model.score_sums_device(torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev),
                                         torch.from_numpy(z).to(dev), per_board=True, max_batch=4096)
    return records


def _score_line(tag: str, d: Optional[dict]) -> str:
    if d is None:
        return f"  new games {tag}: no examples on this rank"
    return (f"  new games {tag}: n={d['n']} policy_loss={d['policy_loss']:.6f} value_loss={d['value_loss']:.6f} "
            f"total_loss={d['total_loss']:.6f} policy_top1={d['policy_top1']:.4f}")


def _load_sidecar(path: str, count: int) -> Optional[np.ndarray]:
    """Weights saved beside a buffer pickle of ``count`` positions, or None: no file, or another buffer's (length)."""
    if not count or not os.path.exists(path):
        return None
    saved = np.load(path, allow_pickle=False)
    return saved if saved.shape == (count,) else None


def train_alphazero(game_name: str = "gomoku", board_size: int = 15, num_iterations: int = 5,
                    games_per_iteration: int = 8, n_simulations: int = 50, buffer_size: int = 10000,
                    batch_size: int = 128, epochs_per_iter: int = 2, temp_threshold: int = 8, eval_games: int = 12,
                    eval_mcts_simulations: int = 200, win_rate_threshold: float = 0.55, cpuct: float = 1.2,
                    model_dir: str = "models", save_every: int = 1, pretrained_model_path: Optional[str] = None,
                    next_iteration_continuation: int = 1, dirichlet_alpha: float = 0.03,
                    dirichlet_epsilon: float = 0.25, dirichlet_n_moves: int = 30, n_res_blocks: int = 3,
                    channels: int = 64, device: Optional[str] = None, max_moves: Optional[int] = None,
                    device_buffer: bool = False, leaf_symmetry=None, eval_symmetry=None,
                    selfplay_precision: Optional[str] = None, score_new_games: bool = False,
                    score_max_examples: int = 4096, history: Optional[list] = None,
                    ema_decay: Optional[float] = None, surprise_weight: Optional[float] = None,
                    playout_cap_prob: Optional[float] = None, playout_cap_fast_sims: Optional[int] = None,
                    average_duplicates: bool = False, search: str = "reference", **reference_worker_kwargs):
    """Reference train.py:575-845.  `reference_worker_kwargs` (selfplay_num_workers,
    selfplay_device, ..., eval_torch_threads) are accepted for drop-in use and
    ignored: concurrency comes from batching games on the GPU.

    device_buffer=True keeps the replay buffer on the GPU (replay.DeviceReplayBuffer):
    self-play hands over canonical positions only, every batch is gathered (encoding +
    dihedral image) by a HIP kernel, and the step reads it in place.  Same batches, same
    model and same buffer pickle as the default host deque under the same seeds.

    leaf_symmetry / eval_symmetry (None, an int 0..7, "random" or "mean8"): evaluate the
    leaves of self-play, respectively of both gating models, under board symmetries
    (network.SymmetricModel; the transform runs inside the forward's kernels).  None, the
    default, is the loop without them, bit for bit.

    selfplay_precision ("exact", "fp16" or None = "exact"): the candidate model's eval
    precision (PyTorchModel.set_eval_precision) during the self-play phase of each
    iteration only; it is back at "exact" before the train steps and before gating,
    whatever self-play raises.  Gating always compares exact forwards.

    score_new_games=True: the candidate scores the iteration's fresh self-play examples
    (the first score_max_examples of them on this rank; PyTorchModel.score_batch: eval-mode
    losses and policy metrics, nothing trained) twice -- before they enter the buffer, when
    the net has never trained on them, and again after the iteration's train steps and BN
    sync -- both in "exact" precision, and rank 0 prints both.  history (a list): one dict
    per iteration is appended, {"iteration", "new_games_before", "new_games_after",
    "last_train_loss"} (the score dicts are None without score_new_games or without local
    examples; last_train_loss is None when the iteration did not train).  Scoring consumes
    no RNG and changes nothing about the buffer, the steps or gating; with the defaults no
    scoring call is made.

    ema_decay (None or in [0, 1)): every candidate keeps an exponential moving average of
    its weights (PyTorchModel.enable_ema), started at the weights the iteration starts from
    and moved by every train step inside the Adam kernel.  Gating plays the AVERAGE
    (model_candidate.ema_model()) against model_best, and on acceptance model_best takes the
    averaged weights with the candidate's optimiser state; the raw weights only train.
    history entries carry "ema_decay".  None, the default, makes no EMA call.

    surprise_weight (None or in [0, 1]; needs device_buffer=True): KataGo's policy surprise
    weighting.  Before this rank's fresh examples enter the buffer the candidate scores ALL
    of them in "exact" precision (score_sums_device, chunks of 4096; the records stay on the
    device) and their policy KL becomes their sampling weight,
    (1 - surprise_weight) + surprise_weight * n * KL_i / sum(KL)
    (DeviceReplayBuffer.add_positions(surprise=..., mix=...)); batches are then drawn in
    proportion to the weights on the device (sample_weighted: with replacement, governed by
    random.seed).  Old positions keep the weight they entered with.  The loss is not
    reweighted by it (see playout_cap_prob for per-example loss weights).  history entries carry "surprise_weight" and "buffer_ess" (the buffer's
    effective sample size in positions, None when off), and the weights are kept beside the
    buffer pickle in replay_weights_latest{suffix}.npy, applied on start when they match the
    loaded buffer's position count (otherwise every loaded position weighs 1.0).  None, the
    default, makes none of these calls: the loop samples uniformly as before.

    playout_cap_prob / playout_cap_fast_sims (both or neither; needs device_buffer=True, as
    the host deque and the reference pickle have no place for a weight): KataGo's playout cap
    randomization.  Each self-play move is searched at n_simulations with probability
    playout_cap_prob, else at playout_cap_fast_sims without root noise
    (NativeSelfPlay(playout_cap=...)).  Every position trains the value head; only fully
    searched ones train the policy head: positions enter the buffer with a policy loss
    weight of 1.0 or 0.0 (add_positions(policy_weight=...)), batches come with it
    (sample(with_policy_weight=True)) and the step weighs each example's policy loss by it
    (train_batch_device(policy_weight=...); the divisor stays the batch size).  The weights
    are kept beside the buffer pickle in replay_policy_weights_latest{suffix}.npy and
    restored on start when their length matches the loaded buffer (otherwise every loaded
    position counts 1.0).  history entries carry "playout_cap": None when off, else
    {"p_full", "fast_sims", "full_moves", "fast_moves"} of this rank's self-play.  With
    surprise_weight also on, the surprise of fast positions is set to 0 before they enter
    the buffer -- their policy target is not trusted, so they get the uniform share only.
    score_new_games is unchanged: its policy metrics then include the fast positions.
    None, the default, makes none of these calls.

    average_duplicates (needs device_buffer=True): position averaging.  Positions in the
    buffer with the same board -- up to a rotation or a flip -- train on the mean of their
    policy targets (weighted by their policy loss weights, so fast playout-cap searches never
    enter it) and the mean of their outcomes (DeviceReplayBuffer.set_target_averaging); the
    means are recomputed on the device once per buffer change, not per batch.  Which positions
    are drawn is unchanged, so it combines freely with surprise_weight and playout_cap_*.  The
    buffer pickle and the sidecars keep the raw targets.  history entries carry
    "buffer_groups": {"positions", "groups", "largest"} of the buffer the iteration trained
    on, None when off.  No effect on playing strength has been measured.  False, the default,
    makes none of these calls.

    search ("reference" or "alphazero"): the tree search of self-play and of both gating
    players.  "reference", the default, is the reference's search bit for bit -- it never
    reads the value head, so the value the loop trains cannot change a move.  "alphazero" backs
    every leaf's value up under virtual loss and re-mixes root noise at every noisy move
    (include/azg_mcts.h).  history entries carry "search"."""
    from _native_mcts import search_mode
    search_mode(search)   # ValueError on an unknown mode, before anything is built
    if average_duplicates and not device_buffer:
        raise ValueError("average_duplicates needs device_buffer=True (the host ReplayBuffer does not merge positions)")
    if (playout_cap_prob is None) != (playout_cap_fast_sims is None):
        raise ValueError("playout_cap_prob and playout_cap_fast_sims must be given together")
    playout_cap = None
    if playout_cap_prob is not None:
        if isinstance(playout_cap_prob, bool) or not 0.0 <= float(playout_cap_prob) <= 1.0:
            raise ValueError(f"playout_cap_prob must be in [0, 1], got {playout_cap_prob!r}")
        if isinstance(playout_cap_fast_sims, bool) or int(playout_cap_fast_sims) != playout_cap_fast_sims \
                or playout_cap_fast_sims < 0:
            raise ValueError(f"playout_cap_fast_sims must be an integer >= 0, got {playout_cap_fast_sims!r}")
        if not device_buffer:
            raise ValueError("playout_cap_prob needs device_buffer=True (the host ReplayBuffer carries no weights)")
        playout_cap = (float(playout_cap_prob), int(playout_cap_fast_sims))
    if surprise_weight is not None:
        if isinstance(surprise_weight, bool) or not isinstance(surprise_weight, (int, float, np.floating, np.integer)) \
                or not 0.0 <= float(surprise_weight) <= 1.0:
            raise ValueError(f"surprise_weight must be None or a number in [0, 1], got {surprise_weight!r}")
        if not device_buffer:
            raise ValueError("surprise_weight needs device_buffer=True (the host ReplayBuffer carries no weights)")
        surprise_weight = float(surprise_weight)
    if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
        raise ValueError(f"ema_decay must be None or in [0, 1), got {ema_decay!r}")
    if selfplay_precision not in (None, "exact", "fp16"):
        raise ValueError(f"selfplay_precision must be None, 'exact' or 'fp16', got {selfplay_precision!r}")
    r, w, _, dev = D.init_from_env()
    device = device or str(dev)
    main = r == 0
    os.makedirs(model_dir, exist_ok=True)
    action_size = board_size * board_size
    if pretrained_model_path and os.path.exists(pretrained_model_path):
        if main:
            print(f"loading pretrained model: {pretrained_model_path}")
        model_best = _new_model(board_size, action_size, device, n_res_blocks, channels)
        model_best.load(pretrained_model_path)
    else:
        if main:
            print("no pretrained model: initialising a new one")
        model_best = _new_model(board_size, action_size, device, n_res_blocks, channels)
    D.broadcast_model(model_best)
    model_candidate = _new_model(board_size, action_size, device, n_res_blocks, channels, like=model_best)
    if ema_decay is not None:
        model_candidate.enable_ema(ema_decay)

    suffix = "" if r == 0 else f"_rank{r}"
    buffer_path = os.path.join(model_dir, f"replay_buffer_latest{suffix}.pkl")
    if device_buffer:
        from replay import new_device_buffer
        buffer = new_device_buffer(load_replay_buffer(buffer_path, capacity=buffer_size), buffer_size, device)
        if average_duplicates:
            buffer.set_target_averaging(True)
    else:
        buffer = load_replay_buffer(buffer_path, capacity=buffer_size) or ReplayBuffer(capacity=buffer_size)
    sidecars = []   # (file, setter, getter) of the buffer's per-position weights in use, kept beside its pickle
    if surprise_weight is not None:
        sidecars.append((f"replay_weights_latest{suffix}.npy", buffer.set_weights, buffer.get_weights))
    if playout_cap is not None:
        sidecars.append((f"replay_policy_weights_latest{suffix}.npy", buffer.set_policy_weights, buffer.get_policy_weights))
    for file, setter, _ in sidecars:
        saved = _load_sidecar(os.path.join(model_dir, file), buffer.count)
        if saved is not None:
            setter(saved)
    sample = buffer.sample if surprise_weight is None else buffer.sample_weighted
    sample_kw = {} if playout_cap is None else {"with_policy_weight": True}
    # a device buffer of single images (nsym = 1: a loaded buffer that is not whole groups
    # of 8) takes the expanded examples like the deque; otherwise it forms the images itself
    host_symmetries = not device_buffer or buffer.nsym == 1
    temp_fn = lambda n: max(0.0, 1.0 - n / temp_threshold)
    max_moves = max_moves or board_size * board_size
    last = next_iteration_continuation + num_iterations - 1
    for it in range(next_iteration_continuation, last + 1):
        t0 = time.time()
        if main:
            print(f"\n=== ITER {it}/{last}: self-play (games={games_per_iteration}, sims={n_simulations}, "
                  f"ranks={w}) {datetime.now():%Y-%m-%d %H:%M:%S} ===")
        n_local = len(D.shard(games_per_iteration))
        sp_model = model_candidate if leaf_symmetry is None else model_candidate.symmetric(leaf_symmetry)
        try:
            if selfplay_precision not in (None, "exact"):
                model_candidate.set_eval_precision(selfplay_precision)
            cap_kw = {} if playout_cap is None else {"playout_cap": playout_cap}
            if search != "reference":
                cap_kw["search"] = search
            examples, winners, drv = selfplay_games(sp_model, GameClass, n_local, n_simulations, cpuct, temp_fn,
                                                    dirichlet_alpha, dirichlet_epsilon, dirichlet_n_moves,
                                                    max_moves=max_moves, board_size=board_size,
                                                    use_symmetries=host_symmetries, **cap_kw)
        finally:
            if selfplay_precision not in (None, "exact"):
                model_candidate.set_eval_precision("exact")
        pol_w = None
        if playout_cap is not None:   # the examples' 4th field leaves them here: the rest of the loop sees 3-tuples
            pol_w = np.array([e[3] for e in examples], dtype=np.float32)
            examples = [e[:3] for e in examples]
        score_before = score_after = None
        if score_new_games:   # before the examples enter the buffer: the net has never trained on them
            score_before = _score_new_games(model_candidate, examples, score_max_examples)
            if main:
                print(_score_line("before training", score_before))
        if device_buffer:
            add_kw = {} if pol_w is None else {"policy_weight": pol_w}
            if surprise_weight is not None and examples:
                kl = _score_surprise(model_candidate, examples)
                if pol_w is not None:   # a fast position's policy target is not trusted: no surprise, the uniform share only
                    kl = kl[:, 0] * torch.from_numpy((pol_w > 0).astype(np.float32)).to(kl.device)
                add_kw.update(surprise=kl, mix=surprise_weight)
            buffer.add_positions(examples, **add_kw)
        else:
            buffer.add(examples)
        t_sp = time.time() - t0
        if main:
            print(f"self-play done: {t_sp / 60:.2f} min, winners={winners}, buffer={len(buffer)}, "
                  f"leaf boards={drv.boards} ({drv.boards / max(t_sp, 1e-9):.0f} boards/s, "
                  f"max batch {drv.max_batch})")

        n_batches = D.allreduce_min_int(len(buffer) // batch_size, model_candidate.engine.device)
        loss_info = None
        if n_batches >= 1:
            for epoch in range(epochs_per_iter):
                te = time.time()
                for _ in range(n_batches):
                    s, p, z, *pw = sample(batch_size, **sample_kw)
                    if pw:   # playout cap: the batch comes with its policy loss weights
                        loss_info = model_candidate.train_batch_device(s, p, z, epochs=1, policy_weight=pw[0])
                    elif device_buffer:   # the synchronous step: a skipped step is redone as on the host path
                        loss_info = model_candidate.train_batch_device(s, p, z, epochs=1)
                    else:
                        loss_info = model_candidate.train_batch(s, p, z, epochs=1)
                if main:
                    print(f"  epoch {epoch + 1}/{epochs_per_iter} {time.time() - te:.1f}s last_loss={loss_info}")
            D.sync_bn_stats(model_candidate)
        elif main:
            print(f"not enough samples (buffer={len(buffer)}, need {batch_size}): skip training")
        if score_new_games:
            score_after = _score_new_games(model_candidate, examples, score_max_examples)
            if main:
                print(_score_line("after training", score_after))
        if history is not None:
            history.append({"iteration": it, "new_games_before": score_before, "new_games_after": score_after,
                            "last_train_loss": loss_info, "ema_decay": ema_decay,
                            "surprise_weight": surprise_weight,
                            "buffer_ess": None if surprise_weight is None else buffer.effective_sample_size(),
                            "playout_cap": None if playout_cap is None else
                            {"p_full": playout_cap[0], "fast_sims": playout_cap[1],
                             "full_moves": drv.full_moves, "fast_moves": drv.fast_moves},
                            "buffer_groups": buffer.duplicate_stats() if average_duplicates else None,
                            "search": search})

        te = time.time()
        # with EMA on, the gated net is the average of the candidate's weights, not its last step
        gated = model_candidate if ema_decay is None else model_candidate.ema_model()
        try:
            ev_new, ev_best = ((gated, model_best) if eval_symmetry is None else
                               (gated.symmetric(eval_symmetry), model_best.symmetric(eval_symmetry)))
            new_wins, win_rate, draws = evaluate_models(ev_new, ev_best, game_name, n_games=eval_games,
                                                        n_simulations=eval_mcts_simulations, cpuct=cpuct,
                                                        **({} if search == "reference" else {"search": search}))
        except TowerFault:
            # a forward that computed on stale inputs and could not be recomputed: an
            # engine fault, not a lost evaluation -- never counted as a rejection
            raise
        except Exception as e:  # reference: evaluation failure counts as a loss (train.py:803-805)
            print(f"evaluation failed: {e}")
            new_wins, win_rate, draws = 0, 0.0, 0
        if main:
            print(f"eval done: {(time.time() - te) / 60:.2f} min, win_rate={win_rate:.3f} "
                  f"({new_wins}/{eval_games}), draws={draws}")
        if win_rate >= win_rate_threshold:
            if main:
                print(" candidate accepted -> best")
            model_best.net.load_state_dict(model_candidate.net.state_dict() if ema_decay is None
                                           else model_candidate.ema_state_dict())
            model_best.optimizer.load_state_dict(model_candidate.optimizer.state_dict())
        elif main:
            print(" candidate rejected -> restore from best")
        model_candidate = _new_model(board_size, action_size, device, n_res_blocks, channels, like=model_best,
                                     with_opt=True)
        if ema_decay is not None:
            model_candidate.enable_ema(ema_decay)
        if main and it % save_every == 0:
            path = os.path.join(model_dir, f"snapshot_iter{it}_{datetime.now():%Y%m%d_%H%M%S}.pt")
            model_best.save(path)
            print(f" saved snapshot: {path}")
        save_replay_buffer(buffer.to_host() if device_buffer else buffer, buffer_path)
        for file, _, getter in sidecars:
            np.save(os.path.join(model_dir, file), getter())
        if main:
            print(f"iteration {it} done in {(time.time() - t0) / 60:.2f} min; winners {winners}")
    if main:
        print("\n=== training done ===")
    return model_best


if __name__ == "__main__":
    train_alphazero(game_name="gomoku", board_size=15, num_iterations=300, games_per_iteration=70,
                    n_simulations=1600, cpuct=1.0, buffer_size=60000, batch_size=128, epochs_per_iter=5,
                    temp_threshold=10, eval_games=60, eval_mcts_simulations=1600, win_rate_threshold=0.5,
                    dirichlet_alpha=0.05, dirichlet_epsilon=0.15, dirichlet_n_moves=10, model_dir="models",
                    save_every=1, pretrained_model_path=None, next_iteration_continuation=1)
