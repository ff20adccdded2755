"""ctypes binding of libazg_mcts.so (C-ABI declared in include/azg_mcts.h): the
native multi-game batched-leaf search.  Host code only (no HIP); the library is
required -- there is no Python fallback behind the native search classes."""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AZG_MCTS_LIB", os.path.join(_HERE, "libazg_mcts.so"))

IDLE, NEED_EVAL, DONE = 0, 1, 2
# search="reference": the reference's search bit for bit, which never reads the net's value;
# search="alphazero": value backup under virtual loss (AZG_MCTS_SEARCH_VALUE in azg_mcts.h)
SEARCH_MODES = {"reference": 0, "alphazero": 1}


def search_mode(search) -> int:
    """The C-ABI mode of a ``search=`` keyword; ValueError on anything else."""
    if not isinstance(search, str) or search not in SEARCH_MODES:
        raise ValueError(f"search must be one of {sorted(SEARCH_MODES)}, got {search!r}")
    return SEARCH_MODES[search]


class MctsConfig(ctypes.Structure):
    _fields_ = [("rules", ctypes.c_int32), ("board", ctypes.c_int32), ("n_simulations", ctypes.c_int32),
                ("batch_size", ctypes.c_int32), ("apply_dirichlet_n_first_moves", ctypes.c_int32),
                ("add_dirichlet_noise", ctypes.c_int32), ("cpuct", ctypes.c_double),
                ("dirichlet_alpha", ctypes.c_double), ("epsilon", ctypes.c_double)]


_P = ctypes.c_void_p
_I32 = ctypes.c_int32
_SIGS = {
    "azg_mcts_last_error": (ctypes.c_char_p, []),
    "azg_mcts_create": (_I32, [ctypes.POINTER(MctsConfig), _I32, ctypes.POINTER(_P)]),
    "azg_mcts_destroy": (_I32, [_P]),
    "azg_mcts_set_root": (_I32, [_P, _I32, _P, _I32, _I32, _I32, _I32, _I32, _I32]),
    "azg_mcts_set_budget": (_I32, [_P, _I32, _I32, _I32]),
    "azg_mcts_advance": (_I32, [_P, _P, _P, _P, ctypes.POINTER(_I32), _I32]),
    "azg_mcts_advance_boards": (_I32, [_P, _P, _P, _P, _P, ctypes.POINTER(_I32), _I32]),
    "azg_mcts_feed": (_I32, [_P, _P, _P]),
    "azg_mcts_noise_request": (_I32, [_P, _I32, _P]),
    "azg_mcts_set_root_prior": (_I32, [_P, _I32, _P]),
    "azg_mcts_get_pi": (_I32, [_P, _I32, _P]),
    "azg_mcts_set_search_mode": (_I32, [_P, _I32]),
    "azg_mcts_get_search_mode": (_I32, [_P]),
    "azg_mcts_get_root_value": (_I32, [_P, _I32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float),
                                       ctypes.POINTER(ctypes.c_int64)]),
    "azg_mcts_inflight": (ctypes.c_int64, [_P, _I32]),
    "azg_mcts_collisions": (ctypes.c_int64, [_P, _I32]),
    "azg_mcts_clear": (_I32, [_P, _I32]),
    "azg_mcts_tree_size": (ctypes.c_int64, [_P, _I32]),
    "azg_mcts_replay": (_I32, [_I32, _I32, _P, _I32, _I32, _I32, _P, _I32, _P, _P, _P, _P]),
}
EXPORTS = tuple(_SIGS)

_lib = None


def load_library() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"native MCTS library not found at {LIB_PATH}. Build it with "
                           "`make -C alphazero-gomoku_amd/csrc` (or __graft_entry__.build()).")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError("libazg_mcts: " + (load_library().azg_mcts_last_error() or b"?").decode())


def _addr(a: np.ndarray) -> int:
    return a.ctypes.data


class SearchForest:
    """One native search tree per game slot.  Thin, allocation-free wrapper: the
    leaf/pi staging arrays are owned here and reused every round."""

    def __init__(self, n_games: int, n_simulations: int, rules: int = 0, board: int = 15, cpuct: float = 1.0,
                 batch_size: int = 32, dirichlet_alpha: float = 0.03, epsilon: float = 0.03,
                 apply_dirichlet_n_first_moves: int = 10, add_dirichlet_noise: bool = True, n_threads: int = 0,
                 search: str = "reference"):
        mode = search_mode(search)
        self.search = search
        self.lib = load_library()
        self.n_games = int(n_games)
        self.board = int(board)
        self.A = self.board * self.board
        self.batch_size = int(batch_size)
        self.n_threads = int(n_threads)
        self.cfg = MctsConfig(int(rules), self.board, int(n_simulations), self.batch_size,
                              int(apply_dirichlet_n_first_moves), int(bool(add_dirichlet_noise)), float(cpuct),
                              float(dirichlet_alpha), float(epsilon))
        self.h = _P()
        _check(self.lib.azg_mcts_create(ctypes.byref(self.cfg), self.n_games, ctypes.byref(self.h)))
        if mode:   # the default makes no call: a forest that never asks is the reference search
            self.set_search_mode(mode)
        self._leaves = None
        self.counts = np.zeros(self.n_games, np.int32)
        self.status = np.zeros(self.n_games, np.int32)
        self._p32 = np.empty(self.A, np.float32)

    @property
    def leaves(self) -> np.ndarray:
        """float32 [n_games*batch_size, 3, H, W] staging for advance() (allocated on first use)."""
        if self._leaves is None:
            self._leaves = np.empty((self.n_games * self.batch_size, 3, self.board, self.board), np.float32)
        return self._leaves

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self.lib.azg_mcts_destroy(h)
            self.h = None

    def set_root(self, g: int, game, move_number: int) -> None:
        board = np.ascontiguousarray(np.asarray(game.board).reshape(-1), dtype=np.int8)
        last = getattr(game, "last_move", None)
        lr, lc = (-1, -1) if last is None else (int(last[0]), int(last[1]))
        caps = getattr(game, "captures", None) or {1: 0, 2: 0}
        _check(self.lib.azg_mcts_set_root(self.h, g, _addr(board), int(game.current_player), lr, lc,
                                          int(caps[1]), int(caps[2]), int(move_number)))

    def set_search_mode(self, mode: int) -> None:
        """azg_mcts_set_search_mode: 0 reference, 1 value search; only with every tree empty and
        no search in progress."""
        _check(self.lib.azg_mcts_set_search_mode(self.h, int(mode)))

    def get_search_mode(self) -> int:
        return int(self.lib.azg_mcts_get_search_mode(self.h))

    def root_value(self, g: int):
        """(q, v_net, visits) of slot g's root: q = sum(W)/sum(N) over its actions from the
        root mover's view (0.0 without visits), the net's value of the root, sum(N)."""
        q, v, n = ctypes.c_double(0.0), ctypes.c_float(0.0), ctypes.c_int64(0)
        _check(self.lib.azg_mcts_get_root_value(self.h, g, ctypes.byref(q), ctypes.byref(v), ctypes.byref(n)))
        return q.value, v.value, n.value

    def inflight(self, g: int) -> int:
        """Test hook: the sum of slot g's in-flight counters (virtual losses)."""
        return int(self.lib.azg_mcts_inflight(self.h, g))

    def collisions(self, g: int) -> int:
        """Simulations of slot g that met a queued leaf (early emits) since its last clear."""
        return int(self.lib.azg_mcts_collisions(self.h, g))

    def set_budget(self, g: int, n_simulations: int = -1, root_noise: int = -1) -> None:
        """Slot g's simulation budget and whether its root may get Dirichlet noise, from the
        next set_root on (azg_mcts_set_budget); a negative value means the forest's own
        n_simulations / add_dirichlet_noise."""
        _check(self.lib.azg_mcts_set_budget(self.h, g, int(n_simulations), int(root_noise)))

    def advance(self) -> int:
        n = _I32(0)
        _check(self.lib.azg_mcts_advance(self.h, _addr(self.leaves), _addr(self.counts), _addr(self.status),
                                         ctypes.byref(n), self.n_threads))
        return n.value

    def advance_boards(self, boards: np.ndarray, players: np.ndarray) -> int:
        """advance() with the leaves written as int8 boards [n,225] + side to move [n]
        into the given C-contiguous int8 arrays (capacity n_games*batch_size), e.g.
        numpy views of pinned host tensors."""
        assert boards.dtype == np.int8 and players.dtype == np.int8
        assert boards.flags.c_contiguous and players.flags.c_contiguous
        assert boards.size >= self.n_games * self.batch_size * self.A and players.size >= self.n_games * self.batch_size
        n = _I32(0)
        _check(self.lib.azg_mcts_advance_boards(self.h, _addr(boards), _addr(players), _addr(self.counts),
                                                _addr(self.status), ctypes.byref(n), self.n_threads))
        return n.value

    def feed(self, probs: np.ndarray, values: np.ndarray) -> None:
        probs = np.ascontiguousarray(probs, dtype=np.float32)
        values = np.ascontiguousarray(values, dtype=np.float32)
        _check(self.lib.azg_mcts_feed(self.h, _addr(probs), _addr(values)))

    def noise_request(self, g: int):
        r = self.lib.azg_mcts_noise_request(self.h, g, _addr(self._p32))
        if r < 0:
            raise RuntimeError("libazg_mcts: bad game index")
        return self._p32.copy() if r else None

    def set_root_prior(self, g: int, p64: np.ndarray) -> None:
        p64 = np.ascontiguousarray(p64, dtype=np.float64)
        _check(self.lib.azg_mcts_set_root_prior(self.h, g, _addr(p64)))

    def get_pi(self, g: int) -> np.ndarray:
        pi = np.empty(self.A, np.float32)
        _check(self.lib.azg_mcts_get_pi(self.h, g, _addr(pi)))
        return pi

    def clear(self, g: int) -> None:
        _check(self.lib.azg_mcts_clear(self.h, g))

    def tree_size(self, g: int) -> int:
        return int(self.lib.azg_mcts_tree_size(self.h, g))


def replay(rules: int, actions, start=None, player: int = 1, caps=(0, 0), board: int = 15):
    """Play `actions` with the native rule engine (azg_mcts_replay): per move the
    board [n, board*board] int8, captured pairs [n, 2], winner [n], game over [n]."""
    lib = load_library()
    acts = np.ascontiguousarray(np.asarray(actions, dtype=np.int32).reshape(-1))
    n = int(acts.size)
    A = board * board
    st = None if start is None else np.ascontiguousarray(np.asarray(start, dtype=np.int8).reshape(-1))
    boards = np.zeros((n, A), np.int8)
    cap = np.zeros((n, 2), np.int32)
    win = np.zeros(n, np.int32)
    over = np.zeros(n, np.int32)
    _check(lib.azg_mcts_replay(int(rules), int(board), None if st is None else _addr(st), int(player), int(caps[0]),
                               int(caps[1]), _addr(acts), n, _addr(boards), _addr(cap), _addr(win), _addr(over)))
    return boards, cap, win, over.astype(bool)
