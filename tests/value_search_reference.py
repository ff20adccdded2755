"""Python restatement of the native value search (AZG_MCTS_SEARCH_VALUE, specified in
include/azg_mcts.h): AlphaZero's search with the net's value backed up under virtual loss,
over a leaf queue of batch_size.  Plain dicts and lists, one edge at a time, written from
the specification and not from the engine, so the tests can compare the two bit for bit.

``ValueSearch`` has the interface of mcts.new_mcts_alpha.MCTS (``run_gen`` yields leaf
batches and is sent (probs, values); ``run``, ``drive``, ``symmetries``, ``clear_tree``),
so it also plays whole games through selfplay.play_game_gen.  Test infrastructure only."""
import math

import numpy as np

from mcts.new_mcts_alpha import MCTS as _PyMCTS


class ValueSearch:
    symmetries = _PyMCTS.symmetries

    def __init__(self, game_class, n_simulations, nn_model=None, cpuct=1.0, batch_size=32, dirichlet_alpha=0.03,
                 epsilon=0.03, apply_dirichlet_n_first_moves=10, add_dirichlet_noise=True, rng=None):
        self.game_class = game_class
        self.n_simulations = n_simulations
        self.nn_model = nn_model
        self.cpuct = float(cpuct)
        self.batch_size = batch_size
        self.dirichlet_alpha = dirichlet_alpha
        self.epsilon = epsilon
        self.apply_dirichlet_n_first_moves = apply_dirichlet_n_first_moves
        self.add_dirichlet_noise = add_dirichlet_noise
        self.rng = np.random if rng is None else rng
        self.clear_tree()

    def clear_tree(self):
        self.tree = {}            # key -> node
        self.mixed_key = None     # the node holding the last mixed root prior
        self.root_key = None
        self.collisions = 0

    @staticmethod
    def key(game):
        return game.board.tobytes() + bytes([game.current_player])

    def tree_size(self):
        return len(self.tree)

    def inflight(self):
        return sum(sum(nd["O"]) for nd in self.tree.values())

    def drive(self, gen):
        try:
            req = next(gen)
            while True:
                req = gen.send(self.nn_model.predict(req))
        except StopIteration as stop:
            return stop.value

    def run(self, game, move_number):
        return self.drive(self.run_gen(game, move_number))

    # ------------------------------------------------------------------ the rules
    def select(self, nd):
        """score = q + u in float64 over valid actions; ties to the lowest index."""
        A = len(nd["N"])
        n = [nd["N"][a] + nd["O"][a] for a in range(A)]
        S = sum(n[a] for a in range(A) if nd["valid"][a])
        sq = math.sqrt(float(1 + S))
        best, best_score = -1, 0.0
        for a in range(A):
            if not nd["valid"][a]:
                continue
            w = float(nd["W"][a]) - float(nd["O"][a])
            q = w / float(n[a]) if n[a] > 0 else 0.0
            p = float(nd["P64"][a]) if nd["P64"] is not None else float(nd["P"][a])
            u = ((self.cpuct * p) * sq) / float(1 + n[a])
            s = q + u
            if best < 0 or s > best_score:
                best, best_score = a, s
        return best

    def backup(self, path, x):
        x = np.float32(x)
        for key, a in reversed(path):
            x = np.float32(-x)
            nd = self.tree[key]
            nd["W"][a] = np.float32(nd["W"][a] + x)
            nd["N"][a] += 1

    def mix(self, key):
        """The Dirichlet mix, always from the node's clean float32 prior."""
        p32 = self.tree[key]["P"]
        noise = self.rng.dirichlet([self.dirichlet_alpha] * len(p32))
        p = (1 - self.epsilon) * p32 + self.epsilon * noise
        p /= np.sum(p)
        self.tree[key]["P64"] = p
        self.mixed_key = key

    def run_gen(self, game, move_number):
        root_key = self.root_key = self.key(game)
        noisy = bool(self.add_dirichlet_noise) and move_number < self.apply_dirichlet_n_first_moves
        if self.mixed_key is not None:                 # the previous root's mix is dropped
            self.tree[self.mixed_key]["P64"] = None
            self.mixed_key = None
        if noisy and root_key in self.tree:            # noise at every noisy move
            self.mix(root_key)
        queue = []                                     # (key, state, path)
        sims_left = self.n_simulations
        waiting = None                                 # the simulation suspended by a collision
        while True:
            if waiting is None:
                if sims_left == 0:
                    if queue:                          # final flush
                        yield from self.flush(queue, noisy, root_key)
                    break
                sims_left -= 1
                g, path = game.clone(), []
            else:
                g, path = waiting                      # its state is a node now
                waiting = None
            emit = False
            while True:
                if g.is_game_over():
                    self.backup(path, 0.0 if g.get_winner() == 0 else -1.0)
                    break
                k = self.key(g)
                if k not in self.tree:
                    if any(k == qk for qk, _, _ in queue):      # collision: emit at once, wait here
                        waiting = (g, path)
                        self.collisions += 1
                        emit = True
                        break
                    for nk, a in path:
                        self.tree[nk]["O"][a] += 1
                    queue.append((k, g.clone(), list(path)))
                    emit = len(queue) >= self.batch_size
                    break
                a = self.select(self.tree[k])
                path.append((k, a))
                g.do_move(divmod(a, g.size))
            if emit:
                yield from self.flush(queue, noisy, root_key)
        assert self.inflight() == 0
        counts = np.array(self.tree[root_key]["N"], dtype=np.float32)
        total = np.sum(counts)
        if total > 0:
            return counts / total
        valid = np.array(self.tree[root_key]["valid"], dtype=np.float32)
        return valid / np.sum(valid)

    def flush(self, queue, noisy, root_key):
        X = np.stack([g.get_encoded_state() for _, g, _ in queue], axis=0).astype(np.float32)
        probs, values = yield X
        values = np.asarray(values, dtype=np.float32).reshape(-1)
        for i, (k, g, path) in enumerate(queue):
            valid = g.get_valid_moves()
            p = np.asarray(probs[i], dtype=np.float32).flatten() * valid
            if np.sum(p) < 1e-8:
                p = valid / np.sum(valid)
            A = len(p)
            self.tree[k] = {"P": p.astype(np.float32), "P64": None, "V": np.float32(values[i]),
                            "N": [0] * A, "W": [np.float32(0.0)] * A, "O": [0] * A,
                            "valid": [bool(x) for x in valid]}
            if noisy and k == root_key:
                self.mix(k)
            for nk, a in path:                          # the path's virtual loss goes
                self.tree[nk]["O"][a] -= 1
            self.backup(path, values[i])
        del queue[:]

    def root_value(self):
        """(q, v_net, visits) of the last root, as azg_mcts_get_root_value defines them."""
        nd = self.tree[self.root_key]
        w = 0.0
        for x in nd["W"]:
            w += float(x)
        n = sum(nd["N"])
        return (w / float(n) if n > 0 else 0.0), float(nd["V"]), n
