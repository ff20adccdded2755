"""Symmetric leaf evaluation on the GPU (azg_pv_forward_boards_sym): the per-leaf transform
and the mean over the 8 images, bit for bit against "transform on the host, plain forward,
transform back" -- the forward is batch-independent, so the two must agree exactly."""
import numpy as np
import pytest
import torch

from conftest import has_gpu
from _native import TUNE
from oracle.boards import synth_positions

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]

_MODELS, _CASES = {}, {}


def model(blocks, ch, seed=0):
    from network import PyTorchModel
    key = (blocks, ch, seed)
    if key not in _MODELS:
        torch.manual_seed(seed)
        _MODELS[key] = PyTorchModel(board_size=15, device="cuda", n_res_blocks=blocks, channels=ch)
    return _MODELS[key]


def positions(B, seed):
    """int8 boards [B,225] + players of oracle.boards.synth_positions; the condition on the
    inputs: at least three quarters of the boards have eight pairwise distinct images, and
    both sides to move occur."""
    from network import apply_symmetry
    b, p = synth_positions(B, seed=seed)
    b = np.ascontiguousarray(b, np.int8).reshape(B, 225)
    p = np.ascontiguousarray(p, np.int8)
    distinct = sum(len({apply_symmetry(x, s).tobytes() for s in range(8)}) == 8 for x in b)
    assert 4 * distinct >= 3 * B, (B, seed, distinct)
    assert set(np.unique(p)) == {1, 2}
    return b, p


def host_reference(m, b, p):
    """Per symmetry s: transform the boards on the host, the plain forward (unmasked and
    masked), the per-square results mapped back.  -> probs [8,B,225], priors [8,B,225],
    values [8,B,1]."""
    from network import apply_symmetry, invert_symmetry
    P, R, V = [], [], []
    for s in range(8):
        img = apply_symmetry(b, s)
        probs, v = m.predict_boards(img, p, masked=False)
        priors, v2 = m.predict_boards(img, p, masked=True)
        assert np.array_equal(v, v2)
        P.append(invert_symmetry(probs, s))
        R.append(invert_symmetry(priors, s))
        V.append(v)
    return np.stack(P), np.stack(R), np.stack(V)


def case(blocks, ch, B, seed):
    """Computed once and shared: the model, the inputs and the host reference (read-only)."""
    key = (blocks, ch, B, seed)
    if key not in _CASES:
        m = model(blocks, ch)
        b, p = positions(B, seed)
        ref = host_reference(m, b, p)
        for a in ref:
            a.setflags(write=False)
        _CASES[key] = (m, b, p) + ref
    return _CASES[key]


def seq_mean8(terms):
    """((t0 + t1) + ... + t7) * 0.125 in float32, the order the kernel adds in."""
    acc = np.zeros_like(terms[0], dtype=np.float32)
    for t in terms:
        acc = (acc + t.astype(np.float32)).astype(np.float32)
    return (acc * np.float32(0.125)).astype(np.float32)


# (1, 64): C = 64; (2, 128, 7): the default arithmetic, boards split over three workgroups;
# (2, 128, 300): one workgroup per board plus the split tail, fused projection; (1, 256): C = 256
@pytest.mark.parametrize("blocks,ch,B,seed", [(1, 64, 5, 11), (2, 128, 7, 12), (2, 128, 300, 13), (1, 256, 9, 14)])
def test_per_board_symmetry_is_bitwise_the_host_transform(blocks, ch, B, seed):
    m, b, p, P, R, V = case(blocks, ch, B, seed)
    syms = np.random.default_rng(seed).permutation(np.arange(B) % 8).astype(np.int8)
    rows = np.arange(B)
    want_probs, want_priors, want_values = P[syms, rows], R[syms, rows], V[syms, rows]
    probs, values = m.predict_boards(b, p, masked=False, symmetry=syms)
    priors, values2 = m.predict_boards(b, p, masked=True, symmetry=syms)
    assert probs.dtype == np.float32 and probs.shape == (B, 225) and values.shape == (B, 1)
    assert np.array_equal(probs, want_probs), float(np.abs(probs - want_probs).max())
    assert np.array_equal(priors, want_priors), float(np.abs(priors - want_priors).max())
    assert np.array_equal(values, want_values) and np.array_equal(values2, want_values)
    # no symmetry / all-zero symmetries / a scalar: the plain call
    for sym in (None, np.zeros(B, np.int8), 0):
        p0, v0 = m.predict_boards(b, p, masked=False, symmetry=sym)
        assert np.array_equal(p0, P[0]) and np.array_equal(v0, V[0])
        r0, _ = m.predict_boards(b, p, masked=True, symmetry=sym)
        assert np.array_equal(r0, R[0])
    p3, v3 = m.predict_boards(b, p, masked=False, symmetry=3)
    assert np.array_equal(p3, P[3]) and np.array_equal(v3, V[3])
    # not an identity implementation: some board with s != 0 differs from the plain result
    moved = [i for i in range(B) if syms[i] != 0 and not np.array_equal(probs[i], P[0][i])]
    assert moved
    assert any(not np.array_equal(values[i], V[0][i]) for i in range(B) if syms[i] != 0)
    # priors: exactly 0 on the ORIGINAL board's occupied squares, probs elsewhere
    assert np.all(priors[b != 0] == 0.0)
    assert np.array_equal(priors, probs * (b == 0))
    if (blocks, ch, B) == (1, 64, 5):   # the VALU reference stem (tuning key 9 = 0): the same bits
        import _native
        lib = _native.load_library()
        prev = lib.azg_pv_set_tuning(TUNE.STEM_KERNEL, 0)
        try:
            pv, vv = m.predict_boards(b, p, masked=False, symmetry=syms)
            rv, _ = m.predict_boards(b, p, masked=True, symmetry=syms)
            mv, mvv = m.predict_boards(b, p, masked=False, symmetry="mean8")
        finally:
            lib.azg_pv_set_tuning(TUNE.STEM_KERNEL, prev)
        assert np.array_equal(pv, probs) and np.array_equal(vv, values) and np.array_equal(rv, priors)
        assert np.array_equal(mv, seq_mean8(P)) and np.array_equal(mvv, seq_mean8(V))


@pytest.mark.parametrize("blocks,ch,B,seed", [(2, 128, 7, 12), (1, 64, 5, 11)])
def test_mean8_is_bitwise_the_sequential_sum_and_equivariant(blocks, ch, B, seed):
    from network import apply_symmetry, invert_symmetry
    m, b, p, P, R, V = case(blocks, ch, B, seed)
    probs, values = m.predict_boards(b, p, masked=False, symmetry="mean8")
    priors, values2 = m.predict_boards(b, p, masked=True, symmetry="mean8")
    want = seq_mean8(P)
    assert np.array_equal(probs, want), float(np.abs(probs - want).max())
    assert np.array_equal(values, seq_mean8(V)) and np.array_equal(values2, values)
    assert np.array_equal(priors, probs * (b == 0)) and np.all(priors[b != 0] == 0.0)
    assert not np.array_equal(probs, P[0])
    # equivariance: the same eight terms summed in another order.  Seven float32 additions of
    # partial sums of at most 8, scaled by 1/8, bound each side's error by 7 * 2^-24 ~ 4.2e-7
    for s in range(8):
        ps, vs = m.predict_boards(apply_symmetry(b, s), p, masked=False, symmetry="mean8")
        dp = float(np.abs(invert_symmetry(ps, s) - probs).max())
        dv = float(np.abs(vs - values).max())
        print(f"mean8 equivariance {blocks}x{ch} s={s}: dprobs={dp:.3e} dvalues={dv:.3e}")
        assert dp <= 1e-6 and dv <= 1e-6, (s, dp, dv)


def test_evaluator_symmetries():
    from network import BoardEvaluator
    m = model(2, 128)
    n = 40
    b, p = positions(n, 15)

    def run(ev):
        ev.boards[:n] = b
        ev.players[:n] = p
        ev.submit(n)
        priors, values = ev.wait()
        return priors.copy(), values.copy()

    ev = m.board_evaluator(64, symmetry="random", seed=5)
    state = np.random.get_state()
    priors, values = run(ev)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    syms = ev.syms[:n].copy()
    assert syms.dtype == np.int8 and syms.min() >= 0 and syms.max() <= 7 and len(np.unique(syms)) > 1
    wp, wv = m.predict_boards(b, p, masked=True, symmetry=syms)
    assert np.array_equal(priors, wp) and np.array_equal(values, wv)
    ev2 = m.board_evaluator(64, symmetry="random", seed=5)
    run(ev2)
    assert np.array_equal(ev2.syms[:n], syms)
    run(ev2)                                  # the next batch draws again
    assert not np.array_equal(ev2.syms[:n], syms)
    # None: today's evaluator
    plain_p, plain_v = m.predict_boards(b, p, masked=True)
    for e in (m.board_evaluator(64), BoardEvaluator(m, 64, symmetry=None)):
        assert e.syms is None and e.d_syms is None
        gp, gv = run(e)
        assert np.array_equal(gp, plain_p) and np.array_equal(gv, plain_v)
    g5p, g5v = run(m.board_evaluator(64, symmetry=5))
    w5p, w5v = m.predict_boards(b, p, masked=True, symmetry=5)
    assert np.array_equal(g5p, w5p) and np.array_equal(g5v, w5v)
    gmp, gmv = run(m.board_evaluator(64, symmetry="mean8"))
    wmp, wmv = m.predict_boards(b, p, masked=True, symmetry="mean8")
    assert np.array_equal(gmp, wmp) and np.array_equal(gmv, wmv)
    with pytest.raises(ValueError, match="2048"):
        m.board_evaluator(4096, symmetry="mean8")


def test_recovery_recomputes_with_the_same_symmetries():
    """The existing range-overflow route (test_h3_range_guard_recomputes_in_fp32): the stem's
    BN gamma x 1e5 drives the first conv's inputs past fp16's range, the split-fp16 launch
    is posted and predict_boards recomputes it with fp32 MFMA -- under the recorded
    symmetries, so the result is bitwise the key 19 = 0 forward."""
    import _native
    lib = _native.load_library()
    m = model(3, 128, seed=8)
    B = 40
    b, p = positions(B, 15)
    syms = np.random.default_rng(4).permutation(np.arange(B) % 8).astype(np.int8)
    gamma = m.net.bn.weight.detach().clone()
    with torch.no_grad():
        m.net.bn.weight.mul_(1e5)
    m.engine.mark_dirty()
    prev_h3 = lib.azg_pv_set_tuning(TUNE.EVAL_ARITH, 0)
    try:
        want_sym = m.predict_boards(b, p, masked=True, symmetry=syms)
        want_mean = m.predict_boards(b, p, masked=True, symmetry="mean8")
        plain = m.predict_boards(b, p, masked=True)
        lib.azg_pv_set_tuning(TUNE.EVAL_ARITH, prev_h3)
        m.engine.tower_diag_clear()
        got_sym = m.predict_boards(b, p, masked=True, symmetry=syms)
        d = m.engine.tower_diag()
        assert d["h3_overflows"] == 1, d
        got_mean = m.predict_boards(b, p, masked=True, symmetry="mean8")
        d = m.engine.tower_diag()
        assert d["h3_overflows"] == 2, d
        for got, want in ((got_sym, want_sym), (got_mean, want_mean)):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert not np.array_equal(got_sym[0], plain[0])
        assert lib.azg_pv_status(m.engine.h) == 0
    finally:
        lib.azg_pv_set_tuning(TUNE.EVAL_ARITH, prev_h3)
        with torch.no_grad():
            m.net.bn.weight.copy_(gamma)
        m.engine.mark_dirty()


def test_search_with_symmetric_evaluation():
    from games.gomoku import Gomoku
    from mcts.native_mcts import NativeMCTS, NativeSelfPlay
    from network import apply_symmetry, invert_symmetry
    m = model(2, 64, seed=2)
    temp = lambda n: 1.0 if n < 3 else 0.0
    seeds = [11, 22]
    kw = dict(cpuct=1.2, dirichlet_alpha=0.3, epsilon=0.25, apply_dirichlet_n_first_moves=3)

    def games(factory):
        sp = NativeSelfPlay(None, Gomoku, 2, 16, evaluator_factory=factory, groups=1, **kw)
        return sp.play(temp, max_moves=6, use_symmetries=False, seeds=seeds)

    def same(ga, gb):
        return all(wa == wb and len(ea) == len(eb) and
                   all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]
                       for x, y in zip(ea, eb))
                   for (ea, wa), (eb, wb) in zip(ga, gb))

    first = games(m.symmetric("random", seed=3).board_evaluator)
    again = games(m.symmetric("random", seed=3).board_evaluator)
    assert same(first, again)
    plain = games(m.board_evaluator)
    assert same(games(m.symmetric(0).board_evaluator), plain)

    class HostMean8:
        """mean8 on the host from eight plain forwards in image order 0..7."""

        def predict(self, X):
            stones = (X[:, 0] + 2.0 * X[:, 1]).astype(np.int8).reshape(len(X), 225)
            ones = np.ones(len(X), np.int8)
            P, V = [], []
            for s in range(8):
                probs, v = m.predict_boards(apply_symmetry(stones, s), ones, masked=False)
                P.append(invert_symmetry(probs, s))
                V.append(v)
            return seq_mean8(P), seq_mean8(V)

    g = Gomoku(size=15)
    for mv in ((7, 7), (7, 8), (6, 8), (3, 11)):
        g.do_move(mv)
    pis = []
    for net in (m.symmetric("mean8"), HostMean8()):
        mc = NativeMCTS(Gomoku, 24, nn_model=net, cpuct=1.2, add_dirichlet_noise=False)
        pis.append(np.asarray(mc.run(g.clone(), len(g.move_history))))
    legal = g.get_valid_moves().reshape(-1) > 0
    assert abs(float(pis[0][legal].sum()) - 1.0) < 1e-6 and np.all(pis[0][~legal] == 0)
    assert np.array_equal(pis[0], pis[1])
