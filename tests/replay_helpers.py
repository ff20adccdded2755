"""Synthetic replay positions shared by the device replay buffer's tests."""


def synthetic_positions(n, seed, distinct_images=False):
    """n canonical examples (state [3,15,15], pi [225], z) from oracle.boards' generators;
    distinct_images: assert that each example's 8 dihedral images are pairwise distinct."""
    from oracle.boards import encode_batch, synth_positions, synth_targets
    boards, players = synth_positions(n, seed=seed)
    states = encode_batch(boards, players)
    pi, z = synth_targets(n, seed=seed + 1)
    out = [(states[i], pi[i], float(z[i, 0])) for i in range(n)]
    if distinct_images:   # the inputs can tell the 8 images apart, in the state AND in pi
        from mcts.new_mcts_alpha import MCTS
        for s, p, _ in out:
            imgs = MCTS.symmetries(None, s, p)
            assert len({si.tobytes() for si, _ in imgs}) == 8 and len({pi_.tobytes() for _, pi_ in imgs}) == 8
    return out
