"""tests/discrete_ref.py against the project's oracles: ed_prefix against oracle.decode_ref.edit_dist (the full distance and
three prefixes each), step_coefs against oracle.pg_ref.pg_objective(..., per_step=True).coef.  No GPU."""
import numpy as np
import pytest

import discrete_ref as D
from oracle import decode_ref, pg_ref


def _pin(ref, hyp):
    ref, hyp = [int(t) for t in ref], [int(t) for t in hyp]
    got = D.ed_prefix(ref, hyp)
    m = len(hyp)
    assert got.shape == (m + 1,) and got[0] == len(ref)
    assert got[m] == decode_ref.edit_dist(ref, hyp)[0] == D.ed(ref, hyp)
    for i in sorted({1, m // 2, max(m - 1, 0)}):
        if i <= m:
            assert got[i] == decode_ref.edit_dist(ref, hyp[:i])[0], (i, ref, hyp)
    return int(got[m])


def test_ed_prefix_random_pairs():
    rng = np.random.default_rng(11)
    for k in range(30):
        alpha = 2 + k % 3
        n, m = (int(v) for v in rng.integers(0, 201, size=2))
        if k == 0:
            n = 0
        if k == 1:
            m = 0
        if k == 2:
            n = m = 0
        _pin(rng.integers(1, alpha + 1, size=n), rng.integers(1, alpha + 1, size=m))


@pytest.mark.parametrize("R,Hy", [(40, 12), (12, 40), (33, 33)])
def test_ed_prefix_planted_pairs(R, Hy):
    for name, ref, hyp, want in D.planted_pairs(R, Hy, np.random.default_rng(R)):
        assert len(ref) <= R and len(hyp) <= Hy
        assert _pin(ref, hyp) == want, name


@pytest.mark.parametrize("seed", [0, 1])
def test_step_coefs_against_pg_objective(seed):
    rng = np.random.default_rng(seed)
    T, B, V, L = 40 + 31 * seed, 4, 5, 7
    logits = rng.normal(size=(T, B, V))
    # long runs and blanks, so that characters start at a fraction of the frames
    paths = np.repeat(rng.integers(0, V, size=(2, (T + 2) // 3, B)), 3, axis=1)[:, :T]
    targets = rng.integers(1, V, size=(B, L))
    in_len = np.array([T, T - 9, 1, T // 2])
    tg_len = np.array([L, 3, 0, 5])
    lam, blank = 0.7, 0
    o = pg_ref.pg_objective(logits, in_len, targets, tg_len, lam=lam, per_step=True, paths=paths[1], greedy_frames=paths[0])
    tok_len = np.zeros(2 * B, np.int64)
    prefix = np.full((2 * B, T + 1), 10 ** 6, np.int64)
    for w in range(2):
        for b in range(B):
            hyp = decode_ref.collapse_path(paths[w, :in_len[b], b], blank)
            tok_len[w * B + b] = len(hyp)
            prefix[w * B + b, :len(hyp) + 1] = D.ed_prefix(targets[b, :tg_len[b]], hyp)
    got = D.step_coefs(paths, in_len, prefix, tok_len, tg_len, lam, 1.0 / B, blank)
    assert np.abs(o.coef).sum() > 0
    np.testing.assert_allclose(got, o.coef, rtol=1e-12, atol=1e-15)
    for b in range(B):
        assert (got[in_len[b]:, b] == 0).all()
    # a tighter table and an over-reported length are clamped, and then change nothing
    P = int(tok_len.max()) + 1
    np.testing.assert_array_equal(D.step_coefs(paths, in_len + 5 * (in_len == T), prefix[:, :P], tok_len, tg_len, lam, 1.0 / B), got)
    cut = prefix[:, :P - 2]
    np.testing.assert_array_equal(D.step_coefs(paths, in_len, cut, np.maximum(tok_len, P - 3) + 3, tg_len, lam, 1.0 / B),
                                  D.step_coefs(paths, in_len, cut, np.full(2 * B, P - 3), tg_len, lam, 1.0 / B))
