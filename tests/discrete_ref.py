"""Oracles for the discrete kernels (edit distance with per-prefix distances, per-frame REINFORCE coefficients) as numpy
statements that stay fast at the kernels' size limits.  tests/test_discrete_ref_cpu.py pins both to the project's own oracles
(oracle.decode_ref.edit_dist, oracle.pg_ref.pg_objective); tests/test_discrete_kernels_gpu.py holds the kernels to them."""
import numpy as np


def ed_prefix(ref, hyp):
    """Levenshtein distance (sub = ins = del = 1) of ``ref`` to every prefix of ``hyp``: out[i] = ED(ref, hyp[:i]), i = 0..len(hyp).
    Row by row over the hypothesis; one row over the reference positions j = 0..n is
        x[j]   = min(row[j] + 1, row[j-1] + (ref[j-1] != h)),  x[0] = i          (up, diagonal)
        new[j] = min_{k <= j} (x[k] + j - k) = minimum.accumulate(x - j) + j      (the chain of left moves)"""
    ref = np.asarray(ref, dtype=np.int64).reshape(-1)
    hyp = np.asarray(hyp, dtype=np.int64).reshape(-1)
    n = len(ref)
    j = np.arange(n + 1, dtype=np.int64)
    row = j.copy()
    out = np.empty(len(hyp) + 1, dtype=np.int64)
    out[0] = n
    x = np.empty(n + 1, dtype=np.int64)
    for i, h in enumerate(hyp, 1):
        x[0] = i
        np.minimum(row[1:] + 1, row[:-1] + (ref != h), out=x[1:])
        row = np.minimum.accumulate(x - j) + j
        out[i] = row[n]
    return out


def ed(ref, hyp):
    return int(ed_prefix(ref, hyp)[-1])


def planted_pairs(R, Hy, rng):
    """Pairs with a known distance that fill strides R (reference) and Hy (hypothesis), both >= 6: [(name, ref, hyp, distance)].
    first_token: the hypothesis is the reference's first token, which no other reference token equals -> n - 1, and every
                 cell right of the first takes its value from the chain of left moves;
    mirror:      the same with the roles exchanged -> m - 1;
    disjoint:    one symbol against another -> max(n, m);
    deletions:   the shorter side is the longer one (neighbours all different) with k tokens deleted -> k;
    insertions:  the hypothesis is the reference (at most 50 tokens) with 10 foreign tokens inserted, the first and the last
                 among them (Hy >= 11) -> 10, and only by an insertion move in the very column of each foreign token."""
    first_r = np.concatenate([[5], rng.integers(1, 5, size=R - 1)])
    first_h = np.concatenate([[5], rng.integers(1, 5, size=Hy - 1)])
    long_n, short_cap = max(R, Hy), min(R, Hy)
    k = max(5, long_n - short_cap)
    long_seq = np.arange(long_n) % 4 + 1
    short_seq = np.delete(long_seq, rng.choice(long_n, size=k, replace=False))
    dele = (long_seq, short_seq) if R >= Hy else (short_seq, long_seq)
    nx = min(R, Hy - 10, 50)
    x = rng.integers(1, 5, size=nx)
    ins = np.insert(x, np.sort(np.concatenate([[0, nx], rng.integers(0, nx + 1, size=8)])), 9)
    return [("insertions", x, ins, 10),
            ("first_token", first_r, np.array([5]), R - 1),
            ("mirror", np.array([5]), first_h, Hy - 1),
            ("disjoint", np.full(R, 1), np.full(Hy, 2), max(R, Hy)),
            ("deletions", dele[0], dele[1], k)]


def char_starts(path, blank=0):
    """bool (T): frame t starts a character of the collapsed path (non-blank and different from frame t - 1)"""
    p = np.asarray(path, dtype=np.int64).reshape(-1)
    if len(p) == 0:
        return np.zeros(0, bool)
    return (p != blank) & np.concatenate([[True], p[1:] != p[:-1]])


def step_coefs(paths, in_len, prefix, tok_len, tg_len, lam, inv_bg, blank=0):
    """The statement above pg_step_coef_kernel in fp64.  paths (2,T,B) greedy then sampled frame labels, prefix (2B,P) the
    per-prefix distances of their collapsed forms, tok_len (2B) the collapsed lengths, tg_len (B) the targets' lengths:
        c_w(t)    = characters of path w started in frames < t, at most n_w = clamp(tok_len_w, 0, P - 1)
        G_w(t)    = prefix_w[c_w(t)] - prefix_w[n_w]
        coef[t,b] = lam * inv_bg * (G_1(t) - G_0(t)) / max(tg_len_b, 1)   for t < T_b = clamp(in_len_b, 0, T), 0 beyond."""
    paths = np.asarray(paths, dtype=np.int64)
    prefix = np.asarray(prefix, dtype=np.int64)
    two, T, B = paths.shape
    assert two == 2 and prefix.shape[0] == 2 * B
    P = prefix.shape[1]
    coef = np.zeros((T, B), dtype=np.float64)
    for b in range(B):
        Tb = min(max(int(in_len[b]), 0), T)
        G = []
        for w in range(2):
            n = min(max(int(tok_len[w * B + b]), 0), P - 1)
            st = char_starts(paths[w, :Tb, b], blank)
            c = np.minimum(np.cumsum(st) - st, n)              # exclusive count
            G.append((prefix[w * B + b, c] - prefix[w * B + b, n]).astype(np.float64))
        coef[:Tb, b] = float(lam) * float(inv_bg) * (G[1] - G[0]) / max(int(tg_len[b]), 1)
    return coef
