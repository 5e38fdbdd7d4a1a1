"""The inputs of the edit-operation alignment tests, shared by tests/test_editops_cpu.py (which proves that they are
discriminating: several optimal alignments each, counts that move under another tie order) and tests/test_editops_gpu.py (which
holds csrc/editops.hip to tests/editops_ref.py on them).  Everything is seed-fixed."""
import numpy as np

# the longer length of a pair: where the cells-per-lane tiling of the kernel changes (64 * J columns hold lengths up to 64 * J - 1)
TILING_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1024)
LONG_LENGTHS = (1025, 2049, 4095)          # one pair each way round and one with equal lengths


def _rows(rng, vocab, n, m, mutate=True):
    """A reference of n symbols and a hypothesis of m that is an edited copy of it where it can be (so the alignment has hits,
    substitutions, deletions and insertions), random where it cannot."""
    ref = rng.integers(0, vocab, n).tolist()
    if not mutate or n == 0 or m == 0:
        return ref, rng.integers(0, vocab, m).tolist()
    hyp = []
    for s in ref:
        u = rng.random()
        if u < 0.12:
            continue                                   # deletion
        hyp.append(int(rng.integers(0, vocab)) if u < 0.27 else s)
        if u > 0.9:
            hyp.append(int(rng.integers(0, vocab)))    # insertion
    while len(hyp) < m:
        hyp.insert(int(rng.integers(0, len(hyp) + 1)), int(rng.integers(0, vocab)))
    while len(hyp) > m:
        del hyp[int(rng.integers(0, len(hyp)))]
    return ref, hyp


def tie_cases():
    """(name, ref, hyp) over small alphabets, where ties are the rule: binary and 4-symbol random strings, 29-symbol edited copies,
    the transposition "ab" / "ba", and runs."""
    rng = np.random.default_rng(20240607)
    a, b = 0, 1
    cases = [("ab/ba", [a, b], [b, a]), ("ba/ab", [b, a], [a, b]), ("aaaa/aa", [a] * 4, [a] * 2), ("aa/aaaa", [a] * 2, [a] * 4),
             ("aaaaaaa/aaa", [a] * 7, [a] * 3), ("abab/baba", [a, b, a, b], [b, a, b, a]), ("aabb/abab", [a, a, b, b], [a, b, a, b]),
             ("aab/ab", [a, a, b], [a, b]), ("abc/ca", [0, 1, 2], [2, 0]),
             # a longer hypothesis (the kernel then lays the HYPOTHESIS across its lanes) where deletion before insertion and
             # insertion before deletion give different strings: the tie rule has to follow the swap
             ("abab/baaba", [a, b, a, b], [b, a, a, b, a]), ("aaba/bbbaab", [a, a, b, a], [b, b, b, a, a, b]),
             ("aabab/abaaba", [a, a, b, a, b], [a, b, a, a, b, a])]
    for vocab, n, m in ((2, 9, 7), (2, 7, 9), (2, 33, 33), (2, 64, 50), (2, 50, 64), (2, 130, 120),
                        (4, 30, 24), (4, 24, 30), (4, 64, 64), (4, 60, 70), (4, 70, 60), (4, 128, 120), (4, 120, 128), (4, 200, 260),
                        (29, 64, 60), (29, 60, 64), (29, 128, 120), (29, 120, 128), (29, 64, 64)):
        ref, hyp = _rows(rng, vocab, n, m, mutate=vocab == 29)
        cases.append(("v%d_%dx%d" % (vocab, n, m), ref, hyp))
    return cases


def length_pairs(longer):
    """The (n, m) pairs tested at a longer length: both ways round and equal, against a shorter side that is empty, tiny and close."""
    if longer == 0:
        return [(0, 0)]
    shorter = sorted({0, 1, max(longer // 2, 1), longer - 1} - {longer})
    return [(longer, s) for s in shorter] + [(s, longer) for s in shorter] + [(longer, longer)]


def length_cases(lengths=TILING_LENGTHS, vocab=4, seed=77):
    """(n, m, ref, hyp) for every pair of ``length_pairs`` at every length, 4 symbols (tie heavy)."""
    rng = np.random.default_rng(seed)
    out = []
    for longer in lengths:
        for n, m in length_pairs(longer):
            ref, hyp = _rows(rng, vocab, n, m, mutate=min(n, m) > 1)
            out.append((n, m, ref, hyp))
    return out


def long_cases(seed=78):
    """One pair each way round and one with equal lengths at every long length; the shorter side is 60 long, so that the serial
    chain stays short, and at equal lengths both sides are full."""
    rng = np.random.default_rng(seed)
    out = []
    for longer in LONG_LENGTHS:
        for n, m in ((longer, 60), (60, longer), (longer, longer)):
            ref, hyp = _rows(rng, 4, n, m)
            out.append((n, m, ref, hyp))
    return out


def pack(cases, extra_ref=3, extra_hyp=5, seed=5):
    """Rows of (ref, hyp) lists as padded numpy matrices whose strides exceed the lengths; the padding is filled with symbols
    that occur in the rows (so a kernel that reads past a length changes its result)."""
    rng = np.random.default_rng(seed)
    R = max(len(c[0]) for c in cases) + extra_ref
    Hy = max(len(c[1]) for c in cases) + extra_hyp
    pool = sorted({s for c in cases for s in list(c[0]) + list(c[1])}) or [0]
    ref = rng.choice(pool, size=(len(cases), R)).astype(np.int32)
    hyp = rng.choice(pool, size=(len(cases), Hy)).astype(np.int32)
    rl = np.zeros(len(cases), dtype=np.int32); hl = np.zeros(len(cases), dtype=np.int32)
    for k, (r, h) in enumerate(cases):
        ref[k, :len(r)] = r; hyp[k, :len(h)] = h
        rl[k], hl[k] = len(r), len(h)
    return ref, rl, hyp, hl
