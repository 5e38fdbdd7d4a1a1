"""The lattice-free CTC scorer (pgasr_ctc_hyp_score, csrc/hyp_score.hip) stated in numpy fp64, and the cases that
tests/test_hyp_score_cpu.py and tests/test_hyp_score_gpu.py share (TEST INFRASTRUCTURE ONLY).

``hyp_score_ref`` is the header's A12-SCORE paragraph line by line: the rows that get +inf without any work, the token check, the
utterance without frames, then the alpha recurrence as a plain loop over frames (vectorised over the pairs and their states) with
lse3's argument order.  Every case is built once per process and its arrays are read-only."""
import functools

import numpy as np

GARBAGE = 1 << 30
# the issue's lengths; the kernel picks 1, 2, 4 or 8 states per thread at 2 * len + 1 <= 256, 512, 1024, so the lengths on either side
# of every switch are 127 / 128, 255 / 256, 511 / 512 -- all of them in the list already
LENGTHS = (0, 1, 2, 31, 32, 127, 128, 255, 256, 511, 512, 1023)
VARIANT_BOUNDARIES = ((127, 128), (255, 256), (511, 512))


def lse3(a0, a1, a2):
    """log(exp(a0) + exp(a1) + exp(a2)) elementwise, -inf where all three are."""
    m = np.maximum(np.maximum(a0, a1), a2)
    dead = np.isneginf(m)
    mz = np.where(dead, 0.0, m)
    with np.errstate(divide="ignore"):
        r = m + np.log(np.exp(a0 - mz) + np.exp(a1 - mz) + np.exp(a2 - mz))
    return np.where(dead, -np.inf, r)


def hyp_score_ref(lp, tokens, lengths, count, in_len, Lh, blank):
    """lp (T,B,V) fp32, tokens (N,B,stride) / lengths (N,B) ints, count (B) or None, in_len (B) -> nll (N,B) float64."""
    T, B, V = lp.shape
    N, _, stride = tokens.shape
    out = np.full((N, B), np.inf)
    pairs = []
    for b in range(B):
        cnt = N if count is None else min(max(int(count[b]), 0), N)
        Tb = min(max(int(in_len[b]), 0), T)
        for n in range(cnt):
            L = max(int(lengths[n, b]), 0)
            if L > Lh or L > stride:
                continue
            y = tokens[n, b, :L].astype(np.int64)
            if ((y < 0) | (y >= V) | (y == blank)).any():
                continue
            if Tb == 0:
                out[n, b] = 0.0 if L == 0 else np.inf
                continue
            pairs.append((n, b, L, Tb, y))
    if not pairs:
        return out
    P = len(pairs)
    Smax = max(2 * L + 1 for _, _, L, _, _ in pairs)
    lab = np.full((P, Smax), blank, dtype=np.int64)
    skip = np.zeros((P, Smax), dtype=bool)
    S = np.array([2 * L + 1 for _, _, L, _, _ in pairs])
    Tbs = np.array([Tb for _, _, _, Tb, _ in pairs])
    bidx = np.array([b for _, b, _, _, _ in pairs])
    for p, (_, _, L, _, y) in enumerate(pairs):
        lab[p, 1:2 * L:2] = y
        if L > 1:
            skip[p, 3:2 * L:2] = y[1:] != y[:-1]
    inside = np.arange(Smax)[None, :] < S[:, None]
    lp64 = lp.astype(np.float64)
    alpha = np.full((P, Smax + 2), -np.inf)          # position s + 2: two guard cells
    emit = lp64[0, bidx[:, None], lab]
    alpha[:, 2:4] = np.where(inside[:, :2], emit[:, :2], -np.inf)
    for t in range(1, int(Tbs.max())):
        a2 = np.where(skip, alpha[:, :-2], -np.inf)
        new = lse3(alpha[:, 2:], alpha[:, 1:-1], a2) + lp64[t, bidx[:, None], lab]
        new = np.where(inside, new, -np.inf)
        alpha[:, 2:] = np.where((Tbs > t)[:, None], new, alpha[:, 2:])
    rows = np.arange(P)
    last = alpha[rows, S - 1 + 2]
    prev = np.where(S > 1, alpha[rows, S - 2 + 2], -np.inf)      # S == 1 reads the guard cell: -inf either way
    ll = lse3(last, prev, np.full(P, -np.inf))
    for p, (n, b, _, _, _) in enumerate(pairs):
        out[n, b] = -ll[p]
    return out


def frames_needed(y):
    """The least number of frames that align y: one per token and one blank between equal neighbours."""
    y = list(y)
    return len(y) + sum(1 for i in range(1, len(y)) if y[i] == y[i - 1])


def log_softmax32(z):
    z = z - z.max(axis=2, keepdims=True)
    return (z - np.log(np.exp(z).sum(axis=2, keepdims=True))).astype(np.float32)


def _draw(rng, V, blank, L, no_repeats=False):
    syms = np.array([v for v in range(V) if v != blank])
    y = rng.choice(syms, size=L)
    if no_repeats:
        for i in range(1, L):
            while y[i] == y[i - 1]:
                y[i] = rng.choice(syms)
    return [int(v) for v in y]


def _pack(rows, stride):
    """rows[n][b] token lists -> tokens (N,B,stride) with zero tails, lengths (N,B)."""
    N, B = len(rows), len(rows[0])
    tokens = np.zeros((N, B, stride), dtype=np.int32)
    lengths = np.zeros((N, B), dtype=np.int32)
    for n in range(N):
        for b in range(B):
            tokens[n, b, :len(rows[n][b])] = rows[n][b]
            lengths[n, b] = len(rows[n][b])
    return tokens, lengths


def _case(lp, rows, stride, count, in_len, Lh, blank):
    tokens, lengths = _pack(rows, stride)
    return dict(lp=lp, tokens=tokens, lengths=lengths, count=None if count is None else np.asarray(count, np.int32),
                in_len=np.asarray(in_len, np.int32), Lh=int(Lh), blank=int(blank))


def _v2_runs(rng):
    # V = 2, blank = V - 1: the one symbol, n times -- 2n - 1 frames.  Utterance 0 has exactly the 11 frames of n = 6, utterance 1 one
    # less, utterance 2 none; hyp_stride > Lh; count NULL
    rows = [[[0] * n for _ in range(3)] for n in range(16)]
    return _case(log_softmax32(rng.normal(size=(11, 3, 2))), rows, 16, None, [11, 10, 0], 15, 1)


def _t1(rng):
    # T = 1, N = 1: one token, none, two (cannot fit)
    rows = [[[1], [], [1, 1]]]
    return _case(log_softmax32(rng.normal(size=(1, 3, 2))), rows, 2, None, [1, 1, 1], 2, 0)


def _v29(rng):
    # N = 17, count below N, input_lengths below T, tokens that are the blank / V / -1 / 2^30
    V, N, B, T = 29, 17, 2, 40
    rows = [[_draw(rng, V, 0, int(rng.integers(0, 21))) for _ in range(B)] for n in range(N)]
    rows[1][0] = [3, 3, 3, 7, 7]
    rows[3][0] = [4, 0, 5]
    rows[4][0] = [4, V, 5]
    rows[5][0] = [-1]
    rows[6][0] = [2, GARBAGE]
    rows[2][1] = []
    return _case(log_softmax32(rng.normal(size=(T, B, V)) * 2.0), rows, 24, [17, 9], [40, 33], 20, 0)


def _v64(rng):
    # blank = V - 1; within the lattice's limits (N = 16, V = 64, hyp_stride >= Lh)
    V, N, B, T = 64, 16, 2, 30
    rows = [[_draw(rng, V, 63, n % 15) for _ in range(B)] for n in range(N)]
    rows[1][0] = [62]
    return _case(log_softmax32(rng.normal(size=(T, B, V)) * 2.0), rows, 14, None, [30, 25], 14, 63)


def _v29_lattice(rng):
    # longer rows for the comparison with pgasr_ctc_hyp_lattice
    V, N, B, T = 29, 16, 2, 120
    rows = [[_draw(rng, V, 0, int(rng.integers(20, 51))) for _ in range(B)] for n in range(N)]
    return _case(log_softmax32(rng.normal(size=(T, B, V)) * 2.0), rows, 50, [16, 11], [120, 97], 50, 0)


def _v65(rng):
    # the first width the lattice refuses; token V - 1 = 64; one utterance, count below N
    V, N, T = 65, 17, 20
    rows = [[_draw(rng, V, 0, n % 9)] for n in range(N)]
    rows[2][0] = [64, 64, 1]
    return _case(log_softmax32(rng.normal(size=(T, 1, V)) * 2.0), rows, 9, [5], [20], 8, 0)


def _v128(rng):
    # N = 128, blank = 70, a count of 0
    V, N, B, T = 128, 128, 2, 24
    rows = [[_draw(rng, V, 70, n % 13) for _ in range(B)] for n in range(N)]
    rows[1][0] = [127]
    return _case(log_softmax32(rng.normal(size=(T, B, V)) * 2.0), rows, 12, [128, 0], [24, 24], 12, 70)


def _v1000(rng):
    # blank = V - 1 = 999; the short half of LENGTHS twice; Lh = 200 skips the rows of 255; hyp_stride = 300 > Lh
    V, B, T = 1000, 2, 300
    lens = LENGTHS[:8] * 2
    rows = [[_draw(rng, V, 999, L) for _ in range(B)] for L in lens]
    rows[1][0] = [998]
    return _case(log_softmax32(rng.normal(size=(T, B, V)) * 2.0), rows, 300, None, [300, 290], 200, 999)


def _v1024_long(rng):
    # every states-per-thread variant under ONE launch (Lh = 1023): 1023, and both sides of 511 / 512, 255 / 256, 127 / 128
    V, T = 1024, 1030
    lens = [[1023, 255], [512, 128], [511, 127], [256, 512]]
    rows = [[_draw(rng, V, 0, L, no_repeats=True) for L in pair] for pair in lens]
    rows[0][0][5] = 1023
    return _case(log_softmax32(rng.normal(size=(T, 2, V)) * 2.0), rows, T, None, [1030, 600], 1023, 0)


def _steep(rng):
    # T = 1000, len ~ 300, V = 1024: a symbol no hypothesis of the utterance holds gets +20 at every frame, so every alignment pays
    # about 20 nats per frame and the row maxima of alpha fall by that much per frame (tests/ctc_cases.py, the "anti" cases)
    V, B, N, T = 1024, 2, 4, 1000
    rows = [[_draw(rng, V - 1, 0, int(rng.integers(290, 301))) for _ in range(B)] for n in range(N)]      # symbols 1 .. V - 2
    z = rng.normal(size=(T, B, V))
    z[:, :, V - 1] += 20.0
    return _case(log_softmax32(z), rows, T, None, [1000, 937], 300, 0)


def _zeros(rng):
    # symbols 5 and 77 have probability 0 at every frame, the blank at one frame of utterance 1: the rows that hold 5 or 77 are +inf
    V, N, B, T = 128, 8, 2, 30
    rows = [[[v for v in _draw(rng, V, 0, 3 + n) if v not in (5, 77)] for _ in range(B)] for n in range(N)]
    for n in (1, 4, 6):
        rows[n][n % 2].insert(1, 5 if n != 4 else 77)
    lp = log_softmax32(rng.normal(size=(T, B, V)) * 2.0)
    lp[:, :, 5] = -np.inf
    lp[:, :, 77] = -np.inf
    lp[9, 1, 0] = -np.inf
    return _case(lp, rows, 16, None, [30, 26], 16, 0)


BUILDERS = {"v2_runs": _v2_runs, "t1": _t1, "v29": _v29, "v64": _v64, "v29_lattice": _v29_lattice, "v65": _v65, "v128": _v128,
            "v1000": _v1000, "v1024_long": _v1024_long, "steep": _steep, "zeros": _zeros}
EDGE = ("v2_runs", "t1", "v29", "v64", "v65", "v128", "v1000", "v1024_long")
LATTICE = ("v2_runs", "v64", "v29_lattice")          # V <= 64, N <= 16, hyp_stride >= Lh
ALL = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """One case with its reference ``want`` (N,B) float64, built once; every array read-only."""
    c = BUILDERS[name](np.random.default_rng(1000 + ALL.index(name)))
    c["want"] = hyp_score_ref(c["lp"], c["tokens"], c["lengths"], c["count"], c["in_len"], c["Lh"], c["blank"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def garbage_tails(c):
    """The case's tokens with 2^30 behind every hypothesis' length."""
    tok = c["tokens"].copy()
    behind = np.arange(tok.shape[2])[None, None, :] >= np.maximum(c["lengths"], 0)[:, :, None]
    tok[behind] = GARBAGE
    return tok


def close(got, want, rel=1e-9):
    """+inf == +inf, everything else within rel of want; nothing is NaN.  Returns the largest relative deviation seen."""
    assert got.shape == want.shape and not np.isnan(got).any() and not np.isnan(want).any()
    fin = np.isfinite(want)
    assert (np.isfinite(got) == fin).all(), (np.argwhere(np.isfinite(got) != fin)[:4], got[np.isfinite(got) != fin][:4])
    assert (got[~fin] == want[~fin]).all()
    if not fin.any():
        return 0.0
    dev = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), np.finfo(np.float64).tiny)
    exact = got[fin] == want[fin]
    worst = float(dev[~exact].max()) if (~exact).any() else 0.0
    assert worst <= rel, worst
    return worst
