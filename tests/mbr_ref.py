"""Helper of the minimum-Bayes-risk tests (not collected): the textbook Levenshtein DP for the distances inside an N-best list --
scalar, and the same recurrence row by row over a batch of pairs in numpy; never the bit-vector form of csrc/mbr.hip --, the
selection of include/pgasr_hip.h (A7-MBR) written as its formulas state it, and the generated cases the CPU and GPU files share."""
import functools

import numpy as np

LMAX = 1024                      # pgasr_nbest_pair_dist's longest hypothesis
EDGE_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024)


def lev(a, b, V=None):
    """Levenshtein distance (sub = ins = del = 1) of two symbol sequences, the plain DP.  With V, a symbol outside [0, V) matches
    nothing, not even itself."""
    prev = list(range(len(a) + 1))
    for i, c in enumerate(b, 1):
        cur = [i] + [0] * len(a)
        for j in range(1, len(a) + 1):
            same = a[j - 1] == c and (V is None or 0 <= c < V)
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if same else 1))
        prev = cur
    return prev[len(a)]


def _lev_rows(A, la, Bm, lb, V):
    """The same recurrence for P pairs at once: A (P,LA) with lengths la, Bm (P,LB) with lengths lb.  Row i of the DP table of every
    pair is formed from row i-1; the dependency on the left neighbour, cur[j] = min(cur[j], cur[j-1] + 1), is a running minimum of
    cur[j] - j."""
    P, LA = A.shape
    ok_a = (A >= 0) & (A < V)
    ramp = np.arange(LA + 1, dtype=np.int32)
    prev = np.broadcast_to(ramp, (P, LA + 1)).copy()
    for i in range(int(lb.max(initial=0))):
        c = Bm[:, i:i + 1]
        cost = np.where((A == c) & ok_a, 0, 1).astype(np.int32)
        cur = np.empty_like(prev)
        cur[:, 0] = i + 1
        cur[:, 1:] = np.minimum(prev[:, 1:] + 1, prev[:, :-1] + cost)
        cur = np.minimum.accumulate(cur - ramp, axis=1) + ramp
        live = (i < lb)[:, None]
        prev = np.where(live, cur, prev)
    return prev[np.arange(P), la]


def pair_dist_ref(tokens, lengths, count, V, Lmax):
    """pgasr_nbest_pair_dist in numpy: tokens (N,B,S), lengths (N,B), count (B) -> dist (B,N,N) int32.  Pairs are taken in buckets of
    similar length so that a few long rows do not pad the whole list."""
    tokens, lengths, count = np.asarray(tokens), np.asarray(lengths), np.asarray(count)
    N, B, S = tokens.shape
    ln = np.clip(lengths, 0, S)
    cnt = np.clip(count, 0, N)
    valid = (np.arange(N)[:, None] < cnt[None, :]) & (ln <= Lmax)
    dist = np.full((B, N, N), -1, dtype=np.int32)
    pb, pn, pm = [], [], []
    for b in range(B):
        for n in range(N):
            if not valid[n, b]:
                continue
            dist[b, n, n] = 0
            for m in range(n + 1, N):
                if valid[m, b]:
                    pb.append(b); pn.append(n); pm.append(m)
    if not pb:
        return dist
    pb, pn, pm = np.array(pb), np.array(pn), np.array(pm)
    la, lb = ln[pn, pb], ln[pm, pb]
    longest = np.maximum(la, lb)
    lo = -1
    for hi in (66, 130, 600, S):
        sel = (longest > lo) & (longest <= hi)
        lo = hi
        if not sel.any():
            continue
        W = max(int(longest[sel].max()), 1)
        d = _lev_rows(tokens[pn[sel], pb[sel], :W], la[sel], tokens[pm[sel], pb[sel], :W], lb[sel], V)
        dist[pb[sel], pn[sel], pm[sel]] = d
        dist[pb[sel], pm[sel], pn[sel]] = d
    return dist


def split_words(row, delimiter):
    """str.split(" ") on a token row: n delimiters give n + 1 words, empty ones included; an empty row is one empty word."""
    words, cur = [], []
    for t in row:
        if t == delimiter:
            words.append(tuple(cur)); cur = []
        else:
            cur.append(int(t))
    words.append(tuple(cur))
    return words


def word_pair_dist_ref(tokens, lengths, count, delimiter, Lmax):
    """The word-level matrix: the same layout and -1 convention, the distance over the word lists of split_words."""
    tokens, lengths, count = np.asarray(tokens), np.asarray(lengths), np.asarray(count)
    N, B, S = tokens.shape
    dist = np.full((B, N, N), -1, dtype=np.int32)
    for b in range(B):
        cnt = min(max(int(count[b]), 0), N)
        rows = {}
        for n in range(cnt):
            L = min(max(int(lengths[n, b]), 0), S)
            if L <= Lmax:
                rows[n] = split_words(list(tokens[n, b, :L]), delimiter)
        for n in rows:
            for m in rows:
                if n <= m:
                    dist[b, n, m] = dist[b, m, n] = lev(rows[n], rows[m])
    return dist


def select_ref(dist, score, count, scale):
    """pgasr_mbr_select as the header states it: dist (B,N,N), score (N,B) float64, count (B) -> (best (B), risk (N,B), posterior (N,B)).
    Every product and sum is one numpy float64 operation, the sums in index order."""
    dist, score, count = np.asarray(dist), np.asarray(score, dtype=np.float64), np.asarray(count)
    B, N, _ = dist.shape
    best = np.zeros(B, dtype=np.int32)
    risk = np.full((N, B), np.inf)
    post = np.zeros((N, B))
    scale = np.float64(scale)
    for b in range(B):
        cnt = min(max(int(count[b]), 0), N)
        valid = [n < cnt and bool(np.isfinite(score[n, b])) and dist[b, n, n] >= 0 for n in range(N)]
        if not any(valid):
            continue
        m = min(score[n, b] for n in range(N) if valid[n])
        w = np.zeros(N)
        z = np.float64(0.0)
        for n in range(N):
            if valid[n]:
                w[n] = np.exp(-(scale * (score[n, b] - m)))
                z = z + w[n]
        for n in range(N):
            if valid[n]:
                post[n, b] = w[n] / z
        for n in range(N):
            if not valid[n]:
                continue
            acc = np.float64(0.0)
            for j in range(N):
                if valid[j]:
                    acc = acc + post[j, b] * np.float64(dist[b, n, j])
            risk[n, b] = acc
        least, arg = None, 0
        for n in range(N):
            if valid[n] and (least is None or risk[n, b] < least):
                least, arg = risk[n, b], n
        best[b] = arg
    return best, risk, post


def best_within_margin(best, ref_risk):
    """The margin rule of the selection tests, on every utterance: ref_risk[best] <= min(ref_risk) + 1e-12 * max(1, min)."""
    ok = []
    for b in range(ref_risk.shape[1]):
        col = ref_risk[:, b]
        if not np.isfinite(col).any():
            ok.append(int(best[b]) == 0)
            continue
        least = col[np.isfinite(col)].min()
        ok.append(bool(col[int(best[b])] <= least + 1e-12 * max(1.0, least)))
    return ok


# ------------------------------------------------------------------------------------------
# generated lists
# ------------------------------------------------------------------------------------------
def _edited(rng, base, V, edits):
    t = list(base)
    for _ in range(edits):
        k = int(rng.integers(0, len(t) + 1)); r = rng.random()
        if r < 0.33 and t:
            t.pop(min(k, len(t) - 1))
        elif r < 0.66:
            t.insert(k, int(rng.integers(0, V)))
        elif t:
            t[min(k, len(t) - 1)] = int(rng.integers(0, V))
    return t


def _pack(rows_per_utt, count, V, rng, slack=7):
    """rows_per_utt[b][n] = token list -> (tokens (N,B,S) int32 with random garbage behind every length, lengths (N,B), count (B))."""
    B, N = len(rows_per_utt), len(rows_per_utt[0])
    S = max(max(len(r) for rows in rows_per_utt for r in rows), 1) + slack
    tokens = rng.integers(1, max(V, 2), size=(N, B, S)).astype(np.int32)        # garbage: never zero, valid-looking symbols
    lengths = np.zeros((N, B), dtype=np.int32)
    for b, rows in enumerate(rows_per_utt):
        for n, r in enumerate(rows):
            tokens[n, b, :len(r)] = r
            lengths[n, b] = len(r)
    return tokens, lengths, np.asarray(count, dtype=np.int32)


# (name, N, B, V, kind, lengths to draw from, counts (N: the list size, -1: N - 1), Lmax)
# Lists of 64 and more hypotheses keep to the short lengths but for two long rows in their first utterance (LONG_ROWS): the oracle
# is a DP, quadratic in the length.
LONG_ROWS = {"n64-mixed": (512, 1024), "n65-mixed": (511, 513), "n128-mixed": (1023, 129)}
PAIR_CASES = [
    ("n1", 1, 3, 29, "unrelated", (0, 65, 1024), (0, 1, 1), LMAX),
    ("n2", 2, 3, 2, "unrelated", (511, 512, 513, 1, 2, 63), (2, 1, 0), LMAX),
    ("n3", 3, 3, 64, "unrelated", (1023, 1024, 513, 64, 0, 129), (3, 2, 1), LMAX),
    ("n16-edges", 16, 1, 29, "unrelated", EDGE_LENGTHS, (16,), LMAX),
    ("n3-near-1018", 3, 3, 64, "near", (1018,), (3, 3, 2), LMAX),
    ("n16-near-511", 16, 1, 64, "near", (511,), (15,), LMAX),
    ("n17-v2", 17, 3, 2, "unrelated", (0, 1, 2, 63, 64, 65, 127, 128, 129), (17, 16, 0), LMAX),
    ("n17-near-129", 17, 1, 29, "near", (129,), (17,), LMAX),
    ("n64-near-127", 64, 1, 29, "near", (127,), (64,), LMAX),
    ("n64-mixed", 64, 3, 64, "unrelated+long", (0, 1, 2, 63, 64, 65), (64, 63, 1), LMAX),
    ("n65-mixed", 65, 1, 2, "unrelated+long", (0, 1, 2, 63, 64, 65, 127, 128, 129), (65,), LMAX),
    ("n128-near-63", 128, 1, 29, "near", (63,), (128,), LMAX),
    ("n128-mixed", 128, 3, 29, "unrelated+long", (0, 1, 2, 63, 64, 65), (128, 127, 0), LMAX),
    ("over-lmax", 8, 3, 29, "over", (5, 64, 3, 70, 64, 65, 1, 0), (8, 8, 7), 64),
    ("symbol-ge-v", 4, 1, 29, "bad-symbol", (9,), (4,), LMAX),
]


@functools.lru_cache(maxsize=None)
def pair_case(name):
    """(tokens, lengths, count, V, Lmax, expected dist) of one case, computed once per process and never written to."""
    _, N, B, V, kind, lens, counts, Lmax = next(c for c in PAIR_CASES if c[0] == name)
    rng = np.random.default_rng(sum(ord(ch) for ch in name) * 7919 + N)
    utts = []
    for b in range(B):
        if kind == "near":
            base = [int(x) for x in rng.integers(0, V, size=lens[0])]
            rows = [_edited(rng, base, V, int(rng.integers(0, 7))) for _ in range(N)]
        elif kind == "bad-symbol":
            base = [int(x) for x in rng.integers(0, V, size=lens[0])]
            rows = [list(base) for _ in range(N)]
            rows[1][4] = V; rows[2][4] = V; rows[3][2] = -3; rows[3][7] = 100      # rows 1 and 2 are equal and still one apart
        elif kind == "over":
            rows = [[int(x) for x in rng.integers(0, V, size=lens[n])] for n in range(N)]
        else:
            pick = [lens[(n + 3 * b) % len(lens)] for n in range(N)] if N >= len(lens) else [lens[(2 * b + n) % len(lens)] for n in range(N)]
            if kind == "unrelated+long" and b == 0:
                pick[5], pick[N - 2] = LONG_ROWS[name]
            rows = [[int(x) for x in rng.integers(0, V, size=L)] for L in pick]
        utts.append(rows)
    tokens, lengths, count = _pack(utts, counts, V, rng)
    for a in (tokens, lengths, count):
        a.setflags(write=False)
    want = pair_dist_ref(tokens, lengths, count, V, Lmax)
    want.setflags(write=False)
    return tokens, lengths, count, V, Lmax, want


def word_case():
    """A list over the alphabet {0: blank, 1..4: letters, 5: the delimiter}: the delimiter at the start, at the end and doubled, an
    empty row, rows that differ in one word only.  (tokens, lengths, count, delimiter)."""
    rng = np.random.default_rng(11)
    d = 5
    rows0 = [[1, 2, d, 3, 4, d, 1], [d, 1, 2, d, 3, 4, d, 1], [1, 2, d, 3, 4, d, 1, d], [1, 2, d, d, 3, 4, d, 1], [], [d], [d, d],
             [1, 2, d, 3, 3, d, 1], [1, 2, 3, 4, 1], [2, d, 3, 4, d, 1, d, 4]]
    rows1 = [[int(x) for x in rng.integers(1, 6, size=L)] for L in (30, 31, 0, 12, 64, 65, 7, 1, 2, 40)]
    tokens, lengths, count = _pack([rows0, rows1], [10, 9], 6, rng)
    return tokens, lengths, count, d


# ------------------------------------------------------------------------------------------
# generated selection cases
# ------------------------------------------------------------------------------------------
def _near_list_dist(rng, N, V, L, outlier_edits):
    """Distances of a list whose row 0 lies `outlier_edits` edits off a base string the other rows stay close to."""
    base = [int(x) for x in rng.integers(0, V, size=L)]
    rows = [_edited(rng, base, V, outlier_edits)] + [_edited(rng, base, V, int(rng.integers(0, 2))) for _ in range(N - 1)]
    return np.array([[lev(a, b) for b in rows] for a in rows], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def select_general():
    """B = 8 lists of 16: the best-scored row 0 is an outlier of its list, the others cluster; scale 1.  (dist, score, count, scale)."""
    rng = np.random.default_rng(5)
    B, N = 8, 16
    dist = np.stack([_near_list_dist(rng, N, 8, 20, 5) for _ in range(B)])
    score = 30.0 + np.sort(rng.random((N, B)) * 2.0, axis=0)          # ascending: row 0 is the MAP row
    count = np.array([16, 16, 15, 16, 9, 16, 2, 16], dtype=np.int32)
    return dist, score, count, 1.0


@functools.lru_cache(maxsize=None)
def select_large():
    """N = 128, B = 3, a caller-made symmetric matrix, scale 0.7."""
    rng = np.random.default_rng(6)
    B, N = 3, 128
    a = rng.integers(0, 40, size=(B, N, N))
    dist = (np.triu(a, 1) + np.transpose(np.triu(a, 1), (0, 2, 1))).astype(np.int32)
    score = 100.0 + rng.random((N, B)) * 6.0
    return dist, score, np.array([128, 127, 50], dtype=np.int32), 0.7


@functools.lru_cache(maxsize=None)
def select_exact():
    """scale = 0 and count in {1, 2, 4, 8, 16}: the posterior 1/count and every partial sum of the risk are exact in fp64, so the
    device must give the helper's bits.  Utterances 5..9 repeat the counts with a tie built in: two rows with the same distances to
    every row (one string twice) at the least risk, the first of them at index count / 2 (0 for count 2) and the second last."""
    rng = np.random.default_rng(7)
    N, counts = 16, (1, 2, 4, 8, 16)
    dists, cnts = [], []
    for c in counts:
        dists.append(_near_list_dist(rng, N, 8, 24, 3)); cnts.append(c)
    for c in counts[1:]:
        base = [int(x) for x in rng.integers(0, 8, size=24)]
        rows = [_edited(rng, base, 8, 4) for _ in range(N)]
        i = c // 2 if c > 2 else 0                                    # count 2: rows 0 and 1 tie, both at distance 0 + d
        j = c - 1
        rows[i] = list(base); rows[j] = list(base)
        dists.append(np.array([[lev(a, b) for b in rows] for a in rows], dtype=np.int32)); cnts.append(c)
    dist = np.stack(dists)
    score = 10.0 + rng.random((N, len(cnts))) * 3.0
    return dist, score, np.array(cnts, dtype=np.int32), 0.0


@functools.lru_cache(maxsize=None)
def select_other():
    """Non-finite scores, a hypothesis over the cap (its diagonal is -1), count = 0, no valid row at all.  scale 2.5."""
    rng = np.random.default_rng(8)
    B, N = 5, 8
    dist = np.stack([_near_list_dist(rng, N, 8, 16, 2) for _ in range(B)])
    score = 5.0 + rng.random((N, B)) * 4.0
    score[0, 0] = np.inf; score[3, 0] = np.nan; score[2, 0] = -np.inf
    dist[1, 0, :] = -1; dist[1, :, 0] = -1                            # utterance 1: row 0 is over the cap
    score[:, 3] = np.inf                                               # utterance 3: nothing valid
    count = np.array([8, 8, 0, 8, 5], dtype=np.int32)
    return dist, score, count, 2.5
