"""Helper of the tie-order tests (not collected): inputs on which the prefix beam search meets EXACT ties that every correct
implementation sees as exact, the search of tests/nbest_ref.py with a report of those ties, and the shared list of cases.

The construction is a symmetry.  Two symbols a, b whose log-prob columns are bit-identical in every frame ("twins") make any two
prefixes related by swapping a and b go through the same operations on the same values, so their totals are bit-equal in the fp64
oracle, the fp64 kernel and both fp32 kernels alike; which of the two survives a cut and which is listed first is decided by the
reference's rule alone (score descending, first touch among equals).  An LM table invariant under the swap keeps that true with
fusion.  Twins come in PAIRS only: with three identical columns mathematically equal prefixes appear that are not related by one
global swap, whose fp64 scores differ by ~1e-13 and which no implementation is bound to order alike.  Blank is never a twin and no
probability is zero (an entry's stay candidate and its own repeat extension then never tie: include/pgasr_hip.h, A7-NBEST)."""
import functools

import numpy as np

import beam_lm_ref as R
import nbest_ref as NR

TIE_B = 5


def lengths_of(T):
    return np.array([min(n, T) for n in (T, T - T // 3, 33, 1, 0)], dtype=np.int32)


def parse(case):
    """(T, V, blank, pairs, beam, order, alpha, beta, seed) of a case with or without the three LM fields (order 0: no LM)."""
    if len(case) == 6:
        T, V, blank, pairs, beam, seed = case
        return T, V, blank, pairs, beam, 0, 0.0, 0.0, seed
    return case


def check_pairs(V, blank, pairs):
    flat = [s for p in pairs for s in p]
    assert all(len(p) == 2 for p in pairs) and len(set(flat)) == len(flat), "twins are disjoint pairs"
    assert blank not in flat and all(0 <= s < V for s in flat)


def swap_symbols(V, pair):
    perm = np.arange(V)
    perm[list(pair)] = pair[::-1]
    return perm


def symmetric_table(V, order, blank, pairs, seed):
    """beam_lm_ref.random_table with, on every axis and for every pair (a, b), the slice at a copied onto the slice at b: invariant
    under the swap of a pair applied to all indices (asserted).  Rows are no longer normalised, which the search never asks for."""
    check_pairs(V, blank, pairs)
    table = R.random_table(V, order, blank, seed)
    for axis in range(order):
        for a, b in pairs:
            idx = [slice(None)] * order
            idx[axis] = b
            table[tuple(idx)] = np.take(table, a, axis=axis)
    assert_table_symmetric(table, pairs)
    return table


def assert_table_symmetric(table, pairs):
    for pair in pairs:
        perm = swap_symbols(table.shape[0], pair)
        assert np.array_equal(table[np.ix_(*([perm] * table.ndim))].view(np.uint32), table.view(np.uint32)), pair


def assert_twin_columns(lp, pairs):
    assert lp.dtype == np.float32 and np.isfinite(lp).all()                     # no zero probabilities
    for a, b in pairs:
        assert np.array_equal(lp[..., a].view(np.uint32), lp[..., b].view(np.uint32)), (a, b)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(log-probs (T,B,V) fp32, lengths (B) int32, table fp32 or None) of one case: the recipe of beam_lm_ref.fast_case_inputs (per-frame
    scale from {0.3, 2.0, 5.0}, +1.5 on blank, fp64 log-softmax rounded to fp32), every utterance its own draw, with column a of the
    logits copied onto column b for every twin pair before the log-softmax.  Callers must not write into the arrays."""
    T, V, blank, pairs, beam, order, alpha, beta, seed = parse(case)
    check_pairs(V, blank, pairs)
    rng = np.random.default_rng(1000003 * seed + 1009 * T + 31 * V + 7 * blank + beam)
    logits = rng.normal(size=(T, TIE_B, V)) * rng.choice([0.3, 2.0, 5.0], size=(T, TIE_B, 1))
    logits[:, :, blank] += 1.5
    for a, b in pairs:
        logits[:, :, b] = logits[:, :, a]
    lp = R.log_softmax32(logits)
    assert_twin_columns(lp, pairs)
    table = symmetric_table(V, order, blank, pairs, seed + 17) if order else None
    for arr in (lp, table):
        if arr is not None:
            arr.setflags(write=False)
    return lp, lengths_of(T), table


def list_size(beam):
    return NR.list_size(beam)


def tie_search(logp, table=None, order=0, alpha=0.0, beta=0.0, beam_size=100, blank=0, nbest=1):
    """nbest_ref.nbest_prefix_beam_search (first touch: the reference's rule, that function's own code path) plus a report.
    Returns (hyps, report): hyps = [(prefix tuple, score)] as that function gives them; report = its ``report`` dict -- "margin",
    "tied", "cut_ties", "frames" -- with "gap" = that function's gap, "last_touch" = the list the same search gives with ties
    resolved last touch first, and "diverge" = the first frame after which the two searches keep different beams (None if none)."""
    kw = dict(logp=logp, table=table, order=order, alpha=alpha, beta=beta, beam_size=beam_size, blank=blank, nbest=nbest)
    report, other = {}, {}
    hyps, gap = NR.nbest_prefix_beam_search(report=report, **kw)
    report["gap"] = gap
    report["last_touch"] = NR.nbest_prefix_beam_search(last_touch=True, report=other, **kw)[0]
    report["diverge"] = next((t for t, (x, y) in enumerate(zip(report["frames"], other["frames"])) if x != y), None)
    return hyps, report


@functools.lru_cache(maxsize=None)
def reference(case):
    """tie_search of every utterance of one case at N = list_size(beam), computed once per process: a tuple over the TIE_B utterances
    of (hyps, report); an utterance without frames has the one empty hypothesis with score -0.0 and a report without decisions."""
    T, V, blank, pairs, beam, order, alpha, beta, seed = parse(case)
    lp, lens, table = case_inputs(case)
    out = []
    for b in range(TIE_B):
        n = int(lens[b])
        if n == 0:
            empty = [((), -0.0)]
            out.append((empty, dict(margin=float("inf"), tied=0, cut_ties=0, frames=[], gap=float("inf"), last_touch=empty, diverge=None)))
        else:
            out.append(tie_search(lp[:n, b].astype(np.float64), table, order, alpha, beta, beam, blank, list_size(beam)))
    return tuple(out)


def case_id(case):
    T, V, blank, pairs, beam, order, alpha, beta, seed = parse(case)
    return "T%d-V%d-b%d-K%d-n%d-s%d" % (T, V, blank, beam, order, seed)


P_A = ((1, 2), (5, 20))
ALPHA, BETA = 0.7, 0.5
# (T, V, blank, pairs, beam[, order, alpha, beta], seed).  Seeds: per case the first of 0, 1, 2, .. for which every condition of
# tests/test_beam_ties_cpu.py holds (NOTES.md has the scan).
GROUPS = {
    # SPL = 8 in the single-wave kernel: one pair within one lane's symbols, one across lanes; three 32-frame chunks
    "A": [(70, 29, 0, P_A, 1, 0), (70, 29, 0, P_A, 2, 2), (70, 29, 0, P_A, 5, 0), (70, 29, 0, P_A, 16, 2)],
    # blank in the middle: an entry's own / extension touch comes before its blank touch for the symbols below blank
    "B": [(70, 29, 3, P_A, 2, 1), (70, 29, 3, P_A, 5, 0), (70, 29, 3, P_A, 16, 9)],
    # blank last: every extension is touched before every stay
    "C": [(70, 29, 28, P_A, 5, 0), (70, 29, 28, P_A, 16, 1)],
    # SPL = 16
    "D": [(70, 40, 0, ((1, 2), (5, 33)), 2, 2), (70, 40, 0, ((1, 2), (5, 33)), 16, 6)],
    # V at the limit, symbol 0 a twin, blank = 63
    "E": [(70, 64, 63, ((0, 40), (5, 62)), 5, 8), (70, 64, 63, ((0, 40), (5, 62)), 16, 49)],
    # fewer candidates than the beam
    "F": [(40, 4, 0, ((1, 2),), 5, 24), (40, 4, 0, ((1, 2),), 16, 4)],
    # beam > 16: the workgroup kernels' bitonic sort only
    "G": [(30, 29, 0, ((1, 2), (5, 6)), 40, 3), (33, 12, 5, ((1, 2), (7, 8)), 32, 10)],
    # LM fusion over A, B, D with a symmetric table
    "L": [(70, 29, 0, P_A, 5, 3, ALPHA, BETA, 1), (70, 29, 0, P_A, 16, 3, ALPHA, BETA, 3),
          (70, 29, 3, P_A, 5, 2, ALPHA, BETA, 7), (70, 29, 3, P_A, 16, 2, ALPHA, BETA, 2),
          (70, 40, 0, ((1, 2), (5, 33)), 5, 2, ALPHA, BETA, 6), (70, 40, 0, ((1, 2), (5, 33)), 16, 2, ALPHA, BETA, 6)],
}
CASES = [c for g in GROUPS.values() for c in g]
SINGLE_WAVE = [c for g in "ABCDEF" for c in GROUPS[g]]        # beam <= 16, no LM: ctc_beam_search's default dispatch
NOLM = [c for g in "ABCDEFG" for c in GROUPS[g]]
LM = GROUPS["L"]


def conditions(case):
    """The conditions tests/test_beam_ties_cpu.py asserts on one case, as a list of failure strings (empty: the case is valid); the
    seed scan and the test share this one statement."""
    T, V, blank, pairs, beam, order, alpha, beta, seed = parse(case)
    lens = lengths_of(T)
    bad, first_differs, cut_ties = [], 0, 0
    for b, (hyps, rep) in enumerate(reference(case)):
        if not rep["margin"] >= R.GAP_MIN:
            bad.append(f"utterance {b}: smallest non-zero margin {rep['margin']:.3e} < {R.GAP_MIN}")
        if lens[b] >= 33:
            same = hyps[0][0] == rep["last_touch"][0][0] if beam == 1 else [h[0] for h in hyps] == [h[0] for h in rep["last_touch"]]
            if same:
                bad.append(f"utterance {b}: the last-touch rule gives the same {'1-best' if beam == 1 else 'list'}")
        first_differs += hyps[0][0] != rep["last_touch"][0][0]
        cut_ties += rep["cut_ties"]
    if not first_differs:
        bad.append("no utterance whose 1-best differs under the last-touch rule")
    if not cut_ties:
        bad.append("no frame whose cut is an exact tie")
    return bad
