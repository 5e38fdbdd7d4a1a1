"""Helper of the N-best tests (not collected): ``nbest_prefix_beam_search`` -- prefix_beam_ref's one loop, under the name the tests
know: the first N entries of the final beam with their scores and the margin of every ranking decision behind such a list --, the
shared no-LM cases of the fp32 path, and a numpy statement of the rescoring kernel (csrc/nbest.hip) term by term."""
import functools

import numpy as np

import beam_lm_ref as R
from prefix_beam_ref import nbest_prefix_beam_search      # noqa: F401 -- the tests call nbest_ref.nbest_prefix_beam_search


# The no-LM cases the fp32 path is compared on token for token at N = min(beam, 16): (T, V, beam, blank, seed), inputs from
# beam_lm_ref.fast_case_inputs with the table left out.  Four of beam_lm_ref.FAST_CASES fall short of GAP_MIN without their table
# (T=120/seed 2, T=100/V=48, T=300/beam 7, T=30/beam 100: 2.7e-5 .. 9.8e-5), so this list has seeds of its own, picked so that every
# utterance of every case has gap >= beam_lm_ref.GAP_MIN (tests/test_nbest_cpu.py asserts it).
NOLM_CASES = [
    (1, 29, 16, 0, 0),
    (8, 29, 5, 0, 1),
    (60, 4, 16, 0, 0),
    (120, 29, 16, 0, 4),
    (200, 29, 5, 0, 0),
    (90, 29, 16, 3, 2),
    (100, 48, 16, 0, 2),
    (80, 64, 5, 63, 0),
    (150, 29, 1, 0, 0),
    (300, 29, 7, 0, 6),
    (30, 29, 100, 0, 16),
]


def nolm_case_inputs(case):
    """(log-probs (T,B,V) fp32, lengths (B) int32 with a 1 and a 0 among them) of one no-LM case."""
    T, V, beam, blank, seed = case
    lp, lens, _ = R.fast_case_inputs((T, V, beam, 1, blank, 0.0, 0.0, seed))
    return lp, lens


def list_size(beam):
    return min(beam, 16)


@functools.lru_cache(maxsize=None)
def fast_reference(case, with_lm):
    """The helper's lists for one shared fp32 case, computed once per process: ``case`` from beam_lm_ref.FAST_CASES (with_lm) or from
    NOLM_CASES.  Returns a tuple over the FAST_B utterances of (hyps, gap) at N = list_size(beam); an utterance without frames has
    the one empty hypothesis with score -0.0 and gap inf."""
    if with_lm:
        T, V, beam, order, blank, alpha, beta, seed = case
        lp, lens, table = R.fast_case_inputs(case)
    else:
        T, V, beam, blank, seed = case
        (lp, lens), table, order, alpha, beta = nolm_case_inputs(case), None, 0, 0.0, 0.0
    out = []
    for b in range(R.FAST_B):
        n = int(lens[b])
        if n == 0:
            out.append(([((), -0.0)], float("inf")))
        else:
            out.append(nbest_prefix_beam_search(logp=lp[:n, b].astype(np.float64), table=table, order=order, alpha=alpha, beta=beta,
                                                beam_size=beam, blank=blank, nbest=list_size(beam)))
    return tuple(out)


def rescore_ref(tokens, lengths, count, am, V, blank, table, order, am_weight, lm_alpha, lm_beta):
    """pgasr_nbest_rescore in numpy: tokens (N,B,S) / lengths (N,B) / count (B) ints, am (N,B) float64, table None or (V,)*order fp32.
    Returns (order (B,N), total (N,B), lm_logp (N,B), abs_sum (N,B)): abs_sum = sum of |table word| per hypothesis, for the
    summation bound.  lm_logp here is an exactly rounded sum (math.fsum): the bound is the device's alone."""
    import math
    N, B, S = tokens.shape
    total = np.full((N, B), np.inf)
    lm_logp = np.zeros((N, B))
    abs_sum = np.zeros((N, B))
    out_order = np.zeros((B, N), dtype=np.int64)
    for b in range(B):
        cnt = min(max(int(count[b]), 0), N)
        for n in range(cnt):
            L = min(max(int(lengths[n, b]), 0), S)
            y = [int(x) for x in tokens[n, b, :L]]
            words = []
            if table is not None:
                n1 = order - 1
                for i, s in enumerate(y):
                    tail = tuple(y[max(0, i - n1):i]) if n1 else ()
                    ctx = (blank,) * (n1 - len(tail)) + tail                 # lm.py's rule: the last order-1 symbols, left-padded with blank
                    words.append(float(table[ctx + (s,)]))
            lm_logp[n, b] = math.fsum(words)
            abs_sum[n, b] = math.fsum(abs(w) for w in words)
            a = float(am[n, b])
            if np.isfinite(a):
                t1 = np.float64(am_weight) * np.float64(a)                     # each product and each sum rounded once, in this order
                t2 = np.float64(lm_alpha) * np.float64(lm_logp[n, b])
                t3 = np.float64(lm_beta) * np.float64(L)
                total[n, b] = (t1 + -t2) + -t3
        out_order[b] = list(np.argsort(total[:cnt, b], kind="stable")) + list(range(cnt, N))
    return out_order, total, lm_logp, abs_sum
