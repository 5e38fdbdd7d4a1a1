"""Helper of the hotword-bias tests (not collected): the bias of a token row straight from its definition, the per-extension bonus
of a ``lm.HotwordBias`` as a callable for prefix_beam_ref's one plain-Python search, and the shared cases and inputs of the CPU and
GPU tests.

The definition (lm.HotwordBias, include/pgasr_hip.h A7-BIAS):
    B(y) = sum over phrases p of (occurrences of p in y, overlapping ones included) * w(p)
           + partial * boost * (length of the longest suffix of y that is a PROPER prefix of some phrase)."""
import functools

import numpy as np

import beam_lm_ref as L
from prefix_beam_ref import nbest_prefix_beam_search


def brute_bias(y, phrases, weights, boost=1.0, partial=1.0):
    """B(y) in Python floats, no automaton."""
    y = tuple(int(t) for t in y)
    total = 0.0
    for p, w in zip(phrases, weights):
        p = tuple(p)
        total += float(w) * sum(1 for i in range(len(y) - len(p) + 1) if y[i:i + len(p)] == p)
    pending = max([k for p in phrases for k in range(1, len(p)) if k <= len(y) and y[len(y) - k:] == tuple(p[:k])], default=0)
    return total + partial * boost * pending


def bonus_callable(bias, gamma, table=None, order=0, alpha=0.0, beta=0.0):
    """bonus(prefix, s) for ``nbest_prefix_beam_search``: ``bias.transition`` along the prefix, memoised.  Without a table
    gamma * float(bonus); with one  alpha * float(table[ctx + (s,)]) + beta + gamma * float(bonus)  in that order, in Python floats --
    the device's roundings."""
    gamma, alpha, beta = float(gamma), float(alpha), float(beta)
    states = {(): 0}

    def state(prefix):
        q = states.get(prefix)
        if q is None:
            q = states[prefix] = bias.transition(state(prefix[:-1]), prefix[-1])[0]
        return q

    def bonus(prefix, s):
        w = gamma * bias.transition(state(prefix), s)[1]
        if table is None:
            return w
        n1 = order - 1
        tail = prefix[-n1:] if n1 else ()
        ctx = (bias.blank,) * (n1 - len(tail)) + tuple(tail)
        return alpha * float(table[ctx + (s,)]) + beta + w

    return bonus


# The shared cases: (T, V, beam, blank, LM order, gamma, kind, seed).  LM weights where there is an LM: ALPHA, BETA.
# kind "mixed": phrases half substrings of the utterances' unbiased 1-best, half random; "overlap": the same over 3 symbols with
# {(1,1,2), (1,2), (2,1,1,3)} among them; "big": the same on top of BIG_PHRASES random phrases of length 8 -- an automaton of more
# than 20000 states (3000 such phrases over 28 symbols cannot reach that: at most 28 + 28^2 + 6 * 3000 = 18812 states).
# Every case must satisfy the qualifying conditions test_hotword_cpu.py asserts; the seeds were picked so.
ALPHA, BETA = 0.7, 1.2
BIG_PHRASES = 3400
B = L.FAST_B
CASES = [
    (1, 29, 16, 0, 0, 1.0, "mixed", 8),
    (60, 4, 16, 0, 0, 1.5, "overlap", 0),
    (120, 29, 16, 0, 3, 1.0, "mixed", 0),
    (90, 29, 40, 3, 0, 1.0, "mixed", 3),            # 1160 candidates: more than BEAM_LM_PRE * 256, so the in-place loads run
    (80, 64, 5, 63, 2, 0.8, "mixed", 0),
    (150, 29, 1, 0, 0, 2.0, "mixed", 0),
    (30, 29, 100, 0, 0, 1.0, "mixed", 4),
    (100, 48, 16, 0, 0, 1.0, "mixed", 2),
    (100, 29, 16, 0, 0, 1.0, "big", 0),
]
EXACT_CASES = (1, 2, 4)      # the cases run on fp64 input as well; 2 and 4 carry the LM


def case_id(c):
    return "T%d-V%d-K%d-b%d-n%d-g%s-%s" % c[:7]


def nbest_of(case):
    return min(case[2], 16)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(log-probs (T,B,V) fp32, lengths (B) int32 with a 1 and a 0 among them, LM table fp32 or None, the lm.HotwordBias, the
    unbiased 1-best of every utterance) of one shared case.  Computed once per process; callers leave the arrays unchanged."""
    from policy_gradient_asr_amd.lm import HotwordBias
    T, V, beam, blank, order, gamma, kind, seed = case
    rng = np.random.default_rng(7919 * seed + 1009 * T + 31 * V + beam)
    logits = rng.normal(size=(T, B, V)) * rng.choice([0.3, 2.0, 5.0], size=(T, B, 1))
    logits[:, :, blank] += 1.5
    lens = np.array([T, max(0, T - T // 3), min(1, T), 0, max(0, T - 7)], dtype=np.int32)
    lp = L.log_softmax32(logits)
    table = L.random_table(V, order, blank, seed + 17) if order else None
    symbols = [s for s in range(V) if s != blank]
    plain = []
    for b in range(B):
        hyps, _ = nbest_prefix_beam_search(logp=lp[:int(lens[b]), b].astype(np.float64), table=table, order=order, alpha=ALPHA,
                                           beta=BETA, beam_size=beam, blank=blank, nbest=1)
        plain.append(tuple(hyps[0][0]))
    phrases = []
    if kind == "overlap":
        phrases += [(1, 1, 2), (1, 2), (2, 1, 1, 3)]
    if kind == "big":
        phrases += [tuple(p) for p in rng.choice(symbols, size=(BIG_PHRASES, 8)).tolist()]
    for y in plain:                                   # half substrings of the 1-best, half random
        for _ in range(2):
            n = int(rng.integers(2, 6))
            if len(y) >= 1:
                n = min(n, len(y))
                i = int(rng.integers(0, len(y) - n + 1))
                phrases.append(tuple(y[i:i + n]))
            phrases.append(tuple(rng.choice(symbols, size=int(rng.integers(2, 6))).tolist()))
    bias = HotwordBias(phrases, V, blank=blank, boost=1.0, partial=1.0)
    return lp, lens, table, bias, tuple(plain)


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """Per utterance (hyps, gap) of the biased plain-Python search at N = nbest_of(case): the list and the smallest margin of any
    ranking decision it depends on (rank 0 against rank 1 included, so the 1-best tests share it)."""
    T, V, beam, blank, order, gamma, kind, seed = case
    lp, lens, table, bias, _ = case_inputs(case)
    out = []
    for b in range(B):
        bonus = bonus_callable(bias, gamma, table, order, ALPHA, BETA)
        out.append(nbest_prefix_beam_search(logp=lp[:int(lens[b]), b].astype(np.float64), beam_size=beam, blank=blank,
                                            nbest=nbest_of(case), bonus=bonus))
    return tuple(out)
