"""Helper of the wide hotword-bias tests (not collected): the shared cases of the biased WIDE search (rows of 65 .. 1024 symbols, with
and without the back-off unit LM), their inputs, phrase lists and reference lists, and the figures the CPU test holds them to.

Nothing is restated here.  The inputs are those of ``beam_wide_cases`` / ``unit_lm_ref`` (the same recipes, through their own
functions), the oracle is ``prefix_beam_ref.nbest_prefix_beam_search(bonus=...)`` at N = ``nbest_ref.list_size(beam)``, and its
callable is composed of ``hotword_ref.bonus_callable`` (gamma * float(bonus) along the automaton) and ``unit_lm_ref.dict_bonus``
(alpha * query + beta over the dict statement): without a model  w = gamma * float(bonus), with one
w = (alpha * query + beta) + gamma * float(bonus), in that order -- the device's roundings (include/pgasr_hip.h, A7-WIDE-BIAS)."""
import functools

import numpy as np

import beam_lm_ref as R
import beam_wide_cases as W
import hotword_ref as H
import nbest_ref as NR
import unit_lm_ref as U
from prefix_beam_ref import nbest_prefix_beam_search

GAP_MIN = R.GAP_MIN
ALPHA, BETA = 0.8, 0.5               # the unit LM's weights where a case has one
BIG_PHRASES, BIG_LEN, BIG_STATES = 1900, 7, 12000
OVERLAP_BOOST = 4.0                  # added to the logits of the three symbols the overlap case spells its hypotheses from

# (T, V, beam, blank, B, unit-LM order or 0, gamma, kind, seed).  seed: per case the first of 0, 1, 2, .. that meets the conditions
# tests/test_wide_hotword_cpu.py asserts (found by a scan on the CPU); it seeds the inputs and the phrases -- the flat case takes
# beam_wide_cases.select_inputs("flat") as they are, and its seed picks the phrases only.
#   "mixed":   half the phrases are substrings of rows of the unbiased reference list (any rank, not only the best), half random, 2 to
#              5 units long;
#   "overlap": symbols a, b, c on different sides of 64-symbol boundaries get +4 on their logits; phrases {(a,a,b), (a,b), (b,a,a,c)}
#              plus mixed ones: failure links, nested phrases, and the negative bonus of leaving a phrase;
#   "flat":    V = 1024, beam 16, near-uniform rows: the threshold list overflows and the counting selection runs unforced;
#   "big":     BIG_PHRASES random phrases of length 7 on top of mixed ones: at least 12000 states, about 100 MB of table, near the
#              limit of 2**24 table words.
CASES = [
    (40, 65, 16, 32, 5, 0, 1.0, "mixed", 0),
    (30, 128, 1, 0, 5, 0, 2.0, "mixed", 0),
    (20, 129, 128, 64, 4, 3, 1.0, "mixed", 0),
    (40, 300, 5, 299, 5, 5, 1.0, "mixed", 0),
    (40, 130, 32, 0, 5, 0, 1.5, "overlap", 0),
    (24, 1000, 32, 7, 3, 0, 1.0, "mixed", 0),
    (6, 1024, 128, 512, 3, 0, 1.5, "mixed", 0),
    (W.FLAT[0], W.SELECT_V, W.SELECT_BEAM, W.SELECT_BLANK, W.FLAT[1], 0, 0.5, "flat", 0),
    (12, 1024, 16, 0, 3, 0, 1.0, "big", 0),
]
EXACT_CASES = (2, 4, 6)      # the cases run on fp64 input as well: the one with the order-3 LM, the overlap one, V = 1024 x beam 128
ZERO_CASES = (0, 2, 5)       # weight 0 against the call without a bias; case 2 carries the LM
OVERLAP_SYMBOLS = (63, 64, 129)


def case_id(c):
    return "T%d-V%d-K%d-b%d-B%d-n%d-g%s-%s-s%d" % c


def list_size(beam):
    return NR.list_size(beam)


def _unit_case(case):
    T, V, beam, blank, B, order, gamma, kind, seed = case
    return (T, V, beam, order, blank, B, ALPHA, BETA, "mixed", seed)


@functools.lru_cache(maxsize=None)
def case_model(case):
    """(dict statement, lm.UnitNgramLM) of the case's unit LM, or (None, None)."""
    return U.case_model(_unit_case(case)) if case[5] else (None, None)


@functools.lru_cache(maxsize=None)
def _unbiased(case):
    """(log-probs (T,B,V) fp32, lengths (B) int32, the reference lists without a bias) of one case."""
    T, V, beam, blank, B, order, gamma, kind, seed = case
    if kind == "flat":
        return W.select_inputs("flat") + (W.select_reference("flat"),)
    if order:
        return U.case_inputs(_unit_case(case)) + (U.reference(_unit_case(case)),)
    if kind == "overlap":        # beam_wide_cases.case_inputs' recipe with the three symbols lifted
        rng = np.random.default_rng(1000003 * seed + 1009 * T + 31 * V + beam)
        logits = rng.normal(size=(T, B, V)) * rng.choice([0.3, 2.0, 5.0], size=(T, B, 1))
        logits[:, :, blank] += 1.5
        logits[:, :, list(OVERLAP_SYMBOLS)] += OVERLAP_BOOST
        lp, lens = R.log_softmax32(logits), W.lengths_of(T, B)
        lp.setflags(write=False)
        return lp, lens, W._reference(lp, lens, beam, blank)
    wcase = (T, V, beam, blank, B, seed)
    return W.case_inputs(wcase) + (W.reference(wcase),)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(log-probs (T,B,V) fp32, lengths (B) int32, the lm.HotwordBias, the unbiased 1-best of every utterance).  Computed once per
    process; callers leave the arrays unchanged."""
    from policy_gradient_asr_amd.lm import HotwordBias
    T, V, beam, blank, B, order, gamma, kind, seed = case
    lp, lens, plain = _unbiased(case)
    rng = np.random.default_rng(7919 * seed + 1009 * T + 31 * V + beam + 5)
    symbols = [s for s in range(V) if s != blank]
    phrases = []
    if kind == "overlap":
        a, b, c = OVERLAP_SYMBOLS
        phrases += [(a, a, b), (a, b), (b, a, a, c)]
        symbols = list(OVERLAP_SYMBOLS)                  # the random phrases too are over the symbols the hypotheses are spelled from
    if kind == "big":
        phrases += [tuple(p) for p in rng.choice(symbols, size=(BIG_PHRASES, BIG_LEN)).tolist()]
    for hyps, _ in plain:
        for _ in range(2):
            y = tuple(hyps[int(rng.integers(0, len(hyps)))][0])      # a row of the list, below the best as well
            if len(y) >= 2:
                n = min(int(rng.integers(2, 6)), len(y))
                i = int(rng.integers(0, len(y) - n + 1))
                phrases.append(y[i:i + n])
            if kind != "flat":
                phrases.append(tuple(rng.choice(symbols, size=int(rng.integers(2, 6))).tolist()))
    bias = HotwordBias(phrases, V, blank=blank, boost=1.0, partial=1.0)
    return lp, lens, bias, tuple(tuple(h[0][0]) for h, _ in plain)


def bonus_of(case):
    """The oracle's callable of one case: hotword_ref's, plus unit_lm_ref's in front of it where the case has a model."""
    T, V, beam, blank, B, order, gamma, kind, seed = case
    hot = H.bonus_callable(case_inputs(case)[2], gamma)
    if not order:
        return hot
    lm = U.dict_bonus(case_model(case)[0], order, blank, ALPHA, BETA)
    return lambda prefix, s: lm(prefix, s) + hot(prefix, s)


@functools.lru_cache(maxsize=None)
def reference(case):
    """Per utterance (hyps, gap) of the biased plain-Python search at N = list_size(beam), computed once per process."""
    T, V, beam, blank, B, order, gamma, kind, seed = case
    lp, lens, bias, _ = case_inputs(case)
    bonus = bonus_of(case)
    out = []
    for b in range(lp.shape[1]):
        n = int(lens[b])
        if n == 0:
            out.append(([((), -0.0)], float("inf")))
        else:
            out.append(nbest_prefix_beam_search(logp=lp[:n, b].astype(np.float64), beam_size=beam, blank=blank, nbest=list_size(beam),
                                                bonus=bonus))
    return tuple(out)


def figures(case):
    """What the qualifying conditions are about: the smallest decision gap, the utterances whose 1-best the bias changes, the
    non-empty utterances and those among them whose best row has B(y) != 0, the most negative bonus on a best row's path, the
    automaton's states."""
    lp, lens, bias, plain = case_inputs(case)
    ref = reference(case)
    gap, changed, live, nonzero, lowest = float("inf"), 0, 0, 0, 0.0
    for b, (hyps, g) in enumerate(ref):
        best = tuple(hyps[0][0])
        gap = min(gap, g)
        changed += best != plain[b]
        if int(lens[b]) > 0:
            live += 1
            nonzero += H.brute_bias(best, bias.phrases, bias.weights) != 0
        q = 0
        for s in best:
            q, w = bias.transition(q, s)
            lowest = min(lowest, w)
    return {"gap": gap, "changed": changed, "live": live, "nonzero": nonzero, "lowest": lowest, "states": bias.n_states}


def qualifies(case, fig=None):
    fig = figures(case) if fig is None else fig
    ok = fig["gap"] >= GAP_MIN and fig["changed"] >= 1 and 2 * fig["nonzero"] >= fig["live"]
    if case[7] == "overlap":
        ok = ok and fig["lowest"] < 0
    if case[7] == "big":
        ok = ok and fig["states"] >= BIG_STATES
    return ok
