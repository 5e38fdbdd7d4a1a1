"""Helper of the word-fusion tests (not collected): the shared cases and inputs of the CPU and GPU tests, the per-extension bonus of a
``lm.WordFusion`` as a callable for prefix_beam_ref's one plain-Python search, and the finalisation as a stable sort over that
search's full final beam.

The contract (lm.WordFusion, include/pgasr_hip.h A7-WORDFUSE): every extension of a prefix y by a non-blank s adds
``fusion.bonus(y, s, alpha, beta)``; with ``finalize`` every entry of the final beam gets ``fusion.final(y, alpha, beta, eos)`` and the
beam is ranked again by lse(p_b, p_nb) + fin, equal totals in the search's order."""
import functools

import numpy as np

import beam_lm_ref as L
from prefix_beam_ref import nbest_prefix_beam_search

NEG_INF = -float("inf")
B = L.FAST_B

# (T, V, beam, blank, delimiter, order, oov_penalty, finalize, eos, alpha, beta, seed).  Between them: beam 1, 16, 40 (at V = 29: 1160
# candidates, more than BEAM_LM_PRE * 256, so the in-place loads run) and 100; the blank at 0 and at the last id; the delimiter next to
# the blank and at the last id; orders 1, 3 and 5; a finite oov_penalty and -inf; finalize and eos on and off.  Words have 1 .. 4 tokens,
# so dozens complete within an utterance.  Every case must satisfy the qualifying conditions test_word_fusion_cpu.py asserts; the
# seeds were picked so.
CASES = [
    (60, 6, 16, 0, 1, 3, -2.0, True, True, 0.5, 2.5, 0),
    (150, 8, 1, 0, 7, 1, -1.5, True, False, 0.6, 3.0, 0),
    (90, 29, 40, 0, 28, 3, -3.0, True, True, 0.4, 2.0, 4),
    (40, 5, 100, 4, 3, 5, NEG_INF, True, True, 0.6, 0.5, 10),
    (120, 7, 16, 6, 0, 5, -2.5, False, False, 0.5, 2.2, 0),
    (80, 8, 16, 0, 1, 3, NEG_INF, True, False, 0.5, 1.0, 0),
]
EXACT_CASES = (0, 3, 4)      # the cases run on fp64 input as well
ZERO_CASES = (0, 2, 4)       # the cases run with zero weights against the unfused search


def case_id(c):
    return "T%d-V%d-K%d-b%d-d%d-n%d-p%s-f%d-e%d" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8])


def nbest_of(case):
    return min(case[2], 16)


def random_word_lm(V, blank, delimiter, order, seed, n_words=30, n_lines=120):
    """A ``lm.WordNgramLM`` over random words of 1 .. 4 tokens (neither blank nor delimiter), estimated from random sentences; the
    lexicon's words as token tuples beside it."""
    from policy_gradient_asr_amd.lm import WordNgramLM
    rng = np.random.default_rng(90001 * seed + 131 * V + order)
    symbols = [s for s in range(V) if s not in (blank, delimiter)]
    char2ind = {chr(ord("a") + s): s for s in range(V)}
    words = sorted({tuple(rng.choice(symbols, size=int(rng.integers(1, 5))).tolist()) for _ in range(n_words)})
    p = rng.dirichlet(np.full(len(words), 0.5))
    lines = []
    for _ in range(n_lines):
        ids = rng.choice(len(words), size=int(rng.integers(1, 9)), p=p)
        lines.append(chr(ord("a") + delimiter).join("".join(chr(ord("a") + t) for t in words[i]) for i in ids))
    lm = WordNgramLM.from_text(lines, char2ind, order=order, delimiter=chr(ord("a") + delimiter), blank=blank)
    return lm, [tuple(s) for s in lm.spellings[3:]]


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(log-probs (T,B,V) fp32, lengths (B) int32 with a 1 and a 0 among them, the lm.WordFusion) of one shared case: the acoustics
    follow a sentence of lexicon words with some tokens swapped, under noise of three strengths.  Computed once per process; callers
    leave the arrays unchanged."""
    from policy_gradient_asr_amd.lm import WordFusion
    T, V, beam, blank, d, order, pen, finalize, eos, alpha, beta, seed = case
    lm, words = random_word_lm(V, blank, d, order, seed)
    fusion = WordFusion(lm, V, d, blank=blank, oov_penalty=pen)
    rng = np.random.default_rng(7919 * seed + 1009 * T + 31 * V + beam)
    symbols = [s for s in range(V) if s not in (blank, d)]
    logits = rng.normal(size=(T, B, V)) * rng.choice([0.3, 1.0, 2.0], size=(T, B, 1))
    logits[:, :, blank] += 2.0
    for b in range(B):
        t = int(rng.integers(0, 3))
        while t < T:
            for tok in words[int(rng.integers(len(words)))] + (d,):
                if rng.random() < 0.1:
                    tok = int(rng.choice(symbols))
                if t < T:
                    logits[t, b, tok] += 4.5
                t += int(rng.integers(1, 4))
    lens = np.array([T, max(0, T - T // 3), min(1, T), 0, max(0, T - 7)], dtype=np.int32)
    return L.log_softmax32(logits), lens, fusion


def bonus_callable(fusion, alpha, beta):
    """bonus(prefix, s) for ``nbest_prefix_beam_search``, from ``WordFusion.bonus`` (which remembers the state of every prefix)."""
    return lambda prefix, s: fusion.bonus(prefix, s, alpha, beta)


def finalise(fusion, beam, alpha, beta, eos, nbest):
    """The finalisation over the helper's full final beam [(prefix, score = -lse)]: total = lse + fin, a stable sort descending in
    it.  Returns (the first ``nbest`` rows as [(prefix, -total)], the smallest margin between adjacent ranks r, r + 1 for r < nbest
    whose better total is not -inf)."""
    tot = [-sc + fusion.final(y, alpha, beta, eos) for y, sc in beam]
    order = sorted(range(len(beam)), key=lambda r: -tot[r])          # sorted() is stable: equal totals keep the search's order
    gap = float("inf")
    for r in range(min(nbest, len(order))):
        if r + 1 < len(order) and tot[order[r]] != NEG_INF:
            gap = min(gap, tot[order[r]] - tot[order[r + 1]])
    return [(beam[r][0], -tot[r]) for r in order[:nbest]], gap


def own_path_count(frames, delimiter):
    """Entries of the kept beams whose last symbol is the delimiter while their parent prefix is in the same beam: the merged term of
    their stay candidate is the device's ``own``."""
    n = 0
    for kept in frames:
        have = set(kept)
        n += sum(1 for y in kept if y and y[-1] == delimiter and y[:-1] in have)
    return n


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """Per utterance a dict: hyps (the N = nbest_of(case) rows the device must return, [(prefix, score)]), gap (the smallest margin
    of any ranking decision they depend on: every frame's cut, every adjacent pair of the search's final beam, and with finalize the
    adjacent pairs of the final ranking), search_best (rank 0 of the search's own list), own (``own_path_count``)."""
    T, V, beam, blank, d, order, pen, finalize, eos, alpha, beta, seed = case
    lp, lens, fusion = case_inputs(case)
    out = []
    for b in range(B):
        report = {}
        full, gap = nbest_prefix_beam_search(logp=lp[:int(lens[b]), b].astype(np.float64), beam_size=beam, blank=blank, nbest=beam,
                                             bonus=bonus_callable(fusion, alpha, beta), report=report)
        hyps = full[:nbest_of(case)]
        if finalize:
            hyps, fgap = finalise(fusion, full, alpha, beta, eos, nbest_of(case))
            gap = min(gap, fgap)
        out.append(dict(hyps=hyps, gap=gap, search_best=full[0][0], own=own_path_count(report["frames"], d)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def plain_best(case):
    """The unfused 1-best of every utterance."""
    T, V, beam, blank = case[:4]
    lp, lens, _ = case_inputs(case)
    return tuple(tuple(nbest_prefix_beam_search(logp=lp[:int(lens[b]), b].astype(np.float64), beam_size=beam, blank=blank, nbest=1)[0][0][0])
                 for b in range(B))
