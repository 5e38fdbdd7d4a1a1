"""Helper of the wide beam-search tests (not collected): the shared cases, their inputs and their reference lists.

The oracle is ``nbest_ref.nbest_prefix_beam_search`` (plain Python over all V symbols); the input recipe is that of
``beam_lm_ref.fast_case_inputs`` without the table, with the number of utterances a field of the case: the plain-Python search needs
seconds per utterance at V = 1024, so the cases above V = 300 are short and have few utterances.  Every case must have a smallest
decision margin of at least ``beam_lm_ref.GAP_MIN`` on every utterance (tests/test_beam_wide_cpu.py asserts it; the seeds are per case
the first of 0, 1, 2, .. that meets it)."""
import functools

import numpy as np

import beam_lm_ref as R
import nbest_ref as NR

GAP_MIN = R.GAP_MIN


def lengths_of(T, B):
    """B lengths with a 1 and a 0 among them (B >= 3)."""
    return np.array([T, max(0, T - T // 3), min(1, T), 0, max(0, T - 7)][:B] if B >= 4 else [T, min(1, T), 0][:B], dtype=np.int32)


# (T, V, beam, blank, B, seed): V in {65, 128, 129, 300, 1000, 1023, 1024}, blank first / in the middle / last, beam in {1, 5, 16, 32, 128}
CASES = [
    (40, 65, 16, 32, 5, 1),
    (30, 128, 1, 0, 5, 0),
    (20, 129, 128, 64, 4, 1),
    (40, 257, 5, 3, 5, 0),
    (50, 300, 16, 299, 5, 3),
    (24, 1000, 32, 7, 3, 0),
    (24, 1023, 5, 1022, 4, 0),
    (30, 1024, 16, 0, 4, 0),
    (6, 1024, 128, 512, 3, 2),
]


def case_id(case):
    return "T%d-V%d-K%d-b%d-B%d-s%d" % case


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(log-probs (T,B,V) fp32, lengths (B) int32) of one case: per-frame scale from {0.3, 2.0, 5.0}, +1.5 on blank, fp64 log-softmax
    rounded to fp32.  Callers must not write into the arrays."""
    T, V, beam, blank, B, seed = case
    rng = np.random.default_rng(1000003 * seed + 1009 * T + 31 * V + beam)
    logits = rng.normal(size=(T, B, V)) * rng.choice([0.3, 2.0, 5.0], size=(T, B, 1))
    logits[:, :, blank] += 1.5
    lp = R.log_softmax32(logits)
    lp.setflags(write=False)
    return lp, lengths_of(T, B)


# The two cases of the selection paths, V = 1024, beam 16, (T, B, seed).  FLAT: near-uniform rows (scale 0.2, no bonus on blank) in the
# odd frames and a peaked row (scale 8) before each: the entries' totals are then spread far wider than a frame's log-probs, the first
# few entries' ~1023 extensions each lie above the threshold, and the kernel's list of 2048 items (WIDE_CAP) overflows.  PEAKED: scale 5 in every
# frame, +1.5 on blank: the list stays short.
FLAT = (8, 2, 1)
PEAKED = (24, 2, 0)
SELECT_V, SELECT_BEAM, SELECT_BLANK = 1024, 16, 0


@functools.lru_cache(maxsize=None)
def select_inputs(kind):
    T, B, seed = FLAT if kind == "flat" else PEAKED
    rng = np.random.default_rng(7919 * seed + 1009 * T + (1 if kind == "flat" else 2))
    if kind == "flat":
        scale = np.where(np.arange(T) % 2 == 0, 8.0, 0.2).reshape(T, 1, 1)
        logits = rng.normal(size=(T, B, SELECT_V)) * scale
    else:
        logits = rng.normal(size=(T, B, SELECT_V)) * 5.0
        logits[:, :, SELECT_BLANK] += 1.5
    lp = R.log_softmax32(logits)
    lp.setflags(write=False)
    return lp, np.full((B,), T, dtype=np.int32)


def list_size(beam):
    return NR.list_size(beam)


def _reference(lp, lens, beam, blank):
    out = []
    for b in range(lp.shape[1]):
        n = int(lens[b])
        if n == 0:
            out.append(([((), -0.0)], float("inf")))
        else:
            out.append(NR.nbest_prefix_beam_search(logp=lp[:n, b].astype(np.float64), beam_size=beam, blank=blank, nbest=list_size(beam)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(case):
    """Per utterance (hyps, gap) at N = list_size(beam), computed once per process."""
    T, V, beam, blank, B, seed = case
    lp, lens = case_inputs(case)
    return _reference(lp, lens, beam, blank)


@functools.lru_cache(maxsize=None)
def select_reference(kind):
    lp, lens = select_inputs(kind)
    return _reference(lp, lens, SELECT_BEAM, SELECT_BLANK)


# Tie cases in beam_tie_ref's form (T, V, blank, pairs, beam, seed): twin pairs that straddle 64-symbol boundaries.  Seeds: from a
# scan over 0, 1, 2, .. for tests/test_beam_wide_cpu.py's conditions (the two V = 130 cases: the first seed that meets all of
# beam_tie_ref.conditions; the V = 1024 case: the first whose cuts include an exact tie).  The V = 1024 case is short (beam_tie_ref's lengths are then [12, 8, 12, 1, 0]) to keep the plain-Python
# searches within seconds, and has eight pairs: among 1024 symbols a single pair seldom reaches the beam.
WIDE_PAIRS = ((63, 960), (64, 65), (5, 700), (127, 128), (255, 256), (511, 512), (300, 900), (31, 992))
TIE_CASES = [
    (40, 130, 0, ((5, 100), (64, 65)), 5, 3),
    (40, 130, 7, ((5, 100), (64, 65)), 16, 9),
    (12, 1024, 0, WIDE_PAIRS, 5, 3),
]
