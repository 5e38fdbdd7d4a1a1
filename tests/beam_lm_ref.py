"""Helper of the LM-fusion tests (not collected): the fused prefix beam search as the best entry of prefix_beam_ref's one loop
(stated there: ``decode_ref.prefix_beam_search`` with  w = alpha * float(table[ctx(prefix), s]) + beta  on every extension), the
shared inputs of the CPU and GPU tests, and the shared list of GPU cases."""
import numpy as np

from prefix_beam_ref import nbest_prefix_beam_search


def fused_prefix_beam_search(probs=None, table=None, order=0, alpha=0.0, beta=0.0, beam_size=100, blank=0, logp=None):
    """probs (T,V) probabilities (their numpy log is taken, like decode_ref) or logp (T,V) log-probabilities.
    table: None or an array of shape (V,)*order.  Returns (prefix tuple, score, gap): score = -lse(p_b, p_nb) of the best
    entry; gap = the smallest margin a ranking decision of this search had -- per frame the score of the last kept candidate
    minus the first dropped one, at the end the best minus the second-best final entry (inf if there was no such decision).
    The loop is prefix_beam_ref's, asked for a list of one."""
    hyps, gap = nbest_prefix_beam_search(probs=probs, table=table, order=order, alpha=alpha, beta=beta, beam_size=beam_size,
                                         blank=blank, logp=logp, nbest=1)
    return hyps[0][0], hyps[0][1], gap


def random_table(V, order, blank, seed, scale=2.0):
    """A random LM: per context a log-softmax over the non-blank symbols of scale * N(0,1) logits, fp32; blank column 0."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((V,) * order, dtype=np.float32) * np.float32(scale)
    z[..., blank] = -np.inf
    m = z.max(axis=-1, keepdims=True)
    t = z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))
    t[..., blank] = 0.0
    return np.ascontiguousarray(t, dtype=np.float32)


def log_softmax32(logits):
    """fp64 log-softmax over the last axis, rounded to fp32: the log-probs BOTH the device and the helper are given."""
    m = logits.max(axis=-1, keepdims=True)
    return (logits - (m + np.log(np.exp(logits - m).sum(axis=-1, keepdims=True)))).astype(np.float32)


# The cases the fp32 device path is compared on token for token: (T, V, beam, order, blank, alpha, beta, seed).
# Every one must have a helper gap >= GAP_MIN on every utterance (test_beam_lm_cpu.py checks it; the seeds were picked so):
# the two fp32 kernels agree with fp64 to ~1e-7 relative on scores of magnitude ~1e2, i.e. ~1e-5 absolute, so 1e-4 leaves
# roughly 10x over the largest error that could flip a cut.
GAP_MIN = 1e-4
FAST_CASES = [
    (1, 29, 16, 3, 0, 0.8, 0.5, 0),
    (8, 29, 5, 2, 0, 0.5, 0.0, 1),
    (60, 4, 16, 3, 0, 1.0, 1.0, 0),
    (120, 29, 16, 3, 0, 0.7, 1.2, 2),
    (200, 29, 5, 4, 0, 0.4, 0.8, 0),
    (90, 29, 16, 2, 3, 0.9, 0.3, 2),
    (100, 48, 16, 3, 0, 0.6, 0.6, 0),
    (80, 64, 5, 2, 63, 1.0, 0.0, 0),
    (150, 29, 1, 3, 0, 0.5, 0.5, 0),
    (300, 29, 7, 1, 0, 1.0, 0.5, 0),
    (30, 29, 100, 3, 0, 0.5, 1.0, 5),
]
FAST_B = 5


def fast_case_inputs(case):
    """(log-probs (T,B,V) fp32, lengths (B) int32 with a 1 and a 0 among them, table fp32) of one shared case."""
    T, V, beam, order, blank, alpha, beta, seed = case
    rng = np.random.default_rng(1000003 * seed + 1009 * T + 31 * V + beam)
    logits = rng.normal(size=(T, FAST_B, V)) * rng.choice([0.3, 2.0, 5.0], size=(T, FAST_B, 1))
    logits[:, :, blank] += 1.5
    lens = np.array([T, max(0, T - T // 3), min(1, T), 0, max(0, T - 7)], dtype=np.int32)
    return log_softmax32(logits), lens, random_table(V, order, blank, seed + 17)


# The headline shape: T = 1000, B = 32, V = 29, beam 16, order 3; utterances HEADLINE_CHECK cut to 150 frames go to the helper.
HEADLINE = (1000, 32, 29, 16, 3, 0, 0.6, 0.8, 3)      # (T, B, V, beam, order, blank, alpha, beta, seed)
HEADLINE_CHECK, HEADLINE_CUT = (0, 31), 150


def headline_inputs():
    T, B, V, beam, order, blank, alpha, beta, seed = HEADLINE
    rng = np.random.default_rng(424242 + seed)
    logits = rng.normal(size=(T, B, V)) * 2.0
    return log_softmax32(logits), random_table(V, order, blank, seed + 5)
