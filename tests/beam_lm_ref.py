"""Helper of the LM-fusion tests (not collected): a plain-Python fused prefix beam search written against
oracle.decode_ref, the shared inputs of the CPU and GPU tests, and the shared list of GPU cases.

The fused search is ``decode_ref.prefix_beam_search`` with ONE change: every term that enters a prefix by an extension with a
non-blank s gets  w = alpha * float(table[ctx(prefix), s]) + beta  added -- (p_b + p) + w, (p_nb + p) + w.  The blank update
and the repeat branch that keeps the prefix are unchanged.  ctx(prefix) = its last order-1 symbols, left-padded with blank."""
import numpy as np

from oracle.decode_ref import NEG_INF, _lse


def fused_prefix_beam_search(probs=None, table=None, order=0, alpha=0.0, beta=0.0, beam_size=100, blank=0, logp=None):
    """probs (T,V) probabilities (their numpy log is taken, like decode_ref) or logp (T,V) log-probabilities.
    table: None or an array of shape (V,)*order.  Returns (prefix tuple, score, gap): score = -lse(p_b, p_nb) of the best
    entry; gap = the smallest margin a ranking decision of this search had -- per frame the score of the last kept candidate
    minus the first dropped one, at the end the best minus the second-best final entry (inf if there was no such decision)."""
    if logp is None:
        with np.errstate(divide="ignore"):
            logp = np.log(probs)
    T, V = logp.shape
    alpha, beta = float(alpha), float(beta)

    def bonus(prefix, s):
        if table is None:
            return 0.0
        n1 = order - 1
        tail = prefix[-n1:] if n1 else ()
        ctx = (blank,) * (n1 - len(tail)) + tuple(tail)
        return alpha * float(table[ctx + (s,)]) + beta

    gap = float("inf")
    beam = [((), 0.0, NEG_INF)]
    for t in range(T):
        tab = {}  # prefix -> [p_b, p_nb]; dict keeps first-touch order

        def slot(key):
            e = tab.get(key)
            if e is None:
                e = [NEG_INF, NEG_INF]
                tab[key] = e
            return e

        for s in range(V):
            p = logp[t, s]
            for prefix, p_b, p_nb in beam:
                if s == blank:
                    e = slot(prefix)
                    e[0] = _lse(e[0], p_b + p, p_nb + p)
                    continue
                last = prefix[-1] if prefix else None
                w = bonus(prefix, s)
                e = slot(prefix + (s,))
                if s != last:
                    e[1] = _lse(e[1], (p_b + p) + w, (p_nb + p) + w)
                else:
                    e[1] = _lse(e[1], (p_b + p) + w)
                    e2 = slot(prefix)
                    e2[1] = _lse(e2[1], p_nb + p)
        ranked = sorted(tab.items(), key=lambda kv: _lse(kv[1][0], kv[1][1]), reverse=True)
        if len(ranked) > beam_size:
            kept, dropped = _lse(*ranked[beam_size - 1][1]), _lse(*ranked[beam_size][1])
            if kept != NEG_INF:
                gap = min(gap, kept - dropped)
        ranked = ranked[:beam_size]
        beam = [(k, v[0], v[1]) for k, v in ranked]
    if len(beam) > 1 and _lse(beam[0][1], beam[0][2]) != NEG_INF:
        gap = min(gap, _lse(beam[0][1], beam[0][2]) - _lse(beam[1][1], beam[1][2]))
    best = beam[0]
    return best[0], -_lse(best[1], best[2]), gap


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
