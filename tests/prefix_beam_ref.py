"""Helper of the decoder tests (not collected): the ONE plain-Python prefix beam search with a per-extension bonus, written against
oracle.decode_ref.  nbest_ref.nbest_prefix_beam_search is this function; beam_lm_ref.fused_prefix_beam_search (N = 1) and
unit_lm_ref.callable_search (a callable bonus) call it.

The search is ``decode_ref.prefix_beam_search`` with ONE change: every term that enters a prefix by an extension with a non-blank s
gets  w = bonus(prefix, s)  added -- (p_b + p) + w, (p_nb + p) + w.  The blank update and the repeat branch that keeps the prefix are
unchanged.  With a dense table, w = alpha * float(table[ctx(prefix), s]) + beta, ctx(prefix) = the last order-1 symbols of the
prefix, left-padded with blank; without table and bonus, w = 0.0."""
import numpy as np

from oracle.decode_ref import NEG_INF, _lse


def nbest_prefix_beam_search(probs=None, table=None, order=0, alpha=0.0, beta=0.0, beam_size=100, blank=0, logp=None, nbest=1,
                             last_touch=False, report=None, bonus=None):
    """probs (T,V) probabilities (their numpy log is taken, like decode_ref) or logp (T,V) log-probabilities.  table: None or an
    array of shape (V,)*order, weighted by alpha and beta; or bonus: a callable (prefix, s) -> float; not both.
    Returns (hyps, gap): hyps = [(prefix tuple, score)] for the first
    min(nbest, len(beam)) entries of the final beam -- the reference's sorted(...)[:N]: score descending, first touch among equals
    -- with score = -lse(p_b, p_nb); gap = the smallest margin of any ranking decision the list depends on: every frame's cut
    (the score of the last kept candidate minus the first dropped one) and every adjacent pair of final ranks (r, r + 1) for r < nbest,
    rank nbest-1 against rank nbest included where rank nbest exists.  inf if there was no such decision; pairs whose better
    entry has probability zero decide nothing (both are -inf: first touch ranks them).
    The two optional arguments serve tests/beam_tie_ref.py and leave everything above as it is when not given.  last_touch: equal
    scores are ranked LAST touch first in every frame -- the wrong rule, stated so that a test can show its inputs tell the two apart.
    report: a dict that receives, over the first min(len, beam_size + 1) ranks of every frame (the in-beam order sets the next frame's
    touch order, so every adjacent pair in it is a decision): "margin" = the smallest non-zero difference of two adjacent ranks (inf
    if none), "tied" = the number of adjacent pairs with exactly equal score, "cut_ties" = the number of frames whose cut (rank
    beam_size - 1 against rank beam_size) is such a pair, "frames" = per frame the tuple of kept prefixes.  The final beam is the last
    frame's kept ranks, so its pairs are among these."""
    if bonus is not None and table is not None:
        raise ValueError("a table or a bonus, not both")
    if report is not None:
        report.update(margin=float("inf"), tied=0, cut_ties=0, frames=[])
    if logp is None:
        with np.errstate(divide="ignore"):
            logp = np.log(probs)
    T, V = logp.shape
    alpha, beta = float(alpha), float(beta)

    def table_bonus(prefix, s):
        if table is None:
            return 0.0
        n1 = order - 1
        tail = prefix[-n1:] if n1 else ()
        ctx = (blank,) * (n1 - len(tail)) + tuple(tail)
        return alpha * float(table[ctx + (s,)]) + beta

    if bonus is None:
        bonus = table_bonus
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
        items = list(tab.items())
        ranked = sorted(items[::-1] if last_touch else items, key=lambda kv: _lse(kv[1][0], kv[1][1]), reverse=True)
        if len(ranked) > beam_size:
            kept, dropped = _lse(*ranked[beam_size - 1][1]), _lse(*ranked[beam_size][1])
            if kept != NEG_INF:
                gap = min(gap, kept - dropped)
        if report is not None:
            top = [_lse(*v) for _, v in ranked[:beam_size + 1]]
            for r in range(len(top) - 1):
                if top[r] == top[r + 1]:
                    report["tied"] += 1
                    report["cut_ties"] += r == beam_size - 1
                else:
                    report["margin"] = min(report["margin"], top[r] - top[r + 1])
            report["frames"].append(tuple(k for k, _ in ranked[:beam_size]))
        ranked = ranked[:beam_size]
        beam = [(k, v[0], v[1]) for k, v in ranked]
    sc = [_lse(b[1], b[2]) for b in beam]
    for r in range(min(nbest, len(beam))):
        if r + 1 < len(beam) and sc[r] != NEG_INF:
            gap = min(gap, sc[r] - sc[r + 1])
    return [(b[0], -s) for b, s in zip(beam[:nbest], sc)], gap
