"""Helper of the unit-LM tests (not collected): a plain-dict statement of the back-off query and of ``logp_sequence`` written
without a look at policy_gradient_asr_amd/lm.py, a sparse random model, the fused prefix beam search in its two forms, and the
shared GPU cases with their inputs and reference lists.

The model as a dict: {k-gram tuple: (logp, bow)} with fp32 values held as Python floats; the key (blank,) is <s>: its logp is never
read, its bow is the back-off weight of the start context.  The query, as include/pgasr_hip.h (A7-WIDE-LM) states it: acc = 0.0 in
fp64, h = the last order-1 symbols of (blank,) + prefix; if h + (s,) is stored return float32(acc + logp); else acc += bow[h] where
h is stored, drop the oldest symbol of h, again."""
import functools

import numpy as np

import beam_lm_ref as R
import beam_wide_cases as W
import nbest_ref as NR

GAP_MIN = R.GAP_MIN
DENSE_MAX = 1 << 25


def context_of(prefix, order, blank):
    h = (blank,) + tuple(int(x) for x in prefix)
    return h[max(0, len(h) - (order - 1)):] if order > 1 else ()


def query(d, order, blank, prefix, s):
    """float32(ln p(s | prefix)) as a Python float, by the rule above."""
    h, acc = context_of(prefix, order, blank), 0.0
    while True:
        e = d.get(h + (s,))
        if e is not None:
            return float(np.float32(acc + e[0]))
        c = d.get(h) if h else None
        if c is not None:
            acc = acc + c[1]
        h = h[1:]


def sequence(d, order, blank, tokens):
    """The fp64 sum in index order of the fp32 queries; no end-of-sentence term."""
    y, total = [int(t) for t in tokens], 0.0
    for i, s in enumerate(y):
        total = total + query(d, order, blank, y[:i], s)
    return total


def _f32(x):
    return float(np.float32(x))


def random_unit_lm(V, order, blank, seed, n_ctx=40, n_succ=6, scale=2.0):
    """(dict, lm.UnitNgramLM) of a sparse random model, not normalised (like beam_lm_ref.random_table: ranking decisions are then rich).
    Unigrams: a log-softmax over the non-blank symbols of scale * N(0,1).  Per order k = 2 .. n: ``n_ctx`` of the stored (k-1)-grams
    become contexts (at k = 2 the start context (blank,) among them, at k = 3 every stored (blank, a)), each with ``n_succ`` random
    successors of logp N(-3, 1.5); every stored k-gram below the top order has a bow in [-1.5, 0) -- so most stored contexts have a
    bow and no successor of their own, there are hits and contexts at every level, and nearly every n-gram is absent at every
    level down to the unigram."""
    from policy_gradient_asr_amd.lm import UnitNgramLM
    rng = np.random.default_rng(seed)
    syms = [s for s in range(V) if s != blank]
    z = rng.standard_normal(V) * scale
    z[blank] = -np.inf
    uni = z - (z.max() + np.log(np.exp(z - z.max()).sum()))
    grams = [{}]
    for s in syms:
        grams[0][(s,)] = (_f32(uni[s]), _f32(-rng.uniform(0.01, 1.5)) if order > 1 else 0.0)
    grams[0][(blank,)] = (_f32(-99.0 * np.log(10.0)), _f32(-rng.uniform(0.01, 1.5)) if order > 1 else 0.0)
    for k in range(2, order + 1):
        prev = sorted(grams[k - 2])
        forced = [g for g in prev if g[0] == blank] if k <= 3 else []
        rest = [g for g in prev if g not in set(forced)]
        pick = [rest[i] for i in rng.permutation(len(rest))[:max(0, n_ctx - len(forced))]]
        cur = {}
        for h in forced[:n_ctx] + pick:
            for s in rng.choice(syms, size=min(n_succ, len(syms)), replace=False):
                cur[h + (int(s),)] = (_f32(rng.normal(-3.0, 1.5)), _f32(-rng.uniform(0.01, 1.5)) if k < order else 0.0)
        grams.append(cur)
    ngrams, logp, bow = [], [], []
    for k in range(1, order + 1):
        keys = sorted(grams[k - 1])
        ngrams.append(np.array(keys, dtype=np.int32).reshape(-1, k))
        logp.append(np.array([grams[k - 1][g][0] for g in keys], dtype=np.float32))
        bow.append(np.array([grams[k - 1][g][1] for g in keys], dtype=np.float32))
    d = {}
    for g in grams:
        d.update(g)
    return d, UnitNgramLM(ngrams, logp, bow, V, blank=blank)


def callable_search(logp, bonus, beam_size, blank, nbest):
    """nbest_ref.nbest_prefix_beam_search with ``bonus(prefix, s)`` in place of the table lookup: V = 1024 at order 3 has no dense
    table.  Returns (hyps, gap) as it does."""
    return NR.nbest_prefix_beam_search(logp=logp, bonus=bonus, beam_size=beam_size, blank=blank, nbest=nbest)


def dict_bonus(d, order, blank, alpha, beta):
    """bonus(prefix, s) = alpha * query + beta over the dict statement, each product and sum rounded once; memoised per context."""
    memo = {}
    alpha, beta = float(alpha), float(beta)

    def bonus(prefix, s):
        key = (context_of(prefix, order, blank), s)
        w = memo.get(key)
        if w is None:
            w = memo[key] = alpha * query(d, order, blank, key[0], s) + beta
        return w
    return bonus


def fused_search(d, model, logp, alpha, beta, beam_size, blank, nbest, form=None):
    """The fused search of one utterance: over the dense table of ``model.to_dense()`` through the existing oracle where V**order <=
    2**25 (form "dense"), else the same loop with the dict statement as its bonus (form "callable"); ``form`` forces one."""
    V, order = model.vocab, model.order
    if form is None:
        form = "dense" if V ** order <= DENSE_MAX else "callable"
    if form == "dense":
        return NR.nbest_prefix_beam_search(logp=logp, table=_dense(model), order=order, alpha=alpha, beta=beta, beam_size=beam_size,
                                           blank=blank, nbest=nbest)
    return callable_search(logp, dict_bonus(d, order, blank, alpha, beta), beam_size, blank, nbest)


_DENSE = {}


def _dense(model):
    t = _DENSE.get(id(model))
    if t is None:
        t = _DENSE[id(model)] = (model, model.to_dense().table)
    return t[1]


# ---- the GPU cases: (T, V, beam, order, blank, B, alpha, beta, kind, seed).  kind "mixed": the recipe of beam_wide_cases.case_inputs
# (per-frame scale from {0.3, 2.0, 5.0}, +1.5 on blank); "peaked": scale 5 in every frame, +1.5 on blank -- a few entries stay for many
# frames while the others churn, which is where an entry keeps its LM row; "flat": beam_wide_cases.select_inputs("flat") as they are,
# with lm_beta = 3.0 lifting extensions over stays, and lm_alpha = 0.2: the model's own spread, scaled by alpha, thins the list as
# peaked frames do -- at alpha = 0.5 the flat frames list at most 1700 of 16384 candidates and nothing overflows, at 0.2 over 5000.  seed: per case the first of 0, 1, 2, .. whose every utterance has a smallest
# decision margin >= GAP_MIN (tests/test_unit_lm_cpu.py asserts it); the model is random_unit_lm(V, order, blank, seed + 17).
CASES = [
    (40, 65, 16, 3, 32, 5, 0.8, 0.5, "mixed", 0),
    (30, 128, 1, 2, 0, 5, 0.5, 0.0, "mixed", 0),
    (20, 129, 128, 3, 64, 4, 1.0, 1.2, "mixed", 0),
    (40, 300, 5, 5, 299, 5, 0.8, 0.5, "peaked", 0),
    (24, 1000, 32, 1, 7, 3, 0.5, 0.0, "mixed", 0),
    (24, 1024, 16, 3, 0, 3, 1.0, 1.2, "mixed", 1),
    (6, 1024, 128, 4, 512, 3, 0.8, 0.5, "mixed", 0),
    (W.FLAT[0], W.SELECT_V, W.SELECT_BEAM, 3, W.SELECT_BLANK, W.FLAT[1], 0.2, 3.0, "flat", 2),
]


def case_id(case):
    return "T%d-V%d-K%d-n%d-b%d-B%d-a%g-c%g-%s-s%d" % case


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(log-probs (T,B,V) fp32, lengths (B) int32 with a 1 and a 0 among them -- all T for the flat case, as its source has them)."""
    T, V, beam, order, blank, B, alpha, beta, kind, seed = case
    if kind == "flat":
        return W.select_inputs("flat")
    rng = np.random.default_rng(1000003 * seed + 1009 * T + 31 * V + beam + 7 * order)
    if kind == "peaked":
        logits = rng.normal(size=(T, B, V)) * 5.0
    else:
        logits = rng.normal(size=(T, B, V)) * rng.choice([0.3, 2.0, 5.0], size=(T, B, 1))
    logits[:, :, blank] += 1.5
    lp = R.log_softmax32(logits)
    lp.setflags(write=False)
    return lp, W.lengths_of(T, B)


@functools.lru_cache(maxsize=None)
def case_model(case):
    T, V, beam, order, blank, B, alpha, beta, kind, seed = case
    return random_unit_lm(V, order, blank, seed + 17)


def list_size(beam):
    return NR.list_size(beam)


@functools.lru_cache(maxsize=None)
def reference(case, form=None):
    """Per utterance (hyps, gap) at N = list_size(beam), computed once per process."""
    T, V, beam, order, blank, B, alpha, beta, kind, seed = case
    lp, lens = case_inputs(case)
    d, model = case_model(case)
    out = []
    for b in range(lp.shape[1]):
        n = int(lens[b])
        if n == 0:
            out.append(([((), -0.0)], float("inf")))
        else:
            out.append(fused_search(d, model, lp[:n, b].astype(np.float64), alpha, beta, beam, blank, list_size(beam), form=form))
    return tuple(out)
