"""The policy-gradient objective of loss.PGCTCLossFn, stated once in numpy float64 (TEST INFRASTRUCTURE ONLY -- see
oracle/__init__.py).  Built on ctc_ref and decode_ref; no torch, no GPU.  tests/test_pg_ref_cpu.py holds it to torch autograd.

With Bg the global batch, K samples per utterance, L_b the target's character count and T_b the utterance's frames:
    pi_k[t,b]   ~ softmax(logits[t,b]) by inverse CDF on Philox word 0 of counter (t*Bg + id_b, offset, 0, k)   (sample_paths)
    R[k,b]      = -ED(y_b, collapse(pi_k[:T_b,b])) / max(L_b,1), or -WED / W(y_b) over the split_words lists (reward_unit="word")
    b[k,b]      = the same reward of the hypothesis -- greedy arg-max collapse, or prefix beam search of width ``beam`` with adjacent
                  repeats removed -- ("hypothesis"), or (S_b - R[k,b]) / (K-1) with S_b = sum_j R[j,b] ("leave_one_out")
    coef[k,b]   = lam (R - b) / (Bg K);   per_step (K = 1): coef[t,b] = lam (G_s(t) - G_g(t)) / (max(L_b,1) Bg), the rewards-to-go
                  of the sampled and the greedy frame path (decode_ref.reward_to_go)
    loss        = sum_b nll_b / (Bg max(L_b,1))                       an infeasible target (nll = +inf) adds 0
                  - sum_k sum_b coef[k,b] sum_{t<T_b} log p(pi_k[t,b])                                    score_function="path"
                  + sum_k sum_b coef[k,b] nll(y_k,b | x_b)   where |y_k,b| <= Lh = min(T, 1023, max_hyp_len); the path term above
                                                              for the longer hypotheses                  score_function="sequence"
                  - sum_b beta / (Bg max(T_b,1)) sum_{t<T_b} H[t,b]                                       entropy_weight = beta
    grad        = d loss / d logits with coef, paths and hypotheses held constant.

The entropy term, with log-probs lp (T,B,V), weight beta and inv_gb = 1 / global batch:
    H[t,b]        = -sum_v p_v ln p_v,  p = exp(lp[t,b]),  0 ln 0 := 0                      (nats)
    ent_mean[b]   = (1 / max(T_b,1)) sum_{t<T_b} H[t,b]
    ent_scale[b]  = beta * inv_gb / max(T_b,1)
    loss term     = -sum_b ent_scale[b] sum_{t<T_b} H[t,b]  =  -sum_b beta inv_gb ent_mean[b]
    d/d(logits)   = ent_scale[b] p_v (ln p_v + H[t,b])     for t < T_b, 0 beyond
(d(-H)/dz_u = sum_v (ln p_v + 1) p_v (delta_uv - p_u) = p_u ln p_u + p_u H.)"""
from types import SimpleNamespace

import numpy as np

from . import ctc_ref, decode_ref


# ---- the sampler ----
def sampler_uniforms(T, ids, K, seed, offset, stride):
    """u[k,t,b]: Philox word 0 of counter (t*stride + ids[b], offset, 0, k), key (seed_lo, seed_hi), 24 high bits * 2^-24."""
    ids = np.asarray(ids, dtype=np.uint64)
    t, i = np.meshgrid(np.arange(T, dtype=np.uint64), ids, indexing="ij")
    c0 = ((t * np.uint64(stride) + i) & np.uint64(0xFFFFFFFF)).astype(np.uint32).ravel()
    c1 = np.full(c0.size, offset & 0xFFFFFFFF, dtype=np.uint32)
    z = np.zeros(c0.size, dtype=np.uint32)
    u = np.empty((K, T, ids.size))
    for k in range(K):
        x0, _, _, _ = decode_ref.philox4x32_10(c0, c1, z, np.full(c0.size, k, dtype=np.uint32), seed & 0xFFFFFFFF,
                                               (seed >> 32) & 0xFFFFFFFF)
        u[k] = ((x0 >> np.uint32(8)).astype(np.float64) * (1.0 / 16777216.0)).reshape(T, ids.size)
    return u


def sample_paths(logits, K, seed, offset, ids=None, stride=None):
    """decode_ref.sample_paths with K draws per frame, column b addressed as utterance ids[b] (default b) of a global batch of
    ``stride`` (default B): (paths (K,T,B), cdf (T,B,V), u (K,T,B))."""
    logits = np.asarray(logits, dtype=np.float64)
    T, B, V = logits.shape
    e = np.exp(logits - logits.max(axis=2, keepdims=True))
    cdf = np.cumsum(e, axis=2) / e.sum(axis=2, keepdims=True)
    u = sampler_uniforms(T, np.arange(B) if ids is None else ids, K, seed, offset, B if stride is None else stride)
    paths = np.minimum((cdf[None] <= u[..., None]).sum(axis=3), V - 1)
    return paths.astype(np.int64), cdf, u


# ---- the word reward ----
def split_words(seq, delimiter):
    """str.split(" ") on a token row: n delimiters give n + 1 words, empty words kept."""
    words, cur = [], []
    for t in seq:
        if int(t) == delimiter:
            words.append(tuple(cur)); cur = []
        else:
            cur.append(int(t))
    words.append(tuple(cur))
    return words


# ---- the entropy term ----
def _p_lnp(lp):
    lp = np.asarray(lp, dtype=np.float64)
    p = np.exp(lp)
    with np.errstate(invalid="ignore"):
        plp = np.where(p > 0, p * np.where(p > 0, lp, 0.0), 0.0)
    return p, plp


def row_entropy(lp):
    """H (T,B) of log-probs (T,B,V)."""
    return -_p_lnp(lp)[1].sum(axis=2)


def frame_mask(T, in_len):
    tb = np.clip(np.asarray(in_len, dtype=np.int64), 0, T)
    return np.arange(T)[:, None] < tb[None, :], tb


def entropy_stats(lp, in_len, beta=0.0, inv_gb=1.0):
    """(ent_mean (B), ent_scale (B))."""
    mask, tb = frame_mask(lp.shape[0], in_len)
    n = np.maximum(tb, 1).astype(np.float64)
    return (row_entropy(lp) * mask).sum(axis=0) / n, beta * inv_gb / n


def entropy_loss(lp, in_len, beta, inv_gb):
    """The term the objective gains: -sum_b beta inv_gb ent_mean[b]."""
    return -(beta * inv_gb * entropy_stats(lp, in_len)[0]).sum()


def entropy_grad(lp, in_len, ent_scale):
    """(T,B,V): ent_scale[b] p (ln p + H) on the utterance's own frames, 0 beyond."""
    p, plp = _p_lnp(lp)
    H = -plp.sum(axis=2)
    mask, _ = frame_mask(lp.shape[0], in_len)
    return (plp + p * H[..., None]) * np.asarray(ent_scale, dtype=np.float64)[None, :, None] * mask[..., None]


# ---- the objective ----
def score_terms(logits, in_len, paths, coef, score_function="path", max_hyp_len=None, blank=0):
    """The K score-function terms for given paths (K,T,B) and coefficients (K,B): (loss, grad (T,B,V), hyps [k][b] -- the paths'
    collapsed hypotheses --, scored (K,B) bool -- which samples took the sequence term), summed in k order."""
    logits = np.asarray(logits, dtype=np.float64)
    T, B, V = logits.shape
    paths, in_len = np.asarray(paths, dtype=np.int64), np.asarray(in_len)
    K = paths.shape[0]
    lp = ctc_ref.log_softmax(logits, axis=2)
    mask = np.arange(T)[:, None] < in_len[None, :]
    hyps = [[decode_ref.collapse_path(paths[k, :in_len[b], b], blank) for b in range(B)] for k in range(K)]
    scored = np.zeros((K, B), dtype=bool)
    loss, grad = 0.0, np.zeros((T, B, V))
    for k in range(K):
        lps = (np.take_along_axis(lp, paths[k][..., None], axis=2)[..., 0] * mask).sum(axis=0)
        if score_function == "sequence":
            hl = np.array([len(h) for h in hyps[k]])
            scored[k] = hl <= min(T, 1023, T if max_hyp_len is None else max_hyp_len)
            ht = np.zeros((B, T), dtype=np.int64)
            for b in range(B):
                ht[b, :hl[b]] = hyps[k][b]
            nll_h, g_h = ctc_ref.ctc_loss_and_grad(logits, ht, in_len, np.where(scored[k], hl, 0), blank)
            loss += (coef[k] * np.where(scored[k], nll_h, -lps)).sum()
            grad = grad + g_h * (coef[k] * scored[k])[None, :, None]
        else:
            loss -= (coef[k] * lps).sum()
        if not scored[k].all():
            grad = grad + decode_ref.reinforce_grad(logits, paths[k], coef[k] * ~scored[k], in_len)
    return loss, grad, hyps, scored


def pg_objective(logits, in_len, targets, tg_len, *, lam=1.0, seed=0, offset=0, global_batch=None, ids=None, num_samples=1,
                 baseline="hypothesis", beam=0, blank=0, per_step=False, reward_unit="char", word_delimiter=None,
                 score_function="path", max_hyp_len=None, entropy_weight=0.0, paths=None, greedy_frames=None, hypotheses=None):
    """The module docstring's objective on logits (T,B,V).  Overrides, for a caller that shares the device's discrete choices:
    ``paths`` (K,T,B) or (T,B) and ``greedy_frames`` (T,B) are frame labels, ``hypotheses`` the collapsed baseline hypothesis per
    utterance.  Returns a namespace: loss, grad (T,B,V), nll (B), R (K,B), R_hyp (B; None with leave_one_out), baselines (K,B),
    coef ((K,B); (T,B) with per_step), paths (K,T,B), hyps [k][b] (the samples' collapsed hypotheses), scored (K,B) bool (which
    samples took the sequence term), ent_mean (B)."""
    logits = np.asarray(logits, dtype=np.float64)
    T, B, V = logits.shape
    K, Bg = num_samples, global_batch or B
    in_len, tg_len = np.asarray(in_len), np.asarray(tg_len)
    lp = ctc_ref.log_softmax(logits, axis=2)
    paths = sample_paths(logits, K, seed, offset, ids, Bg)[0] if paths is None else np.asarray(paths, dtype=np.int64).reshape(K, T, B)
    if greedy_frames is None:
        greedy_frames = np.argmax(logits, axis=2)
    Lf = np.maximum(tg_len, 1).astype(np.float64)

    def reward(y, hyp, b):
        if reward_unit == "word":
            wy = split_words(y, word_delimiter)
            return -decode_ref.edit_dist(wy, split_words(hyp, word_delimiter))[0] / len(wy)
        return -decode_ref.edit_dist(y, hyp)[0] / Lf[b]

    ys = [[int(t) for t in targets[b][:tg_len[b]]] for b in range(B)]
    R = np.array([[reward(ys[b], decode_ref.collapse_path(paths[k, :in_len[b], b], blank), b) for b in range(B)] for k in range(K)])
    R_hyp = None
    if baseline == "hypothesis":
        R_hyp = np.zeros(B)
        for b in range(B):
            if hypotheses is not None:
                hyp = hypotheses[b]
            elif beam:      # the reference's reward hypothesis (policy_grad.py:6-8): prefix beam search -> collapse_fn
                hyp, _ = decode_ref.prefix_beam_search(np.exp(lp[:in_len[b], b]), beam_size=beam, blank=blank)
                hyp = [h for i, h in enumerate(hyp) if i == 0 or h != hyp[i - 1]]
            else:
                hyp = decode_ref.collapse_path(greedy_frames[:in_len[b], b], blank)
            R_hyp[b] = reward(ys[b], [int(t) for t in hyp], b)
        bk = np.broadcast_to(R_hyp, R.shape)
    else:
        bk = (R.sum(axis=0, keepdims=True) - R) / (K - 1)
    coef = lam * (R - bk) / (Bg * K)

    nll, g_ctc = ctc_ref.ctc_loss_and_grad(logits, targets, in_len, tg_len, blank)
    scale = 1.0 / (Lf * Bg)
    loss = (np.where(np.isfinite(nll), nll, 0.0) * scale).sum()
    grad = g_ctc * scale[None, :, None]
    if per_step:
        coef = np.zeros((T, B))
        for b in range(B):
            Gs, _, _ = decode_ref.reward_to_go(paths[0, :in_len[b], b], ys[b], blank)
            Gg, _, _ = decode_ref.reward_to_go(greedy_frames[:in_len[b], b], ys[b], blank)
            coef[:in_len[b], b] = lam * (Gs - Gg) / (max(int(tg_len[b]), 1) * Bg)
        loss -= (coef * np.take_along_axis(lp, paths[0][..., None], axis=2)[..., 0]).sum()
        grad = grad + decode_ref.reinforce_grad(logits, paths[0], coef, in_len)
    # per_step: the frame-level term above is the score term; zero coefficients here leave hyps and scored only
    s_loss, s_grad, hyps, scored = score_terms(logits, in_len, paths, np.zeros((K, B)) if per_step else coef, score_function,
                                               max_hyp_len, blank)
    loss, grad = loss + s_loss, grad + s_grad
    ent_mean, ent_scale = entropy_stats(lp, in_len, entropy_weight, 1.0 / Bg)
    if entropy_weight:
        loss += entropy_loss(lp, in_len, entropy_weight, 1.0 / Bg)
        grad = grad + entropy_grad(lp, in_len, ent_scale)
    return SimpleNamespace(loss=loss, grad=grad, nll=nll, R=R, R_hyp=R_hyp, baselines=bk, coef=coef, paths=paths, hyps=hyps,
                           scored=scored, ent_mean=ent_mean)
