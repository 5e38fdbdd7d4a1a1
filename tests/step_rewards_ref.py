"""Helper of the per-step multi-sample tests (not collected): the statement of include/pgasr_hip.h, A12-STEP, in numpy fp64 on
oracle/decode_ref.reward_to_go -- the per-frame coefficients of K sampled paths against the greedy path's or the other samples'
reward-to-go at the same frame, and the objective they enter (CTC and entropy parts from oracle/pg_ref.pg_objective with lam = 0,
the KL part from tests/kl_ref.py, the REINFORCE part from decode_ref.reinforce_grad per sample) -- and the constructed inputs the
GPU tests share."""
from types import SimpleNamespace

import numpy as np

from oracle import ctc_ref, decode_ref, pg_ref

import kl_ref


def rewards_to_go(rows, in_len, targets, tg_len, blank=0):
    """G (P,T,B) fp64 of frame-label rows (P,T,B): decode_ref.reward_to_go over each utterance's own frames, 0 beyond them."""
    rows = np.asarray(rows, dtype=np.int64)
    P, T, B = rows.shape
    G = np.zeros((P, T, B))
    for b in range(B):
        Tb = int(np.clip(in_len[b], 0, T))
        y = [int(v) for v in targets[b][:int(tg_len[b])]]
        for w in range(P):
            G[w, :Tb, b] = decode_ref.reward_to_go(rows[w, :Tb, b], y, blank)[0]
    return G


def step_coefs(paths, greedy_frames, in_len, targets, tg_len, baseline="hypothesis", lam=1.0, Bg=None, blank=0):
    """coef (K,T,B) fp64: kf_b (G_k(t) - G_greedy(t)) ("hypothesis") or kf_b (G_k(t) - (S(t) - G_k(t)) / (K-1)) ("leave_one_out") with
    kf_b = lam / (Bg K max(L_b,1)); 0 for t >= T_b.  paths (K,T,B); greedy_frames (T,B), read by "hypothesis" alone."""
    paths = np.asarray(paths, dtype=np.int64)
    K, T, B = paths.shape
    Bg = Bg or B
    G = rewards_to_go(paths, in_len, targets, tg_len, blank)
    if baseline == "hypothesis":
        base = np.broadcast_to(rewards_to_go(np.asarray(greedy_frames)[None], in_len, targets, tg_len, blank), G.shape)
    else:
        base = (G.sum(axis=0, keepdims=True) - G) / (K - 1)
    kf = lam / (Bg * K * np.maximum(np.asarray(tg_len), 1).astype(np.float64))
    mask = np.arange(T)[:, None] < np.clip(np.asarray(in_len), 0, T)[None, :]
    return kf[None, None, :] * (G - base) * mask[None]


def step_objective(logits, in_len, targets, tg_len, *, paths, greedy_frames=None, baseline="hypothesis", lam=1.0, global_batch=None,
                   blank=0, entropy_weight=0.0, kl_weight=0.0, ref_log_probs=None, coef=None):
    """The A12-STEP objective on logits (T,B,V) for given paths (K,T,B): namespace of loss, grad (T,B,V), coef (K,T,B), nll (B).
    coef: given coefficients instead of step_coefs' (the kernel tests of the gradient pass and the loss value)."""
    logits = np.asarray(logits, dtype=np.float64)
    T, B, V = logits.shape
    paths = np.asarray(paths, dtype=np.int64)
    K = paths.shape[0]
    Bg = global_batch or B
    in_len, tg_len = np.asarray(in_len), np.asarray(tg_len)
    if coef is None:
        coef = step_coefs(paths, greedy_frames, in_len, targets, tg_len, baseline, lam, Bg, blank)
    coef = np.asarray(coef, dtype=np.float64)
    # CTC and entropy: the one statement of them, with no REINFORCE term
    o = pg_ref.pg_objective(logits, in_len, targets, tg_len, lam=0.0, global_batch=Bg, blank=blank, entropy_weight=entropy_weight,
                            paths=paths[:1], greedy_frames=paths[0])
    loss, grad = o.loss, o.grad
    lp = ctc_ref.log_softmax(logits, axis=2)
    mask = np.arange(T)[:, None] < np.clip(in_len, 0, T)[None, :]
    for k in range(K):
        loss -= (coef[k] * np.take_along_axis(lp, paths[k][..., None], axis=2)[..., 0] * mask).sum()
        grad = grad + decode_ref.reinforce_grad(logits, paths[k], coef[k], np.clip(in_len, 0, T))
    if kl_weight:
        loss += kl_ref.kl_loss(lp, ref_log_probs, in_len, kl_weight, 1.0 / Bg)
        grad = grad + kl_ref.kl_grad(lp, ref_log_probs, in_len, kl_ref.kl_stats(lp, ref_log_probs, in_len, kl_weight, 1.0 / Bg)[1])
    return SimpleNamespace(loss=loss, grad=grad, coef=coef, nll=o.nll)


# ---- the constructed inputs of the GPU tests ----
COEF_T = (1, 63, 64, 65, 130, 257, 1030)     # 1030: above the 1024 frames a workgroup of pgasr_pg_step_coefs_multi covers in one pass
COEF_K = (1, 2, 3, 16)
COEF_B, COEF_V = 3, 5


def seam_case(T, K, blank, baseline, seed=0):
    """Frame paths over {blank, 1, 2, 3} for B = 3 utterances, built run by run (not sampled from a model): P rows -- the greedy row
    first with the hypothesis baseline --, runs of 1..3 frames, and around every 64-frame seam s a character that starts at s - 1 and
    another at s in every row.  in_len = (T, max(T - 5, 0), 0); targets of 7, 0 (the empty one) and 5 symbols."""
    rng = np.random.default_rng(1000 * T + 10 * K + seed + (1 if blank else 0) + (3 if baseline == "leave_one_out" else 0))
    B = COEF_B
    P = K + (1 if baseline == "hypothesis" else 0)
    rows = np.zeros((P, T, B), dtype=np.int64)
    for w in range(P):
        for b in range(B):
            t = 0
            while t < T:
                n = int(rng.integers(1, 4))
                rows[w, t:t + n, b] = int(rng.integers(0, 4))
                t += n
            for s in range(64, T, 64):
                a = int(rng.integers(1, 4))
                c = 1 + (a + int(rng.integers(0, 2))) % 3
                if s >= 2:
                    rows[w, s - 2, b] = 0
                rows[w, s - 1, b], rows[w, s, b] = a, c
    rows[rows == 0] = -1
    rows[rows == -1] = blank
    tg_len = np.array([7, 0, 5], dtype=np.int32)
    targets = np.zeros((B, 9), dtype=np.int32)
    for b in range(B):
        targets[b, :tg_len[b]] = rng.integers(1, 4, tg_len[b])
    in_len = np.array([T, max(T - 5, 0), 0], dtype=np.int32)
    greedy = rows[0] if baseline == "hypothesis" else None
    return SimpleNamespace(rows=rows.astype(np.int32), paths=rows[P - K:], greedy=greedy, in_len=in_len, targets=targets, tg_len=tg_len,
                           T=T, B=B, K=K, P=P, blank=blank, baseline=baseline)


def starts(row, Tb, blank):
    """Frames of a (T,) row at which a character starts."""
    return [t for t in range(Tb) if row[t] != blank and (t == 0 or row[t] != row[t - 1])]
