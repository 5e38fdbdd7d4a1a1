"""The entropy regularisation of the frame policy, stated in fp64 numpy (the reference of tests/test_entropy_gpu.py).

With log-probs lp (T,B,V), lengths T_b, weight beta and inv_gb = 1 / global batch:
    H[t,b]        = -sum_v p_v ln p_v,  p = exp(lp[t,b]),  0 ln 0 := 0                      (nats)
    ent_mean[b]   = (1 / max(T_b,1)) sum_{t<T_b} H[t,b]
    ent_scale[b]  = beta * inv_gb / max(T_b,1)
    loss term     = -sum_b ent_scale[b] sum_{t<T_b} H[t,b]  =  -sum_b beta inv_gb ent_mean[b]
    d/d(logits)   = ent_scale[b] p_v (ln p_v + H[t,b])     for t < T_b, 0 beyond
(d(-H)/dz_u = sum_v (ln p_v + 1) p_v (delta_uv - p_u) = p_u ln p_u + p_u H.)"""
import numpy as np


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
