"""Helper of the KL-penalty tests (not collected): the fp64 statement of the term of include/pgasr_hip.h (A12, KL penalty) in numpy --
per-frame KL(p || q) of a policy's log-probs against a frozen reference's, floored at PGASR_KL_LOG_FLOOR, the per-utterance mean
and scale, the value the objective gains and its derivative with respect to the logits."""
import numpy as np

from oracle import pg_ref

LOG_FLOOR = -104.0           # PGASR_KL_LOG_FLOOR: just under ln 2^-149


def _terms(lp, ref_lp):
    """(p, d) with d = p (ln p - lnq), exactly 0 where p = 0 (no 0 * inf); lnq = max(ref_lp, LOG_FLOOR)."""
    lp = np.asarray(lp, dtype=np.float64)
    lq = np.maximum(np.asarray(ref_lp, dtype=np.float64), LOG_FLOOR)
    p = np.exp(lp)
    live = p > 0
    d = np.where(live, p * (np.where(live, lp, 0.0) - lq), 0.0)
    return p, d


def row_kl(lp, ref_lp):
    """KL (T,B) of log-probs (T,B,V) from the reference's (T,B,V), nats."""
    return _terms(lp, ref_lp)[1].sum(axis=2)


def kl_stats(lp, ref_lp, in_len, gamma=0.0, inv_gb=1.0):
    """(kl_mean (B), kl_scale (B)): the mean over the utterance's own frames (0 for an empty one, not clamped) and
    gamma * inv_gb / max(T_b,1)."""
    mask, tb = pg_ref.frame_mask(np.asarray(lp).shape[0], in_len)
    n = np.maximum(tb, 1).astype(np.float64)
    return (row_kl(lp, ref_lp) * mask).sum(axis=0) / n, gamma * inv_gb / n


def kl_loss(lp, ref_lp, in_len, gamma, inv_gb):
    """The term the objective gains: sum_b gamma inv_gb kl_mean[b]."""
    return (gamma * inv_gb * kl_stats(lp, ref_lp, in_len)[0]).sum()


def kl_grad(lp, ref_lp, in_len, kl_scale):
    """(T,B,V): kl_scale[b] p (ln p - lnq - KL) on the utterance's own frames, 0 beyond."""
    p, d = _terms(lp, ref_lp)
    kl = d.sum(axis=2)
    mask, _ = pg_ref.frame_mask(p.shape[0], in_len)
    return (d - p * kl[..., None]) * np.asarray(kl_scale, dtype=np.float64)[None, :, None] * mask[..., None]
