"""Helper of the MWER tests (not collected): the MWER objective over a GIVEN N-best list in fp64 -- loss and d(logits) twice, by
torch-CPU autograd through ``ctc_loss`` of ``log_softmax`` and in closed form from ``oracle.ctc_ref.ctc_loss_and_grad`` per hypothesis
with the coefficients of include/pgasr_hip.h (A13-MWER) --, the risks from ``oracle.decode_ref.edit_dist``, and a numpy statement of
``pgasr_mwer_weights`` term by term."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import ctc_ref, decode_ref, pg_ref


def risks(targets, tg_len, tokens, lengths, delimiter=None):
    """dist (N,B) int64 and risk_len (B) int64: the edit distance of every list row (rows beyond count are empty rows) to its target
    and the target's length -- over characters, or over the words str.split(" ") cuts at ``delimiter``."""
    N, B = lengths.shape
    dist, risk_len = np.zeros((N, B), dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        ref = [int(x) for x in targets[b][:int(tg_len[b])]]
        if delimiter is not None:
            ref = pg_ref.split_words(ref, delimiter)
        risk_len[b] = len(ref)
        for n in range(N):
            hyp = [int(x) for x in tokens[n, b][:int(lengths[n, b])]]
            if delimiter is not None:
                hyp = pg_ref.split_words(hyp, delimiter)
            dist[n, b] = decode_ref.edit_dist(ref, hyp)[0]
    return dist, risk_len


def weights_ref(dist, risk_len, tg_len, hyp_nll, hyp_len, count, nll, Lh, lam, inv_gb):
    """pgasr_mwer_weights in numpy fp64, term by term: valid, m, p, r, rbar, coef, utt_scale, terms."""
    hyp_nll = np.asarray(hyp_nll, dtype=np.float64)
    N, B = hyp_nll.shape
    valid = (np.arange(N)[:, None] < np.asarray(count)[None, :]) & (np.asarray(hyp_len) <= Lh) & np.isfinite(hyp_nll)
    p, rbar = np.zeros((N, B)), np.zeros(B)
    r = np.asarray(dist, dtype=np.float64) / np.maximum(np.asarray(risk_len, dtype=np.float64), 1.0)[None, :]
    for b in range(B):
        v = valid[:, b]
        if v.any():
            m = hyp_nll[v, b].min()
            e = np.where(v, np.exp(-(np.where(v, hyp_nll[:, b], m) - m)), 0.0)
            p[:, b] = e / e.sum()
        rbar[b] = (p[:, b] * r[:, b]).sum()
    coef = np.where(valid, -lam * inv_gb * p * (r - rbar[None, :]), 0.0)
    utt_scale = inv_gb / np.maximum(np.asarray(tg_len, dtype=np.float64), 1.0)
    with np.errstate(invalid="ignore"):
        terms = np.asarray(nll, dtype=np.float64) * utt_scale + lam * inv_gb * rbar
    return SimpleNamespace(valid=valid, p=p, r=r, rbar=rbar, coef=coef, utt_scale=utt_scale, terms=terms)


def hyp_nlls(logits, in_len, tokens, lengths, count, Lh, blank=0):
    """(hyp_nll (N,B), per-hypothesis gradients (N,T,B,V), lat_len (N,B)): the exact CTC nll and d nll / d logits of every list row;
    a row over the cap or beyond count is scored as the EMPTY hypothesis (what the host layer hands the lattice kernel)."""
    N, B = lengths.shape
    lat_len = np.where((np.asarray(lengths) > Lh) | (np.arange(N)[:, None] >= np.asarray(count)[None, :]), 0, lengths)
    nll, grads = np.zeros((N, B)), []
    for n in range(N):
        L = max(int(lat_len[n].max()), 1)
        nll[n], g = ctc_ref.ctc_loss_and_grad(logits, np.asarray(tokens[n])[:, :L], in_len, lat_len[n], blank=blank)
        grads.append(g)
    return nll, np.stack(grads), lat_len


def mwer_closed_form(logits, in_len, targets, tg_len, tokens, lengths, count, Lh, lam, global_batch, dist, risk_len, blank=0):
    """The objective and d(logits) from the per-hypothesis CTC gradients and the coefficients: loss, grad (T,B,V), w (weights_ref)."""
    logits = np.asarray(logits, dtype=np.float64)
    inv_gb = 1.0 / float(global_batch)
    nll, g_ctc = ctc_ref.ctc_loss_and_grad(logits, targets, in_len, tg_len, blank=blank)
    hn, hg, _ = hyp_nlls(logits, in_len, tokens, lengths, count, Lh, blank)
    w = weights_ref(dist, risk_len, tg_len, hn, lengths, count, nll, Lh, lam, inv_gb)
    grad = g_ctc * w.utt_scale[None, :, None]
    for n in range(lengths.shape[0]):
        grad = grad + hg[n] * w.coef[n][None, :, None]
    return SimpleNamespace(loss=float(w.terms.sum()), grad=grad, w=w, nll=nll, hyp_nll=hn)


def mwer_autograd(logits, in_len, targets, tg_len, tokens, lengths, count, Lh, lam, global_batch, dist, risk_len, blank=0):
    """The same by torch-CPU autograd through ctc_loss of log_softmax (fp64): loss, grad (T,B,V).  Utterances need frames."""
    import torch.nn.functional as F
    lg = torch.as_tensor(np.asarray(logits, dtype=np.float64)).clone().requires_grad_(True)
    lp = torch.log_softmax(lg, dim=2)
    N, B = lengths.shape
    il, tl = torch.as_tensor(np.asarray(in_len)).long(), torch.as_tensor(np.asarray(tg_len)).long()
    inv_gb = 1.0 / float(global_batch)
    nll = F.ctc_loss(lp, torch.as_tensor(np.asarray(targets)).long(), il, tl, blank=blank, reduction="none", zero_infinity=False)
    loss = (nll * inv_gb / tl.clamp(min=1).double()).sum()
    r = torch.as_tensor(np.asarray(dist, dtype=np.float64) / np.maximum(np.asarray(risk_len, dtype=np.float64), 1.0)[None, :])
    for b in range(B):
        rows = [n for n in range(N) if n < int(count[b]) and int(lengths[n, b]) <= Lh]
        nl = []
        for n in rows:
            L = int(lengths[n, b])
            tk = torch.as_tensor(np.asarray(tokens[n, b][:max(L, 1)])).long().view(1, -1)
            nl.append(F.ctc_loss(lp[:, b:b + 1], tk, il[b:b + 1], torch.tensor([L]), blank=blank, reduction="none", zero_infinity=False)[0])
        keep = [i for i, x in enumerate(nl) if bool(torch.isfinite(x))]
        if not keep:
            continue
        post = torch.softmax(-torch.stack([nl[i] for i in keep]), dim=0)
        loss = loss + lam * inv_gb * (post * r[[rows[i] for i in keep], b]).sum()
    loss.backward()
    g = lg.grad.numpy().copy()
    for b in range(B):
        g[int(in_len[b]):, b] = 0.0
    return float(loss.detach()), g
