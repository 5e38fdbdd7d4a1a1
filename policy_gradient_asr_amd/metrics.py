"""Drop-in for the reference's metrics.py (edit_dist, evaluate, save_predictions) on the HIP
Levenshtein kernel (csrc/editdist.hip)."""
import os

import torch

from . import hipops
from .CTCdecoder import _device


def _encode(seqs):
    """Map arbitrary hashable symbols (chars or word strings) to dense int32 ids >= 1."""
    table = {}
    out = []
    for s in seqs:
        ids = []
        for tok in s:
            if tok not in table:
                table[tok] = len(table) + 1
            ids.append(table[tok])
        out.append(ids)
    return out


def edit_dist_batch(refs, hyps, device=None):
    """Levenshtein distances of many (reference, hypothesis) pairs in one launch.
    refs/hyps: lists of sequences (str or list of tokens).  Returns a list of ints."""
    dev = _device(device)
    n = len(refs)
    enc = [_encode([r, h]) for r, h in zip(refs, hyps)]
    R = max(max((len(e[0]) for e in enc), default=0), 1)
    Hy = max(max((len(e[1]) for e in enc), default=0), 1)
    ref = torch.zeros(n, R, dtype=torch.int32); hyp = torch.zeros(n, Hy, dtype=torch.int32)
    rl = torch.zeros(n, dtype=torch.int32); hl = torch.zeros(n, dtype=torch.int32)
    for i, (r, h) in enumerate(enc):
        ref[i, :len(r)] = torch.tensor(r, dtype=torch.int32); hyp[i, :len(h)] = torch.tensor(h, dtype=torch.int32)
        rl[i], hl[i] = len(r), len(h)
    d = hipops.edit_distance(ref.to(dev), rl.to(dev), hyp.to(dev), hl.to(dev))
    return [int(x) for x in d.tolist()]


def edit_dist(s1, s2):
    """(distance, len(s1)) between reference s1 and prediction s2 (metrics.py:4-21); str for CER,
    list of words for WER."""
    return edit_dist_batch([s1], [s2])[0], len(s1)


def evaluate(s1, s2):
    """(CER, WER) (metrics.py:23-31).  Like the reference, divides by zero on an empty reference."""
    w1, w2 = s1.split(" "), s2.split(" ")
    d = edit_dist_batch([s1, w1], [s2, w2])
    cer = d[0] / len(s1)
    wer = d[1] / len(w1)
    return cer, wer


def edit_counts(targets, tg_len, tokens, tok_len, delimiter):
    """What ``evaluate`` computes for a whole batch of token rows, without the division and without a host round trip:
    targets (B,L) / tokens (B,T) int32 on the GPU with their lengths, words split at the token ``delimiter`` (the alphabet's " ").
    Returns (character distance, character length, word distance, word count), each (B,) int32 on the device; CER = cd / cl and
    WER = wd / wc as evaluate() gives them on the decoded strings."""
    cd = hipops.edit_distance(targets, tg_len, tokens, tok_len)
    wd, wc, _ = hipops.word_edit_distance(targets, tg_len, tokens, tok_len, delimiter)
    return cd, tg_len, wd, wc


def nbest_oracle(targets, tg_len, nb):
    """The best the list could have done: targets (B,L) / tg_len (B) int32 on the GPU, ``nb`` a ``hipops.CTCNBest``.
    Returns (min character edit distance over the utterance's count hypotheses (B) int32, the first rank that reaches it (B) int32),
    on the device without a host round trip: one ``hipops.edit_distance`` launch over the N * B (target, hypothesis) pairs.
    Oracle CER = distance / tg_len; a rank > 0 says the search had a better hypothesis than the one it ranked first."""
    N, B, T = nb.tokens.shape
    L = targets.shape[1]
    ref = targets.unsqueeze(0).expand(N, B, L).reshape(N * B, L).contiguous()
    ref_len = tg_len.unsqueeze(0).expand(N, B).reshape(N * B).contiguous()
    dist = hipops.edit_distance(ref, ref_len, nb.tokens.reshape(N * B, T), nb.lengths.reshape(N * B)).view(N, B)
    rows = torch.arange(N, dtype=torch.int32, device=dist.device).unsqueeze(1)
    dist = torch.where(rows < nb.count.unsqueeze(0), dist, torch.full_like(dist, torch.iinfo(torch.int32).max))
    best = dist.min(0).values
    rank = torch.where(dist == best.unsqueeze(0), rows.expand(N, B), torch.full_like(dist, N)).min(0).values
    return best, rank


def frame_entropy(log_probs, in_len):
    """Mean frame entropy of the policy per utterance: log_probs (T,B,V) fp32 log-softmax outputs and in_len (B) int32 on the GPU ->
    (B,) fp32 on the device, the mean over each utterance's own frames of H = -sum_v p ln p in nats (0 for an empty utterance;
    ln V for a uniform policy, 0 for a collapsed one).  The kernel of the trainer's ``entropy_weight`` term with weight 0
    (hipops.frame_entropy): lets ``predict`` or validation code watch for collapse without training.  No host round trip."""
    return hipops.frame_entropy(log_probs, in_len, 0.0, 1.0)[0]


def frame_kl(log_probs, ref_log_probs, in_len):
    """Mean frame KL(p || q) of the policy from a reference policy per utterance: log_probs and ref_log_probs (T,B,V) fp32 log-softmax
    outputs for the same batch and in_len (B) int32 on the GPU -> (B,) fp32 on the device, the mean over each utterance's own frames of
    sum_v p (ln p - max(ln q, -104)) in nats (0 for an empty utterance and where the two agree).  The kernel of the trainer's
    ``kl_weight`` term with weight 0 (hipops.frame_kl): how far a fine-tuned model has drifted from its start.  No host round trip."""
    return hipops.frame_kl(log_probs, ref_log_probs, in_len, 0.0, 1.0)[0]


def save_predictions(target, predicted, model_path):
    """predicted.txt with one 'target|prediction' line per utterance (metrics.py:33-37)."""
    path = os.path.join(model_path, "predicted.txt")
    with open(path, "w") as fo:
        for i in range(len(target)):
            fo.write(target[i] + "|" + predicted[i] + "\n")
