"""CTC forced alignment (Viterbi) as a numpy fp64 statement -- what ``pgasr_ctc_forced_align`` must reproduce BIT FOR BIT -- and
a brute-force enumerator over all V^T frame paths for tiny cases.

States s = 0 .. 2L: even states are blank, state 2i+1 is token i; a label outside [0,V) is treated as blank.
    delta_0(0) = lp[0][blank], delta_0(1) = lp[0][tok_0], -inf elsewhere
    delta_t(s) = max(c0, c1, c2) + lp[t][label(s)];  c0 = delta_{t-1}(s) (stay), c1 = delta_{t-1}(s-1) (step),
                 c2 = delta_{t-1}(s-2) (skip) only for odd s >= 3 with tok[i] != tok[i-1]
    backpointer: the smallest move wins a tie -- 1 only if c1 > c0, 2 only if c2 > max(c0, c1)
    end state:   2L, unless L > 0 and delta(2L-1) > delta(2L)
Everything is max and add in fp64 on the fp32 inputs, vectorised over the states (no sum over states, so the order of the
vector operations cannot change a bit)."""
import itertools
from types import SimpleNamespace

import numpy as np


def align_one(lp, tokens, blank=0):
    """lp (T,V) float32 log-probs of one utterance (its real frames only), tokens a sequence of L labels.
    -> SimpleNamespace(score, frame_label (T), frame_token (T), token_start (L), token_end (L), token_logp (L))."""
    lp = np.asarray(lp, dtype=np.float32)
    T, V = lp.shape
    tok = np.asarray(tokens, dtype=np.int64).reshape(-1)
    L = len(tok)
    none = SimpleNamespace(score=np.inf, frame_label=np.full(T, -1, np.int32), frame_token=np.full(T, -1, np.int32),
                           token_start=np.full(L, -1, np.int32), token_end=np.full(L, -1, np.int32),
                           token_logp=np.zeros(L, np.float64))
    if T == 0:
        none.score = 0.0 if L == 0 else np.inf
        return none
    S = 2 * L + 1
    label = np.full(S, blank, np.int64)
    label[1::2] = np.where((tok >= 0) & (tok < V), tok, blank)
    skip = np.zeros(S, bool)
    if L > 1:
        skip[3::2] = tok[1:] != tok[:-1]
    lp64 = lp.astype(np.float64)
    delta = np.full(S, -np.inf)
    delta[0] = lp64[0, blank]
    if S > 1:
        delta[1] = lp64[0, label[1]]
    bp = np.zeros((T, S), np.int8)
    ninf = np.full(2, -np.inf)
    for t in range(1, T):
        c0 = delta
        c1 = np.concatenate([ninf[:1], delta[:-1]])
        c2 = np.where(skip, np.concatenate([ninf, delta[:-2]])[:S], -np.inf)
        m01 = np.where(c1 > c0, c1, c0)
        k = np.where(c1 > c0, 1, 0)
        m = np.where(c2 > m01, c2, m01)
        k = np.where(c2 > m01, 2, k)
        bp[t] = k
        delta = m + lp64[t, label]
    end = S - 1
    if S > 1 and delta[S - 2] > delta[S - 1]:
        end = S - 2
    if delta[end] == -np.inf:
        return none
    states = np.empty(T, np.int64)
    s = end
    for t in range(T - 1, -1, -1):
        states[t] = s
        if t > 0:
            s -= int(bp[t, s])
    odd = (states & 1) == 1
    ftok = np.where(odd, states >> 1, -1).astype(np.int32)
    out = SimpleNamespace(score=-delta[end], frame_label=label[states].astype(np.int32), frame_token=ftok,
                          token_start=np.full(L, -1, np.int32), token_end=np.full(L, -1, np.int32),
                          token_logp=np.zeros(L, np.float64))
    for i in range(L):
        fr = np.nonzero(ftok == i)[0]
        out.token_start[i], out.token_end[i] = fr[0], fr[-1] + 1
        acc = np.float64(0.0)
        for t in fr:                               # ascending t
            acc = acc + lp64[t, label[2 * i + 1]]
        out.token_logp[i] = acc
    return out


def align_batch(log_probs, tokens, input_lengths, token_lengths, blank=0):
    """The padded batch form of the entry point: log_probs (T,B,V) float32, tokens (B,Lmax), lengths (B) (clamped like the device
    clamps them) -> SimpleNamespace of score (B) f64, frame_label / frame_token (B,T) i32 (-1 padded), token_start / token_end
    (B,Lmax) i32 (-1 padded), token_logp (B,Lmax) f64 (0 padded)."""
    log_probs = np.asarray(log_probs, dtype=np.float32)
    tokens = np.asarray(tokens)
    T, B, V = log_probs.shape
    Lmax = tokens.shape[1]
    out = SimpleNamespace(score=np.zeros(B, np.float64), frame_label=np.full((B, T), -1, np.int32),
                          frame_token=np.full((B, T), -1, np.int32), token_start=np.full((B, Lmax), -1, np.int32),
                          token_end=np.full((B, Lmax), -1, np.int32), token_logp=np.zeros((B, Lmax), np.float64))
    for b in range(B):
        Tb = min(max(int(input_lengths[b]), 0), T)
        Lb = min(max(int(token_lengths[b]), 0), Lmax)
        r = align_one(log_probs[:Tb, b], tokens[b, :Lb], blank)
        out.score[b] = r.score
        out.frame_label[b, :Tb], out.frame_token[b, :Tb] = r.frame_label, r.frame_token
        out.token_start[b, :Lb], out.token_end[b, :Lb], out.token_logp[b, :Lb] = r.token_start, r.token_end, r.token_logp
    return out


def collapse(path, blank=0):
    out, prev = [], None
    for k in path:
        if k != prev and k != blank:
            out.append(int(k))
        prev = k
    return out


def brute_force_score(lp, tokens, blank=0):
    """min over all V^T frame paths that collapse to ``tokens`` of -sum_t lp[t][path_t] (fp64); +inf when there is none."""
    lp64 = np.asarray(lp, dtype=np.float32).astype(np.float64)
    T, V = lp64.shape
    want = [int(k) for k in tokens]
    best = np.inf
    if T == 0:
        return 0.0 if not want else np.inf
    for path in itertools.product(range(V), repeat=T):
        if collapse(path, blank) == want:
            best = min(best, -sum(lp64[t, k] for t, k in enumerate(path)))
    return best
