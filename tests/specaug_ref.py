"""The SpecAugment masking function of include/pgasr_hip.h (A0-AUG) in plain numpy: a statement of the specification beside the
tests, not a test.  Every interval comes from one block of oracle.decode_ref.philox4x32_10.

policy: anything with the fields freq_masks, freq_width, time_masks, time_width, time_ratio, fill -- a features.SpecAugment, or a
dict of them (time_ratio None means 1.0)."""
import numpy as np

from oracle.decode_ref import philox4x32_10

DOM_FREQ, DOM_TIME = 2, 3           # Philox counter word 2; the samplers use 0 and 1 there
FIELDS = ("freq_masks", "freq_width", "time_masks", "time_width", "time_ratio", "fill")


def fields(policy):
    get = policy.get if isinstance(policy, dict) else lambda k, d=None: getattr(policy, k, d)
    nF, Wf, nT, Wt = (int(get(k)) for k in FIELDS[:4])
    p = get("time_ratio", 1.0)
    return nF, Wf, nT, Wt, np.float32(1.0 if p is None else p), get("fill", "row_mean")


def time_width_cap(Wt, p, length):
    """W of a time mask: min(Wt, len, (int)(fp32(p) * fp32(len))) -- one fp32 multiply, then truncation."""
    return int(min(Wt, length, int(np.float32(p) * np.float32(length))))


def philox_words(uid, offset, dom, m, seed):
    """Words 0 and 1 of the block at counter (uid, offset, dom, m), key (seed lo32, seed hi32), as python ints."""
    one = lambda v: np.array([v & 0xFFFFFFFF], dtype=np.uint32)
    w = philox4x32_10(one(uid), one(offset), one(dom), one(m), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return int(w[0][0]), int(w[1][0])


def interval(w0, w1, W, span):
    """(start, width): width uniform on 0..W, start uniform on 0..span - width; python integers, no float."""
    width = ((w0 >> 8) * (W + 1)) >> 24
    start = ((w1 >> 8) * (span - width + 1)) >> 24
    return start, width


def mask_intervals(lengths, ids, policy, F, seed, offset):
    """(B, freq_masks + time_masks, 2) int32 of (start, width), frequency masks first; a row with id < 0 has none: zeros.
    Lengths below 0 count as 0."""
    nF, Wf, nT, Wt, p, _ = fields(policy)
    out = np.zeros((len(lengths), nF + nT, 2), dtype=np.int32)
    for b, (n, uid) in enumerate(zip(lengths, ids)):
        n, uid = max(int(n), 0), int(uid)
        if uid < 0:
            continue
        for m in range(nF):
            out[b, m] = interval(*philox_words(uid, offset, DOM_FREQ, m, seed), min(Wf, F), F)
        for m in range(nT):
            out[b, nF + m] = interval(*philox_words(uid, offset, DOM_TIME, m, seed), time_width_cap(Wt, p, n), n)
    return out


def hit_mask(iv, lengths, n_freq, F, T):
    """(B,F,T) bool: the cells the intervals ``iv`` of mask_intervals replace -- t < len_b, and f in a frequency interval or t in a
    time interval of b."""
    hit = np.zeros((len(lengths), F, T), dtype=bool)
    for b, n in enumerate(lengths):
        for m, (s, w) in enumerate(iv[b]):
            if m < n_freq:
                hit[b, s:s + w, :] = True
            else:
                hit[b, :, s:s + w] = True
        hit[b, :, max(int(n), 0):] = False
    return hit


def apply(x, lengths, ids, policy, seed, offset):
    """x (B,F,T) fp32 -> (masked copy, fill (B,F) fp32): fill[b,f] is the mean of the original x[b,f,:len_b] summed and divided in
    fp64, rounded to fp32 (0 where len_b <= 0), whatever the fill mode; cells t < len_b in a frequency or time interval of b take
    fill[b,f] ("row_mean") or 0 ("zero"); everything else is copied."""
    x = np.asarray(x, dtype=np.float32)
    B, F, T = x.shape
    nF = fields(policy)[0]
    mode = fields(policy)[5]
    iv = mask_intervals(lengths, ids, policy, F, seed, offset)
    hit = hit_mask(iv, lengths, nF, F, T)
    out = x.copy()
    fill = np.zeros((B, F), dtype=np.float32)
    for b in range(B):
        n = min(max(int(lengths[b]), 0), T)
        if n <= 0 or int(ids[b]) < 0:
            continue
        fill[b] = (x[b, :, :n].astype(np.float64).sum(axis=1) / np.float64(n)).astype(np.float32)
        val = fill[b][:, None] if mode == "row_mean" else np.float32(0.0)
        out[b] = np.where(hit[b], val, x[b])
    return out, fill
