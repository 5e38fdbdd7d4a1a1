"""The resampling function of include/pgasr_hip.h (A0-RS) in plain numpy: a statement of the specification beside the tests, not a
test.  A polyphase Hann-windowed sinc filter of ratio L / M (output rate / input rate, reduced), 6 zero crossings, rolloff 0.99;
the table in fp64 rounded to fp32 once, the taps summed in ascending order in fp64, the sum rounded to fp32 once.  The speed draw
goes through oracle.decode_ref.philox4x32_10 (specaug_ref.philox_words)."""
import math

import numpy as np

from specaug_ref import philox_words

ZEROS, ROLLOFF = 6, 0.99
DOM_SPEED = 4                 # Philox counter word 2: the samplers hold 0 and 1, SpecAugment 2 and 3


def filter_table(L, M):
    """(h (L, W) fp32, base (L,) int32, half) of the reduced ratio L / M."""
    assert math.gcd(L, M) == 1
    fc = ROLLOFF * min(1.0, L / M)
    half = int(math.ceil(ZEROS / fc))
    W = 2 * half + 1
    h = np.zeros((L, W), dtype=np.float64)
    base = np.zeros(L, dtype=np.int32)
    for j in range(L):
        base[j] = (j * M) // L
        frac = ((j * M) % L) / L
        for k in range(W):
            t = fc * ((k - half) - frac)
            if abs(t) < ZEROS:
                h[j, k] = fc * np.sinc(t) * math.cos(math.pi * t / (2 * ZEROS)) ** 2       # np.sinc(t) = sin(pi t) / (pi t)
    return h.astype(np.float32), base, half


def length(n, L, M):
    return (max(int(n), 0) * int(L) + int(M) - 1) // int(M)


def resample(x, L, M, table=None):
    """x (n,) fp32 -> (ceil(n L / M),) fp32.  Output i * L + j is the sum over k = 0 .. W-1, in that order, of fp64(h[j][k]) *
    fp64(x[i * M + base_j - half + k]) in an fp64 accumulator starting at +0.0, taps outside [0, n) skipped; 1/1 is the input."""
    x = np.asarray(x, dtype=np.float32)
    if (L, M) == (1, 1):
        return x.copy()
    h, base, half = table if table is not None else filter_table(L, M)
    n, W = x.shape[0], h.shape[1]
    idx = np.arange(length(n, L, M), dtype=np.int64)
    i, j = idx // L, idx % L
    m0 = i * M + base[j].astype(np.int64) - half
    h64, x64 = h.astype(np.float64), x.astype(np.float64)
    acc = np.zeros(idx.shape[0], dtype=np.float64)
    for k in range(W):
        m = m0 + k
        ok = (m >= 0) & (m < n)
        acc[ok] = acc[ok] + h64[j[ok], k] * x64[m[ok]]          # the product of two fp32 numbers is exact in fp64
    return acc.astype(np.float32)


def speed_draw(utt_id, n_factors, seed, offset):
    """idx = ((w0 >> 8) * n_factors) >> 24, w0 = word 0 of the block at counter (utt_id, offset, 4, 0), key = seed."""
    w0, _ = philox_words(utt_id, offset, DOM_SPEED, 0, seed)
    return ((w0 >> 8) * n_factors) >> 24
