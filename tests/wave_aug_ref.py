"""The waveform-augmentation functions of include/pgasr_hip.h (A0-WA) in plain numpy, and the case lists the CPU and GPU tests share:
a statement of the specification beside the tests, not a test.  Reverberation is a direct-form FIR summed in ascending tap order in
fp64 and rounded to fp32 once; the power is a sum of squares in fp64; the gains are formed in fp64, each operation rounded once, and
rounded to fp32 before the mix uses them.  The draws go through oracle.decode_ref.philox4x32_10."""
import math

import numpy as np

from oracle.decode_ref import philox4x32_10

DOM_NOISE, DOM_RIR = 5, 6        # Philox counter word 2: the samplers hold 0 and 1, SpecAugment 2 and 3, speed perturbation 4
TILE, CHUNK, MAX_TAPS = 2048, 512, 16384      # hipops.REVERB_TILE / REVERB_CHUNK / REVERB_MAX_TAPS (test_wave_aug_cpu checks them)


def philox4(uid, offset, dom, seed):
    """The four words of the block at counter (uid, offset, dom, 0), key (seed lo32, seed hi32), as python ints."""
    one = lambda v: np.array([v & 0xFFFFFFFF], dtype=np.uint32)
    w = philox4x32_10(one(uid), one(offset), one(dom), one(0), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return tuple(int(v[0]) for v in w)


def draws(ids, seed, offset, noise_lengths=None, n_rirs=0, snr_db=(5.0, 20.0), noise_prob=1.0, rir_prob=0.5):
    """Per id: (noise_idx, noise_start, snr_db, amp, rir_idx); -1 / 0 / 0.0 / 0.0 / -1 where nothing applies or the id is < 0."""
    out = []
    for u in ids:
        ni, ns, snr, amp, ri = -1, 0, 0.0, 0.0, -1
        if u >= 0 and noise_lengths:
            w = philox4(u, offset, DOM_NOISE, seed)
            if (w[0] >> 8) < int(round(noise_prob * 2 ** 24)):
                ni = ((w[1] >> 8) * len(noise_lengths)) >> 24
                snr = snr_db[0] + (snr_db[1] - snr_db[0]) * (w[2] >> 8) / float(2 ** 24)
                ns = ((w[3] >> 8) * int(noise_lengths[ni])) >> 24
                amp = 10.0 ** (-snr / 20.0)
        if u >= 0 and n_rirs:
            w = philox4(u, offset, DOM_RIR, seed)
            if (w[0] >> 8) < int(round(rir_prob * 2 ** 24)):
                ri = ((w[1] >> 8) * n_rirs) >> 24
        out.append((ni, ns, snr, amp, ri))
    return out


def reverb(x, h, d, rounded=True):
    """y[i] = fp32( sum_{k = 0 .. K-1} fp64(h[k]) * fp64(x[i + d - k]) ), ascending k, accumulator from +0.0, terms outside [0, n)
    skipped.  The outer loop runs over the taps, or -- where the row is shorter than the response -- over the samples from the last
    to the first, which visits every output's taps in the same ascending order.  rounded=False: the fp64 accumulator."""
    x64, h64 = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(h, dtype=np.float32).astype(np.float64)
    n, K = x64.shape[0], h64.shape[0]
    d = min(max(int(d), 0), max(K - 1, 0))
    acc = np.zeros(n, dtype=np.float64)
    if K <= n:
        for k in range(K):
            i0, i1 = max(0, k - d), min(n, n + k - d)
            if i1 > i0:
                acc[i0:i1] = acc[i0:i1] + h64[k] * x64[i0 + d - k:i1 + d - k]      # the product of two fp32 numbers is exact in fp64
    else:
        for j in range(n - 1, -1, -1):
            i0, i1 = max(0, j - d), min(n, K + j - d)
            if i1 > i0:
                acc[i0:i1] = acc[i0:i1] + h64[i0 + d - j:i1 + d - j] * x64[j]
    return acc.astype(np.float32) if rounded else acc


def power(src, n, start=0, period=None):
    """sum_{i < n} fp64(src[(start + i) mod period])^2, exactly rounded (math.fsum): the device sums in another fixed order."""
    src = np.asarray(src, dtype=np.float32).astype(np.float64)
    if n <= 0:
        return 0.0
    if period is None:
        seg = src[:n]
    else:
        seg = src[(int(start) % int(period) + np.arange(n, dtype=np.int64)) % int(period)]
    return math.fsum((seg * seg).tolist())


def gains(p_dry, p_wet, p_noise, amp, noisy=True):
    """(a, g) as fp32: a = fp32(sqrt(p_dry / p_wet)), 1 where a power is 0 or the result no finite positive fp32;
    g = fp32(amp * sqrt((fp64(a)^2 * p_wet) / p_noise)), 0 where a power or amp is 0, the row takes no noise or the result is no
    finite positive fp32."""
    a = np.float32(1.0)
    if p_wet > 0.0 and p_dry > 0.0:
        t = np.float32(math.sqrt(p_dry / p_wet))
        if t > 0 and np.isfinite(t):
            a = t
    g = np.float32(0.0)
    if noisy and p_wet > 0.0 and p_noise > 0.0 and amp > 0.0:
        aa = float(a) * float(a)
        with np.errstate(over="ignore"):
            t = np.float32(amp * math.sqrt((aa * p_wet) / p_noise))
        if t > 0 and np.isfinite(t):
            g = t
    return a, g


def mix(x, a, g, noise=None, start=0, period=None):
    """fp32( fp64(a) x[i] + fp64(g) noise[(start + i) mod period] ); g = 0: the term is dropped."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    if float(g) == 0.0 or noise is None:
        return (float(a) * x64).astype(np.float32)
    nz = np.asarray(noise, dtype=np.float32).astype(np.float64)
    seg = nz[(int(start) % int(period) + np.arange(x64.shape[0], dtype=np.int64)) % int(period)]
    return (float(a) * x64 + float(g) * seg).astype(np.float32)


def chain(x, draw, noises, rirs, delays):
    """One utterance through the whole chain.  draw = (noise_idx, noise_start, snr, amp, rir_idx) of ``draws``; noises / rirs: lists
    of fp32 arrays; delays: one per response.  Returns (out fp32, (a, g), (p_dry, p_wet, p_noise))."""
    ni, ns, _, amp, ri = draw
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    wet = reverb(x, rirs[ri], delays[ri]) if ri >= 0 else x.copy()
    p_dry, p_wet = power(x, n), power(wet, n)
    noisy = ni >= 0 and n >= 1
    p_noise = power(noises[ni], n, ns, noises[ni].shape[0]) if noisy else 0.0
    a, g = gains(p_dry, p_wet, p_noise, amp, noisy)
    out = mix(wet, a, g, noises[ni] if noisy else None, ns, noises[ni].shape[0] if noisy else None)
    return out, (a, g), (p_dry, p_wet, p_noise)


# ---- the reverberation cases: (K, n, d), every K with every n and delay it can go wrong at; the longest response with a selection ----
def reverb_cases():
    cases = []
    for K in (1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        ds = sorted({0, min(1, K - 1), K // 2, K - 1})
        for n in (0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
            cases += [(K, n, d) for d in ds]
        cases.append((K, K, K // 2))                       # n = K
    K = MAX_TAPS                                           # n < K throughout
    cases += [(K, 1, 0), (K, 2, K - 1), (K, TILE - 1, K // 2), (K, TILE, 1), (K, TILE + 1, K - 1), (K, 2 * TILE + 1, 0),
              (K, 2 * TILE + 1, K // 2)]
    return cases


# ---- the whole-chain case: a small corpus and the ids whose draws cover every kind of row ----
CHAIN_SEED, CHAIN_OFFSET = 20241, 3
CHAIN_POLICY = {"snr_db": (5.0, 20.0), "noise_prob": 0.7, "rir_prob": 0.5}
NOISE_LENGTHS = (100, 5000, 777)          # the first wraps many times; the last is silent
RIR_LENGTHS = (1, 37, 600)
SILENT_NOISE = 2


def chain_corpus():
    """(noises, rirs) as fp32 arrays; the responses are raw (the bank builder scales them and finds their delays)."""
    rng = np.random.default_rng(CHAIN_SEED)
    noises = [(0.3 * rng.standard_normal(m)).astype(np.float32) for m in NOISE_LENGTHS]
    noises[SILENT_NOISE][:] = 0.0
    rirs = []
    for K in RIR_LENGTHS:
        h = (rng.standard_normal(K) * np.exp(-np.arange(K) / max(K / 4.0, 1.0))).astype(np.float32)
        if K > 8:
            h[5] = 8.0                                      # a direct path that is not the first tap
        rirs.append(h)
    return noises, rirs


def normalise_rir(h):
    """(unit-energy fp32 response, delay): what features.RirBank makes of a response."""
    h64 = np.asarray(h, dtype=np.float32).astype(np.float64)
    e = float(np.sum(h64 ** 2))
    out = (h64 / math.sqrt(e)).astype(np.float32)
    return out, int(np.argmax(np.abs(out)))


def chain_rows():
    """(ids, rows): utterances whose draws under CHAIN_POLICY cover noise + response, noise alone, response alone, neither, the silent
    noise and a silent utterance, beside an id of -1 and an empty row.  The ids are found by scanning 0, 1, 2, ..: the draws are a
    function of the id."""
    want = {"both": None, "noise_only": None, "rir_only": None, "neither": None, "silent_noise": None, "wrapping_noise": None}
    u = 0
    while any(v is None for v in want.values()) and u < 4096:
        ni, _, _, _, ri = draws([u], CHAIN_SEED, CHAIN_OFFSET, NOISE_LENGTHS, len(RIR_LENGTHS), **CHAIN_POLICY)[0]
        kind = ("both" if ri >= 0 else "noise_only") if ni >= 0 else ("rir_only" if ri >= 0 else "neither")
        if ni == SILENT_NOISE and want["silent_noise"] is None:
            kind = "silent_noise"
        elif ni == 0 and want["wrapping_noise"] is None:
            kind = "wrapping_noise"
        if want[kind] is None:
            want[kind] = u
        u += 1
    assert all(v is not None for v in want.values()), want
    rng = np.random.default_rng(CHAIN_SEED + 1)
    lengths = {"both": 2500, "noise_only": 1000, "rir_only": 4097, "neither": 300, "silent_noise": 640, "wrapping_noise": 1501}
    ids, rows = [], []
    for kind, uid in want.items():
        ids.append(uid)
        rows.append((0.1 * rng.standard_normal(lengths[kind])).astype(np.float32))
    silent = 5000                                          # a silent utterance that draws noise and a response
    while True:
        ni, _, _, _, ri = draws([silent], CHAIN_SEED, CHAIN_OFFSET, NOISE_LENGTHS, len(RIR_LENGTHS), **CHAIN_POLICY)[0]
        if ni >= 0 and ni != SILENT_NOISE and ri >= 0:
            break
        silent += 1
    ids += [silent, -1, silent + 1]                        # .., padding, an empty row
    rows += [np.zeros(900, dtype=np.float32), (0.1 * rng.standard_normal(450)).astype(np.float32), np.zeros(0, dtype=np.float32)]
    return ids, rows
