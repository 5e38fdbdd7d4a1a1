"""The feature front end (include/pgasr_hip.h, N3) restated in float32 numpy, and the edge-case inputs the end-to-end tests run:
a statement of what fp32 arithmetic can hold on each input, beside the tests, not a test.

``mfcc_deltas`` / ``log_mel`` follow oracle/features_ref.py step by step with every value and every product in float32: the window
0.5 - 0.5 cos(2 pi k / 400) evaluated in fp32, the DFT / mel / DCT matrices built in fp64 and rounded to fp32 once (as
features._constants does), the three contractions accumulated in fp32 in ascending k (``matmul32``: one defined order, so the
figures below do not depend on a BLAS), |X|^2, 10 log10 and the delta filter in fp32.  The worst absolute difference between this
chain and the fp64 oracle on a case is that case's FLOOR: no fp32 implementation can be asked for much less, and the device, whose
GEMMs accumulate in another order, is held to max(2e-3, 4 x floor) (tests/test_features_gpu.py).

FLOORS records the figures, in dB, as (MFCCDeltas, LogMel(80)); tests/test_features_cpu.py asserts that this module still
reproduces each of them within 10 %, so a tolerance of the GPU test cannot drift unseen.

    case            MFCCDeltas   LogMel(80)   input
    tone            4.09e-4      4.56e-5      440 Hz at 0.9, no noise: 90 % of the cells sit on the top_db clamp
    zeros_tone      3.04e-4      3.78e-5      3000 samples of digital zero, a tone at 0.5, 2000 of zero (94 % clamped)
    zeros_noise     1.10e-3      1.29e-5      zeros, white noise at 0.3, zeros (54 % clamped)
    int16           1.85e-4      4.20e-4      two tones + noise rounded to the int16 grid
    square          1.06e-4      8.15e-5      full-scale 300 Hz square wave
    click           1.21e-3      8.31e-7      one sample of 1.0 in silence (94 % clamped)
    tone_1e-3       1.30e-3      4.13e-5      440 Hz at 1e-3: max - 80 dB meets the 1e-10 floor
    tone_1e-5       1.61e-3      1.67e-5      440 Hz at 1e-5: most cells on the 1e-10 floor, the clamp idle
    dc              2.42e-3      5.12e-3      0.5 + 1e-3 of noise: every cell is the cancelled leakage of a large DC term
    clipped_T261    7.46e-5      4.56e-5      52000 samples of noise clipped to [-1, 1]: 261 frames
    short           9.15e-5      1.45e-4      a batch of 201, 399, 400, 599, 600, 800, 1000 samples: T = 2, 2, 3, 3, 4, 5, 6
    loud_quiet      4.98e-4      4.69e-4      a batch of two tones + noise and the same waveform times 1e-3

Only tone_1e-3, tone_1e-5, dc, click and zeros_noise (all through their MFCC figure, dc through both) reach 4 x floor > 2e-3."""
import zlib

import numpy as np

from oracle import features_ref as fr

N_FFT, HOP, N_BINS = fr.N_FFT, fr.HOP, fr.N_FFT // 2 + 1
F32 = np.float32


def matmul32(a, b):
    """(M, K) @ (K, N) in float32, the K products of an output added one by one in ascending k."""
    a = np.asarray(a, dtype=F32)
    b = np.asarray(b, dtype=F32)
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=F32)
    for k in range(a.shape[1]):
        acc += a[:, k:k + 1] * b[k][None, :]
    return acc


def hann32():
    k = np.arange(N_FFT, dtype=F32)
    return F32(0.5) - F32(0.5) * np.cos(F32(6.283185307179586) * k / F32(N_FFT), dtype=F32)


def dft32():
    n = np.arange(N_FFT, dtype=np.float64)[:, None]
    k = np.arange(N_BINS, dtype=np.float64)[None, :]
    ang = 2.0 * np.pi * n * k / N_FFT
    return np.concatenate((np.cos(ang), -np.sin(ang)), axis=1).astype(F32)


def mel_db(wave, n_mels):
    """1-D waveform -> (T, n_mels) float32: the dB-scaled mel spectrogram, floored at the utterance's maximum - 80 dB."""
    x = np.asarray(wave, dtype=F32)
    pad = N_FFT // 2
    if x.shape[0] <= pad:
        raise ValueError("reflect padding needs more than n_fft/2 samples")
    xp = np.pad(x, (pad, pad), mode="reflect")
    T = fr.n_frames(x.shape[0])
    idx = np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :]
    frames = xp[idx] * hann32()[None, :]
    spec = matmul32(frames, dft32())
    re, im = spec[:, :N_BINS], spec[:, N_BINS:]
    power = re * re + im * im
    mel = matmul32(power, fr.mel_filterbank(n_mels=n_mels).astype(F32))
    db = F32(10.0) * np.log10(np.maximum(mel, F32(fr.AMIN)), dtype=F32)
    return np.maximum(db, db.max() - F32(fr.TOP_DB))


def deltas32(x):
    """(C, T) -> (C, T) in float32: (2 (x[t+2] - x[t-2]) + (x[t+1] - x[t-1])) / 10 over replicate padding."""
    T = x.shape[1]
    at = lambda m: x[:, np.clip(np.arange(T) + m, 0, T - 1)]
    return (F32(2.0) * (at(2) - at(-2)) + (at(1) - at(-1))) / F32(10.0)


def mfcc_deltas(wave):
    """1-D waveform -> (120, T) float32."""
    mfcc = matmul32(mel_db(wave, fr.N_MELS), fr.dct_matrix().astype(F32)).T
    d1 = deltas32(mfcc)
    return np.concatenate((mfcc, d1, deltas32(d1)), axis=0)


def log_mel(wave, n_mels=80):
    """1-D waveform -> (n_mels, T) float32."""
    return mel_db(wave, n_mels).T


def _pad(feats):
    out = np.zeros((len(feats), feats[0].shape[0], max(f.shape[1] for f in feats)), dtype=feats[0].dtype)
    for i, f in enumerate(feats):
        out[i, :, :f.shape[1]] = f
    return out


def extract(kind, waves):
    """kind "mfcc" or "logmel80", list of waveforms -> (B, F, Tmax) float32, zero padded."""
    return _pad([mfcc_deltas(w) if kind == "mfcc" else log_mel(w, 80) for w in waves])


def oracle(kind, waves):
    """The fp64 oracle on the same fp32 waveforms -> (B, F, Tmax) float64, zero padded."""
    w64 = [np.asarray(w, dtype=np.float64) for w in waves]
    return (fr.extract_feats(w64) if kind == "mfcc" else fr.extract_logmel(w64, 80))[0]


def _tone(n, amp, hz=440.0):
    return (amp * np.sin(2.0 * np.pi * hz * np.arange(n) / fr.SAMPLE_RATE)).astype(F32)


def _speech_like(n, rng, i=0):
    t = np.arange(n) / fr.SAMPLE_RATE
    return (0.3 * np.sin(2 * np.pi * (200.0 + 150.0 * i) * t) + 0.1 * np.sin(2 * np.pi * 3100.0 * t)
            + 0.02 * rng.standard_normal(n)).astype(F32)


SHORT_COUNTS = (201, 399, 400, 599, 600, 800, 1000)           # T = 2, 2, 3, 3, 4, 5, 6


def case(name):
    """name -> list of 1-D float32 waveforms (one batch).  Seeded: the same arrays on every call."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    z = lambda n: np.zeros(n, dtype=F32)
    if name == "tone":
        return [_tone(8000, 0.9)]
    if name == "zeros_tone":
        return [np.concatenate((z(3000), _tone(4000, 0.5), z(2000)))]
    if name == "zeros_noise":
        return [np.concatenate((z(3000), (0.3 * rng.standard_normal(4000)).astype(F32), z(2000)))]
    if name == "int16":
        return [(np.round(_speech_like(6000, rng).astype(np.float64) * 32767.0) / 32768.0).astype(F32)]
    if name == "square":
        return [np.where(np.sin(2.0 * np.pi * 300.0 * (np.arange(6000) + 0.5) / fr.SAMPLE_RATE) >= 0, 1.0, -1.0).astype(F32)]
    if name == "click":
        x = z(6000)
        x[2500] = 1.0
        return [x]
    if name == "tone_1e-3":
        return [_tone(8000, 1e-3)]
    if name == "tone_1e-5":
        return [_tone(8000, 1e-5)]
    if name == "dc":
        return [(0.5 + 1e-3 * rng.standard_normal(6000)).astype(F32)]
    if name == "clipped_T261":
        return [np.clip(0.8 * rng.standard_normal(52000), -1.0, 1.0).astype(F32)]
    if name == "short":
        return [_speech_like(n, rng, i) for i, n in enumerate(SHORT_COUNTS)]
    if name == "loud_quiet":
        loud = _speech_like(6000, rng)
        return [loud, loud * F32(1e-3)]
    raise KeyError(name)


# case -> (floor of MFCCDeltas, floor of LogMel(80)) in dB: max |this module - fp64 oracle| over the batch
FLOORS = {
    "tone": (4.09e-4, 4.56e-5),
    "zeros_tone": (3.04e-4, 3.78e-5),
    "zeros_noise": (1.10e-3, 1.29e-5),
    "int16": (1.85e-4, 4.20e-4),
    "square": (1.06e-4, 8.15e-5),
    "click": (1.21e-3, 8.31e-7),
    "tone_1e-3": (1.30e-3, 4.13e-5),
    "tone_1e-5": (1.61e-3, 1.67e-5),
    "dc": (2.42e-3, 5.12e-3),
    "clipped_T261": (7.46e-5, 4.56e-5),
    "short": (9.15e-5, 1.45e-4),
    "loud_quiet": (4.98e-4, 4.69e-4),
}
CASES = tuple(FLOORS)
KINDS = ("mfcc", "logmel80")
# the cases that claim the top_db clamp: at least this share of the 80-band log-mel cells lies below (max - 80 dB) before the clamp
CLAMPED_SHARE = {"tone": 0.85, "zeros_tone": 0.85, "zeros_noise": 0.5, "click": 0.85}


def tolerance(name, kind):
    """The device's bound on one case, in dB: max(2e-3, 4 x floor)."""
    return max(2e-3, 4.0 * FLOORS[name][KINDS.index(kind)])


def clamped_share(wave, n_mels=80):
    """Share of the fp64 oracle's log-mel cells that the top_db clamp raises."""
    mel = fr.power_spectrogram(np.asarray(wave, dtype=np.float64)) @ fr.mel_filterbank(n_mels=n_mels)
    db = 10.0 * np.log10(np.maximum(mel, fr.AMIN))
    return float((db < db.max() - fr.TOP_DB).mean())


def measure(name, kind):
    """The floor of one case: max |float32 chain - fp64 oracle| in dB."""
    waves = case(name)
    return float(np.abs(extract(kind, waves).astype(np.float64) - oracle(kind, waves)).max())
