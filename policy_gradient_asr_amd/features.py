"""Feature front end of the reference on the GPU (data.py:44-79).

``LogMel(80)(waves)`` is the same front end stopped in front of the DCT with an 80-band HTK mel bank: (B,80,Tmax) dB-scaled
log-mel features -- the "mel-spectrogram" input (F = 80) the benchmark's shapes are quoted on; feat / fmask stay on the device.
``MFCCDeltas()(waves)`` returns what ``extract_feats`` returns there: ``feat`` (B,120,Tmax) fp32 zero padded and
``fmask`` (B,1,Tmax) -- MFCC(40) + delta + delta-delta with torchaudio's default parameters, which the reference
uses unchanged (``torchaudio.transforms.MFCC()``, ``ComputeDeltas()``).  torchaudio itself is not needed: framing,
power, the dB map and the delta filters are HIP kernels (csrc/features.hip), the DFT / mel / DCT contractions run
on the matrix cores through ``pgasr_gemm_f32`` in exact-fp32 mode.  No CPU path."""
import math

import torch

from . import _lib, hipops

SAMPLE_RATE, N_FFT, HOP, N_MELS, N_MFCC, TOP_DB = 16000, 400, 200, 128, 40, 80.0
N_BINS = N_FFT // 2 + 1


def _constants(device, n_mels=N_MELS):
    """DFT basis (400, 402) = [cos | -sin], HTK mel bank (201, n_mels), orthonormal DCT-II (n_mels, 40); built in fp64."""
    N_MELS = n_mels
    n = torch.arange(N_FFT, dtype=torch.float64)[:, None]
    k = torch.arange(N_BINS, dtype=torch.float64)[None, :]
    ang = 2.0 * math.pi * n * k / N_FFT
    dft = torch.cat((torch.cos(ang), -torch.sin(ang)), dim=1)
    all_freqs = torch.linspace(0, SAMPLE_RATE // 2, N_BINS, dtype=torch.float64)
    m_max = 2595.0 * math.log10(1.0 + (SAMPLE_RATE / 2.0) / 700.0)
    m_pts = torch.linspace(0.0, m_max, N_MELS + 2, dtype=torch.float64)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    fb = torch.clamp(torch.minimum(-slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]), min=0.0)
    nn_ = torch.arange(N_MELS, dtype=torch.float64)[None, :]
    kk = torch.arange(N_MFCC, dtype=torch.float64)[:, None]
    dct = torch.cos(math.pi / N_MELS * (nn_ + 0.5) * kk)
    dct[0] *= 1.0 / math.sqrt(2.0)
    dct *= math.sqrt(2.0 / N_MELS)
    return tuple(t.to(torch.float32).contiguous().to(device) for t in (dft, fb, dct.t()))


class _FrontEnd:
    """Shared part: waveforms -> dB-scaled mel spectrogram rows (B * Tmax, n_mels) on the device."""

    def __init__(self, device="cuda:0", n_mels=N_MELS):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PgasrError("the feature front end runs on the MI355X only; there is no CPU path")
        self.n_mels = int(n_mels)
        self.dft, self.fb, self.dct = _constants(self.device, self.n_mels)

    def mel_db(self, waves):
        lib = _lib.load()
        dev = self.device
        B = len(waves)
        ns = [int(w.numel()) for w in waves]
        if min(ns) <= N_FFT // 2:
            raise ValueError("reflect-centred framing needs more than n_fft/2 = 200 samples per utterance")
        nmax = (max(ns) + 3) // 4 * 4
        wave = torch.zeros(B, nmax, dtype=torch.float32, device=dev)
        for i, w in enumerate(waves):
            wave[i, :ns[i]] = w.reshape(-1).to(device=dev, dtype=torch.float32)
        n_samples = torch.tensor(ns, dtype=torch.int32, device=dev)
        nf = [1 + n // HOP for n in ns]
        n_frames = torch.tensor(nf, dtype=torch.int32, device=dev)
        Tmax = max(nf)
        rows = B * Tmax
        st = torch.cuda.current_stream().cuda_stream
        frames = torch.empty(rows, N_FFT, dtype=torch.float32, device=dev)
        _lib.check(lib.pgasr_feat_frames(wave.data_ptr(), n_samples.data_ptr(), n_frames.data_ptr(), B, nmax, Tmax,
                                         frames.data_ptr(), st), "pgasr_feat_frames")
        spec = torch.empty(rows, 2 * N_BINS, dtype=torch.float32, device=dev)
        hipops.gemm(frames, self.dft, spec, M=rows, N=2 * N_BINS, K=N_FFT, precision=0)
        power = torch.empty(rows, N_BINS, dtype=torch.float32, device=dev)
        _lib.check(lib.pgasr_feat_power(spec.data_ptr(), rows, power.data_ptr(), st), "pgasr_feat_power")
        mel = torch.empty(rows, self.n_mels, dtype=torch.float32, device=dev)
        hipops.gemm(power, self.fb, mel, M=rows, N=self.n_mels, K=N_BINS, precision=0)
        _lib.check(lib.pgasr_feat_db(mel.data_ptr(), n_frames.data_ptr(), B, Tmax, self.n_mels, TOP_DB, st), "pgasr_feat_db")
        return mel, n_frames, B, Tmax


class MFCCDeltas(_FrontEnd):
    """waves: list of 1-D float tensors (any device; moved to ``device``) -> (feat (B,120,Tmax), fmask (B,1,Tmax))."""

    def __init__(self, device="cuda:0"):
        super().__init__(device, N_MELS)

    def __call__(self, waves):
        lib = _lib.load()
        dev = self.device
        mel, n_frames, B, Tmax = self.mel_db(waves)
        rows = B * Tmax
        st = torch.cuda.current_stream().cuda_stream
        mfcc = torch.empty(rows, N_MFCC, dtype=torch.float32, device=dev)
        hipops.gemm(mel, self.dct, mfcc, M=rows, N=N_MFCC, K=N_MELS, precision=0)
        feat = torch.empty(B, 3 * N_MFCC, Tmax, dtype=torch.float32, device=dev)
        fmask = torch.empty(B, 1, Tmax, dtype=torch.float32, device=dev)
        _lib.check(lib.pgasr_feat_deltas_stack(mfcc.data_ptr(), n_frames.data_ptr(), B, Tmax, N_MFCC, feat.data_ptr(),
                                               fmask.data_ptr(), st), "pgasr_feat_deltas_stack")
        return feat, fmask


class LogMel(_FrontEnd):
    """waves -> (feat (B,n_mels,Tmax), fmask (B,1,Tmax)) on the device: the dB-scaled mel spectrogram the MFCC chain computes in
    front of its DCT (torchaudio's MelSpectrogram + AmplitudeToDB("power", top_db=80) defaults), with an ``n_mels``-band HTK bank --
    80 bands give the F = 80 input of the benchmark (``Encoder(n_feats=80)``), feeding the instance norm / affine (A1-A2) directly."""

    def __init__(self, n_mels=80, device="cuda:0"):
        super().__init__(device, n_mels)

    def __call__(self, waves):
        lib = _lib.load()
        mel, n_frames, B, Tmax = self.mel_db(waves)
        feat = torch.empty(B, self.n_mels, Tmax, dtype=torch.float32, device=self.device)
        fmask = torch.empty(B, 1, Tmax, dtype=torch.float32, device=self.device)
        _lib.check(lib.pgasr_feat_stack(mel.data_ptr(), n_frames.data_ptr(), B, Tmax, self.n_mels, feat.data_ptr(), fmask.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream), "pgasr_feat_stack")
        return feat, fmask


class SpecAugment:
    """The SpecAugment policy (Park et al., arXiv:1904.08779): ``freq_masks`` bands of at most ``freq_width`` feature rows and
    ``time_masks`` spans of at most min(``time_width``, ``time_ratio`` x the utterance's frames) frames are replaced by ``fill`` --
    "row_mean" (default: the mean of the feature row over the utterance's real frames; the encoder's instance norm runs over the
    whole plane afterwards, so such a cell carries no information) or "zero" (in dB-scaled log-mel the loudest possible cell).
    Widths and positions are uniform draws, a function of (seed, offset, global utterance index) only (include/pgasr_hip.h,
    A0-AUG): a rank, a shard or a micro-batch masks what one process holding the whole batch masks.  Limits: 0 <= masks of a kind
    <= MAX_MASKS, widths >= 0, 0 < time_ratio <= 1 (None: 1.0).  Immutable; ``state()`` / ``from_state()`` for checkpoints.
    ``aug(feat, lengths_or_fmask, seed, offset, utt_ids=None)`` masks a (B,F,T) fp32 batch on the device, out of place: lengths (B)
    int32, or the front end's fmask (B,1,T) / (B,T); utt_ids: None (row b is utterance b), or one global index per row."""
    MAX_MASKS = hipops.SPECAUG_MAX_MASKS
    FILLS = tuple(hipops.SPECAUG_FILLS)
    FIELDS = ("freq_masks", "freq_width", "time_masks", "time_width", "time_ratio", "fill")
    __slots__ = FIELDS

    def __init__(self, freq_masks=2, freq_width=27, time_masks=2, time_width=100, time_ratio=1.0, fill="row_mean"):
        import ctypes
        import numbers
        set_ = lambda k, v: object.__setattr__(self, k, v)
        for k, v in (("freq_masks", freq_masks), ("freq_width", freq_width), ("time_masks", time_masks), ("time_width", time_width)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral):
                raise TypeError(f"SpecAugment: {k} must be an integer (got {v!r})")
            if v < 0:
                raise ValueError(f"SpecAugment: {k} must be >= 0 (got {v})")
            if k.endswith("masks") and v > self.MAX_MASKS:
                raise ValueError(f"SpecAugment: {k} must be <= {self.MAX_MASKS} (got {v})")
            if v > 2 ** 31 - 1:
                raise ValueError(f"SpecAugment: {k} must be <= 2^31 - 1 (got {v})")
            set_(k, int(v))
        if time_ratio is None:
            time_ratio = 1.0
        if isinstance(time_ratio, bool) or not isinstance(time_ratio, numbers.Real):
            raise TypeError(f"SpecAugment: time_ratio must be a real number or None (got {time_ratio!r})")
        time_ratio = float(time_ratio)
        if not (0.0 < ctypes.c_float(time_ratio).value and time_ratio <= 1.0):       # NaN included; it travels as fp32
            raise ValueError(f"SpecAugment: time_ratio must lie in (0, 1] (got {time_ratio!r})")
        set_("time_ratio", time_ratio)
        if fill not in self.FILLS:
            raise ValueError(f"SpecAugment: fill must be one of {self.FILLS} (got {fill!r})")
        set_("fill", fill)

    def __setattr__(self, k, v):
        raise AttributeError("SpecAugment is immutable")

    __delattr__ = __setattr__

    def state(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    @classmethod
    def from_state(cls, state):
        unknown = sorted(set(state) - set(cls.FIELDS))
        if unknown:
            raise ValueError(f"SpecAugment: unknown fields {unknown}")
        return cls(**state)

    @classmethod
    def coerce(cls, value, what="spec_augment"):
        """None, a SpecAugment or a dict of its fields -> None or a SpecAugment; anything else: TypeError."""
        if value is None or isinstance(value, cls):
            return value
        if isinstance(value, dict):
            return cls.from_state(value)
        raise TypeError(f"{what} must be None, a features.SpecAugment or a dict of its fields (got {value!r})")

    def __eq__(self, other):
        return isinstance(other, SpecAugment) and self.state() == other.state()

    def __hash__(self):
        return hash(tuple(self.state().values()))

    def __repr__(self):
        return "SpecAugment({})".format(", ".join(f"{k}={getattr(self, k)!r}" for k in self.FIELDS))

    def __call__(self, feat, lengths_or_fmask, seed, offset, utt_ids=None):
        if not isinstance(feat, torch.Tensor) or not feat.is_cuda:
            raise _lib.PgasrError("SpecAugment masks on the MI355X only; there is no CPU path")
        dev = feat.device
        lengths = lengths_or_fmask
        if not isinstance(lengths, torch.Tensor):
            lengths = torch.tensor(list(lengths), dtype=torch.int32)
        if lengths.is_floating_point():          # a frame mask of 1 / 0
            lengths = lengths.reshape(lengths.shape[0], -1).sum(dim=1)
        lengths = lengths.to(device=dev, dtype=torch.int32).contiguous()
        if utt_ids is not None:
            if not isinstance(utt_ids, torch.Tensor):
                utt_ids = torch.tensor(list(utt_ids), dtype=torch.int32)
            utt_ids = utt_ids.to(device=dev, dtype=torch.int32).contiguous()
        return hipops.spec_augment(feat, lengths, self, seed, offset, utt_ids=utt_ids)


def read_wav(path):
    """PCM-16 / PCM-32 / float32 RIFF WAV -> (1-D float32 tensor in [-1,1), sample rate): the stand-in for
    ``torchaudio.load`` (data.py:53) where torchaudio is absent; first channel only, like ``.squeeze(0)`` on mono."""
    import wave as _wave
    import numpy as np
    with _wave.open(path, "rb") as f:
        sr, nch, width, n = f.getframerate(), f.getnchannels(), f.getsampwidth(), f.getnframes()
        raw = f.readframes(n)
    if width == 2:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif width == 4:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    else:
        raise ValueError(f"unsupported sample width {width}")
    return torch.from_numpy(x.reshape(-1, nch)[:, 0].copy()), sr
