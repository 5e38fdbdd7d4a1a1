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
        self._resample = None

    def mel_db(self, waves, rates=None, target_rate=None, speed=None, wave_aug=None):
        """rates / target_rate: the items' sample rates and the rate the front end works at (16000) -- an item at another rate is
        converted on the device first (Resample); speed: one resampling ratio (L, M) per item (SpeedPerturb.ratios), or None.  Both
        on one item compose into one ratio and one pass.  All three None: no resampling code runs.
        wave_aug: None, or a callable (wave (B, stride), n (B) int32) -> wave of the same shape (``WaveAugment.bind``): noise and
        reverberation of the packed batch, after the resampling and in front of the framing.  None: no such code runs."""
        lib = _lib.load()
        dev = self.device
        B = len(waves)
        if (rates is None or target_rate is None) and speed is None:
            ns = [int(w.numel()) for w in waves]
            if min(ns) <= N_FFT // 2:
                raise ValueError("reflect-centred framing needs more than n_fft/2 = 200 samples per utterance")
            nmax = (max(ns) + 3) // 4 * 4
            wave = torch.zeros(B, nmax, dtype=torch.float32, device=dev)
            for i, w in enumerate(waves):
                wave[i, :ns[i]] = w.reshape(-1).to(device=dev, dtype=torch.float32)
        else:
            if self._resample is None:
                self._resample = Resample(dev)
            wave, ns = self._resample.apply(waves, item_ratios(B, rates, target_rate, speed))
            if min(ns) <= N_FFT // 2:
                raise ValueError("reflect-centred framing needs more than n_fft/2 = 200 samples per utterance (after resampling)")
            nmax = wave.stride(0)          # the row stride: the resampler's buffer may be wider than the longest result
        n_samples = torch.tensor(ns, dtype=torch.int32, device=dev)
        if wave_aug is not None:
            wave = wave.contiguous()       # the resampler's result may be a view of a wider buffer
            nmax = wave.shape[1]
            aug = wave_aug(wave, n_samples)
            if tuple(aug.shape) != tuple(wave.shape) or aug.dtype != torch.float32 or not aug.is_contiguous():
                raise ValueError("wave_aug must return a contiguous fp32 batch of the shape it was given")
            wave = aug
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
    """waves: list of 1-D float tensors (any device; moved to ``device``) -> (feat (B,120,Tmax), fmask (B,1,Tmax)).
    rates / target_rate / speed: optional resampling in front of the framing; wave_aug: optional noise / reverberation behind it
    (``_FrontEnd.mel_db``)."""

    def __init__(self, device="cuda:0"):
        super().__init__(device, N_MELS)

    def __call__(self, waves, rates=None, target_rate=None, speed=None, wave_aug=None):
        lib = _lib.load()
        dev = self.device
        mel, n_frames, B, Tmax = self.mel_db(waves, rates, target_rate, speed, wave_aug)
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

    def __call__(self, waves, rates=None, target_rate=None, speed=None, wave_aug=None):
        lib = _lib.load()
        mel, n_frames, B, Tmax = self.mel_db(waves, rates, target_rate, speed, wave_aug)
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


class FrameStack:
    """The low-frame-rate input policy (Sak et al., Interspeech 2015; Pundak & Sainath, Interspeech 2016): ``stack`` neighbouring
    frames are stacked into one and every ``skip``-th one is kept, so the encoder, the lattice, the sampler and every decoder see
    n' = ceil(n / skip) frames of stack * F features (include/pgasr_hip.h, A0-LFR):
        feat'[b, j*F + f, t'] = feat[b, f, clamp(t'*skip + j - left, 0, n-1)],   j = 0 .. stack-1   (offset-major, as Kaldi's splice)
    ``left`` of the stacked frames lie in front of the anchor frame t'*skip; the edges replicate the first / last real frame.
    Limits: 1 <= stack, skip <= 16, 0 <= left < stack.  Parameter-free, so there is no backward pass: it sits in front of the train
    step.  ORDER: SpecAugment masks the UNSTACKED (B,F,T) tensor first -- a band mask then is one band of rows and a time mask a run
    of input frames -- and stacking comes last, directly in front of the model.
    Immutable; ``state()`` / ``from_state()`` for checkpoints.  ``fs(feat, fmask)`` -> (feat' (B, stack*F, T'), fmask' (B,1,T')) on the
    device, T' = ceil(T / skip); fmask (B,1,T) / (B,T), or lengths (B) int32.  No CPU path."""
    FIELDS = ("stack", "skip", "left")
    __slots__ = FIELDS

    def __init__(self, stack=3, skip=3, left=0):
        stack, skip, left = hipops.frame_stack_check(stack, skip, left, "FrameStack")
        for k, v in zip(self.FIELDS, (stack, skip, left)):
            object.__setattr__(self, k, v)

    def __setattr__(self, k, v):
        raise AttributeError("FrameStack is immutable")

    def __delattr__(self, k):
        raise AttributeError("FrameStack is immutable")

    def state(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    @classmethod
    def from_state(cls, state):
        unknown = sorted(set(state) - set(cls.FIELDS))
        if unknown:
            raise ValueError(f"FrameStack: unknown fields {unknown}")
        return cls(**state)

    @classmethod
    def coerce(cls, value, what="frame_stack"):
        """None, a FrameStack, a dict of its fields or (stack, skip[, left]) -> None or a FrameStack; anything else: TypeError."""
        if value is None or isinstance(value, cls):
            return value
        if isinstance(value, dict):
            return cls.from_state(value)
        if isinstance(value, (tuple, list)) and len(value) in (2, 3):
            return cls(*value)
        raise TypeError(f"{what} must be None, a features.FrameStack, a dict of its fields or (stack, skip[, left]) (got {value!r})")

    def __eq__(self, other):
        return isinstance(other, FrameStack) and self.state() == other.state()

    def __hash__(self):
        return hash(tuple(self.state().values()))

    def __repr__(self):
        return "FrameStack({})".format(", ".join(f"{k}={getattr(self, k)!r}" for k in self.FIELDS))

    def out_feats(self, F):
        """Features per stacked frame."""
        return self.stack * int(F)

    def out_frames(self, n):
        """Frames that n input frames leave: ceil(n / skip) (a python int, or elementwise on an integer tensor / array)."""
        return (n + (self.skip - 1)) // self.skip

    def input_span(self, start, end, n):
        """The input frames [start*skip, min(end*skip, n)) that the stacked frames [start, end) of an utterance of n input frames are
        anchored at: stacked frame t' stands at input frame t'*skip."""
        return int(start) * self.skip, min(int(end) * self.skip, int(n))

    def fits(self, trans, tg_len, n_out, blank=0):
        """(B) bool: the transcript still has a CTC alignment over the stacked frames, L + repeats <= n' (repeats: positions whose
        symbol equals the one in front of it, which need a blank between them).  trans (B,Lmax) integer ids; tg_len (B), or None:
        the count of ids != blank; n_out (B).  Tensor operations on the tensors' device only: no host synchronisation."""
        trans = torch.as_tensor(trans)
        n_out = torch.as_tensor(n_out, device=trans.device)
        if tg_len is None:
            tg_len = (trans != blank).sum(dim=1)
        tg_len = torch.as_tensor(tg_len, device=trans.device).to(torch.int64)
        pos = torch.arange(1, trans.shape[1], device=trans.device)[None, :]
        repeats = ((trans[:, 1:] == trans[:, :-1]) & (pos < tg_len[:, None])).sum(dim=1)
        return tg_len + repeats <= n_out.to(torch.int64)

    def __call__(self, feat, fmask):
        if not isinstance(feat, torch.Tensor) or not feat.is_cuda:
            raise _lib.PgasrError("FrameStack stacks on the MI355X only; there is no CPU path")
        if isinstance(fmask, torch.Tensor) and fmask.is_floating_point():
            out, fmask_out, _ = hipops.frame_stack(feat, fmask=fmask, **self.state())
        else:
            if not isinstance(fmask, torch.Tensor):
                fmask = torch.tensor(list(fmask), dtype=torch.int32)
            out, fmask_out, _ = hipops.frame_stack(feat, lengths=fmask.to(device=feat.device, dtype=torch.int32).contiguous(),
                                                   **self.state())
        return out, fmask_out


RESAMPLE_ZEROS, RESAMPLE_ROLLOFF = 6, 0.99              # torchaudio's default sinc_interp_hann resampler
RESAMPLE_MAX_LM, RESAMPLE_MAX_FACTOR, RESAMPLE_MAX_RATIOS = hipops.RESAMPLE_MAX_LM, hipops.RESAMPLE_MAX_FACTOR, hipops.RESAMPLE_MAX_RATIOS


def reduce_ratio(L, M):
    """(L, M) -> the reduced ratio as python ints; ValueError unless it lies within the kernel's limits (include/pgasr_hip.h, A0-RS)."""
    L, M = int(L), int(M)
    if L < 1 or M < 1:
        raise ValueError(f"a resampling ratio needs L, M >= 1 (got {L}/{M})")
    g = math.gcd(L, M)
    L, M = L // g, M // g
    if L > RESAMPLE_MAX_LM or M > RESAMPLE_MAX_LM or L > RESAMPLE_MAX_FACTOR * M or M > RESAMPLE_MAX_FACTOR * L:
        raise ValueError(f"resampling ratio {L}/{M} is beyond the limits: L, M <= {RESAMPLE_MAX_LM} after reduction and "
                         f"1/{RESAMPLE_MAX_FACTOR} <= L/M <= {RESAMPLE_MAX_FACTOR}")
    return L, M


_filters = {}


def resample_filter(L, M):
    """The polyphase Hann-windowed sinc filter of the reduced ratio L / M (A0-RS): (h (L, W) fp32, base (L,) int32, half), computed
    in fp64 and rounded to fp32 once; cached per (L, M), the arrays are read-only."""
    import numpy as np
    L, M = int(L), int(M)
    hit = _filters.get((L, M))
    if hit is not None:
        return hit
    if reduce_ratio(L, M) != (L, M):
        raise ValueError(f"resample_filter wants a reduced ratio (got {L}/{M})")
    fc = RESAMPLE_ROLLOFF * (L / M if L < M else 1.0)
    half = int(math.ceil(RESAMPLE_ZEROS / fc))
    W = 2 * half + 1
    j = np.arange(L, dtype=np.int64)
    base = (j * M) // L
    frac = (j * M).astype(np.float64) / np.float64(L) - base.astype(np.float64)
    d = (np.arange(W, dtype=np.float64)[None, :] - half) - frac[:, None]
    t = fc * d
    pt = np.pi * t
    sinc = np.where(t == 0.0, 1.0, np.sin(pt) / np.where(t == 0.0, 1.0, pt))
    h = np.where(np.abs(t) < RESAMPLE_ZEROS, fc * sinc * np.cos(pt / (2.0 * RESAMPLE_ZEROS)) ** 2, 0.0).astype(np.float32)
    base = base.astype(np.int32)
    h.setflags(write=False); base.setflags(write=False)
    _filters[(L, M)] = (h, base, half)
    return _filters[(L, M)]


def resample_length(n, L, M):
    """Samples a ratio L / M makes of n: ceil(n * L / M), in python integers (no overflow)."""
    n, L, M = int(n), int(L), int(M)
    return (max(n, 0) * L + M - 1) // M


class Resample:
    """Sample-rate conversion on the device (hipops.resample, one polyphase windowed-sinc kernel):
    ``Resample(device)(waves, rates, target_rate=16000)`` -> (wave (B, nmax) fp32 on the device, zero beyond each length; lengths, a
    list of python ints).  waves: 1-D float tensors (any device); rates: one sample rate per item (None: the item is at the target).
    An item already at the target is copied, not filtered.  ``apply(waves, ratios)`` takes one reduced (L, M) per item instead.
    A batch with more than 8 distinct ratios is split into several launches.  Lengths are computed on the host: no synchronisation."""

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PgasrError("resampling runs on the MI355X only; there is no CPU path")

    def __call__(self, waves, rates, target_rate=SAMPLE_RATE):
        return self.apply(waves, item_ratios(len(waves), rates, target_rate, None))

    def apply(self, waves, ratios):
        dev = self.device
        B = len(waves)
        if len(ratios) != B:
            raise ValueError(f"{B} waveforms but {len(ratios)} ratios")
        ratios = [reduce_ratio(*r) for r in ratios]
        distinct = sorted(set(ratios))
        # a launch takes 8 ratios and contiguous rows: with more distinct ones the batch is laid out group by group (a stable sort:
        # one group leaves the rows where they are)
        groups = [distinct[k:k + RESAMPLE_MAX_RATIOS] for k in range(0, len(distinct), RESAMPLE_MAX_RATIOS)]
        group_of = {r: g for g, rs in enumerate(groups) for r in rs}
        order = sorted(range(B), key=lambda i: group_of[ratios[i]])
        ns = [int(w.numel()) for w in waves]
        lengths = [resample_length(n, *r) for n, r in zip(ns, ratios)]
        in_stride = max((max(ns) + 3) // 4 * 4, 4)
        nmax = max((max(lengths) + 3) // 4 * 4, 4)
        wave = torch.zeros(B, in_stride, dtype=torch.float32, device=dev)
        for row, i in enumerate(order):
            wave[row, :ns[i]] = waves[i].reshape(-1).to(device=dev, dtype=torch.float32)
        if distinct == [(1, 1)]:
            return wave, lengths
        # the kernel wants room for what the longest row would give at the batch's largest ratio; the result is the view of the
        # first nmax columns
        out_stride = (max(resample_length(in_stride, *r) for r in distinct) + 3) // 4 * 4
        n_in = torch.tensor([ns[i] for i in order], dtype=torch.int32, device=dev)
        out = torch.empty(B, out_stride, dtype=torch.float32, device=dev)
        n_out = torch.empty(B, dtype=torch.int32, device=dev)
        s = 0
        for g, rs in enumerate(groups):
            e = s + sum(1 for i in order if group_of[ratios[i]] == g)
            idx = torch.tensor([rs.index(ratios[i]) for i in order[s:e]], dtype=torch.int32, device=dev)
            hipops.resample(wave[s:e], n_in[s:e], rs, ratio_idx=idx, out=out[s:e], n_out=n_out[s:e])
            s = e
        if order != list(range(B)):
            inv = [0] * B
            for row, i in enumerate(order):
                inv[i] = row
            out = out[torch.tensor(inv, device=dev)]
        return out[:, :nmax], lengths


def item_ratios(B, rates, target_rate, speed):
    """One reduced (L, M) per item: the rate conversion target_rate / rate (rate None, or target_rate None: none) composed with the
    item's speed ratio ``speed[i]`` = (L, M) (None: none) into ONE ratio, so one pass does both."""
    out = []
    for i in range(B):
        L, M = 1, 1
        rate = rates[i] if (rates is not None and target_rate is not None) else None
        if rate is not None:
            if int(rate) != rate or int(target_rate) != target_rate or rate < 1 or target_rate < 1:
                raise ValueError(f"sample rates must be positive integers (got {rate!r} -> {target_rate!r})")
            L, M = int(target_rate), int(rate)
        if speed is not None and speed[i] is not None:
            L, M = L * int(speed[i][0]), M * int(speed[i][1])
        out.append(reduce_ratio(L, M))
    return out


def _philox4x32_10(c, k):
    """One Philox4x32-10 block (Salmon et al. 2011) in python integers: counter (c0..c3), key (k0, k1) -> four 32-bit words; the
    constants of csrc/common.h."""
    c0, c1, c2, c3 = (int(v) & 0xFFFFFFFF for v in c)
    k0, k1 = (int(v) & 0xFFFFFFFF for v in k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


class SpeedPerturb:
    """The speed-perturbation policy (Ko et al., Interspeech 2015): every utterance is resampled by one of ``factors`` (default 0.9,
    1.0, 1.1), drawn uniformly, and the result is still called 16 kHz -- a factor f = p / q makes an utterance f times faster and 1 / f
    times as long: the resampling ratio L / M = q / p.  Factors are given as floats (or Fractions, or (p, q) pairs) and stored as
    reduced fractions; one that is no ratio within the kernel's limits (p, q <= 1024, 1/16 <= f <= 16) is refused.
    The draw for the utterance with global index u is a function of (seed, offset, u) only:
        idx = ((w0 >> 8) * len(factors)) >> 24,   w0 = word 0 of philox4x32_10(ctr = (u, offset, 4, 0), key = (seed lo32, seed hi32))
    (counter word 2: the samplers hold 0 and 1, SpecAugment 2 and 3, so one seed serves all three) -- a rank, a shard or a micro-batch
    perturbs what one process holding the whole batch perturbs.  It is drawn on the host, which needs the output lengths to size the
    batch anyway.  Immutable; ``state()`` / ``from_state()`` for checkpoints.  ``ratios(utt_ids, seed, offset)`` -> one (L, M) per id."""
    DOMAIN = 4
    __slots__ = ("factors",)

    def __init__(self, factors=(0.9, 1.0, 1.1)):
        import fractions
        import numbers
        if isinstance(factors, (str, bytes, numbers.Number)):
            raise TypeError(f"SpeedPerturb: factors must be a sequence of speed factors (got {factors!r})")
        fr = []
        for f in factors:
            if isinstance(f, (tuple, list)) and len(f) == 2:
                q = fractions.Fraction(int(f[0]), int(f[1])) if int(f[0]) > 0 and int(f[1]) > 0 else None
            elif isinstance(f, bool) or not isinstance(f, (numbers.Real, fractions.Fraction)):
                raise TypeError(f"SpeedPerturb: a factor must be a real number or a (p, q) pair (got {f!r})")
            elif not (f > 0 and f < float("inf")):
                q = None
            else:
                q = fractions.Fraction(f).limit_denominator(RESAMPLE_MAX_LM)
                if abs(float(q) - float(f)) > 1e-9 * float(f):
                    q = None
            if q is None or q.numerator > RESAMPLE_MAX_LM or q.denominator > RESAMPLE_MAX_LM or \
                    q > RESAMPLE_MAX_FACTOR or q * RESAMPLE_MAX_FACTOR < 1:
                raise ValueError(f"SpeedPerturb: factor {f!r} is no ratio p/q within the limits p, q <= {RESAMPLE_MAX_LM}, "
                                 f"1/{RESAMPLE_MAX_FACTOR} <= p/q <= {RESAMPLE_MAX_FACTOR}")
            fr.append((q.numerator, q.denominator))
        if not fr:
            raise ValueError("SpeedPerturb: factors must not be empty")
        object.__setattr__(self, "factors", tuple(fr))

    def __setattr__(self, k, v):
        raise AttributeError("SpeedPerturb is immutable")

    __delattr__ = __setattr__

    def state(self):
        return {"factors": [list(f) for f in self.factors]}

    @classmethod
    def from_state(cls, state):
        unknown = sorted(set(state) - {"factors"})
        if unknown:
            raise ValueError(f"SpeedPerturb: unknown fields {unknown}")
        return cls(**state)

    @classmethod
    def coerce(cls, value, what="speed_perturb"):
        """None, a SpeedPerturb, a dict of its state or a sequence of factors -> None or a SpeedPerturb; anything else: TypeError."""
        if value is None or isinstance(value, cls):
            return value
        if isinstance(value, dict):
            return cls.from_state(value)
        if isinstance(value, (tuple, list)):
            return cls(value)
        raise TypeError(f"{what} must be None, a features.SpeedPerturb, a dict of its state or a sequence of factors (got {value!r})")

    def __eq__(self, other):
        return isinstance(other, SpeedPerturb) and self.factors == other.factors

    def __hash__(self):
        return hash(self.factors)

    def __repr__(self):
        return "SpeedPerturb(factors=({}))".format(", ".join(f"{p}/{q}" for p, q in self.factors))

    def draw(self, utt_id, seed, offset):
        """The index into ``factors`` of utterance ``utt_id``."""
        seed = int(seed) & (2 ** 64 - 1)
        w0 = _philox4x32_10((int(utt_id), int(offset), self.DOMAIN, 0), (seed & 0xFFFFFFFF, seed >> 32))[0]
        return ((w0 >> 8) * len(self.factors)) >> 24

    def ratios(self, utt_ids, seed, offset):
        """One resampling ratio (L, M) = (q, p) per utterance id."""
        out = []
        for u in utt_ids:
            p, q = self.factors[self.draw(u, seed, offset)]
            out.append((q, p))
        return out


REVERB_MAX_TAPS = hipops.REVERB_MAX_TAPS


def _pack_bank(waves, rates, target_rate, device, what):
    """Waveforms -> (wave (R, stride) fp32 on the device, lengths): packed once, brought to target_rate with ``Resample``."""
    waves = list(waves)
    if not waves:
        raise ValueError(f"{what}: no waveforms")
    if any(int(w.numel()) < 1 for w in waves):
        raise ValueError(f"{what}: an empty waveform")
    if rates is not None and len(rates) != len(waves):
        raise ValueError(f"{what}: {len(waves)} waveforms but {len(rates)} rates")
    wave, lengths = Resample(device)(waves, rates, target_rate)
    return wave.contiguous(), [int(v) for v in lengths]


class NoiseBank:
    """Noise recordings for ``WaveAugment``, packed on the device once: ``NoiseBank(waves, rates=None, target_rate=16000, device=...)``;
    waves: 1-D float tensors, rates: one sample rate per item (None: at the target).  ``wave`` (R, stride) fp32, ``lengths`` (python
    ints), ``len_dev`` (R) int32.  A recording shorter than an utterance is repeated cyclically from the drawn start."""

    def __init__(self, waves, rates=None, target_rate=SAMPLE_RATE, device="cuda:0"):
        self.device = torch.device(device)
        self.wave, self.lengths = _pack_bank(waves, rates, target_rate, self.device, "NoiseBank")
        self.len_dev = torch.tensor(self.lengths, dtype=torch.int32, device=self.device)

    def __len__(self):
        return len(self.lengths)


class RirBank:
    """Room impulse responses for ``WaveAugment``, packed on the device once like ``NoiseBank``; each is cut to ``REVERB_MAX_TAPS``
    taps, scaled to unit energy (fp64 sum of squares, one division per tap in fp64, rounded to fp32) and its direct path -- the first
    index of max |h| -- is found here, on the host: ``wave`` (R, stride) fp32, ``lengths``, ``delays`` (python ints), ``len_dev``,
    ``delay_dev`` (R) int32.  An all-zero response is refused."""

    def __init__(self, waves, rates=None, target_rate=SAMPLE_RATE, device="cuda:0"):
        import numpy as np
        self.device = torch.device(device)
        wave, lengths = _pack_bank(waves, rates, target_rate, self.device, "RirBank")
        h = wave.cpu().numpy()[:, :REVERB_MAX_TAPS].copy()
        self.lengths = [min(n, REVERB_MAX_TAPS) for n in lengths]
        self.delays = []
        for r, K in enumerate(self.lengths):
            h[r, K:] = 0.0
            e = float(np.sum(h[r, :K].astype(np.float64) ** 2))
            if not (e > 0.0 and math.isfinite(e)):
                raise ValueError(f"RirBank: impulse response {r} is all zero or not finite")
            h[r, :K] = (h[r, :K].astype(np.float64) / math.sqrt(e)).astype(np.float32)
            self.delays.append(int(np.argmax(np.abs(h[r, :K]))))
        pad = -h.shape[1] % 4
        if pad:
            h = np.concatenate((h, np.zeros((h.shape[0], pad), dtype=np.float32)), axis=1)
        self.wave = torch.from_numpy(np.ascontiguousarray(h)).to(self.device)
        self.len_dev = torch.tensor(self.lengths, dtype=torch.int32, device=self.device)
        self.delay_dev = torch.tensor(self.delays, dtype=torch.int32, device=self.device)

    def __len__(self):
        return len(self.lengths)


class WaveAugment:
    """Additive noise at a drawn signal-to-noise ratio and reverberation of waveforms on the device (the Kaldi / ESPnet "noise + RIR"
    recipe; include/pgasr_hip.h, A0-WA): ``WaveAugment(noise=None, snr_db=(5.0, 20.0), noise_prob=1.0, rir=None, rir_prob=0.5)`` with a
    ``NoiseBank`` and / or a ``RirBank`` (``draws`` needs only their ``lengths``).  A reverberated utterance is brought back to its dry
    level; the noise -- a segment of one recording from a drawn start, repeated cyclically -- is scaled to the drawn SNR against it.
    The draws of the utterance with global index u are a function of (seed, offset, u) only, made on the host from two Philox4x32-10
    blocks, key = (seed lo32, seed hi32) (counter word 2: the samplers hold 0 and 1, SpecAugment 2 and 3, speed perturbation 4):
        w = philox4x32_10(ctr = (u, offset, 5, 0)):  noise applies iff (w0 >> 8) < round(noise_prob * 2^24);  recording r = ((w1 >> 8) * Rn) >> 24;
            snr = lo + (hi - lo) * (w2 >> 8) / 2^24 dB;  start = ((w3 >> 8) * m_r) >> 24,  m_r the recording's length
        w = philox4x32_10(ctr = (u, offset, 6, 0)):  reverberation applies iff (w0 >> 8) < round(rir_prob * 2^24);  response ((w1 >> 8) * Rr) >> 24
    so a rank, a shard or a micro-batch augments what one process holding the whole batch augments.  An id < 0 (padding) is never
    augmented.  Immutable; ``state()`` for checkpoints (the policy and the banks' lengths).
    ``aug.draws(ids, seed, offset)`` -> dict of host arrays; ``aug(wave, n, ids, seed, offset)`` -> the augmented (B, stride) batch."""
    NOISE_DOMAIN, RIR_DOMAIN = 5, 6
    FIELDS = ("noise", "snr_db", "noise_prob", "rir", "rir_prob")
    __slots__ = FIELDS

    def __init__(self, noise=None, snr_db=(5.0, 20.0), noise_prob=1.0, rir=None, rir_prob=0.5):
        import numbers
        set_ = lambda k, v: object.__setattr__(self, k, v)
        for k, bank in (("noise", noise), ("rir", rir)):
            if bank is not None:
                lengths = getattr(bank, "lengths", None)
                if not lengths or any(int(v) < 1 for v in lengths):
                    raise ValueError(f"WaveAugment: {k} must be None or a bank with positive lengths")
            set_(k, bank)
        if noise is None and rir is None:
            raise ValueError("WaveAugment needs a noise bank, an impulse-response bank or both")
        if isinstance(snr_db, numbers.Real) and not isinstance(snr_db, bool):
            snr_db = (snr_db, snr_db)
        try:
            lo, hi = (float(v) for v in snr_db)
        except (TypeError, ValueError):
            raise TypeError(f"WaveAugment: snr_db must be a number or a (low, high) pair in dB (got {snr_db!r})") from None
        if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi and -200.0 <= lo and hi <= 200.0):
            raise ValueError(f"WaveAugment: snr_db must be finite, low <= high, within +-200 dB (got {snr_db!r})")
        set_("snr_db", (lo, hi))
        for k, v in (("noise_prob", noise_prob), ("rir_prob", rir_prob)):
            if isinstance(v, bool) or not isinstance(v, numbers.Real):
                raise TypeError(f"WaveAugment: {k} must be a real number (got {v!r})")
            if not 0.0 <= float(v) <= 1.0:
                raise ValueError(f"WaveAugment: {k} must lie in [0, 1] (got {v!r})")
            set_(k, float(v))

    def __setattr__(self, k, v):
        raise AttributeError("WaveAugment is immutable")

    __delattr__ = __setattr__

    def state(self):
        return {"snr_db": list(self.snr_db), "noise_prob": self.noise_prob, "rir_prob": self.rir_prob,
                "noise_lengths": None if self.noise is None else [int(v) for v in self.noise.lengths],
                "rir_lengths": None if self.rir is None else [int(v) for v in self.rir.lengths]}

    @classmethod
    def coerce(cls, value, what="wave_augment"):
        """None or a WaveAugment -> itself; anything else: TypeError (the banks live on the device: a dict cannot rebuild them)."""
        if value is None or isinstance(value, cls):
            return value
        raise TypeError(f"{what} must be None or a features.WaveAugment (got {value!r})")

    def __eq__(self, other):
        return isinstance(other, WaveAugment) and self.state() == other.state() and self.noise is other.noise and self.rir is other.rir

    def __hash__(self):
        return hash((self.snr_db, self.noise_prob, self.rir_prob, id(self.noise), id(self.rir)))

    def __repr__(self):
        return "WaveAugment(noise={}, snr_db={}, noise_prob={}, rir={}, rir_prob={})".format(
            None if self.noise is None else f"<{len(self.noise.lengths)} recordings>", self.snr_db, self.noise_prob,
            None if self.rir is None else f"<{len(self.rir.lengths)} responses>", self.rir_prob)

    @staticmethod
    def _noise_from_words(w, prob, lengths, snr_db):
        """(apply, recording, snr in dB, start) from one block's four words: integer arithmetic except the SNR."""
        apply = (w[0] >> 8) < int(round(prob * (1 << 24)))
        r = ((w[1] >> 8) * len(lengths)) >> 24
        snr = snr_db[0] + (snr_db[1] - snr_db[0]) * (w[2] >> 8) / float(1 << 24)
        start = ((w[3] >> 8) * int(lengths[r])) >> 24
        return apply, r, snr, start

    @staticmethod
    def _rir_from_words(w, prob, n_rirs):
        return (w[0] >> 8) < int(round(prob * (1 << 24))), ((w[1] >> 8) * n_rirs) >> 24

    def draws(self, ids, seed, offset):
        """Host arrays, one entry per id: noise_idx, noise_start, rir_idx (int32; -1 / 0 / -1 where nothing applies), snr_db and
        amp = 10^(-snr / 20) (float64; 0 where no noise applies)."""
        import numpy as np
        seed = int(seed) & (2 ** 64 - 1)
        key = (seed & 0xFFFFFFFF, seed >> 32)
        ids = [int(u) for u in ids]
        B = len(ids)
        out = {"noise_idx": np.full(B, -1, dtype=np.int32), "noise_start": np.zeros(B, dtype=np.int32),
               "rir_idx": np.full(B, -1, dtype=np.int32), "snr_db": np.zeros(B, dtype=np.float64), "amp": np.zeros(B, dtype=np.float64)}
        for b, u in enumerate(ids):
            if u < 0:
                continue
            if self.noise is not None:
                w = _philox4x32_10((u, int(offset), self.NOISE_DOMAIN, 0), key)
                apply, r, snr, start = self._noise_from_words(w, self.noise_prob, self.noise.lengths, self.snr_db)
                if apply:
                    out["noise_idx"][b], out["noise_start"][b], out["snr_db"][b] = r, start, snr
                    out["amp"][b] = 10.0 ** (-snr / 20.0)
            if self.rir is not None:
                w = _philox4x32_10((u, int(offset), self.RIR_DOMAIN, 0), key)
                apply, r = self._rir_from_words(w, self.rir_prob, len(self.rir.lengths))
                if apply:
                    out["rir_idx"][b] = r
        return out

    def bind(self, ids, seed, offset):
        """The callable (wave, n) -> wave the front ends take as ``wave_aug``: this policy on these ids, in place where it can."""
        ids = [int(u) for u in ids]
        return lambda wave, n: self(wave, n, ids, seed, offset, out=wave)

    def __call__(self, wave, n, ids, seed, offset, out=None, want_gains=False):
        """wave (B, stride) fp32 on the device, zero or anything beyond each length; n: (B) int32 on the device (or python ints);
        ids: one global utterance index per row (< 0: padding, copied).  Returns the augmented batch, zero beyond each length -- a new
        tensor, or ``out`` (``out=wave``: in place where no row is reverberated) -- and with ``want_gains`` the (B, 2) fp32 gains too.
        The chain -- reverberation, three powers, gains, mix -- runs on the current stream without a host synchronisation."""
        if not isinstance(wave, torch.Tensor) or not wave.is_cuda:
            raise _lib.PgasrError("WaveAugment runs on the MI355X only; there is no CPU path")
        dev = wave.device
        if not isinstance(n, torch.Tensor):
            n = torch.tensor([int(v) for v in n], dtype=torch.int32)
        n = n.to(device=dev, dtype=torch.int32).contiguous()
        if isinstance(ids, torch.Tensor):
            ids = ids.tolist()
        d = self.draws(ids, seed, offset)
        if len(d["rir_idx"]) != wave.shape[0]:
            raise ValueError(f"{wave.shape[0]} waveforms but {len(d['rir_idx'])} ids")
        # the draws travel in ONE pinned buffer and one asynchronous copy: amp (fp64) in front, then the three int32 rows
        B = wave.shape[0]
        host = torch.empty(5 * B, dtype=torch.int32, pin_memory=True)
        hn = host.numpy()
        hn[:2 * B].view("float64")[:] = d["amp"]
        hn[2 * B:3 * B], hn[3 * B:4 * B], hn[4 * B:] = d["noise_idx"], d["noise_start"], d["rir_idx"]
        up = host.to(dev, non_blocking=True)
        amp, nidx, nstart, ridx = up[:2 * B].view(torch.float64), up[2 * B:3 * B], up[3 * B:4 * B], up[4 * B:]
        p_dry = hipops.wave_power(wave, n)
        if self.rir is not None and bool((d["rir_idx"] >= 0).any()):
            wet = hipops.reverb(wave, n, self.rir.wave, self.rir.len_dev, self.rir.delay_dev, ridx,
                                out=out if (out is not None and out is not wave) else None)
            p_wet = hipops.wave_power(wet, n)
            if out is None:
                out = wet
        else:
            wet, p_wet = wave, p_dry
        if self.noise is not None and bool((d["noise_idx"] >= 0).any()):
            p_noise = hipops.wave_power(self.noise.wave, n, row=nidx, start=nstart, period=self.noise.len_dev[nidx.clamp(min=0).long()])
            res, gains = hipops.wave_mix(wet, n, p_dry, p_wet, p_noise, amp, self.noise.wave, self.noise.len_dev, nidx, nstart, out=out)
        else:
            res, gains = hipops.wave_mix(wet, n, p_dry, p_wet, out=out)
        return (res, gains) if want_gains else res


def read_wav(path):
    """Integer PCM-16 / PCM-32 RIFF WAV -> (1-D float32 tensor, sample rate): the stand-in for ``torchaudio.load`` (data.py:53) where
    torchaudio is absent; first channel only, like ``.squeeze(0)`` on mono.  A sample is its integer / 2^15 (2^31), rounded to fp32
    once: PCM-16 lies in [-1, 1), PCM-32 in [-1, 1] (the largest integers round up to 1.0).  Anything else is refused with a
    ValueError: 8- and 24-bit PCM, a file that is no RIFF WAV (an empty one included), and above all IEEE-float WAV (format tag 3),
    whose 4-byte samples must never be taken for PCM-32."""
    import wave as _wave
    import numpy as np
    try:
        with _wave.open(path, "rb") as f:
            sr, nch, width, n = f.getframerate(), f.getnchannels(), f.getsampwidth(), f.getnframes()
            raw = f.readframes(n)
    except (_wave.Error, EOFError) as e:       # the wave module reads integer PCM only: format tag 3 ends here, as "unknown format: 3"
        raise ValueError(f"{path}: not an integer-PCM RIFF WAV file ({str(e) or 'file too short'}); IEEE-float (format tag 3) and "
                         f"compressed WAV are not read -- convert to PCM-16 or PCM-32") from e
    if width == 2:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif width == 4:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    else:
        raise ValueError(f"{path}: unsupported sample width {width} bytes (PCM-16 and PCM-32 are read)")
    return torch.from_numpy(x.reshape(-1, nch)[:, 0].copy()), sr
