"""N3, stage by stage: each kernel of csrc/features.hip called on its own through the C ABI, on inputs built here, against fp64
numpy applied to THE SAME fp32 inputs -- no stage inherits another's rounding, and every tolerance follows from the stage's own
arithmetic.  Padding is poisoned (a sentinel, NaN, or values above every live one) wherever "was it read" can be told from the
output, every output buffer is pre-filled with NaN and carries a guard tail that must come back untouched, and time runs past
the 256-frame block of the two stacking kernels."""
import numpy as np
import pytest
import torch

from oracle import features_ref as fr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_FFT, HOP, N_BINS = fr.N_FFT, fr.HOP, fr.N_FFT // 2 + 1
GUARD = 256
F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def _run(fn, *args):
    """Call an entry point on the current stream and wait for it.  A numpy array travels as a device copy and a tensor as its
    address; both are held here until the kernel has finished, so no address is one the allocator has already handed on."""
    from policy_gradient_asr_amd import _lib
    held = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if isinstance(a, np.ndarray) else a for a in args]
    _lib.check(fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in held], torch.cuda.current_stream().cuda_stream),
               fn.__name__)
    torch.cuda.synchronize()


def _i32(values):
    return np.array(values, dtype=np.int32)


def _out(n):
    """n floats of NaN and a guard tail of NaN behind them."""
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)


def _split(buf, n):
    """-> (the n outputs, True if the guard tail still holds its NaN bit pattern)."""
    a = buf.cpu().numpy()
    return a[:n], bool(np.array_equal(a[n:].view(np.int32), np.full(GUARD, np.nan, dtype=F32).view(np.int32)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


# ------------------------------------------------------------------------------------------------------- pgasr_feat_frames
SENTINEL = F32(1e30)            # fills the slack of a wave row: a live frame that holds it has read past its utterance
FRAME_COUNTS = [[201], [399], [400], [401], [599], [600], [1000], [51400], [51400, 201, 600]]


def frames_case(ns):
    rng = np.random.default_rng(1000 + sum(ns))
    stride = (max(ns) + 3) // 4 * 4 + 8                         # wider than the longest row
    wave = np.full((len(ns), stride), SENTINEL, dtype=F32)
    for b, n in enumerate(ns):
        wave[b, :n] = rng.uniform(-1.0, 1.0, n)
    return wave


def frames_expected(x):
    """-> (x[reflect(t * 200 - 200 + k)] * hann64[k], |x[reflect(..)]|), both (T, 400) fp64; the reflect rule of power_spectrogram."""
    xp = np.pad(x.astype(np.float64), (N_FFT // 2, N_FFT // 2), mode="reflect")
    idx = np.arange(fr.n_frames(x.shape[0]))[:, None] * HOP + np.arange(N_FFT)[None, :]
    return xp[idx] * fr.hann_periodic()[None, :], np.abs(xp[idx])


@pytest.mark.parametrize("ns", FRAME_COUNTS, ids=lambda ns: "-".join(map(str, ns)))
def test_frames_reflect_window_and_padding(lib, ns):
    """|frame - x[i] hann64[k]| <= 2e-6 |x[i]|: the fp32 window 0.5 - 0.5 cosf(2 pi k / 400) carries about 5e-7 absolute error
    (argument rounding, cosf, one subtract, one multiply); the bound is 4 times that."""
    wave = frames_case(ns)
    B, stride = wave.shape
    nf = [fr.n_frames(n) for n in ns]
    Tmax = max(nf)
    buf = _out(B * Tmax * N_FFT)
    _run(lib.pgasr_feat_frames, wave, _i32(ns), _i32(nf), B, stride, Tmax, buf)
    got, guard_ok = _split(buf, B * Tmax * N_FFT)
    got = got.reshape(B, Tmax, N_FFT)
    assert guard_ok
    worst = 0.0
    for b, n in enumerate(ns):
        want, mag = frames_expected(wave[b, :n])
        live = got[b, :nf[b]].astype(np.float64)
        assert np.isfinite(live).all() and np.abs(live).max() <= 1.0          # neither the NaN pre-fill nor the sentinel
        err = np.abs(live - want)
        worst = max(worst, float((err / np.maximum(mag, 1e-300)).max()))
        assert (err <= 2e-6 * mag).all(), (b, n, worst)
        assert not _bits(got[b, nf[b]:]).any()                                 # rows past the utterance: +0.0 exactly
    print(f"frames {ns}: worst |err| / |x[i]| = {worst:.3e} (bound 2e-6)")


# -------------------------------------------------------------------------------------------------------- pgasr_feat_power
@pytest.mark.parametrize("rows", [1, 3, 257])
def test_power_every_row_and_nothing_behind_the_last(lib, rows):
    """|power - (re^2 + im^2)| <= 4e-7 (re^2 + im^2): two roundings of re * re + im * im, contracted or not, and a margin of 2.
    rows * 201 is no multiple of 256 for any of these, so the last workgroup is cut by the i >= rows * 201 guard."""
    assert (rows * N_BINS) % 256 != 0
    rng = np.random.default_rng(rows)
    spec = rng.standard_normal((rows, 2 * N_BINS)).astype(F32)
    if rows >= 3:
        spec[1] = 0.0
        spec[2] = (1e4 * rng.uniform(0.5, 2.0, 2 * N_BINS) * rng.choice([-1.0, 1.0], 2 * N_BINS)).astype(F32)
    buf = _out(rows * N_BINS)
    _run(lib.pgasr_feat_power, spec, rows, buf)
    got, guard_ok = _split(buf, rows * N_BINS)
    got = got.reshape(rows, N_BINS).astype(np.float64)
    assert guard_ok
    s = spec.astype(np.float64)
    want = s[:, :N_BINS] ** 2 + s[:, N_BINS:] ** 2
    err = np.abs(got - want)
    print(f"power rows={rows}: worst relative error {float((err / np.maximum(want, 1e-300)).max()):.3e} (bound 4e-7)")
    assert (err <= 4e-7 * want).all()
    assert (err[-1] <= 4e-7 * want[-1]).all() and want[-1].min() > 0          # the last row, cell by cell
    if rows >= 3:
        assert not _bits(got[1].astype(F32)).any() and want[2].min() > 1e7


# ----------------------------------------------------------------------------------------------------------- pgasr_feat_db
DB_SCALES = (1.0, 1e-6, 1e3, 1e-3)         # one loudness per utterance: a maximum shared across the batch is plainly wrong
DB_AMIN = float(F32(1e-10))


def db_lengths(Tmax):
    return [Tmax, 1, 9, Tmax - 1]


def db_case(Tmax, n_mels, peak, seed=0):
    """mel (4, Tmax, n_mels) fp32: live cells log-uniform over 1e-14 .. 1e6 times the utterance's scale, the utterance's maximum
    (2e6 times the scale) at ``peak`` -- "first", "last" (the last live cell) or "lane1023" (the last live cell whose index is
    1023 mod 1024, which thread 1023 alone visits; the last cell where there are fewer than 1024) -- and padded rows of 1e20 .. 2e20,
    above every live value of the batch."""
    rng = np.random.default_rng(seed + 7 * Tmax + n_mels)
    mel = np.empty((4, Tmax * n_mels), dtype=F32)
    for b, T in enumerate(db_lengths(Tmax)):
        n = T * n_mels
        mel[b, :n] = 10.0 ** rng.uniform(-14.0, 6.0, n) * DB_SCALES[b]
        at = {"first": 0, "last": n - 1, "lane1023": (n // 1024) * 1024 - 1 if n >= 1024 else n - 1}[peak]
        mel[b, at] = 2e6 * DB_SCALES[b]
        mel[b, n:] = 1e20 * rng.uniform(1.0, 2.0, Tmax * n_mels - n)
    return mel.reshape(4, Tmax, n_mels)


def db_expected(mel, lengths, top_db):
    """-> (max(10 log10(max(x, float32(1e-10))), own max - top_db) in fp64, the same expression in numpy float32, the share of
    clamped cells per utterance); padded rows as they came."""
    B, Tmax, n_mels = mel.shape
    want = mel.astype(np.float64).reshape(B, -1).copy()
    want32 = mel.reshape(B, -1).copy()
    shares = []
    for b, T in enumerate(lengths):
        n = T * n_mels
        db = 10.0 * np.log10(np.maximum(want[b, :n], DB_AMIN))
        want[b, :n] = np.maximum(db, db.max() - top_db)
        shares.append(float((db < db.max() - top_db).mean()))
        db32 = F32(10.0) * np.log10(np.maximum(want32[b, :n], F32(1e-10)), dtype=F32)
        want32[b, :n] = np.maximum(db32, db32.max() - F32(top_db))
    return want.reshape(mel.shape), want32.reshape(mel.shape), shares


def _check_db(lib, Tmax, n_mels, peak, top_db):
    lengths = db_lengths(Tmax)
    mel = db_case(Tmax, n_mels, peak)
    want, want32, shares = db_expected(mel, lengths, top_db)
    n_all = mel.size
    buf = _out(n_all)
    buf[:n_all] = torch.from_numpy(mel.reshape(-1))
    _run(lib.pgasr_feat_db, buf, _i32(lengths), 4, Tmax, n_mels, top_db)
    got, guard_ok = _split(buf, n_all)
    got = got.reshape(mel.shape)
    assert guard_ok
    dev_err = f32_err = 0.0
    for b, T in enumerate(lengths):
        assert np.array_equal(_bits(got[b, T:]), _bits(mel[b, T:])), b          # padded rows: bit for bit what they were
        dev_err = max(dev_err, float(np.abs(got[b, :T].astype(np.float64) - want[b, :T]).max()))
        f32_err = max(f32_err, float(np.abs(want32[b, :T].astype(np.float64) - want[b, :T]).max()))
    # The bound is measured, not derived: numpy's float32 evaluation of the same expression against fp64 on these inputs is the
    # floor, and the device gets 4 x that because its log10f is another implementation.  On these cases numpy's float32 error is
    # 1.34e-5 .. 1.62e-5 dB (half an ulp of values up to 100 dB is 3.8e-6), so the bound is 5.3e-5 .. 6.5e-5 dB; the MI355X's
    # own worst error on them is 1.12e-5 .. 1.37e-5 dB.  Both figures are printed.
    print(f"db Tmax={Tmax} n_mels={n_mels} peak={peak} top_db={top_db}: device {dev_err:.3e} dB, numpy float32 floor "
          f"{f32_err:.3e} dB, bound {4 * f32_err:.3e} dB; clamped shares {[round(s, 2) for s in shares]}")
    assert 1e-6 < f32_err < 1e-4                # a floor of 0 or of a whole dB would make the bound below meaningless
    assert dev_err <= 4.0 * f32_err, (dev_err, f32_err)
    return want, shares


@pytest.mark.parametrize("peak", ["first", "last", "lane1023"])
@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("Tmax", [9, 300])
def test_db_floors_each_utterance_at_its_own_maximum(lib, Tmax, n_mels, peak):
    """Lengths [Tmax, 1, 9, Tmax - 1]: one utterance with fewer than 1024 cells, one with many more; every utterance's own
    (max - 80 dB) cuts through its values, and the padding holds larger values than any live cell."""
    _, shares = _check_db(lib, Tmax, n_mels, peak, 80.0)
    assert all(0.2 <= s <= 0.8 for s in shares), shares            # the clamp neither idle nor everywhere


def test_db_honours_top_db(lib):
    want20, shares20 = _check_db(lib, 300, 80, "lane1023", 20.0)
    want80, _, shares80 = db_expected(db_case(300, 80, "lane1023"), db_lengths(300), 80.0)
    assert all(a > b + 0.2 and a < 1.0 for a, b in zip(shares20, shares80)), (shares20, shares80)
    assert np.abs(want20 - want80).max() == pytest.approx(60.0)


# ------------------------------------------------------------------------- pgasr_feat_deltas_stack and pgasr_feat_stack
STACK_LENGTHS = [[6, 1, 2, 3], [5, 4], [257, 1, 256, 255], [513, 300]]        # T = 1 .. 6 and 255, 256, 257, 513


def poisoned(lengths, C, seed):
    """(B, Tmax, C) fp32, NaN in every row t >= T of an utterance."""
    x = (10.0 * np.random.default_rng(seed).standard_normal((len(lengths), max(lengths), C))).astype(F32)
    for b, T in enumerate(lengths):
        x[b, T:] = np.nan
    return x


def _stacked(fn, x, lengths, rows_out, with_mask):
    B, Tmax, C = x.shape
    feat, mask = _out(B * rows_out * Tmax), _out(B * Tmax)
    _run(fn, x, _i32(lengths), B, Tmax, C, feat, mask if with_mask else None)
    f, f_guard = _split(feat, B * rows_out * Tmax)
    m, m_guard = _split(mask, B * Tmax)
    assert f_guard and m_guard
    if with_mask:
        want = (np.arange(Tmax)[None, :] < np.array(lengths)[:, None]).astype(F32)
        assert np.array_equal(_bits(m.reshape(B, Tmax)), _bits(want))          # exactly 1.0 / +0.0
    else:
        assert np.isnan(m).all()                                              # not written
    return f.reshape(B, rows_out, Tmax)


@pytest.mark.parametrize("C", [1, 40])
@pytest.mark.parametrize("lengths", STACK_LENGTHS, ids=lambda v: "-".join(map(str, v)))
def test_deltas_stack_edges_blocks_and_poisoned_padding(lib, lengths, C):
    """Each of the 3C rows against compute_deltas applied once and twice in fp64, within 2e-6 max|x| of its (b, c) row: about eight
    fp32 roundings weighted by coefficients that sum to 0.6 give about 3e-7; the bound is roughly 6 times that."""
    x = poisoned(lengths, C, seed=sum(lengths) + C)
    got = _stacked(lib.pgasr_feat_deltas_stack, x, lengths, 3 * C, True)
    assert np.array_equal(_bits(got), _bits(_stacked(lib.pgasr_feat_deltas_stack, x, lengths, 3 * C, False)))      # fmask = NULL
    worst = 0.0
    for b, T in enumerate(lengths):
        assert not _bits(got[b, :, T:]).any()                                  # +0.0 past the utterance, whatever the NaN rows held
        live = got[b, :, :T]
        assert np.isfinite(live).all()
        base = x[b, :T].T.astype(np.float64)                                   # (C, T)
        d1 = fr.compute_deltas(base)
        want = np.concatenate((base, d1, fr.compute_deltas(d1)), axis=0)
        assert np.array_equal(_bits(live[:C]), _bits(x[b, :T].T))              # the static rows are a copy
        scale = np.tile(np.abs(base).max(axis=1), 3)[:, None]
        err = np.abs(live.astype(np.float64) - want) / scale
        worst = max(worst, float(err.max()))
        assert (err <= 2e-6).all(), (b, T, worst)
        if T == 1:
            assert not _bits(live[C:]).any()                                   # one frame: both deltas exactly 0
    print(f"deltas {lengths} C={C}: worst |err| / max|x| = {worst:.3e} (bound 2e-6)")


@pytest.mark.parametrize("C", [1, 80])
@pytest.mark.parametrize("lengths", STACK_LENGTHS, ids=lambda v: "-".join(map(str, v)))
def test_stack_is_the_bit_exact_transpose(lib, lengths, C):
    x = poisoned(lengths, C, seed=3 * sum(lengths) + C)
    want = np.zeros((len(lengths), C, max(lengths)), dtype=F32)
    for b, T in enumerate(lengths):
        want[b, :, :T] = x[b, :T].T
    for with_mask in (True, False):
        got = _stacked(lib.pgasr_feat_stack, x, lengths, C, with_mask)
        assert np.array_equal(_bits(got), _bits(want)), with_mask
