"""SpecAugment without a GPU: the export and binding of pgasr_spec_augment, its refusals (no device is touched), the policy's
validation, and the properties of the numpy statement of the masking function (tests/specaug_ref.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import specaug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")

# the maintainer's case: seed 4, offsets 1 and 2, ids 0..7, F = 80
SEED, F = 4, 80
LENGTHS = (60, 57, 54, 51, 48, 1, 0, 33)
POLICY = dict(freq_masks=2, freq_width=27, time_masks=2, time_width=20, time_ratio=0.2, fill="row_mean")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.pgasr_spec_augment.restype = ctypes.c_int
    return lib


def test_abi_export_and_binding(lib):
    from policy_gradient_asr_amd import _lib
    assert hasattr(lib, "pgasr_spec_augment") and "pgasr_spec_augment" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["pgasr_spec_augment"]
    assert res is ctypes.c_int
    header = open(os.path.join(ROOT, "include", "pgasr_hip.h")).read()
    decl = re.search(r"int pgasr_spec_augment\((.*?)\);", header, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert len(decl.split(",")) == len(args) == 18
    lib.pgasr_abi_version.restype = ctypes.c_int
    assert lib.pgasr_abi_version() == 7


def test_refusals_need_no_gpu(lib):
    INVALID, UNSUPPORTED = 1, 4
    p, fake = ctypes.c_void_p, 0x1000         # never dereferenced: every call below is refused before any HIP call

    def call(x=fake, lengths=fake, out=fake, B=2, F=8, T=16, n_freq=2, freq_width=3, n_time=2, time_width=4, ratio=1.0, fill=0):
        return lib.pgasr_spec_augment(p(x), p(lengths), p(None), ctypes.c_int(0), B, F, T, n_freq, freq_width, n_time, time_width,
                                      ctypes.c_float(ratio), fill, ctypes.c_ulonglong(4), ctypes.c_uint(1), p(out), p(None), p(None))
    for missing in ("x", "lengths", "out"):
        assert call(**{missing: None}) == INVALID, missing
    for bad in ({"B": 0}, {"F": 0}, {"T": 0}, {"B": -1}, {"n_freq": -1}, {"n_time": -1}, {"freq_width": -1}, {"time_width": -1},
                {"ratio": 0.0}, {"ratio": -0.5}, {"ratio": 1.5}, {"ratio": float("nan")}, {"fill": 2}, {"fill": -1}):
        assert call(**bad) == INVALID, bad
    assert call(n_freq=9) == UNSUPPORTED and call(n_time=9) == UNSUPPORTED
    # a bad argument is INVALID_ARG even beside too many masks, and nothing is read from the null pointer first
    assert call(n_freq=9, x=None) == INVALID


def test_policy_validation_and_state():
    from policy_gradient_asr_amd.features import SpecAugment
    d = SpecAugment()
    assert d.state() == dict(freq_masks=2, freq_width=27, time_masks=2, time_width=100, time_ratio=1.0, fill="row_mean")
    for bad in (dict(freq_masks=-1), dict(time_masks=-1), dict(freq_width=-1), dict(time_width=-3), dict(freq_masks=9),
                dict(time_masks=9), dict(time_ratio=0), dict(time_ratio=0.0), dict(time_ratio=1.5), dict(time_ratio=float("nan")),
                dict(time_ratio=1e-60), dict(fill="median"), dict(freq_width=2 ** 31)):
        with pytest.raises(ValueError, match="SpecAugment"):
            SpecAugment(**bad)
    with pytest.raises(ValueError, match="<= 8"):        # the limit is named
        SpecAugment(freq_masks=9)
    for bad in (dict(freq_masks=True), dict(time_masks=False), dict(freq_width=2.0), dict(time_width="7"), dict(time_ratio=True),
                dict(time_ratio="0.5")):
        with pytest.raises(TypeError, match="SpecAugment"):
            SpecAugment(**bad)
    a = SpecAugment(2, 27, 2, 20, 0.2)
    assert (a.freq_masks, a.freq_width, a.time_masks, a.time_width, a.time_ratio, a.fill) == (2, 27, 2, 20, 0.2, "row_mean")
    assert SpecAugment.from_state(a.state()) == a and SpecAugment.from_state(a.state()).state() == a.state()
    assert SpecAugment(time_ratio=None).time_ratio == 1.0 and SpecAugment(0, 0, 8, 0, 1, "zero").time_masks == 8
    assert SpecAugment(np.int64(3)).freq_masks == 3 and type(SpecAugment(np.int64(3)).freq_masks) is int
    with pytest.raises(AttributeError):
        a.freq_masks = 3
    with pytest.raises(ValueError):
        SpecAugment.from_state(dict(a.state(), median=1))
    # off the device it refuses, it does not fall back
    import torch
    from policy_gradient_asr_amd._lib import PgasrError
    with pytest.raises(PgasrError):
        a(torch.zeros(1, 4, 8), [8], seed=0, offset=1)


def test_coerce_takes_a_policy_a_dict_or_none():
    from policy_gradient_asr_amd.features import SpecAugment
    for bad in ("yes", 1, True, [2, 27, 2, 100]):
        with pytest.raises(TypeError, match="spec_augment"):
            SpecAugment.coerce(bad)
    with pytest.raises(ValueError, match="SpecAugment"):
        SpecAugment.coerce({"freq_masks": 9})
    a = SpecAugment(1, 5, 1, 10, 0.5, "zero")
    assert SpecAugment.coerce(None) is None and SpecAugment.coerce(a) is a and SpecAugment.coerce(a.state()) == a


def _check_intervals(iv, lengths, ids, pol, F):
    nF, Wf, nT, Wt, p, _ = R.fields(pol)
    for b, (n, uid) in enumerate(zip(lengths, ids)):
        if uid < 0:
            assert not iv[b].any()
            continue
        for m, (s, w) in enumerate(iv[b].tolist()):
            span = F if m < nF else n
            W = min(Wf, F) if m < nF else R.time_width_cap(Wt, p, n)
            assert 0 <= w <= W and 0 <= s and s + w <= span, (b, m, s, w, W, span)


def test_reference_on_the_maintainers_case():
    ids = list(range(8))
    iv1 = R.mask_intervals(LENGTHS, ids, POLICY, F, SEED, 1)
    iv2 = R.mask_intervals(LENGTHS, ids, POLICY, F, SEED, 2)
    assert iv1.shape == iv2.shape == (8, 4, 2) and iv1.dtype == np.int32
    _check_intervals(iv1, LENGTHS, ids, POLICY, F)
    _check_intervals(iv2, LENGTHS, ids, POLICY, F)
    # the quoted draws: offset 2, id 0 has the overlapping frequency masks [4,31) (the full width 27) and [3,27)
    assert iv2[0, 0].tolist() == [4, 27] and iv2[0, 1].tolist() == [3, 24]
    assert (np.concatenate((iv1, iv2))[:, :, 1] == 0).any()              # zero-width masks occur
    for iv in (iv1, iv2):                                                # lengths 1 and 0: 0.2 * len truncates to 0
        assert (iv[5, 2:, 1] == 0).all() and (iv[6, 2:, 1] == 0).all() and (iv[6, 2:, 0] == 0).all()
    # the time cap: min(20, len, int(0.2 * len))
    assert [R.time_width_cap(20, np.float32(0.2), n) for n in LENGTHS] == [12, 11, 10, 10, 9, 0, 0, 6]
    assert R.time_width_cap(100, np.float32(1.0), 60) == 60 and R.time_width_cap(20, np.float32(1.0), 60) == 20
    # other offsets and other ids give other intervals
    assert not np.array_equal(iv1, iv2)
    assert not np.array_equal(iv1[0, :2], iv1[1, :2])
    shifted = R.mask_intervals(LENGTHS, [i + 8 for i in ids], POLICY, F, SEED, 1)
    assert not np.array_equal(shifted, iv1)
    assert np.array_equal(R.mask_intervals(LENGTHS[::-1], ids[::-1], POLICY, F, SEED, 1), iv1[::-1])    # a function of the id, not of the row


def test_reference_properties_on_random_triples():
    rng = np.random.default_rng(11)
    lengths = rng.integers(0, 1200, size=200).tolist()
    ids = rng.integers(0, 2 ** 31 - 1, size=200).tolist()
    ids[::17] = [-1] * len(ids[::17])
    for pol in (POLICY, dict(freq_masks=8, freq_width=200, time_masks=8, time_width=100, time_ratio=None, fill="zero"),
                dict(freq_masks=1, freq_width=0, time_masks=3, time_width=7, time_ratio=0.05, fill="zero")):
        for k in range(0, 200, 50):
            offset = int(rng.integers(0, 2 ** 32))
            sl = slice(k, k + 50)
            iv = R.mask_intervals(lengths[sl], ids[sl], pol, F, SEED, offset)
            _check_intervals(iv, lengths[sl], ids[sl], pol, F)


def test_reference_apply():
    rng = np.random.default_rng(5)
    T = 60
    x = rng.standard_normal((8, F, T)).astype(np.float32)
    for b, n in enumerate(LENGTHS):
        x[b, :, n:] = 0
    ids = [0, 1, -1, 3, 4, 5, 6, 7]
    for mode in ("row_mean", "zero"):
        pol = dict(POLICY, fill=mode)
        out, fill = R.apply(x, LENGTHS, ids, pol, SEED, 2)
        iv = R.mask_intervals(LENGTHS, ids, pol, F, SEED, 2)
        assert out.dtype == np.float32 and not np.array_equal(out, x)
        for b, n in enumerate(LENGTHS):
            assert np.array_equal(out[b, :, n:], x[b, :, n:])            # frames >= len: untouched
        assert np.array_equal(out[2], x[2]) and np.array_equal(out[6], x[6])      # id -1, length 0
        # utterance 0: rows 3..30 are masked over all real frames, and so are frames [48,55) and [35,39) of every row
        want = fill[0][:, None] if mode == "row_mean" else 0.0
        assert np.array_equal(out[0, 3:31, :60], np.broadcast_to(want, (F, 60))[3:31])
        assert np.array_equal(out[0, :, 48:55], np.broadcast_to(want, (F, 60))[:, 48:55])
        keep = np.ones((F, T), bool); keep[3:31] = False; keep[:, 48:55] = False; keep[:, 35:39] = False
        assert np.array_equal(out[0][keep], x[0][keep])
        assert iv[0].tolist() == [[4, 27], [3, 24], [48, 7], [35, 4]]
        np.testing.assert_allclose(fill[0], x[0, :, :60].astype(np.float64).mean(axis=1), rtol=1e-6, atol=1e-7)
    # no masks of either kind: the identity
    ident = dict(POLICY, freq_masks=0, time_masks=0)
    assert np.array_equal(R.apply(x, LENGTHS, ids, ident, SEED, 1)[0], x)
    assert R.mask_intervals(LENGTHS, ids, ident, F, SEED, 1).shape == (8, 0, 2)


def test_counters_are_disjoint_from_the_samplers():
    """The samplers' counters are (t * stride + id, offset, 0 or 1, k) (include/pgasr_hip.h); the masks' are (id, offset, 2 or 3, m):
    word 2 separates them under one seed and one offset, and the blocks differ accordingly."""
    assert {R.DOM_FREQ, R.DOM_TIME} == {2, 3} and not {R.DOM_FREQ, R.DOM_TIME} & {0, 1}
    blocks = {(dom, m): R.philox_words(5, 1, dom, m, SEED) for dom in (0, 1, 2, 3) for m in range(8)}
    assert len(set(blocks.values())) == len(blocks)
