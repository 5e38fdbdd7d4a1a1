"""Sample-rate conversion and speed perturbation without a GPU: the numpy statement of the resampling function reproduces tones,
the package's filter tables against the statement's, the output lengths, the SpeedPerturb policy and its draws, the export, binding
and refusals of pgasr_resample (no device is touched), and the defaults of the data layer."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")

# ratio L / M and the input rate the tone is synthesised at
TONE_CASES = [((1, 3), 48000), ((160, 441), 44100), ((10, 9), 16000), ((10, 11), 16000), ((2, 1), 8000)]
RATIOS = [r for r, _ in TONE_CASES] + [(3, 1), (1, 16), (16, 1), (8, 33), (1, 1)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.pgasr_resample.restype = ctypes.c_int
    return lib


def test_reference_reproduces_tones():
    """A 0.5 s tone at 200 Hz and at 1 kHz, resampled by the statement, against the same tone synthesised at the output rate; 200
    samples at each end (the filter's run-in) are ignored.  The bound is a property of the filter (6 zero crossings, Hann window)."""
    worst = {}
    for (L, M), rate in TONE_CASES:
        n = rate // 2
        for f in (200.0, 1000.0):
            x = np.sin(2.0 * np.pi * f * np.arange(n, dtype=np.float64) / rate).astype(np.float32)
            y = R.resample(x, L, M)
            assert y.dtype == np.float32 and y.shape[0] == R.length(n, L, M)
            want = np.sin(2.0 * np.pi * f * np.arange(y.shape[0], dtype=np.float64) * M / (L * rate))
            err = float(np.abs(y.astype(np.float64) - want)[200:-200].max())
            worst[(L, M, int(f))] = err
    print("worst tone error per (L, M, Hz):", {k: f"{v:.2e}" for k, v in worst.items()})
    print("worst of all: {:.2e}".format(max(worst.values())))
    assert max(worst.values()) <= 2e-3, worst


def test_filter_tables_against_the_statement():
    from policy_gradient_asr_amd.features import resample_filter
    for L, M in RATIOS:
        h, base, half = resample_filter(L, M)
        h_ref, base_ref, half_ref = R.filter_table(L, M)
        assert half == half_ref and h.shape == h_ref.shape == (L, 2 * half + 1), (L, M)
        assert h.dtype == np.float32 and base.dtype == np.int32 and np.array_equal(base, base_ref), (L, M)
        # values of magnitude <= 1 rounded to fp32 from two fp64 evaluations that may differ in the last place
        assert np.abs(h.astype(np.float64) - h_ref.astype(np.float64)).max() <= 2.0 ** -24, (L, M)
        # DC: the taps of a phase sample fc * sinc(fc d) * window(d) at unit spacing, whose integral over d is the filter's gain at
        # 0 Hz, 1; the statement's own tables say how close the sampled sum comes, and the package must say the same
        dc_ref = h_ref.astype(np.float64).sum(axis=1)
        dc = h.astype(np.float64).sum(axis=1)
        assert np.abs(dc_ref - 1.0).max() <= 1e-3, (L, M, dc_ref)
        assert np.abs(dc - dc_ref).max() <= h.shape[1] * 2.0 ** -24, (L, M)
        assert resample_filter(L, M)[0] is h                          # cached
        assert not h.flags.writeable and not base.flags.writeable      # .. so nobody may edit it
    assert resample_filter(1, 16)[0].shape[1] == 195 and resample_filter(160, 441)[0].shape == (160, 35)
    for bad in ((2, 4), (0, 1), (1, 0), (1025, 1024), (17, 1), (1, 17)):
        with pytest.raises(ValueError):
            resample_filter(*bad)


def test_resample_length():
    from policy_gradient_asr_amd.features import resample_length
    for L, M in RATIOS:
        for n in list(range(2001)) + [2 ** 31 - 1]:
            got = resample_length(n, L, M)
            assert got == -((-n * L) // M) == R.length(n, L, M), (n, L, M)       # ceil in python integers
    assert resample_length(2 ** 31 - 1, 16, 1) == 16 * (2 ** 31 - 1)             # no overflow
    assert resample_length(np.int32(2 ** 31 - 1), np.int32(1024), np.int32(1023)) == ((2 ** 31 - 1) * 1024 + 1022) // 1023
    assert isinstance(resample_length(np.int32(7), 1, 3), int)


def test_speed_perturb_draws():
    from policy_gradient_asr_amd.features import SpeedPerturb
    sp = SpeedPerturb()
    assert sp.factors == ((9, 10), (1, 1), (11, 10))
    seed = 0x1234567887654321
    for offset in (0, 1, 2 ** 32 - 1):
        for u in list(range(60)) + [2 ** 31 - 1, 2 ** 31 - 2, 12345678, 99999]:
            assert sp.draw(u, seed, offset) == R.speed_draw(u, 3, seed, offset), (u, offset)
    ids = list(range(64))
    ratios = sp.ratios(ids, 5, 2)
    assert ratios == [((10, 9), (1, 1), (10, 11))[R.speed_draw(u, 3, 5, 2)] for u in ids]         # factor p/q is the ratio q/p
    assert sp.ratios(ids[::-1], 5, 2) == ratios[::-1]                                            # a function of the id, not of the row
    assert sp.ratios(ids, 5, 3) != ratios and sp.ratios(ids, 6, 2) != ratios
    counts = np.bincount([sp.draw(u, 7, 1) for u in range(3000)], minlength=3)
    print("draws per factor over 3000 ids:", counts.tolist())
    assert counts.sum() == 3000 and (np.abs(counts - 1000) <= 130).all(), counts                  # 5 sigma of Binomial(3000, 1/3)


def test_speed_perturb_policy():
    from fractions import Fraction
    from policy_gradient_asr_amd.features import SpeedPerturb
    sp = SpeedPerturb((0.9, 1.0, 1.1))
    assert sp == SpeedPerturb() and hash(sp) == hash(SpeedPerturb())
    assert SpeedPerturb.from_state(sp.state()) == sp and SpeedPerturb.from_state(sp.state()).state() == sp.state()
    assert sp.state() == {"factors": [[9, 10], [1, 1], [11, 10]]}
    assert SpeedPerturb([Fraction(19, 20), (21, 20), 1]).factors == ((19, 20), (21, 20), (1, 1))
    assert SpeedPerturb([2.0, 0.5, 16.0, 1 / 16]).factors == ((2, 1), (1, 2), (16, 1), (1, 16))
    assert SpeedPerturb([0.9]) != sp and SpeedPerturb.coerce(None) is None and SpeedPerturb.coerce(sp) is sp
    assert SpeedPerturb.coerce(sp.state()) == sp and SpeedPerturb.coerce((0.9, 1.0, 1.1)) == sp
    for bad in ([], (), [17.0], [1 / 17], [0.0], [-0.9], [float("nan")], [float("inf")], [0.9001234567], [(1025, 1024)], [(0, 1)]):
        with pytest.raises(ValueError, match="SpeedPerturb"):
            SpeedPerturb(bad)
    for bad in (0.9, "0.9", [True], ["0.9"], [None]):
        with pytest.raises(TypeError, match="SpeedPerturb"):
            SpeedPerturb(bad)
    with pytest.raises(TypeError, match="speed_perturb"):
        SpeedPerturb.coerce(1.1)
    with pytest.raises(ValueError):
        SpeedPerturb.from_state({"factors": [0.9], "seed": 1})
    with pytest.raises(AttributeError):
        sp.factors = ()


def test_abi_export_and_binding(lib):
    from policy_gradient_asr_amd import _lib
    assert hasattr(lib, "pgasr_resample") and "pgasr_resample" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["pgasr_resample"]
    assert res is ctypes.c_int
    header = open(os.path.join(ROOT, "include", "pgasr_hip.h")).read()
    assert re.search(r"#define PGASR_ABI_VERSION 7\b", header)
    decl = re.search(r"int pgasr_resample\((.*?)\);", header, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert len(decl.split(",")) == len(args) == 13
    lib.pgasr_abi_version.restype = ctypes.c_int
    assert lib.pgasr_abi_version() == 7


def test_refusals_need_no_gpu(lib):
    INVALID, UNSUPPORTED = 1, 4
    p, fake = ctypes.c_void_p, 0x1000         # never dereferenced: every call below is refused before any HIP call

    def desc(*rows):
        return (ctypes.c_int32 * (4 * len(rows)))(*[v for row in rows for v in row])

    def w_of(L, M):
        return 2 * int(math.ceil(6 / (0.99 * min(1.0, L / M)))) + 1

    def call(wave=fake, n_in=fake + 0x100, tables=fake + 0x200, bases=fake + 0x300, out=fake + 0x400, n_out=fake + 0x500,
             B=2, in_stride=1000, out_stride=4000, rows=((1, 3, 39, 0),), n_ratios=None, no_desc=False):
        d = desc(*rows)
        return lib.pgasr_resample(p(wave), in_stride, p(n_in), B, p(None), len(rows) if n_ratios is None else n_ratios,
                                  None if no_desc else d, p(tables), p(bases), p(out), out_stride, p(n_out), p(None))
    assert w_of(1, 3) == 39 and w_of(2, 1) == 15 and w_of(1, 16) == 195
    for missing in ("wave", "n_in", "tables", "bases", "out", "n_out"):
        assert call(**{missing: None}) == INVALID, missing
    assert call(no_desc=True) == INVALID
    assert call(out=fake) == INVALID                                   # out == wave
    for bad in ({"B": 0}, {"B": -1}, {"in_stride": 0}, {"out_stride": 0}, {"in_stride": -4}, {"n_ratios": 0}, {"n_ratios": -1}):
        assert call(**bad) == INVALID, bad
    nine = tuple((1, 3, 39, 0) for _ in range(9))
    assert call(rows=nine) == UNSUPPORTED                              # at most 8 ratios per call
    assert call(rows=nine, wave=None) == INVALID                       # .. but a bad argument beside it is INVALID_ARG
    for row in ((0, 3, 39, 0), (1, 0, 39, 0), (-1, 3, 39, 0), (2, 6, 39, 0), (4, 2, 15, 0)):      # L or M < 1; not reduced
        assert call(rows=(row,)) == INVALID, row
    for L, M in ((1025, 1024), (1024, 1025), (17, 1), (1, 17), (1025, 64)):
        assert call(rows=((L, M, w_of(L, M), 0),), out_stride=2 ** 30) == UNSUPPORTED, (L, M)
    for row in ((1, 3, 37, 0), (1, 3, 41, 0), (1, 3, 15, 0), (2, 1, 39, 0), (1, 3, 0, 0), (1, 3, 39, -4)):      # W of another ratio; offset
        assert call(rows=(row,)) == INVALID, row
    assert call(rows=((1, 3, 39, 0), (2, 1, 14, 0))) == INVALID        # the second descriptor is checked like the first
    # room for what the largest ratio makes of in_stride samples: 2000 at 2/1, 16000 at 16/1
    assert call(rows=((2, 1, 15, 0),), out_stride=1999) == INVALID
    assert call(rows=((1, 3, 39, 0), (2, 1, 15, 640)), out_stride=1999) == INVALID
    assert call(rows=((16, 1, 15, 0),), out_stride=15999) == INVALID
    assert call(rows=((1, 3, 39, 0),), out_stride=333) == INVALID


def test_defaults_unchanged():
    import torch
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd._lib import PgasrError
    from policy_gradient_asr_amd.data import Indexed, collate_custom, extract_feats
    from policy_gradient_asr_amd.features import Resample, SpeedPerturb
    g = torch.Generator().manual_seed(3)
    char2ind = {"_": 0, "a": 1, "b": 2}
    items = [{"feat": torch.randn(5, n, generator=g), "trans": "ab"[:k], "charmap": char2ind} for n, k in ((7, 1), (4, 2), (9, 2))]
    feat, fmask = extract_feats(items)
    feat2, fmask2 = extract_feats(items, target_rate=None, speed_perturb=None, seed=0, offset=0)
    assert torch.equal(feat, feat2) and torch.equal(fmask, fmask2) and feat.shape == (3, 5, 9)
    feat3, _ = extract_feats(items, target_rate=16000, seed=5, offset=2)          # precomputed features have no rate
    assert torch.equal(feat, feat3)
    a, b = collate_custom(items), collate_custom(items, target_rate=None, speed_perturb=None, seed=0, offset=0)
    assert sorted(a) == sorted(b) == ["feat", "fmask", "tmask", "trans"] and all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(ValueError, match="precomputed"):
        extract_feats(items, speed_perturb=SpeedPerturb())
    ds = Indexed(items)
    assert len(ds) == 3 and [ds[i]["idx"] for i in range(3)] == [0, 1, 2] and ds[torch.tensor(2)]["idx"] == 2
    assert ds[1]["feat"] is items[1]["feat"] and "idx" not in items[1]
    # off the device the product refuses, it does not fall back
    with pytest.raises(PgasrError):
        hipops.resample(torch.zeros(2, 64), torch.tensor([64, 64], dtype=torch.int32), [(1, 3)])
    with pytest.raises(PgasrError):
        Resample("cpu")
