"""The feature front end (N3) on a GPU-less host: the five ``pgasr_feat_*`` entry points are bound with the header's argument
counts and reject invalid arguments before any device work; the float32 restatement beside the tests (features_f32_ref.py) still
gives the floors it records, on inputs that are what they claim to be; ``read_wav`` reads what its docstring says and refuses the
rest."""
import os
import re
import struct
import wave

import numpy as np
import pytest
import torch

import features_f32_ref as f32
from oracle import features_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
ENTRY_POINTS = ("pgasr_feat_frames", "pgasr_feat_power", "pgasr_feat_db", "pgasr_feat_deltas_stack", "pgasr_feat_stack")
OK_, INVALID_ARG = 0, 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def test_feat_signatures_have_the_headers_argument_counts(lib):
    from policy_gradient_asr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in ENTRY_POINTS] == [8, 4, 7, 8, 8]


def _rejected(call, good, bad):
    """Every (position, value) of ``bad`` put into the argument list ``good`` gives PGASR_ERR_INVALID_ARG."""
    for pos, value in bad:
        args = list(good)
        args[pos] = value
        assert call(*args) == INVALID_ARG, (call.__name__, pos, value)


def test_invalid_arguments_are_rejected_without_a_device(lib):
    """Every call below returns before anything is launched: the dummy addresses are never dereferenced."""
    p, big = 0x1000, 65536
    ints = (0, -1)
    # wave, n_samples, n_frames, B, wave_stride, Tmax, frames, stream
    _rejected(lib.pgasr_feat_frames, (p, p, p, 2, 1000, 6, p, None),
              [(i, None) for i in (0, 1, 2, 6)] + [(i, v) for i in (3, 4, 5) for v in ints]
              + [(4, -(1 << 40))])
    assert lib.pgasr_feat_frames(p, p, p, 1 << 16, 1000, 1 << 15, p, None) == INVALID_ARG     # B * Tmax = 2^31 rows: past the grid
    assert lib.pgasr_feat_frames(p, p, p, 2147483647, 1000, 2147483647, p, None) == INVALID_ARG
    # spec, rows, power, stream
    _rejected(lib.pgasr_feat_power, (p, 3, p, None), [(0, None), (2, None), (1, 0), (1, -1), (1, -(1 << 40))])
    # mel, n_frames, B, Tmax, n_mels, top_db, stream
    _rejected(lib.pgasr_feat_db, (p, p, 2, 6, 80, 80.0, None),
              [(0, None), (1, None)] + [(i, v) for i in (2, 3, 4) for v in ints]
              + [(5, v) for v in (0.0, -0.0, -80.0, float("nan"), float("-inf"), 1e-60)])    # 1e-60 is 0 as a float
    # mfcc / x, n_frames, B, Tmax, n_mfcc / C, feat, fmask, stream -- fmask (position 6) alone may be NULL
    for call in (lib.pgasr_feat_deltas_stack, lib.pgasr_feat_stack):
        _rejected(call, (p, p, 2, 6, 40, p, p, None),
                  [(0, None), (1, None), (5, None)] + [(i, v) for i in (2, 3, 4) for v in ints] + [(2, big), (4, big)])
        _rejected(call, (p, p, 2, 6, 40, p, None, None), [(0, None), (1, None), (5, None), (2, big), (4, big), (3, 0)])


def test_the_float32_restatement_reproduces_its_recorded_floors():
    """The table of features_f32_ref.py, re-measured: each figure within 10 %.  The GPU test's tolerances are 4 x these."""
    assert set(f32.FLOORS) == set(f32.CASES) and len(f32.CASES) == 12
    for name in f32.CASES:
        for kind, recorded in zip(f32.KINDS, f32.FLOORS[name]):
            got = f32.measure(name, kind)
            print(f"{name:13s} {kind:9s} floor {got:.3e} (recorded {recorded:.3e})")
            assert abs(got - recorded) <= 0.1 * recorded, (name, kind, got, recorded)
            assert f32.tolerance(name, kind) == max(2e-3, 4.0 * recorded)
    # the docstring's table is the dictionary
    for name, (a, b) in f32.FLOORS.items():
        row = re.search(r"^\s+%s\s+(\S+)\s+(\S+)\s" % re.escape(name), f32.__doc__, flags=re.M)
        assert row and float(row.group(1)) == a and float(row.group(2)) == b, name


def test_the_cases_are_what_they_claim():
    lengths = {name: [w.shape[0] for w in f32.case(name)] for name in f32.CASES}
    for name, ns in lengths.items():
        waves = f32.case(name)
        assert min(ns) > 200, name                                  # reflect-centred framing needs more than n_fft / 2
        assert all(w.dtype == np.float32 and w.ndim == 1 and np.isfinite(w).all() for w in waves), name
        assert all(np.array_equal(a, b) for a, b in zip(waves, f32.case(name))), name            # seeded
    for name, least in f32.CLAMPED_SHARE.items():
        share = f32.clamped_share(f32.case(name)[0])
        print(f"{name}: {100 * share:.0f} % of the log-mel cells on the top_db clamp")
        assert least <= share < 1.0, (name, share)
    assert f32.clamped_share(f32.case("tone_1e-5")[0]) == 0.0       # the 1e-10 floor, not the clamp
    assert lengths["short"] == [201, 399, 400, 599, 600, 800, 1000]
    assert [fr.n_frames(n) for n in lengths["short"]] == [2, 2, 3, 3, 4, 5, 6]
    assert fr.n_frames(lengths["clipped_T261"][0]) == 261
    z = f32.case("zeros_tone")[0]
    assert not z[:3000].any() and not z[-2000:].any() and z[3000:-2000].any()
    z = f32.case("zeros_noise")[0]
    assert not z[:3000].any() and not z[-2000:].any()
    assert np.count_nonzero(f32.case("click")[0]) == 1
    g = f32.case("int16")[0].astype(np.float64) * 32768.0
    assert np.array_equal(g, np.round(g)) and np.abs(g).max() <= 32767
    assert set(np.unique(f32.case("square")[0])) == {-1.0, 1.0}
    assert np.abs(f32.case("clipped_T261")[0]).max() == 1.0
    loud, quiet = f32.case("loud_quiet")
    assert np.array_equal(quiet, loud * np.float32(1e-3))
    assert abs(float(f32.case("dc")[0].mean()) - 0.5) < 1e-4


def test_the_float32_pieces_restate_the_oracles():
    assert np.abs(f32.hann32().astype(np.float64) - fr.hann_periodic()).max() < 5e-7
    x = np.random.default_rng(3).standard_normal((3, 7)).astype(np.float32)
    assert np.abs(f32.deltas32(x) - fr.compute_deltas(x.astype(np.float64))).max() < 1e-6
    one = np.full((2, 1), 3.3, dtype=np.float32)
    assert not f32.deltas32(one).any()
    a, b = x, np.random.default_rng(4).standard_normal((7, 5)).astype(np.float32)
    assert np.abs(f32.matmul32(a, b) - a.astype(np.float64) @ b.astype(np.float64)).max() < 1e-5
    with pytest.raises(ValueError):
        f32.mel_db(np.zeros(200, dtype=np.float32), 80)


def _write(path, width, channels, frames, rate=16000):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels); f.setsampwidth(width); f.setframerate(rate)
        f.writeframes(frames)
    return str(path)


def test_read_wav_pcm16_mono_stereo_and_full_scale(tmp_path):
    from policy_gradient_asr_amd.features import read_wav
    s = np.array([0, 1, -1, 32767, -32768, 12345, -20000], dtype="<i2")
    x, sr = read_wav(_write(tmp_path / "m.wav", 2, 1, s.tobytes(), rate=8000))
    assert sr == 8000 and x.dtype == torch.float32 and x.ndim == 1
    assert x.tolist() == [0.0, 2.0 ** -15, -2.0 ** -15, 32767 / 32768, -1.0, 12345 / 32768, -20000 / 32768]       # exact in fp32
    other = np.array([7, 7, 7, 7, 7, 7, 7], dtype="<i2")
    x2, sr2 = read_wav(_write(tmp_path / "s.wav", 2, 2, np.stack((s, other), axis=1).tobytes()))
    assert sr2 == 16000 and torch.equal(x2, x)                                                  # the first channel
    x0, _ = read_wav(_write(tmp_path / "none.wav", 2, 1, b""))
    assert x0.dtype == torch.float32 and tuple(x0.shape) == (0,)                                # a header and no frames


def test_read_wav_pcm32(tmp_path):
    from policy_gradient_asr_amd.features import read_wav
    s = np.array([0, 1 << 30, -(1 << 30), -(1 << 31), (1 << 31) - 1, 3 << 8, 123456789], dtype="<i4")
    x, sr = read_wav(_write(tmp_path / "p32.wav", 4, 1, s.tobytes()))
    assert sr == 16000 and x.dtype == torch.float32
    # the integer rounded to fp32 once, over 2^31: the largest integer rounds up to 1.0
    assert x.tolist() == [0.0, 0.5, -0.5, -1.0, 1.0, 3 * 2.0 ** -23, float(np.float32(123456789)) / 2.0 ** 31]


@pytest.mark.parametrize("width", [1, 3])
def test_read_wav_refuses_8_and_24_bit(tmp_path, width):
    from policy_gradient_asr_amd.features import read_wav
    with pytest.raises(ValueError, match="sample width"):
        read_wav(_write(tmp_path / "w.wav", width, 1, bytes(12 * width)))


def _float_wav(path, samples, extensible=False):
    """A RIFF WAV of IEEE-float samples (format tag 3, or WAVE_FORMAT_EXTENSIBLE with the IEEE-float sub-format), mono 16 kHz."""
    data = np.asarray(samples, dtype="<f4").tobytes()
    if extensible:
        guid = struct.pack("<IHH", 3, 0x0000, 0x0010) + bytes((0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71))
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, 1, 16000, 64000, 4, 32, 22, 32, 4) + guid
    else:
        fmt = struct.pack("<HHIIHH", 3, 1, 16000, 64000, 4, 32)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return str(path)


@pytest.mark.parametrize("extensible", [False, True])
def test_read_wav_refuses_ieee_float_and_never_reads_it_as_pcm32(tmp_path, extensible):
    """0.5f is 0x3F000000: taken for PCM-32 it would come back as 0.4921875 without a word."""
    from policy_gradient_asr_amd.features import read_wav
    with pytest.raises(ValueError, match="IEEE-float"):
        read_wav(_float_wav(tmp_path / "f.wav", [0.5, -0.25, 0.0, 1.0], extensible))


def test_read_wav_refuses_what_is_no_wav(tmp_path):
    from policy_gradient_asr_amd.features import read_wav
    empty = tmp_path / "empty.wav"
    empty.write_bytes(b"")
    with pytest.raises(ValueError, match="RIFF WAV"):
        read_wav(str(empty))
    junk = tmp_path / "junk.wav"
    junk.write_bytes(b"not a wave file at all, but long enough to hold a header")
    with pytest.raises(ValueError, match="RIFF WAV"):
        read_wav(str(junk))
