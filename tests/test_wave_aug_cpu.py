"""Noise and reverberation augmentation off the device: the numpy statement of the functions (tests/wave_aug_ref.py) against
np.convolve and the drawn SNR, the id-addressed draws of features.WaveAugment, the data layer's refusals, and the condition the GPU
test's inputs must meet -- no fp32 gain of the shared cases sits within 1e-12 of a rounding boundary."""
import ctypes
import math

import numpy as np
import pytest
import torch

import wave_aug_ref as W
from resample_ref import speed_draw
from specaug_ref import philox_words


class Lengths:
    """What ``WaveAugment.draws`` needs of a bank."""

    def __init__(self, lengths):
        self.lengths = list(lengths)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_limits_agree_with_the_library_and_the_reference():
    from policy_gradient_asr_amd import _lib, features, hipops
    t, c, m = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert _lib.load().pgasr_reverb_limits(ctypes.byref(t), ctypes.byref(c), ctypes.byref(m)) == 0
    assert (t.value, c.value, m.value) == (hipops.REVERB_TILE, hipops.REVERB_CHUNK, hipops.REVERB_MAX_TAPS) == (W.TILE, W.CHUNK, W.MAX_TAPS)
    assert hipops.REVERB_MAX_TAPS >= 16000 and features.REVERB_MAX_TAPS == hipops.REVERB_MAX_TAPS
    assert _lib.load().pgasr_reverb_limits(None, None, None) == 0


def test_delta_and_pure_delay_return_the_input_bits():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(333).astype(np.float32)
    assert np.array_equal(bits(W.reverb(x, np.ones(1, dtype=np.float32), 0)), bits(x))
    x[7] = -0.0
    want = x.copy()
    want[7] = 0.0              # -0.0 * 1 enters an accumulator that starts at +0.0: the one input whose bits a filter does not keep
    assert np.array_equal(bits(W.reverb(x, np.ones(1, dtype=np.float32), 0)), bits(want))
    for d in (1, 5, 40):
        h = np.zeros(41, dtype=np.float32)
        h[d] = 1.0
        assert np.array_equal(bits(W.reverb(x, h, d)), bits(want))
    # a response longer than the row takes the other loop order: the same bits
    h = np.zeros(500, dtype=np.float32)
    h[123] = 1.0
    assert np.array_equal(bits(W.reverb(x, h, 123)), bits(want))


@pytest.mark.parametrize("n,K,d", [(700, 64, 0), (700, 64, 20), (50, 300, 299), (300, 300, 150), (1, 5, 2)])
def test_reference_fir_against_np_convolve(n, K, d):
    rng = np.random.default_rng(n + K + d)
    x = rng.standard_normal(n).astype(np.float32)
    h = (rng.standard_normal(K) * np.exp(-np.arange(K) / 30.0)).astype(np.float32)
    got = W.reverb(x, h, d, rounded=False)
    x64, h64 = x.astype(np.float64), h.astype(np.float64)
    want = np.convolve(x64, h64)[d:d + n]
    bound = K * 2.0 ** -52 * np.convolve(np.abs(x64), np.abs(h64))[d:d + n]
    assert np.all(np.abs(got - want) <= bound)
    # both loop orders of the reference give the same bits
    if K <= n:
        long_h = np.concatenate((h, np.zeros(n + 1 - K, dtype=np.float32)))           # K > n: the loop over samples
        assert np.array_equal(W.reverb(x, long_h, d, rounded=False).view(np.int64), got.view(np.int64))


def test_reference_output_has_the_drawn_snr():
    noises, rirs = W.chain_corpus()
    hs, delays = zip(*(W.normalise_rir(h) for h in rirs))
    ids, rows = W.chain_rows()
    dr = W.draws(ids, W.CHAIN_SEED, W.CHAIN_OFFSET, W.NOISE_LENGTHS, len(W.RIR_LENGTHS), **W.CHAIN_POLICY)
    checked = 0
    for x, d in zip(rows, dr):
        out, (a, g), (p_dry, p_wet, p_noise) = W.chain(x, d, noises, hs, delays)
        assert np.all(np.isfinite(out)) and np.isfinite(a) and np.isfinite(g)
        if g > 0:
            snr = 10.0 * math.log10((float(a) ** 2 * p_wet) / (float(g) ** 2 * p_noise))
            assert abs(snr - d[2]) < 1e-6, (snr, d)
            assert 5.0 <= d[2] <= 20.0
            checked += 1
        if d[4] >= 0 and p_wet > 0:               # the dry level is restored within the fp32 gain's rounding
            assert abs(float(a) ** 2 * p_wet / p_dry - 1.0) < 4 * 2.0 ** -24
    assert checked >= 3


def test_draws_are_addressed_by_seed_offset_and_id():
    from policy_gradient_asr_amd.features import SpeedPerturb, WaveAugment, _philox4x32_10
    aug = WaveAugment(noise=Lengths(W.NOISE_LENGTHS), rir=Lengths(W.RIR_LENGTHS), **W.CHAIN_POLICY)
    ids = list(range(64)) + [-1, 2 ** 31 - 1]
    d = aug.draws(ids, W.CHAIN_SEED, W.CHAIN_OFFSET)
    ref = W.draws(ids, W.CHAIN_SEED, W.CHAIN_OFFSET, W.NOISE_LENGTHS, len(W.RIR_LENGTHS), **W.CHAIN_POLICY)
    assert d["noise_idx"].dtype == d["noise_start"].dtype == d["rir_idx"].dtype == np.int32 and d["amp"].dtype == np.float64
    for b, (ni, ns, snr, amp, ri) in enumerate(ref):
        assert (d["noise_idx"][b], d["noise_start"][b], d["rir_idx"][b]) == (ni, ns, ri)
        assert d["snr_db"][b] == snr and d["amp"][b] == amp
    assert d["noise_idx"][64] == -1 and d["rir_idx"][64] == -1 and d["amp"][64] == 0.0          # padding
    again = aug.draws(ids, W.CHAIN_SEED, W.CHAIN_OFFSET)
    assert all(np.array_equal(d[k], again[k]) for k in d)
    key = lambda dd: [tuple(dd[k][b] for k in ("noise_idx", "noise_start", "rir_idx", "snr_db")) for b in range(64)]
    assert key(aug.draws(ids, W.CHAIN_SEED + 1, W.CHAIN_OFFSET)) != key(d)
    assert key(aug.draws(ids, W.CHAIN_SEED, W.CHAIN_OFFSET + 1)) != key(d)
    assert key(aug.draws([u + 64 for u in ids[:64]], W.CHAIN_SEED, W.CHAIN_OFFSET)) != key(d)
    # a shard draws what the whole batch draws
    part = aug.draws(ids[10:20], W.CHAIN_SEED, W.CHAIN_OFFSET)
    assert all(np.array_equal(part[k], d[k][10:20]) for k in d)
    # the blocks are not the speed-perturbation block of the same (u, offset)
    for u in range(8):
        speed = philox_words(u, W.CHAIN_OFFSET, 4, 0, W.CHAIN_SEED)
        for dom in (W.DOM_NOISE, W.DOM_RIR):
            w = W.philox4(u, W.CHAIN_OFFSET, dom, W.CHAIN_SEED)
            assert w[:2] != speed
            assert w == _philox4x32_10((u, W.CHAIN_OFFSET, dom, 0), (W.CHAIN_SEED & 0xFFFFFFFF, W.CHAIN_SEED >> 32))
    assert SpeedPerturb.DOMAIN not in (WaveAugment.NOISE_DOMAIN, WaveAugment.RIR_DOMAIN) and \
        (WaveAugment.NOISE_DOMAIN, WaveAugment.RIR_DOMAIN) == (W.DOM_NOISE, W.DOM_RIR)
    assert speed_draw(0, 3, W.CHAIN_SEED, W.CHAIN_OFFSET) in (0, 1, 2)


def test_draws_stay_in_range_at_the_extreme_words():
    from policy_gradient_asr_amd.features import WaveAugment
    top = 2 ** 32 - 1
    lengths = (1, 7, 2 ** 31 - 1)
    for w in ((0, 0, 0, 0), (top, top, top, top)):
        for prob in (0.0, 0.3, 1.0):
            apply, r, snr, start = WaveAugment._noise_from_words(w, prob, lengths, (5.0, 20.0))
            assert 0 <= r < len(lengths) and 0 <= start < lengths[r] and 5.0 <= snr < 20.0
            assert apply == (prob == 1.0 or (prob > 0 and w[0] == 0))
            apply, r = WaveAugment._rir_from_words(w, prob, 5)
            assert 0 <= r < 5 and apply == (prob == 1.0 or (prob > 0 and w[0] == 0))
    for w1 in (0, top):
        assert WaveAugment._noise_from_words((0, w1, 0, top), 1.0, (3,), (0.0, 0.0))[1:] == (0, 0.0, 2)


def test_probability_zero_and_one():
    from policy_gradient_asr_amd.features import WaveAugment
    ids = list(range(200))
    none = WaveAugment(noise=Lengths((10, 20)), rir=Lengths((4,)), noise_prob=0.0, rir_prob=0.0).draws(ids, 1, 0)
    assert np.all(none["noise_idx"] == -1) and np.all(none["rir_idx"] == -1) and np.all(none["amp"] == 0.0)
    every = WaveAugment(noise=Lengths((10, 20)), rir=Lengths((4,)), noise_prob=1.0, rir_prob=1.0, snr_db=10.0).draws(ids, 1, 0)
    assert np.all(every["noise_idx"] >= 0) and np.all(every["rir_idx"] == 0) and set(every["noise_idx"]) == {0, 1}
    assert np.all(every["snr_db"] == 10.0) and np.all(every["amp"] == 10.0 ** -0.5)
    assert np.all(every["noise_start"] < np.array([10, 20])[every["noise_idx"]])
    half = WaveAugment(noise=Lengths((10,)), noise_prob=0.5).draws(ids, 1, 0)
    assert 60 <= int((half["noise_idx"] >= 0).sum()) <= 140 and np.all(half["rir_idx"] == -1)


def test_policy_is_immutable_and_checked():
    from policy_gradient_asr_amd.features import WaveAugment
    aug = WaveAugment(noise=Lengths((10,)), snr_db=(0, 30), noise_prob=0.25)
    with pytest.raises(AttributeError):
        aug.noise_prob = 1.0
    assert aug.state() == {"snr_db": [0.0, 30.0], "noise_prob": 0.25, "rir_prob": 0.5, "noise_lengths": [10], "rir_lengths": None}
    assert WaveAugment.coerce(None) is None and WaveAugment.coerce(aug) is aug
    with pytest.raises(TypeError):
        WaveAugment.coerce({"noise_prob": 1.0})
    for bad in ({"noise": None}, {"noise": Lengths(())}, {"noise": Lengths((0,))}, {"snr_db": (20.0, 5.0)}, {"snr_db": float("nan")},
                {"noise_prob": 1.5}, {"rir_prob": -0.1}):
        with pytest.raises(ValueError):
            WaveAugment(**{"noise": Lengths((10,)), **bad})
    with pytest.raises(TypeError):
        WaveAugment(noise=Lengths((10,)), noise_prob="1")


def test_data_layer_refusals_and_cpu_tensors():
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd._lib import PgasrError
    from policy_gradient_asr_amd.data import collate_custom, extract_feats
    from policy_gradient_asr_amd.features import WaveAugment
    aug = WaveAugment(noise=Lengths((10,)))
    char2ind = {"a": 1, "b": 2}
    feats = [{"feat": torch.zeros(5, 7), "trans": "a", "charmap": char2ind, "idx": i} for i in range(2)]
    with pytest.raises(ValueError, match="precomputed"):
        extract_feats(feats, wave_augment=aug)
    with pytest.raises(ValueError, match="precomputed"):
        collate_custom(feats, wave_augment=aug)
    waves = [{"wave": torch.zeros(400), "trans": "a", "charmap": char2ind}]
    with pytest.raises(ValueError, match='"idx"'):
        extract_feats(waves, wave_augment=aug)
    # with nothing asked for, the data layer does what it did
    a, b = collate_custom(feats), collate_custom(feats, wave_augment=None)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    # off the device the product refuses, it does not fall back
    n = torch.tensor([8, 8], dtype=torch.int32)
    with pytest.raises(PgasrError):
        hipops.reverb(torch.zeros(2, 8), n, torch.ones(1, 4), n[:1], n[:1], n)
    with pytest.raises(PgasrError):
        hipops.wave_power(torch.zeros(2, 8), n)
    with pytest.raises(PgasrError):
        hipops.wave_mix(torch.zeros(2, 8), n, gains=torch.ones(2, 2))
    with pytest.raises(PgasrError):
        aug(torch.zeros(2, 8), n, [0, 1], 0, 0)


def test_shared_chain_inputs_are_robust_to_the_last_bits_of_the_powers():
    """The device sums the squares in another order than the reference: its fp64 powers may differ in the last bits (1e-13 relative
    is what test_wave_aug_gpu holds them to).  The gains are compared bit for bit, so no gain of the shared cases may sit so close to
    an fp32 rounding boundary that a relative change of 1e-12 in any power moves it."""
    noises, rirs = W.chain_corpus()
    hs, delays = zip(*(W.normalise_rir(h) for h in rirs))
    ids, rows = W.chain_rows()
    dr = W.draws(ids, W.CHAIN_SEED, W.CHAIN_OFFSET, W.NOISE_LENGTHS, len(W.RIR_LENGTHS), **W.CHAIN_POLICY)
    kinds = set()
    for x, d in zip(rows, dr):
        _, (a, g), p = W.chain(x, d, noises, hs, delays)
        noisy = d[0] >= 0 and x.shape[0] >= 1
        kinds.add((d[0] >= 0, d[4] >= 0, bool(g > 0)))
        for i in range(3):
            for e in (-1e-12, 1e-12):
                q = list(p)
                q[i] = q[i] * (1.0 + e)
                if d[4] < 0 and i < 2:             # no response: the wet row IS the dry row, its power moves with it
                    q[0] = q[1] = p[0] * (1.0 + e)
                a2, g2 = W.gains(q[0], q[1], q[2], d[3], noisy)
                assert bits(a2) == bits(a) and bits(g2) == bits(g), (d, i, e)
    # every kind of row is there: noise and response, either alone, neither; a noise that gives no gain (silent noise or silent row)
    assert {(True, True, True), (True, False, True), (False, True, False), (False, False, False)} <= kinds
    assert (True, False, False) in kinds or (True, True, False) in kinds
    assert -1 in ids and any(r.shape[0] == 0 for r in rows) and any(r.shape[0] > 0 and not r.any() for r in rows)


def test_train_reads_its_banks_from_directories_of_wav_files(tmp_path):
    import wave
    from policy_gradient_asr_amd.model import _read_wav_dir, _wave_augment
    assert _wave_augment(None, None, (5.0, 20.0), 1.0, 0.5, "cuda:0") is None          # nothing asked for: nothing built
    for name, rate, n in (("b.wav", 16000, 320), ("a.WAV", 8000, 100)):
        with wave.open(str(tmp_path / name), "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(rate)
            f.writeframes((np.arange(n) % 7 * 1000).astype("<i2").tobytes())
    (tmp_path / "notes.txt").write_text("not audio")
    waves, rates = _read_wav_dir(str(tmp_path))
    assert rates == [8000, 16000] and [int(w.numel()) for w in waves] == [100, 320]     # sorted by name, other files ignored
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError, match="no .wav"):
        _read_wav_dir(str(empty))
