"""Noise and reverberation augmentation on the MI355X: pgasr_reverb and pgasr_wave_mix against the numpy statement of the functions
(tests/wave_aug_ref.py) bit for bit, pgasr_wave_power within 1e-13 of the exactly rounded sum, the whole chain of
features.WaveAugment with its gains, halves / shards of a batch, the front end's composition with it, and the data layer.
Every buffer holds NaN beyond its rows; every output must be finite, a second run must give the same bits, inputs are not written."""
import functools

import numpy as np
import pytest
import torch

import wave_aug_ref as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def nan_rows(rows, stride):
    """(B, stride) fp32 numpy holding the rows and NaN beyond each."""
    buf = np.full((len(rows), stride), np.nan, dtype=np.float32)
    for b, x in enumerate(rows):
        buf[b, :x.shape[0]] = x
    return buf


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def same_bits(t, buf):
    return torch.equal(t.view(torch.int32).cpu(), torch.from_numpy(buf).view(torch.int32))


def check_rows(got, want_rows, what):
    """got (B, stride) numpy: row b is want_rows[b] bit for bit, zero beyond, finite throughout."""
    assert np.all(np.isfinite(got)), what
    for b, w in enumerate(want_rows):
        assert np.array_equal(bits(got[b, :w.shape[0]]), bits(w)), (what, b, w.shape[0])
        assert not bits(got[b, w.shape[0]:]).any(), (what, b, w.shape[0])


# ---------------------------------------------------------------- reverberation
@functools.lru_cache(maxsize=None)
def reverb_problem():
    """One launch's worth of every case: the bank (one row per (K, d)), the rows, their response index and the reference outputs."""
    from policy_gradient_asr_amd import hipops
    assert (hipops.REVERB_TILE, hipops.REVERB_CHUNK, hipops.REVERB_MAX_TAPS) == (W.TILE, W.CHUNK, W.MAX_TAPS)
    rng = np.random.default_rng(77)
    cases = W.reverb_cases()
    bank_key = sorted({(K, d) for K, _, d in cases})
    hs = [(rng.standard_normal(K) * np.exp(-np.arange(K) / max(K / 3.0, 1.0))).astype(np.float32) for K, _ in bank_key]
    rows, idx, want = [], [], []
    for K, n, d in cases:
        r = bank_key.index((K, d))
        x = rng.standard_normal(n).astype(np.float32)
        rows.append(x); idx.append(r); want.append(W.reverb(x, hs[r], d))
    for n in (0, 5, W.TILE + 1):                            # no response: copied
        x = rng.standard_normal(n).astype(np.float32)
        rows.append(x); idx.append(-1); want.append(x.copy())
    return bank_key, hs, rows, idx, want


def test_reverb_cases_cover_the_edges():
    cases = W.reverb_cases()
    Ks, ns = {K for K, _, _ in cases}, {n for _, n, _ in cases}
    assert Ks == {1, 2, 3, W.CHUNK - 1, W.CHUNK, W.CHUNK + 1, 2 * W.CHUNK + 1, W.MAX_TAPS}
    assert {0, 1, 2, W.TILE - 1, W.TILE, W.TILE + 1, 2 * W.TILE + 1} <= ns
    for K in Ks:
        ds = {d for k, _, d in cases if k == K}
        assert {0, min(1, K - 1), K // 2, K - 1} <= ds
    assert any(n < K for K, n, _ in cases) and any(n == K for K, n, _ in cases) and any(n > K for K, n, _ in cases)


@pytest.mark.parametrize("pad", [0, 1], ids=["stride%4==0", "stride%4==1"])
def test_reverb_equals_reference_bit_for_bit(pad):
    from policy_gradient_asr_amd import hipops
    bank_key, hs, rows, idx, want = reverb_problem()
    stride = (2 * W.TILE + 1 + 3) // 4 * 4 + pad
    buf = nan_rows(rows, stride)
    bank = nan_rows(hs, W.MAX_TAPS + 4 * pad + pad)         # a bank stride that is no multiple of 4 beside the one that is
    wave, rirs = torch.from_numpy(buf).to(DEV), torch.from_numpy(bank).to(DEV)
    n, rir_idx = i32(x.shape[0] for x in rows), i32(idx)
    rir_len, rir_delay = i32(K for K, _ in bank_key), i32(d for _, d in bank_key)
    out = torch.full((len(rows), stride), 7.0, dtype=torch.float32, device=DEV)
    got = hipops.reverb(wave, n, rirs, rir_len, rir_delay, rir_idx, out=out)
    assert got is out
    again = hipops.reverb(wave, n, rirs, rir_len, rir_delay, rir_idx)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    assert same_bits(wave, buf) and same_bits(rirs, bank)
    check_rows(got.cpu().numpy(), want, "reverb")


def test_reverb_refuses_aliasing_and_bad_shapes():
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd._lib import PgasrError
    wave = torch.zeros(2, 16, device=DEV)
    n, one = i32([16, 16]), i32([1])
    rirs = torch.ones(1, 4, device=DEV)
    with pytest.raises(PgasrError, match="alias"):
        hipops.reverb(wave, n, rirs, one, i32([0]), i32([0, 0]), out=wave)
    with pytest.raises(PgasrError, match="alias"):
        hipops.reverb(wave[:1], n[:1], rirs, one, i32([0]), i32([0]), out=wave.view(-1)[8:24].view(1, 16))
    with pytest.raises(PgasrError):
        hipops.reverb(wave, n, rirs, one, i32([0]), i32([0]))              # rir_idx of the wrong length
    with pytest.raises(PgasrError):
        hipops.reverb(wave, n, rirs, i32([1, 1]), i32([0]), i32([0, 0]))   # rir_len of the wrong length


# ---------------------------------------------------------------- power
def test_wave_power_within_1e13_of_the_exact_sum():
    from policy_gradient_asr_amd import hipops
    rng = np.random.default_rng(5)
    ns = [0, 1, 5, 1023, 4096, 4097, 10001]
    rows = [rng.standard_normal(n).astype(np.float32) for n in ns]
    want = np.array([W.power(x, x.shape[0]) for x in rows])
    got = {}
    for stride in (10004, 10005):
        buf = nan_rows(rows, stride)
        src = torch.from_numpy(buf).to(DEV)
        p = hipops.wave_power(src, i32(ns))
        assert p.dtype == torch.float64 and torch.equal(p, hipops.wave_power(src, i32(ns))) and same_bits(src, buf)
        got[stride] = p.cpu().numpy()
        assert np.all(np.isfinite(got[stride])) and got[stride][0] == 0.0
        assert np.all(np.abs(got[stride] - want) <= 1e-13 * want)
        # a row's power does not depend on the rest of the batch
        part = hipops.wave_power(src[3:6].contiguous(), i32(ns[3:6])).cpu().numpy()
        assert np.array_equal(part.view(np.int64), got[stride][3:6].view(np.int64))
    assert np.array_equal(got[10004].view(np.int64), got[10005].view(np.int64))         # nor on the alignment

    # cyclically wrapped segments of a noise bank: a period below n (several wraps), a start at period - 1, no row, n = 0
    lengths = [100, 5000, 777]
    noises = [rng.standard_normal(m).astype(np.float32) for m in lengths]
    cases = [(0, 99, 1501), (0, 0, 100), (0, 37, 99), (1, 4999, 5000), (1, 4999, 12000), (2, 776, 778), (2, 5, 0), (-1, 0, 300), (1, 123, 1)]
    for stride in (5000, 5003):
        bank = nan_rows(noises, stride)
        src = torch.from_numpy(bank).to(DEV)
        row, start, n = i32(c[0] for c in cases), i32(c[1] for c in cases), i32(c[2] for c in cases)
        period = i32(lengths[c[0]] if c[0] >= 0 else 1 for c in cases)
        p = hipops.wave_power(src, n, row=row, start=start, period=period)
        assert torch.equal(p, hipops.wave_power(src, n, row=row, start=start, period=period)) and same_bits(src, bank)
        p = p.cpu().numpy()
        want = np.array([W.power(noises[r], m, s, lengths[r]) if r >= 0 else 0.0 for r, s, m in cases])
        assert np.all(np.isfinite(p)) and p[6] == 0.0 and p[7] == 0.0
        assert np.all(np.abs(p - want) <= 1e-13 * want)


# ---------------------------------------------------------------- mix
@pytest.mark.parametrize("stride", [4100, 4101])
def test_wave_mix_with_given_gains_bit_for_bit(stride):
    from policy_gradient_asr_amd import hipops
    rng = np.random.default_rng(stride)
    lengths = [100, 5000, 777]
    noises = [rng.standard_normal(m).astype(np.float32) for m in lengths]
    #        n     a     g     noise start
    cases = [(4097, 0.75, 0.31, 0, 99), (1000, 1.0, 0.05, 1, 4999), (1025, 1.3, 2.0, 2, 5), (300, 1.0, 0.0, 1, 0), (640, 0.5, 0.7, -1, 0),
             (0, 1.0, 0.5, 0, 3), (1, 0.9, 0.4, 0, 42), (4096, 1.0, 1.0, 1, 2500)]
    rows = [rng.standard_normal(c[0]).astype(np.float32) for c in cases]
    rows[3][5] = -0.0                                      # a = 1, g = 0: the bits of the input, a signed zero included
    gains = np.array([[c[1], c[2]] for c in cases], dtype=np.float32)
    want = [W.mix(x, np.float32(c[1]), np.float32(c[2] if c[3] >= 0 else 0.0), noises[c[3]] if c[3] >= 0 else None, c[4],
                  lengths[c[3]] if c[3] >= 0 else None) for x, c in zip(rows, cases)]
    assert np.array_equal(bits(want[3]), bits(rows[3]))
    buf, bank = nan_rows(rows, stride), nan_rows(noises, 5000 + stride % 4)
    wave, noise = torch.from_numpy(buf).to(DEV), torch.from_numpy(bank).to(DEV)
    n, g = i32(c[0] for c in cases), torch.from_numpy(gains).to(DEV)
    args = dict(noise=noise, noise_len=i32(lengths), noise_idx=i32(c[3] for c in cases), noise_start=i32(c[4] for c in cases), gains=g)
    out, g_out = hipops.wave_mix(wave, n, **args)
    assert g_out is g and same_bits(g, gains) and same_bits(wave, buf) and same_bits(noise, bank)
    check_rows(out.cpu().numpy(), want, "mix")
    again, _ = hipops.wave_mix(wave, n, **args)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    inplace, _ = hipops.wave_mix(wave, n, out=wave, **args)
    assert inplace is wave
    check_rows(wave.cpu().numpy(), want, "mix in place")


# ---------------------------------------------------------------- the whole chain
@functools.lru_cache(maxsize=None)
def chain_problem():
    from policy_gradient_asr_amd.features import NoiseBank, RirBank, WaveAugment
    noises, rirs = W.chain_corpus()
    nb = NoiseBank([torch.from_numpy(v) for v in noises], device=DEV)
    rb = RirBank([torch.from_numpy(v) for v in rirs], device=DEV)
    aug = WaveAugment(noise=nb, rir=rb, **W.CHAIN_POLICY)
    hs, delays = zip(*(W.normalise_rir(h) for h in rirs))
    ids, rows = W.chain_rows()
    dr = W.draws(ids, W.CHAIN_SEED, W.CHAIN_OFFSET, W.NOISE_LENGTHS, len(W.RIR_LENGTHS), **W.CHAIN_POLICY)
    want = [W.chain(x, d, noises, hs, delays) for x, d in zip(rows, dr)]
    return aug, ids, rows, want, (noises, hs, delays)


def run_chain(aug, ids, rows, stride):
    buf = nan_rows(rows, stride)
    wave = torch.from_numpy(buf).to(DEV)
    out, gains = aug(wave, i32(x.shape[0] for x in rows), ids, W.CHAIN_SEED, W.CHAIN_OFFSET, want_gains=True)
    assert same_bits(wave, buf) and out.data_ptr() != wave.data_ptr()
    return out.cpu().numpy(), gains.cpu().numpy()


def test_banks_are_packed_scaled_and_located():
    aug, _, _, _, (noises, hs, delays) = chain_problem()
    assert list(aug.noise.lengths) == list(W.NOISE_LENGTHS) and list(aug.rir.lengths) == list(W.RIR_LENGTHS)
    nw, rw = aug.noise.wave.cpu().numpy(), aug.rir.wave.cpu().numpy()
    for r, v in enumerate(noises):
        assert np.array_equal(bits(nw[r, :v.shape[0]]), bits(v))
    for r, h in enumerate(hs):
        assert np.array_equal(bits(rw[r, :h.shape[0]]), bits(h)) and not rw[r, h.shape[0]:].any()
        assert abs(float(np.sum(rw[r].astype(np.float64) ** 2)) - 1.0) < 1e-6
    assert list(aug.rir.delays) == list(delays) == [0, 5, 5] and aug.rir.delay_dev.cpu().tolist() == list(delays)
    from policy_gradient_asr_amd.features import NoiseBank, RirBank
    with pytest.raises(ValueError):
        NoiseBank([torch.zeros(0)], device=DEV)
    with pytest.raises(ValueError):
        RirBank([torch.zeros(8)], device=DEV)
    long_rir = RirBank([torch.ones(W.MAX_TAPS + 100)], device=DEV)         # cut to the cap, then scaled
    assert long_rir.lengths == [W.MAX_TAPS] and abs(float(long_rir.wave.double().pow(2).sum()) - 1.0) < 1e-6


@pytest.mark.parametrize("stride", [4100, 4101])
def test_chain_equals_reference_bit_for_bit(stride):
    aug, ids, rows, want, _ = chain_problem()
    out, gains = run_chain(aug, ids, rows, stride)
    check_rows(out, [w[0] for w in want], "chain")
    assert np.all(np.isfinite(gains))
    for b, w in enumerate(want):
        assert bits(gains[b, 0]) == bits(w[1][0]) and bits(gains[b, 1]) == bits(w[1][1]), (b, gains[b], w[1])
    out2, gains2 = run_chain(aug, ids, rows, stride)
    assert np.array_equal(bits(out), bits(out2)) and np.array_equal(bits(gains), bits(gains2))
    # padding and the rows nothing was drawn for are copies
    for b, u in enumerate(ids):
        if u < 0:
            assert np.array_equal(bits(out[b, :rows[b].shape[0]]), bits(rows[b])) and tuple(gains[b]) == (1.0, 0.0)


def test_halves_interleaved_order_and_padded_shard_reproduce_the_batch():
    aug, ids, rows, want, _ = chain_problem()
    whole, gains = run_chain(aug, ids, rows, 4100)
    B = len(ids)

    def check(sel, stride):
        out, g = run_chain(aug, [ids[b] if b is not None else -1 for b in sel],
                           [rows[b] if b is not None else np.zeros(0, dtype=np.float32) for b in sel], stride)
        for i, b in enumerate(sel):
            if b is None:
                assert not bits(out[i]).any() and tuple(g[i]) == (1.0, 0.0)
                continue
            n = rows[b].shape[0]
            assert np.array_equal(bits(out[i, :n]), bits(whole[b, :n])) and not bits(out[i, n:]).any(), (sel, b)
            assert np.array_equal(bits(g[i]), bits(gains[b])), (sel, b)
    check(list(range(B // 2)), 4100)
    check(list(range(B // 2, B)), 4100)
    check(list(range(1, B, 2)) + list(range(0, B, 2)), 4104)
    check([3, None, 0, None, None], 4101)
    # a shard none of whose rows draws a response, and one none of whose rows draws noise, skip those launches: still the same bits
    dr = W.draws(ids, W.CHAIN_SEED, W.CHAIN_OFFSET, W.NOISE_LENGTHS, len(W.RIR_LENGTHS), **W.CHAIN_POLICY)
    no_rir = [b for b in range(B) if dr[b][4] < 0]
    no_noise = [b for b in range(B) if dr[b][0] < 0]
    assert len(no_rir) >= 2 and len(no_noise) >= 2
    check(no_rir, 4100)
    check(no_noise, 4100)


# ---------------------------------------------------------------- front end and data layer
def front_end_waves():
    rng = np.random.default_rng(9)
    return [torch.from_numpy((0.1 * rng.standard_normal(n)).astype(np.float32)) for n in (3000, 1201, 2048)], [0, 1, 2]


def test_front_end_composes_with_the_augmentation():
    from policy_gradient_asr_amd.features import LogMel
    aug = chain_problem()[0]
    waves, _ = front_end_waves()
    ids = chain_problem()[1][:3]                             # noise + response, noise alone, response alone
    fe = LogMel(80, DEV)
    plain, pmask = fe(waves)
    none, nmask = fe(waves, wave_aug=None)
    assert torch.equal(plain, none) and torch.equal(pmask, nmask)
    feat, fmask = fe(waves, wave_aug=aug.bind(ids, W.CHAIN_SEED, W.CHAIN_OFFSET))
    # the same waves augmented separately, then the plain front end
    ns = [int(w.numel()) for w in waves]
    buf = nan_rows([w.numpy() for w in waves], 3001)
    sep = aug(torch.from_numpy(buf).to(DEV), i32(ns), ids, W.CHAIN_SEED, W.CHAIN_OFFSET)
    want, wmask = fe([sep[b, :n].clone() for b, n in enumerate(ns)])
    assert torch.equal(feat.view(torch.int32), want.view(torch.int32)) and torch.equal(fmask, wmask)
    assert torch.isfinite(feat).all() and not torch.equal(feat, plain)
    # behind a rate conversion too: the augmentation sees the resampled batch
    feat2, _ = fe(waves, rates=[8000, 16000, 16000], target_rate=16000, wave_aug=aug.bind(ids, W.CHAIN_SEED, W.CHAIN_OFFSET))
    assert torch.isfinite(feat2).all() and feat2.shape[2] > feat.shape[2]


def test_collate_runs_end_to_end_with_the_augmentation():
    from policy_gradient_asr_amd.data import collate_custom
    from policy_gradient_asr_amd.features import LogMel
    aug = chain_problem()[0]
    waves, _ = front_end_waves()
    ids = chain_problem()[1][:3]
    char2ind = {"a": 1, "b": 2}
    items = [{"wave": w, "trans": "ab", "charmap": char2ind, "idx": u} for w, u in zip(waves, ids)]
    batch = collate_custom(items, device=DEV, features="logmel80", wave_augment=aug, seed=W.CHAIN_SEED, offset=W.CHAIN_OFFSET)
    assert sorted(batch) == ["feat", "fmask", "tmask", "trans"] and batch["feat"].is_cuda and torch.isfinite(batch["feat"]).all()
    want, _ = LogMel(80, DEV)(waves, wave_aug=aug.bind(ids, W.CHAIN_SEED, W.CHAIN_OFFSET))
    assert torch.equal(batch["feat"], want)
    plain = collate_custom(items, device=DEV, features="logmel80")
    assert plain["feat"].shape == batch["feat"].shape and not torch.equal(plain["feat"], batch["feat"])


def test_train_builds_its_policy_from_wav_directories(tmp_path):
    import wave
    from policy_gradient_asr_amd.model import _wave_augment
    rng = np.random.default_rng(3)
    for sub, files in (("noise", (("n0.wav", 16000, 700), ("n1.wav", 8000, 400))), ("rir", (("r0.wav", 16000, 64),))):
        (tmp_path / sub).mkdir()
        for name, rate, n in files:
            with wave.open(str(tmp_path / sub / name), "wb") as f:
                f.setnchannels(1); f.setsampwidth(2); f.setframerate(rate)
                f.writeframes((rng.standard_normal(n) * 3000).astype("<i2").tobytes())
    aug = _wave_augment(str(tmp_path / "noise"), str(tmp_path / "rir"), (0.0, 10.0), 1.0, 1.0, torch.device(DEV))
    assert aug.noise.lengths == [700, 800] and aug.rir.lengths == [64]          # the 8 kHz recording is brought to 16 kHz
    assert aug.state() == {"snr_db": [0.0, 10.0], "noise_prob": 1.0, "rir_prob": 1.0, "noise_lengths": [700, 800], "rir_lengths": [64]}
    x = (0.1 * rng.standard_normal(1000)).astype(np.float32)
    out, gains = aug(torch.from_numpy(nan_rows([x], 1001)).to(DEV), i32([1000]), [0], 1, 1, want_gains=True)
    out = out.cpu().numpy()
    assert np.all(np.isfinite(out)) and not out[0, 1000:].any() and gains[0, 1] > 0 and not np.array_equal(out[0, :1000], x)
    only_noise = _wave_augment(str(tmp_path / "noise"), None, (0.0, 10.0), 1.0, 1.0, torch.device(DEV))
    assert only_noise.rir is None and only_noise.noise.lengths == [700, 800]
