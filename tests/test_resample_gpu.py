"""Sample-rate conversion and speed perturbation on the MI355X: pgasr_resample against the numpy statement of the resampling function
(tests/resample_ref.py) bit for bit, the batched / split launches of features.Resample, the id-addressed speed draws, the front
end's composition with it, and the data layer."""
import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the last ratio's table (441 x 15 words) does not fit the kernel's LDS table and is read through L2
RATIOS = [(1, 3), (3, 1), (160, 441), (10, 9), (10, 11), (2, 1), (1, 16), (441, 160)]
# output lengths at which a tile of 256, 512, 768 or 1024 outputs ends: just short of, at and just past an edge, and further on
EDGE_OUTPUTS = (255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 2047, 2048, 2049, 4097)

_tables = {}


def table(L, M):
    if (L, M) not in _tables:
        _tables[(L, M)] = R.filter_table(L, M)
    return _tables[(L, M)]


def ref(x, L, M):
    return R.resample(x, L, M, table=None if (L, M) == (1, 1) else table(L, M))


def lengths_for(L, M):
    half = table(L, M)[2]
    ns = [0, 1, 2, half - 1, half, half + 1, 2 * half + 1, 255, 256, 257, 1023, 1024, 1025, 4097]
    for e in EDGE_OUTPUTS:                       # the smallest input that gives e outputs
        n = ((e - 1) * M) // L + 1
        if R.length(n, L, M) == e and n <= 8200:
            ns.append(n)
    return ns


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def run_rows(rows, ratios, ratio_idx, in_stride, out_stride=None):
    """rows: list of fp32 arrays -> (out (B, out_stride) numpy, n_out numpy); the input buffer holds NaN beyond every row."""
    from policy_gradient_asr_amd import hipops
    B = len(rows)
    buf = np.full((B, in_stride), np.nan, dtype=np.float32)
    for b, x in enumerate(rows):
        buf[b, :x.shape[0]] = x
    wave = torch.from_numpy(buf).to(DEV)
    n_in = torch.tensor([x.shape[0] for x in rows], dtype=torch.int32, device=DEV)
    idx = None if ratio_idx is None else torch.tensor(ratio_idx, dtype=torch.int32, device=DEV)
    out = None if out_stride is None else torch.full((B, out_stride), 7.0, dtype=torch.float32, device=DEV)
    got, n_out = hipops.resample(wave, n_in, ratios, ratio_idx=idx, out=out)
    if out is None:
        got2, n_out2 = hipops.resample(wave, n_in, ratios, ratio_idx=idx)          # a second run: the same bits
        assert torch.equal(got.view(torch.int32), got2.view(torch.int32)) and torch.equal(n_out, n_out2)
    assert torch.equal(wave.view(torch.int32).cpu(), torch.from_numpy(buf).view(torch.int32))       # the input is not written
    return got.cpu().numpy(), n_out.cpu().numpy()


@pytest.mark.parametrize("L,M", RATIOS)
def test_kernel_equals_reference_bit_for_bit(L, M):
    rng = np.random.default_rng(1000 * L + M)
    ns = lengths_for(L, M)
    rows = [rng.standard_normal(n).astype(np.float32) for n in ns]
    want = [ref(x, L, M) for x in rows]
    # in_stride a multiple of 4 (16-byte loads) and not (one sample per thread), both beyond the longest row
    for in_stride in ((max(ns) + 7) // 4 * 4, (max(ns) + 7) // 4 * 4 + 1):
        got, n_out = run_rows(rows, [(L, M)], None, in_stride)
        assert got.shape[1] >= R.length(in_stride, L, M)
        assert np.array_equal(n_out, np.array([w.shape[0] for w in want], dtype=np.int32))
        for b, w in enumerate(want):
            assert np.array_equal(bits(got[b, :w.shape[0]]), bits(w)), (L, M, in_stride, ns[b])
            assert np.array_equal(bits(got[b, w.shape[0]:]), np.zeros(got.shape[1] - w.shape[0], dtype=np.int32)), (L, M, ns[b])


def test_one_call_mixed_ratios_and_split_launches():
    from policy_gradient_asr_amd.features import Resample
    rng = np.random.default_rng(7)
    ratios = [(1, 3), (10, 9), (1, 1), (160, 441), (2, 1)]
    idx = [0, 1, 2, 3, 4, 2, 0, 3]
    ns = [3001, 1500, 777, 4410, 999, 2049, 6150, 12]
    rows = [rng.standard_normal(n).astype(np.float32) for n in ns]
    # the rows that are copied: every kind of bit pattern survives
    rows[2][:6] = np.array([0x80000000, 0x00000001, 0x7FC01234, 0xFF800000, 0x7F800000, 0x807FFFFF], dtype=np.uint32).view(np.float32)
    in_stride = 6152
    out_stride = R.length(in_stride, 2, 1) + 4                 # room for the largest ratio, as the kernel asks; prefilled with 7.0
    got, n_out = run_rows(rows, ratios, idx, in_stride, out_stride=out_stride)
    for b, x in enumerate(rows):
        w = ref(x, *ratios[idx[b]])
        assert n_out[b] == w.shape[0]
        assert np.array_equal(bits(got[b, :w.shape[0]]), bits(w)), b
        assert not got[b, w.shape[0]:].any() and not np.signbit(got[b, w.shape[0]:]).any(), b
    assert np.array_equal(bits(got[2, :777]), bits(rows[2])) and np.array_equal(bits(got[5, :2049]), bits(rows[5]))
    # an index without a ratio: an empty row, not a fault
    got, n_out = run_rows(rows[:3], ratios, [0, 5, -1], in_stride, out_stride=out_stride)
    assert n_out.tolist() == [1001, 0, 0] and not got[1:].any() and np.array_equal(bits(got[0, :1001]), bits(ref(rows[0], 1, 3)))

    # nine distinct ratios through features.Resample: two launches, rows back in the caller's order
    nine = [(1, 3), (10, 9), (1, 1), (160, 441), (2, 1), (10, 11), (3, 1), (1, 2), (147, 160)]
    order = [8, 0, 4, 2, 7, 1, 8, 3, 6, 5, 0]
    ns = [900 + 37 * k for k in range(len(order))]
    rows = [rng.standard_normal(n).astype(np.float32) for n in ns]
    rs = Resample(DEV)
    out, lengths = rs.apply([torch.from_numpy(x) for x in rows], [nine[k] for k in order])
    out = out.cpu().numpy()
    assert out.shape[0] == len(order) and out.shape[1] == (max(lengths) + 3) // 4 * 4
    for b, x in enumerate(rows):
        w = ref(x, *nine[order[b]])
        assert lengths[b] == w.shape[0]
        assert np.array_equal(bits(out[b, :w.shape[0]]), bits(w)), b
        assert not out[b, w.shape[0]:].any(), b
    # rates instead of ratios; an item at the target (or without a rate) is copied
    out, lengths = rs([torch.from_numpy(x) for x in rows[:4]], [48000, 16000, None, 44100], target_rate=16000)
    out = out.cpu().numpy()
    for b, (L, M) in enumerate([(1, 3), (1, 1), (1, 1), (160, 441)]):
        w = ref(rows[b], L, M)
        assert lengths[b] == w.shape[0] and np.array_equal(bits(out[b, :w.shape[0]]), bits(w)), b
    with pytest.raises(ValueError):
        rs([torch.from_numpy(rows[0])], [1000], target_rate=48000)           # 48 / 1 is beyond the limits


def test_speed_perturb_is_addressed_by_utterance_id():
    from policy_gradient_asr_amd.features import Resample, SpeedPerturb
    rng = np.random.default_rng(3)
    sp, rs, seed, offset = SpeedPerturb(), Resample(DEV), 11, 4
    ids = [40, 41, 42, 43, 44, 45, 46, 47]
    waves = [torch.from_numpy(rng.standard_normal(1200 + 111 * k).astype(np.float32)) for k in range(8)]
    assert len(set(sp.ratios(ids, seed, offset))) == 3                      # all three factors occur among these ids

    def run(sel):
        out, lengths = rs.apply([waves[k] for k in sel], sp.ratios([ids[k] for k in sel], seed, offset))
        out = out.cpu().numpy()
        return {k: bits(out[r, :lengths[r]]).copy() for r, k in enumerate(sel)}
    whole = run(range(8))
    for k in range(8):
        L, M = ((10, 9), (1, 1), (10, 11))[R.speed_draw(ids[k], 3, seed, offset)]
        assert np.array_equal(whole[k], bits(ref(waves[k].numpy(), L, M))), k
    for sel in ([0, 1, 2, 3], [4, 5, 6, 7], [6, 1, 4, 3, 0, 7, 2, 5]):
        part = run(sel)
        for k in sel:
            assert np.array_equal(part[k], whole[k]), (sel, k)


def _tone(f, rate, n):
    return torch.from_numpy(np.sin(2.0 * np.pi * f * np.arange(n) / rate).astype(np.float32))


def test_front_end_composition():
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.features import LogMel, MFCCDeltas
    g = torch.Generator().manual_seed(5)
    fe = LogMel(80, DEV)
    waves16 = [0.1 * torch.randn(n, generator=g) for n in (3000, 2400, 3333)]
    before = fe(waves16)

    def resampled(waves, L, M):
        ns = [int(w.numel()) for w in waves]
        buf = torch.zeros(len(waves), (max(ns) + 3) // 4 * 4)
        for b, w in enumerate(waves):
            buf[b, :ns[b]] = w
        out, n_out = hipops.resample(buf.to(DEV), torch.tensor(ns, dtype=torch.int32, device=DEV), [(L, M)])
        return [out[b, :n] for b, n in enumerate(n_out.tolist())]

    waves48 = [0.1 * torch.randn(n, generator=g) for n in (9000, 7201, 9999)]
    feat, fmask = fe(waves48, rates=[48000] * 3, target_rate=16000)
    feat2, fmask2 = fe(resampled(waves48, 1, 3))
    assert feat.shape == feat2.shape == (3, 80, 1 + 3333 // 200) and torch.equal(feat, feat2) and torch.equal(fmask, fmask2)
    assert fmask.sum(dim=(1, 2)).tolist() == [1 + 3000 // 200, 1 + 2401 // 200, 1 + 3333 // 200]
    # a rate conversion and a speed change on one item are ONE ratio: 1/3 x 10/9 = 10/27
    feat, fmask = fe(waves48, rates=[48000] * 3, target_rate=16000, speed=[(10, 9)] * 3)
    feat2, fmask2 = fe(resampled(waves48, 10, 27))
    assert torch.equal(feat, feat2) and torch.equal(fmask, fmask2)

    mf = MFCCDeltas(DEV)
    feat, fmask = mf(waves16, speed=[(10, 11)] * 3)
    feat2, fmask2 = mf(resampled(waves16, 10, 11))
    assert feat.shape[1] == 120 and torch.equal(feat, feat2) and torch.equal(fmask, fmask2)
    assert not torch.equal(fmask, mf(waves16)[1])                            # shorter than the unperturbed batch
    # per-item speeds, one of them none
    feat, fmask = mf(waves16, speed=[(10, 11), None, (10, 9)])
    feat2, fmask2 = mf([resampled([w], *r)[0] for w, r in zip(waves16, ((10, 11), (1, 1), (10, 9)))])
    assert torch.equal(feat, feat2) and torch.equal(fmask, fmask2)
    assert fmask.sum(dim=(1, 2)).tolist() == [1 + R.length(3000, 10, 11) // 200, 1 + 2400 // 200, 1 + R.length(3333, 10, 9) // 200]

    # the plain call is what it was: nothing the resampling path keeps is shared with it
    after = fe(waves16)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])

    # a 1 kHz tone recorded at 48 kHz lands in the band of a 1 kHz tone at 16 kHz once converted -- and three times too low without
    peak = lambda feat: int(feat[0].mean(dim=1).argmax())
    want = peak(fe([_tone(1000.0, 16000, 8000)])[0])
    conv, cmask = fe([_tone(1000.0, 48000, 24000)], rates=[48000], target_rate=16000)
    raw, rmask = fe([_tone(1000.0, 48000, 24000)])
    assert peak(conv) == want and int(cmask.sum()) == 41
    assert peak(raw) != want and peak(raw) < want and int(rmask.sum()) == 121


def test_collate_converts_and_perturbs():
    from policy_gradient_asr_amd.data import collate_custom
    from policy_gradient_asr_amd.features import SpeedPerturb, reduce_ratio, resample_length
    g = torch.Generator().manual_seed(9)
    char2ind = {"_": 0, "a": 1, "b": 2}
    sp, seed, offset = SpeedPerturb(), 21, 3
    rates = [48000, 16000, 32000, 44100, None, 48000]
    ns = [9000, 3100, 7000, 8820, 2500, 12001]
    ids = [100, 7, 33, 2, 58, 19]
    items = [{"wave": 0.1 * torch.randn(n, generator=g), "trans": "ab", "charmap": char2ind, "idx": u}
             for n, u in zip(ns, ids)]
    for it, r in zip(items, rates):
        if r is not None:
            it["rate"] = r
    batch = collate_custom(items, device=DEV, features="logmel80", target_rate=16000, speed_perturb=sp, seed=seed, offset=offset)
    assert batch["feat"].is_cuda and batch["feat"].shape[:2] == (6, 80)
    want = []
    for n, r, u in zip(ns, rates, ids):
        p, q = sp.factors[R.speed_draw(u, 3, seed, offset)]
        L, M = reduce_ratio(16000 * q, (r or 16000) * p)
        want.append(1 + resample_length(n, L, M) // 200)
    assert batch["fmask"].sum(dim=(1, 2)).tolist() == want and batch["feat"].shape[2] == max(want)
    # the rate alone; and nothing at all: the frames of before
    only = collate_custom(items, device=DEV, features="logmel80", target_rate=16000)
    assert only["fmask"].sum(dim=(1, 2)).tolist() == [1 + resample_length(n, *reduce_ratio(16000, r or 16000)) // 200 for n, r in zip(ns, rates)]
    plain = collate_custom(items, device=DEV, features="logmel80")
    assert plain["fmask"].sum(dim=(1, 2)).tolist() == [1 + n // 200 for n in ns]
    with pytest.raises(ValueError, match="idx"):
        collate_custom([{k: v for k, v in it.items() if k != "idx"} for it in items], device=DEV, speed_perturb=sp)
