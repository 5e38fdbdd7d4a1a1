"""SpecAugment masking on the MI355X: pgasr_spec_augment against the numpy statement of the masking function
(tests/specaug_ref.py) bit for bit -- both fill modes, the vector and the scalar path, in place, caller-named ids -- the host
layer's refusals, the callable policy, and shards / micro-batches against the whole batch."""
import numpy as np
import pytest
import torch

import specaug_ref as R
from pg_harness import DEV

pytestmark = pytest.mark.gpu

SEED = 4
FIELDS = dict(freq_masks=2, freq_width=27, time_masks=2, time_width=20, time_ratio=0.2)
# B, F, T -> lengths, policy fields
SHAPES = {
    (8, 80, 60): ((60, 57, 54, 51, 48, 1, 0, 33), FIELDS),                          # the vector path, the maintainer's case
    (3, 120, 61): ((61, 40, 7), dict(FIELDS, time_width=100, time_ratio=None)),     # scalar tail, MFCC width
    (1, 5, 7): ((6,), dict(FIELDS, time_width=100, time_ratio=None)),               # smaller than one wave
    (2, 80, 1031): ((1031, 1000), dict(FIELDS, time_width=100, time_ratio=None)),   # rows longer than one pass of a workgroup
    (2, 3, 1028): ((1027, 1026), dict(FIELDS, time_width=100, time_ratio=None)),    # .. on the vector path, a length inside a quad
}


def _policy(fields, fill="row_mean"):
    from policy_gradient_asr_amd.features import SpecAugment
    return SpecAugment(fill=fill, **fields)


def _features(B, F, T, lengths, seed=0):
    """dB-like features (mean -40, far from 0 so that a fill cannot pass for the input), zero beyond each length."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, F, T)) * 10.0 - 40.0).astype(np.float32)
    for b, n in enumerate(lengths):
        x[b, :, n:] = 0
    return x


def _dev_lengths(lengths):
    return torch.tensor(list(lengths), dtype=torch.int32, device=DEV)


def _check_against_reference(got, got_masks, x, lengths, ids, pol, offset):
    """masks ==, untouched cells ==, "zero" == everywhere, "row_mean" within one ulp beyond the error of an fp64 sum of T terms."""
    B, F, T = x.shape
    want, _ = R.apply(x, lengths, ids, pol, SEED, offset)
    iv = R.mask_intervals(lengths, ids, pol, F, SEED, offset)
    hit = R.hit_mask(iv, lengths, pol.freq_masks, F, T)
    assert got_masks.dtype == np.int32 and np.array_equal(got_masks, iv)
    assert np.array_equal(got[~hit], x[~hit])
    if pol.fill == "zero":
        assert np.array_equal(got, want)
        return hit
    mean_abs = np.zeros((B, F))
    for b, n in enumerate(lengths):
        if n > 0:
            mean_abs[b] = np.abs(x[b, :, :n].astype(np.float64)).mean(axis=1)
    tol = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + (T * 2.0 ** -52 * mean_abs)[:, :, None]
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"[specaug] {x.shape} offset {offset}: {int(hit.sum())} filled cells, {int((got != want)[hit].sum())} differ from the "
          f"reference's bits, worst error / bound {float((err[hit] / tol[hit]).max()) if hit.any() else 0.0:.3f}")
    assert (err[hit] <= tol[hit]).all()
    return hit


@pytest.mark.parametrize("fill", ["row_mean", "zero"])
@pytest.mark.parametrize("shape", sorted(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_reference(shape, fill):
    from policy_gradient_asr_amd import hipops
    B, F, T = shape
    lengths, fields = SHAPES[shape]
    pol = _policy(fields, fill)
    x = _features(B, F, T, lengths)
    xd, ld = torch.from_numpy(x).to(DEV), _dev_lengths(lengths)
    ids = list(range(B))
    n_hit = 0
    for offset in (1, 2):
        out, masks = hipops.spec_augment(xd, ld, pol, SEED, offset, want_masks=True)
        assert out.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu(), torch.from_numpy(x))      # out of place: x is not modified
        n_hit += _check_against_reference(out.cpu().numpy(), masks.cpu().numpy(), x, lengths, ids, pol, offset).sum()
        # two runs: the same bits; without the masks: the same tensor
        again = hipops.spec_augment(xd, ld, pol, SEED, offset)
        assert torch.equal(again, out)
        # in place
        xin = xd.clone()
        res = hipops.spec_augment(xin, ld, pol, SEED, offset, out=xin)
        assert res is xin and torch.equal(xin, out)
    assert n_hit > 0
    # ids from the caller: a permutation, a base, then -1 in one row
    perm = [B - 1 - b for b in range(B)]
    pd = torch.tensor(perm, dtype=torch.int32, device=DEV)
    out, masks = hipops.spec_augment(xd, ld, pol, SEED, 1, utt_ids=pd, want_masks=True)
    _check_against_reference(out.cpu().numpy(), masks.cpu().numpy(), x, lengths, perm, pol, 1)
    out_b, masks_b = hipops.spec_augment(xd, ld, pol, SEED, 1, batch_offset=8, want_masks=True)
    _check_against_reference(out_b.cpu().numpy(), masks_b.cpu().numpy(), x, lengths, [8 + b for b in range(B)], pol, 1)
    perm[0] = -1
    pd = torch.tensor(perm, dtype=torch.int32, device=DEV)
    out, masks = hipops.spec_augment(xd, ld, pol, SEED, 1, utt_ids=pd, want_masks=True)
    _check_against_reference(out.cpu().numpy(), masks.cpu().numpy(), x, lengths, perm, pol, 1)
    assert torch.equal(out[0], xd[0]) and not masks[0].any()


def test_identity_refusals_and_the_callable():
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd._lib import PgasrError
    (B, F, T), (lengths, fields) = (8, 80, 60), SHAPES[(8, 80, 60)]
    x = _features(B, F, T, lengths)
    xd, ld = torch.from_numpy(x).to(DEV), _dev_lengths(lengths)
    none = _policy(dict(fields, freq_masks=0, time_masks=0))
    out, masks = hipops.spec_augment(xd, ld, none, SEED, 1, want_masks=True)
    assert torch.equal(out, xd) and tuple(masks.shape) == (B, 0, 2)
    assert hipops.spec_augment(xd, ld, none, SEED, 1, out=xd) is xd and torch.equal(xd.cpu(), torch.from_numpy(x))
    pol = _policy(fields)
    for bad in (lambda: hipops.spec_augment(xd.double(), ld, pol, SEED, 1), lambda: hipops.spec_augment(xd, ld.long(), pol, SEED, 1),
                lambda: hipops.spec_augment(xd.transpose(1, 2), ld, pol, SEED, 1), lambda: hipops.spec_augment(xd.cpu(), ld, pol, SEED, 1),
                lambda: hipops.spec_augment(xd, ld[:4], pol, SEED, 1), lambda: hipops.spec_augment(xd, ld, pol, SEED, 1, out=xd[:4]),
                lambda: hipops.spec_augment(xd, ld, pol, SEED, 1, utt_ids=ld.cpu())):
        with pytest.raises(PgasrError):
            bad()
    # the callable: lengths as a tensor, a host list, or the front end's frame mask
    want = hipops.spec_augment(xd, ld, pol, SEED, 3)
    fmask = (torch.arange(T, device=DEV)[None, :] < ld[:, None]).float()
    for lens in (ld, list(lengths), fmask, fmask[:, None, :]):
        assert torch.equal(pol(xd, lens, seed=SEED, offset=3), want)
    ids = [7, 6, 5, 4, 3, 2, 1, 0]
    assert torch.equal(pol(xd, ld, SEED, 3, utt_ids=ids),
                       hipops.spec_augment(xd, ld, pol, SEED, 3, utt_ids=torch.tensor(ids, dtype=torch.int32, device=DEV)))


def test_shards_and_micro_batches_mask_what_the_whole_batch_masks():
    """Rows 0..15 and 16..31 of a 32-utterance batch masked apart (batch_offset, then ids), an interleaved assignment (even ids, odd
    ids), and a shard padded with empty utterances of id -1: every row gets the bits it gets in one call over the whole batch."""
    from policy_gradient_asr_amd import hipops
    B, F, T = 32, 80, 60
    lengths = [T - (3 * b) % 17 for b in range(B)]
    pol = _policy(FIELDS)
    xd, ld = torch.from_numpy(_features(B, F, T, lengths, seed=3)).to(DEV), _dev_lengths(lengths)
    whole, wmasks = hipops.spec_augment(xd, ld, pol, SEED, 1, want_masks=True)
    assert np.array_equal(wmasks.cpu().numpy(), R.mask_intervals(lengths, list(range(B)), pol, F, SEED, 1))
    for parts, by_offset in (([list(range(16)), list(range(16, 32))], True), ([list(range(0, 32, 2)), list(range(1, 32, 2))], False)):
        for p in parts:
            idx = torch.tensor(p, device=DEV)
            xs, ls = xd.index_select(0, idx).contiguous(), ld.index_select(0, idx).contiguous()
            got, gm = hipops.spec_augment(xs, ls, pol, SEED, 1, utt_ids=idx.to(torch.int32), want_masks=True)
            assert torch.equal(got, whole.index_select(0, idx)) and torch.equal(gm, wmasks.index_select(0, idx))
            if by_offset:
                got, gm = hipops.spec_augment(xs, ls, pol, SEED, 1, batch_offset=p[0], want_masks=True)
                assert torch.equal(got, whole.index_select(0, idx)) and torch.equal(gm, wmasks.index_select(0, idx))
    # five real rows padded to 16 with empty utterances of id -1
    xs = torch.cat((xd[:5], xd.new_zeros(11, F, T)))
    ls = torch.cat((ld[:5], ld.new_zeros(11)))
    ids = torch.tensor(list(range(5)) + [-1] * 11, dtype=torch.int32, device=DEV)
    got, gm = hipops.spec_augment(xs, ls, pol, SEED, 1, utt_ids=ids, want_masks=True)
    assert torch.equal(got[:5], whole[:5]) and not got[5:].any() and torch.equal(gm[:5], wmasks[:5]) and not gm[5:].any()
    # another offset (the next step) draws other intervals
    assert not torch.equal(hipops.spec_augment(xd, ld, pol, SEED, 2, want_masks=True)[1], wmasks)
