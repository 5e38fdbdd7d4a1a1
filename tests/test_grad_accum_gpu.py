"""Gradient accumulation over micro-batches on the MI355X: the id-addressed samplers against the oracle's Philox, an accumulated
step of the real trainer against the whole batch in one call, the once-per-step rules (one Adam update, one clip), peak memory,
train mode, the unchanged default path and ``model.train(accumulate_steps=)``."""
import numpy as np
import pytest
import torch

from oracle import pg_ref
from pg_harness import (ACC_F as F, ACC_L as L, ACC_T as T, ACC_V as V, DEV, _batch, _lens, _rows, _slices, _trainer, make_batch,
                        rel_err, tiny_corpus)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("V_", [29, 64])
def test_id_samplers_vs_philox_oracle(V_):
    from policy_gradient_asr_amd import hipops
    T_, B, K, seed, offset = 200, 8, 8, 1234567, 9
    g = torch.Generator().manual_seed(V_)
    logits = torch.randn(T_, B, V_, generator=g, dtype=torch.float64) * 2      # test_multi_sampler_vs_fp64's inputs
    logits[:, :, 0] += 1.5
    x = logits.float().to(DEV)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    ids = torch.tensor(perm, dtype=torch.int32, device=DEV)
    # the whole batch's draws, column b of the id form = column perm[b] of the draws' addresses: feed row perm[b]'s scores to
    # row b, and the id form must return the whole batch's columns permuted
    xp = x[:, perm].contiguous()
    g_whole, s_whole = hipops.frame_sample_multi(x, K, seed=seed, offset=offset, want_greedy=True)
    g_ids, s_ids = hipops.frame_sample_multi(xp, K, seed=seed, offset=offset, want_greedy=True, batch_stride=B, utt_ids=ids)
    assert torch.equal(s_ids, s_whole[:, :, perm]) and torch.equal(g_ids, g_whole[:, perm])
    g1w, s1w = hipops.frame_argmax_sample(x, seed=seed, offset=offset)
    g1, s1 = hipops.frame_argmax_sample(xp, seed=seed, offset=offset, batch_stride=B, utt_ids=ids)
    assert torch.equal(s1, s1w[:, perm]) and torch.equal(g1, g1w[:, perm]) and torch.equal(s1, s_ids[0])
    # ids = base + arange: the batch_offset form, bit for bit, for both bases of a 4 + 4 split
    for base in (0, 4):
        half = x[:, base:base + 4].contiguous()
        hid = torch.arange(base, base + 4, dtype=torch.int32, device=DEV)
        a = hipops.frame_sample_multi(half, K, seed=seed, offset=offset, want_greedy=True, batch_stride=B, batch_offset=base)
        b = hipops.frame_sample_multi(half, K, seed=seed, offset=offset, want_greedy=True, batch_stride=B, utt_ids=hid)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        a = hipops.frame_argmax_sample(half, seed=seed, offset=offset, batch_stride=B, batch_offset=base)
        b = hipops.frame_argmax_sample(half, seed=seed, offset=offset, batch_stride=B, utt_ids=hid)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # id -1 (and an id >= the stride): a row beyond the global batch, as ctr_base + b >= ctr_stride through the old entry point
    # (rows 5 .. 7 of a batch of 8 with a global batch of 5)
    old1 = hipops.frame_argmax_sample(x, seed=seed, offset=offset, batch_stride=5, batch_offset=0)[1]
    oldk = hipops.frame_sample_multi(x, K, seed=seed, offset=offset, batch_stride=5, batch_offset=0)[1]
    for outside in (-1, 5, 2 ** 31 - 1):
        oid = torch.tensor([0, 1, 2, 3, 4, outside, -1, outside], dtype=torch.int32, device=DEV)
        assert torch.equal(hipops.frame_argmax_sample(x, seed=seed, offset=offset, batch_stride=5, utt_ids=oid)[1], old1)
        assert torch.equal(hipops.frame_sample_multi(x, K, seed=seed, offset=offset, batch_stride=5, utt_ids=oid)[1], oldk)
    assert not torch.equal(old1[:, 5:], s1w[:, 5:])            # .. which is another domain than the ids 5 .. 7
    # the oracle's Philox on counters t * stride + id
    want, cdf, u = pg_ref.sample_paths(xp.double().cpu().numpy(), K, seed, offset, ids=perm, stride=B)
    got = s_ids.cpu().numpy()
    bad = got != want
    near = (np.abs(cdf[None] - u[..., None]) < 1e-6).any(axis=3)
    print(f"[id sampler] V={V_}: {int(bad.sum())} of {bad.size} draws differ, {int(near.sum())} draws near a cdf step")
    assert not (bad & ~near).any()
    assert bad.sum() <= 4
    # the host layer states the counter limit
    with pytest.raises(ValueError):
        hipops.frame_argmax_sample(x, batch_stride=2 ** 25, utt_ids=ids)             # 200 * 2^25 > 2^32
    with pytest.raises(ValueError):
        hipops.frame_sample_multi(x, K, utt_ids=ids)                                 # ids without the global batch


# ---- the accumulated step against the whole batch, through the real trainer ----
def _balanced_parts(B):
    from policy_gradient_asr_amd.train_step import balance_by_frames
    return balance_by_frames(_lens(B)[0], 2)


CASES = {
    "2x16": (32, lambda: _slices((16, 16)), False, {}),
    "3x16": (48, lambda: _slices((16, 16, 16)), False, {}),
    "balanced_ids": (32, lambda: _balanced_parts(32), True, {}),
    "leave_one_out": (32, lambda: _slices((16, 16)), False, {"num_samples": 4, "reward_baseline": "leave_one_out"}),
    "beam": (32, lambda: _slices((16, 16)), False, {"reward_decoder": "beam", "beam_size": 16}),
    "ragged_16_9_7": (32, lambda: _slices((16, 9, 7)), False, {}),
}


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_accumulated_step_is_the_whole_batch(case, precision):
    """accumulate_gradients over micro-batches of the global batch (all padded to T = 60) against compute_gradients of the whole
    batch in one call, identically built trainers, eval mode, lambda = 1: the same sampled paths and rewards exactly, nll and loss
    within 1e-6, gflat within 1e-5 (f32; the bounds of test_ragged_batch_is_padded_with_empty_utterances, which holds the same
    utterances in another batch shape to them) or 1e-3 (bf16x3, that mode's bound in tests/test_train_step_gpu.py)."""
    from policy_gradient_asr_amd import hipops
    B, parts, explicit, kw = CASES[case]
    parts = parts()
    batch, _ = _batch(B)
    whole = _trainer(precision, **kw)
    loss_w = float(whole.compute_gradients(*batch))
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    acc = _trainer(precision, **kw)
    loss_a = float(acc.accumulate_gradients([_rows(batch, p) for p in parts], utt_ids=parts if explicit else None))
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    order = torch.tensor([i for p in parts for i in p], device=DEV)          # row r of the concatenation is utterance order[r]
    nll_w, Rs_w, Rg_w = (s_[order] for s_ in whole.last_stats)
    nll_a, Rs_a, Rg_a = acc.last_stats
    assert all(s_.shape == (B,) for s_ in acc.last_stats)
    K = kw.get("num_samples", 1)
    assert acc.last_sample_rewards.shape == (K, B)
    gerr = rel_err(acc.gflat.cpu(), whole.gflat.cpu())
    nerr = rel_err(nll_a.cpu(), nll_w.cpu())
    lerr = abs(loss_a - loss_w) / abs(loss_w)
    print(f"[grad accum] {case} {precision}: gflat {gerr:.2e} nll {nerr:.2e} loss {lerr:.2e} "
          f"R_s equal {bool(torch.equal(Rs_a, Rs_w))} R_b equal {bool(torch.equal(Rg_a, Rg_w))}")
    gbound, sbound = (1e-5, 1e-6) if precision == "f32" else (1e-3, 1e-3)
    assert torch.equal(acc.last_sample_rewards, whole.last_sample_rewards[:, order])
    assert torch.equal(Rs_a, Rs_w) and torch.equal(Rg_a, Rg_w)
    assert nerr < sbound
    assert lerr <= sbound
    assert gerr < gbound
    assert float(acc.gflat.abs().max()) > 0
    assert acc.nstep == 0


def test_one_optimizer_step_and_one_clip():
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.train_step import FLAG_PAD
    batch, _ = _batch(32)
    mbs = [_rows(batch, p) for p in _slices((16, 16))]
    tr, twin = _trainer(lr=1e-3), _trainer(lr=1e-3)
    flat0 = tr.flat.clone()
    twin.accumulate_gradients(mbs)
    tr.step_accumulated(mbs)
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    assert tr.applied_steps() == 1 and tr.nstep == 1 and twin.nstep == 0
    m, v = torch.zeros_like(flat0), torch.zeros_like(flat0)
    hipops.adam_step(flat0, twin.gflat, m, v, 1, lr=1e-3)
    assert torch.equal(tr.gflat, twin.gflat)
    assert torch.equal(tr.flat, flat0) and torch.equal(tr.exp_avg, m) and torch.equal(tr.exp_avg_sq, v)
    # the next accumulated step draws other paths (offset = nstep + 1)
    first = tr.last_sample_rewards.clone()
    tr.lr = 0.0
    tr.step_accumulated(mbs)
    torch.cuda.synchronize()
    assert tr.nstep == 2 and tr.applied_steps() == 2
    assert not torch.equal(tr.last_sample_rewards, first)

    # clipping: one norm of the accumulated gradient, one count
    tr = _trainer(lr=1e-3, max_grad_norm=1.0)
    tr.step_accumulated(mbs)
    torch.cuda.synchronize()
    want = np.float32(tr.gflat[FLAG_PAD:].double().norm().item())
    got = np.float32(tr.last_grad_norm.item())
    print(f"[grad accum] clip: norm {got!r} against fp64 {want!r}")
    assert abs(got - want) <= np.spacing(want)
    assert want > 1.0 and tr.clip_counts() == (1, 0) and tr.applied_steps() == 1


def test_peak_memory_does_not_grow_with_the_number_of_micro_batches():
    T_ = 200
    lens, tlens = [T_ - (3 * b) % 17 for b in range(64)], [max(1, L - b % 4) for b in range(64)]
    batch = tuple(v.to(DEV) for v in make_batch(64, F, T_, V, L, lens, tlens, 8))
    mbs = [_rows(batch, p) for p in _slices((16,) * 4)]
    one_mb = sum(t.numel() * t.element_size() for t in mbs[0])
    tr = _trainer(lr=1e-4)

    def peak(fn):
        fn()                                            # warm-up: workspaces, streams, weight packs
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    p_step = peak(lambda: tr.step(*batch))
    p4 = peak(lambda: tr.step_accumulated(mbs))
    p2 = peak(lambda: tr.step_accumulated(mbs[:2]))
    print(f"[grad accum] peak bytes: step(B=64) {p_step}  4 x 16 {p4}  2 x 16 {p2}  one micro-batch's inputs {one_mb}")
    assert p4 < p_step
    assert p4 <= p2 + one_mb


def test_train_mode_two_accumulated_steps():
    from policy_gradient_asr_amd import hipops
    batch, _ = _batch(32)
    mbs = [_rows(batch, p) for p in _slices((16, 16))]
    tr = _trainer(train=True, lr=1e-3)
    enc = tr.model.encoder
    calls = [enc._drop_calls]
    orig = tr.forward_loss

    def counted(b, gb):
        out = orig(b, gb)
        calls.append(enc._drop_calls)
        return out
    tr.forward_loss = counted
    losses = [float(tr.step_accumulated(mbs)) for _ in range(2)]
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    assert all(np.isfinite(losses))
    assert [b - a for a, b in zip(calls, calls[1:])] == [3, 3, 3, 3]      # three dropout sites per micro-batch: distinct mask offsets
    assert tr.nstep == 2 and tr.applied_steps() == 2


@pytest.mark.parametrize("B", [32, 21])
def test_default_path_is_unchanged(B):
    """step(batch) and step_accumulated([batch]) run the same launches in the same order: bit-equal gradients and parameters
    (B = 21: a padded batch on one rank keeps the sample_base addressing)."""
    batch, _ = _batch(B)
    a, b = _trainer(lr=1e-3), _trainer(lr=1e-3)
    la = a.step(*batch)
    lb = b.step_accumulated([batch])
    torch.cuda.synchronize()
    assert torch.equal(a.gflat, b.gflat) and torch.equal(a.flat, b.flat) and torch.equal(la, lb)
    assert all(torch.equal(s_, t_) for s_, t_ in zip(a.last_stats, b.last_stats))
    assert a.nstep == b.nstep == 1


def test_model_train_accumulate_steps(tmp_path, capsys):
    from policy_gradient_asr_amd.model import train
    corpus, out, ds = tiny_corpus(tmp_path, 48)                  # 3 loader batches of 16 per epoch: groups of 2 and 1
    kw = dict(train_dataset=ds, n_feats=20, lam=0.0, lr=3e-3, log_every=0)
    l1, _ = train(str(corpus), str(out), 2, 16, 0, accumulate_steps=2, **kw)
    st = torch.load(out / "checkpoint_last.pth", map_location="cpu")
    assert st["nstep"] == 4 and st["applied_steps"] == 4 and st["accumulate_steps"] == 2      # 2 optimizer steps per epoch, not 3
    assert len(l1) == 2 and all(np.isfinite(l1))
    capsys.readouterr()
    l2, _ = train(str(corpus), str(out), 3, 16, 0, accumulate_steps=2, **kw)                  # resumes
    assert len(l2) == 3 and l2[:2] == pytest.approx(l1)
    assert torch.load(out / "checkpoint_last.pth", map_location="cpu")["nstep"] == 6
    assert "Warning" not in capsys.readouterr().out
    train(str(corpus), str(out), 4, 16, 0, accumulate_steps=1, **kw)                          # another value: warned, 3 steps
    assert "resuming with accumulate_steps=1 but the checkpoint was written with 2" in capsys.readouterr().out
    assert torch.load(out / "checkpoint_last.pth", map_location="cpu")["nstep"] == 9
    with pytest.raises(ValueError):
        train(str(corpus), str(out), 5, 16, 0, accumulate_steps=0, **kw)
