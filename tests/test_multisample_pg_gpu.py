"""Multi-sample REINFORCE (K sampled paths per utterance, hypothesis or leave-one-out baseline) against fp64 references:
the multi-draw sampler, the K-path CTC + REINFORCE gradient pass, the rewards / coefficients / loss value, the whole trainer
step in f32 mode, the data-parallel shard identity and the argument checks."""
import numpy as np
import pytest
import torch

from oracle import ctc_ref, decode_ref, pg_ref
from pg_harness import DEV, lattice_case, rel_err, shards_vs_whole, tiny_corpus, trainer_step_vs_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("V", [29, 64])
def test_multi_sampler_vs_fp64(V):
    from policy_gradient_asr_amd import hipops
    T, B, K, seed, offset = 200, 8, 8, 1234567, 9
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(T, B, V, generator=g, dtype=torch.float64) * 2
    logits[:, :, 0] += 1.5
    x = logits.float().to(DEV)
    greedy, samples = hipops.frame_sample_multi(x, K, seed=seed, offset=offset, want_greedy=True)
    assert samples.shape == (K, T, B)
    want, cdf, u = pg_ref.sample_paths(x.double().cpu().numpy(), K, seed, offset)
    got = samples.cpu().numpy()
    bad = got != want
    # a disagreement is only allowed where u lies within 1e-6 of a cdf step (fp32 prefix sum against fp64)
    near = (np.abs(cdf[None] - u[..., None]) < 1e-6).any(axis=3)
    print(f"[multi sampler] V={V}: {int(bad.sum())} of {bad.size} draws differ, {int(near.sum())} draws near a cdf step")
    assert not (bad & ~near).any()
    assert bad.sum() <= 4
    # the K draws are distinct draws (not one draw repeated)
    assert (got[0] != got[1]).mean() > 0.3
    g1, s1 = hipops.frame_argmax_sample(x, seed=seed, offset=offset)
    assert torch.equal(samples[0], s1) and torch.equal(greedy, g1)
    # two half-batches addressed globally draw what the whole batch draws
    halves = [hipops.frame_sample_multi(x[:, h * 4:(h + 1) * 4].contiguous(), K, seed=seed, offset=offset, batch_stride=B,
                                        batch_offset=4 * h)[1] for h in range(2)]
    assert torch.equal(torch.cat(halves, dim=2), samples)


@pytest.mark.parametrize("K", [4, 16])
def test_multi_path_ctc_grad_vs_fp64(K):
    from policy_gradient_asr_amd import hipops
    T, B, V, L = 160, 6, 29, 14
    logits, targets, in_len, tg_len = lattice_case(T, B, V, L, 40 + K)
    g = torch.Generator().manual_seed(K)
    paths = torch.randint(0, V, (K, T, B), generator=g, dtype=torch.int32)
    coef = torch.randn(K, B, generator=g) * 0.1
    scale = torch.rand(B, generator=g) + 0.5
    lp = hipops.log_softmax_rows(logits.float().to(DEV))
    il, tl, tg = in_len.to(DEV), tg_len.to(DEV), targets.to(DEV)
    nll, handle = hipops.ctc_lattice(lp, tg, il, tl)
    grad = hipops.ctc_grad_from_lattice_multi(lp, il, tl, handle, scale.to(DEV), coef.to(DEV), paths.to(DEV))
    lg = lp.double().cpu().numpy()           # the device's log-probs: d/dlogits is the same for any logits with this softmax
    _, g_ctc = ctc_ref.ctc_loss_and_grad(lg, targets.numpy(), in_len.numpy(), tg_len.numpy())
    want = g_ctc * scale.double().numpy()[None, :, None]
    for k in range(K):
        want = want + decode_ref.reinforce_grad(lg, paths[k].numpy(), coef[k].double().numpy(), in_len.numpy())
    err = rel_err(grad.cpu().numpy(), want)
    print(f"[multi grad] K={K}: rel err {err:.2e}")
    assert err < 1e-5
    # K = 1 through the multi kernel is the single-path pass, bit for bit
    one = hipops.ctc_grad_from_lattice_multi(lp, il, tl, handle, scale.to(DEV), coef[:1].to(DEV), paths[:1].to(DEV))
    ref1 = hipops.ctc_grad_from_lattice(lp, il, tl, handle, utt_scale=scale.to(DEV), pg_coef=coef[0].to(DEV),
                                        pg_path=paths[0].to(DEV))
    assert torch.equal(one, ref1)


@pytest.mark.parametrize("mode", ["hypothesis", "leave_one_out"])
def test_multi_rewards_and_loss_value_vs_numpy(mode):
    from policy_gradient_asr_amd import hipops
    B, K, lam, Bg = 37, 5, 0.7, 64
    rng = np.random.default_rng(3)
    H = 1 if mode == "hypothesis" else 0
    dist = rng.integers(0, 30, size=(H + K) * B).astype(np.int32)
    tg_len = rng.integers(0, 25, size=B).astype(np.int32)
    R_b, R_s, coef, us = hipops.pg_rewards_multi(torch.from_numpy(dist).to(DEV), torch.from_numpy(tg_len).to(DEV), K, lam, 1.0 / Bg,
                                                 baseline=mode)
    # fp32 in the kernel's order
    f = np.float32
    Lf = np.maximum(tg_len, 1).astype(f)
    R = -(dist[H * B:].reshape(K, B).astype(f)) / Lf
    if mode == "hypothesis":
        bk = np.broadcast_to(-(dist[:B].astype(f)) / Lf, (K, B))
        Rb = bk[0]
    else:
        S = np.zeros(B, dtype=f)
        for k in range(K):
            S = (S + R[k]).astype(f)
        bk = ((S[None] - R) / f(K - 1)).astype(f)
        Rb = np.zeros(B, dtype=f)
        for k in range(K):
            Rb = (Rb + bk[k]).astype(f)
        Rb = Rb / f(K)
    scale = (f(lam) * f(1.0 / Bg)) / f(K)
    np.testing.assert_allclose(R_s.cpu().numpy(), R, rtol=1e-7, atol=0)
    np.testing.assert_allclose(coef.cpu().numpy(), scale * (R - bk), rtol=2e-7, atol=1e-12)
    np.testing.assert_allclose(R_b.cpu().numpy(), Rb, rtol=2e-7, atol=1e-12)
    np.testing.assert_allclose(us.cpu().numpy(), f(1.0 / Bg) / Lf, rtol=1e-7)
    # the same against the fp64 definition
    R64 = -dist[H * B:].reshape(K, B) / np.maximum(tg_len, 1)
    b64 = np.broadcast_to(-dist[:B] / np.maximum(tg_len, 1), R64.shape) if H else (R64.sum(axis=0, keepdims=True) - R64) / (K - 1)
    np.testing.assert_allclose(coef.cpu().numpy(), lam / (Bg * K) * (R64 - b64), rtol=1e-5, atol=1e-8)

    # loss value: nll_b utt_scale_b - sum_k coef[k,b] sum_{t<T_b} log p(paths[k,t,b])
    T, V = 90, 29
    g = torch.Generator().manual_seed(5)
    lp = torch.log_softmax(torch.randn(T, B, V, generator=g, dtype=torch.float64), dim=2)
    paths = torch.randint(0, V, (K, T, B), generator=g, dtype=torch.int32)
    in_len = torch.randint(0, T + 1, (B,), generator=g, dtype=torch.int32)
    nll = torch.rand(B, generator=g) * 50
    terms = hipops.pg_loss_value_multi(lp.float().to(DEV), paths.to(DEV), in_len.to(DEV), nll.to(DEV), us, coef)
    lp32 = lp.float().double().numpy()
    mask = np.arange(T)[:, None] < in_len.numpy()[None, :]
    c64, u64 = coef.cpu().double().numpy(), us.cpu().double().numpy()
    want = nll.double().numpy() * u64
    for k in range(K):
        lps = (np.take_along_axis(lp32, paths[k].long().numpy()[..., None], axis=2)[..., 0] * mask).sum(axis=0)
        want = want - c64[k] * lps
    assert rel_err(terms.cpu().numpy(), want) < 1e-6
    assert abs(float(terms.sum()) - want.sum()) / abs(want.sum()) < 1e-6
    again = hipops.pg_loss_value_multi(lp.float().to(DEV), paths.to(DEV), in_len.to(DEV), nll.to(DEV), us, coef)
    assert torch.equal(terms, again)


def _multi_step_vs_oracle(reward_baseline, beam, K=4, seed=51):
    """One lambda = 1 trainer step (f32 mode) with K samples against the torch-CPU model in FP64 on the same weights: rewards exact,
    loss within 1e-5, every parameter gradient within 1e-4 (max norm)."""
    r = trainer_step_vs_oracle(dict(reward_decoder="beam" if beam else "greedy", beam_size=beam or 16, num_samples=K,
                                    reward_baseline=reward_baseline),
                               dict(num_samples=K, baseline=reward_baseline, beam=beam), seed=seed,
                               label=f"[multi step] K={K} {reward_baseline} beam={beam}")
    tr = r.trainer
    assert all(s_.shape == (4,) for s_ in tr.last_stats) and tr.last_sample_rewards.shape == (K, 4)


def test_multi_sample_step_greedy_hypothesis_vs_oracle():
    _multi_step_vs_oracle("hypothesis", beam=0)


def test_multi_sample_step_leave_one_out_vs_oracle():
    _multi_step_vs_oracle("leave_one_out", beam=0)


def test_multi_sample_step_beam_hypothesis_vs_oracle():
    _multi_step_vs_oracle("hypothesis", beam=16)


def test_leave_one_out_shards_sum_to_the_whole_batch():
    """Two pg_ctc_loss calls on the halves of a batch (global_batch, sample_base set) give the whole batch's logits gradient:
    the leave-one-out baseline of an utterance uses that utterance's samples alone."""
    T, B, V, L, K = 150, 8, 29, 12, 4
    r = shards_vs_whole(dict(lam=1.0, seed=11, offset=4, num_samples=K, baseline="leave_one_out"), lattice_case(T, B, V, L, 77))
    assert r.R_s.shape == (K, B) and r.R_b.shape == (B,)
    assert (r.R_s != r.R_s[:1]).any()                   # the samples are not all alike


def test_multi_sample_argument_checks():
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    from policy_gradient_asr_amd.model import Seq2Seq
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    m = Seq2Seq(29, n_feats=80).to(DEV)
    with pytest.raises(ValueError, match="16"):
        PolicyGradientTrainer(m, num_samples=17)
    with pytest.raises(ValueError, match="leave-one-out"):
        PolicyGradientTrainer(m, num_samples=1, reward_baseline="leave_one_out")
    with pytest.raises(ValueError, match="per-step"):
        PolicyGradientTrainer(m, num_samples=4, reward_mode="per_step")
    with pytest.raises(ValueError):
        PolicyGradientTrainer(m, num_samples=4, reward_baseline="batch_mean")
    tr = PolicyGradientTrainer(m, num_samples=16, reward_baseline="leave_one_out")
    assert (tr.num_samples, tr.reward_baseline) == (16, "leave_one_out")
    logits, targets, in_len, tg_len = lattice_case(40, 2, 29, 5, 1)
    args = (logits.float().to(DEV), in_len.to(DEV), targets.to(DEV), tg_len.to(DEV))
    with pytest.raises(ValueError):
        pg_ctc_loss(*args, num_samples=17)
    with pytest.raises(ValueError):
        pg_ctc_loss(*args, num_samples=1, baseline="leave_one_out")
    with pytest.raises(ValueError):
        pg_ctc_loss(*args, num_samples=4, per_step=True)


def test_train_driver_records_multi_sample_settings(tmp_path, capsys):
    """model.train(num_samples, reward_baseline): trains with them, records them in the checkpoint, warns on a resume with others."""
    from policy_gradient_asr_amd.model import train
    corpus, out, ds = tiny_corpus(tmp_path)
    l1, _ = train(str(corpus), str(out), 2, 16, 0, train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=0,
                  num_samples=4, reward_baseline="leave_one_out")
    assert len(l1) == 2 and all(np.isfinite(l1))
    st = torch.load(out / "checkpoint_last.pth", map_location="cpu")
    assert (st["num_samples"], st["reward_baseline"]) == (4, "leave_one_out")
    capsys.readouterr()
    train(str(corpus), str(out), 3, 16, 0, train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=0, num_samples=2)
    printed = capsys.readouterr().out
    assert "num_samples=2" in printed and "reward_baseline=hypothesis" in printed
