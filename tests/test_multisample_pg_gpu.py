"""Multi-sample REINFORCE (K sampled paths per utterance, hypothesis or leave-one-out baseline) against fp64 references:
the multi-draw sampler, the K-path CTC + REINFORCE gradient pass, the rewards / coefficients / loss value, the whole trainer
step in f32 mode, the data-parallel shard identity and the argument checks."""
import numpy as np
import pytest
import torch

from oracle import ctc_ref, decode_ref, model_ref
from test_train_step_gpu import _make

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def multi_uniforms(T, B, K, seed, offset, stride=None, base=0):
    """u[k,t,b]: Philox word 0 of counter (t*stride + base + b, offset, 0, k), key (seed_lo, seed_hi), 24 high bits * 2^-24."""
    stride = B if stride is None else stride
    t, b = np.meshgrid(np.arange(T, dtype=np.uint64), np.arange(B, dtype=np.uint64), indexing="ij")
    c0 = ((t * np.uint64(stride) + np.uint64(base) + b) & np.uint64(0xFFFFFFFF)).astype(np.uint32).ravel()
    c1 = np.full(c0.size, offset & 0xFFFFFFFF, dtype=np.uint32)
    z = np.zeros(c0.size, dtype=np.uint32)
    u = np.empty((K, T, B))
    for k in range(K):
        x0, _, _, _ = decode_ref.philox4x32_10(c0, c1, z, np.full(c0.size, k, dtype=np.uint32), seed & 0xFFFFFFFF,
                                               (seed >> 32) & 0xFFFFFFFF)
        u[k] = ((x0 >> np.uint32(8)).astype(np.float64) * (1.0 / 16777216.0)).reshape(T, B)
    return u


def multi_sample_paths(logits, K, seed, offset):
    """decode_ref.sample_paths with K draws per frame: (paths (K,T,B), cdf (T,B,V), u (K,T,B))."""
    logits = np.asarray(logits, dtype=np.float64)
    T, B, V = logits.shape
    e = np.exp(logits - logits.max(axis=2, keepdims=True))
    cdf = np.cumsum(e, axis=2) / e.sum(axis=2, keepdims=True)
    u = multi_uniforms(T, B, K, seed, offset)
    paths = np.minimum((cdf[None] <= u[..., None]).sum(axis=3), V - 1)
    return paths.astype(np.int64), cdf, u


def baselines(R, R_hyp, mode):
    """b[k,b] in fp64: the hypothesis reward, or the mean of the other samples' rewards."""
    K = R.shape[0]
    if mode == "hypothesis":
        return np.broadcast_to(R_hyp, R.shape)
    return (R.sum(axis=0, keepdims=True) - R) / (K - 1)


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
    want, cdf, u = multi_sample_paths(x.double().cpu().numpy(), K, seed, offset)
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


def _lattice_case(T, B, V, L, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(T, B, V, generator=g, dtype=torch.float64) * 2
    targets = torch.randint(1, V, (B, L), generator=g, dtype=torch.int32)
    in_len = torch.tensor([T - 37 * (b % 4) for b in range(B)], dtype=torch.int32)
    tg_len = torch.tensor([L - 3 * (b % 3) for b in range(B)], dtype=torch.int32)
    return logits, targets, in_len, tg_len


@pytest.mark.parametrize("K", [4, 16])
def test_multi_path_ctc_grad_vs_fp64(K):
    from policy_gradient_asr_amd import hipops
    T, B, V, L = 160, 6, 29, 14
    logits, targets, in_len, tg_len = _lattice_case(T, B, V, L, 40 + K)
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
    b64 = baselines(R64, -dist[:B] / np.maximum(tg_len, 1) if H else None, mode)
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
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.model import Seq2Seq
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    B, F, T, V, L = 4, 80, 120, 29, 12
    lens, tlens = [120, 90, 120, 64], [12, 9, 12, 5]
    x, targets, fmask, tmask = _make(B, F, T, V, L, lens, tlens, seed)
    p = model_ref.init_params(n_feats=F, vocab=V, seed=seed + 1)
    pr = {k: v.double().requires_grad_(True) for k, v in p.items()}
    m = Seq2Seq(V, n_feats=F)
    m.load_state_dict({("encoder." + k if not k.startswith("head.") else k): v for k, v in p.items()}, strict=True)
    m = m.to(DEV).eval()
    tr = PolicyGradientTrainer(m, lam=1.0, seed=3, reward_decoder="beam" if beam else "greedy", beam_size=beam or 16,
                               precision="f32", num_samples=K, reward_baseline=reward_baseline)
    loss = tr.compute_gradients(x.to(DEV), targets.to(DEV), fmask.to(DEV), tmask.to(DEV))
    nll, R_s, R_b = tr.last_stats
    R_all = tr.last_sample_rewards
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    assert R_s.shape == (B,) and R_b.shape == (B,) and R_all.shape == (K, B)

    enc = model_ref.encoder_forward_torch(pr, x.double(), fmask, packed=True)
    logits_ref = model_ref.head_logits_torch(pr, enc)
    lg = logits_ref.detach().numpy()
    il, tl_, tg = np.array(lens), np.array(tlens), targets.numpy()
    paths, _, _ = multi_sample_paths(lg, K, seed=3, offset=1)          # the trainer's first step samples with offset 1
    lp64 = ctc_ref.log_softmax(lg, axis=2)
    Lf = np.maximum(tl_, 1).astype(np.float64)
    R = np.zeros((K, B)); R_hyp = np.zeros(B)
    for b in range(B):
        y = list(tg[b][:tlens[b]])
        for k in range(K):
            R[k, b] = -decode_ref.edit_dist(y, decode_ref.collapse_path(paths[k, :lens[b], b]))[0] / Lf[b]
        if reward_baseline == "hypothesis":
            if beam:
                hyp, _ = decode_ref.prefix_beam_search(np.exp(lp64[:lens[b], b]), beam_size=beam)
                hyp = [h for i, h in enumerate(hyp) if i == 0 or h != hyp[i - 1]]
            else:
                hyp = decode_ref.collapse_path(np.argmax(lg[:lens[b], b], axis=1))
            R_hyp[b] = -decode_ref.edit_dist(y, hyp)[0] / Lf[b]
    bk = baselines(R, R_hyp, reward_baseline)
    coef = (R - bk) / (B * K)
    mask = np.arange(T)[:, None] < il[None, :]
    nll_o, g_ctc = ctc_ref.ctc_loss_and_grad(lg, tg, il, tl_)
    scale = 1.0 / (Lf * B)
    w_loss = (nll_o * scale).sum()
    w_grad = g_ctc * scale[None, :, None]
    for k in range(K):
        lps = (np.take_along_axis(lp64, paths[k][..., None], axis=2)[..., 0] * mask).sum(axis=0)
        w_loss -= (coef[k] * lps).sum()
        w_grad = w_grad + decode_ref.reinforce_grad(lg, paths[k], coef[k], il)
    np.testing.assert_allclose(R_all.cpu().numpy(), R, rtol=1e-6)
    np.testing.assert_allclose(R_s.cpu().numpy(), R.mean(axis=0), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(R_b.cpu().numpy(), bk.mean(axis=0), rtol=1e-6, atol=1e-7)
    assert abs(float(loss) - w_loss) / abs(w_loss) < 1e-5, (float(loss), w_loss)
    logits_ref.backward(torch.from_numpy(w_grad))
    errs = {}
    for k, v in m.named_parameters():
        rk = k[len("encoder."):] if k.startswith("encoder.") else k
        errs[rk] = rel_err(v.grad.cpu(), pr[rk].grad)
    worst = max(errs, key=errs.get)
    print(f"[multi step] K={K} {reward_baseline} beam={beam}: loss rel err {abs(float(loss) - w_loss) / abs(w_loss):.2e}; "
          f"worst parameter gradient {worst} {errs[worst]:.2e}")
    assert errs[worst] < 1e-4, (worst, errs[worst])


def test_multi_sample_step_greedy_hypothesis_vs_oracle():
    _multi_step_vs_oracle("hypothesis", beam=0)


def test_multi_sample_step_leave_one_out_vs_oracle():
    _multi_step_vs_oracle("leave_one_out", beam=0)


def test_multi_sample_step_beam_hypothesis_vs_oracle():
    _multi_step_vs_oracle("hypothesis", beam=16)


def test_leave_one_out_shards_sum_to_the_whole_batch():
    """Two pg_ctc_loss calls on the halves of a batch (global_batch, sample_base set) give the whole batch's logits gradient:
    the leave-one-out baseline of an utterance uses that utterance's samples alone."""
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    T, B, V, L, K = 150, 8, 29, 12, 4
    logits, targets, in_len, tg_len = _lattice_case(T, B, V, L, 77)
    lg = logits.float().to(DEV)
    tg, il, tl = targets.to(DEV), in_len.to(DEV), tg_len.to(DEV)
    kw = dict(lam=1.0, seed=11, offset=4, num_samples=K, baseline="leave_one_out")
    whole = lg.clone().requires_grad_(True)
    loss, nll, R_s, R_b = pg_ctc_loss(whole, il, tg, tl, **kw)
    loss.backward()
    assert R_s.shape == (K, B) and R_b.shape == (B,)
    assert (R_s != R_s[:1]).any()                   # the samples are not all alike
    grads, total = [], 0.0
    for h in range(2):
        sl = slice(4 * h, 4 * h + 4)
        part = lg[:, sl].contiguous().requires_grad_(True)
        l_h, _, Rs_h, _ = pg_ctc_loss(part, il[sl].contiguous(), tg[sl].contiguous(), tl[sl].contiguous(), global_batch=B,
                                      sample_base=4 * h, **kw)
        l_h.backward()
        grads.append(part.grad)
        total += float(l_h.detach())
        assert torch.equal(Rs_h, R_s[:, sl])
    diff = (torch.cat(grads, dim=1) - whole.grad).abs().max()
    assert float(diff) <= 1e-6 * float(whole.grad.abs().max()), float(diff)
    assert abs(total - float(loss)) <= 1e-6 * abs(float(loss))


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
    logits, targets, in_len, tg_len = _lattice_case(40, 2, 29, 5, 1)
    args = (logits.float().to(DEV), in_len.to(DEV), targets.to(DEV), tg_len.to(DEV))
    with pytest.raises(ValueError):
        pg_ctc_loss(*args, num_samples=17)
    with pytest.raises(ValueError):
        pg_ctc_loss(*args, num_samples=1, baseline="leave_one_out")
    with pytest.raises(ValueError):
        pg_ctc_loss(*args, num_samples=4, per_step=True)


def test_train_driver_records_multi_sample_settings(tmp_path, capsys):
    """model.train(num_samples, reward_baseline): trains with them, records them in the checkpoint, warns on a resume with others."""
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.model import train
    corpus = tmp_path / "corpus"; out = tmp_path / "run"
    corpus.mkdir()
    (corpus / "alphabet.txt").write_text("a\nb\nc\nd\n \n")
    char2ind = {"<pad>": 0, "a": 1, "b": 2, "c": 3, "d": 4, " ": 5}
    ds = SyntheticSpeech(32, char2ind, n_feats=20, seed=1)
    l1, _ = train(str(corpus), str(out), 2, 16, 0, train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=0,
                  num_samples=4, reward_baseline="leave_one_out")
    assert len(l1) == 2 and all(np.isfinite(l1))
    st = torch.load(out / "checkpoint_last.pth", map_location="cpu")
    assert (st["num_samples"], st["reward_baseline"]) == (4, "leave_one_out")
    capsys.readouterr()
    train(str(corpus), str(out), 3, 16, 0, train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=0, num_samples=2)
    printed = capsys.readouterr().out
    assert "num_samples=2" in printed and "reward_baseline=hypothesis" in printed
