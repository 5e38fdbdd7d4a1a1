"""Per-step rewards with K samples, the leave-one-out baseline and wide alphabets (include/pgasr_hip.h, A12-STEP) on the device:
pgasr_pg_step_coefs_multi, pgasr_ctc_grad_from_lattice_multi_steps and pgasr_pg_loss_value_multi_steps against
tests/step_rewards_ref.py, then pg_ctc_loss, shards, one trainer step and the train driver with step_objectives=True.

Bounds.
    coefficients  |device - ref| <= 1e-6 * kf_b * max(1, max |G|): the integers G, S and their differences are exact in fp32; kf_b takes
                  three fp32 roundings and the leave-one-out expression a quotient and a product more -- at most five roundings of
                  2^-24, 3e-7, each relative to an intermediate of at most kf_b times a small multiple of max |G|.  The difference
                  G_k - b_k cancels, so the bound is absolute in units of kf_b max |G|, not relative to the coefficient.
    gradient pass max-norm error < 1e-5, absolute and relative to the largest reference entry, and the loss value's terms within 1e-6
                  relative (max norm): the bounds of tests/test_wide_pg_gpu.py and tests/test_multisample_pg_gpu.py for the same passes
                  with per-utterance coefficients -- the same arithmetic at another coefficient address.
    objective     loss 1e-5 relative, d(logits) 1e-5 of the oracle's max norm; trainer step: loss 1e-5, parameter gradients 1e-4."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import ctc_ref, pg_ref

import kl_ref
import step_rewards_ref as sr
from pg_harness import DEV, lattice_case, oracle_model, oracle_step, param_errs, rel_err, shards_vs_whole, step_batch, tiny_corpus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from policy_gradient_asr_amd import hipops
    return hipops


def _i32(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the coefficient kernel ----
def _device_rows(ops, c):
    """The collapsed forms and per-prefix distances of the case's rows as the loss section makes them."""
    rows, il, tg, tl = _i32(c.rows), _i32(c.in_len), _i32(c.targets), _i32(c.tg_len)
    tokens, tok_len = ops.ctc_collapse(rows, il, blank=c.blank)
    _, prefix = ops.edit_distance(tg.repeat(c.P, 1), tl.repeat(c.P), tokens.view(c.P * c.B, c.T), tok_len.view(c.P * c.B), want_prefix=True)
    return rows, il, tl, prefix, tok_len


@pytest.mark.parametrize("baseline", ["hypothesis", "leave_one_out"])
@pytest.mark.parametrize("K", sr.COEF_K)
@pytest.mark.parametrize("T", sr.COEF_T)
def test_step_coefs_multi_vs_fp64(ops, T, K, baseline):
    if baseline == "leave_one_out" and K == 1:
        from policy_gradient_asr_amd import _lib
        c = sr.seam_case(T, 1, 0, "hypothesis")
        rows, il, tl, prefix, tok_len = _device_rows(ops, c)
        with pytest.raises(_lib.PgasrError):
            ops.pg_step_coefs_multi(rows[1:], il, prefix[c.B:], tok_len[1:].reshape(-1), tl, 1, 0.7, 0.25, baseline="leave_one_out")
        return
    lam, Bg = 0.7, 4
    for blank in (0, sr.COEF_V - 1):
        c = sr.seam_case(T, K, blank, baseline)
        rows, il, tl, prefix, tok_len = _device_rows(ops, c)
        got = ops.pg_step_coefs_multi(rows, il, prefix, tok_len.reshape(-1), tl, K, lam, 1.0 / Bg, baseline=baseline, blank=blank)
        assert got.shape == (K, T, c.B)
        want = sr.step_coefs(c.paths, c.greedy, c.in_len, c.targets, c.tg_len, baseline, lam, Bg, blank)
        G = np.abs(sr.rewards_to_go(c.rows, c.in_len, c.targets, c.tg_len, blank)).max(axis=(0, 1))             # (B,)
        kf = lam / (Bg * K * np.maximum(c.tg_len, 1))
        err = np.abs(got.cpu().numpy().astype(np.float64) - want).max(axis=(0, 1))
        bound = 1e-6 * kf * np.maximum(1, G)
        print(f"[step coefs] T={T} K={K} {baseline} blank={blank}: max err / bound {np.max(err / bound):.2e}, max |G| {G.max():.0f}, "
              f"max |coef| {np.abs(want).max():.3f}")
        assert (err <= bound).all(), (err, bound)
        g = got.cpu().numpy()
        for b in range(c.B):
            assert (g[:, c.in_len[b]:, b] == 0).all()
        if T > 1:
            assert np.abs(want).max() > 0
        again = ops.pg_step_coefs_multi(rows, il, prefix, tok_len.reshape(-1), tl, K, lam, 1.0 / Bg, baseline=baseline, blank=blank)
        assert torch.equal(_bits(got), _bits(again))
        if K == 1 and baseline == "hypothesis":
            one = ops.pg_step_coefs(rows, il, prefix, tok_len.reshape(-1), tl, lam, 1.0 / Bg, blank=blank)
            assert torch.equal(_bits(got[0]), _bits(one))


# ---- the gradient pass and the loss value ----
GRAD_V = (2, 29, 64, 65, 200, 300, 1024)          # NV = 1, 1, 1, 2, 4, 8, 16
GT, GB, GL, GK = 20, 3, 5, 4
TAILS = ["none", "entropy", "entropy+kl"]
BETA, GAMMA = 2.0, 2.0


@functools.lru_cache(maxsize=None)
def _grad_case(V):
    """T = 20, B = 3, L = 5 on random log-probs: utterance 1 has 8 frames for a target of five equal symbols, which needs 9 (nll =
    +inf, no CTC part), utterance 2 has 13 of the 20 frames.  Four paths per utterance from the device's sampler, per-frame
    coefficients and scales random, a second random tensor as the KL reference."""
    from policy_gradient_asr_amd import hipops
    g = torch.Generator().manual_seed(4000 + V)
    logits = torch.randn(GT, GB, V, generator=g, dtype=torch.float64) * 2
    lp = torch.log_softmax(logits, dim=2).float()
    lq = torch.log_softmax(torch.randn(GT, GB, V, generator=g, dtype=torch.float64) * 2, dim=2).float()
    targets = torch.randint(1, V, (GB, GL), generator=g, dtype=torch.int32)
    # utterance 1: five equal symbols need 5 + 4 = 9 frames; with in_len 8 the target is infeasible (nll = +inf)
    targets[1, :] = 1
    in_len = torch.tensor([20, 8, 13], dtype=torch.int32)
    tg_len = torch.tensor([5, 5, 3], dtype=torch.int32)
    coef = torch.randn(GK, GT, GB, generator=g) * 0.1
    scale = torch.rand(GB, generator=g) + 0.5
    lpd = lp.to(DEV)
    _, paths = hipops.frame_sample_multi(lpd, GK, seed=11, offset=4)
    lg = lp.double().numpy()
    nll, _ = ctc_ref.ctc_loss_and_grad(lg, targets.numpy(), in_len.numpy(), tg_len.numpy())
    assert np.isinf(nll[1]) and np.isfinite(nll[[0, 2]]).all()
    return dict(V=V, lp=lpd, lg=lg, ref=lq.to(DEV), rg=lq.double().numpy(), targets=targets, tg=targets.to(DEV), in_len=in_len,
                il=in_len.to(DEV), tg_len=tg_len, tl=tg_len.to(DEV), paths=paths, pn=paths.cpu().numpy(), coef=coef, scale=scale)


def _tails(ops, c, tail):
    kw, want = {}, 0.0
    il = c["in_len"].numpy()
    if tail in ("entropy", "entropy+kl"):
        kw["ent_scale"] = ops.frame_entropy(c["lp"], c["il"], BETA, 1.0 / GB)[1]
        want = want + pg_ref.entropy_grad(c["lg"], il, kw["ent_scale"].double().cpu().numpy())
    if tail == "entropy+kl":
        kw.update(ref_log_probs=c["ref"], kl_scale=ops.frame_kl(c["lp"], c["ref"], c["il"], GAMMA, 1.0 / GB)[1])
        want = want + kl_ref.kl_grad(c["lg"], c["rg"], il, kw["kl_scale"].double().cpu().numpy())
    return kw, want


@pytest.mark.parametrize("K", [1, GK])
@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("V", GRAD_V)
def test_gradient_pass_and_loss_value_with_frame_coefficients(ops, V, tail, K):
    c = _grad_case(V)
    il = c["in_len"].numpy()
    coef, paths, scale = c["coef"][:K].contiguous().to(DEV), c["paths"][:K].contiguous(), c["scale"].to(DEV)
    kw, want_tail = _tails(ops, c, tail)
    nll, handle = ops.ctc_lattice(c["lp"], c["tg"], c["il"], c["tl"])
    grad = ops.ctc_grad_from_lattice_multi(c["lp"], c["il"], c["tl"], handle, scale, coef, paths, **kw)
    assert torch.equal(_bits(grad), _bits(ops.ctc_grad_from_lattice_multi(c["lp"], c["il"], c["tl"], handle, scale, coef, paths, **kw)))
    # the reference on the device's fp32 log-probs: CTC part with the test's scales, the K per-frame REINFORCE terms, the tails
    nll64, g_ctc = ctc_ref.ctc_loss_and_grad(c["lg"], c["targets"].numpy(), il, c["tg_len"].numpy())
    sc64, c64 = c["scale"].double().numpy(), c["coef"][:K].double().numpy()
    o = sr.step_objective(c["lg"], il, c["targets"].numpy(), c["tg_len"].numpy(), paths=c["pn"][:K], coef=c64)
    # step_objective scales the CTC part by 1 / (Bg max(L,1)); put the test's own scales in its place
    own = 1.0 / (GB * np.maximum(c["tg_len"].numpy(), 1))
    want = o.grad + g_ctc * (sc64 - own)[None, :, None] + want_tail
    got = grad.cpu().numpy().astype(np.float64)
    err, rerr = float(np.abs(got - want).max()), rel_err(got, want)
    print(f"[step grad] V={V} K={K} {tail}: max err {err:.2e}, rel {rerr:.2e} (largest reference entry {np.abs(want).max():.2f})")
    assert np.isfinite(got).all() and err < 1e-5 and rerr < 1e-5
    beyond = np.arange(GT)[:, None] >= il[None, :]
    assert beyond.any() and (got[beyond] == 0).all()
    # the per-frame coefficients are visible at this bound: the per-utterance form with frame 0's coefficients is far away
    flat = ops.ctc_grad_from_lattice_multi(c["lp"], c["il"], c["tl"], handle, scale, coef[:, 0].contiguous(), paths, **kw)
    assert rel_err(flat.cpu().numpy(), want) > 1e-3

    terms = ops.pg_loss_value_multi(c["lp"], paths, c["il"], nll, scale, coef)
    mask = np.arange(GT)[:, None] < il[None, :]
    want_terms = nll.double().cpu().numpy() * sc64
    for k in range(K):
        want_terms = want_terms - (c64[k] * np.take_along_axis(c["lg"], c["pn"][k].astype(np.int64)[..., None], axis=2)[..., 0] * mask).sum(axis=0)
    live = np.isfinite(want_terms)
    assert live.sum() == 2 and np.array_equal(np.isfinite(terms.cpu().numpy()), live)
    assert rel_err(terms.cpu().numpy()[live], want_terms[live]) < 1e-6
    assert torch.equal(_bits(terms), _bits(ops.pg_loss_value_multi(c["lp"], paths, c["il"], nll, scale, coef)))


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("V", GRAD_V)
def test_constant_frame_coefficients_give_the_per_utterance_bits(ops, V, tail):
    c = _grad_case(V)
    kw, _ = _tails(ops, c, tail)
    nll, handle = ops.ctc_lattice(c["lp"], c["tg"], c["il"], c["tl"])
    scale = c["scale"].to(DEV)
    # Coefficients +-2^-(2..5): the per-frame loss value weighs every term inside the sum where the per-utterance one weighs the sum,
    # and scaling by a power of two commutes with every rounding, so the two sums have the same bits.  (The gradient pass reads one
    # coefficient per row either way and would agree for any value.)
    pow2 = torch.tensor([[0.25, -0.125, 0.0625], [-0.03125, 0.25, -0.25], [0.125, 0.0625, -0.125], [-0.25, 0.03125, 0.125]])
    for K in (1, GK):
        paths = c["paths"][:K].contiguous()
        utt = pow2[:K].contiguous().to(DEV)                                  # (K,B)
        frames = utt[:, None, :].expand(K, GT, GB).contiguous()              # (K,T,B), constant over t
        g_u = ops.ctc_grad_from_lattice_multi(c["lp"], c["il"], c["tl"], handle, scale, utt, paths, **kw)
        g_f = ops.ctc_grad_from_lattice_multi(c["lp"], c["il"], c["tl"], handle, scale, frames, paths, **kw)
        assert torch.equal(_bits(g_u), _bits(g_f)) and float(g_u.abs().max()) > 0
        t_u = ops.pg_loss_value_multi(c["lp"], paths, c["il"], nll, scale, utt)
        t_f = ops.pg_loss_value_multi(c["lp"], paths, c["il"], nll, scale, frames)
        assert torch.equal(_bits(t_u), _bits(t_f))
    if V <= 64 and tail == "none":
        # K = 1: the multi per-frame pass is the single-path pass with a (T,B) coefficient, and so is the loss value
        one = c["coef"][:1].contiguous().to(DEV)
        g_m = ops.ctc_grad_from_lattice_multi(c["lp"], c["il"], c["tl"], handle, scale, one, c["paths"][:1].contiguous())
        g_s = ops.ctc_grad_from_lattice(c["lp"], c["il"], c["tl"], handle, utt_scale=scale, pg_coef=one[0].contiguous(),
                                        pg_path=c["paths"][0].contiguous())
        assert torch.equal(_bits(g_m), _bits(g_s))
        t_m = ops.pg_loss_value_multi(c["lp"], c["paths"][:1].contiguous(), c["il"], nll, scale, one)
        t_s = ops.pg_loss_value(c["lp"], c["paths"][0].contiguous(), c["il"], nll, scale, one[0].contiguous())
        assert torch.equal(_bits(t_m), _bits(t_s))


# ---- pg_ctc_loss ----
OBJ = dict(T=120, B=4, L=12)
OBJ_IL, OBJ_TL = np.array([120, 90, 120, 64]), np.array([12, 9, 12, 5])


@functools.lru_cache(maxsize=None)
def _objective_inputs(V):
    g = torch.Generator().manual_seed(5 + V)
    logits = torch.randn(OBJ["T"], OBJ["B"], V, generator=g) * 2
    targets = torch.randint(1, V, (OBJ["B"], OBJ["L"]), generator=g, dtype=torch.int32)
    ref = torch.log_softmax(torch.randn(OBJ["T"], OBJ["B"], V, generator=g, dtype=torch.float64) * 2, dim=2).float()
    return logits, targets, ref


@pytest.mark.parametrize("baseline", ["hypothesis", "leave_one_out"])
@pytest.mark.parametrize("V", [29, 300])
def test_pg_ctc_loss_per_step_vs_oracle(ops, V, baseline):
    """K = 4 with the entropy bonus and the KL anchor against step_objective on the DEVICE's paths and greedy frames; R_s and R_b are
    the utterance-level call's bits; without the keyword the call is refused as it always was."""
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    K, beta, gamma = 4, 0.1, 0.1
    logits, targets, ref = _objective_inputs(V)
    ild, tld = _i32(OBJ_IL), _i32(OBJ_TL)
    wide = {"wide_objectives": True} if V > 64 else {}
    call = dict(lam=1.0, seed=3, offset=1, num_samples=K, baseline=baseline, entropy_weight=beta, kl_weight=gamma,
                ref_log_probs=ref.to(DEV), **wide)
    z = logits.to(DEV).requires_grad_(True)
    loss, nll, R_s, R_b = pg_ctc_loss(z, ild, targets.to(DEV), tld, per_step=True, step_objectives=True, **call)
    loss.backward()
    lp_dev = ops.log_softmax_rows(logits.to(DEV))
    greedy, paths = ops.frame_sample_multi(lp_dev, K, seed=3, offset=1, want_greedy=True)
    o = sr.step_objective(logits.double().numpy(), OBJ_IL, targets.numpy(), OBJ_TL, paths=paths.cpu().numpy(),
                          greedy_frames=greedy.cpu().numpy(), baseline=baseline, lam=1.0, entropy_weight=beta, kl_weight=gamma,
                          ref_log_probs=ref.double().numpy())
    lerr = abs(float(loss) - o.loss) / abs(o.loss)
    gerr = rel_err(z.grad.cpu(), o.grad)
    print(f"[step objective] V={V} {baseline}: loss rel err {lerr:.2e}, d(logits) rel err {gerr:.2e}, max |coef| {np.abs(o.coef).max():.2e}")
    assert lerr <= 1e-5 and gerr <= 1e-5
    assert np.ptp(o.coef[:, :60], axis=1).max() > 0
    _, _, R_s_u, R_b_u = pg_ctc_loss(logits.to(DEV), ild, targets.to(DEV), tld, **call)
    assert torch.equal(_bits(R_s), _bits(R_s_u)) and torch.equal(_bits(R_b), _bits(R_b_u)) and R_s.shape == (K, OBJ["B"])
    with pytest.raises(ValueError, match="one sampled path"):
        pg_ctc_loss(logits.to(DEV), ild, targets.to(DEV), tld, per_step=True, **call)


def test_one_sample_keeps_its_launches_and_bits(ops, monkeypatch):
    """K = 1 against the greedy path without tails: with the keyword the call is the call without it -- the single-path kernels, none
    of the multi-sample family, the same bits -- at 29 symbols; at 300 symbols, where the keyword is what admits the call, the
    single-path wide gradient pass runs with per-frame coefficients for the first time and is held to the oracle."""
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    ild, tld = _i32(OBJ_IL), _i32(OBJ_TL)
    logits, targets, _ = _objective_inputs(29)
    real = {fn: getattr(ops, fn) for fn in ("frame_sample_multi", "ctc_grad_from_lattice_multi", "pg_loss_value_multi",
                                            "pg_step_coefs_multi")}
    called = []
    for fn in real:
        monkeypatch.setattr(ops, fn, lambda *a, _fn=fn, **k: called.append(_fn))
    out = []
    for kw in ({}, {"step_objectives": True}):
        z = logits.to(DEV).requires_grad_(True)
        loss, _, R_s, R_b = pg_ctc_loss(z, ild, targets.to(DEV), tld, lam=1.0, seed=3, offset=1, per_step=True, **kw)
        loss.backward()
        out.append((loss.detach(), z.grad, R_s, R_b))
    assert not called
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*out))

    logits, targets, _ = _objective_inputs(300)
    with pytest.raises(ValueError, match="per_step"):
        pg_ctc_loss(logits.to(DEV), ild, targets.to(DEV), tld, lam=1.0, seed=3, offset=1, per_step=True)
    z = logits.to(DEV).requires_grad_(True)
    loss, _, R_s, R_b = pg_ctc_loss(z, ild, targets.to(DEV), tld, lam=1.0, seed=3, offset=1, per_step=True, step_objectives=True)
    loss.backward()
    assert not called
    for fn, f in real.items():
        monkeypatch.setattr(ops, fn, f)
    greedy, sample = ops.frame_argmax_sample(ops.log_softmax_rows(logits.to(DEV)), seed=3, offset=1)
    o = sr.step_objective(logits.double().numpy(), OBJ_IL, targets.numpy(), OBJ_TL, paths=sample.cpu().numpy()[None],
                          greedy_frames=greedy.cpu().numpy(), lam=1.0)
    lerr, gerr = abs(float(loss) - o.loss) / abs(o.loss), rel_err(z.grad.cpu(), o.grad)
    print(f"[step objective] V=300 K=1 single-path wide pass: loss rel err {lerr:.2e}, d(logits) rel err {gerr:.2e}")
    assert lerr <= 1e-5 and gerr <= 1e-5 and np.abs(o.coef).max() > 0 and R_s.shape == (OBJ["B"],)


def test_one_sample_with_tails_above_64_symbols(ops):
    """K = 1, greedy baseline, entropy and KL at 300 symbols: the multi-sample per-frame family with K = 1; R_s stays (B,)."""
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    logits, targets, ref = _objective_inputs(300)
    ild, tld = _i32(OBJ_IL), _i32(OBJ_TL)
    z = logits.to(DEV).requires_grad_(True)
    loss, _, R_s, R_b = pg_ctc_loss(z, ild, targets.to(DEV), tld, lam=1.0, seed=3, offset=1, per_step=True, step_objectives=True,
                                    wide_objectives=True, entropy_weight=0.1, kl_weight=0.1, ref_log_probs=ref.to(DEV))
    loss.backward()
    greedy, paths = ops.frame_sample_multi(ops.log_softmax_rows(logits.to(DEV)), 1, seed=3, offset=1, want_greedy=True)
    o = sr.step_objective(logits.double().numpy(), OBJ_IL, targets.numpy(), OBJ_TL, paths=paths.cpu().numpy(),
                          greedy_frames=greedy.cpu().numpy(), lam=1.0, entropy_weight=0.1, kl_weight=0.1, ref_log_probs=ref.double().numpy())
    lerr, gerr = abs(float(loss) - o.loss) / abs(o.loss), rel_err(z.grad.cpu(), o.grad)
    print(f"[step objective] V=300 K=1 with tails: loss rel err {lerr:.2e}, d(logits) rel err {gerr:.2e}")
    assert lerr <= 1e-5 and gerr <= 1e-5 and R_s.shape == (OBJ["B"],) and R_b.shape == (OBJ["B"],)


# ---- shards ----
def test_shards_reproduce_the_whole_batch():
    kw = dict(lam=1.0, seed=9, offset=2, num_samples=4, baseline="leave_one_out", per_step=True, step_objectives=True)
    r = shards_vs_whole(kw, lattice_case(150, 4, 29, 12, 77))
    assert r.R_s.shape == (4, 4) and float(r.grad.abs().max()) > 0 and bool(torch.isfinite(r.loss))


# ---- one trainer step ----
def test_trainer_step_per_step_vs_oracle(ops, monkeypatch):
    """One f32 eval-mode step with four samples, leave one out, per-step rewards and the entropy bonus against the torch-CPU model in
    fp64 on the same weights, the oracle taking the device's paths: loss within 1e-5, every parameter gradient within 1e-4."""
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    batch, lens, tlens = step_batch(4, seed=51)
    _, pr, m = oracle_model(80, 29, 52)
    recorded = []
    real = ops.frame_sample_multi

    def recording(*a, **k):
        out = real(*a, **k)
        recorded.append(out[1])
        return out
    monkeypatch.setattr(ops, "frame_sample_multi", recording)
    tr = PolicyGradientTrainer(m, lam=1.0, seed=3, precision="f32", reward_mode="per_step", step_objectives=True, num_samples=4,
                               reward_baseline="leave_one_out", entropy_weight=0.1)
    loss = tr.compute_gradients(*(t.to(DEV) for t in batch))
    torch.cuda.synchronize()
    ops.lstm_assert_no_timeouts()
    assert len(recorded) == 1
    paths = recorded[0][:, :, :4].cpu().numpy()
    r = oracle_step(pr, batch, lens, tlens, num_samples=4, baseline="leave_one_out", entropy_weight=0.1, paths=paths)
    logits64, il, tg, tl = r.args
    o = sr.step_objective(logits64, il, tg, tl, paths=paths, baseline="leave_one_out", lam=1.0, entropy_weight=0.1)
    np.testing.assert_allclose(tr.last_sample_rewards.cpu().numpy(), r.oracle.R, rtol=1e-6)
    lerr = abs(float(loss) - o.loss) / abs(o.loss)
    errs = param_errs(m, r.backprop(o.grad))
    worst = max(errs, key=errs.get)
    print(f"[step trainer] loss rel err {lerr:.2e}; worst parameter gradient {worst} {errs[worst]:.2e}")
    assert lerr <= 1e-5, (float(loss), o.loss)
    assert errs[worst] <= 1e-4, (worst, errs[worst])
    # the utterance-level objective on the same paths is another number: the step did use the per-frame coefficients
    assert abs(r.oracle.loss - o.loss) > 1e-4 * abs(o.loss)


# ---- the driver ----
def test_train_driver_per_step(tmp_path):
    from policy_gradient_asr_amd.model import train
    corpus, out, ds = tiny_corpus(tmp_path)
    kw = dict(train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=0, reward_mode="per_step", step_objectives=True, num_samples=2)
    losses, _ = train(str(corpus), str(out), 1, 16, 0, **kw)
    assert len(losses) == 1 and np.isfinite(losses[0])
    st = torch.load(os.path.join(str(out), "checkpoint_last.pth"), map_location="cpu")
    assert st["step_objectives"] is True and st["reward_mode"] == "per_step" and st["num_samples"] == 2 and st["epoch"] == 1
    losses, _ = train(str(corpus), str(out), 2, 16, 0, **kw)
    assert len(losses) == 2 and np.isfinite(losses[1])
    assert torch.load(os.path.join(str(out), "checkpoint_last.pth"), map_location="cpu")["epoch"] == 2
    with pytest.raises(ValueError, match="one sampled path"):
        train(str(corpus), str(tmp_path / "other"), 1, 16, 0, **{**kw, "step_objectives": None})
