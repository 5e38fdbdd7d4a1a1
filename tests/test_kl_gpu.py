"""The KL penalty towards a frozen reference policy (kl_weight) on the MI355X, against the fp64 statement in tests/kl_ref.py: the KL
kernel, the KL term of the three gradient passes on its own, beside the entropy term and beside CTC + REINFORCE, a reference equal to
the policy, the null KL pointers, and the trainer -- a full step against the fp64 oracle model with a second oracle model as the
reference, weight 0 as the default step, the frozen reference, shards, accumulation, a ragged batch, the direction the term moves the
policy in and the train driver's two-stage recipe."""
import functools

import numpy as np
import pytest
import torch

import kl_ref
from oracle import ctc_ref, decode_ref, model_ref, pg_ref
from pg_harness import (ACC_F, ACC_V, DEV, _batch, _rows, _slices, _trainer, fused_grad_ref, lattice_case, oracle_model, oracle_step,
                        param_errs, rel_err, sampled_case, step_batch, tiny_corpus)

pytestmark = pytest.mark.gpu

# idle lanes; the multi-sample tests' shape; all 64 lanes with T*B = 165 rows, no multiple of the four waves of a gradient
# workgroup; the single-symbol alphabet (KL = 0 exactly)
SHAPES = [(7, 3, 5), (160, 6, 29), (33, 5, 64), (5, 2, 1)]
IN_LEN = {3: [7, 0, 4], 6: [160, 0, 123, 1, 160, 77], 5: [33, 0, 17, 32, 33], 2: [5, 0]}        # ragged, 0 and T included
ENTRIES = ["single", "single_per_frame", "multi", "seq"]
TOL = 1e-5          # the bound of test_entropy_gpu and test_multi_path_ctc_grad_vs_fp64 for the same kernels


def _policy_case(T, B, V, K=2):
    """fp32 log-probs with the awkward rows -- two -inf entries in row (1, 0), row (2, 2) exactly one-hot on the blank (ln p = 0
    there, -inf elsewhere) -- and everything the gradient entries want beside them.  The -inf symbols occur in no target and no
    sampled path, and utterance 2 has an empty target and all-blank paths: the CTC and REINFORCE parts of those rows stay finite."""
    g = torch.Generator().manual_seed(100 * T + V)
    z = torch.randn(T, B, V, generator=g, dtype=torch.float64) * 2
    if V >= 5:
        z[1, 0, V - 2:] = -float("inf")
    lp = torch.log_softmax(z, dim=2)
    if V >= 5:
        lp[2, 2, :] = -float("inf")
        lp[2, 2, 0] = 0.0
    lp = lp.float()
    hi = max(V - 2, 2)
    targets = torch.randint(1, hi, (B, 3), generator=g, dtype=torch.int32)
    tg_len = torch.tensor([3, 2, 0, 1, 3, 2][:B], dtype=torch.int32)
    paths = torch.randint(0, hi, (K, T, B), generator=g, dtype=torch.int32)
    if V == 1:
        targets.zero_(); tg_len.zero_(); paths.zero_()
    if B > 2:
        paths[:, :, 2] = 0
    in_len = torch.tensor(IN_LEN[B], dtype=torch.int32)
    c = dict(T=T, B=B, V=V, K=K, lp=lp.to(DEV), lg=lp.double().numpy(), in_len=in_len, il=in_len.to(DEV), targets=targets,
             tg=targets.to(DEV), tg_len=tg_len, tl=tg_len.to(DEV), paths=paths.to(DEV))
    c["ref"], c["rg"] = _reference(T, B, V)
    return c


def _reference(T, B, V):
    """The reference's fp32 log-probs on the device and the same numbers in fp64: log_softmax in fp64 of 2 * randn; for V >= 5 logit
    [3, 0, 1] is -inf, a zero reference probability under a live policy row (the floor)."""
    g = torch.Generator().manual_seed(7000 + 100 * T + V)
    z = torch.randn(T, B, V, generator=g, dtype=torch.float64) * 2
    if V >= 5:
        z[3, 0, 1] = -float("inf")
    lq = torch.log_softmax(z, dim=2).float()
    return lq.to(DEV), lq.double().numpy()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lattices(c):
    """The target lattice and, for the seq entry, the lattices of the paths' collapsed hypotheses (every one sequence-scored)."""
    from policy_gradient_asr_amd import hipops
    if "handle" not in c:
        _, c["handle"] = hipops.ctc_lattice(c["lp"], c["tg"], c["il"], c["tl"])
        if "tokens" not in c:
            c["tokens"], c["tok_len"] = hipops.ctc_collapse(c["paths"], c["il"])
        _, c["hyp_handle"] = hipops.ctc_hyp_lattice(c["lp"], c["tokens"], c["tok_len"], c["il"], c["T"])
    return c


def _grad(entry, c, utt_scale, coef, coef_tb, **terms):
    """One of the three gradient passes through its hipops wrapper: coef (K,B) -- the single-path pass takes sample 0 --, coef_tb
    (T,B) the per-frame form of the single-path pass; terms: ent_scale, ref_log_probs, kl_scale."""
    from policy_gradient_asr_amd import hipops
    _lattices(c)
    lp, il, tl, h = c["lp"], c["il"], c["tl"], c["handle"]
    if entry == "single":
        return hipops.ctc_grad_from_lattice(lp, il, tl, h, utt_scale=utt_scale, pg_coef=coef[0].contiguous(),
                                            pg_path=c["paths"][0].contiguous(), **terms)
    if entry == "single_per_frame":
        return hipops.ctc_grad_from_lattice(lp, il, tl, h, utt_scale=utt_scale, pg_coef=coef_tb, pg_path=c["paths"][0].contiguous(),
                                            **terms)
    if entry == "multi":
        return hipops.ctc_grad_from_lattice_multi(lp, il, tl, h, utt_scale, coef, c["paths"], **terms)
    return hipops.ctc_grad_from_lattices_seq(lp, il, tl, h, c["hyp_handle"], utt_scale, coef, c["paths"], c["tok_len"], **terms)


def _raw(entry, suffix, c, utt_scale, coef, coef_tb, pointers):
    """The ``_ent`` or ``_kl`` entry point itself; pointers: what it takes between the paths and grad_logits -- (ent_scale,) or
    (ent_scale, ref_log_probs, kl_scale), tensors or None."""
    from policy_gradient_asr_amd import _lib
    lib = _lib.load()
    _lattices(c)
    T, B, V, K = c["T"], c["B"], c["V"], c["K"]
    ws, Lmax, blank = c["handle"]
    grad = torch.empty_like(c["lp"])
    head = (c["lp"].data_ptr(), c["il"].data_ptr(), c["tl"].data_ptr(), T, B, V, Lmax, blank, utt_scale.data_ptr())
    mid = tuple(None if t is None else t.data_ptr() for t in pointers)
    tail = (grad.data_ptr(), ws.data_ptr(), ws.numel())
    st = torch.cuda.current_stream().cuda_stream
    p0 = c["paths"][0].contiguous()
    if entry == "single":
        c0 = coef[0].contiguous()
        rc = getattr(lib, "pgasr_ctc_grad_from_lattice" + suffix)(*head, c0.data_ptr(), p0.data_ptr(), 0, *mid, *tail, st)
    elif entry == "single_per_frame":
        rc = getattr(lib, "pgasr_ctc_grad_from_lattice" + suffix)(*head, coef_tb.data_ptr(), p0.data_ptr(), 1, *mid, *tail, st)
    elif entry == "multi":
        rc = getattr(lib, "pgasr_ctc_grad_from_lattice_multi" + suffix)(*head, K, coef.data_ptr(), c["paths"].data_ptr(), *mid, *tail, st)
    else:
        hws, _, Lh = c["hyp_handle"]
        rc = getattr(lib, "pgasr_ctc_grad_from_lattices_seq" + suffix)(*head, K, coef.data_ptr(), c["paths"].data_ptr(),
                                                                      c["tok_len"].data_ptr(), Lh, *mid, *tail, hws.data_ptr(),
                                                                      hws.numel(), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return grad


@pytest.mark.parametrize("T,B,V", SHAPES)
def test_frame_kl_vs_fp64(T, B, V):
    """kl_mean and kl_scale against fp64 on the device's own fp32 tensors (rel err < 1e-5), finite with a zero reference probability,
    exactly 0 for an empty utterance, for the single-symbol alphabet and for a reference equal to the policy, equal bits from two
    calls; metrics.frame_kl is the same kernel and weight 0 the monitoring call."""
    from policy_gradient_asr_amd import hipops, metrics
    c = _policy_case(T, B, V)
    gamma, inv_gb = 2.0, 1.0 / 8
    mean, scale = hipops.frame_kl(c["lp"], c["ref"], c["il"], gamma, inv_gb)
    mean2, scale2 = hipops.frame_kl(c["lp"], c["ref"], c["il"], gamma, inv_gb)
    il = c["in_len"].numpy()
    w_mean, w_scale = kl_ref.kl_stats(c["lg"], c["rg"], il, gamma, inv_gb)
    e_mean = rel_err(mean.cpu().numpy(), w_mean) if V > 1 else float(mean.abs().max())
    e_scale = rel_err(scale.cpu().numpy(), w_scale)
    rows = kl_ref.row_kl(c["lg"], c["rg"])[np.arange(T)[:, None] < il[None, :]]
    print(f"[frame kl] T={T} B={B} V={V}: kl_mean rel err {e_mean:.2e}, kl_scale rel err {e_scale:.2e}, per-frame KL "
          f"{rows.min():.3f} .. {rows.max():.3f} nats, mean {w_mean.max():.3f}")
    assert mean.shape == (B,) and scale.shape == (B,)
    assert e_mean < TOL and e_scale < TOL
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(scale).all())
    empty = c["in_len"] == 0
    assert bool(empty.any()) and bool((mean.cpu()[empty] == 0).all())
    if V == 1:
        assert bool((mean == 0).all())
    else:
        assert float(mean.max()) > 0.05
    same, _ = hipops.frame_kl(c["lp"], c["lp"], c["il"], gamma, inv_gb)
    assert bool((same == 0).all())                                              # q = p: exactly 0 everywhere
    assert torch.equal(_bits(mean), _bits(mean2)) and torch.equal(_bits(scale), _bits(scale2))
    assert torch.equal(_bits(metrics.frame_kl(c["lp"], c["ref"], c["il"])), _bits(mean))
    assert bool((hipops.frame_kl(c["lp"], c["ref"], c["il"])[1] == 0).all())    # weight 0: the monitoring call


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("T,B,V", SHAPES)
def test_kl_only_gradient_vs_fp64(T, B, V, entry):
    """utt_scale = 0, pg_coef = 0 and no ent_scale leave the KL term alone: kl_scale_b p (ln p - lnq - KL) to rel err < 1e-5, finite
    everywhere (the floored reference symbol included), rows beyond T_b exactly 0, every row summing to <= 1e-5 of its largest entry,
    the one-hot policy row and the -inf policy entries exactly 0."""
    c = _policy_case(T, B, V)
    g = torch.Generator().manual_seed(B)
    kl_scale = torch.rand(B, generator=g) + 0.5
    zeros = lambda *s: torch.zeros(*s, device=DEV)
    grad = _grad(entry, c, zeros(B), zeros(c["K"], B), zeros(T, B), ref_log_probs=c["ref"], kl_scale=kl_scale.to(DEV)).cpu().numpy()
    il = c["in_len"].numpy()
    want = kl_ref.kl_grad(c["lg"], c["rg"], il, kl_scale.double().numpy())
    err = rel_err(grad, want) if V > 1 else float(np.abs(grad).max())
    rows = np.abs(grad.astype(np.float64).sum(axis=2))
    tops = np.abs(grad).max(axis=2)
    live = tops > 0
    print(f"[kl grad] {entry} T={T} B={B} V={V}: rel err {err:.2e}, worst row sum / row max "
          f"{(rows[live] / tops[live]).max() if live.any() else 0.0:.2e}")
    assert np.isfinite(grad).all()
    assert err < TOL
    beyond = np.arange(T)[:, None] >= il[None, :]
    assert beyond.any() and (grad[beyond] == 0).all()
    assert (rows <= 1e-5 * tops).all()
    if V >= 5:
        assert (grad[2, 2] == 0).all()                    # the one-hot policy row: 1 * (KL - KL)
        assert (grad[1, 0, V - 2:] == 0).all() and np.abs(grad[1, 0]).max() > 0
        assert np.abs(grad[3, 0]).max() > 0               # the row with the zero reference probability: finite, not zero
    if V == 1:
        assert (grad == 0).all()


def _full_case(seed):
    T, B, V, K = 160, 6, 29, 4
    c = sampled_case(T, B, V, K)                  # lattice_case's logits and targets (L = 14), sampled paths, their hypotheses
    c.update(il=c["in_len"].to(DEV), tl=c["tg_len"].to(DEV), tg=c["targets"].to(DEV))
    c["ref"], c["rg"] = _reference(T, B, V)
    g = torch.Generator().manual_seed(seed)
    coef = torch.randn(K, B, generator=g) * 0.1
    coef_tb = torch.randn(T, B, generator=g) * 0.1
    scale = torch.rand(B, generator=g) + 0.5
    return c, coef, coef_tb, scale


@pytest.mark.parametrize("with_entropy", [False, True], ids=["kl", "entropy+kl"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_reference_equal_to_the_policy_adds_nothing(entry, with_entropy):
    """ref_log_probs = log_probs: every lane's p (ln p - lnq) is exactly 0, and the _kl form gives the bits of the same call without
    the KL arguments."""
    from policy_gradient_asr_amd import hipops
    c, coef, coef_tb, scale = _full_case(3)
    ent = {"ent_scale": hipops.frame_entropy(c["lp"], c["il"], 2.0, 1.0 / 6)[1]} if with_entropy else {}
    _, kl_scale = hipops.frame_kl(c["lp"], c["lp"], c["il"], 2.0, 1.0 / 6)
    assert float(kl_scale.min()) > 0
    plain = _grad(entry, c, scale.to(DEV), coef.to(DEV), coef_tb.to(DEV), **ent)
    kl = _grad(entry, c, scale.to(DEV), coef.to(DEV), coef_tb.to(DEV), ref_log_probs=c["lp"], kl_scale=kl_scale, **ent)
    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) > 0
    assert torch.equal(_bits(plain), _bits(kl))


@pytest.mark.parametrize("with_entropy", [False, True], ids=["null", "ent_scale"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_null_kl_pointers_are_the_ent_entry(entry, with_entropy):
    """The _kl entry point with ref_log_probs = kl_scale = NULL against the _ent entry on the same inputs: equal bits."""
    from policy_gradient_asr_amd import hipops
    c, coef, coef_tb, scale = _full_case(3)
    es = hipops.frame_entropy(c["lp"], c["il"], 2.0, 1.0 / 6)[1] if with_entropy else None
    args = (c, scale.to(DEV), coef.to(DEV), coef_tb.to(DEV))
    old = _raw(entry, "_ent", *args, (es,))
    new = _raw(entry, "_kl", *args, (es, None, None))
    assert bool(torch.isfinite(old).all()) and float(old.abs().max()) > 0
    assert torch.equal(_bits(old), _bits(new))


@pytest.mark.parametrize("entry", ENTRIES)
def test_full_gradient_with_entropy_and_kl_vs_fp64(entry):
    """CTC + K REINFORCE terms + entropy (beta = 2) + KL (gamma = 2), both scales from their kernels, at T,B,V,L,K = 160,6,29,14,4
    against ctc_ref + decode_ref.reinforce_grad / fused_grad_ref + pg_ref.entropy_grad + kl_ref.kl_grad: rel err < 1e-5."""
    from policy_gradient_asr_amd import hipops
    c, coef, coef_tb, scale = _full_case(7)
    T, B, K = c["T"], c["B"], c["K"]
    beta, gamma, inv_gb = 2.0, 2.0, 1.0 / B
    _, ent_scale = hipops.frame_entropy(c["lp"], c["il"], beta, inv_gb)
    _, kl_scale = hipops.frame_kl(c["lp"], c["ref"], c["il"], gamma, inv_gb)
    grad = _grad(entry, c, scale.to(DEV), coef.to(DEV), coef_tb.to(DEV), ent_scale=ent_scale, ref_log_probs=c["ref"], kl_scale=kl_scale)
    lg, il = c["lg"], c["in_len"].numpy()
    pn = c["paths"].cpu().numpy()
    _, g_ctc = ctc_ref.ctc_loss_and_grad(lg, c["targets"].numpy(), il, c["tg_len"].numpy())
    base = g_ctc * scale.double().numpy()[None, :, None]
    if entry == "single":
        want = base + decode_ref.reinforce_grad(lg, pn[0], coef[0].double().numpy(), il)
    elif entry == "single_per_frame":
        want = base + decode_ref.reinforce_grad(lg, pn[0], coef_tb.double().numpy(), il)
    elif entry == "multi":
        want = base
        for k in range(K):
            want = want + decode_ref.reinforce_grad(lg, pn[k], coef[k].double().numpy(), il)
    else:
        want = fused_grad_ref(c, coef, scale, T)
    want = want + pg_ref.entropy_grad(lg, il, pg_ref.entropy_stats(lg, il, beta, inv_gb)[1])
    kl = kl_ref.kl_grad(lg, c["rg"], il, kl_ref.kl_stats(lg, c["rg"], il, gamma, inv_gb)[1])
    err = rel_err(grad.cpu().numpy(), want + kl)
    print(f"[full grad + entropy + kl] {entry}: rel err {err:.2e}; without the KL term the reference differs by "
          f"{rel_err(want, want + kl):.2e}")
    assert rel_err(want, want + kl) > 10 * TOL        # the term is visible at this bound
    assert err < TOL


# ---- the trainer ----
# init_params starts from a policy within 1e-3 nats of uniform, where p (ln p - ln q - KL) vanishes for two such policies; with the
# head's weight and bias times 80 (the entropy tests' gain) policy and reference are about 3.7 .. 4.4 nats apart per frame, and with
# gamma = 2 the term is 1.9e-2 .. 3.7e-2 of the oracle's loss and moves every parameter gradient by 9e-2 .. 6e-1 (fp64, on the CPU).
HEAD_GAIN = 80.0
GAMMA = 2.0


@functools.lru_cache(maxsize=None)
def _oracle_reference(B, seed):
    """(the reference Seq2Seq on the device, its fp64 logits on step_batch(B) from model_ref): oracle_model's seed + 2."""
    batch, _, _ = step_batch(B, False, seed)
    _, prq, mq = oracle_model(80, 29, seed + 2, HEAD_GAIN)
    x, _, fmask, _ = batch
    with torch.no_grad():
        zq = model_ref.head_logits_torch(prq, model_ref.encoder_forward_torch(prq, x.double(), fmask, packed=True)).numpy()
    return mq, zq


def _kl_step_vs_oracle(mode, B=4, K=4, gamma=GAMMA, beta=0.0, seed=51):
    """One lambda = 1 trainer step (f32 mode, greedy hypothesis, eval-mode dropout) with kl_weight = gamma against the torch-CPU model
    in FP64 on the same weights: pg_harness.oracle_step's objective plus kl_ref's value and logits-gradient, back-propagated --
    rewards exact, loss within 1e-5, every parameter gradient within 1e-4 (max norm), last_kl within 1e-5 of the oracle's."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    K = 1 if mode == "per_step" else K
    tkw, okw = {"multi": ({}, {}), "sequence": (dict(score_function="sequence"),) * 2,
                "per_step": (dict(reward_mode="per_step"), dict(per_step=True))}[mode]
    ent = {"entropy_weight": beta} if beta else {}
    batch, lens, tlens = step_batch(B, False, seed)
    _, pr, m = oracle_model(80, 29, seed + 1, HEAD_GAIN)
    mq, zq = _oracle_reference(B, seed)
    before = [p.detach().clone() for p in mq.parameters()]
    tr = PolicyGradientTrainer(m, lam=1.0, seed=3, precision="f32", reward_decoder="greedy", num_samples=K, kl_weight=gamma,
                               kl_reference=mq, **ent, **tkw)
    loss = tr.compute_gradients(*(t.to(DEV) for t in batch))
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    r = oracle_step(pr, batch, lens, tlens, num_samples=K, **ent, **okw)
    o = r.oracle
    il = np.array(lens)
    lp, lq = ctc_ref.log_softmax(r.args[0], axis=2), ctc_ref.log_softmax(zq, axis=2)
    kl_mean, kl_scale = kl_ref.kl_stats(lp, lq, il, gamma, 1.0 / B)
    kl_loss = kl_ref.kl_loss(lp, lq, il, gamma, 1.0 / B)
    want_loss = o.loss + kl_loss
    want = r.backprop(o.grad + kl_ref.kl_grad(lp, lq, il, kl_scale))
    # sensitivity, on the oracle alone: without the term every parameter gradient is more than 100 bounds away and so is the loss
    moved = {k: rel_err(r.grads[k], want[k]) for k in want}
    least = min(moved, key=moved.get)
    label = f"[kl step] {mode} B={B} K={K} gamma={gamma} beta={beta}"
    print(f"{label}: the term is {abs(kl_loss) / abs(want_loss):.2e} of the loss and moves the oracle's gradients by "
          f"{moved[least]:.2e} ({least}) .. {max(moved.values()):.2e}; oracle kl_mean {kl_mean}")
    assert moved[least] > 100 * 1e-4, (least, moved[least])
    assert abs(kl_loss) / abs(want_loss) > 100 * 1e-5
    nll, R_s, R_b = tr.last_stats
    np.testing.assert_allclose(tr.last_sample_rewards.cpu().numpy(), o.R, rtol=1e-6)
    np.testing.assert_allclose(R_s.cpu().numpy(), o.R.mean(axis=0), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(R_b.cpu().numpy(), o.baselines.mean(axis=0), rtol=1e-6, atol=1e-7)
    lerr = abs(float(loss) - want_loss) / abs(want_loss)
    errs = param_errs(m, want)
    worst = max(errs, key=errs.get)
    kerr = float(np.abs(tr.last_kl.cpu().numpy() / kl_mean - 1).max())
    print(f"{label}: loss rel err {lerr:.2e}; worst parameter gradient {worst} {errs[worst]:.2e}; last_kl rel err {kerr:.2e}")
    assert lerr < 1e-5, (float(loss), want_loss)
    assert errs[worst] < 1e-4, (worst, errs[worst])
    assert tr.last_kl.shape == (B,) and not tr.last_kl.requires_grad
    np.testing.assert_allclose(tr.last_kl.cpu().numpy(), kl_mean, rtol=1e-5)
    if beta:
        np.testing.assert_allclose(tr.last_entropy.cpu().numpy(), o.ent_mean, rtol=1e-5)
    # the reference took no step and no gradient
    assert all(torch.equal(_bits(a), _bits(b)) and b.grad is None for a, b in zip(before, mq.parameters())) and not mq.training
    return tr


@pytest.mark.parametrize("mode", ["multi", "sequence", "per_step"])
def test_kl_step_vs_oracle(mode):
    _kl_step_vs_oracle(mode)


def test_kl_step_with_entropy_vs_oracle():
    _kl_step_vs_oracle("multi", beta=2.0)


def test_ragged_batch_with_kl_vs_oracle():
    """B = 3 is padded to 16 with empty utterances: the reference runs on the padded batch, the empty rows add no KL, last_kl covers
    the three real rows, and loss and gradients are the oracle's over the three real utterances."""
    tr = _kl_step_vs_oracle("multi", B=3)
    assert tr.last_kl.shape == (3,) and bool((tr.last_kl > 0).all())
    from policy_gradient_asr_amd.loss import PGCTCLossFn
    assert PGCTCLossFn.last_kl.shape == (16,) and bool((PGCTCLossFn.last_kl[3:] == 0).all())


def _other_model(seed=1, train=False, head_gain=1.0):
    """A Seq2Seq of the accumulation tests' shape with other weights than _trainer's model (seed 0): a reference that is not the policy.
    head_gain multiplies the head's weight and bias (``weights`` starts both models near the uniform policy, a fraction of a nat apart)."""
    from policy_gradient_asr_amd.model import Seq2Seq, weights
    torch.manual_seed(seed)
    m = Seq2Seq(ACC_V, n_feats=ACC_F); m.apply(weights)
    with torch.no_grad():
        m.head.weight.mul_(head_gain); m.head.bias.mul_(head_gain)
    m = m.to(DEV)
    return m.train() if train else m.eval()


def _count_logits(module, calls):
    real = module.logits
    module.logits = lambda *a, **k: (calls.append(1), real(*a, **k))[1]


@pytest.mark.parametrize("kw", [{}, {"num_samples": 4}, {"score_function": "sequence"}, {"reward_mode": "per_step"}],
                         ids=["single", "multi", "sequence", "per_step"])
def test_weight_zero_is_the_default_step(kw, monkeypatch):
    """kl_weight = 0.0, with and without a reference: the same bits in loss and every gradient as a trainer built without the
    arguments, no KL launch and no forward of the reference."""
    from policy_gradient_asr_amd import hipops
    kl_calls, ref_calls = [], []
    real = hipops.frame_kl
    monkeypatch.setattr(hipops, "frame_kl", lambda *a, **k: (kl_calls.append(1), real(*a, **k))[1])
    ref = _other_model()
    _count_logits(ref, ref_calls)
    batch, _ = _batch(16)
    res = []
    for extra in ({}, {"kl_weight": 0.0}, {"kl_weight": 0.0, "kl_reference": ref}, {"kl_reference": "initial"}):
        tr = _trainer(**kw, **extra)
        loss = tr.compute_gradients(*batch)
        torch.cuda.synchronize()
        hipops.lstm_assert_no_timeouts()
        assert tr.last_kl is None
        res.append((loss.clone(), tr.gflat.clone()))
    assert not kl_calls and not ref_calls
    for loss, gflat in res[1:]:
        assert torch.equal(_bits(res[0][0]), _bits(loss)) and torch.equal(_bits(res[0][1]), _bits(gflat))
    assert float(res[0][1].abs().max()) > 0
    tr = _trainer(**kw, kl_weight=0.5, kl_reference=ref)            # .. and the counters do count
    tr.compute_gradients(*batch)
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    assert len(kl_calls) == 1 and len(ref_calls) == 1 and tr.last_kl.shape == (16,)
    assert not torch.equal(tr.gflat, res[0][1])


def test_reference_is_frozen_and_the_policy_state_untouched():
    """One step() in train mode with lr > 0: every reference parameter keeps its bits and has no .grad, the reference stays in eval
    mode (its forward draws no dropout mask), and the policy encoder's dropout counter reads what the same step without KL leaves."""
    from policy_gradient_asr_amd import hipops
    batch, _ = _batch(16)
    ref = _other_model(train=True)                      # the trainer puts it in eval mode
    before = [p.detach().clone() for p in ref.parameters()]
    ref_drop = ref.encoder._drop_calls
    plain = _trainer(train=True, lr=1e-3)
    plain.step(*batch)
    tr = _trainer(train=True, lr=1e-3, kl_weight=0.5, kl_reference=ref)
    start = tr.flat.clone()
    loss = tr.step(*batch)
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    assert np.isfinite(float(loss)) and tr.applied_steps() == 1 and not torch.equal(tr.flat, start)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(before, ref.parameters()))
    assert all(p.grad is None and not p.requires_grad for p in ref.parameters())
    assert not ref.training and tr.model.training
    assert ref.encoder._drop_calls == ref_drop
    assert tr.model.encoder._drop_calls == plain.model.encoder._drop_calls > 0
    assert tr.model.encoder.dropout_seed == plain.model.encoder.dropout_seed
    assert tr.flat.numel() == plain.flat.numel()        # the reference's parameters are in no flat buffer


def test_kl_shards_sum_to_the_whole_batch():
    """pg_harness.shards_vs_whole written out for a per-shard tensor (it hands every call the same keywords): two pg_ctc_loss calls on
    the halves, ref_log_probs sliced like the logits and global_batch set, against one call on the whole batch at
    T,B,V,L,K = 150,8,29,12,4 with kl_weight = 2 -- the same rewards bit for bit, logits gradient and loss within 1e-6, and the
    halves' last_kl, concatenated, the whole's bits."""
    from policy_gradient_asr_amd.loss import PGCTCLossFn, pg_ctc_loss
    T, B, V, L, K = 150, 8, 29, 12, 4
    kw = dict(lam=1.0, seed=11, offset=4, num_samples=K, baseline="leave_one_out", kl_weight=2.0)
    logits, targets, in_len, tg_len = lattice_case(T, B, V, L, 77)
    ref, _ = _reference(T, B, V)
    half = B // 2
    lg = logits.float().to(DEV)
    tg, il, tl = targets.to(DEV), in_len.to(DEV), tg_len.to(DEV)
    whole = lg.clone().requires_grad_(True)
    loss, nll, R_s, R_b = pg_ctc_loss(whole, il, tg, tl, ref_log_probs=ref, **kw)
    kl_whole = PGCTCLossFn.last_kl
    loss.backward()
    grads, total, kl_parts = [], 0.0, []
    for h in range(2):
        sl = slice(half * h, half * h + half)
        part = lg[:, sl].contiguous().requires_grad_(True)
        l_h, _, Rs_h, Rb_h = pg_ctc_loss(part, il[sl].contiguous(), tg[sl].contiguous(), tl[sl].contiguous(), global_batch=B,
                                         sample_base=half * h, ref_log_probs=ref[:, sl].contiguous(), **kw)
        kl_parts.append(PGCTCLossFn.last_kl)
        l_h.backward()
        grads.append(part.grad)
        total += float(l_h.detach())
        assert torch.equal(Rs_h, R_s[..., sl]) and torch.equal(Rb_h, R_b[sl])
    diff = (torch.cat(grads, dim=1) - whole.grad).abs().max()
    assert float(diff) <= 1e-6 * float(whole.grad.abs().max()), float(diff)
    assert abs(total - float(loss.detach())) <= 1e-6 * abs(float(loss.detach()))
    plain = lg.clone().requires_grad_(True)
    pg_ctc_loss(plain, il, tg, tl, **dict(kw, kl_weight=0.0))[0].backward()
    assert float((plain.grad - whole.grad).abs().max()) > 1e-3 * float(whole.grad.abs().max())       # the term is in there
    assert kl_whole.shape == (B,) and torch.equal(_bits(torch.cat(kl_parts)), _bits(kl_whole))


def test_kl_accumulated_step_is_the_whole_batch():
    """step_accumulated over two micro-batches of 16 (padded to one T) against one step on their concatenation, kl_weight = 2, K = 4:
    test_accumulated_step_is_the_whole_batch's f32 bounds (loss 1e-6, gflat 1e-5); last_kl holds all 32 real rows in call order.
    last_kl is held to 1e-5 (max norm), the bound of gflat: it is a function of the two models' log-probs alone, which the batch
    shapes 16 and 32 compute in different summation orders, and with log-prob errors of e it moves by at most e (2 + max |ln p - ln q|)
    -- a few fp32 ulps of ln q against a KL of order one nat.  (The reference's head is scaled so that the KL IS of that order: two
    ``weights``-initialised models are so close that their KL is the rounding of its own terms.)"""
    from policy_gradient_asr_amd import hipops
    batch, _ = _batch(32)
    parts = _slices((16, 16))
    ref = _other_model(head_gain=30.0)
    kw = dict(num_samples=4, kl_weight=2.0, kl_reference=ref, lr=1e-3)
    whole = _trainer(**kw)
    loss_w = float(whole.step(*batch))
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    acc = _trainer(**kw)
    loss_a = float(acc.step_accumulated([_rows(batch, p) for p in parts]))
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    gerr = rel_err(acc.gflat.cpu(), whole.gflat.cpu())
    lerr = abs(loss_a - loss_w) / abs(loss_w)
    kerr = rel_err(acc.last_kl.cpu(), whole.last_kl.cpu())
    print(f"[kl accum] gflat {gerr:.2e} loss {lerr:.2e} last_kl {kerr:.2e} (last_kl {float(whole.last_kl.min()):.4f} .. "
          f"{float(whole.last_kl.max()):.4f} nats)")
    assert acc.last_kl.shape == (32,) and whole.last_kl.shape == (32,)
    assert torch.equal(acc.last_sample_rewards, whole.last_sample_rewards)
    # the order is checked: the two micro-batches the other way round would miss the bound below
    assert rel_err(whole.last_kl.cpu().roll(16), whole.last_kl.cpu()) > 100 * 1e-5
    assert kerr < 1e-5
    assert lerr <= 1e-6
    assert gerr < 1e-5
    assert acc.nstep == 1 and acc.applied_steps() == 1


def test_kl_penalty_pulls_the_policy_towards_the_reference():
    """Ten plain gradient steps on a free logits tensor through pg_ctc_loss at T,B,V = 40,4,29, the same seed with gamma = 5 and with
    gamma = 0: with the penalty the batch-mean frame KL from the reference falls and ends below the run without it.  Only the
    direction is asserted -- it follows from the sign of the term.  lam = 0, as in test_entropy_bonus_keeps_the_policy_wider: ten
    steps of this size with lam = 1 are dominated by the sampled REINFORCE term's noise (measured once: 3.02 -> 3.14 nats with the
    penalty against 4.31 without), which says nothing about the term under test; CTC + KL alone in torch fp64 on the CPU give
    3.02 -> 2.20 against 4.30."""
    from policy_gradient_asr_amd import metrics
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    T, B, V, L, lr = 40, 4, 29, 5, 20.0
    logits, targets, _, _ = lattice_case(T, B, V, L, 5)
    il = torch.tensor([40, 33, 40, 21], dtype=torch.int32, device=DEV)
    tl = torch.tensor([5, 4, 3, 5], dtype=torch.int32, device=DEV)
    tg = targets.to(DEV)
    ref, _ = _reference(T, B, V)
    seen = {}
    for gamma in (5.0, 0.0):
        z = logits.float().to(DEV).requires_grad_(True)
        trace = []
        for i in range(10):
            trace.append(float(metrics.frame_kl(torch.log_softmax(z.detach(), dim=2).contiguous(), ref, il).mean()))
            loss, _, _, _ = pg_ctc_loss(z, il, tg, tl, lam=0.0, seed=9, offset=i + 1, kl_weight=gamma, ref_log_probs=ref)
            z.grad = None
            loss.backward()
            with torch.no_grad():
                z -= lr * z.grad
        trace.append(float(metrics.frame_kl(torch.log_softmax(z.detach(), dim=2).contiguous(), ref, il).mean()))
        seen[gamma] = trace
    print(f"[kl behaviour] batch-mean frame KL over ten steps: gamma 5 {seen[5.0][0]:.4f} -> {seen[5.0][-1]:.4f}, "
          f"gamma 0 {seen[0.0][0]:.4f} -> {seen[0.0][-1]:.4f}")
    assert all(np.isfinite(v) for t_ in seen.values() for v in t_)
    assert seen[5.0][0] == seen[0.0][0] > 0
    assert seen[5.0][-1] < seen[5.0][0]
    assert seen[5.0][-1] < seen[0.0][-1]


def test_train_driver_two_stage_recipe(tmp_path, capsys, monkeypatch):
    """model.train: two epochs at lam = 0, then a run that starts from its model_best.pth (init_from) anchored to it by kl_weight = 0.5
    with num_samples = 2 -- the start weights are the file's, the log lines carry the batch-mean KL, the checkpoint records the
    weight and the reference's path, a resume with another weight warns, and a weight without a path raises."""
    from policy_gradient_asr_amd.model import train
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    corpus, out, ds = tiny_corpus(tmp_path)
    l0, _ = train(str(corpus), str(out), 2, 16, 0, train_dataset=ds, n_feats=20, lam=0.0, lr=3e-3, log_every=0)
    best = out / "model_best.pth"
    assert len(l0) == 2 and best.exists()
    capsys.readouterr()
    seen = {}
    real_step = PolicyGradientTrainer.step

    def step(self, *a, **k):
        if "start" not in seen:
            seen["start"] = {n: v.detach().clone() for n, v in self.model.state_dict().items()}
        seen["trainer"] = self
        return real_step(self, *a, **k)

    monkeypatch.setattr(PolicyGradientTrainer, "step", step)
    out2 = tmp_path / "run2"
    l1, _ = train(str(corpus), str(out2), 2, 16, 0, train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=1, num_samples=2,
                  init_from=str(best), kl_weight=0.5)
    assert len(l1) == 2 and all(np.isfinite(l1))
    want = torch.load(best, map_location=DEV)
    assert set(want) == set(seen["start"]) and all(torch.equal(want[n], seen["start"][n]) for n in want)
    tr = seen["trainer"]
    assert tr.kl_weight == 0.5 and tr.kl_reference is not tr.model and not tr.kl_reference.training
    assert all(torch.equal(want[n], v) for n, v in tr.kl_reference.state_dict().items())       # the reference is still the file
    assert tr.last_kl.shape == (16,) and bool(torch.isfinite(tr.last_kl).all()) and float(tr.last_kl.min()) >= -1e-6
    printed = capsys.readouterr().out
    shown = [float(line.split("KL:")[1]) for line in printed.splitlines() if "KL:" in line]
    assert len(shown) == 4 and all(np.isfinite(v) and v >= -1e-6 for v in shown)
    assert "Initialised from" in printed
    st = torch.load(out2 / "checkpoint_last.pth", map_location="cpu")
    assert st["kl_weight"] == 0.5 and st["kl_reference_path"] == str(best)
    train(str(corpus), str(out2), 3, 16, 0, train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=0, num_samples=2,
          init_from=str(best), kl_weight=0.25)
    printed = capsys.readouterr().out
    assert "kl_weight=0.25" in printed and "Resumed from epoch 2" in printed and "Initialised from" not in printed
    with pytest.raises(ValueError, match="kl_reference_path or init_from"):
        train(str(corpus), str(tmp_path / "run3"), 1, 16, 0, train_dataset=ds, n_feats=20, kl_weight=0.5)
