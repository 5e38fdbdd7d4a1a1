"""Entropy regularisation of the frame policy (entropy_weight) on the MI355X, against the fp64 statement in oracle/pg_ref.py:
the entropy kernel, the entropy term of the three gradient passes on its own and beside CTC + REINFORCE, the null ent_scale, and the
trainer -- a full step against the fp64 oracle model, weight 0 as the default path, shards, accumulation, a ragged batch, the train
driver and the direction the term moves the policy in."""
import numpy as np
import pytest
import torch

from oracle import ctc_ref, decode_ref, pg_ref
from pg_harness import (DEV, _batch, _rows, _slices, _trainer, fused_grad_ref, lattice_case, rel_err, sampled_case,
                        shards_vs_whole, tiny_corpus, trainer_step_vs_oracle)

pytestmark = pytest.mark.gpu

# idle lanes; the multi-sample tests' shape; all 64 lanes with T*B = 165 rows, no multiple of the four waves of a gradient
# workgroup; the single-symbol alphabet (H = 0 exactly)
SHAPES = [(7, 3, 5), (160, 6, 29), (33, 5, 64), (5, 2, 1)]
IN_LEN = {3: [7, 0, 4], 6: [160, 0, 123, 1, 160, 77], 5: [33, 0, 17, 32, 33], 2: [5, 0]}        # ragged, 0 and T included
ENTRIES = ["single", "single_per_frame", "multi", "seq"]


def _policy_case(T, B, V, K=2):
    """fp32 log-probs with the awkward rows -- two -inf entries in row (1, 0), row (2, 2) exactly one-hot on the blank (ln p = 0
    there, -inf elsewhere) -- and everything the gradient entries want beside them.  The -inf symbols occur in no target and no
    sampled path, and utterance 2 has an empty target and all-blank paths: the CTC and REINFORCE parts of those rows stay finite, so
    what the tests see there is the entropy term."""
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
    return dict(T=T, B=B, V=V, K=K, lp=lp.to(DEV), lg=lp.double().numpy(), in_len=in_len, il=in_len.to(DEV), targets=targets,
                tg=targets.to(DEV), tg_len=tg_len, tl=tg_len.to(DEV), paths=paths.to(DEV))


def _lattices(c):
    """The target lattice and, for the seq entry, the lattices of the paths' collapsed hypotheses (every one sequence-scored)."""
    from policy_gradient_asr_amd import hipops
    if "handle" not in c:
        _, c["handle"] = hipops.ctc_lattice(c["lp"], c["tg"], c["il"], c["tl"])
        if "tokens" not in c:
            c["tokens"], c["tok_len"] = hipops.ctc_collapse(c["paths"], c["il"])
        _, c["hyp_handle"] = hipops.ctc_hyp_lattice(c["lp"], c["tokens"], c["tok_len"], c["il"], c["T"])
    return c


def _grad(entry, c, utt_scale, coef, coef_tb, ent_scale):
    """One of the three gradient passes through its hipops wrapper: coef (K,B) -- the single-path pass takes sample 0 --, coef_tb
    (T,B) the per-frame form of the single-path pass."""
    from policy_gradient_asr_amd import hipops
    _lattices(c)
    lp, il, tl, h = c["lp"], c["il"], c["tl"], c["handle"]
    if entry == "single":
        return hipops.ctc_grad_from_lattice(lp, il, tl, h, utt_scale=utt_scale, pg_coef=coef[0].contiguous(),
                                            pg_path=c["paths"][0].contiguous(), ent_scale=ent_scale)
    if entry == "single_per_frame":
        return hipops.ctc_grad_from_lattice(lp, il, tl, h, utt_scale=utt_scale, pg_coef=coef_tb, pg_path=c["paths"][0].contiguous(),
                                            ent_scale=ent_scale)
    if entry == "multi":
        return hipops.ctc_grad_from_lattice_multi(lp, il, tl, h, utt_scale, coef, c["paths"], ent_scale=ent_scale)
    return hipops.ctc_grad_from_lattices_seq(lp, il, tl, h, c["hyp_handle"], utt_scale, coef, c["paths"], c["tok_len"],
                                             ent_scale=ent_scale)


def _raw_null(entry, c, utt_scale, coef, coef_tb):
    """The NEW entry point itself with ent_scale = NULL (the wrappers call the old entry when they have no ent_scale)."""
    from policy_gradient_asr_amd import _lib
    lib = _lib.load()
    _lattices(c)
    T, B, V, K = c["T"], c["B"], c["V"], c["K"]
    ws, Lmax, blank = c["handle"]
    grad = torch.empty_like(c["lp"])
    head = (c["lp"].data_ptr(), c["il"].data_ptr(), c["tl"].data_ptr(), T, B, V, Lmax, blank, utt_scale.data_ptr())
    tail = (grad.data_ptr(), ws.data_ptr(), ws.numel())
    st = torch.cuda.current_stream().cuda_stream
    p0 = c["paths"][0].contiguous()
    if entry == "single":
        c0 = coef[0].contiguous()
        rc = lib.pgasr_ctc_grad_from_lattice_ent(*head, c0.data_ptr(), p0.data_ptr(), 0, None, *tail, st)
    elif entry == "single_per_frame":
        rc = lib.pgasr_ctc_grad_from_lattice_ent(*head, coef_tb.data_ptr(), p0.data_ptr(), 1, None, *tail, st)
    elif entry == "multi":
        rc = lib.pgasr_ctc_grad_from_lattice_multi_ent(*head, K, coef.data_ptr(), c["paths"].data_ptr(), None, *tail, st)
    else:
        hws, _, Lh = c["hyp_handle"]
        rc = lib.pgasr_ctc_grad_from_lattices_seq_ent(*head, K, coef.data_ptr(), c["paths"].data_ptr(), c["tok_len"].data_ptr(), Lh,
                                                      None, *tail, hws.data_ptr(), hws.numel(), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return grad


@pytest.mark.parametrize("T,B,V", SHAPES)
def test_frame_entropy_vs_fp64(T, B, V):
    """ent_mean and ent_scale against fp64 on the device's own fp32 log-probs (rel err < 1e-5), exactly 0 for an empty utterance
    and for the single-symbol alphabet, equal bits from two calls; metrics.frame_entropy is the same kernel."""
    from policy_gradient_asr_amd import hipops, metrics
    c = _policy_case(T, B, V)
    beta, inv_gb = 2.0, 1.0 / 8
    mean, scale = hipops.frame_entropy(c["lp"], c["il"], beta, inv_gb)
    mean2, scale2 = hipops.frame_entropy(c["lp"], c["il"], beta, inv_gb)
    w_mean, w_scale = pg_ref.entropy_stats(c["lg"], c["in_len"].numpy(), beta, inv_gb)
    e_mean, e_scale = rel_err(mean.cpu().numpy(), w_mean), rel_err(scale.cpu().numpy(), w_scale)
    print(f"[frame entropy] T={T} B={B} V={V}: ent_mean rel err {e_mean:.2e}, ent_scale rel err {e_scale:.2e}, "
          f"mean entropy {w_mean.max():.3f} of ln V = {np.log(V):.3f}")
    assert mean.shape == (B,) and scale.shape == (B,)
    assert e_mean < 1e-5 and e_scale < 1e-5
    assert bool(torch.isfinite(mean).all())
    empty = c["in_len"] == 0
    assert bool(empty.any()) and bool((mean.cpu()[empty] == 0).all())
    if V == 1:
        assert bool((mean == 0).all())
    else:
        assert float(mean.max()) > 0.1
    assert torch.equal(mean, mean2) and torch.equal(scale, scale2)
    assert torch.equal(metrics.frame_entropy(c["lp"], c["il"]), mean)
    assert bool((hipops.frame_entropy(c["lp"], c["il"])[1] == 0).all())          # weight 0: the monitoring call


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("T,B,V", SHAPES)
def test_entropy_only_gradient_vs_fp64(T, B, V, entry):
    """utt_scale = 0 and pg_coef = 0 leave the entropy term alone: ent_scale_b p (ln p + H) to rel err < 1e-5 (the bar of
    test_multi_path_ctc_grad_vs_fp64 for the same kernels; an fp32 emulation of the expression sits at 1.5e-7 .. 2.7e-7), rows
    beyond T_b exactly 0, every row summing to <= 1e-5 of its largest entry, finite everywhere -- the -inf rows included."""
    c = _policy_case(T, B, V)
    g = torch.Generator().manual_seed(B)
    ent_scale = torch.rand(B, generator=g) + 0.5
    zeros = lambda *s: torch.zeros(*s, device=DEV)
    grad = _grad(entry, c, zeros(B), zeros(c["K"], B), zeros(T, B), ent_scale.to(DEV)).cpu().numpy()
    il = c["in_len"].numpy()
    want = pg_ref.entropy_grad(c["lg"], il, ent_scale.double().numpy())
    err = rel_err(grad, want) if V > 1 else float(np.abs(grad).max())
    rows = np.abs(grad.astype(np.float64).sum(axis=2))
    tops = np.abs(grad).max(axis=2)
    live = tops > 0
    print(f"[entropy grad] {entry} T={T} B={B} V={V}: rel err {err:.2e}, worst row sum / row max "
          f"{(rows[live] / tops[live]).max() if live.any() else 0.0:.2e}")
    assert np.isfinite(grad).all()
    assert err < 1e-5
    beyond = np.arange(T)[:, None] >= il[None, :]
    assert beyond.any() and (grad[beyond] == 0).all()
    assert (rows <= 1e-5 * tops).all()
    if V >= 5:
        assert (grad[2, 2] == 0).all()                    # the one-hot row: H = 0, a finite, zero gradient
        assert (grad[1, 0, V - 2:] == 0).all() and np.abs(grad[1, 0]).max() > 0
    if V == 1:
        assert (grad == 0).all()


@pytest.mark.parametrize("entry", ENTRIES)
def test_full_gradient_with_entropy_vs_fp64(entry):
    """CTC + K REINFORCE terms + entropy (beta = 2, ent_scale from the entropy kernel) at T,B,V,L = 160,6,29,14 against ctc_ref +
    decode_ref.reinforce_grad + the entropy helper: rel err < 1e-5."""
    from policy_gradient_asr_amd import hipops
    T, B, V, K = 160, 6, 29, 4
    c = sampled_case(T, B, V, K)                  # lattice_case's logits and targets (L = 14), sampled paths, their hypotheses
    c.update(il=c["in_len"].to(DEV), tl=c["tg_len"].to(DEV), tg=c["targets"].to(DEV))
    g = torch.Generator().manual_seed(7)
    coef = torch.randn(K, B, generator=g) * 0.1
    coef_tb = torch.randn(T, B, generator=g) * 0.1
    scale = torch.rand(B, generator=g) + 0.5
    beta, inv_gb = 2.0, 1.0 / B
    _, ent_scale = hipops.frame_entropy(c["lp"], c["il"], beta, inv_gb)
    grad = _grad(entry, c, scale.to(DEV), coef.to(DEV), coef_tb.to(DEV), ent_scale)
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
    ent = pg_ref.entropy_grad(lg, il, pg_ref.entropy_stats(lg, il, beta, inv_gb)[1])
    err = rel_err(grad.cpu().numpy(), want + ent)
    print(f"[full grad + entropy] {entry}: rel err {err:.2e}; without the entropy term the reference differs by "
          f"{rel_err(want, want + ent):.2e}")
    assert rel_err(want, want + ent) > 10 * 1e-5      # the term is visible at this bound
    assert err < 1e-5


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_ent_scale_is_the_existing_entry(entry):
    """The new entry point with ent_scale = NULL against the existing one on the same inputs: equal bits."""
    T, B, V, K = 160, 6, 29, 4
    c = sampled_case(T, B, V, K)
    c.update(il=c["in_len"].to(DEV), tl=c["tg_len"].to(DEV), tg=c["targets"].to(DEV))
    g = torch.Generator().manual_seed(3)
    coef = (torch.randn(K, B, generator=g) * 0.1).to(DEV)
    coef_tb = (torch.randn(T, B, generator=g) * 0.1).to(DEV)
    scale = (torch.rand(B, generator=g) + 0.5).to(DEV)
    old = _grad(entry, c, scale, coef, coef_tb, None)
    new = _raw_null(entry, c, scale, coef, coef_tb)
    assert bool(torch.isfinite(old).all()) and float(old.abs().max()) > 0
    assert torch.equal(old, new)


# ---- the trainer ----
HEAD_GAIN = 80.0


def _entropy_step_vs_oracle(mode, B=4, K=4, beta=2.0, seed=51):
    """test_multisample_pg_gpu._multi_step_vs_oracle with entropy_weight = beta: one lambda = 1 trainer step (f32 mode, greedy
    hypothesis) against the torch-CPU model in FP64 on the same weights -- rewards exact, loss within 1e-5, every parameter gradient
    within 1e-4 (max norm), last_entropy within 1e-5 of the entropy of the oracle's logits.  mode: "multi" (K paths, path-level
    score), "sequence" (K paths, sequence-level score), "per_step" (one path, per-frame coefficients).
    The same shapes, seeds and weights, except that the head's weight and bias are multiplied by HEAD_GAIN: init_params starts from
    a policy within 1e-3 nats of uniform, and p (ln p + H) VANISHES at the uniform policy -- there the entropy term moves the
    oracle's parameter gradients by 2e-3 .. 8e-3 only, which a 1e-4 bound does not separate from a missing term by the two orders
    the sensitivity condition asks for.  With the gain the policy's mean frame entropy is about 1.0 nat and the term moves every
    parameter gradient by 1.5e-2 .. 1.4e-1."""
    K = 1 if mode == "per_step" else K
    tkw, okw = {"multi": ({}, {}), "sequence": (dict(score_function="sequence"),) * 2,
                "per_step": (dict(reward_mode="per_step"), dict(per_step=True))}[mode]
    r = trainer_step_vs_oracle(dict(reward_decoder="greedy", num_samples=K, entropy_weight=beta, **tkw),
                               dict(num_samples=K, entropy_weight=beta, **okw), B=B, head_gain=HEAD_GAIN, seed=seed,
                               label=f"[entropy step] {mode} B={B} K={K} beta={beta}")
    tr, o = r.trainer, r.oracle
    assert all(s_.shape == (B,) for s_ in tr.last_stats) and tr.last_sample_rewards.shape == (K, B)
    assert tr.last_entropy.shape == (B,) and not tr.last_entropy.requires_grad
    np.testing.assert_allclose(tr.last_entropy.cpu().numpy(), o.ent_mean, rtol=1e-5)
    # sensitivity: without the term EVERY parameter gradient of the oracle is more than 100 bounds away, so the bound cannot hide a
    # missing term
    plain = pg_ref.pg_objective(*r.args, **dict(r.kw, entropy_weight=0.0))
    without = r.backprop(plain.grad)
    moved = {k: rel_err(without[k], r.grads[k]) for k in r.grads}
    least = min(moved, key=moved.get)
    print(f"[entropy step] {mode} B={B} K={K} beta={beta}: the term is {abs(o.loss - plain.loss) / abs(o.loss):.2e} of the loss and "
          f"moves the oracle's gradients by {moved[least]:.2e} ({least}) .. {max(moved.values()):.2e}")
    assert moved[least] > 100 * 1e-4, (least, moved[least])
    assert abs(o.loss - plain.loss) / abs(o.loss) > 100 * 1e-5
    assert np.abs(o.coef).max() > 0
    return tr


@pytest.mark.parametrize("mode", ["multi", "sequence", "per_step"])
def test_entropy_step_vs_oracle(mode):
    _entropy_step_vs_oracle(mode)


def test_ragged_batch_with_entropy_vs_oracle():
    """B = 3 is padded to 16 with empty utterances: they add no entropy, last_entropy covers the three real rows, and loss and
    gradients are the oracle's over the three real utterances."""
    tr = _entropy_step_vs_oracle("multi", B=3)
    assert tr.last_entropy.shape == (3,) and bool((tr.last_entropy > 0).all())
    from policy_gradient_asr_amd.loss import PGCTCLossFn
    assert PGCTCLossFn.last_entropy.shape == (16,) and bool((PGCTCLossFn.last_entropy[3:] == 0).all())


@pytest.mark.parametrize("kw", [{}, {"num_samples": 4}, {"score_function": "sequence"}, {"reward_mode": "per_step"}],
                         ids=["single", "multi", "sequence", "per_step"])
def test_weight_zero_is_the_default_step(kw, monkeypatch):
    """entropy_weight = 0.0: the same bits in loss and every gradient as a trainer built without the argument, no entropy launch."""
    from policy_gradient_asr_amd import hipops
    calls = []
    real = hipops.frame_entropy
    monkeypatch.setattr(hipops, "frame_entropy", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    batch, _ = _batch(16)
    res = []
    for extra in ({}, {"entropy_weight": 0.0}):
        tr = _trainer(**kw, **extra)
        loss = tr.compute_gradients(*batch)
        torch.cuda.synchronize()
        hipops.lstm_assert_no_timeouts()
        assert tr.last_entropy is None
        res.append((loss.clone(), tr.gflat.clone()))
    assert not calls
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][1].abs().max()) > 0
    tr = _trainer(**kw, entropy_weight=0.5)            # .. and the counter does count
    tr.compute_gradients(*batch)
    torch.cuda.synchronize()
    assert len(calls) == 1 and tr.last_entropy.shape == (16,)
    assert not torch.equal(tr.gflat, res[0][1])


def test_entropy_shards_sum_to_the_whole_batch():
    """test_leave_one_out_shards_sum_to_the_whole_batch with entropy_weight = 2: nothing in the term is sampled and ent_scale is
    normalised by the global batch, so two halves give the whole batch's gradient and loss (its 1e-6)."""
    from policy_gradient_asr_amd.loss import PGCTCLossFn, pg_ctc_loss
    T, B, V, L, K = 150, 8, 29, 12, 4
    kw = dict(lam=1.0, seed=11, offset=4, num_samples=K, baseline="leave_one_out", entropy_weight=2.0)
    r = shards_vs_whole(kw, lattice_case(T, B, V, L, 77), extra=lambda: PGCTCLossFn.last_entropy)
    plain = r.lg.clone().requires_grad_(True)
    pg_ctc_loss(plain, r.il, r.tg, r.tl, **dict(kw, entropy_weight=0.0))[0].backward()
    assert float((plain.grad - r.grad).abs().max()) > 1e-3 * float(r.grad.abs().max())       # the term is in there
    assert torch.equal(torch.cat(r.extra_parts), r.extra_whole)


def test_entropy_accumulated_step_is_the_whole_batch():
    """step_accumulated over two micro-batches of 16 (padded to one T) against one step on their concatenation, entropy_weight = 2,
    K = 4: test_accumulated_step_is_the_whole_batch's f32 bounds (loss 1e-6, gflat 1e-5); last_entropy holds all 32 real rows in call
    order."""
    from policy_gradient_asr_amd import hipops
    batch, _ = _batch(32)
    parts = _slices((16, 16))
    kw = dict(num_samples=4, entropy_weight=2.0, lr=1e-3)
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
    eerr = rel_err(acc.last_entropy.cpu(), whole.last_entropy.cpu())
    print(f"[entropy accum] gflat {gerr:.2e} loss {lerr:.2e} last_entropy {eerr:.2e}")
    assert acc.last_entropy.shape == (32,) and whole.last_entropy.shape == (32,)
    assert torch.equal(acc.last_sample_rewards, whole.last_sample_rewards)
    # the order is checked: the two micro-batches the other way round would miss the bound below
    assert rel_err(whole.last_entropy.cpu().roll(16), whole.last_entropy.cpu()) > 1e-6
    assert eerr < 1e-6
    assert lerr <= 1e-6
    assert gerr < 1e-5
    assert acc.nstep == 1 and acc.applied_steps() == 1


def test_train_driver_records_entropy_weight(tmp_path, capsys):
    """model.train(entropy_weight=): trains with it, prints the batch-mean entropy, records it in the checkpoint, warns on a resume
    with another weight."""
    from policy_gradient_asr_amd.model import train
    corpus, out, ds = tiny_corpus(tmp_path)
    l1, _ = train(str(corpus), str(out), 2, 16, 0, train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=1, entropy_weight=0.5)
    assert len(l1) == 2 and all(np.isfinite(l1))
    printed = capsys.readouterr().out
    shown = [float(line.split("Entropy:")[1]) for line in printed.splitlines() if "Entropy:" in line]
    assert len(shown) == 4 and all(0.0 < h <= np.log(6) + 1e-6 for h in shown)
    st = torch.load(out / "checkpoint_last.pth", map_location="cpu")
    assert st["entropy_weight"] == 0.5
    train(str(corpus), str(out), 3, 16, 0, train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=0, entropy_weight=0.25)
    printed = capsys.readouterr().out
    assert "entropy_weight=0.25" in printed and "Entropy:" not in printed
    with pytest.raises(ValueError, match="entropy_weight"):
        train(str(corpus), str(out), 3, 16, 0, train_dataset=ds, n_feats=20, entropy_weight=-1.0)


def test_entropy_bonus_keeps_the_policy_wider():
    """Ten steps on one fixed batch with lam = 0 and lr = 3e-3, eval-mode dropout: with entropy_weight = 5 the batch-mean entropy the
    tenth step sees is strictly above that of the same run with weight 0.  Only the direction is asserted -- it follows from the sign
    of the term."""
    from policy_gradient_asr_amd import hipops, metrics
    batch, _ = _batch(16)
    x, _, fmask, _ = batch
    seen = {}
    for w in (0.0, 5.0):
        tr = _trainer(lr=3e-3, entropy_weight=w)
        tr.lam = 0.0
        for i in range(10):
            if i == 9:
                with torch.no_grad():
                    logits, in_len = tr.model.logits(x, fmask)
                    monitor = metrics.frame_entropy(hipops.log_softmax_rows(logits.detach().contiguous()), in_len)
            tr.step(*batch)
        torch.cuda.synchronize()
        hipops.lstm_assert_no_timeouts()
        assert tr.applied_steps() == 10
        if w > 0:
            # what the step reports is what the monitoring call measures on the same weights
            assert rel_err(tr.last_entropy.cpu(), monitor.cpu()) < 1e-5
            seen[w] = float(tr.last_entropy.mean())
        else:
            assert tr.last_entropy is None
            seen[w] = float(monitor.mean())
    print(f"[entropy behaviour] batch-mean frame entropy at step 10: weight 0 -> {seen[0.0]:.4f}, weight 5 -> {seen[5.0]:.4f} "
          f"(ln V = {np.log(29):.4f})")
    assert np.isfinite(seen[0.0]) and np.isfinite(seen[5.0])
    assert seen[5.0] > seen[0.0]
