"""score_function="sequence" on the MI355X: the hypothesis lattices, the gradient pass over K+1 lattices and the loss value against
fp64 references, the composition of the existing kernels on a K-fold expanded batch, the whole trainer step against the torch-CPU
fp64 model, shards and micro-batches, the untouched default and the train driver."""
import numpy as np
import pytest
import torch

from oracle import ctc_ref
from pg_harness import (D, DEV, _batch, _rows, _slices, _trainer, fused_grad_ref, lattice_case, rel_err, sampled_case,
                        shards_vs_whole, tiny_corpus, trainer_step_vs_oracle)

pytestmark = pytest.mark.gpu


def _hyp_nll_ref(c):
    """nll(y_k,b | x_b) in fp64 on the device's log-probs."""
    tn, ln = c["tokens"].cpu().numpy(), c["tok_len"].cpu().numpy()
    out = np.zeros((c["K"], c["B"]))
    for k in range(c["K"]):
        for b in range(c["B"]):
            Tb = int(c["in_len"][b])
            if Tb == 0:
                out[k, b] = 0.0 if ln[k, b] == 0 else np.inf
                continue
            out[k, b] = ctc_ref.ctc_alpha_beta(c["lg"][:Tb, b], tn[k, b, :ln[k, b]].astype(np.int64))[2]
    return out


@pytest.mark.parametrize("name,T,B,V,K", [("base", 160, 6, 29, 4), ("V64", 160, 6, 64, 4), ("long", 1000, 2, 29, 2)])
def test_hypothesis_nll_vs_fp64(name, T, B, V, K):
    """Hypotheses = collapse of sampled paths, one utterance without frames, one all-blank path; T = 1000 with 900+-token
    hypotheses runs the 8-states-per-thread variant.  rtol 1e-5: test_ctc_headline_size_properties' bar for the target lattice."""
    from policy_gradient_asr_amd import hipops
    in_len = [T - 37 * (b % 4) for b in range(B)]
    if name != "long":
        in_len[4] = 0
    c = sampled_case(T, B, V, K, in_len=in_len, blank_path=(1, 2) if name != "long" else None)
    Lh = hipops.hyp_len_cap(T)
    ln = c["tok_len"].cpu().numpy()
    if name == "long":
        assert ln.max() >= 900 and 2 * ln.max() + 1 > 4 * 256
    else:
        assert ln[1, 2] == 0 and (ln[:, 4] == 0).all()
    hyp_nll, _ = hipops.ctc_hyp_lattice(c["lp"], c["tokens"], c["tok_len"], c["in_len"].to(DEV), Lh)
    again, _ = hipops.ctc_hyp_lattice(c["lp"], c["tokens"], c["tok_len"], c["in_len"].to(DEV), Lh)
    want = _hyp_nll_ref(c)
    got = hyp_nll.cpu().numpy()
    assert np.isfinite(want).all()            # a hypothesis is always feasible: its own path aligns it
    print(f"[hyp nll] {name}: lengths {ln.min()}..{ln.max()}, max rel err "
          f"{np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-30) * (want != 0)):.2e}")
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)
    assert torch.equal(hyp_nll, again)        # run-to-run reproducible
    # a cap below a pair's length skips it: nll reads 0, the others are unchanged bit for bit
    cap = int(np.median(ln))
    capped, _ = hipops.ctc_hyp_lattice(c["lp"], c["tokens"], c["tok_len"], c["in_len"].to(DEV), cap)
    keep = c["tok_len"] <= cap
    assert torch.equal(capped[keep], hyp_nll[keep]) and (capped[~keep] == 0).all() and bool((~keep).any())


def _fused(c, coef, scale, Lh):
    from policy_gradient_asr_amd import hipops
    il, tl, tg = c["in_len"].to(DEV), c["tg_len"].to(DEV), c["targets"].to(DEV)
    nll, handle = hipops.ctc_lattice(c["lp"], tg, il, tl)
    hyp_nll, hh = hipops.ctc_hyp_lattice(c["lp"], c["tokens"], c["tok_len"], il, Lh)
    grad = hipops.ctc_grad_from_lattices_seq(c["lp"], il, tl, handle, hh, scale.to(DEV), coef.to(DEV), c["paths"], c["tok_len"])
    return nll, hyp_nll, grad


@pytest.mark.parametrize("cap", ["all", "median", "zero"])
@pytest.mark.parametrize("K", [1, 4, 16])
def test_fused_gradient_vs_fp64(K, cap):
    """Random pg_coef of both signs; Lh = T (all sequence-scored), the median collapsed length (mixed) and 0 (only the empty
    hypothesis).  Max-norm relative error < 1e-5, test_multi_path_ctc_grad_vs_fp64's bound."""
    T, B, V = 160, 6, 29
    c = sampled_case(T, B, V, K, blank_path=(0, 1))
    ln = c["tok_len"].cpu().numpy()
    Lh = {"all": T, "median": int(np.median(ln)), "zero": 0}[cap]
    share = float((ln <= Lh).mean())
    print(f"[fused grad] K={K} cap={cap}: lengths {ln.min()}..{ln.max()}, Lh {Lh}, {int((ln <= Lh).sum())} of {ln.size} sequence-scored")
    if cap == "median":
        assert 0.25 <= share <= 0.75          # really mixed: each branch holds at least a quarter of the samples
    elif cap == "zero":
        assert (ln <= Lh).sum() == 1
    else:
        assert share == 1.0
    g = torch.Generator().manual_seed(K)
    coef = torch.randn(K, B, generator=g) * 0.1
    assert (coef > 0).any() and (coef < 0).any()
    scale = torch.rand(B, generator=g) + 0.5
    _, _, grad = _fused(c, coef, scale, Lh)
    err = rel_err(grad.cpu().numpy(), fused_grad_ref(c, coef, scale, Lh))
    print(f"[fused grad] K={K} cap={cap}: rel err {err:.2e}")
    assert err < 1e-5
    _, _, again = _fused(c, coef, scale, Lh)
    assert torch.equal(grad, again)


def test_fused_gradient_is_the_existing_kernels_on_an_expanded_batch():
    """No K-fold copy of the log-probs, same answer: ctc_loss_grad on (T, K*B, V) with utt_scale = pg_coef, summed over k in
    fp64, plus the target part."""
    from policy_gradient_asr_amd import hipops
    T, B, V, K = 160, 6, 29, 4
    c = sampled_case(T, B, V, K, blank_path=(0, 1))
    g = torch.Generator().manual_seed(9)
    coef = torch.randn(K, B, generator=g) * 0.1
    scale = torch.rand(B, generator=g) + 0.5
    nll, hyp_nll, grad = _fused(c, coef, scale, T)
    il, tl, tg = c["in_len"].to(DEV), c["tg_len"].to(DEV), c["targets"].to(DEV)
    nll_t, g_t = hipops.ctc_loss_grad(c["lp"], tg, il, tl, utt_scale=scale.to(DEV))
    g_t = g_t.double().clone()
    lp_exp = c["lp"].repeat(1, K, 1).contiguous()                     # column k*B + b = utterance b
    nll_h, g_h = hipops.ctc_loss_grad(lp_exp, c["tokens"].view(K * B, T), il.repeat(K), c["tok_len"].view(K * B),
                                      utt_scale=coef.to(DEV).view(K * B).contiguous())
    want = g_t + g_h.double().view(T, K, B, V).sum(dim=1)
    err = rel_err(grad.cpu().numpy(), want.cpu().numpy())
    print(f"[fused vs expanded batch] rel err {err:.2e}")
    assert err < 1e-5
    assert torch.equal(nll, nll_t)
    np.testing.assert_allclose(hyp_nll.view(-1).cpu().numpy(), nll_h.cpu().numpy(), rtol=1e-6)


def test_loss_value_vs_fp64_and_reproducible():
    """terms[b] against fp64 arithmetic on the kernel's inputs (as test_multi_rewards_and_loss_value_vs_numpy checks the path-level
    value): < 1e-6 relative; the same with the hypothesis nll from the fp64 lattice: the nll's own bar, 1e-5.  Mixed cap."""
    from policy_gradient_asr_amd import hipops
    T, B, V, K = 160, 6, 29, 4
    c = sampled_case(T, B, V, K, blank_path=(0, 1))
    ln = c["tok_len"].cpu().numpy()
    Lh = int(np.median(ln))
    g = torch.Generator().manual_seed(2)
    coef = (torch.randn(K, B, generator=g) * 0.1).to(DEV)
    us = (torch.rand(B, generator=g) * 0.1 + 0.01).to(DEV)
    il = c["in_len"].to(DEV)
    nll, _ = hipops.ctc_lattice(c["lp"], c["targets"].to(DEV), il, c["tg_len"].to(DEV))
    hyp_nll, _ = hipops.ctc_hyp_lattice(c["lp"], c["tokens"], c["tok_len"], il, Lh)
    terms = hipops.pg_loss_value_seq(c["lp"], c["paths"], il, nll, us, coef, hyp_nll, c["tok_len"], Lh)
    again = hipops.pg_loss_value_seq(c["lp"], c["paths"], il, nll, us, coef, hyp_nll, c["tok_len"], Lh)
    assert torch.equal(terms, again)
    mask = np.arange(T)[:, None] < c["in_len"].numpy()[None, :]
    pn = c["paths"].cpu().numpy().astype(np.int64)
    c64, u64 = coef.cpu().double().numpy(), us.cpu().double().numpy()
    seq = ln <= Lh
    assert seq.any() and (~seq).any()

    def value(hn):
        want = nll.cpu().double().numpy() * u64
        for k in range(K):
            lps = (np.take_along_axis(c["lg"], pn[k][..., None], axis=2)[..., 0] * mask).sum(axis=0)
            want = want + c64[k] * np.where(seq[k], hn[k], -lps)
        return want

    on_inputs = rel_err(terms.cpu().numpy(), value(hyp_nll.cpu().double().numpy()))
    ref = _hyp_nll_ref(c)
    on_oracle = rel_err(terms.cpu().numpy(), value(np.where(seq, ref, 0.0)))
    per_utt = np.abs(terms.cpu().numpy() - value(hyp_nll.cpu().double().numpy())) / np.abs(value(hyp_nll.cpu().double().numpy()))
    print(f"[seq loss value] rel err on the kernel's inputs {on_inputs:.2e} (per utterance max {per_utt.max():.2e}), "
          f"with the fp64 lattice's nll {on_oracle:.2e}")
    assert on_inputs < 1e-6 and per_utt.max() < 1e-6
    assert on_oracle < 1e-5
    # Lh = T: no path sum at all; Lh = 0 and no empty hypothesis left: pg_loss_value_multi's value
    ones = torch.ones_like(c["tok_len"])
    all_path = hipops.pg_loss_value_seq(c["lp"], c["paths"], il, nll, us, coef, hyp_nll, ones, 0)
    multi = hipops.pg_loss_value_multi(c["lp"], c["paths"], il, nll, us, coef)
    assert rel_err(all_path.cpu().numpy(), multi.cpu().numpy()) < 1e-6


def _seq_step_vs_oracle(reward_baseline, beam, K, word=False, seed=51):
    """One lambda = 1 trainer step (f32 mode, score_function="sequence") against the torch-CPU model in FP64 on the same weights, as
    test_multisample_pg_gpu._multi_step_vs_oracle: rewards exact (rtol 1e-6), loss within 1e-5, every parameter gradient within
    1e-4 (max norm).  The oracle collapses its own sampled paths and takes the hypotheses' gradients from ctc_ref."""
    unit = dict(reward_unit="word", word_delimiter=D) if word else {}
    r = trainer_step_vs_oracle(dict(reward_decoder="beam" if beam else "greedy", beam_size=beam or 16, num_samples=K,
                                    reward_baseline=reward_baseline, score_function="sequence", **unit),
                               dict(num_samples=K, baseline=reward_baseline, beam=beam, score_function="sequence", **unit),
                               word=word, seed=seed, label=f"[seq step] K={K} {reward_baseline} beam={beam} word={word}")
    tr = r.trainer
    assert all(s_.shape == (4,) for s_ in tr.last_stats) and tr.last_sample_rewards.shape == (K, 4)
    scored = tr.last_sequence_scored
    assert scored.shape == (K, 4) and scored.dtype == torch.bool and bool(scored.all())       # T <= 1023, no cap
    assert r.oracle.scored.all() and np.abs(r.oracle.coef).max() > 0


@pytest.mark.parametrize("baseline,beam,K,word", [("hypothesis", 0, 4, False), ("leave_one_out", 0, 4, False),
                                                  ("hypothesis", 16, 4, False), ("hypothesis", 0, 1, False),
                                                  ("leave_one_out", 0, 4, True)])
def test_sequence_step_vs_oracle(baseline, beam, K, word):
    _seq_step_vs_oracle(baseline, beam, K, word)


@pytest.mark.parametrize("max_hyp_len", [None, 100])
def test_sequence_shards_sum_to_the_whole_batch(max_hyp_len):
    """Two pg_ctc_loss calls on the halves of a batch (global_batch, sample_base) give the whole batch's logits gradient, 1e-6 of
    its max, as test_leave_one_out_shards_sum_to_the_whole_batch; with a cap that splits the samples too."""
    from policy_gradient_asr_amd.loss import PGCTCLossFn, pg_ctc_loss
    T, B, V, L, K = 150, 8, 29, 12, 4
    kw = dict(lam=1.0, seed=11, offset=4, num_samples=K, baseline="leave_one_out", score_function="sequence", max_hyp_len=max_hyp_len)
    r = shards_vs_whole(kw, lattice_case(T, B, V, L, 77), extra=lambda: PGCTCLossFn.last_sequence_scored)
    scored = r.extra_whole
    assert scored.shape == (K, B)
    if max_hyp_len is None:
        assert bool(scored.all())
    else:
        assert bool(scored.any()) and not bool(scored.all())
    assert torch.equal(torch.cat(r.extra_parts, dim=1), scored)
    # the sequence-level gradient is another estimator than the path-level one, around the same CTC part
    other = r.lg.clone().requires_grad_(True)
    kw_path = {k: v for k, v in kw.items() if k not in ("score_function", "max_hyp_len")}
    pg_ctc_loss(other, r.il, r.tg, r.tl, **kw_path)[0].backward()
    assert float((other.grad - r.grad).abs().max()) > 1e-6 * float(r.grad.abs().max())


@pytest.mark.parametrize("sizes", [(16, 16), (16, 9, 7)])
def test_sequence_accumulated_step_is_the_whole_batch(sizes):
    """One step_accumulated over micro-batches (ragged ones are padded with empty utterances) against one step on the whole batch:
    the same rewards and scored flags, loss within 1e-6 and gflat within 1e-5, test_accumulated_step_is_the_whole_batch's f32
    bounds."""
    from policy_gradient_asr_amd import hipops
    kw = dict(num_samples=4, reward_baseline="leave_one_out", score_function="sequence", max_hyp_len=48)
    batch, _ = _batch(32)
    parts = _slices(sizes)
    whole = _trainer("f32", **kw)
    loss_w = float(whole.step(*batch))
    acc = _trainer("f32", **kw)
    loss_a = float(acc.step_accumulated([_rows(batch, p) for p in parts]))
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    assert whole.nstep == acc.nstep == 1 and whole.applied_steps() == acc.applied_steps() == 1
    assert whole.last_sequence_scored.shape == acc.last_sequence_scored.shape == (4, 32)
    assert torch.equal(acc.last_sequence_scored, whole.last_sequence_scored)
    share = float(whole.last_sequence_scored.float().mean())
    assert torch.equal(acc.last_sample_rewards, whole.last_sample_rewards)
    gerr = rel_err(acc.gflat.cpu(), whole.gflat.cpu())
    lerr = abs(loss_a - loss_w) / abs(loss_w)
    print(f"[seq accum] {sizes}: gflat {gerr:.2e} loss {lerr:.2e}, {share:.2f} of the samples sequence-scored")
    assert share > 0.0
    assert lerr <= 1e-6
    assert gerr < 1e-5
    assert float(acc.gflat.abs().max()) > 0


def test_default_score_function_is_path_bit_for_bit():
    from policy_gradient_asr_amd.loss import PGCTCLossFn, pg_ctc_loss
    T, B, V, L = 150, 8, 29, 12
    logits, targets, in_len, tg_len = lattice_case(T, B, V, L, 78)
    lg = logits.float().to(DEV)
    tg, il, tl = targets.to(DEV), in_len.to(DEV), tg_len.to(DEV)
    for extra in ({}, {"num_samples": 4, "baseline": "leave_one_out"}, {"beam": 8}):
        out = []
        for kw in ({}, {"score_function": "path"}):
            z = lg.clone().requires_grad_(True)
            res = pg_ctc_loss(z, il, tg, tl, lam=1.0, seed=5, offset=2, **extra, **kw)
            res[0].backward()
            assert PGCTCLossFn.last_sequence_scored is None
            out.append((res[0].detach(), z.grad) + tuple(res[1:]))
        assert all(torch.equal(a, b) for a, b in zip(*out))
    batch, _ = _batch(16)
    a, b = _trainer("f32"), _trainer("f32", score_function="path")
    la, lb = a.step(*batch), b.step(*batch)
    assert torch.equal(la, lb) and torch.equal(a.gflat, b.gflat) and torch.equal(a.flat, b.flat)
    assert a.last_sequence_scored is None and b.last_sequence_scored is None
    # K = 1 with the hypothesis baseline is legal with "sequence" and runs the multi-sample section
    c = _trainer("f32", score_function="sequence")
    lc = c.step(*batch)
    assert c.last_sequence_scored.shape == (1, 16) and np.isfinite(float(lc))
    assert torch.equal(c.last_stats[1], a.last_stats[1])         # the same draws, the same rewards


def test_train_driver_records_score_function(tmp_path, capsys):
    """model.train(score_function, max_hyp_len): trains with them, records them in the checkpoint, warns on a resume with others."""
    from policy_gradient_asr_amd.model import train
    corpus, out, ds = tiny_corpus(tmp_path)
    common = dict(train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=0, num_samples=4, reward_baseline="leave_one_out")
    l1, _ = train(str(corpus), str(out), 2, 16, 0, score_function="sequence", **common)
    assert len(l1) == 2 and all(np.isfinite(l1))
    st = torch.load(out / "checkpoint_last.pth", map_location="cpu")
    assert (st["score_function"], st["max_hyp_len"]) == ("sequence", None)
    capsys.readouterr()
    train(str(corpus), str(out), 3, 16, 0, score_function="sequence", max_hyp_len=50, **common)
    printed = capsys.readouterr().out
    assert "max_hyp_len=50" in printed and "score_function" not in printed
    train(str(corpus), str(out), 4, 16, 0, **common)
    printed = capsys.readouterr().out
    assert "score_function=path" in printed
