"""MWER training over N-best lists on the device: the single-wave beam kernel's N-best tail (csrc/beam.hip, NBEST = true) against
the plain-Python helper of tests/nbest_ref.py and against the in-step 1-best search bit for bit, the weights kernel (csrc/nbest.hip)
against its numpy statement, ``mwer_ctc_loss`` against the fp64 reference of tests/mwer_ref.py on the device's own lists, its
identities, and ``MWERTrainer`` against the fp64 oracle, under accumulation and clipping, and through the train driver."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as R  # noqa: E402
import mwer_ref as MR  # noqa: E402
import nbest_ref as NR  # noqa: E402
import pg_harness as H  # noqa: E402
from oracle import model_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = H.DEV
GARBAGE = 0x5A5A5A5A


def _fast_nbest_raw(lp, lens, beam, N, blank, collapse=False, flags=8):
    """pgasr_ctc_beam_search_nbest with the fast bit, into GARBAGE-FILLED outputs: a store the kernel misses shows."""
    from policy_gradient_asr_amd import _lib, hipops
    lib = _lib.load()
    T, B, V = lp.shape
    tokens = torch.full((N, B, T), GARBAGE, dtype=torch.int32, device=DEV)
    tl = torch.full((N, B), GARBAGE, dtype=torch.int32, device=DEV)
    score = torch.full((N, B), float("nan"), dtype=torch.float64, device=DEV)
    count = torch.full((B,), GARBAGE, dtype=torch.int32, device=DEV)
    ws = hipops._workspace(lib.pgasr_beam_workspace_bytes(T, B, V, beam), lp.device, "beam")
    st = lib.pgasr_ctc_beam_search_nbest(lp.data_ptr(), 0, lp.stride(0), lp.stride(1), lens.data_ptr(), T, B, V, beam, blank,
                                         int(collapse) | flags, N, tokens.data_ptr(), T, tl.data_ptr(), score.data_ptr(), count.data_ptr(),
                                         ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream, None, 0, 0.0, 0.0)
    _lib.check(st, "pgasr_ctc_beam_search_nbest")
    return hipops.CTCNBest(tokens, tl, score, count)


def _check_list(nb, b, hyps, rel):
    tok, ln, sc = nb.tokens[:, b].cpu().numpy(), nb.lengths[:, b].cpu().numpy(), nb.score[:, b].cpu().numpy()
    assert int(nb.count[b]) == len(hyps)
    for r, (want, wscore) in enumerate(hyps):
        assert list(tok[r, :ln[r]]) == list(want), (b, r)
        assert sc[r] == pytest.approx(wscore, rel=rel), (b, r)
        assert not tok[r, ln[r]:].any()
    for r in range(len(hyps), tok.shape[0]):
        assert ln[r] == 0 and sc[r] == np.inf and not tok[r].any(), (b, r)


@pytest.mark.parametrize("case", NR.NOLM_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_single_wave_nbest_matches_the_helper(case):
    """The fast call on the shared no-LM fp32 cases (B = 5 ragged lengths with a 0 and a 1) at N = list_size(beam): every rank token
    for token, scores 1e-6 relative (the fp32 bound of tests/test_nbest_gpu.py), rows beyond count and token tails as documented,
    every utterance's margin >= GAP_MIN.  The beam-100 case is outside the single-wave kernel: the call of today, bit for bit."""
    from policy_gradient_asr_amd import hipops
    T, V, beam, blank, seed = case
    lp_h, lens_h = NR.nolm_case_inputs(case)
    lp, lens = torch.from_numpy(lp_h).to(DEV), torch.from_numpy(lens_h).to(DEV)
    N = NR.list_size(beam)
    nb = _fast_nbest_raw(lp, lens, beam, N, blank)
    ref = NR.fast_reference(case, False)
    for b in range(R.FAST_B):
        hyps, gap = ref[b]
        print(f"single-wave {case} b={b} n={int(lens_h[b])}: {len(hyps)} ranks, gap {gap:.3e}, score[0] {float(nb.score[0, b])!r} reference {hyps[0][1]!r}")
        assert gap >= R.GAP_MIN
        _check_list(nb, b, hyps, 1e-6)
        if lens_h[b] == 0:
            assert int(nb.count[b]) == 1 and int(nb.lengths[0, b]) == 0 and float(nb.score[0, b]) == 0.0 and np.signbit(float(nb.score[0, b]))
    via = hipops.ctc_beam_search_nbest(lp, lens, beam=beam, nbest=N, blank=blank, fast=True)
    assert all(torch.equal(a, b_) for a, b_ in zip(via, nb))
    if beam > 16:
        slow = hipops.ctc_beam_search_nbest(lp, lens, beam=beam, nbest=N, blank=blank)
        assert all(torch.equal(a, b_) for a, b_ in zip(slow, nb))


@pytest.mark.parametrize("V", [29, 64])
def test_row_0_is_the_in_step_1_best_bit_for_bit(V):
    """fast=True: row 0 == ctc_beam_search(...) in its default dispatch (the single-wave kernel) in tokens, length and score, with and
    without collapse; a shorter list is the bitwise prefix of a longer one; collapsed rows are the plain rows with adjacent duplicates
    removed, the scores untouched."""
    from policy_gradient_asr_amd import hipops
    T, B, beam, N = 120, 4, 16, 16
    rng = np.random.default_rng(5 + V)
    logits = rng.normal(size=(T, B, V)) * 1.2
    logits[10:13, :, 3] += 8.0; logits[13:15, :, 0] += 8.0; logits[15:18, :, 3] += 8.0      # "3, blank, 3": an adjacent duplicate
    lp = torch.from_numpy(R.log_softmax32(logits)).to(DEV)
    lens = torch.tensor([T, 83, 1, 0], dtype=torch.int32, device=DEV)
    plain, coll = _fast_nbest_raw(lp, lens, beam, N, 0), _fast_nbest_raw(lp, lens, beam, N, 0, collapse=True)
    for flag, nb in ((False, plain), (True, coll)):
        one = hipops.ctc_beam_search(lp, lens, beam=beam, collapse=flag)
        assert torch.equal(nb.tokens[0], one[0]) and torch.equal(nb.lengths[0], one[1]) and torch.equal(nb.score[0], one[2])
        for n in (1, 5):
            short = _fast_nbest_raw(lp, lens, beam, n, 0, collapse=flag)
            assert torch.equal(short.tokens, nb.tokens[:n]) and torch.equal(short.lengths, nb.lengths[:n])
            assert torch.equal(short.score, nb.score[:n]) and torch.equal(short.count, nb.count.clamp(max=n))
    assert torch.equal(plain.score, coll.score) and torch.equal(plain.count, coll.count)
    dups = 0
    for b in range(B):
        tok, ln = plain.tokens[:, b].cpu().numpy(), plain.lengths[:, b].cpu().numpy()
        ctok, cln = coll.tokens[:, b].cpu().numpy(), coll.lengths[:, b].cpu().numpy()
        for r in range(N):
            seq = list(tok[r, :ln[r]])
            dedup = [x for i, x in enumerate(seq) if i == 0 or x != seq[i - 1]]
            dups += len(dedup) < len(seq)
            assert list(ctok[r, :cln[r]]) == dedup and not ctok[r, cln[r]:].any() and not tok[r, ln[r]:].any()
    assert dups > 0 and plain.count.tolist()[2:] == [min(N, V), 1]


@pytest.mark.parametrize("N", [1, 2, 5, 16])
def test_weights_kernel_matches_its_numpy_statement(N):
    """B = 7, one special utterance each: rows beyond count, a hypothesis over Lh, a +inf hypothesis nll, no valid entry, all nll
    equal, nll spread over 300 nats (finite, no NaN), a +inf target nll.  p, r, coef, rbar, terms within 1e-6 relative of the fp64
    statement rounded to fp32 (the outputs' format; below the smallest normal fp32 a value has no such relative precision, hence
    atol = 1.2e-38), utt_scale too; two runs bit-equal."""
    from policy_gradient_asr_amd import hipops
    B, Lh, lam, inv_gb = 7, 20, 0.8, 1.0 / 11
    rng = np.random.default_rng(100 + N)
    hyp_nll = rng.uniform(20.0, 26.0, size=(N, B)).astype(np.float32)
    hyp_len = rng.integers(0, Lh + 1, size=(N, B)).astype(np.int32)
    count = np.full(B, N, dtype=np.int32)
    dist = rng.integers(0, 9, size=(N, B)).astype(np.int32)
    tg_len = np.array([5, 1, 0, 7, 3, 9, 4], dtype=np.int32)
    risk_len = np.array([2, 1, 0, 7, 1, 3, 4], dtype=np.int32)
    nll = rng.uniform(5.0, 50.0, size=B).astype(np.float32)
    count[0] = (N + 1) // 2
    hyp_len[0, 1] = Lh + 1
    hyp_nll[N - 1, 2] = np.inf
    count[3] = 0
    hyp_nll[:, 4] = 33.25
    hyp_nll[:, 5] = np.linspace(10.0, 310.0, N, dtype=np.float32)
    nll[6] = np.inf
    want = MR.weights_ref(dist, risk_len, tg_len, hyp_nll, hyp_len, count, nll, Lh, float(np.float32(lam)), float(np.float32(inv_gb)))
    d = lambda a: torch.from_numpy(a).to(DEV)
    args = (d(dist), d(risk_len), d(tg_len), d(hyp_nll), d(hyp_len), d(count), d(nll), Lh, lam, inv_gb)
    got = [t.clone() for t in hipops.mwer_weights(*args)]
    again = hipops.mwer_weights(*args)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    p, r, coef, utt_scale, rbar, terms = (t.cpu().numpy() for t in got)
    for name, g, w in (("p", p, want.p), ("r", r, want.r), ("coef", coef, want.coef), ("utt_scale", utt_scale, want.utt_scale),
                       ("rbar", rbar, want.rbar), ("terms", terms, want.terms)):
        assert g.dtype == np.float32 and not np.isnan(g).any(), name
        with np.errstate(over="ignore"):
            w32 = w.astype(np.float32)
        with np.errstate(invalid="ignore"):
            print(f"weights N={N} {name}: max rel err {np.max(np.abs(g - w32)[np.isfinite(w32)] / np.maximum(np.abs(w32[np.isfinite(w32)]), 1e-30)):.2e}")
        np.testing.assert_allclose(g, w32, rtol=1e-6, atol=1.2e-38, err_msg=name)
    valid = want.valid
    assert (p[~valid] == 0).all() and (coef[~valid] == 0).all() and not p[:, 3].any() and rbar[3] == 0 and terms[6] == np.inf
    assert np.isfinite(p[:, 5]).all() and np.isfinite(coef[:, 5]).all() and (N == 1 or p[0, 5] > 0.9)
    assert np.allclose(p[:, 4][valid[:, 4]], 1.0 / N, rtol=1e-6)
    assert np.abs(coef.sum(axis=0)).max() <= 1e-6 * np.abs(coef).max() + 1e-12


# ---- the loss against the fp64 reference, on the device's own lists ----
LOSS_CASES = [(60, 4, 29, 16, 16, 0), (40, 4, 6, 8, 4, 0), (9, 3, 5, 4, 2, 0), (40, 4, 6, 8, 4, 5)]      # T, B, V, beam, N, blank


def _loss_case(T, B, V, blank, seed, scale=2.0):
    """pg_harness.lattice_case's logits (randn * 2, fp64 -> fp32) with lengths of this module's: in_len from T down to a single frame
    (B = 4), targets that avoid the blank."""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(T, B, V, generator=g, dtype=torch.float64) * scale).float()
    in_len = torch.tensor([T, T - T // 4, T // 2, 1][:B] if B == 4 else [T, T - 2, T // 2][:B], dtype=torch.int32)
    tg_len = torch.tensor([max(1, min(6, T // 3)), max(1, min(5, T // 4)), max(1, min(4, T // 5)), 1][:B], dtype=torch.int32)
    syms = torch.tensor([s for s in range(V) if s != blank])
    targets = syms[torch.randint(0, V - 1, (B, int(tg_len.max())), generator=g)].to(torch.int32)
    for b in range(B):
        targets[b, int(tg_len[b]):] = 0
    return logits, targets, in_len, tg_len


def _device_loss(logits, targets, in_len, tg_len, **kw):
    from policy_gradient_asr_amd.mwer import MWERLossFn, mwer_ctc_loss
    lg = logits.to(DEV).requires_grad_(True)
    out = mwer_ctc_loss(lg, in_len.to(DEV), targets.to(DEV), tg_len.to(DEV), **kw)
    out[0].backward()
    torch.cuda.synchronize()
    nb = MWERLossFn.last_nbest
    return (float(out[0]), lg.grad.cpu().double().numpy(), [t.cpu().numpy() for t in nb], MWERLossFn.last_posterior.cpu().numpy(),
            [t.detach().cpu().numpy() for t in out[1:]])


def _reference(logits, targets, in_len, tg_len, lists, Lh, lam, gb, blank=0, delimiter=None):
    tokens, lengths, _, count = lists
    dist, risk_len = MR.risks(targets.numpy(), tg_len.numpy(), tokens, lengths, delimiter)
    return MR.mwer_closed_form(logits.double().numpy(), in_len.numpy(), targets.numpy(), tg_len.numpy(), tokens, lengths, count, Lh,
                               lam, gb, dist, risk_len, blank=blank)


def _compare(label, loss, grad, ref, post, stats):
    lerr = abs(loss - ref.loss) / abs(ref.loss)
    gerr = np.abs(grad - ref.grad).max() / np.abs(ref.grad).max()
    perr = np.abs(post - ref.w.p).max()
    print(f"{label}: loss {loss!r} reference {ref.loss!r} rel err {lerr:.2e}; d(logits) max-norm rel err {gerr:.2e}; posterior abs err {perr:.2e}; "
          f"top posteriors {np.round(ref.w.p.max(axis=0), 3).tolist()}")
    assert lerr <= 1e-5 and gerr <= 1e-5
    nll, expected, top = stats
    np.testing.assert_allclose(nll, ref.nll, rtol=1e-5)
    np.testing.assert_allclose(expected, -ref.w.rbar, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(top, -ref.w.r[0], rtol=1e-6)
    np.testing.assert_allclose(post, ref.w.p, rtol=0, atol=1e-4)


@pytest.mark.parametrize("T,B,V,beam,N,blank", LOSS_CASES)
def test_loss_and_gradient_match_the_fp64_reference(T, B, V, beam, N, blank):
    """mwer_ctc_loss against mwer_ref's closed form on the lists the device itself returned: loss 1e-5 relative, d(logits) 1e-5
    max-norm relative (the bounds of tests/test_seq_score_gpu.py for the same lattices).  Not vacuous: every utterance with at least two
    frames has count >= 2, coefficients of both signs occur, no utterance's top posterior exceeds 0.9."""
    logits, targets, in_len, tg_len = _loss_case(T, B, V, blank, seed=200 + T + V + blank)
    loss, grad, lists, post, stats = _device_loss(logits, targets, in_len, tg_len, lam=1.0, beam=beam, nbest=N, blank=blank)
    tokens, lengths, score, count = lists
    assert tokens.shape == (N, B, T) and post.shape == (N, B)
    ref = _reference(logits, targets, in_len, tg_len, lists, min(T, 1023), 1.0, B, blank)
    assert all(count[b] >= 2 for b in range(B) if in_len[b] >= 2) or N == 1
    assert (ref.w.coef > 0).any() and (ref.w.coef < 0).any()
    assert ref.w.p.max() <= 0.9
    inside = np.arange(T)[None, None, :] < lengths[:, :, None]
    assert not (tokens[inside] == blank).any() and not tokens[~inside].any()      # raw prefixes hold no blank; zero tails
    _compare(f"mwer loss T={T} B={B} V={V} beam={beam} N={N} blank={blank}", loss, grad, ref, post, stats)
    for b in range(B):
        assert not grad[int(in_len[b]):, b].any()


def test_a_capped_hypothesis_leaves_the_posterior():
    """max_hyp_len below the longest hypothesis: those entries have posterior 0 and add nothing to the gradient, the rest is
    renormalised (one utterance loses part of its list, another may lose all of it), and loss and gradient match the reference to the
    same bounds.  Between one entry and half of them are excluded."""
    T, B, V, beam, N = 40, 4, 6, 8, 4
    logits, targets, in_len, tg_len = _loss_case(T, B, V, 0, seed=246)
    _, _, lists, post_full, _ = _device_loss(logits, targets, in_len, tg_len, beam=beam, nbest=N)
    lengths, count = lists[1], lists[3]
    listed = np.arange(N)[:, None] < count[None, :]
    # the largest cap under which some utterance loses part of its list (so that the rest of it is renormalised)
    caps = [c for c in range(int(lengths.max()) - 1, -1, -1)
            if any(0 < ((lengths[:, b] > c) & listed[:, b]).sum() < listed[:, b].sum() for b in range(B))]
    assert caps
    cap = caps[0]
    over = (lengths > cap) & listed
    assert 1 <= over.sum() <= listed.sum() // 2, (over.sum(), listed.sum())
    loss, grad, lists_c, post, stats = _device_loss(logits, targets, in_len, tg_len, beam=beam, nbest=N, max_hyp_len=cap)
    assert all(np.array_equal(a, b) for a, b in zip(lists, lists_c))          # the cap does not touch the search
    assert (post[over] == 0).all() and (post_full[over] > 0).all()
    keep = np.where(over, 0.0, post_full)
    np.testing.assert_allclose(post, keep / np.maximum(keep.sum(axis=0, keepdims=True), 1e-30), rtol=1e-5, atol=1e-7)
    ref = _reference(logits, targets, in_len, tg_len, lists_c, cap, 1.0, B)
    assert (ref.w.coef[over] == 0).all()
    _compare(f"mwer cap {cap}", loss, grad, ref, post, stats)


def test_identities():
    """lam = 0 gives the loss and gradient of pg_ctc_loss(lam=0); nbest = 1 gives its gradient, and its loss plus the constant
    lam / Bg * sum_b r[0,b] that the objective's definition puts there (the one-entry posterior is 1: the risk term has no gradient);
    two half-batches with global_batch = B give the whole batch's loss and gradient.  All within 1e-6."""
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    from policy_gradient_asr_amd.mwer import mwer_ctc_loss
    T, B, V, beam = 40, 4, 6, 8
    logits, targets, in_len, tg_len = _loss_case(T, B, V, 0, seed=77)
    lg, il, tg, tl = logits.to(DEV), in_len.to(DEV), targets.to(DEV), tg_len.to(DEV)
    base = lg.clone().requires_grad_(True)
    l0, nll0, _, _ = pg_ctc_loss(base, il, tg, tl, lam=0.0)
    l0.backward()
    gmax = float(base.grad.abs().max())

    def run(sl=slice(None), **kw):
        x = lg[:, sl].contiguous().requires_grad_(True)
        out = mwer_ctc_loss(x, il[sl].contiguous(), tg[sl].contiguous(), tl[sl].contiguous(), beam=beam, **kw)
        out[0].backward()
        return float(out[0]), x.grad, out

    l_a, g_a, _ = run(lam=0.0, nbest=4)
    assert abs(l_a - float(l0)) <= 1e-6 * abs(float(l0)) and float((g_a - base.grad).abs().max()) <= 1e-6 * gmax
    l_b, g_b, out = run(lam=1.0, nbest=1)
    const = float((-out[3]).double().sum()) / B                              # lam / Bg * sum_b r[0,b]
    assert const > 0 and abs((l_b - const) - float(l0)) <= 1e-6 * abs(float(l0))
    assert float((g_b - base.grad).abs().max()) <= 1e-6 * gmax
    assert torch.equal(out[2], out[3])                                       # one entry: the expected reward is the top one's
    l_w, g_w, _ = run(lam=1.0, nbest=4)
    parts = [run(slice(2 * h, 2 * h + 2), lam=1.0, nbest=4, global_batch=B) for h in range(2)]
    assert abs(parts[0][0] + parts[1][0] - l_w) <= 1e-6 * abs(l_w)
    assert float((torch.cat([p[1] for p in parts], dim=1) - g_w).abs().max()) <= 1e-6 * float(g_w.abs().max())
    assert float((g_w - base.grad).abs().max()) > 1e-3 * gmax               # .. and the risk term is there


# ---- the trainer ----
@pytest.mark.parametrize("word", [False, True], ids=["char", "word"])
def test_trainer_step_matches_the_fp64_oracle(word):
    """MWERTrainer.compute_gradients on pg_harness.step_batch / oracle_model against model_ref forward, mwer_ref on the device's lists
    and backprop: loss < 1e-5, every parameter gradient < 1e-4 (trainer_step_vs_oracle's bars)."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.mwer import MWERLossFn, MWERTrainer
    seed, N, beam = 61, 4, 16
    batch, lens, tlens = H.step_batch(4, word, seed)
    p, pr, m = H.oracle_model(80, 29, seed + 1)
    tr = MWERTrainer(m, lam=1.0, seed=3, precision="f32", beam_size=beam, nbest=N, risk_unit="word" if word else "char",
                     word_delimiter=H.D if word else None)
    loss = tr.compute_gradients(*(t.to(DEV) for t in batch))
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    B = len(lens)
    nb = MWERLossFn.last_nbest
    tokens, lengths, count = nb.tokens[:, :B].cpu().numpy(), nb.lengths[:, :B].cpu().numpy(), nb.count[:B].cpu().numpy()
    x, targets, fmask, _ = batch
    logits_ref = model_ref.head_logits_torch(pr, model_ref.encoder_forward_torch(pr, x.double(), fmask, packed=True))
    T = logits_ref.shape[0]
    dist, risk_len = MR.risks(targets.numpy(), np.array(tlens), tokens, lengths, H.D if word else None)
    ref = MR.mwer_closed_form(logits_ref.detach().numpy(), np.array(lens), targets.numpy(), np.array(tlens), tokens, lengths, count,
                              min(T, 1023), 1.0, B, dist, risk_len)
    assert (count >= 2).all() and (ref.w.coef != 0).any()
    logits_ref.backward(torch.from_numpy(ref.grad))
    errs = H.param_errs(m, {k: v.grad for k, v in pr.items()})
    lerr = abs(float(loss) - ref.loss) / abs(ref.loss)
    worst = max(errs, key=errs.get)
    print(f"mwer step {'word' if word else 'char'}: loss {float(loss)!r} oracle {ref.loss!r} rel err {lerr:.2e}; worst parameter gradient {worst} {errs[worst]:.2e}; "
          f"top posteriors {np.round(ref.w.p.max(axis=0), 3).tolist()}")
    assert lerr < 1e-5
    assert errs[worst] < 1e-4, (worst, errs[worst])
    nll, expected, top = tr.last_stats
    assert tr.last_sample_rewards.shape == (N, B) and tr.last_posterior.shape == (N, B) and nll.shape == (B,)
    np.testing.assert_allclose(tr.last_sample_rewards.cpu().numpy(), -ref.w.r, rtol=1e-6)
    np.testing.assert_allclose(expected.cpu().numpy(), -ref.w.rbar, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(top.cpu().numpy(), -ref.w.r[0], rtol=1e-6)


def _mwer_trainer(**kw):
    from policy_gradient_asr_amd.model import Seq2Seq, weights
    from policy_gradient_asr_amd.mwer import MWERTrainer
    torch.manual_seed(0)
    m = Seq2Seq(H.ACC_V, n_feats=H.ACC_F); m.apply(weights); m = m.to(DEV).eval()
    return MWERTrainer(m, lam=1.0, precision="f32", **kw)


def test_accumulated_step_is_the_whole_batch_and_clipping_works():
    """step_accumulated over two micro-batches padded to one T against step on the whole batch, identically built trainers: the same
    lists' rewards, loss within 1e-6 and gflat within 1e-5 (the f32 bounds of tests/test_grad_accum_gpu.py for this identity); then
    max_grad_norm clips the accumulated gradient once and clip_counts() reports it."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.train_step import FLAG_PAD
    batch, _ = H._batch(32)
    mbs = [H._rows(batch, p) for p in H._slices((16, 16))]
    whole, acc = _mwer_trainer(lr=1e-3, nbest=4, beam_size=8), _mwer_trainer(lr=1e-3, nbest=4, beam_size=8)
    loss_w = float(whole.step(*batch))
    loss_a = float(acc.step_accumulated(mbs))
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    gerr = H.rel_err(acc.gflat.cpu(), whole.gflat.cpu())
    lerr = abs(loss_a - loss_w) / abs(loss_w)
    print(f"mwer accumulation: gflat {gerr:.2e} loss {lerr:.2e}")
    assert acc.last_sample_rewards.shape == (4, 32) and all(s_.shape == (32,) for s_ in acc.last_stats)
    assert torch.equal(acc.last_sample_rewards, whole.last_sample_rewards)
    assert H.rel_err(acc.last_stats[0].cpu(), whole.last_stats[0].cpu()) < 1e-6
    assert lerr <= 1e-6 and gerr < 1e-5 and float(acc.gflat.abs().max()) > 0
    assert acc.nstep == whole.nstep == 1 and acc.applied_steps() == whole.applied_steps() == 1
    tr = _mwer_trainer(lr=1e-3, nbest=4, beam_size=8, max_grad_norm=0.05)
    tr.step_accumulated(mbs)
    torch.cuda.synchronize()
    want = np.float32(tr.gflat[FLAG_PAD:].double().norm().item())
    got = np.float32(tr.last_grad_norm.item())
    assert abs(got - want) <= 4 * np.spacing(want)
    assert want > 0.05 and tr.clip_counts() == (1, 0) and tr.applied_steps() == 1


def test_train_driver_with_the_mwer_objective(tmp_path):
    """model.train(objective="mwer") on the tiny corpus for one epoch, word risk from alphabet.txt's " ": a finite loss, the checkpoint."""
    from policy_gradient_asr_amd.model import train
    corpus, out, ds = H.tiny_corpus(tmp_path)
    losses, _ = train(str(corpus), str(out), 1, 16, 0, train_dataset=ds, n_feats=20, lam=1.0, lr=1e-3, log_every=1, objective="mwer",
                      mwer_nbest=4, mwer_beam=8, reward_unit="word")
    assert len(losses) == 1 and np.isfinite(losses[0]) and losses[0] > 0
    assert os.path.exists(out / "checkpoint_last.pth") and os.path.exists(out / "model_last.pth")
    with pytest.raises(ValueError):
        train(str(corpus), str(out), 1, 16, 0, train_dataset=ds, n_feats=20, objective="mwer", num_samples=2)
