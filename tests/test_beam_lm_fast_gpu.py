"""Language-model fusion in the single-wave beam search (csrc/beam.hip, sb::beam_small_kernel<SPL, NBEST, LM = true>; flags bit 4)
on the device: 1-best and N-best against the plain-Python fused search of tests/beam_lm_ref.py / tests/nbest_ref.py token for token
(the cases' margins are asserted on the CPU), against the workgroup LM kernel, zero weights against the search without an LM bit for
bit, the order-5 table at the size limit, the constructed flip, the dispatch without the bit, MWER over LM-fused lists against the
fp64 closed form, and ``predict(lm_fast=True)``.  Outputs are written into garbage-filled buffers, so a missed store shows."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as R  # noqa: E402
import beam_lm_fast_ref as F  # noqa: E402
import mwer_ref as MR  # noqa: E402
import nbest_ref as NR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GARBAGE = 0x5A5A5A5A
FAST, FAST_LM = 8, 16
REL = 1e-6          # the bound test_beam_lm_gpu.test_fast_path_matches_the_fused_reference holds the fp32 workgroup kernel to


def _lm(table, order, blank=0):
    from policy_gradient_asr_amd.lm import CharNgramLM
    return CharNgramLM(table, order, blank=blank)


def _ids(c):
    return "T%d-V%d-K%d-n%d-b%d-s%d" % (c[0], c[1], c[2], c[3], c[4], c[7])


def _raw_1best(lp, lens, beam, blank, lm, alpha, beta, flags):
    """pgasr_ctc_beam_search_lm into a garbage-filled length and score (tokens zero-filled, as the entry point asks)."""
    from policy_gradient_asr_amd import _lib, hipops
    lib = _lib.load()
    T, B, V = lp.shape
    tokens = torch.zeros(B, T, dtype=torch.int32, device=DEV)
    tl = torch.full((B,), GARBAGE, dtype=torch.int32, device=DEV)
    score = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
    ws = hipops._workspace(lib.pgasr_beam_workspace_bytes(T, B, V, beam), lp.device, "beam")
    table = lm.device_table(lp.device) if lm is not None else None
    st = lib.pgasr_ctc_beam_search_lm(lp.data_ptr(), 0, lp.stride(0), lp.stride(1), lens.data_ptr(), T, B, V, beam, blank, flags,
                                      tokens.data_ptr(), tl.data_ptr(), score.data_ptr(), ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream().cuda_stream, None if table is None else table.data_ptr(),
                                      0 if lm is None else lm.order, alpha, beta)
    _lib.check(st, "pgasr_ctc_beam_search_lm")
    return tokens, tl, score


def _raw_nbest(lp, lens, beam, N, blank, lm, alpha, beta, flags):
    """pgasr_ctc_beam_search_nbest into GARBAGE-FILLED outputs."""
    from policy_gradient_asr_amd import _lib, hipops
    lib = _lib.load()
    T, B, V = lp.shape
    tokens = torch.full((N, B, T), GARBAGE, dtype=torch.int32, device=DEV)
    tl = torch.full((N, B), GARBAGE, dtype=torch.int32, device=DEV)
    score = torch.full((N, B), float("nan"), dtype=torch.float64, device=DEV)
    count = torch.full((B,), GARBAGE, dtype=torch.int32, device=DEV)
    ws = hipops._workspace(lib.pgasr_beam_workspace_bytes(T, B, V, beam), lp.device, "beam")
    table = lm.device_table(lp.device) if lm is not None else None
    st = lib.pgasr_ctc_beam_search_nbest(lp.data_ptr(), 0, lp.stride(0), lp.stride(1), lens.data_ptr(), T, B, V, beam, blank, flags,
                                         N, tokens.data_ptr(), T, tl.data_ptr(), score.data_ptr(), count.data_ptr(),
                                         ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream,
                                         None if table is None else table.data_ptr(), 0 if lm is None else lm.order, alpha, beta)
    _lib.check(st, "pgasr_ctc_beam_search_nbest")
    return hipops.CTCNBest(tokens, tl, score, count)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", F.INSIDE, ids=_ids)
def test_1_best_matches_the_helper_and_the_workgroup_kernel(case):
    """ctc_beam_search(lm=, fast_lm=True) on the shared fp32 cases with beam <= 16: the helper's tokens, its score to 1e-6 relative,
    the workgroup LM kernel's tokens; collapse=True is the plain output with adjacent duplicates removed; the Python call is the raw
    call with flags bit 4."""
    from policy_gradient_asr_amd import hipops
    T, V, beam, order, blank, alpha, beta, seed = case
    lp_h, lens_h, table = R.fast_case_inputs(case)
    lm = _lm(table, order, blank)
    lp, lens = torch.from_numpy(lp_h).to(DEV), torch.from_numpy(lens_h).to(DEV)
    tok, tl, score = _raw_1best(lp, lens, beam, blank, lm, alpha, beta, FAST_LM)
    via = hipops.ctc_beam_search(lp, lens, beam=beam, blank=blank, lm=lm, lm_alpha=alpha, lm_beta=beta, fast_lm=True)
    assert _same(via, (tok, tl, score))
    wg = hipops.ctc_beam_search(lp, lens, beam=beam, blank=blank, lm=lm, lm_alpha=alpha, lm_beta=beta)
    ctok, ctl, cscore = hipops.ctc_beam_search(lp, lens, beam=beam, blank=blank, collapse=True, lm=lm, lm_alpha=alpha, lm_beta=beta,
                                               fast_lm=True)
    assert torch.equal(score, cscore)
    ref = NR.fast_reference(case, True)
    for b in range(R.FAST_B):
        n = int(lens_h[b])
        hyps, gap = ref[b]
        want, wscore = hyps[0]
        got = list(tok[b, :tl[b]].cpu().numpy())
        print(f"single-wave LM {case} b={b} n={n}: score {float(score[b])!r} reference {wscore!r} workgroup {float(wg[2][b])!r} gap {gap:.3e}")
        assert got == list(want), (b, n)
        assert float(score[b]) == pytest.approx(wscore, rel=REL), (b, n)
        assert got == list(wg[0][b, :wg[1][b]].cpu().numpy()), (b, n)
        assert int(tok[b, tl[b]:].abs().sum()) == 0
        dedup = [x for i, x in enumerate(got) if i == 0 or x != got[i - 1]]
        assert list(ctok[b, :ctl[b]].cpu().numpy()) == dedup and int(ctok[b, ctl[b]:].abs().sum()) == 0
        if n == 0:
            assert int(tl[b]) == 0 and float(score[b]) == 0.0 and np.signbit(float(score[b]))


@pytest.mark.parametrize("case", F.OUTSIDE, ids=_ids)
def test_outside_the_limits_the_bit_changes_nothing(case):
    """beam 100: the call with fast_lm=True equals the call without it, bit for bit -- 1-best and list."""
    from policy_gradient_asr_amd import hipops
    T, V, beam, order, blank, alpha, beta, seed = case
    lp_h, lens_h, table = R.fast_case_inputs(case)
    lm = _lm(table, order, blank)
    lp, lens = torch.from_numpy(lp_h).to(DEV), torch.from_numpy(lens_h).to(DEV)
    assert not hipops.beam_lm_single_wave_ok(T, V, beam, False, order)
    kw = dict(beam=beam, blank=blank, lm=lm, lm_alpha=alpha, lm_beta=beta)
    assert _same(hipops.ctc_beam_search(lp, lens, fast_lm=True, **kw), hipops.ctc_beam_search(lp, lens, **kw))
    N = NR.list_size(beam)
    assert _same(_raw_nbest(lp, lens, beam, N, blank, lm, alpha, beta, FAST | FAST_LM), hipops.ctc_beam_search_nbest(lp, lens, nbest=N, **kw))


@pytest.mark.parametrize("case", F.INSIDE, ids=_ids)
def test_nbest_matches_the_helper(case):
    """The list at N = list_size(beam): every rank token for token, scores 1e-6 relative, rows beyond count and token tails as
    documented; row 0 is the 1-best fast_lm call bit for bit, with and without collapse; a shorter list is the bitwise prefix."""
    from policy_gradient_asr_amd import hipops
    T, V, beam, order, blank, alpha, beta, seed = case
    lp_h, lens_h, table = R.fast_case_inputs(case)
    lm = _lm(table, order, blank)
    lp, lens = torch.from_numpy(lp_h).to(DEV), torch.from_numpy(lens_h).to(DEV)
    N = NR.list_size(beam)
    nb = _raw_nbest(lp, lens, beam, N, blank, lm, alpha, beta, FAST_LM)
    ref = NR.fast_reference(case, True)
    for b in range(R.FAST_B):
        hyps, gap = ref[b]
        tok, ln, sc = nb.tokens[:, b].cpu().numpy(), nb.lengths[:, b].cpu().numpy(), nb.score[:, b].cpu().numpy()
        print(f"single-wave LM list {case} b={b} n={int(lens_h[b])}: {len(hyps)} ranks, gap {gap:.3e}, score[0] {sc[0]!r} reference {hyps[0][1]!r}")
        assert gap >= R.GAP_MIN
        assert int(nb.count[b]) == len(hyps)
        for r, (want, wscore) in enumerate(hyps):
            assert list(tok[r, :ln[r]]) == list(want), (b, r)
            assert sc[r] == pytest.approx(wscore, rel=REL), (b, r)
            assert not tok[r, ln[r]:].any()
        for r in range(len(hyps), N):
            assert ln[r] == 0 and sc[r] == np.inf and not tok[r].any(), (b, r)
        if lens_h[b] == 0:
            assert int(nb.count[b]) == 1 and ln[0] == 0 and sc[0] == 0.0 and np.signbit(sc[0])
    kw = dict(beam=beam, blank=blank, lm=lm, lm_alpha=alpha, lm_beta=beta)
    assert _same(hipops.ctc_beam_search_nbest(lp, lens, nbest=N, fast=True, fast_lm=True, **kw), nb)
    for flag in (False, True):
        full = nb if not flag else _raw_nbest(lp, lens, beam, N, blank, lm, alpha, beta, FAST_LM | 1)
        one = hipops.ctc_beam_search(lp, lens, collapse=flag, fast_lm=True, **kw)
        assert torch.equal(full.tokens[0], one[0]) and torch.equal(full.lengths[0], one[1]) and torch.equal(full.score[0], one[2])
        for n in sorted({1, min(3, N)}):
            short = _raw_nbest(lp, lens, beam, n, blank, lm, alpha, beta, FAST_LM | int(flag))
            assert torch.equal(short.tokens, full.tokens[:n]) and torch.equal(short.lengths, full.lengths[:n])
            assert torch.equal(short.score, full.score[:n]) and torch.equal(short.count, full.count.clamp(max=n))


@pytest.mark.parametrize("V", [29, 64])
def test_zero_weights_are_the_single_wave_search_without_lm_bit_for_bit(V):
    """alpha = beta = 0 with a table: x + 0.0 == x, so tokens, lengths and scores equal the single-wave kernel's without an LM; and the
    weights do reach the kernel."""
    from policy_gradient_asr_amd import hipops
    T, B, beam, order = 120, 4, 16, 3 if V == 29 else 2
    rng = np.random.default_rng(T + V)
    lp = torch.from_numpy(R.log_softmax32(rng.normal(size=(T, B, V)) * 2.0)).to(DEV)
    lens = torch.tensor([T, T - 9, 1, 0], dtype=torch.int32, device=DEV)
    lm = _lm(R.random_table(V, order, 0, seed=3), order)
    a = hipops.ctc_beam_search(lp, lens, beam=beam)                                   # the single-wave kernel, no LM
    z = _raw_1best(lp, lens, beam, 0, lm, 0.0, 0.0, FAST_LM)
    assert _same(a, z)
    w = hipops.ctc_beam_search(lp, lens, beam=beam, lm=lm, lm_alpha=0.5, lm_beta=0.5, fast_lm=True)
    assert not torch.equal(a[2], w[2])
    la = hipops.ctc_beam_search_nbest(lp, lens, beam=beam, nbest=beam, fast=True)
    lz = _raw_nbest(lp, lens, beam, beam, 0, lm, 0.0, 0.0, FAST_LM)
    assert _same(la, lz)


def test_order_5_table_at_the_size_limit():
    """29^5 entries, just under 2^25: the context index arithmetic at its largest.  Tokens equal the helper's (margins asserted on
    the CPU), scores to 1e-6 relative."""
    from policy_gradient_asr_amd import hipops
    T, V, beam, order, blank, alpha, beta, seed = F.ORDER5_CASE
    lp_h, lens_h, table = F.order5_inputs()
    lm = _lm(table, order, blank)
    lp, lens = torch.from_numpy(lp_h).to(DEV), torch.from_numpy(lens_h).to(DEV)
    assert hipops.beam_lm_single_wave_ok(T, V, beam, False, order)
    tok, tl, score = _raw_1best(lp, lens, beam, blank, lm, alpha, beta, FAST_LM)
    for b, (want, wscore, gap) in enumerate(F.order5_reference()):
        print(f"order 5 b={b} n={int(lens_h[b])}: score {float(score[b])!r} reference {wscore!r} gap {gap:.3e}")
        assert list(tok[b, :tl[b]].cpu().numpy()) == list(want), b
        assert float(score[b]) == pytest.approx(wscore, rel=REL), b


def test_constructed_flip():
    """The input of test_beam_lm_gpu.test_constructed_flip through fast_lm=True: the hypothesis changes with alpha > 0 and not with
    alpha = 0, as the helper says."""
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    T, V = 9, 3
    probs = np.zeros((T, V))
    probs[:] = [0.9, 0.05, 0.05]
    probs[2] = [0.1, 0.46, 0.44]
    table = np.array([0.0, np.log(0.02), np.log(0.98)], dtype=np.float32)
    dec = CTCDecoder(["-", "a", "b"], lm=_lm(table, 1), lm_alpha=0.0, lm_beta=0.0, fast_lm=True)
    assert R.fused_prefix_beam_search(probs, table, 1, 0.0, 0.0, beam_size=8)[0] == (1,)
    assert R.fused_prefix_beam_search(probs, table, 1, 1.0, 0.0, beam_size=8)[0] == (2,)
    lp = torch.from_numpy(np.log(probs)).float().view(T, 1, V).to(DEV)
    t0, l0, _ = dec.decode_batch(lp, None, beam_size=8)
    t1, l1, _ = dec.decode_batch(lp, None, beam_size=8, lm_alpha=1.0)
    assert t0[0, :l0[0]].tolist() == [1] and t1[0, :l1[0]].tolist() == [2]
    # an order-2 LM that only dislikes "a" after "a": the flip happens at the second character
    probs2 = probs.copy(); probs2[6] = probs[2]
    t2 = np.zeros((3, 3), dtype=np.float32); t2[:, 1:] = np.log(0.5); t2[1, 1], t2[1, 2] = np.log(0.02), np.log(0.98)
    d2 = CTCDecoder(["-", "a", "b"], lm=_lm(t2, 2), lm_alpha=1.0)
    lp2 = torch.from_numpy(np.log(probs2)).float().view(T, 1, V).to(DEV)
    a, la, _ = d2.decode_batch(lp2, None, beam_size=8, lm_alpha=0.0, fast_lm=True)
    b, lb, _ = d2.decode_batch(lp2, None, beam_size=8, fast_lm=True)
    assert a[0, :la[0]].tolist() == [1, 1]
    assert tuple(b[0, :lb[0]].tolist()) == (1, 2) == R.fused_prefix_beam_search(probs2, t2, 2, 1.0, 0.0, beam_size=8)[0]


def test_bit_4_alone_changes_nothing():
    """Bit 4 without a table is the acoustic dispatch; bit 3 with a table but without bit 4 stays on the workgroup kernel."""
    from policy_gradient_asr_amd import hipops
    T, B, V, beam = 120, 4, 29, 16
    rng = np.random.default_rng(21)
    lp = torch.from_numpy(R.log_softmax32(rng.normal(size=(T, B, V)) * 2.0)).to(DEV)
    lens = torch.tensor([T, 77, 1, 0], dtype=torch.int32, device=DEV)
    lm = _lm(R.random_table(V, 3, 0, seed=5), 3)
    for coll in (False, True):
        assert _same(_raw_1best(lp, lens, beam, 0, None, 0.0, 0.0, FAST_LM | int(coll)), hipops.ctc_beam_search(lp, lens, beam=beam, collapse=coll))
        assert _same(_raw_1best(lp, lens, beam, 0, None, 0.0, 0.0, FAST_LM | 2 | int(coll)),
                     hipops.ctc_beam_search(lp, lens, beam=beam, collapse=coll, generic=True))
    assert _same(_raw_nbest(lp, lens, beam, 8, 0, None, 0.0, 0.0, FAST_LM | FAST), hipops.ctc_beam_search_nbest(lp, lens, beam=beam, nbest=8, fast=True))
    assert _same(_raw_nbest(lp, lens, beam, 8, 0, None, 0.0, 0.0, FAST_LM), hipops.ctc_beam_search_nbest(lp, lens, beam=beam, nbest=8))
    slow = hipops.ctc_beam_search_nbest(lp, lens, beam=beam, nbest=8, lm=lm, lm_alpha=0.6, lm_beta=0.8)
    assert _same(_raw_nbest(lp, lens, beam, 8, 0, lm, 0.6, 0.8, FAST), slow)
    assert _same(hipops.ctc_beam_search_nbest(lp, lens, beam=beam, nbest=8, lm=lm, lm_alpha=0.6, lm_beta=0.8, fast=True), slow)
    one = hipops.ctc_beam_search(lp, lens, beam=beam, lm=lm, lm_alpha=0.6, lm_beta=0.8)
    assert torch.equal(slow.tokens[0], one[0]) and torch.equal(slow.score[0], one[2])


def test_mwer_with_an_lm():
    """mwer_ctc_loss_lm on (T, B, V, beam, N) = (40, 4, 6, 8, 4) with an order-2 table: the list is ctc_beam_search_nbest(lm=, fast=True,
    fast_lm=True) bit for bit and differs from the acoustic list; loss and d(logits) match mwer_ref's closed form on that list to 1e-5
    (the bounds of test_mwer_gpu.test_loss_and_gradient_match_the_fp64_reference); lm=None is mwer_ctc_loss bit for bit."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.mwer import MWERLossFn, mwer_ctc_loss, mwer_ctc_loss_lm
    T, B, V, beam, N, blank = F.MWER_SHAPE
    order, alpha, beta, _ = F.MWER_LM
    logits, targets, in_len, tg_len = F.mwer_case()
    lm = _lm(F.mwer_table(), order, blank)

    def run(fn, *a, **kw):
        lg = logits.to(DEV).requires_grad_(True)
        out = fn(lg, in_len.to(DEV), targets.to(DEV), tg_len.to(DEV), *a, beam=beam, nbest=N, blank=blank, **kw)
        out[0].backward()
        torch.cuda.synchronize()
        return out[0].detach().clone(), lg.grad.clone(), [t.clone() for t in MWERLossFn.last_nbest], MWERLossFn.last_posterior.clone(), out

    loss, grad, lists, post, out = run(mwer_ctc_loss_lm, lm, alpha, beta)
    lp = hipops.log_softmax_rows(logits.to(DEV).contiguous())
    direct = hipops.ctc_beam_search_nbest(lp, in_len.to(DEV), beam=beam, nbest=N, blank=blank, lm=lm, lm_alpha=alpha, lm_beta=beta,
                                          fast=True, fast_lm=True)
    assert _same(lists, direct)
    base_loss, base_grad, base_lists, _, _ = run(mwer_ctc_loss)
    differs = [not torch.equal(lists[0][:, b], base_lists[0][:, b]) for b in range(B)]
    assert any(differs), differs
    tokens, lengths, _, count = (t.cpu().numpy() for t in lists)
    dist, risk_len = MR.risks(targets.numpy(), tg_len.numpy(), tokens, lengths, None)
    ref = MR.mwer_closed_form(logits.double().numpy(), in_len.numpy(), targets.numpy(), tg_len.numpy(), tokens, lengths, count,
                              min(T, 1023), 1.0, B, dist, risk_len, blank=blank)
    lerr = abs(float(loss) - ref.loss) / abs(ref.loss)
    gerr = np.abs(grad.cpu().double().numpy() - ref.grad).max() / np.abs(ref.grad).max()
    print(f"mwer with LM: loss {float(loss)!r} reference {ref.loss!r} rel err {lerr:.2e}; d(logits) max-norm rel err {gerr:.2e}; lists differ {differs}")
    assert lerr <= 1e-5 and gerr <= 1e-5
    np.testing.assert_allclose(post.cpu().numpy(), ref.w.p, rtol=0, atol=1e-4)
    np.testing.assert_allclose(out[1].cpu().numpy(), ref.nll, rtol=1e-5)
    none_loss, none_grad, none_lists, _, _ = run(mwer_ctc_loss_lm, None, 0.7, 0.3)
    assert torch.equal(none_loss, base_loss) and torch.equal(none_grad, base_grad) and _same(none_lists, base_lists)


def test_predict_with_lm_fast(tmp_path):
    """predict(lm_path=, lm_fast=True) on a tiny SyntheticSpeech model writes the predictions of lm_fast=False."""
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.model import build_lm, predict, train
    corpus = tmp_path / "corpus"; out = tmp_path / "run"
    corpus.mkdir()
    (corpus / "alphabet.txt").write_text("a\nb\nc\nd\n \n")
    char2ind = {"<pad>": 0, "a": 1, "b": 2, "c": 3, "d": 4, " ": 5}
    ds = SyntheticSpeech(48, char2ind, n_feats=20, seed=1)
    dv = SyntheticSpeech(16, char2ind, n_feats=20, seed=2)
    train(str(corpus), str(out), 3, 16, 0, train_dataset=ds, dev_dataset=dv, n_feats=20, lam=0.0, lr=3e-3, log_every=0)
    build_lm(str(corpus), order=3, train_dataset=ds)
    lm_path, alphabet = str(corpus / "lm.npz"), str(corpus / "alphabet.txt")
    kw = dict(test_dataset=dv, n_feats=20, lm_path=lm_path, lm_alpha=0.5, lm_beta=0.5)
    slow = predict(None, None, alphabet, str(out), 8, **kw)
    slow_lines = open(out / "predicted.txt").read()
    os.remove(out / "predicted.txt")
    fast = predict(None, None, alphabet, str(out), 8, lm_fast=True, **kw)
    assert open(out / "predicted.txt").read() == slow_lines and len(slow_lines.splitlines()) == 16
    assert fast == slow
