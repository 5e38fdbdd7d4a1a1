"""N-best output of the CTC beam search (csrc/beam.hip, NBEST = true) and second-pass rescoring (csrc/nbest.hip) on the device:
the lists against the plain-Python helper of tests/nbest_ref.py -- all ranks token for token, scores to 1e-9 relative on the exact
(fp64) path and 1e-6 on the fp32 path, whose cases carry the margin condition of tests/test_nbest_cpu.py --, row 0 against the
1-best search bit for bit, the rescoring kernel against its numpy statement, and the host layer on top of both."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as R  # noqa: E402
import nbest_ref as NR  # noqa: E402
from oracle import decode_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lm(table, order, blank=0):
    from policy_gradient_asr_amd.lm import CharNgramLM
    return CharNgramLM(table, order, blank=blank)


def _rows(nb, b):
    """Utterance b of a CTCNBest on the host: (count, [token lists of ALL rows], lengths, scores, raw token rows)."""
    tok, ln, sc = nb.tokens[:, b].cpu().numpy(), nb.lengths[:, b].cpu().numpy(), nb.score[:, b].cpu().numpy()
    return int(nb.count[b]), [list(tok[r, :ln[r]]) for r in range(tok.shape[0])], ln, sc, tok


def _check_list(nb, b, hyps, rel):
    """Utterance b of the device list against the helper's: count, every rank's tokens and length ==, scores to ``rel`` (inf == inf);
    rows beyond count are length 0 / +inf / zero tokens; every token tail is zero."""
    count, seqs, ln, sc, tok = _rows(nb, b)
    assert count == len(hyps)
    for r, (want, wscore) in enumerate(hyps):
        assert seqs[r] == list(want), (b, r)
        assert sc[r] == pytest.approx(wscore, rel=rel), (b, r)
        assert not tok[r, ln[r]:].any()
    for r in range(count, tok.shape[0]):
        assert ln[r] == 0 and sc[r] == np.inf and not tok[r].any(), (b, r)


# (T, V, beam, LM order, blank, sparse): T in {1, 8, 60}, V in {4, 29, 64}, beam in {1, 5, 16, 100, 128}; every list size N in
# {1, 3, beam}.  beam * V is limited by the kernel's LDS (beam 100 and 128 go with V <= 29).  T >= 8 has frames with zero
# probabilities; sparse: only blank and ONE symbol have a non-zero probability in any frame (T = 1: two symbols have none), so most
# of every beam -- the final one included -- are entries of probability zero, ranked among themselves by first touch alone.  The
# sparse cases have blank = 0: with another blank an entry's "stay" candidate and its own repeat extension can carry the same
# first-touch time in the kernel (NOTES.md 0.13), which decides nothing unless both have probability zero.
EXACT_CASES = [
    (1, 4, 1, 2, 0, False), (1, 4, 16, 1, 0, True), (1, 29, 16, 3, 0, False), (1, 64, 5, 2, 63, False), (1, 29, 128, 2, 0, True),
    (8, 4, 128, 4, 2, False), (8, 4, 128, 2, 0, True), (8, 29, 5, 2, 0, False), (8, 64, 16, 2, 0, True), (8, 29, 100, 3, 0, False),
    (8, 29, 100, 2, 0, True), (8, 4, 1, 1, 0, False),
    (60, 4, 100, 3, 0, False), (60, 4, 100, 1, 0, True), (60, 29, 16, 3, 0, False), (60, 64, 5, 4, 63, False), (60, 29, 128, 2, 0, False),
    (60, 64, 1, 1, 0, False), (60, 4, 16, 4, 0, False),
]


@pytest.mark.parametrize("with_lm", [False, True], ids=["nolm", "lm"])
@pytest.mark.parametrize("T,V,beam,order,blank,sparse", EXACT_CASES)
def test_exact_path_matches_the_helper(T, V, beam, order, blank, sparse, with_lm):
    """fp64 log-probabilities (numpy's log of a probability matrix with exact zeros): count, lengths and tokens of every rank ==
    the helper's, scores 1e-9 relative (the exact path's bound), +inf where the helper has it.  Fails without the feature."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    rng = np.random.default_rng(11 * T + V + beam + order)
    logits = rng.normal(size=(T, V)) * rng.choice([0.3, 2.0, 5.0], size=(T, 1))
    logits[:, blank] += 1.5
    probs = np.exp(logits - logits.max(axis=1, keepdims=True))
    syms = [s for s in range(V) if s != blank]
    if sparse and T == 1:
        probs[0, syms[1:3]] = 0.0
    elif sparse:
        probs[:, [s for s in syms if s != syms[2]]] = 0.0
    elif T >= 8:
        probs[3, syms[:2]] = 0.0                                            # zero probabilities (log p = -inf)
        probs[5, :] = 0.0; probs[5, (blank + 2) % V] = 1.0                  # .. and a frame that leaves one symbol
    probs = probs / probs.sum(axis=1, keepdims=True)
    table, alpha, beta = (R.random_table(V, order, blank, seed=T + order), 0.7, 0.9) if with_lm else (None, 0.0, 0.0)
    lm = _lm(table, order, blank) if with_lm else None
    hyps, gap = NR.nbest_prefix_beam_search(probs, table, order, alpha, beta, beam_size=beam, blank=blank, nbest=beam)
    with np.errstate(divide="ignore"):
        lp = torch.from_numpy(np.log(probs)).to(DEV).view(T, 1, V)
    sizes = sorted({1, min(3, beam), beam})
    for N in sizes:
        nb = hipops.ctc_beam_search_nbest(lp, None, beam=beam, nbest=N, blank=blank, lm=lm, lm_alpha=alpha, lm_beta=beta)
        assert nb.tokens.shape == (N, 1, T) and nb.lengths.shape == (N, 1) and nb.score.shape == (N, 1) and nb.count.shape == (1,)
        _check_list(nb, 0, hyps[:N], 1e-9)
    zero = sum(s == np.inf for _, s in hyps)
    print(f"exact T={T} V={V} beam={beam} lm={with_lm} sparse={sparse}: {len(hyps)} entries, {zero} of probability zero, gap {gap:.3e}")
    assert (zero >= 2) == sparse                                            # the sparse cases do put such entries into the list
    # the drop-in decoder returns the same list as (label tuple, score) pairs
    got = CTCDecoder(list(range(V)), lm=lm, lm_alpha=alpha, lm_beta=beta).decode(probs, beam_size=beam, blank=blank, nbest=sizes[-1])
    assert [g[0] for g in got] == [h[0] for h in hyps]
    assert [g[1] for g in got] == [pytest.approx(h[1], rel=1e-9) for h in hyps]


def _fast_ids(c):
    return "-".join(str(x) for x in c)


@pytest.mark.parametrize("with_lm,case", [(True, c) for c in R.FAST_CASES] + [(False, c) for c in NR.NOLM_CASES],
                         ids=lambda v: _fast_ids(v) if isinstance(v, tuple) else ("lm" if v else "nolm"))
def test_fast_path_matches_the_helper(with_lm, case):
    """decode_batch(nbest=min(beam, 16)) on fp32 log-probs with ragged lengths (0 and 1 among them): every rank token for token,
    scores 1e-6 relative (the fp32 path's bound); rows beyond count and token tails as documented."""
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    if with_lm:
        T, V, beam, order, blank, alpha, beta, seed = case
        lp, lens, table = R.fast_case_inputs(case)
        dec = CTCDecoder(list(range(V)), lm=_lm(table, order, blank), lm_alpha=alpha, lm_beta=beta)
    else:
        T, V, beam, blank, seed = case
        lp, lens = NR.nolm_case_inputs(case)
        dec = CTCDecoder(list(range(V)))
    N = NR.list_size(beam)
    nb = dec.decode_batch(torch.from_numpy(lp).to(DEV), torch.from_numpy(lens).to(DEV), beam_size=beam, blank=blank, nbest=N)
    ref = NR.fast_reference(case, with_lm)
    for b in range(R.FAST_B):
        hyps, gap = ref[b]
        print(f"fast {case} b={b} n={int(lens[b])}: {len(hyps)} ranks, gap {gap:.3e}, score[0] {float(nb.score[0, b])!r} reference {hyps[0][1]!r}")
        assert gap >= R.GAP_MIN
        _check_list(nb, b, hyps, 1e-6)
        if lens[b] == 0:
            assert int(nb.count[b]) == 1 and int(nb.lengths[0, b]) == 0 and float(nb.score[0, b]) == 0.0 and np.signbit(float(nb.score[0, b]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("with_lm", [False, True], ids=["nolm", "lm"])
def test_row_0_is_the_1_best_bit_for_bit(dtype, with_lm):
    """Row 0 == ctc_beam_search(generic=True) (no LM) / ctc_beam_search(lm=...) in tokens, length and score, collapse on and off;
    a shorter list is the bitwise prefix of a longer one; collapsed rows are the plain rows with adjacent duplicates removed."""
    from policy_gradient_asr_amd import hipops
    T, B, V, beam, N = 120, 4, 29, 16, 16
    rng = np.random.default_rng(5)
    logits = rng.normal(size=(T, B, V)) * 1.2
    logits[10:13, :, 3] += 8.0; logits[13:15, :, 0] += 8.0; logits[15:18, :, 3] += 8.0      # "3, blank, 3": hypotheses with an adjacent duplicate
    lp = torch.from_numpy(R.log_softmax32(logits)).to(DEV).to(dtype)
    lens = torch.tensor([T, 83, 1, 0], dtype=torch.int32, device=DEV)
    kw = dict(lm=_lm(R.random_table(V, 3, 0, seed=2), 3), lm_alpha=0.6, lm_beta=0.7) if with_lm else {}
    plain = hipops.ctc_beam_search_nbest(lp, lens, beam=beam, nbest=N, **kw)
    coll = hipops.ctc_beam_search_nbest(lp, lens, beam=beam, nbest=N, collapse=True, **kw)
    for flag, nb in ((False, plain), (True, coll)):
        one = hipops.ctc_beam_search(lp, lens, beam=beam, collapse=flag, generic=True, **kw)
        assert torch.equal(nb.tokens[0], one[0]) and torch.equal(nb.lengths[0], one[1]) and torch.equal(nb.score[0], one[2])
        for n in (1, 5):
            short = hipops.ctc_beam_search_nbest(lp, lens, beam=beam, nbest=n, collapse=flag, **kw)
            assert torch.equal(short.tokens, nb.tokens[:n]) and torch.equal(short.lengths, nb.lengths[:n])
            assert torch.equal(short.score, nb.score[:n]) and torch.equal(short.count, nb.count.clamp(max=n))
    assert torch.equal(plain.score, coll.score) and torch.equal(plain.count, coll.count)
    dups = 0
    for b in range(B):
        count, seqs, _, _, _ = _rows(plain, b)
        _, cseqs, cln, _, ctok = _rows(coll, b)
        for r in range(N):
            dedup = [x for i, x in enumerate(seqs[r]) if i == 0 or x != seqs[r][i - 1]]
            dups += len(dedup) < len(seqs[r])
            assert cseqs[r] == dedup and not ctok[r, cln[r]:].any()
    assert dups > 0 and plain.count.tolist()[2:] == [min(N, V), 1]      # some row did collapse; one frame gives V entries, none gives one


def _rescore_inputs(N, B, V, S, order, blank, seed):
    rng = np.random.default_rng(seed)
    lens_pool = [0, 1, 63, 64, 65, 200]
    lengths = np.array([[lens_pool[(n + 2 * b) % 6] for b in range(B)] for n in range(N)], dtype=np.int32)
    syms = np.array([s for s in range(V) if s != blank])
    tokens = np.zeros((N, B, S), dtype=np.int32)
    for n in range(N):
        for b in range(B):
            tokens[n, b, :lengths[n, b]] = rng.choice(syms, size=lengths[n, b])
    count = np.array([N, max(1, N - 2), max(1, N // 2)][:B], dtype=np.int32)
    am = rng.uniform(5.0, 400.0, size=(N, B))
    table = R.random_table(V, order, blank, seed + 1) if order else None
    return tokens, lengths, count, am, table


@pytest.mark.parametrize("N,V,order,blank", [(1, 29, 3, 0), (5, 7, 4, 0), (64, 29, 2, 3), (65, 64, 1, 63), (128, 29, 3, 0), (128, 5, 0, 0)])
def test_rescore_kernel_matches_its_numpy_statement(N, V, order, blank):
    """lm_logp within the fp64 summation bound 2 L 2^-53 sum|x_i| of the exactly rounded sum; total == the stated expression of the
    device's own lm_logp, bit for bit; order == the stable argsort of the reference totals, whose adjacent values differ by more than
    the bound (asserted); rows beyond count and a non-finite am as documented."""
    from policy_gradient_asr_amd import hipops
    B, S = 3, 203
    tokens, lengths, count, am, table = _rescore_inputs(N, B, V, S, order, blank, seed=N + V)
    if N >= 5:
        am[2, 0], am[3, 1] = np.nan, np.inf               # non-finite acoustic scores: total = +inf, last among the utterance's count
    w, alpha, beta = 0.9, 1.3, 0.4
    want_order, want_total, want_lm, abs_sum = NR.rescore_ref(tokens, lengths, count, am, V, blank, table, order, w, alpha, beta)
    d = lambda a: torch.from_numpy(a).to(DEV)
    lm = _lm(table, order, blank) if order else None
    got_order, got_total, got_lm = hipops.nbest_rescore(d(tokens), d(lengths), d(count), d(am), V, blank=blank, lm=lm, am_weight=w,
                                                        lm_alpha=alpha, lm_beta=beta)
    got_order, got_total, got_lm = got_order.cpu().numpy(), got_total.cpu().numpy(), got_lm.cpu().numpy()
    u = 2.0 ** -53
    bound = 2.0 * lengths * u * abs_sum
    assert (np.abs(got_lm - want_lm) <= bound).all(), np.max(np.abs(got_lm - want_lm) - bound)
    valid = np.arange(N)[:, None] < count[None, :]
    assert (got_lm[~valid] == 0).all() and (got_total[~valid] == np.inf).all()
    fin = valid & np.isfinite(am)
    stated = (np.float64(w) * am + -(np.float64(alpha) * got_lm)) + -(np.float64(beta) * lengths.astype(np.float64))
    assert np.array_equal(got_total[fin], stated[fin]) and (got_total[valid & ~np.isfinite(am)] == np.inf).all()
    # the reference totals are apart by more than the two sums' bounds and a few roundings of the expression: the order is decided
    err = alpha * bound + 8 * u * (np.abs(w * am) + np.abs(alpha * want_lm) + beta * lengths)
    for b in range(B):
        idx = want_order[b, :count[b]]
        idx = idx[np.isfinite(want_total[idx, b])]
        t = want_total[idx, b]
        assert (np.diff(t) > (err[idx[1:], b] + err[idx[:-1], b])).all()
    assert np.array_equal(got_order, want_order)
    assert (np.sort(got_order, axis=1) == np.arange(N)[None, :]).all()


def test_rescore_equal_totals_keep_the_first_pass_order():
    """Zero weights and equal am: every total is 0, order is the identity -- the rank is stable."""
    from policy_gradient_asr_amd import hipops
    N, B, V = 128, 3, 29
    tokens, lengths, count, am, table = _rescore_inputs(N, B, V, 203, 2, 0, seed=9)
    am[:] = 7.0
    d = lambda a: torch.from_numpy(a).to(DEV)
    order, total, lm_logp = hipops.nbest_rescore(d(tokens), d(lengths), d(count), d(am), V, lm=_lm(table, 2), am_weight=0.0,
                                                 lm_alpha=0.0, lm_beta=0.0)
    valid = torch.arange(N, device=DEV)[:, None] < d(count)[None, :]
    assert (total[valid] == 0).all() and (total[~valid] == np.inf).all() and (lm_logp[valid & d(lengths > 0)] < 0).all()
    assert torch.equal(order.cpu(), torch.arange(N, dtype=torch.int32).expand(B, N))
    # equal am with the LM switched off but a length bonus: longer first, equal lengths in list order
    order, total, _ = hipops.nbest_rescore(d(tokens), d(lengths), d(count), d(am), V, am_weight=1.0, lm_beta=0.5)
    want = NR.rescore_ref(tokens, lengths, count, am, V, 0, None, 0, 1.0, 0.0, 0.5)[0]
    assert np.array_equal(order.cpu().numpy(), want)


def test_rescore_with_the_exact_ctc_likelihood():
    """acoustic="ctc": am is -log p(y|x) over all alignments -- torch-CPU fp64 ctc_loss of every hypothesis, rtol 1e-5 (the bar
    test_seq_score_gpu holds pgasr_ctc_hyp_lattice to); a hypothesis over max_hyp_len is skipped and ranked last."""
    import torch.nn.functional as F
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    T, B, V, beam, N = 40, 3, 6, 8, 4
    rng = np.random.default_rng(3)
    lp32 = R.log_softmax32(rng.normal(size=(T, B, V)) * 1.5)
    lens = np.array([40, 33, 25], dtype=np.int32)
    lp, d_len = torch.from_numpy(lp32).to(DEV), torch.from_numpy(lens).to(DEV)
    dec = CTCDecoder(list(range(V)))
    nb = dec.decode_batch(lp, d_len, beam_size=beam, nbest=N)
    rs = dec.rescore(lp, d_len, nb, lm=None)
    assert not rs.skipped.any() and nb.count.tolist() == [N] * B
    tok, ln = nb.tokens.cpu().long(), nb.lengths.cpu().long()
    want = torch.empty(N, B, dtype=torch.float64)
    for n in range(N):
        want[n] = F.ctc_loss(torch.from_numpy(lp32).double(), tok[n, :, :max(int(ln[n].max()), 1)], torch.from_numpy(lens).long(), ln[n],
                             blank=0, reduction="none", zero_infinity=False)
    np.testing.assert_allclose(rs.am.cpu().numpy(), want.numpy(), rtol=1e-5, atol=0)
    # no LM, weight 1: total IS am.  The search sums a subset of the hypothesis' alignments, so its score is no smaller than the exact
    # negative log-likelihood -- up to the two kernels' own errors (1e-5 and 1e-6 relative)
    assert torch.equal(rs.total, rs.am) and (rs.am <= nb.score * (1 + 2e-5)).all()
    assert torch.equal(rs.order.cpu().long(), torch.argsort(rs.total.cpu(), dim=0, stable=True).t())
    first = rs.order[:, 0].long()
    assert torch.equal(rs.best_tokens, nb.tokens[first, torch.arange(B, device=DEV)]) and torch.equal(rs.best_len, nb.lengths[first, torch.arange(B, device=DEV)])
    # first-pass scores as acoustic scores: the list's own order comes back
    fp = dec.rescore(lp, d_len, nb, lm=None, acoustic="first_pass")
    assert torch.equal(fp.am, nb.score) and torch.equal(fp.order.cpu(), torch.arange(N, dtype=torch.int32).expand(B, N))
    # a cap below the longest hypothesis: skipped, total +inf, ranked behind every scored one
    cap = int(ln.max()) - 1
    capped = dec.rescore(lp, d_len, nb, lm=None, max_hyp_len=cap)
    skipped = capped.skipped.cpu()
    assert torch.equal(skipped, ln > cap) and skipped.any() and not skipped.all()
    assert (capped.total.cpu()[skipped] == np.inf).all() and torch.equal(capped.total.cpu()[~skipped], rs.total.cpu()[~skipped])
    for b in range(B):
        k = int(skipped[:, b].sum())
        if k:
            assert sorted(capped.order[b, N - k:].tolist()) == [n for n in range(N) if skipped[n, b]]


def test_constructed_flip_by_rescoring():
    """Acoustics slightly prefer "a", the LM strongly prefers "b": "b" sits at a first-pass rank >= 1, rescoring puts it first, and
    with zero LM weights it does not."""
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    T, V = 9, 3
    probs = np.zeros((T, V))
    probs[:] = [0.9, 0.05, 0.05]
    probs[2] = [0.1, 0.46, 0.44]
    table = np.array([0.0, np.log(0.02), np.log(0.98)], dtype=np.float32)
    lm = _lm(table, 1)
    dec = CTCDecoder(["-", "a", "b"])
    lp = torch.from_numpy(np.log(probs)).float().view(T, 1, V).to(DEV)
    nb = dec.decode_batch(lp, None, beam_size=8, nbest=8)
    count, seqs, _, _, _ = _rows(nb, 0)
    assert seqs[0] == [1] and [2] in seqs[1:count]
    r_b = seqs.index([2])
    helper = NR.nbest_prefix_beam_search(probs, beam_size=8, nbest=8)[0]
    assert [list(h) for h, _ in helper] == seqs[:count]
    for acoustic in ("ctc", "first_pass"):
        on = dec.rescore(lp, None, nb, lm=lm, lm_alpha=1.0, lm_beta=0.0, acoustic=acoustic)
        off = dec.rescore(lp, None, nb, lm=lm, lm_alpha=0.0, lm_beta=0.0, acoustic=acoustic)
        assert int(on.order[0, 0]) == r_b and on.best_tokens[0, :on.best_len[0]].tolist() == [2]
        assert int(off.order[0, 0]) == 0 and off.best_tokens[0, :off.best_len[0]].tolist() == [1]
        assert float(on.lm_logp[r_b, 0]) == pytest.approx(float(table[2]), rel=1e-15)
    # the decoder's own LM is the default of rescore
    own = CTCDecoder(["-", "a", "b"], lm=lm, lm_alpha=1.0).rescore(lp, None, nb)
    assert int(own.order[0, 0]) == r_b


def test_nbest_oracle_matches_a_loop_over_the_oracle_edit_distance():
    from policy_gradient_asr_amd import hipops, metrics
    T, B, V, beam, N = 50, 5, 8, 8, 8
    rng = np.random.default_rng(21)
    lp = torch.from_numpy(R.log_softmax32(rng.normal(size=(T, B, V)) * 2.5)).to(DEV)
    lens = torch.tensor([50, 41, 1, 0, 30], dtype=torch.int32, device=DEV)
    nb = hipops.ctc_beam_search_nbest(lp, lens, beam=beam, nbest=N, collapse=True)
    L = T
    tg_len = np.array([12, 7, 1, 0, 9], dtype=np.int32)
    targets = np.zeros((B, L), dtype=np.int32)
    for b in range(B):
        targets[b, :tg_len[b]] = rng.integers(1, V, size=tg_len[b])
    # make one target a hypothesis of rank 2: the oracle finds it (or an equal string ranked above it)
    count, seqs, _, _, _ = _rows(nb, 0)
    assert count > 2 and 0 < len(seqs[2]) <= L
    tg_len[0] = len(seqs[2]); targets[0] = 0; targets[0, :tg_len[0]] = seqs[2]
    dist, rank = metrics.nbest_oracle(torch.from_numpy(targets).to(DEV), torch.from_numpy(tg_len).to(DEV), nb)
    assert dist.shape == (B,) and rank.shape == (B,)
    for b in range(B):
        count, seqs, _, _, _ = _rows(nb, b)
        ds = [decode_ref.edit_dist(list(targets[b, :tg_len[b]]), seqs[r])[0] for r in range(count)]
        assert int(dist[b]) == min(ds) and int(rank[b]) == ds.index(min(ds)), (b, ds)
    assert int(dist[0]) == 0 and int(rank[0]) <= 2


def test_predict_with_nbest(tmp_path):
    """predict(nbest=4) on a tiny SyntheticSpeech model: the CER / WER of nbest=1 when nothing is rescored, a well-formed nbest.tsv
    whose rank-0 lines are predicted.txt's hypotheses, and a rescored run that writes totals."""
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.model import build_lm, predict, train
    corpus = tmp_path / "corpus"; out = tmp_path / "run"
    corpus.mkdir()
    (corpus / "alphabet.txt").write_text("a\nb\nc\nd\n \n")
    char2ind = {"<pad>": 0, "a": 1, "b": 2, "c": 3, "d": 4, " ": 5}
    ds = SyntheticSpeech(48, char2ind, n_feats=20, seed=1)
    dv = SyntheticSpeech(16, char2ind, n_feats=20, seed=2)
    train(str(corpus), str(out), 6, 16, 0, train_dataset=ds, dev_dataset=dv, n_feats=20, lam=0.0, lr=3e-3, log_every=0)
    build_lm(str(corpus), order=3, train_dataset=ds)
    alphabet = str(corpus / "alphabet.txt")
    base = predict(None, None, alphabet, str(out), 8, test_dataset=dv, n_feats=20)
    assert not os.path.exists(out / "nbest.tsv")                      # the default writes what it always wrote
    base_lines = open(out / "predicted.txt").read().splitlines()
    got = predict(None, None, alphabet, str(out), 8, test_dataset=dv, n_feats=20, nbest=4)
    assert got == base
    lines = open(out / "predicted.txt").read().splitlines()
    assert lines == base_lines and len(lines) == 16
    rows = [ln.split("\t") for ln in open(out / "nbest.tsv").read().splitlines()]
    assert all(len(r) == 5 for r in rows)
    by_utt = {}
    for u, r, score, total, text in rows:
        assert total == "" and np.isfinite(float(score))
        by_utt.setdefault(int(u), []).append((int(r), float(score), text))
    assert sorted(by_utt) == list(range(16))
    for u, hyps in by_utt.items():
        assert [h[0] for h in hyps] == list(range(len(hyps))) and 1 <= len(hyps) <= 4
        assert [h[1] for h in hyps] == sorted(h[1] for h in hyps)
        assert hyps[0][2] == lines[u].split("|", 1)[1]
    cer, wer = predict(None, None, alphabet, str(out), 8, test_dataset=dv, n_feats=20, nbest=4,
                       rescore_lm_path=str(corpus / "lm.npz"), rescore_alpha=0.5, rescore_beta=0.5)
    assert 0.0 <= cer and np.isfinite(wer)
    rows = [ln.split("\t") for ln in open(out / "nbest.tsv").read().splitlines()]
    assert all(len(r) == 5 and np.isfinite(float(r[3])) for r in rows)
    with pytest.raises(ValueError):
        predict(None, None, alphabet, str(out), 8, test_dataset=dv, n_feats=20, nbest=9)
    with pytest.raises(ValueError):
        predict(None, None, alphabet, str(out), 8, test_dataset=dv, n_feats=20, rescore_lm_path=str(corpus / "lm.npz"))
