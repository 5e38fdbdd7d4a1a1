"""The lattice-free CTC scorer (csrc/hyp_score.hip, ``hipops.ctc_hyp_score``) on the MI355X and the second pass it opens for wide
and long lists: the device against the numpy statement of tests/hyp_score_ref.py at 1e-9 relative (+inf compared by ==) on the
cases tests/test_hyp_score_cpu.py holds to torch fp64, against pgasr_ctc_hyp_lattice within its limits, and the wiring into
``CTCDecoder.rescore`` / ``mbr_decode`` and ``model.predict``."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as R  # noqa: E402
import hyp_score_ref as H  # noqa: E402
import mbr_ref as M  # noqa: E402
import nbest_ref as NR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _d(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def _run(c, tokens=None):
    from policy_gradient_asr_amd import hipops
    out = hipops.ctc_hyp_score(_d(c["lp"]), _d(c["tokens"] if tokens is None else tokens), _d(c["lengths"]), _d(c["in_len"]), c["Lh"],
                               count=_d(c["count"]), blank=c["blank"])
    assert out.dtype == torch.float64 and tuple(out.shape) == c["lengths"].shape
    return out.cpu().numpy()


@pytest.mark.parametrize("name", H.EDGE)
def test_edge_grid_meets_the_statement(name):
    """V in {2, 29, 64, 65, 128, 1000, 1024}, blank in {0, 70, V-1}, the lengths of hyp_score_ref.LENGTHS (both sides of every
    states-per-thread switch among them), runs of one symbol at the least feasible frame count and one less, T = 1, utterances
    without frames, N in {1, 16, 17, 128}, count 0 / below N / NULL, rows over Lh, hyp_stride > Lh, tokens that are no symbols:
    1e-9 relative, +inf == +inf, no NaN; token tails of 2^30 and a second call give the same bits.  Fails without the feature."""
    c = H.case(name)
    got = _run(c)
    worst = H.close(got, c["want"])
    print(f"{name}: largest relative deviation {worst:.2e}")
    assert np.array_equal(_run(c, H.garbage_tails(c)).view(np.int64), got.view(np.int64))
    assert np.array_equal(_run(c).view(np.int64), got.view(np.int64))


def test_long_and_steep():
    """T = 1000, B = 2, N = 4, V = 1024, len ~ 300, row maxima falling ~20 nats per frame (nll ~ 2e4): 1e-9 relative."""
    c = H.case("steep")
    got = _run(c)
    print(f"steep: largest relative deviation {H.close(got, c['want']):.2e}")


def test_zero_probabilities():
    """Symbols of probability exactly 0: the hypotheses that hold one are +inf, the others meet the statement, nothing is NaN."""
    c = H.case("zeros")
    got = _run(c)
    H.close(got, c["want"])
    assert (got == np.inf).any() and np.isfinite(got).any()


@pytest.mark.parametrize("name", H.LATTICE)
def test_against_the_lattice(name):
    """V <= 64, N <= 16: float32(ctc_hyp_score) within one fp32 ulp of pgasr_ctc_hyp_lattice's hyp_nll wherever the pair has a
    lattice (both are roundings of values that agree far below an fp32 ulp); +inf where the lattice has +inf."""
    from policy_gradient_asr_amd import hipops
    c = H.case(name)
    got = _run(c)
    nll, _ = hipops.ctc_hyp_lattice(_d(c["lp"]), _d(c["tokens"]), _d(c["lengths"]), _d(c["in_len"]), c["Lh"], blank=c["blank"])
    nll = nll.cpu().numpy()
    cnt = np.full(got.shape[1], got.shape[0]) if c["count"] is None else c["count"]
    rows = (np.arange(got.shape[0])[:, None] < cnt[None, :]) & (c["lengths"] <= c["Lh"])
    assert rows.any()
    g32 = got.astype(np.float32)
    fin = np.isfinite(nll) & rows
    assert (np.isfinite(g32) == np.isfinite(nll))[rows].all()
    assert (np.abs(g32[fin] - nll[fin]) <= np.spacing(np.abs(nll[fin]))).all()


def _nbest_case(T, B, V, beam, N, seed, lens):
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    rng = np.random.default_rng(seed)
    lp32 = H.log_softmax32(rng.normal(size=(T, B, V)) * 1.5)
    lens = np.asarray(lens, dtype=np.int32)
    dec = CTCDecoder(list(range(V)), wide_search=V > 64)
    lp, d_len = _d(lp32), _d(lens)
    return dec, lp32, lens, lp, d_len, dec.decode_batch(lp, d_len, beam_size=beam, nbest=N)


def _statement_for(nb, lp32, lens, Lh, blank=0):
    return H.hyp_score_ref(lp32, nb.tokens.cpu().numpy(), nb.lengths.cpu().numpy(), nb.count.cpu().numpy(), lens, Lh, blank)


def test_rescore_takes_32_rows():
    """V = 29, N = 32, acoustic="ctc": it succeeds (PGASR_ERR_INVALID_ARG before the forward scorer: fails without the feature), am
    meets the statement, order is the stable argsort of total; with a character LM the total is the stated expression of the
    device's am and lm_logp bit for bit, and tests/nbest_ref.py's rescore_ref applied to the device's am gives the same totals up
    to the LM sum's bound (2 L 2^-53 sum|x|, as tests/test_nbest_gpu.py) and a few roundings of the expression."""
    from policy_gradient_asr_amd.lm import CharNgramLM
    T, B, V, N = 40, 2, 29, 32
    dec, lp32, lens, lp, d_len, nb = _nbest_case(T, B, V, 32, N, 5, [40, 31])
    assert nb.count.tolist() == [N] * B
    rs = dec.rescore(lp, d_len, nb, lm=None)
    want = _statement_for(nb, lp32, lens, int(nb.lengths.max()))
    H.close(rs.am.cpu().numpy(), want)
    assert torch.equal(rs.total, rs.am) and not rs.skipped.any()
    assert torch.equal(rs.order.cpu().long(), torch.argsort(rs.total.cpu(), dim=0, stable=True).t())
    assert torch.equal(dec.rescore(lp, d_len, nb, lm=None, scorer="forward").am, rs.am)
    with pytest.raises(ValueError, match="lattice"):
        dec.rescore(lp, d_len, nb, lm=None, scorer="lattice")
    table = R.random_table(V, 2, 0, 11)
    w, alpha, beta = 0.9, 0.7, 0.3
    on = dec.rescore(lp, d_len, nb, lm=CharNgramLM(table, 2, blank=0), lm_alpha=alpha, lm_beta=beta, am_weight=w)
    am, tokens, lengths, count = on.am.cpu().numpy(), nb.tokens.cpu().numpy(), nb.lengths.cpu().numpy(), nb.count.cpu().numpy()
    assert np.array_equal(am, rs.am.cpu().numpy())
    got_total, got_lm = on.total.cpu().numpy(), on.lm_logp.cpu().numpy()
    stated = (np.float64(w) * am + -(np.float64(alpha) * got_lm)) + -(np.float64(beta) * lengths.astype(np.float64))
    assert np.array_equal(got_total, stated)
    ref_order, ref_total, ref_lm, abs_sum = NR.rescore_ref(tokens, lengths, count, am, V, 0, table, 2, w, alpha, beta)
    u = 2.0 ** -53
    err = alpha * 2.0 * lengths * u * abs_sum + 8 * u * (np.abs(w * am) + np.abs(alpha * ref_lm) + beta * lengths)
    assert (np.abs(got_total - ref_total) <= err).all()
    assert torch.equal(on.order.cpu().long(), torch.argsort(on.total.cpu(), dim=0, stable=True).t())


def test_rescore_default_stays_on_the_lattice():
    """N = 4, V = 6: scorer=None is scorer="lattice", every field bit for bit; "forward" may be forced and agrees to the lattice's bar."""
    dec, lp32, lens, lp, d_len, nb = _nbest_case(40, 3, 6, 8, 4, 3, [40, 33, 25])
    a, b = dec.rescore(lp, d_len, nb, lm=None), dec.rescore(lp, d_len, nb, lm=None, scorer="lattice")
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x, y)
    assert torch.equal(a.total.view(torch.int64), b.total.view(torch.int64)) and torch.equal(a.am.view(torch.int64), b.am.view(torch.int64))
    f = dec.rescore(lp, d_len, nb, lm=None, scorer="forward")
    H.close(f.am.cpu().numpy(), _statement_for(nb, lp32, lens, int(nb.lengths.max())))
    np.testing.assert_allclose(a.am.cpu().numpy(), f.am.cpu().numpy(), rtol=1e-5, atol=0)       # tests/test_nbest_gpu.py's bar for the lattice


def test_rescore_a_wide_list():
    """V = 300, decode_batch(nbest=8) on CTCDecoder(wide_search=True): am meets the statement, total is (am_weight * am + -0.0) +
    -(lm_beta * len) bit for bit, am <= the first-pass score (a partial sum) up to the two kernels' errors, lm= and word_lm= raise
    by name."""
    dec, lp32, lens, lp, d_len, nb = _nbest_case(30, 3, 300, 8, 8, 7, [30, 24, 17])
    w, beta = 0.8, 0.25
    rs = dec.rescore(lp, d_len, nb, lm=None, am_weight=w, lm_beta=beta)
    am, lengths = rs.am.cpu().numpy(), nb.lengths.cpu().numpy()
    H.close(am, _statement_for(nb, lp32, lens, int(nb.lengths.max())))
    stated = (np.float64(w) * am + -0.0) + -(np.float64(beta) * lengths.astype(np.float64))
    valid = np.arange(8)[:, None] < nb.count.cpu().numpy()[None, :]
    assert valid.all() and np.array_equal(rs.total.cpu().numpy().view(np.int64), stated.view(np.int64))
    assert (rs.am <= nb.score * (1 + 2e-5)).all() and not rs.lm_logp.any() and not rs.skipped.any()
    assert torch.equal(rs.order.cpu().long(), torch.argsort(rs.total.cpu(), dim=0, stable=True).t())
    first = rs.order[:, 0].long()
    assert torch.equal(rs.best_tokens, nb.tokens[first, torch.arange(3, device=DEV)])
    for name, kw in (("lm", dict(lm=object())), ("word_lm", dict(lm=None, word_lm=object(), word_delimiter=4))):
        with pytest.raises(ValueError, match="^" + name + ":"):
            dec.rescore(lp, d_len, nb, **kw)


def _close12(got, want):
    fin = np.isfinite(want)
    assert (np.isfinite(got) == fin).all() and (got[~fin] == want[~fin]).all()
    assert (np.abs(got[fin] - want[fin]) <= 1e-12 * np.abs(want[fin])).all()


def test_mbr_decode_over_a_wide_list():
    """V = 300, nbest 8: dist == the plain DP of tests/mbr_ref.py over units; posterior and risk 1e-12 against its selection on the
    device's totals, the choice within the margin (tests/test_mbr_gpu.py's checks), == at scale 0; word units raise."""
    dec, lp32, lens, lp, d_len, _ = _nbest_case(30, 3, 300, 8, 8, 7, [30, 24, 17])
    T, V = 30, 300
    md = dec.mbr_decode(lp, d_len, beam_size=8, nbest=8, posterior_scale=0.8)
    nb = md.nbest
    tokens, lengths, count = nb.tokens.cpu().numpy(), nb.lengths.cpu().numpy(), nb.count.cpu().numpy()
    total = dec.rescore(lp, d_len, nb).total.cpu().numpy()
    want = M.pair_dist_ref(tokens, lengths, count, V, T)
    assert (md.dist.cpu().numpy() == want).all() and (want[:, 0, 1:] > 0).all()
    rbest, rrisk, rpost = M.select_ref(want, total, count, 0.8)
    best = md.best.cpu().numpy()
    assert all(M.best_within_margin(best, rrisk))
    _close12(md.posterior.cpu().numpy(), rpost); _close12(md.risk.cpu().numpy(), rrisk)
    for b in range(3):
        assert md.lengths[b] == lengths[best[b], b] and (md.tokens[b].cpu().numpy() == tokens[best[b], b]).all()
    m0 = dec.mbr_from_list(nb, nb.score, vocab=V, posterior_scale=0.0, max_hyp_len=T)
    b0, r0, p0 = M.select_ref(want, nb.score.cpu().numpy(), count, 0.0)
    assert np.array_equal(m0.risk.cpu().numpy(), r0) and np.array_equal(m0.posterior.cpu().numpy(), p0)
    assert np.array_equal(m0.best.cpu().numpy(), b0)
    with pytest.raises(ValueError, match="unit='word'"):
        dec.mbr_from_list(nb, nb.score, vocab=V, risk_unit="word", word_delimiter=4)


def test_predict_with_the_wide_second_pass(tmp_path, capsys):
    """model.predict(units_path=, wide_beam=True, wide_second_pass=True, nbest=4, mbr=True) on SyntheticSpeech over 100 units
    (tests/test_beam_wide_gpu.py's setup): finite totals in nbest.tsv, mbr.tsv written; mbr_unit="word" and the options that stay
    refused raise by name."""
    import itertools
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.model import Seq2Seq, _read_alphabet, predict
    from policy_gradient_asr_amd.units import SubwordUnits
    corpus = tmp_path / "corpus"; out = tmp_path / "run"
    corpus.mkdir(); out.mkdir()
    base = ["a", "b", "c", "d", " "]
    two = ["".join(q) for q in itertools.product(base, repeat=2)]
    three = ["".join(q) for q in itertools.product(base, repeat=3)]
    upath = str(corpus / "units.txt")
    SubwordUnits(base + two + three[:70]).save(upath)
    _, char2ind = _read_alphabet(upath)
    ds = SyntheticSpeech(16, char2ind, n_feats=20, max_chars=4, seed=1)
    torch.manual_seed(0)
    torch.save(Seq2Seq(alphabet_size=101, n_feats=20).state_dict(), os.path.join(str(out), "model_best.pth"))
    kw = dict(test_dataset=ds, n_feats=20, units_path=upath, beam_size=4, wide_beam=True, wide_second_pass=True)
    for name, arg in (("mbr_unit='word'", dict(mbr=True, mbr_unit="word", nbest=4)), ("rescore_word_lm_path", dict(rescore_word_lm_path="x.npz", nbest=4)),
                      ("rescore_lm_path", dict(rescore_lm_path="x.npz", nbest=4)), ("lm_path", dict(lm_path="x.npz", nbest=4)),
                      ("error_report", dict(error_report=True, nbest=4)), ("nbest", dict())):
        with pytest.raises(ValueError, match=name):
            predict(None, None, None, str(out), 8, **arg, **kw)
    capsys.readouterr()
    cer, wer = predict(None, None, None, str(out), 8, nbest=4, mbr=True, **kw)
    assert np.isfinite(cer) and np.isfinite(wer) and "MAP CER" in capsys.readouterr().out
    rows = [ln.split("\t") for ln in open(os.path.join(str(out), "nbest.tsv")).read().splitlines()]
    assert {int(r[0]) for r in rows} == set(range(len(ds))) and all(len(r) == 5 for r in rows)
    assert all(r[3] != "" and np.isfinite(float(r[3])) and float(r[3]) <= float(r[2]) * (1 + 2e-5) + 1e-6 for r in rows)
    lines = open(os.path.join(str(out), "mbr.tsv")).read().splitlines()
    assert [int(ln.split("\t")[0]) for ln in lines] == list(range(len(ds)))
    for ln in lines:
        _, rank, chosen, first = ln.split("\t")
        assert 0 <= int(rank) < 4 and 0.0 <= float(chosen) <= float(first) + 1e-6
    assert len(open(os.path.join(str(out), "predicted.txt")).read().splitlines()) >= len(ds)
    # without mbr: the re-ranked best row is written, nbest.tsv keeps its totals and no mbr.tsv is produced anew
    os.remove(os.path.join(str(out), "mbr.tsv"))
    cer2, wer2 = predict(None, None, None, str(out), 8, nbest=4, **kw)
    assert np.isfinite(cer2) and np.isfinite(wer2) and not os.path.exists(os.path.join(str(out), "mbr.tsv"))
