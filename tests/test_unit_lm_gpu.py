"""The back-off unit n-gram LM on the MI355X (lm.UnitNgramLM; csrc/beam_wide.hip with a model, csrc/unit_lm.hip): the fused wide search
against the oracles of tests/unit_lm_ref.py on its cases, the counting selection against the threshold list, zero weights against the
search without a model, bit-equality with the narrow workgroup kernel over the dense form, the second pass against the dict
statement, and the wiring into CTCDecoder and model.predict.  Score bounds are those of tests/test_nbest_gpu.py: 1e-9 relative for
fp64 input, 1e-6 relative for fp32 input."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as R  # noqa: E402
import beam_wide_cases as W  # noqa: E402
import nbest_ref as NR  # noqa: E402
import unit_lm_ref as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = {torch.float64: 1e-9, torch.float32: 1e-6}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])


def _rows(nb, b):
    tok, ln, sc = nb.tokens[:, b].cpu().numpy(), nb.lengths[:, b].cpu().numpy(), nb.score[:, b].cpu().numpy()
    return int(nb.count[b]), [list(tok[r, :ln[r]]) for r in range(tok.shape[0])], ln, sc, tok


def _check_list(nb, b, hyps, rel):
    """Utterance b of the device list against the oracle's: count, every rank's tokens and length ==, scores to ``rel``; rows beyond
    count are length 0 / +inf / zero tokens; every token tail is zero."""
    count, seqs, ln, sc, tok = _rows(nb, b)
    assert count == len(hyps), (b, count, len(hyps))
    for r, (want, wscore) in enumerate(hyps):
        assert seqs[r] == list(want), (b, r)
        assert sc[r] == pytest.approx(wscore, rel=rel), (b, r)
        assert not tok[r, ln[r]:].any()
    for r in range(count, tok.shape[0]):
        assert ln[r] == 0 and sc[r] == np.inf and not tok[r].any(), (b, r)


def _same(a, b):
    """Two CTCNBest, every output word bit for bit (scores as their 64-bit images)."""
    return (torch.equal(a.tokens, b.tokens) and torch.equal(a.lengths, b.lengths) and torch.equal(a.count, b.count)
            and torch.equal(a.score.view(torch.int64), b.score.view(torch.int64)))


def _dev(lp, lens, dtype):
    return torch.from_numpy(np.array(lp)).to(DEV).to(dtype), torch.from_numpy(np.array(lens)).to(DEV)


@DTYPES
@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_fused_lists_match_the_oracle(case, dtype):
    """Tokens, lengths and count == the oracle's lists at N = min(beam, 16); scores within the arithmetic's bound; counting=True
    changes no output word; the flat case with lm_beta = 3 overflows the threshold list without being forced."""
    from policy_gradient_asr_amd import hipops
    T, V, beam, order, blank, B, alpha, beta, kind, seed = case
    lp, lens = U.case_inputs(case)
    _, model = U.case_model(case)
    x, n = _dev(lp, lens, dtype)
    N = U.list_size(beam)
    kw = dict(beam=beam, nbest=N, blank=blank, unit_lm=model, lm_alpha=alpha, lm_beta=beta)
    nb, frames = hipops.ctc_beam_search_wide(x, n, stats=True, **kw)
    for b, (hyps, gap) in enumerate(U.reference(case)):
        print(f"{U.case_id(case)} b={b} n={int(lens[b])}: gap {gap:.3e}, score[0] {float(nb.score[0, b])!r} reference {hyps[0][1]!r}, "
              f"counting frames {int(frames[b])}")
        _check_list(nb, b, hyps, REL[dtype])
    if kind == "flat":
        assert any(f > 0 for f in frames.tolist()), frames.tolist()
    forced, fframes = hipops.ctc_beam_search_wide(x, n, counting=True, stats=True, **kw)
    assert _same(forced, nb)
    assert fframes.tolist() == lens.tolist()
    assert all(0 <= f <= t for f, t in zip(frames.tolist(), lens.tolist()))
    tok, tl, sc = hipops.ctc_beam_search_wide(x, n, **dict(kw, nbest=None))
    assert torch.equal(tok, nb.tokens[0]) and torch.equal(tl, nb.lengths[0]) and torch.equal(sc.view(torch.int64), nb.score[0].view(torch.int64))


@DTYPES
@pytest.mark.parametrize("case", [U.CASES[0], U.CASES[3], U.CASES[5]], ids=U.case_id)
def test_zero_weights_equal_the_search_without_a_model(case, dtype):
    """alpha = beta = 0 with a table: every output word of the call without a model, for both selections."""
    from policy_gradient_asr_amd import hipops
    T, V, beam, order, blank, B, alpha, beta, kind, seed = case
    lp, lens = U.case_inputs(case)
    _, model = U.case_model(case)
    x, n = _dev(lp, lens, dtype)
    N = U.list_size(beam)
    want = hipops.ctc_beam_search_wide(x, n, beam=beam, nbest=N, blank=blank)
    assert _same(hipops.ctc_beam_search_wide(x, n, beam=beam, nbest=N, blank=blank, unit_lm=model), want)
    assert _same(hipops.ctc_beam_search_wide(x, n, beam=beam, nbest=N, blank=blank, unit_lm=model, counting=True), want)


NARROW = [c for c in R.FAST_CASES if c[1] in (29, 64) and c[3] in (2, 3)] + [(80, 64, 5, 3, 63, 0.6, 0.6, 0)]


@DTYPES
@pytest.mark.parametrize("case", NARROW, ids=lambda c: "-".join(str(x) for x in c))
def test_narrow_rows_equal_the_narrow_lm_kernel_bit_for_bit(case, dtype):
    """V in {29, 64}, orders 2 and 3, the shared fp32 inputs of beam_lm_ref: every output word of the wide entry with the sparse model
    == ctc_beam_search_nbest(lm=to_dense()) without ``fast`` (the workgroup kernel over the dense table), both selections."""
    from policy_gradient_asr_amd import hipops
    T, V, beam, order, blank, alpha, beta, seed = case
    lp, lens, _ = R.fast_case_inputs(case)
    _, model = U.random_unit_lm(V, order, blank, seed + 17)
    x, n = _dev(lp, lens, dtype)
    N = NR.list_size(beam)
    want = hipops.ctc_beam_search_nbest(x, n, beam=beam, nbest=N, blank=blank, lm=model.to_dense(), lm_alpha=alpha, lm_beta=beta)
    kw = dict(beam=beam, nbest=N, blank=blank, unit_lm=model, lm_alpha=alpha, lm_beta=beta)
    assert _same(hipops.ctc_beam_search_wide(x, n, **kw), want)
    assert _same(hipops.ctc_beam_search_wide(x, n, counting=True, **kw), want)


def _random_lists(V, blank, seed, N=12, B=4, S=40):
    """tokens (N,B,S) with ragged lengths, count < N in some utterances, an empty row, a row with a symbol outside [0, V), one with
    the blank; garbage behind every length."""
    rng = np.random.default_rng(seed)
    syms = np.array([s for s in range(V) if s != blank])
    tokens = rng.integers(-5, V + 5, size=(N, B, S)).astype(np.int32)
    lengths = rng.integers(1, S + 1, size=(N, B)).astype(np.int32)
    for n in range(N):
        for b in range(B):
            tokens[n, b, :lengths[n, b]] = rng.choice(syms, size=lengths[n, b])
    lengths[1, 0] = 0
    tokens[2, 0, lengths[2, 0] // 2] = V
    tokens[3, 1, 0] = blank
    tokens[4, 1, lengths[4, 1] - 1] = -1
    count = np.array([N, N - 3, 1, 0][:B], dtype=np.int32)
    return tokens, lengths, count


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("V", [29, 300, 1024])
def test_nbest_unit_lm_score_equals_the_dict_statement(V, order):
    from policy_gradient_asr_amd import hipops
    blank = V // 3
    d, model = U.random_unit_lm(V, order, blank, 5 + V + order)
    tokens, lengths, count = _random_lists(V, blank, V + order)
    got = hipops.nbest_unit_lm_score(torch.from_numpy(tokens).to(DEV), torch.from_numpy(lengths).to(DEV), torch.from_numpy(count).to(DEV),
                                     model).cpu().numpy()
    N, B, S = tokens.shape
    for b in range(B):
        for n in range(N):
            y = tokens[n, b, :lengths[n, b]].tolist()
            if n >= count[b]:
                want = 0.0
            elif any(t < 0 or t >= V or t == blank for t in y):
                want = -np.inf
            else:
                want = U.sequence(d, order, blank, y)
                assert want == model.logp_sequence(y)
            assert got[n, b] == want, (n, b, got[n, b], want)


@pytest.mark.parametrize("acoustic", ["first_pass", "ctc"])
@pytest.mark.parametrize("case", [U.CASES[3], NARROW[1]], ids=["V300", "V29"])
def test_rescore_with_a_unit_lm(case, acoustic):
    """rescore(unit_lm=) on a wide and on a narrow list: unit_logp == the dict statement, total == the formula with the roundings of
    nbest_ref.rescore_ref (each product and sum rounded once) on the returned am, order == its stable ascending rank;
    mbr_decode(unit_lm=) takes its posterior from those totals."""
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    if len(case) == 10:
        T, V, beam, order, blank = case[:5]
        lp, lens = U.case_inputs(case)
        d, model = U.case_model(case)
    else:
        T, V, beam, order, blank = case[:5]
        lp, lens, _ = R.fast_case_inputs(case)
        d, model = U.random_unit_lm(V, order, blank, 3)
    x, n = _dev(lp, lens, torch.float32)
    dec = CTCDecoder(list(range(V)), wide_search=True)
    N = min(beam, 4)
    nb = dec.decode_batch(x, n, beam_size=beam, blank=blank, nbest=N)
    ua, ub, lb, aw = 0.7, 0.3, 0.2, 0.9
    rs = dec.rescore(x, n, nb, lm=None, lm_beta=lb, acoustic=acoustic, am_weight=aw, blank=blank, unit_lm=model, unit_lm_alpha=ua,
                     unit_lm_beta=ub)
    assert rs._fields[-1] == "unit_logp"
    tok, ln, cnt = nb.tokens.cpu().numpy(), nb.lengths.cpu().numpy(), nb.count.cpu().numpy()
    am, total, ulp, order_ = rs.am.cpu().numpy(), rs.total.cpu().numpy(), rs.unit_logp.cpu().numpy(), rs.order.cpu().numpy()
    for b in range(tok.shape[1]):
        want = np.full(N, np.inf)
        for r in range(N):
            if r >= cnt[b]:
                assert ulp[r, b] == 0.0 and total[r, b] == np.inf
                continue
            L = int(ln[r, b])
            assert ulp[r, b] == U.sequence(d, order, blank, tok[r, b, :L].tolist())
            if np.isfinite(am[r, b]):
                base = (np.float64(aw) * np.float64(am[r, b]) + -(np.float64(0.0) * np.float64(0.0))) + -(np.float64(lb) * np.float64(L))
                want[r] = (base + -(np.float64(ua) * np.float64(ulp[r, b]))) + -(np.float64(ub) * np.float64(L))
            assert total[r, b] == want[r], (b, r, total[r, b], want[r])
        assert order_[b].tolist() == list(np.argsort(want[:cnt[b]], kind="stable")) + list(range(cnt[b], N))
    md = dec.mbr_decode(x, n, beam_size=beam, nbest=N, acoustic=acoustic, lm=None, lm_beta=lb, am_weight=aw, blank=blank, unit_lm=model,
                        unit_lm_alpha=ua, unit_lm_beta=ub)
    ref = dec.mbr_from_list(nb, rs.total, vocab=V)
    assert torch.equal(md.posterior.view(torch.int64), ref.posterior.view(torch.int64)) and torch.equal(md.best, ref.best)


def test_decoder_wiring():
    """CTCDecoder(wide_search=True, unit_lm=): decode and its nbest form == the oracle on a probability matrix; decode_batch is the
    hipops call, for wide and for narrow rows."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    case = U.CASES[0]
    T, V, beam, order, blank, B, alpha, beta, kind, seed = case
    lp, lens = U.case_inputs(case)
    d, model = U.case_model(case)
    dec = CTCDecoder(list(range(V)), wide_search=True, unit_lm=model, lm_alpha=alpha, lm_beta=beta)
    probs = np.exp(lp[:, 0].astype(np.float64))
    with np.errstate(divide="ignore"):
        hyps, gap = U.fused_search(d, model, np.log(probs), alpha, beta, beam, blank, 4)
    got = dec.decode(probs, beam_size=beam, blank=blank)
    assert gap > 1e-9 and got[0] == tuple(hyps[0][0]) and got[1] == pytest.approx(hyps[0][1], rel=1e-9)
    lst = dec.decode(probs, beam_size=beam, blank=blank, nbest=4)
    assert [h[0] for h in lst] == [tuple(h[0]) for h in hyps] and [h[1] for h in lst] == [pytest.approx(h[1], rel=1e-9) for h in hyps]
    x, n = _dev(lp, lens, torch.float32)
    kw = dict(beam=beam, blank=blank, unit_lm=model, lm_alpha=alpha, lm_beta=beta)
    assert _same(dec.decode_batch(x, n, beam_size=beam, blank=blank, nbest=4), hipops.ctc_beam_search_wide(x, n, nbest=4, **kw))
    assert all(torch.equal(a, b) for a, b in zip(dec.decode_batch(x, n, beam_size=beam, blank=blank), hipops.ctc_beam_search_wide(x, n, **kw)))
    ncase = NARROW[0]
    nlp, nlens, _ = R.fast_case_inputs(ncase)
    _, nmodel = U.random_unit_lm(ncase[1], ncase[3], ncase[4], 1)
    y, m = _dev(nlp, nlens, torch.float32)
    ndec = CTCDecoder(list(range(ncase[1])), wide_search=True, unit_lm=nmodel, lm_alpha=0.5, lm_beta=0.1)
    assert _same(ndec.decode_batch(y, m, beam_size=ncase[2], blank=ncase[4], nbest=2),
                 hipops.ctc_beam_search_wide(y, m, beam=ncase[2], nbest=2, blank=ncase[4], unit_lm=nmodel, lm_alpha=0.5, lm_beta=0.1))


def test_predict_with_a_unit_lm(tmp_path, capsys):
    """model.build_unit_lm writes unit_lm.npz from the transcripts; predict(units_path=, wide_beam=True, unit_lm_path=) on SyntheticSpeech
    over 100 units writes the fused hypotheses (first-pass scores differ from the run without the model); with wide_second_pass and
    rescore_unit_lm_path nbest.tsv carries the total and, as its last column, unit_logp (a finite log-probability)."""
    import itertools
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.lm import UnitNgramLM
    from policy_gradient_asr_amd.model import Seq2Seq, _read_alphabet, build_unit_lm, predict
    from policy_gradient_asr_amd.units import SubwordUnits
    corpus = tmp_path / "corpus"; out = tmp_path / "run"
    corpus.mkdir(); out.mkdir()
    base = ["a", "b", "c", "d", " "]
    two = ["".join(q) for q in itertools.product(base, repeat=2)]
    three = ["".join(q) for q in itertools.product(base, repeat=3)]
    units = SubwordUnits(base + two + three[:70])
    upath = str(corpus / "units.txt")
    units.save(upath)
    _, char2ind = _read_alphabet(upath)
    ds = SyntheticSpeech(16, char2ind, n_feats=20, max_chars=4, seed=1)
    lm = build_unit_lm(str(corpus), upath, order=3, train_dataset=ds)
    lpath = str(corpus / "unit_lm.npz")
    assert os.path.exists(lpath) and lm.vocab == 101 and lm.order == 3
    torch.manual_seed(0)
    torch.save(Seq2Seq(alphabet_size=101, n_feats=20).state_dict(), os.path.join(str(out), "model_best.pth"))
    kw = dict(test_dataset=ds, n_feats=20, units_path=upath, beam_size=4, wide_beam=True, nbest=2)

    def rows():
        return [ln.split("\t") for ln in open(os.path.join(str(out), "nbest.tsv")).read().splitlines()]
    predict(None, None, None, str(out), 8, **kw)
    plain = rows()
    cer, wer = predict(None, None, None, str(out), 8, unit_lm_path=lpath, unit_lm_alpha=0.8, unit_lm_beta=0.5, **kw)
    fused = rows()
    assert np.isfinite(cer) and np.isfinite(wer) and all(len(r) == 5 for r in fused)
    assert [r[2] for r in fused] != [r[2] for r in plain]
    predict(None, None, None, str(out), 8, wide_second_pass=True, rescore_unit_lm_path=lpath, rescore_unit_alpha=0.5,
            rescore_unit_beta=0.1, **kw)
    second = rows()
    assert {int(r[0]) for r in second} == set(range(len(ds))) and all(len(r) == 6 and np.isfinite(float(r[3])) for r in second)
    assert UnitNgramLM.load(lpath).n_ngrams == lm.n_ngrams
    assert all(np.isfinite(float(r[5])) and float(r[5]) <= 0.0 for r in second) and any(float(r[5]) < 0.0 for r in second)
    with pytest.raises(ValueError, match="rescore_unit_lm_path"):
        predict(None, None, None, str(out), 8, rescore_unit_lm_path=lpath, **kw)
