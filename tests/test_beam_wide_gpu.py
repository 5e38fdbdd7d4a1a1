"""The exact prefix beam search over rows of up to 1024 symbols (csrc/beam_wide.hip, ``hipops.ctc_beam_search_wide``) on the MI355X:
lists against the plain-Python oracle of tests/nbest_ref.py on the cases of tests/beam_wide_cases.py, bit-equality with the narrow
workgroup kernel at V <= 64, the counting selection against the threshold list, exact ties straddling 64-symbol boundaries, the
edges of the interface and the wiring into CTCDecoder and model.predict.  Score bounds are those tests/test_nbest_gpu.py holds the
same two arithmetics to: 1e-9 relative for fp64 input (test_exact_path_matches_the_helper), 1e-6 relative for fp32 input
(test_fast_path_matches_the_helper)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_tie_ref as TR  # noqa: E402
import beam_wide_cases as W  # noqa: E402
import nbest_ref as NR  # noqa: E402
from oracle import decode_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = {torch.float64: 1e-9, torch.float32: 1e-6}      # tests/test_nbest_gpu.py: the exact path's bound, the fp32 path's bound
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])


def _rows(nb, b):
    tok, ln, sc = nb.tokens[:, b].cpu().numpy(), nb.lengths[:, b].cpu().numpy(), nb.score[:, b].cpu().numpy()
    return int(nb.count[b]), [list(tok[r, :ln[r]]) for r in range(tok.shape[0])], ln, sc, tok


def _check_list(nb, b, hyps, rel):
    """Utterance b of the device list against the oracle's: count, every rank's tokens and length ==, scores to ``rel`` (inf == inf);
    rows beyond count are length 0 / +inf / zero tokens; every token tail is zero."""
    count, seqs, ln, sc, tok = _rows(nb, b)
    assert count == len(hyps), (b, count, len(hyps))
    for r, (want, wscore) in enumerate(hyps):
        assert seqs[r] == list(want), (b, r)
        assert sc[r] == pytest.approx(wscore, rel=rel), (b, r)
        assert not tok[r, ln[r]:].any()
    for r in range(count, tok.shape[0]):
        assert ln[r] == 0 and sc[r] == np.inf and not tok[r].any(), (b, r)


def _same(a, b):
    """Two CTCNBest, every output word bit for bit (scores as their 64-bit images: -0.0 is not +0.0)."""
    return (torch.equal(a.tokens, b.tokens) and torch.equal(a.lengths, b.lengths) and torch.equal(a.count, b.count)
            and torch.equal(a.score.view(torch.int64), b.score.view(torch.int64)))


def _dev(lp, lens, dtype):
    return torch.from_numpy(np.ascontiguousarray(lp)).to(DEV).to(dtype), torch.from_numpy(lens).to(DEV)


@DTYPES
@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_lists_match_the_reference(case, dtype):
    """Tokens, lengths and count == the oracle's lists at N = min(beam, 16); scores within the arithmetic's bound; with counting=True
    every output word is the same, bit for bit."""
    from policy_gradient_asr_amd import hipops
    T, V, beam, blank, B, seed = case
    lp, lens = W.case_inputs(case)
    x, n = _dev(lp, lens, dtype)
    N = W.list_size(beam)
    nb, frames = hipops.ctc_beam_search_wide(x, n, beam=beam, nbest=N, blank=blank, stats=True)
    assert nb.tokens.shape == (N, B, T) and nb.lengths.shape == (N, B) and nb.score.shape == (N, B) and nb.count.shape == (B,)
    for b, (hyps, gap) in enumerate(W.reference(case)):
        print(f"{W.case_id(case)} b={b} n={int(lens[b])}: gap {gap:.3e}, score[0] {float(nb.score[0, b])!r} reference {hyps[0][1]!r}, "
              f"counting frames {int(frames[b])}")
        _check_list(nb, b, hyps, REL[dtype])
        if lens[b] == 0:
            assert int(nb.count[b]) == 1 and int(nb.lengths[0, b]) == 0 and float(nb.score[0, b]) == 0.0 and np.signbit(float(nb.score[0, b]))
    forced, fframes = hipops.ctc_beam_search_wide(x, n, beam=beam, nbest=N, blank=blank, counting=True, stats=True)
    assert _same(forced, nb)
    assert fframes.tolist() == lens.tolist()                           # every frame of every utterance took the counting selection
    assert all(0 <= f <= t for f, t in zip(frames.tolist(), lens.tolist()))
    # nbest=None: the triple of ctc_beam_search, row 0 of the list
    tok, tl, sc = hipops.ctc_beam_search_wide(x, n, beam=beam, blank=blank)
    assert torch.equal(tok, nb.tokens[0]) and torch.equal(tl, nb.lengths[0]) and torch.equal(sc.view(torch.int64), nb.score[0].view(torch.int64))


@DTYPES
@pytest.mark.parametrize("kind", ["flat", "peaked"])
def test_both_selections_run_and_agree(kind, dtype):
    """Flat rows at V = 1024 overflow the threshold list (out_counting_frames > 0 without the flag), peaked rows never do (== 0);
    both are held to the oracle, and counting=True changes no output word."""
    from policy_gradient_asr_amd import hipops
    lp, lens = W.select_inputs(kind)
    x, n = _dev(lp, lens, dtype)
    kw = dict(beam=W.SELECT_BEAM, nbest=W.list_size(W.SELECT_BEAM), blank=W.SELECT_BLANK)
    nb, frames = hipops.ctc_beam_search_wide(x, n, stats=True, **kw)
    print(f"{kind}: counting frames {frames.tolist()} of {lens.tolist()}")
    for b, (hyps, gap) in enumerate(W.select_reference(kind)):
        assert gap >= W.GAP_MIN
        _check_list(nb, b, hyps, REL[dtype])
    if kind == "flat":
        assert all(f > 0 for f in frames.tolist())
    else:
        assert frames.tolist() == [0] * len(lens)
    forced, fframes = hipops.ctc_beam_search_wide(x, n, counting=True, stats=True, **kw)
    assert _same(forced, nb) and fframes.tolist() == lens.tolist()


NARROW = [c for c in NR.NOLM_CASES if c[1] in (29, 64)][:6] + [(60, 2, 16, 0, 0), (40, 2, 5, 1, 1)]


@DTYPES
@pytest.mark.parametrize("case", NARROW, ids=lambda c: "-".join(str(x) for x in c))
def test_narrow_rows_equal_the_narrow_kernel_bit_for_bit(case, dtype):
    """V in {2, 29, 64}, finite log-probs: every output word of the wide entry == ctc_beam_search_nbest without ``fast`` (the
    workgroup-per-utterance kernel), for the default and the counting selection."""
    from policy_gradient_asr_amd import hipops
    T, V, beam, blank, seed = case
    lp, lens = NR.nolm_case_inputs(case)
    assert np.isfinite(lp).all()
    x, n = _dev(lp, lens, dtype)
    N = NR.list_size(beam)
    want = hipops.ctc_beam_search_nbest(x, n, beam=beam, nbest=N, blank=blank)
    assert _same(hipops.ctc_beam_search_wide(x, n, beam=beam, nbest=N, blank=blank), want)
    assert _same(hipops.ctc_beam_search_wide(x, n, beam=beam, nbest=N, blank=blank, counting=True), want)
    assert _same(hipops.ctc_beam_search_wide(x, n, beam=beam, nbest=N, blank=blank, collapse=True),
                 hipops.ctc_beam_search_nbest(x, n, beam=beam, nbest=N, blank=blank, collapse=True))


@DTYPES
@pytest.mark.parametrize("case", W.TIE_CASES, ids=TR.case_id)
def test_exact_ties_follow_the_reference(case, dtype):
    """Twin columns straddling 64-symbol boundaries: lists == beam_tie_ref.tie_search (score descending, first touch among equals),
    for both selections."""
    from policy_gradient_asr_amd import hipops
    T, V, blank, pairs, beam, order, alpha, beta, seed = TR.parse(case)
    lp, lens, _ = TR.case_inputs(case)
    x, n = _dev(lp, lens, dtype)
    N = TR.list_size(beam)
    for counting in (False, True):
        nb = hipops.ctc_beam_search_wide(x, n, beam=beam, nbest=N, blank=blank, counting=counting)
        for b, (hyps, rep) in enumerate(TR.reference(case)):
            _check_list(nb, b, hyps, REL[dtype])


def test_edges():
    """A strided view (stride_b != V), lengths=None, nbest beyond the final beam, a column of -inf, collapse, two calls on one stream
    sharing the workspace."""
    from policy_gradient_asr_amd import hipops
    case = W.CASES[3]                                                   # V = 257, beam 5
    T, V, beam, blank, B, seed = case
    lp, lens = W.case_inputs(case)
    x, n = _dev(lp, lens, torch.float32)
    want = hipops.ctc_beam_search_wide(x, n, beam=beam, nbest=beam, blank=blank)
    # strided: the rows sit in a wider buffer
    big = torch.full((T, B, V + 37), float("nan"), device=DEV)
    big[:, :, 5:5 + V] = x
    view = big[:, :, 5:5 + V]
    assert view.stride(1) == V + 37 and view.stride(2) == 1
    assert _same(hipops.ctc_beam_search_wide(view, n, beam=beam, nbest=beam, blank=blank), want)
    # lengths=None: every utterance has T frames
    full = hipops.ctc_beam_search_wide(x, None, beam=beam, nbest=beam, blank=blank)
    every = hipops.ctc_beam_search_wide(x, torch.full((B,), T, dtype=torch.int32, device=DEV), beam=beam, nbest=beam, blank=blank)
    assert _same(full, every) and torch.equal(full.tokens[:, 0], want.tokens[:, 0])
    # two calls back to back on one stream share one workspace: the second starts from a clean trie
    a = hipops.ctc_beam_search_wide(x, n, beam=beam, nbest=beam, blank=blank)
    b2 = hipops.ctc_beam_search_wide(x.flip(1).contiguous(), n.flip(0).contiguous(), beam=beam, nbest=beam, blank=blank)
    torch.cuda.synchronize()
    assert _same(a, want)
    assert torch.equal(b2.tokens.flip(1), want.tokens) and torch.equal(b2.score.flip(1).view(torch.int64), want.score.view(torch.int64))
    # collapse: each row is the plain row with adjacent duplicates removed
    coll = hipops.ctc_beam_search_wide(x, n, beam=beam, nbest=beam, blank=blank, collapse=True)
    assert torch.equal(coll.score.view(torch.int64), want.score.view(torch.int64)) and torch.equal(coll.count, want.count)
    for b in range(B):
        _, seqs, _, _, _ = _rows(want, b)
        _, cseqs, cln, _, ctok = _rows(coll, b)
        for r in range(beam):
            assert cseqs[r] == [v for i, v in enumerate(seqs[r]) if i == 0 or v != seqs[r][i - 1]] and not ctok[r, cln[r]:].any()
    # nbest larger than the final beam: V = 2, T = 1 leaves two entries
    two = torch.log(torch.tensor([[[0.25, 0.75]]], dtype=torch.float64, device=DEV))
    nb = hipops.ctc_beam_search_wide(two, None, beam=8, nbest=8, blank=0)
    assert nb.count.tolist() == [2] and nb.lengths[:, 0].tolist() == [1, 0] + [0] * 6 and int(nb.tokens[0, 0, 0]) == 1
    assert nb.score[:2, 0].tolist() == pytest.approx([-np.log(0.75), -np.log(0.25)], rel=1e-12) and bool(torch.isinf(nb.score[2:, 0]).all())
    # a column of -inf log-probs (probability zero in every frame): the ranks of finite score are the oracle's
    T2, V2, beam2 = 12, 70, 16
    rng = np.random.default_rng(3)
    probs = np.exp(rng.normal(size=(T2, V2)) * 2.0)
    probs[:, 66] = 0.0
    probs /= probs.sum(axis=1, keepdims=True)
    hyps, gap = NR.nbest_prefix_beam_search(probs, beam_size=beam2, blank=0, nbest=beam2)
    finite = [h for h in hyps if np.isfinite(h[1])]
    with np.errstate(divide="ignore"):
        z = torch.from_numpy(np.log(probs)).to(DEV).view(T2, 1, V2)
    nb = hipops.ctc_beam_search_wide(z, None, beam=beam2, nbest=beam2, blank=0)
    count, seqs, ln, sc, tok = _rows(nb, 0)
    assert count == len(hyps) and len(finite) >= 2
    for r, (wt, ws) in enumerate(finite):
        assert seqs[r] == list(wt) and sc[r] == pytest.approx(ws, rel=1e-9)
    assert all(66 not in s for s in seqs[:len(finite)])


def test_decoder_wiring():
    """CTCDecoder(wide_search=True).decode on a 300-symbol probability matrix == oracle.decode_ref.prefix_beam_search; the nbest form is
    the oracle's list; decode_batch(nbest=4) is the hipops call; rows of <= 64 symbols make the calls they always made."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    T, V, beam = 30, 300, 8
    rng = np.random.default_rng(12)
    logits = rng.normal(size=(T, V)) * rng.choice([0.3, 2.0, 5.0], size=(T, 1))
    logits[:, 0] += 1.5
    probs = np.exp(logits - logits.max(axis=1, keepdims=True))
    probs /= probs.sum(axis=1, keepdims=True)
    dec = CTCDecoder(list(range(V)), wide_search=True)
    want = decode_ref.prefix_beam_search(probs, beam_size=beam, blank=0)
    got = dec.decode(probs, beam_size=beam, blank=0)
    assert got[0] == tuple(want[0]) and got[1] == pytest.approx(want[1], rel=1e-9)
    hyps, gap = NR.nbest_prefix_beam_search(probs, beam_size=beam, blank=0, nbest=4)
    lst = dec.decode(probs, beam_size=beam, blank=0, nbest=4)
    assert gap > 1e-9 and [h[0] for h in lst] == [h[0] for h in hyps] and [h[1] for h in lst] == [pytest.approx(h[1], rel=1e-9) for h in hyps]
    case = W.CASES[4]                                                   # V = 300, beam 16
    lp, lens = W.case_inputs(case)
    x, n = _dev(lp, lens, torch.float32)
    assert _same(dec.decode_batch(x, n, beam_size=16, blank=299, nbest=4), hipops.ctc_beam_search_wide(x, n, beam=16, nbest=4, blank=299))
    one = dec.decode_batch(x, n, beam_size=16, blank=299)
    ref1 = hipops.ctc_beam_search_wide(x, n, beam=16, blank=299)
    assert all(torch.equal(a, b) for a, b in zip(one, ref1))
    with pytest.raises(ValueError, match="greed"):
        CTCDecoder(list(range(V))).decode_batch(x, n, beam_size=16, blank=299)
    # narrow rows: the decoder with the flag makes the call it makes without it
    ncase = NR.NOLM_CASES[1]
    nlp, nlens = NR.nolm_case_inputs(ncase)
    y, m = _dev(nlp, nlens, torch.float32)
    a = CTCDecoder(list(range(29)), wide_search=True).decode_batch(y, m, beam_size=5)
    b = CTCDecoder(list(range(29))).decode_batch(y, m, beam_size=5)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_predict_with_the_wide_beam(tmp_path, capsys):
    """model.predict(units_path=, beam_size=4, wide_beam=True, nbest=2) on SyntheticSpeech over 100 units: predicted.txt and nbest.tsv
    are written, the rates are finite and the oracle error rate over units is printed; without wide_beam the refusal stands, and the
    options the wide lists do not take yet are refused by name."""
    import itertools
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.model import Seq2Seq, _read_alphabet, predict
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
    torch.manual_seed(0)
    torch.save(Seq2Seq(alphabet_size=101, n_feats=20).state_dict(), os.path.join(str(out), "model_best.pth"))      # an untrained model: the wiring is the subject
    kw = dict(test_dataset=ds, n_feats=20, units_path=upath)
    with pytest.raises(ValueError, match="beam_size=0"):
        predict(None, None, None, str(out), 8, beam_size=4, **kw)
    for name, arg in (("lm_path", dict(lm_path="x.npz")), ("rescore_lm_path", dict(rescore_lm_path="x.npz", nbest=2)),
                      ("rescore_word_lm_path", dict(rescore_word_lm_path="x.npz", nbest=2)), ("mbr", dict(mbr=True, nbest=2)),
                      ("error_report", dict(error_report=True))):
        with pytest.raises(ValueError, match=name):
            predict(None, None, None, str(out), 8, beam_size=4, wide_beam=True, **arg, **kw)
    capsys.readouterr()
    cer, wer = predict(None, None, None, str(out), 8, beam_size=4, wide_beam=True, nbest=2, **kw)
    assert np.isfinite(cer) and np.isfinite(wer)
    assert "Oracle unit error rate (2-best)" in capsys.readouterr().out
    assert len(open(os.path.join(str(out), "predicted.txt")).read().splitlines()) >= len(ds)
    rows = [ln.split("\t") for ln in open(os.path.join(str(out), "nbest.tsv")).read().splitlines()]
    assert {int(r[0]) for r in rows} == set(range(len(ds))) and all(len(r) == 5 and r[3] == "" and np.isfinite(float(r[2])) for r in rows)
    assert all(int(r[1]) in (0, 1) for r in rows)
    cer1, wer1 = predict(None, None, None, str(out), 8, beam_size=4, wide_beam=True, **kw)
    assert np.isfinite(cer1) and np.isfinite(wer1)
