"""Word n-gram LM and lexicon fusion on the device (csrc/beam.hip WORDS = true) against the plain-Python search with
``lm.WordFusion``'s bonus and finalisation (tests/word_fusion_ref.py): every N-best row token for token, scores to 1e-6 relative on
the fp32 path (cases with a margin condition: tests/test_word_fusion_cpu.py) and 1e-9 on the exact path; zero weights against the
search without a model, bit for bit; the decoder's routing; the refusals by name."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as L  # noqa: E402
import word_fusion_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _kw(case, fusion):
    T, V, beam, blank, d, order, pen, finalize, eos, alpha, beta, seed = case
    return dict(beam=beam, nbest=W.nbest_of(case), blank=blank, fusion=fusion, alpha=alpha, beta=beta, finalize=finalize, eos=eos)


def _compare(case, nb, rel, tag):
    ref = W.case_reference(case)
    N = W.nbest_of(case)
    ntok, nlen, nsc, ncnt = nb.tokens.cpu().numpy(), nb.lengths.cpu().numpy(), nb.score.cpu().numpy(), nb.count.cpu().numpy()
    for b in range(W.B):
        hyps, gap = ref[b]["hyps"], ref[b]["gap"]
        print(f"{tag} {W.case_id(case)} b={b}: score {float(nsc[0, b])!r} reference {hyps[0][1]!r} gap {gap:.3e}")
        assert int(ncnt[b]) == len(hyps), b
        for r, (want, wscore) in enumerate(hyps):
            assert list(ntok[r, b, :nlen[r, b]]) == list(want), (b, r)
            assert not ntok[r, b, nlen[r, b]:].any()
            assert (nsc[r, b] == wscore) if np.isinf(wscore) else (nsc[r, b] == pytest.approx(wscore, rel=rel)), (b, r)
        for r in range(len(hyps), N):
            assert nlen[r, b] == 0 and nsc[r, b] == np.inf and not ntok[r, b].any()


@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_fast_path_matches_the_fused_reference(case):
    """fp32 log-probs with ragged lengths (0 and 1 among them): tokens and lengths of every N-best row == the helper's, scores 1e-6
    relative; the 1-best form (nbest = 1) is row 0 of the list, bit for bit."""
    from policy_gradient_asr_amd import hipops
    lp, lens, fusion = W.case_inputs(case)
    d_lp, d_len = torch.from_numpy(lp).to(DEV), torch.from_numpy(lens).to(DEV)
    nb = hipops.ctc_beam_search_words(d_lp, d_len, **_kw(case, fusion))
    _compare(case, nb, 1e-6, "fp32")
    one = hipops.ctc_beam_search_words(d_lp, d_len, **dict(_kw(case, fusion), nbest=1))
    assert torch.equal(one.tokens[0], nb.tokens[0]) and torch.equal(one.lengths[0], nb.lengths[0]) and torch.equal(one.score[0], nb.score[0])


@pytest.mark.parametrize("case", [W.CASES[i] for i in W.EXACT_CASES], ids=W.case_id)
def test_exact_path_matches_the_fused_reference(case):
    """The same inputs as fp64 on the exact instantiation: tokens identical, scores 1e-9 relative."""
    from policy_gradient_asr_amd import hipops
    lp, lens, fusion = W.case_inputs(case)
    d_lp, d_len = torch.from_numpy(lp).double().to(DEV), torch.from_numpy(lens).to(DEV)
    _compare(case, hipops.ctc_beam_search_words(d_lp, d_len, **_kw(case, fusion)), 1e-9, "exact")


@pytest.mark.parametrize("case", [W.CASES[i] for i in W.ZERO_CASES], ids=W.case_id)
@pytest.mark.parametrize("f64", [False, True])
def test_zero_weights_are_the_unfused_search_bit_for_bit(case, f64):
    """alpha = beta = oov_penalty = 0, eos off, finalize on and off: every output word (tokens, lengths, scores, count) equals
    ``ctc_beam_search_nbest``'s -- and the weights do reach the kernel."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.lm import WordFusion
    lp, lens, fusion = W.case_inputs(case)
    T, V, beam, blank, d = case[:5]
    zero = WordFusion(fusion.word_lm, V, d, blank=blank, oov_penalty=0.0)
    d_lp, d_len = torch.from_numpy(lp).to(DEV), torch.from_numpy(lens).to(DEV)
    if f64:
        d_lp = d_lp.double()
    N = W.nbest_of(case)
    a = hipops.ctc_beam_search_nbest(d_lp, d_len, beam=beam, nbest=N, blank=blank)
    for finalize in (True, False):
        z = hipops.ctc_beam_search_words(d_lp, d_len, beam=beam, nbest=N, blank=blank, fusion=zero, alpha=0.0, beta=0.0,
                                         finalize=finalize, eos=False)
        assert all(torch.equal(x, y) for x, y in zip(a, z)), finalize
    w = hipops.ctc_beam_search_words(d_lp, d_len, **_kw(case, fusion))
    assert not torch.equal(a.score, w.score)


def test_decoder_routes_through_the_fused_call():
    """``CTCDecoder(fused_word_lm=)``: decode_batch's triple is row 0 of the hipops call (finalize and eos on), its nbest= form the
    list; ``decode`` on probabilities is the fp64 call's row 0; a ``WordNgramLM`` is made the same ``WordFusion``."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    case = W.CASES[0]
    T, V, beam, blank, d, order, pen, finalize, eos, alpha, beta, seed = case
    lp, lens, fusion = W.case_inputs(case)
    d_lp, d_len = torch.from_numpy(lp).to(DEV), torch.from_numpy(lens).to(DEV)
    alphabet = [chr(ord("a") + s) for s in range(V)]
    want = hipops.ctc_beam_search_words(d_lp, d_len, beam=beam, nbest=4, blank=0, fusion=fusion, alpha=alpha, beta=beta)
    for given in (fusion, fusion.word_lm):
        dec = CTCDecoder(alphabet, fused_word_lm=given, fused_word_alpha=alpha, fused_word_beta=beta, word_delimiter=d, oov_penalty=pen)
        tok, tl, sc = dec.decode_batch(d_lp, d_len, beam_size=beam)
        assert torch.equal(tok, want.tokens[0]) and torch.equal(tl, want.lengths[0]) and torch.equal(sc, want.score[0])
        nb = dec.decode_batch(d_lp, d_len, beam_size=beam, nbest=4)
        assert all(torch.equal(x, y) for x, y in zip(nb, want))
    probs = np.exp(lp[:, 0].astype(np.float64))
    one = hipops.ctc_beam_search_words(torch.from_numpy(np.log(probs)).view(T, 1, V).to(DEV), None, beam=beam, nbest=3, blank=0,
                                       fusion=fusion, alpha=alpha, beta=beta)
    y, score = dec.decode(probs, beam_size=beam)
    assert list(y) == one.tokens[0, 0, :one.lengths[0, 0]].tolist() and score == float(one.score[0, 0])
    rows = dec.decode(probs, beam_size=beam, nbest=3)
    assert [list(r[0]) for r in rows] == [one.tokens[r, 0, :one.lengths[r, 0]].tolist() for r in range(3)]
    assert list(y) == list(W.case_reference(case)[0]["hyps"][0][0])


def test_the_edge_of_the_lds_check():
    """beam 128 x V 32 -- 4096 candidates, the largest sort the 160 KB check admits -- runs with the word state in LDS; beam 128 x
    V 64 is refused up front as it is without a model."""
    from policy_gradient_asr_amd import _lib, hipops
    from policy_gradient_asr_amd.lm import WordFusion
    T, Bn, beam = 12, 2, 128
    rng = np.random.default_rng(3)
    for V, ok in ((32, True), (64, False)):
        lm, _ = W.random_word_lm(V, 0, 1, 3, 5)
        zero, fusion = WordFusion(lm, V, 1), WordFusion(lm, V, 1, oov_penalty=-1.0)
        lp = torch.from_numpy(L.log_softmax32(rng.normal(size=(T, Bn, V)) * 2.0)).to(DEV)
        if not ok:
            with pytest.raises(_lib.PgasrError, match="status 4"):
                hipops.ctc_beam_search_words(lp, None, beam=beam, nbest=4, fusion=fusion, alpha=0.5, beta=0.5)
            continue
        a = hipops.ctc_beam_search_nbest(lp, None, beam=beam, nbest=beam)
        z = hipops.ctc_beam_search_words(lp, None, beam=beam, nbest=beam, fusion=zero, eos=False)
        assert all(torch.equal(x, y) for x, y in zip(a, z))
        w = hipops.ctc_beam_search_words(lp, None, beam=beam, nbest=beam, fusion=fusion, alpha=0.5, beta=0.5)
        assert torch.isfinite(w.score).all() and not torch.equal(a.score, w.score)
        assert bool((w.score[1:] >= w.score[:-1]).all())                 # the final ranking: totals descending


def test_refusals_raise_by_name_on_device_tensors():
    """Every refusal of the host layer names its option, with the log-probs already on the device."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    from policy_gradient_asr_amd.lm import CharNgramLM, HotwordBias, WordFusion
    case = W.CASES[0]
    V, blank, d = case[1], case[3], case[4]
    lp, lens, fusion = W.case_inputs(case)
    d_lp = torch.from_numpy(lp).to(DEV)
    alphabet = [chr(ord("a") + s) for s in range(V)]
    with pytest.raises(ValueError, match="fusion"):
        hipops.ctc_beam_search_words(d_lp, None, fusion=fusion.word_lm)
    with pytest.raises(ValueError, match="fusion"):
        hipops.ctc_beam_search_words(d_lp, None, blank=2, fusion=fusion)
    with pytest.raises(ValueError, match="fusion"):
        hipops.ctc_beam_search_words(d_lp[:, :, :V - 1], None, fusion=fusion)
    for name in ("alpha", "beta"):
        with pytest.raises(ValueError, match=name):
            hipops.ctc_beam_search_words(d_lp, None, fusion=fusion, **{name: float("nan")})
    lm = CharNgramLM(L.random_table(V, 2, 0, 0), 2)
    for name, kw in (("lm", dict(lm=lm)), ("hotwords", dict(hotwords=HotwordBias([(2, 3)], V))), ("fast_lm", dict(fast_lm=True)),
                     ("wide_search", dict(wide_search=True))):
        with pytest.raises(ValueError, match=name):
            CTCDecoder(alphabet, fused_word_lm=fusion, **kw)
    dec = CTCDecoder(alphabet, fused_word_lm=fusion)
    with pytest.raises(ValueError, match="lm"):
        dec.decode_batch(d_lp, None, lm=lm)
    with pytest.raises(ValueError, match="fast_lm"):
        dec.decode_batch(d_lp, None, fast_lm=True)
    with pytest.raises(ValueError, match="hotwords"):
        dec.set_hotwords([alphabet[2] + alphabet[3]])
    with pytest.raises(ValueError, match="fused_word_lm"):
        dec.decode_batch(torch.zeros(4, 1, 70, device=DEV), None)
    with pytest.raises(ValueError, match="fused_word_lm"):
        CTCDecoder(list(range(70)), fused_word_lm=fusion)
    with pytest.raises(ValueError, match="oov_penalty"):
        WordFusion(fusion.word_lm, V, d, blank=blank, oov_penalty=0.5)
