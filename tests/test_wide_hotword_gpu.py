"""Hotword biasing inside the wide beam search on the MI355X (csrc/beam_wide.hip with a WideBias; include/pgasr_hip.h, A7-WIDE-BIAS):
the biased lists against the plain-Python oracle on the shared cases of tests/wide_hotword_ref.py, the counting selection against the
threshold list, weight 0 against the search without a bias, bit-equality with the narrow workgroup kernel's biased lists, a
constructed near miss that only the bias turns into the phrase, and the wiring into CTCDecoder, rescore and model.predict.  Score
bounds are those of tests/test_unit_lm_gpu.py: 1e-9 relative for fp64 input, 1e-6 relative for fp32 input."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hotword_ref as H  # noqa: E402
import nbest_ref as NR  # noqa: E402
import unit_lm_ref as U  # noqa: E402
import wide_hotword_ref as WH  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = {torch.float64: 1e-9, torch.float32: 1e-6}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])


def _check_list(nb, b, hyps, rel):
    """Utterance b of the device list against the oracle's: count, every rank's tokens and length ==, scores to ``rel``; rows beyond
    count are length 0 / +inf / zero tokens; every token tail is zero."""
    tok, ln, sc = nb.tokens[:, b].cpu().numpy(), nb.lengths[:, b].cpu().numpy(), nb.score[:, b].cpu().numpy()
    assert int(nb.count[b]) == len(hyps), (b, int(nb.count[b]), len(hyps))
    for r, (want, wscore) in enumerate(hyps):
        assert ln[r] == len(want) and list(tok[r, :ln[r]]) == list(want), (b, r)
        assert sc[r] == pytest.approx(wscore, rel=rel), (b, r)
        assert not tok[r, ln[r]:].any()
    for r in range(len(hyps), tok.shape[0]):
        assert ln[r] == 0 and sc[r] == np.inf and not tok[r].any(), (b, r)


def _same(a, b):
    """Two CTCNBest, every output word bit for bit (scores as their 64-bit images)."""
    return (torch.equal(a.tokens, b.tokens) and torch.equal(a.lengths, b.lengths) and torch.equal(a.count, b.count)
            and torch.equal(a.score.view(torch.int64), b.score.view(torch.int64)))


def _dev(lp, lens, dtype):
    return torch.from_numpy(np.array(lp)).to(DEV).to(dtype), torch.from_numpy(np.array(lens)).to(DEV)


def _keywords(case):
    """The keywords of hipops.ctc_beam_search_wide for one shared case, at N = list_size(beam)."""
    T, V, beam, blank, B, order, gamma, kind, seed = case
    kw = dict(beam=beam, nbest=WH.list_size(beam), blank=blank, bias=WH.case_inputs(case)[2], bias_weight=gamma)
    if order:
        kw.update(unit_lm=WH.case_model(case)[1], lm_alpha=WH.ALPHA, lm_beta=WH.BETA)
    return kw


def _biased_lists_match_the_oracle(case, dtype):
    from policy_gradient_asr_amd import hipops
    lp, lens, bias, plain = WH.case_inputs(case)
    x, n = _dev(lp, lens, dtype)
    kw = _keywords(case)
    nb, frames = hipops.ctc_beam_search_wide(x, n, stats=True, **kw)
    for b, (hyps, gap) in enumerate(WH.reference(case)):
        print(f"{WH.case_id(case)} b={b} n={int(lens[b])}: gap {gap:.3e}, score[0] {float(nb.score[0, b])!r} reference {hyps[0][1]!r}, "
              f"counting frames {int(frames[b])}, states {bias.n_states}")
        _check_list(nb, b, hyps, REL[dtype])
    if case[7] == "flat":
        assert any(f > 0 for f in frames.tolist()), frames.tolist()
    forced, fframes = hipops.ctc_beam_search_wide(x, n, counting=True, stats=True, **kw)
    assert _same(forced, nb)
    assert fframes.tolist() == lens.tolist()
    assert all(0 <= f <= t for f, t in zip(frames.tolist(), lens.tolist()))
    tok, tl, sc = hipops.ctc_beam_search_wide(x, n, **dict(kw, nbest=None))
    assert torch.equal(tok, nb.tokens[0]) and torch.equal(tl, nb.lengths[0])
    assert torch.equal(sc.view(torch.int64), nb.score[0].view(torch.int64))


@pytest.mark.parametrize("case", WH.CASES, ids=WH.case_id)
def test_fast_path_matches_the_biased_reference(case):
    """fp32 input: count, every rank's tokens and lengths == the oracle's at N = list_size(beam), scores within 1e-6 relative, rows
    beyond count empty; counting=True changes no output word and its frame counts are the lengths; nbest=None is row 0 bit for bit;
    the flat case overflows the threshold list without being forced."""
    _biased_lists_match_the_oracle(case, torch.float32)


@pytest.mark.parametrize("case", [WH.CASES[i] for i in WH.EXACT_CASES], ids=WH.case_id)
def test_exact_path_matches_the_biased_reference(case):
    """fp64 input, the exact kernels: the same, scores within 1e-9 relative."""
    _biased_lists_match_the_oracle(case, torch.float64)


@DTYPES
@pytest.mark.parametrize("case", [WH.CASES[i] for i in WH.ZERO_CASES], ids=WH.case_id)
def test_zero_weight_is_the_search_without_a_bias_bit_for_bit(case, dtype):
    """bias_weight = 0 with a table: every output word of the call without a bias, for both selections, with and without the LM."""
    from policy_gradient_asr_amd import hipops
    lp, lens, bias, _ = WH.case_inputs(case)
    x, n = _dev(lp, lens, dtype)
    kw = dict(_keywords(case), bias_weight=0.0)
    plain = {k: v for k, v in kw.items() if k not in ("bias", "bias_weight")}
    for counting in (False, True):
        want = hipops.ctc_beam_search_wide(x, n, counting=counting, **plain)
        assert _same(hipops.ctc_beam_search_wide(x, n, counting=counting, **kw), want)
    biased = hipops.ctc_beam_search_wide(x, n, **dict(kw, bias_weight=case[6]))
    assert not torch.equal(biased.tokens, want.tokens)                       # the table is not ignored


@DTYPES
@pytest.mark.parametrize("case", [c for c in H.CASES if c[1] <= 64], ids=H.case_id)
def test_narrow_rows_equal_the_narrow_biased_kernel_bit_for_bit(case, dtype):
    """The V <= 64 cases of hotword_ref: every output word of the wide entry with the bias == ctc_beam_search_nbest(bias=...), the
    workgroup kernel; with an LM the sparse model on the wide side and its dense form on the narrow one; both selections."""
    from policy_gradient_asr_amd import hipops
    T, V, beam, blank, order, gamma, kind, seed = case
    lp, lens, _, bias, _ = H.case_inputs(case)
    x, n = _dev(lp, lens, dtype)
    N = NR.list_size(beam)
    narrow, wide = {}, {}
    if order:
        _, model = U.random_unit_lm(V, order, blank, seed + 17)
        narrow = dict(lm=model.to_dense(), lm_alpha=H.ALPHA, lm_beta=H.BETA)
        wide = dict(unit_lm=model, lm_alpha=H.ALPHA, lm_beta=H.BETA)
    want = hipops.ctc_beam_search_nbest(x, n, beam=beam, nbest=N, blank=blank, bias=bias, bias_weight=gamma, **narrow)
    kw = dict(beam=beam, nbest=N, blank=blank, bias=bias, bias_weight=gamma, **wide)
    assert _same(hipops.ctc_beam_search_wide(x, n, **kw), want)
    assert _same(hipops.ctc_beam_search_wide(x, n, counting=True, **kw), want)


def test_a_near_miss_decodes_to_the_phrase_only_with_the_bias():
    """A (T = 40, V = 300) utterance whose acoustics spell a near miss of a ten-unit phrase (one unit differs, 0.55 against 0.45):
    with the phrase as a hotword the wide search returns the phrase, without it the near miss; decode (fp64), its N-best form and
    decode_batch (fp32) agree, and weight 0 is the acoustic answer."""
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    from policy_gradient_asr_amd.lm import HotwordBias
    V, T = 300, 40
    phrase = (70, 131, 260, 5, 199, 64, 290, 128, 17, 255)
    heard = phrase[:6] + (63,) + phrase[7:]
    probs = 0.002 * np.exp(np.random.default_rng(3).normal(size=(T, V)) * 1.5)
    probs[:, 0] = 1.0
    for k, (c, h) in enumerate(zip(phrase, heard)):
        for t in (4 * k, 4 * k + 1):
            probs[t, 0] = 0.002
            if c == h:
                probs[t, c] = 1.0
            else:
                probs[t, h], probs[t, c] = 0.55, 0.45
    probs /= probs.sum(axis=1, keepdims=True)
    units = list(range(V))
    assert CTCDecoder(units, wide_search=True).decode(probs, beam_size=16)[0] == heard
    dec = CTCDecoder(units, wide_search=True, wide_hotwords=True, hotwords=HotwordBias([phrase], V))
    assert dec.decode(probs, beam_size=16)[0] == phrase
    assert dec.decode(probs, beam_size=16, nbest=4)[0][0] == phrase
    lp = torch.from_numpy(np.log(probs)).float().view(T, 1, V).to(DEV)
    tok, tl, _ = dec.decode_batch(lp, None, beam_size=16)
    assert tuple(tok[0, :tl[0]].tolist()) == phrase
    dec.set_hotwords(None)
    tok, tl, _ = dec.decode_batch(lp, None, beam_size=16)
    assert tuple(tok[0, :tl[0]].tolist()) == heard
    dec.set_hotwords(HotwordBias([phrase], V), 0.0)
    assert dec.decode(probs, beam_size=16)[0] == heard


@pytest.mark.parametrize("case", [WH.CASES[0], WH.CASES[2]], ids=WH.case_id)
def test_decoder_wiring(case):
    """CTCDecoder(wide_search=True, wide_hotwords=True, hotwords=): decode_batch and its nbest form are the hipops call, decode is
    that call on the fp64 log of its probabilities, without and with unit_lm; rescore(acoustic="first_pass") keeps the first pass'
    fused scores in am, acoustic="ctc" has the exact likelihoods there -- what it has for the same list without a bias."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    T, V, beam, blank, B, order, gamma, kind, seed = case
    lp, lens, bias, _ = WH.case_inputs(case)
    kw = _keywords(case)
    lm = {} if not order else dict(unit_lm=kw["unit_lm"], lm_alpha=WH.ALPHA, lm_beta=WH.BETA)
    dec = CTCDecoder(list(range(V)), wide_search=True, wide_hotwords=True, hotwords=bias, hotword_weight=gamma, **lm)
    x, n = _dev(lp, lens, torch.float32)
    nb = dec.decode_batch(x, n, beam_size=beam, blank=blank, nbest=4)
    assert _same(nb, hipops.ctc_beam_search_wide(x, n, **dict(kw, nbest=4)))
    assert not _same(nb, hipops.ctc_beam_search_wide(x, n, **dict(kw, nbest=4, bias=None)))
    assert all(torch.equal(a, b) for a, b in zip(dec.decode_batch(x, n, beam_size=beam, blank=blank),
                                                 hipops.ctc_beam_search_wide(x, n, **dict(kw, nbest=None))))
    probs = np.exp(lp[:, 0].astype(np.float64))
    with np.errstate(divide="ignore"):
        x64 = torch.from_numpy(np.log(probs)).to(DEV).view(T, 1, V)
    want = hipops.ctc_beam_search_wide(x64, None, **dict(kw, nbest=4))
    rows = [(tuple(want.tokens[r, 0, :want.lengths[r, 0]].tolist()), float(want.score[r, 0])) for r in range(int(want.count[0]))]
    assert dec.decode(probs, beam_size=beam, blank=blank, nbest=4) == rows
    assert dec.decode(probs, beam_size=beam, blank=blank) == rows[0]
    first = dec.rescore(x, n, nb, acoustic="first_pass", blank=blank, lm=None)
    assert torch.equal(first.am.view(torch.int64), nb.score.view(torch.int64))
    exact = dec.rescore(x, n, nb, acoustic="ctc", blank=blank, lm=None, max_hyp_len=T)
    plain = CTCDecoder(list(range(V)), wide_search=True).rescore(x, n, nb, acoustic="ctc", blank=blank, lm=None, max_hyp_len=T)
    assert torch.equal(exact.am, plain.am) and not torch.equal(exact.am, nb.score)


def test_predict_with_wide_hotwords(tmp_path):
    """predict(units_path=, wide_beam=True, wide_hotwords=True, hotwords_path=) on SyntheticSpeech over 100 units writes predicted.txt
    from the biased first pass (its first-pass scores differ from the run without the phrases), alone and together with
    unit_lm_path; with wide_second_pass=True and nbest= as well nbest.tsv carries the total and, as its last column, B(y)."""
    import itertools
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.lm import HotwordBias
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
    build_unit_lm(str(corpus), upath, order=3, train_dataset=ds)
    lpath = str(corpus / "unit_lm.npz")
    hot = corpus / "hot.txt"
    lines = ["ab", "dc a", "", "b", "cc", "a", "d", "c"]
    hot.write_text("\n".join(lines) + "\n")
    torch.manual_seed(0)
    torch.save(Seq2Seq(alphabet_size=101, n_feats=20).state_dict(), os.path.join(str(out), "model_best.pth"))
    kw = dict(test_dataset=ds, n_feats=20, units_path=upath, beam_size=4, wide_beam=True)

    def rows():
        return [ln.split("\t") for ln in open(os.path.join(str(out), "nbest.tsv")).read().splitlines()]
    predicted = os.path.join(str(out), "predicted.txt")
    predict(None, None, None, str(out), 8, nbest=2, **kw)
    plain = rows()
    os.remove(predicted)
    cer, wer = predict(None, None, None, str(out), 8, wide_hotwords=True, hotwords_path=str(hot), hotword_weight=2.0, **kw)
    assert np.isfinite(cer) and np.isfinite(wer) and os.path.exists(predicted)
    predict(None, None, None, str(out), 8, wide_hotwords=True, hotwords_path=str(hot), hotword_weight=2.0, nbest=2, **kw)
    fused = rows()
    assert all(len(r) == 5 for r in fused) and [r[2] for r in fused] != [r[2] for r in plain]
    predict(None, None, None, str(out), 8, wide_hotwords=True, hotwords_path=str(hot), hotword_weight=2.0, nbest=2,
            unit_lm_path=lpath, unit_lm_alpha=0.8, unit_lm_beta=0.5, **kw)
    both = rows()
    assert all(len(r) == 5 for r in both) and [r[2] for r in both] != [r[2] for r in fused]
    predict(None, None, None, str(out), 8, wide_hotwords=True, hotwords_path=str(hot), hotword_weight=2.0, nbest=2,
            wide_second_pass=True, **kw)
    second = rows()
    assert {int(r[0]) for r in second} == set(range(len(ds))) and all(len(r) == 6 and np.isfinite(float(r[3])) for r in second)
    assert HotwordBias.from_units(lines, units).n_states > 1
    assert all(np.isfinite(float(r[5])) and float(r[5]) >= 0.0 for r in second) and any(float(r[5]) > 0.0 for r in second)   # B(y) >= 0
