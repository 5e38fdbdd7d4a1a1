"""The tie rule of the CTC beam searches (csrc/beam.hip) on the device: "candidate order, prefix merging and the stable descending sort
(ties -> first insertion) follow the reference exactly" (include/pgasr_hip.h, A7 / A7-LM / A7-NBEST), held on inputs whose exact ties
DECIDE the output.  The cases of tests/beam_tie_ref.py have twin symbol columns, so prefixes related by swapping the twins are bit-equal
in every implementation, and tests/test_beam_ties_cpu.py asserts that on every utterance of >= 33 frames another tie rule gives another
list while every non-zero margin leaves the fp32 kernels their room.  Every entry point that takes a case's shape runs on the same fp32
log-probs (fp64: their exact widening); every utterance equals the helper's first-touch list -- tokens, lengths and counts exactly, scores
to the bounds the tests of the same entry points use (1e-6 relative for fp32 input, 1e-9 for fp64) -- and the bitwise identities between
the entry points hold on tied input too."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_tie_ref as TR  # noqa: E402
import nbest_ref as NR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL32, REL64 = 1e-6, 1e-9


def _lm_of(case):
    T, V, blank, pairs, beam, order, alpha, beta, seed = TR.parse(case)
    if not order:
        return {}
    from policy_gradient_asr_amd.lm import CharNgramLM
    return dict(lm=CharNgramLM(TR.case_inputs(case)[2].copy(), order, blank=blank), lm_alpha=alpha, lm_beta=beta)      # the shared table is read-only


def _device_inputs(case):
    lp, lens, _ = TR.case_inputs(case)
    lp32 = torch.from_numpy(lp.copy()).to(DEV)
    return lp32, lp32.double(), torch.from_numpy(lens).to(DEV)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _check_1best(what, case, out, rel):
    """Every utterance of a (tokens, lengths, score) triple against row 0 of the helper's first-touch list."""
    tok, tl, score = (t.cpu().numpy() for t in out)
    lens = TR.lengths_of(case[0])
    for b, (hyps, rep) in enumerate(TR.reference(case)):
        want, wscore = hyps[0]
        got = list(tok[b, :tl[b]])
        print(f"{what} {TR.case_id(case)} b={b} n={int(lens[b])}: score {float(score[b])!r} reference {wscore!r}; {rep['tied']} tied ranks, "
              f"{rep['cut_ties']} tied cuts, first frame another rule shows: {rep['diverge']}; got the last-touch winner: "
              f"{tuple(got) == rep['last_touch'][0][0] != want}")
        assert got == list(want), (what, b)
        assert float(score[b]) == pytest.approx(wscore, rel=rel), (what, b)
        assert not tok[b, tl[b]:].any()
        if lens[b] == 0:
            assert tl[b] == 0 and score[b] == 0.0 and np.signbit(score[b])


def _check_list(what, case, nb, rel):
    """Every utterance of a CTCNBest against the helper's first-touch list: count, every row's tokens and length in list order, scores;
    rows beyond count and token tails as documented."""
    lens = TR.lengths_of(case[0])
    for b, (hyps, rep) in enumerate(TR.reference(case)):
        tok, ln, sc = nb.tokens[:, b].cpu().numpy(), nb.lengths[:, b].cpu().numpy(), nb.score[:, b].cpu().numpy()
        got = [tuple(tok[r, :ln[r]]) for r in range(int(nb.count[b]))]
        wrong = [r for r, (g, h) in enumerate(zip(got, hyps)) if g != h[0]]
        print(f"{what} {TR.case_id(case)} b={b} n={int(lens[b])}: {len(hyps)} ranks, {rep['tied']} tied ranks, {rep['cut_ties']} tied cuts, "
              f"score[0] {sc[0]!r} reference {hyps[0][1]!r}; rows that differ: {wrong}; is the last-touch list: "
              f"{got == [h[0] for h in rep['last_touch']] != [h[0] for h in hyps]}")
        assert int(nb.count[b]) == len(hyps), (what, b)
        for r, (want, wscore) in enumerate(hyps):
            assert got[r] == want, (what, b, r)
            assert sc[r] == pytest.approx(wscore, rel=rel), (what, b, r)
            assert not tok[r, ln[r]:].any()
        for r in range(len(hyps), tok.shape[0]):
            assert ln[r] == 0 and sc[r] == np.inf and not tok[r].any(), (what, b, r)


def _row0_is(nb, one):
    return torch.equal(nb.tokens[0], one[0]) and torch.equal(nb.lengths[0], one[1]) and torch.equal(nb.score[0], one[2])


@pytest.mark.parametrize("case", TR.NOLM, ids=TR.case_id)
def test_1_best_without_lm(case):
    """ctc_beam_search: the single-wave kernel (beam <= 16), the workgroup kernel with fast arithmetic (generic=True) and the exact fp64
    workgroup kernel; a second call gives the same bits."""
    from policy_gradient_asr_amd import hipops
    T, V, blank, pairs, beam, order, alpha, beta, seed = TR.parse(case)
    lp32, lp64, lens = _device_inputs(case)
    runs = [("workgroup fp32", lambda: hipops.ctc_beam_search(lp32, lens, beam=beam, blank=blank, generic=True), REL32),
            ("workgroup fp64", lambda: hipops.ctc_beam_search(lp64, lens, beam=beam, blank=blank), REL64)]
    if case in TR.SINGLE_WAVE:
        runs.insert(0, ("single-wave", lambda: hipops.ctc_beam_search(lp32, lens, beam=beam, blank=blank), REL32))
    for what, run, rel in runs:
        out = run()
        _check_1best(what, case, out, rel)
        assert _same(out, run()), what


@pytest.mark.parametrize("case", TR.NOLM, ids=TR.case_id)
def test_n_best_without_lm(case):
    """ctc_beam_search_nbest at N = min(beam, 16): fast=True on fp32 (the single-wave kernel, beam <= 16), without fast on fp32 and on
    fp64.  Row 0 of the fast list is ctc_beam_search(...) bit for bit, row 0 of the fp32 list without fast is
    ctc_beam_search(generic=True), row 0 of the fp64 list is the fp64 search; a second call gives the same bits."""
    from policy_gradient_asr_amd import hipops
    T, V, blank, pairs, beam, order, alpha, beta, seed = TR.parse(case)
    lp32, lp64, lens = _device_inputs(case)
    kw = dict(beam=beam, blank=blank)
    N = TR.list_size(beam)
    runs = [("workgroup fp32 list", lambda: hipops.ctc_beam_search_nbest(lp32, lens, nbest=N, **kw), REL32,
             lambda: hipops.ctc_beam_search(lp32, lens, generic=True, **kw)),
            ("workgroup fp64 list", lambda: hipops.ctc_beam_search_nbest(lp64, lens, nbest=N, **kw), REL64,
             lambda: hipops.ctc_beam_search(lp64, lens, **kw))]
    if case in TR.SINGLE_WAVE:
        runs.insert(0, ("single-wave list", lambda: hipops.ctc_beam_search_nbest(lp32, lens, nbest=N, fast=True, **kw), REL32,
                        lambda: hipops.ctc_beam_search(lp32, lens, **kw)))
    for what, run, rel, one in runs:
        nb = run()
        _check_list(what, case, nb, rel)
        assert _row0_is(nb, one()), what
        assert _same(nb, run()), what


@pytest.mark.parametrize("case", TR.LM, ids=TR.case_id)
def test_with_a_symmetric_lm(case):
    """LM fusion with a table invariant under the twins' swap: ctc_beam_search(lm=) on fp32 and fp64 (the workgroup LM kernels),
    ctc_beam_search(lm=, fast_lm=True) (the single-wave LM kernel: beam_lm_single_wave_ok asserted), and the three lists; row 0 of each
    list is the 1-best of the same form bit for bit; a second call gives the same bits."""
    from policy_gradient_asr_amd import hipops
    T, V, blank, pairs, beam, order, alpha, beta, seed = TR.parse(case)
    lp32, lp64, lens = _device_inputs(case)
    kw = dict(beam=beam, blank=blank, **_lm_of(case))
    N = TR.list_size(beam)
    assert hipops.beam_lm_single_wave_ok(T, V, beam, False, order)
    for what, lp, extra, rel in (("workgroup LM fp32", lp32, {}, REL32), ("workgroup LM fp64", lp64, {}, REL64),
                                 ("single-wave LM", lp32, dict(fast_lm=True), REL32)):
        one = hipops.ctc_beam_search(lp, lens, **extra, **kw)
        _check_1best(what, case, one, rel)
        nb = hipops.ctc_beam_search_nbest(lp, lens, nbest=N, **extra, **kw)
        _check_list(what + " list", case, nb, rel)
        assert _row0_is(nb, one), what
        assert _same(one, hipops.ctc_beam_search(lp, lens, **extra, **kw)), what
        assert _same(nb, hipops.ctc_beam_search_nbest(lp, lens, nbest=N, **extra, **kw)), what


def _collapsed(tokens):
    from policy_gradient_asr_amd.CTCdecoder import collapse_fn
    return [ord(ch) - 48 for ch in collapse_fn("".join(chr(48 + int(x)) for x in tokens))]


# (kernel, case, fp64 input, arguments of ctc_beam_search, arguments of ctc_beam_search_nbest that take the same kernel)
COLLAPSE = [("single-wave", TR.GROUPS["B"][2], False, dict(), dict(fast=True)),
            ("workgroup fp32", TR.GROUPS["G"][1], False, dict(generic=True), dict()),
            ("workgroup fp64", TR.GROUPS["E"][1], True, dict(), dict()),
            ("workgroup LM fp32", TR.GROUPS["L"][0], False, dict(), dict()),
            ("workgroup LM fp64", TR.GROUPS["L"][5], True, dict(), dict()),
            ("single-wave LM", TR.GROUPS["L"][5], False, dict(fast_lm=True), dict(fast_lm=True))]


@pytest.mark.parametrize("what,case,f64,one_kw,list_kw", COLLAPSE, ids=[c[0].replace(" ", "-") for c in COLLAPSE])
def test_collapse_follows_the_tied_winner(what, case, f64, one_kw, list_kw):
    """collapse=True on one tied case per kernel: the score and collapse_fn of the un-collapsed winner -- the tie changes nothing
    downstream; the list's rows likewise."""
    from policy_gradient_asr_amd import hipops
    T, V, blank, pairs, beam, order, alpha, beta, seed = TR.parse(case)
    lp32, lp64, lens = _device_inputs(case)
    lp = lp64 if f64 else lp32
    kw = dict(beam=beam, blank=blank, **_lm_of(case))
    plain = hipops.ctc_beam_search(lp, lens, **one_kw, **kw)
    coll = hipops.ctc_beam_search(lp, lens, collapse=True, **one_kw, **kw)
    _check_1best(what, case, plain, REL64 if f64 else REL32)
    assert torch.equal(plain[2], coll[2])
    shorter = 0
    for b in range(TR.TIE_B):
        got, winner = coll[0][b, :coll[1][b]].tolist(), plain[0][b, :plain[1][b]].tolist()
        assert got == _collapsed(winner) and not coll[0][b, coll[1][b]:].any(), (what, b)
    N = TR.list_size(beam)
    nb = hipops.ctc_beam_search_nbest(lp, lens, nbest=N, **list_kw, **kw)
    cnb = hipops.ctc_beam_search_nbest(lp, lens, nbest=N, collapse=True, **list_kw, **kw)
    assert _row0_is(nb, plain) and _row0_is(cnb, coll) and torch.equal(nb.score, cnb.score) and torch.equal(nb.count, cnb.count)
    for b in range(TR.TIE_B):
        for r in range(int(nb.count[b])):
            row = nb.tokens[r, b, :nb.lengths[r, b]].tolist()
            assert cnb.tokens[r, b, :cnb.lengths[r, b]].tolist() == _collapsed(row), (what, b, r)
            assert not cnb.tokens[r, b, cnb.lengths[r, b]:].any()
            shorter += len(_collapsed(row)) < len(row)
    assert shorter > 0                                                   # some hypothesis did have an adjacent duplicate


def test_the_drop_in_decoder_on_tied_probabilities():
    """CTCDecoder.decode(np.exp(lp)) -- the fp64 drop-in, which logs the probabilities itself: the 1-best and the list of the search
    under the helper on the same probabilities (its own log, like the decoder's), and the hypotheses of the case's own list (the round
    trip moves each word by a rounding, the same on twin columns, far below the margins)."""
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    case = TR.GROUPS["B"][1]
    T, V, blank, pairs, beam, order, alpha, beta, seed = TR.parse(case)
    lp, lens, _ = TR.case_inputs(case)
    dec = CTCDecoder(list(range(V)))
    for b, (hyps, rep) in enumerate(TR.reference(case)):
        n = int(lens[b])
        probs = np.exp(lp[:n, b].astype(np.float64))
        got, score = dec.decode(probs, beam_size=beam, blank=blank)
        lst = dec.decode(probs, beam_size=beam, blank=blank, nbest=beam)
        if n == 0:
            assert (got, score) == ((), 0.0) and lst == [((), 0.0)]
            continue
        want = NR.nbest_prefix_beam_search(probs, beam_size=beam, blank=blank, nbest=beam)[0]
        print(f"drop-in {TR.case_id(case)} b={b} n={n}: score {score!r} reference {want[0][1]!r}; {rep['tied']} tied ranks, {rep['cut_ties']} tied cuts")
        assert [h[0] for h in want] == [h[0] for h in hyps]
        assert got == want[0][0] and score == pytest.approx(want[0][1], rel=REL64)
        assert [g[0] for g in lst] == [h[0] for h in want]
        assert [g[1] for g in lst] == [pytest.approx(h[1], rel=REL64) for h in want]
