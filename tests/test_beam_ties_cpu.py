"""The tied-input cases of tests/beam_tie_ref.py are what tests/test_beam_ties_gpu.py takes them for (no device needed): twin columns
and symmetric tables are bit-exact, every non-zero margin of a ranking decision leaves the fp32 kernels their room (beam_lm_ref.GAP_MIN),
exact ties do occur -- at the cut too --, they do decide the output (the last-touch rule gives another list), and the helper's first-touch
lists are those of the searches the other tests already trust.  These are conditions on the inputs: a seed that fails one is replaced
in beam_tie_ref.GROUPS, never excused here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as R  # noqa: E402
import beam_tie_ref as TR  # noqa: E402
import nbest_ref as NR  # noqa: E402
from oracle import decode_ref  # noqa: E402


def test_the_case_list_covers_what_it_names():
    """The groups hold the shapes, blanks, pairs and beams they are there for; every case is listed once."""
    def shapes(g):
        return {(c[0], c[1], c[2], c[3]) for c in TR.GROUPS[g]}

    def beams(g):
        return sorted(c[4] for c in TR.GROUPS[g])

    assert shapes("A") == {(70, 29, 0, ((1, 2), (5, 20)))} and beams("A") == [1, 2, 5, 16]
    assert shapes("B") == {(70, 29, 3, ((1, 2), (5, 20)))} and beams("B") == [2, 5, 16]
    assert shapes("C") == {(70, 29, 28, ((1, 2), (5, 20)))} and beams("C") == [5, 16]
    assert shapes("D") == {(70, 40, 0, ((1, 2), (5, 33)))} and beams("D") == [2, 16]
    assert shapes("E") == {(70, 64, 63, ((0, 40), (5, 62)))} and beams("E") == [5, 16]
    assert shapes("F") == {(40, 4, 0, ((1, 2),))} and beams("F") == [5, 16]
    assert {c[:5] for c in TR.GROUPS["G"]} == {(30, 29, 0, ((1, 2), (5, 6)), 40), (33, 12, 5, ((1, 2), (7, 8)), 32)}
    assert {c[:8] for c in TR.GROUPS["L"]} == {s + (k, n, 0.7, 0.5) for g, n in (("A", 3), ("B", 2), ("D", 2)) for s in shapes(g) for k in (5, 16)}
    assert len(set(TR.CASES)) == len(TR.CASES) == 23
    assert all(TR.parse(c)[4] <= 16 for c in TR.SINGLE_WAVE + TR.LM) and all(TR.parse(c)[4] > 16 for c in TR.GROUPS["G"])


@pytest.mark.parametrize("case", TR.CASES, ids=TR.case_id)
def test_inputs_are_symmetric(case):
    """Twin columns are bit-identical fp32 with no zero probability, blank is no twin, lengths are [T, T - T // 3, 33, 1, 0] capped
    at T, the table is invariant under each swap and CharNgramLM takes it as it is."""
    T, V, blank, pairs, beam, order, alpha, beta, seed = TR.parse(case)
    lp, lens, table = TR.case_inputs(case)
    assert lp.shape == (T, TR.TIE_B, V) and lens.tolist() == [min(n, T) for n in (T, T - T // 3, 33, 1, 0)]
    TR.check_pairs(V, blank, pairs)
    TR.assert_twin_columns(lp, pairs)
    others = [s for s in range(V) if s not in [x for p in pairs for x in p[1:]]]
    assert len({lp[:, :, s].tobytes() for s in others}) == len(others)             # pairs only: no third identical column
    assert (table is None) == (order == 0)
    if table is not None:
        from policy_gradient_asr_amd.lm import CharNgramLM
        TR.assert_table_symmetric(table, pairs)
        assert not np.array_equal(table, R.random_table(V, order, blank, seed + 17))
        lm = CharNgramLM(table, order, blank=blank)
        assert np.array_equal(lm.table, table)


@pytest.mark.parametrize("case", TR.CASES, ids=TR.case_id)
def test_ties_are_exact_decisive_and_everything_else_has_a_margin(case):
    """Every utterance: every non-zero margin among the first beam + 1 ranks of every frame >= GAP_MIN.  Every utterance of >= 33
    frames: the list at N = min(beam, 16) (beam 1: the 1-best) differs under the last-touch rule.  The case: some 1-best differs, some
    frame's cut is an exact tie."""
    T, V, blank, pairs, beam, order, alpha, beta, seed = TR.parse(case)
    lens = TR.lengths_of(T)
    for b, (hyps, rep) in enumerate(TR.reference(case)):
        print(f"{TR.case_id(case)} b={b} n={int(lens[b])}: margin {rep['margin']:.3e}, {rep['tied']} tied adjacent ranks, {rep['cut_ties']} tied cuts, "
              f"first frame the last-touch search leaves the beam: {rep['diverge']}, 1-best differs: {hyps[0][0] != rep['last_touch'][0][0]}")
        assert rep["gap"] >= rep["margin"] or rep["gap"] == 0.0        # the list's own decisions are among the reported ones
    assert TR.conditions(case) == []


@pytest.mark.parametrize("case", TR.CASES, ids=TR.case_id)
def test_first_touch_lists_are_those_of_the_trusted_searches(case):
    """The helper's lists == nbest_ref.nbest_prefix_beam_search without the optional arguments, tokens and scores exactly; without a
    table row 0 == decode_ref.prefix_beam_search and beam_lm_ref.fused_prefix_beam_search(table=None)."""
    T, V, blank, pairs, beam, order, alpha, beta, seed = TR.parse(case)
    lp, lens, table = TR.case_inputs(case)
    ref = TR.reference(case)
    for b in range(TR.TIE_B):
        n = int(lens[b])
        hyps = ref[b][0]
        if n == 0:
            assert hyps == [((), -0.0)] and np.signbit(hyps[0][1])
            continue
        logp = lp[:n, b].astype(np.float64)
        plain, gap = NR.nbest_prefix_beam_search(logp=logp, table=table, order=order, alpha=alpha, beta=beta, beam_size=beam, blank=blank,
                                                 nbest=TR.list_size(beam))
        assert hyps == plain and gap == ref[b][1]["gap"]
        assert len(hyps) == min(TR.list_size(beam), len(ref[b][1]["frames"][-1]))
        if table is None:
            assert hyps[0] == R.fused_prefix_beam_search(logp=logp, table=None, beam_size=beam, blank=blank)[:2]
            with np.errstate(under="ignore"):
                probs = np.exp(logp)
            # the oracle takes probabilities and logs them: given the same probabilities the search under the helper is the oracle
            # exactly; the round trip moves every word by a rounding, the same on twin columns and far below the margins, so the
            # oracle's hypothesis is also the one of the case's own log-probs
            want = decode_ref.prefix_beam_search(probs, beam_size=beam, blank=blank)
            assert NR.nbest_prefix_beam_search(probs, beam_size=beam, blank=blank, report={})[0][0] == want
            assert hyps[0][0] == want[0] and hyps[0][1] == pytest.approx(want[1], rel=1e-12)


def test_the_optional_arguments_leave_the_plain_search_alone():
    """On an un-tied shared case of nbest_ref the report changes neither list nor gap, and the last-touch rule gives the same list."""
    case = NR.NOLM_CASES[5]
    lp, lens = NR.nolm_case_inputs(case)
    T, V, beam, blank, seed = case
    logp = lp[:, 0].astype(np.float64)
    kw = dict(logp=logp, beam_size=beam, blank=blank, nbest=beam)
    rep = {}
    plain = NR.nbest_prefix_beam_search(**kw)
    assert NR.nbest_prefix_beam_search(report=rep, **kw) == plain
    assert NR.nbest_prefix_beam_search(last_touch=True, **kw) == plain
    assert rep["tied"] == 0 and rep["cut_ties"] == 0 and 0 < rep["margin"] <= plain[1] and len(rep["frames"]) == T
