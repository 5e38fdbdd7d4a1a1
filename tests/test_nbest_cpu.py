"""N-best output of the CTC beam search and second-pass rescoring on a GPU-less host: the list helper of tests/nbest_ref.py against
the oracle and against the fused helper, the new entry points' export, binding and refusals (all before any HIP call), the host
layer's refusals and unchanged defaults, and the margin condition of every case the fp32 device path is compared on."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as R  # noqa: E402
import nbest_ref as NR  # noqa: E402
from oracle import decode_ref  # noqa: E402

HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
INVALID_ARG, WORKSPACE, UNSUPPORTED = 1, 3, 4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def test_helper_rank_0_is_the_oracle_and_the_fused_helper(golden_dir):
    z = np.load(os.path.join(golden_dir, "beam_inputs.npz"))
    done = 0
    for key in z.files:
        probs = z[key]
        if probs.ndim != 2:
            continue
        T, V = probs.shape
        beam = 5 if T > 100 else 16
        want, nll = decode_ref.prefix_beam_search(probs, beam_size=beam)
        hyps, gap = NR.nbest_prefix_beam_search(probs, beam_size=beam, nbest=beam)
        assert hyps[0] == (want, nll) and 1 <= len(hyps) <= beam
        scores = [s for _, s in hyps]
        assert scores == sorted(scores) and len({h for h, _ in hyps}) == len(hyps)      # ranked, and every prefix once
        assert NR.nbest_prefix_beam_search(probs, beam_size=beam, nbest=3)[0] == hyps[:3]
        tab = R.random_table(V, 2, 0, seed=done)
        got, score, _ = R.fused_prefix_beam_search(probs, tab, 2, 0.6, 0.4, beam_size=beam)
        lm_hyps, lm_gap = NR.nbest_prefix_beam_search(probs, tab, 2, 0.6, 0.4, beam_size=beam, nbest=4)
        assert lm_hyps[0] == (got, score)
        done += 1
    assert done == 20


def test_helper_gap_counts_the_final_ranks():
    """Two frames, three symbols: the final beam's adjacent margins enter the gap up to rank N-1 against rank N, and no further."""
    probs = np.array([[0.5, 0.3, 0.2], [0.6, 0.25, 0.15]])
    hyps, _ = NR.nbest_prefix_beam_search(probs, beam_size=8, nbest=8)
    lse = [-s for _, s in hyps]
    for n in (1, 2, 3):
        g = NR.nbest_prefix_beam_search(probs, beam_size=8, nbest=n)[1]
        assert g == min(lse[r] - lse[r + 1] for r in range(n))
    assert NR.nbest_prefix_beam_search(probs, beam_size=8, nbest=1)[1] == R.fused_prefix_beam_search(probs, beam_size=8)[2]


def test_new_symbols_exported_and_bound_abi_stays_7(lib):
    from policy_gradient_asr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("pgasr_ctc_beam_search_nbest", "pgasr_nbest_rescore"):
        assert hasattr(lib, name)
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1])
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    lm = re.search(r"\bpgasr_ctc_beam_search_lm\s*\(([^)]*)\)", src)
    assert len(_lib.SIGNATURES["pgasr_ctc_beam_search_nbest"][1]) == lm.group(1).count(",") + 1 + 3      # nbest, tok_stride, out_count
    assert _lib.SIGNATURES["pgasr_ctc_beam_search_nbest"][1][-4:] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double]
    assert int(re.search(r"#define PGASR_ABI_VERSION (\d+)", src).group(1)) == 7 and lib.pgasr_abi_version() == 7


P = 0x1000          # fake pointers: every call below must return before dereferencing or launching anything


def _nbest(lib, T=10, V=29, beam=5, nbest=3, stride=10, tokens=P, length=P, score=P, count=P, ws=None, ws_bytes=0,
           table=None, order=0, alpha=0.5, beta=0.5, lp=P, blank=0):
    return lib.pgasr_ctc_beam_search_nbest(lp, 0, 64, 64, None, T, 1, V, beam, blank, 0, nbest, tokens, stride, length, score, count,
                                           ws, ws_bytes, None, table, order, alpha, beta)


def test_nbest_refusals_need_no_device(lib):
    assert _nbest(lib, nbest=0) == INVALID_ARG and _nbest(lib, nbest=-1) == INVALID_ARG
    assert _nbest(lib, nbest=6) == INVALID_ARG                       # nbest > beam
    assert _nbest(lib, stride=9) == INVALID_ARG                      # tok_stride < T
    for name in ("tokens", "length", "score", "count"):
        assert _nbest(lib, **{name: None}) == INVALID_ARG, name
    # the search's own checks, the LM's and the workspace's are those of pgasr_ctc_beam_search_lm
    assert _nbest(lib, lp=None) == INVALID_ARG and _nbest(lib, T=0, stride=0) == INVALID_ARG and _nbest(lib, blank=29) == INVALID_ARG
    assert _nbest(lib, V=65) == UNSUPPORTED and _nbest(lib, beam=129, nbest=1) == UNSUPPORTED
    assert _nbest(lib, table=None, order=2) == INVALID_ARG and _nbest(lib, table=P, order=0) == INVALID_ARG
    assert _nbest(lib, table=P, order=2, alpha=float("nan")) == INVALID_ARG
    assert _nbest(lib, table=P, order=6) == UNSUPPORTED and _nbest(lib, V=64, table=P, order=5) == UNSUPPORTED
    assert _nbest(lib, V=65, nbest=0) == UNSUPPORTED                 # .. and come first
    assert _nbest(lib, table=P, order=6, nbest=0) == UNSUPPORTED
    # a well-formed request gets as far as the workspace check (still before any HIP call)
    assert _nbest(lib) == WORKSPACE and _nbest(lib, nbest=5, stride=11) == WORKSPACE and _nbest(lib, nbest=1) == WORKSPACE
    assert _nbest(lib, table=P, order=5) == WORKSPACE
    need = lib.pgasr_beam_workspace_bytes(10, 1, 29, 5)
    assert need > 0 and _nbest(lib, ws=P, ws_bytes=need - 1) == WORKSPACE
    assert _nbest(lib, ws=P, ws_bytes=need, nbest=0) == INVALID_ARG


def _rescore(lib, N=4, B=2, V=29, stride=10, blank=0, table=P, order=2, w=1.0, a=0.5, b=0.5, tokens=P, length=P, count=P, am=P,
             lm=P, total=P, out_order=P):
    return lib.pgasr_nbest_rescore(tokens, stride, length, count, am, N, B, V, blank, table, order, w, a, b, lm, total, out_order, None)


def test_rescore_refusals_need_no_device(lib):
    for name in ("tokens", "length", "count", "am", "lm", "total", "out_order"):
        assert _rescore(lib, **{name: None}) == INVALID_ARG, name
    assert _rescore(lib, N=0) == INVALID_ARG and _rescore(lib, B=0) == INVALID_ARG and _rescore(lib, stride=0) == INVALID_ARG
    assert _rescore(lib, blank=29) == INVALID_ARG and _rescore(lib, blank=-1) == INVALID_ARG
    assert _rescore(lib, table=None, order=2) == INVALID_ARG and _rescore(lib, table=P, order=0) == INVALID_ARG
    assert _rescore(lib, order=-1) == INVALID_ARG
    for bad in (float("nan"), float("inf")):
        assert _rescore(lib, w=bad) == INVALID_ARG and _rescore(lib, a=bad) == INVALID_ARG and _rescore(lib, b=bad) == INVALID_ARG
    assert _rescore(lib, N=129) == UNSUPPORTED and _rescore(lib, V=65) == UNSUPPORTED
    assert _rescore(lib, order=6) == UNSUPPORTED and _rescore(lib, V=64, order=5) == UNSUPPORTED      # oversized tables: refused
    assert _rescore(lib, V=2, order=26) == UNSUPPORTED


def test_host_layer_refuses_cpu_tensors_and_mismatched_lms():
    import torch
    from policy_gradient_asr_amd import hipops, metrics, _lib
    from policy_gradient_asr_amd.lm import CharNgramLM
    with pytest.raises(_lib.PgasrError):
        hipops.ctc_beam_search_nbest(torch.zeros(3, 1, 5), None, beam=4, nbest=2)
    with pytest.raises(_lib.PgasrError):
        hipops.ctc_beam_search_nbest(torch.zeros(3, 1, 5), None, beam=4, nbest=2, lm=CharNgramLM(R.random_table(5, 2, 0, 0), 2))
    tok, ln = torch.zeros(2, 1, 4, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(_lib.PgasrError):
        hipops.nbest_rescore(tok, ln, torch.ones(1, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.float64), 5)
    nb = hipops.CTCNBest(tok, ln, torch.zeros(2, 1, dtype=torch.float64), torch.ones(1, dtype=torch.int32))
    assert nb._fields == ("tokens", "lengths", "score", "count")
    with pytest.raises(_lib.PgasrError):
        metrics.nbest_oracle(torch.zeros(1, 3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), nb)
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder, NBestRescored
    assert NBestRescored._fields == ("order", "total", "am", "lm_logp", "best_tokens", "best_len", "skipped")
    with pytest.raises(ValueError):
        CTCDecoder(list("abcd")).rescore(torch.zeros(3, 1, 5), None, nb, acoustic="viterbi")
    with pytest.raises(_lib.PgasrError):
        CTCDecoder(list("abcd")).rescore(torch.zeros(3, 1, 5), None, nb, acoustic="first_pass")


def test_defaults_keep_their_signatures():
    from policy_gradient_asr_amd import model
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    for fn in (CTCDecoder.decode, CTCDecoder.decode_batch):
        sig = inspect.signature(fn)
        assert list(sig.parameters)[-1] == "nbest" and sig.parameters["nbest"].default is None
    assert list(inspect.signature(CTCDecoder.decode).parameters)[:4] == ["self", "probs", "beam_size", "blank"]
    assert inspect.signature(CTCDecoder.decode).parameters["beam_size"].default == 100
    assert inspect.signature(CTCDecoder.decode_batch).parameters["beam_size"].default == 5
    sig = inspect.signature(model.predict)
    assert [sig.parameters[k].default for k in ("nbest", "rescore_lm_path", "rescore_alpha", "rescore_beta")] == [1, None, 0.0, 0.0]
    # T = 0 needs no device: the pair as before, and a one-entry list
    assert CTCDecoder(list("ab"), device="cpu").decode(np.zeros((0, 3))) == (tuple(), -0.0)
    assert CTCDecoder(list("ab"), device="cpu").decode(np.zeros((0, 3)), nbest=4) == [(tuple(), -0.0)]


@pytest.mark.parametrize("case", R.FAST_CASES, ids=lambda c: "T%d-V%d-K%d-n%d-b%d-s%d" % (c[0], c[1], c[2], c[3], c[4], c[7]))
def test_margin_condition_of_the_lm_cases(case):
    """The fused cases of beam_lm_ref qualify unchanged as N-best cases at N = min(beam, 16): no frame cut and no final rank
    up to N-1 against N is decided by less than GAP_MIN -- on every utterance, none left out."""
    lp, lens, tab = R.fast_case_inputs(case)
    gaps = [g for _, g in NR.fast_reference(case, True)]
    assert len(gaps) == R.FAST_B == len(lens) and min(gaps) >= R.GAP_MIN, gaps


@pytest.mark.parametrize("case", NR.NOLM_CASES, ids=lambda c: "T%d-V%d-K%d-b%d-s%d" % c)
def test_margin_condition_of_the_no_lm_cases(case):
    lp, lens = NR.nolm_case_inputs(case)
    assert 0 in lens and 1 in lens and np.isfinite(lp).all()
    gaps = [g for _, g in NR.fast_reference(case, False)]
    assert len(gaps) == R.FAST_B == len(lens) and min(gaps) >= R.GAP_MIN, gaps


def test_no_lm_list_covers_the_shapes_of_the_lm_list():
    assert [(c[0], c[1], c[2], c[4]) for c in R.FAST_CASES] == [c[:4] for c in NR.NOLM_CASES]


def test_rescore_ref_on_a_hand_case():
    """Two hypotheses, order 2, V = 3: every term written out."""
    tab = np.log(np.array([[1.0, 0.5, 0.5], [1.0, 0.25, 0.75], [1.0, 0.9, 0.1]], dtype=np.float32)).astype(np.float32)
    tokens = np.array([[[1, 2, 0]], [[2, 2, 1]]]); lengths = np.array([[2], [3]]); count = np.array([2]); am = np.array([[3.0], [2.5]])
    order, total, lm_logp, abs_sum = NR.rescore_ref(tokens, lengths, count, am, 3, 0, tab, 2, 1.0, 2.0, 0.5)
    l0 = float(tab[0, 1]) + float(tab[1, 2]); l1 = float(tab[0, 2]) + float(tab[2, 2]) + float(tab[2, 1])
    assert lm_logp[0, 0] == pytest.approx(l0, rel=1e-15) and lm_logp[1, 0] == pytest.approx(l1, rel=1e-15)
    assert total[0, 0] == pytest.approx(3.0 - 2.0 * l0 - 1.0, rel=1e-15) and total[1, 0] == pytest.approx(2.5 - 2.0 * l1 - 1.5, rel=1e-15)
    assert list(order[0]) == ([0, 1] if total[0, 0] <= total[1, 0] else [1, 0])
    # equal totals keep the list's order; rows beyond count follow; a non-finite am sorts last
    order, total, _, _ = NR.rescore_ref(np.zeros((4, 1, 2), dtype=int), np.zeros((4, 1), dtype=int), np.array([3]),
                                        np.array([[1.0], [np.nan], [1.0], [0.0]]), 3, 0, None, 0, 1.0, 0.0, 0.0)
    assert list(order[0]) == [0, 2, 1, 3] and total[1, 0] == np.inf and total[3, 0] == np.inf
