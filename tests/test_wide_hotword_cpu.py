"""Hotword biasing inside the wide beam search, without a GPU: the qualifying conditions of the shared cases
(tests/wide_hotword_ref.py), the argument checks of pgasr_ctc_beam_search_wide_bias on host memory (nothing could have run) and the
keywords and refusals of the host layer, each before a device is touched."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_hotword_ref as WH  # noqa: E402

from policy_gradient_asr_amd.lm import HotwordBias  # noqa: E402


@pytest.fixture(autouse=True)
def _the_wide_entry_takes_a_bias():
    """Everything below is about hipops.ctc_beam_search_wide(bias=): without that keyword the cases qualify for nothing."""
    from policy_gradient_asr_amd import hipops
    assert "bias" in inspect.signature(hipops.ctc_beam_search_wide).parameters


# ---------------------------------------------------------------- the shared cases
def test_the_cases_cover_the_shapes():
    V = {c[1] for c in WH.CASES}
    assert {65, 300, 1000, 1024} <= V and V & {128, 129}
    assert {c[2] for c in WH.CASES} >= {1, 5, 16, 32, 128}
    first, last = {c[3] == 0 for c in WH.CASES}, {c[3] == c[1] - 1 for c in WH.CASES}
    assert first == last == {False, True} and any(0 < c[3] < c[1] - 1 for c in WH.CASES)
    orders = sorted(c[5] for c in WH.CASES if c[5])
    assert len(orders) >= 2 and 3 in orders and orders[-1] in (4, 5)
    assert any(c[0] <= 6 and c[1] == 1024 and c[2] == 128 for c in WH.CASES)
    assert {c[7] for c in WH.CASES} == {"mixed", "overlap", "flat", "big"}
    assert any(WH.CASES[i][5] for i in WH.EXACT_CASES) and any(WH.CASES[i][7] == "overlap" for i in WH.EXACT_CASES)
    assert len(WH.EXACT_CASES) >= 3 and len(WH.ZERO_CASES) == 3 and any(WH.CASES[i][5] for i in WH.ZERO_CASES)
    a, b, c = WH.OVERLAP_SYMBOLS
    assert a // 64 != b // 64 != c // 64 and a // 64 != c // 64


@pytest.mark.parametrize("case", WH.CASES, ids=WH.case_id)
def test_gpu_cases_qualify(case):
    """Every utterance's decision gap is at least GAP_MIN at N = list_size(beam); at least one utterance's 1-best differs from its
    unbiased 1-best; at least half the non-empty utterances' best rows have B(y) != 0; the overlap case has a negative bonus on a
    best row's path; the big automaton has at least 12000 states."""
    fig = WH.figures(case)
    print(WH.case_id(case), fig)
    assert fig["gap"] >= WH.GAP_MIN
    assert fig["changed"] >= 1
    assert 2 * fig["nonzero"] >= fig["live"]
    if case[7] == "overlap":
        assert fig["lowest"] < 0
        assert {(63, 63, 64), (63, 64), (64, 63, 63, 129)} <= set(WH.case_inputs(case)[2].phrases)
    if case[7] == "big":
        assert fig["states"] >= 12000
        assert fig["states"] * case[1] <= 1 << 24                 # near the limit of table words, not past it
    assert WH.qualifies(case, fig)


# ---------------------------------------------------------------- ABI
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, 1, 3, 4


def _search_args(T=6, B=2, V=70, beam=4, flags=0, nbest=3):
    """Valid arguments of the wide search up to and including stream, all in HOST memory and with NO workspace: whatever passed the
    checks would stop at PGASR_ERR_WORKSPACE before any HIP call."""
    keep = [np.zeros((T, B, V), dtype=np.float32), np.zeros((nbest, B, T), dtype=np.int32), np.zeros((nbest, B), dtype=np.int32),
            np.zeros((nbest, B), dtype=np.float64), np.zeros(B, dtype=np.int32), np.zeros(V * 4, dtype=np.int64)]
    lp, tok, tl, sc, cnt, table = (a.ctypes.data for a in keep)
    return keep, table, [lp, 0, B * V, V, None, T, B, V, beam, 0, flags, nbest, tok, T, tl, sc, cnt, None, None, 0, None]


def _host_tables(V, blank=0, order=2):
    """A pgasr_unit_lm_tables over host arrays that passes the model's checks."""
    from policy_gradient_asr_amd import _lib
    states, succ = np.zeros((V + 2, 4), dtype=np.int32), np.zeros((V - 1, 4), dtype=np.int32)
    t = _lib.UnitLMTables()
    t.states, t.succ = states.ctypes.data, succ.ctypes.data
    t.order, t.vocab, t.blank, t.n_states, t.n_succ, t.start = order, V, blank, V + 2, V - 1, 1 + blank
    return (states, succ, t), ctypes.byref(t)


def test_entry_point_refuses_bad_bias_arguments():
    from policy_gradient_asr_amd import _lib
    lib = _lib.load()
    fn = lib.pgasr_ctc_beam_search_wide_bias
    V = 70
    keep, table, args = _search_args(V=V)
    nolm = (None, 0.0, 0.0)
    assert fn(*args, *nolm, table, 4, 1.0) == WORKSPACE                    # a good table passes the checks (and stops at the workspace)
    assert fn(*args, *nolm, None, 0, 1.0) == lib.pgasr_ctc_beam_search_wide(*args) == WORKSPACE       # no table, no model: the call without
    assert fn(*args, *nolm, None, 4, 1.0) == INVALID                       # a null table with states
    assert fn(*args, *nolm, table, 0, 1.0) == INVALID                      # bias_states < 1
    assert fn(*args, *nolm, table, -3, 1.0) == INVALID
    assert fn(*args, *nolm, table, (1 << 24) // V + 1, 1.0) == INVALID     # bias_states * V > 2^24
    assert fn(*args, *nolm, table, (1 << 24) // V, 1.0) == WORKSPACE
    for w in (float("nan"), float("inf"), -float("inf")):
        assert fn(*args, *nolm, table, 4, w) == INVALID                    # a weight that is not finite
    # the order: A7-WIDE's own checks come first ...
    for flags in (2, 8, 16, 64):
        fkeep, ftable, fargs = _search_args(V=V, flags=flags)
        assert fn(*fargs, *nolm, ftable, 4, 1.0) == INVALID                # unknown flag bits
        assert fn(*fargs, *nolm, None, 4, 1.0) == INVALID
    wkeep, wtable, wargs = _search_args(V=1025)
    assert fn(*wargs, *nolm, wtable, 4, 1.0) == UNSUPPORTED                # V > 1024 before the bias is looked at
    assert fn(*wargs, *nolm, None, 4, 1.0) == UNSUPPORTED
    bkeep, btable, bargs = _search_args(V=V, beam=129, nbest=3)
    assert fn(*bargs, *nolm, None, 4, 1.0) == UNSUPPORTED                  # beam > 128 likewise
    nkeep, ntable, nargs = _search_args(V=V)
    nargs[11] = 5                                                          # nbest > beam
    assert fn(*nargs, *nolm, ntable, 4, 1.0) == INVALID
    # ... then the model's, then the bias', then the workspace
    held, tables = _host_tables(V)
    assert fn(*args, tables, 0.5, 0.1, table, 4, 1.0) == WORKSPACE
    assert fn(*args, tables, 0.5, 0.1, None, 0, 0.0) == lib.pgasr_ctc_beam_search_wide_lm(*args, tables, 0.5, 0.1) == WORKSPACE
    assert fn(*args, tables, float("nan"), 0.1, table, 4, 1.0) == INVALID
    assert fn(*args, tables, 0.5, 0.1, None, 4, 1.0) == INVALID
    assert fn(*args, tables, 0.5, 0.1, table, 4, float("inf")) == INVALID
    held[2].order = 6                                                      # the model's UNSUPPORTED comes before the bias' INVALID
    assert fn(*args, tables, 0.5, 0.1, None, 4, 1.0) == UNSUPPORTED
    assert lib.pgasr_ctc_beam_search_wide_lm(*args, tables, 0.5, 0.1) == UNSUPPORTED
    del keep, fkeep, wkeep, bkeep, nkeep, held


def test_new_symbol_is_exported():
    from policy_gradient_asr_amd import _lib
    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "policy_gradient_asr_amd",
                                   "libpgasr_hip.so"))
    assert hasattr(lib, "pgasr_ctc_beam_search_wide_bias")
    res, argtypes = _lib.SIGNATURES["pgasr_ctc_beam_search_wide_bias"]
    lm_res, lm_argtypes = _lib.SIGNATURES["pgasr_ctc_beam_search_wide_lm"]
    assert res is lm_res and list(argtypes[:len(lm_argtypes)]) == list(lm_argtypes)
    assert list(argtypes[len(lm_argtypes):]) == [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
    lib.pgasr_abi_version.restype = ctypes.c_int
    assert lib.pgasr_abi_version() == 7


# ---------------------------------------------------------------- host layer
def test_keyword_defaults_and_positions():
    from policy_gradient_asr_amd import hipops, model
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    sig = inspect.signature(hipops.ctc_beam_search_wide).parameters
    assert list(sig)[-2:] == ["bias", "bias_weight"] and sig["bias"].default is None and sig["bias_weight"].default == 0.0
    assert list(sig)[-5:-2] == ["unit_lm", "lm_alpha", "lm_beta"]
    sig = inspect.signature(CTCDecoder.__init__).parameters
    assert list(sig)[-3:] == ["wide_hotwords", "hotwords", "hotword_weight"] and sig["wide_hotwords"].default is False
    sig = inspect.signature(model.predict).parameters
    assert list(sig)[-4:] == ["wide_hotwords", "hotwords_path", "hotword_weight", "hotword_boost"]
    assert sig["wide_hotwords"].default is False
    assert "wide_hotwords" in CTCDecoder.rescore.__doc__.split("bias:")[1]
    assert "A7-WIDE-BIAS" in hipops.ctc_beam_search_wide.__doc__


def test_refusals_by_name_touch_no_device(tmp_path):
    """Every refusal raises a ValueError that names the option, on CPU tensors; a call that gets past the checks raises PgasrError:
    there is no CPU path."""
    from policy_gradient_asr_amd import _lib, hipops, model
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    V = 70
    hb = HotwordBias([(1, 2)], V)
    lp = torch.zeros(4, 1, V)
    units = list(range(V))
    with pytest.raises(ValueError, match="wide_hotwords"):
        CTCDecoder(units, wide_hotwords=True, hotwords=hb)
    with pytest.raises(ValueError, match="wide_hotwords"):
        CTCDecoder(units, wide_hotwords=True)
    # only a HotwordBias, never raw tensors
    for raw in (torch.zeros(V * 2, 2, dtype=torch.int32), (hb.next, hb.bonus)):
        with pytest.raises(ValueError, match="HotwordBias"):
            hipops.ctc_beam_search_wide(lp, None, bias=raw, bias_weight=1.0)
    # a bias of another vocabulary or blank
    for other in (HotwordBias([(1, 2)], V + 1), HotwordBias([(1, 2)], V, blank=3)):
        with pytest.raises(ValueError, match="bias"):
            hipops.ctc_beam_search_wide(lp, None, bias=other)
        with pytest.raises(ValueError, match="bias"):
            hipops.ctc_beam_search_wide(lp, None, nbest=2, bias=other, bias_weight=1.0)
        dec = CTCDecoder(units, wide_search=True, wide_hotwords=True, hotwords=other)
        with pytest.raises(ValueError, match="hotwords"):
            dec.decode_batch(lp, None)
        with pytest.raises(ValueError, match="hotwords"):
            dec.decode_batch(lp, None, nbest=2)
        with pytest.raises(ValueError, match="hotwords"):
            CTCDecoder(units, wide_search=True, wide_hotwords=True, hotwords=other, device="cpu").decode(np.full((4, V), 1 / V))
    # without wide_hotwords the wide search keeps refusing hotwords; set_hotwords works as before on a decoder that has it
    with pytest.raises(ValueError, match="hotwords"):
        CTCDecoder(units, wide_search=True, hotwords=hb).decode_batch(lp, None)
    dec = CTCDecoder(units, wide_search=True, wide_hotwords=True)
    assert dec.hotwords is None and dec.wide_hotwords
    dec.set_hotwords(hb, 2.0)
    assert dec.hotwords is hb and dec.hotword_weight == 2.0
    with pytest.raises(ValueError, match="hotwords"):
        dec.set_hotwords("ab")
    with pytest.raises(ValueError, match="hotword_weight"):
        dec.set_hotwords(hb, float("nan"))
    # past the checks: the library is asked, and it has no CPU path
    with pytest.raises(_lib.PgasrError):
        hipops.ctc_beam_search_wide(lp, None, bias=hb, bias_weight=1.0)
    with pytest.raises(_lib.PgasrError):
        dec.decode_batch(lp, None, nbest=2)
    # predict
    hot = tmp_path / "hot.txt"; hot.write_text("ab\n")
    wide = tmp_path / "units.txt"; wide.write_text("".join(f"{chr(0x100 + i)}\n" for i in range(80)))
    common = dict(test_dataset=[], n_feats=8, wide_hotwords=True)
    with pytest.raises(ValueError, match="^wide_beam:"):
        model.predict(None, None, None, str(tmp_path), 2, units_path=str(wide), hotwords_path=str(hot), **common)
    with pytest.raises(ValueError, match="^units_path:"):
        model.predict(None, None, str(wide), str(tmp_path), 2, wide_beam=True, hotwords_path=str(hot), **common)
    with pytest.raises(ValueError, match="^hotwords_path:"):
        model.predict(None, None, None, str(tmp_path), 2, units_path=str(wide), wide_beam=True, **common)
