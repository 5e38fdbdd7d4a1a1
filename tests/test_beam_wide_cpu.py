"""The cases of tests/beam_wide_cases.py are what tests/test_beam_wide_gpu.py takes them for, and what the wide search checks on the
host works without a device: every case has the margin the fp32 kernel needs on every utterance, the tie cases do meet exact ties that
decide the output, pgasr_ctc_beam_search_wide refuses bad arguments before any HIP call (through ctypes, no GPU), and
CTCDecoder(wide_search=True) with a language model is refused before a device is asked for.  The margin and tie conditions are conditions
on the inputs: a seed that fails one is replaced in beam_wide_cases, never excused here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_tie_ref as TR  # noqa: E402
import beam_wide_cases as W  # noqa: E402


def test_the_case_list_covers_what_it_names():
    vs = {c[1] for c in W.CASES}
    assert {65, 128, 129, 300, 1023, 1024} <= vs and all(65 <= v <= 1024 for v in vs)
    assert {c[2] for c in W.CASES} == {1, 5, 16, 32, 128}
    blanks = {("first" if c[3] == 0 else "last" if c[3] == c[1] - 1 else "middle") for c in W.CASES}
    assert blanks == {"first", "middle", "last"}
    for c in W.CASES:
        lens = W.case_inputs(c)[1].tolist()
        assert 0 in lens and 1 in lens and max(lens) == c[0]
        assert c[1] <= 300 or (c[0] <= 24 or c[2] <= 16) and c[4] <= 4      # the plain-Python oracle stays within seconds per case
    assert len(set(W.CASES)) == len(W.CASES)


@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_every_case_has_the_margin(case):
    """The smallest decision margin of the reference search is >= GAP_MIN on every utterance; no log-prob is -inf."""
    lp, lens = W.case_inputs(case)
    assert lp.dtype == np.float32 and np.isfinite(lp).all() and lp.shape == (case[0], case[4], case[1])
    for b, (hyps, gap) in enumerate(W.reference(case)):
        print(f"{W.case_id(case)} b={b} n={int(lens[b])}: {len(hyps)} ranks, gap {gap:.3e}")
        assert gap >= W.GAP_MIN, (b, gap)
        assert len(hyps) == (1 if lens[b] == 0 else min(W.list_size(case[2]), len(hyps)))


@pytest.mark.parametrize("kind", ["flat", "peaked"])
def test_the_selection_cases_have_the_margin(kind):
    lp, lens = W.select_inputs(kind)
    assert lp.shape[2] == W.SELECT_V == 1024 and np.isfinite(lp).all()
    if kind == "flat":      # near-uniform: the odd frames' log-probs lie within +-1.2 of ln(1/1024)
        assert np.abs(lp[1::2] - np.log(1.0 / 1024)).max() < 1.2
    for b, (hyps, gap) in enumerate(W.select_reference(kind)):
        print(f"{kind} b={b}: gap {gap:.3e}")
        assert gap >= W.GAP_MIN, (b, gap)


def test_tie_cases_are_tie_cases():
    """Twin pairs straddle 64-symbol boundaries; per case every non-zero margin >= GAP_MIN, exact ties occur among the kept ranks
    (tied > 0) and the last-touch rule gives another list on some utterance; over the cases some cut is an exact tie."""
    cut_ties = 0
    for case in W.TIE_CASES:
        T, V, blank, pairs, beam, order, alpha, beta, seed = TR.parse(case)
        assert V > 64 and any(a // 64 != b // 64 for a, b in pairs)
        lp, lens, table = TR.case_inputs(case)
        TR.assert_twin_columns(lp, pairs)
        assert table is None
        tied = differ = 0
        for b, (hyps, rep) in enumerate(TR.reference(case)):
            print(f"{TR.case_id(case)} b={b} n={int(lens[b])}: margin {rep['margin']:.3e}, {rep['tied']} tied ranks, {rep['cut_ties']} tied cuts, "
                  f"diverges at {rep['diverge']}")
            assert rep["margin"] >= W.GAP_MIN
            tied += rep["tied"]
            cut_ties += rep["cut_ties"]
            differ += [h[0] for h in hyps] != [h[0] for h in rep["last_touch"]]
        assert tied > 0 and differ > 0, (case, tied, differ)
    assert cut_ties > 0


# ---- the C entry's argument checks: before any HIP call, so a host without a GPU runs them ----
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, 1, 3, 4


def _lib():
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def _call(lib, **kw):
    """pgasr_ctc_beam_search_wide with dummy non-NULL pointers that a refused call never reads."""
    a = dict(log_probs=16, is_f64=0, stride_t=0, stride_b=0, lengths=0, T=10, B=2, V=300, beam=8, blank=0, flags=0, nbest=4,
             out_tokens=16, tok_stride=10, out_len=16, out_score=16, out_count=16, frames=0, ws=16, ws_bytes=None, stream=0)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = 0 if a["ws"] == 0 else 1 << 40
    return lib.pgasr_ctc_beam_search_wide(a["log_probs"], a["is_f64"], a["stride_t"], a["stride_b"], a["lengths"], a["T"], a["B"], a["V"],
                                          a["beam"], a["blank"], a["flags"], a["nbest"], a["out_tokens"], a["tok_stride"], a["out_len"],
                                          a["out_score"], a["out_count"], a["frames"], a["ws"], a["ws_bytes"], a["stream"])


def test_the_symbols_are_in_the_signature_table():
    from policy_gradient_asr_amd import _lib
    assert _lib.SIGNATURES["pgasr_beam_wide_workspace_bytes"] == (C.c_size_t, [C.c_int] * 4)
    assert len(_lib.SIGNATURES["pgasr_ctc_beam_search_wide"][1]) == 21
    assert _lib.load().pgasr_abi_version() == 7


def test_workspace_query():
    lib = _lib()
    q = lib.pgasr_beam_wide_workspace_bytes
    for T, B, beam in ((1, 1, 1), (10, 2, 8), (1000, 32, 16), (24, 4, 128)):
        nn = T * beam + 1
        H = 1024
        while H < 2 * nn:
            H *= 2
        pad = lambda n: (n + 255) // 256 * 256      # noqa: E731
        want = pad(B * H * 8) + pad(B * nn * 4)
        assert q(T, B, 1024, beam) == q(T, B, 65, beam) == want      # a hash table of >= 2 slots per node and the node store; V plays no part
    assert q(0, 1, 300, 4) == q(4, 0, 300, 4) == q(4, 1, 300, 0) == 0


def test_arguments_are_checked_before_any_hip_call():
    """The order and the codes of pgasr_ctc_beam_search_nbest: pointers and sizes (INVALID), the limits (UNSUPPORTED), the flags and the
    list's arguments (INVALID), the workspace (WORKSPACE), the node-id width (UNSUPPORTED).  Every call here is refused, so none of the
    dummy pointers is read and no device is needed."""
    lib = _lib()
    for name in ("log_probs", "out_tokens", "out_len", "out_score"):
        assert _call(lib, **{name: 0}) == INVALID, name
    for kw in (dict(T=0), dict(B=0), dict(V=0), dict(beam=0), dict(blank=-1), dict(blank=300), dict(T=-3)):
        assert _call(lib, **kw) == INVALID, kw
    assert _call(lib, V=1025, blank=1024) == UNSUPPORTED and _call(lib, beam=129, nbest=1) == UNSUPPORTED
    assert _call(lib, V=1025, blank=1025) == INVALID                   # blank outside [0, V) comes first
    assert _call(lib, V=1025, nbest=0) == UNSUPPORTED                  # .. and the limits before the list's arguments
    for flags in (2, 4, 8, 16, 64, 1 << 20, 1 | 2, 32 | 8):
        assert _call(lib, flags=flags) == INVALID, flags
    for kw in (dict(nbest=0), dict(nbest=9), dict(tok_stride=9), dict(out_count=0)):
        assert _call(lib, **kw) == INVALID, kw
    need = lib.pgasr_beam_wide_workspace_bytes(10, 2, 300, 8)
    assert _call(lib, ws=0) == WORKSPACE and _call(lib, ws_bytes=need - 1) == WORKSPACE
    for flags in (0, 1, 32, 33):                                       # the accepted flags get as far as the workspace check
        assert _call(lib, flags=flags, ws=0) == WORKSPACE
    assert _call(lib, nbest=0, ws=0) == INVALID                        # the list's arguments before the workspace
    # node ids are 22 bits: T * beam + 1 >= 2^22 is refused (after the workspace check, as in A7-NBEST)
    T = (1 << 22) // 128
    assert _call(lib, T=T, beam=128, nbest=1, tok_stride=T) == UNSUPPORTED
    assert _call(lib, T=T, beam=128, nbest=1, tok_stride=T, ws=0) == WORKSPACE
    assert _call(lib, T=T - 1, beam=128, nbest=1, tok_stride=T, ws=0) == WORKSPACE


def test_wide_decoder_refusals_need_no_device():
    """CTCDecoder(wide_search=True) with a language model and a 300-symbol alphabet: ValueError naming lm from decode and decode_batch,
    before a device is asked for; lm=None for the call lifts it (and then a host without a GPU fails on the device, not on the LM).  The default
    decoder's refusal above 64 symbols is the one it always was."""
    import torch
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder

    class FakeLM:
        vocab, blank, order = 300, 0, 2

    assert hipops.MAX_VOCAB_SEARCH_WIDE == 1024
    probs = np.full((3, 300), 1.0 / 300)
    dec = CTCDecoder(list(range(300)), lm=FakeLM(), lm_alpha=0.5, wide_search=True)
    with pytest.raises(ValueError, match="lm"):
        dec.decode(probs, beam_size=4)
    with pytest.raises(ValueError, match="lm"):
        dec.decode(probs, beam_size=4, nbest=2)
    with pytest.raises(ValueError, match="lm"):
        dec.decode_batch(torch.zeros(3, 1, 300), beam_size=4)
    with pytest.raises(ValueError, match="1024"):
        CTCDecoder(list(range(1025)), wide_search=True).decode_batch(torch.zeros(3, 1, 1025), beam_size=4)
    with pytest.raises(ValueError, match="greed"):
        CTCDecoder(list(range(300))).decode_batch(torch.zeros(3, 1, 300), beam_size=4)
    with pytest.raises(ValueError, match="greed"):
        CTCDecoder(list(range(300)), lm=FakeLM()).decode_batch(torch.zeros(3, 1, 300), beam_size=4)
