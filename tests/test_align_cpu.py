"""CTC forced alignment without a GPU: the numpy statement (tests/align_ref.py) against brute force, its tie rule on fully tied
inputs, the C entry points' exports and refusals, and the pure-host helpers."""
import ctypes
import math
import os

import numpy as np
import pytest

import align_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")

# frame labels of the best alignment of uniform rows (every lp = -ln V), T = 7, blank = 0, derived by hand from "the smallest move
# wins a tie": all reachable states of a frame hold the same delta, the alignment ends in the last blank (state 4, since
# delta(3) > delta(4) is false) and STAYS there as long as the state was reachable a frame earlier; state 4 is first reachable at
# frame 2 for (1,2) (the skip 1 -> 3 exists) and at frame 3 for (1,1) (no skip between equal labels), and below that every
# backpointer is the only finite one.
TIED = {(1, 2): [1, 2, 0, 0, 0, 0, 0],       # states 1 3 4 4 4 4 4
        (1, 1): [1, 0, 1, 0, 0, 0, 0]}       # states 1 2 3 4 4 4 4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.pgasr_ctc_align_workspace_bytes.restype = ctypes.c_size_t
    lib.pgasr_ctc_align_workspace_bytes.argtypes = [ctypes.c_int] * 3
    lib.pgasr_ctc_forced_align.restype = ctypes.c_int
    return lib


def test_reference_against_brute_force():
    rng = np.random.default_rng(7)
    n_inf = 0
    for case in range(40):
        T, L = int(rng.integers(0, 7)), int(rng.integers(0, 4))
        lp = np.log(rng.dirichlet(np.ones(3), size=T)).astype(np.float32).reshape(T, 3)
        tok = rng.integers(1, 3, size=L)
        r = R.align_one(lp, tok, blank=0)
        want = R.brute_force_score(lp, tok, blank=0)
        if math.isinf(want):
            n_inf += 1
            assert r.score == np.inf, (case, T, tok)
            assert (r.frame_label == -1).all() and (r.token_start == -1).all() and (r.token_logp == 0).all()
        else:
            assert abs(r.score - want) <= 1e-12, (case, T, tok, r.score, want)
            # the alignment IS a path with that score, and its spans describe it
            assert R.collapse(r.frame_label.tolist(), 0) == tok.tolist()
            assert -sum(np.float64(lp[t, k]) for t, k in enumerate(r.frame_label)) == pytest.approx(r.score, abs=1e-12)
            for i in range(L):
                fr = np.nonzero(r.frame_token == i)[0]
                assert fr[0] == r.token_start[i] and fr[-1] + 1 == r.token_end[i] and len(fr) == fr[-1] + 1 - fr[0]
    assert 0 < n_inf < 40          # both kinds occur


@pytest.mark.parametrize("tok", sorted(TIED))
def test_tie_rule_on_fully_tied_input(tok):
    lp = np.full((7, 3), -math.log(3.0), np.float32)
    r = R.align_one(lp, tok, blank=0)
    assert r.frame_label.tolist() == TIED[tok]
    acc = np.float64(lp[0, 0])
    for _ in range(6):
        acc = acc + np.float64(lp[0, 0])
    assert r.score == -acc


def test_abi_exports_and_workspace(lib):
    from policy_gradient_asr_amd import _lib
    for name in ("pgasr_ctc_align_workspace_bytes", "pgasr_ctc_forced_align"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["pgasr_ctc_forced_align"][1]) == 18
    lib.pgasr_abi_version.restype = ctypes.c_int
    assert lib.pgasr_abi_version() == 7
    # one byte per backpointer, the 201 states of a row rounded up to 64
    assert lib.pgasr_ctc_align_workspace_bytes(1000, 32, 100) >= 32 * 1000 * 256
    assert lib.pgasr_ctc_align_workspace_bytes(0, 32, 100) == 0
    assert lib.pgasr_ctc_align_workspace_bytes(1000, 0, 100) == 0 and lib.pgasr_ctc_align_workspace_bytes(1000, 32, 0) == 0


def test_refusals_need_no_gpu(lib):
    INVALID, WORKSPACE, UNSUPPORTED = 1, 3, 4
    p = ctypes.c_void_p
    buf = ctypes.create_string_buffer(4096)       # never dereferenced: every call below is refused before any HIP call
    a = ctypes.cast(buf, p)

    def call(lp=a, tok=a, il=a, tl=a, T=10, B=2, V=5, Lmax=4, blank=0, score=a, fl=a, ws=a, ws_bytes=1 << 40):
        return lib.pgasr_ctc_forced_align(p(lp.value if lp else None), p(tok.value if tok else None), p(il.value if il else None),
                                          p(tl.value if tl else None), T, B, V, Lmax, blank, p(score.value if score else None),
                                          p(fl.value if fl else None), p(None), p(None), p(None), p(None),
                                          p(ws.value if ws else None), ctypes.c_size_t(ws_bytes), p(None))
    for missing in ("lp", "tok", "il", "tl", "score", "fl"):
        assert call(**{missing: None}) == INVALID, missing
    for bad in ({"T": 0}, {"B": 0}, {"V": 0}, {"Lmax": 0}, {"blank": 5}, {"blank": -1}):
        assert call(**bad) == INVALID, bad
    assert call(Lmax=1024) == UNSUPPORTED
    assert call(ws_bytes=0) == WORKSPACE and call(ws=None) == WORKSPACE
    need = lib.pgasr_ctc_align_workspace_bytes(10, 2, 4)
    assert need > 0 and call(ws_bytes=need - 1) == WORKSPACE


def test_word_spans():
    from policy_gradient_asr_amd.CTCdecoder import word_spans
    sp = 5
    #        a  b  _  c
    tokens = [1, 2, sp, 3]
    st, en = [0, 2, 5, 7], [2, 3, 6, 9]
    assert word_spans(st, en, tokens, sp) == [(0, 3), (7, 9)]
    # leading, trailing and double delimiters give empty words, as "".split(" ") does
    assert word_spans([0, 1, 3], [1, 2, 4], [sp, 1, sp], sp) == [(-1, -1), (1, 2), (-1, -1)]
    assert word_spans([0, 1, 2, 3], [1, 2, 3, 4], [1, sp, sp, 2], sp) == [(0, 1), (-1, -1), (3, 4)]
    assert word_spans([], [], [], sp) == [(-1, -1)]
    assert len(word_spans([0, 1, 3], [1, 2, 4], [sp, 1, sp], sp)) == len(" a ".split(" "))
    # an unaligned character leaves its word without a span
    assert word_spans([-1, -1, -1], [-1, -1, -1], [1, sp, 2], sp) == [(-1, -1), (-1, -1)]
    with pytest.raises(ValueError):
        word_spans([0], [1, 2], [1], sp)


def test_align_rejects_bad_labels_before_the_device():
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    dec = CTCDecoder(["<pad>", "a", "b"])
    probs = np.full((6, 3), 1.0 / 3.0)
    for labels, blank in (([1, 0], 0), ([3], 0), ([-1], 0), ([1, 2], 2)):
        with pytest.raises(ValueError):
            dec.align(probs, labels, blank=blank)
    with pytest.raises(ValueError):
        dec.align(probs, [1], blank=3)
    # no frames: answered on the host, as decode() does
    assert dec.align(np.zeros((0, 3)), []) == (tuple(), [], 0.0)
    assert dec.align(np.zeros((0, 3)), [1])[2] == float("inf")
