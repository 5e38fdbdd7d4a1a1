"""The lattice-free CTC scorer (pgasr_ctc_hyp_score, csrc/hyp_score.hip) on a GPU-less host: the numpy statement the device is held
to (tests/hyp_score_ref.py) against torch-CPU fp64 ctc_loss on every case of the GPU tests, the entry point's checks and their
order (every call is refused before any HIP call: the pointers are fake), the host layer's refusals, and the refusals that stay."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hyp_score_ref as H  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def _torch_rows(c):
    """(mask of the rows torch can be asked about, torch-CPU fp64 ctc_loss there).  Left out: the rows the contract settles without
    a sweep (beyond count, over Lh, a token that is the blank or no symbol, an utterance without frames)."""
    import torch.nn.functional as F
    lp, tokens, lengths, in_len, blank = c["lp"], c["tokens"], c["lengths"], c["in_len"], c["blank"]
    T, B, V = lp.shape
    N, _, stride = tokens.shape
    ln = np.maximum(lengths, 0)
    inside = np.arange(stride)[None, None, :] < ln[:, :, None]
    bad = (((tokens < 0) | (tokens >= V) | (tokens == blank)) & inside).any(axis=2)
    cnt = np.full(B, N) if c["count"] is None else np.clip(c["count"], 0, N)
    ask = (np.arange(N)[:, None] < cnt[None, :]) & (ln <= min(c["Lh"], stride)) & ~bad & (np.clip(in_len, 0, T) > 0)[None, :]
    safe = next(v for v in range(V) if v != blank)
    tok = np.where(ask[:, :, None] & inside, tokens, safe).astype(np.int64)
    got = np.full((N, B), np.nan)
    lp64 = torch.from_numpy(lp.copy()).double()
    il = torch.from_numpy(np.clip(in_len, 1, T).astype(np.int64))
    for n in range(N):
        tl = torch.from_numpy(np.where(ask[n], ln[n], 0).astype(np.int64))
        got[n] = F.ctc_loss(lp64, torch.from_numpy(tok[n, :, :max(int(tl.max()), 1)]), il, tl, blank=blank, reduction="none",
                            zero_infinity=False).numpy()
    return ask, got


@pytest.mark.parametrize("name", H.ALL)
def test_statement_agrees_with_torch_fp64(name):
    """1e-9 relative on every finite row (fp64 against fp64: the bound tests/test_nbest_gpu.py holds its exact path to), +inf where
    torch has +inf; the rows settled by contract are +inf, or 0 for the empty hypothesis of an utterance without frames.
    Largest deviation seen over all cases: 2.7e-16 (NOTES.md 0.27)."""
    c = H.case(name)
    want = c["want"]
    ask, got = _torch_rows(c)
    assert not np.isnan(want).any()
    worst = H.close(want[ask], got[ask]) if ask.any() else 0.0
    print(f"{name}: {int(ask.sum())} rows against torch, {int(np.isfinite(want).sum())} finite, largest deviation {worst:.2e}")
    rest = want[~ask]
    no_frames = (np.clip(c["in_len"], 0, None) == 0)[None, :] & (np.maximum(c["lengths"], 0) == 0) & ~ask
    assert ((rest == np.inf) | (rest == 0.0)).all() and (want[no_frames & np.isfinite(want)] == 0.0).all()
    assert ((want == 0.0) <= no_frames).all()


def test_cases_cover_what_they_are_there_for():
    """The premises of the GPU tests: the lengths and variant boundaries, the least feasible frame count and one less, finite and
    infinite rows in every edge case that has both by design."""
    seen = set()
    for name in H.EDGE:
        c = H.case(name)
        seen |= set(int(v) for v in c["lengths"].ravel())
    assert set(H.LENGTHS) <= seen and all(a in seen and b in seen and b == a + 1 for a, b in H.VARIANT_BOUNDARIES)
    r = H.case("v2_runs")
    assert H.frames_needed([0] * 6) == 11 == r["in_len"][0] == r["in_len"][1] + 1
    assert np.isfinite(r["want"][6, 0]) and r["want"][7, 0] == np.inf and r["want"][6, 1] == np.inf and np.isfinite(r["want"][5, 1])
    assert r["want"][0, 2] == 0.0 and (r["want"][1:, 2] == np.inf).all()
    t1 = H.case("t1")["want"]
    assert np.isfinite(t1[0, 0]) and np.isfinite(t1[0, 1]) and t1[0, 2] == np.inf
    v29 = H.case("v29")
    assert (v29["want"][3:7, 0] == np.inf).all() and np.isfinite(v29["want"][1, 0]) and (v29["want"][9:, 1] == np.inf).all()
    v1000 = H.case("v1000")
    assert (v1000["want"][v1000["lengths"] > 200] == np.inf).all() and np.isfinite(v1000["want"][v1000["lengths"] <= 200]).all()
    assert v1000["tokens"].shape[2] > v1000["Lh"]
    assert np.isfinite(H.case("v1024_long")["want"]).all() and np.isfinite(H.case("steep")["want"]).all()
    assert (H.case("steep")["want"] > 15.0 * 900).all()                      # ~20 nats per frame
    z = H.case("zeros")
    uses = np.array([[any(v in (5, 77) for v in z["tokens"][n, b, :z["lengths"][n, b]]) for b in range(2)] for n in range(8)])
    assert uses.any() and (z["want"][uses] == np.inf).all() and np.isfinite(z["want"][~uses]).all()
    for name in H.ALL:
        c = H.case(name)
        toks = c["tokens"][np.arange(c["tokens"].shape[2])[None, None, :] < c["lengths"][:, :, None]]
        if c["lp"].shape[2] > 64:
            assert (toks >= 64).any(), name
    assert any((H.case(n)["tokens"] == H.case(n)["lp"].shape[2] - 1).any() for n in ("v65", "v128", "v1024_long"))


def test_symbol_exported_and_bound_abi_stays_7(lib):
    from policy_gradient_asr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bpgasr_ctc_hyp_score\s*\(([^)]*)\)", src)
    assert m and hasattr(lib, "pgasr_ctc_hyp_score")
    assert m.group(1).count(",") + 1 == len(_lib.SIGNATURES["pgasr_ctc_hyp_score"][1]) == 14
    assert _lib.SIGNATURES["pgasr_ctc_hyp_score"][0] is ctypes.c_int
    assert int(re.search(r"#define PGASR_ABI_VERSION (\d+)", src).group(1)) == 7 and lib.pgasr_abi_version() == 7


def _score(lib, lp=0x1000, tok=0x1000, stride=8, ln=0x1000, count=0x1000, il=0x1000, T=10, B=2, V=29, N=4, Lh=5, blank=0, out=0x1000):
    return lib.pgasr_ctc_hyp_score(lp, tok, stride, ln, count, il, T, B, V, N, Lh, blank, out, None)


def test_status_codes_and_their_order(lib):
    """Every call below must return before dereferencing a pointer or launching: the pointers are fake.  Invalid arguments come
    before unsupported sizes."""
    for kw in (dict(lp=None), dict(tok=None), dict(ln=None), dict(il=None), dict(out=None), dict(T=0), dict(B=0), dict(N=0),
               dict(stride=0), dict(Lh=-1), dict(V=0), dict(blank=-1), dict(blank=29), dict(V=1025, blank=1025), dict(N=-3)):
        assert _score(lib, **kw) == INVALID_ARG, kw
    for kw in (dict(V=1025), dict(N=129), dict(Lh=1024), dict(V=1025, N=129, Lh=4000)):
        assert _score(lib, **kw) == UNSUPPORTED, kw
    # an invalid argument wins over an unsupported size, whichever comes first in the list
    for kw in (dict(V=1025, T=0), dict(N=129, blank=40), dict(Lh=1024, out=None), dict(N=129, stride=-1)):
        assert _score(lib, **kw) == INVALID_ARG, kw
    # a NULL count is no error: with everything else in range the next thing would be the launch, so only the refusals around it
    # are asserted here -- the limits themselves are accepted values
    assert _score(lib, count=None, V=1025) == UNSUPPORTED and _score(lib, count=None, T=0) == INVALID_ARG


def test_refusals_that_stay(lib):
    """pgasr_ctc_hyp_lattice keeps its limits: V = 65 unsupported, K = 17 invalid; pgasr_nbest_rescore and pgasr_nbest_pair_dist
    keep refusing V = 65."""
    p = 0x1000
    assert lib.pgasr_ctc_hyp_lattice(p, p, 10, p, p, 10, 2, 65, 4, 5, 0, p, p, 1 << 40, None) == UNSUPPORTED
    assert lib.pgasr_ctc_hyp_lattice(p, p, 10, p, p, 10, 2, 29, 17, 5, 0, p, p, 1 << 40, None) == INVALID_ARG
    assert lib.pgasr_ctc_hyp_workspace_bytes(10, 2, 29, 17, 5) == 0 and lib.pgasr_ctc_hyp_workspace_bytes(10, 2, 65, 4, 5) == 0
    assert lib.pgasr_nbest_rescore(p, 8, p, p, p, 4, 2, 65, 0, None, 0, 1.0, 0.0, 0.0, p, p, p, None) == UNSUPPORTED
    assert lib.pgasr_nbest_pair_dist(p, 8, p, p, 4, 2, 65, 8, p, None) == UNSUPPORTED


def test_host_layer_refusals_need_no_device():
    """What the Python layer refuses before it touches a tensor's memory: CPU tensors (there is no CPU path), an unknown scorer,
    the lattice outside its limits, language models over a wide list."""
    from policy_gradient_asr_amd import _lib, hipops
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    lp = torch.zeros(5, 2, 29)
    tok = torch.zeros(3, 2, 4, dtype=torch.int32)
    ln = torch.zeros(3, 2, dtype=torch.int32)
    il = torch.full((2,), 5, dtype=torch.int32)
    with pytest.raises(_lib.PgasrError):
        hipops.ctc_hyp_score(lp, tok, ln, il, 4)
    nb = hipops.CTCNBest(tok, ln, torch.zeros(3, 2, dtype=torch.float64), torch.full((2,), 3, dtype=torch.int32))
    dec = CTCDecoder(list(range(29)))
    with pytest.raises(ValueError, match="scorer"):
        dec.rescore(lp, il, nb, lm=None, scorer="backward")
    big = hipops.CTCNBest(torch.zeros(17, 2, 4, dtype=torch.int32), torch.zeros(17, 2, dtype=torch.int32),
                          torch.zeros(17, 2, dtype=torch.float64), torch.full((2,), 17, dtype=torch.int32))
    with pytest.raises(ValueError, match="lattice"):
        dec.rescore(lp, il, big, lm=None, scorer="lattice")
    wide = CTCDecoder(list(range(300)), wide_search=True)
    lpw = torch.zeros(5, 2, 300)
    with pytest.raises(ValueError, match="lattice"):
        wide.rescore(lpw, il, nb, lm=None, scorer="lattice")
    with pytest.raises(ValueError, match="^lm:"):
        wide.rescore(lpw, il, nb, lm=object())
    with pytest.raises(ValueError, match="^word_lm:"):
        wide.rescore(lpw, il, nb, lm=None, word_lm=object(), word_delimiter=4)
