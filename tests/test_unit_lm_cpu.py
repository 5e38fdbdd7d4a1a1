"""lm.UnitNgramLM on the host (no GPU): the contractual back-off query against the plain-dict statement of tests/unit_lm_ref.py and
against the dense form, the estimator, the ARPA and npz round trips, the constructor's refusals, the two forms of the fused reference
search against each other, the decision margins of the GPU cases, and the Python layer's refusals."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as R  # noqa: E402
import unit_lm_ref as U  # noqa: E402

from policy_gradient_asr_amd.lm import CharNgramLM, UnitNgramLM  # noqa: E402


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("V", [5, 65])
def test_query_equals_the_dict_statement_and_the_dense_form(V, order):
    """dict statement == UnitNgramLM.logp == to_dense() (where V**order <= 2**25) on every reachable (context, s): exhaustively
    while there are at most 300000 pairs (V = 5 at every order, V = 65 up to order 3); at V = 65, orders 4 and 5 (17 and 1074
    million pairs) on every stored n-gram, every stored context extended by every symbol, and 20000 random prefixes."""
    blank = V // 2
    d, m = U.random_unit_lm(V, order, blank, 11 * V + order, n_ctx=12, n_succ=4)
    dense = m.to_dense() if V ** order <= U.DENSE_MAX else None
    assert (dense is None) == (V == 65 and order == 5)
    syms = [s for s in range(V) if s != blank]
    if len(syms) ** order <= 300000:
        prefixes = [y for k in range(order) for y in itertools.product(syms, repeat=k)]
    else:
        rng = np.random.default_rng(V + order)
        prefixes = [tuple(g[1:] if g[0] == blank else g) for g in d if g != (blank,)]
        prefixes += [tuple(int(x) for x in rng.choice(syms, size=rng.integers(0, order + 2))) for _ in range(20000 // len(syms) + 1)]
    n = 0
    for y in prefixes:
        for s in syms:
            want = U.query(d, order, blank, y, s)
            assert m.logp(y, s) == want, (y, s)
            if dense is not None:
                assert dense.logp(y, s) == want, (y, s)
            n += 1
    assert n >= len(syms)
    if dense is not None:                  # contexts the sparse model cannot have: counted from their last blank on; the blank column
        assert dense.table.shape == (V,) * order and not dense.table[..., blank].any()
        if order >= 3:
            a, b = syms[0], syms[1]
            assert dense.table[(a,) * (order - 3) + (a, blank, b)] == np.float32(U.query(d, order, blank, (), b))
            assert dense.table[(a,) * (order - 3) + (blank, blank, b)] == np.float32(U.query(d, order, blank, (), b))
    y = [int(x) for x in np.random.default_rng(1).choice(syms, size=12)]
    assert m.logp_sequence(y) == U.sequence(d, order, blank, y) and m.logp_sequence([]) == 0.0


def test_the_random_model_holds_what_the_cases_need():
    """Contexts and hits at every level, a stored context with a bow and no successor, start-pad contexts, n-grams absent at every
    level down to the unigram."""
    V, order, blank = 65, 4, 32
    d, m = U.random_unit_lm(V, order, blank, 17)
    by_len = {k: [g for g in d if len(g) == k] for k in range(1, order + 1)}
    assert all(by_len[k] for k in by_len)
    ctxs = {g[:-1] for g in d if len(g) > 1}
    assert {len(c) for c in ctxs} == {1, 2, 3}
    assert any(g not in ctxs and d[g][1] != 0.0 for g in by_len[2])
    assert (blank,) in ctxs and any(c[0] == blank and len(c) == 2 for c in ctxs)
    y = (1, 2, 3)
    assert all((y[i:] + (5,)) not in d for i in range(3)) and (5,) in d
    packed = m.pack()
    assert packed["states"].shape == (1 + V + len(by_len[2]) + len(by_len[3]), 4) and packed["start"] == 1 + blank
    assert packed["succ"].shape == (V - 1 + len(by_len[2]) + len(by_len[3]) + len(by_len[4]), 4)


def _estimate_query(grams, h, s):
    d = {}
    for g in grams:
        d.update(g)
    acc, h = 0.0, tuple(h)
    while True:
        e = d.get(h + (s,))
        if e is not None:
            return acc + e[0]
        c = d.get(h) if h else None
        if c is not None:
            acc += c[1]
        h = h[1:]


def test_the_estimator_normalises_and_agrees_with_the_dense_one():
    """sum_s p(s | h) = 1 within 1e-12 on seen and unseen contexts, on the estimator's fp64 values (``UnitNgramLM.estimate``: the fp32
    model rounds each of them once, |ln p| * 2**-24 < 2e-6 relative, and is held to 1e-5); at orders 1 to 3 and V = 29 the
    probabilities equal CharNgramLM.from_transcripts' within 1e-6 on the contexts both have -- a dense context of two blanks is
    the one the sparse model cannot have: it keeps exactly one start symbol."""
    V, blank = 29, 0
    rng = np.random.default_rng(0)
    seqs = [list(rng.integers(1, 8, size=rng.integers(0, 14))) for _ in range(120)] + [[28, 27, 26]]
    for order, min_count in ((1, 1), (2, 1), (3, 1), (4, 1), (5, 2), (3, 3)):
        grams = UnitNgramLM.estimate(seqs, V, order=order, blank=blank, min_count=min_count)
        m = UnitNgramLM.from_transcripts(seqs, V, order=order, blank=blank, min_count=min_count)
        seen = [g[:-1] for g in grams[-1]][:40] if order > 1 else [()]
        unseen = [tuple([20, 21, 22, 23][:order - 1]), (blank,) + tuple([25, 24, 23][:max(order - 2, 0)])] if order > 1 else []
        for h in seen + unseen:
            assert abs(sum(np.exp(_estimate_query(grams, h, s)) for s in range(1, V)) - 1.0) < 1e-12, (order, h)
            y = h[1:] if h and h[0] == blank else h
            if len(h) == order - 1 or (h and h[0] == blank):
                assert abs(sum(np.exp(m.logp(y, s)) for s in range(1, V)) - 1.0) < 1e-5, (order, h)
    for order in (1, 2, 3):
        u = UnitNgramLM.from_transcripts(seqs, V, order=order, blank=blank)
        c = CharNgramLM.from_transcripts(seqs, V, order=order, blank=blank)
        n = 0
        for y in seqs:
            for i in range(len(y)):
                if order == 3 and i == 0:
                    continue                                   # the dense context (blank, blank)
                assert abs(np.exp(u.logp(y[:i], y[i])) - np.exp(c.logp(y[:i], y[i]))) < 1e-6
                n += 1
        assert n > 500


def test_round_trips_preserve_every_query_bit(tmp_path):
    V, order, blank = 65, 4, 7
    d, m = U.random_unit_lm(V, order, blank, 5)
    names = ["u%d" % i for i in range(V)]
    m.to_arpa(str(tmp_path / "m.arpa"), names=names)
    m.save(str(tmp_path / "m.npz"))
    text = open(str(tmp_path / "m.arpa")).read().replace("\\2-grams:\n", "\\2-grams:\n-1.5\tu1 </s>\n-2.5\t<unk> u1\n")
    open(str(tmp_path / "extra.arpa"), "w").write(text)
    for back in (UnitNgramLM.from_arpa(str(tmp_path / "m.arpa"), V, blank=blank, names=names), UnitNgramLM.load(str(tmp_path / "m.npz")),
                 UnitNgramLM.from_arpa(str(tmp_path / "extra.arpa"), V, blank=blank, names=names)):
        assert back.order == order and back.vocab == V and back.blank == blank
        for k in range(order):
            assert np.array_equal(back.ngrams[k], m.ngrams[k]) and np.array_equal(back.lp[k].view(np.int32), m.lp[k].view(np.int32))
            if k < order - 1:
                assert np.array_equal(back.bw[k].view(np.int32), m.bw[k].view(np.int32))
        rng = np.random.default_rng(2)
        for _ in range(300):
            y = [int(x) for x in rng.integers(8, V, size=rng.integers(0, 6))]
            s = int(rng.integers(8, V))
            assert back.logp(y, s) == U.query(d, order, blank, y, s)
    with pytest.raises(ValueError, match="no symbol"):
        UnitNgramLM.from_arpa(str(tmp_path / "m.arpa"), V, blank=blank, names=["v%d" % i for i in range(V)])


def test_constructor_refusals():
    V, blank = 6, 0
    uni = np.arange(V).reshape(-1, 1)
    lp1, bw1 = np.full(V, -1.5, dtype=np.float32), np.zeros(V, dtype=np.float32)
    ok2 = np.array([[0, 1], [1, 2]])
    UnitNgramLM([uni, ok2], [lp1, [-1.0, -2.0]], [bw1, [0.0, 0.0]], V, blank=blank)
    with pytest.raises(ValueError, match="unigram is missing"):
        UnitNgramLM([uni[:-1]], [lp1[:-1]], [bw1[:-1]], V, blank=blank)
    bad = lp1.copy(); bad[3] = -np.inf
    with pytest.raises(ValueError, match="non-finite"):
        UnitNgramLM([uni], [bad], [bw1], V, blank=blank)
    with pytest.raises(ValueError, match="non-finite"):
        UnitNgramLM([uni, ok2], [lp1, [-1.0, np.nan]], [bw1, [0.0, 0.0]], V, blank=blank)
    with pytest.raises(ValueError, match="context is not stored"):
        UnitNgramLM([uni, ok2, np.array([[2, 3, 4]])], [lp1, [-1.0, -2.0], [-1.0]], [bw1, [0.0, 0.0], [0.0]], V, blank=blank)
    with pytest.raises(ValueError, match="blank stands inside"):
        UnitNgramLM([uni, np.array([[1, 0]])], [lp1, [-1.0]], [bw1, [0.0]], V, blank=blank)
    with pytest.raises(ValueError, match="blank stands inside"):
        UnitNgramLM([uni, ok2, np.array([[1, 0, 2]])], [lp1, [-1.0, -2.0], [-1.0]], [bw1, [0.0, 0.0], [0.0]], V, blank=blank)
    with pytest.raises(ValueError, match="order 1 .. 5"):
        UnitNgramLM([uni] * 6, [lp1] * 6, [bw1] * 6, V, blank=blank)
    with pytest.raises(ValueError, match="order 1 .. 5"):
        UnitNgramLM.from_transcripts([[1, 2]], V, order=6)
    big = np.arange(1025).reshape(-1, 1)
    with pytest.raises(ValueError, match="1024"):
        UnitNgramLM([big], [np.zeros(1025)], [np.zeros(1025)], 1025)
    with pytest.raises(ValueError, match="lexicographic"):
        UnitNgramLM([uni, ok2[::-1]], [lp1, [-1.0, -2.0]], [bw1, [0.0, 0.0]], V, blank=blank)
    with pytest.raises(ValueError, match="blank"):
        UnitNgramLM([uni], [lp1], [bw1], V, blank=blank).logp((), blank)
    with pytest.raises(ValueError, match="2\\*\\*25"):
        U.random_unit_lm(65, 5, 0, 1)[1].to_dense()


SHARED = [c for c in U.CASES if c[1] ** c[3] <= U.DENSE_MAX]


@pytest.mark.parametrize("case", SHARED, ids=U.case_id)
def test_the_two_forms_of_the_search_agree(case):
    """Where both apply (V**order <= 2**25) the restated loop over the dict statement and nbest_ref's loop over the dense table return
    equal lists, scores and margins: this validates the loop the V = 1024 cases of order 3 and 4 rely on."""
    dense, call = U.reference(case), U.reference(case, "callable")
    assert len(SHARED) >= 4
    for (h1, g1), (h2, g2) in zip(dense, call):
        assert [tuple(h[0]) for h in h1] == [tuple(h[0]) for h in h2]
        assert [h[1] for h in h1] == [h[1] for h in h2] and g1 == g2


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_gpu_cases_have_decision_margins(case):
    """Every utterance of every GPU case has a smallest decision margin >= beam_lm_ref.GAP_MIN, and the seed is the first of 0, 1, 2, ..
    of which that holds; the lengths have a 1 and a 0 among them (the flat case keeps its source's full lengths)."""
    T, V, beam, order, blank, B, alpha, beta, kind, seed = case
    assert (alpha, beta) in ((0.8, 0.5), (0.5, 0.0), (1.0, 1.2)) or (kind == "flat" and beta == 3.0)
    lp, lens = U.case_inputs(case)
    assert lp.shape == (T, B, V) and (kind == "flat" or (1 in lens and 0 in lens))
    gaps = [g for _, g in U.reference(case)]
    print(U.case_id(case), ["%.3e" % g for g in gaps])
    assert min(gaps) >= U.GAP_MIN
    for earlier in range(seed):
        assert min(g for _, g in U.reference(case[:-1] + (earlier,))) < U.GAP_MIN, earlier


def test_python_layer_refusals_touch_no_device(monkeypatch):
    """Each refusal names its option and is raised before a device is asked for; the refusals of lm= / word_lm= over wide rows and of
    lm_path with the wide beam stand as they were."""
    import torch
    from policy_gradient_asr_amd import CTCdecoder, hipops
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(CTCdecoder, "_device", no_device)
    monkeypatch.setattr(hipops._lib, "load", no_device)
    _, m = U.random_unit_lm(100, 3, 0, 1)
    dense = CharNgramLM(R.random_table(29, 2, 0, 1), 2, 0)
    with pytest.raises(ValueError, match="unit_lm"):
        CTCDecoder(list(range(100)), unit_lm=m)                                  # needs wide_search=True
    with pytest.raises(ValueError, match="unit_lm"):
        CTCDecoder(list(range(29)), wide_search=True, unit_lm=m, lm=dense)
    dec = CTCDecoder(list(range(100)), wide_search=True, unit_lm=m, lm_alpha=0.5)
    probs = np.full((4, 100), 0.01)
    with pytest.raises(ValueError, match="unit_lm"):
        dec.decode(np.full((4, 90), 1.0 / 90))                                   # V differs
    with pytest.raises(ValueError, match="unit_lm"):
        dec.decode(probs, blank=3)                                               # blank differs
    with pytest.raises(ValueError, match="unit_lm"):
        dec.decode(probs, lm=dense)
    with pytest.raises(ValueError, match="unit_lm"):
        dec.decode_batch(torch.zeros(4, 2, 90))
    with pytest.raises(ValueError, match="unit_lm"):
        hipops.ctc_beam_search_wide(torch.zeros(4, 2, 100), unit_lm=dense)       # not a UnitNgramLM
    with pytest.raises(ValueError, match="unit_lm"):
        hipops.ctc_beam_search_wide(torch.zeros(4, 2, 100), unit_lm=m, blank=1)
    with pytest.raises(ValueError, match="unit_lm"):
        hipops.nbest_unit_lm_score(torch.zeros(2, 2, 4, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32),
                                   torch.zeros(2, dtype=torch.int32), dense)
    nb = hipops.CTCNBest(torch.zeros(2, 2, 4, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.float64),
                         torch.zeros(2, dtype=torch.int32))
    plain = CTCDecoder(list(range(100)), wide_search=True)
    with pytest.raises(ValueError, match="unit_lm"):
        plain.rescore(torch.zeros(4, 2, 90), None, nb, unit_lm=m)
    # what stood before stands: lm= in the wide search, lm= / word_lm= over wide lists
    with pytest.raises(ValueError, match="lm: the wide beam search"):
        plain.decode(probs, lm=dense)
    for name in ("lm", "word_lm"):
        with pytest.raises(ValueError, match="^%s: not over a list of 100" % name):
            plain.rescore(torch.zeros(4, 2, 100), None, nb, **{name: dense})


def test_predict_refusals(tmp_path):
    """unit_lm_path needs the wide beam; rescore_unit_lm_path a list and, over a wide alphabet, the second pass; lm_path with the wide
    beam is refused as before.  All before a device or a model file is asked for."""
    from policy_gradient_asr_amd.model import predict
    from policy_gradient_asr_amd.units import SubwordUnits
    units = SubwordUnits(["a", "b", " "] + ["%s%s%s" % q for q in itertools.product("ab ", repeat=3)] + ["%s%s%s%s" % q for q in itertools.product("ab ", repeat=4)][:70])
    upath = str(tmp_path / "units.txt")
    units.save(upath)
    assert len(units) > 64
    kw = dict(units_path=upath, test_dataset=[])
    for match, arg in (("unit_lm_path", dict(unit_lm_path="x.npz", beam_size=4)),
                       ("unit_lm_path", dict(unit_lm_path="x.npz", beam_size=0, wide_beam=True)),
                       ("rescore_unit_lm_path", dict(rescore_unit_lm_path="x.npz", beam_size=4, wide_beam=True)),
                       ("rescore_unit_lm_path", dict(rescore_unit_lm_path="x.npz", beam_size=4, wide_beam=True, nbest=2)),
                       ("lm_path", dict(lm_path="x.npz", beam_size=4, wide_beam=True)),
                       ("lm_path", dict(lm_path="x.npz", unit_lm_path="y.npz", beam_size=4, wide_beam=True))):
        with pytest.raises(ValueError, match=match):
            predict(None, None, None, str(tmp_path), 8, **arg, **kw)


# ---- the C entries' argument checks: before any HIP call, so a host without a GPU runs them ----
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, 1, 3, 4


def _tables(**kw):
    from policy_gradient_asr_amd import _lib
    a = dict(states=16, succ=16, order=3, vocab=300, blank=0, n_states=400, n_succ=500, start=1)
    a.update(kw)
    return _lib.UnitLMTables(a["states"], a["succ"], a["order"], a["vocab"], a["blank"], a["n_states"], a["n_succ"], a["start"])


def _search(lib, tables, alpha=0.5, beta=0.5, **kw):
    """pgasr_ctc_beam_search_wide_lm with dummy non-NULL pointers that a refused call never reads."""
    import ctypes
    a = dict(log_probs=16, T=10, B=2, V=300, beam=8, blank=0, flags=0, nbest=4, out_tokens=16, tok_stride=10, out_count=16, ws=16,
             ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = 0 if a["ws"] == 0 else 1 << 40
    return lib.pgasr_ctc_beam_search_wide_lm(a["log_probs"], 0, 0, 0, 0, a["T"], a["B"], a["V"], a["beam"], a["blank"], a["flags"], a["nbest"],
                                             a["out_tokens"], a["tok_stride"], 16, 16, a["out_count"], 0, a["ws"], a["ws_bytes"], 0,
                                             None if tables is None else ctypes.byref(tables), alpha, beta)


def test_c_entries_check_their_arguments_before_any_hip_call():
    """pgasr_ctc_beam_search_wide_lm: A7-WIDE's checks in their order, the model's where that entry checks its flags, then the trie's part
    of the workspace, the node-id width, the whole workspace.  pgasr_nbest_unit_lm_score: limits, pointers and sizes, the model.
    Every call here is refused, so none reaches HIP.  Both symbols are in the signature table and the ABI number is 7."""
    import ctypes
    from policy_gradient_asr_amd import _lib
    lib = _lib.load()
    assert len(_lib.SIGNATURES["pgasr_ctc_beam_search_wide_lm"][1]) == 24 and len(_lib.SIGNATURES["pgasr_nbest_unit_lm_score"][1]) == 11
    assert _lib.SIGNATURES["pgasr_beam_wide_lm_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 4) and lib.pgasr_abi_version() == 7
    t = _tables()
    assert _search(lib, t, log_probs=0) == INVALID and _search(lib, t, blank=300) == INVALID
    assert _search(lib, t, V=1025) == UNSUPPORTED and _search(lib, t, beam=129, nbest=1) == UNSUPPORTED
    assert _search(lib, None, V=1025) == UNSUPPORTED                          # the limits before the model
    assert _search(lib, t, flags=2) == INVALID and _search(lib, t, nbest=9) == INVALID and _search(lib, t, out_count=0) == INVALID
    assert _search(lib, None) == INVALID and _search(lib, _tables(states=0)) == INVALID and _search(lib, _tables(succ=0)) == INVALID
    for kw in (dict(order=0), dict(order=6), dict(n_succ=(1 << 24) + 1), dict(n_states=(1 << 24) + 2)):
        assert _search(lib, _tables(**kw)) == UNSUPPORTED, kw
    for kw in (dict(vocab=299), dict(blank=1), dict(n_states=0), dict(n_succ=298), dict(start=-1), dict(start=400)):
        assert _search(lib, _tables(**kw)) == INVALID, kw
    assert _search(lib, t, alpha=float("nan")) == INVALID and _search(lib, t, beta=float("inf")) == INVALID
    assert _search(lib, _tables(order=6), ws=0) == UNSUPPORTED                # the model before the workspace
    trie, whole = lib.pgasr_beam_wide_workspace_bytes(10, 2, 300, 8), lib.pgasr_beam_wide_lm_workspace_bytes(10, 2, 300, 8)
    assert whole == trie + (2 * 2 * 8 * 2 * 300 * 4 + 255) // 256 * 256
    assert lib.pgasr_beam_wide_lm_workspace_bytes(0, 2, 300, 8) == 0
    assert _search(lib, t, ws=0) == WORKSPACE and _search(lib, t, ws_bytes=trie - 1) == WORKSPACE and _search(lib, t, ws_bytes=whole - 1) == WORKSPACE
    T = (1 << 22) // 128
    assert _search(lib, t, T=T, beam=128, nbest=1, tok_stride=T) == UNSUPPORTED

    def score(tables, tokens=16, stride=10, ln=16, count=16, N=4, B=2, V=300, blank=0, out=16):
        return lib.pgasr_nbest_unit_lm_score(tokens, stride, ln, count, N, B, V, blank, None if tables is None else ctypes.byref(tables), out, 0)
    assert score(t, N=0) == UNSUPPORTED and score(t, N=129) == UNSUPPORTED and score(t, V=1025) == UNSUPPORTED
    assert score(t, N=129, tokens=0) == UNSUPPORTED                           # the limits first
    for kw in (dict(tokens=0), dict(ln=0), dict(count=0), dict(out=0), dict(B=0), dict(stride=0), dict(blank=300), dict(blank=-1)):
        assert score(t, **kw) == INVALID, kw
    assert score(None) == INVALID and score(_tables(order=6)) == UNSUPPORTED and score(_tables(vocab=299)) == INVALID
