"""Word n-gram LM and lexicon fusion without a GPU: the identity that ties ``lm.WordFusion``'s bonuses to ``WordNgramLM.logp_sentence``,
the host model (trie, persistence, refusals), the new entry point's argument checks (CPU pointers: nothing could have run), the
refusals of the host layer before a device is touched, and the qualifying conditions of the shared GPU cases."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as L  # noqa: E402
import word_fusion_ref as W  # noqa: E402

from policy_gradient_asr_amd.lm import UNK, WordFusion, WordNgramLM  # noqa: E402

NEG_INF = -float("inf")


def _lm_with_long_words(V, blank, d, order, seed):
    """A word LM over V symbols whose lexicon holds a word of 32 tokens beside short ones (a word of 33 cannot be stored)."""
    rng = np.random.default_rng(100 * seed + V + order)
    symbols = [s for s in range(V) if s not in (blank, d)]
    ch = lambda t: chr(ord("a") + t)
    words = {tuple(rng.choice(symbols, size=int(rng.integers(1, 5))).tolist()) for _ in range(25)}
    long32 = tuple(rng.choice(symbols, size=32).tolist())
    words = sorted(words) + [long32]
    lines = [ch(d).join("".join(ch(t) for t in words[int(i)]) for i in rng.integers(0, len(words), size=int(rng.integers(1, 7))))
             for _ in range(80)]
    lm = WordNgramLM.from_text(lines, {ch(s): s for s in range(V)}, order=order, delimiter=ch(d), blank=blank)
    return lm, [tuple(s) for s in lm.spellings[3:]], long32


def _identity(fusion, y, alpha, beta):
    """(sum of the bonuses along y + final with eos, alpha * word_logp + beta * n_words + oov_penalty * n_oov)."""
    total = 0.0
    for i, s in enumerate(y):
        total = total + fusion.bonus(y[:i], s, alpha, beta)
    total = total + fusion.final(y, alpha, beta, eos=True)
    logp, n_words, n_oov = fusion.word_lm.logp_sentence(y, fusion.delimiter)
    return total, alpha * logp + beta * n_words + (fusion.oov_penalty * n_oov if n_oov else 0.0)


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("pen", [-1.75, NEG_INF])
def test_bonuses_add_up_to_the_sentence_score(order, pen):
    """The identity, within 1e-12 relative: random rows over alphabets of 5 to 8 symbols; rows that start with d, end with d or hold
    d d; a word of 32 tokens (in the lexicon) and one of 33 (in the sink by construction); a non-terminal prefix closed by d."""
    V = 5 + (order + (pen == NEG_INF)) % 4
    blank, d = (0, 1) if order % 2 else (V - 1, 0)
    lm, words, long32 = _lm_with_long_words(V, blank, d, order, order)
    fusion = WordFusion(lm, V, d, blank=blank, oov_penalty=pen)
    rng = np.random.default_rng(order)
    symbols = [s for s in range(V) if s != blank]
    other = next(s for s in symbols if s != d and s != long32[-1])
    proper = next(w[:k] for w in words for k in range(1, len(w)) if w[:k] not in set(words))        # a node that is no word
    rows = [tuple(rng.choice(symbols, size=int(rng.integers(0, 40))).tolist()) for _ in range(60)]
    for _ in range(40):                                         # sentences of lexicon words, some letters swapped
        y = []
        for i in rng.integers(0, len(words), size=int(rng.integers(1, 8))):
            y += [t if rng.random() > 0.1 else int(rng.choice(symbols)) for t in words[int(i)]] + [d]
        rows.append(tuple(y[:-1] if rng.random() < 0.5 else y))
    rows += [(), (d,), (d, d), (d,) + words[0], words[0] + (d,), words[0] + (d, d) + words[1], (d, d) + words[2] + (d, d),
             long32, long32 + (d,) + words[0], long32 + (other,), words[1] + (d,) + long32 + (other, d) + words[0],
             proper, proper + (d,), words[0] + (d,) + proper + (d,) + words[1]]
    oov_rows = finite_rows = 0
    for y in rows:
        got, want = _identity(fusion, y, 0.7, 1.3)
        n_oov = lm.logp_sentence(y, d)[2]
        oov_rows += n_oov > 0
        if want == NEG_INF:
            assert got == NEG_INF and pen == NEG_INF and n_oov > 0, y
        else:
            finite_rows += 1
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (y, got, want)
    assert oov_rows >= 10 and finite_rows >= 10
    assert lm.logp_sentence(long32, d)[2] == 0 and lm.logp_sentence(long32 + (other,), d)[2] == 1
    q = 0
    for t in long32:
        q = fusion.transition(q, t)[0]
    assert fusion.node_word[q] == lm.word_id(long32) and fusion.transition(q, other) == (fusion.sink, fusion.oov_penalty)
    assert fusion.transition(fusion.sink, other) == (fusion.sink, 0.0)


def test_trie_is_deterministic_and_survives_save_and_load(tmp_path):
    lm, words, _ = _lm_with_long_words(7, 0, 6, 3, 2)
    a = WordFusion(lm, 7, 6, oov_penalty=-2.5)
    b = WordFusion(WordNgramLM.load(_saved(lm, tmp_path)), 7, 6, oov_penalty=-2.5)
    for f in (a, b):
        S = f.n_states
        assert f.next.shape == f.trie_bonus.shape == (S, 7) and f.next.dtype == np.int32 and f.trie_bonus.dtype == np.float32
        assert f.node_word.shape == (S,) and f.node_word.dtype == np.int32 and f.node_word[0] == -1 and f.sink == S - 1
    assert np.array_equal(a.next, b.next) and np.array_equal(a.trie_bonus, b.trie_bonus) and np.array_equal(a.node_word, b.node_word)
    # breadth first, children by symbol: the children of all nodes, read node by node and symbol by symbol, are 1, 2, 3, ..
    kids = [int(a.next[q, s]) for q in range(a.sink) for s in range(1, 6) if a.next[q, s] != a.sink]
    assert kids == list(range(1, a.sink))
    assert sorted(int(w) for w in a.node_word[1:a.sink] if w != UNK) == list(range(3, lm.n_words))
    assert (a.next[:, 0] == np.arange(a.n_states)).all() and (a.next[:, 6] == 0).all() and not a.trie_bonus[:, 0].any()
    inner = (a.node_word == UNK) & (np.arange(a.n_states) != a.sink)
    assert (a.trie_bonus[inner, 6] == np.float32(-2.5)).all() and not a.trie_bonus[~inner, 6].any() and inner.any()
    path = str(tmp_path / "fusion.npz")
    a.save(path)
    c = WordFusion.load(path)
    assert (c.vocab, c.delimiter, c.blank, c.oov_penalty) == (7, 6, 0, -2.5) and c.word_lm.order == 3
    assert np.array_equal(a.next, c.next) and np.array_equal(a.trie_bonus, c.trie_bonus) and np.array_equal(a.node_word, c.node_word)
    y = words[0] + (6,) + words[1][:1] + (6, 3)
    assert _identity(a, y, 0.4, 0.9) == _identity(c, y, 0.4, 0.9)
    inf = WordFusion(lm, 7, 6, oov_penalty=NEG_INF)
    inf.save(path)
    assert WordFusion.load(path).oov_penalty == NEG_INF


def _saved(lm, tmp_path):
    path = str(tmp_path / "lm.npz")
    lm.save(path)
    return path


def test_host_model_refuses_by_argument_name():
    lm, words, _ = _lm_with_long_words(7, 0, 6, 2, 3)
    used = sorted({t for w in words for t in w})
    with pytest.raises(ValueError, match="delimiter"):
        WordFusion(lm, 7, used[0])                             # a delimiter inside a spelling
    with pytest.raises(ValueError, match="blank"):
        WordFusion(lm, 7, 6, blank=used[1])                    # a blank inside a spelling
    with pytest.raises(ValueError, match="vocab"):
        WordFusion(lm, 65, 6)
    with pytest.raises(ValueError, match="vocab"):
        WordFusion(lm, max(used), 0, blank=1)                  # a spelling holds a token outside the symbols
    with pytest.raises(ValueError, match="delimiter"):
        WordFusion(lm, 7, 0, blank=0)
    with pytest.raises(ValueError, match="delimiter"):
        WordFusion(lm, 7, 7)
    for bad in (0.25, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="oov_penalty"):
            WordFusion(lm, 7, 6, oov_penalty=bad)
    with pytest.raises(ValueError, match="word_lm"):
        WordFusion(object(), 7, 6)
    assert WordFusion(lm, 64, 6).vocab == 64


@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_gpu_cases_qualify(case):
    """Every utterance's helper gap is at least beam_lm_ref.GAP_MIN at N = min(beam, 16), and the fused 1-best differs from the
    unfused one for at least one utterance."""
    ref, plain = W.case_reference(case), W.plain_best(case)
    changed = 0
    for b in range(W.B):
        print(f"{W.case_id(case)} b={b}: gap {ref[b]['gap']:.3e} best {ref[b]['hyps'][0][0]} plain {plain[b]} own {ref[b]['own']}")
        assert ref[b]["gap"] >= L.GAP_MIN, (b, ref[b]["gap"])
        changed += tuple(ref[b]["hyps"][0][0]) != plain[b]
    assert changed >= 1
    d = case[4]
    assert max(sum(1 for t in r["hyps"][0][0] if t == d) for r in ref) >= 3           # words do complete


def test_the_case_list_covers_what_it_must():
    cases = W.CASES
    assert {c[2] for c in cases} >= {1, 16, 40, 100} and any(c[1] == 29 and c[2] * c[1] > 1024 for c in cases)
    assert all(5 <= c[1] <= 8 or c[1] == 29 for c in cases) and sum(c[1] == 29 for c in cases) == 1
    assert all(40 <= c[0] <= 150 for c in cases)
    assert {c[3] == 0 for c in cases} == {True, False} and any(c[3] == c[1] - 1 for c in cases)
    assert any(abs(c[4] - c[3]) == 1 for c in cases) and any(c[4] == c[1] - 1 for c in cases)
    assert {c[5] for c in cases} >= {1, 3, 5}
    assert any(c[6] == NEG_INF for c in cases) and any(np.isfinite(c[6]) for c in cases)
    assert {c[7] for c in cases} == {True, False} and {c[8] for c in cases} == {True, False}
    refs = [W.case_reference(c) for c in cases]
    # at least one case's finalisation changes rank 0, and at least one case runs the `own` path
    assert any(tuple(r["hyps"][0][0]) != tuple(r["search_best"]) for c, ref in zip(cases, refs) if c[7] for r in ref)
    assert any(r["own"] > 0 for ref in refs for r in ref)


# ---------------------------------------------------------------- ABI
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, 1, 3, 4


def _entry_args(T=6, B=2, V=29, beam=4, blank=0, flags=0, nbest=3, order=3, n_words=10, cap=16):
    """Valid arguments of the new entry, all in HOST memory and with NO workspace: whatever passes the checks stops at
    PGASR_ERR_WORKSPACE before any HIP call."""
    from policy_gradient_asr_amd import _lib
    keep = [np.zeros((T, B, V), dtype=np.float32), np.zeros((nbest, B, T), dtype=np.int32), np.zeros((nbest, B), dtype=np.int32),
            np.zeros((nbest, B), dtype=np.float64), np.zeros(B, dtype=np.int32), np.zeros(V * 4, dtype=np.int64),
            np.zeros(4, dtype=np.int32), np.zeros(n_words, dtype=np.float32), np.zeros((cap, 4), dtype=np.int32)]
    lp, tok, tl, sc, cnt, trie, node_word, uni, slots = (a.ctypes.data for a in keep)
    tables = _lib.WordLMTables(uni, uni, uni, uni, uni, slots, order, n_words, 16, cap, 0)
    keep.append(tables)
    head = [lp, 0, B * V, V, None, T, B, V, beam, blank, flags, nbest, tok, T, tl, sc, cnt, None, 0, None, None, 0, 0.0, 0.0]
    return keep, head, dict(trie=trie, trie_states=4, node_word=node_word, tables=ctypes.addressof(tables), delimiter=1, alpha=0.5,
                            beta=0.5, flags2=3)


def _run(fn, head, words, **change):
    w = dict(words, **change)
    return fn(*head, w["trie"], w["trie_states"], w["node_word"], w["tables"], w["delimiter"], w["alpha"], w["beta"], w["flags2"])


def test_entry_point_refuses_bad_arguments():
    from policy_gradient_asr_amd import _lib
    lib = _lib.load()
    fn = lib.pgasr_ctc_beam_search_words
    keep, head, words = _entry_args()
    assert _run(fn, head, words) == WORKSPACE                                     # good arguments stop at the workspace
    for name in ("trie", "node_word", "tables"):
        assert _run(fn, head, words, **{name: None}) == INVALID                   # null pointers
    assert _run(fn, head, words, trie_states=0) == INVALID and _run(fn, head, words, trie_states=-2) == INVALID
    assert _run(fn, head, words, trie_states=(1 << 24) // 29 + 1) == INVALID       # trie_states * V > 2^24
    assert _run(fn, head, words, trie_states=(1 << 24) // 29) == WORKSPACE
    for x in (float("nan"), float("inf"), -float("inf")):
        assert _run(fn, head, words, alpha=x) == INVALID and _run(fn, head, words, beta=x) == INVALID
    for dl in (-1, 29, 0):                                                        # outside [0, V), or the blank
        assert _run(fn, head, words, delimiter=dl) == INVALID
    assert _run(fn, head, words, flags2=4) == INVALID
    for f2 in (0, 1, 2):
        assert _run(fn, head, words, flags2=f2) == WORKSPACE
    for order in (0, 6, -1):
        k2, h2, w2 = _entry_args(order=order)
        assert _run(fn, h2, w2) == UNSUPPORTED
    for order in (1, 5):
        k2, h2, w2 = _entry_args(order=order)
        assert _run(fn, h2, w2) == WORKSPACE
    k2, h2, w2 = _entry_args(cap=12)
    assert _run(fn, h2, w2) == INVALID                                            # a capacity that is no power of two
    k2, h2, w2 = _entry_args(n_words=2)
    assert _run(fn, h2, w2) == INVALID
    k2, h2, w2 = _entry_args(V=65)
    assert _run(fn, h2, w2) == UNSUPPORTED                                        # V > 64
    k2, h2, w2 = _entry_args(beam=129)
    assert _run(fn, h2, w2) == UNSUPPORTED
    for flags in (8, 16, 24, 9):
        k2, h2, w2 = _entry_args(flags=flags)
        assert _run(fn, h2, w2) == UNSUPPORTED                                    # the single-wave kernel's bits
    table = np.zeros(29 ** 2, dtype=np.float32)
    h3 = list(head)
    h3[-4:] = [table.ctypes.data, 2, 0.5, 0.5]
    assert _run(fn, h3, words) == UNSUPPORTED                                     # a character table beside the word model
    k2, h2, w2 = _entry_args(nbest=3, beam=2)
    assert _run(fn, h2, w2) == INVALID                                            # the list's own checks: nbest > beam


def test_new_symbol_signature_and_abi_version():
    from policy_gradient_asr_amd import _lib
    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "policy_gradient_asr_amd",
                                   "libpgasr_hip.so"))
    assert hasattr(lib, "pgasr_ctc_beam_search_words")
    lib.pgasr_abi_version.restype = ctypes.c_int
    assert lib.pgasr_abi_version() == 7
    res, args = _lib.SIGNATURES["pgasr_ctc_beam_search_words"]
    assert res is ctypes.c_int and args[:len(_lib.SIGNATURES["pgasr_ctc_beam_search_nbest"][1])] == _lib.SIGNATURES["pgasr_ctc_beam_search_nbest"][1]
    assert args[-8:] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                         ctypes.c_int]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pgasr_hip.h")).read()
    assert "A7-WORDFUSE" in header and "pgasr_ctc_beam_search_words(" in header


# ---------------------------------------------------------------- host layer
def test_keyword_defaults():
    from policy_gradient_asr_amd import hipops, model
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    sig = inspect.signature(hipops.ctc_beam_search_words).parameters
    assert list(sig) == ["log_probs", "lengths", "beam", "nbest", "blank", "collapse", "fusion", "alpha", "beta", "finalize", "eos"]
    assert sig["finalize"].default is True and sig["eos"].default is True
    sig = inspect.signature(CTCDecoder.__init__).parameters
    assert [sig[k].default for k in ("fused_word_lm", "fused_word_alpha", "fused_word_beta", "word_delimiter", "oov_penalty")] == \
        [None, 0.0, 0.0, None, 0.0]
    sig = inspect.signature(model.predict).parameters
    assert [sig[k].default for k in ("fused_word_lm_path", "fused_word_alpha", "fused_word_beta", "oov_penalty")] == [None, 0.0, 0.0, 0.0]
    assert CTCDecoder(list("ab d")).fused_word_lm is None


def test_refusals_by_name_touch_no_device(tmp_path):
    """Every refusal raises a ValueError that names the option, on CPU tensors: a call that got past it would raise PgasrError
    (there is no CPU path) instead."""
    from policy_gradient_asr_amd import hipops, model
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    from policy_gradient_asr_amd.lm import CharNgramLM, HotwordBias
    lm, words, _ = _lm_with_long_words(7, 0, 6, 2, 4)
    fusion = WordFusion(lm, 7, 6, oov_penalty=-1.0)
    alphabet = list("_abcde ")
    lp = torch.zeros(4, 1, 7)
    with pytest.raises(ValueError, match="fusion"):
        hipops.ctc_beam_search_words(lp, None, fusion=lm)                         # only a WordFusion
    with pytest.raises(ValueError, match="fusion"):
        hipops.ctc_beam_search_words(torch.zeros(4, 1, 8), None, fusion=fusion)
    with pytest.raises(ValueError, match="fusion"):
        hipops.ctc_beam_search_words(lp, None, blank=3, fusion=fusion)
    with pytest.raises(ValueError, match="alpha"):
        hipops.ctc_beam_search_words(lp, None, fusion=fusion, alpha=float("inf"))
    with pytest.raises(ValueError, match="beta"):
        hipops.ctc_beam_search_words(lp, None, fusion=fusion, beta=float("nan"))
    clm = CharNgramLM(L.random_table(7, 2, 0, 0), 2)
    for name, kw in (("lm", dict(lm=clm)), ("hotwords", dict(hotwords=HotwordBias([(1, 2)], 7))), ("fast_lm", dict(fast_lm=True)),
                     ("wide_search", dict(wide_search=True))):
        with pytest.raises(ValueError, match=name):
            CTCDecoder(alphabet, fused_word_lm=fusion, **kw)
    with pytest.raises(ValueError, match="fused_word_lm"):
        CTCDecoder(list(range(70)), fused_word_lm=fusion)                         # more than 64 symbols
    with pytest.raises(ValueError, match="fused_word_lm"):
        CTCDecoder(alphabet, fused_word_lm="lm.npz")
    with pytest.raises(ValueError, match="oov_penalty"):
        CTCDecoder(alphabet, fused_word_lm=lm, oov_penalty=1.0)
    with pytest.raises(ValueError, match="word_delimiter"):
        CTCDecoder(list("_abcdef"), fused_word_lm=lm)                             # an alphabet without ' '
    dec = CTCDecoder(alphabet, fused_word_lm=lm, fused_word_alpha=0.5, fused_word_beta=1.0, oov_penalty=-1.0, device="cpu")
    assert isinstance(dec.fused_word_lm, WordFusion) and dec.fused_word_lm.delimiter == 6 and dec.fused_word_lm.oov_penalty == -1.0
    with pytest.raises(ValueError, match="lm"):
        dec.decode_batch(lp, None, lm=clm)
    with pytest.raises(ValueError, match="fast_lm"):
        dec.decode_batch(lp, None, fast_lm=True)
    with pytest.raises(ValueError, match="fused_word_lm"):
        dec.decode_batch(torch.zeros(4, 1, 70), None)
    with pytest.raises(ValueError, match="lm"):
        dec.decode(np.full((4, 7), 1 / 7), lm=clm)
    with pytest.raises(ValueError, match="hotwords"):
        dec.set_hotwords(["ab"])
    # T = 0 needs no device: the empty prefix with its finalisation
    want = -(0.0 + dec.fused_word_lm.final((), 0.5, 1.0, True))
    assert dec.decode(np.zeros((0, 7))) == (tuple(), want) and dec.decode(np.zeros((0, 7)), nbest=3) == [(tuple(), want)]
    # rescore(word_lm=) stays the second pass it is
    assert inspect.signature(CTCDecoder.rescore).parameters["word_lm"].default is None
    # predict
    path = str(tmp_path / "lm.npz")
    lm.save(path)
    narrow = tmp_path / "alphabet.txt"; narrow.write_text("a\nb\nc\n")
    wide = tmp_path / "units.txt"; wide.write_text("".join(f"{chr(0x100 + i)}\n" for i in range(80)))
    hot = tmp_path / "hot.txt"; hot.write_text("ab\n")
    common = dict(test_dataset=[], n_feats=8, fused_word_lm_path=path)
    with pytest.raises(ValueError, match="fused_word_lm_path"):
        model.predict(None, None, str(narrow), str(tmp_path), 2, beam_size=0, **common)
    for name, kw in (("lm_path", dict(lm_path="x.npz")), ("hotwords_path", dict(hotwords_path=str(hot))), ("lm_fast", dict(lm_fast=True)),
                     ("wide_beam", dict(wide_beam=True)), ("unit_lm_path", dict(unit_lm_path="x.npz", wide_beam=True))):
        with pytest.raises(ValueError, match=name):
            model.predict(None, None, str(narrow), str(tmp_path), 2, **kw, **common)
    with pytest.raises(ValueError, match="fused_word_lm_path"):
        model.predict(None, None, str(wide), str(tmp_path), 2, **common)          # more than 64 symbols
    with pytest.raises(ValueError, match="fused_word_lm_path"):
        model.predict(None, None, str(narrow), str(tmp_path), 2, **common)        # an alphabet without ' '
