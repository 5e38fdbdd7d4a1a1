"""The word n-gram LM of the second pass on a GPU-less host: ``lm.WordNgramLM``'s smoothing against Witten-Bell values worked out by
hand, its ARPA reader on hand-checked queries, the round trips, the packed tables under a numpy emulation of the device's probe,
the two new entry points' export, binding and refusals (all before any HIP call), the host layer's refusals and unchanged defaults,
and the premises of the generated cases tests/test_word_lm_gpu.py compares the device on -- asserted on tests/word_lm_ref.py alone.
Words are confirmed on their full spelling (there is no fingerprint narrower than the spelling), so the collision cases here are
words that share a home slot."""
import ctypes
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import word_lm_ref as W  # noqa: E402
from policy_gradient_asr_amd import lm as L  # noqa: E402

HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
INVALID_ARG, UNSUPPORTED = 1, 4
LN10 = math.log(10.0)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def _entry(m, *words):
    """(logp, bow) of the stored n-gram of these words ('<s>', '</s>', '<unk>' or a spelling in W.CHAR2IND), as float64."""
    ids = tuple({"<s>": L.BOS, "</s>": L.EOS, "<unk>": L.UNK}.get(w, None) if w.startswith("<") else m.word_id(W.enc(w)) for w in words)
    k = len(ids)
    hit = np.flatnonzero((m.ngrams[k - 1] == np.array(ids)).all(axis=1))
    assert hit.size == 1, words
    return float(m.logp[k - 1][hit[0]]), float(m.bow[k - 1][hit[0]])


# ------------------------------------------------------------------------------------------ smoothing
def test_witten_bell_on_a_hand_corpus():
    """'a b a' / 'a c' / 'b a b': 11 predicted tokens (a 4, b 3, c 1, </s> 3), 4 distinct; p_0 = 1 / (3 words + 2)."""
    m = L.WordNgramLM.from_text(["a b a", "a c", "b a b\n"], W.CHAR2IND, order=3)
    p0 = 1.0 / 5.0
    uni = {w: (c + 4 * p0) / (11 + 4) for w, c in (("a", 4), ("b", 3), ("c", 1), ("</s>", 3), ("<unk>", 0))}
    for w, p in uni.items():
        assert _entry(m, w)[0] == pytest.approx(math.log(p), rel=1e-6), w
    assert _entry(m, "<s>")[0] == pytest.approx(-99.0 * LN10, rel=1e-6)
    # after <s>: a, a, b -- 3 tokens, 2 distinct; after a: b, </s>, c, b -- 4 tokens, 3 distinct; after b: a, a, </s> -- 3 and 2
    assert _entry(m, "<s>")[1] == pytest.approx(math.log(2 / 5), rel=1e-6)
    assert _entry(m, "a")[1] == pytest.approx(math.log(3 / 7), rel=1e-6)
    assert _entry(m, "b")[1] == pytest.approx(math.log(2 / 5), rel=1e-6)
    assert _entry(m, "c")[1] == pytest.approx(math.log(1 / 2), rel=1e-6)                     # after c: </s> once
    p_a_s = (2 + 2 * uni["a"]) / 5
    p_b_a = (2 + 3 * uni["b"]) / 7
    p_c_a = (1 + 3 * uni["c"]) / 7
    p_e_c = (1 + 1 * uni["</s>"]) / 2
    assert _entry(m, "<s>", "a")[0] == pytest.approx(math.log(p_a_s), rel=1e-6)
    assert _entry(m, "a", "b")[0] == pytest.approx(math.log(p_b_a), rel=1e-6)
    assert _entry(m, "a", "c")[0] == pytest.approx(math.log(p_c_a), rel=1e-6)
    assert _entry(m, "c", "</s>")[0] == pytest.approx(math.log(p_e_c), rel=1e-6)
    # order 3: after (<s>, a): b, c -- 2 tokens, 2 distinct; after (a, c): </s> once
    assert _entry(m, "<s>", "a")[1] == pytest.approx(math.log(2 / 4), rel=1e-6)
    assert _entry(m, "<s>", "a", "b")[0] == pytest.approx(math.log((1 + 2 * p_b_a) / 4), rel=1e-6)
    assert _entry(m, "<s>", "a", "c")[0] == pytest.approx(math.log((1 + 2 * p_c_a) / 4), rel=1e-6)
    assert _entry(m, "a", "c", "</s>")[0] == pytest.approx(math.log((1 + 1 * p_e_c) / 2), rel=1e-6)
    # the sentence 'a c': (<s>, <s>, a) is not stored and neither is (<s>, <s>): weight 0, then (<s>, a); the rest is stored at order 3
    want = _entry(m, "<s>", "a")[0] + _entry(m, "<s>", "a", "c")[0] + _entry(m, "a", "c", "</s>")[0]
    assert m.logp_sentence(W.enc("a c")) == (want, 2, 0)
    with pytest.raises(ValueError):
        L.WordNgramLM.from_text(["a z"], W.CHAR2IND)                                      # a character outside the alphabet
    with pytest.raises(ValueError):
        L.WordNgramLM.from_text(["a"], {"<pad>": 0, "a": 1})                              # no delimiter in the alphabet
    # min_count and the length limit: rare and over-long words count as <unk>
    m2 = L.WordNgramLM.from_text(["a b a", "a c", "a" * 33], W.CHAR2IND, order=2, min_count=2)
    assert [bytes(s) for s in m2.spellings[3:]] == [bytes(W.enc("a"))]
    assert m2.logp_sentence(W.enc("b"))[2] == 1 and m2.logp_sentence(W.enc("a" * 33))[2] == 1


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_every_stored_context_sums_to_one(order):
    m = L.WordNgramLM.from_text(W.corpus()[:12], W.CHAR2IND, order=order)
    contexts = [()]
    for k in range(1, order):
        contexts += [tuple(r) for r in m.ngrams[k - 1].tolist() if r[-1] != L.EOS]
    assert len(contexts) > 10 * (order - 1)
    for h in contexts:
        s = sum(math.exp(m.score(h, w)) for w in range(1, m.n_words))                    # </s>, <unk> and every word; <s> is never predicted
        assert abs(s - 1.0) < 1e-6, (h, s)


# ------------------------------------------------------------------------------------------ ARPA
ARPA = """\\data\\
ngram 1=6
ngram 2=6
ngram 3=2

\\1-grams:
-99\t<s>\t-0.5
-1.0\t</s>
-2.0\t<unk>\t-0.25
-0.5\tab\t-0.3
-0.7\tcd\t-0.4
-1.1\te\t-0.2

\\2-grams:
-0.2\t<s> ab\t-0.1
-0.4\tab cd\t-0.15
-0.8\tab e
-0.6\tcd </s>
-0.9\t<unk> cd\t-0.05
-0.35\te ab

\\3-grams:
-0.05\t<s> ab cd
-0.3\tab cd </s>

\\end\\
"""


def _f(x):
    return float(np.float32(x * LN10))              # a stored value: log10 -> ln, rounded to fp32, widened again


def _sum(*groups):
    """The contractual sum: per word from 0 its terms in order, the words added in order."""
    total = 0.0
    for g in groups:
        acc = 0.0
        for x in g:
            acc = acc + _f(x)
        total = total + acc
    return total


def test_arpa_queries_by_hand(tmp_path):
    path = tmp_path / "hand.arpa"
    path.write_text(ARPA)
    m = L.WordNgramLM.from_arpa(str(path), W.CHAR2IND)
    assert m.order == 3 and m.n_words == 6 and [g.shape[0] for g in m.ngrams] == [6, 6, 2]
    q = lambda text: m.logp_sentence(W.enc(text))
    # 'ab cd': ab through the missing contexts (<s>,<s>) (weight 0) to (<s>,ab); cd and </s> stored at the top order
    assert q("ab cd") == (_sum([-0.2], [-0.05], [-0.3]), 2, 0)
    # 'ab e': one back-off -- bow(<s>,ab), then (ab,e); </s> after (ab,e): that bigram has no weight given (0), (e,</s>) is missing:
    # bow(e), the unigram
    assert q("ab e") == (_sum([-0.2], [-0.1, -0.8], [0.0, -0.2, -1.0]), 2, 0)
    # 'cd ab': down to the unigrams -- bow(<s>); missing (<s>,cd) then bow(cd); missing (cd,ab) then bow(ab)
    assert q("cd ab") == (_sum([-0.5, -0.7], [-0.4, -0.5], [-0.3, -1.0]), 2, 0)
    # 'ee cd': an OOV as the word -- bow(<s>) and <unk>'s unigram --, then in the context: (<unk>,cd) is stored; then its bow and (cd,</s>)
    assert q("ee cd") == (_sum([-0.5, -2.0], [-0.9], [-0.05, -0.6]), 2, 1)
    # 'e ab cd': cd after (e,ab) -- (e,ab,cd) is missing, bow(e,ab) is 0 (none given), (ab,cd) is stored; (ab,cd,</s>) is stored
    assert q("e ab cd") == (_sum([-0.5, -1.1], [-0.35], [0.0, -0.4], [-0.3]), 3, 0)
    # 'ee cd e': e after (<unk>,cd) -- its bow, (cd,e) is missing, bow(cd), the unigram
    assert q("ee cd e")[0] == _sum([-0.5, -2.0], [-0.9], [-0.05, -0.4, -1.1], [-0.2, -1.0])
    # the empty sentence, and delimiters alone: score(</s> | <s>)
    assert q("") == (_sum([-0.5, -1.0]), 0, 0) == q("   ")
    # str.split(), not str.split(" ")
    assert q("  ab   cd ") == q("ab cd")
    # the plain reference says the same
    ref = W.Ref(m)
    for text in ("ab cd", "ab e", "cd ab", "ee cd", "e ab cd", "", " ab  cd"):
        assert W.sentence(ref, W.enc(text), W.DELIM) == q(text), text


def test_arpa_unspellable_words_and_round_trips(tmp_path):
    bad = ARPA.replace("ngram 1=6", "ngram 1=7").replace("-1.1\te\t-0.2\n", "-1.1\te\t-0.2\n-1.5\txyz\t-0.1\n")
    bad = bad.replace("-0.35\te ab\n", "-0.35\te ab\n-0.45\txyz ab\n")
    path = tmp_path / "bad.arpa"
    path.write_text(bad)
    with pytest.raises(ValueError):
        L.WordNgramLM.from_arpa(str(path), W.CHAR2IND)
    good = tmp_path / "good.arpa"
    good.write_text(ARPA)
    m, kept = L.WordNgramLM.from_arpa(str(good), W.CHAR2IND), L.WordNgramLM.from_arpa(str(path), W.CHAR2IND, skip_unknown=True)
    big = W.model(4)
    for a, name in ((m, "hand"), (big, "big")):
        out = tmp_path / (name + ".arpa")
        a.to_arpa(str(out), {i: c for c, i in W.CHAR2IND.items()})
        b = L.WordNgramLM.from_arpa(str(out), W.CHAR2IND)
        npz = tmp_path / (name + ".npz")
        a.save(str(npz))
        c = L.WordNgramLM.load(str(npz))
        for other in (b, c) + ((kept,) if name == "hand" else ()):
            assert other.order == a.order and (other.word_pool == a.word_pool).all() and (other.word_off == a.word_off).all()
            for k in range(a.order):
                assert (other.ngrams[k] == a.ngrams[k]).all() and other.logp[k].dtype == np.float32
                assert (other.logp[k] == a.logp[k]).all() and (other.bow[k] == a.bow[k]).all()
        assert c.delimiter == a.delimiter and c.blank == a.blank
    with np.load(str(tmp_path / "big.npz"), allow_pickle=False) as z:
        assert "word_pool" in z.files


def test_constructor_refusals():
    m = W.model(2)
    args = lambda: dict(word_pool=m.word_pool.copy(), word_off=m.word_off.copy(), ngrams=[g.copy() for g in m.ngrams],
                        logp=[x.copy() for x in m.logp], bow=[x.copy() for x in m.bow])
    L.WordNgramLM(**args())
    a = args(); a["ngrams"] = a["ngrams"] * 3; a["logp"] = a["logp"] * 3; a["bow"] = a["bow"] * 3           # order 6
    with pytest.raises(ValueError):
        L.WordNgramLM(**a)
    a = args(); a["logp"][1][0] = np.inf
    with pytest.raises(ValueError):
        L.WordNgramLM(**a)
    a = args(); a["ngrams"][1] = a["ngrams"][1][::-1]                                                        # not in canonical order
    with pytest.raises(ValueError):
        L.WordNgramLM(**a)
    a = args(); a["ngrams"][0] = a["ngrams"][0][:-1]; a["logp"][0] = a["logp"][0][:-1]; a["bow"][0] = a["bow"][0][:-1]
    with pytest.raises(ValueError):
        L.WordNgramLM(**a)                                                                                    # a word without a unigram
    a = args(); a["word_pool"][0] = 0                                                                        # the blank in a spelling
    with pytest.raises(ValueError):
        L.WordNgramLM(**a)
    # an n-gram whose context is not stored
    m3 = W.model(3)
    a = dict(word_pool=m3.word_pool, word_off=m3.word_off, ngrams=[m3.ngrams[0], m3.ngrams[1][1:], m3.ngrams[2]],
             logp=[m3.logp[0], m3.logp[1][1:], m3.logp[2]], bow=[m3.bow[0], m3.bow[1][1:], m3.bow[2]])
    assert (m3.ngrams[2][:, :2] == m3.ngrams[1][0]).all(axis=1).any()
    with pytest.raises(ValueError):
        L.WordNgramLM(**a)
    # the limits are checked, never applied by truncation: 2^22 + 1 words
    n = L.MAX_WORDS + 1
    with pytest.raises(ValueError, match="2\\*\\*22"):
        L.WordNgramLM(np.zeros(n - 3, dtype=np.uint8) + 2, np.concatenate([[0, 0, 0], np.arange(n - 2)]), [np.arange(n)[:, None]],
                      [np.zeros(n, dtype=np.float32)], [np.zeros(n, dtype=np.float32)])


# ------------------------------------------------------------------------------------------ packing
def _probe_word(p, spelling):
    """The device's word lookup in numpy: (word id or -1, slots visited)."""
    cap = p["word_slots"].size
    s = int(L.hash_word([bytes(spelling)])[0]) & (cap - 1)
    for step in range(1, cap + 1):
        e = int(p["word_slots"][s])
        if e < 0:
            return -1, step
        if bytes(p["word_pool"][p["word_off"][e]:p["word_off"][e + 1]]) == bytes(spelling):
            return e, step
        s = (s + 1) & (cap - 1)
    raise AssertionError("a full table")


def _probe_ngram(p, ctx, word):
    cap = p["ngram_slots"].shape[0]
    s = int(L.hash_ngram([ctx], [word])[0] & np.uint64(cap - 1))
    for step in range(1, cap + 1):
        c, w = int(p["ngram_slots"][s, 0]), int(p["ngram_slots"][s, 1])
        if c < 0:
            return -1, step
        if (c, w) == (ctx, word):
            return s, step
        s = (s + 1) & (cap - 1)
    raise AssertionError("a full table")


def test_hashes_are_the_documented_integer_functions():
    h = 2166136261
    for c in b"\x02\x03":
        h = ((h ^ c) * 16777619) % 2 ** 32
    h ^= h >> 16; h = h * 0x85EBCA6B % 2 ** 32; h ^= h >> 13; h = h * 0xC2B2AE35 % 2 ** 32; h ^= h >> 16
    assert int(L.hash_word([b"\x02\x03"])[0]) == h
    x = (77 << 32) | 5
    x ^= x >> 30; x = x * 0xBF58476D1CE4E5B9 % 2 ** 64; x ^= x >> 27; x = x * 0x94D049BB133111EB % 2 ** 64; x ^= x >> 31
    assert int(L.hash_ngram([77], [5])[0]) == x
    src = open(os.path.join(ROOT, "policy_gradient_asr_amd", "csrc", "word_lm.hip")).read()
    for const in ("2166136261u", "16777619u", "0x85EBCA6Bu", "0xC2B2AE35u", "0xBF58476D1CE4E5B9ull", "0x94D049BB133111EBull"):
        assert const in src, const


def test_the_probe_finds_every_word_and_every_ngram_of_the_packed_model():
    m = W.model(5)
    p = m.pack()
    assert m.pack() is p                                                                   # made once
    wcap, ncap = p["word_slots"].size, p["ngram_slots"].shape[0]
    n_high = sum(g.shape[0] for g in m.ngrams[1:])
    assert wcap & (wcap - 1) == 0 and ncap & (ncap - 1) == 0
    assert 2 * (m.n_words - 3) <= wcap < 4 * (m.n_words - 3) and 2 * n_high <= ncap < 4 * n_high      # load factor in (0.25, 0.5]
    assert (p["word_slots"] >= 0).sum() == m.n_words - 3 and (p["ngram_slots"][:, 0] >= 0).sum() == n_high
    longest = 0
    for i in range(3, m.n_words):
        e, steps = _probe_word(p, m.spellings[i])
        assert e == i
        longest = max(longest, steps)
    assert longest >= 3                                                                    # chains of colliding words exist
    # every n-gram through its chain of contexts, as the kernel walks them
    longest = 0
    for k in range(2, m.order + 1):
        for row, lp, bw in zip(m.ngrams[k - 1].tolist(), m.logp[k - 1], m.bow[k - 1]):
            e = row[0]
            for w in row[1:]:
                s, steps = _probe_ngram(p, e, w)
                assert s >= 0, row
                longest = max(longest, steps)
                e = m.n_words + s
            assert p["ngram_slots"][s, 2:].view(np.float32).tolist() == [lp, bw]
    assert longest >= 3
    assert (p["uni_logp"] == m.logp[0]).all() and (p["uni_bow"] == m.bow[0]).all()
    # words outside the vocabulary that start on the home slot of a vocabulary word are not taken for it
    homes = {int(h) & (wcap - 1) for h in L.hash_word(m.spellings[3:])}
    rng = np.random.default_rng(0)
    clash = 0
    for _ in range(400):
        w = bytes(rng.integers(2, W.V, size=int(rng.integers(3, 9))).tolist())
        if w in m._word_id:
            continue
        clash += (int(L.hash_word([w])[0]) & (wcap - 1)) in homes
        assert _probe_word(p, w)[0] == -1
    assert clash >= 50
    assert _probe_ngram(p, 3, L.BOS)[0] == -1                                              # <s> is never predicted


# ------------------------------------------------------------------------------------------ ABI and refusals
def test_new_symbols_exported_and_bound_abi_stays_7(lib):
    from policy_gradient_asr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in (("pgasr_nbest_word_lm_score", 12), ("pgasr_nbest_combine_rank", 11)):
        assert hasattr(lib, name)
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]) == nargs
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    assert _lib.SIGNATURES["pgasr_nbest_combine_rank"][1][6:8] == [ctypes.c_double, ctypes.c_double]
    assert int(re.search(r"#define PGASR_ABI_VERSION (\d+)", src).group(1)) == 7 and lib.pgasr_abi_version() == 7
    assert "A7-WORDLM" in open(HEADER).read() and "A7-WORDLM" in open(os.path.join(ROOT, "policy_gradient_asr_amd", "csrc",
                                                                                     "word_lm.hip")).read()
    # the ctypes struct is the header's: six pointers, six 32-bit integers
    body = re.search(r"typedef struct pgasr_word_lm_tables \{(.*?)\}", src, flags=re.S).group(1)
    assert body.count("*") == 6 and [f[0] for f in _lib.WordLMTables._fields_[6:]] == \
        [x.strip() for x in re.search(r"int32_t ([^;]*);", body).group(1).split(",")]
    assert ctypes.sizeof(_lib.WordLMTables) == 6 * 8 + 6 * 4
    assert int(re.search(r"#define PGASR_WORD_LM_MAX_STRIDE (\d+)", src).group(1)) >= 4096


P = 0x1000          # fake pointers: every call below must return before dereferencing or launching anything


def _tables(**kw):
    from policy_gradient_asr_amd import _lib
    f = dict(word_pool=P, word_off=P, word_slots=P, uni_logp=P, uni_bow=P, ngram_slots=P, order=3, n_words=10, word_cap=16,
             ngram_cap=64, pool_bytes=40, reserved=0)
    f.update(kw)
    return _lib.WordLMTables(**f)


def _score(lib, N=4, B=2, stride=10, delim=1, tokens=P, length=P, count=P, logp=P, words=P, oov=P, tables=None, **kw):
    t = _tables(**kw) if tables is None else tables
    return lib.pgasr_nbest_word_lm_score(tokens, stride, length, count, N, B, delim, None if t is False else ctypes.byref(t),
                                         logp, words, oov, None)


def test_word_lm_score_refusals_need_no_device(lib):
    assert _score(lib, order=0) == UNSUPPORTED and _score(lib, order=6) == UNSUPPORTED
    assert _score(lib, N=0) == UNSUPPORTED and _score(lib, N=129) == UNSUPPORTED
    assert _score(lib, stride=4097) == UNSUPPORTED
    assert _score(lib, n_words=(1 << 22) + 1, word_cap=1 << 24) == UNSUPPORTED and _score(lib, ngram_cap=1 << 26) == UNSUPPORTED
    for name in ("tokens", "length", "count", "logp", "words", "oov"):
        assert _score(lib, **{name: None}) == INVALID_ARG, name
    for name in ("word_pool", "word_off", "word_slots", "uni_logp", "uni_bow", "ngram_slots"):
        assert _score(lib, **{name: None}) == INVALID_ARG, name
    assert _score(lib, tables=False) == INVALID_ARG
    assert _score(lib, B=0) == INVALID_ARG and _score(lib, stride=0) == INVALID_ARG
    # inconsistent sizes: fewer than the reserved words, capacities that are no powers of two, a word table more than half full, a pool
    # longer than 32 bytes per word or of negative size
    assert _score(lib, n_words=2) == INVALID_ARG
    assert _score(lib, word_cap=12) == INVALID_ARG and _score(lib, ngram_cap=0) == INVALID_ARG and _score(lib, ngram_cap=48) == INVALID_ARG
    assert _score(lib, n_words=12) == INVALID_ARG
    assert _score(lib, pool_bytes=7 * 32 + 1) == INVALID_ARG and _score(lib, pool_bytes=-1) == INVALID_ARG
    assert _score(lib, order=6, tokens=None) == UNSUPPORTED                               # the limits come first


def _combine(lib, N=4, B=2, alpha=0.5, beta=0.5, base=P, logp=P, words=P, count=P, total=P, order=P):
    return lib.pgasr_nbest_combine_rank(base, logp, words, count, N, B, alpha, beta, total, order, None)


def test_combine_rank_refusals_need_no_device(lib):
    assert _combine(lib, N=0) == UNSUPPORTED and _combine(lib, N=129) == UNSUPPORTED
    for name in ("base", "logp", "words", "count", "total", "order"):
        assert _combine(lib, **{name: None}) == INVALID_ARG, name
    assert _combine(lib, B=0) == INVALID_ARG
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert _combine(lib, alpha=bad) == INVALID_ARG and _combine(lib, beta=bad) == INVALID_ARG
    assert _combine(lib, N=129, alpha=float("nan")) == UNSUPPORTED


# ------------------------------------------------------------------------------------------ the host layer
def test_host_layer_refusals_and_unchanged_defaults(tmp_path):
    import torch
    from policy_gradient_asr_amd import hipops, model, _lib
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder, NBestRescored, NBestRescoredWords
    tok, ln, cnt = torch.zeros(2, 1, 4, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    with pytest.raises(_lib.PgasrError):
        hipops.nbest_word_lm_score(tok, ln, cnt, W.model(2), W.DELIM)                      # no CPU path
    with pytest.raises(_lib.PgasrError):
        hipops.nbest_combine_rank(torch.zeros(2, 1, dtype=torch.float64), torch.zeros(2, 1, dtype=torch.float64), ln, cnt)
    assert NBestRescoredWords._fields == NBestRescored._fields + ("word_logp", "n_words", "n_oov") and len(NBestRescored._fields) == 7
    sig = inspect.signature(CTCDecoder.rescore).parameters
    assert [sig[k].default for k in ("word_lm", "word_lm_alpha", "word_lm_beta", "word_delimiter")] == [None, 0.0, 0.0, None]
    assert [sig[k].default for k in ("acoustic", "am_weight", "max_hyp_len", "blank")] == ["ctc", 1.0, None, 0]
    sig = inspect.signature(CTCDecoder.mbr_decode).parameters
    assert [sig[k].default for k in ("word_lm", "word_lm_alpha", "word_lm_beta")] == [None, 0.0, 0.0]
    nb = hipops.CTCNBest(tok, ln, torch.zeros(2, 1, dtype=torch.float64), cnt)
    lp = torch.zeros(4, 1, 5)
    with pytest.raises(ValueError, match="delimiter"):
        CTCDecoder(list("abcde")).rescore(lp, None, nb, word_lm=W.model(2))               # an alphabet without ' '
    assert CTCDecoder(W.ALPHABET)._word_delimiter(None) == W.DELIM and CTCDecoder(list("abcde"))._word_delimiter(3) == 3
    sig = inspect.signature(model.predict).parameters
    assert [sig[k].default for k in ("rescore_word_lm_path", "rescore_word_alpha", "rescore_word_beta")] == [None, 0.0, 0.0]
    assert [sig[k].default for k in ("beam_size", "nbest", "rescore_lm_path", "mbr")] == [5, 1, None, False]
    with pytest.raises(ValueError):
        model.predict(None, None, os.devnull, os.devnull, 1, rescore_word_lm_path="x.npz")            # needs a list
    sig = inspect.signature(model.build_word_lm).parameters
    assert [sig[k].default for k in ("order", "min_count")] == [3, 1]
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    (corpus / "alphabet.txt").write_text(" \na\nb\nc\nd\ne\nf\n")
    got = model.build_word_lm(str(corpus), order=2, train_dataset=[{"trans": t} for t in W.corpus()])
    assert os.path.exists(corpus / "word_lm.npz") and (L.WordNgramLM.load(str(corpus / "word_lm.npz")).logp[1] == got.logp[1]).all()
    assert (got.logp[1] == W.model(2).logp[1]).all() and got.delimiter == W.DELIM


# ------------------------------------------------------------------------------------------ premises of the GPU cases
def test_rows_hold_what_they_are_meant_to():
    rows = W.rows()
    ref = W.Ref(W.model(3))
    assert sorted(len(rows[f"len-{n}"]) for n in W.EDGE_LENGTHS) == sorted(W.EDGE_LENGTHS)
    assert rows["delimiter-first"][0] == W.DELIM and rows["delimiter-last"][-1] == W.DELIM
    assert rows["delimiters-63-64"][63] == rows["delimiters-63-64"][64] == W.DELIM
    assert any(a == b == W.DELIM for a, b in zip(rows["doubled"], rows["doubled"][1:]))
    assert W.sentence(ref, rows["only-delimiters"], W.DELIM)[1:] == (0, 0) == W.sentence(ref, rows["only-delimiter"], W.DELIM)[1:]
    for k in W.WORD_COUNTS:
        assert W.sentence(ref, rows[f"words-{k}"], W.DELIM)[1] == k
    assert {1, 64, 65, 129, 256, 257} <= set(W.WORD_COUNTS)
    # words of exactly 32 tokens (one in the vocabulary, one not) and of 33
    assert [len(w) for w in W.split(rows["word-32"], W.DELIM)] == [1, 32, 1] and W.sentence(ref, rows["word-32"], W.DELIM)[1:] == (3, 0)
    assert [len(w) for w in W.split(rows["word-33"], W.DELIM)] == [1, 33, 1] and W.sentence(ref, rows["word-33"], W.DELIM)[1:] == (3, 1)
    assert [len(w) for w in W.split(rows["word-32-other"], W.DELIM)] == [32] and W.sentence(ref, rows["word-32-other"], W.DELIM)[1:] == (1, 1)
    # a vocabulary word across positions 63 / 64 and across 127 / 128
    r = rows["straddle"]
    assert W.DELIM not in r[62:66] and r[61] == r[66] == W.DELIM and W.DELIM not in r[127:131] and r[126] == W.DELIM and len(r) == 131
    assert W.sentence(ref, r, W.DELIM)[2] == 0
    # the blank and out-of-range tokens inside words: those words are OOV, their neighbours are not; 258 is not 'a'
    assert 0 in rows["blank-inside"] and W.sentence(ref, rows["blank-inside"], W.DELIM)[1:] == (4, 1)
    assert {300, -1, 258} <= set(rows["out-of-range"]) and W.sentence(ref, rows["out-of-range"], W.DELIM)[1:] == (5, 3)
    assert W.word_id(ref, (258 & 255,)) != W.UNK


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_lists_reach_every_back_off_depth(order):
    ref = W.Ref(W.model(order))
    depths, oov = set(), 0
    for name in W.LISTS:
        tokens, lengths, count = W.list_case(name)
        N, B, S = tokens.shape
        assert S == W.STRIDE and (lengths > S).sum() == (1 if name != "n1-b1" else 0)
        for n in range(N):
            for b in range(B):
                L_ = min(int(lengths[n, b]), S)
                assert (tokens[n, b, L_:] >= 2).all()                                     # letters behind every length, never zeros
        logp, nw, noov = W.list_ref(ref, tokens, lengths, count, W.DELIM, depths)
        oov += int(noov.sum())
        assert np.isfinite(logp).all() and (logp[nw > 0] < 0).all()
        for b in range(B):
            assert (logp[count[b]:, b] == 0).all() and (nw[count[b]:, b] == 0).all()
    assert depths == set(range(order)) and oov >= 10
    assert {tuple(W.list_case(n)[0].shape[:2]) for n in W.LISTS} == {(5, 3), (128, 1), (1, 1)}
    assert 0 in W.list_case("n5-b3")[2] and (W.list_case("n128-b1")[2] < 128).all()


def test_combine_case_holds_ties_and_non_finite_bases():
    base, logp, nw, count = W.combine_case()
    total, order = W.combine_ref(base, logp, nw, count, 0.7, 1.3)
    assert total[1, 0] == total[3, 0] == total[7, 0] and list(order[0]).index(1) + 2 == list(order[0]).index(3) + 1 == list(order[0]).index(7)
    assert np.isinf(total[[2, 5, 9], 1]).all() and np.isinf(total[12:, 1]).all() and order[1, 12:].tolist() == [12, 13, 14, 15]
    assert set(order[1, 9:12].tolist()) == {2, 5, 9} and order[1, 9:12].tolist() == [2, 5, 9]
    assert order[2].tolist() == list(range(16)) and order[3].tolist() == list(range(16)) and np.isinf(total[:, 3]).all()
    # alpha = beta = 0 returns a finite base bit for bit
    t0, _ = W.combine_ref(base, logp, nw, count, 0.0, 0.0)
    assert (t0[:, 0] == base[:, 0]).all()
