"""A plain statement of the word n-gram LM of the second pass (include/pgasr_hip.h, A7-WORDLM), for the tests: a dict from n-gram
tuples to (logp, bow) filled from a model's fp32 arrays, the word split, the back-off score and the sentence score in numpy fp64,
the combine formula and the stable rank.  Nothing here knows of hash tables.  Also the shared, read-only cases of
tests/test_word_lm_gpu.py, whose premises tests/test_word_lm_cpu.py asserts on this file alone."""
import functools

import numpy as np

BOS, EOS, UNK = 0, 1, 2
MAX_WORD_LEN = 32


class Ref:
    """The model as dicts: ``grams`` from tuples of word ids to (logp, bow) in fp64, ``vocab`` from spellings (tuples of token
    ids) to word ids."""

    def __init__(self, lm):
        self.order = len(lm.ngrams)
        self.grams = {}
        for k in range(self.order):
            for row, lp, bw in zip(lm.ngrams[k].tolist(), lm.logp[k], lm.bow[k]):
                self.grams[tuple(row)] = (np.float64(lp), np.float64(bw))
        pool, off = lm.word_pool.tolist(), lm.word_off.tolist()
        self.vocab = {tuple(pool[off[i]:off[i + 1]]): i for i in range(3, len(off) - 1)}


def split(tokens, delimiter):
    """The maximal runs of non-delimiter tokens: str.split(), not str.split(" ")."""
    words, cur = [], []
    for t in list(tokens) + [delimiter]:
        if t == delimiter:
            if cur:
                words.append(tuple(cur))
            cur = []
        else:
            cur.append(int(t))
    return words


def word_id(ref, word):
    if len(word) > MAX_WORD_LEN:
        return UNK
    return ref.vocab.get(tuple(word), UNK)


def score(ref, hist, w):
    """(score(w | the last order-1 words of hist), how many times the context was shortened): fp64, from 0, the back-off weights
    from the longest context to the shortest, then the found logp."""
    h = tuple(hist)[len(hist) - (ref.order - 1):] if ref.order > 1 else ()
    acc, depth = np.float64(0.0), 0
    while (h + (w,)) not in ref.grams:
        if h in ref.grams:
            acc = acc + ref.grams[h][1]
        h = h[1:]
        depth += 1
    return acc + ref.grams[h + (w,)][0], depth


def sentence(ref, tokens, delimiter, depths=None):
    """(word_logp, n_words, n_oov) of a sentence of token ids."""
    ids = [word_id(ref, w) for w in split(tokens, delimiter)]
    hist = [BOS] * (ref.order - 1)
    total = np.float64(0.0)
    for w in ids + [EOS]:
        s, d = score(ref, hist, w)
        if depths is not None:
            depths.add(d)
        total = total + s
        hist.append(w)
    return total, len(ids), sum(1 for w in ids if w == UNK)


def list_ref(ref, tokens, lengths, count, delimiter, depths=None):
    """The three outputs of pgasr_nbest_word_lm_score for a list (N,B,stride) / (N,B) / (B)."""
    N, B, S = tokens.shape
    logp, nw, noov = np.zeros((N, B)), np.zeros((N, B), dtype=np.int32), np.zeros((N, B), dtype=np.int32)
    for b in range(B):
        for n in range(min(max(int(count[b]), 0), N)):
            L = min(max(int(lengths[n, b]), 0), S)
            logp[n, b], nw[n, b], noov[n, b] = sentence(ref, tokens[n, b, :L].tolist(), delimiter, depths)
    return logp, nw, noov


def combine_ref(base, word_logp, n_words, count, alpha, beta):
    """(total (N,B), order (B,N)) of pgasr_nbest_combine_rank: every product and sum rounded once."""
    base = np.asarray(base, dtype=np.float64)
    N, B = base.shape
    t2 = np.float64(alpha) * np.asarray(word_logp, dtype=np.float64)
    t3 = np.float64(beta) * np.asarray(n_words).astype(np.float64)
    with np.errstate(invalid="ignore"):
        total = (base + -t2) + -t3
    total = np.where(np.isfinite(base), total, np.inf)
    total = np.where(np.isnan(total), np.inf, total)
    order = np.zeros((B, N), dtype=np.int32)
    for b in range(B):
        c = min(max(int(count[b]), 0), N)
        total[c:, b] = np.inf
        order[b] = sorted(range(c), key=lambda n: (total[n, b], n)) + list(range(c, N))
    return total, order


# ------------------------------------------------------------------------------------------ the shared test model
LETTERS = "abcdef"
ALPHABET = ["<pad>", " "] + list(LETTERS)
CHAR2IND = {c: i for i, c in enumerate(ALPHABET)}
V, DELIM = len(ALPHABET), CHAR2IND[" "]
LONG = ("abcdef" * 6)[:32]                      # a vocabulary word of exactly MAX_WORD_LEN tokens
NON_WORDS = ("ce", "ec")                        # two-letter strings kept out of the vocabulary


def vocabulary():
    two = [a + b for a in LETTERS for b in LETTERS if a != b and a + b not in NON_WORDS]
    return list(LETTERS) + two + ["abc", "def", "fed", "abcd", "cdef", "abcde", LONG]


@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.default_rng(5)
    words = vocabulary()
    p = 1.0 / np.arange(1, len(words) + 1)
    p /= p.sum()
    perm = rng.permutation(len(words))
    lines = [" ".join(words[perm[i]] for i in rng.choice(len(words), size=int(rng.integers(1, 9)), p=p)) for _ in range(70)]
    lines += [" ".join(words), "ab cd", "ab cd ef", LONG + " a " + LONG]      # every word at least once
    return tuple(lines)


@functools.lru_cache(maxsize=None)
def model(order):
    from policy_gradient_asr_amd.lm import WordNgramLM
    return WordNgramLM.from_text(corpus(), CHAR2IND, order=order)


def enc(text):
    return [CHAR2IND[c] for c in text]


STRIDE = 600
EDGE_LENGTHS = (0, 1, 63, 64, 65, 128, 129, STRIDE)
WORD_COUNTS = (1, 64, 65, 129, 256, 257)        # the loop edges of a wave and of the 256-thread workgroup


@functools.lru_cache(maxsize=None)
def rows():
    """Named token rows (lists of ints), every one at most STRIDE long."""
    rng = np.random.default_rng(11)
    lines, words = corpus(), vocabulary()
    text = " ".join(lines[i] for i in rng.permutation(len(lines)))
    out = {}
    for L in EDGE_LENGTHS:
        out[f"len-{L}"] = enc(text[7:7 + L])                                   # cut anywhere: a cut word is usually no word
    out["only-delimiter"] = [DELIM]
    out["only-delimiters"] = [DELIM] * 5
    out["delimiter-first"] = enc(" " + lines[0])
    out["delimiter-last"] = enc(lines[1] + " ")
    out["doubled"] = enc("ab  cd   ef " + lines[2].replace(" ", "  "))
    t = list(enc((lines[3] + " " + lines[4] + " " + lines[5] + " " + text)[:100]))
    t[63] = t[64] = DELIM
    out["delimiters-63-64"] = t
    out["straddle"] = enc("a " * 31 + "abcd " + "b " * 30 + "abcd")         # 'abcd' on 62..65 and on 127..130
    out["word-32"] = enc("a " + LONG + " b")
    out["word-33"] = enc("a " + LONG + "a b")
    out["word-32-other"] = enc(LONG[:31] + ("a" if LONG[31] != "a" else "b"))
    out["blank-inside"] = enc("ab a ") +[CHAR2IND["a"], 0, CHAR2IND["b"]] + enc(" cd")
    out["out-of-range"] = enc("ab ") + [CHAR2IND["a"], 300, CHAR2IND["b"], DELIM, -1, DELIM, 256 + CHAR2IND["a"], DELIM] + enc("cd")
    for k in WORD_COUNTS:
        out[f"words-{k}"] = enc(" ".join(words[int(i)] if len(words[int(i)]) < 2 else "a" for i in rng.integers(0, 12, size=k)))
    for i in range(6):
        out[f"lines-{i}"] = enc(" ".join(lines[int(j)] for j in rng.integers(0, len(lines), size=4)))
        out[f"random-{i}"] = enc(" ".join(words[int(j)] for j in rng.integers(0, len(words) - 1, size=12)))
    assert all(len(r) <= STRIDE for r in out.values())
    return out


LISTS = ("n5-b3", "n128-b1", "n1-b1")


@functools.lru_cache(maxsize=None)
def list_case(name):
    """(tokens (N,B,STRIDE), lengths (N,B), count (B)) int32: the rows above in turn; behind every length the row holds letters,
    never zeros, and one length of every list is beyond the stride (it is clamped)."""
    N, B = {"n5-b3": (5, 3), "n128-b1": (128, 1), "n1-b1": (1, 1)}[name]
    rng = np.random.default_rng(N)
    pool = list(rows().values())
    tokens = rng.integers(2, V, size=(N, B, STRIDE)).astype(np.int32)
    lengths = np.zeros((N, B), dtype=np.int32)
    start = {"n5-b3": 0, "n128-b1": 0, "n1-b1": list(rows()).index("straddle")}[name]
    for n in range(N):
        for b in range(B):
            r = pool[(start + n * B + b) % len(pool)]
            tokens[n, b, :len(r)] = r
            lengths[n, b] = len(r)
    count = np.array({"n5-b3": [5, 3, 0], "n128-b1": [100], "n1-b1": [1]}[name], dtype=np.int32)
    full = [(n, b) for n in range(N) for b in range(B) if lengths[n, b] == STRIDE and n < count[b]]
    if full:
        lengths[full[0]] = STRIDE + 50
    tokens.setflags(write=False); lengths.setflags(write=False); count.setflags(write=False)
    return tokens, lengths, count


def combine_case():
    """base with exact ties, +inf, -inf and NaN, rows beyond count, and two rows equal in everything (a tie of the totals)."""
    rng = np.random.default_rng(3)
    N, B = 16, 4
    base = np.round(rng.normal(50.0, 5.0, size=(N, B)), 1)
    logp = -np.round(rng.uniform(5.0, 40.0, size=(N, B)), 3)
    nw = rng.integers(0, 12, size=(N, B)).astype(np.int32)
    base[3, 0] = base[7, 0] = base[1, 0]; logp[3, 0] = logp[7, 0] = logp[1, 0]; nw[3, 0] = nw[7, 0] = nw[1, 0]
    base[2, 1], base[5, 1], base[9, 1] = np.inf, np.nan, -np.inf
    base[:, 2] = 7.0; logp[:, 2] = -3.0; nw[:, 2] = 2                            # all tied: the list's order
    count = np.array([16, 12, 16, 0], dtype=np.int32)
    return base, logp, nw, count
