"""Character n-gram language model for the fused CTC prefix beam search (csrc/beam.hip, ``pgasr_ctc_beam_search_lm``).

An LM of order ``n >= 1`` over ``V`` symbols is a dense fp32 table of natural-log probabilities of shape ``(V,)*n``:
``table[c_1, .., c_{n-1}, s] = ln p(s | c_1 .. c_{n-1})`` with ``c_{n-1}`` the most recent symbol.  The blank index never occurs
inside a prefix, so it serves as the start-of-sentence pad: the context of a prefix shorter than ``n-1`` is left-padded with
``blank``.  The column ``s == blank`` is never read and holds 0.  Building, saving and loading are host-side numpy work; the
search reads the table on the device (``device_table``).

``WordNgramLM`` is the word-level model of the second pass: a back-off n-gram model (ARPA form, order <= 5) over words spelled in
the acoustic alphabet, queried on the host by ``logp_sentence`` and on the device by csrc/word_lm.hip through ``device_tables``.

``WordFusion`` puts that word model and its vocabulary, as a lexicon trie, into the first pass itself (csrc/beam.hip WORDS = true,
``pgasr_ctc_beam_search_words``): it builds the trie the search reads and states every term the search adds (``bonus``, ``final``).

``UnitNgramLM`` is the sparse model over the acoustic units themselves, for alphabets the dense table cannot hold (up to 1024
symbols at order <= 5): a back-off n-gram model fused into the wide search (csrc/beam_wide.hip) and applied to N-best lists
(csrc/unit_lm.hip) through ``device_tables``, queried on the host by ``logp`` / ``logp_sequence``.

The two are the same ARPA-form model over different symbols, and what they share is stated once, in ``_BackoffNgramLM`` and the
functions before it: the per-order arrays and their checks, the canonical order (``_sorted_arrays``), the ARPA reader and writer,
the npz members, the Witten-Bell estimate in back-off form (``_witten_bell``), the dict of entries and the back-off walk.  The classes
keep what a symbol is, how n-grams are counted, their own checks and their ``pack()`` layouts.  ``_on_device`` is the one "tensor
once per device" rule of all three models."""
import collections
import math

import numpy as np

MAX_ENTRIES = 1 << 25      # V**n words (128 MiB): order 5 at V = 29, order 4 at V = 64 -- csrc/beam.hip refuses more


def _check_size(V, order):
    if isinstance(order, bool) or int(order) != order or order < 1:
        raise ValueError(f"LM order must be an integer >= 1 (got {order!r})")
    if V < 2:
        raise ValueError("an LM needs at least one symbol beside the blank")
    if V ** int(order) > MAX_ENTRIES:
        raise ValueError(f"an order-{order} table over {V} symbols has {V ** int(order)} entries; the limit is 2**25")


def _on_device(cache, device, make):
    """``make(device)``, made once per device and kept in ``cache``; a bare "cuda" is the current device."""
    import torch
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    t = cache.get(device)
    if t is None:
        t = cache[device] = make(device)
    return t


class CharNgramLM:
    def __init__(self, table, order, blank=0):
        table = np.ascontiguousarray(np.asarray(table), dtype=np.float32)
        if table.ndim < 1:
            raise ValueError("the LM table must have shape (V,)*order")
        V = table.shape[0]
        _check_size(V, order)
        order = int(order)
        if table.shape != (V,) * order:
            raise ValueError(f"the LM table must have shape (V,)*order = {(V,) * order}, not {table.shape}")
        if not 0 <= int(blank) < V:
            raise ValueError("blank must be a symbol of the table")
        # every entry the search can read must be finite (checked once, here): all columns but the blank one
        cols = np.moveaxis(table, -1, 0)
        for s in range(V):
            if s != int(blank) and not np.isfinite(cols[s]).all():
                raise ValueError(f"the LM table holds a non-finite log-probability for symbol {s}")
        self.table, self.order, self.blank, self.vocab = table, order, int(blank), V
        self._device_tables = {}

    # ---------------------------------------------------------------- construction
    @classmethod
    def from_transcripts(cls, seqs_of_token_ids, vocab, order=3, blank=0):
        """Interpolated Witten-Bell smoothing, dense, in float64 on the host:
            p_0(s)   = 1 / (V-1) for s != blank,
            p_k(s|h) = (c(h,s) + N1+(h.) p_{k-1}(s|h')) / (c(h) + N1+(h.)),  h' = h without its oldest symbol,
            p_k      = p_{k-1} where c(h) = 0,
        with c counted over the transcripts left-padded with order-1 blanks and N1+(h.) the number of distinct symbols seen
        after h.  Every probability of a non-blank symbol is positive, so every log is finite."""
        V, blank = int(vocab), int(blank)
        _check_size(V, order)
        order = int(order)
        if not 0 <= blank < V:
            raise ValueError("blank must be a symbol of the vocabulary")
        seqs = [np.asarray(list(s), dtype=np.int64).reshape(-1) for s in seqs_of_token_ids]
        for s in seqs:
            if s.size and (s.min() < 0 or s.max() >= V or (s == blank).any()):
                raise ValueError("transcripts must hold symbols of the vocabulary other than the blank")
        p = np.full(V, 1.0 / (V - 1))
        p[blank] = 0.0
        for k in range(1, order + 1):
            counts = np.zeros((V,) * k, dtype=np.float64)
            for s in seqs:
                if not s.size:
                    continue
                padded = np.concatenate([np.full(k - 1, blank, dtype=np.int64), s])
                idx = tuple(padded[i:i + s.size] for i in range(k))      # idx[k-1] = the symbol, idx[:k-1] its context
                np.add.at(counts, idx, 1.0)
            c_h = counts.sum(axis=-1, keepdims=True)
            n1 = (counts > 0).sum(axis=-1, keepdims=True).astype(np.float64)
            lower = np.broadcast_to(p, counts.shape)                        # p_{k-1}(s | h'): the oldest symbol is a new leading axis
            with np.errstate(invalid="ignore", divide="ignore"):
                p = np.where(c_h > 0, (counts + n1 * lower) / (c_h + n1), lower)
        with np.errstate(divide="ignore"):
            table = np.log(p)
        table[..., blank] = 0.0
        return cls(table.astype(np.float32), order, blank)

    @classmethod
    def from_text(cls, lines, char2ind, order=3, blank=0):
        """Lines of text -> token ids through ``char2ind`` (the alphabet's map, ``<pad>`` = blank = 0).  A character outside the
        alphabet raises."""
        vocab = max(char2ind.values()) + 1
        seqs = []
        for ln in lines:
            try:
                seqs.append([char2ind[c] for c in ln.rstrip("\n")])
            except KeyError as e:
                raise ValueError(f"character {e.args[0]!r} is not in the alphabet") from None
        return cls.from_transcripts(seqs, vocab, order=order, blank=blank)

    # ---------------------------------------------------------------- persistence
    def save(self, path):
        with open(path, "wb") as fo:
            np.savez(fo, table=self.table, order=np.int64(self.order), blank=np.int64(self.blank))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(z["table"], int(z["order"]), int(z["blank"]))

    # ---------------------------------------------------------------- queries
    def context(self, prefix):
        """The last order-1 symbols of ``prefix``, left-padded with blank, as a tuple."""
        n1 = self.order - 1
        tail = tuple(int(c) for c in prefix)[-n1:] if n1 else ()
        return (self.blank,) * (n1 - len(tail)) + tail

    def logp(self, context, s):
        """ln p(s | context): ``context`` is any sequence of earlier symbols, most recent last."""
        return float(self.table[self.context(context) + (int(s),)])

    def device_table(self, device):
        """The table as a contiguous fp32 tensor on ``device`` (made once per device)."""
        import torch
        return _on_device(self._device_tables, device, lambda dev: torch.from_numpy(self.table).to(dev).contiguous())


# ------------------------------------------------------------------------------------------
# Word n-gram model for second-pass rescoring (csrc/word_lm.hip; include/pgasr_hip.h, section A7-WORDLM)
# ------------------------------------------------------------------------------------------
MAX_WORD_LEN = 32          # tokens per vocabulary word: a longer word is OOV by definition
MAX_WORD_ORDER = 5
MAX_WORDS = 1 << 22        # vocabulary entries, the three reserved ones included
MAX_NGRAMS = 1 << 24       # stored n-grams of all orders
BOS, EOS, UNK = 0, 1, 2    # the reserved word ids: <s>, </s>, <unk> (no spelling)
N_RESERVED = 3
ARPA_RESERVED = ("<s>", "</s>", "<unk>")
ARPA_NEVER = -99.0         # log10 p of an entry that is never predicted (<s>), ARPA's convention
_LN10 = math.log(10.0)


def hash_word(spellings):
    """The integer hash of a word's spelling, as csrc/word_lm.hip computes it: FNV-1a over the token bytes, then murmur3's 32-bit
    finaliser, all in wrapping uint32.  ``spellings``: a sequence of byte strings; returns a uint32 array."""
    spellings = list(spellings)
    n = len(spellings)
    width = max([len(s) for s in spellings] + [1])
    mat = np.zeros((n, width), dtype=np.uint32)
    lens = np.zeros(n, dtype=np.int64)
    for i, s in enumerate(spellings):
        mat[i, :len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
        lens[i] = len(s)
    h = np.full(n, 2166136261, dtype=np.uint32)
    for j in range(width):
        live = j < lens
        h = np.where(live, (h ^ mat[:, j]) * np.uint32(16777619), h)
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    h = h ^ (h >> np.uint32(16))
    return h


def hash_ngram(ctx, word):
    """The integer hash of an n-gram's key (index of its context entry, word id), as csrc/word_lm.hip computes it: splitmix64's
    finaliser of ctx * 2^32 + word in wrapping uint64.  Arrays in, a uint64 array out."""
    x = (np.atleast_1d(np.asarray(ctx)).astype(np.uint64) << np.uint64(32)) | np.atleast_1d(np.asarray(word)).astype(np.uint64)
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    x = x ^ (x >> np.uint64(31))
    return x


def _table_size(n):
    """The smallest power of two >= max(2, 2 n): a load factor of at most 0.5."""
    cap = 2
    while cap < 2 * n:
        cap *= 2
    return cap


def _place(home, used):
    """Linear probing, deterministic and vectorised: every item starts at its home slot; per round, among the items standing on the
    same free slot the one of lowest index takes it and the others, like those standing on a taken slot, move one slot on.  An
    item therefore only ever passes taken slots, which is what a probe that stops at the first empty slot needs.  ``used`` (bool
    per slot) is updated in place; returns the slot of every item."""
    cap = used.size
    pos = np.full(home.size, -1, dtype=np.int64)
    cur = home.astype(np.int64) & (cap - 1)
    pending = np.arange(home.size)
    while pending.size:
        c = cur[pending]
        free = ~used[c]
        slots, first = np.unique(c[free], return_index=True)
        pos[pending[free][first]] = slots
        used[slots] = True
        pending = pending[pos[pending] < 0]
        cur[pending] = (cur[pending] + 1) & (cap - 1)
    return pos


# ------------------------------------------------------------------------------------------
# The back-off n-gram core: what WordNgramLM and UnitNgramLM both are, stated once
# ------------------------------------------------------------------------------------------
def _sorted_arrays(grams, ident=int):
    """grams[k-1]: dict from tuples of k symbols to (logp, bow) in natural log; ``ident`` gives a symbol's id.  Returns (ngrams, logp,
    bow) in canonical order: the k-grams of an order ascending in their ids, lexicographically; int32 and fp32."""
    ngrams, logp, bow = [], [], []
    for k, items in enumerate(grams, 1):
        g = np.array([[ident(w) for w in key] for key in items], dtype=np.int32).reshape(-1, k)
        vals = np.array(list(items.values()), dtype=np.float64).reshape(-1, 2)
        idx = np.lexsort(tuple(g[:, j] for j in range(k - 1, -1, -1))) if g.shape[0] else np.zeros(0, dtype=np.int64)
        ngrams.append(g[idx]); logp.append(vals[idx, 0].astype(np.float32)); bow.append(vals[idx, 1].astype(np.float32))
    return ngrams, logp, bow


def _witten_bell(counts, p0, unigrams, start):
    """Interpolated Witten-Bell smoothing written out in back-off form, in float64: counts[k-1][h][w] = c(hw) for the k-1 symbols h
    and k = 1 .. order -> a list over k of dicts {k-gram tuple: (ln p, ln bow)}.  With N1+(h.) the number of distinct w counted after h:
        p_0(w)   = ``p0``
        p_k(w|h) = (c(hw) + N1+(h.) p_{k-1}(w|h')) / (c(h) + N1+(h.))   for a counted hw, h' = h without its oldest symbol
        bow(h)   = ln(N1+(h.) / (c(h) + N1+(h.)))                        0.0 where h was no context, and at the top order
    p_{k-1}(w|h') being the back-off model of order k-1 itself.  Every symbol of ``unigrams`` gets a unigram (c = 0 where unseen);
    ``start`` is never predicted (log10 p = -99) and carries the bow of the context (start,)."""
    order = len(counts)
    prob = [dict() for _ in range(order)]                    # prob[k-1][h + (w,)] = p_k(w | h)
    bowp = [dict() for _ in range(order)]                    # bowp[k-1][h] = the back-off mass of the k-1 symbols h

    def lower(k, h, w):                                      # the model of order k at (w | h), len(h) == k - 1
        if k == 0:
            return p0
        p = prob[k - 1].get(h + (w,))
        if p is not None:
            return p
        return bowp[k - 1].get(h, 1.0) * lower(k - 1, h[1:], w)

    def ln_bow(k, key):
        return math.log(bowp[k].get(key, 1.0)) if k < order else 0.0

    for k in range(1, order + 1):
        for h, cw in counts[k - 1].items():
            c, n1 = float(sum(cw.values())), float(len(cw))
            bowp[k - 1][h] = n1 / (c + n1)
            for w in (list(cw) if k > 1 else unigrams):
                prob[k - 1][h + (w,)] = (cw.get(w, 0) + n1 * lower(k - 1, h[1:], w)) / (c + n1)
    grams = [{key: (math.log(p), ln_bow(k, key)) for key, p in prob[k - 1].items()} for k in range(1, order + 1)]
    grams[0][(start,)] = (ARPA_NEVER * _LN10, ln_bow(1, (start,)))
    return grams


def _read_arpa(path, max_order, key_of):
    """The sections of a standard ARPA text file as grams[k-1] = {key: (ln p, ln bow)} (log10 -> ln; 0.0 where a line gives no
    bow).  ``key_of(k, names)`` turns the k names of a line into the model's key, returns None for a line the model skips, or
    raises."""
    grams, k = [], 0
    with open(path, "r") as fo:
        for raw in fo:
            ln = raw.strip()
            if not ln or ln == "\\data\\" or ln.startswith("ngram "):
                continue
            if ln == "\\end\\":
                break
            if ln.startswith("\\") and ln.endswith("-grams:"):
                k = int(ln[1:-len("-grams:")])
                if k != len(grams) + 1 or k > max_order:
                    raise ValueError(f"{path}: the sections must be 1-grams .. n-grams in order, n <= {max_order} (got {k})")
                grams.append({})
                continue
            if k == 0:
                raise ValueError(f"{path}: {ln!r} stands before the first section")
            f = ln.split()
            if len(f) not in (k + 1, k + 2):
                raise ValueError(f"{path}: {ln!r} is no {k}-gram line")
            key = key_of(k, f[1:k + 1])
            if key is not None:
                grams[k - 1][key] = (float(f[0]) * _LN10, float(f[k + 1]) * _LN10 if len(f) == k + 2 else 0.0)
    if not grams:
        raise ValueError(f"{path}: no n-gram section")
    return grams


class _BackoffNgramLM:
    """The arrays of an ARPA-form back-off model and everything that depends on them alone.  A subclass names itself (KIND, MAX_ORDER,
    SYMBOL: the words of the error messages), runs its own checks between ``_canonical`` and ``_set_arrays`` and keeps the
    arrays under the public names it likes; here they are ``ngrams``, ``_logp`` and ``_bow``."""
    KIND = MAX_ORDER = SYMBOL = None

    @classmethod
    def _check_order(cls, order, *per_order):
        """1 <= order <= MAX_ORDER, and every list of ``per_order`` has one entry per order."""
        if not 1 <= order <= cls.MAX_ORDER or any(len(a) != order for a in per_order):
            what = " with one n-gram, logp and bow array per order" if per_order else ""
            raise ValueError(f"a {cls.KIND} LM has order 1 .. {cls.MAX_ORDER}{what} (got {order})")

    @classmethod
    def _canonical(cls, k, ngrams, logp, bow, n_symbols):
        """The arrays of order k as (M, k) int32 and (M,) fp32, equally long, every id below ``n_symbols``."""
        g = np.ascontiguousarray(np.asarray(ngrams[k - 1]), dtype=np.int32).reshape(-1, k)
        lp = np.ascontiguousarray(np.asarray(logp[k - 1]), dtype=np.float32).reshape(-1)
        bw = np.ascontiguousarray(np.asarray(bow[k - 1]), dtype=np.float32).reshape(-1)
        if lp.size != g.shape[0] or bw.size != g.shape[0]:
            raise ValueError(f"order {k}: n-grams, logp and bow differ in length")
        if g.size and (g.min() < 0 or g.max() >= n_symbols):
            raise ValueError(f"order {k}: a {cls.SYMBOL} outside the vocabulary")
        return g, lp, bw

    @staticmethod
    def _check_finite(k, lp, bw):
        if not (np.isfinite(lp).all() and np.isfinite(bw).all()):
            raise ValueError(f"order {k}: a non-finite logp or bow")

    def _set_arrays(self, per_order):
        """per_order[k-1]: the (n-grams, logp, bow) of order k, checked."""
        total = sum(g.shape[0] for g, _, _ in per_order)
        if total > MAX_NGRAMS:
            raise ValueError(f"{total} n-grams exceed the limit of 2**24; a model is never truncated")
        self.ngrams, self._logp, self._bow = (list(a) for a in zip(*per_order))
        self.order = len(per_order)
        self._table = None
        self._packed = None
        self._device_tables = {}

    def _write_arpa(self, path, names):
        """The standard ARPA text format (ln -> log10, 17 significant digits: the readers return the same arrays)."""
        with open(path, "w") as fo:
            fo.write("\\data\\\n")
            for k in range(1, self.order + 1):
                fo.write(f"ngram {k}={self.ngrams[k - 1].shape[0]}\n")
            for k in range(1, self.order + 1):
                fo.write(f"\n\\{k}-grams:\n")
                g, lp, bw = self.ngrams[k - 1], self._logp[k - 1].astype(np.float64) / _LN10, self._bow[k - 1].astype(np.float64) / _LN10
                for i in range(g.shape[0]):
                    text = " ".join(names[j] for j in g[i])
                    fo.write(f"{float(lp[i])!r}\t{text}" + (f"\t{float(bw[i])!r}\n" if k < self.order else "\n"))
            fo.write("\n\\end\\\n")

    def _save(self, path, **own):
        """The npz file: the model's ``own`` members in its own sequence ("order" among them), then ngrams_k, logp_k, bow_k for
        k = 1 .. order."""
        arrays = dict(own)
        for k in range(1, self.order + 1):
            arrays[f"ngrams_{k}"], arrays[f"logp_{k}"], arrays[f"bow_{k}"] = self.ngrams[k - 1], self._logp[k - 1], self._bow[k - 1]
        with open(path, "wb") as fo:
            np.savez(fo, **arrays)

    @staticmethod
    def _saved_arrays(z):
        ks = range(1, int(z["order"]) + 1)
        return [z[f"ngrams_{k}"] for k in ks], [z[f"logp_{k}"] for k in ks], [z[f"bow_{k}"] for k in ks]

    def _entries(self):
        """{n-gram tuple: (logp, bow)} over all orders, every fp32 widened to fp64 (made once)."""
        if self._table is None:
            tab = {}
            for g, lp, bw in zip(self.ngrams, self._logp, self._bow):
                tab.update(zip(map(tuple, g.tolist()), zip(lp.astype(np.float64).tolist(), bw.astype(np.float64).tolist())))
            self._table = tab
        return self._table

    def _backoff(self, h, w):
        """The contractual query in fp64: from 0.0, the bows of those of the contexts h, h[1:], .. that are stored, until one holds
        (.., w); then its logp is added.  A context has at most order-1 symbols, so the bow of a top-order entry is never read."""
        tab, acc = self._entries(), 0.0
        while True:
            e = tab.get(h + (w,))
            if e is not None:
                return acc + e[0]
            c = tab.get(h)
            if c is not None:
                acc = acc + c[1]
            h = h[1:]


WordLMDeviceTables = collections.namedtuple("WordLMDeviceTables", "struct tensors")


class WordNgramLM(_BackoffNgramLM):
    """A back-off word n-gram model of order 1 <= n <= 5 in ARPA form.

    A word is a non-empty tuple of at most MAX_WORD_LEN token ids of the acoustic alphabet (stored as bytes: ids <= 255), without
    the delimiter and without the blank; ids 0, 1, 2 are <s>, </s>, <unk> and have no spelling.  Every stored n-gram has ``logp``
    and, below the top order, ``bow`` (natural log, fp32).  With h the last n-1 words (<s>-padded at the sentence start, OOV words
    replaced by <unk>):
        score(w | h) = logp(h, w) if that n-gram is stored, else (bow(h) if h is stored else 0) + score(w | h without its oldest word)
    ending at the unigram, which every vocabulary entry has.  The arithmetic is contractual (the device repeats it bit for bit):
    every fp32 is widened to fp64; one word's score starts from 0 and adds the back-off weights from the longest context to the
    shortest, then the found logp; a sentence's score is the sum of its words' scores in word order, then the score of </s>.

    Arrays (canonical: words ordered by spelling, n-grams of an order by their word ids, so equal models have equal arrays):
        word_pool uint8, word_off int32 (n_words + 1): the spelling of word i is word_pool[word_off[i] : word_off[i + 1]]
        ngrams[k-1] (M_k, k) int32, logp[k-1] / bow[k-1] (M_k,) fp32 for k = 1 .. order; the unigram of word i is row i.
    The context (all words but the last) of every stored n-gram must itself be stored, as in every ARPA file a toolkit writes."""

    KIND, MAX_ORDER, SYMBOL = "word", MAX_WORD_ORDER, "word id"

    def __init__(self, word_pool, word_off, ngrams, logp, bow, blank=0, delimiter=-1):
        order = len(ngrams)
        self._check_order(order, logp, bow)
        self.word_pool = np.array(word_pool, dtype=np.uint8).reshape(-1)         # a copy: the caller's may be a read-only view of bytes
        self.word_off = np.ascontiguousarray(np.asarray(word_off), dtype=np.int32).reshape(-1)
        n_words = self.word_off.size - 1
        if n_words < N_RESERVED:
            raise ValueError("a word LM holds at least <s>, </s> and <unk>")
        if n_words > MAX_WORDS:
            raise ValueError(f"{n_words} words exceed the limit of 2**22; a model is never truncated")
        lens = np.diff(self.word_off.astype(np.int64))
        if self.word_off[0] != 0 or self.word_off[-1] != self.word_pool.size or (lens[:N_RESERVED] != 0).any() \
                or (lens[N_RESERVED:] < 1).any() or (lens > MAX_WORD_LEN).any():
            raise ValueError(f"every word but the three reserved ones has 1 .. {MAX_WORD_LEN} tokens, the reserved ones none")
        self.blank, self.delimiter = int(blank), int(delimiter)
        if (self.word_pool == self.blank).any() or (0 <= self.delimiter <= 255 and (self.word_pool == self.delimiter).any()):
            raise ValueError("a word's spelling holds neither the blank nor the delimiter")
        pool = self.word_pool.tobytes()
        self.spellings = [pool[self.word_off[i]:self.word_off[i + 1]] for i in range(n_words)]
        self._word_id = {s: i for i, s in enumerate(self.spellings) if i >= N_RESERVED}
        if len(self._word_id) != n_words - N_RESERVED:
            raise ValueError("two words of the vocabulary have the same spelling")
        per_order = []
        for k in range(1, order + 1):
            g, lp, bw = self._canonical(k, ngrams, logp, bow, n_words)
            self._check_finite(k, lp, bw)
            per_order.append((g, lp, bw))
        self._set_arrays(per_order)
        self.logp, self.bow = self._logp, self._bow
        if self.ngrams[0].shape[0] != n_words or (self.ngrams[0][:, 0] != np.arange(n_words)).any():
            raise ValueError("every vocabulary entry has a unigram, stored at its own id")
        self.n_words = n_words
        self.ctx_row = self._context_rows()

    def _context_rows(self):
        """Per order k >= 2, the row at order k-1 of every n-gram's context.  Rows are in lexicographic order, so the key
        (context row, last word) is ascending and a binary search finds it."""
        rows = [np.arange(self.n_words, dtype=np.int64)]
        keys = [np.arange(self.n_words, dtype=np.int64)]        # keys[j-1]: the ascending key of every row of order j
        for k in range(2, self.order + 1):
            g = self.ngrams[k - 1].astype(np.int64)
            p = g[:, 0]                                          # the row at order j of the n-gram's first j words, j = 1 .. k-1
            for j in range(2, k):
                p = self._search(keys[j - 1], (p << 32) | g[:, j - 1], j)
            key = (p << 32) | g[:, k - 1]
            if key.size > 1 and (np.diff(key) <= 0).any():
                raise ValueError(f"order {k}: the n-grams are not in ascending order of their word ids, or one is stored twice")
            rows.append(p)
            keys.append(key)
        return rows

    @staticmethod
    def _search(keys, want, k):
        if want.size == 0:
            return want
        if keys.size == 0:
            raise ValueError(f"an n-gram's context is not stored at order {k}")
        i = np.minimum(np.searchsorted(keys, want), keys.size - 1)
        if (keys[i] != want).any():
            raise ValueError(f"an n-gram's context is not stored at order {k}")
        return i

    # ---------------------------------------------------------------- construction
    @classmethod
    def _build(cls, grams, order, blank, delimiter):
        """grams[k-1]: dict from tuples of k words -- a reserved id (int) or a spelling (bytes) each -- to (logp, bow) in natural
        log.  Words are the spellings of the unigrams; arrays come out in canonical order."""
        words = sorted(w[0] for w in grams[0] if not isinstance(w[0], int))
        wid = {s: N_RESERVED + i for i, s in enumerate(words)}
        wid.update({BOS: BOS, EOS: EOS, UNK: UNK})
        off = np.zeros(N_RESERVED + len(words) + 1, dtype=np.int64)
        off[N_RESERVED + 1:] = np.cumsum([len(s) for s in words])
        pool = np.frombuffer(b"".join(words), dtype=np.uint8)
        if off[-1] >= 2 ** 31:
            raise ValueError("the spellings exceed 2**31 bytes")
        return cls(pool, off, *_sorted_arrays(grams[:order], wid.__getitem__), blank=blank, delimiter=delimiter)

    @classmethod
    def from_text(cls, lines, char2ind, order=3, min_count=1, delimiter=" ", blank=0):
        """Interpolated Witten-Bell smoothing (as ``CharNgramLM``), written out in back-off form, in float64 on the host
        (``_witten_bell``).  A line is <s> w_1 .. w_m </s>, its words cut at ``delimiter`` as str.split() cuts them; an n-gram of
        order k is every window of k of these whose last entry is not <s>.  p_0(w) = 1 / (words + 2): uniform over the vocabulary,
        </s> and <unk>.  Every vocabulary entry gets a unigram (c = 0 where unseen), so <unk> always has a finite probability; <s> is
        never predicted (log10 p = -99).  Words seen fewer than ``min_count`` times or longer than MAX_WORD_LEN count as <unk>.  A
        character outside the alphabet raises."""
        order = int(order)
        cls._check_order(order)
        if delimiter not in char2ind:
            raise ValueError(f"the alphabet has no delimiter {delimiter!r}")
        sents, freq = [], collections.Counter()
        for ln in lines:
            sent = []
            for w in ln.rstrip("\n").split(delimiter):
                if not w:
                    continue
                try:
                    ids = [char2ind[c] for c in w]
                except KeyError as e:
                    raise ValueError(f"character {e.args[0]!r} is not in the alphabet") from None
                if max(ids) > 255 or int(blank) in ids:
                    raise ValueError("a word LM needs token ids <= 255 other than the blank")
                sent.append(bytes(ids))
            freq.update(sent)
            sents.append(sent)
        if not sents:
            raise ValueError("from_text needs at least one line")
        vocab = {w for w, c in freq.items() if c >= int(min_count) and len(w) <= MAX_WORD_LEN}
        seqs = [[BOS] + [w if w in vocab else UNK for w in s] + [EOS] for s in sents]
        counts = []                                              # counts[k-1][h][w]
        for k in range(1, order + 1):
            ck = collections.defaultdict(collections.Counter)
            for s in seqs:
                for i in range(max(1, k - 1), len(s)):
                    ck[tuple(s[i - k + 1:i])][s[i]] += 1
            counts.append(ck)
        grams = _witten_bell(counts, 1.0 / (len(vocab) + 2), sorted(vocab) + [EOS, UNK], BOS)
        return cls._build(grams, order, int(blank), int(char2ind[delimiter]))

    @classmethod
    def from_arpa(cls, path, char2ind, skip_unknown=False, blank=0, delimiter=" "):
        """Read the standard ARPA text format (log10 -> ln).  A word is spelled through ``char2ind``; <s>, </s>, <unk> are the
        reserved entries (added with log10 p = -99 and no back-off weight where the file lacks them).  An n-gram with a word that
        cannot be spelled in the alphabet (a character outside it, more than MAX_WORD_LEN characters, or a word without a
        unigram) raises, or is dropped with ``skip_unknown=True``: the decoder can never emit such a word."""
        reserved = {name: i for i, name in enumerate(ARPA_RESERVED)}
        known = {BOS, EOS, UNK}

        def spell(w):
            if w in reserved:
                return reserved[w]
            if not 1 <= len(w) <= MAX_WORD_LEN:
                return None
            ids = [char2ind.get(c, -1) for c in w]
            if min(ids) < 0 or max(ids) > 255 or int(blank) in ids:
                return None
            return bytes(ids)

        def key_of(k, names):
            key = tuple(spell(w) for w in names)
            if any(w is None for w in key) or (k > 1 and any(w not in known for w in key)):
                if skip_unknown:
                    return None
                raise ValueError(f"{path}: {' '.join(names)!r} holds a word that cannot be spelled in the alphabet")
            if k == 1:
                known.add(key[0])
            return key

        grams = _read_arpa(path, MAX_WORD_ORDER, key_of)
        for r in (BOS, EOS, UNK):
            grams[0].setdefault((r,), (ARPA_NEVER * _LN10, 0.0))
        return cls._build(grams, len(grams), int(blank), int(char2ind.get(delimiter, -1)))

    def to_arpa(self, path, ind2char):
        """Write the standard ARPA text format (ln -> log10, 17 significant digits: ``from_arpa`` returns the same arrays)."""
        self._write_arpa(path, list(ARPA_RESERVED) + ["".join(ind2char[int(t)] for t in s) for s in self.spellings[N_RESERVED:]])

    # ---------------------------------------------------------------- persistence
    def save(self, path):
        self._save(path, word_pool=self.word_pool, word_off=self.word_off, order=np.int64(self.order), blank=np.int64(self.blank),
                   delimiter=np.int64(self.delimiter))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(z["word_pool"], z["word_off"], *cls._saved_arrays(z), blank=int(z["blank"]), delimiter=int(z["delimiter"]))

    # ---------------------------------------------------------------- queries (the host's own statement)
    def word_id(self, tokens):
        """The id of the word spelled by ``tokens``, or UNK: a word longer than MAX_WORD_LEN, or with a token outside the byte
        range, is in no vocabulary."""
        tokens = [int(t) for t in tokens]
        if not 1 <= len(tokens) <= MAX_WORD_LEN or min(tokens) < 0 or max(tokens) > 255:
            return UNK
        return self._word_id.get(bytes(tokens), UNK)

    def score(self, context, w):
        """ln p(w | context) by the back-off rule: ``context`` any sequence of earlier word ids, most recent last."""
        h = tuple(int(c) for c in context)[-(self.order - 1):] if self.order > 1 else ()
        return self._backoff((BOS,) * (self.order - 1 - len(h)) + h, int(w))

    def split(self, token_ids, delimiter=None):
        """The words of a sentence: the maximal runs of non-delimiter tokens, as str.split() cuts them."""
        d = self.delimiter if delimiter is None else int(delimiter)
        words, cur = [], []
        for t in token_ids:
            if int(t) == d:
                if cur:
                    words.append(tuple(cur))
                cur = []
            else:
                cur.append(int(t))
        if cur:
            words.append(tuple(cur))
        return words

    def logp_sentence(self, token_ids, delimiter=None):
        """(word_logp, n_words, n_oov) of a sentence of token ids: the fp64 sum of its words' scores in word order, then the score
        of </s>; n_words does not count </s>; an empty sentence scores score(</s> | <s>)."""
        ids = [self.word_id(w) for w in self.split(token_ids, delimiter)]
        hist, total = [BOS] * (self.order - 1), 0.0
        for w in ids + [EOS]:
            total = total + self.score(hist, w)
            hist.append(w)
        return total, len(ids), sum(1 for w in ids if w == UNK)

    # ---------------------------------------------------------------- the device's tables
    def pack(self):
        """The tables csrc/word_lm.hip reads, as numpy arrays (deterministic; both hash tables are open-addressed with linear
        probing and at most half full):
            word_slots (word_cap) int32: a word id or -1; a word is found from hash_word(spelling) & (word_cap - 1) on, and
                confirmed on its spelling in word_pool / word_off.
            uni_logp, uni_bow (n_words) fp32: the unigrams, at the word's id.  Entry index of a unigram: the word id.
            ngram_slots (ngram_cap, 4) int32: (index of the context entry, word id, logp bits, bow bits), or ctx = -1 for an empty
                slot; the n-grams of all orders >= 2 share the table.  Entry index of the n-gram in slot s: n_words + s.  An
                n-gram is found from hash_ngram(ctx, word) & (ngram_cap - 1) on, and confirmed on the pair (ctx, word)."""
        if self._packed is not None:
            return self._packed
        n_real = self.n_words - N_RESERVED
        word_cap = _table_size(n_real)
        word_slots = np.full(word_cap, -1, dtype=np.int32)
        if n_real:
            pos = _place(hash_word(self.spellings[N_RESERVED:]).astype(np.int64), np.zeros(word_cap, dtype=bool))
            word_slots[pos] = np.arange(N_RESERVED, self.n_words, dtype=np.int32)
        n_high = sum(g.shape[0] for g in self.ngrams[1:])
        ngram_cap = _table_size(n_high)
        slots = np.zeros((ngram_cap, 4), dtype=np.int32)
        slots[:, 0] = -1
        used = np.zeros(ngram_cap, dtype=bool)
        entry = np.arange(self.n_words, dtype=np.int64)         # entry index of every row of the order below
        for k in range(2, self.order + 1):
            g = self.ngrams[k - 1]
            ctx = entry[self.ctx_row[k - 1]] if g.shape[0] else np.zeros(0, dtype=np.int64)
            pos = _place((hash_ngram(ctx, g[:, k - 1]) & np.uint64(ngram_cap - 1)).astype(np.int64), used)
            slots[pos, 0] = ctx
            slots[pos, 1] = g[:, k - 1]
            slots[pos, 2] = self.logp[k - 1].view(np.int32)
            slots[pos, 3] = self.bow[k - 1].view(np.int32)
            entry = self.n_words + pos
        self._packed = {"word_pool": self.word_pool if self.word_pool.size else np.zeros(1, dtype=np.uint8),
                        "word_off": self.word_off, "word_slots": word_slots,
                        "uni_logp": self.logp[0], "uni_bow": self.bow[0], "ngram_slots": slots}
        return self._packed

    def device_tables(self, device):
        """The packed tables as tensors on ``device`` and the POD struct of their addresses that pgasr_nbest_word_lm_score takes
        (made once per device; the tensors live as long as the model)."""
        import torch
        from . import _lib

        def make(device):
            p = self.pack()
            tensors = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device).contiguous() for k, v in p.items()}
            st = _lib.WordLMTables(tensors["word_pool"].data_ptr(), tensors["word_off"].data_ptr(), tensors["word_slots"].data_ptr(),
                                   tensors["uni_logp"].data_ptr(), tensors["uni_bow"].data_ptr(), tensors["ngram_slots"].data_ptr(),
                                   self.order, self.n_words, p["word_slots"].size, p["ngram_slots"].shape[0], self.word_pool.size)
            return WordLMDeviceTables(st, tensors)
        return _on_device(self._device_tables, device, make)


# ------------------------------------------------------------------------------------------
# Back-off n-gram model over the acoustic units themselves (csrc/beam_wide.hip with a model, csrc/unit_lm.hip; include/pgasr_hip.h,
# section A7-WIDE-LM)
# ------------------------------------------------------------------------------------------
MAX_UNIT_VOCAB = 1024
MAX_UNIT_ORDER = 5
UnitLMDeviceTables = collections.namedtuple("UnitLMDeviceTables", "struct tensors")


def _gram_keys(g, V):
    """Rows of symbols -> their base-V number: ascending keys are lexicographic order (V**5 <= 2**50)."""
    key = np.zeros(g.shape[0], dtype=np.int64)
    for j in range(g.shape[1]):
        key = key * V + g[:, j].astype(np.int64)
    return key


def _find_keys(keys, want):
    """Index of every ``want`` in the ascending ``keys``, -1 where absent."""
    if keys.size == 0 or want.size == 0:
        return np.full(want.shape, -1, dtype=np.int64)
    i = np.minimum(np.searchsorted(keys, want), keys.size - 1)
    return np.where(keys[i] == want, i, -1)


class UnitNgramLM(_BackoffNgramLM):
    """A back-off n-gram model of order 1 <= n <= 5 over the V <= 1024 ids of the acoustic alphabet (subword units or characters),
    natural logs, fp32.  Unlike ``CharNgramLM`` it is sparse, so V = 1024 at order 5 is a model like any other.

    The blank never occurs inside a prefix: it is the start-of-sentence symbol, exactly one of it (ARPA's <s>).  The context of a
    prefix y is the last n-1 symbols of (blank,) + y -- shorter than n-1 near the start.  Stored k-grams are (c_1 .. c_{k-1}, s)
    with s != blank; blank may stand only as c_1.  Every k-gram has ``logp`` and, below the top order, ``bow`` (0 where a file gives
    none).  The unigram array has V rows, row = symbol: the row of the blank is <s> itself, whose logp is never read and whose bow
    is the back-off weight of the context (blank,).  The context of every stored n-gram is itself stored.

    The query is contractual (every device path returns its bits): acc = 0.0 in fp64, h = the context; if (h, s) is stored return
    float32(acc + (double)logp[h, s]); else add (double)bow[h] where h is stored, drop the oldest symbol of h, and again.  The
    sums run from the longest context to the shortest with ONE rounding to fp32, at the end.  ``logp_sequence`` is the fp64 sum in
    index order of those fp32 values; there is no end-of-sentence term.

    Arrays (canonical: the k-grams of an order in lexicographic order, so equal models have equal arrays):
        ngrams[k-1] (M_k, k) int32, lp[k-1] / bw[k-1] (M_k,) fp32 (logp and bow) for k = 1 .. order; M_1 = V."""

    KIND, MAX_ORDER, SYMBOL = "unit", MAX_UNIT_ORDER, "symbol"

    def __init__(self, ngrams, logp, bow, vocab, blank=0):
        order = len(ngrams)
        self._check_order(order, logp, bow)
        V, blank = self._check_symbols(vocab, blank)
        per_order, self._keys = [], []
        for k in range(1, order + 1):
            g, lp, bw = self._canonical(k, ngrams, logp, bow, V)
            if k == 1:
                if g.shape[0] != V or (g[:, 0] != np.arange(V)).any():
                    raise ValueError("every symbol has a unigram, stored at its own id (the row of the blank is <s>): "
                                     "a unigram is missing")
                self._check_finite(k, lp[np.arange(V) != blank], bw)       # the logp of <s> is never read
            else:
                if (g[:, 1:] == blank).any():
                    raise ValueError(f"order {k}: the blank stands inside a context or is predicted; it may only be an n-gram's first symbol")
                self._check_finite(k, lp, bw)
            key = _gram_keys(g, V)
            if key.size > 1 and (np.diff(key) <= 0).any():
                raise ValueError(f"order {k}: the n-grams are not in lexicographic order, or one is stored twice")
            if k > 1 and (_find_keys(self._keys[k - 2], key // V) < 0).any():
                raise ValueError(f"order {k}: an n-gram's context is not stored at order {k - 1}")
            per_order.append((g, lp, bw)); self._keys.append(key)
        self._set_arrays(per_order)
        self.lp, self.bw = self._logp, self._bow
        self.vocab, self.blank = V, blank

    @staticmethod
    def _check_symbols(vocab, blank):
        V, blank = int(vocab), int(blank)
        if not 2 <= V <= MAX_UNIT_VOCAB:
            raise ValueError(f"a unit LM is over 2 .. {MAX_UNIT_VOCAB} symbols, the blank included (got {V})")
        if not 0 <= blank < V:
            raise ValueError("blank must be a symbol of the vocabulary")
        return V, blank

    @property
    def n_ngrams(self):
        """Stored n-grams of all orders, <s> not counted."""
        return sum(g.shape[0] for g in self.ngrams) - 1

    # ---------------------------------------------------------------- construction
    @classmethod
    def _build(cls, grams, vocab, blank):
        """grams[k-1]: dict from tuples of k symbols to (logp, bow) in natural log; arrays come out in canonical order."""
        return cls(*_sorted_arrays(grams), vocab, blank=blank)

    @staticmethod
    def estimate(seqs_of_token_ids, vocab, order=3, blank=0, min_count=1):
        """The fp64 estimate behind ``from_transcripts``: a list over k = 1 .. order of dicts {k-gram tuple: (ln p, ln bow)}.
        ``_witten_bell``: the estimator of ``WordNgramLM.from_text`` and, context by context, of ``CharNgramLM.from_transcripts``.
        A transcript y is counted as (blank,) + y; a k-gram is every window of k of these whose last entry is not the blank.
        p_0(s) = 1 / (V - 1), and every one of the V-1 symbols gets a unigram (c = 0 where unseen; the uniform one where no token
        was seen at all).  A k-gram with k >= 2 seen fewer than ``min_count`` times is not stored and takes no part in c and N1+:
        the model stays normalised."""
        V, blank, order = int(vocab), int(blank), int(order)
        UnitNgramLM._check_order(order)
        UnitNgramLM._check_symbols(V, blank)
        counts = [collections.defaultdict(collections.Counter) for _ in range(order)]      # counts[k-1][h][s]
        for y in seqs_of_token_ids:
            s = [blank] + [int(t) for t in y]
            if any(t < 0 or t >= V or t == blank for t in s[1:]):
                raise ValueError("transcripts must hold symbols of the vocabulary other than the blank")
            for i in range(1, len(s)):
                for k in range(1, min(order, i + 1) + 1):
                    counts[k - 1][tuple(s[i - k + 1:i])][s[i]] += 1
        for k in range(2, order + 1):
            for h in list(counts[k - 1]):
                kept = collections.Counter({w: c for w, c in counts[k - 1][h].items() if c >= int(min_count)})
                if kept:
                    counts[k - 1][h] = kept
                else:
                    del counts[k - 1][h]
        p0 = 1.0 / (V - 1)
        symbols = [s for s in range(V) if s != blank]
        if not counts[0]:                                            # no token at all: the uniform unigram, nothing above it
            uniform = {(w,): (math.log(p0), 0.0) for w in symbols}
            uniform[(blank,)] = (ARPA_NEVER * _LN10, 0.0)
            return [uniform] + [{} for _ in range(order - 1)]
        return _witten_bell(counts, p0, symbols, blank)

    @classmethod
    def from_transcripts(cls, seqs_of_token_ids, vocab, order=3, blank=0, min_count=1):
        """Sequences of token ids -> the model of ``estimate``, rounded to fp32."""
        return cls._build(cls.estimate(seqs_of_token_ids, vocab, order=order, blank=blank, min_count=min_count), vocab, blank)

    @classmethod
    def from_text(cls, lines, units, order=3, blank=0, min_count=1):
        """Lines of text -> token ids through ``units.encode`` (a ``SubwordUnits``: V = len(units), the blank is id 0)."""
        return cls.from_transcripts([units.encode(ln.rstrip("\n")) for ln in lines], len(units), order=order, blank=blank,
                                    min_count=min_count)

    @classmethod
    def from_arpa(cls, path, vocab, blank=0, names=None):
        """Read the standard ARPA text format (log10 -> ln).  ``names``: the V symbols' spellings in the file (default: their
        decimal ids; the entry of the blank is ignored); <s> is the blank.  Entries with </s> or <unk> are skipped: the model has
        no end-of-sentence term and no unknown unit.  Any other name outside ``names`` raises."""
        V, blank = int(vocab), int(blank)
        names = [str(i) for i in range(V)] if names is None else [str(x) for x in names]
        if len(names) != V:
            raise ValueError(f"names must list the {V} symbols")
        ids = {nm: i for i, nm in enumerate(names) if i != blank}
        ids["<s>"] = blank

        def key_of(k, words):
            if any(w in ("</s>", "<unk>") for w in words):
                return None
            try:
                return tuple(ids[w] for w in words)
            except KeyError as e:
                raise ValueError(f"{path}: {e.args[0]!r} is no symbol of the alphabet") from None

        grams = _read_arpa(path, MAX_UNIT_ORDER, key_of)
        grams[0].setdefault((blank,), (ARPA_NEVER * _LN10, 0.0))
        return cls._build(grams, V, blank)

    def to_arpa(self, path, names=None):
        """Write the standard ARPA text format (ln -> log10, 17 significant digits: ``from_arpa`` returns the same arrays)."""
        names = [str(i) for i in range(self.vocab)] if names is None else [str(x) for x in names]
        self._write_arpa(path, [("<s>" if i == self.blank else nm) for i, nm in enumerate(names)])

    # ---------------------------------------------------------------- persistence
    def save(self, path):
        self._save(path, order=np.int64(self.order), vocab=np.int64(self.vocab), blank=np.int64(self.blank))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(*cls._saved_arrays(z), int(z["vocab"]), blank=int(z["blank"]))

    # ---------------------------------------------------------------- queries (the host's own statement)
    def context(self, prefix):
        """The last order-1 symbols of (blank,) + prefix.  A prefix that holds the blank counts from its last blank on."""
        y = [int(c) for c in prefix]
        if self.blank in y:
            y = y[len(y) - y[::-1].index(self.blank):]
        h = [self.blank] + y
        return tuple(h[max(0, len(h) - (self.order - 1)):]) if self.order > 1 else ()

    def logp(self, context, s):
        """ln p(s | context) by the contractual query, as a Python float holding an fp32 value.  ``context``: any sequence of
        earlier symbols, most recent last (``context`` cuts it)."""
        s = int(s)
        if not 0 <= s < self.vocab or s == self.blank:
            raise ValueError(f"symbol {s} is the blank or outside [0, {self.vocab})")
        return float(np.float32(self._backoff(self.context(context), s)))

    def logp_sequence(self, tokens):
        """The fp64 sum, in index order, of logp(tokens[:i], tokens[i]); 0.0 for no tokens."""
        y, total = [int(t) for t in tokens], 0.0
        for i, s in enumerate(y):
            total = total + self.logp(y[max(0, i - self.order):i], s)
        return total

    # ---------------------------------------------------------------- the dense form
    def to_dense(self):
        """The equivalent ``CharNgramLM`` where V**order <= 2**25: table[ctx + (s,)] = logp(ctx from its last blank on, s), the
        blank column 0 -- bit for bit what the query returns, so the dense kernels and their oracles apply."""
        V, n = self.vocab, self.order
        _check_size(V, n)
        C = V ** (n - 1)
        ctx = np.zeros((C, n - 1), dtype=np.int64)
        rem = np.arange(C, dtype=np.int64)
        for j in range(n - 2, -1, -1):
            ctx[:, j] = rem % V
            rem //= V
        # eff[c]: symbols the query's context keeps -- from the last blank on, or all n-1 plus nothing (no blank: the oldest are cut)
        isb = ctx == self.blank
        lastb = np.where(isb.any(axis=1), (n - 2) - np.argmax(isb[:, ::-1], axis=1), -1) if n > 1 else np.full(C, -1)
        eff = np.where(lastb >= 0, (n - 1) - lastb, n - 1)
        table = np.zeros((C, V), dtype=np.float32)
        done = np.zeros((C, V), dtype=bool)
        acc = np.zeros(C, dtype=np.float64)
        for k in range(n, 0, -1):                                 # k-grams: the context is the last k-1 symbols
            if k == 1:
                rows = np.zeros(C, dtype=np.int64)
                live = np.ones(C, dtype=bool)
            else:
                live = eff >= k - 1
                rows = _find_keys(self._keys[k - 2], _gram_keys(ctx[:, n - k:], V))
                live &= rows >= 0
            who = np.nonzero(live)[0]
            if who.size == 0:
                continue
            if k == 1:
                lo, hi = np.zeros(who.size, dtype=np.int64), np.full(who.size, V, dtype=np.int64)
            else:
                pk = self._keys[k - 1] // V
                want = self._keys[k - 2][rows[who]]
                lo, hi = np.searchsorted(pk, want, side="left"), np.searchsorted(pk, want, side="right")
            cnt = hi - lo
            c_of = np.repeat(who, cnt)
            i_of = np.repeat(lo - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(int(cnt.sum()))
            sym = self.ngrams[k - 1][i_of, k - 1].astype(np.int64)
            val = (acc[c_of] + self.lp[k - 1][i_of].astype(np.float64)).astype(np.float32)
            new = ~done[c_of, sym] & (sym != self.blank)
            table[c_of[new], sym[new]] = val[new]
            done[c_of[new], sym[new]] = True
            if k > 1:
                acc[who] = acc[who] + self.bw[k - 2][rows[who]].astype(np.float64)
        table[:, self.blank] = 0.0
        return CharNgramLM(table.reshape((V,) * n), n, self.blank)

    # ---------------------------------------------------------------- the device's tables
    def pack(self):
        """The tables the kernels read, as numpy arrays (deterministic).  A STATE is a context the model stores: state 0 the empty
        context, then every stored k-gram with k < order in canonical order (the unigram of symbol c is state 1 + c, <s> = the blank
        included).  A SUCCESSOR is a stored n-gram, listed behind its context: the V-1 unigrams (blank left out) are the successors of
        state 0, then the 2-grams, .., in canonical order, so one state's successors are consecutive and ascending in their symbol.
            states (S, 4) int32: (bow bits, back-off state, first successor, one past the last).  The back-off state is the longest
                proper suffix of the context that is a state (0 at the latest).
            succ (M, 4) int32: (symbol, logp bits, next state, 0).  The next state is the longest suffix of context + symbol, of at
                most order-1 symbols, that is a state: the n-gram itself below the top order.
            start: the state of the empty prefix, (blank,) from order 2 on."""
        if self._packed is not None:
            return self._packed
        V, n, blank = self.vocab, self.order, self.blank
        sizes = [g.shape[0] for g in self.ngrams]
        st_off = np.concatenate([[1], 1 + np.cumsum(sizes[:n - 1])]).astype(np.int64)       # st_off[k-1]: first state of the k-grams
        S = int(st_off[-1]) if n > 1 else 1
        su_off = np.concatenate([[0], np.cumsum([V - 1] + sizes[1:])]).astype(np.int64)     # su_off[k-1]: first successor of order k
        M = int(su_off[-1])
        states = np.zeros((S, 4), dtype=np.int32)
        succ = np.zeros((M, 4), dtype=np.int32)

        def longest_suffix(g, k, top):
            """State of the longest suffix of the k-grams g with at most ``top`` symbols (0: none but the empty one)."""
            out = np.zeros(g.shape[0], dtype=np.int64)
            for j in range(1, min(top, k, n - 1) + 1):             # ascending: the longer suffix overwrites
                r = _find_keys(self._keys[j - 1], _gram_keys(g[:, k - j:], V))
                out = np.where(r >= 0, st_off[j - 1] + r, out)
            return out

        real = np.arange(V) != blank
        states[0] = (0, 0, 0, V - 1)
        succ[:V - 1, 0] = np.arange(V)[real]
        succ[:V - 1, 1] = self.lp[0][real].view(np.int32)
        succ[:V - 1, 2] = (1 + np.arange(V)[real]) if n > 1 else 0
        for k in range(1, n + 1):
            g = self.ngrams[k - 1].astype(np.int64)
            if k < n:                                              # the k-grams as states
                sl = slice(int(st_off[k - 1]), int(st_off[k - 1]) + sizes[k - 1])
                states[sl, 0] = self.bw[k - 1].view(np.int32)
                states[sl, 1] = longest_suffix(g, k, k - 1)
                pk = self._keys[k] // V
                states[sl, 2] = su_off[k] + np.searchsorted(pk, self._keys[k - 1], side="left")
                states[sl, 3] = su_off[k] + np.searchsorted(pk, self._keys[k - 1], side="right")
            if k >= 2:                                             # the k-grams as successors
                sl = slice(int(su_off[k - 1]), int(su_off[k - 1]) + sizes[k - 1])
                succ[sl, 0] = g[:, k - 1]
                succ[sl, 1] = self.lp[k - 1].view(np.int32)
                succ[sl, 2] = (st_off[k - 1] + np.arange(sizes[k - 1])) if k < n else longest_suffix(g, k, k - 1)
        self._packed = {"states": states, "succ": succ, "start": int(1 + blank) if n > 1 else 0}
        return self._packed

    def device_tables(self, device):
        """The packed tables as tensors on ``device`` and the POD struct of their addresses that the kernels take (made once per
        device; the tensors live as long as the model)."""
        import torch
        from . import _lib

        def make(device):
            p = self.pack()
            tensors = {k: torch.from_numpy(p[k]).to(device).contiguous() for k in ("states", "succ")}
            st = _lib.UnitLMTables(tensors["states"].data_ptr(), tensors["succ"].data_ptr(), self.order, self.vocab, self.blank,
                                   p["states"].shape[0], p["succ"].shape[0], p["start"])
            return UnitLMDeviceTables(st, tensors)
        return _on_device(self._device_tables, device, make)


# ------------------------------------------------------------------------------------------
# Hotword (contextual phrase) biasing (csrc/beam.hip BIAS = true, csrc/hotword.hip; include/pgasr_hip.h, section A7-BIAS)
# ------------------------------------------------------------------------------------------
MAX_BIAS_WORDS = 1 << 24   # S * V table words of 8 bytes (128 MiB): the entry points refuse more


class HotwordBias:
    """A list of phrases to bias the CTC beam search towards, compiled to a weighted automaton.

    ``phrases`` is a list of token-id sequences (no blank, ids in [0, vocab), no empty phrase; duplicates are merged, the first
    one's weight kept).  The weight of phrase p is ``weights[p]`` if given, else ``boost * len(p)``.  The bias of a token row y is

        B(y) = sum over phrases p of (occurrences of p in y, overlapping ones included) * w(p)
               + partial * boost * (length of the longest suffix of y that is a PROPER prefix of some phrase).

    The second term is pending credit: it rewards a hypothesis for being on the way into a phrase and is taken back by the
    transition that leaves the phrase.  The automaton is the Aho-Corasick machine of the phrase trie: state 0 is the root, states are
    numbered in breadth-first order with children in symbol order; ``next`` (S, V) int32 is the dense goto with the failure links
    resolved, ``bonus`` (S, V) float32 the increment of B on that transition, out(next) + pend(next) - pend(q) with out the summed
    weights over the dictionary links, formed in float64 and rounded once.  The blank's column is next = q, bonus = 0.
    ``transition`` / ``score_sequence`` are the host statements of the query the device makes; ``device_table`` is what the kernels
    read: S * V 8-byte little-endian words {int32 next; float32 bonus}, at most 2**24 of them (ValueError beyond, never truncated)."""

    def __init__(self, phrases, vocab, blank=0, boost=1.0, weights=None, partial=1.0):
        V, blank = int(vocab), int(blank)
        if V < 2:
            raise ValueError("a bias needs at least one symbol beside the blank")
        if not 0 <= blank < V:
            raise ValueError("blank must be a symbol of the vocabulary")
        boost, partial = float(boost), float(partial)
        if not (math.isfinite(boost) and math.isfinite(partial)):
            raise ValueError("boost and partial must be finite")
        rows = [tuple(int(t) for t in p) for p in phrases]
        if weights is not None:
            weights = [float(w) for w in weights]
            if len(weights) != len(rows):
                raise ValueError("weights: one per phrase")
            if not all(math.isfinite(w) for w in weights):
                raise ValueError("weights must be finite")
        merged = {}
        for i, p in enumerate(rows):
            if not p:
                raise ValueError("an empty phrase cannot be a hotword")
            if any(t < 0 or t >= V or t == blank for t in p):
                raise ValueError(f"phrase {i} holds the blank or a symbol outside [0, {V})")
            merged.setdefault(p, weights[i] if weights is not None else boost * len(p))
        self.phrases = list(merged)
        self.weights = np.asarray([merged[p] for p in self.phrases], dtype=np.float64).reshape(-1)
        self.vocab, self.blank, self.boost, self.partial = V, blank, boost, partial
        self._build()
        self._device_tables = {}

    def _build(self):
        V, blank = self.vocab, self.blank
        # the trie, in insertion order ...
        kids, own = [{}], [0.0]
        for p, w in zip(self.phrases, self.weights):
            q = 0
            for t in p:
                nx = kids[q].get(t)
                if nx is None:
                    nx = len(kids)
                    kids[q][t] = nx
                    kids.append({})
                    own.append(0.0)
                q = nx
            own[q] += float(w)
        S = len(kids)
        if S * V > MAX_BIAS_WORDS:
            raise ValueError(f"the bias automaton has {S} states over {V} symbols: {S * V} table words, the limit is 2**24")
        # ... renumbered breadth first, children in symbol order
        order, new_of = [0], {0: 0}
        parent, sym, depth = [0], [-1], [0]
        head = 0
        while head < len(order):
            old = order[head]
            for t in sorted(kids[old]):
                c = kids[old][t]
                new_of[c] = len(order)
                order.append(c)
                parent.append(head); sym.append(t); depth.append(depth[head] + 1)
            head += 1
        nxt = np.zeros((S, V), dtype=np.int32)
        out = np.zeros(S, dtype=np.float64)
        plen = np.zeros(S, dtype=np.int64)        # length of the longest suffix that is a proper prefix of some phrase
        fail = np.zeros(S, dtype=np.int64)
        has_kids = np.array([bool(kids[o]) for o in order])
        for q in range(S):                        # breadth-first order: a state's failure state comes before it
            if q:
                f = int(nxt[fail[parent[q]], sym[q]]) if parent[q] else 0
                fail[q] = f
                nxt[q] = nxt[f]
                out[q] = own[order[q]] + out[f]
                plen[q] = depth[q] if has_kids[q] else plen[f]
            for t, c in kids[order[q]].items():
                nxt[q, t] = new_of[c]
        pend = (self.partial * self.boost) * plen.astype(np.float64)
        bonus64 = out[nxt] + pend[nxt] - pend[:, None]
        nxt[:, blank] = np.arange(S, dtype=np.int32)
        bonus64[:, blank] = 0.0
        bonus = bonus64.astype(np.float32)
        assert nxt.min() >= 0 and nxt.max() < S, "a transition leaves the automaton"
        assert np.isfinite(bonus).all(), "a bonus is not finite"
        self.next, self.bonus, self.n_states = np.ascontiguousarray(nxt), np.ascontiguousarray(bonus), S
        self.depth = np.asarray(depth, dtype=np.int64)

    # ---------------------------------------------------------------- construction
    @classmethod
    def from_strings(cls, lines, alphabet, blank=0, boost=1.0, weights=None, partial=1.0):
        """One phrase per line, encoded character by character.  ``alphabet``: the list of symbols in index order (the decoder's;
        entries may carry their line break) or a ``char2ind`` dict.  Empty lines are skipped (then give no ``weights``); a
        character outside the alphabet raises."""
        if hasattr(alphabet, "items"):
            char2ind = dict(alphabet)
            vocab = max(char2ind.values()) + 1
        else:
            char2ind = {str(a).replace("\n", ""): i for i, a in enumerate(alphabet)}
            vocab = len(alphabet)
        phrases = []
        for ln in lines:
            ln = ln.rstrip("\n").rstrip("\r")
            if not ln:
                if weights is not None:
                    raise ValueError("an empty line cannot carry a weight")
                continue
            try:
                phrases.append([char2ind[c] for c in ln])
            except KeyError as e:
                raise ValueError(f"character {e.args[0]!r} of hotword {ln!r} is not in the alphabet") from None
        return cls(phrases, vocab, blank=blank, boost=boost, weights=weights, partial=partial)

    @classmethod
    def from_units(cls, lines, units, blank=0, boost=1.0, weights=None, partial=1.0):
        """One phrase per line, encoded with ``units.encode`` (``units.SubwordUnits``, greedy longest match).  A phrase is
        segmented IN ISOLATION: inside a sentence the same characters can be cut into other units (a unit may span the phrase's
        boundary), and such an occurrence is not matched.  Empty lines are skipped (then give no ``weights``)."""
        phrases = []
        for ln in lines:
            ln = ln.rstrip("\n").rstrip("\r")
            if not ln:
                if weights is not None:
                    raise ValueError("an empty line cannot carry a weight")
                continue
            phrases.append(units.encode(ln))
        return cls(phrases, len(units), blank=blank, boost=boost, weights=weights, partial=partial)

    # ---------------------------------------------------------------- persistence
    def save(self, path):
        """The phrases and their weights (.npz); ``load`` compiles them again, to the same bits."""
        flat = np.asarray([t for p in self.phrases for t in p], dtype=np.int32)
        off = np.cumsum([0] + [len(p) for p in self.phrases]).astype(np.int64)
        with open(path, "wb") as fo:
            np.savez(fo, tokens=flat, offsets=off, weights=self.weights, vocab=np.int64(self.vocab), blank=np.int64(self.blank),
                     boost=np.float64(self.boost), partial=np.float64(self.partial))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            flat, off = z["tokens"], z["offsets"]
            phrases = [flat[int(off[i]):int(off[i + 1])].tolist() for i in range(len(off) - 1)]
            return cls(phrases, int(z["vocab"]), blank=int(z["blank"]), boost=float(z["boost"]), weights=z["weights"].tolist(),
                       partial=float(z["partial"]))

    # ---------------------------------------------------------------- queries
    def transition(self, q, s):
        """(next state, bonus as a Python float) of token ``s`` in state ``q``; a token outside [0, vocab) or equal to the blank
        leaves the state unchanged and adds nothing."""
        q, s = int(q), int(s)
        if s < 0 or s >= self.vocab or s == self.blank:
            return q, 0.0
        return int(self.next[q, s]), float(self.bonus[q, s])

    def score_sequence(self, tokens):
        """The Python-float sum of float(bonus) along ``tokens`` from state 0, in token order: B(tokens) up to the table's fp32."""
        q, total = 0, 0.0
        for s in tokens:
            q, w = self.transition(q, s)
            total = total + w
        return total

    def device_table(self, device):
        """The table as an (S * V, 2) int32 tensor on ``device`` -- word (q, s) = {next, the bonus' bits} -- made once per device."""
        import torch

        def make(dev):
            words = np.empty((self.n_states * self.vocab, 2), dtype="<i4")
            words[:, 0] = self.next.reshape(-1)
            words[:, 1] = self.bonus.reshape(-1).view(np.int32)
            return torch.from_numpy(words).to(dev).contiguous()
        return _on_device(self._device_tables, device, make)


# ------------------------------------------------------------------------------------------
# The word model and its lexicon inside the first pass (csrc/beam.hip WORDS = true; include/pgasr_hip.h, section A7-WORDFUSE)
# ------------------------------------------------------------------------------------------
MAX_FUSION_VOCAB = 64      # the workgroup-per-utterance search: one symbol per lane
WordFusionDeviceTables = collections.namedtuple("WordFusionDeviceTables", "trie node_word word_lm")


class WordFusion:
    """A ``WordNgramLM`` and its vocabulary as a lexicon, in the form the fused CTC prefix beam search reads
    (``hipops.ctc_beam_search_words``), and the host's own statement of every term that search adds.

    ``delimiter`` d is the token that ends a word, ``blank`` the CTC blank.  The lexicon is the vocabulary of ``word_lm`` (ids 3 and
    up) as a trie over the spellings: state 0 is the root, the nodes follow in breadth-first order with children in symbol order, and
    the LAST state is the one sink for everything outside the lexicon.  For a prefix y, u(y) is the pending word (the tokens behind the
    last d) and hist(y) the ids of the completed words, cut as ``WordNgramLM.split`` cuts them, a word outside the lexicon being <unk>.
    ``bonus(y, s)`` is what an extension of y by the non-blank s adds:
        s != d: 0.0 into a child node; ``oov_penalty`` from a trie node into the sink; 0.0 inside the sink
        s == d: 0.0 behind an empty u; else alpha * score(hist, word) + beta with word = the id at a terminal node and <unk>
                elsewhere, plus ``oov_penalty`` (one more addition) at a node that is neither terminal nor the sink -- the sink was
                charged on the way in.
    ``final(y)`` is the d-bonus of a pending word (0.0 without one) and, with ``eos``, alpha * score(hist', </s>) added to it.  The
    bonuses along y plus final(y, eos=True) are alpha * word_logp + beta * n_words + oov_penalty * n_oov of
    ``word_lm.logp_sentence(y)``.  ``oov_penalty`` is an fp32 value <= 0; -inf is the hard lexicon constraint.

    Arrays: ``next`` (S, V) int32 and ``trie_bonus`` (S, V) float32 -- the blank's column is next = q, the delimiter's next = 0 with
    ``oov_penalty`` in the bonus where a delimiter behind state q is charged it -- and ``node_word`` (S,) int32: the word id at a
    terminal node, <unk> elsewhere, -1 at the root."""

    def __init__(self, word_lm, vocab, delimiter, blank=0, oov_penalty=0.0):
        if not isinstance(word_lm, WordNgramLM):
            raise ValueError("word_lm: a lm.WordNgramLM is wanted")
        V, d, blank = int(vocab), int(delimiter), int(blank)
        if not 2 <= V <= MAX_FUSION_VOCAB:
            raise ValueError(f"vocab: the fused search takes 2 .. {MAX_FUSION_VOCAB} symbols (got {V})")
        if not 0 <= blank < V:
            raise ValueError(f"blank: {blank} is no symbol of the {V}")
        if not 0 <= d < V:
            raise ValueError(f"delimiter: {d} is no symbol of the {V}")
        if d == blank:
            raise ValueError("delimiter: the word delimiter cannot be the blank")
        pen = float(oov_penalty)
        if pen != pen or pen > 0.0:
            raise ValueError(f"oov_penalty: a value <= 0 is wanted, -inf for the hard lexicon constraint (got {oov_penalty!r})")
        pool = word_lm.word_pool
        if pool.size and int(pool.max()) >= V:
            raise ValueError(f"vocab: a word's spelling holds token {int(pool.max())}, outside the {V} symbols")
        if (pool == d).any():
            raise ValueError(f"delimiter: token {d} stands inside a word's spelling")
        if (pool == blank).any():
            raise ValueError(f"blank: token {blank} stands inside a word's spelling")
        self.word_lm, self.vocab, self.delimiter, self.blank = word_lm, V, d, blank
        self.oov_penalty = float(np.float32(pen))
        self._build()
        self._states = {(): (0, ())}
        self._device_tables = {}

    def _build(self):
        V, d, blank, lm = self.vocab, self.delimiter, self.blank, self.word_lm
        kids, word = [{}], [-1]                               # the trie in insertion order ...
        for wid in range(N_RESERVED, lm.n_words):
            q = 0
            for t in lm.spellings[wid]:
                nx = kids[q].get(t)
                if nx is None:
                    nx = len(kids)
                    kids[q][t] = nx
                    kids.append({})
                    word.append(UNK)
                q = nx
            word[q] = wid
        S = len(kids) + 1
        if S * V > MAX_BIAS_WORDS:
            raise ValueError(f"word_lm: the lexicon trie has {S} states over {V} symbols: {S * V} table words, the limit is 2**24")
        order, new_of, head = [0], {0: 0}, 0                  # ... renumbered breadth first, children in symbol order
        while head < len(order):
            old = order[head]
            for t in sorted(kids[old]):
                new_of[kids[old][t]] = len(order)
                order.append(kids[old][t])
            head += 1
        sink = S - 1
        nxt = np.full((S, V), sink, dtype=np.int32)
        bonus = np.zeros((S, V), dtype=np.float32)
        bonus[:sink] = np.float32(self.oov_penalty)           # out of the lexicon, unless a child says otherwise
        node_word = np.full(S, UNK, dtype=np.int32)
        for q, old in enumerate(order):
            node_word[q] = word[old]
            for t, c in kids[old].items():
                nxt[q, t] = new_of[c]
                bonus[q, t] = 0.0
        nxt[:, blank] = np.arange(S, dtype=np.int32)
        bonus[:, blank] = 0.0
        nxt[:, d] = 0
        bonus[:, d] = np.where(node_word == UNK, np.float32(self.oov_penalty), np.float32(0.0))      # a non-terminal node closed by d
        bonus[0, d] = bonus[sink, d] = 0.0
        self.next, self.trie_bonus, self.node_word = np.ascontiguousarray(nxt), np.ascontiguousarray(bonus), node_word
        self.n_states, self.sink = S, sink

    # ---------------------------------------------------------------- persistence
    def save(self, path):
        """The word model's arrays and the fusion's own arguments (.npz); ``load`` builds the same trie again."""
        lm = self.word_lm
        lm._save(path, word_pool=lm.word_pool, word_off=lm.word_off, order=np.int64(lm.order), blank=np.int64(lm.blank),
                 delimiter=np.int64(lm.delimiter), fusion_vocab=np.int64(self.vocab), fusion_delimiter=np.int64(self.delimiter),
                 fusion_blank=np.int64(self.blank), oov_penalty=np.float32(self.oov_penalty))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            lm = WordNgramLM(z["word_pool"], z["word_off"], *WordNgramLM._saved_arrays(z), blank=int(z["blank"]),
                             delimiter=int(z["delimiter"]))
            return cls(lm, int(z["fusion_vocab"]), int(z["fusion_delimiter"]), blank=int(z["fusion_blank"]),
                       oov_penalty=float(z["oov_penalty"]))

    # ---------------------------------------------------------------- queries (the host's own statement)
    def transition(self, q, s):
        """(next state, the trie's bonus as a Python float) of token ``s`` in state ``q``: for the delimiter the root and the
        ``oov_penalty`` a delimiter behind ``q`` is charged (the word model's term is ``bonus``'s); a token outside [0, vocab) or
        equal to the blank leaves the state unchanged and adds nothing."""
        q, s = int(q), int(s)
        if s < 0 or s >= self.vocab or s == self.blank:
            return q, 0.0
        return int(self.next[q, s]), float(self.trie_bonus[q, s])

    def _state(self, prefix):
        """(trie state, the last order-1 completed word ids) of a prefix, remembered per prefix."""
        prefix = tuple(int(t) for t in prefix)
        st = self._states.get(prefix)
        if st is not None:
            return st
        if len(self._states) > (1 << 20):
            self._states = {(): (0, ())}
        k = len(prefix)
        while prefix[:k] not in self._states:
            k -= 1
        st = self._states[prefix[:k]]
        keep = self.word_lm.order - 1
        for i in range(k, len(prefix)):
            q, hist = st
            s = prefix[i]
            if s == self.delimiter:
                if q != 0:
                    hist = (hist + (int(self.node_word[q]),))[-keep:] if keep else ()
                st = (0, hist)
            else:
                st = (self.transition(q, s)[0], hist)
            self._states[prefix[:i + 1]] = st
        return st

    def _dbonus(self, q, hist, alpha, beta):
        word = int(self.node_word[q])
        w = alpha * self.word_lm.score(hist, word) + beta
        if word == UNK and q != self.sink:
            w = w + float(self.trie_bonus[q, self.delimiter])
        return w

    def bonus(self, prefix, s, alpha, beta):
        """What the extension of ``prefix`` by the non-blank token ``s`` adds, in Python floats with the device's rounding order."""
        q, hist = self._state(prefix)
        s = int(s)
        if s != self.delimiter:
            return self.transition(q, s)[1]
        if q == 0:
            return 0.0
        return self._dbonus(q, hist, float(alpha), float(beta))

    def final(self, prefix, alpha, beta, eos=True):
        """fin(prefix): the delimiter's bonus of a pending word, and with ``eos`` alpha * score(hist', </s>) added to it."""
        q, hist = self._state(prefix)
        alpha, beta = float(alpha), float(beta)
        fin = 0.0
        if q != 0:
            fin = self._dbonus(q, hist, alpha, beta)
        if eos:
            if q != 0:
                hist = hist + (int(self.node_word[q]),)
            fin = fin + alpha * self.word_lm.score(hist, EOS)
        return fin

    # ---------------------------------------------------------------- the device's tables
    def device_tables(self, device):
        """(trie, node_word, word_lm) on ``device``, made once per device: the trie as an (S * V, 2) int32 tensor -- word (q, s) =
        {next, the bonus' bits}, the layout of ``HotwordBias.device_table`` --, node_word (S,) int32, and the word model's own
        ``device_tables``."""
        import torch

        def make(dev):
            words = np.empty((self.n_states * self.vocab, 2), dtype="<i4")
            words[:, 0] = self.next.reshape(-1)
            words[:, 1] = self.trie_bonus.reshape(-1).view(np.int32)
            return WordFusionDeviceTables(torch.from_numpy(words).to(dev).contiguous(),
                                          torch.from_numpy(self.node_word).to(dev).contiguous(), self.word_lm.device_tables(dev))
        return _on_device(self._device_tables, device, make)
