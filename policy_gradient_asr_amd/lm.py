"""Character n-gram language model for the fused CTC prefix beam search (csrc/beam.hip, ``pgasr_ctc_beam_search_lm``).

An LM of order ``n >= 1`` over ``V`` symbols is a dense fp32 table of natural-log probabilities of shape ``(V,)*n``:
``table[c_1, .., c_{n-1}, s] = ln p(s | c_1 .. c_{n-1})`` with ``c_{n-1}`` the most recent symbol.  The blank index never occurs
inside a prefix, so it serves as the start-of-sentence pad: the context of a prefix shorter than ``n-1`` is left-padded with
``blank``.  The column ``s == blank`` is never read and holds 0.  Building, saving and loading are host-side numpy work; the
search reads the table on the device (``device_table``)."""
import numpy as np

MAX_ENTRIES = 1 << 25      # V**n words (128 MiB): order 5 at V = 29, order 4 at V = 64 -- csrc/beam.hip refuses more


def _check_size(V, order):
    if isinstance(order, bool) or int(order) != order or order < 1:
        raise ValueError(f"LM order must be an integer >= 1 (got {order!r})")
    if V < 2:
        raise ValueError("an LM needs at least one symbol beside the blank")
    if V ** int(order) > MAX_ENTRIES:
        raise ValueError(f"an order-{order} table over {V} symbols has {V ** int(order)} entries; the limit is 2**25")


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
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._device_tables.get(device)
        if t is None:
            t = self._device_tables[device] = torch.from_numpy(self.table).to(device).contiguous()
        return t
