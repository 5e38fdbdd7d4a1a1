"""Drop-in for the reference's metrics.py (edit_dist, evaluate, save_predictions) on the HIP
Levenshtein kernel (csrc/editdist.hip), and the error breakdown on the alignment kernel (csrc/editops.hip)."""
import collections
import os

import torch

from . import hipops
from .CTCdecoder import _device


def _encode(seqs):
    """Map arbitrary hashable symbols (chars or word strings) to dense int32 ids >= 1."""
    table = {}
    out = []
    for s in seqs:
        ids = []
        for tok in s:
            if tok not in table:
                table[tok] = len(table) + 1
            ids.append(table[tok])
        out.append(ids)
    return out


def edit_dist_batch(refs, hyps, device=None):
    """Levenshtein distances of many (reference, hypothesis) pairs in one launch.
    refs/hyps: lists of sequences (str or list of tokens).  Returns a list of ints."""
    dev = _device(device)
    n = len(refs)
    enc = [_encode([r, h]) for r, h in zip(refs, hyps)]
    R = max(max((len(e[0]) for e in enc), default=0), 1)
    Hy = max(max((len(e[1]) for e in enc), default=0), 1)
    ref = torch.zeros(n, R, dtype=torch.int32); hyp = torch.zeros(n, Hy, dtype=torch.int32)
    rl = torch.zeros(n, dtype=torch.int32); hl = torch.zeros(n, dtype=torch.int32)
    for i, (r, h) in enumerate(enc):
        ref[i, :len(r)] = torch.tensor(r, dtype=torch.int32); hyp[i, :len(h)] = torch.tensor(h, dtype=torch.int32)
        rl[i], hl[i] = len(r), len(h)
    d = hipops.edit_distance(ref.to(dev), rl.to(dev), hyp.to(dev), hl.to(dev))
    return [int(x) for x in d.tolist()]


def edit_dist(s1, s2):
    """(distance, len(s1)) between reference s1 and prediction s2 (metrics.py:4-21); str for CER,
    list of words for WER."""
    return edit_dist_batch([s1], [s2])[0], len(s1)


def evaluate(s1, s2):
    """(CER, WER) (metrics.py:23-31).  Like the reference, divides by zero on an empty reference."""
    w1, w2 = s1.split(" "), s2.split(" ")
    d = edit_dist_batch([s1, w1], [s2, w2])
    cer = d[0] / len(s1)
    wer = d[1] / len(w1)
    return cer, wer


def edit_counts(targets, tg_len, tokens, tok_len, delimiter):
    """What ``evaluate`` computes for a whole batch of token rows, without the division and without a host round trip:
    targets (B,L) / tokens (B,T) int32 on the GPU with their lengths, words split at the token ``delimiter`` (the alphabet's " ").
    Returns (character distance, character length, word distance, word count), each (B,) int32 on the device; CER = cd / cl and
    WER = wd / wc as evaluate() gives them on the decoded strings."""
    cd = hipops.edit_distance(targets, tg_len, tokens, tok_len)
    wd, wc, _ = hipops.word_edit_distance(targets, tg_len, tokens, tok_len, delimiter)
    return cd, tg_len, wd, wc


def error_counts(targets, tg_len, tokens, tok_len, delimiter):
    """``edit_counts`` with the errors told apart: (character counts (B,4), word counts (B,4)) int32 on the device, columns hits,
    substitutions, deletions, insertions of the canonical alignment (``hipops.edit_ops``: diagonal before deletion before insertion);
    words split at the token ``delimiter``.  Per row S + D + I is the distance and H + S + D the reference length that
    ``edit_counts`` returns.  No host round trip."""
    cc = hipops.edit_ops(targets, tg_len, tokens, tok_len, want_ops=False).counts
    wc = hipops.word_edit_ops(targets, tg_len, tokens, tok_len, delimiter, want_ops=False).counts
    return cc, wc


def hyp_correct(targets, tg_len, hyp, hyp_len, unit="char", delimiter=None):
    """Which positions of a hypothesis are right: targets (B,L) / hyp (B,T) int32 on the GPU with their lengths (B).  Returns
    (correct (B,T+1) float64, n (B) int32) on the device: correct[b, j] = 1.0 where the canonical alignment of hypothesis b to its
    transcript (``hipops.edit_ops``) has a hit on hypothesis position j, 0.0 elsewhere and from n[b] on, n the hypothesis' length.
    unit="word": positions are words, split at the token ``delimiter`` as str.split(" ") cuts them (correct is (B,T+2), n the
    word counts).  The slot-mass kernel with side="hyp", one pair per group and weight 1 (include/pgasr_hip.h, A10-CONF): the
    labels ``confidence_nce`` scores confidences against.  No host round trip."""
    if unit not in ("char", "word"):
        raise ValueError(f"unit must be 'char' or 'word' (got {unit!r})")
    if unit == "word":
        if delimiter is None or int(delimiter) < 0:
            raise ValueError("unit='word' needs delimiter, the token id of the alphabet's ' ' symbol")
        targets, tg_len, hyp, hyp_len = hipops.word_ids(targets, tg_len, hyp, hyp_len, int(delimiter))
    eo = hipops.edit_ops(targets, tg_len, hyp, hyp_len, want_ops=True)
    one = torch.ones(hyp.shape[0], dtype=torch.float64, device=hyp.device)
    sm = hipops.edit_ops_slot_mass(eo.ops, eo.n_ops, one, 1, side="hyp", slots=hyp.shape[1])
    return sm.hit, sm.n_slots


def confidence_nce(conf, correct, eps=1e-12):
    """NIST's normalised cross entropy of confidences, (H_max - H_conf) / H_max in bits: conf and correct equally shaped tensors
    (or sequences) over the scored positions, correct > 0.5 meaning right.  H_max = -(n_c log2 p_c + (n - n_c) log2(1 - p_c))
    with p_c = n_c / n the base rate, H_conf = -(sum over the right positions of log2 c + sum over the wrong ones of
    log2(1 - c)), c clipped to [eps, 1 - eps]; computed in fp64.  1 for perfect confidences, 0 for the base rate everywhere,
    negative for worse; NaN when all or none (or no) positions are right.  Returns a Python float (synchronises)."""
    conf = torch.as_tensor(conf).to(torch.float64).reshape(-1)
    right = torch.as_tensor(correct).to(conf.device).to(torch.float64).reshape(-1) > 0.5
    if conf.numel() != right.numel():
        raise ValueError("confidence_nce: conf and correct must have as many elements")
    n, nc = int(right.numel()), int(right.sum())
    if n == 0 or nc == 0 or nc == n:
        return float("nan")
    c = conf.clamp(float(eps), 1.0 - float(eps))
    pc = torch.tensor(nc / n, dtype=torch.float64)
    h_max = -(nc * torch.log2(pc) + (n - nc) * torch.log2(1.0 - pc))
    h_conf = -(torch.log2(c[right]).sum() + torch.log2(1.0 - c[~right]).sum())
    return float((h_max - h_conf.cpu()) / h_max)


def unit_error_counts(targets, tg_len, tokens, tok_len, spelling):
    """``edit_counts`` for rows of SUBWORD UNITS, counted on their spelled text: targets (B,L) / tokens (B,T) int32 unit rows on the GPU
    with their lengths, ``spelling`` the alphabet's ``units.UnitSpelling`` (with a " ").  Both sides go through ``hipops.unit_spell``;
    returns (character distance, character length, word distance, word count), each (B,) int32 on the device -- CER = cd / cl and
    WER = wd / wc as ``evaluate`` gives them on the decoded strings.  No host round trip."""
    delim = spelling.word_delimiter("unit_error_counts")
    rc, rl = hipops.unit_spell(targets, tg_len, spelling)
    hc, hl = hipops.unit_spell(tokens, tok_len, spelling)
    cd = hipops.edit_distance(rc, rl, hc, hl)
    wd, wc, _ = hipops.word_edit_distance(rc, rl, hc, hl, delim)
    return cd, rl, wd, wc


def _pad_rows(seqs, device):
    n = len(seqs)
    width = max(max((len(s) for s in seqs), default=0), 1)
    rows = torch.zeros(n, width, dtype=torch.int32)
    lens = torch.zeros(n, dtype=torch.int32)
    for i, s in enumerate(seqs):
        if len(s):
            rows[i, :len(s)] = torch.tensor(s, dtype=torch.int32)
        lens[i] = len(s)
    return rows.to(device), lens.to(device)


def edit_ops_batch(refs, hyps, device=None):
    """The canonical alignments of many (reference, hypothesis) pairs in one launch, beside ``edit_dist_batch``: refs / hyps are lists
    of sequences (str or list of tokens).  Returns per pair (hits, substitutions, deletions, insertions, ops), ops the list of
    operations left to right: 0 hit, 1 substitution, 2 deletion, 3 insertion."""
    dev = _device(device)
    enc = [_encode([r, h]) for r, h in zip(refs, hyps)]
    if not enc:
        return []
    ref, rl = _pad_rows([e[0] for e in enc], dev)
    hyp, hl = _pad_rows([e[1] for e in enc], dev)
    eo = hipops.edit_ops(ref, rl, hyp, hl)
    counts, ops, n_ops = eo.counts.tolist(), eo.ops.cpu(), eo.n_ops.tolist()
    return [(c[0], c[1], c[2], c[3], ops[i, :n_ops[i]].tolist()) for i, c in enumerate(counts)]


OP_LETTERS = (" ", "S", "D", "I")


def _aligned_lines(ref, hyp, ops, gap="*"):
    """sclite-style REF / HYP / OPS columns of one alignment: every column as wide as its widest entry, a run of ``gap`` where a
    side has no partner, substituted entries in upper case."""
    cols, i, j = [], 0, 0
    for o in ops:
        if o in (0, 1):
            a, b = str(ref[i]), str(hyp[j]); i += 1; j += 1
            if o == 1:
                a, b = a.upper(), b.upper()
        elif o == 2:
            a = str(ref[i]); i += 1; b = gap * max(len(a), 1)
        else:
            b = str(hyp[j]); j += 1; a = gap * max(len(b), 1)
        wd = max(len(a), len(b), 1)
        cols.append((a.ljust(wd), b.ljust(wd), OP_LETTERS[o].ljust(wd)))
    return tuple(" ".join(c[k] for c in cols).rstrip() for k in range(3))


class ErrorReport:
    """Corpus-level error statistics of decoded strings: S / D / I totals for characters and words, the character confusion matrix
    and the word confusions, the line every ASR toolkit prints.

    alphabet: the symbols, index = token id (at most 64; a character outside it is scored but stays out of the matrix);
    delimiter: the symbol words are split at (str.split(delimiter) of the strings, as ``evaluate`` does).
    ``add(refs, hyps)`` aligns a batch on the device (``hipops.edit_ops`` / ``word_edit_ops``): totals and the character confusion
    matrix accumulate there, nothing is copied back until ``summary`` / ``write``.  Word confusions are read off the word operation
    paths on the host, because words have no bounded vocabulary."""

    def __init__(self, alphabet, delimiter=" ", device=None):
        self.symbols = [str(s) for s in alphabet]
        self.vocab = len(self.symbols)
        if not 1 <= self.vocab <= hipops.EDIT_OPS_MAX_VOCAB:
            raise ValueError(f"ErrorReport: the alphabet must have 1 .. {hipops.EDIT_OPS_MAX_VOCAB} symbols (got {self.vocab})")
        self.delimiter = delimiter
        self.sym2id = {}
        for i, s in enumerate(self.symbols):
            self.sym2id.setdefault(s, i)
        # words are cut at the delimiter's token; an alphabet without it has one word per string, cut at a token that never occurs
        self.delim_id = self.sym2id.get(delimiter, 1 << 30)
        self.device = _device(device)
        self.confusion = torch.zeros(self.vocab + 1, self.vocab + 1, dtype=torch.int64, device=self.device)
        self.char_totals = torch.zeros(4, dtype=torch.int64, device=self.device)
        self.word_totals = torch.zeros(4, dtype=torch.int64, device=self.device)
        self._batches = []
        self._extra = {}

    def _ids(self, s):
        out = []
        for ch in s:
            k = self.sym2id.get(ch)
            if k is None:                  # outside the alphabet: an id of its own beyond the matrix
                k = self._extra.setdefault(ch, self.vocab + 1 + len(self._extra))
            out.append(k)
        return out

    def add(self, refs, hyps):
        """refs / hyps: equally long lists of strings (reference, hypothesis).  No host synchronisation."""
        refs, hyps = list(refs), list(hyps)
        if len(refs) != len(hyps):
            raise ValueError("ErrorReport.add: as many hypotheses as references")
        if not refs:
            return
        ref, rl = _pad_rows([self._ids(s) for s in refs], self.device)
        hyp, hl = _pad_rows([self._ids(s) for s in hyps], self.device)
        ch = hipops.edit_ops(ref, rl, hyp, hl, want_ops=True, confusion=self.confusion, vocab=self.vocab)
        wd = hipops.word_edit_ops(ref, rl, hyp, hl, self.delim_id, want_ops=True)
        self.char_totals += ch.counts.sum(0)
        self.word_totals += wd.counts.sum(0)
        self._batches.append((refs, hyps, ch, wd))

    def utterances(self):
        """Per utterance (ref, hyp, character counts, character ops, word counts, word ops), copied from the device."""
        out = []
        for refs, hyps, ch, wd in self._batches:
            cc, co, cn = ch.counts.tolist(), ch.ops.cpu(), ch.n_ops.tolist()
            wc, wo, wn = wd.counts.tolist(), wd.ops.cpu(), wd.n_ops.tolist()
            for i in range(len(refs)):
                out.append((refs[i], hyps[i], cc[i], co[i, :cn[i]].tolist(), wc[i], wo[i, :wn[i]].tolist()))
        return out

    def confusions(self):
        """Every confusion as (kind, ref, hyp, count), kind in char_sub / char_del / char_ins / word_sub / word_del / word_ins, sorted
        by falling count (ties: kind, ref, hyp)."""
        rows = []
        cm = self.confusion.cpu()
        V = self.vocab
        for r in range(V + 1):
            for h in range(V + 1):
                c = int(cm[r, h])
                if c == 0 or r == h:
                    continue
                if h == V:
                    rows.append(("char_del", self.symbols[r], "", c))
                elif r == V:
                    rows.append(("char_ins", "", self.symbols[h], c))
                else:
                    rows.append(("char_sub", self.symbols[r], self.symbols[h], c))
        words = collections.Counter()
        for ref, hyp, _, _, _, wops in self.utterances():
            rw, hw, i, j = ref.split(self.delimiter), hyp.split(self.delimiter), 0, 0
            for o in wops:
                if o == 1:
                    words[("word_sub", rw[i], hw[j])] += 1
                elif o == 2:
                    words[("word_del", rw[i], "")] += 1
                elif o == 3:
                    words[("word_ins", "", hw[j])] += 1
                i += o != 3; j += o != 2
        rows += [(k[0], k[1], k[2], c) for k, c in words.items()]
        rows.sort(key=lambda x: (-x[3], x[0], x[1], x[2]))
        return rows

    def summary(self, top_k=10):
        """Corpus-level rates, (S + D + I) / reference length, with their breakdown: {"utterances", "cer", "wer", "char": {"ref",
        "hits", "sub", "del", "ins"}, "word": {...}, "top_confusions": the first top_k rows of ``confusions``}.  Synchronises."""
        out = {"utterances": sum(len(b[0]) for b in self._batches)}
        for name, tot in (("char", self.char_totals.tolist()), ("word", self.word_totals.tolist())):
            h, s, d, i = (int(x) for x in tot)
            out[name] = {"ref": h + s + d, "hits": h, "sub": s, "del": d, "ins": i}
            out["cer" if name == "char" else "wer"] = (s + d + i) / max(h + s + d, 1)
        out["top_confusions"] = self.confusions()[:int(top_k)]
        return out

    def totals_lines(self):
        """The two corpus-level lines, e.g. ``%WER 12.32 [ 456 / 3700, 40 ins, 96 del, 320 sub ]``."""
        s = self.summary(top_k=0)
        return ["%{} {:.2f} [ {} / {}, {} ins, {} del, {} sub ]".format(
            tag, 100.0 * s[rate], v["sub"] + v["del"] + v["ins"], v["ref"], v["ins"], v["del"], v["sub"])
            for tag, rate, v in (("CER", "cer", s["char"]), ("WER", "wer", s["word"]))]

    def write(self, directory):
        """errors.txt: per utterance a header with its counts and a REF / HYP / OPS triple of padded, aligned lines over words
        (sclite style: a run of * where a side has no partner, substituted words in upper case), then the two totals lines.
        confusions.tsv: a header, then kind, ref, hyp, count per confusion, sorted by falling count."""
        with open(os.path.join(directory, "errors.txt"), "w") as fo:
            for k, (ref, hyp, cc, _, wc, wops) in enumerate(self.utterances()):
                fo.write("utt {}  char H/S/D/I {} {} {} {}  word H/S/D/I {} {} {} {}\n".format(k, *cc, *wc))
                lines = _aligned_lines(ref.split(self.delimiter), hyp.split(self.delimiter), wops)
                for tag, line in zip(("REF", "HYP", "OPS"), lines):
                    fo.write("{}: {}\n".format(tag, line))
                fo.write("\n")
            for line in self.totals_lines():
                fo.write(line + "\n")
        with open(os.path.join(directory, "confusions.tsv"), "w") as fo:
            fo.write("kind\tref\thyp\tcount\n")
            for kind, r, h, c in self.confusions():
                fo.write("{}\t{}\t{}\t{}\n".format(kind, r, h, c))


def nbest_oracle(targets, tg_len, nb, spelling=None, unit="char"):
    """The best the list could have done: targets (B,L) / tg_len (B) int32 on the GPU, ``nb`` a ``hipops.CTCNBest``.
    Returns (min character edit distance over the utterance's count hypotheses (B) int32, the first rank that reaches it (B) int32),
    on the device without a host round trip: one ``hipops.edit_distance`` launch over the N * B (target, hypothesis) pairs.
    Oracle CER = distance / tg_len; a rank > 0 says the search had a better hypothesis than the one it ranked first.
    spelling: None (default: the distance over the rows' own symbols, the unit error rate of a subword list) or the alphabet's
    ``units.UnitSpelling``: targets and list are spelled first and the distance is over the characters of the text (unit="char") or
    its words (unit="word"); a third value is then returned, the references' spelled lengths or word counts (B) int32, the
    denominator of the oracle CER / WER."""
    N, B, T = nb.tokens.shape
    L = targets.shape[1]
    ref_count = None
    if spelling is not None:
        if unit not in ("char", "word"):
            raise ValueError(f"unit must be 'char' or 'word' (got {unit!r})")
        delim = spelling.word_delimiter() if unit == "word" else None
        tc, tl = hipops.unit_spell(targets, tg_len, spelling)
        hc, hl = hipops.unit_spell(nb.tokens, nb.lengths, spelling)
        ref, ref_len = tc.repeat(N, 1), tl.repeat(N)
        hyp, hyp_len = hc.view(N * B, hc.shape[2]), hl.view(N * B)
        if unit == "word":
            dist, words, _ = hipops.word_edit_distance(ref, ref_len, hyp, hyp_len, delim)
            dist, ref_count = dist.view(N, B), words[:B]
        else:
            dist, ref_count = hipops.edit_distance(ref, ref_len, hyp, hyp_len).view(N, B), tl
    else:
        ref = targets.unsqueeze(0).expand(N, B, L).reshape(N * B, L).contiguous()
        ref_len = tg_len.unsqueeze(0).expand(N, B).reshape(N * B).contiguous()
        dist = hipops.edit_distance(ref, ref_len, nb.tokens.reshape(N * B, T), nb.lengths.reshape(N * B)).view(N, B)
    rows = torch.arange(N, dtype=torch.int32, device=dist.device).unsqueeze(1)
    dist = torch.where(rows < nb.count.unsqueeze(0), dist, torch.full_like(dist, torch.iinfo(torch.int32).max))
    best = dist.min(0).values
    rank = torch.where(dist == best.unsqueeze(0), rows.expand(N, B), torch.full_like(dist, N)).min(0).values
    return (best, rank) if spelling is None else (best, rank, ref_count)


def frame_entropy(log_probs, in_len):
    """Mean frame entropy of the policy per utterance: log_probs (T,B,V) fp32 log-softmax outputs and in_len (B) int32 on the GPU ->
    (B,) fp32 on the device, the mean over each utterance's own frames of H = -sum_v p ln p in nats (0 for an empty utterance;
    ln V for a uniform policy, 0 for a collapsed one).  The kernel of the trainer's ``entropy_weight`` term with weight 0
    (hipops.frame_entropy): lets ``predict`` or validation code watch for collapse without training.  No host round trip."""
    return hipops.frame_entropy(log_probs, in_len, 0.0, 1.0)[0]


def frame_kl(log_probs, ref_log_probs, in_len):
    """Mean frame KL(p || q) of the policy from a reference policy per utterance: log_probs and ref_log_probs (T,B,V) fp32 log-softmax
    outputs for the same batch and in_len (B) int32 on the GPU -> (B,) fp32 on the device, the mean over each utterance's own frames of
    sum_v p (ln p - max(ln q, -104)) in nats (0 for an empty utterance and where the two agree).  The kernel of the trainer's
    ``kl_weight`` term with weight 0 (hipops.frame_kl): how far a fine-tuned model has drifted from its start.  No host round trip."""
    return hipops.frame_kl(log_probs, ref_log_probs, in_len, 0.0, 1.0)[0]


def save_predictions(target, predicted, model_path):
    """predicted.txt with one 'target|prediction' line per utterance (metrics.py:33-37)."""
    path = os.path.join(model_path, "predicted.txt")
    with open(path, "w") as fo:
        for i in range(len(target)):
            fo.write(target[i] + "|" + predicted[i] + "\n")
