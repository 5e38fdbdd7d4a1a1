"""Subword units: an alphabet whose symbols are strings of one or more characters (word pieces, BPE units).

A units file has the ``alphabet.txt`` format -- one unit per line, index = line number + 1, index 0 the pad / CTC blank that
``model._read_alphabet`` puts in front -- so a units file can stand wherever an alphabet file stands.  Pure Python, no third-party
import: the encoder is host string work in front of the data loader."""


class SubwordUnits:
    """SubwordUnits(units): ``units[i]`` is the string of token id i + 1; id 0 is the pad / blank and never produced.

    ``encode`` is greedy longest match, left to right, over a trie of the units.  Where every single character of the texts is a
    unit (``learn_bpe`` guarantees it for its base alphabet) every string encodes; a position where no unit matches raises."""

    def __init__(self, units):
        units = [str(u) for u in units]
        if not units:
            raise ValueError("SubwordUnits needs at least one unit")
        seen = set()
        for u in units:
            if u == "" or "\n" in u or "\r" in u:
                raise ValueError(f"a unit is a non-empty string without line breaks (got {u!r})")
            if u in seen:
                raise ValueError(f"unit {u!r} is listed twice")
            seen.add(u)
        self.units = units
        self.unit2ind = {u: i + 1 for i, u in enumerate(units)}
        # trie: node = (children by character, id of the unit that ends here or 0)
        self._trie = [{}, 0]
        for u, i in self.unit2ind.items():
            node = self._trie
            for ch in u:
                node = node[0].setdefault(ch, [{}, 0])
            node[1] = i

    def __len__(self):
        """Symbols of the output layer: the units and the blank."""
        return len(self.units) + 1

    def encode(self, text):
        """text -> list of token ids, the longest unit that matches at every position."""
        out, pos, n = [], 0, len(text)
        while pos < n:
            node, best, best_end, i = self._trie, 0, pos, pos
            while i < n:
                node = node[0].get(text[i])
                if node is None:
                    break
                i += 1
                if node[1]:
                    best, best_end = node[1], i
            if not best:
                raise ValueError(f"no unit matches {text[pos]!r} at position {pos} of {text!r}")
            out.append(best)
            pos = best_end
        return out

    def decode(self, ids):
        """token ids -> text; id 0 (pad / blank) adds nothing."""
        return "".join(self.units[int(i) - 1] for i in ids if int(i) != 0)

    @classmethod
    def learn_bpe(cls, lines, n_units, alphabet=None):
        """Byte-pair encoding (Sennrich et al., arXiv:1508.07909) over whole lines, spaces included: start from the single characters
        -- ``alphabet`` (an iterable of characters, kept in its order) or, by default, the sorted characters of ``lines`` -- and merge
        the most frequent adjacent pair of units until there are ``n_units``; ties go to the lexicographically smallest pair
        (left unit, then right unit), so the result depends on the text alone.  Stops early when no pair that spells a new unit is left.
        The merged unit is appended, so the base characters keep the first indices."""
        base = list(dict.fromkeys(alphabet)) if alphabet is not None else sorted({ch for line in lines for ch in line})
        for ch in base:
            if len(ch) != 1:
                raise ValueError(f"the base alphabet holds single characters (got {ch!r})")
        known = set(base)
        seqs = []
        for line in lines:
            line = line.rstrip("\n")
            for ch in line:
                if ch not in known:
                    raise ValueError(f"character {ch!r} is not in the base alphabet")
            if line:
                seqs.append(list(line))
        if int(n_units) < len(base):
            raise ValueError(f"n_units = {n_units} is less than the {len(base)} characters of the base alphabet")
        units = list(base)
        have = set(units)
        while len(units) < int(n_units):
            counts = {}
            for seq in seqs:
                for a, b in zip(seq, seq[1:]):
                    counts[(a, b)] = counts.get((a, b), 0) + 1
            # the merged string must be new: two pairs can spell the same unit
            cand = [(-c, p) for p, c in counts.items() if p[0] + p[1] not in have]
            if not cand:
                break
            _, (a, b) = min(cand)
            merged = a + b
            units.append(merged)
            have.add(merged)
            for k, seq in enumerate(seqs):
                out, i = [], 0
                while i < len(seq):
                    if i + 1 < len(seq) and seq[i] == a and seq[i + 1] == b:
                        out.append(merged)
                        i += 2
                    else:
                        out.append(seq[i])
                        i += 1
                seqs[k] = out
        return cls(units)

    def save(self, path):
        """One unit per line, the ``alphabet.txt`` format."""
        with open(path, "w") as fo:
            fo.writelines(u + "\n" for u in self.units)

    @classmethod
    def load(cls, path):
        with open(path, "r") as fo:
            return cls([line.rstrip("\n") for line in fo.readlines() if line.rstrip("\n") != ""])


SPELL_MAX_UNIT_CHARS = 64        # PGASR_SPELL_MAX_UNIT_CHARS
SPELL_MAX_SYMBOLS = 64           # the spelled rows feed the kernels that hold one symbol per lane (hipops.MAX_VOCAB_NARROW)


class UnitSpelling:
    """UnitSpelling(units, alphabet=None): the character spelling of every unit of a ``SubwordUnits``, as the tables
    ``pgasr_unit_spell`` reads.  A unit may hold a space (``learn_bpe`` merges across spaces), so unit rows have no word boundaries of
    their own; the spelled row is the text itself (``decode(encode(text)) == text``), a row over at most 64 character ids.

    alphabet: the characters in the order of the corpus' ``alphabet.txt``; default: the sorted characters that occur in the units.
    Character ids are 1 .. C in that order, id 0 is never produced, and C + 1 <= 64 is required (ValueError).
    offsets (V + 1 ints, V = len(units)): token id v spells chars[offsets[v] : offsets[v + 1]]; id 0, the blank / pad, spells nothing.
    max_unit_chars <= SPELL_MAX_UNIT_CHARS (ValueError).  delimiter: the id of " ", or None -- every word-level use then raises.
    char_alphabet: the characters, for ``metrics.ErrorReport(spelling.char_alphabet, " ")``."""

    def __init__(self, units, alphabet=None):
        if not isinstance(units, SubwordUnits):
            units = SubwordUnits(units)
        if alphabet is None:
            alphabet = sorted({ch for u in units.units for ch in u})
        alphabet = list(alphabet)
        for ch in alphabet:
            if not isinstance(ch, str) or len(ch) != 1:
                raise ValueError(f"the spelling alphabet holds single characters (got {ch!r})")
        if len(set(alphabet)) != len(alphabet):
            raise ValueError("a character is listed twice in the spelling alphabet")
        if len(alphabet) + 1 > SPELL_MAX_SYMBOLS:
            raise ValueError(f"{len(alphabet)} characters and the pad are more than {SPELL_MAX_SYMBOLS} symbols: the spelled rows must "
                             f"fit the kernels that hold one symbol per lane")
        self.units = units
        self.char_alphabet = alphabet
        self.char2ind = {ch: i + 1 for i, ch in enumerate(alphabet)}
        offsets, chars = [0, 0], []
        for u in units.units:
            if len(u) > SPELL_MAX_UNIT_CHARS:
                raise ValueError(f"unit {u!r} has {len(u)} characters, more than the {SPELL_MAX_UNIT_CHARS} that pgasr_unit_spell takes")
            for ch in u:
                if ch not in self.char2ind:
                    raise ValueError(f"character {ch!r} of unit {u!r} is not in the spelling alphabet")
                chars.append(self.char2ind[ch])
            offsets.append(len(chars))
        self.offsets = offsets                      # V + 1 entries
        self.chars = chars
        self.vocab = len(units)                     # V: the units and the blank
        self.n_symbols = len(alphabet) + 1          # the spelled rows' alphabet: the characters and the pad
        self.max_unit_chars = max(len(u) for u in units.units)
        self.delimiter = self.char2ind.get(" ")
        self._device = {}

    def word_delimiter(self, what="unit='word'"):
        """The id of ' ' for a word-level use, named in the error when the alphabet has none."""
        if self.delimiter is None:
            raise ValueError(f"{what} needs words, and the spelling alphabet has no ' ' character to split them at")
        return self.delimiter

    def spell(self, ids):
        """token ids -> list of character ids: the contract of pgasr_unit_spell on the host.  An id outside [0, V) adds nothing."""
        out = []
        for i in ids:
            i = int(i)
            if 0 <= i < self.vocab:
                out.extend(self.chars[self.offsets[i]:self.offsets[i + 1]])
        return out

    def text(self, char_ids):
        """character ids -> text; id 0 adds nothing."""
        return "".join(self.char_alphabet[int(c) - 1] for c in char_ids if int(c) != 0)

    def to(self, device):
        """(offsets, chars) as int32 tensors on ``device``, made once per device."""
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        got = self._device.get(device)
        if got is None:
            got = (torch.tensor(self.offsets, dtype=torch.int32, device=device),
                   torch.tensor(self.chars if self.chars else [0], dtype=torch.int32, device=device))
            self._device[device] = got
        return got

    @classmethod
    def load(cls, units_path, alphabet_path=None):
        """From a units file and, where given, the corpus' alphabet file (one character per line, the line's text as it stands)."""
        alphabet = None
        if alphabet_path is not None:
            with open(alphabet_path, "r") as fo:
                alphabet = [line.rstrip("\n") for line in fo.readlines() if line.rstrip("\n") != ""]
        return cls(SubwordUnits.load(units_path), alphabet)
