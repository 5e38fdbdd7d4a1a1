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
