#!/usr/bin/env python3
"""Generate tests/golden/lm_*: what policy_gradient_asr_amd/lm.py wrote for three tiny models at the commit BEFORE its two back-off
models were given one shared core (it was run once, there; tests/test_lm_golden_cpu.py holds every later lm.py to these bytes):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_lm_golden.py

  word3  WordNgramLM.from_text, order 3, min_count=2 over a corpus with two words seen once, so that <unk> carries counts
  unit3  UnitNgramLM.from_transcripts, order 3, V = 12, blank 3, min_count=2
  unit1  the same transcripts at order 1

Per model: lm_NAME.arpa (``to_arpa``), lm_NAME.npz (``save``), the arrays of ``pack()`` in lm_pack.npz under "NAME.key"; lm_golden.json
holds the corpora, the query rows and the values ``logp_sentence`` / ``logp_sequence`` returned for them as float.hex() strings."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(1, os.path.dirname(HERE))

from policy_gradient_asr_amd.lm import UnitNgramLM, WordNgramLM     # noqa: E402
import word_lm_ref as WR                                            # noqa: E402

ALPHABET = ["<pad>", " ", "a", "b", "c"]
WORD_LINES = ["ab c ab", "ab c", "c ab ba", "ab ab c", "ca ab", "c"]        # "ba" and "ca" once each: <unk> at min_count=2
WORD_ROWS = ["ab c ab", "", "ba ab", "c c c", "ab  ca", "abc ab c"]         # an empty row, OOV words, (c, c, c) backs off twice
UNIT_V, UNIT_BLANK = 12, 3
UNIT_SEQS = [[0, 1, 2, 0, 1], [0, 1, 2], [4, 0, 1, 2], [5, 5, 5], [], [0, 1, 4], [11, 0, 1]]
UNIT_ROWS = [[], [0, 1, 2, 0, 1], [5, 5, 5, 5], [11, 10, 9], [2, 2, 0, 1, 2], [4]]   # (10, 9) after 11: down to the unigram


def main():
    c2i = {c: i for i, c in enumerate(ALPHABET)}
    pack, meta = {}, {"alphabet": ALPHABET, "word_lines": WORD_LINES, "word_rows": WORD_ROWS, "unit_vocab": UNIT_V,
                      "unit_blank": UNIT_BLANK, "unit_seqs": UNIT_SEQS, "unit_rows": UNIT_ROWS}
    word = WordNgramLM.from_text(WORD_LINES, c2i, order=3, min_count=2)
    ref, depths, oov = WR.Ref(word), set(), 0
    for row in WORD_ROWS:
        oov += WR.sentence(ref, [c2i[c] for c in row], c2i[" "], depths)[2]
    assert oov >= 2 and 2 in depths and word.n_words == 3 + 2, (oov, depths, word.n_words)
    word.to_arpa(os.path.join(HERE, "lm_word3.arpa"), {i: c for c, i in c2i.items()})
    word.save(os.path.join(HERE, "lm_word3.npz"))
    pack.update({"word3." + k: v for k, v in word.pack().items()})
    meta["word3"] = [[float(r[0]).hex(), int(r[1]), int(r[2])] for r in (word.logp_sentence([c2i[c] for c in row]) for row in WORD_ROWS)]
    for name, order in (("unit3", 3), ("unit1", 1)):
        unit = UnitNgramLM.from_transcripts(UNIT_SEQS, UNIT_V, order=order, blank=UNIT_BLANK, min_count=2)
        unit.to_arpa(os.path.join(HERE, f"lm_{name}.arpa"))
        unit.save(os.path.join(HERE, f"lm_{name}.npz"))
        p = unit.pack()
        pack.update({f"{name}.states": p["states"], f"{name}.succ": p["succ"], f"{name}.start": np.int64(p["start"])})
        meta[name] = [float(unit.logp_sequence(r)).hex() for r in UNIT_ROWS]
        if order == 3:
            assert unit.ngrams[2].shape[0] and not {(11, 10), (10, 9)} & {tuple(g) for g in unit.ngrams[1].tolist()}
    with open(os.path.join(HERE, "lm_pack.npz"), "wb") as fo:
        np.savez(fo, **pack)
    with open(os.path.join(HERE, "lm_golden.json"), "w") as fo:
        json.dump(meta, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()
