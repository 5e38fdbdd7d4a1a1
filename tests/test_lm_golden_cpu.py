"""lm.py against the files it wrote before its two back-off models were given one shared core (tests/golden/make_lm_golden.py, run
once at that commit): every array, every byte of the ARPA text, every packed table and every query value, equal and not close."""
import json
import os

import numpy as np
import pytest

from policy_gradient_asr_amd.lm import UnitNgramLM, WordNgramLM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "lm_golden.json")) as _fo:
    META = json.load(_fo)
C2I = {c: i for i, c in enumerate(META["alphabet"])}
NAMES = ("word3", "unit3", "unit1")


def build(name):
    if name == "word3":
        return WordNgramLM.from_text(META["word_lines"], C2I, order=3, min_count=2)
    return UnitNgramLM.from_transcripts(META["unit_seqs"], META["unit_vocab"], order=int(name[-1]), blank=META["unit_blank"],
                                        min_count=2)


def from_arpa(name, path):
    if name == "word3":
        return WordNgramLM.from_arpa(path, C2I)
    return UnitNgramLM.from_arpa(path, META["unit_vocab"], blank=META["unit_blank"])


def members(model):
    """The members of the model's npz file, from the live object."""
    if isinstance(model, WordNgramLM):
        out = {"word_pool": model.word_pool, "word_off": model.word_off, "order": np.int64(model.order),
               "blank": np.int64(model.blank), "delimiter": np.int64(model.delimiter)}
        logp, bow = model.logp, model.bow
    else:
        out = {"order": np.int64(model.order), "vocab": np.int64(model.vocab), "blank": np.int64(model.blank)}
        logp, bow = model.lp, model.bw
    for k in range(1, model.order + 1):
        out[f"ngrams_{k}"], out[f"logp_{k}"], out[f"bow_{k}"] = model.ngrams[k - 1], logp[k - 1], bow[k - 1]
    return out


def same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), what


def same_members(model, name):
    with np.load(os.path.join(GOLDEN, f"lm_{name}.npz"), allow_pickle=False) as z:
        got = members(model)
        assert list(got) == list(z.files)
        for key in z.files:
            same_bytes(got[key], z[key], (name, key))


@pytest.mark.parametrize("name", NAMES)
def test_the_estimate_rebuilds_every_array(name):
    same_members(build(name), name)


@pytest.mark.parametrize("name", NAMES)
def test_arpa_text_is_written_byte_for_byte(name, tmp_path):
    path = str(tmp_path / "out.arpa")
    if name == "word3":
        build(name).to_arpa(path, {i: c for c, i in C2I.items()})
    else:
        build(name).to_arpa(path)
    with open(path, "rb") as got, open(os.path.join(GOLDEN, f"lm_{name}.arpa"), "rb") as want:
        assert got.read() == want.read()


@pytest.mark.parametrize("name", NAMES)
def test_the_parents_files_read_back_into_equal_arrays(name, tmp_path):
    same_members(from_arpa(name, os.path.join(GOLDEN, f"lm_{name}.arpa")), name)
    loaded = type(build(name)).load(os.path.join(GOLDEN, f"lm_{name}.npz"))
    same_members(loaded, name)
    again = str(tmp_path / "again.npz")
    loaded.save(again)
    with np.load(again, allow_pickle=False) as new, np.load(os.path.join(GOLDEN, f"lm_{name}.npz"), allow_pickle=False) as old:
        assert new.files == old.files                        # member names in the file's own sequence
        for key in old.files:
            same_bytes(new[key], old[key], (name, key))


@pytest.mark.parametrize("name", NAMES)
def test_packed_tables_are_equal(name):
    p = build(name).pack()
    with np.load(os.path.join(GOLDEN, "lm_pack.npz"), allow_pickle=False) as z:
        want = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + ".")}
    assert sorted(p) == sorted(want)
    for key, v in want.items():
        if key == "start":
            assert type(p[key]) is int and p[key] == int(v)
        else:
            same_bytes(p[key], v, (name, key))


def test_sentence_values_are_the_same_fp64_bits():
    word = build("word3")
    for row, (logp, n_words, n_oov) in zip(META["word_rows"], META["word3"]):
        got = word.logp_sentence([C2I[c] for c in row])
        assert type(got[0]) is float and (got[0].hex(), got[1], got[2]) == (logp, n_words, n_oov), row
    for name in ("unit3", "unit1"):
        unit = build(name)
        for row, logp in zip(META["unit_rows"], META[name]):
            got = unit.logp_sequence(row)
            assert type(got) is float and got.hex() == logp, (name, row)
