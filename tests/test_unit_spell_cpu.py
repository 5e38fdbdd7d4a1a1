"""Spelling subword units into characters, host side (no GPU): ``units.UnitSpelling``'s tables against the strings, its refusals,
the new entry point in the ABI table, the refusals above 64 symbols that stay word for word without a spelling, what a spelling
admits in their place, and the fixed case set of tests/unit_spell_ref.py proving itself discriminating on the reference alone."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import unit_spell_ref as R
from policy_gradient_asr_amd import _lib, hipops
from policy_gradient_asr_amd.loss import PGOptions, check_options
from policy_gradient_asr_amd.units import SPELL_MAX_UNIT_CHARS, SubwordUnits, UnitSpelling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")


def test_tables_round_trip_the_units():
    """Every unit's spelling is its string; a row's spelling is ``SubwordUnits.decode``'s text -- interior, leading and trailing
    spaces, " " alone, consecutive spaces (empty words) --, id 0 and ids outside the table add nothing, id 0 is never produced."""
    units = SubwordUnits(R.UNITS)
    sp = UnitSpelling(units, R.ALPHABET)
    assert sp.vocab == len(units) == len(R.UNITS) + 1 and len(sp.offsets) == sp.vocab + 1 and sp.offsets[:2] == [0, 0]
    assert sp.char_alphabet == R.ALPHABET and sp.delimiter == 1 and sp.n_symbols == len(R.ALPHABET) + 1
    assert sp.max_unit_chars == 3 and 0 not in sp.chars and max(sp.chars) == len(R.ALPHABET)
    for i, u in enumerate(R.UNITS, 1):
        assert sp.text(sp.chars[sp.offsets[i]:sp.offsets[i + 1]]) == u
    for name, rows in R.CASES.items():
        for row in rows:
            assert sp.text(sp.spell(row)) == units.decode(row) == R.text(R.UNITS, row), name
            assert sp.spell(row) == R.char_ids(R.UNITS, row, R.ALPHABET)
    assert sp.spell([0, 1, -1, sp.vocab, sp.vocab + 5, 2]) == sp.spell([1, 2])
    for text in ("ab cd e", "a  b", " de ", "e   "):
        assert sp.text(sp.spell(units.encode(text))) == text                # decode(encode(text)) == text: the target is the transcript
    assert [w for w in R.text(R.UNITS, R.CASES["empty-words"][0]).split(" ")] == ["a", "", "b"]
    # the default alphabet: the sorted characters that occur in the units
    assert UnitSpelling(units).char_alphabet == sorted(set("".join(R.UNITS)))
    off, pool = sp.to("cpu")
    assert off.dtype == pool.dtype == torch.int32 and off.tolist() == sp.offsets and pool.tolist() == sp.chars
    assert sp.to("cpu")[0] is off                                           # the device cache


def test_refusals_of_the_spelling():
    many = [chr(0x100 + i) for i in range(64)]
    with pytest.raises(ValueError, match="64 symbols"):
        UnitSpelling(SubwordUnits(many))                                    # 64 characters and the pad: more than 63
    assert UnitSpelling(SubwordUnits(many[:63])).n_symbols == 64
    with pytest.raises(ValueError, match="more than the 64"):
        UnitSpelling(SubwordUnits(["a", "a" * (SPELL_MAX_UNIT_CHARS + 1)]))
    assert UnitSpelling(SubwordUnits(["a", "a" * SPELL_MAX_UNIT_CHARS])).max_unit_chars == SPELL_MAX_UNIT_CHARS
    with pytest.raises(ValueError, match="not in the spelling alphabet"):
        UnitSpelling(SubwordUnits(["a", "b"]), alphabet=["a"])
    no_space = UnitSpelling(SubwordUnits(["a", "b", "ab"]))
    assert no_space.delimiter is None
    with pytest.raises(ValueError, match="no ' ' character"):
        no_space.word_delimiter()
    with pytest.raises(ValueError, match="reward_unit='word'.*no ' ' character"):
        check_options(PGOptions(reward_unit="word", unit_spelling=no_space), vocab=4)
    check_options(PGOptions(reward_unit="char", unit_spelling=no_space), vocab=4)
    t = torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="no ' ' character"):
        hipops.spelled_edit_distance(t, t[:, 0], t, t[:, 0], no_space, unit="word")
    with pytest.raises(ValueError, match="no ' ' character"):
        hipops.nbest_pair_distance_spelled(t[None], t[None, :, 0], t[0, :1], no_space, unit="word")


def test_entry_point_in_the_abi_table():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+pgasr_unit_spell\s*\(([^)]*)\)", src)
    assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES["pgasr_unit_spell"][1]) == 12
    assert _lib.SIGNATURES["pgasr_unit_spell"][0] is ctypes.c_int
    assert int(re.search(r"#define\s+PGASR_SPELL_MAX_UNIT_CHARS\s+(\d+)", src).group(1)) == SPELL_MAX_UNIT_CHARS == hipops.SPELL_MAX_UNIT_CHARS
    lib = _lib.load()
    assert lib.pgasr_unit_spell.argtypes == _lib.SIGNATURES["pgasr_unit_spell"][1]
    # checked before any HIP call: no GPU is needed for the refusals
    for args in ((0, 0, 4, 0, 0, 0, 3, 0, 4, 0, 0, 0), (0, 1, -1, 1, 1, 1, 3, 0, 4, 1, 0, 0), (0, 1, 4, 1, 1, 1, 3, 0, -1, 1, 0, 0),
                 (0, 1, 4, 1, 1, 1, 0, 0, 4, 1, 0, 0)):
        assert lib.pgasr_unit_spell(*args) == 1                             # PGASR_ERR_INVALID_ARG


def test_the_refusals_above_64_symbols_keep_their_text_without_a_spelling():
    from policy_gradient_asr_amd import model, mwer
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    word = dict(reward_unit="word", word_delimiter=5)
    with pytest.raises(ValueError) as e:
        check_options(PGOptions(**word), vocab=300, frames=100, symbols=12)
    assert str(e.value) == ("reward_unit='word' takes an alphabet of at most 64 symbols (got 300): above the 64-symbol limit only the "
                            "default objective runs -- num_samples=1, baseline='hypothesis', beam=0, score_function='path', "
                            "entropy_weight=0, kl_weight=0, reward_unit='char', no per-step rewards")
    with pytest.raises(ValueError) as e:
        check_options(PGOptions(**word), vocab=300, frames=100, symbols=12, wide_objectives=True)
    assert str(e.value).endswith("baseline='leave_one_out', entropy_weight and kl_weight, and nothing else -- beam=0, "
                                 "score_function='path', reward_unit='char', no per-step rewards")
    with pytest.raises(ValueError) as e:
        check_options(PGOptions(**word), vocab=300, frames=100, symbols=12, wide_sequence=True)
    assert str(e.value).endswith("nothing else -- beam=0, reward_unit='char', no per-step rewards")
    with pytest.raises(ValueError) as e:
        mwer.check_mwer_options(mwer.MWERWideOptions(risk_unit="word", word_delimiter=5), vocab=300)
    assert "a subword unit may span a space, so a list of units has no word boundaries of its own" in str(e.value)
    # hipops.nbest_pair_distance and CTCDecoder.mbr_from_list look at their tensors first: their refusal is held on the GPU
    assert list(inspect.signature(hipops.nbest_pair_distance).parameters)[-1] == "delimiter"      # its parameter list is fixed
    assert inspect.signature(CTCDecoder.mbr_from_list).parameters["unit_spelling"].default is None
    # the drivers: spelled needs a units file, and is refused before anything is read
    with pytest.raises(ValueError, match="needs units_path"):
        model.predict(None, None, os.devnull, os.devnull, 1, spelled=True)
    assert inspect.signature(model.predict).parameters["spelled"].default is False
    assert inspect.signature(model.train).parameters["spelled_reward"].default is False


def test_what_a_spelling_admits_and_what_it_does_not():
    from policy_gradient_asr_amd import mwer
    units, alphabet = R.random_units(300, 1)
    sp = UnitSpelling(SubwordUnits(units), alphabet)
    for kw in (dict(), dict(wide_objectives=True), dict(wide_sequence=True), dict(wide_objectives=True, wide_sequence=True)):
        opt = check_options(PGOptions(reward_unit="word", unit_spelling=sp), vocab=300, frames=5000, symbols=12, **kw)
        assert opt.unit_spelling is sp and opt.word_delimiter is None
    check_options(PGOptions(reward_unit="word", unit_spelling=sp, num_samples=4, baseline="leave_one_out", entropy_weight=0.1),
                  vocab=300, wide_objectives=True)
    with pytest.raises(ValueError, match="num_samples=4 takes an alphabet of at most 64"):
        check_options(PGOptions(reward_unit="word", unit_spelling=sp, num_samples=4), vocab=300)
    with pytest.raises(ValueError, match="beam=4 takes an alphabet of at most 64"):
        check_options(PGOptions(unit_spelling=sp, beam=4), vocab=300, wide_objectives=True, wide_sequence=True)
    with pytest.raises(ValueError, match="per_step does not take unit_spelling"):
        check_options(PGOptions(unit_spelling=sp, per_step=True), vocab=300)
    with pytest.raises(ValueError, match="give no word_delimiter"):
        check_options(PGOptions(reward_unit="word", word_delimiter=1, unit_spelling=sp), vocab=300)
    with pytest.raises(ValueError, match="spells 300 symbols"):
        check_options(PGOptions(unit_spelling=sp), vocab=299)
    with pytest.raises(ValueError, match="must be a units.UnitSpelling"):
        check_options(PGOptions(unit_spelling=object()), vocab=300)
    assert PGOptions().unit_spelling is None
    # MWER: the word risk above 64 symbols, with a spelling only
    opt = mwer.check_mwer_options(mwer._options(True, None, None, 0.0, 0.0, sp, risk_unit="word"), vocab=300, frames=5000, symbols=12)
    assert isinstance(opt, mwer.MWERSpelledOptions) and opt.unit_spelling is sp and opt.wide
    with pytest.raises(ValueError, match="needs wide_sequence=True"):
        mwer.check_mwer_options(mwer._options(False, None, None, 0.0, 0.0, sp, risk_unit="word"), vocab=300)
    assert type(mwer._options(False, None, None, 0.0, 0.0)) is mwer.MWEROptions               # without a spelling: the options as ever
    assert type(mwer._options(True, None, None, 0.0, 0.0)) is mwer.MWERWideOptions
    # a narrow units model takes a spelling too
    nu, na = R.random_units(40, 2)
    check_options(PGOptions(reward_unit="word", unit_spelling=UnitSpelling(SubwordUnits(nu), na), beam=4, score_function="sequence"), vocab=40)


def test_the_cases_discriminate_on_the_reference_alone():
    """The three metrics must be able to disagree on this case set, or a kernel that spelled nothing could pass: unit, character
    and word distance order hypotheses A and B differently, and one hypothesis is equal in words but unequal in units."""
    table = R.case_table()
    order = lambda a, b: (a > b) - (a < b)
    orders = {name: tuple(order(da[i], db[i]) for i in range(3)) for name, (da, db, _, _) in table.items()}
    assert any(o[0] != o[1] and o[0] != 0 and o[1] != 0 for o in orders.values()), orders       # units against characters
    assert any(o[1] != o[2] and o[1] != 0 and o[2] != 0 for o in orders.values()), orders       # characters against words
    assert any(o[0] != o[2] and o[0] != 0 and o[2] != 0 for o in orders.values()), orders       # units against words
    assert any(d[2] == 0 and d[0] > 0 for da, db, _, _ in table.values() for d in (da, db))      # same words, other units
    assert table["resegmented"] == ((3, 0, 0), (1, 1, 1), 7, 3)
    assert table["unit-spans-space"][0] == (1, 2, 2)                        # one wrong unit breaks two words
    assert table["empty-words"][3] == 3 and table["empty"][2:] == (0, 1)    # "a  b" has three words; the empty row one empty word
    assert R.levenshtein("kitten", "sitting") == 3 and R.levenshtein("", "abc") == 3 and R.levenshtein([], []) == 0
    out, ol, fl = R.spell_rows(R.UNITS, R.ALPHABET, [R.CASES["resegmented"][0] + [0, 0]], [5], 5)
    assert fl.tolist() == [7] and ol.tolist() == [5] and R.text(R.ALPHABET, out[0]) == "ab cd"


def test_the_objective_helper_is_the_oracles_objective():
    """tests/unit_spell_ref.objective with the unit reward is oracle.pg_ref.pg_objective, term for term: what the GPU tests change
    about the fp64 reference is the reward alone."""
    from oracle import decode_ref, pg_ref
    from pg_harness import lattice_case
    logits, targets, il, tl = lattice_case(40, 3, 9, 6, 5)
    lg, il, tl, tg = logits.numpy(), il.numpy().clip(1, 40), tl.numpy(), targets.numpy()
    for kw in (dict(num_samples=1), dict(num_samples=3, baseline="leave_one_out", entropy_weight=0.1),
               dict(num_samples=2, score_function="sequence", max_hyp_len=12)):
        o = pg_ref.pg_objective(lg, il, tg, tl, lam=1.0, seed=3, offset=1, **kw)
        K = kw.pop("num_samples")
        reward = lambda y, h: -decode_ref.edit_dist(y, h)[0] / max(len(y), 1)
        mine = R.objective(lg, il, tg, tl, reward, paths=o.paths, greedy_frames=np.argmax(lg, axis=2), **kw)
        assert mine.loss == o.loss and np.array_equal(mine.grad, o.grad) and np.array_equal(mine.R, o.R) and o.paths.shape[0] == K
