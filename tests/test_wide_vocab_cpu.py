"""Alphabets of 65 .. 1024 symbols on a GPU-less host: the four wide entry points' export, binding and argument checks (no compute
call: every rejection happens before a launch), the option rule of ``loss.check_options`` above 64 symbols, and
``units.SubwordUnits`` (encoder, BPE learner, file format)."""
import os
import random

import pytest

from policy_gradient_asr_amd import hipops
from policy_gradient_asr_amd.loss import PGOptions, check_options
from policy_gradient_asr_amd.units import SubwordUnits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
NEW = ("pgasr_log_softmax_rows_wide", "pgasr_frame_argmax_sample_wide", "pgasr_ctc_loss_grad_wide", "pgasr_ctc_grad_from_lattice_wide")
INVALID_ARG, UNSUPPORTED, WORKSPACE = 1, 4, 3


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def test_wide_symbols_exported_and_bound(lib):
    from policy_gradient_asr_amd import _lib
    header = open(HEADER).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and name + "(" in header
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1]
    assert "#define PGASR_MAX_VOCAB_WIDE 1024" in header and hipops.MAX_VOCAB_WIDE == 1024
    assert lib.pgasr_abi_version() == 7
    # the CTC pair takes its narrow twin's arguments, one for one
    assert _lib.SIGNATURES["pgasr_ctc_loss_grad_wide"] == _lib.SIGNATURES["pgasr_ctc_loss_grad"]
    assert _lib.SIGNATURES["pgasr_ctc_grad_from_lattice_wide"] == _lib.SIGNATURES["pgasr_ctc_grad_from_lattice"]


def test_wide_argument_checks_need_no_device(lib):
    """Every rejection below happens before a launch: the pointers are never dereferenced."""
    p, big = 0x1000, 1 << 40
    lsm = lib.pgasr_log_softmax_rows_wide
    assert lsm(p, 10, 1025, p, None) == UNSUPPORTED
    assert lsm(p, 10, 0, p, None) == INVALID_ARG and lsm(p, 0, 65, p, None) == INVALID_ARG
    assert lsm(None, 10, 65, p, None) == INVALID_ARG and lsm(p, 10, 65, None, None) == INVALID_ARG

    fas = lib.pgasr_frame_argmax_sample_wide
    assert fas(p, 10, 2, 1025, 0, 0, 0, 0, None, p, p, None) == UNSUPPORTED
    assert fas(p, 10, 2, 0, 0, 0, 0, 0, None, p, p, None) == INVALID_ARG
    assert fas(None, 10, 2, 65, 0, 0, 0, 0, None, p, p, None) == INVALID_ARG
    assert fas(p, 0, 2, 65, 0, 0, 0, 0, None, p, p, None) == INVALID_ARG
    assert fas(p, 10, 2, 65, 0, 0, 4, 4, None, p, p, None) == INVALID_ARG           # ctr_base outside the global batch
    assert fas(p, 10, 2, 65, 0, 0, 0, 0, p, p, p, None) == INVALID_ARG              # ids need ctr_stride >= 1
    assert fas(p, 4096, 2, 65, 0, 0, (1 << 20) + 1, 0, p, p, p, None) == UNSUPPORTED      # T * ctr_stride > 2^32 with ids
    assert fas(p, 10, 2, 1024, 0, 0, 0, 0, None, None, None, None) == 0             # nothing to write: no launch

    one = lib.pgasr_ctc_loss_grad_wide
    #        lp tg il tl  T  B    V  L bl us cf pa nll g ws bytes st
    assert one(p, p, p, p, 10, 2, 1025, 3, 0, p, p, p, p, p, p, big, None) == UNSUPPORTED
    assert one(p, p, p, p, 10, 2, 300, 1024, 0, p, p, p, p, p, p, big, None) == UNSUPPORTED          # 2 * Lmax + 1 > 2048
    assert one(p, p, p, p, 10, 2, 0, 3, 0, p, p, p, p, p, p, big, None) == INVALID_ARG
    assert one(p, p, p, p, 10, 2, 300, 3, 300, p, p, p, p, p, p, big, None) == INVALID_ARG           # blank outside [0, V)
    assert one(p, p, p, p, 10, 2, 300, 3, -1, p, p, p, p, p, p, big, None) == INVALID_ARG
    assert one(None, p, p, p, 10, 2, 300, 3, 0, p, p, p, p, p, p, big, None) == INVALID_ARG
    assert one(p, None, p, p, 10, 2, 300, 3, 0, p, p, p, p, p, p, big, None) == INVALID_ARG
    assert one(p, p, p, p, 10, 2, 300, 3, 0, p, p, p, None, p, p, big, None) == INVALID_ARG          # nll
    assert one(p, p, p, p, 10, 2, 300, 3, 0, p, p, None, p, p, p, big, None) == INVALID_ARG          # coefficient without path
    assert one(p, p, p, p, 10, 2, 300, 3, 0, p, p, p, p, p, p, 16, None) == WORKSPACE

    two = lib.pgasr_ctc_grad_from_lattice_wide
    #        lp il tl  T  B    V  L bl us cf pa pf g ws bytes st
    assert two(p, p, p, 10, 2, 1025, 3, 0, p, p, p, 0, p, p, big, None) == UNSUPPORTED
    assert two(p, p, p, 10, 2, 300, 1024, 0, p, p, p, 0, p, p, big, None) == UNSUPPORTED
    assert two(p, p, p, 10, 2, 0, 3, 0, p, p, p, 0, p, p, big, None) == INVALID_ARG
    assert two(p, p, p, 10, 2, 300, 3, 300, p, p, p, 0, p, p, big, None) == INVALID_ARG
    assert two(p, p, p, 10, 2, 300, 3, 0, p, p, p, 0, None, p, big, None) == INVALID_ARG             # grad
    assert two(p, None, p, 10, 2, 300, 3, 0, p, p, p, 0, p, p, big, None) == INVALID_ARG
    assert two(p, p, p, 10, 2, 300, 3, 0, p, p, p, 0, p, p, 16, None) == WORKSPACE
    # the narrow twins still refuse 65 symbols
    assert lib.pgasr_log_softmax_rows(p, 10, 65, p, None) == UNSUPPORTED
    assert lib.pgasr_ctc_loss_grad(p, p, p, p, 10, 2, 65, 3, 0, p, p, p, p, p, p, big, None) == UNSUPPORTED


NON_DEFAULT = [("num_samples", dict(num_samples=2)), ("baseline", dict(num_samples=2, baseline="leave_one_out")),
               ("beam", dict(beam=4)), ("score_function", dict(score_function="sequence")),
               ("entropy_weight", dict(entropy_weight=0.1)), ("kl_weight", dict(kl_weight=0.1)),
               ("reward_unit", dict(reward_unit="word", word_delimiter=3)), ("per_step", dict(per_step=True))]


@pytest.mark.parametrize("vocab", [65, 1024])
def test_check_options_admits_the_default_objective_above_64(vocab):
    opt = check_options(PGOptions(lam=0.5, seed=3, global_batch=8), vocab=vocab, frames=100, symbols=12)
    assert opt.num_samples == 1 and opt.baseline == "hypothesis"


@pytest.mark.parametrize("name,fields", NON_DEFAULT)
def test_check_options_refuses_every_other_option_above_64(name, fields):
    check_options(PGOptions(**fields), vocab=64, frames=100, symbols=12)          # fine at 64 symbols
    # (leave-one-out needs two samples at any alphabet size, so that case carries both; the baseline is the option named)
    for vocab in (65, 1024):
        with pytest.raises(ValueError, match=name + "=") as e:
            check_options(PGOptions(**fields), vocab=vocab, frames=100, symbols=12)
        assert "64" in str(e.value)


def test_check_options_refuses_more_than_1024_symbols():
    with pytest.raises(ValueError, match="1025"):
        check_options(PGOptions(), vocab=1025)


# ---- units.SubwordUnits ----
def test_longest_match_beats_a_shorter_prefix():
    u = SubwordUnits(["a", "b", "c", "ab", "abc", "bc"])
    assert u.encode("abc") == [5]                   # not "ab" + "c", not "a" + "bc"
    assert u.encode("abca") == [5, 1]
    assert u.encode("abb") == [4, 2]                # "abc" fails at its third character: back to the longest unit that ended
    assert u.encode("cab") == [3, 4]
    assert u.encode("") == []
    assert len(u) == 7
    with pytest.raises(ValueError, match="no unit matches"):
        u.encode("abd")
    with pytest.raises(ValueError):
        SubwordUnits(["a", "a"])
    with pytest.raises(ValueError):
        SubwordUnits(["a", ""])


def test_decode_inverts_encode_on_random_strings():
    base = list("abcde ")
    u = SubwordUnits(base + ["ab", "abc", "cd", "e ", " a", "dea", "bcde"])
    rng = random.Random(7)
    for _ in range(300):
        s = "".join(rng.choice(base) for _ in range(rng.randint(0, 40)))
        ids = u.encode(s)
        assert u.decode(ids) == s and all(1 <= i < len(u) for i in ids)
    assert u.decode([0, 1, 0, 2]) == "ab"           # the pad / blank adds nothing


CORPUS = ["the cat sat on the mat", "the dog ate the bone", "a cat and a dog", "that is the thing", "on and on and on",
          "the then than that", "to eat or not to eat", "hot tea at ten", "she sees the sea", "he hid the hat"]
# 15 characters in sorted order, then the merges: ('t','h') occurs 13 times; then 'at' and 'e ' tie at 11 and ('a','t') < ('e',' ')
LEARNED = [" ", "a", "b", "c", "d", "e", "g", "h", "i", "m", "n", "o", "r", "s", "t",
           "th", "at", "e ", "the ", "at ", "n ", "d ", "a ", "an", "and ", "on ", " e", " t", " the ", "cat ",
           "do", "dog", "he ", "n th", "o e", "on", "ot", "on and ", "ot t", "s the "]


def test_learn_bpe_is_deterministic_on_a_ten_line_corpus():
    u = SubwordUnits.learn_bpe(CORPUS, 40)
    assert u.units == LEARNED
    assert SubwordUnits.learn_bpe(list(reversed(CORPUS)), 40).units == LEARNED      # the text's order plays no part
    # the first merge, counted here: the most frequent adjacent pair, ties to the smallest pair
    counts = {}
    for line in CORPUS:
        for a, b in zip(line, line[1:]):
            counts[(a, b)] = counts.get((a, b), 0) + 1
    first = min(counts, key=lambda p: (-counts[p], p))
    assert first == ("t", "h") and u.units[15] == "th"
    for line in CORPUS:
        assert u.decode(u.encode(line)) == line
    assert len(u.encode("the cat sat on the mat")) < len("the cat sat on the mat") // 2
    # a given base alphabet keeps its order and its extra characters; a character outside it raises
    v = SubwordUnits.learn_bpe(["abab"], 4, alphabet="zba")
    assert v.units == ["z", "b", "a", "ab"]
    with pytest.raises(ValueError, match="base alphabet"):
        SubwordUnits.learn_bpe(["abc"], 5, alphabet="ab")


def test_save_load_round_trip_and_read_alphabet(tmp_path):
    from policy_gradient_asr_amd.model import _read_alphabet
    u = SubwordUnits.learn_bpe(CORPUS, 40)
    path = str(tmp_path / "units.txt")
    u.save(path)
    w = SubwordUnits.load(path)
    assert w.units == u.units and w.unit2ind == u.unit2ind
    alphabet, char2ind = _read_alphabet(path)
    assert len(alphabet) == len(u) == 41 and char2ind["<pad>"] == 0
    assert {k: v for k, v in char2ind.items() if v > 0} == u.unit2ind
    assert char2ind[" "] == 1 and char2ind["the "] == u.encode("the ")[0]


def test_encode_trans_takes_units():
    from policy_gradient_asr_amd.data import encode_trans
    u = SubwordUnits(["a", "b", "ab"])
    char2ind = {"<pad>": 0, "a": 1, "b": 2, "ab": 3}
    batch = [{"trans": "abab", "charmap": char2ind}, {"trans": "b", "charmap": char2ind}]
    t, m = encode_trans(batch)
    assert t.tolist() == [[1, 2, 1, 2], [2, 0, 0, 0]]
    t, m = encode_trans(batch, u)
    assert t.tolist() == [[3, 3], [2, 0]] and m.tolist() == [[1, 1], [1, 0]]
    t, _ = encode_trans([dict(b, units=u) for b in batch])
    assert t.tolist() == [[3, 3], [2, 0]]


def test_trainers_take_wide_alphabet_only_where_it_runs():
    import torch
    from policy_gradient_asr_amd.mwer import MWERTrainer
    from policy_gradient_asr_amd.train_step import DataParallelStep, PolicyGradientTrainer

    class Toy(torch.nn.Module):
        def __init__(self, V):
            super().__init__()
            self.head = torch.nn.Linear(4, V)

    assert DataParallelStep(Toy(5)).wide_alphabet is False
    assert PolicyGradientTrainer(Toy(300), wide_alphabet=True).MAX_VOCAB == 1024
    assert PolicyGradientTrainer(Toy(300)).MAX_VOCAB == 64
    with pytest.raises(ValueError, match="num_samples"):
        PolicyGradientTrainer(Toy(300), wide_alphabet=True, num_samples=2)
    with pytest.raises(ValueError, match="beam"):
        PolicyGradientTrainer(Toy(300), wide_alphabet=True, reward_decoder="beam")
    with pytest.raises(ValueError, match="1025"):
        PolicyGradientTrainer(Toy(1025), wide_alphabet=True)
    PolicyGradientTrainer(Toy(40), wide_alphabet=True, num_samples=2)               # at most 64 symbols: every option, as ever
    with pytest.raises(ValueError, match="wide_alphabet"):
        MWERTrainer(Toy(29), wide_alphabet=True)
