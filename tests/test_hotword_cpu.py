"""Hotword biasing without a GPU: the automaton of lm.HotwordBias against the bias' definition (tests/hotword_ref.py), the
qualifying conditions of the GPU cases, the new entry points' argument refusals (CPU pointers: nothing could have run) and the
refusals of the host layer, each before a device is touched."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as L  # noqa: E402
import hotword_ref as H  # noqa: E402

from policy_gradient_asr_amd.lm import HotwordBias  # noqa: E402

OVERLAP = [(1, 1, 2), (1, 2), (2, 1, 1, 3)]


def _phrase_sets(V, rng):
    """Phrase sets that force failure links and overlaps: the overlapping triple, nested phrases (ab, abc), a phrase that is a
    suffix of another, and random ones."""
    a, b, c, d = (1, 2, 3, 1) if V == 4 else (5, 9, 2, 7)
    sets = [OVERLAP,
            [(a, b), (a, b, c)],                                   # nested
            [(a, b, c, d), (c, d), (d,)],                          # suffixes of another
            [(a, a), (a, a, a), (a,)]]                             # self-overlapping
    sets.append(sets[0] + sets[1] + sets[2] + [tuple(rng.integers(1, V, size=int(rng.integers(1, 6))).tolist()) for _ in range(12)])
    return sets


@pytest.mark.parametrize("V", [4, 29, 300])
@pytest.mark.parametrize("partial", [0.0, 1.0])
def test_builder_matches_the_definition(V, partial):
    """score_sequence(y) == the brute-force B(y) within 1e-5 * max(1, |B|) (the table is fp32, the brute force fp64) on random rows,
    some with phrases planted in them, with boost * length weights and with per-phrase weights."""
    rng = np.random.default_rng(100 * V + int(partial))
    for k, phrases in enumerate(_phrase_sets(V, rng)):
        for weights in (None, [0.25 * (i + 1) for i in range(len(phrases))]):
            hb = HotwordBias(phrases, V, boost=1.5, weights=weights, partial=partial)
            assert len(hb.phrases) == len(set(phrases)) and hb.next.shape == hb.bonus.shape == (hb.n_states, V)
            hits = 0
            for _ in range(60):
                hi = 4 if k < 4 and V > 4 else V               # few symbols: the small sets' phrases then occur by chance ...
                y = rng.integers(1, hi, size=int(rng.integers(0, 24))).tolist()
                if V > 4 and k < 4:
                    y = [(5, 9, 2, 7)[t] for t in y]
                if rng.random() < 0.5 and y:                   # ... and are planted as well
                    p = phrases[int(rng.integers(len(phrases)))]
                    i = int(rng.integers(0, len(y)))
                    y = y[:i] + list(p) + y[i:]
                want = H.brute_bias(y, hb.phrases, hb.weights, boost=1.5, partial=partial)
                got = hb.score_sequence(y)
                assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (phrases, y, got, want)
                hits += want != 0
            assert hits >= 10


def test_blank_column_numbering_and_persistence(tmp_path):
    hb = HotwordBias(OVERLAP + [(3, 3)], 5, blank=4, boost=2.0, partial=0.5)
    S = hb.n_states
    # the blank column is the identity; blank and foreign tokens leave the state and add nothing
    assert np.array_equal(hb.next[:, 4], np.arange(S)) and not hb.bonus[:, 4].any()
    assert hb.transition(3, 4) == (3, 0.0) and hb.transition(3, 5) == (3, 0.0) and hb.transition(3, -1) == (3, 0.0)
    assert hb.score_sequence([1, 4, 1, 9, 2]) == hb.score_sequence([1, 1, 2])
    # breadth-first numbering, children in symbol order: root; 1, 2, 3; 11, 12, 21, 33; 112, 211; 2113
    paths = [(), (1,), (2,), (3,), (1, 1), (1, 2), (2, 1), (3, 3), (1, 1, 2), (2, 1, 1), (2, 1, 1, 3)]
    assert S == len(paths)
    for q, path in enumerate(paths):
        st = 0
        for t in path:
            st = int(hb.next[st, t])
        assert st == q and hb.depth[q] == len(path)
    # failure links resolved: after 1 1 2 the machine sits where "2" continues to "2 1"
    assert int(hb.next[8, 1]) == 6
    # duplicates are merged
    assert HotwordBias(OVERLAP + OVERLAP, 5, blank=4).n_states == HotwordBias(OVERLAP, 5, blank=4).n_states
    path = str(tmp_path / "hot.npz")
    hb.save(path)
    back = HotwordBias.load(path)
    assert back.phrases == hb.phrases and (back.vocab, back.blank, back.boost, back.partial) == (5, 4, 2.0, 0.5)
    assert np.array_equal(back.next, hb.next) and np.array_equal(back.bonus.view(np.int32), hb.bonus.view(np.int32))
    assert hb.next.dtype == np.int32 and hb.bonus.dtype == np.float32
    for bad in ([()], [(4,)], [(5,)], [(-1, 2)]):
        with pytest.raises(ValueError):
            HotwordBias(bad, 5, blank=4)
    with pytest.raises(ValueError):
        HotwordBias(OVERLAP, 5, weights=[1.0])
    with pytest.raises(ValueError):
        HotwordBias(OVERLAP, 5, weights=[1.0, float("inf"), 0.0])


def test_strings_and_units():
    from policy_gradient_asr_amd.units import SubwordUnits
    alphabet = ["<pad>", "a\n", "b\n", " \n"]
    hb = HotwordBias.from_strings(["ab\n", "", "b a"], alphabet, boost=2.0)
    assert hb.phrases == [(1, 2), (2, 3, 1)] and hb.vocab == 4 and list(hb.weights) == [4.0, 6.0]
    assert HotwordBias.from_strings(["ab"], {"<pad>": 0, "a": 1, "b": 2}).phrases == [(1, 2)]
    with pytest.raises(ValueError, match="not in the alphabet"):
        HotwordBias.from_strings(["abc"], alphabet)
    units = SubwordUnits(["a", "b", "ab", "c"])
    hu = HotwordBias.from_units(["abc", "ba"], units)
    assert hu.phrases == [(3, 4), (2, 1)] and hu.vocab == 5
    assert "isolation" in HotwordBias.from_units.__doc__.lower()


def test_large_automata_and_the_size_limit():
    """3000 random phrases of length 8 over 28 symbols: one state per distinct non-empty prefix (at most 28 + 28^2 + 6 * 3000 =
    18812 of them: 20000 is out of reach for such a list); 3400 phrases give more than 20000 states; both are accepted.  S * V > 2^24
    raises."""
    rng = np.random.default_rng(5)
    for n, more_than in ((3000, 18000), (H.BIG_PHRASES, 20000)):
        phrases = rng.integers(1, 29, size=(n, 8)).tolist()
        hb = HotwordBias(phrases, 29)
        assert hb.n_states == 1 + len({tuple(p[:k]) for p in phrases for k in range(1, 9)}) > more_than
        y = phrases[7] + phrases[11][2:] + phrases[7]
        assert abs(hb.score_sequence(y) - H.brute_bias(y, hb.phrases, hb.weights)) <= 1e-5 * 16
    with pytest.raises(ValueError, match="2\\*\\*24"):
        HotwordBias(rng.integers(1, 1024, size=(2400, 8)).tolist(), 1024)       # ~17700 states x 1024 symbols


@pytest.mark.parametrize("case", H.CASES, ids=H.case_id)
def test_gpu_cases_qualify(case):
    """(a) every utterance's helper gap is at least beam_lm_ref.GAP_MIN, at N = min(beam, 16); (b) at least one utterance's 1-best
    with the bias differs from its 1-best at weight 0 and at least half the utterances' best rows have B(y) != 0."""
    lp, lens, table, bias, plain = H.case_inputs(case)
    ref = H.case_reference(case)
    changed = nonzero = 0
    for b in range(H.B):
        hyps, gap = ref[b]
        print(f"{H.case_id(case)} b={b}: gap {gap:.3e} best {hyps[0][0]} plain {plain[b]}")
        assert gap >= L.GAP_MIN, (b, gap)
        changed += tuple(hyps[0][0]) != plain[b]
        nonzero += H.brute_bias(hyps[0][0], bias.phrases, bias.weights) != 0
    assert changed >= 1 and 2 * nonzero >= H.B, (changed, nonzero)
    if case[6] == "big":
        assert bias.n_states > 20000


# ---------------------------------------------------------------- ABI
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, 1, 3, 4


def _search_args(lib, nbest, T=6, B=2, V=29, beam=4, flags=0):
    """Valid arguments of the two searches, all in HOST memory and with NO workspace: whatever passed the checks would stop at
    PGASR_ERR_WORKSPACE before any HIP call."""
    keep = [np.zeros((T, B, V), dtype=np.float32), np.zeros((max(nbest, 1), B, T), dtype=np.int32),
            np.zeros((max(nbest, 1), B), dtype=np.int32), np.zeros((max(nbest, 1), B), dtype=np.float64), np.zeros(B, dtype=np.int32),
            np.zeros(V * 4, dtype=np.int64)]
    lp, tok, tl, sc, cnt, table = (a.ctypes.data for a in keep)
    head = [lp, 0, B * V, V, None, T, B, V, beam, 0, flags]
    if nbest:
        return keep, table, head + [nbest, tok, T, tl, sc, cnt, None, 0, None, None, 0, 0.0, 0.0]
    return keep, table, head + [tok, tl, sc, None, 0, None, None, 0, 0.0, 0.0]


@pytest.mark.parametrize("nbest", [0, 3])
def test_entry_points_refuse_bad_bias_arguments(nbest):
    from policy_gradient_asr_amd import _lib
    lib = _lib.load()
    fn = lib.pgasr_ctc_beam_search_nbest_bias if nbest else lib.pgasr_ctc_beam_search_bias
    plain = lib.pgasr_ctc_beam_search_nbest if nbest else lib.pgasr_ctc_beam_search_lm
    keep, table, args = _search_args(lib, nbest)
    assert fn(*args, table, 4, 1.0) == WORKSPACE                     # a good table passes the checks (and stops at the workspace)
    assert fn(*args, None, 0, 1.0) == plain(*args) == WORKSPACE      # no table, no states: the call without
    assert fn(*args, None, 4, 1.0) == INVALID                        # a null table
    assert fn(*args, table, 0, 1.0) == INVALID                       # bias_states < 1
    assert fn(*args, table, -3, 1.0) == INVALID
    assert fn(*args, table, (1 << 24) // 29 + 1, 1.0) == INVALID     # bias_states * V > 2^24
    assert fn(*args, table, (1 << 24) // 29, 1.0) == WORKSPACE
    for w in (float("nan"), float("inf"), -float("inf")):
        assert fn(*args, table, 4, w) == INVALID                     # a weight that is not finite
    for flags in (8, 16, 24, 9):
        fkeep, ftable, fargs = _search_args(lib, nbest, flags=flags)
        assert fn(*fargs, ftable, 4, 1.0) == UNSUPPORTED             # the single-wave kernel's bits
        assert fn(*fargs, None, 0, 1.0) == WORKSPACE                 # without a table they are what they were


def test_second_pass_entry_refuses_bad_arguments():
    from policy_gradient_asr_amd import _lib
    lib = _lib.load()
    tok, ln, cnt = np.zeros((2, 1, 4), dtype=np.int32), np.zeros((2, 1), dtype=np.int32), np.zeros(1, dtype=np.int32)
    out, table = np.zeros((2, 1)), np.zeros(29 * 4, dtype=np.int64)
    p = [a.ctypes.data for a in (tok, ln, cnt)]
    fn = lib.pgasr_nbest_bias_score
    assert fn(*p, 129, 1, 4, 29, table.ctypes.data, 4, out.ctypes.data, None) == UNSUPPORTED
    assert fn(*p, 0, 1, 4, 29, table.ctypes.data, 4, out.ctypes.data, None) == UNSUPPORTED
    assert fn(*p, 2, 1, 4, 1025, table.ctypes.data, 4, out.ctypes.data, None) == UNSUPPORTED
    assert fn(*p, 2, 1, 4, 29, None, 4, out.ctypes.data, None) == INVALID
    assert fn(*p, 2, 1, 4, 29, table.ctypes.data, 0, out.ctypes.data, None) == INVALID
    assert fn(*p, 2, 1, 4, 29, table.ctypes.data, (1 << 24) // 29 + 1, out.ctypes.data, None) == INVALID
    assert fn(*p, 2, 0, 4, 29, table.ctypes.data, 4, out.ctypes.data, None) == INVALID
    assert fn(*p, 2, 1, 0, 29, table.ctypes.data, 4, out.ctypes.data, None) == INVALID
    assert fn(p[0], None, p[2], 2, 1, 4, 29, table.ctypes.data, 4, out.ctypes.data, None) == INVALID
    assert fn(*p, 2, 1, 4, 29, table.ctypes.data, 4, None, None) == INVALID


def test_new_symbols_are_exported():
    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "policy_gradient_asr_amd",
                                   "libpgasr_hip.so"))
    for name in ("pgasr_ctc_beam_search_bias", "pgasr_ctc_beam_search_nbest_bias", "pgasr_nbest_bias_score"):
        assert hasattr(lib, name)
    lib.pgasr_abi_version.restype = ctypes.c_int
    assert lib.pgasr_abi_version() == 7


# ---------------------------------------------------------------- host layer
def test_keyword_defaults_and_pinned_parameter_lists():
    from policy_gradient_asr_amd import hipops, model
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    for fn in (hipops.ctc_beam_search, hipops.ctc_beam_search_nbest):
        sig = inspect.signature(fn).parameters
        assert list(sig)[-2:] == ["bias", "bias_weight"] and sig["bias"].default is None and sig["bias_weight"].default == 0.0
    assert list(inspect.signature(hipops.nbest_bias_score).parameters) == ["tokens", "lengths", "count", "bias"]
    sig = inspect.signature(CTCDecoder.__init__).parameters
    assert list(sig)[-2:] == ["hotwords", "hotword_weight"] and sig["hotwords"].default is None and sig["hotword_weight"].default == 1.0
    assert list(inspect.signature(CTCDecoder.set_hotwords).parameters)[:2] == ["self", "hotwords"]
    for fn in (CTCDecoder.decode, CTCDecoder.decode_batch):
        assert list(inspect.signature(fn).parameters)[-1] == "nbest"
    for fn in (CTCDecoder.rescore, CTCDecoder.mbr_decode):
        sig = inspect.signature(fn).parameters
        assert list(sig)[-2:] == ["bias", "bias_weight"] and sig["bias"].default is None and sig["bias_weight"].default == 0.0
    assert "first_pass" in CTCDecoder.rescore.__doc__.split("bias:")[1]
    sig = inspect.signature(model.predict).parameters
    assert list(sig)[-3:] == ["hotwords_path", "hotword_weight", "hotword_boost"]
    assert [sig[k].default for k in ("hotwords_path", "hotword_weight", "hotword_boost")] == [None, 1.0, 1.0]


def test_refusals_by_name_touch_no_device(tmp_path):
    """Every refusal raises a ValueError that names the option, on CPU tensors: a call that got past it would raise PgasrError
    (there is no CPU path) instead."""
    from policy_gradient_asr_amd import hipops, model
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    from policy_gradient_asr_amd.lm import CharNgramLM
    from policy_gradient_asr_amd.model import Seq2Seq
    from policy_gradient_asr_amd.mwer import MWERTrainer
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    hb = HotwordBias([(1, 2)], 5)
    lp = torch.zeros(4, 1, 5)
    lm = CharNgramLM(L.random_table(5, 2, 0, 0), 2)
    nb = hipops.CTCNBest(torch.zeros(2, 1, 4, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32),
                         torch.zeros(2, 1, dtype=torch.float64), torch.ones(1, dtype=torch.int32))
    # hotwords together with fast_lm
    with pytest.raises(ValueError, match="fast_lm"):
        hipops.ctc_beam_search(lp, None, lm=lm, fast_lm=True, bias=hb, bias_weight=1.0)
    with pytest.raises(ValueError, match="fast_lm"):
        hipops.ctc_beam_search_nbest(lp, None, nbest=2, lm=lm, fast_lm=True, bias=hb)
    with pytest.raises(ValueError, match="fast"):
        hipops.ctc_beam_search_nbest(lp, None, nbest=2, fast=True, bias=hb)
    with pytest.raises(ValueError, match="fast_lm"):
        CTCDecoder(list("abcde"), lm=lm, fast_lm=True, hotwords=hb)
    with pytest.raises(ValueError, match="fast_lm"):
        CTCDecoder(list("abcde"), lm=lm, hotwords=hb).decode_batch(lp, None, fast_lm=True)
    # only a HotwordBias, never raw tensors
    for raw in (torch.zeros(10, 2, dtype=torch.int32), (hb.next, hb.bonus)):
        with pytest.raises(ValueError, match="HotwordBias"):
            hipops.ctc_beam_search(lp, None, bias=raw)
        with pytest.raises(ValueError, match="HotwordBias"):
            hipops.nbest_bias_score(nb.tokens, nb.lengths, nb.count, raw)
        with pytest.raises(ValueError, match="HotwordBias"):
            CTCDecoder(list("abcde")).rescore(lp, None, nb, acoustic="first_pass", bias=raw)
    # a bias whose vocabulary or blank differs from the call's
    for other in (HotwordBias([(1, 2)], 6), HotwordBias([(1, 2)], 5, blank=3)):
        with pytest.raises(ValueError, match="bias"):
            hipops.ctc_beam_search(lp, None, bias=other)
        with pytest.raises(ValueError, match="bias"):
            hipops.ctc_beam_search_nbest(lp, None, nbest=2, bias=other)
        with pytest.raises(ValueError, match="hotwords"):
            CTCDecoder(list("abcde"), hotwords=other).decode_batch(lp, None)
        with pytest.raises(ValueError, match="hotwords"):
            CTCDecoder(list("abcde"), hotwords=other, device="cpu").decode(np.full((4, 5), 0.2))
        with pytest.raises(ValueError, match="bias"):
            CTCDecoder(list("abcde")).rescore(lp, None, nb, acoustic="first_pass", bias=other)
    # hotwords in the wide search itself
    wide_hb = HotwordBias([(1, 2)], 70)
    with pytest.raises(ValueError, match="hotwords"):
        CTCDecoder(list(range(70)), wide_search=True, hotwords=wide_hb).decode_batch(torch.zeros(4, 1, 70), None)
    with pytest.raises(ValueError, match="hotwords"):
        CTCDecoder(list(range(70)), wide_search=True, hotwords=wide_hb, device="cpu").decode(np.full((4, 70), 1 / 70))
    dec = CTCDecoder(list("abcde"))
    with pytest.raises(ValueError, match="hotwords"):
        dec.set_hotwords("ab")
    dec.set_hotwords(["bc", "de"], 2.0)                      # strings compile with the decoder's alphabet, blank 0
    assert dec.hotwords.phrases == [(1, 2), (3, 4)] and dec.hotwords.vocab == 5
    assert dec.hotword_weight == 2.0 and dec.hotwords.blank == 0
    with pytest.raises(ValueError):
        dec.set_hotwords(["ab"])                             # "a" is symbol 0, the blank
    dec.set_hotwords(None)
    assert dec.hotwords is None
    # training
    m = Seq2Seq(6, n_feats=8)
    with pytest.raises(ValueError, match="hotwords"):
        MWERTrainer(m, hotwords=hb)
    with pytest.raises(ValueError, match="hotwords"):
        PolicyGradientTrainer(m, reward_decoder="beam", hotwords=hb)
    # predict
    hot = tmp_path / "hot.txt"; hot.write_text("ab\n")
    narrow = tmp_path / "alphabet.txt"; narrow.write_text("a\nb\nc\n")
    wide = tmp_path / "units.txt"; wide.write_text("".join(f"{chr(0x100 + i)}\n" for i in range(80)))
    common = dict(test_dataset=[], n_feats=8, hotwords_path=str(hot))
    with pytest.raises(ValueError, match="hotwords_path"):
        model.predict(None, None, str(narrow), str(tmp_path), 2, beam_size=0, **common)
    with pytest.raises(ValueError, match="lm_fast"):
        model.predict(None, None, str(narrow), str(tmp_path), 2, lm_fast=True, **common)
    with pytest.raises(ValueError, match="unit_lm_path"):
        model.predict(None, None, str(narrow), str(tmp_path), 2, wide_beam=True, unit_lm_path="x.npz", **common)
    with pytest.raises(ValueError, match="units_path"):
        model.predict(None, None, str(wide), str(tmp_path), 2, wide_beam=True, wide_second_pass=True, nbest=2, **common)
    with pytest.raises(ValueError, match="wide_second_pass"):
        model.predict(None, None, None, str(tmp_path), 2, units_path=str(wide), wide_beam=True, nbest=2, **common)
    with pytest.raises(ValueError, match="wide_beam"):
        model.predict(None, None, None, str(tmp_path), 2, units_path=str(wide), **common)
