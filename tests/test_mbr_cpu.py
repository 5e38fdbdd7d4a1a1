"""Minimum-Bayes-risk decoding on a GPU-less host: the helper's DP against the oracle's edit distance on the goldens, the two new
entry points' export, binding and refusals (all before any HIP call), the host layer's refusals and unchanged defaults, and the
premises of the generated cases the GPU file compares the device on -- asserted here on the helper alone."""
import ctypes
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mbr_ref as M  # noqa: E402
from oracle import decode_ref  # noqa: E402

HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
INVALID_ARG, UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def test_helper_dp_is_the_oracles_edit_distance(golden_dir):
    vec = json.load(open(os.path.join(golden_dir, "reference_vectors.json")))["text"]
    pairs = [(a, b, w[0]) for a, b, w in vec["edit_dist"]] + [(a, b, w[0]) for a, b, w in vec["edit_dist_tokens"]]
    assert len(pairs) >= 30
    for a, b, want in pairs:
        assert M.lev(list(a), list(b)) == want == decode_ref.edit_dist(a, b)[0]
    # the row-wise form is the same recurrence: the strings of the goldens as one batch of pairs, and as one list
    strs = [a for a, _, _ in pairs if isinstance(a, str)] + [b for _, b, _ in pairs if isinstance(b, str)]
    S = max(len(s) for s in strs) + 3
    tokens = np.full((len(strs), 1, S), 7, dtype=np.int32)
    lengths = np.array([[len(s)] for s in strs], dtype=np.int32)
    for n, s in enumerate(strs):
        tokens[n, 0, :len(s)] = [ord(c) for c in s]
    dist = M.pair_dist_ref(tokens, lengths, np.array([len(strs)]), 256, M.LMAX)
    for n, a in enumerate(strs):
        for m, b in enumerate(strs):
            assert dist[0, n, m] == decode_ref.edit_dist(a, b)[0]


def test_helper_rules_on_hand_cases():
    assert M.lev([1, 2, 3], [1, 2, 3], V=4) == 0 and M.lev([1, 4, 3], [1, 4, 3], V=4) == 1 and M.lev([-1], [-1], V=4) == 1
    tokens = np.array([[[1, 2, 9]], [[1, 2, 9]], [[1, 5, 5]], [[3, 3, 3]]]); lengths = np.array([[2], [3], [1], [3]])
    d = M.pair_dist_ref(tokens, lengths, np.array([3]), 4, 2)
    assert d[0].tolist() == [[0, -1, 1, -1], [-1, -1, -1, -1], [1, -1, 0, -1], [-1, -1, -1, -1]]       # row 1 over Lmax, row 3 beyond count
    assert M.split_words([], 5) == [()] and M.split_words([5], 5) == [(), ()] and M.split_words([1, 5, 5, 2], 5) == [(1,), (), (2,)]
    assert [len(M.split_words(r, 5)) for r in ([5, 1], [1, 5], [1, 2])] == [len(s.split(" ")) for s in (" a", "a ", "ab")]
    # the selection on two rows: p = (1/(1+e^-1), e^-1/(1+e^-1)), risk = the other row's mass times the distance
    best, risk, post = M.select_ref(np.array([[[0, 3], [3, 0]]]), np.array([[2.0], [3.0]]), np.array([2]), 1.0)
    p0 = 1.0 / (1.0 + np.exp(-1.0))
    assert post[:, 0] == pytest.approx([p0, 1 - p0], rel=1e-15) and risk[:, 0] == pytest.approx([3 * (1 - p0), 3 * p0], rel=1e-15)
    assert best[0] == 0
    best, risk, post = M.select_ref(np.array([[[0, 3], [3, 0]]]), np.array([[2.0], [3.0]]), np.array([2]), 0.0)
    assert post[:, 0].tolist() == [0.5, 0.5] and risk[:, 0].tolist() == [1.5, 1.5] and best[0] == 0      # a tie: the first wins


def test_new_symbols_exported_and_bound_abi_stays_7(lib):
    from policy_gradient_asr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("pgasr_nbest_pair_dist", "pgasr_mbr_select"):
        assert hasattr(lib, name)
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]) == 10
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    assert _lib.SIGNATURES["pgasr_mbr_select"][1][5] is ctypes.c_double
    assert int(re.search(r"#define PGASR_ABI_VERSION (\d+)", src).group(1)) == 7 and lib.pgasr_abi_version() == 7
    assert "A7-MBR" in open(HEADER).read()


P = 0x1000          # fake pointers: every call below must return before dereferencing or launching anything


def _pair(lib, N=4, B=2, V=29, stride=10, Lmax=10, tokens=P, length=P, count=P, dist=P):
    return lib.pgasr_nbest_pair_dist(tokens, stride, length, count, N, B, V, Lmax, dist, None)


def test_pair_dist_refusals_need_no_device(lib):
    assert _pair(lib, N=0) == UNSUPPORTED and _pair(lib, N=129) == UNSUPPORTED
    assert _pair(lib, V=0) == UNSUPPORTED and _pair(lib, V=65) == UNSUPPORTED
    assert _pair(lib, Lmax=-1) == UNSUPPORTED and _pair(lib, Lmax=1025) == UNSUPPORTED
    for name in ("tokens", "length", "count", "dist"):
        assert _pair(lib, **{name: None}) == INVALID_ARG, name
    assert _pair(lib, B=0) == INVALID_ARG and _pair(lib, stride=0) == INVALID_ARG
    assert _pair(lib, N=129, B=0) == UNSUPPORTED and _pair(lib, V=65, tokens=None) == UNSUPPORTED      # the limits come first


def _select(lib, N=4, B=2, scale=1.0, dist=P, score=P, count=P, post=P, risk=P, best=P):
    return lib.pgasr_mbr_select(dist, score, count, N, B, scale, post, risk, best, None)


def test_mbr_select_refusals_need_no_device(lib):
    assert _select(lib, N=0) == UNSUPPORTED and _select(lib, N=129) == UNSUPPORTED
    for name in ("dist", "score", "count", "post", "risk", "best"):
        assert _select(lib, **{name: None}) == INVALID_ARG, name
    assert _select(lib, B=0) == INVALID_ARG
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
        assert _select(lib, scale=bad) == INVALID_ARG, bad
    assert _select(lib, N=129, scale=-1.0) == UNSUPPORTED


def test_host_layer_refusals_and_unchanged_defaults():
    import torch
    from policy_gradient_asr_amd import hipops, model, _lib
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder, MBRDecoded
    tok, ln, cnt = torch.zeros(2, 1, 4, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    with pytest.raises(_lib.PgasrError):
        hipops.nbest_pair_distance(tok, ln, cnt, 5, max_hyp_len=4)
    with pytest.raises(_lib.PgasrError):
        hipops.mbr_select(torch.zeros(1, 2, 2, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.float64), cnt)
    assert MBRDecoded._fields == ("tokens", "lengths", "best", "risk", "posterior", "dist", "nbest")
    nb = hipops.CTCNBest(tok, ln, torch.zeros(2, 1, dtype=torch.float64), cnt)
    with pytest.raises(ValueError):
        CTCDecoder(list("abcd")).mbr_from_list(nb, nb.score, risk_unit="phone")
    with pytest.raises(_lib.PgasrError):
        CTCDecoder(list("abcd")).mbr_from_list(nb, nb.score, max_hyp_len=4)
    sig = inspect.signature(CTCDecoder.mbr_decode).parameters
    assert [sig[k].default for k in ("lengths", "beam_size", "nbest", "risk_unit", "word_delimiter", "acoustic", "posterior_scale",
                                     "am_weight", "max_hyp_len", "blank")] == [None, 16, 16, "char", None, "ctc", 1.0, 1.0, None, 0]
    sig = inspect.signature(hipops.nbest_pair_distance).parameters
    assert list(sig) == ["tokens", "lengths", "count", "vocab", "max_hyp_len", "unit", "delimiter"]
    assert inspect.signature(hipops.mbr_select).parameters["scale"].default == 1.0
    sig = inspect.signature(model.predict).parameters
    assert [sig[k].default for k in ("mbr", "mbr_unit", "mbr_scale")] == [False, "char", 1.0]
    assert [sig[k].default for k in ("beam_size", "nbest", "rescore_lm_path", "lm_fast", "target_rate")] == [5, 1, None, False, None]
    with pytest.raises(ValueError):
        model.predict(None, None, os.devnull, os.devnull, 1, mbr=True)            # needs a list: refused before anything is read


def test_the_case_list_covers_what_it_must():
    cases = M.PAIR_CASES
    assert {c[1] for c in cases} >= {1, 2, 3, 16, 17, 64, 65, 128} and {c[3] for c in cases} >= {2, 29, 64}
    assert {c[2] for c in cases} == {1, 3}
    seen = set()
    for c in cases:
        seen |= {"0" if k == 0 else "1" if k == 1 else "N" if k == c[1] else "N-1" if k == c[1] - 1 else "other" for k in c[6]}
    assert seen >= {"0", "1", "N-1", "N"}
    assert {c[4] for c in cases} >= {"near", "unrelated", "over", "bad-symbol"}


@pytest.mark.parametrize("name", ["n3", "n16-edges", "n17-v2", "over-lmax", "symbol-ge-v", "n17-near-129"])
def test_pair_cases_satisfy_their_premises(name):
    tokens, lengths, count, V, Lmax, want = M.pair_case(name)
    N, B, S = tokens.shape
    assert S > lengths.max()
    # the garbage behind every length really differs from zero
    for n in range(N):
        for b in range(B):
            assert (tokens[n, b, lengths[n, b]:] != 0).all()
    assert (want == np.transpose(want, (0, 2, 1))).all()
    if name == "n16-edges":
        assert sorted(set(lengths[:, 0].tolist())) == sorted(M.EDGE_LENGTHS)
    if name == "n3":
        assert {1023, 1024, 513, 64, 0, 129} == set(lengths.reshape(-1).tolist())
    if name == "over-lmax":
        over = lengths > Lmax
        assert over.any() and Lmax == 64
        for b in range(B):
            for n in range(N):
                if over[n, b]:
                    assert (want[b, n, :] == -1).all() and (want[b, :, n] == -1).all()
                elif n < count[b]:
                    assert want[b, n, n] == 0
        assert (want[2, 7, :] == -1).all()                                      # count 7: the last row is beyond it
    if name == "symbol-ge-v":
        assert (tokens[1, 0, :9] == tokens[2, 0, :9]).all() and want[0, 1, 2] == 1 and want[0, 0, 1] == 1 and want[0, 3, 3] == 0
        assert ((tokens[:, 0, :9] >= V) | (tokens[:, 0, :9] < 0)).sum() == 4
    if name == "n17-near-129":
        assert 0 < want.max() <= 12                                              # two rows of <= 6 edits each


def test_selection_cases_satisfy_their_premises():
    dist, score, count, scale = M.select_general()
    best, risk, post = M.select_ref(dist, score, count, scale)
    assert (best != 0).sum() * 4 >= len(best) and (np.argmin(score, axis=0) == 0).all()         # the MAP row is row 0 and loses
    assert post.sum(axis=0) == pytest.approx(np.ones(len(best)), rel=1e-14)
    # the exactness cases: scale 0, power-of-two counts, and in the second half two least risks that are exactly equal
    dist, score, count, scale = M.select_exact()
    assert scale == 0.0 and sorted(set(count.tolist())) == [1, 2, 4, 8, 16]
    best, risk, post = M.select_ref(dist, score, count, scale)
    for b, c in enumerate(count):
        assert (post[:c, b] == 1.0 / c).all() and (post[c:, b] == 0).all() and np.isinf(risk[c:, b]).all()
        assert (risk[:c, b] * c == np.round(risk[:c, b] * c)).all()              # multiples of 1 / count: nothing was rounded
    for b in range(5, len(count)):
        c = int(count[b])
        col = risk[:c, b]
        first, second = (0, 1) if c == 2 else (c // 2, c - 1)
        assert col[first] == col[second] == col.min() and (col == col.min()).sum() == 2 and best[b] == first
    assert (best[5:][count[5:] > 2] != 0).all()
    dist, score, count, scale = M.select_other()
    best, risk, post = M.select_ref(dist, score, count, scale)
    assert not np.isfinite(score[[0, 2, 3], 0]).any() and (post[[0, 2, 3], 0] == 0).all() and np.isinf(risk[[0, 2, 3], 0]).all()
    assert post[0, 1] == 0 and np.isinf(risk[0, 1]) and best[1] != 0
    assert (post[:, 2] == 0).all() and best[2] == 0 and (post[:, 3] == 0).all() and best[3] == 0 and np.isinf(risk[:, 3]).all()
    assert (post[5:, 4] == 0).all() and post[:5, 4].sum() == pytest.approx(1.0, rel=1e-14)
    assert all(M.best_within_margin(best, risk))


def test_word_case_holds_every_delimiter_position():
    tokens, lengths, count, d = M.word_case()
    rows = [list(tokens[n, 0, :lengths[n, 0]]) for n in range(tokens.shape[0])]
    assert any(r and r[0] == d for r in rows) and any(r and r[-1] == d for r in rows)
    assert any(any(a == d and b == d for a, b in zip(r, r[1:])) for r in rows) and [] in rows
    want = M.word_pair_dist_ref(tokens, lengths, count, d, M.LMAX)
    assert want[0, 0, 1] == 1 and want[0, 0, 2] == 1 and want[0, 0, 3] == 1 and want[0, 0, 7] == 1      # one (empty or changed) word apart
    assert want[0, 4, 5] == 1 and want[0, 5, 6] == 1                                                     # '' / ' ' / '  ': 1, 2, 3 empty words
    assert (want[1, 9, :] == -1).all()
