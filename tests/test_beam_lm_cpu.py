"""Language-model fusion of the CTC prefix beam search on a GPU-less host: the Witten-Bell table builder against a brute-force
dict implementation, persistence, the refusals, the fused reference search of tests/beam_lm_ref.py against the oracle at zero
weights, the new entry point's export and argument checks, and the margin condition of the cases the fp32 device path is
compared on token for token."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as R  # noqa: E402
from oracle import decode_ref  # noqa: E402

HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
INVALID_ARG, WORKSPACE, UNSUPPORTED = 1, 3, 4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def _transcripts(V, blank, seed, n=40):
    rng = np.random.default_rng(seed)
    syms = [s for s in range(V) if s != blank]
    # a skewed source so that many contexts are unseen and many are seen once
    return [[syms[int(k)] for k in np.minimum(rng.geometric(0.35, size=int(rng.integers(0, 12))) - 1, len(syms) - 1)] for _ in range(n)]


def _witten_bell_dict(seqs, V, order, blank):
    """The recursion of the issue, symbol by symbol, with dicts: returns p(s | h) as a function."""
    counts = [dict() for _ in range(order + 1)]          # counts[k][(h, s)], |h| = k - 1
    for seq in seqs:
        padded = [blank] * (order - 1) + list(seq)
        for i in range(order - 1, len(padded)):
            for k in range(1, order + 1):
                h = tuple(padded[i - k + 1:i])
                counts[k][(h, padded[i])] = counts[k].get((h, padded[i]), 0) + 1

    def p(k, h, s):
        if k == 0:
            return 0.0 if s == blank else 1.0 / (V - 1)
        c_h = sum(c for (hh, _), c in counts[k].items() if hh == h)
        lower = p(k - 1, h[1:], s)
        if c_h == 0:
            return lower
        n1 = sum(1 for (hh, _), c in counts[k].items() if hh == h and c > 0)
        return (counts[k].get((h, s), 0) + n1 * lower) / (c_h + n1)
    return p


@pytest.mark.parametrize("order,V,blank", [(1, 6, 0), (2, 6, 0), (3, 5, 0), (4, 4, 0), (3, 5, 2), (2, 7, 6)])
def test_from_transcripts_equals_brute_force_witten_bell(order, V, blank):
    from policy_gradient_asr_amd.lm import CharNgramLM
    seqs = _transcripts(V, blank, 10 * order + V)
    lm = CharNgramLM.from_transcripts(seqs, V, order=order, blank=blank)
    assert lm.table.shape == (V,) * order and lm.table.dtype == np.float32 and lm.order == order and lm.blank == blank
    p = _witten_bell_dict(seqs, V, order, blank)
    for ctx in itertools.product(range(V), repeat=order - 1):
        row = np.exp(lm.table[ctx].astype(np.float64))
        for s in range(V):
            if s == blank:
                assert lm.table[ctx + (s,)] == 0.0
            else:
                assert row[s] == pytest.approx(p(order, ctx, s), rel=1e-6), (ctx, s)
        # every context row sums to 1 over the non-blank symbols
        assert sum(row[s] for s in range(V) if s != blank) == pytest.approx(1.0, abs=1e-6), ctx
    assert np.isfinite(lm.table).all()
    # logp pads short contexts with blank and keeps the most recent symbols of long ones
    s = (blank + 1) % V
    assert lm.logp((), s) == float(lm.table[(blank,) * (order - 1) + (s,)])
    long_ctx = [(blank + 1 + i) % V for i in range(order + 2)]
    long_ctx = [c for c in long_ctx if c != blank]
    assert lm.logp(long_ctx, s) == float(lm.table[lm.context(long_ctx) + (s,)])
    assert lm.context(long_ctx) == (tuple(long_ctx[len(long_ctx) - (order - 1):]) if order > 1 else ())


def test_from_text_and_empty_corpus():
    from policy_gradient_asr_amd.lm import CharNgramLM
    char2ind = {"<pad>": 0, "a": 1, "b": 2, " ": 3}
    lm = CharNgramLM.from_text(["ab ab\n", "ba", ""], char2ind, order=2)
    want = CharNgramLM.from_transcripts([[1, 2, 3, 1, 2], [2, 1], []], 4, order=2)
    assert np.array_equal(lm.table, want.table)
    assert lm.logp([1], 2) > lm.logp([1], 1)                # "ab" was seen, "aa" never
    with pytest.raises(ValueError):
        CharNgramLM.from_text(["abc"], char2ind, order=2)
    empty = CharNgramLM.from_transcripts([], 5, order=3)      # nothing seen: uniform over the non-blank symbols
    assert np.allclose(np.exp(empty.table[..., 1:]), 0.25) and (empty.table[..., 0] == 0).all()
    with pytest.raises(ValueError):
        CharNgramLM.from_transcripts([[1, 0, 2]], 4, order=2)   # a blank inside a transcript


def test_save_load_round_trip_is_exact(tmp_path):
    from policy_gradient_asr_amd.lm import CharNgramLM
    lm = CharNgramLM(R.random_table(7, 3, 2, seed=4), 3, blank=2)
    path = str(tmp_path / "lm.npz")
    lm.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["blank", "order", "table"]
    back = CharNgramLM.load(path)
    assert back.order == 3 and back.blank == 2 and back.vocab == 7
    assert back.table.dtype == np.float32 and np.array_equal(back.table, lm.table)


def test_over_cap_and_non_finite_tables_raise():
    from policy_gradient_asr_amd.lm import CharNgramLM
    with pytest.raises(ValueError):
        CharNgramLM.from_transcripts([[1, 2]], 29, order=6)            # 29**6 > 2**25
    with pytest.raises(ValueError):
        CharNgramLM.from_transcripts([[1, 2]], 64, order=5)
    with pytest.raises(ValueError):
        CharNgramLM(np.zeros((2,) * 26, dtype=np.float32), 26)          # 2**26 entries
    CharNgramLM.from_transcripts([[1, 2]], 29, order=1)                 # within the cap
    t = R.random_table(5, 2, 0, seed=1)
    for bad in (np.inf, -np.inf, np.nan):
        u = t.copy(); u[3, 2] = bad
        with pytest.raises(ValueError):
            CharNgramLM(u, 2)
    u = t.copy(); u[3, 0] = -np.inf                                     # the blank column is never read
    CharNgramLM(u, 2)
    with pytest.raises(ValueError):
        CharNgramLM(t, 3)                                               # shape is not (V,)*order
    with pytest.raises(ValueError):
        CharNgramLM(t, 0)


def test_helper_at_zero_weights_is_the_oracle(golden_dir):
    """alpha = beta = 0: x + 0.0 == x, so tokens and score are the oracle's, compared with ==."""
    z = np.load(os.path.join(golden_dir, "beam_inputs.npz"))
    done = 0
    for key in z.files:
        probs = z[key]
        if probs.ndim != 2:
            continue
        T, V = probs.shape
        for beam in (1, 5, 16) if T <= 100 else (5,):
            want, nll = decode_ref.prefix_beam_search(probs, beam_size=beam)
            for order in (1, 3):
                tab = R.random_table(V, order, 0, seed=order)
                got, score, gap = R.fused_prefix_beam_search(probs, tab, order, 0.0, 0.0, beam_size=beam)
                assert got == want and score == nll
            got, score, _ = R.fused_prefix_beam_search(probs, None, 0, 0.7, 0.3, beam_size=beam)
            assert got == want and score == nll
            done += 1
    assert done >= 3
    # and with weights the search does change on a case where the LM disagrees with the acoustics
    probs = np.full((6, 3), 0.0); probs[:, 0] = 0.2; probs[:, 1] = 0.41; probs[:, 2] = 0.39
    tab = np.array([0.0, np.log(0.02), np.log(0.98)], dtype=np.float32)
    assert R.fused_prefix_beam_search(probs, tab, 1, 0.0, 0.0, beam_size=8)[0] != R.fused_prefix_beam_search(probs, tab, 1, 1.0, 0.0, beam_size=8)[0]


def test_new_symbol_exported_and_bound_abi_stays_7(lib):
    from policy_gradient_asr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    name = "pgasr_ctc_beam_search_lm"
    assert hasattr(lib, name)
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
    old = re.search(r"\bpgasr_ctc_beam_search\s*\(([^)]*)\)", src)
    assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]) == old.group(1).count(",") + 1 + 4
    assert _lib.SIGNATURES[name][0] is ctypes.c_int
    assert _lib.SIGNATURES[name][1][-4:] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double]
    assert int(re.search(r"#define PGASR_ABI_VERSION (\d+)", src).group(1)) == 7 and lib.pgasr_abi_version() == 7


def _call(lib, V, table, order, alpha=0.5, beta=0.5, ws_bytes=0):
    p = 0x1000          # fake pointers: every call below must return before dereferencing or launching anything
    return lib.pgasr_ctc_beam_search_lm(p, 0, 64, 64, None, 10, 1, V, 5, 0, 0, p, p, p, None, ws_bytes, None,
                                        table, order, alpha, beta)


def test_argument_checks_need_no_device(lib):
    p = 0x2000
    assert _call(lib, 29, None, 1) == INVALID_ARG            # an order without a table
    assert _call(lib, 29, None, 3) == INVALID_ARG
    assert _call(lib, 29, p, -1) == INVALID_ARG and _call(lib, 29, None, -1) == INVALID_ARG
    assert _call(lib, 29, p, 0) == INVALID_ARG               # a table without an order
    assert _call(lib, 29, p, 2, alpha=float("nan")) == INVALID_ARG and _call(lib, 29, p, 2, beta=float("inf")) == INVALID_ARG
    assert _call(lib, 29, p, 6) == UNSUPPORTED               # 29**6 > 2**25
    assert _call(lib, 64, p, 5) == UNSUPPORTED
    assert _call(lib, 2, p, 26) == UNSUPPORTED and _call(lib, 2, p, 1000) == UNSUPPORTED
    # within the cap the call gets as far as the workspace check (still before any HIP call): 29**5, 64**4, 2**25 are admitted
    assert _call(lib, 29, p, 5) == WORKSPACE and _call(lib, 64, p, 4) == WORKSPACE and _call(lib, 2, p, 25) == WORKSPACE
    assert _call(lib, 29, None, 0) == WORKSPACE              # no table: the old entry point's path
    assert _call(lib, 65, p, 2) == UNSUPPORTED               # the search's own limits come first, as before


def test_host_layer_refuses_a_mismatched_lm():
    import torch
    from policy_gradient_asr_amd import hipops, _lib
    from policy_gradient_asr_amd.lm import CharNgramLM
    with pytest.raises(_lib.PgasrError):
        hipops.ctc_beam_search(torch.zeros(3, 1, 5), None, lm=CharNgramLM(R.random_table(5, 2, 0, 0), 2))    # CPU tensor
    from policy_gradient_asr_amd.CTCdecoder import _UNSET, CTCDecoder
    dec = CTCDecoder(list("abcd"), lm=CharNgramLM(R.random_table(5, 2, 0, 0), 2), lm_alpha=0.5, lm_beta=1.0)
    assert dec._lm_args(R, None, 2.0) == {"lm": R, "lm_alpha": 0.5, "lm_beta": 2.0}       # per-call overrides
    assert dec._lm_args(None, 0.0, None) == {"lm": None, "lm_alpha": 0.0, "lm_beta": 1.0}
    assert CTCDecoder(list("abcd"))._lm_args(_UNSET, None, None) == {"lm": None, "lm_alpha": 0.0, "lm_beta": 0.0}


def _fast_gaps(case):
    T, V, beam, order, blank, alpha, beta, seed = case
    lp, lens, tab = R.fast_case_inputs(case)
    out = []
    for b in range(R.FAST_B):
        n = int(lens[b])
        if n:
            out.append(R.fused_prefix_beam_search(logp=lp[:n, b].astype(np.float64), table=tab, order=order, alpha=alpha, beta=beta,
                                                  beam_size=beam, blank=blank)[2])
    return out


@pytest.mark.parametrize("case", R.FAST_CASES, ids=lambda c: "T%d-V%d-K%d-n%d-b%d-s%d" % (c[0], c[1], c[2], c[3], c[4], c[7]))
def test_margin_condition_of_the_fp32_cases(case):
    """Every case the fp32 device path is compared on token for token has, on every utterance, no ranking decision closer
    than 1e-4 log units -- roughly 10x the largest error of the fp32 kernels (~1e-7 relative on scores ~1e2)."""
    lp, lens, tab = R.fast_case_inputs(case)
    assert 0 in lens and 1 in lens and np.isfinite(lp).all() and np.isfinite(tab).all()
    gaps = _fast_gaps(case)
    assert gaps and min(gaps) >= R.GAP_MIN, gaps


def test_margin_condition_of_the_headline_utterances():
    T, B, V, beam, order, blank, alpha, beta, seed = R.HEADLINE
    lp, tab = R.headline_inputs()
    assert lp.shape == (T, B, V) and tab.shape == (V,) * order
    for b in R.HEADLINE_CHECK:
        gap = R.fused_prefix_beam_search(logp=lp[:R.HEADLINE_CUT, b].astype(np.float64), table=tab, order=order, alpha=alpha,
                                         beta=beta, beam_size=beam, blank=blank)[2]
        assert gap >= R.GAP_MIN, (b, gap)
