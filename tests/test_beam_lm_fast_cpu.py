"""The single-wave LM-fused beam search on a GPU-less host: the dispatch predicate pgasr_beam_lm_single_wave_ok against its limit
table, the argument checks of the two entry points with flags bit 4 (the codes they return without it, before any HIP call), the ABI
version, the MWER options' language-model checks, and the margin conditions of the cases tests/test_beam_lm_fast_gpu.py compares
token for token."""
import ctypes
import dataclasses
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as R  # noqa: E402
import beam_lm_fast_ref as F  # noqa: E402

HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
INVALID_ARG, WORKSPACE, UNSUPPORTED = 1, 3, 4
FAST, FAST_LM = 8, 16


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def test_predicate_answers_the_limit_table(lib):
    """beam 16 / 17, V 64 / 65, T * beam 24576 / 24577, T 4096 / 4097, fp64, no table: one case just inside and one just outside
    every limit.  The symbol is exported, bound and declared; the Python wrapper gives the same answers."""
    from policy_gradient_asr_amd import _lib, hipops
    assert hasattr(lib, "pgasr_beam_lm_single_wave_ok")
    assert _lib.SIGNATURES["pgasr_beam_lm_single_wave_ok"] == (ctypes.c_int, [ctypes.c_int] * 5)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+pgasr_beam_lm_single_wave_ok\s*\(\s*int T,\s*int V,\s*int beam,\s*int is_f64,\s*int lm_order\s*\)", src)
    for args, want in F.PREDICATE_TABLE:
        assert lib.pgasr_beam_lm_single_wave_ok(*args) == want, args
        assert hipops.beam_lm_single_wave_ok(*args) is bool(want), args
    T, V, beam = 1000, 29, 16
    for (t, v, k) in ((T, V, beam + 1), (T, 65, beam), (1537, V, beam), (4097, V, 5)):
        assert lib.pgasr_beam_lm_single_wave_ok(t, v, k, 0, 3) == 0
    # every shared case with beam <= 16 is inside, the beam-100 case outside
    assert len(F.INSIDE) == 10 and len(F.OUTSIDE) == 1
    for T, V, beam, order, blank, alpha, beta, seed in F.INSIDE + [F.ORDER5_CASE]:
        assert lib.pgasr_beam_lm_single_wave_ok(T, V, beam, 0, order) == 1
    for T, V, beam, order, blank, alpha, beta, seed in F.OUTSIDE:
        assert lib.pgasr_beam_lm_single_wave_ok(T, V, beam, 0, order) == 0


def test_abi_version_stays_7(lib):
    src = open(HEADER).read()
    assert int(re.search(r"#define PGASR_ABI_VERSION (\d+)", src).group(1)) == 7 and lib.pgasr_abi_version() == 7
    assert "flags bit 4" in src and "flags bit 3" in src


def _one(lib, flags, V=29, table=0x2000, order=2, alpha=0.5, beta=0.5, beam=5):
    p = 0x1000          # fake pointers: every call below must return before dereferencing or launching anything
    return lib.pgasr_ctc_beam_search_lm(p, 0, 64, 64, None, 10, 1, V, beam, 0, flags, p, p, p, None, 0, None, table, order, alpha, beta)


def _list(lib, flags, V=29, table=0x2000, order=2, alpha=0.5, beta=0.5, beam=5, nbest=2):
    p = 0x1000
    return lib.pgasr_ctc_beam_search_nbest(p, 0, 64, 64, None, 10, 1, V, beam, 0, flags, nbest, p, 10, p, p, p, None, 0, None,
                                           table, order, alpha, beta)


@pytest.mark.parametrize("call", [_one, _list], ids=["lm", "nbest"])
def test_argument_checks_are_the_same_with_bit_4(lib, call):
    """Every refusal below is made before any HIP call (the pointers are fake and there is no device), and is the same code with
    and without flags bit 4, alone and beside the bits it can meet."""
    big = 2 ** 25 + 1
    assert 29 ** 5 < 2 ** 25 < 29 ** 6 < big ** 2
    seen = set()
    for kw, want in ((dict(table=None, order=2), INVALID_ARG),                   # an order without a table
                     (dict(order=0), INVALID_ARG),                               # a table without an order
                     (dict(alpha=float("nan")), INVALID_ARG),                    # non-finite weights
                     (dict(alpha=float("inf")), INVALID_ARG),
                     (dict(beta=float("-inf")), INVALID_ARG),
                     (dict(order=6), UNSUPPORTED),                               # 29^6 > 2^25 entries
                     (dict(V=64, order=5), UNSUPPORTED),
                     (dict(V=2, order=26), UNSUPPORTED),
                     (dict(V=65), UNSUPPORTED),                                  # the search's own limits
                     (dict(order=5), WORKSPACE),                                 # admitted: as far as the workspace check
                     (dict(), WORKSPACE),
                     (dict(table=None, order=0), WORKSPACE)):
        base = call(lib, 0, **kw)
        assert base == want, kw
        for flags in (FAST_LM, FAST_LM | 1, FAST_LM | 2, FAST_LM | FAST, FAST_LM | FAST | 1):
            assert call(lib, flags, **kw) == base, (kw, flags)
        seen.add(base)
    assert seen == {INVALID_ARG, WORKSPACE, UNSUPPORTED}


def test_nbest_over_beam_is_refused_with_bit_4(lib):
    for flags in (0, FAST, FAST_LM, FAST_LM | FAST):
        assert _list(lib, flags, beam=5, nbest=6) == INVALID_ARG
        assert _list(lib, flags, beam=16, nbest=17) == INVALID_ARG
        assert _list(lib, flags, beam=5, nbest=0) == INVALID_ARG
        assert _list(lib, flags, beam=5, nbest=5) == WORKSPACE


def test_host_layer_defaults():
    from policy_gradient_asr_amd import hipops, model, mwer
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    for fn in (hipops.ctc_beam_search, hipops.ctc_beam_search_nbest):
        assert inspect.signature(fn).parameters["fast_lm"].default is False
    assert inspect.signature(CTCDecoder.__init__).parameters["fast_lm"].default is False
    assert inspect.signature(CTCDecoder.decode_batch).parameters["fast_lm"].default is None
    assert "fast_lm" not in inspect.signature(CTCDecoder.decode).parameters          # the fp64 drop-in stays on the exact kernel
    assert CTCDecoder(list("ab")).fast_lm is False and CTCDecoder(list("ab"), fast_lm=True).fast_lm is True
    assert inspect.signature(model.predict).parameters["lm_fast"].default is False
    sig = inspect.signature(model.train)
    assert [sig.parameters[k].default for k in ("mwer_lm_path", "mwer_lm_alpha", "mwer_lm_beta")] == [None, 0.0, 0.0]
    for fn in (mwer.mwer_ctc_loss_lm, mwer.MWERTrainer.__init__):
        sig = inspect.signature(fn)
        assert [sig.parameters[k].default for k in ("lm", "lm_alpha", "lm_beta")] == [None, 0.0, 0.0]
    with pytest.raises(ValueError):
        model.train("/nonexistent", "/nonexistent", 1, 2, 0, mwer_lm_path="/nonexistent/lm.npz")      # belongs to objective="mwer"


def test_mwer_options_check_the_lm_before_any_kernel():
    """An LM of another vocabulary or blank raises ValueError (CPU tensors: nothing could have run); non-finite weights too; without
    an LM the options are exactly the ones of before."""
    import torch
    from policy_gradient_asr_amd import _lib
    from policy_gradient_asr_amd.lm import CharNgramLM
    from policy_gradient_asr_amd.model import Seq2Seq
    from policy_gradient_asr_amd.mwer import MWEROptions, MWERTrainer, check_mwer_options, mwer_ctc_loss_lm
    good = CharNgramLM(R.random_table(6, 2, 0, 1), 2)
    other_v = CharNgramLM(R.random_table(5, 2, 0, 1), 2)
    other_blank = CharNgramLM(R.random_table(6, 2, 3, 1), 2, blank=3)
    for lm in (other_v, other_blank):
        with pytest.raises(ValueError):
            check_mwer_options(MWEROptions(lm=lm), vocab=6)
    with pytest.raises(ValueError):
        check_mwer_options(MWEROptions(lm=good, blank=3), vocab=6)
    for kw in (dict(lm_alpha=float("nan")), dict(lm_beta=float("inf"))):
        with pytest.raises(ValueError):
            check_mwer_options(MWEROptions(lm=good, **kw), vocab=6)
    opt = check_mwer_options(MWEROptions(lm=good, lm_alpha=0.5, lm_beta=1.5), vocab=6)
    assert opt.lm is good and (opt.lm_alpha, opt.lm_beta) == (0.5, 1.5)
    assert check_mwer_options(MWEROptions(lm=good), vocab=None).lm is good            # vocabulary unknown: the blank is still checked
    # defaults: the options of before, field for field
    d = dataclasses.asdict(MWEROptions())
    assert (d.pop("lm"), d.pop("lm_alpha"), d.pop("lm_beta")) == (None, 0.0, 0.0)
    assert d == dict(lam=1.0, beam=16, nbest=4, global_batch=1, blank=0, risk_unit="char", word_delimiter=None, max_hyp_len=None)
    # the loss: refused by ValueError, before the device check that a call without an LM reaches
    lg, il = torch.zeros(6, 2, 6), torch.tensor([6, 5], dtype=torch.int32)
    tg, tl = torch.ones(2, 2, dtype=torch.int32), torch.tensor([2, 1], dtype=torch.int32)
    for lm in (other_v, other_blank):
        with pytest.raises(ValueError):
            mwer_ctc_loss_lm(lg, il, tg, tl, lm)
    with pytest.raises(_lib.PgasrError):
        mwer_ctc_loss_lm(lg, il, tg, tl, good)
    # the trainer
    m = Seq2Seq(6, n_feats=8)
    for lm in (other_v, other_blank):
        with pytest.raises(ValueError):
            MWERTrainer(m, lm=lm)
    plain = MWERTrainer(m, beam_size=8, nbest=3)
    assert plain.mwer_options == check_mwer_options(MWEROptions(beam=8, nbest=3), vocab=6) == MWEROptions(beam=8, nbest=3)
    assert plain.mwer_lm is None and MWERTrainer(m, lm=None, lm_alpha=0.7, lm_beta=0.2).mwer_options == MWEROptions()
    fused = MWERTrainer(m, lm=good, lm_alpha=0.7, lm_beta=0.2)
    assert fused.mwer_lm is good and (fused.mwer_lm_alpha, fused.mwer_lm_beta) == (0.7, 0.2)


def test_margin_condition_of_the_order_5_case():
    """Order 5 at V = 29 (29^5 entries, just under 2^25): every utterance's smallest ranking margin is >= GAP_MIN, so the fp32 device
    search must return the helper's tokens; lengths hold a 0 and a 1."""
    T, V, beam, order, blank, alpha, beta, seed = F.ORDER5_CASE
    lp, lens, table = F.order5_inputs()
    assert table.shape == (V,) * order and 2 ** 24 < table.size <= 2 ** 25 < table.size * V
    assert 0 in lens and 1 in lens and np.isfinite(lp).all()
    gaps = [g for (_, _, g) in F.order5_reference()]
    print("order-5 margins", gaps)
    assert min(gaps) >= R.GAP_MIN, gaps
    # the largest index the search can form is inside the table: ctx < V^(n-1), so ctx V + s < V^n
    assert (V ** (order - 1) - 1) * V + (V - 1) == table.size - 1


def test_the_mwer_case_lists_differ_with_the_lm():
    """The MWER case's alpha was chosen so that the fused search's list differs from the acoustic one on at least one utterance, by
    margins far above the fp32 kernels' error."""
    ac, lm = F.mwer_lists(False), F.mwer_lists(True)
    differs = [[h[0] for h in a[0]] != [h[0] for h in f[0]] for a, f in zip(ac, lm)]
    assert any(differs)
    assert min(min(a[1], f[1]) for a, f in zip(ac, lm)) >= R.GAP_MIN
