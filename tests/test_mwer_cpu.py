"""MWER training over N-best lists on a GPU-less host: the fp64 reference of tests/mwer_ref.py against itself (closed form against
torch autograd) and its identities, the new entry points' export, binding and refusals (all before any HIP call), and the host
layer's refusals and defaults."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mwer_ref as MR  # noqa: E402
import nbest_ref as NR  # noqa: E402
from oracle import ctc_ref  # noqa: E402

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


T, B, V, N = 12, 3, 5, 4


@pytest.fixture(scope="module")
def case():
    """T = 12, B = 3, V = 5, N = 4: random logits, ragged lengths, lists from the helper's search (raw prefixes)."""
    rng = np.random.default_rng(7)
    logits = rng.normal(size=(T, B, V)) * 1.5
    in_len, tg_len = np.array([12, 9, 6]), np.array([3, 2, 1])
    targets = np.zeros((B, 3), dtype=np.int64)
    for b in range(B):
        targets[b, :tg_len[b]] = rng.integers(1, V, size=tg_len[b])
    lp = ctc_ref.log_softmax(logits, axis=2)
    tokens, lengths, count = np.zeros((N, B, T), dtype=np.int64), np.zeros((N, B), dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        hyps, _ = NR.nbest_prefix_beam_search(logp=lp[:in_len[b], b], beam_size=8, nbest=N)
        count[b] = len(hyps)
        for n, (h, _) in enumerate(hyps):
            lengths[n, b] = len(h); tokens[n, b, :len(h)] = h
    assert (count == N).all()
    dist, risk_len = MR.risks(targets, tg_len, tokens, lengths)
    return dict(logits=logits, in_len=in_len, targets=targets, tg_len=tg_len, tokens=tokens, lengths=lengths, count=count,
                dist=dist, risk_len=risk_len)


def _both(c, Lh=T, lam=0.7, gb=B, **over):
    a = {**c, **over}
    args = (a["logits"], a["in_len"], a["targets"], a["tg_len"], a["tokens"], a["lengths"], a["count"], Lh, lam, gb, a["dist"], a["risk_len"])
    return MR.mwer_closed_form(*args), MR.mwer_autograd(*args)


def test_closed_form_equals_autograd(case):
    cf, (loss, grad) = _both(case)
    assert abs(cf.loss - loss) <= 1e-10 * abs(loss)
    assert np.abs(cf.grad - grad).max() <= 1e-10 * np.abs(grad).max()
    assert np.abs(cf.w.coef.sum(axis=0)).max() <= 1e-15                       # sum_n coef[n,b] = 0
    assert np.allclose(cf.w.p.sum(axis=0), 1.0, rtol=0, atol=1e-14) and cf.w.p.max() < 0.95 and (cf.w.coef > 0).any() and (cf.w.coef < 0).any()
    # the word risk goes through the same arithmetic
    dist, risk_len = MR.risks(case["targets"], case["tg_len"], case["tokens"], case["lengths"], delimiter=4)
    cf, (loss, grad) = _both(case, dist=dist, risk_len=risk_len)
    assert abs(cf.loss - loss) <= 1e-10 * abs(loss) and np.abs(cf.grad - grad).max() <= 1e-10 * np.abs(grad).max()


def test_one_entry_and_zero_weight_give_the_ctc_gradient(case):
    nll, g = ctc_ref.ctc_loss_and_grad(case["logits"], case["targets"], case["in_len"], case["tg_len"])
    want = g / (B * np.maximum(case["tg_len"], 1))[None, :, None]
    one = {k: case[k][:1] for k in ("tokens", "lengths", "dist")}
    cf, (loss, grad) = _both(case, count=np.ones(B, dtype=np.int64), **one)
    assert np.abs(cf.grad - want).max() <= 1e-14 * np.abs(want).max() and np.abs(grad - want).max() <= 1e-10 * np.abs(want).max()
    cf0, (loss0, grad0) = _both(case, lam=0.0)
    assert np.array_equal(cf0.grad, want) or np.abs(cf0.grad - want).max() <= 1e-15
    assert np.abs(grad0 - want).max() <= 1e-10 * np.abs(want).max()
    assert abs(cf0.loss - (nll / (B * np.maximum(case["tg_len"], 1))).sum()) <= 1e-14 * abs(cf0.loss)


def test_an_excluded_entry_renormalises_the_rest(case):
    """A cap below one entry's length: its posterior is 0, the others' is p / (1 - p_excluded); closed form == autograd still."""
    full, _ = _both(case)
    cap = int(case["lengths"].max()) - 1
    over = case["lengths"] > cap
    assert over.any() and not over.all(axis=0).any()
    cf, (loss, grad) = _both(case, Lh=cap)
    assert (cf.w.p[over] == 0).all() and (cf.w.coef[over] == 0).all()
    want = np.where(over, 0.0, full.w.p) / np.where(over, 0.0, full.w.p).sum(axis=0, keepdims=True)
    assert np.allclose(cf.w.p, want, rtol=1e-12, atol=0)
    assert abs(cf.loss - loss) <= 1e-10 * abs(loss) and np.abs(cf.grad - grad).max() <= 1e-10 * np.abs(grad).max()
    # rows beyond count and a non-finite nll are excluded the same way; no valid entry gives zeros
    w = MR.weights_ref(case["dist"], case["risk_len"], case["tg_len"], np.where(over, np.inf, full.hyp_nll), case["lengths"],
                       case["count"], full.nll, T, 0.7, 1.0 / B)
    assert np.allclose(w.p, want, rtol=1e-12, atol=0)
    w = MR.weights_ref(case["dist"], case["risk_len"], case["tg_len"], full.hyp_nll, case["lengths"], np.zeros(B, dtype=int),
                       full.nll, T, 0.7, 1.0 / B)
    assert not w.p.any() and not w.coef.any() and not w.rbar.any()


def test_new_symbols_exported_and_bound_abi_stays_7(lib):
    from policy_gradient_asr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in (("pgasr_mwer_weights", 19), ("pgasr_ctc_grad_from_lattices_nbest", 19)):
        assert hasattr(lib, name)
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m and m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]) == nargs
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    seq = re.search(r"\bpgasr_ctc_grad_from_lattices_seq\s*\(([^)]*)\)", src)
    assert len(_lib.SIGNATURES["pgasr_ctc_grad_from_lattices_nbest"][1]) == seq.group(1).count(",") + 1 - 1      # no path tensor
    assert int(re.search(r"#define PGASR_ABI_VERSION (\d+)", src).group(1)) == 7 and lib.pgasr_abi_version() == 7


P = 0x1000          # fake pointers: every call below must return before dereferencing or launching anything


def _weights(lib, N=4, B=2, Lh=10, lam=1.0, inv=0.5, **null):
    names = ("dist", "risk_len", "tg_len", "hyp_nll", "hyp_len", "count", "nll", "p", "r", "coef", "utt_scale", "rbar", "terms")
    a = {k: (None if null.get(k, 1) is None else P) for k in names}
    return lib.pgasr_mwer_weights(a["dist"], a["risk_len"], a["tg_len"], a["hyp_nll"], a["hyp_len"], a["count"], a["nll"], N, B, Lh,
                                  lam, inv, a["p"], a["r"], a["coef"], a["utt_scale"], a["rbar"], a["terms"], None)


def test_weights_refusals_need_no_device(lib):
    for name in ("dist", "risk_len", "tg_len", "hyp_nll", "hyp_len", "count", "nll", "p", "r", "coef", "utt_scale", "rbar", "terms"):
        assert _weights(lib, **{name: None}) == INVALID_ARG, name
    assert _weights(lib, N=0) == INVALID_ARG and _weights(lib, N=17) == INVALID_ARG and _weights(lib, B=0) == INVALID_ARG
    assert _weights(lib, Lh=-1) == INVALID_ARG
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert _weights(lib, lam=bad) == INVALID_ARG and _weights(lib, inv=bad) == INVALID_ARG
    assert _weights(lib, inv=0.0) == INVALID_ARG and _weights(lib, inv=-0.5) == INVALID_ARG


def _grad(lib, T=10, B=2, V=29, Lmax=4, blank=0, N=4, Lh=10, ws=None, ws_bytes=0, hws=None, hws_bytes=0, **null):
    names = ("lp", "in_len", "tg_len", "utt_scale", "coef", "hyp_len", "grad")
    a = {k: (None if null.get(k, 1) is None else P) for k in names}
    return lib.pgasr_ctc_grad_from_lattices_nbest(a["lp"], a["in_len"], a["tg_len"], T, B, V, Lmax, blank, a["utt_scale"], N, a["coef"],
                                                  a["hyp_len"], Lh, a["grad"], ws, ws_bytes, hws, hws_bytes, None)


def test_gradient_refusals_need_no_device(lib):
    for name in ("lp", "in_len", "tg_len", "coef", "hyp_len", "grad"):
        assert _grad(lib, **{name: None}) == INVALID_ARG, name
    assert _grad(lib, N=0) == INVALID_ARG and _grad(lib, N=17) == INVALID_ARG and _grad(lib, Lh=-1) == INVALID_ARG
    assert _grad(lib, T=0) == INVALID_ARG and _grad(lib, blank=29) == INVALID_ARG and _grad(lib, Lmax=-1) == INVALID_ARG
    assert _grad(lib, V=65) == UNSUPPORTED and _grad(lib, Lh=1024) == UNSUPPORTED and _grad(lib, Lmax=1024) == UNSUPPORTED
    # a well-formed request gets as far as the workspaces (still before any HIP call)
    assert _grad(lib) == WORKSPACE
    need = lib.pgasr_ctc_workspace_bytes(10, 2, 29, 4)
    assert _grad(lib, ws=P, ws_bytes=need - 1) == WORKSPACE and _grad(lib, ws=P, ws_bytes=need) == WORKSPACE
    hneed = lib.pgasr_ctc_hyp_workspace_bytes(10, 2, 29, 4, 10)
    assert hneed > 0 and _grad(lib, ws=P, ws_bytes=need, hws=P, hws_bytes=hneed - 1) == WORKSPACE


def _nbest(lib, flags, T=10, V=29, beam=5, nbest=3, stride=10, tokens=P, length=P, score=P, count=P, ws=None, ws_bytes=0,
           table=None, order=0, alpha=0.5, beta=0.5, lp=P, blank=0):
    return lib.pgasr_ctc_beam_search_nbest(lp, 0, 64, 64, None, T, 1, V, beam, blank, flags, nbest, tokens, stride, length, score, count,
                                           ws, ws_bytes, None, table, order, alpha, beta)


def test_the_fast_flag_refuses_what_the_call_refuses_without_it(lib):
    need = lib.pgasr_beam_workspace_bytes(10, 1, 29, 5)
    cases = [dict(nbest=0), dict(nbest=-1), dict(nbest=6), dict(stride=9), dict(tokens=None), dict(length=None), dict(score=None),
             dict(count=None), dict(lp=None), dict(T=0, stride=0), dict(blank=29), dict(V=65), dict(beam=129, nbest=1),
             dict(table=None, order=2), dict(table=P, order=0), dict(table=P, order=2, alpha=float("nan")), dict(table=P, order=6),
             dict(V=65, nbest=0), dict(), dict(nbest=5, stride=11), dict(nbest=1), dict(table=P, order=5),
             dict(ws=P, ws_bytes=need - 1), dict(ws=P, ws_bytes=need, nbest=0)]
    seen = set()
    for kw in cases:
        got = _nbest(lib, 8, **kw)
        assert got == _nbest(lib, 0, **kw) == _nbest(lib, 9, **kw) and got != 0, kw
        seen.add(got)
    assert seen == {INVALID_ARG, WORKSPACE, UNSUPPORTED}


def test_host_layer_refusals_and_defaults():
    from policy_gradient_asr_amd import _lib, hipops, model
    from policy_gradient_asr_amd.mwer import MWERTrainer, mwer_ctc_loss
    from policy_gradient_asr_amd.model import Seq2Seq
    lg, il = torch.zeros(6, 2, 5), torch.tensor([6, 5], dtype=torch.int32)
    tg, tl = torch.ones(2, 2, dtype=torch.int32), torch.tensor([2, 1], dtype=torch.int32)
    for kw in (dict(nbest=0), dict(nbest=5, beam=4), dict(nbest=17, beam=32), dict(nbest=2.5), dict(beam=True),
               dict(risk_unit="phone"), dict(risk_unit="word"), dict(risk_unit="word", word_delimiter=0),
               dict(risk_unit="word", word_delimiter=5), dict(max_hyp_len=-1), dict(max_hyp_len=2.0), dict(max_hyp_len=True)):
        with pytest.raises(ValueError):
            mwer_ctc_loss(lg, il, tg, tl, **kw)
    with pytest.raises(_lib.PgasrError):
        mwer_ctc_loss(lg, il, tg, tl)                                        # CPU tensors: there is no CPU path
    with pytest.raises(_lib.PgasrError):
        hipops.mwer_weights(torch.zeros(2, 2, dtype=torch.int32), tl, tl, torch.zeros(2, 2), torch.zeros(2, 2, dtype=torch.int32), tl,
                            torch.zeros(2), 4, 1.0, 0.5)
    sig = inspect.signature(mwer_ctc_loss)
    assert list(sig.parameters) == ["logits", "in_len", "targets", "tg_len", "lam", "beam", "nbest", "global_batch", "blank",
                                    "risk_unit", "word_delimiter", "max_hyp_len", "log_probs"]
    assert [sig.parameters[k].default for k in ("lam", "beam", "nbest", "global_batch", "blank", "risk_unit", "word_delimiter",
                                                "max_hyp_len", "log_probs")] == [1.0, 16, 4, None, 0, "char", None, None, None]
    assert inspect.signature(hipops.ctc_beam_search_nbest).parameters["fast"].default is False
    m = Seq2Seq(6, n_feats=8)
    for kw in (dict(num_samples=2), dict(reward_baseline="leave_one_out"), dict(score_function="sequence"), dict(reward_mode="per_step"),
               dict(reward_decoder="beam"), dict(entropy_weight=0.1), dict(nbest=0), dict(nbest=9, beam_size=8), dict(nbest=17, beam_size=32),
               dict(risk_unit="word"), dict(max_hyp_len=-3)):
        with pytest.raises(ValueError):
            MWERTrainer(m, **kw)
    with pytest.raises(TypeError):
        MWERTrainer(m, sample_temperature=2.0)
    sig = inspect.signature(MWERTrainer.__init__)
    assert [sig.parameters[k].default for k in ("beam_size", "nbest", "risk_unit", "word_delimiter", "max_hyp_len")] == [16, 4, "char", None, None]
    sig = inspect.signature(model.train)
    assert [sig.parameters[k].default for k in ("objective", "mwer_nbest", "mwer_beam")] == ["reinforce", 4, 16]
    with pytest.raises(ValueError):
        model.train("/nonexistent", "/nonexistent", 1, 2, 0, objective="mbr")
