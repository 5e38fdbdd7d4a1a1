"""The planted CTC cases of tests/ctc_cases.py and the fp64 oracle they are judged by, on the CPU: the oracle against torch's
fp64 ctc_loss + autograd on every case, the cases being what their table says they are, and the oracle's gradient at p = 0."""
import warnings

import numpy as np
import pytest
import torch

import ctc_cases as cc
from oracle import ctc_ref


@pytest.mark.parametrize("name", list(cc.CASES))
def test_oracle_equals_torch_fp64_on_every_case(name):
    c = cc.case(name)
    n64, g64 = c.torch64()
    assert np.abs(c.nll - n64).max() <= 1e-10 and np.abs(c.grad - g64).max() <= 1e-10


@pytest.mark.parametrize("name", list(cc.CASES))
def test_cases_are_what_the_table_says(name):
    c, kw = cc.case(name), cc.CASES[name]
    assert np.isfinite(c.nll).all() and np.isfinite(c.grad).all()
    assert c.logits.dtype == np.float32 and c.targets.dtype == c.il.dtype == c.tl.dtype == np.int32
    assert c.logits.shape == (kw["T"], kw["B"], kw["V"]) and c.targets.shape == (kw["B"], max(kw["L"], 1))
    real = [c.targets[b, :c.tl[b]] for b in range(kw["B"])]
    assert all((r != c.blank).all() and (r >= 0).all() and (r < kw["V"]).all() for r in real)
    if name in cc.ANTI:
        assert (c.nll > 100).all()
    if c.blank != 0:
        assert all((r == 0).any() for r in real)                      # symbol 0 is an ordinary label
    if kw.get("repeats"):
        assert all((r[1::2] == r[0:-1:2][:r[1::2].size]).all() for r in real)
    if kw.get("pad_garbage"):
        pads = np.concatenate([c.targets[b, c.tl[b]:] for b in range(kw["B"])])
        assert pads.size and set(pads.tolist()) <= {-1, kw["V"] + 5}
    if name == "sat8":
        assert sorted(int(t) % 4 for t in c.il) == [0, 1, 2, 3]
    if name == "min_T":
        assert (c.il == 2 * c.tl + 1).all()
    for n, S in (("S63", 63), ("S65", 65), ("S255", 255), ("S257", 257)):
        if name == n:
            assert (2 * c.tl + 1 == S).all()
    if name == "nspt4":
        assert 2 * kw["L"] + 1 > 2 * 256 and 2 * int(c.tl[1]) + 1 == 513
    if name == "nspt8":
        assert 2 * kw["L"] + 1 > 4 * 256 and 2 * int(c.tl[1]) + 1 == 1025


def test_planted_is_deterministic_and_leaves_the_shared_case_alone():
    kw = cc.CASES["blank_last"]
    a, b = cc.planted(seed=cc.SEED, **kw), cc.planted(seed=cc.SEED, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(a[0], cc.case("blank_last").logits)
    with pytest.raises(ValueError):
        cc.case("sat8").grad[0, 0, 0] = 1.0
    with pytest.raises(ValueError):
        cc.planted(T=2, B=1, V=4, L=2, seed=0, scale=1.0, repeats=True)      # a a needs the blank between: 3 frames


def test_oracle_gradient_at_zero_probability():
    """-inf logits: no NaN, exact zeros at the masked entries, and the same numbers as -1000 in their place -- from the oracle
    itself and from torch's fp64 autograd -- to 1e-12."""
    logits, targets, il, tl, masked = cc.masked_case()
    assert len({(b, v == 0, v in targets[b]) for _, b, v in masked}) == 3       # the blank, a target label, an outside symbol
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                          # and no RuntimeWarning on the way
        nll, grad = ctc_ref.ctc_loss_and_grad(logits, targets, il, tl)
    assert np.isfinite(nll).all() and np.isfinite(grad).all()
    for t, b, v in masked:
        assert grad[t, b, v] == 0.0
    finite = np.where(np.isneginf(logits), -1000.0, logits)
    nll_f, grad_f = ctc_ref.ctc_loss_and_grad(finite, targets, il, tl)
    n64, g64 = cc.torch_ctc(finite, targets, il, tl, 0, torch.float64)
    assert np.abs(nll - nll_f).max() <= 1e-12 and np.abs(grad - grad_f).max() <= 1e-12
    assert np.abs(nll - n64).max() <= 1e-12 and np.abs(grad - g64).max() <= 1e-12
    # the masks matter: the unmasked input has another nll
    plain = cc.planted(T=30, B=2, V=8, L=4, seed=3, scale=5.0)
    assert np.abs(ctc_ref.ctc_loss_and_grad(*plain)[0] - nll).min() > 1e-6


def test_oracle_impossible_label_is_the_infeasible_contract():
    logits, targets, il, tl = cc.impossible_label_case()
    nll, grad = ctc_ref.ctc_loss_and_grad(logits, targets, il, tl)
    assert np.isposinf(nll[0]) and np.isfinite(nll[1])
    assert (grad[:, 0] == 0).all() and np.isfinite(grad).all() and np.abs(grad[:, 1]).max() > 0


def test_oracle_finite_outputs_keep_their_bits():
    """The p = 0 definition is a select on the occupancy term: where the log-prob is finite the expression is the one it was."""
    c = cc.case("sat20")
    lp = ctc_ref.log_softmax(c.logits[:, 0].astype(np.float64), axis=1)
    tgt = c.targets[0, :c.tl[0]].astype(np.int64)
    alpha, beta, nll, ext = ctc_ref.ctc_alpha_beta(lp, tgt)
    occ = np.full(lp.shape, -np.inf)
    for s in range(len(ext)):
        occ[:, ext[s]] = ctc_ref._lse2(occ[:, ext[s]], (alpha + beta)[:, s])
    with np.errstate(over="ignore"):
        want = np.exp(lp) - np.exp(occ + nll - lp)
    assert np.array_equal(c.grad[:, 0], want) and c.nll[0] == nll
