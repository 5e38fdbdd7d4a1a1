"""csrc/ctc.hip against the fp64 oracle where its design has to earn its keep (NOTES.md 0.14): saturated rows, rows whose
likely symbols are the wrong ones (the row maxima fall by tens of nats per frame), every states-per-thread instantiation and
the group boundaries of the storer, blank != 0, and exact zero probabilities through every gradient pass.

The bounds come from the project and from the arithmetic the kernel replaces, not from the kernel:
    nll   |err| <= max(1e-5 |nll| + 2e-7 T, 2 e32_nll)        README's f32 loss bound; the kernel header's 1e-7 per step
    grad  |err| <= max(5e-5, 2 e32_grad)                      README's f32 gradient bound (unscaled entries, in [-1, 1])
with e32 the error of torch's fp32 CPU ctc_loss + autograd on the same input against the same oracle (ctc_cases.Case)."""
import numpy as np
import pytest
import torch

import ctc_cases as cc
from oracle import ctc_ref, decode_ref, pg_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(*arrays):
    return tuple(torch.tensor(np.asarray(a)).to(DEV) for a in arrays)


def _bounds(nll_ref, T, e32_nll=0.0, e32_grad=0.0):
    return np.maximum(1e-5 * np.abs(nll_ref) + 2e-7 * T, 2 * e32_nll), max(5e-5, 2 * e32_grad)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_ctc_loss_grad_planted_vs_fp64(name):
    from policy_gradient_asr_amd import hipops
    c = cc.case(name)
    lp = torch.log_softmax(torch.tensor(c.logits), 2)                # fp32, on the CPU
    tg, il, tl = _dev(c.targets, c.il, c.tl)
    nll, grad = hipops.ctc_loss_grad(lp.to(DEV), tg, il, tl, blank=c.blank)
    nll, grad = nll.cpu().numpy().astype(np.float64), grad.cpu().numpy().astype(np.float64)
    err_nll, err_grad = np.abs(nll - c.nll), float(np.abs(grad - c.grad).max())
    b_nll, b_grad = _bounds(c.nll, c.T, c.e32_nll, c.e32_grad)
    print(f"[ctc numerics] {name}: nll {np.array2string(c.nll, precision=2)} err {err_nll.max():.2e} (bound {b_nll.min():.2e}, "
          f"e32 {c.e32_nll:.2e}); grad err {err_grad:.2e} (bound {b_grad:.2e}, e32 {c.e32_grad:.2e})")
    assert np.isfinite(nll).all() and np.isfinite(grad).all()
    assert (err_nll <= b_nll).all()
    assert err_grad <= b_grad
    if name in cc.ANTI:
        assert err_grad < c.e32_grad                                    # what the fp64 carries are for
        # ... and what the storer's reference is for.  With a reference at most 3 frames stale an fp32 offset carries 3
        # frames' fall of the row maximum per side, where fp32 log space carries all T = 120 frames' -- 6 / 120 of the
        # magnitude, and no accumulation.  A quarter of e32 leaves a factor 5 for what the two compositions of roundings
        # differ in; a reference refreshed every 64th frame carries 126 / 120 of the magnitude and fails this (NOTES.md 0.14).
        assert c.T == 120 and err_grad < c.e32_grad / 4
    for b in range(len(c.il)):
        assert (grad[int(c.il[b]):, b] == 0).all()


@pytest.mark.parametrize("name", ["sat40", "nspt4", "blank_last"])
def test_split_call_is_the_one_call_bit_for_bit(name):
    from policy_gradient_asr_amd import hipops
    c = cc.case(name)
    lp = torch.log_softmax(torch.tensor(c.logits), 2).to(DEV)
    tg, il, tl = _dev(c.targets, c.il, c.tl)
    B = len(c.il)
    us = torch.linspace(0.1, 0.5, B, device=DEV)
    nll1, g1 = hipops.ctc_loss_grad(lp, tg, il, tl, blank=c.blank, utt_scale=us)
    nll2, handle = hipops.ctc_lattice(lp, tg, il, tl, blank=c.blank)
    g2 = hipops.ctc_grad_from_lattice(lp, il, tl, handle, utt_scale=us)
    assert torch.equal(nll1, nll2) and torch.equal(g1, g2)
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0


# ---- exact zero probabilities (log p = -inf) ----
@pytest.fixture(scope="module")
def zeros():
    """The masked case on the device with its fp64 statement: nll and G = softmax - occupancy from the oracle (0 at p = 0)."""
    logits, targets, il, tl, masked = cc.masked_case()
    lp = torch.log_softmax(torch.tensor(logits), 2)
    assert all(lp[t, b, v] == -float("inf") for t, b, v in masked) and int(torch.isinf(lp).sum()) == len(masked)
    nll, G = ctc_ref.ctc_loss_and_grad(logits, targets, il, tl)
    assert np.isfinite(nll).all() and np.isfinite(G).all()
    T, B, V = logits.shape
    rng = np.random.default_rng(5)
    paths = rng.integers(0, V, size=(2, T, B)).astype(np.int32)
    for t, b, v in masked:                                               # a sampled path never takes a symbol of probability 0
        paths[:, t, b] = (v + 1) % V
    tg, ild, tld = _dev(targets, il, tl)
    return dict(logits=logits, lp=lp.to(DEV), lp64=ctc_ref.log_softmax(logits, axis=2), targets=targets, il=il, tl=tl, masked=masked,
                nll=nll, G=G, paths=paths, tg=tg, ild=ild, tld=tld, T=T, B=B, V=V,
                us=np.array([0.5, 0.3]), bounds=_bounds(nll, T))


def _check_zeros(z, label, grad, want):
    grad = grad.cpu().numpy().astype(np.float64)
    err = float(np.abs(grad - want).max())
    print(f"[ctc zeros] {label}: grad err {err:.2e} (bound {z['bounds'][1]:.2e})")
    assert np.isfinite(grad).all()
    assert err <= z["bounds"][1]
    for t, b, v in z["masked"]:
        assert grad[t, b, v] == 0.0
    assert np.abs(want).max() > 0.1                                      # the statement is not a vacuous one


def test_zero_probability_loss_grad(zeros):
    from policy_gradient_asr_amd import hipops
    z = zeros
    nll, grad = hipops.ctc_loss_grad(z["lp"], z["tg"], z["ild"], z["tld"])
    err = np.abs(nll.cpu().numpy().astype(np.float64) - z["nll"])
    print(f"[ctc zeros] nll {z['nll']} err {err.max():.2e} (bound {z['bounds'][0].min():.2e})")
    assert torch.isfinite(nll).all() and (err <= z["bounds"][0]).all()
    _check_zeros(z, "ctc_loss_grad", grad, z["G"])


def test_zero_probability_entropy_pass(zeros):
    """ctc_grad_from_lattice with ent_scale: us (softmax - occ) + ent_scale p (ln p + H), the entropy term 0 at p = 0."""
    from policy_gradient_asr_amd import hipops
    z = zeros
    ent = np.array([0.05, 0.02])
    us, ent_d = _dev(z["us"].astype(np.float32), ent.astype(np.float32))
    _, handle = hipops.ctc_lattice(z["lp"], z["tg"], z["ild"], z["tld"])
    grad = hipops.ctc_grad_from_lattice(z["lp"], z["ild"], z["tld"], handle, utt_scale=us, ent_scale=ent_d)
    want = z["G"] * z["us"][None, :, None] + pg_ref.entropy_grad(z["lp64"], z["il"], ent)
    _check_zeros(z, "ctc_grad_from_lattice_ent", grad, want)


def test_zero_probability_multi_pass(zeros):
    """ctc_grad_from_lattice_multi, K = 2: us (softmax - occ) + sum_k coef[k,b] (softmax - onehot(path_k))."""
    from policy_gradient_asr_amd import hipops
    z = zeros
    coef = np.array([[0.2, -0.1], [-0.15, 0.25]])
    us, coef_d, paths = _dev(z["us"].astype(np.float32), coef.astype(np.float32), z["paths"])
    _, handle = hipops.ctc_lattice(z["lp"], z["tg"], z["ild"], z["tld"])
    grad = hipops.ctc_grad_from_lattice_multi(z["lp"], z["ild"], z["tld"], handle, us, coef_d, paths)
    want = z["G"] * z["us"][None, :, None]
    for k in range(2):
        want = want + decode_ref.reinforce_grad(z["logits"], z["paths"][k], coef[k], z["il"])
    _check_zeros(z, "ctc_grad_from_lattice_multi", grad, want)


def test_zero_probability_seq_pass(zeros):
    """ctc_grad_from_lattices_seq with one hypothesis equal to the target and coefficient c: (us + c) (softmax - occ)."""
    from policy_gradient_asr_amd import hipops
    z = zeros
    c = np.array([[0.25, -0.2]])
    us, c_d, paths, hyp, hyp_len = _dev(z["us"].astype(np.float32), c.astype(np.float32), z["paths"][:1], z["targets"][None],
                                        z["tl"][None])
    Lh = z["targets"].shape[1]
    nll, handle = hipops.ctc_lattice(z["lp"], z["tg"], z["ild"], z["tld"])
    hyp_nll, hyp_handle = hipops.ctc_hyp_lattice(z["lp"], hyp, hyp_len, z["ild"], Lh)
    err = np.abs(hyp_nll[0].cpu().numpy().astype(np.float64) - z["nll"])
    assert (err <= z["bounds"][0]).all()                                 # the hypothesis is the target: the same nll
    grad = hipops.ctc_grad_from_lattices_seq(z["lp"], z["ild"], z["tld"], handle, hyp_handle, us, c_d, paths, hyp_len)
    want = z["G"] * (z["us"] + c[0])[None, :, None]
    _check_zeros(z, "ctc_grad_from_lattices_seq", grad, want)


def test_label_of_zero_probability_everywhere_is_the_infeasible_contract():
    """A target label at -inf on every frame: no alignment, nll = +inf and an all-zero gradient for that utterance -- the
    existing infeasible contract, reached through zeros; the other utterance is untouched by it."""
    from policy_gradient_asr_amd import hipops
    logits, targets, il, tl = cc.impossible_label_case()
    nll_ref, G = ctc_ref.ctc_loss_and_grad(logits, targets, il, tl)
    lp = torch.log_softmax(torch.tensor(logits), 2).to(DEV)
    nll, grad = hipops.ctc_loss_grad(lp, *_dev(targets, il, tl))
    nll, grad = nll.cpu().numpy().astype(np.float64), grad.cpu().numpy().astype(np.float64)
    assert np.isposinf(nll_ref[0]) and np.isposinf(nll[0])
    assert (grad[:, 0] == 0).all() and np.isfinite(grad).all()
    b_nll, b_grad = _bounds(nll_ref[1:], logits.shape[0])
    assert abs(nll[1] - nll_ref[1]) <= b_nll[0] and np.abs(grad[:, 1] - G[:, 1]).max() <= b_grad
