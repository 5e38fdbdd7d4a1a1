"""The KL penalty towards a frozen reference policy (kl_weight, ref_log_probs, kl_reference) on a GPU-less host: the new entry points
are exported and bound with the header's argument counts, the ABI stays 7, the C entries reject what they cannot take before touching
a pointer (exactly one of the two KL pointers included), the host layer checks the weight and the reference where the caller can read
the reason and takes the weight with every other option, and the fp64 statement the GPU tests are held to (tests/kl_ref.py) is the
derivative autograd takes."""
import ctypes
import os
import re

import numpy as np
import pytest

import kl_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
NEW = ("pgasr_frame_kl", "pgasr_ctc_grad_from_lattice_kl", "pgasr_ctc_grad_from_lattice_multi_kl",
       "pgasr_ctc_grad_from_lattices_seq_kl")
INVALID_ARG, WORKSPACE, UNSUPPORTED = 1, 3, 4
BAD_WEIGHTS = (-0.1, float("nan"), float("inf"), True, "0.5")
GOOD_WEIGHTS = (0, 0.0, 0.5)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def test_kl_symbols_exported_and_bound_abi_stays_7(lib):
    from policy_gradient_asr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int, name
    # a _kl entry is its _ent entry's argument list with ref_log_probs and kl_scale between ent_scale and grad_logits
    for name in NEW[1:]:
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[name[:-3] + "_ent"][1]) + 2, name
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert re.search(r"const float\*\s*ent_scale,\s*const float\*\s*ref_log_probs,\s*const float\*\s*kl_scale,\s*float\*\s*grad_logits",
                         args), name
    assert float(re.search(r"#define PGASR_KL_LOG_FLOOR \((-[\d.]+)f\)", src).group(1)) == kl_ref.LOG_FLOOR
    assert int(re.search(r"#define PGASR_ABI_VERSION (\d+)", src).group(1)) == 7
    assert lib.pgasr_abi_version() == 7


def test_kl_entries_reject_bad_arguments_without_a_device(lib):
    """The pointers below are fake: every call must return before dereferencing or launching anything."""
    p = 0x1000
    kl = lambda *a: lib.pgasr_frame_kl(*a)
    assert kl(p, p, p, 10, 2, 29, -0.5, 0.5, p, p, None) == INVALID_ARG
    assert kl(p, p, p, 10, 2, 29, float("nan"), 0.5, p, p, None) == INVALID_ARG
    assert kl(p, p, p, 10, 2, 29, 1.0, 0.0, p, p, None) == INVALID_ARG
    assert kl(p, p, p, 10, 2, 29, 1.0, -1.0, p, p, None) == INVALID_ARG
    assert kl(p, p, p, 0, 2, 29, 1.0, 0.5, p, p, None) == INVALID_ARG
    assert kl(None, p, p, 10, 2, 29, 1.0, 0.5, p, p, None) == INVALID_ARG
    assert kl(p, None, p, 10, 2, 29, 1.0, 0.5, p, p, None) == INVALID_ARG
    assert kl(p, p, None, 10, 2, 29, 1.0, 0.5, p, p, None) == INVALID_ARG
    assert kl(p, p, p, 10, 2, 29, 1.0, 0.5, None, p, None) == INVALID_ARG
    assert kl(p, p, p, 10, 2, 29, 1.0, 0.5, p, None, None) == INVALID_ARG
    assert kl(p, p, p, 10, 2, 65, 1.0, 0.5, p, p, None) == UNSUPPORTED
    big = 1 << 40
    # exactly one of ref_log_probs / kl_scale: refused, with and without ent_scale
    for es in (p, None):
        for ref, ks in ((p, None), (None, p)):
            assert lib.pgasr_ctc_grad_from_lattice_kl(p, p, p, 10, 2, 29, 3, 0, p, p, p, 0, es, ref, ks, p, p, big, None) == INVALID_ARG
            assert lib.pgasr_ctc_grad_from_lattice_multi_kl(p, p, p, 10, 2, 29, 3, 0, p, 4, p, p, es, ref, ks, p, p, big,
                                                            None) == INVALID_ARG
            assert lib.pgasr_ctc_grad_from_lattices_seq_kl(p, p, p, 10, 2, 29, 3, 0, p, 4, p, p, p, 5, es, ref, ks, p, p, big, p, big,
                                                           None) == INVALID_ARG
    # the gradient entries keep their parents' checks, with and without the KL pair and ent_scale
    for es in (p, None):
        for ref, ks in ((p, p), (None, None)):
            one = lambda *a: lib.pgasr_ctc_grad_from_lattice_kl(*a)
            assert one(p, p, p, 10, 2, 29, 3, 0, p, p, None, 0, es, ref, ks, p, p, big, None) == INVALID_ARG
            assert one(p, p, p, 10, 2, 29, 3, 0, p, p, p, 0, es, ref, ks, None, p, big, None) == INVALID_ARG
            assert one(p, p, p, 10, 2, 65, 3, 0, p, p, p, 0, es, ref, ks, p, p, big, None) == UNSUPPORTED
            assert one(p, p, p, 10, 2, 29, 3, 0, p, p, p, 0, es, ref, ks, p, p, 16, None) == WORKSPACE
            multi = lambda *a: lib.pgasr_ctc_grad_from_lattice_multi_kl(*a)
            assert multi(p, p, p, 10, 2, 29, 3, 0, p, 17, p, p, es, ref, ks, p, p, big, None) == INVALID_ARG
            assert multi(p, p, p, 10, 2, 29, 3, 0, p, 4, p, p, es, ref, ks, p, p, 16, None) == WORKSPACE
            seq = lambda *a: lib.pgasr_ctc_grad_from_lattices_seq_kl(*a)
            assert seq(p, p, p, 10, 2, 29, 3, 0, p, 0, p, p, p, 5, es, ref, ks, p, p, big, p, big, None) == INVALID_ARG
            assert seq(p, p, p, 10, 2, 29, 3, 0, p, 4, p, p, p, 1024, es, ref, ks, p, p, big, p, big, None) == UNSUPPORTED
            assert seq(p, p, p, 10, 2, 29, 3, 0, p, 4, p, p, p, 5, es, ref, ks, p, p, big, p, 16, None) == WORKSPACE


OTHER_OPTIONS = ({"per_step": True}, {"num_samples": 4}, {"num_samples": 4, "baseline": "leave_one_out"},
                 {"reward_unit": "word", "word_delimiter": 5}, {"score_function": "sequence"}, {"entropy_weight": 2.0})


def test_check_options_takes_the_weight_with_every_other_option():
    import dataclasses
    from policy_gradient_asr_amd.loss import PGOptions, check_kl_weight, check_options
    assert PGOptions().kl_weight == 0.0
    for bad in BAD_WEIGHTS + (None,):
        with pytest.raises(ValueError, match="kl_weight"):
            check_options(PGOptions(kl_weight=bad))
        with pytest.raises(ValueError, match="kl_weight"):
            check_kl_weight(bad)
    for good in GOOD_WEIGHTS + (np.float32(0.25), 3):
        for kw in ({},) + OTHER_OPTIONS:
            opt = check_options(PGOptions(kl_weight=good, **kw), vocab=29)
            assert isinstance(opt.kl_weight, float) and opt.kl_weight == float(good)
            assert dataclasses.replace(opt, kl_weight=0.0) == check_options(PGOptions(**kw), vocab=29)


def test_pg_ctc_loss_checks_weight_and_reference_before_any_kernel():
    """Every refusal below comes as a ValueError on CPU tensors: a kernel launch would fail differently."""
    import torch
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    z = torch.zeros(5, 2, 29)
    il = torch.full((2,), 5, dtype=torch.int32)
    tg = torch.ones(2, 2, dtype=torch.int32)
    tl = torch.full((2,), 2, dtype=torch.int32)
    ref = torch.log_softmax(torch.zeros(5, 2, 29), dim=2)
    for bad in BAD_WEIGHTS:
        for kw in ({},) + OTHER_OPTIONS:
            with pytest.raises(ValueError, match="kl_weight"):
                pg_ctc_loss(z, il, tg, tl, kl_weight=bad, ref_log_probs=ref, **kw)
    for kw in ({},) + OTHER_OPTIONS:
        with pytest.raises(ValueError, match="ref_log_probs"):
            pg_ctc_loss(z, il, tg, tl, kl_weight=0.5, **kw)                      # weight > 0 needs the reference
    wrong = {"dtype": ref.double(), "shape": ref[:4].contiguous(), "contiguous": ref.transpose(0, 1).contiguous().transpose(0, 1),
             "detached": ref.clone().requires_grad_(True), "tensor": ref.numpy()}
    assert not wrong["contiguous"].is_contiguous() and wrong["contiguous"].shape == ref.shape
    for what, bad_ref in wrong.items():
        with pytest.raises(ValueError, match="ref_log_probs"):
            pg_ctc_loss(z, il, tg, tl, kl_weight=0.5, ref_log_probs=bad_ref)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="device"):
            pg_ctc_loss(z.cuda(), il.cuda(), tg.cuda(), tl.cuda(), kl_weight=0.5, ref_log_probs=ref)


class _Tiny:
    """The smallest thing the trainer's constructor takes as a model and as a reference: a head and a ``logits`` method."""

    @staticmethod
    def make(vocab=3):
        import torch

        class Tiny(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.head = torch.nn.Linear(4, vocab)

            def logits(self, x, fmask, lengths=None):
                return self.head(x), lengths

        return Tiny()


def test_trainer_checks_weight_and_reference_and_takes_them_with_every_mode():
    import torch
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    m = _Tiny.make()
    for bad in BAD_WEIGHTS:
        with pytest.raises(ValueError, match="kl_weight"):
            PolicyGradientTrainer(m, kl_weight=bad, kl_reference="initial")
    tr = PolicyGradientTrainer(m)
    assert tr.kl_weight == 0.0 and tr.kl_reference is None and tr.last_kl is None
    with pytest.raises(ValueError, match="kl_reference"):
        PolicyGradientTrainer(m, kl_weight=0.5)                                 # weight > 0 needs a reference
    for w in (0.0, 0.5):
        with pytest.raises(ValueError, match="trained model itself"):
            PolicyGradientTrainer(m, kl_weight=w, kl_reference=m)
    with pytest.raises(ValueError, match="kl_reference"):
        PolicyGradientTrainer(m, kl_weight=0.5, kl_reference="pretrained")
    with pytest.raises(ValueError, match="kl_reference"):
        PolicyGradientTrainer(m, kl_weight=0.5, kl_reference=torch.nn.Linear(4, 3))     # no logits()
    with pytest.raises(ValueError, match="alphabet"):
        PolicyGradientTrainer(m, kl_weight=0.5, kl_reference=_Tiny.make(vocab=5))
    shared = _Tiny.make()
    shared.head.weight = m.head.weight
    with pytest.raises(ValueError, match="shares parameter storage"):
        PolicyGradientTrainer(m, kl_weight=0.5, kl_reference=shared)
    modes = ({"reward_mode": "per_step"}, {"num_samples": 4}, {"num_samples": 4, "reward_baseline": "leave_one_out"},
             {"reward_unit": "word", "word_delimiter": 2}, {"score_function": "sequence"}, {"entropy_weight": 2.0})
    for good in GOOD_WEIGHTS:
        for kw in ({},) + modes:
            for ref in ("initial", _Tiny.make().train()):
                tr = PolicyGradientTrainer(m, kl_weight=good, kl_reference=ref, **kw)
                assert tr.kl_weight == float(good) and isinstance(tr.kl_weight, float) and tr.last_kl is None
                r = tr.kl_reference
                assert r is not m and not r.training and all(not p.requires_grad and p.grad is None for p in r.parameters())
                own = {p.untyped_storage().data_ptr() for p in m.parameters()}
                assert not any(p.untyped_storage().data_ptr() in own for p in r.parameters())
                # the reference's parameters are not in the flat buffers the optimizer steps
                assert tr.gflat.numel() == tr.flat.numel() == PolicyGradientTrainer(m).flat.numel()
    init = PolicyGradientTrainer(m, kl_weight=0.5, kl_reference="initial").kl_reference
    assert all(torch.equal(a, b) for a, b in zip(init.parameters(), m.parameters()))          # "initial": the model as it stands
    x, t = torch.zeros(2, 4, 5), torch.zeros(2, 3, dtype=torch.long)
    tr.kl_weight = -1.0               # a setting changed after construction is caught where the step checks its limits
    with pytest.raises(ValueError, match="kl_weight"):
        tr._check_limits(x, t)
    tr = PolicyGradientTrainer(m)
    tr.kl_weight = 0.5                # .. and so is a weight switched on without a reference
    with pytest.raises(ValueError, match="kl_reference"):
        tr._check_limits(x, t)


def test_train_driver_wants_a_reference_path_with_the_weight(tmp_path):
    from policy_gradient_asr_amd.model import train
    with pytest.raises(ValueError, match="kl_reference_path or init_from"):
        train(str(tmp_path), str(tmp_path / "run"), 1, 16, 0, kl_weight=0.5)
    with pytest.raises(ValueError, match="kl_weight"):
        train(str(tmp_path), str(tmp_path / "run"), 1, 16, 0, kl_weight=-1.0, init_from="x.pth")


def test_the_fp64_statement_is_the_derivative_autograd_takes():
    """kl_ref against torch autograd in fp64 on ragged lengths (0 and T included): a policy row with two -inf entries, a one-hot policy
    row, a reference entry of -inf where p > 0 (the floor); value, gradient, zero rows beyond T_b, rows that sum to 0, q = p exactly 0."""
    import torch
    T, B, V, gamma, inv_gb = 9, 4, 6, 2.0, 0.25
    g = torch.Generator().manual_seed(0)
    z = torch.randn(T, B, V, generator=g, dtype=torch.float64) * 2
    z[1, 0, 4:] = -float("inf")
    z[2, 2, 1:] = -float("inf")
    zq = torch.randn(T, B, V, generator=g, dtype=torch.float64) * 2
    zq[3, 0, 1] = -float("inf")                                   # q = 0 under a live policy row: the floor
    zq[1, 0, 5] = -float("inf")                                   # q = 0 where p = 0 too: adds exactly 0
    lq = torch.log_softmax(zq, 2)
    in_len = np.array([9, 0, 5, 1])
    zz = z.clone().requires_grad_(True)
    lp = torch.log_softmax(zz, 2)
    p = lp.exp()
    lqf = torch.clamp(lq, min=kl_ref.LOG_FLOOR)
    d = torch.where(p > 0, p * (torch.where(p > 0, lp, torch.zeros_like(lp)) - lqf), torch.zeros_like(lp))
    KL = d.sum(2)
    mask = torch.from_numpy(np.arange(T)[:, None] < in_len[None, :])
    n = torch.from_numpy(np.maximum(in_len, 1).astype(np.float64))
    term = (gamma * inv_gb * ((KL * mask).sum(0) / n)).sum()
    term.backward()
    lpn, lqn = lp.detach().numpy(), lq.numpy()
    mean, scale = kl_ref.kl_stats(lpn, lqn, in_len, gamma, inv_gb)
    np.testing.assert_allclose(mean, ((KL * mask).sum(0) / n).detach().numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(scale, gamma * inv_gb / np.maximum(in_len, 1), rtol=1e-15)
    assert mean[1] == 0.0 and np.isfinite(mean).all()
    rk = kl_ref.row_kl(lpn, lqn)
    floored, milder = lqn.copy(), lqn.copy()
    floored[3, 0, 1], milder[3, 0, 1] = kl_ref.LOG_FLOOR, -50.0
    assert np.isfinite(rk).all() and np.array_equal(rk, kl_ref.row_kl(lpn, floored))             # -inf reads as the floor ..
    assert rk[3, 0] > kl_ref.row_kl(lpn, milder)[3, 0] + 50.0 * float(p[3, 0, 1].detach())              # .. a large, finite penalty
    assert abs(kl_ref.kl_loss(lpn, lqn, in_len, gamma, inv_gb) - float(term.detach())) <= 1e-12 * abs(float(term.detach()))
    want = kl_ref.kl_grad(lpn, lqn, in_len, scale)
    got = torch.nan_to_num(zz.grad, nan=0.0).numpy()              # autograd leaves nan at the -inf logits themselves
    finite = np.isfinite(z.numpy())
    np.testing.assert_allclose(want[finite], got[finite], rtol=1e-12, atol=1e-15)
    assert np.isfinite(want).all() and (want[~finite] == 0).all()
    assert (want[2, 2] == 0).all()                                # the one-hot policy row: p (ln p - lnq - KL) = 1 * (KL - KL)
    assert (want[~mask.numpy()] == 0).all() and np.abs(want).max() > 1e-3
    assert np.abs(want.sum(axis=2)).max() < 1e-13 * np.abs(want).max() + 1e-15
    # q = p: value and gradient exactly 0
    assert (kl_ref.row_kl(lpn, lpn) == 0).all() and (kl_ref.kl_stats(lpn, lpn, in_len, gamma, inv_gb)[0] == 0).all()
    assert kl_ref.kl_loss(lpn, lpn, in_len, gamma, inv_gb) == 0.0
    assert (kl_ref.kl_grad(lpn, lpn, in_len, scale) == 0).all()
