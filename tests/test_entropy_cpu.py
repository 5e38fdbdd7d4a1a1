"""Entropy regularisation of the frame policy (entropy_weight) on a GPU-less host: the new entry points are exported and bound with
the header's argument counts, the ABI stays 7, the C entries reject what they cannot take before touching a pointer, the host layer
checks the weight where the caller can read the reason and takes it with every other option, and the fp64 statement the GPU tests
are held to (oracle/pg_ref.py) is the derivative autograd takes."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import pg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
NEW = ("pgasr_frame_entropy", "pgasr_ctc_grad_from_lattice_ent", "pgasr_ctc_grad_from_lattice_multi_ent",
       "pgasr_ctc_grad_from_lattices_seq_ent")
INVALID_ARG, WORKSPACE, UNSUPPORTED = 1, 3, 4
BAD_WEIGHTS = (-0.1, float("nan"), float("inf"), True)
GOOD_WEIGHTS = (0, 0.0, 0.5)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def test_entropy_symbols_exported_and_bound_abi_stays_7(lib):
    from policy_gradient_asr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int, name
    # an _ent entry is its parent's argument list with ent_scale before grad_logits
    for name in NEW[1:]:
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[name[:-4]][1]) + 1, name
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert re.search(r"const float\*\s*ent_scale,\s*float\*\s*grad_logits", args), name
    assert int(re.search(r"#define PGASR_ABI_VERSION (\d+)", src).group(1)) == 7
    assert lib.pgasr_abi_version() == 7


def test_entropy_entries_reject_bad_arguments_without_a_device(lib):
    """The pointers below are fake: every call must return before dereferencing or launching anything."""
    p = 0x1000
    ent = lambda *a: lib.pgasr_frame_entropy(*a)
    assert ent(p, p, 10, 2, 29, -0.5, 0.5, p, p, None) == INVALID_ARG
    assert ent(p, p, 10, 2, 29, float("nan"), 0.5, p, p, None) == INVALID_ARG
    assert ent(p, p, 10, 2, 29, 1.0, 0.0, p, p, None) == INVALID_ARG
    assert ent(p, p, 0, 2, 29, 1.0, 0.5, p, p, None) == INVALID_ARG
    assert ent(None, p, 10, 2, 29, 1.0, 0.5, p, p, None) == INVALID_ARG
    assert ent(p, p, 10, 2, 29, 1.0, 0.5, None, p, None) == INVALID_ARG
    assert ent(p, p, 10, 2, 29, 1.0, 0.5, p, None, None) == INVALID_ARG
    assert ent(p, p, 10, 2, 65, 1.0, 0.5, p, p, None) == UNSUPPORTED
    # the gradient entries keep their parents' checks, with and without ent_scale
    for es in (p, None):
        assert lib.pgasr_ctc_grad_from_lattice_ent(p, p, p, 10, 2, 29, 3, 0, p, p, None, 0, es, p, p, 1 << 40, None) == INVALID_ARG
        assert lib.pgasr_ctc_grad_from_lattice_ent(p, p, p, 10, 2, 65, 3, 0, p, p, p, 0, es, p, p, 1 << 40, None) == UNSUPPORTED
        assert lib.pgasr_ctc_grad_from_lattice_ent(p, p, p, 10, 2, 29, 3, 0, p, p, p, 0, es, p, p, 16, None) == WORKSPACE
        assert lib.pgasr_ctc_grad_from_lattice_multi_ent(p, p, p, 10, 2, 29, 3, 0, p, 17, p, p, es, p, p, 1 << 40, None) == INVALID_ARG
        assert lib.pgasr_ctc_grad_from_lattice_multi_ent(p, p, p, 10, 2, 29, 3, 0, p, 4, p, p, es, p, p, 16, None) == WORKSPACE
        assert lib.pgasr_ctc_grad_from_lattices_seq_ent(p, p, p, 10, 2, 29, 3, 0, p, 0, p, p, p, 5, es, p, p, 1 << 40, p, 1 << 40,
                                                        None) == INVALID_ARG
        assert lib.pgasr_ctc_grad_from_lattices_seq_ent(p, p, p, 10, 2, 29, 3, 0, p, 4, p, p, p, 1024, es, p, p, 1 << 40, p, 1 << 40,
                                                        None) == UNSUPPORTED
        assert lib.pgasr_ctc_grad_from_lattices_seq_ent(p, p, p, 10, 2, 29, 3, 0, p, 4, p, p, p, 5, es, p, p, 1 << 40, p, 16,
                                                        None) == WORKSPACE


OTHER_OPTIONS = ({"per_step": True}, {"num_samples": 4}, {"num_samples": 4, "baseline": "leave_one_out"},
                 {"reward_unit": "word", "word_delimiter": 5}, {"score_function": "sequence"})


def test_check_options_takes_the_weight_with_every_other_option():
    import dataclasses
    from policy_gradient_asr_amd.loss import PGOptions, check_options
    assert PGOptions().entropy_weight == 0.0
    for bad in BAD_WEIGHTS + ("0.5", None):
        with pytest.raises(ValueError, match="entropy_weight"):
            check_options(PGOptions(entropy_weight=bad))
    for good in GOOD_WEIGHTS + (np.float32(0.25), 3):
        for kw in ({},) + OTHER_OPTIONS:
            opt = check_options(PGOptions(entropy_weight=good, **kw), vocab=29)
            assert isinstance(opt.entropy_weight, float) and opt.entropy_weight == float(good)
            assert dataclasses.replace(opt, entropy_weight=0.0) == check_options(PGOptions(**kw), vocab=29)


def test_pg_ctc_loss_checks_the_weight_before_any_kernel():
    import torch
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    z = torch.zeros(5, 2, 29)
    il = torch.full((2,), 5, dtype=torch.int32)
    tg = torch.ones(2, 2, dtype=torch.int32)
    tl = torch.full((2,), 2, dtype=torch.int32)
    for bad in BAD_WEIGHTS:
        with pytest.raises(ValueError, match="entropy_weight"):
            pg_ctc_loss(z, il, tg, tl, entropy_weight=bad)
        for kw in OTHER_OPTIONS:
            with pytest.raises(ValueError, match="entropy_weight"):
                pg_ctc_loss(z, il, tg, tl, entropy_weight=bad, **kw)


def test_trainer_checks_the_weight_and_takes_it_with_every_mode():
    import torch
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    m = torch.nn.Linear(4, 3)
    for bad in BAD_WEIGHTS:
        with pytest.raises(ValueError, match="entropy_weight"):
            PolicyGradientTrainer(m, entropy_weight=bad)
    assert PolicyGradientTrainer(m).entropy_weight == 0.0
    modes = ({"reward_mode": "per_step"}, {"num_samples": 4}, {"num_samples": 4, "reward_baseline": "leave_one_out"},
             {"reward_unit": "word", "word_delimiter": 2}, {"score_function": "sequence"})
    for good in GOOD_WEIGHTS:
        for kw in ({},) + modes:
            tr = PolicyGradientTrainer(m, entropy_weight=good, **kw)
            assert tr.entropy_weight == float(good) and isinstance(tr.entropy_weight, float) and tr.last_entropy is None
    tr.entropy_weight = -1.0          # a setting changed after construction is caught where the step checks its limits
    with pytest.raises(ValueError, match="entropy_weight"):
        tr._check_limits(torch.zeros(2, 4, 5), torch.zeros(2, 3, dtype=torch.long))


def test_the_fp64_statement_is_the_derivative_autograd_takes():
    """pg_ref's entropy term against torch autograd in fp64 on ragged lengths (0 and T included), a row with two -inf entries and a one-hot
    row: value, gradient, zero rows beyond T_b, rows that sum to 0."""
    import torch
    T, B, V, beta, inv_gb = 9, 4, 6, 2.0, 0.25
    g = torch.Generator().manual_seed(0)
    z = torch.randn(T, B, V, generator=g, dtype=torch.float64) * 2
    z[1, 0, 4:] = -float("inf")
    z[2, 2, 1:] = -float("inf")
    in_len = np.array([9, 0, 5, 1])
    zz = z.clone().requires_grad_(True)
    lp = torch.log_softmax(zz, 2)
    p = lp.exp()
    H = -torch.where(p > 0, p * torch.where(p > 0, lp, torch.zeros_like(lp)), torch.zeros_like(lp)).sum(2)
    mask = torch.from_numpy(np.arange(T)[:, None] < in_len[None, :])
    n = torch.from_numpy(np.maximum(in_len, 1).astype(np.float64))
    term = -(beta * inv_gb * ((H * mask).sum(0) / n)).sum()
    term.backward()
    lpn = lp.detach().numpy()
    mean, scale = pg_ref.entropy_stats(lpn, in_len, beta, inv_gb)
    np.testing.assert_allclose(mean, ((H * mask).sum(0) / n).detach().numpy(), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(scale, beta * inv_gb / np.maximum(in_len, 1), rtol=1e-15)
    assert mean[1] == 0.0 and pg_ref.row_entropy(lpn)[2, 2] == 0.0
    assert abs(pg_ref.entropy_loss(lpn, in_len, beta, inv_gb) - float(term.detach())) < 1e-14
    want = pg_ref.entropy_grad(lpn, in_len, scale)
    got = torch.nan_to_num(zz.grad, nan=0.0).numpy()          # autograd leaves nan at the -inf logits themselves
    finite = np.isfinite(z.numpy())
    np.testing.assert_allclose(want[finite], got[finite], rtol=1e-12, atol=1e-15)
    assert np.isfinite(want).all() and (want[~finite] == 0).all() and (want[2, 2] == 0).all()
    assert (want[~mask.numpy()] == 0).all() and np.abs(want).max() > 1e-3
    assert np.abs(want.sum(axis=2)).max() < 1e-15
    # uniform rows: H = ln V, no gradient
    u = np.full((3, 2, 5), -np.log(5.0))
    np.testing.assert_allclose(pg_ref.row_entropy(u), np.log(5.0), rtol=1e-15)
    assert np.abs(pg_ref.entropy_grad(u, [3, 3], [1.0, 1.0])).max() < 1e-15
