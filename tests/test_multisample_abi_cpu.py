"""The multi-sample REINFORCE entry points on a GPU-less host: exported, bound with the header's argument counts, and
rejecting an invalid sample count or baseline before any device work (no compute calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
NEW = ("pgasr_frame_sample_multi", "pgasr_ctc_grad_from_lattice_multi", "pgasr_pg_rewards_multi", "pgasr_pg_loss_value_multi")
INVALID_ARG = 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_multi_sample_symbols_exported_and_bound(lib):
    from policy_gradient_asr_amd import _lib
    src = _header()
    for name in NEW:
        assert hasattr(lib, name), name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int


def test_multi_sample_limits_agree():
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    src = open(HEADER).read()
    assert int(re.search(r"#define PGASR_MAX_SAMPLES (\d+)", src).group(1)) == hipops.MAX_SAMPLES == PolicyGradientTrainer.MAX_SAMPLES
    assert int(re.search(r"#define PGASR_BASELINE_HYPOTHESIS (\d+)", src).group(1)) == hipops.BASELINES["hypothesis"]
    assert int(re.search(r"#define PGASR_BASELINE_LEAVE_ONE_OUT (\d+)", src).group(1)) == hipops.BASELINES["leave_one_out"]


def test_invalid_sample_counts_are_rejected_without_a_device(lib):
    """K < 1, K > 16 and leave-one-out with K = 1 return PGASR_ERR_INVALID_ARG before anything is launched (the pointers below
    are never dereferenced)."""
    p = 0x1000
    for K in (0, 17):
        assert lib.pgasr_frame_sample_multi(p, 10, 2, 29, K, 0, 0, 0, 0, None, p, None) == INVALID_ARG
        assert lib.pgasr_ctc_grad_from_lattice_multi(p, p, p, 10, 2, 29, 3, 0, p, K, p, p, p, p, 1 << 20, None) == INVALID_ARG
        assert lib.pgasr_pg_rewards_multi(p, p, 2, K, 0, 1.0, 0.5, p, p, p, p, None) == INVALID_ARG
        assert lib.pgasr_pg_loss_value_multi(p, p, K, p, p, p, p, 10, 2, 29, p, None) == INVALID_ARG
    assert lib.pgasr_pg_rewards_multi(p, p, 2, 1, 1, 1.0, 0.5, p, p, p, p, None) == INVALID_ARG      # leave one out, K = 1
    assert lib.pgasr_pg_rewards_multi(p, p, 2, 4, 2, 1.0, 0.5, p, p, p, p, None) == INVALID_ARG      # unknown baseline


def test_loss_argument_checks_need_no_device():
    """pg_ctc_loss's multi-sample arguments are checked before any kernel runs."""
    import torch
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    z = torch.zeros(5, 2, 29)
    il = torch.full((2,), 5, dtype=torch.int32)
    tg = torch.ones(2, 2, dtype=torch.int32)
    tl = torch.full((2,), 2, dtype=torch.int32)
    for kw in ({"num_samples": 17}, {"num_samples": 0}, {"num_samples": 1, "baseline": "leave_one_out"},
               {"num_samples": 4, "per_step": True}, {"num_samples": 4, "baseline": "batch_mean"}):
        with pytest.raises(ValueError):
            pg_ctc_loss(z, il, tg, tl, **kw)
