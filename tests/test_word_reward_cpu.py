"""The word-level (WER) reward on a GPU-less host: the new entry points are exported and bound with the header's argument counts,
the ABI version is unchanged, invalid arguments are rejected before any device work, and pg_ctc_loss checks its word arguments
before any kernel runs."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
NEW = ("pgasr_word_ids", "pgasr_pg_rewards_multi_ex")
INVALID_ARG, UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_word_reward_symbols_exported_and_bound(lib):
    from policy_gradient_asr_amd import _lib
    src = _header()
    for name in NEW:
        assert hasattr(lib, name), name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int


def test_abi_version_is_still_7(lib):
    assert int(re.search(r"#define PGASR_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == 7
    assert lib.pgasr_abi_version() == 7


def test_word_stride_limit_agrees():
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    lim = int(re.search(r"#define PGASR_WORD_MAX_STRIDE (\d+)", open(HEADER).read()).group(1))
    assert lim == 4094 == hipops.WORD_MAX_STRIDE == PolicyGradientTrainer.MAX_WORD_FRAMES


def test_word_ids_invalid_arguments_need_no_device(lib):
    """A negative delimiter and N <= 0 give INVALID_ARG, a stride above 4094 UNSUPPORTED, before anything is launched (the
    pointers below are never dereferenced)."""
    p = 0x1000
    assert lib.pgasr_word_ids(p, p, 10, p, p, 20, 4, -1, p, p, p, p, None) == INVALID_ARG
    assert lib.pgasr_word_ids(p, p, 10, p, p, 20, 0, 5, p, p, p, p, None) == INVALID_ARG
    assert lib.pgasr_word_ids(p, p, 10, p, p, 20, -3, 5, p, p, p, p, None) == INVALID_ARG
    assert lib.pgasr_word_ids(p, p, 4095, p, p, 20, 4, 5, p, p, p, p, None) == UNSUPPORTED
    assert lib.pgasr_word_ids(p, p, 10, p, p, 4095, 4, 5, p, p, p, p, None) == UNSUPPORTED
    # the multi-sample checks of pgasr_pg_rewards_multi hold for the variant with a separate normaliser
    for K in (0, 17):
        assert lib.pgasr_pg_rewards_multi_ex(p, p, p, 2, K, 0, 1.0, 0.5, p, p, p, p, None) == INVALID_ARG
    assert lib.pgasr_pg_rewards_multi_ex(p, p, p, 2, 1, 1, 1.0, 0.5, p, p, p, p, None) == INVALID_ARG
    assert lib.pgasr_pg_rewards_multi_ex(p, p, p, 2, 4, 2, 1.0, 0.5, p, p, p, p, None) == INVALID_ARG
    assert lib.pgasr_pg_rewards_multi_ex(p, None, p, 2, 4, 0, 1.0, 0.5, p, p, p, p, None) == INVALID_ARG


def test_loss_word_argument_checks_need_no_device():
    """pg_ctc_loss's word-reward arguments are checked before any kernel runs."""
    import torch
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    z = torch.zeros(5, 2, 29)
    il = torch.full((2,), 5, dtype=torch.int32)
    tg = torch.ones(2, 2, dtype=torch.int32)
    tl = torch.full((2,), 2, dtype=torch.int32)
    for kw in ({"reward_unit": "phoneme", "word_delimiter": 3}, {"reward_unit": "word"},
               {"reward_unit": "word", "word_delimiter": 3, "per_step": True}, {"reward_unit": "word", "word_delimiter": -1},
               {"reward_unit": "word", "word_delimiter": 0}, {"reward_unit": "word", "word_delimiter": 29}):
        with pytest.raises(ValueError):
            pg_ctc_loss(z, il, tg, tl, **kw)
