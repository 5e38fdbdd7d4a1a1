"""The sequence-level score function (score_function="sequence") on a GPU-less host: its entry points are exported and bound with
the header's argument counts, reject what they cannot take before touching a pointer, size their workspace by the documented
formula; the host layer's argument checks; and the identity the feature rests on, by enumeration with the fp64 oracle."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
NEW = {"pgasr_ctc_hyp_workspace_bytes": ctypes.c_size_t, "pgasr_ctc_hyp_lattice": ctypes.c_int,
       "pgasr_ctc_grad_from_lattices_seq": ctypes.c_int, "pgasr_pg_loss_value_seq": ctypes.c_int}
INVALID_ARG, WORKSPACE, UNSUPPORTED = 1, 3, 4


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def test_seq_symbols_exported_and_bound_abi_stays_7(lib):
    from policy_gradient_asr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, res in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is res, name
    assert int(re.search(r"#define PGASR_ABI_VERSION (\d+)", src).group(1)) == 7
    assert lib.pgasr_abi_version() == 7


def _lattice(lib, K, Lh, ws_bytes=1 << 40, stride=2048):
    p = 0x1000
    return lib.pgasr_ctc_hyp_lattice(p, p, stride, p, p, 10, 2, 29, K, Lh, 0, p, p, ws_bytes, None)


def _grad(lib, K, Lh, ws_bytes=1 << 40):
    p = 0x1000
    return lib.pgasr_ctc_grad_from_lattices_seq(p, p, p, 10, 2, 29, 3, 0, p, K, p, p, p, Lh, p, p, ws_bytes, p, ws_bytes, None)


def _value(lib, K, Lh):
    p = 0x1000
    return lib.pgasr_pg_loss_value_seq(p, p, K, p, p, p, p, p, p, Lh, 10, 2, 29, p, None)


def test_invalid_and_unsupported_sizes_are_rejected_without_a_device(lib):
    """The pointers below are fake: every call must return before dereferencing or launching anything."""
    for K in (0, -1, 17):
        assert _lattice(lib, K, 5) == INVALID_ARG
        assert _grad(lib, K, 5) == INVALID_ARG
        assert _value(lib, K, 5) == INVALID_ARG
        assert lib.pgasr_ctc_hyp_workspace_bytes(10, 2, 29, K, 5) == 0
    assert _lattice(lib, 4, -1) == INVALID_ARG
    assert _grad(lib, 4, -1) == INVALID_ARG
    assert _value(lib, 4, -1) == INVALID_ARG
    assert lib.pgasr_ctc_hyp_workspace_bytes(10, 2, 29, 4, -1) == 0
    # 2*Lh+1 > 2048
    assert _lattice(lib, 4, 1024) == UNSUPPORTED
    assert _grad(lib, 4, 1024) == UNSUPPORTED
    assert lib.pgasr_ctc_hyp_workspace_bytes(10, 2, 29, 4, 1024) == 0
    # V > 64
    p = 0x1000
    assert lib.pgasr_ctc_hyp_lattice(p, p, 10, p, p, 10, 2, 65, 4, 5, 0, p, p, 1 << 40, None) == UNSUPPORTED
    # null pointers, a short workspace
    assert lib.pgasr_ctc_hyp_lattice(None, p, 10, p, p, 10, 2, 29, 4, 5, 0, p, p, 1 << 40, None) == INVALID_ARG
    assert lib.pgasr_ctc_hyp_lattice(p, p, 10, p, p, 10, 2, 29, 4, 5, 0, None, p, 1 << 40, None) == INVALID_ARG
    assert lib.pgasr_pg_loss_value_seq(p, p, 4, p, p, p, p, None, p, 5, 10, 2, 29, p, None) == INVALID_ARG
    assert lib.pgasr_ctc_hyp_lattice(p, p, 4, p, p, 10, 2, 29, 4, 5, 0, p, p, 1 << 40, None) == INVALID_ARG     # token rows shorter than Lh
    assert _lattice(lib, 4, 5, ws_bytes=16) == WORKSPACE
    assert _grad(lib, 4, 5, ws_bytes=16) == WORKSPACE
    assert lib.pgasr_ctc_hyp_lattice(p, p, 10, p, p, 10, 2, 29, 4, 5, 0, p, None, 1 << 40, None) == WORKSPACE


def _formula(T, B, V, K, Lh):
    """The lattices, 2 * K*B*T * roundup64(2*Lh+1) * 4 bytes, plus the per-pair tables: two fp64 row maxima per (pair, frame), one
    fp64 nll, V+1 label offsets and 2*Lh+1 label states per pair -- every array rounded up to 256 bytes."""
    up = lambda n: (n + 255) // 256 * 256
    P, S = K * B, 2 * Lh + 1
    SP = (S + 63) // 64 * 64
    lattices = 2 * up(P * T * SP * 4)
    tables = 2 * up(P * T * 8) + up(P * 8) + up(P * (V + 1) * 4) + up(P * S * 4)
    return lattices, tables


def test_hyp_workspace_bytes_is_the_documented_formula(lib):
    from policy_gradient_asr_amd import hipops
    for T, B, V, K, Lh in ((1000, 32, 29, 4, 1000), (1000, 32, 29, 4, 200), (160, 6, 64, 16, 160), (50, 3, 29, 1, 0)):
        lattices, tables = _formula(T, B, V, K, Lh)
        assert hipops.ctc_hyp_workspace_bytes(T, B, V, K, Lh) == lattices + tables
        assert tables < 0.02 * lattices + 4096
    # the headline figures of the docstring
    assert abs(_formula(1000, 32, 29, 4, 1000)[0] - 2.1e9) < 0.05e9
    assert abs(_formula(1000, 32, 29, 4, 200)[0] - 0.46e9) < 0.01e9
    sizes_k = [hipops.ctc_hyp_workspace_bytes(200, 8, 29, K, 100) for K in range(1, 17)]
    assert all(a < b for a, b in zip(sizes_k, sizes_k[1:]))
    sizes_l = [hipops.ctc_hyp_workspace_bytes(200, 8, 29, 4, Lh) for Lh in range(0, 201)]
    assert all(a <= b for a, b in zip(sizes_l, sizes_l[1:])) and sizes_l[0] < sizes_l[-1]
    assert hipops.hyp_len_cap(1000) == 1000 and hipops.hyp_len_cap(4000) == 1023 == hipops.MAX_HYP_LEN
    assert hipops.hyp_len_cap(1000, 200) == 200 and hipops.hyp_len_cap(100, 200) == 100


def test_loss_argument_checks_need_no_device():
    import torch
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    z = torch.zeros(5, 2, 29)
    il = torch.full((2,), 5, dtype=torch.int32)
    tg = torch.ones(2, 2, dtype=torch.int32)
    tl = torch.full((2,), 2, dtype=torch.int32)
    for kw in ({"score_function": "sequence", "per_step": True}, {"score_function": "hypothesis"}, {"score_function": None},
               {"score_function": "sequence", "max_hyp_len": -1}, {"score_function": "sequence", "max_hyp_len": 2.5},
               {"score_function": "sequence", "max_hyp_len": True}, {"score_function": "sequence", "max_hyp_len": "3"},
               {"score_function": "path", "max_hyp_len": 3}, {"max_hyp_len": 0}):
        with pytest.raises(ValueError):
            pg_ctc_loss(z, il, tg, tl, **kw)


def test_trainer_argument_checks_need_no_device():
    import torch
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    m = torch.nn.Linear(4, 3)
    with pytest.raises(ValueError, match="per-step"):
        PolicyGradientTrainer(m, score_function="sequence", reward_mode="per_step")
    with pytest.raises(ValueError, match="score_function"):
        PolicyGradientTrainer(m, score_function="token")
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="max_hyp_len"):
            PolicyGradientTrainer(m, score_function="sequence", max_hyp_len=bad)
    with pytest.raises(ValueError, match="max_hyp_len"):
        PolicyGradientTrainer(m, max_hyp_len=10)
    tr = PolicyGradientTrainer(m, score_function="sequence", max_hyp_len=0, num_samples=4, reward_baseline="leave_one_out")
    assert (tr.score_function, tr.max_hyp_len, tr.last_sequence_scored) == ("sequence", 0, None)
    assert PolicyGradientTrainer(m).score_function == "path"
    tr.score_function = "token"          # a setting changed after construction is caught where the step checks its limits
    with pytest.raises(ValueError, match="score_function"):
        tr._check_limits(torch.zeros(2, 4, 5), torch.zeros(2, 3, dtype=torch.long))
    assert PolicyGradientTrainer.MAX_HYP_LEN == 1023


def test_path_and_sequence_level_expectations_agree_by_enumeration():
    """E_pi[(R(y) - b) grad log p(pi|x)] = E_y[(R(y) - b) grad log p(y|x)], y = collapse(pi): all 243 paths of a T = 5, V = 3 case
    against the sum over their distinct hypotheses, gradients from the fp64 oracle."""
    from oracle import ctc_ref, decode_ref
    T, V = 5, 3
    rng = np.random.default_rng(7)
    logits = rng.normal(size=(T, 1, V)) * 1.5
    lp = ctc_ref.log_softmax(logits, axis=2)
    target = [1, 2, 1]
    base = -0.4
    il = np.array([T])
    reward = lambda y: -decode_ref.edit_dist(target, list(y))[0] / len(target)
    g_path = np.zeros((T, 1, V))
    p_y = {}
    for pi in itertools.product(range(V), repeat=T):
        path = np.array(pi, dtype=np.int64)[:, None]
        p = float(np.exp(lp[np.arange(T), 0, path[:, 0]].sum()))
        y = tuple(decode_ref.collapse_path(path[:, 0]))
        p_y[y] = p_y.get(y, 0.0) + p
        g_path += decode_ref.reinforce_grad(logits, path, np.array([p * (reward(y) - base)]), il)
    g_seq = np.zeros((T, 1, V))
    total = 0.0
    for y, p_enum in p_y.items():
        tg = np.array([list(y) + [0] * (T - len(y))], dtype=np.int64)
        nll, g = ctc_ref.ctc_loss_and_grad(logits, tg, il, np.array([len(y)]))
        p = float(np.exp(-nll[0]))
        assert abs(p - p_enum) < 1e-12          # the lattice sums exactly the paths that collapse to y
        total += p
        g_seq += p * (reward(y) - base) * g
    assert abs(total - 1.0) < 1e-12
    assert len(p_y) > 20
    assert np.abs(g_path).max() > 1e-3
    assert np.abs(g_path - g_seq).max() < 1e-12
