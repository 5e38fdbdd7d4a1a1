"""Per-step rewards with K samples (include/pgasr_hip.h, A12-STEP) on a GPU-less host: the fp64 statement against the single-path
oracle, unbiasedness by enumeration, per-frame properties, the GPU tests' inputs, the ABI and the option checks."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from oracle import ctc_ref, decode_ref, pg_ref

import step_rewards_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
NEW = ("pgasr_pg_step_coefs_multi", "pgasr_ctc_grad_from_lattice_multi_steps", "pgasr_pg_loss_value_multi_steps")
INVALID_ARG = 1


def _case(T=12, B=3, V=5, L=4, K=1, seed=0):
    rng = np.random.default_rng(seed)
    logits = rng.normal(size=(T, B, V)) * 1.5
    targets = rng.integers(1, V, (B, L)).astype(np.int32)
    in_len = np.array([T, T - 3, T - 1][:B])
    tg_len = np.array([L, L - 1, 2][:B])
    paths = pg_ref.sample_paths(logits, K, seed=5, offset=2)[0]
    return logits, in_len, targets, tg_len, paths, np.argmax(logits, axis=2)


# ---- (a) K = 1 against the greedy path is the single-path per-step objective ----
def test_one_sample_hypothesis_is_the_single_path_objective():
    logits, in_len, targets, tg_len, paths, greedy = _case()
    want = pg_ref.pg_objective(logits, in_len, targets, tg_len, lam=0.7, per_step=True, paths=paths, greedy_frames=greedy)
    got = sr.step_objective(logits, in_len, targets, tg_len, paths=paths, greedy_frames=greedy, lam=0.7)
    assert got.coef.shape == (1,) + want.coef.shape
    assert np.abs(got.coef[0] - want.coef).max() <= 1e-12
    assert abs(got.loss - want.loss) <= 1e-12 * abs(want.loss)
    assert np.abs(got.grad - want.grad).max() <= 1e-12
    assert np.abs(want.coef).max() > 0


# ---- (b) unbiasedness by enumeration: T = 4, V = 3, y = [1, 2] ----
def _enumeration():
    T, V, y = 4, 3, [1, 2]
    rng = np.random.default_rng(3)
    logits = rng.normal(size=(T, V))
    p = np.exp(ctc_ref.log_softmax(logits, axis=1))
    all_paths = np.array(list(itertools.product(range(V), repeat=T)))                  # (81, T)
    prob = np.prod(p[np.arange(T)[None, :], all_paths], axis=1)
    assert abs(prob.sum() - 1) < 1e-14
    # d log p(pi[t]) / d logits[t] = onehot - softmax, frame by frame: (81, T, V)
    score = np.eye(V)[all_paths] - p[None]
    G0 = np.array([decode_ref.reward_to_go(q, y)[0][0] for q in all_paths])            # |y| - ED(y, collapse(pi))
    exact = np.einsum("i,i,itv->tv", prob, G0, score)                                   # grad of E[G(0)] = sum_pi p(pi) G(0) grad log p(pi)
    return T, V, y, all_paths, prob, score, exact, np.argmax(p, axis=1)


def test_estimator_is_unbiased_one_sample_against_greedy():
    T, V, y, all_paths, prob, score, exact, greedy = _enumeration()
    N = len(all_paths)
    greedy_frames = np.tile(greedy[:, None], (1, N))                                    # the greedy path, for every "utterance"
    targets = np.tile(np.array(y, dtype=np.int32), (N, 1))
    coef = sr.step_coefs(all_paths.T[None], greedy_frames, np.full(N, T), targets, np.full(N, 2), "hypothesis", lam=1.0, Bg=1)
    est = np.einsum("i,ti,itv->tv", prob, coef[0], score) * len(y)                      # coef carries 1 / (K max(L,1))
    err = np.abs(est - exact).max()
    print(f"K = 1 against the greedy path: |E[estimator] - grad E[G(0)]| = {err:.1e} on {np.abs(exact).max():.2f}")
    assert err <= 1e-12 and np.abs(exact).max() > 0.05


def test_estimator_is_unbiased_two_samples_leave_one_out():
    T, V, y, all_paths, prob, score, exact, _ = _enumeration()
    N = len(all_paths)
    i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    i, j = i.ravel(), j.ravel()                                                         # 81^2 pairs, one "utterance" each
    pair_paths = np.stack((all_paths[i].T, all_paths[j].T))                            # (2, T, 6561)
    targets = np.tile(np.array(y, dtype=np.int32), (N * N, 1))
    coef = sr.step_coefs(pair_paths, None, np.full(N * N, T), targets, np.full(N * N, 2), "leave_one_out", lam=1.0, Bg=1)
    w = prob[i] * prob[j]
    est = (np.einsum("n,tn,ntv->tv", w, coef[0], score[i]) + np.einsum("n,tn,ntv->tv", w, coef[1], score[j])) * len(y)
    err = np.abs(est - exact).max()
    print(f"K = 2 leave one out: |E[estimator] - grad E[G(0)]| = {err:.1e} on {np.abs(exact).max():.2f}")
    assert err <= 1e-12


# ---- (c) per-frame properties ----
@pytest.mark.parametrize("baseline", ["hypothesis", "leave_one_out"])
def test_frame_properties(baseline):
    K = 4
    logits, in_len, targets, tg_len, paths, greedy = _case(K=K, seed=1)
    coef = sr.step_coefs(paths, greedy, in_len, targets, tg_len, baseline, lam=0.9, Bg=6)
    utt = pg_ref.pg_objective(logits, in_len, targets, tg_len, lam=0.9, global_batch=6, num_samples=K, baseline=baseline, paths=paths,
                              greedy_frames=greedy)
    assert np.abs(coef[:, 0, :] - utt.coef).max() <= 1e-12 and np.abs(utt.coef).max() > 0
    for b, n in enumerate(in_len):
        assert not coef[:, n:, b].any()
    if baseline == "leave_one_out":
        assert np.abs(coef.sum(axis=0)).max() <= 1e-12 * np.abs(coef).max()


# ---- (d) the inputs of the GPU tests are discriminating ----
def test_gpu_inputs_cross_every_seam_and_tell_the_baselines_apart():
    for T in (130, 257, 1030):
        for blank in (0, sr.COEF_V - 1):
            c = sr.seam_case(T, 3, blank, "hypothesis")
            assert set(np.unique(c.rows)) <= {blank, 1, 2, 3}
            for w in range(c.P):
                st = set(sr.starts(c.rows[w, :, 0], T, blank))
                for s in range(64, T, 64):
                    assert s - 1 in st and s in st, (T, w, s)
            hyp = sr.step_coefs(c.paths, c.greedy, c.in_len, c.targets, c.tg_len, "hypothesis", blank=blank)
            loo = sr.step_coefs(c.paths, None, c.in_len, c.targets, c.tg_len, "leave_one_out", blank=blank)
            for b in (0, 1):                                             # utterance 2 is empty
                n = c.in_len[b]
                assert (np.ptp(hyp[:, :n, b], axis=1) > 0).all() and (np.ptp(loo[:, :n, b], axis=1) > 0).all()
            assert np.abs(hyp - loo).max() > 0.1 * np.abs(hyp).max()
    c = sr.seam_case(257, 2, 0, "leave_one_out")
    assert c.in_len.min() == 0 and 0 < c.in_len[1] < 257 and c.tg_len.min() == 0


# ---- (e) ABI ----
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    from policy_gradient_asr_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert m.group(1).count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    assert lib.pgasr_abi_version() == 7


def test_invalid_arguments_are_rejected_without_a_device(lib):
    """K = 0, K = 17, leave one out with K = 1 and an unknown baseline return PGASR_ERR_INVALID_ARG before anything is launched (the
    pointers below are never dereferenced)."""
    p = 0x1000
    coefs = lambda K, baseline: lib.pgasr_pg_step_coefs_multi(p, p, p, 8, p, p, 10, 2, K, baseline, 0, 1.0, 0.5, p, None)
    for K in (0, 17):
        assert coefs(K, 0) == INVALID_ARG
        assert lib.pgasr_ctc_grad_from_lattice_multi_steps(p, p, p, 10, 2, 29, 3, 0, p, K, p, p, None, None, None, p, p, 1 << 20,
                                                           None) == INVALID_ARG
        assert lib.pgasr_pg_loss_value_multi_steps(p, p, K, p, p, p, p, 10, 2, 29, p, None) == INVALID_ARG
    assert coefs(1, 1) == INVALID_ARG            # leave one out, K = 1
    assert coefs(4, 2) == INVALID_ARG            # unknown baseline
    assert lib.pgasr_pg_step_coefs_multi(p, p, None, 8, p, p, 10, 2, 4, 0, 0, 1.0, 0.5, p, None) == INVALID_ARG
    # the KL pointers come together
    assert lib.pgasr_ctc_grad_from_lattice_multi_steps(p, p, p, 10, 2, 29, 3, 0, p, 2, p, p, None, p, None, p, p, 1 << 20,
                                                       None) == INVALID_ARG


# ---- (f) options ----
def _opt(per_step=True, **kw):
    from policy_gradient_asr_amd.loss import PGOptions
    return PGOptions(per_step=per_step, **kw)


ADMITTED = [dict(), dict(num_samples=4), dict(num_samples=16, baseline="leave_one_out"), dict(num_samples=2, baseline="leave_one_out"),
            dict(entropy_weight=0.1), dict(num_samples=4, kl_weight=0.2, entropy_weight=0.1),
            dict(num_samples=3, sample_base=2, global_batch=8)]


@pytest.mark.parametrize("kw", ADMITTED)
def test_step_objectives_admits(kw):
    from policy_gradient_asr_amd.loss import check_options
    for vocab, wide in ((29, {}), (64, {}), (300, dict(wide_objectives=True)), (1024, dict(wide_objectives=True))):
        opt = check_options(_opt(**kw), vocab=vocab, frames=50, symbols=8, step_objectives=True, **wide)
        assert opt.step_objectives and opt.per_step
        assert check_options(_opt(step_objectives=True, **kw), vocab=vocab, frames=50, symbols=8, **wide).step_objectives
    # above 64 symbols the keyword alone admits one sample against the greedy path without tails
    assert check_options(_opt(), vocab=300, step_objectives=True).step_objectives
    # without per_step the keyword changes nothing
    from policy_gradient_asr_amd.loss import PGOptions
    assert check_options(PGOptions(num_samples=4), vocab=29, step_objectives=True).num_samples == 4


def test_step_objectives_keeps_refusing():
    from policy_gradient_asr_amd.loss import check_options
    from policy_gradient_asr_amd.units import UnitSpelling  # noqa: F401
    for name, kw in (("beam", dict(beam=4)), ("score_function", dict(score_function="sequence")),
                     ("reward_unit", dict(reward_unit="word", word_delimiter=3))):
        for vocab, wide in ((29, {}), (300, dict(wide_objectives=True))):
            with pytest.raises(ValueError, match=name):
                check_options(_opt(num_samples=2, **kw), vocab=vocab, step_objectives=True, **wide)
    with pytest.raises(ValueError, match="beam") as e:                          # .. and no longer says that per-step rewards are refused
        check_options(_opt(beam=4, per_step=False), vocab=300, step_objectives=True, wide_objectives=True)
    assert "per-step" not in str(e.value)
    with pytest.raises(ValueError, match="leave-one-out"):
        check_options(_opt(baseline="leave_one_out"), vocab=29, step_objectives=True)
    with pytest.raises(ValueError, match="num_samples"):
        check_options(_opt(num_samples=17), vocab=29, step_objectives=True)
    # above 64 symbols everything but one sample against the greedy path needs wide_objectives as well, and is refused naming it
    for name, kw in (("num_samples", dict(num_samples=4)), ("baseline", dict(num_samples=2, baseline="leave_one_out")),
                     ("entropy_weight", dict(entropy_weight=0.1)), ("kl_weight", dict(kl_weight=0.1))):
        with pytest.raises(ValueError, match="wide_objectives") as e:
            check_options(_opt(**kw), vocab=300, step_objectives=True)
        assert name in str(e.value)
    # without the keyword the refusals are what they were
    with pytest.raises(ValueError, match="one sampled path"):
        check_options(_opt(num_samples=4), vocab=29)
    with pytest.raises(ValueError, match="per_step"):
        check_options(_opt(), vocab=300, wide_objectives=True)


def test_unit_spelling_stays_refused_with_per_step():
    from policy_gradient_asr_amd.loss import check_options

    class Spelling:      # the attributes _check_spelling looks for
        offsets = chars = delimiter = to = None
        max_unit_chars, vocab = 4, 29

    with pytest.raises(ValueError, match="unit_spelling"):
        check_options(_opt(num_samples=2, unit_spelling=Spelling()), vocab=29, step_objectives=True)


def test_trainers_and_driver_take_the_keyword():
    import inspect
    from policy_gradient_asr_amd import model
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    from policy_gradient_asr_amd.mwer import MWERTrainer
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    assert inspect.signature(pg_ctc_loss).parameters["step_objectives"].default is False
    assert inspect.signature(PolicyGradientTrainer.__init__).parameters["step_objectives"].default is False
    sig = inspect.signature(model.train).parameters
    assert sig["reward_mode"].default == "utterance" and sig["step_objectives"].default is None
    assert MWERTrainer._FIXED["reward_mode"] == "utterance" and "step_objectives" not in MWERTrainer._FIXED


def test_loss_argument_checks_need_no_device():
    """pg_ctc_loss checks the per-step arguments before any kernel runs, with and without the keyword."""
    import torch
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    z = torch.zeros(5, 2, 29)
    il = torch.full((2,), 5, dtype=torch.int32)
    tg = torch.ones(2, 2, dtype=torch.int32)
    tl = torch.full((2,), 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="one sampled path"):
        pg_ctc_loss(z, il, tg, tl, num_samples=4, per_step=True)
    for kw in (dict(beam=3), dict(score_function="sequence"), dict(num_samples=1, baseline="leave_one_out"), dict(num_samples=17)):
        with pytest.raises(ValueError):
            pg_ctc_loss(z, il, tg, tl, per_step=True, step_objectives=True, **kw)
