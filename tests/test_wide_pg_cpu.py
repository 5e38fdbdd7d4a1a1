"""The multi-sample, entropy and KL objectives for alphabets of 65 .. 1024 symbols on a GPU-less host: the four A12-WIDE entry
points' export, binding and argument checks (no compute call: every rejection happens before a launch), the ``wide_objectives``
option rule of ``loss.check_options`` and of the trainer, and the precondition of the sampler's GPU test -- that the fp64 reference
stays inside the project's sampler rule against ANY float32 evaluation of the kernels' cdf rule."""
import os

import numpy as np
import pytest

import wide_pg_cases as wc
from policy_gradient_asr_amd import hipops
from policy_gradient_asr_amd.loss import PGOptions, check_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
NEW = ("pgasr_frame_sample_multi_wide", "pgasr_frame_entropy_wide", "pgasr_frame_kl_wide", "pgasr_ctc_grad_from_lattice_multi_wide")
INVALID_ARG, UNSUPPORTED, WORKSPACE = 1, 4, 3


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    from policy_gradient_asr_amd import _lib
    header = open(HEADER).read()
    assert "A12-WIDE" in header
    for name in NEW:
        assert name in _lib.SIGNATURES and name + "(" in header
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.pgasr_abi_version() == 7
    # the statistics take their narrow twins' arguments, one for one; the sampler those of the single-sample wide entry plus K
    assert _lib.SIGNATURES["pgasr_frame_entropy_wide"] == _lib.SIGNATURES["pgasr_frame_entropy"]
    assert _lib.SIGNATURES["pgasr_frame_kl_wide"] == _lib.SIGNATURES["pgasr_frame_kl"]
    assert len(_lib.SIGNATURES["pgasr_frame_sample_multi_wide"][1]) == len(_lib.SIGNATURES["pgasr_frame_argmax_sample_wide"][1]) + 1
    assert _lib.SIGNATURES["pgasr_ctc_grad_from_lattice_multi_wide"] == _lib.SIGNATURES["pgasr_ctc_grad_from_lattice_multi_kl"]


def test_argument_checks_need_no_device(lib):
    """Every rejection below happens before a launch: the pointers are never dereferenced."""
    p, big = 0x1000, 1 << 40
    smp = lib.pgasr_frame_sample_multi_wide
    #          sc   T  B     V  K sd of st ba ids  g  s  stream
    assert smp(p, 10, 2, 1025, 4, 0, 0, 0, 0, None, p, p, None) == UNSUPPORTED
    assert smp(p, 10, 2, 300, 0, 0, 0, 0, 0, None, p, p, None) == INVALID_ARG
    assert smp(p, 10, 2, 300, 17, 0, 0, 0, 0, None, p, p, None) == INVALID_ARG
    assert smp(p, 10, 2, 0, 4, 0, 0, 0, 0, None, p, p, None) == INVALID_ARG
    assert smp(p, 0, 2, 300, 4, 0, 0, 0, 0, None, p, p, None) == INVALID_ARG
    assert smp(None, 10, 2, 300, 4, 0, 0, 0, 0, None, p, p, None) == INVALID_ARG
    assert smp(p, 10, 2, 300, 4, 0, 0, 0, 0, None, p, None, None) == INVALID_ARG             # the samples are required
    assert smp(p, 10, 2, 300, 4, 0, 0, 4, 4, None, p, p, None) == INVALID_ARG                # ctr_base outside the global batch
    assert smp(p, 10, 2, 300, 4, 0, 0, 0, 0, p, p, p, None) == INVALID_ARG                   # ids need ctr_stride >= 1
    assert smp(p, 4096, 2, 300, 4, 0, 0, (1 << 20) + 1, 0, p, p, p, None) == UNSUPPORTED     # T * ctr_stride > 2^32 with ids

    ent = lib.pgasr_frame_entropy_wide
    assert ent(p, p, 10, 2, 1025, 0.0, 1.0, p, p, None) == UNSUPPORTED
    assert ent(p, p, 10, 2, 0, 0.0, 1.0, p, p, None) == INVALID_ARG
    assert ent(p, p, 10, 0, 300, 0.0, 1.0, p, p, None) == INVALID_ARG
    assert ent(None, p, 10, 2, 300, 0.0, 1.0, p, p, None) == INVALID_ARG
    assert ent(p, None, 10, 2, 300, 0.0, 1.0, p, p, None) == INVALID_ARG
    assert ent(p, p, 10, 2, 300, 0.0, 1.0, None, p, None) == INVALID_ARG
    assert ent(p, p, 10, 2, 300, -1.0, 1.0, p, p, None) == INVALID_ARG
    assert ent(p, p, 10, 2, 300, 0.0, 0.0, p, p, None) == INVALID_ARG

    kl = lib.pgasr_frame_kl_wide
    assert kl(p, p, p, 10, 2, 1025, 0.0, 1.0, p, p, None) == UNSUPPORTED
    assert kl(p, p, p, 10, 2, 0, 0.0, 1.0, p, p, None) == INVALID_ARG
    assert kl(p, None, p, 10, 2, 300, 0.0, 1.0, p, p, None) == INVALID_ARG                   # the reference
    assert kl(p, p, None, 10, 2, 300, 0.0, 1.0, p, p, None) == INVALID_ARG
    assert kl(p, p, p, 10, 2, 300, 0.0, 1.0, p, None, None) == INVALID_ARG
    assert kl(p, p, p, 10, 2, 300, float("nan"), 1.0, p, p, None) == INVALID_ARG

    gm = lib.pgasr_ctc_grad_from_lattice_multi_wide
    #         lp il tl   T  B     V  L bl us  K cf pa es rf ks  g ws bytes st
    assert gm(p, p, p, 10, 2, 1025, 3, 0, p, 4, p, p, p, p, p, p, p, big, None) == UNSUPPORTED
    assert gm(p, p, p, 10, 2, 300, 1024, 0, p, 4, p, p, p, p, p, p, p, big, None) == UNSUPPORTED        # 2 * Lmax + 1 > 2048
    assert gm(p, p, p, 10, 2, 300, 3, 0, p, 0, p, p, p, p, p, p, p, big, None) == INVALID_ARG
    assert gm(p, p, p, 10, 2, 300, 3, 0, p, 17, p, p, p, p, p, p, p, big, None) == INVALID_ARG
    assert gm(p, p, p, 10, 2, 0, 3, 0, p, 4, p, p, p, p, p, p, p, big, None) == INVALID_ARG
    assert gm(p, p, p, 10, 2, 300, 3, 300, p, 4, p, p, p, p, p, p, p, big, None) == INVALID_ARG         # blank outside [0, V)
    assert gm(p, p, p, 10, 2, 300, 3, -1, p, 4, p, p, p, p, p, p, p, big, None) == INVALID_ARG
    assert gm(None, p, p, 10, 2, 300, 3, 0, p, 4, p, p, p, p, p, p, p, big, None) == INVALID_ARG
    assert gm(p, None, p, 10, 2, 300, 3, 0, p, 4, p, p, p, p, p, p, p, big, None) == INVALID_ARG
    assert gm(p, p, p, 10, 2, 300, 3, 0, p, 4, None, p, p, p, p, p, p, big, None) == INVALID_ARG        # the coefficients
    assert gm(p, p, p, 10, 2, 300, 3, 0, p, 4, p, None, p, p, p, p, p, big, None) == INVALID_ARG        # the paths
    assert gm(p, p, p, 10, 2, 300, 3, 0, p, 4, p, p, p, p, p, None, p, big, None) == INVALID_ARG        # grad
    assert gm(p, p, p, 10, 2, 300, 3, 0, p, 4, p, p, p, p, None, p, p, big, None) == INVALID_ARG        # ref_log_probs without kl_scale
    assert gm(p, p, p, 10, 2, 300, 3, 0, p, 4, p, p, None, None, p, p, p, big, None) == INVALID_ARG     # kl_scale without ref_log_probs
    for tails in ((None, None, None), (p, None, None), (None, p, p), (p, p, p)):
        assert gm(p, p, p, 10, 2, 300, 3, 0, p, 4, p, p, *tails, p, p, 16, None) == WORKSPACE
        assert gm(p, p, p, 10, 2, 300, 3, 0, p, 4, p, p, *tails, p, None, big, None) == WORKSPACE
    # the narrow twins still refuse 65 symbols
    assert lib.pgasr_frame_sample_multi(p, 10, 2, 65, 4, 0, 0, 0, 0, p, p, None) == UNSUPPORTED
    assert lib.pgasr_frame_sample_multi_ids(p, 10, 2, 65, 4, 0, 0, 2, p, p, p, None) == UNSUPPORTED
    assert lib.pgasr_frame_entropy(p, p, 10, 2, 65, 0.0, 1.0, p, p, None) == UNSUPPORTED
    assert lib.pgasr_frame_kl(p, p, p, 10, 2, 65, 0.0, 1.0, p, p, None) == UNSUPPORTED
    assert lib.pgasr_ctc_grad_from_lattice_multi_kl(p, p, p, 10, 2, 65, 3, 0, p, 4, p, p, p, p, p, p, p, big, None) == UNSUPPORTED


OPENED = [dict(num_samples=2), dict(num_samples=16), dict(num_samples=2, baseline="leave_one_out"), dict(entropy_weight=0.1),
          dict(kl_weight=0.1), dict(num_samples=4, baseline="leave_one_out", entropy_weight=0.1, kl_weight=0.2)]
STILL_REFUSED = [("beam", dict(beam=4)), ("score_function", dict(score_function="sequence")),
                 ("reward_unit", dict(reward_unit="word", word_delimiter=3)), ("per_step", dict(per_step=True))]


@pytest.mark.parametrize("vocab", [65, 1024])
@pytest.mark.parametrize("fields", OPENED, ids=lambda f: "+".join(f))
def test_wide_objectives_admits_the_four_options(vocab, fields):
    opt = check_options(PGOptions(**fields), vocab=vocab, frames=100, symbols=12, wide_objectives=True)
    assert opt.num_samples == fields.get("num_samples", 1) and opt.baseline == fields.get("baseline", "hypothesis")
    assert opt.entropy_weight == fields.get("entropy_weight", 0.0) and opt.kl_weight == fields.get("kl_weight", 0.0)
    if fields != OPENED[-1]:
        name = "baseline" if "baseline" in fields else next(iter(fields))
        with pytest.raises(ValueError, match=name + "="):                       # without the keyword: refused as ever
            check_options(PGOptions(**fields), vocab=vocab, frames=100, symbols=12)
    check_options(PGOptions(**fields), vocab=64, frames=100, symbols=12, wide_objectives=True)      # at 64 symbols it changes nothing
    # the options' own rules hold with it
    with pytest.raises(ValueError, match="num_samples"):
        check_options(PGOptions(num_samples=17), vocab=vocab, wide_objectives=True)
    with pytest.raises(ValueError, match="leave-one-out"):
        check_options(PGOptions(baseline="leave_one_out"), vocab=vocab, wide_objectives=True)
    with pytest.raises(ValueError, match="1025"):
        check_options(PGOptions(), vocab=1025, wide_objectives=True)


@pytest.mark.parametrize("name,fields", STILL_REFUSED)
def test_wide_objectives_still_refuses_the_rest_by_name(name, fields):
    for vocab in (65, 1024):
        for more in ({}, dict(entropy_weight=0.1)) if name != "per_step" else ({},):
            with pytest.raises(ValueError, match=name + "=") as e:
                check_options(PGOptions(**fields, **more), vocab=vocab, frames=100, symbols=12, wide_objectives=True)
            msg = str(e.value)
            assert "64" in msg and "wide_objectives" in msg                      # and says what the keyword does open
            assert all(opened in msg for opened in ("num_samples", "leave_one_out", "entropy_weight", "kl_weight"))
    check_options(PGOptions(**fields), vocab=64, frames=100, symbols=12, wide_objectives=True)


def test_trainer_takes_wide_objectives_with_wide_alphabet_only():
    import torch
    from policy_gradient_asr_amd.mwer import MWERTrainer
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer

    class Toy(torch.nn.Module):
        def __init__(self, V):
            super().__init__()
            self.head = torch.nn.Linear(4, V)

        def logits(self, x, fmask, lengths=None):
            raise NotImplementedError

    tr = PolicyGradientTrainer(Toy(300), wide_alphabet=True, wide_objectives=True, num_samples=4, reward_baseline="leave_one_out",
                               entropy_weight=0.1, kl_weight=0.1, kl_reference="initial")
    assert tr.wide_objectives and tr.MAX_VOCAB == 1024 and tr.num_samples == 4 and tr.kl_reference is not None
    assert PolicyGradientTrainer(Toy(300), wide_alphabet=True).wide_objectives is False
    PolicyGradientTrainer(Toy(1024), wide_alphabet=True, wide_objectives=True, num_samples=16)
    PolicyGradientTrainer(Toy(300), wide_alphabet=True, wide_objectives=True)                     # the default objective, as ever
    with pytest.raises(ValueError, match="wide_alphabet"):
        PolicyGradientTrainer(Toy(300), wide_objectives=True)
    with pytest.raises(ValueError, match="wide_alphabet"):
        PolicyGradientTrainer(Toy(29), wide_objectives=True, num_samples=2)
    with pytest.raises(ValueError, match="num_samples"):                                          # without the keyword: as ever
        PolicyGradientTrainer(Toy(300), wide_alphabet=True, num_samples=2)
    with pytest.raises(ValueError, match="kl_reference"):
        PolicyGradientTrainer(Toy(300), wide_alphabet=True, wide_objectives=True, kl_weight=0.1)
    for name, kw in (("beam", dict(reward_decoder="beam")), ("score_function", dict(score_function="sequence")),
                     ("reward_unit", dict(reward_unit="word", word_delimiter=3)), ("per_step", dict(reward_mode="per_step"))):
        with pytest.raises(ValueError, match=name):
            PolicyGradientTrainer(Toy(300), wide_alphabet=True, wide_objectives=True, **kw)
    with pytest.raises(ValueError, match="1025"):
        PolicyGradientTrainer(Toy(1025), wide_alphabet=True, wide_objectives=True)
    # a setting changed after construction is checked before the step, with the keyword's rule
    tr = PolicyGradientTrainer(Toy(300), wide_alphabet=True, wide_objectives=True)
    tr.entropy_weight = 0.1
    assert tr._checked_options(frames=100, symbols=12).entropy_weight == 0.1
    tr.score_function = "sequence"
    with pytest.raises(ValueError, match="score_function"):
        tr._checked_options(frames=100, symbols=12)
    with pytest.raises((ValueError, TypeError)):
        MWERTrainer(Toy(29), wide_objectives=True)


def test_wrappers_route_by_vocab_and_refuse_cpu_tensors():
    import torch
    from policy_gradient_asr_amd import _lib
    assert hipops._wide(300, None, "x") and not hipops._wide(64, None, "x") and hipops._wide(29, True, "x")
    for call in (lambda: hipops.frame_sample_multi(torch.zeros(2, 2, 300), 2, wide=False),
                 lambda: hipops.frame_entropy(torch.zeros(2, 2, 300), torch.zeros(2, dtype=torch.int32), wide=False),
                 lambda: hipops.frame_kl(torch.zeros(2, 2, 300), torch.zeros(2, 2, 300), torch.zeros(2, dtype=torch.int32), wide=False)):
        with pytest.raises(_lib.PgasrError):
            call()


@pytest.mark.parametrize("V", wc.WIDE_V)
def test_the_samplers_cap_is_reachable(V):
    """The precondition of the GPU sampler test: a plain numpy float32 evaluation of the cdf rule (fp32 exp, fp32 sequential
    cumsum, cdf <= u * total) differs from the fp64 reference only inside the project's sampler rule -- where |cdf - u| < 2e-6, in
    at most max(1, draws // 1000) of a case's 5120 draws -- so the reference leaves the kernels room to pass.  Measured when this test
    was written: at most 2 of a case's 5120 draws at V = 1024, none at the other four V, the largest |cdf - u| at a differing draw
    2.6e-7."""
    from oracle import decode_ref
    for kind in wc.KINDS:
        paths, cdf, u = wc.oracle_draws(V, kind)
        got = wc.f32_draws(wc.sampler_scores(V, kind).numpy(), wc.K_MAX)
        assert got.shape == paths.shape == (16, 40, 8) and got.min() >= 0 and got.max() < V
        n, worst = wc.draw_mismatches(got, paths, cdf, u)
        print(f"[wide pg sampler, float32 numpy] V={V} {kind}: {n} of {got.size} draws differ (largest |cdf - u| there {worst:.2e})")
        assert n <= (2 if V == 1024 else 0)
        # draw 0 is decode_ref's single-sample draw: the K-draw reference extends the single-sample one
        assert np.array_equal(decode_ref.sample_paths(wc.sampler_scores(V, kind).numpy(), seed=wc.SEED, offset=wc.OFFSET)[0], paths[0])
