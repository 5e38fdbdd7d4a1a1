"""Sequence-level REINFORCE and MWER for alphabets of 65 .. 1024 symbols on a GPU-less host: the three A13-WIDE entry points'
export, binding and argument checks (no compute call: every rejection happens before a launch), the ``wide_sequence`` option rule
of ``loss.check_options``, of the two trainers and of ``mwer.check_mwer_options``, and the wrappers' routing."""
import os

import pytest

from policy_gradient_asr_amd import hipops
from policy_gradient_asr_amd.loss import PGOptions, check_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pgasr_hip.h")
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
NEW = ("pgasr_ctc_hyp_workspace_bytes_wide", "pgasr_ctc_hyp_lattice_wide", "pgasr_ctc_grad_from_lattices_seq_wide")
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
    assert "A13-WIDE" in header
    for name in NEW:
        assert name in _lib.SIGNATURES and name + "(" in header
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.pgasr_abi_version() == 7
    # the query and the lattice take their narrow twins' arguments, one for one; the pass those of the _seq_kl entry
    assert _lib.SIGNATURES["pgasr_ctc_hyp_workspace_bytes_wide"] == _lib.SIGNATURES["pgasr_ctc_hyp_workspace_bytes"]
    assert _lib.SIGNATURES["pgasr_ctc_hyp_lattice_wide"] == _lib.SIGNATURES["pgasr_ctc_hyp_lattice"]
    assert _lib.SIGNATURES["pgasr_ctc_grad_from_lattices_seq_wide"] == _lib.SIGNATURES["pgasr_ctc_grad_from_lattices_seq_kl"]


def test_workspace_query(lib):
    q, qw = lib.pgasr_ctc_hyp_workspace_bytes, lib.pgasr_ctc_hyp_workspace_bytes_wide
    for T, B, K, Lh in ((48, 3, 4, 20), (1000, 32, 16, 300), (7, 1, 1, 0)):
        assert qw(T, B, 64, K, Lh) == q(T, B, 64, K, Lh) > 0
        assert qw(T, B, 1024, K, Lh) > qw(T, B, 64, K, Lh)               # the same layout with longer label-offset tables
    assert q(48, 3, 65, 4, 20) == 0 and qw(48, 3, 65, 4, 20) > 0
    assert qw(48, 3, 1025, 4, 20) == 0 and qw(48, 3, 300, 0, 20) == 0 and qw(48, 3, 300, 17, 20) == 0 and qw(48, 3, 300, 4, 1024) == 0
    # the formula of the documents: 2 * K*B*T * roundup64(2*Lh+1) * 4 bytes of alpha / beta, 2.1 GB at K = 4, B = 32, T = 1000, Lh = 1000
    lattices = 2 * 4 * 32 * 1000 * 2048 * 4
    assert lattices <= qw(1000, 32, 1024, 4, 1000) < lattices * 1.01 and round(lattices / 1e9, 1) == 2.1


def test_argument_checks_need_no_device(lib):
    """Every rejection below happens before a launch: the pointers are never dereferenced."""
    p, big = 0x1000, 1 << 40
    lat = lib.pgasr_ctc_hyp_lattice_wide
    #          lp hy st hl il   T  B    V  K  Lh bl nll ws bytes st
    assert lat(p, p, 30, p, p, 10, 2, 1025, 4, 20, 0, p, p, big, None) == UNSUPPORTED
    assert lat(p, p, 1024, p, p, 10, 2, 300, 4, 1024, 0, p, p, big, None) == UNSUPPORTED        # 2 * Lh + 1 > 2048
    assert lat(p, p, 30, p, p, 10, 2, 300, 0, 20, 0, p, p, big, None) == INVALID_ARG
    assert lat(p, p, 30, p, p, 10, 2, 300, 17, 20, 0, p, p, big, None) == INVALID_ARG
    assert lat(p, p, 30, p, p, 10, 2, 0, 4, 20, 0, p, p, big, None) == INVALID_ARG
    assert lat(p, p, 30, p, p, 0, 2, 300, 4, 20, 0, p, p, big, None) == INVALID_ARG
    assert lat(p, p, 30, p, p, 10, 2, 300, 4, 20, 300, p, p, big, None) == INVALID_ARG           # blank outside [0, V)
    assert lat(p, p, 30, p, p, 10, 2, 300, 4, 20, -1, p, p, big, None) == INVALID_ARG
    assert lat(p, p, 19, p, p, 10, 2, 300, 4, 20, 0, p, p, big, None) == INVALID_ARG             # hyp_stride < Lh
    assert lat(p, p, 0, p, p, 10, 2, 300, 4, 0, 0, p, p, big, None) == INVALID_ARG               # hyp_stride < 1
    for i in (0, 1, 3, 4, 11):                                                                   # a null pointer each
        args = [p, p, 30, p, p, 10, 2, 300, 4, 20, 0, p, p, big, None]
        args[i] = None
        assert lat(*args) == INVALID_ARG, i
    assert lat(p, p, 30, p, p, 10, 2, 300, 4, 20, 0, p, p, 16, None) == WORKSPACE
    assert lat(p, p, 30, p, p, 10, 2, 300, 4, 20, 0, p, None, big, None) == WORKSPACE
    need = lib.pgasr_ctc_hyp_workspace_bytes_wide(10, 2, 300, 4, 20)
    assert lat(p, p, 30, p, p, 10, 2, 300, 4, 20, 0, p, p, need - 1, None) == WORKSPACE

    def gs(**kw):
        a = dict(lp=p, il=p, tl=p, T=10, B=2, V=300, L=3, bl=0, us=p, K=4, cf=p, pa=p, hl=p, Lh=20, es=None, rf=None, ks=None, g=p,
                 ws=p, wb=big, hws=p, hwb=big)
        a.update(kw)
        return lib.pgasr_ctc_grad_from_lattices_seq_wide(*a.values(), None)

    assert gs(V=1025) == UNSUPPORTED and gs(Lh=1024) == UNSUPPORTED and gs(L=1024) == UNSUPPORTED
    assert gs(K=0) == INVALID_ARG and gs(K=17) == INVALID_ARG
    assert gs(V=0) == INVALID_ARG and gs(T=0) == INVALID_ARG and gs(B=0) == INVALID_ARG and gs(Lh=-1) == INVALID_ARG and gs(L=-1) == INVALID_ARG
    assert gs(bl=300) == INVALID_ARG and gs(bl=-1) == INVALID_ARG
    for name in ("lp", "il", "tl", "cf", "hl", "g"):
        assert gs(**{name: None}) == INVALID_ARG, name
    assert gs(rf=p) == INVALID_ARG and gs(ks=p) == INVALID_ARG                   # ref_log_probs without kl_scale and the reverse
    assert gs(pa=None, es=p) == INVALID_ARG and gs(pa=None, rf=p, ks=p) == INVALID_ARG       # the N-best form has no tails
    for tails in (dict(), dict(es=p), dict(rf=p, ks=p), dict(es=p, rf=p, ks=p), dict(pa=None)):
        assert gs(wb=16, **tails) == WORKSPACE and gs(ws=None, **tails) == WORKSPACE
        assert gs(hwb=16, **tails) == WORKSPACE and gs(hws=None, **tails) == WORKSPACE
    # the narrow twins still refuse 65 symbols
    assert lib.pgasr_ctc_hyp_workspace_bytes(10, 2, 65, 4, 20) == 0
    assert lib.pgasr_ctc_hyp_lattice(p, p, 30, p, p, 10, 2, 65, 4, 20, 0, p, p, big, None) == UNSUPPORTED
    assert lib.pgasr_ctc_grad_from_lattices_seq_kl(p, p, p, 10, 2, 65, 3, 0, p, 4, p, p, p, 20, p, p, p, p, p, big, p, big, None) == UNSUPPORTED
    assert lib.pgasr_ctc_grad_from_lattices_seq(p, p, p, 10, 2, 65, 3, 0, p, 4, p, p, p, 20, p, p, big, p, big, None) == UNSUPPORTED
    assert lib.pgasr_ctc_grad_from_lattices_nbest(p, p, p, 10, 2, 65, 3, 0, p, 4, p, p, 20, p, p, big, p, big, None) == UNSUPPORTED


SEQ = dict(score_function="sequence", max_hyp_len=40)
WITH_OBJECTIVES = [dict(num_samples=4), dict(num_samples=4, baseline="leave_one_out"), dict(entropy_weight=0.1), dict(kl_weight=0.1),
                   dict(num_samples=16, baseline="leave_one_out", entropy_weight=0.1, kl_weight=0.2)]
STILL_REFUSED = [("beam", dict(beam=4)), ("reward_unit", dict(reward_unit="word", word_delimiter=3)), ("per_step", dict(per_step=True))]


def _todays_message(name, given, vocab, wide_objectives):
    """The refusals of loss._check_wide as they read before the keyword existed."""
    if wide_objectives:
        return (f"{name}={given!r} takes an alphabet of at most 64 symbols (got {vocab}): above the 64-symbol limit "
                f"wide_objectives=True opens num_samples 1..16, baseline='leave_one_out', entropy_weight and kl_weight, and nothing "
                f"else -- beam=0, score_function='path', reward_unit='char', no per-step rewards")
    return (f"{name}={given!r} takes an alphabet of at most 64 symbols (got {vocab}): above the 64-symbol limit only the default "
            f"objective runs -- num_samples=1, baseline='hypothesis', beam=0, score_function='path', entropy_weight=0, kl_weight=0, "
            f"reward_unit='char', no per-step rewards")


@pytest.mark.parametrize("vocab", [65, 1024])
def test_wide_sequence_admits_the_sequence_score_function(vocab):
    for fields in (dict(score_function="sequence"), SEQ):
        opt = check_options(PGOptions(**fields), vocab=vocab, frames=100, symbols=12, wide_sequence=True)
        assert opt.score_function == "sequence" and opt.num_samples == 1 and opt.max_hyp_len == fields.get("max_hyp_len")
    for more in WITH_OBJECTIVES:
        opt = check_options(PGOptions(**SEQ, **more), vocab=vocab, frames=100, symbols=12, wide_sequence=True, wide_objectives=True)
        assert opt.score_function == "sequence" and opt.num_samples == more.get("num_samples", 1)
        # without wide_objectives only K = 1 against the greedy hypothesis is admitted: the other option is named
        name = "baseline" if "baseline" in more else next(iter(more))
        with pytest.raises(ValueError, match=name + "=") as e:
            check_options(PGOptions(**SEQ, **more), vocab=vocab, frames=100, symbols=12, wide_sequence=True)
        assert "wide_objectives=True" in str(e.value)
    check_options(PGOptions(), vocab=vocab, wide_sequence=True)                                  # the default objective, as ever
    with pytest.raises(ValueError, match="1025"):
        check_options(PGOptions(**SEQ), vocab=1025, wide_sequence=True)
    with pytest.raises(ValueError, match="per_step"):                                            # the options' own rules hold with it
        check_options(PGOptions(per_step=True, **SEQ), vocab=vocab, wide_sequence=True)


@pytest.mark.parametrize("name,fields", STILL_REFUSED)
def test_wide_sequence_still_refuses_the_rest_by_name(name, fields):
    for vocab in (65, 1024):
        for objectives in (False, True):
            for more in ({}, SEQ) if name != "per_step" else ({},):
                with pytest.raises(ValueError, match=name + "=") as e:
                    check_options(PGOptions(**fields, **more), vocab=vocab, frames=100, symbols=12, wide_sequence=True,
                                  wide_objectives=objectives)
                assert "64" in str(e.value) and "wide_sequence=True" in str(e.value)
    check_options(PGOptions(**fields), vocab=64, frames=100, symbols=12, wide_sequence=True)


def test_nothing_changes_without_the_keyword_or_at_64_symbols():
    cases = [("score_function", "sequence", dict(score_function="sequence")), ("beam", 4, dict(beam=4)),
             ("num_samples", 2, dict(num_samples=2)), ("entropy_weight", 0.1, dict(entropy_weight=0.1))]
    for vocab in (65, 300):
        for objectives in (False, True):
            for name, given, fields in cases:
                if objectives and name in ("num_samples", "entropy_weight"):
                    continue
                with pytest.raises(ValueError) as e:
                    check_options(PGOptions(**fields), vocab=vocab, frames=100, symbols=12, wide_objectives=objectives)
                assert str(e.value) == _todays_message(name, given, vocab, objectives)
                with pytest.raises(ValueError) as e2:
                    check_options(PGOptions(**fields), vocab=vocab, frames=100, symbols=12, wide_objectives=objectives, wide_sequence=False)
                assert str(e2.value) == str(e.value)
    for fields in (dict(), SEQ, dict(beam=4, **SEQ), dict(reward_unit="word", word_delimiter=3), dict(per_step=True), dict(num_samples=4)):
        a = check_options(PGOptions(**fields), vocab=64, frames=100, symbols=12)
        assert check_options(PGOptions(**fields), vocab=64, frames=100, symbols=12, wide_sequence=True) == a


def _toy(V):
    import torch

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.head = torch.nn.Linear(4, V)

        def logits(self, x, fmask, lengths=None):
            raise NotImplementedError

    return Toy()


def test_trainers_take_wide_sequence():
    from types import SimpleNamespace
    from policy_gradient_asr_amd.mwer import MWERTrainer, MWEROptions, MWERWideOptions, check_mwer_options
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer

    with pytest.raises(ValueError, match="wide_alphabet"):
        PolicyGradientTrainer(_toy(300), wide_sequence=True)
    tr = PolicyGradientTrainer(_toy(300), wide_alphabet=True, wide_sequence=True, score_function="sequence", max_hyp_len=40)
    assert tr.wide_sequence and tr.MAX_VOCAB == 1024 and tr._checked_options(frames=100, symbols=12).score_function == "sequence"
    assert PolicyGradientTrainer(_toy(300), wide_alphabet=True).wide_sequence is False
    with pytest.raises(ValueError, match="num_samples"):
        PolicyGradientTrainer(_toy(300), wide_alphabet=True, wide_sequence=True, score_function="sequence", num_samples=2)
    tr = PolicyGradientTrainer(_toy(1024), wide_alphabet=True, wide_sequence=True, wide_objectives=True, score_function="sequence",
                               num_samples=4, reward_baseline="leave_one_out", entropy_weight=0.1)
    assert tr._checked_options(frames=100, symbols=12).num_samples == 4
    with pytest.raises(ValueError, match="score_function"):                                      # without the keyword: as ever
        PolicyGradientTrainer(_toy(300), wide_alphabet=True, wide_objectives=True, score_function="sequence")
    for name, kw in (("beam", dict(reward_decoder="beam")), ("reward_unit", dict(reward_unit="word", word_delimiter=3)),
                     ("per_step", dict(reward_mode="per_step"))):
        with pytest.raises(ValueError, match=name):
            PolicyGradientTrainer(_toy(300), wide_alphabet=True, wide_sequence=True, **kw)

    tr = MWERTrainer(_toy(300), wide_sequence=True)
    assert tr.MAX_VOCAB == 1024 and tr.wide_sequence and isinstance(tr.mwer_options, MWERWideOptions) and tr.mwer_options.wide and tr.mwer_unit_lm is None
    assert tr._list_fields() == {"wide_sequence": True, "unit_lm": None}
    assert MWERTrainer(_toy(1024), wide_sequence=True, beam_size=128, nbest=16).nbest == 16
    with pytest.raises(ValueError, match="risk_unit"):
        MWERTrainer(_toy(300), wide_sequence=True, risk_unit="word", word_delimiter=3)
    with pytest.raises(ValueError, match="unit_lm="):
        MWERTrainer(_toy(300), wide_sequence=True, lm=SimpleNamespace(vocab=300, blank=0))
    with pytest.raises(ValueError, match="beam"):
        MWERTrainer(_toy(300), wide_sequence=True, beam_size=129)
    with pytest.raises(ValueError, match="nbest"):
        MWERTrainer(_toy(300), wide_sequence=True, beam_size=32, nbest=17)
    with pytest.raises(ValueError, match="1025"):
        MWERTrainer(_toy(1025), wide_sequence=True)
    with pytest.raises(ValueError, match="wide_sequence"):
        MWERTrainer(_toy(29), unit_lm=SimpleNamespace())
    # wide_alphabet=True without the keyword keeps raising the message it raises
    with pytest.raises(ValueError) as e:
        MWERTrainer(_toy(29), wide_alphabet=True)
    assert str(e.value) == ("MWERTrainer takes an alphabet of at most 64 symbols: the beam search and the N-best kernels hold one "
                            "symbol per lane (wide_alphabet=True is PolicyGradientTrainer's default objective only)")
    # at most 64 symbols the keyword leaves the trainer's calls as they were: the narrow list, the word risk, the dense LM
    tr = MWERTrainer(_toy(29), wide_sequence=True, risk_unit="word", word_delimiter=3)
    assert tr.risk_unit == "word"
    from policy_gradient_asr_amd.mwer import _wide_list
    assert not _wide_list(tr.mwer_options, 29) and not _wide_list(tr.mwer_options, 64) and _wide_list(tr.mwer_options, 65)
    assert not _wide_list(MWEROptions(), 300)
    assert check_mwer_options(MWEROptions(), vocab=29) == MWEROptions()
    with pytest.raises(ValueError, match="wide_sequence=True"):
        check_mwer_options(MWEROptions(), vocab=65)


def test_wrappers_route_by_vocab_and_refuse_cpu_tensors():
    import torch
    from policy_gradient_asr_amd import _lib
    from policy_gradient_asr_amd.mwer import mwer_ctc_loss, mwer_ctc_loss_lm
    assert hipops.ctc_hyp_workspace_bytes(48, 3, 64, 4, 20) == hipops.ctc_hyp_workspace_bytes(48, 3, 64, 4, 20, wide=True) > 0
    assert hipops.ctc_hyp_workspace_bytes(48, 3, 65, 4, 20) == hipops.ctc_hyp_workspace_bytes(48, 3, 65, 4, 20, wide=True) > 0
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    lp = torch.zeros(6, 2, 300)
    handle, hyp_handle = (torch.zeros(256, dtype=torch.uint8), 3, 0), (torch.zeros(256, dtype=torch.uint8), 2, 4)
    for call in (lambda: hipops.ctc_hyp_workspace_bytes(48, 3, 65, 4, 20, wide=False),
                 lambda: hipops.ctc_hyp_lattice(lp, i32(2, 2, 6), i32(2, 2), i32(2), 4, wide=False),
                 lambda: hipops.ctc_hyp_lattice(lp, i32(2, 2, 6), i32(2, 2), i32(2), 4),                  # CPU tensors
                 lambda: hipops.ctc_grad_from_lattices_seq(lp, i32(2), i32(2), handle, hyp_handle, torch.zeros(2), torch.zeros(2, 2),
                                                           i32(2, 6, 2), i32(2, 2), wide=False),
                 lambda: hipops.ctc_grad_from_lattices_seq(lp, i32(2), i32(2), handle, hyp_handle, torch.zeros(2), torch.zeros(2, 2),
                                                           i32(2, 6, 2), i32(2, 2)),
                 lambda: hipops.ctc_grad_from_lattices_nbest(lp, i32(2), i32(2), handle, hyp_handle, torch.zeros(2), torch.zeros(2, 2),
                                                             i32(2, 2), wide=False),
                 lambda: hipops.ctc_grad_from_lattices_nbest(lp, i32(2), i32(2), handle, hyp_handle, torch.zeros(2), torch.zeros(2, 2),
                                                             i32(2, 2)),
                 lambda: mwer_ctc_loss_lm(lp, i32(2), i32(2, 3), i32(2), beam=4, nbest=2, wide_sequence=True)):
        with pytest.raises(_lib.PgasrError):
            call()
    with pytest.raises(ValueError, match="wide_sequence=True"):
        mwer_ctc_loss(lp, i32(2), i32(2, 3), i32(2), beam=4, nbest=2)
