"""Alphabets of 65 .. 1024 symbols on the device: the four wide kernels (csrc/wide_vocab.hip and the wide pair of csrc/ctc.hip)
against fp64 statements, the wide entries against the narrow ones where both run (V <= 64), and the default objective, a trainer
step, greedy decoding and the drivers at V = 300 / 101.

Bounds (none of them comes from the kernels under test):
    log-softmax  |err| <= 4 eps32 max(|x|_max, |lse|) + 2e-6: the roundings of x - max, max + log(sum) and x - lse at the magnitude
                 of the row, and 2e-6 for the fast exp / log of a sum of at most 1024 terms in [1, V] (tests/test_kernels_gpu.py
                 holds no bound of its own for the narrow kernel; tests/test_dense_lstm_gpu.py holds it to 1e-5 on N(0,1) rows,
                 which this is inside of)
    arg-max      exact
    sampler      tests/test_kernels_gpu.py::test_argmax_bit_exact_and_sampler's rule: equal to oracle.decode_ref.sample_paths but
                 where u lies within 2e-6 of a cdf boundary, at most max(1, rows // 1000) such rows
    CTC          tests/test_ctc_numerics_gpu.py's bounds without their e32 allowance: nll 1e-5 |nll| + 2e-7 T, gradient 5e-5 on
                 the unscaled entries
    step         the small-shape step tests' (tests/test_train_step_gpu.py): f32 loss 1e-5, parameter gradients 1e-4 (max norm),
                 logits 1e-5; bf16x3 1e-3."""
import functools

import numpy as np
import pytest
import torch

import ctc_cases as cc
from frame_rows_ref import lsm_check as _lsm_check
from oracle import ctc_ref, decode_ref, model_ref, pg_ref
from pg_harness import DEV, load_params, make_batch, param_errs, rel_err

pytestmark = pytest.mark.gpu

WIDE_V = [65, 128, 129, 257, 1024]          # NV = 2, 2, 4, 8, 16; 65 / 129 / 257 end in a ragged group
SHAPES = [(1, 1), (17, 3), (33, 5)]
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def ops():
    from policy_gradient_asr_amd import hipops
    return hipops


# ---- log-softmax ----
# the check and its bound live in tests/frame_rows_ref.py, which holds the narrow kernel to the same


@pytest.mark.parametrize("V", WIDE_V)
def test_log_softmax_vs_fp64(ops, V):
    g = torch.Generator().manual_seed(V)
    for T, B in SHAPES:
        x = torch.randn(T, B, V, generator=g) * 3
        x[0, 0, :] = 0.0
        x[-1, -1, V // 2] = 80.0                    # a saturated row
        if T > 1:
            x[1, 0, ::3] = -float("inf")            # p = 0 entries, the last partial group included
            x[1, 0, V - 1] = -float("inf")
        _lsm_check(ops, x, f"V={V} T={T} B={B}", DEV)


def test_log_softmax_maximum_in_the_last_column(ops):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(17, 3, 65, generator=g)
    x[:, :, 64] += 12.0                             # the one label of lane 32's group, alone in the ragged tail
    _lsm_check(ops, x, "V=65 max last", DEV)
    # misaligned tensors take the scalar loads: a view that starts 4 bytes into the allocation
    base = torch.randn(5 * 128 + 1, generator=g).to(DEV)
    x = base[1:].view(5, 1, 128)
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    got = ops.log_softmax_rows(x)
    want = torch.log_softmax(x.double().cpu(), -1)
    assert float((got.cpu().double() - want).abs().max()) <= 4 * EPS32 * 8 + 2e-6


# ---- arg-max ----
@pytest.mark.parametrize("V", WIDE_V)
def test_argmax_first_maximum_wins(ops, V):
    g = torch.Generator().manual_seed(V + 1)
    nv = next(n for n in (1, 2, 4, 8, 16) if 64 * n >= V)
    for T, B in SHAPES:
        x = torch.randn(T, B, V, generator=g) * 3
        x[0, 0, :] = 0.5                                            # every label ties: label 0
        if T > 1:
            x[1, 0, nv * 3] = x[1, 0, nv * 3 + nv - 1] = 9.0        # a tie inside one lane's group
            x[2, 0, nv * 5 + 1] = x[2, 0, nv * 2 + 1] = 9.0         # across lanes
            x[3, 0, V - 1] = x[3, 0, ((V - 1) // nv) * nv] = 9.0    # inside the last, partial group (one label wide at 65, 129, 257)
            x[4, 0, V - 1] = x[4, 0, 7] = 9.0                       # the last label against an early one
            x[5, 0, V - 1] = 9.0                                    # the last label alone
        greedy, _ = ops.frame_argmax_sample(x.to(DEV), want_sample=False)
        assert np.array_equal(greedy.cpu().numpy(), np.argmax(x.numpy(), axis=2))


# ---- sampler ----
SEED, OFFSET, BOUND = 0xDEADBEEF1234, 3, 2e-6


@functools.lru_cache(maxsize=None)
def _sampler_scores(V, kind):
    g = torch.Generator().manual_seed(V * 7 + len(kind))
    if kind == "const":
        return torch.full((40, 8, V), 0.25)
    return torch.randn(40, 8, V, generator=g) * (3.0 if kind == "wide" else 0.5)


@functools.lru_cache(maxsize=None)
def _oracle_samples(V, kind):
    return decode_ref.sample_paths(_sampler_scores(V, kind).numpy(), seed=SEED, offset=OFFSET)


def _sampler_mismatches(s, paths, cdf, u):
    diff = np.argwhere(s != paths)
    worst = 0.0
    for t, b in diff:
        k = min(s[t, b], paths[t, b])
        worst = max(worst, abs(cdf[t, b, k] - u[t, b]))
        assert abs(cdf[t, b, k] - u[t, b]) < BOUND, (t, b, s[t, b], paths[t, b])
    assert len(diff) <= max(1, s.size // 1000)
    return len(diff), worst


@pytest.mark.parametrize("kind", ["wide", "flat", "const"])
@pytest.mark.parametrize("V", WIDE_V)
def test_sampler_vs_oracle(ops, V, kind):
    scores = _sampler_scores(V, kind)
    _, sample = ops.frame_argmax_sample(scores.to(DEV), seed=SEED, offset=OFFSET, want_greedy=False)
    s = sample.cpu().numpy()
    assert s.min() >= 0 and s.max() < V
    paths, cdf, u = _oracle_samples(V, kind)
    n, worst = _sampler_mismatches(s, paths, cdf, u)
    print(f"[wide sampler] V={V} {kind}: {n} of {s.size} rows differ from the fp64 oracle (largest |cdf - u| there {worst:.2e})")


@pytest.mark.parametrize("V", [65, 1024])
def test_sampler_addressing(ops, V):
    """Halves of a batch (batch_stride / batch_offset) and interleaved ids (utt_ids) draw the whole batch's samples; a row beyond
    the global batch draws from its own domain, the same with either addressing."""
    scores = _sampler_scores(V, "wide").to(DEV)
    T, B, _ = scores.shape
    _, whole = ops.frame_argmax_sample(scores, seed=SEED, offset=OFFSET, want_greedy=False)
    half = B // 2
    for h in range(2):
        part = scores[:, half * h:half * h + half].contiguous()
        _, got = ops.frame_argmax_sample(part, seed=SEED, offset=OFFSET, want_greedy=False, batch_stride=B, batch_offset=half * h)
        assert torch.equal(got, whole[:, half * h:half * h + half])
    for rows in ([0, 2, 4, 6], [7, 5, 3, 1]):
        ids = torch.tensor(rows, dtype=torch.int32, device=DEV)
        part = scores[:, rows].contiguous()
        _, got = ops.frame_argmax_sample(part, seed=SEED, offset=OFFSET, want_greedy=False, batch_stride=B, utt_ids=ids)
        assert torch.equal(got, whole[:, rows])
    # rows 2, 3 of a padded shard lie beyond a global batch of 6: local rows 2, 3 with base 4 <-> ids 4, 5, -1, 9
    part = scores[:, 4:8].contiguous()
    _, by_base = ops.frame_argmax_sample(part, seed=SEED, offset=OFFSET, want_greedy=False, batch_stride=6, batch_offset=4)
    ids = torch.tensor([4, 5, -1, 9], dtype=torch.int32, device=DEV)
    _, by_ids = ops.frame_argmax_sample(part, seed=SEED, offset=OFFSET, want_greedy=False, batch_stride=6, utt_ids=ids)
    assert torch.equal(by_base, by_ids)
    _, six = ops.frame_argmax_sample(scores[:, :6].contiguous(), seed=SEED, offset=OFFSET, want_greedy=False)
    assert torch.equal(by_base[:, :2], six[:, 4:6]) and not torch.equal(by_base[:, 2:], whole[:, 6:8])


@pytest.mark.parametrize("V", [2, 29, 64])
def test_narrow_rows_through_the_wide_kernels(ops, V):
    """V <= 64 through the wide entries: the arg-max is the narrow kernel's, the samples are its samples except at a cdf boundary
    (with one label per lane the cdf is the narrow kernel's scan), log-softmax agrees to the bound above."""
    g = torch.Generator().manual_seed(V)
    cpu = torch.randn(33, 5, V, generator=g) * 3
    scores = cpu.to(DEV)
    g_n, s_n = ops.frame_argmax_sample(scores, seed=SEED, offset=OFFSET)
    g_w, s_w = ops.frame_argmax_sample(scores, seed=SEED, offset=OFFSET, wide=True)
    assert torch.equal(g_n, g_w)
    # where the two differ, both must be at a boundary of the oracle's cdf for the oracle's u: the u is the same
    paths, cdf, u = decode_ref.sample_paths(cpu.numpy(), seed=SEED, offset=OFFSET)
    n_w, _ = _sampler_mismatches(s_w.cpu().numpy(), paths, cdf, u)
    n_n, _ = _sampler_mismatches(s_n.cpu().numpy(), paths, cdf, u)
    print(f"[wide sampler] V={V}: wide == narrow samples: {torch.equal(s_n, s_w)} (rows off the oracle: wide {n_w}, narrow {n_n})")
    # shards and rows beyond the global batch: the same counters in both kernels (rows 4 of 5 lie beyond a global batch of 7 at base 3)
    kw = dict(seed=SEED, offset=OFFSET, batch_stride=7, batch_offset=3, want_greedy=False)
    _, a_n = ops.frame_argmax_sample(scores, **kw)
    _, a_w = ops.frame_argmax_sample(scores, wide=True, **kw)
    assert int((a_n != a_w).sum()) <= max(1, a_n.numel() // 1000)
    assert not torch.equal(a_n, s_n)
    got = ops.log_softmax_rows(scores, wide=True).cpu().double()
    assert float((got - torch.log_softmax(cpu.double(), 2)).abs().max()) <= 4 * EPS32 * 16 + 2e-6


# ---- CTC ----
def _ctc_bounds(nll_ref, T):
    return 1e-5 * np.abs(nll_ref) + 2e-7 * T, 5e-5


@functools.lru_cache(maxsize=None)
def _ctc_case(V, blank_last):
    """T = 40, B = 4, L <= 12: utterance 0 full length with labels of the row's last (partial) group; 1 a target of one repeated
    label; 2 empty (no frames and no labels; with blank = V - 1: frames and no labels); 3 infeasible (12 labels, 5 frames)."""
    blank = V - 1 if blank_last else 0
    T, B, L = 40, 4, 12
    rng = np.random.default_rng(V + blank)
    logits = (rng.normal(size=(T, B, V)) * 2).astype(np.float32)
    symbols = np.array([v for v in range(V) if v != blank])
    targets = rng.choice(symbols, size=(B, L)).astype(np.int32)
    targets[0, :4] = symbols[[-1, -2, -1, 0]]             # the last labels of the row, one of them twice with a label between
    targets[0, 6] = targets[0, 5]                         # and an adjacent repeat
    targets[1, :] = symbols[len(symbols) // 2]
    il = np.array([40, 33, 17 if blank_last else 0, 5], np.int32)
    tl = np.array([12, 6, 0, 12], np.int32)
    ok = [0, 1] + ([2] if blank_last else [])             # what torch's ctc_loss takes: frames, and an alignment
    nll_t, grad_t = cc.torch_ctc(logits[:, ok], targets[ok], il[ok], tl[ok], blank, torch.float64)
    nll = np.array([0.0, 0.0, 0.0, np.inf]); grad = np.zeros((T, B, V))
    nll[ok] = nll_t; grad[:, ok] = grad_t
    # the project's oracle says the same, the two special utterances included
    nll_o, grad_o = ctc_ref.ctc_loss_and_grad(logits, targets, il, tl, blank=blank)
    assert np.array_equal(np.isinf(nll_o), np.isinf(nll)) and np.abs(grad_o - grad).max() < 1e-9
    for a in (logits, targets, il, tl, nll, grad):
        a.setflags(write=False)
    return dict(logits=logits, targets=targets, il=il, tl=tl, blank=blank, nll=nll, grad=grad, T=T, B=B, V=V)


def _dev(*arrays):
    return tuple(torch.tensor(np.asarray(a)).to(DEV) for a in arrays)


@pytest.mark.parametrize("blank_last", [False, True])
@pytest.mark.parametrize("V", WIDE_V)
def test_ctc_loss_grad_vs_torch_fp64(ops, V, blank_last):
    c = _ctc_case(V, blank_last)
    lp = torch.log_softmax(torch.tensor(c["logits"]), 2).to(DEV)
    tg, il, tl = _dev(c["targets"], c["il"], c["tl"])
    nll, grad = ops.ctc_loss_grad(lp, tg, il, tl, blank=c["blank"])
    nll2, grad2 = ops.ctc_loss_grad(lp, tg, il, tl, blank=c["blank"])
    assert torch.equal(nll, nll2) and torch.equal(grad, grad2)              # two runs, the same bits
    nll, grad = nll.cpu().numpy().astype(np.float64), grad.cpu().numpy().astype(np.float64)
    fin = np.isfinite(c["nll"])
    b_nll, b_grad = _ctc_bounds(c["nll"][fin], c["T"])
    err_nll, err_grad = np.abs(nll[fin] - c["nll"][fin]), float(np.abs(grad - c["grad"]).max())
    print(f"[wide ctc] V={V} blank={c['blank']}: nll err / bound {float((err_nll / b_nll).max()):.2f} (largest err {err_nll.max():.2e}); "
          f"grad err {err_grad:.2e} (bound {b_grad:.0e})")
    assert np.array_equal(np.isinf(nll), ~fin) and np.isfinite(grad).all()
    assert (err_nll <= b_nll).all() and err_grad <= b_grad
    assert (grad[:, 3] == 0).all()                                           # the infeasible utterance
    for b in range(c["B"]):
        assert (grad[int(c["il"][b]):, b] == 0).all()
    assert np.abs(c["grad"][:, 0]).max() > 0.1 and np.abs(c["grad"][:, 1]).max() > 0.1


@pytest.mark.parametrize("V", [129, 1024])
def test_ctc_fused_reinforce_term_vs_fp64(ops, V):
    """utt_scale_b (p - occ) + coef (p - onehot(path)), the coefficient per utterance and per frame, on the split call."""
    c = _ctc_case(V, False)
    T, B = c["T"], c["B"]
    lp = torch.log_softmax(torch.tensor(c["logits"]), 2).to(DEV)
    tg, il, tl = _dev(c["targets"], c["il"], c["tl"])
    rng = np.random.default_rng(3)
    path = rng.integers(0, V, size=(T, B)).astype(np.int32)
    path[0, 0], path[1, 0] = V - 1, 0
    us = np.array([0.5, 0.3, 0.7, 0.2])
    p = np.exp(ctc_ref.log_softmax(c["logits"].astype(np.float64), axis=2))
    onehot = np.zeros_like(p); np.put_along_axis(onehot, path[:, :, None].astype(np.int64), 1.0, axis=2)
    live = (np.arange(T)[:, None] < c["il"][None, :])[:, :, None]
    nll, handle = ops.ctc_lattice(lp, tg, il, tl)
    for label, coef in (("per utterance", np.array([0.3, -0.7, 1.5, 0.4])), ("per frame", rng.normal(size=(T, B)))):
        cf = coef[None, :, None] if coef.ndim == 1 else coef[:, :, None]
        want = (c["grad"] * us[None, :, None] + cf * (p - onehot)) * live
        us_d, coef_d, path_d = _dev(us.astype(np.float32), coef.astype(np.float32), path)
        got = ops.ctc_grad_from_lattice(lp, il, tl, handle, utt_scale=us_d, pg_coef=coef_d, pg_path=path_d)
        again = ops.ctc_grad_from_lattice(lp, il, tl, handle, utt_scale=us_d, pg_coef=coef_d, pg_path=path_d)
        assert torch.equal(got, again)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        # the unscaled entries' bound, times the magnitudes the two parts are scaled by (fp32 coefficients: 1 ulp more)
        bound = 5e-5 * (us.max() + np.abs(coef).max())
        print(f"[wide ctc] V={V} fused term, coefficient {label}: err {err:.2e} (bound {bound:.2e})")
        assert err <= bound
        if coef.ndim == 1:
            _, one = ops.ctc_loss_grad(lp, tg, il, tl, utt_scale=us_d, pg_coef=coef_d, pg_path=path_d)
            assert torch.equal(one, got)                                     # the one-call form is the split call


def test_ctc_two_states_per_thread(ops):
    """L = 130 (S = 261 > 256): the NSPT = 2 lattice under the wide label lists and gradient pass."""
    logits, targets, il, tl = cc.planted(T=300, B=1, V=257, L=130, seed=2, scale=6.0)
    nll_w, grad_w = cc.torch_ctc(logits, targets, il, tl, 0, torch.float64)
    lp = torch.log_softmax(torch.tensor(logits), 2).to(DEV)
    nll, grad = ops.ctc_loss_grad(lp, *_dev(targets, il, tl))
    b_nll, b_grad = _ctc_bounds(nll_w, 300)
    err = float(np.abs(grad.cpu().numpy().astype(np.float64) - grad_w).max())
    print(f"[wide ctc] NSPT=2: nll err {abs(float(nll[0]) - nll_w[0]):.2e} (bound {b_nll[0]:.2e}); grad err {err:.2e}")
    assert abs(float(nll[0]) - nll_w[0]) <= b_nll[0] and err <= b_grad


def test_ctc_zero_probabilities(ops):
    """log p = -inf exactly, for the blank, a label of the target and a symbol outside it, the last label of the row among them:
    occupancy 0, gradient entry 0, no NaN anywhere."""
    V = 129
    logits, targets, il, tl = cc.planted(T=30, B=2, V=V, L=4, seed=3, scale=5.0)
    targets = targets.copy(); logits = logits.copy()
    peak = logits.argmax(axis=2)
    label = int(targets[0, 1])
    outside = V - 1 if V - 1 not in targets[1] else next(v for v in range(1, V) if v not in targets[1])
    t_blank = next(t for t in range(5, 30) if peak[t, 0] != 0)
    t_label = next(t for t in range(7, 30) if peak[t, 0] not in (0, label) and t != t_blank)
    masked = [(t_blank, 0, 0), (t_label, 0, label), (9, 1, outside)]
    for t, b, v in masked:
        logits[t, b, v] = -np.inf
    nll_w, grad_w = ctc_ref.ctc_loss_and_grad(logits, targets, il, tl)
    assert np.isfinite(nll_w).all() and np.isfinite(grad_w).all()
    lp = torch.log_softmax(torch.tensor(logits), 2)
    assert int(torch.isinf(lp).sum()) == len(masked)
    nll, grad = ops.ctc_loss_grad(lp.to(DEV), *_dev(targets, il, tl))
    nll, grad = nll.cpu().numpy().astype(np.float64), grad.cpu().numpy().astype(np.float64)
    b_nll, b_grad = _ctc_bounds(nll_w, 30)
    assert np.isfinite(nll).all() and np.isfinite(grad).all()
    assert (np.abs(nll - nll_w) <= b_nll).all() and np.abs(grad - grad_w).max() <= b_grad
    for t, b, v in masked:
        assert grad[t, b, v] == 0.0
    # a target label at -inf on every frame: no alignment, nll = +inf, a zero gradient
    logits[:, 0, label] = -np.inf
    nll, grad = ops.ctc_loss_grad(torch.log_softmax(torch.tensor(logits), 2).to(DEV), *_dev(targets, il, tl))
    assert torch.isinf(nll[0]) and torch.isfinite(nll[1]) and torch.isfinite(grad).all() and (grad[:, 0] == 0).all()


@pytest.mark.parametrize("V", [2, 29, 64])
def test_ctc_wide_entries_against_the_narrow_ones(ops, V):
    """The same lattice kernel: nll bit for bit.  The gradient pass adds the same terms in the same order: within 1e-7."""
    L = 1 if V == 2 else 10
    logits, targets, il, tl = cc.planted(T=64, B=4, V=V, L=L, seed=V, scale=4.0, il=[64, 63, 50, 41], tl=[L, L, max(L - 3, 0), 1],
                                         repeats=V > 2)
    lp = torch.log_softmax(torch.tensor(logits), 2).to(DEV)
    tg, ild, tld = _dev(targets, il, tl)
    rng = np.random.default_rng(V)
    us, coef, path = _dev(rng.uniform(0.1, 0.5, 4).astype(np.float32), rng.normal(size=4).astype(np.float32),
                          rng.integers(0, V, size=(64, 4)).astype(np.int32))
    n_n, g_n = ops.ctc_loss_grad(lp, tg, ild, tld, utt_scale=us, pg_coef=coef, pg_path=path)
    n_w, g_w = ops.ctc_loss_grad(lp, tg, ild, tld, utt_scale=us, pg_coef=coef, pg_path=path, wide=True)
    assert torch.equal(n_n, n_w)
    print(f"[wide ctc] V={V}: wide gradient bit-equal to the narrow one: {torch.equal(g_n, g_w)}; max diff {float((g_n - g_w).abs().max()):.1e}")
    assert float((g_n - g_w).abs().max()) <= 1e-7
    # either pass runs over the other's lattice (one workspace format)
    _, h_n = ops.ctc_lattice(lp, tg, ild, tld)
    g_x = ops.ctc_grad_from_lattice(lp, ild, tld, h_n, utt_scale=us, pg_coef=coef, pg_path=path, wide=True)
    _, h_w = ops.ctc_lattice(lp, tg, ild, tld, wide=True)
    g_y = ops.ctc_grad_from_lattice(lp, ild, tld, h_w, utt_scale=us, pg_coef=coef, pg_path=path, wide=False)
    assert torch.equal(g_x, g_w) and torch.equal(g_y, g_n)


# ---- the objective, a trainer step, decoding, the drivers ----
STEP = dict(B=4, F=80, T=120, V=300, L=12, lens=[120, 90, 120, 64], tlens=[12, 9, 12, 5])


@functools.lru_cache(maxsize=None)
def _step_inputs():
    s = STEP
    batch = make_batch(s["B"], s["F"], s["T"], s["V"], s["L"], s["lens"], s["tlens"], 61)
    return batch, model_ref.init_params(n_feats=s["F"], vocab=s["V"], seed=62)


@pytest.mark.parametrize("lam", [0.0, 1.0])
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_trainer_step_at_300_symbols_vs_oracle(mode, lam):
    """One eval-mode step of the whole model through PolicyGradientTrainer(wide_alphabet=True) against the torch-CPU model in fp64
    on the same weights (the lines of tests/test_train_step_gpu.py::_pg_step_vs_oracle that this shape needs).  The device makes
    its discrete choices on ITS logits, the oracle on its own; the two logit tensors differ by the mode's bound e (1e-5 / 1e-3), so
    a frame's sampled label can differ where u lies within ~e |z| of a cdf step and its arg-max where the two best scores do:
    at most 1 + 2 e max|z| frames of each kind may differ, and the oracle then takes the device's labels there -- everything
    downstream of the choices (collapse, edit distance, rewards, loss, d(logits), the backward pass) is its own."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.model import Seq2Seq
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    s = STEP
    (x, targets, fmask, tmask), p = _step_inputs()
    tol_loss, tol_grad, tol_logits = (1e-5, 1e-4, 1e-5) if mode == "f32" else (1e-3, 1e-3, 1e-3)
    pr = {k: v.double().requires_grad_(True) for k, v in p.items()}
    m = load_params(Seq2Seq(s["V"], n_feats=s["F"]), p).to(DEV).eval()
    batch = tuple(t_.to(DEV) for t_ in (x, targets, fmask, tmask))
    with hipops.precision(mode):
        tr = PolicyGradientTrainer(m, lam=lam, seed=3, wide_alphabet=True)
        loss = tr.compute_gradients(*batch)
        nll, R_s, R_b = tr.last_stats
        torch.cuda.synchronize()
        hipops.lstm_assert_no_timeouts()
        with torch.no_grad():
            logits, in_len = m.logits(batch[0], batch[2])
    enc = model_ref.encoder_forward_torch(pr, x.double(), fmask, packed=True)
    logits_ref = model_ref.head_logits_torch(pr, enc)
    e_logits = rel_err(logits.cpu(), logits_ref.detach())
    assert e_logits < tol_logits, e_logits
    lg = logits_ref.detach().numpy()
    il, tl_ = np.array(s["lens"]), np.array(s["tlens"])
    paths, _, _ = decode_ref.sample_paths(lg, seed=3, offset=1)
    greedy_frames = np.argmax(lg, axis=2)
    lp_dev = hipops.log_softmax_rows(logits.contiguous())
    d_greedy, d_sample = (t_.cpu().numpy().astype(np.int64) for t_ in hipops.frame_argmax_sample(lp_dev, seed=3, offset=1))
    fm = np.arange(s["T"])[:, None] < il[None, :]
    n_s, n_g = int(((d_sample != paths) & fm).sum()), int(((d_greedy != greedy_frames) & fm).sum())
    allowed = 1 + int(2 * tol_logits * np.abs(lg).max() * fm.sum())
    print(f"[wide step] {mode} lam={lam}: logits rel err {e_logits:.2e}; frame labels that differ: sampled {n_s}, arg-max {n_g} "
          f"of {int(fm.sum())} (allowed {allowed})")
    assert n_s <= allowed and n_g <= allowed
    paths, greedy_frames = np.where(fm, d_sample, paths), np.where(fm, d_greedy, greedy_frames)
    o = pg_ref.pg_objective(lg, il, targets.numpy(), tl_, lam=lam, paths=paths, greedy_frames=greedy_frames)
    np.testing.assert_allclose(R_b.cpu().numpy(), o.R_hyp, rtol=1e-6)
    np.testing.assert_allclose(R_s.cpu().numpy(), o.R[0], rtol=1e-6)
    lerr = abs(float(loss) - o.loss) / abs(o.loss)
    logits_ref.backward(torch.from_numpy(o.grad))
    errs = param_errs(m, {k: v.grad for k, v in pr.items()})
    worst = max(errs, key=errs.get)
    print(f"[wide step] {mode} lam={lam}: loss rel err {lerr:.2e}; worst parameter gradient {worst} {errs[worst]:.2e}")
    assert lerr < tol_loss, (float(loss), o.loss)
    assert errs[worst] < tol_grad, (worst, errs[worst])


def test_pg_ctc_loss_at_300_symbols_vs_oracle():
    """loss.pg_ctc_loss on given logits (no model): loss, rewards and d(logits) against oracle.pg_ref at lam = 0 and 1; CTCLoss is
    the lam = 0 call."""
    from policy_gradient_asr_amd.loss import CTCLoss, pg_ctc_loss
    T, B, V, L = 120, 4, 300, 12
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(T, B, V, generator=g) * 2
    targets = torch.randint(1, V, (B, L), generator=g, dtype=torch.int32)
    il, tl = np.array([120, 90, 120, 64]), np.array([12, 9, 12, 5])
    ild, tld = _dev(il.astype(np.int32), tl.astype(np.int32))
    for lam in (0.0, 1.0):
        z = logits.to(DEV).requires_grad_(True)
        loss, nll, R_s, R_g = pg_ctc_loss(z, ild, targets.to(DEV), tld, lam=lam, seed=3, offset=1)
        loss.backward()
        o = pg_ref.pg_objective(logits.double().numpy(), il, targets.numpy(), tl, lam=lam, seed=3, offset=1)
        np.testing.assert_allclose(R_g.cpu().numpy(), o.R_hyp, rtol=1e-6)
        np.testing.assert_allclose(R_s.cpu().numpy(), o.R[0], rtol=1e-6)
        assert abs(float(loss) - o.loss) / abs(o.loss) < 1e-5            # the f32 loss bound
        assert rel_err(z.grad.cpu(), o.grad) < 1e-4                       # the f32 gradient bound (max norm)
        if lam == 0.0:
            assert float(CTCLoss()(logits.to(DEV), ild, targets.to(DEV), tld)) == float(loss)
    with pytest.raises(ValueError, match="num_samples"):
        pg_ctc_loss(logits.to(DEV), ild, targets.to(DEV), tld, num_samples=2)
    with pytest.raises(ValueError, match="entropy_weight"):
        pg_ctc_loss(logits.to(DEV), ild, targets.to(DEV), tld, entropy_weight=0.1)


def test_trainer_refusals_at_300_symbols():
    from policy_gradient_asr_amd.model import Seq2Seq
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    s = STEP
    (x, targets, fmask, tmask), p = _step_inputs()
    m = load_params(Seq2Seq(s["V"], n_feats=s["F"]), p).to(DEV).eval()
    batch = tuple(t_.to(DEV) for t_ in (x, targets, fmask, tmask))
    with pytest.raises(ValueError, match="alphabet"):
        PolicyGradientTrainer(m).step(*batch)
    with pytest.raises(ValueError, match="alphabet"):
        PolicyGradientTrainer(m, wide_alphabet=False).step(*batch)
    with pytest.raises(ValueError, match="num_samples"):
        PolicyGradientTrainer(m, wide_alphabet=True, num_samples=2)
    tr = PolicyGradientTrainer(m, wide_alphabet=True)
    tr.entropy_weight = 0.1                        # changed after construction: refused before the step launches anything
    with pytest.raises(ValueError, match="entropy_weight"):
        tr.step(*batch)


def test_greedy_decode_and_beam_refusal_at_300_symbols():
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder, greedy_decode
    T, B, V = 120, 6, 300
    g = torch.Generator().manual_seed(4)
    scores = torch.randn(T, B, V, generator=g)
    scores[:, :, 0] += 2.5
    scores[::7, :, V - 1] += 6.0                    # the last label wins some frames
    lengths = torch.tensor([120, 100, 1, 0, 77, 120], dtype=torch.int32)
    tok, tl = greedy_decode(scores.to(DEV), lengths.to(DEV))
    want = decode_ref.greedy_decode(scores.numpy(), lengths.numpy())
    for b in range(B):
        assert list(tok[b, :tl[b]].cpu().numpy()) == want[b]
    assert any(V - 1 in w for w in want)
    dec = CTCDecoder(["<pad>"] + [str(i) for i in range(V - 1)])
    lp = torch.log_softmax(scores, 2).to(DEV)
    with pytest.raises(ValueError, match="greed"):
        dec.decode_batch(lp, lengths.to(DEV), beam_size=4)
    with pytest.raises(ValueError, match="greed"):
        dec.decode(np.exp(lp[:, 0].cpu().numpy()), beam_size=4)


def test_drivers_with_a_units_file(tmp_path):
    """model.train(units_path=) for one epoch on SyntheticSpeech over 100 units (101 symbols: the wide path by default), then
    model.predict(units_path=, beam_size=0): predicted.txt is written and the rates are finite; beam_size > 0 raises up front."""
    import itertools
    import os
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.model import _read_alphabet, predict, train
    from policy_gradient_asr_amd.units import SubwordUnits
    corpus = tmp_path / "corpus"; out = tmp_path / "run"
    corpus.mkdir()
    base = ["a", "b", "c", "d", " "]
    two = ["".join(q) for q in itertools.product(base, repeat=2)]
    three = ["".join(q) for q in itertools.product(base, repeat=3)]
    units = SubwordUnits(base + two + three[:70])
    assert len(units) == 101
    upath = str(corpus / "units.txt")
    units.save(upath)
    _, char2ind = _read_alphabet(upath)
    ds = SyntheticSpeech(32, char2ind, n_feats=20, max_chars=4, seed=1)          # transcripts of 2 .. 4 units, 2 .. 12 characters
    losses, _ = train(str(corpus), str(out), 1, 16, 0, train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=0, units_path=upath)
    assert len(losses) == 1 and np.isfinite(losses[0])
    st = torch.load(os.path.join(str(out), "checkpoint_last.pth"), map_location="cpu")
    assert st["units_path"] == upath and st["wide_alphabet"] is True and st["model"]["head.weight"].shape[0] == 101
    with pytest.raises(ValueError, match="beam_size=0"):
        predict(None, None, None, str(out), 8, test_dataset=ds, n_feats=20, units_path=upath, beam_size=5)
    cer, wer = predict(None, None, None, str(out), 8, test_dataset=ds, n_feats=20, units_path=upath, beam_size=0)
    assert np.isfinite(cer) and np.isfinite(wer)
    lines = open(os.path.join(str(out), "predicted.txt")).read().splitlines()
    assert len(lines) >= len(ds)
