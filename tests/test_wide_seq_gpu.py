"""Sequence-level REINFORCE and MWER for alphabets of 65 .. 1024 symbols on the GPU (include/pgasr_hip.h, A13-WIDE): the hypothesis
lattices and the gradient pass over K+1 lattices against fp64 (oracle/ctc_ref.py, oracle/pg_ref.py, tests/kl_ref.py,
tests/mwer_ref.py) and, at V <= 64, bit for bit against the narrow entries; ``mwer_ctc_loss_lm(wide_sequence=True)`` over the
device's own N-best lists; ``pg_ctc_loss(score_function="sequence", wide_sequence=True)`` on the device's own paths."""
import functools

import numpy as np
import pytest
import torch

import kl_ref
import mwer_ref as MR
import wide_pg_cases as wc
from oracle import ctc_ref, pg_ref
from pg_harness import DEV, rel_err

pytestmark = pytest.mark.gpu

WIDE_V, NARROW_V = wc.WIDE_V, wc.NARROW_V
T, B = 48, 3
IN_LEN = [48, 0, 31]                         # ragged, one utterance of 0 frames; 144 rows, 36 workgroups
TOL = 1e-5
BETA, GAMMA = 2.0, 2.0


@pytest.fixture(scope="module")
def ops():
    from policy_gradient_asr_amd import hipops
    return hipops


def _bits(t):
    return t.contiguous().view(torch.int32)


def _nv(V):
    n = (V + 63) // 64
    return next(p for p in (1, 2, 4, 8, 16) if n <= p)


# ---- 1. the lattices ----
LH = 40


def _lattice_hyps(V, K, blank, seed):
    """(tokens (K,B,T), lengths (K,B)): by (k + b) % 5 -- 0 the empty hypothesis, 1 a random one, 2 one label six times (blanks are
    forced between them), 3 thirty times one label (59 frames needed, 48 there: infeasible), 4 forty-five tokens, more than Lh = 40."""
    g = np.random.default_rng(seed)
    syms = np.array([s for s in range(V) if s != blank])
    tokens, lengths = np.zeros((K, B, T), dtype=np.int32), np.zeros((K, B), dtype=np.int32)
    for k in range(K):
        for b in range(B):
            kind = (k + b) % 5
            h = [[], list(g.choice(syms, size=int(g.integers(1, 11)))), [syms[(k * 7 + b) % len(syms)]] * 6,
                 [syms[(k + 3 * b) % len(syms)]] * 30, list(g.choice(syms, size=45))][kind]
            tokens[k, b, :len(h)], lengths[k, b] = h, len(h)
    return tokens, lengths


def _lattice_logits(V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(T, B, V, generator=g, dtype=torch.float64) * 2, dim=2).float()


@pytest.mark.parametrize("blank_last", [False, True], ids=["blank0", "blankV-1"])
@pytest.mark.parametrize("K", [1, 4, 16])
@pytest.mark.parametrize("V", WIDE_V)
def test_hypothesis_lattices_vs_fp64(ops, V, K, blank_last):
    """hyp_nll of pgasr_ctc_hyp_lattice_wide against mwer_ref.hyp_nlls (fp64) at rtol 1e-5, the bound of tests/test_seq_score_gpu.py
    for the narrow entry: +inf where no alignment exists, 0 for a pair over the cap, equal bits from two calls."""
    blank = V - 1 if blank_last else 0
    lp = _lattice_logits(V, 300 + V)
    tokens, lengths = _lattice_hyps(V, K, blank, 17 * V + K)
    il = np.array(IN_LEN)
    want, _, lat_len = MR.hyp_nlls(lp.double().numpy(), il, tokens, lengths, np.full(B, K), LH, blank=blank)
    over = lengths > LH
    want = np.where(over, 0.0, want)
    args = (lp.to(DEV), torch.tensor(tokens).to(DEV), torch.tensor(lengths).to(DEV), torch.tensor(IN_LEN, dtype=torch.int32).to(DEV), LH)
    got, handle = ops.ctc_hyp_lattice(*args, blank=blank)
    again, _ = ops.ctc_hyp_lattice(*args, blank=blank)
    assert torch.equal(_bits(got), _bits(again)) and handle[1:] == (K, LH)
    got = got.cpu().numpy().astype(np.float64)
    fin = np.isfinite(want)
    print(f"[wide hyp nll] V={V} K={K} blank={blank}: {int((~fin).sum())} infeasible, {int(over.sum())} over the cap, max rel err "
          f"{np.max(np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-30)):.2e}")
    assert (np.isposinf(got) == ~fin).all() and not np.isnan(got).any()
    if K > 1:
        assert (~fin).any() and over.any() and (lengths == 0).any()
    assert (got[over] == 0).all()
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-5, atol=0)


def test_hypothesis_lattice_at_the_variant_switch(ops):
    """T = 300, B = 2, K = 2, Lh = 200: 2 * Lh + 1 = 401 states take the two-states-per-thread variant, in which the 10-token
    hypotheses run the one-state variant and the 190-token ones the two-state one; V = 129."""
    V, T2, Lh = 129, 300, 200
    g = torch.Generator().manual_seed(77)
    lp = torch.log_softmax(torch.randn(T2, 2, V, generator=g, dtype=torch.float64) * 2, dim=2).float()
    r = np.random.default_rng(5)
    tokens, lengths = np.zeros((2, 2, T2), dtype=np.int32), np.array([[10, 190], [190, 10]], dtype=np.int32)
    for k in range(2):
        for b in range(2):
            h = r.integers(1, V, size=lengths[k, b])
            h[1:][h[1:] == h[:-1]] = 0                         # no adjacent repeats ...
            h[h == 0] = 1 + (np.arange(len(h))[h == 0] % 2)    # ... so 190 tokens fit the frames
            tokens[k, b, :len(h)] = h
    il = np.array([300, 280])
    want, _, _ = MR.hyp_nlls(lp.double().numpy(), il, tokens, lengths, np.full(2, 2), Lh)
    assert np.isfinite(want).all()
    got, _ = ops.ctc_hyp_lattice(lp.to(DEV), torch.tensor(tokens).to(DEV), torch.tensor(lengths).to(DEV),
                                 torch.tensor(il.astype(np.int32)).to(DEV), Lh)
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-5, atol=0)


# ---- 2. the gradient pass on given lists ----
LH2, KMAX = 10, 16


def _labels(V, blank=0):
    """(a, c, far): the last label of lane 1 and the first of lane 2 (one lane boundary), and labels of the row's last lanes."""
    nv = _nv(V)
    ok = lambda s: 0 <= s < V and s != blank
    a = 2 * nv - 1 if ok(2 * nv - 1) else 1
    c = 2 * nv if ok(2 * nv) else a
    far = [s for s in (V - 1, V - 2) if ok(s)] or [a]
    return a, c, far


@functools.lru_cache(maxsize=None)
def _grad_case(V):
    """Targets and K = 16 hypotheses per utterance in which labels a = v0 + NV - 1 and c = v0 + NV of one lane boundary both occur
    several times; the hypotheses also hold labels of the last lanes, none of which is in a target.  The hypotheses are the
    collapse of given paths (token i at frame 2 i + 1), lengths 0 .. 14 around the cap Lh = 10.  Two -inf log-probs in row (1, 0)."""
    from policy_gradient_asr_amd import hipops
    a, c, far = _labels(V)
    g = torch.Generator().manual_seed(4000 + V)
    logits = torch.randn(T, B, V, generator=g, dtype=torch.float64) * 2
    if V >= 5:
        logits[1, 0, V - 2:] = -float("inf")
    lp = torch.log_softmax(logits, dim=2).float()
    zq = torch.randn(T, B, V, generator=g, dtype=torch.float64) * 2
    lq = torch.log_softmax(zq, dim=2).float()
    targets = torch.tensor([[a, c, a, c, a, 1, c, a], [c, a, 1, 1, a, c, 0, 0], [c, c, a, 1, a, c, 0, 0]], dtype=torch.int32)
    tg_len = torch.tensor([8, 6, 6], dtype=torch.int32)
    r = np.random.default_rng(V)
    pool = [a, c, a, c] + far + [1]
    paths = np.zeros((KMAX, T, B), dtype=np.int32)
    for k in range(KMAX):
        for b in range(B):
            n = (k + 4 * b) % 15                                # 0 .. 14 tokens; 2 n + 1 <= 29 frames
            h = [pool[int(i)] for i in r.integers(0, len(pool), size=n)]
            if h and h[0] in far:
                h[0] = a                                        # frame 1 of utterance 0 holds the -inf symbols: never on a path
            for i, s in enumerate(h):
                paths[k, 2 * i + 1, b] = s
    in_len = torch.tensor(IN_LEN, dtype=torch.int32)
    coef = torch.randn(KMAX, B, generator=g) * 0.1
    coef[0, 0] = 0.0
    scale = torch.rand(B, generator=g) + 0.5
    lpd, pd, ild = lp.to(DEV), torch.tensor(paths).to(DEV), in_len.to(DEV)
    tokens, tok_len = hipops.ctc_collapse(pd, ild)
    lg, il = lp.double().numpy(), in_len.numpy()
    nll, g_ctc = ctc_ref.ctc_loss_and_grad(lg, targets.numpy(), il, tg_len.numpy())
    assert np.isfinite(g_ctc).all() and np.isinf(nll[1]) and np.isfinite(nll[[0, 2]]).all()
    g_ctc.setflags(write=False)
    return dict(V=V, lp=lpd, lg=lg, ref=lq.to(DEV), rg=lq.double().numpy(), tg=targets.to(DEV), in_len=in_len, il=ild, tl=tg_len.to(DEV),
                paths=pd, pn=paths, tokens=tokens, tok_len=tok_len, coef=coef, scale=scale, g_ctc=g_ctc, labels=(a, c, far),
                targets=targets, tg_len=tg_len)


def _tails(ops, c, tail):
    kw, want = {}, 0.0
    il = c["in_len"].numpy()
    if tail in ("entropy", "entropy+kl"):
        kw["ent_scale"] = ops.frame_entropy(c["lp"], c["il"], BETA, 1.0 / B)[1]
        want = want + pg_ref.entropy_grad(c["lg"], il, kw["ent_scale"].double().cpu().numpy())
    if tail in ("kl", "entropy+kl"):
        kw.update(ref_log_probs=c["ref"], kl_scale=ops.frame_kl(c["lp"], c["ref"], c["il"], GAMMA, 1.0 / B)[1])
        want = want + kl_ref.kl_grad(c["lg"], c["rg"], il, kw["kl_scale"].double().cpu().numpy())
    return kw, want


FORMS = ["nbest", "none", "entropy", "entropy+kl", "kl"]      # "kl": the KL tail with a NULL ent_scale


def _run(ops, c, K, form, wide=None, lat_wide=None, lp=None, ref=None):
    """The lattices of the first K hypotheses and one gradient pass of the given form."""
    lp = c["lp"] if lp is None else lp
    coef, scale = c["coef"][:K].contiguous().to(DEV), c["scale"].to(DEV)
    tokens, tok_len = c["tokens"][:K].contiguous(), c["tok_len"][:K].contiguous()
    _, handle = ops.ctc_lattice(lp, c["tg"], c["il"], c["tl"], wide=lat_wide)
    hyp_nll, hh = ops.ctc_hyp_lattice(lp, tokens, tok_len, c["il"], LH2, wide=lat_wide)
    if form == "nbest":
        return hyp_nll, ops.ctc_grad_from_lattices_nbest(lp, c["il"], c["tl"], handle, hh, scale, coef, tok_len, wide=wide)
    kw, _ = _tails(ops, c, form)
    if ref is not None:
        kw["ref_log_probs"] = ref
    return hyp_nll, ops.ctc_grad_from_lattices_seq(lp, c["il"], c["tl"], handle, hh, scale, coef, c["paths"][:K].contiguous(), tok_len,
                                                   wide=wide, **kw)


@pytest.mark.parametrize("K", [1, 2, 16])
@pytest.mark.parametrize("V", WIDE_V)
def test_gradient_pass_vs_fp64(ops, V, K):
    """Both forms of pgasr_ctc_grad_from_lattices_seq_wide -- N-best, and sampled paths with the tails none / entropy / entropy + KL
    -- against ctc_ref + pg_ref.score_terms(.., "sequence", max_hyp_len) + pg_ref.entropy_grad + kl_ref.kl_grad in fp64 with the
    device's scales: max-norm error < 1e-5 (tests/test_wide_pg_gpu.py's bound), rows t >= T_b exactly 0, the entries of probability
    0 exactly 0 and no NaN, equal bits from two calls."""
    c = _grad_case(V)
    il = c["in_len"].numpy()
    a, cc, far = c["labels"]
    ln = c["tok_len"].cpu().numpy()
    hyps = c["tokens"].cpu().numpy()
    # the inputs are what the test is about
    assert (c["targets"].numpy() == a).sum() >= 6 and (c["targets"].numpy() == cc).sum() >= 6 and cc == a + 1 and a % _nv(V) == _nv(V) - 1
    assert all(((hyps[:K, b, :] == s) & (np.arange(T)[None, :] < ln[:K, b, None])).sum() >= (2 if K > 2 else 0) for b in (0, 2) for s in (a, cc))
    assert not np.isin(c["targets"].numpy(), far).any()
    if K == 16:
        assert np.isin(hyps[:, 0, :3], far).any() and np.isin(hyps[:, 2, :3], far).any()
        for b in (0, 2):
            assert (ln[:, b] <= LH2).any() and (ln[:, b] > LH2).any()            # sequence- and path-scored pairs in one utterance
    coef64 = c["coef"][:K].double().numpy()
    assert c["coef"][0, 0] == 0
    for form in FORMS:
        _, grad = _run(ops, c, K, form)
        _, again = _run(ops, c, K, form)
        assert torch.equal(_bits(grad), _bits(again))
        use = coef64 * (ln[:K] <= LH2) if form == "nbest" else coef64           # the N-best form: a pair over the cap adds nothing
        _, g_pg, _, scored = pg_ref.score_terms(c["lg"], il, c["pn"][:K], use, "sequence", LH2)
        assert (scored == (ln[:K] <= LH2)).all()
        want = c["g_ctc"] * c["scale"].double().numpy()[None, :, None] + g_pg + (0.0 if form == "nbest" else _tails(ops, c, form)[1])
        got = grad.cpu().numpy().astype(np.float64)
        err, rerr = float(np.abs(got - want).max()), rel_err(got, want)
        print(f"[wide seq grad] V={V} K={K} {form}: max err {err:.2e}, rel {rerr:.2e} (largest reference entry {np.abs(want).max():.2f})")
        assert np.isfinite(got).all()
        assert err < TOL and rerr < TOL
        beyond = np.arange(T)[:, None] >= il[None, :]
        assert beyond.any() and (got[beyond] == 0).all()
        assert (got[1, 0, V - 2:] == 0).all() and np.abs(got[1, 0]).max() > 0      # the two symbols of probability 0


@pytest.mark.parametrize("V", [128, 1024])
def test_misaligned_tensors_take_the_scalar_loads(ops, V):
    """Views that start 4 bytes into their allocation (no 16-byte row alignment): the same bits as the aligned tensors."""
    c = _grad_case(V)

    def shifted(t):
        base = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        v = base[1:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v
    lp_m, ref_m = shifted(c["lp"]), shifted(c["ref"])
    for form in ("nbest", "entropy+kl"):
        _, want = _run(ops, c, 4, form)
        for lp_x, ref_x in ((lp_m, None), (None, ref_m), (lp_m, ref_m)):
            if form == "nbest" and lp_x is None:
                continue
            _, got = _run(ops, c, 4, form, lp=lp_x, ref=ref_x if form != "nbest" else None)
            assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("V", NARROW_V)
def test_narrow_rows_are_the_narrow_entries_bit_for_bit(ops, V):
    """V <= 64: hyp_nll and every form of the gradient pass have the bits of pgasr_ctc_hyp_lattice and
    pgasr_ctc_grad_from_lattices_nbest / _seq / _seq_ent / _seq_kl -- over the narrow entry's workspace and over the wide one's."""
    c = _grad_case(V)
    for K in (1, 2, 16):
        for form in FORMS:
            n_n, g_nn = _run(ops, c, K, form, wide=False, lat_wide=False)
            n_w, g_wn = _run(ops, c, K, form, wide=False, lat_wide=True)          # the narrow pass over the wide entry's workspace
            _, g_ww = _run(ops, c, K, form, wide=True, lat_wide=True)
            _, g_nw = _run(ops, c, K, form, wide=True, lat_wide=False)
            assert bool(torch.isfinite(g_ww).all()) and float(g_ww.abs().max()) > 0
            assert torch.equal(_bits(n_n), _bits(n_w))
            assert torch.equal(_bits(g_nn), _bits(g_wn))
            assert torch.equal(_bits(g_nn), _bits(g_ww)), (V, K, form, float((g_nn - g_ww).abs().max()))
            assert torch.equal(_bits(g_nn), _bits(g_nw))


# ---- 3. MWER over the device's own lists ----
MWER_CASES = [(60, 4, 300, 8, 4, 0), (40, 3, 65, 4, 2, 0), (40, 3, 1024, 4, 4, 0), (40, 3, 129, 4, 4, 128)]      # T, B, V, beam, N, blank
# Seeds chosen on the CPU with tests/prefix_beam_ref.py so that the REFERENCE list of some utterance holds two entries of different
# risks (with randn * 2 rows of 65 or 1024 symbols most lists hold hypotheses of one length and one distance: every coefficient 0);
# the smallest ranking margin of these lists is 6e-4 nats, far above the searches' fp32 agreement.
MWER_SEEDS = {(40, 3, 65): 1, (40, 3, 1024): 4}


def _loss_case(T_, B_, V, blank, seed, scale=2.0):
    """tests/test_mwer_gpu.py::_loss_case: randn * 2 logits, lengths from T down to a single frame (B = 4), targets without the blank."""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(T_, B_, V, generator=g, dtype=torch.float64) * scale).float()
    in_len = torch.tensor([T_, T_ - T_ // 4, T_ // 2, 1][:B_] if B_ == 4 else [T_, T_ - 2, T_ // 2][:B_], dtype=torch.int32)
    tg_len = torch.tensor([max(1, min(6, T_ // 3)), max(1, min(5, T_ // 4)), max(1, min(4, T_ // 5)), 1][:B_], dtype=torch.int32)
    syms = torch.tensor([s for s in range(V) if s != blank])
    targets = syms[torch.randint(0, V - 1, (B_, int(tg_len.max())), generator=g)].to(torch.int32)
    for b in range(B_):
        targets[b, int(tg_len[b]):] = 0
    return logits, targets, in_len, tg_len


def _device_loss(logits, targets, in_len, tg_len, **kw):
    from policy_gradient_asr_amd.mwer import MWERLossFn, mwer_ctc_loss_lm
    lg = logits.to(DEV).requires_grad_(True)
    out = mwer_ctc_loss_lm(lg, in_len.to(DEV), targets.to(DEV), tg_len.to(DEV), **kw)
    out[0].backward()
    torch.cuda.synchronize()
    nb = MWERLossFn.last_nbest
    return (out[0].detach(), lg.grad, [t.cpu().numpy() for t in nb], MWERLossFn.last_posterior.cpu().numpy(),
            MWERLossFn.last_risk.cpu().numpy(), [t.detach().cpu().numpy() for t in out[1:]])


@pytest.mark.parametrize("T_,B_,V,beam,N,blank", MWER_CASES)
def test_mwer_loss_and_gradient_match_the_fp64_reference(T_, B_, V, beam, N, blank):
    """mwer_ctc_loss_lm(wide_sequence=True) against mwer_ref's closed form on the list the device itself returned, with the bounds of
    tests/test_mwer_gpu.py::test_loss_and_gradient_match_the_fp64_reference: loss and d(logits) 1e-5 relative, nll and expected
    reward rtol 1e-5, top reward rtol 1e-6, posterior atol 1e-4.  Not vacuous: an utterance has two valid entries of different
    risks.  The same call without the keyword raises."""
    from policy_gradient_asr_amd import _lib
    from policy_gradient_asr_amd.mwer import mwer_ctc_loss_lm
    logits, targets, in_len, tg_len = _loss_case(T_, B_, V, blank, seed=MWER_SEEDS.get((T_, B_, V), 200 + T_ + V + blank))
    loss, grad, lists, post, risk, stats = _device_loss(logits, targets, in_len, tg_len, lam=1.0, beam=beam, nbest=N, blank=blank,
                                                        wide_sequence=True)
    tokens, lengths, score, count = lists
    assert tokens.shape == (N, B_, T_) and post.shape == (N, B_)
    dist, risk_len = MR.risks(targets.numpy(), tg_len.numpy(), tokens, lengths)
    ref = MR.mwer_closed_form(logits.double().numpy(), in_len.numpy(), targets.numpy(), tg_len.numpy(), tokens, lengths, count,
                              min(T_, 1023), 1.0, B_, dist, risk_len, blank=blank)
    assert any(ref.w.valid[:, b].sum() >= 2 and np.ptp(ref.w.r[ref.w.valid[:, b], b]) > 0 for b in range(B_))
    assert np.abs(ref.w.coef).max() > 0
    loss, grad = float(loss), grad.cpu().double().numpy()
    lerr = abs(loss - ref.loss) / abs(ref.loss)
    gerr = np.abs(grad - ref.grad).max() / np.abs(ref.grad).max()
    print(f"[wide mwer] T={T_} B={B_} V={V} beam={beam} N={N} blank={blank}: loss rel err {lerr:.2e}; d(logits) max-norm rel err {gerr:.2e}; "
          f"posterior abs err {np.abs(post - ref.w.p).max():.2e}; largest |coef| {np.abs(ref.w.coef).max():.2e}")
    assert lerr <= 1e-5 and gerr <= 1e-5
    nll, expected, top = stats
    np.testing.assert_allclose(nll, ref.nll, rtol=1e-5)
    np.testing.assert_allclose(expected, -ref.w.rbar, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(top, -ref.w.r[0], rtol=1e-6)
    np.testing.assert_allclose(post, ref.w.p, rtol=0, atol=1e-4)
    np.testing.assert_allclose(risk, ref.w.r, rtol=1e-6)
    for b in range(B_):
        assert not grad[int(in_len[b]):, b].any()
    with pytest.raises((ValueError, _lib.PgasrError)):
        mwer_ctc_loss_lm(logits.to(DEV), in_len.to(DEV), targets.to(DEV), tg_len.to(DEV), lam=1.0, beam=beam, nbest=N, blank=blank)


def test_mwer_at_29_symbols_is_untouched_by_the_keyword():
    logits, targets, in_len, tg_len = _loss_case(60, 4, 29, 0, seed=289)
    a = _device_loss(logits, targets, in_len, tg_len, lam=1.0, beam=16, nbest=4)
    b = _device_loss(logits, targets, in_len, tg_len, lam=1.0, beam=16, nbest=4, wide_sequence=True)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2])) and float(a[1].abs().max()) > 0


# ---- 4. the unit LM ----
def test_mwer_list_comes_from_the_fused_wide_search(ops):
    from policy_gradient_asr_amd.lm import UnitNgramLM
    T_, B_, V, beam, N = 40, 3, 129, 4, 4
    logits, targets, in_len, tg_len = _loss_case(T_, B_, V, 0, seed=411, scale=1.0)
    r = np.random.default_rng(3)
    lm = UnitNgramLM.from_transcripts([[int(x) for x in r.integers(1, 12, size=20)] for _ in range(30)], V, order=2, blank=0)
    plain = _device_loss(logits, targets, in_len, tg_len, lam=1.0, beam=beam, nbest=N, wide_sequence=True)
    zero = _device_loss(logits, targets, in_len, tg_len, lam=1.0, beam=beam, nbest=N, wide_sequence=True, unit_lm=lm)
    assert torch.equal(_bits(plain[0]), _bits(zero[0])) and torch.equal(_bits(plain[1]), _bits(zero[1]))      # lm_alpha = lm_beta = 0
    fused = _device_loss(logits, targets, in_len, tg_len, lam=1.0, beam=beam, nbest=N, wide_sequence=True, unit_lm=lm, lm_alpha=2.0,
                         lm_beta=0.5)
    lp = ops.log_softmax_rows(logits.to(DEV))
    nb = ops.ctc_beam_search_wide(lp, in_len.to(DEV), beam=beam, nbest=N, blank=0, collapse=False, unit_lm=lm, lm_alpha=2.0, lm_beta=0.5)
    assert all(np.array_equal(x, y.cpu().numpy()) for x, y in zip(fused[2], nb))
    assert not np.array_equal(fused[2][0], plain[2][0])                        # the model really changes the list


# ---- 5. the sampled objective ----
OBJ = dict(T=120, B=4, V=300, L=12)
OBJ_CASES = {"K1-greedy": (dict(), False), "K1-greedy-capped": (dict(max_hyp_len=100), False),
             "K4-leave-one-out-entropy-kl": (dict(num_samples=4, baseline="leave_one_out", entropy_weight=0.1, kl_weight=0.1), True),
             "K4-leave-one-out-entropy-kl-capped": (dict(num_samples=4, baseline="leave_one_out", entropy_weight=0.1, kl_weight=0.1,
                                                         max_hyp_len=100), True)}


@functools.lru_cache(maxsize=None)
def _objective_inputs():
    """The inputs of tests/test_wide_pg_gpu.py::_objective_inputs."""
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(OBJ["T"], OBJ["B"], OBJ["V"], generator=g) * 2
    targets = torch.randint(1, OBJ["V"], (OBJ["B"], OBJ["L"]), generator=g, dtype=torch.int32)
    ref = torch.log_softmax(torch.randn(OBJ["T"], OBJ["B"], OBJ["V"], generator=g, dtype=torch.float64) * 2, dim=2).float()
    return logits, targets, np.array([120, 90, 120, 64]), np.array([12, 9, 12, 5]), ref


@pytest.mark.parametrize("name", list(OBJ_CASES))
def test_pg_ctc_loss_with_the_sequence_score_function_vs_oracle(ops, name):
    """pg_ctc_loss(score_function="sequence", wide_sequence=True) at 300 symbols against oracle.pg_ref.pg_objective on the DEVICE's
    paths: rewards rtol 1e-6, loss 1e-5, d(logits) 1e-4 (max norm), the bounds of
    tests/test_wide_pg_gpu.py::test_pg_ctc_loss_with_wide_objectives_vs_oracle.  With max_hyp_len = 100 (random rows collapse to 64 ..
    120 tokens) sequence- and path-scored samples are mixed.  The same call without the keyword raises."""
    from policy_gradient_asr_amd.loss import PGCTCLossFn, pg_ctc_loss
    kw, objectives = OBJ_CASES[name]
    K = kw.get("num_samples", 1)
    beta, gamma = kw.get("entropy_weight", 0.0), kw.get("kl_weight", 0.0)
    logits, targets, il, tl, ref = _objective_inputs()
    ild, tld = (torch.tensor(a.astype(np.int32)).to(DEV) for a in (il, tl))
    z = logits.to(DEV).requires_grad_(True)
    call = dict(lam=1.0, seed=3, offset=1, score_function="sequence", **kw, **({"ref_log_probs": ref.to(DEV)} if gamma else {}),
                **({"wide_objectives": True} if objectives else {}))
    loss, nll, R_s, R_b = pg_ctc_loss(z, ild, targets.to(DEV), tld, wide_sequence=True, **call)
    scored = PGCTCLossFn.last_sequence_scored.cpu().numpy()
    loss.backward()
    lp_dev = ops.log_softmax_rows(logits.to(DEV))
    greedy, paths = ops.frame_sample_multi(lp_dev, K, seed=3, offset=1, want_greedy=True)
    lg = logits.double().numpy()
    o = pg_ref.pg_objective(lg, il, targets.numpy(), tl, lam=1.0, num_samples=K, baseline=kw.get("baseline", "hypothesis"),
                            score_function="sequence", max_hyp_len=kw.get("max_hyp_len"), entropy_weight=beta,
                            paths=paths.cpu().numpy(), greedy_frames=greedy.cpu().numpy())
    want_loss, want_grad = o.loss, o.grad
    if gamma:
        lp64, lq64 = ctc_ref.log_softmax(lg, axis=2), ref.double().numpy()
        _, k_scale = kl_ref.kl_stats(lp64, lq64, il, gamma, 1.0 / OBJ["B"])
        want_loss = want_loss + kl_ref.kl_loss(lp64, lq64, il, gamma, 1.0 / OBJ["B"])
        want_grad = want_grad + kl_ref.kl_grad(lp64, lq64, il, k_scale)
    assert scored.shape == (K, OBJ["B"]) and (scored == o.scored).all()
    if "max_hyp_len" in kw:
        assert scored.any() and (~scored).any()
    else:
        assert scored.all()
    lerr, gerr = abs(float(loss.detach()) - want_loss) / abs(want_loss), rel_err(z.grad.cpu(), want_grad)
    print(f"[wide seq objective] {name}: loss rel err {lerr:.2e}, d(logits) rel err {gerr:.2e}, sequence-scored {int(scored.sum())} of {scored.size}")
    np.testing.assert_allclose(R_s.cpu().numpy().reshape(K, OBJ["B"]), o.R, rtol=1e-6)      # the sequence form keeps (K,B) at K = 1
    assert lerr < 1e-5, (float(loss.detach()), want_loss)
    assert gerr < 1e-4
    with pytest.raises(ValueError, match="score_function" if objectives else "="):
        pg_ctc_loss(logits.to(DEV), ild, targets.to(DEV), tld, **call)


# ---- 6. the trainer, shards, the driver ----
STEP = dict(B=4, F=80, T=120, V=300, L=12, lens=[120, 90, 120, 64], tlens=[12, 9, 12, 5])


def test_mwer_trainer_step_matches_the_fp64_oracle():
    """One f32 step of MWERTrainer(wide_sequence=True, beam_size=8, nbest=4) at 300 symbols (pg_harness.make_batch / oracle_model, the
    batch and weights of tests/test_wide_pg_gpu.py's step test) against model_ref's forward, mwer_ref on the device's lists and
    backprop, with the bounds of tests/test_mwer_gpu.py::test_trainer_step_matches_the_fp64_oracle: loss < 1e-5, every parameter
    gradient < 1e-4, rewards rtol 1e-6, expected reward rtol 1e-4.  The trainer pads the batch: the statistics are the real rows'."""
    from oracle import model_ref
    from pg_harness import make_batch, oracle_model, param_errs
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.mwer import MWERLossFn, MWERTrainer
    s, N, beam = STEP, 4, 8
    batch = make_batch(s["B"], s["F"], s["T"], s["V"], s["L"], s["lens"], s["tlens"], 61)
    _, pr, m = oracle_model(s["F"], s["V"], 62)
    tr = MWERTrainer(m, lam=1.0, seed=3, precision="f32", beam_size=beam, nbest=N, wide_sequence=True)
    assert tr.MAX_VOCAB == 1024
    loss = tr.compute_gradients(*(t.to(DEV) for t in batch))
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    Bn = s["B"]
    nb = MWERLossFn.last_nbest
    assert nb.tokens.shape[1] >= Bn
    tokens, lengths, count = nb.tokens[:, :Bn].cpu().numpy(), nb.lengths[:, :Bn].cpu().numpy(), nb.count[:Bn].cpu().numpy()
    x, targets, fmask, _ = batch
    logits_ref = model_ref.head_logits_torch(pr, model_ref.encoder_forward_torch(pr, x.double(), fmask, packed=True))
    T_ = logits_ref.shape[0]
    lens, tlens = np.array(s["lens"]), np.array(s["tlens"])
    dist, risk_len = MR.risks(targets.numpy(), tlens, tokens, lengths)
    ref = MR.mwer_closed_form(logits_ref.detach().numpy(), lens, targets.numpy(), tlens, tokens, lengths, count, min(T_, 1023), 1.0, Bn,
                              dist, risk_len)
    assert (count >= 2).all() and (ref.w.coef != 0).any()
    assert any(np.ptp(ref.w.r[ref.w.valid[:, b], b]) > 0 for b in range(Bn))
    logits_ref.backward(torch.from_numpy(ref.grad))
    errs = param_errs(m, {k: v.grad for k, v in pr.items()})
    lerr = abs(float(loss) - ref.loss) / abs(ref.loss)
    worst = max(errs, key=errs.get)
    print(f"[wide mwer step] loss {float(loss)!r} oracle {ref.loss!r} rel err {lerr:.2e}; worst parameter gradient {worst} {errs[worst]:.2e}; "
          f"largest |coef| {np.abs(ref.w.coef).max():.2e}")
    assert lerr < 1e-5
    assert errs[worst] < 1e-4, (worst, errs[worst])
    nll, expected, top = tr.last_stats
    assert tr.last_sample_rewards.shape == (N, Bn) and tr.last_posterior.shape == (N, Bn) and nll.shape == (Bn,)
    np.testing.assert_allclose(tr.last_sample_rewards.cpu().numpy(), -ref.w.r, rtol=1e-6)
    np.testing.assert_allclose(tr.last_posterior.cpu().numpy(), ref.w.p, rtol=0, atol=1e-4)
    np.testing.assert_allclose(expected.cpu().numpy(), -ref.w.rbar, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(top.cpu().numpy(), -ref.w.r[0], rtol=1e-6)
    # the update itself: one Adam step over the gradient just checked moves the parameters and counts one applied step
    before = [q.detach().clone() for q in m.parameters()]
    tr.step(*(t.to(DEV) for t in batch))
    torch.cuda.synchronize()
    assert tr.applied_steps() >= 1 and any(not torch.equal(a, q.detach()) for a, q in zip(before, m.parameters()))
    assert all(bool(torch.isfinite(q).all()) for q in m.parameters())


def test_mwer_shards_sum_to_the_whole_batch():
    """Two mwer_ctc_loss_lm(wide_sequence=True, global_batch=B) calls on the halves of a batch of 300 symbols against one call on the
    whole batch: the same lists, risks and posteriors bit for bit, d(logits) and loss within 1e-6 -- pg_harness.shards_vs_whole's
    bounds; nothing is sampled, so a shard needs no addressing."""
    from pg_harness import lattice_case
    from policy_gradient_asr_amd.mwer import MWERLossFn, mwer_ctc_loss_lm
    logits, targets, in_len, tg_len = lattice_case(150, 4, 300, 12, 77)
    Bn, half = 4, 2
    lg, tg, il, tl = logits.float().to(DEV), targets.to(DEV), in_len.to(DEV), tg_len.to(DEV)
    kw = dict(lam=1.0, beam=8, nbest=4, wide_sequence=True)
    whole = lg.clone().requires_grad_(True)
    loss = mwer_ctc_loss_lm(whole, il, tg, tl, **kw)[0]
    nb, post, risk = MWERLossFn.last_nbest, MWERLossFn.last_posterior, MWERLossFn.last_risk
    loss.backward()
    grads, total = [], 0.0
    for h in range(2):
        sl = slice(half * h, half * h + half)
        part = lg[:, sl].contiguous().requires_grad_(True)
        l_h = mwer_ctc_loss_lm(part, il[sl].contiguous(), tg[sl].contiguous(), tl[sl].contiguous(), global_batch=Bn, **kw)[0]
        assert torch.equal(MWERLossFn.last_nbest.tokens, nb.tokens[:, sl]) and torch.equal(MWERLossFn.last_nbest.count, nb.count[sl])
        assert torch.equal(_bits(MWERLossFn.last_posterior), _bits(post[:, sl])) and torch.equal(_bits(MWERLossFn.last_risk), _bits(risk[:, sl]))
        l_h.backward()
        grads.append(part.grad)
        total += float(l_h.detach())
    diff = float((torch.cat(grads, dim=1) - whole.grad).abs().max())
    print(f"[wide mwer shards] d(logits) max diff {diff:.2e} of {float(whole.grad.abs().max()):.2e}; loss {total!r} against {float(loss.detach())!r}")
    assert float(whole.grad.abs().max()) > 0 and float((risk.max(dim=0).values - risk.min(dim=0).values).max()) > 0
    assert diff <= 1e-6 * float(whole.grad.abs().max())
    assert abs(total - float(loss.detach())) <= 1e-6 * abs(float(loss.detach()))


def test_sequence_shards_draw_and_sum_to_the_whole_batch():
    """pg_harness.shards_vs_whole at 300 symbols with score_function="sequence", four samples, the leave-one-out baseline and the
    entropy bonus: the same rewards bit for bit, d(logits) and loss within 1e-6, the same samples sequence-scored."""
    from pg_harness import lattice_case, shards_vs_whole
    from policy_gradient_asr_amd.loss import PGCTCLossFn
    kw = dict(lam=1.0, seed=9, offset=2, num_samples=4, baseline="leave_one_out", entropy_weight=0.1, score_function="sequence",
              max_hyp_len=140, wide_objectives=True, wide_sequence=True)
    r = shards_vs_whole(kw, lattice_case(150, 4, 300, 12, 77), extra=lambda: PGCTCLossFn.last_sequence_scored.clone())
    assert r.R_s.shape == (4, 4) and float(r.grad.abs().max()) > 0 and bool(torch.isfinite(r.loss))
    assert torch.equal(torch.cat(r.extra_parts, dim=1), r.extra_whole) and bool(r.extra_whole.any())


def test_train_driver_with_mwer_over_units(tmp_path):
    """model.train(units_path=, objective="mwer", wide_sequence=True) for one epoch over 100 units: it runs, the checkpoint holds the
    keyword, a second call without the keyword resumes with what the checkpoint holds, and a fresh run without it is refused."""
    import itertools
    import os
    from pg_harness import tiny_corpus
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.model import _read_alphabet, train
    from policy_gradient_asr_amd.units import SubwordUnits
    corpus, out, _ = tiny_corpus(tmp_path)
    base = ["a", "b", "c", "d", " "]
    two = ["".join(q) for q in itertools.product(base, repeat=2)]
    three = ["".join(q) for q in itertools.product(base, repeat=3)]
    upath = str(corpus / "units.txt")
    SubwordUnits(base + two + three[:70]).save(upath)
    _, char2ind = _read_alphabet(upath)
    assert len(char2ind) == 101
    ds = SyntheticSpeech(32, char2ind, n_feats=20, max_chars=4, seed=1)
    kw = dict(train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=0, units_path=upath, objective="mwer", mwer_nbest=4, mwer_beam=8)
    losses, _ = train(str(corpus), str(out), 1, 16, 0, wide_sequence=True, **kw)
    assert len(losses) == 1 and np.isfinite(losses[0])
    st = torch.load(os.path.join(str(out), "checkpoint_last.pth"), map_location="cpu")
    assert st["wide_sequence"] is True and st["wide_alphabet"] is True and st["epoch"] == 1
    losses, _ = train(str(corpus), str(out), 2, 16, 0, **kw)                     # wide_sequence=None: restored from the checkpoint
    assert len(losses) == 2 and np.isfinite(losses[1])
    assert torch.load(os.path.join(str(out), "checkpoint_last.pth"), map_location="cpu")["epoch"] == 2
    with pytest.raises(ValueError, match="mwer"):                                # without the keyword: refused as ever
        train(str(corpus), str(tmp_path / "other"), 1, 16, 0, **kw)
