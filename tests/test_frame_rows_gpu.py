"""The V <= 64 row kernels of csrc/frame_ops.hip, the samplers' wide twins and the fused CTC head on the device, against the fp64
oracles, per-element bounds and case tables of tests/frame_rows_ref.py (tests/test_frame_rows_ref_cpu.py holds the numpy fp32
restatements to half of the same bounds and shows that the bounds reject the mistakes these kernels invite).

    samplers       every row of a batch draws one planted u (the Philox counter is addressed through utt_ids): u = 1 - 2^-24 on rows
                   with trailing labels of probability 0, u = 0 on rows with leading ones, u = 3/4 and ordinary draws on constant
                   rows, where the fp32 cdf is exact.  No draw may return a label whose exp(x - max) is 0 in fp32.
    log-softmax    4 EPS32 max(|x|_max, |lse|) + 2e-6 per element, the -inf pattern the oracle's, nothing written past rows * V
    reinforce_grad |coef_b| C EPS32 absolute with C = 4
    rewards        rtol 1e-6 / atol 1e-9; leave-one-out at equal rewards (K + 3) EPS32 scale max|R|; exact zeros where the oracle's are
    loss values    gamma_n (sum |coef lp| + |nll us|), n = ceil(T_b / 256) + 10 (single and multi alike)
    batch_prep     exact
    head           logits gamma_{K+1} (sum |x W| + |b|), log-probs the row's largest logit bound + the log-softmax bound

Worst err / bound on the MI355X (printed with -s): NOTES.md 0.35.  The whole file takes about 3 s there."""
import numpy as np
import pytest
import torch

import frame_rows_ref as fr
from oracle import decode_ref, pg_ref
from pg_harness import DEV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from policy_gradient_asr_amd import hipops
    return hipops


@pytest.fixture(scope="module")
def lib():
    from policy_gradient_asr_amd import _lib
    return _lib.load()


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)            # a copy: the cached case tables are read-only


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- A. samplers at a chosen u ----
def _planted_draws(ops, x, name, wide):
    """x (R, V) as a (1, R, V) batch in which every row is utterance PLANTED[name]'s row of a global batch of 64: single sample,
    K multi samples (both (.., R) int64 numpy)."""
    offset, row, _ = fr.PLANTED[name]
    scores = _dev(x[None])
    ids = torch.full((x.shape[0],), row, dtype=torch.int32, device=DEV)
    kw = dict(seed=fr.SAMPLER_SEED, offset=offset, batch_stride=fr.SAMPLER_STRIDE, utt_ids=ids, wide=True if wide else None)
    _, s = ops.frame_argmax_sample(scores, want_greedy=False, **kw)
    _, sm = ops.frame_sample_multi(scores, fr.SAMPLER_K, **kw)
    return s[0].cpu().numpy().astype(np.int64), sm[:, 0].cpu().numpy().astype(np.int64)


def _check_multi(x, s, sm, offset, row):
    """Draw 0 is the single sampler's bit for bit; no draw returns a zero-e label; every draw follows the oracle's rule at its own
    u up to the boundary rule."""
    assert np.array_equal(sm[0], s)
    ze = fr.zero_e(x)
    r = np.arange(len(x))
    us = pg_ref.sampler_uniforms(1, [row], fr.SAMPLER_K, fr.SAMPLER_SEED, offset, fr.SAMPLER_STRIDE)[:, 0, 0]
    for k in range(fr.SAMPLER_K):
        assert sm[k].min() >= 0 and sm[k].max() < x.shape[1] and not ze[r, sm[k]].any(), k
        if k:
            want, cdf = fr.planted_oracle(x, us[k])
            diff = np.nonzero(sm[k] != want)[0]
            for i in diff:
                assert abs(cdf[i, min(sm[k][i], want[i])] - us[k]) < fr.BOUNDARY
            assert len(diff) <= fr.sampler_cap(len(x))


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_sampler_at_u_max_never_returns_a_zero_probability_label(ops, wide):
    offset, row, u = fr.PLANTED["umax"]
    excused = rows = 0
    for V, w, m, kind in fr.umax_cases():
        if w != wide:
            continue
        x = fr.umax_rows(V, m, kind)
        s, sm = _planted_draws(ops, x, "umax", wide)
        ze = fr.zero_e(x)
        r = np.arange(len(x))
        above = int((s > m).sum())
        assert above == 0, f"V={V} m={m} {kind}: {above} of {len(x)} rows return a label above the last one with non-zero probability"
        assert s.min() >= 0 and not ze[r, s].any()
        want, cdf = fr.planted_oracle(x, u)
        diff = np.nonzero(s != want)[0]
        for i in diff:
            k = min(s[i], want[i])
            assert k >= m - 1 and abs(cdf[i, k] - u) < fr.BOUNDARY, (V, m, kind, i, s[i], want[i])
        assert len(diff) <= fr.sampler_cap(len(x))
        excused += len(diff)
        rows += len(x)
        _check_multi(x, s, sm, offset, row)
    print(f"[sampler u = 1 - 2^-24, {'wide' if wide else 'narrow'}] {rows} rows, none above m, {excused} excused at the last non-zero label")


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_sampler_at_u_zero_returns_the_first_label_with_probability(ops, wide):
    offset, row, _ = fr.PLANTED["uzero"]
    for V, w, f in fr.uzero_cases():
        if w != wide:
            continue
        x = fr.uzero_rows(V, f)
        s, sm = _planted_draws(ops, x, "uzero", wide)
        assert (s == f).all(), (V, f, np.unique(s))
        _check_multi(x, s, sm, offset, row)


def test_sampler_on_constant_rows_is_the_oracle_exactly(ops):
    """e = 1, exact sums, cdf_k = (k + 1) / V exactly: no boundary rule.  Ordinary addressing over a (40, 8, V) tensor, through the
    narrow and the wide entry; u = 3/4 planted, where c_k == u * total exactly for V >= 4; V = 1 returns 0."""
    offset, row, u34 = fr.PLANTED["u34"]
    for V in fr.CONST_V:
        scores = np.full((40, 8, V), 0.25, dtype=np.float32)
        want, _, _ = decode_ref.sample_paths(scores, seed=fr.SAMPLER_SEED, offset=3)
        want4, _, _ = pg_ref.sample_paths(scores, fr.SAMPLER_K, fr.SAMPLER_SEED, 3)
        for wide in (None, True):
            _, s = ops.frame_argmax_sample(_dev(scores), seed=fr.SAMPLER_SEED, offset=3, want_greedy=False, wide=wide)
            assert np.array_equal(s.cpu().numpy(), want), (V, wide)
            _, sm = ops.frame_sample_multi(_dev(scores), fr.SAMPLER_K, seed=fr.SAMPLER_SEED, offset=3, wide=wide)
            assert np.array_equal(sm.cpu().numpy(), want4), (V, wide)
            x = np.full((fr.SAMPLER_ROWS, V), -1.5, dtype=np.float32)
            s, sm = _planted_draws(ops, x, "u34", bool(wide))
            assert (s == min(int(u34 * V), V - 1)).all() and np.array_equal(sm[0], s), (V, wide)
        if V == 1:
            assert not want.any()
    # the wide kernels hold several labels per lane: constant rows of 128 and 1024 labels are as exact
    for V in (128, 1024):
        scores = np.full((40, 8, V), 0.25, dtype=np.float32)
        want, _, _ = decode_ref.sample_paths(scores, seed=fr.SAMPLER_SEED, offset=3)
        _, s = ops.frame_argmax_sample(_dev(scores), seed=fr.SAMPLER_SEED, offset=3, want_greedy=False)
        assert np.array_equal(s.cpu().numpy(), want), V
        x = np.full((fr.SAMPLER_ROWS, V), -1.5, dtype=np.float32)
        s, _ = _planted_draws(ops, x, "u34", True)
        assert (s == int(u34 * V)).all()


# ---- B. log-softmax, V <= 64 ----
def test_log_softmax_rows_edges(ops, lib):
    """Every case of the table through the C entry, into a slice of a sentinel-filled tensor."""
    worst, pad = 0.0, 64
    for V, rows, kind in fr.lsm_cases():
        x = fr.lsm_case(V, rows, kind)
        big = torch.full((rows * V + 2 * pad,), fr.SENTINEL, dtype=torch.float32, device=DEV)
        xd = x.to(DEV)
        st = lib.pgasr_log_softmax_rows(xd.data_ptr(), rows, V, big.data_ptr() + 4 * pad, _stream())
        assert st == 0
        out = big.cpu()
        assert (out[:pad] == fr.SENTINEL).all() and (out[pad + rows * V:] == fr.SENTINEL).all(), (V, rows, kind)
        got = out[pad:pad + rows * V].view(rows, V)
        ratio, _ = fr.lsm_ratio(got.double(), x)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (V, rows, kind, ratio)
        if kind == "underflow":
            mx = x.max(-1, keepdim=True).values
            assert torch.equal(got, x - mx) and (got.max(-1).values == 0).all(), (V, rows)
        if kind in ("shift+", "shift-"):                    # shift invariance: the same row unshifted agrees to both bounds
            base = x - (1e4 if kind == "shift+" else -1e4)
            want0, bound0, _ = fr.lsm_oracle(base)
            _, bound1, _ = fr.lsm_oracle(x)
            assert ((got.double() - want0).abs() <= bound0 + bound1 + 4 * fr.EPS32 * 1e4).all()
    print(f"[narrow log-softmax] {len(fr.lsm_cases())} cases: worst err / bound {worst:.3f}")
    # the wrapper takes the narrow entry for V <= 64 and gives the same bits
    x = fr.lsm_case(33, 29, "saturated")
    fr.lsm_check(ops, x, "V=33 rows=29 saturated through hipops", DEV, tag="narrow log-softmax")


# ---- C. reinforce_grad ----
def test_reinforce_grad_edges(ops):
    worst = 0.0
    for V in fr.REINFORCE_V:
        for T, B in fr.REINFORCE_TB:
            scores, path, coef, lengths = fr.reinforce_case(T, B, V)
            want = decode_ref.reinforce_grad(scores, path, coef, lengths)
            bound = fr.reinforce_bound(coef, want.shape)
            d = [_dev(a) for a in (scores, path, coef, lengths)]
            got = ops.reinforce_grad(*d).cpu().numpy()
            err = np.abs(got.astype(np.float64) - want)
            nz = bound > 0
            assert (err[~nz] == 0).all(), (T, B, V)
            if nz.any():
                worst = max(worst, float((err[nz] / bound[nz]).max()))
            assert (err <= bound).all(), (T, B, V, float((err[nz] / bound[nz]).max()))
            pad = np.arange(T)[:, None] >= lengths[None, :]
            assert (got[pad] == 0).all()                                           # padded frames: exactly 0
            if V > 2 and T > 1:
                assert (got[T - 1, 0, 1::3] == 0).all()                            # -inf labels: exactly 0
            # accumulate onto a random tensor: padded frames keep their bits, the rest is base + g to a rounding of the sum
            base = torch.randn(T, B, V, generator=torch.Generator().manual_seed(T + V)).to(DEV)
            acc = base.clone()
            ops.reinforce_grad(*d, out=acc, accumulate=True)
            a, b0 = acc.cpu().numpy(), base.cpu().numpy()
            assert np.array_equal(a[pad].view(np.uint32), b0[pad].view(np.uint32))
            assert (np.abs(a.astype(np.float64) - (b0 + want)) <= bound + fr.EPS32 * np.abs(b0 + want)).all()
            # lengths = None is lengths all T
            full = _dev(np.full(B, T, dtype=np.int32))
            g_none = ops.reinforce_grad(d[0], d[1], d[2], None)
            assert torch.equal(g_none, ops.reinforce_grad(d[0], d[1], d[2], full))
            want_full = decode_ref.reinforce_grad(scores, path, coef, np.full(B, T))
            assert (np.abs(g_none.cpu().numpy() - want_full) <= bound).all()
    print(f"[reinforce_grad] C = {fr.REINFORCE_C}: worst err / bound {worst:.3f}")


# ---- D. rewards, loss values, batch preparation ----
def test_pg_rewards_edges(ops):
    worst, worst_loo = 0.0, 0.0
    lam, inv_bg = fr.REWARD_LAM, fr.REWARD_INV_BG
    for B in fr.REWARD_B:
        for K in fr.REWARD_K:
            for kind in fr.REWARD_KINDS:
                dist, tl, rl = fr.reward_case(B, K, kind)
                for loo in (False, True):
                    if loo and K < 2:
                        continue
                    d = _dev((dist[1:] if loo else dist).reshape(-1))
                    for lens in (None, rl):
                        want = fr.rewards_oracle(dist, tl, K, loo, rl=lens)
                        got = ops.pg_rewards_multi(d, _dev(tl), K, lam, inv_bg, baseline="leave_one_out" if loo else "hypothesis",
                                                   reward_lengths=None if lens is None else _dev(lens))
                        got = [g.cpu().numpy() for g in got]
                        for i, (g, w) in enumerate(zip(got, want)):
                            assert g.shape == w.shape
                            if kind == "equal" and i == 2:
                                if not loo:
                                    assert not g.any()                                   # equal distances: exactly 0
                                else:
                                    b = fr.reward_loo_equal_bound(K, want[1])
                                    assert (np.abs(g) <= b[None, :]).all(), (B, K)
                                    if (b > 0).any():
                                        worst_loo = max(worst_loo, float((np.abs(g)[:, b > 0] / b[b > 0]).max()))
                                continue
                            tol = fr.REWARD_ATOL + fr.REWARD_RTOL * np.abs(w)
                            r = float((np.abs(g - w) / tol).max())
                            worst = max(worst, r)
                            assert r <= 1.0, (B, K, kind, loo, i, r)
                    if K == 1 and not loo:                                              # the single-sample entry: the same bits
                        one = ops.pg_rewards(_dev(dist.reshape(-1)), _dev(tl), lam, inv_bg)
                        multi = ops.pg_rewards_multi(_dev(dist.reshape(-1)), _dev(tl), 1, lam, inv_bg)
                        for a, b in zip(one, (multi[0], multi[1][0], multi[2][0], multi[3])):
                            assert torch.equal(a, b)
    print(f"[pg_rewards] worst err / (atol + rtol |want|) {worst:.3f}; leave-one-out at equal rewards err / bound {worst_loo:.3f}")


def test_pg_loss_value_edges(ops):
    worst = 0.0
    for T in fr.LOSS_T:
        for V in fr.LOSS_V:
            for flip in (False, True):
                for K, per_frame in ((1, False), (1, True), (4, False)):
                    case = fr.loss_case(T, V, K, flip, per_frame)
                    want, bound = fr.loss_oracle(*case, per_frame=per_frame)
                    lp, paths, in_len, nll, us, coef = (_dev(a) for a in case)
                    if K == 1:
                        call = lambda: ops.pg_loss_value(lp, paths[0], in_len, nll, us, coef if per_frame else coef[0])
                    else:
                        call = lambda: ops.pg_loss_value_multi(lp, paths, in_len, nll, us, coef)
                    got = call()
                    assert torch.equal(got, call())                                     # fixed-order reduction: equal bits
                    g = got.cpu().numpy().astype(np.float64)
                    assert np.isfinite(g).all()                                         # nothing off the path (-inf) was read
                    err = np.abs(g - want)
                    ok = bound > 0
                    assert (err[~ok] == 0).all()
                    if ok.any():
                        worst = max(worst, float((err[ok] / bound[ok]).max()))
                    assert (err <= bound).all(), (T, V, K, flip, per_frame, err, bound)
                    if K == 1 and not per_frame:
                        plain = ops.pg_loss_value(lp, None, in_len, nll, us, None)
                        assert np.array_equal(plain.cpu().numpy().view(np.uint32), (case[3] * case[4]).view(np.uint32))
                        # the multi entry with K = 1 is the single entry
                        m1 = ops.pg_loss_value_multi(lp, paths, in_len, nll, us, coef)
                        assert (np.abs(m1.cpu().numpy() - want) <= bound).all()
    print(f"[pg_loss_value] worst err / bound {worst:.3f}")


def test_batch_prep_edges(ops):
    for T in fr.PREP_T:
        for L in fr.PREP_L:
            fmask, tmask, targets, lens, tls = fr.prep_case(T, L)
            f, m, t = torch.from_numpy(fmask), torch.from_numpy(tmask), torch.from_numpy(targets)
            in_len, tg_len, tg32 = ops.batch_prep(f.to(DEV), m.to(DEV), t.to(DEV))
            assert torch.equal(in_len.cpu(), f.sum(1).int()) and torch.equal(tg_len.cpu(), m.sum(1).int())
            assert torch.equal(tg32.cpu(), t.int()) and int(tg32.max()) == 2 ** 31 - 1
            assert np.array_equal(in_len.cpu().numpy(), lens) and np.array_equal(tg_len.cpu().numpy(), tls)


# ---- E. fused head ----
def _head_call(lib, xw, W, b, rows, K, V, want_logits=True, pad=32):
    """pgasr_head_logsoftmax into slices of sentinel-filled tensors -> (status, logits or None, lp, untouched)."""
    xd, Wd = _dev(xw), _dev(W)
    bd = None if b is None else _dev(b)
    outs = [torch.full((rows * V + 2 * pad,), fr.SENTINEL, dtype=torch.float32, device=DEV) for _ in range(2)]
    st = lib.pgasr_head_logsoftmax(xd.data_ptr(), rows, K, xw.shape[1], Wd.data_ptr(), 0 if bd is None else bd.data_ptr(), V,
                                   outs[0].data_ptr() + 4 * pad if want_logits else 0, outs[1].data_ptr() + 4 * pad, _stream())
    torch.cuda.synchronize()
    res, clean = [], True
    for o in outs:
        o = o.cpu()
        clean = clean and bool((o[:pad] == fr.SENTINEL).all()) and bool((o[pad + rows * V:] == fr.SENTINEL).all())
        res.append(o[pad:pad + rows * V].view(rows, V).numpy())
    if not want_logits:
        clean = clean and bool((res[0] == fr.SENTINEL).all())
    return st, (res[0] if want_logits else None), res[1], clean


@pytest.mark.parametrize("case", fr.HEAD_CASES, ids=lambda c: f"rows{c[0]}-K{c[1]}-V{c[2]}-{'bias' if c[3] else 'nobias'}-ldx+{c[4]}")
def test_head_edges(lib, ops, case):
    rows, K, V, bias, pad = case
    xw, W, b, want = fr.head_case(*case)
    st, z, lp, clean = _head_call(lib, xw, W, b, rows, K, V)
    assert st == 0 and clean
    rz = float((np.abs(z - want["z"]) / want["zb"]).max())
    rl = float((np.abs(lp - want["lp"]) / want["lpb"]).max())
    print(f"[head] rows={rows} K={K} V={V} bias={bias} ldx=K+{pad}: err / bound logits {rz:.3f}, log-probs {rl:.3f}")
    assert rz <= 1.0 and rl <= 1.0
    st, none, lp2, clean = _head_call(lib, xw, W, b, rows, K, V, want_logits=False)
    assert st == 0 and clean and none is None and np.array_equal(lp2.view(np.uint32), lp.view(np.uint32))
    if bias and pad == 0:                                                           # the wrapper reaches the same kernel
        z3, lp3 = ops.head_logsoftmax(_dev(xw), _dev(W), _dev(b))
        assert np.array_equal(z3.cpu().numpy(), z) and np.array_equal(lp3.cpu().numpy(), lp)


def test_head_refusals(lib):
    """Everything the kernel cannot take is refused on the host, before any launch: the outputs keep their sentinel."""
    rows, K, V = 8, 64, 5
    x = torch.zeros(rows * 1100 + 8, dtype=torch.float32, device=DEV)
    W = torch.zeros(33 * 1088, dtype=torch.float32, device=DEV)
    out = torch.full((2, rows * 33), fr.SENTINEL, dtype=torch.float32, device=DEV)
    call = lambda xp, K_, ldx, V_: lib.pgasr_head_logsoftmax(xp, rows, K_, ldx, W.data_ptr(), 0, V_, out[0].data_ptr(), out[1].data_ptr(), _stream())
    assert x.data_ptr() % 16 == 0
    assert call(x.data_ptr(), K, K, V) == 0
    out.fill_(fr.SENTINEL)
    for what, args in (("ldx not a multiple of 4", (x.data_ptr(), K, K + 2, V)), ("x misaligned", (x.data_ptr() + 4, K, K + 4, V)),
                       ("K = 1088", (x.data_ptr(), 1088, 1088, V)), ("V = 33", (x.data_ptr(), K, K, 33)),
                       ("ldx < K", (x.data_ptr(), K, K - 4, V)), ("K = 96", (x.data_ptr(), 96, 96, V))):
        assert call(*args) != 0, what
    torch.cuda.synchronize()
    assert (out == fr.SENTINEL).all()
