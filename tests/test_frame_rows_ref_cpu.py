"""The bounds and case tables of tests/frame_rows_ref.py against the reference arithmetic, without a GPU: every case meets the
preconditions its bound was written for, the numpy fp32 restatement of each kernel's documented formula stays within HALF of the
bound the kernel is held to (tests/test_frame_rows_gpu.py), and the bounds reject the mistakes these kernels invite.

The sampler's part also shows the defect of the rule the kernels had (k = #{c <= u total} alone): at u = 1 - 2^-24 a share of the
table's rows returns a label of probability 0, and a threshold inside the one-ulp gap of an interior flat stretch does the same;
the rule with the move off e == 0 does neither.

Worst restatement err / bound (printed with -s): NOTES.md 0.35."""
import numpy as np
import pytest
import torch

import frame_rows_ref as fr
from oracle import decode_ref, pg_ref


# ---- A. samplers ----
def test_planted_uniforms():
    for name, (offset, row, u) in fr.PLANTED.items():
        got = decode_ref.sampler_uniforms(1, fr.SAMPLER_STRIDE, fr.SAMPLER_SEED, offset)[0, row]
        assert got == u, (name, got)
        # the id-addressed form the GPU test uses: every row with utt_id = row draws it, draw 0 of the multi-sample form too
        ids = np.full(5, row)
        assert (pg_ref.sampler_uniforms(1, ids, fr.SAMPLER_K, fr.SAMPLER_SEED, offset, fr.SAMPLER_STRIDE)[0] == u).all()
    assert np.float32(fr.U_MAX) == fr.U_MAX < 1.0


def test_sampler_tables_keep_the_oracle_inside_the_cap():
    """Rows whose oracle cdf passes within 2e-6 of u at a label other than the planted edge: at most max(1, rows // 1000) per
    case.  (At u = 1 - 2^-24 the last non-zero label's cdf of 1 is always that near: the one place a u-max row may be excused;
    at u = 0 nothing is excused.)"""
    cap = fr.sampler_cap(fr.SAMPLER_ROWS)
    worst = 0
    cases = fr.umax_cases()
    assert {(V, w) for V, w, _, _ in cases} == {(V, False) for V in fr.NARROW_V} | {(V, True) for V in fr.WIDE_V}
    for V, wide, m, kind in cases:
        x = fr.umax_rows(V, m, kind)
        assert (fr.zero_e(x)[:, m + 1:]).all() and not fr.zero_e(x)[:, m].any()
        want, cdf = fr.planted_oracle(x, fr.U_MAX)
        assert (want == m).sum() >= fr.SAMPLER_ROWS - cap
        n = int(fr.boundary_rows(cdf, np.full(len(x), fr.U_MAX), 0, m).sum())
        worst = max(worst, n)
        assert n <= cap, (V, m, kind, n)
    for V, wide in {(V, w) for V, w, _, _ in cases if w}:
        nv = fr.wide_nv(V)
        ms = fr.umax_ms(V, True)
        assert any(m % nv == nv - 1 and 0 < m < V - 2 for m in ms) and any(m % nv != nv - 1 and 0 < m < V - 2 for m in ms)
    for V, wide, f in fr.uzero_cases():
        x = fr.uzero_rows(V, f)
        want, cdf = fr.planted_oracle(x, 0.0)
        assert (want == f).all() and not fr.boundary_rows(cdf, np.zeros(len(x)), f + 1, None).any()
    # draws 1 .. K - 1 of the multi-sample runs use other uniforms at the same counter: the same cap, at any label
    worst_multi = 0
    for name, tables in (("umax", [fr.umax_rows(V, m, kind) for V, _, m, kind in cases]),
                         ("uzero", [fr.uzero_rows(V, f) for V, _, f in fr.uzero_cases()])):
        us = fr.multi_uniforms(name)
        assert us[0] == fr.PLANTED[name][2] and (us[1:] > 1e-3).all() and (us[1:] < 1 - 1e-3).all()
        for x in tables:
            for k in range(1, fr.SAMPLER_K):
                _, cdf = fr.planted_oracle(x, us[k])
                n = int(fr.boundary_rows(cdf, np.full(len(x), us[k])).sum())
                worst_multi = max(worst_multi, n)
                assert n <= cap, (name, x.shape, k, n)
    print(f"[sampler tables] most rows of one case near a boundary at draws 1 .. {fr.SAMPLER_K - 1}: {worst_multi} (cap {cap})")
    # the ordinary-addressing tables: constant rows are exact, so no row is near a boundary unless u is exactly k / V
    for V in fr.CONST_V:
        _, cdf, u = decode_ref.sample_paths(np.full((40, 8, V), 0.25, dtype=np.float32), seed=fr.SAMPLER_SEED, offset=3)
        assert np.array_equal(cdf, np.broadcast_to((np.arange(V) + 1) / V, cdf.shape))
        assert not fr.boundary_rows(cdf, u).any()
    print(f"[sampler tables] most rows of one case near a boundary away from the planted edge: {worst} (cap {cap})")


def test_sampler_rule_at_u_max_parent_defect_and_fix():
    """The parent rule returns a label above m (probability 0) in a non-zero share of the u-max rows; the fixed rule never does,
    agrees with the oracle up to the boundary rule, and returns what the parent rule returns wherever that has e > 0."""
    shares = {}
    for V, wide, m, kind in fr.umax_cases():
        x = fr.umax_rows(V, m, kind)
        nv = fr.wide_nv(V) if wide else 1
        old = fr.sampler_f32(x, fr.U_MAX, rule="parent", nv=nv)
        new = fr.sampler_f32(x, fr.U_MAX, rule="fixed", nv=nv)
        ze = fr.zero_e(x)
        r = np.arange(len(x))
        assert new.max() <= m and not ze[r, new].any()
        keep = ~ze[r, old]
        assert np.array_equal(new[keep], old[keep])                           # a draw with e > 0 keeps its value
        want, cdf = fr.planted_oracle(x, fr.U_MAX)
        diff = np.nonzero(new != want)[0]
        for i in diff:
            k = min(new[i], want[i])
            assert abs(cdf[i, k] - fr.U_MAX) < fr.BOUNDARY
        assert len(diff) <= fr.sampler_cap(len(x))
        shares[(V, wide, m, kind)] = float((old > m).mean())
    bad = {k: v for k, v in shares.items() if v > 0}
    print("[sampler at u = 1 - 2^-24] share of rows where the parent rule returns a zero-probability label:")
    for (V, wide, m, kind), v in shares.items():
        print(f"    V={V} {'wide' if wide else 'narrow'} m={m} {kind}: {v:.3f}")
    # every narrow V below 64 and every wide V shows it; V = 64 narrow with m = V - 2 leaves one zero label only
    for V in (8, 29) + fr.WIDE_V:
        assert max(v for (v_, _, _, _), v in bad.items() if v_ == V) > 0.05, V
    assert sum(v > 0 for v in shares.values()) >= len(shares) // 3


def test_sampler_rule_in_an_interior_flat_stretch():
    """Labels 10 .. 19 of 29 carry probability 0.  On a row whose fp32 scan is not constant over the stretch, a threshold inside
    that gap makes the parent rule return a label of the stretch; the fixed rule returns label 20 or a neighbour with e > 0."""
    x = (np.random.default_rng(5).normal(size=(2000, 29)) * 2).astype(np.float32)
    x[:, 10:20] = -np.inf
    e, c, total = fr.sampler_scan_f32(x)
    flat = c[:, 9:20]
    rows = np.nonzero(flat.min(axis=1) != flat.max(axis=1))[0]
    assert rows.size > 0
    print(f"[sampler interior] {rows.size} of {len(x)} rows have a scan that is not constant over the flat stretch")
    hit = 0
    for r in rows[:50]:
        for thr in np.unique(flat[r]):
            old = fr.sampler_f32(x[r:r + 1], None, rule="parent", thr=thr)[0]
            new = fr.sampler_f32(x[r:r + 1], None, rule="fixed", thr=thr)[0]
            assert e[r, new] > 0 and (new == old or e[r, old] == 0)
            if e[r, old] == 0:
                hit += 1
                assert new == 20
    assert hit > 0
    # rows without a zero label: the scan need not be monotone either, and the fix changes nothing there
    y = (np.random.default_rng(6).normal(size=(20000, 29)) * 2).astype(np.float32)
    _, cy, _ = fr.sampler_scan_f32(y)
    print(f"[sampler interior] {float((np.diff(cy, axis=1) < 0).any(axis=1).mean()):.4f} of all-positive rows have a scan that is not monotone")
    u = np.random.default_rng(7).random(len(y)).astype(np.float32)
    assert np.array_equal(fr.sampler_f32(y, u, rule="parent"), fr.sampler_f32(y, u, rule="fixed"))


def test_sampler_exact_cases_and_mistakes():
    # constant rows: e = 1, exact sums, cdf_k = (k + 1) / V: the restatement IS the oracle, at every u and at u = j / V exactly
    for V in fr.CONST_V:
        x = np.full((64, V), 0.25, dtype=np.float32)
        u = np.concatenate([np.arange(32) / 32, np.random.default_rng(V).random(32)]).astype(np.float32)
        want = np.minimum(np.floor(u.astype(np.float64) * V), V - 1)
        for nv in (1, 2, 16):
            assert np.array_equal(fr.sampler_f32(x, u, nv=nv), want)
        if V > 1:
            assert not np.array_equal(fr.sampler_f32(x, u, strict=True), want)          # c < thr: off at every u = j / V
        else:
            assert not fr.sampler_f32(x, u).any()
    offset, row, u34 = fr.PLANTED["u34"]
    assert fr.sampler_f32(np.zeros((1, 64), np.float32), u34)[0] == 48 and fr.sampler_f32(np.zeros((1, 64), np.float32), u34, strict=True)[0] == 47
    # a clamp to V: out of range on u-max rows without a zero label (c_{V-1} < total through the padding lanes)
    x = fr.umax_rows(29, 28, "none")
    assert fr.sampler_f32(x, fr.U_MAX).max() == 28 and fr.sampler_f32(x, fr.U_MAX, rule="parent", clamp=29).max() == 29
    # u = 0 with c < thr counts nothing: label 0, which has probability 0 (the parent rule); the fixed rule hides that mistake at
    # u = 0, the constant rows above do not
    x = fr.uzero_rows(29, 14)
    assert (fr.sampler_f32(x, 0.0) == 14).all() and (fr.sampler_f32(x, 0.0, rule="parent", strict=True) == 0).all()


# ---- B. log-softmax ----
def test_log_softmax_restatement_and_mistakes():
    worst = 0.0
    cases = fr.lsm_cases()
    assert {c[0] for c in cases} == set(fr.LSM_V) and {c[1] for c in cases} == set(fr.LSM_ROWS)
    rejected = {"lanes32": 0, "le": 0}
    for V, rows, kind in cases:
        x = fr.lsm_case(V, rows, kind)
        assert torch.isfinite(x).any(-1).all()
        got = fr.lsm_f32(x.numpy())
        ratio, _ = fr.lsm_ratio(torch.from_numpy(got).double(), x)
        worst = max(worst, ratio)
        assert ratio <= 0.5, (V, rows, kind, ratio)
        if kind == "underflow":
            mx = x.max(-1, keepdim=True).values
            assert np.array_equal(got, (x - mx).numpy()) and (got.max(axis=1) == 0).all()
        if kind == "const":
            assert np.abs(got.astype(np.float64) + np.log(V)).max() <= 4 * fr.EPS32 * 4 + 2e-6
        for name, kw in (("lanes32", dict(lanes=32)), ("le", dict(le=True))):
            bad = torch.from_numpy(fr.lsm_f32(x.numpy(), **kw)).double()
            want, bound, finite = fr.lsm_oracle(x)
            with np.errstate(invalid="ignore"):
                off = (not torch.equal(torch.isneginf(bad), torch.isneginf(want))) or bool(((bad - want).abs()[finite] > bound[finite]).any()) \
                    or not bool(torch.isfinite(bad[finite]).all())
            rejected[name] += int(off)
    print(f"[log-softmax restatement] worst err / bound {worst:.3f}; cases rejecting max-over-32-lanes {rejected['lanes32']}, lane <= V {rejected['le']}")
    assert rejected["lanes32"] >= 5 and rejected["le"] >= 50


# ---- C. reinforce_grad ----
def test_reinforce_restatement_and_c():
    """C = 4 unless the restatement needs more (twice what the whole bound needs, and enough for half); and at every element of
    the table the bound is no looser than the rtol 1e-4 / atol 1e-6 of tests/test_kernels_gpu.py::test_reinforce_grad_vs_oracle."""
    c_pass = 0.0
    for V in fr.REINFORCE_V:
        for T, B in fr.REINFORCE_TB:
            assert (T * B) % 4 != 0 or (T, B) == (9, 4)
            scores, path, coef, lengths = fr.reinforce_case(T, B, V)
            want = decode_ref.reinforce_grad(scores, path, coef, lengths)
            bound = fr.reinforce_bound(coef, want.shape)
            assert (bound <= 1e-6 + 1e-4 * np.abs(want)).all()
            got = fr.reinforce_f32(scores, path, coef, lengths)
            err = np.abs(got.astype(np.float64) - want)
            nz = bound > 0
            assert (err[~nz] == 0).all()
            if nz.any():
                c_pass = max(c_pass, float((err[nz] / (bound[nz] / fr.REINFORCE_C)).max()))
            assert (err <= 0.5 * bound).all(), (T, B, V)
            assert np.abs(want[0, 0, V - 1]) <= 1e-20 * max(abs(float(coef[0])), 1e-30) or V == 1     # p = 1 on the path: g about 0
            assert (got[lengths[None, :].repeat(T, 0) <= np.arange(T)[:, None]] == 0).all()
            if V > 2 and T > 1:
                assert (got[T - 1, 0, 1::3] == 0).all() and (want[T - 1, 0, 1::3] == 0).all()
            # the mistakes
            if V > 1:
                bad = fr.reinforce_f32(scores, path, coef, lengths, shift=1)
                assert (np.abs(bad - want) > bound).any()
            if V > 1 and (lengths < T).any() and np.abs(coef[lengths < T]).max() > 0:
                bad = fr.reinforce_f32(scores, path, coef, lengths, ignore_lengths=True)
                assert (np.abs(bad - want) > bound).any()
    print(f"[reinforce restatement] C = {fr.REINFORCE_C}: worst err / bound {c_pass / fr.REINFORCE_C:.3f}; whole bound from C = {c_pass:.2f}")
    assert fr.REINFORCE_C >= 4 and fr.REINFORCE_C >= 2 * c_pass
    assert fr.REINFORCE_C == 4 or fr.REINFORCE_C / 2 < 2 * c_pass
    assert {abs(c) for c in fr.REINFORCE_COEFS} >= {0.0, 1e-30} and min(fr.REINFORCE_COEFS) < 0


# ---- D. rewards, loss values, batch preparation ----
def test_rewards_restatement():
    worst, worst_loo = 0.0, 0.0
    for B in fr.REWARD_B:
        for K in fr.REWARD_K:
            for kind in fr.REWARD_KINDS:
                dist, tl, rl = fr.reward_case(B, K, kind)
                for loo in (False, True):
                    if loo and K < 2:
                        continue
                    for lens in (None, rl):
                        want = fr.rewards_oracle(dist, tl, K, loo, rl=lens)
                        got = fr.rewards_oracle(dist, tl, K, loo, rl=lens, dtype=np.float32)
                        for i, (g, w) in enumerate(zip(got, want)):
                            if kind == "equal" and i == 2:
                                if not loo:
                                    assert not g.any() and not w.any()                     # equal distances: exactly 0
                                else:
                                    b = fr.reward_loo_equal_bound(K, want[1])
                                    ok = b > 0
                                    assert (g[:, ~ok] == 0).all()
                                    if ok.any():
                                        worst_loo = max(worst_loo, float((np.abs(g)[:, ok] / b[ok]).max()))
                                    assert (np.abs(g) <= 0.5 * b[None, :]).all(), (B, K)
                                continue
                            tol = fr.REWARD_ATOL + fr.REWARD_RTOL * np.abs(w)
                            r = float((np.abs(g - w) / tol).max())
                            worst = max(worst, r)
                            assert r <= 0.5, (B, K, kind, loo, i, r)
    print(f"[rewards restatement] worst err / (atol + rtol |want|) {worst:.3f}; leave-one-out at equal rewards err / bound {worst_loo:.3f}")


def test_loss_value_restatement_and_stride():
    worst = 0.0
    caught = 0
    for T in fr.LOSS_T:
        for V in fr.LOSS_V:
            for flip in (False, True):
                for K, per_frame in ((1, False), (1, True), (4, False)):
                    case = fr.loss_case(T, V, K, flip, per_frame)
                    lp, paths = case[0], case[1]
                    # nothing off the paths is finite
                    on = np.zeros(lp.shape, dtype=bool)
                    tt, bb = np.meshgrid(np.arange(T), np.arange(fr.LOSS_B), indexing="ij")
                    for k in range(K):
                        on[tt, bb, paths[k]] = True
                    assert np.isneginf(lp[~on]).all() and np.isfinite(lp[on]).all()
                    want, bound = fr.loss_oracle(*case, per_frame=per_frame)
                    got = fr.loss_f32(*case, per_frame=per_frame)
                    ok = bound > 0
                    assert (got[~ok] == want[~ok]).all()
                    r = float((np.abs(got - want)[ok] / bound[ok]).max()) if ok.any() else 0.0
                    worst = max(worst, r)
                    assert r <= 0.5, (T, V, K, flip, per_frame, r)
                    if T > 255 and K == 1 and not per_frame:
                        bad = fr.loss_f32(*case, stride=255)
                        caught += int((np.abs(bad - want) > bound).any())
    print(f"[loss value restatement] worst err / bound {worst:.3f}; stride-255 caught in {caught} cases")
    assert caught >= 2 * 3 * 3


def test_batch_prep_tables():
    for T in fr.PREP_T:
        for L in fr.PREP_L:
            fmask, tmask, targets, lens, tls = fr.prep_case(T, L)
            assert targets.max() == 2 ** 31 - 1 and targets.min() >= 0
            assert np.array_equal(fmask.sum(1).astype(np.int32), lens) and np.array_equal(tmask.sum(1).astype(np.int32), tls)
            assert 0 in lens and T in lens and 0 in tls and L in tls


# ---- E. fused head ----
def test_head_restatement_and_mistakes():
    worst = [0.0, 0.0]
    ks = {c[1] // 64 for c in fr.HEAD_CASES}
    assert {3, 5} <= ks and any(c[0] == fr.HEAD_BIG_ROWS and c[1] == 64 and c[2] == 7 for c in fr.HEAD_CASES)
    assert {31, 32, 33} <= {c[0] for c in fr.HEAD_CASES} and any(c[2] == 32 and c[0] % 32 for c in fr.HEAD_CASES)
    assert any(not c[3] and c[4] == 4 for c in fr.HEAD_CASES)
    assert fr.HEAD_BIG_ROWS * 64 * 4 < 34e6 and fr.head_rows_first_pass(fr.HEAD_BIG_ROWS) == fr.HEAD_BIG_ROWS - 33
    for rows, K, V, bias, pad in fr.HEAD_CASES:
        xw, W, b, want = fr.head_case(rows, K, V, bias, pad)
        z, lp = fr.head_f32(xw, W, b, K)
        rz = float((np.abs(z - want["z"]) / want["zb"]).max())
        rl = float((np.abs(lp - want["lp"]) / want["lpb"]).max())
        worst = [max(worst[0], rz), max(worst[1], rl)]
        assert rz <= 0.5 and rl <= 0.5, (rows, K, V, rz, rl)
        if (K // 64) % 2 == 1 and K > 64:
            zb, _ = fr.head_f32(xw, W, b, K, drop_last_chunk=True)
            assert (np.abs(zb - want["z"]) > want["zb"]).any()
        if rows > fr.head_rows_first_pass(rows):
            zb, lb = fr.head_f32(xw, W, b, K, rows_done=fr.head_rows_first_pass(rows))
            assert (np.abs(zb - want["z"]) > want["zb"]).any() and (np.abs(lb - want["lp"]) > want["lpb"]).any()
    print(f"[head restatement] worst err / bound: logits {worst[0]:.3f}, log-probs {worst[1]:.3f}")
