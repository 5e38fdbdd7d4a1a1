"""The bounds of tests/elementwise_ref.py against the reference arithmetic, without a GPU: for every case of its tables the numpy
fp32 restatement of a kernel's documented formula stays within HALF of the bound the kernel itself is held to
(tests/test_elementwise_edges_gpu.py), and the case meets the preconditions its bound was written for.  A bound that plain fp32
arithmetic needs more than half of is a wrong bound; this is where that is found.  The two constants nobody has derived for the
device's expf / tanhf (K of the LSTM cell, C of the attention context) are checked against the rule that chose them.

Worst restatement err / bound (printed with -s): Adam p 0.498, exp_avg 0.468, exp_avg_sq 0.463; LSTM cell c' 0.369, h' 0.491 at
K = 32; attention 0.335 at C = 4.  NOTES.md 0.33."""
import numpy as np
import pytest

import elementwise_ref as er


# ---- A. batch copy: the size tables reach what they claim to reach ----
def test_copy_tables_reach_every_loop_and_cover_every_vector_once():
    assert len(er.COPY_SIZES) == len(set(er.COPY_SIZES)) == 26 and max(er.COPY_SIZES) < 2 ** 20
    assert er.COPY_TYPED_BYTES % 8 == 0 and er.COPY_TYPED_BYTES % 16 != 0
    reached = {}
    for nbytes in er.COPY_SIZES:
        paths, hits = er.copy_paths(nbytes)
        assert (hits == 1).all(), nbytes                      # the model of the two loops writes every vector exactly once
        reached[nbytes] = paths
    want = {"tail only": {"tail"}, "remainder": {"remainder"}, "remainder + tail": {"remainder", "tail"}, "body": {"body"},
            "body + tail": {"body", "tail"}, "body + remainder": {"body", "remainder"}, "all three": {"body", "remainder", "tail"}}
    for what, paths in want.items():
        assert paths in reached.values(), what
    # 16384 vectors are exactly one pass of the 8-deep body with 8 workgroups: one vector fewer and the last lane takes the
    # remainder loop for all eight of its vectors, one more and lane 0 takes it once behind the body
    assert er.copy_paths(16384 * 16)[0] == {"body"} and er.copy_paths(2049 * 16)[0] == {"remainder"}
    assert er.copy_paths(16383 * 16)[0] == er.copy_paths(16385 * 16)[0] == {"body", "remainder"}
    for wg, nbytes in er.COPY_WORKGROUP_CASES:
        paths, hits = er.copy_paths(nbytes, wg)
        assert (hits == 1).all()
    assert er.copy_paths(er.COPY_WORKGROUP_CASES[0][1], 1)[0] == {"body", "remainder", "tail"}
    assert er.copy_paths(er.COPY_WORKGROUP_CASES[1][1], 1024)[0] == {"remainder", "tail"}
    assert er.copy_paths(er.COPY_WORKGROUP_CASES[2][1], 64)[0] == {"body", "remainder"} and er.COPY_WORKGROUP_CASES[2][1] > 2 ** 21
    src = er.copy_source(64, 0)
    assert np.isnan(src.view("<f4")[:4]).all() and np.isinf(src.view("<f4")[4:6]).all()
    assert er.copy_source(3, 0).shape == (3,)


# ---- B. Adam ----
def test_adam_oracle_rounds_the_hyper_parameters_first():
    """1 - beta from the fp32 beta is the kernel's fp32 1.f - beta exactly for beta in [0.5, 1); the exact decimal 0.999 is not
    what any fp32 Adam computes with (1.3e-5 relative in exp_avg_sq: the oracle's matter, not a kernel's)."""
    for name in er.ADAM_HYPER:
        _, b1, b2, _, _ = er.adam_hyper32(name)
        for b in (b1, b2):
            assert 0.5 <= float(b) < 1.0
            assert float(np.float32(1) - b) == 1.0 - float(b)
    assert abs((1.0 - float(np.float32(0.999))) / (1.0 - 0.999) - 1.0) > 1e-5
    assert er.adam_oracle(*(np.ones(1, np.float32),) * 4, 1, "default")["r_t"] == pytest.approx(6.1e-5, rel=0.01)
    assert er.adam_oracle(*(np.ones(1, np.float32),) * 4, 1000, "default")["r_t"] == pytest.approx(4.7e-8, rel=0.01)


def _adam_check(p, g, m, v, t, name, label, worst):
    want = er.adam_oracle(p, g, m, v, t, name)
    er.adam_preconditions(p, g, m, v, want)
    p2, m2, v2 = er.adam_f32(p, g, m, v, t, name)
    r = er.adam_ratios(p2, m2, v2, want)
    print(f"[adam restatement] {label} t={t}: err / bound p {r[0]:.3f} exp_avg {r[1]:.3f} exp_avg_sq {r[2]:.3f}")
    assert max(r) <= 0.5, (label, t, r)
    for k in range(3):
        worst[k] = max(worst[k], r[k])
    zero, cancel = er.adam_index_sets(p.shape[0])
    if zero.size and er.ADAM_HYPER[name][4] == 0:            # g = m = v = 0 and no decay: nothing moves, bit for bit
        assert np.array_equal(p2[zero].view(np.uint32), p[zero].view(np.uint32)) and not m2[zero].any() and not v2[zero].any()
        assert not want["u"][zero].any()
    return p2, m2, v2, want


def test_adam_restatement_within_half_of_the_bounds():
    worst = [0.0, 0.0, 0.0]
    cancelled = 0
    for name, p_zero in er.ADAM_CHAINS:
        p, m, v = er.adam_state(er.ADAM_CHAIN_N, name, 11, p_zero=p_zero, fresh=True)
        for k, t in enumerate(er.ADAM_CHAIN_T):
            g = er.adam_grad(p, m, name, 100 + k, call=k)
            p2, m2, v2, want = _adam_check(p, g, m, v, t, name, f"chain {name} p0={p_zero}", worst)
            if p_zero and k == 0:                            # p' = -u: the update itself against E_u, and 2 eps |u| is a quarter of it at most
                assert not p.any() and (want["E_p"] <= 1.25 * want["E_u"]).all()
            # the cancel set really cancels: |m'| is a rounding of its operands
            hit = np.abs(want["m"]) < 1e-6 * np.abs(float(er.adam_hyper32(name)[1]) * m.astype(np.float64))
            cancelled += int(hit.sum())
            p, m, v = p2, m2, v2
    assert cancelled >= 100
    for n, t in er.ADAM_SINGLE:
        for name in er.ADAM_HYPER:
            p, m, v = er.adam_state(n, name, n)
            _adam_check(p, er.adam_grad(p, m, name, n + 1), m, v, t, name, f"single n={n} {name}", worst)
    print(f"[adam restatement] worst err / bound: p {worst[0]:.3f} exp_avg {worst[1]:.3f} exp_avg_sq {worst[2]:.3f}")


# ---- D. LSTM cell ----
def test_lstm_cell_restatement_and_k():
    """K is the smallest power of two at which the restatement stays within half of E_c and E_h on the whole table; that is never
    below 4 nor below twice the smallest K at which it stays within the whole bound (the bounds are affine in K)."""
    k_pass, k_half, worst = 0.0, 0.0, {"c": 0.0, "h": 0.0}
    saturated = 0
    for B, H in er.LSTM_SHAPES:
        for gs, cs in er.LSTM_SCALES:
            gh, xp, c, _ = er.lstm_case(B, H, gs, cs)
            want = er.lstm_oracle(gh, xp, c)
            er.lstm_preconditions(gh, xp, c, want)
            w0, w1 = er.lstm_oracle(gh, xp, c, K=0), er.lstm_oracle(gh, xp, c, K=1)
            c2, h2 = er.lstm_f32(gh, xp, c)
            assert np.isfinite(c2).all() and np.isfinite(h2).all()
            saturated += int((np.abs(gh + xp) > 88.8).sum())
            for key, got in (("c", c2), ("h", h2)):
                err = np.abs(got.astype(np.float64) - want[key])
                ratio = float((err / want["E_" + key]).max())
                b0, b1 = w0["E_" + key], w1["E_" + key] - w0["E_" + key]
                ok = b1 > 0                                  # (b1 = 0 only where the output is exactly 0: nothing to bound)
                k_pass = max(k_pass, float(((err - b0)[ok] / b1[ok]).max()))
                k_half = max(k_half, float(((2 * err - b0)[ok] / b1[ok]).max()))
                worst[key] = max(worst[key], ratio)
                print(f"[lstm cell restatement] B={B} H={H} scales ({gs:g}, {cs:g}) {key}': err / bound {ratio:.3f}")
                assert ratio <= 0.5, (B, H, gs, cs, key, ratio)
    print(f"[lstm cell restatement] K = {er.LSTM_K}: worst err / bound c' {worst['c']:.3f} h' {worst['h']:.3f}; "
          f"whole bound from K = {k_pass:.2f}, half from K = {k_half:.2f}; {saturated} gates with |s| > 88.8 (fp32 exp overflows or underflows)")
    assert saturated >= 100
    assert er.LSTM_K >= 4 and er.LSTM_K >= 2 * k_pass and er.LSTM_K >= k_half
    assert er.LSTM_K / 2 < max(4.0, 2 * k_pass, k_half)       # and no power of two more than it needs


# ---- E. attention context ----
def test_attention_restatement_and_c():
    """C is 4 unless the restatement needs more: at least twice the C at which the restatement meets the whole bound, and enough
    for half of it."""
    c_pass, c_half, worst = -np.inf, -np.inf, 0.0
    shapes = set()
    for case in er.ATTN_CASES:
        d, e = er.attn_case(*case)
        want = er.attn_oracle(d, e)
        er.attn_preconditions(want)
        got = er.attn_f32(d, e)
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - want["c"])
        ratio = float((err / er.attn_bound(want)).max())
        b0 = er.attn_bound(want, C=0)
        b1 = er.attn_bound(want, C=1) - b0
        c_pass = max(c_pass, float(((err - b0) / b1).max()))
        c_half = max(c_half, float(((2 * err - b0) / b1).max()))
        worst = max(worst, ratio)
        shapes.add(case[:4])
        print(f"[attention restatement] L,B,H,T,scale={case[:5]}: err / bound {ratio:.3f}, max |d e| {want['X'].max():.1f}, "
              f"max |m1 - m2| {want['shift']:.1f}, max |c| {np.abs(want['c']).max():.2e}, err / max |c| {err.max() / np.abs(want['c']).max():.1e}")
        assert ratio <= 0.5, (case, ratio)
    print(f"[attention restatement] C = {er.ATTN_C}: worst err / bound {worst:.3f}; whole bound from C = {c_pass:.2f}, half from C = {c_half:.2f}")
    assert shapes == {(1, 2, 64, 3), (3, 2, 37, 5), (2, 3, 257, 4), (1, 1, 1, 1), (2, 2, 300, 3), (1, 2, 512, 2), (1, 1, 256, 1)}
    assert er.ATTN_C >= 4 and er.ATTN_C >= 2 * c_pass and er.ATTN_C >= c_half
    assert er.ATTN_C == 4 or er.ATTN_C / 2 < max(2 * c_pass, c_half)
    # the large-product case is large: the shifts m1, m2 are what keeps the kernel's fp32 sums finite there
    d, e = er.attn_case(*er.ATTN_CASES[4])
    want = er.attn_oracle(d, e)
    assert want["X"].max() > 60 and np.abs(want["c"]).max() > 1e25


# ---- the bounds tell a wrong kernel from a right one ----
def test_bounds_reject_plausible_mistakes():
    """Each bound is tight enough to fail the mistakes these kernels invite: a bias correction that counts calls instead of
    applied updates (t off by one), a dropped weight decay, eps under the root, gates in another order, a sigmoid good to 1e-5
    only, the softmax a textbook attention would take, and a sign rule of the shifts that ignores the sign."""
    name = "decay"
    p, m, v = er.adam_state(1027, name, 3)
    g = er.adam_grad(p, m, name, 4)
    for t in (1, 2, 3, 10):
        want = er.adam_oracle(p, g, m, v, t, name)
        assert max(er.adam_ratios(*er.adam_f32(p, g, m, v, t, name), want)) <= 0.5
        assert er.adam_ratios(*er.adam_f32(p, g, m, v, t + 1, name), want)[0] > 1            # p only: the moments do not see t
    want = er.adam_oracle(p, g, m, v, 1000, name)
    assert min(er.adam_ratios(*er.adam_f32(p, g, m, v, 1000, "default"), want)) > 1          # no decay: p, m and v all off
    lr, b1, b2, eps, wd = er.adam_hyper32("coarse")
    pc, mc, vc = er.adam_state(1027, "coarse", 3)
    gc = er.adam_grad(pc, mc, "coarse", 4)
    want = er.adam_oracle(pc, gc, mc, vc, 1000, "coarse")
    _, m2, v2 = er.adam_f32(pc, gc, mc, vc, 1000, "coarse")
    with np.errstate(under="ignore"):
        bc2 = np.float32(1) - np.power(b2, np.float32(1000))
    wrong = pc - lr * m2 / np.sqrt(v2 / bc2 + eps * eps)                                     # (bc1 is 1 at t = 1000)
    assert float((np.abs(wrong.astype(np.float64) - want["p"]) / want["E_p"]).max()) > 1

    gh, xp, c, _ = er.lstm_case(3, 37, 1.0, 1.0)
    want = er.lstm_oracle(gh, xp, c)
    ratio = lambda got, key: float((np.abs(got.astype(np.float64) - want[key]) / want["E_" + key]).max())
    H = 37
    swapped = np.concatenate([gh[:, :2 * H], gh[:, 3 * H:], gh[:, 2 * H:3 * H]], axis=1), np.concatenate([xp[:, :2 * H], xp[:, 3 * H:], xp[:, 2 * H:3 * H]], axis=1)
    assert ratio(er.lstm_f32(*swapped, c)[0], "c") > 1                                       # i, f, o, g
    c2, _ = er.lstm_f32(gh, xp, c)
    f = 1.0 / (1.0 + np.exp(-(gh.astype(np.float64) + xp)[:, H:2 * H]))
    assert ratio(c2 + (1e-5 * f * c).astype(np.float32), "c") > 1                            # forget gate good to 1e-5 relative

    d, e = er.attn_case(*er.ATTN_CASES[1])
    want = er.attn_oracle(d, e)
    x = np.einsum("lbr,bik->lbirk", d.astype(np.float64), e.astype(np.float64))
    a = np.exp(x); a = a / a.sum(-1, keepdims=True)
    textbook = (a * e.astype(np.float64)[None, :, :, None, :]).sum(axis=(2, 3))
    assert float((np.abs(textbook - want["c"]) / er.attn_bound(want)).max()) > 1
    assert float((np.abs(want["c"] * (1 + 1e-4) - want["c"]) / er.attn_bound(want)).max()) > 1   # an exp good to 1e-4 only
