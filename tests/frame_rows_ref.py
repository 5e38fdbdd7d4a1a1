"""Oracles, bounds, fp32 restatements and case tables for the row kernels of csrc/frame_ops.hip (V <= 64: samplers, log-softmax,
REINFORCE gradient, rewards, loss values, batch preparation), the samplers' wide twins (csrc/wide_vocab.hip, csrc/wide_pg.hip) and
the fused CTC head (csrc/head.hip).  A helper, not collected: tests/test_frame_rows_ref_cpu.py holds the restatements to HALF of
every bound (no GPU), tests/test_frame_rows_gpu.py holds the kernels to the whole bound.

Per kernel, as in tests/elementwise_ref.py, none of which calls the kernel:
    oracle        the operation in float64, taken from the fp32 inputs the kernel is given
    bound         per element, from the oracle's own operand magnitudes
    restatement   the kernel's documented formula in numpy float32, one rounding per operation, in the kernel's order of additions;
                  every restatement takes switches for the mistakes the kernel invites, which the bounds must reject

EPS32 = 2^-23 (an fp32 ulp, relative: what tests/test_wide_vocab_gpu.py calls EPS32), U = 2^-24 (the unit roundoff)."""
import functools

import numpy as np
import torch

from oracle import decode_ref, pg_ref

EPS32 = float(np.finfo(np.float32).eps)
U = 2.0 ** -24
F32 = np.float32
NEG_INF = -float("inf")
SENTINEL = -12345.5


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the relative forward error of n fp32 roundings in a row."""
    return n * U / (1.0 - n * U)


def wave_sum_f32(v):
    """common.h wave_sum: the xor butterfly over 64 lanes, (rows, 64) fp32 -> (rows,) fp32 (every lane ends with the same bits)."""
    v = np.asarray(v, dtype=F32)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    assert v.dtype == F32
    return v[:, 0]


def exp_f32(d):
    """fp32 exp as the device's fast exp gives it at the edges: a result under the normal range is 0 (no denormals)."""
    with np.errstate(under="ignore"):
        e = np.exp(np.asarray(d, dtype=F32))
    e[e < F32(2.0 ** -126)] = 0
    assert e.dtype == F32
    return e


def _lanes(x, fill):
    """(rows, V) -> (rows, 64) fp32, lanes past V filled."""
    rows, V = x.shape
    out = np.full((rows, 64), fill, dtype=F32)
    out[:, :V] = x
    return out


# ------------------------------------------------------------------------------------------------------------------------
# A. samplers: k = #{v : c_v <= u * total} clamped to V - 1, c the fp32 Hillis-Steele lane scan of e = exp(x - max), then (rule
#    "fixed", include/pgasr_hip.h A9 / A12) moved off a label with e == 0
# ------------------------------------------------------------------------------------------------------------------------
SAMPLER_SEED = 0x5EED
SAMPLER_STRIDE = 64              # batch_stride of the planted runs: T = 1, every row's utt_id = the planted row
SAMPLER_ROWS = 256
U_MAX = 1.0 - 2.0 ** -24
# name -> (offset, row, u): decode_ref.sampler_uniforms(1, 64, SAMPLER_SEED, offset)[0, row] == u.  Found by a search over offsets
# (u = 3/4: the first 4000 offsets; the other two: about a million).
PLANTED = {"umax": (159170, 20, U_MAX), "uzero": (1127429, 41, 0.0), "u34": (3753, 21, 0.75)}
SAMPLER_K = 4                    # draws of the multi-sample runs
NARROW_V = (2, 8, 29, 64)
WIDE_V = (65, 257, 1024)
CONST_V = (1, 2, 4, 8, 16, 32, 64)
BOUNDARY = 2e-6                  # tests/test_kernels_gpu.py::test_argmax_bit_exact_and_sampler's rule


def wide_nv(V):
    return next(n for n in (1, 2, 4, 8, 16) if 64 * n >= V)


def umax_ms(V, wide):
    """The last non-zero label m of the u-max rows.  Narrow: 0, V // 2, V - 2.  Wide: also inside a lane's group of NV labels and
    on a group's last label."""
    ms = {0, V // 2, max(V - 2, 0)}
    if wide:
        nv = wide_nv(V)
        g = (V // 2) // nv
        ms |= {g * nv + nv // 2 - 1, g * nv + nv - 1}
    return tuple(sorted(ms))


def umax_cases():
    """(V, wide entry, m, kind): kind "inf" / "under" carry the labels after m as -inf / as max - 200; "none" has no zero label
    (m = V - 1)."""
    out = []
    for wide, vs in ((False, NARROW_V), (True, WIDE_V)):
        for V in vs:
            for m in umax_ms(V, wide):
                out += [(V, wide, m, "inf"), (V, wide, m, "under")]
            out.append((V, wide, V - 1, "none"))
    return tuple(out)


def uzero_cases():
    """(V, wide entry, f): labels before f are -inf, so f is the first label with non-zero probability."""
    out = []
    for wide, vs in ((False, NARROW_V), (True, WIDE_V)):
        for V in vs:
            fs = {0, 1, V // 2, V - 1}
            if wide:
                nv = wide_nv(V)
                fs |= {(V // 2) // nv * nv, (V // 2) // nv * nv + nv - 1}
            out += [(V, wide, f) for f in sorted(fs)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def multi_uniforms(name):
    """The SAMPLER_K uniforms of a planted row's counter: draw 0 is PLANTED[name]'s u, draws 1 .. K - 1 whatever Philox gives."""
    offset, row, _ = PLANTED[name]
    return pg_ref.sampler_uniforms(1, [row], SAMPLER_K, SAMPLER_SEED, offset, SAMPLER_STRIDE)[:, 0, 0]


def _draw_rows(make, name):
    """make(rng) of the first seed under which the ORACLE alone stays inside the cap at draws 1 .. K - 1 as well: at most
    sampler_cap rows whose fp64 cdf passes within BOUNDARY of that draw's u at any label (a thousand labels are a thousand
    boundaries per row, so one seed in a few puts two rows of 256 that near).  seed: an int, then [int, attempt]."""
    us = multi_uniforms(name)
    for attempt in range(16):
        x = make(attempt)
        worst = max(int(boundary_rows(planted_oracle(x, u)[1], np.full(len(x), u)).sum()) for u in us[1:])
        if worst <= sampler_cap(len(x)):
            x.setflags(write=False)
            return x
    raise AssertionError("no seed keeps the oracle inside the cap")


@functools.lru_cache(maxsize=None)
def umax_rows(V, m, kind):
    """(SAMPLER_ROWS, V) fp32 scores ~ N(0, 2^2) whose labels after m carry probability 0 in fp32.  Label m's score is made
    non-negative: among a thousand labels a p_m under 2e-6 is common, and then cdf_{m-1} is a second boundary next to u."""
    def make(attempt):
        seed = 1000 * V + 7 * m + len(kind)
        x = (np.random.default_rng(seed if attempt == 0 else [seed, attempt]).normal(size=(SAMPLER_ROWS, V)) * 2).astype(F32)
        x[:, m] = np.abs(x[:, m])
        if kind == "inf":
            x[:, m + 1:] = NEG_INF
        elif kind == "under":
            x[:, m + 1:] = (x[:, :m + 1].max(axis=1, keepdims=True) - F32(200)).astype(F32)
        return x
    return _draw_rows(make, "umax")


@functools.lru_cache(maxsize=None)
def uzero_rows(V, f):
    def make(attempt):
        seed = 2000 * V + f
        x = (np.random.default_rng(seed if attempt == 0 else [seed, attempt]).normal(size=(SAMPLER_ROWS, V)) * 2).astype(F32)
        x[:, :f] = NEG_INF
        return x
    return _draw_rows(make, "uzero")


def zero_e(x):
    """True where exp(x - max) is 0 in fp32: the labels no draw may return."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore"):
        return exp_f32(x - x.max(axis=-1, keepdims=True)) == 0


def planted_oracle(x, u):
    """decode_ref.sample_paths's rule on rows (R, V) that all draw the same known u: (labels (R,), cdf (R, V) fp64)."""
    x64 = np.asarray(x, dtype=np.float64)
    e = np.exp(x64 - x64.max(axis=1, keepdims=True))
    cdf = np.cumsum(e, axis=1) / e.sum(axis=1, keepdims=True)
    return np.minimum((cdf <= u).sum(axis=1), x.shape[1] - 1), cdf


def boundary_rows(cdf, u, lo=None, hi=None):
    """Rows with |cdf_k - u| < BOUNDARY for some k in [lo, hi) (default: every k): the rows the boundary rule may have to excuse."""
    near = np.abs(cdf - np.asarray(u)[..., None]) < BOUNDARY
    return near[..., lo:hi].any(axis=-1)


def sampler_cap(rows):
    return max(1, rows // 1000)


def sampler_scan_f32(x, nv=1, lanes=64):
    """The samplers' cdf in fp32 -> (e, c, total), e and c (rows, V).  nv = 1: frame_argmax_sample_kernel's Hillis-Steele scan over
    the 64 lanes.  nv > 1: the wide kernels' sequential prefix within a lane's nv labels on top of the exclusive scan of the lane
    totals.  lanes = 32 restates a maximum taken over half the wave."""
    x = np.asarray(x, dtype=F32)
    rows, V = x.shape
    mx = x[:, :min(V, lanes * nv)].max(axis=1, keepdims=True)
    e = np.zeros((rows, 64 * nv), dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        e[:, :V] = exp_f32(x - mx)
    run = e.reshape(rows, 64, nv).copy()
    for i in range(1, nv):
        run[:, :, i] = run[:, :, i - 1] + run[:, :, i]
    scan = run[:, :, nv - 1].copy()
    for o in (1, 2, 4, 8, 16, 32):
        scan = np.concatenate([scan[:, :o], scan[:, o:] + scan[:, :-o]], axis=1)
    total = scan[:, 63]
    if nv == 1:
        c = scan
    else:
        excl = np.concatenate([np.zeros((rows, 1), dtype=F32), scan[:, :-1]], axis=1)
        c = (excl[:, :, None] + run).reshape(rows, 64 * nv)
    assert c.dtype == F32 and total.dtype == F32
    return e[:, :V], c[:, :V], total


def skip_zero(k, pos):
    """The fixed rule: k stays where pos[k]; else the nearest label above with pos, else the last label with pos."""
    V = pos.shape[1]
    out = k.copy()
    idx = np.arange(V)
    for r in np.nonzero(~pos[np.arange(len(k)), np.minimum(k, V - 1)])[0]:
        above = idx[(idx >= k[r]) & pos[r]]
        anyp = idx[pos[r]]
        out[r] = above[0] if above.size else (anyp[-1] if anyp.size else k[r])
    return out


def sampler_f32(x, u, rule="fixed", nv=1, thr=None, strict=False, clamp=None, lanes=64):
    """The sampler's documented formula in fp32 at a given u (scalar or per row) -> labels (rows,).  rule "parent": the count alone,
    as the kernels stood before the fix; "fixed": moved off labels with e == 0.  thr: the threshold itself instead of u * total.
    Mistakes: strict (c < thr), clamp = V (instead of V - 1), lanes = 32."""
    e, c, total = sampler_scan_f32(x, nv, lanes)
    V = x.shape[1]
    t = (np.broadcast_to(np.asarray(u, dtype=F32), total.shape) * total) if thr is None else np.broadcast_to(np.asarray(thr, dtype=F32), total.shape)
    assert t.dtype == F32
    k = ((c < t[:, None]) if strict else (c <= t[:, None])).sum(axis=1)
    k = np.minimum(k, V - 1 if clamp is None else clamp)
    return k if rule == "parent" else skip_zero(k, e > 0)


# ------------------------------------------------------------------------------------------------------------------------
# B. log_softmax_rows, V <= 64: tests/test_wide_vocab_gpu.py's bound (moved here), 4 EPS32 max(|x|_max, |lse|) + 2e-6 per element
# ------------------------------------------------------------------------------------------------------------------------
LSM_V = (1, 2, 31, 32, 33, 63, 64)
LSM_ROWS = (1, 3, 4, 5, 4 * 7 + 1)
LSM_KINDS = ("const", "saturated", "shift+", "shift-", "inf_first", "inf_last", "inf_third", "max_last", "underflow")


def lsm_oracle(x):
    """x (.., V) fp32 torch -> (log_softmax in fp64, the per-element bound, the oracle's finite entries)."""
    xd = x.double()
    want = torch.log_softmax(xd, -1)
    finite = torch.isfinite(want)
    lse = torch.logsumexp(xd, -1, keepdim=True)
    mag = torch.maximum(xd.masked_fill(~torch.isfinite(x), 0).abs().amax(-1, keepdim=True), lse.abs())
    return want, (4 * EPS32 * mag + 2e-6).expand_as(want), finite


def lsm_ratio(got, x):
    """Worst err / bound of got (fp64 torch, x's shape) against lsm_oracle(x); the -inf pattern must be the oracle's."""
    want, bound, finite = lsm_oracle(x)
    assert torch.equal(torch.isneginf(got), torch.isneginf(want)) and torch.isfinite(got[finite]).all()
    err = (got - want).abs()
    return float((err[finite] / bound[finite]).max()), float(err[finite].max())


def lsm_check(ops, x, label, dev, tag="wide log-softmax"):
    got = ops.log_softmax_rows(x.to(dev)).cpu().double()
    worst, max_err = lsm_ratio(got, x)
    print(f"[{tag}] {label}: worst err / bound {worst:.2f}, max err {max_err:.2e}")
    assert worst <= 1.0
    return worst


def lsm_cases():
    """(V, rows, kind) for every kind that leaves a finite label in each row."""
    return tuple((V, rows, kind) for V in LSM_V for rows in LSM_ROWS for kind in LSM_KINDS
                 if not (kind.startswith("inf") and V == 1))


def lsm_case(V, rows, kind):
    """(rows, V) fp32 torch.  Rows are N(0, 3^2) with the kind's edit; "underflow": one label (the last one in row 0) at N(0,1),
    every other label more than 200 under it, so that lp is exactly 0 there and exactly x - max elsewhere."""
    g = torch.Generator().manual_seed(100 * V + rows + 7 * LSM_KINDS.index(kind))
    x = torch.randn(rows, V, generator=g) * 3
    r = torch.arange(rows)
    if kind == "const":
        x[:] = torch.randn(rows, 1, generator=g)
    elif kind == "saturated":
        x[r, (r * 5 + V // 2) % V] = 80.0
    elif kind in ("shift+", "shift-"):
        x = x + (1e4 if kind == "shift+" else -1e4)
    elif kind == "inf_first":
        x[:, 0] = NEG_INF
    elif kind == "inf_last":
        x[:, V - 1] = NEG_INF
    elif kind == "inf_third":
        x[:, ::3] = NEG_INF
    elif kind == "max_last":
        x[:, V - 1] += 12.0
    elif kind == "underflow":
        x = -250.0 - 50.0 * torch.rand(rows, V, generator=g)
        x[r, (V - 1 - r * 3) % V] = torch.randn(rows, generator=g)
    return x.float().contiguous()


def lsm_f32(x, lanes=64, le=False):
    """log_softmax_rows_kernel in numpy fp32: wave_max, exp, wave_sum, mx + log, v - lse.  Mistakes: lanes = 32 (the maximum over
    half the wave), le (lane <= V: lane V reads the next row's first label, 0.0 behind the last row)."""
    x = np.asarray(x, dtype=F32)
    rows, V = x.shape
    v = _lanes(x, NEG_INF)
    if le and V < 64:
        v[:, V] = np.append(x[1:, 0], F32(0))
    mx = v[:, :lanes].max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = np.where(np.isneginf(v), F32(0), np.exp(v - mx)).astype(F32)
        lse = mx[:, 0] + np.log(wave_sum_f32(e))
        y = x - lse[:, None]
    assert y.dtype == F32
    return y


# ------------------------------------------------------------------------------------------------------------------------
# C. reinforce_grad against decode_ref.reinforce_grad: |err| <= |coef_b| REINFORCE_C EPS32
# ------------------------------------------------------------------------------------------------------------------------
# g = coef (e / tot - onehot): 2^-24 times (1/2 + |d| for exp(d), where p |d| <= 0.37; up to 3 for the six additions of the wave
# sum; 1/2 each for the quotient, the difference and the product) <= 3 EPS32 |coef| when every rounding goes one way; the
# restatement (an exact exp) is asked for half.  Chosen as ATTN_C is: 4 unless the restatement needs more.
REINFORCE_C = 4
REINFORCE_V = (1, 2, 29, 64)
REINFORCE_TB = ((1, 1), (3, 5), (9, 4))
REINFORCE_COEFS = (0.5, -1.25, 0.0, 1e-30, 2.0)          # |coef| <= 2: C EPS32 |coef| stays under the old test's atol 1e-6


def reinforce_case(T, B, V):
    """fp32 scores (T,B,V), int32 path (T,B), fp32 coef (B,), int32 lengths (B,): lengths cycle through 0, 1, T, T + 3; the path
    label V - 1 in frame 0; utterance 0's frame 0 has p(path) = 1 in fp32; its last frame (T > 1, V > 2) carries -inf at every
    third label from label 1, where g is exactly 0.  Lengths are T, 0, 1, T + 3 in turn."""
    rng = np.random.default_rng(10000 * T + 100 * B + V)
    scores = (rng.normal(size=(T, B, V)) * 2).astype(F32)
    path = rng.integers(0, V, size=(T, B)).astype(np.int32)
    path[0, :] = V - 1
    coef = np.array([REINFORCE_COEFS[(b + T) % len(REINFORCE_COEFS)] for b in range(B)], dtype=F32)
    lengths = np.array([(T, 0, 1, T + 3)[b % 4] for b in range(B)], dtype=np.int32)
    scores[0, 0, :] = -60.0
    scores[0, 0, V - 1] = 0.0                               # p = 1 to fp32 on the path label
    if V > 2 and T > 1:
        scores[T - 1, 0, 1::3] = NEG_INF
        path[T - 1, 0] = 0
    return scores, path, coef, lengths


def reinforce_bound(coef, shape, C=REINFORCE_C):
    return np.broadcast_to((np.abs(np.asarray(coef, dtype=np.float64)) * C * EPS32)[None, :, None], shape)


def reinforce_f32(scores, path, coef, lengths, shift=0, ignore_lengths=False):
    """reinforce_grad_kernel in numpy fp32 (accumulate = 0).  Mistakes: shift = 1 (the one-hot at k + 1), ignore_lengths."""
    T, B, V = scores.shape
    x = _lanes(scores.reshape(T * B, V), NEG_INF)
    mx = x.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.where(np.isneginf(x), F32(0), np.exp(x - mx)).astype(F32)
    tot = wave_sum_f32(e)
    onehot = (np.arange(64)[None, :] == (path.reshape(-1, 1) + shift)).astype(F32)
    g = np.repeat(coef[None, :], T, axis=0).reshape(-1, 1) * (e / tot[:, None] - onehot)
    g = g[:, :V].reshape(T, B, V)
    assert g.dtype == F32
    if not ignore_lengths and lengths is not None:
        g = g * (np.arange(T)[:, None] < lengths[None, :])[..., None].astype(F32)
    return g


# ------------------------------------------------------------------------------------------------------------------------
# D. rewards, loss values, batch preparation
# ------------------------------------------------------------------------------------------------------------------------
MAX_SAMPLES = 16
REWARD_B = (1, 255, 256, 257)
REWARD_K = (1, 2, MAX_SAMPLES)
REWARD_RTOL, REWARD_ATOL = 1e-6, 1e-9                     # tests/test_discrete_kernels_gpu.py's, for these quantities
REWARD_LAM, REWARD_INV_BG = 0.7, 1.0 / 24
REWARD_KINDS = ("extreme", "equal")


def reward_case(B, K, kind):
    """int32 dist (1 + K, B) [hypothesis row, then the K samples], target lengths (B,) cycling 0, 1, 300, reward lengths (B,).
    kind "extreme": distances 0 and 10^6; "equal": one distance per utterance for every row (0, 10^6 or small), where the
    hypothesis baseline gives exactly 0 and leave-one-out only roundings.  (Distances whose rewards nearly cancel are not in the
    table: rtol 1e-6 on a difference of two rounded quotients is not a bound fp32 can meet; tests/test_kernels_gpu.py holds random
    distances to 1e-5.)"""
    rng = np.random.default_rng(100 * B + K + len(kind))
    tl = np.array([(0, 1, 300)[b % 3] for b in range(B)], dtype=np.int32)
    rl = np.array([(7, 0, 1, 300)[b % 4] for b in range(B)], dtype=np.int32)
    if kind == "extreme":
        dist = rng.integers(0, 2, size=(1 + K, B)) * 10 ** 6
    else:
        dist = np.repeat(np.array([(0, 10 ** 6, 17, 3)[b % 4] for b in range(B)])[None, :], 1 + K, axis=0)
    return dist.astype(np.int32), tl, rl


def rewards_oracle(dist, tl, K, loo, lam=REWARD_LAM, inv_bg=REWARD_INV_BG, rl=None, dtype=np.float64):
    """pg_rewards_multi_kernel's documented formula (include/pgasr_hip.h) in ``dtype``: float64 is the oracle, float32 the
    restatement (sums in k order).  dist (1 + K, B): row 0 is the hypothesis row, unused by leave-one-out.  lam and inv_bg as the
    C ABI passes them: rounded to fp32.  -> R_b (B,), R_s (K,B), coef (K,B), utt_scale (B,)."""
    f = dtype
    lam, inv_bg = f(F32(lam)), f(F32(inv_bg))
    Lr = np.maximum(tl if rl is None else rl, 1).astype(f)
    Lt = np.maximum(tl, 1).astype(f)
    scale = (lam * inv_bg) / f(K)
    R_s = -dist[1:].astype(f) / Lr[None, :]
    if not loo:
        R_b = -dist[0].astype(f) / Lr
        coef = scale * (R_s - R_b[None, :])
    else:
        S = np.zeros_like(Lr)
        for k in range(K):
            S = S + R_s[k]
        bk = (S[None, :] - R_s) / f(K - 1)
        coef = scale * (R_s - bk)
        bsum = np.zeros_like(Lr)
        for k in range(K):
            bsum = bsum + bk[k]
        R_b = bsum / f(K)
    us = inv_bg / Lt
    for a in (R_b, R_s, coef, us):
        assert a.dtype == f
    return R_b, R_s, coef, us


def reward_loo_equal_bound(K, R_s, lam=REWARD_LAM, inv_bg=REWARD_INV_BG):
    """Leave-one-out with equal rewards R: S carries K - 1 roundings of up to K|R| U each over K - 1, the quotient, the difference
    and the product one more each: |coef| <= (K + 3) EPS32 scale max|R|."""
    scale = float(F32(lam)) * float(F32(inv_bg)) / K
    return (K + 3) * EPS32 * scale * np.abs(R_s).max(axis=0)


LOSS_T = (1, 255, 256, 257, 513)
LOSS_B = 3
LOSS_V = (1, 29, 64)


def loss_case(T, V, K, flip, per_frame=False):
    """lp (T,B,V) fp32: -inf everywhere but on the K paths; paths (K,T,B) int32; in_len (B,) from {0, 1, T} or {T + 5, T, 1};
    nll, utt_scale (B,); coef (K,B), or (T,B) per frame (K = 1)."""
    B = LOSS_B
    rng = np.random.default_rng(1000 * T + 10 * V + K + (5 if flip else 0))
    paths = rng.integers(0, V, size=(K, T, B)).astype(np.int32)
    lp = np.full((T, B, V), NEG_INF, dtype=F32)
    tt, bb = np.meshgrid(np.arange(T), np.arange(B), indexing="ij")
    for k in range(K):
        lp[tt, bb, paths[k]] = -(rng.random(size=(T, B)) * 8 + 0.01).astype(F32)
    in_len = np.array([T + 5, T, 1] if flip else [0, 1, T], dtype=np.int32)
    nll = (rng.random(B) * 50).astype(F32)
    us = (rng.random(B) * 0.1 + 0.01).astype(F32)
    coef = rng.normal(size=(T, B) if per_frame else (K, B)).astype(F32)
    return lp, paths, in_len, nll, us, coef


def loss_oracle(lp, paths, in_len, nll, us, coef, per_frame=False):
    """terms_b = nll_b us_b - sum_k coef[k,b] sum_{t < T_b} lp[t,b,paths[k,t,b]] (per frame: coef[t,b] inside the sum) in fp64, and
    the bound gamma_n (sum |coef lp| + |nll us|), n = ceil(T_b / 256) + 10 for the single and the multi kernel alike: a thread's
    additions, the eight of the tree, the products and the difference.  (The multi kernel's K - 1 additions over k get no allowance
    of their own: each path's sum uses far less than its share.)"""
    K, T, B = paths.shape
    want, bound = np.zeros(B), np.zeros(B)
    for b in range(B):
        Tb = min(int(in_len[b]), T)
        acc = absacc = 0.0
        for k in range(K):
            v = lp[np.arange(Tb), b, paths[k, :Tb, b]].astype(np.float64)
            c = coef[:Tb, b].astype(np.float64) if per_frame else float(coef[k, b])
            acc += float((c * v).sum())
            absacc += float(np.abs(c * v).sum())
        base = float(nll[b]) * float(us[b])
        want[b] = base - acc
        bound[b] = gamma(-(-Tb // 256) + 10) * (absacc + abs(base))
    return want, bound


def loss_f32(lp, paths, in_len, nll, us, coef, per_frame=False, stride=256):
    """pg_loss_value(_multi)_kernel in numpy fp32: thread i adds frames i, i + stride, .. in t order, then the halving tree over 256
    partial sums; the K products in k order.  Mistake: stride = 255 (frames 255, 510, .. are added twice)."""
    K, T, B = paths.shape
    out = np.zeros(B, dtype=F32)
    for b in range(B):
        Tb = min(int(in_len[b]), T)
        acc = F32(0)
        for k in range(K):
            red = np.zeros(256, dtype=F32)
            for i in range(256):
                for t in range(i, Tb, stride):
                    v = lp[t, b, paths[k, t, b]]
                    red[i] = red[i] + (coef[t, b] * v if per_frame else v)
            o = 128
            while o > 0:
                red[:o] = red[:o] + red[o:2 * o]
                o >>= 1
            acc = acc + (red[0] if per_frame else coef[k, b] * red[0])
        out[b] = nll[b] * us[b] - acc
    return out


PREP_T = (1, 255, 256, 257, 1000)
PREP_L = (1, 256, 257)


def prep_case(T, L):
    """fmask (B,T) fp32, tmask (B,L) int64, targets (B,L) int64 with values up to 2^31 - 1, for lengths 0, full and between."""
    B = 4
    rng = np.random.default_rng(T * 1000 + L)
    lens = np.array([0, T, T // 2, min(T, 1)])
    tls = np.array([L, 0, L // 2, min(L, 1)])
    fmask = (np.arange(T)[None, :] < lens[:, None]).astype(F32)
    tmask = (np.arange(L)[None, :] < tls[:, None]).astype(np.int64)
    targets = rng.integers(0, 2 ** 31, size=(B, L), dtype=np.int64)
    targets[0, 0] = 2 ** 31 - 1
    targets[0, L - 1] = 2 ** 31 - 1
    return fmask, tmask, targets, lens.astype(np.int32), tls.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------------
# E. fused head (pgasr_head_logsoftmax): z = x W^T + b in exact fp32 MFMA, lp = z - lse(z)
# ------------------------------------------------------------------------------------------------------------------------
HEAD_GRID = 1024                 # workgroups at most; 4 waves each, a wave owns 32 rows per pass
HEAD_BIG_ROWS = 4 * 32 * HEAD_GRID + 33
# (rows, K, V, bias, ldx - K): odd chunk counts above one; the second pass of the grid with a ragged last block; rows around one
# block; V = 32 ragged; no bias and a padded leading dimension
HEAD_CASES = (
    (33, 192, 29, True, 0), (70, 320, 29, True, 0), (HEAD_BIG_ROWS, 64, 7, True, 0), (31, 128, 29, True, 0), (32, 128, 29, True, 0),
    (33, 128, 29, True, 0), (45, 64, 32, True, 0), (97, 256, 32, True, 0), (50, 192, 5, False, 4), (129, 64, 1, False, 0),
    (40, 128, 29, True, 4), (33, 1024, 3, True, 0),
)


@functools.lru_cache(maxsize=None)
def head_case(rows, K, V, bias, pad):
    """x (rows, K + pad) fp32 of which the first K columns are the operand (the rest a sentinel that must not be read into the
    result), W (V,K), b (V,) or None -- and the fp64 oracle with its bounds."""
    rng = np.random.default_rng(rows + 10 * K + V)
    xw = np.full((rows, K + pad), 1e6, dtype=F32)
    xw[:, :K] = rng.normal(size=(rows, K)).astype(F32)
    W = (rng.normal(size=(V, K)) / np.sqrt(K)).astype(F32)
    b = rng.normal(size=V).astype(F32) if bias else None
    x64, W64 = xw[:, :K].astype(np.float64), W.astype(np.float64)
    b64 = b.astype(np.float64) if bias else np.zeros(V)
    z = x64 @ W64.T + b64
    zb = gamma(K + 1) * (np.abs(x64) @ np.abs(W64).T + np.abs(b64))
    zt = torch.from_numpy(z)
    lse = torch.logsumexp(zt, -1, keepdim=True).numpy()
    lp = z - lse
    mag = np.maximum(np.abs(z).max(axis=1, keepdims=True), np.abs(lse))
    lpb = zb.max(axis=1, keepdims=True) + (4 * EPS32 * mag + 2e-6) + np.zeros_like(z)
    for a in (xw, W, z, zb, lp, lpb):
        a.setflags(write=False)
    return xw, W, b, {"z": z, "zb": zb, "lp": lp, "lpb": lpb}


def head_f32(xw, W, b, K, rows_done=None, drop_last_chunk=False):
    """The head in numpy fp32 (any order of the k sum is inside the bound) -> (logits, lp), SENTINEL where nothing is written.
    Mistakes: rows_done = head_rows_first_pass(rows) (the second grid pass skipped), drop_last_chunk (the last 64-deep chunk
    dropped when their count is odd and above one)."""
    rows, V = xw.shape[0], W.shape[0]
    kk = K - 64 if (drop_last_chunk and (K // 64) % 2 == 1 and K > 64) else K
    z = xw[:, :kk] @ W[:, :kk].T
    if b is not None:
        z = z + b
    z = z.astype(F32)
    mx = z.max(axis=1, keepdims=True)
    lse = mx + np.log(np.exp(z - mx).sum(axis=1, keepdims=True, dtype=F32))
    lp = (z - lse).astype(F32)
    if rows_done is not None:
        z[rows_done:] = SENTINEL
        lp[rows_done:] = SENTINEL
    return z, lp


def head_rows_first_pass(rows):
    """Rows written by the first pass of the grid-stride loop."""
    return min(rows, 4 * 32 * HEAD_GRID)
