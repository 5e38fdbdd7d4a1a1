"""Oracles, bounds, fp32 restatements and case tables for the small kernels of csrc/optim.hip (batch copy, Adam, error flag) and
csrc/attention.hip (decoder LSTM cell, attention context).  A helper, not collected: tests/test_elementwise_ref_cpu.py holds the
restatements to HALF of every bound (no GPU), tests/test_elementwise_edges_gpu.py holds the kernels to the whole bound.

Three things per kernel, none of which calls the kernel:
    oracle        the operation in numpy float64, taken from the fp32 inputs the kernel is given
    bound         per element, from the oracle's own operand magnitudes (so it holds where a sum cancels)
    restatement   the kernel's documented formula in numpy float32, one rounding per operation, no fused multiply-add

eps = 2^-24 (half an fp32 ulp, relative) and FL = 2^-125 (a floor under which nothing is asked) throughout."""
import numpy as np

from oracle import attn_ref

EPS = 2.0 ** -24
FL = 2.0 ** -125
F32 = np.float32
F32_MAX = float(np.finfo(np.float32).max)


def ulp32(x):
    """Distance from fp32(x) to the next fp32 away from zero."""
    return float(np.spacing(np.abs(F32(x))))


# ------------------------------------------------------------------------------------------------------------------------
# A. batch copy (pgasr_stream_copy): a byte oracle, so only sizes, sources and a host model of the kernel's loops live here
# ------------------------------------------------------------------------------------------------------------------------
COPY_WORKGROUPS = 8                      # hipops.stream_copy's default: one pass of the 8-deep body is 8 * 8 * 256 vectors
COPY_N16 = (0, 1, 2047, 2048, 2049, 16383, 16384, 16385, 3 * 16384 + 5)
COPY_TAIL = (0, 1, 15)
COPY_SIZES = tuple(n16 * 16 + tail for n16 in COPY_N16 for tail in COPY_TAIL if (n16, tail) != (0, 0))
# (workgroups, bytes): one workgroup for everything; almost every lane idle; 2 MiB through 64 workgroups (one body pass + 3 vectors)
COPY_WORKGROUP_CASES = ((1, 2049 * 16 + 7), (1024, 5 * 16 + 3), (64, (8 * 64 * 256 + 3) * 16))
COPY_TYPED_BYTES = 2049 * 16 + 8         # the size that also runs as int64 and float32 (a multiple of 8: whole elements)
# quiet and signalling NaNs with payloads, both infinities, -0.0, the smallest denormal: a copy through a float register that
# canonicalised any of them would change these bytes
COPY_BIT_PATTERNS = (0x7FC00000, 0x7F800001, 0xFFC12345, 0x7FBFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001)
COPY_FILL = 0xA5


def copy_source(nbytes, seed):
    """nbytes random bytes whose leading float32 words hold COPY_BIT_PATTERNS (as many as fit)."""
    src = np.random.default_rng(seed).integers(0, 256, size=nbytes, dtype=np.uint8)
    k = min(len(COPY_BIT_PATTERNS), nbytes // 4)
    src[:4 * k] = np.array(COPY_BIT_PATTERNS[:k], dtype="<u4").view(np.uint8)
    return src


def copy_paths(nbytes, workgroups=COPY_WORKGROUPS):
    """Host model of stream_copy_kernel's loops: which of them a size reaches, and how often each 16-byte vector is written.
    -> (set of "body" / "remainder" / "tail", per-vector write counts)."""
    n16, tail = nbytes // 16, nbytes % 16
    stride = workgroups * 256
    i = np.arange(stride, dtype=np.int64)
    hits = np.zeros(n16, dtype=np.int64)
    paths = set()
    while True:
        live = i + 7 * stride < n16
        if not live.any():
            break
        paths.add("body")
        for k in range(8):
            np.add.at(hits, i[live] + k * stride, 1)
        i = np.where(live, i + 8 * stride, i)
    while True:
        live = i < n16
        if not live.any():
            break
        paths.add("remainder")
        np.add.at(hits, i[live], 1)
        i = np.where(live, i + stride, i)
    if tail:
        paths.add("tail")
    return paths, hits


# ------------------------------------------------------------------------------------------------------------------------
# B. Adam (pgasr_adam_step): one fp64 step from the fp32 state the kernel is given
# ------------------------------------------------------------------------------------------------------------------------
# name -> (lr, beta1, beta2, eps, weight_decay, scale of the gradients).  The betas stay in [0.5, 1): there fp32 1 - beta is exact.
ADAM_HYPER = {
    "default": (5e-4, 0.9, 0.999, 1e-8, 0.0, 0.1),
    "decay": (5e-4, 0.9, 0.999, 1e-8, 0.01, 0.1),
    "coarse": (1e-2, 0.5, 0.9, 1e-3, 0.1, 10.0),
}
ADAM_CHAIN_N = 10007
ADAM_CHAIN_T = (1, 2, 3, 10, 1000, 20000)
# (hyper-parameter set, p starts at zero).  From p = 0, p' = -u: the update itself is held to E_u, not hidden under 2 eps |p|.
ADAM_CHAINS = (("default", False), ("decay", False), ("coarse", False), ("default", True))
# n -> t of the single call at that n.  2^21 + 7: the grid is capped at 2048 * 256 lanes of 4, so lane 0 runs a second full quad
# and lane 1 the 3-element tail behind it.
ADAM_SINGLE = ((1, 1), (3, 2), (4, 3), (5, 10), (1023, 1000), (1027, 20000), (2 ** 21 + 7, 3))


def adam_hyper32(name):
    """(lr, beta1, beta2, eps, weight_decay) as the C ABI receives them: rounded to fp32."""
    return tuple(F32(x) for x in ADAM_HYPER[name][:5])


def adam_index_sets(n):
    """(zero, cancel): indices whose g, m, v are all zero, and indices whose gradient is built so that m' cancels."""
    i = np.arange(n)
    return i[i % 7 == 3], i[i % 7 == 5]


def adam_state(n, name, seed, p_zero=False, fresh=False):
    """fp32 (p, m, v): a state in mid-training (fresh: the zero moments of a new optimiser).  No denormals: |m| and sqrt(v) are
    N(0, (0.1 s)^2) draws, and the zero set holds exact zeros."""
    rng = np.random.default_rng(seed)
    s = ADAM_HYPER[name][5]
    p = rng.normal(size=n).astype(F32)
    m = (rng.normal(size=n) * 0.1 * s).astype(F32)
    v = ((rng.normal(size=n) * 0.1 * s) ** 2).astype(F32)
    if p_zero:
        p[:] = 0
    if fresh:
        m[:] = 0; v[:] = 0
    zero, _ = adam_index_sets(n)
    m[zero] = 0; v[zero] = 0
    return p, m, v


def adam_grad(p, m, name, seed, call=None):
    """fp32 gradient for one call on the state (p, m): N(0, s^2); zero on the zero set; on the cancel set (where m != 0) the
    fp32 nearest to -beta1 m / (1 - beta1) - wd p, so that a = beta1 m and b = (1 - beta1) g' cancel to within a rounding.
    In a chain, call k takes every eighth element of the cancel set, starting at the k-th: an m' that cancelled once is some
    1e-8 |m|, and cancelling the same element call after call would walk the state down to a denormal."""
    _, b1, _, _, wd = (float(x) for x in adam_hyper32(name))
    n = p.shape[0]
    g = (np.random.default_rng(seed).normal(size=n) * ADAM_HYPER[name][5]).astype(F32)
    zero, cancel = adam_index_sets(n)
    if call is not None:
        cancel = cancel[call % 8::8]
    cancel = cancel[np.abs(m[cancel]) >= 2.0 ** -40]
    g[cancel] = (-b1 * m[cancel].astype(np.float64) / (1.0 - b1) - wd * p[cancel].astype(np.float64)).astype(F32)
    g[zero] = 0
    return g


def adam_oracle(p, g, m, v, t, name):
    """One Adam step in fp64 from fp32 (p, g, m, v) at bias-correction count t, and the bounds E_p, E_m, E_v, E_u (all from the
    oracle's own quantities).  r_t allows powf 2 ulp through the two corrections formed in fp32."""
    lr, b1, b2, eps, wd = (float(x) for x in adam_hyper32(name))
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    wp = wd * p
    gp = g + wp
    a = b1 * m
    b = (1.0 - b1) * gp
    m2 = a + b
    v2 = b2 * v + (1.0 - b2) * gp * gp
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    den = np.sqrt(v2) / np.sqrt(bc2) + eps
    u = (lr / bc1) * m2 / den
    p2 = p - u
    E_g = 2 * EPS * (np.abs(g) + np.abs(wp)) if wd != 0 else np.zeros_like(g)
    E_m = 4 * EPS * (np.abs(a) + np.abs(b)) + (1.0 - b1) * E_g + FL
    E_v = 6 * EPS * v2 + (1.0 - b2) * (2 * np.abs(gp) * E_g + E_g ** 2) + FL
    r_t = 2 * ulp32(b1 ** t) / bc1 + ulp32(b2 ** t) / bc2
    E_u = (lr / bc1) * E_m / den + np.abs(u) * (8 * EPS + r_t + E_v / (2 * np.maximum(v2, FL)))
    E_p = E_u + 2 * EPS * np.abs(p2)
    return {"p": p2, "m": m2, "v": v2, "u": u, "E_p": E_p, "E_m": E_m, "E_v": E_v, "E_u": E_u, "r_t": r_t}


def adam_f32(p, g, m, v, t, name):
    """The kernel's documented formula in numpy fp32 (optim.hip: adam_kernel), one rounding per operation -> (p', m', v')."""
    lr, b1, b2, eps, wd = adam_hyper32(name)
    one = F32(1)
    with np.errstate(under="ignore"):
        bc1 = one - np.power(b1, F32(t))
        bc2_sqrt = np.sqrt(one - np.power(b2, F32(t)))
    step = lr / bc1
    gk = g + wd * p
    m2 = b1 * m + (one - b1) * gk
    v2 = b2 * v + (one - b2) * gk * gk
    p2 = p - step * m2 / (np.sqrt(v2) / bc2_sqrt + eps)
    assert p2.dtype == m2.dtype == v2.dtype == F32
    return p2, m2, v2


def adam_ratios(got_p, got_m, got_v, want):
    """Worst err / bound of (p, m, v) against an adam_oracle result."""
    return tuple(float((np.abs(np.asarray(got, dtype=np.float64) - want[k]) / want["E_" + k]).max())
                 for got, k in ((got_p, "p"), (got_m, "m"), (got_v, "v")))


def adam_preconditions(p, g, m, v, want):
    """Finite everywhere, no denormal state: a nonzero |m| or v of the state given and a nonzero v' lie in [2^-100, 2^100]."""
    for x in (p, g, m, v, want["p"], want["m"], want["v"], want["E_p"]):
        assert np.isfinite(x).all()
    for x in (np.abs(m), v, want["v"]):
        nz = np.asarray(x, dtype=np.float64)
        nz = nz[nz != 0]
        assert nz.size == 0 or (nz.min() >= 2.0 ** -100 and nz.max() <= 2.0 ** 100)
    assert (np.asarray(v) >= 0).all()


# ------------------------------------------------------------------------------------------------------------------------
# D. decoder LSTM cell (pgasr_lstm_cell_f32): gate order i, f, g, o; s = gh + xp per gate
# ------------------------------------------------------------------------------------------------------------------------
LSTM_SHAPES = ((1, 1), (3, 37), (5, 64), (2, 300), (7, 256))
LSTM_SCALES = ((1.0, 1.0), (6.0, 50.0), (30.0, 1.0), (30.0, 1e4))        # (gates, c).  At 30 expf overflows: the gate must be 0 or 1
LSTM_K = 32          # chosen by tests/test_elementwise_ref_cpu.py::test_lstm_cell_restatement_and_k (NOTES.md 0.33)
LSTM_GATE_UNDER = -87.0   # a sigmoid of less than this is under fp32's normal range (ln 2^-126 = -87.3) or about to be


def lstm_case(B, H, gate_scale, c_scale):
    """fp32 gh, xp (B,4H) ~ N(0, gate_scale^2) each, c (B,H) ~ N(0, c_scale^2), h (B,H) ~ N(0,1) (an input the cell must overwrite).
    Beside a forget gate under fp32's normal range c is scaled by 2^-20, so that the product such a gate drops when it comes
    out as 0 stays under the floor (lstm_preconditions): the analogue of not building a denormal Adam state."""
    rng = np.random.default_rng(1000 * B + H + int(gate_scale) + int(c_scale))
    gh = (rng.normal(size=(B, 4 * H)) * gate_scale).astype(F32)
    xp = (rng.normal(size=(B, 4 * H)) * gate_scale).astype(F32)
    c = (rng.normal(size=(B, H)) * c_scale).astype(F32)
    h = rng.normal(size=(B, H)).astype(F32)
    c[(gh + xp)[:, H:2 * H] < LSTM_GATE_UNDER] *= F32(2.0 ** -20)
    return gh, xp, c, h


def lstm_oracle(gh, xp, c, K=LSTM_K):
    """fp64 c', h' of one cell step and the sensitivity bounds E_c, E_h with the one constant K (affine in K)."""
    gh, xp, c = (np.asarray(x, dtype=np.float64) for x in (gh, xp, c))
    H = c.shape[1]
    s = gh + xp
    E_s = EPS * (np.abs(gh) + np.abs(xp))
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    gate = lambda k: (s[:, k * H:(k + 1) * H], E_s[:, k * H:(k + 1) * H])
    (si, Ei), (sf, Ef), (sg, Eg), (so, Eo) = gate(0), gate(1), gate(2), gate(3)
    dsig = lambda x, E: sig(x) * sig(-x) * E + K * EPS * sig(x)          # sigma (1 - sigma) E_s + K eps sigma
    i, f, o, g = sig(si), sig(sf), sig(so), np.tanh(sg)
    dg = Eg / np.cosh(sg) ** 2 + K * EPS * np.abs(g)                    # (1 - g^2) E_s + K eps |g|
    c2 = f * c + i * g
    E_c = FL + dsig(sf, Ef) * np.abs(c) + dsig(si, Ei) * np.abs(g) + i * dg + K * EPS * (np.abs(f * c) + np.abs(i * g))
    tc = np.tanh(c2)
    h2 = o * tc
    with np.errstate(over="ignore"):                                     # cosh of a saturated c' is inf: 1 - tanh^2 is 0 there
        E_h = FL + dsig(so, Eo) * np.abs(tc) + o * (E_c / np.cosh(c2) ** 2 + K * EPS * np.abs(tc)) + 2 * EPS * np.abs(h2)
    return {"c": c2, "h": h2, "E_c": E_c, "E_h": E_h}


def lstm_preconditions(gh, xp, c, want):
    """Finite, and no forget gate under fp32's normal range beside a large c.  A sigmoid below 2^-126 (expf has overflowed, or
    the quotient is a denormal) comes out as 0 or with a few bits, an error of up to its whole value, which K eps sigma does not
    grant.  Times |g| <= 1 or |tanh c'| <= 1 (input and output gate) that is under FL / 2; times c it must be as well."""
    for x in (want["c"], want["h"], want["E_c"], want["E_h"]):
        assert np.isfinite(x).all()
    H = c.shape[1]
    sf = (np.asarray(gh, dtype=np.float64) + np.asarray(xp, dtype=np.float64))[:, H:2 * H]
    f = 1.0 / (1.0 + np.exp(-sf))
    under = f < 2.0 ** -126
    assert (f[under] * np.abs(c[under]) <= FL / 2).all()


def lstm_f32(gh, xp, c):
    """lstm_cell_kernel's formula in numpy fp32 with accurate exp / tanh -> (c', h')."""
    H = c.shape[1]
    one = F32(1)
    s = gh + xp
    with np.errstate(over="ignore", under="ignore"):
        sig = lambda x: one / (one + np.exp(-x))
        i, f, o = sig(s[:, :H]), sig(s[:, H:2 * H]), sig(s[:, 3 * H:])
        c2 = f * c + i * np.tanh(s[:, 2 * H:3 * H])
        h2 = o * np.tanh(c2)
    assert c2.dtype == h2.dtype == F32
    return c2, h2


# ------------------------------------------------------------------------------------------------------------------------
# E. attention context (pgasr_attention_ctx) against oracle.attn_ref.attention_ctx, one query block of B rows at a time
# ------------------------------------------------------------------------------------------------------------------------
# (L, B, H, T, scale of d and e, seed).  Seeds are picked so that every case meets attn_preconditions.
ATTN_CASES = (
    (1, 2, 64, 3, 0.5, 1),       # golden-like
    (3, 2, 37, 5, 1.0, 1),       # H < 64 and NQ = 3 B
    (2, 3, 257, 4, 1.0, 1),      # the second 256-column tile holds one column
    (1, 1, 1, 1, 2.0, 1),
    (2, 2, 300, 3, 2.5, 1),      # large products
    (1, 2, 512, 2, 2.0, 1),
    (1, 1, 256, 1, 1.0, 1),      # exactly one full tile, T = 1
)
ATTN_X_MAX = 80.0
ATTN_C = 4           # chosen by tests/test_elementwise_ref_cpu.py::test_attention_restatement_and_c (NOTES.md 0.33)


def attn_case(L, B, H, T, scale, seed):
    rng = np.random.default_rng(seed)
    d = (rng.normal(size=(L, B, H)) * scale).astype(F32)
    e = (rng.normal(size=(B, T, H)) * scale).astype(F32)
    return d, e


def attn_oracle(d, e):
    """fp64 context (L,B,H) from oracle.attn_ref, block by block, with what the bound and the preconditions need:
    A[l,b,k] = sum_i |e_ik| S1 / S2, X[l,b] = max |d_r e_k| over the query's frames, the largest |m1 - m2| and the largest of the
    reference's own (unshifted) sums S1, S2."""
    L, B, H = d.shape
    c = np.stack([attn_ref.attention_ctx(d[l], e) for l in range(L)])
    d64, e64 = d.astype(np.float64), e.astype(np.float64)
    x = np.einsum("lbr,bik->lbirk", d64, e64)                # [l,b,i,r,k] = d_r e_k
    ex = np.exp(x)
    S1, S2 = ex.sum(axis=3), ex.sum(axis=4)                  # over r per k; over k' per row (used at index k: the quirk)
    A = (np.abs(e64)[None] * S1 / S2).sum(axis=2)
    direct = (e64[None] * S1 / S2).sum(axis=2)
    X = np.abs(x).max(axis=(2, 3, 4))
    shift = np.abs(x.max(axis=3) - x.max(axis=4)).max()
    return {"c": c, "A": A, "X": X, "direct": direct, "shift": float(shift), "S_max": float(max(S1.max(), S2.max()))}


def attn_bound(want, C=ATTN_C):
    return (C * EPS * (1.0 + want["X"][..., None]) + 2e-6) * want["A"] + FL


def attn_preconditions(want):
    assert np.isfinite(want["c"]).all() and np.isfinite(want["A"]).all()
    assert want["X"].max() <= ATTN_X_MAX and want["shift"] <= ATTN_X_MAX
    assert want["S_max"] < F32_MAX and np.abs(want["c"]).max() < F32_MAX and want["A"].max() < F32_MAX
    # the shifted oracle and the sums taken as the reference takes them are one function while nothing overflows
    assert np.abs(want["direct"] - want["c"]).max() <= 1e-12 * want["A"].max()


def attn_f32(d, e):
    """attention_ctx_kernel's formula in numpy fp32: m1, m2 by the kernel's sign rule, both sums over r in index order."""
    L, B, H = d.shape
    T = e.shape[1]
    out = np.zeros((L, B, H), dtype=F32)
    zero = F32(0)
    with np.errstate(under="ignore"):
        for l in range(L):
            for b in range(B):
                dq = d[l, b]
                dmax, dmin = dq.max(), dq.min()
                acc = np.zeros(H, dtype=F32)
                for i in range(T):
                    ei = e[b, i]
                    emax, emin = ei.max(), ei.min()
                    m1 = np.where(ei > zero, ei * dmax, ei * dmin)
                    m2 = np.where(dq > zero, dq * emax, dq * emin)
                    s1 = np.zeros(H, dtype=F32); s2 = np.zeros(H, dtype=F32)
                    for r in range(H):
                        s1 = s1 + np.exp(dq[r] * ei - m1)
                        s2 = s2 + np.exp(dq * ei[r] - m2)
                    acc = acc + ei * np.exp(m1 - m2) * s1 / s2
                out[l, b] = acc
    assert out.dtype == F32
    return out
