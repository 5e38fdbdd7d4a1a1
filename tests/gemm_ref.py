"""Contract-level reference, error bound and guarded buffers for ``pgasr_gemm_f32`` and ``pgasr_colsum_f32``.  A plain module:
no test, no fixture.

``gemm_ref`` is written from the header's contract (include/pgasr_hip.h), not from the kernel: flat buffers, index arithmetic
``off + b * stride + row * ld + col``, one einsum per batch, everything in fp64.  It knows nothing of tiles, slabs or vector widths.

The bound (``gemm_bound``), derived and never measured.  Notation: u = 2^-24 (fp32 unit roundoff), a', b' the operands after the
optional (x - shift[b]) * scale[b], Z = splitk * (batch if sum_batches else 1) the number of partial slabs that are added up, and

    S[m, n] = |alpha| * sum_k |a'[m, k]| |b'[k, n]| + |bias[n]| + |bias2[n]| + |C0[m, n]|      (C0 counts with accumulate only)

* precision 0 -- the fp32 MFMA is an fmaf chain: K fused multiply-adds, one rounding each, give the classical
  gamma_K = K u / (1 - K u) relative to sum |a'||b'| (Higham, Accuracy and Stability, section 3.1; K u is below 1e-4 here, so the
  denominator is inside the slack below).  Adding Z slabs in index order is Z more roundings of partial sums that are each bounded
  by S.  The rest is a fixed number of roundings, each relative to a quantity bounded by S: two for the normalisation of an
  operand element (subtract, multiply), one each for alpha *, bias + bias2, + bias, the leaky multiply, the leaky' multiply and
  the accumulate add: eight, rounded up to ten.  leaky_relu is 1-Lipschitz and the leaky' factor is at most 1, so neither widens
  an error that is already there.                                        bound0 = (K + Z + 10) u S
* precision 1 -- every element is split x = hi + lo + res with hi = bf16(x), lo = bf16(x - hi); bf16 carries 8 significand bits,
  unit roundoff 2^-8, so |lo| <= 2^-8 |x| and |res| <= 2^-16 |x|.  The kernel sums hi*hi + hi*lo + lo*hi; what it drops is
  lo*lo + res*b + a*res - ..., three terms of at most 2^-16 |a'||b'| each: 3 * 2^-16 S.  The three kept products are exact in fp32
  (8 x 8 bits) and are accumulated in fp32: 3 K additions.  The order and the internal rounding of the 16-deep bf16 MFMA are not
  documented, so that term carries a factor 2.                            bound1 = (3 * 2^-16 + 2 (3 K + Z + 10) u) S

``split_emulation`` and ``fmaf_chain`` emulate the two arithmetics in numpy (tests/test_gemm_ref_cpu.py holds them to the bounds).
"""
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
GUARD = 256
SENTINEL = np.float32(-12345.678)            # finite; no test output equals it
SENTINEL_BITS = int(np.array([SENTINEL], dtype=np.float32).view(np.int32)[0])


def _flat64(x):
    if x is None:
        return None
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64).reshape(-1)


def _index(off, row_stride, col_stride, rows, cols):
    return off + np.arange(rows, dtype=np.int64)[:, None] * row_stride + np.arange(cols, dtype=np.int64)[None, :] * col_stride


def gemm_expect(A, B, C, M, N, K, transA=False, transB=False, lda=None, ldb=None, ldc=None, alpha=1.0,
                strideA=0, strideB=0, strideC=0, batch=1, sum_batches=False, splitk=1, bias=None, bias2=None,
                act=0, slope=0.01, accumulate=False, dact_y=None, norm_operand=0, shift=None, scale=None,
                a_off=0, b_off=0, c_off=0, precision=0, xcc_busy=None):
    """The arguments of ``hipops.gemm`` on CPU buffers.  A, B, C (and dact_y, which starts at C's base address + c_off) are flat;
    C holds the contents before the call.  Returns ref (the whole C buffer afterwards, fp64), written (bool, the elements the
    call may write) and bound (per element; 0 where nothing is written)."""
    A, B, C0 = _flat64(A), _flat64(B), _flat64(C)
    bias, bias2, dact_y, shift, scale = map(_flat64, (bias, bias2, dact_y, shift, scale))
    lda = lda if lda is not None else (M if transA else K)
    ldb = ldb if ldb is not None else (K if transB else N)
    ldc = ldc if ldc is not None else N
    alpha = float(np.float32(alpha)); slope = float(np.float32(slope))
    ref = C0.copy()
    written = np.zeros(C0.shape, dtype=bool)
    bound = np.zeros(C0.shape, dtype=np.float64)
    Z = splitk * (batch if sum_batches else 1)
    if precision == 0:
        factor = (K + Z + 10) * U
    elif precision == 1:
        factor = 3 * 2.0 ** -16 + 2 * (3 * K + Z + 10) * U
    else:
        raise ValueError("precision 0 or 1")
    badd = np.zeros(N); babs = np.zeros(N)
    for t in (bias, bias2):
        if t is not None:
            badd = badd + t[:N]; babs = babs + np.abs(t[:N])

    def product(b):
        ia = _index(a_off + b * strideA, 1, lda, M, K) if transA else _index(a_off + b * strideA, lda, 1, M, K)
        ib = _index(b_off + b * strideB, 1, ldb, K, N) if transB else _index(b_off + b * strideB, ldb, 1, K, N)
        assert ia.min() >= 0 and ia.max() < A.size and ib.min() >= 0 and ib.max() < B.size, "operand outside its buffer"
        a, bm = A[ia], B[ib]
        if norm_operand == 1:
            a = (a - shift[b]) * scale[b]
        elif norm_operand == 2:
            bm = (bm - shift[b]) * scale[b]
        return alpha * np.einsum("mk,kn->mn", a, bm), abs(alpha) * np.einsum("mk,kn->mn", np.abs(a), np.abs(bm))

    def epilogue(b, v, s):
        ic = _index(c_off + b * strideC, ldc, 1, M, N)
        assert ic.min() >= 0 and ic.max() < C0.size, "output outside its buffer"
        v = v + badd[None, :]
        s = s + babs[None, :]
        if act == 1:
            v = np.where(v > 0, v, v * slope)
        if dact_y is not None:
            v = v * np.where(dact_y[ic - c_off] > 0, 1.0, slope)
        if accumulate:
            v = v + C0[ic]
            s = s + np.abs(C0[ic])
        ref[ic] = v; written[ic] = True; bound[ic] = factor * s

    if sum_batches:
        v = np.zeros((M, N)); s = np.zeros((M, N))
        for b in range(batch):
            p, q = product(b)
            v += p; s += q
        epilogue(0, v, s)
    else:
        for b in range(batch):
            epilogue(b, *product(b))
    return SimpleNamespace(ref=ref, written=written, bound=bound)


def gemm_ref(*args, **kw):
    """Expected contents of the whole C buffer, fp64."""
    return gemm_expect(*args, **kw).ref


def gemm_bound(*args, **kw):
    """Per-element error bound of the whole C buffer (module docstring)."""
    return gemm_expect(*args, **kw).bound


# ---- numpy emulations of the two arithmetics (fp32 accumulate, k in order) ----
def _bf16(x):
    """Round fp32 to bf16 (nearest even), returned as fp32."""
    bits = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32)


def split_emulation(a, b):
    """(M, K) @ (K, N) in the bf16x3 arithmetic: hi*hi + hi*lo + lo*hi, each product exact, one fp32 chain."""
    a = np.asarray(a, dtype=np.float32); b = np.asarray(b, dtype=np.float32)
    ah = _bf16(a); al = _bf16(a - ah); bh = _bf16(b); bl = _bf16(b - bh)
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    for k in range(a.shape[1]):
        for x, y in ((ah, bh), (ah, bl), (al, bh)):
            acc = (acc.astype(np.float64) + x[:, k, None].astype(np.float64) * y[None, k, :].astype(np.float64)).astype(np.float32)
    return acc


def fmaf_chain(a, b):
    """(M, K) @ (K, N) as one fused-multiply-add chain per element (the product of two fp32 values is exact in fp64)."""
    a = np.asarray(a, dtype=np.float32); b = np.asarray(b, dtype=np.float32)
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    for k in range(a.shape[1]):
        acc = (acc.astype(np.float64) + a[:, k, None].astype(np.float64) * b[None, k, :].astype(np.float64)).astype(np.float32)
    return acc


def colsum_bound(x, out0=None):
    """pgasr_colsum_f32: rows are summed in blocks of 512 -- four interleaved chains of at most 128 additions, a two-level tree --
    and the blocks in index order, one more addition with accumulate: an element passes through at most
    ceil(min(rows, 512) / 4) + 2 + ceil(rows / 512) + 1 roundings, fewer than rows + 8 for every rows >= 1, each relative to a
    partial sum bounded by sum |x| + |out0|.  So (rows + 8) u (sum |x| + |out0|) per column (loose for long columns, by design:
    it assumes nothing about the blocking)."""
    x = np.asarray(x, dtype=np.float64)
    s = np.abs(x).sum(0)
    if out0 is not None:
        s = s + np.abs(np.asarray(out0, dtype=np.float64))
    return (x.shape[0] + 8) * U * s


# ---- guarded buffers ----
def guarded(n, device="cpu"):
    """A flat fp32 buffer of n elements with GUARD elements in front and behind, all of it the sentinel.
    Returns (whole, view): hand ``view`` to the kernel, ``whole`` to ``assert_untouched``."""
    import torch
    whole = torch.full((int(n) + 2 * GUARD,), float(SENTINEL), dtype=torch.float32, device=device)
    return whole, whole[GUARD:GUARD + int(n)]


def assert_untouched(whole, written=None, what=""):
    """Every element of ``whole`` outside the write set (a bool array over the guarded view; None: nothing may be written) still
    holds the sentinel, bit for bit."""
    bits = whole.detach().cpu().numpy().view(np.int32)
    keep = np.ones(bits.shape, dtype=bool)
    if written is not None:
        assert written.size == bits.size - 2 * GUARD
        keep[GUARD:GUARD + written.size] = ~np.asarray(written, dtype=bool)
    bad = np.flatnonzero(keep & (bits != SENTINEL_BITS))
    assert bad.size == 0, f"{what}: {bad.size} elements outside the write set were overwritten, first at {bad[:8] - GUARD} (view index)"
