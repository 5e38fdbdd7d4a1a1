"""tests/gemm_ref.py against direct einsum and a hand-computed case, the two emulated arithmetics against the derived bounds, and
the argument checks of pgasr_gemm_f32 / pgasr_colsum_f32 (refusals return before any launch: no GPU is touched)."""
import ctypes
import os

import numpy as np
import pytest

import gemm_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "policy_gradient_asr_amd", "libpgasr_hip.so")
OK, INVALID, LAUNCH, WORKSPACE, UNSUPPORTED = 0, 1, 2, 3, 4


def test_hand_computed_2x2x2():
    A = np.array([1, 2, 3, 4], dtype=np.float32)            # [[1, 2], [3, 4]]
    B = np.array([5, 6, 7, 8], dtype=np.float32)            # [[5, 6], [7, 8]]
    C = np.array([100, 200, 300, 400], dtype=np.float32)
    assert gr.gemm_ref(A, B, C, 2, 2, 2).tolist() == [19, 22, 43, 50]
    assert gr.gemm_ref(A, B, C, 2, 2, 2, transA=True).tolist() == [26, 30, 38, 44]          # [[1, 3], [2, 4]] B
    assert gr.gemm_ref(A, B, C, 2, 2, 2, transB=True).tolist() == [17, 23, 39, 53]          # A [[5, 7], [6, 8]]
    assert gr.gemm_ref(A, B, C, 2, 2, 2, transA=True, transB=True).tolist() == [23, 31, 34, 46]
    # alpha, both biases, leaky, leaky' mask (0 and -0.0 count as not positive), accumulate -- in the header's order
    bias = np.array([-30, 1], dtype=np.float32); bias2 = np.array([1, 1], dtype=np.float32)
    y = np.array([1.0, 0.0, -0.0, -2.0], dtype=np.float32)
    got = gr.gemm_ref(A, B, C, 2, 2, 2, alpha=-1.0, bias=bias, bias2=bias2, act=1, slope=0.5, dact_y=y, accumulate=True)
    # alpha*AB + bias + bias2 = [[-48, -20], [-72, -48]] -> leaky(0.5) halves all -> mask [1, .5, .5, .5] -> + C
    assert got.tolist() == [100 - 24, 200 - 5, 300 - 18, 400 - 12]
    # the bound of the plain product: (K + Z + 10) u S with S = |A||B|
    assert np.allclose(gr.gemm_bound(A, B, C, 2, 2, 2), 13 * gr.U * np.array([19, 22, 43, 50]), rtol=1e-12)
    assert np.allclose(gr.gemm_bound(A, B, C, 2, 2, 2, precision=1, splitk=2, bias=bias, accumulate=True),
                       (3 * 2.0 ** -16 + 2 * (6 + 2 + 10) * gr.U) * (np.array([19, 22, 43, 50]) + [30, 1, 30, 1] + C), rtol=1e-12)


@pytest.mark.parametrize("tA,tB", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_ref_equals_einsum_on_strided_batches(tA, tB):
    rng = np.random.default_rng(7 + 2 * tA + tB)
    M, N, K, batch = 5, 4, 3, 3
    lda, ldb, ldc = (M if tA else K) + 2, (K if tB else N) + 3, N + 1
    sA, sB, sC = -40, 0, 30                                                     # negative, zero and positive batch strides
    a_off, b_off, c_off = 2 * 40 + 1, 3, 2
    A = rng.standard_normal(a_off + 40).astype(np.float32)
    B = rng.standard_normal(b_off + 8 * ldb).astype(np.float32)
    C = rng.standard_normal(c_off + 3 * 30).astype(np.float32)
    shift = np.array([0.5, -1.0, 2.0], dtype=np.float32); scale = np.array([2.0, 0.5, 3.0], dtype=np.float32)
    kw = dict(transA=bool(tA), transB=bool(tB), lda=lda, ldb=ldb, ldc=ldc, strideA=sA, strideB=sB, strideC=sC, batch=batch,
              a_off=a_off, b_off=b_off, c_off=c_off, norm_operand=1, shift=shift, scale=scale, alpha=2.0)
    e = gr.gemm_expect(A, B, C, M, N, K, **kw)
    want = C.astype(np.float64).copy(); mask = np.zeros(C.size, dtype=bool)
    Bm = B[b_off:b_off + (N if tB else K) * ldb].reshape(-1, ldb).astype(np.float64)
    Bm = Bm[:N, :K].T if tB else Bm[:K, :N]
    for b in range(batch):
        Ab = A[a_off + b * sA:a_off + b * sA + (K if tA else M) * lda].reshape(-1, lda).astype(np.float64)
        Ab = Ab[:K, :M].T if tA else Ab[:M, :K]
        Ab = (Ab - float(shift[b])) * float(scale[b])
        rows = want[c_off + b * sC:c_off + b * sC + M * ldc].reshape(M, ldc)
        rows[:, :N] = 2.0 * np.einsum("mk,kn->mn", Ab, Bm)
        mask[c_off + b * sC:c_off + b * sC + M * ldc].reshape(M, ldc)[:, :N] = True
    assert np.array_equal(e.written, mask) and np.allclose(e.ref, want, rtol=1e-13, atol=0)
    assert np.all(e.bound[~mask] == 0) and np.all(e.bound[mask] > 0)
    # the batch sum lands in batch 0's rows only, and split-K changes nothing but the bound
    s = gr.gemm_expect(A, B, C, M, N, K, **kw, sum_batches=True, splitk=2)
    first = np.zeros(C.size, dtype=bool); first[c_off:c_off + M * ldc].reshape(M, ldc)[:, :N] = True
    tot = sum((e.ref[c_off + b * sC:c_off + b * sC + M * ldc].reshape(M, ldc)[:, :N] for b in range(batch)))
    assert np.array_equal(s.written, first) and np.allclose(s.ref[first].reshape(M, N), tot, rtol=1e-13)


def _scaled(rng, rows, cols):
    """The GPU cases' distribution: randn with per-row scales from {1e-3, 1, 50}."""
    return (rng.standard_normal((rows, cols)) * np.array([1e-3, 1.0, 50.0])[np.arange(rows) % 3, None]).astype(np.float32)


@pytest.mark.parametrize("K", [1, 33, 170, 512])
def test_emulated_arithmetics_stay_within_the_bounds(K):
    rng = np.random.default_rng(K)
    M, N = 24, 20
    a, b = _scaled(rng, M, K), _scaled(rng, K, N)
    C = np.zeros(M * N, dtype=np.float32)
    e0 = gr.gemm_expect(a, b, C, M, N, K, precision=0)
    e1 = gr.gemm_expect(a, b, C, M, N, K, precision=1)
    r0 = np.abs(gr.fmaf_chain(a, b).reshape(-1) - e0.ref) / e0.bound
    r1 = np.abs(gr.split_emulation(a, b).reshape(-1) - e1.ref) / e1.bound
    print(f"K={K}: worst err/bound fp32 chain {r0.max():.3f}, bf16 split {r1.max():.3f}")
    assert r0.max() <= 1.0 and r1.max() <= 1.0
    # and the bounds are not vacuous: the split's error is visible at the scale of its own bound
    assert r1.max() > 1e-3


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -7, -3.14159], dtype=np.float32)
    got = gr._bf16(x)
    assert got[:4].tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]            # ties go to the even significand
    assert abs(got[4] - x[4]) <= 2.0 ** -8 * abs(x[4]) and (got.view(np.uint32) & 0xFFFF).max() == 0


def test_colsum_bound_and_guards():
    import torch
    x = np.arange(12, dtype=np.float32).reshape(4, 3) - 5
    assert np.allclose(gr.colsum_bound(x, out0=[1, -1, 0]), 12 * gr.U * (np.abs(x).sum(0) + [1, 1, 0]))
    whole, view = gr.guarded(10)
    assert whole.numel() == 10 + 2 * gr.GUARD and view.data_ptr() == whole.data_ptr() + 4 * gr.GUARD
    gr.assert_untouched(whole)
    view[3] = 1.0
    w = np.zeros(10, dtype=bool); w[3] = True
    gr.assert_untouched(whole, w)
    with pytest.raises(AssertionError):
        gr.assert_untouched(whole)
    whole[gr.GUARD - 1] = float(gr.SENTINEL) + 1.0                                # one ulp-scale change in the front guard is seen
    with pytest.raises(AssertionError):
        gr.assert_untouched(whole, w)
    assert torch.isfinite(whole).all()


# ---- refusals through the C ABI ----
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from policy_gradient_asr_amd import _lib
    h = ctypes.CDLL(LIB)
    for name in ("pgasr_gemm_f32", "pgasr_colsum_f32", "pgasr_colsum_workspace_bytes", "pgasr_gemm_workspace_bytes"):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return h


class _Host:
    """Non-null dummy pointers (host memory): every call below is refused before anything is launched."""

    def __init__(self):
        self.buf = (ctypes.c_float * 4096)()
        self.p = ctypes.addressof(self.buf)


def _gemm(lib, h, **over):
    a = dict(transA=0, transB=0, M=8, N=8, K=8, alpha=1.0, A=h.p, lda=8, strideA=0, B=h.p, ldb=8, strideB=0, C=h.p, ldc=8, strideC=0,
             batch=1, sum_batches=0, splitk=1, bias=None, bias2=None, act=0, slope=0.01, accumulate=0, dact_y=None, norm_operand=0,
             shift=None, scale=None, precision=0, xcc_busy=None, workspace=h.p, workspace_bytes=4096 * 4, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return lib.pgasr_gemm_f32(*a.values())


GEMM_REFUSALS = [
    ("dact_y with split-K", dict(dact_y="p", splitk=2)),
    ("dact_y with a batch sum", dict(dact_y="p", sum_batches=1, batch=2)),
    ("norm_operand without shift", dict(norm_operand=1, scale="p")),
    ("norm_operand without scale", dict(norm_operand=2, shift="p")),
    ("norm_operand out of range", dict(norm_operand=3, shift="p", scale="p")),
    ("act out of range", dict(act=2)), ("act negative", dict(act=-1)),
    ("precision out of range", dict(precision=3)), ("precision negative", dict(precision=-1)),
    ("M = 0", dict(M=0)), ("N = 0", dict(N=0)), ("K = 0", dict(K=0)), ("K < 0", dict(K=-8)),
    ("batch = 0", dict(batch=0)), ("splitk = 0", dict(splitk=0)),
    ("null A", dict(A=None)), ("null B", dict(B=None)), ("null C", dict(C=None)),
    # new with these tests: a leading dimension shorter than the row it strides
    ("lda < K", dict(lda=7)), ("lda < M, transA", dict(transA=1, M=9, lda=8, ldc=8)),
    ("ldb < N", dict(ldb=7)), ("ldb < K, transB", dict(transB=1, K=9, ldb=8, lda=9)),
    ("ldc < N", dict(ldc=7)), ("ldc = 0", dict(ldc=0)), ("lda negative", dict(lda=-8)),
]


@pytest.mark.parametrize("what,over", GEMM_REFUSALS, ids=[w for w, _ in GEMM_REFUSALS])
def test_gemm_refuses(lib, what, over):
    h = _Host()
    over = {k: (h.p if v == "p" else v) for k, v in over.items()}
    assert _gemm(lib, h, **over) == INVALID, what


def test_gemm_leading_dimension_rule_is_exact(lib):
    """lda == the row length passes the argument checks in each orientation: with a partial-slab product and no workspace the call
    then stops at the workspace check (still before any launch), which a refused leading dimension never reaches."""
    h = _Host()
    for over in (dict(M=5, N=6, K=7, lda=7, ldb=6, ldc=6), dict(transA=1, M=5, N=6, K=7, lda=5, ldb=6, ldc=6),
                 dict(transB=1, M=5, N=6, K=7, lda=7, ldb=7, ldc=6), dict(transA=1, transB=1, M=5, N=6, K=7, lda=5, ldb=7, ldc=6)):
        assert _gemm(lib, h, splitk=2, workspace=None, workspace_bytes=0, **over) == WORKSPACE, over
        for ld, short in (("lda", over["lda"] - 1), ("ldb", over["ldb"] - 1), ("ldc", over["ldc"] - 1)):
            assert _gemm(lib, h, splitk=2, workspace=None, workspace_bytes=0, **{**over, ld: short}) == INVALID, (over, ld)
    # a workspace that is one byte short of pgasr_gemm_workspace_bytes is refused as well
    need = lib.pgasr_gemm_workspace_bytes(8, 8, 1, 2, 0)
    assert need == 256 + 2 * 8 * 8 * 4
    assert _gemm(lib, h, splitk=2, workspace_bytes=need - 1) == WORKSPACE


def test_two_plane_kernels_refuse_padded_rows_past_their_offsets(lib):
    """pgasr_gemm_x3w_f32 / _feed_f32 address whole 256-row tiles with 32-bit offsets: an M whose own span is below the limit but whose
    last tile is not is PGASR_ERR_UNSUPPORTED (callers fall back to pgasr_gemm_f32), as hipops.gemm_x3w_ok(planes=2) predicts."""
    from policy_gradient_asr_amd import _lib, hipops
    for name in ("pgasr_gemm_x3w_f32", "pgasr_gemm_x3w_feed_f32"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    h = _Host()
    p = (h.p + 15) & ~15                                     # the alignment check comes first
    M = 2047 * 256 + 1
    assert M * 2048 * 4 < 2 ** 32 and not hipops.gemm_x3w_ok(M, 2048, 512, planes=2)
    assert lib.pgasr_gemm_x3w_f32(M, 2048, 512, p, 512, p, p, p, 2048, None, None, 0.01, None) == UNSUPPORTED
    M = 1023 * 256 + 1
    assert M * 2048 * 4 < 2 ** 31
    assert lib.pgasr_gemm_x3w_feed_f32(M, 2048, 512, p, 512, p, p, p, 2048, None, None, p, 0, 0, 0, p, 4096, None) == UNSUPPORTED


def test_colsum_refuses(lib):
    h = _Host()
    cs = lib.pgasr_colsum_f32
    assert cs(h.p, 4, 8, 7, h.p, None, 0, h.p, 4096, None) == INVALID                 # ld < cols
    assert cs(h.p, 0, 8, 8, h.p, None, 0, h.p, 4096, None) == INVALID
    assert cs(h.p, 4, 0, 8, h.p, None, 0, h.p, 4096, None) == INVALID
    assert cs(h.p, -1, 8, 8, h.p, None, 0, h.p, 4096, None) == INVALID
    assert cs(None, 4, 8, 8, h.p, None, 0, h.p, 4096, None) == INVALID
    assert cs(h.p, 4, 8, 8, None, None, 0, h.p, 4096, None) == INVALID
    need = lib.pgasr_colsum_workspace_bytes(1500, 300)
    assert need == 3 * 300 * 4 and lib.pgasr_colsum_workspace_bytes(512, 1) == 4 and lib.pgasr_colsum_workspace_bytes(513, 1) == 8
    assert cs(h.p, 1500, 300, 300, h.p, None, 0, h.p, need - 1, None) == WORKSPACE
    assert cs(h.p, 1500, 300, 300, h.p, None, 0, None, need, None) == WORKSPACE
