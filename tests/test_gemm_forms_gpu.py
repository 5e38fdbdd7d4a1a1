"""pgasr_gemm_f32 in every form a call site uses -- strides, offsets, batches, batch sums, split-K, the epilogues, normalised
operands, queue mode, the 64-bit epilogue at the 4 GiB edge -- and pgasr_colsum_f32, each against the contract-level fp64
reference of tests/gemm_ref.py.  Every case asserts |got - ref| <= the DERIVED bound elementwise (gemm_ref's docstring), the
max-norm figures of test_gemm_layouts (1e-5 exact fp32, 3e-5 bf16x3), and that every element next to the output -- guards, ldc
gaps, rows >= M, other batches' rows -- still holds its sentinel bit for bit.  Each case prints its worst err/bound ratio.

Worst err/bound over this file on an MI355X (`pytest -s` prints them): 0.21 exact fp32 (K = 9 split in two, the second slab
empty), 0.41 bf16x3 (K = 1: the split's dropped terms are the whole error); 0.19 / 0.36 at the 4 GiB edge; column sums 0.16.  A ratio
above 1 means that the kernel or the derivation is wrong."""
import numpy as np
import pytest
import torch

import gemm_ref as gr
from pg_harness import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAXNORM = {0: 1e-5, 1: 3e-5}              # test_gemm_layouts' figures
WORST = {0: (0.0, ""), 1: (0.0, "")}      # worst err/bound seen so far, per precision
ROW_SCALES = np.array([1e-3, 1.0, 50.0])
TRANSPOSES = [(0, 0), (0, 1), (1, 0), (1, 1)]


def _data(rng, size, ld):
    """randn with a scale from {1e-3, 1, 50} per storage row, so that small elements exist next to large ones."""
    return (rng.standard_normal(size) * ROW_SCALES[(np.arange(size) // max(ld, 1)) % 3]).astype(np.float32)


def _span(off, stride, batch, rows, cols, ld):
    starts = [off + b * stride for b in range(batch)]
    return min(starts), max(starts) + (rows - 1) * ld + cols


def run_gemm(name, M, N, K, precision, seed=0, with_bias=False, with_bias2=False, with_dact=False, **kw):
    """Build the buffers of one call (kw: the arguments of hipops.gemm), run it, and make the three assertions.  Returns the
    output buffer (guards included) as it came back."""
    from policy_gradient_asr_amd import hipops
    rng = np.random.default_rng(1000 * seed + 7 * M + 3 * N + K)
    tA, tB = bool(kw.get("transA", False)), bool(kw.get("transB", False))
    batch = kw.get("batch", 1)
    lda = kw.setdefault("lda", M if tA else K); ldb = kw.setdefault("ldb", K if tB else N); ldc = kw.setdefault("ldc", N)
    a_off, b_off, c_off = kw.get("a_off", 0), kw.get("b_off", 0), kw.get("c_off", 0)
    sA, sB, sC = kw.get("strideA", 0), kw.get("strideB", 0), kw.get("strideC", 0)
    a_lo, a_hi = _span(a_off, sA, batch, K if tA else M, M if tA else K, lda)
    b_lo, b_hi = _span(b_off, sB, batch, N if tB else K, K if tB else N, ldb)
    cb = 1 if kw.get("sum_batches") else batch
    c_lo, c_hi = _span(c_off, sC, cb, M, N, ldc)
    assert a_lo >= 0 and b_lo >= 0 and c_lo >= 0, "the case's offsets must keep every batch inside its buffer"
    A = _data(rng, a_hi + 3, lda); B = _data(rng, b_hi + 3, ldb)
    if kw.get("norm_operand"):
        # per-batch shift around 50 against data of unit spread: a padded cell that is not zeroed contributes -shift * scale
        shift = (50.0 + 3.0 * np.arange(batch) + rng.standard_normal(batch)).astype(np.float32)
        scale = (0.6 + 0.2 * np.arange(batch)).astype(np.float32)
        X, ld, off, st, t, rows, cols = (A, lda, a_off, sA, tA, M, K) if kw["norm_operand"] == 1 else (B, ldb, b_off, sB, not tB, N, K)
        r, c = (cols, rows) if t else (rows, cols)          # storage rows x cols of the operand
        for b in range(batch):
            idx = off + b * st + np.arange(r)[:, None] * ld + np.arange(c)[None, :]
            X[idx] = (shift[b] + rng.standard_normal((r, c))).astype(np.float32)
        kw["shift"], kw["scale"] = shift, scale
    C0 = np.full(c_hi + 3, gr.SENTINEL, dtype=np.float32)
    if kw.get("accumulate"):
        for b in range(cb):
            idx = c_off + b * sC + np.arange(M)[:, None] * ldc + np.arange(N)[None, :]
            C0[idx] = _data(rng, M * N, N).reshape(M, N)
    if with_bias:
        kw["bias"] = (rng.standard_normal(N) * 3).astype(np.float32)
    if with_bias2:
        kw["bias2"] = rng.standard_normal(N).astype(np.float32)
    if with_dact:
        assert sC >= 0
        y = rng.standard_normal(c_hi - c_off + 3).astype(np.float32)
        pick = rng.random(y.size)
        y[pick < 0.2] = 0.0; y[pick < 0.1] = -0.0            # exact zeros of both signs: leaky' is `slope` there
        kw["dact_y"] = y
    e = gr.gemm_expect(A, B, C0, M, N, K, precision=precision, **kw)

    dev = {k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    whole, view = gr.guarded(C0.size, DEV)
    view.copy_(torch.from_numpy(C0))
    dev.setdefault("xcc_busy", 0)
    hipops.gemm(torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV), view, M, N, K, precision=precision, **dev)
    torch.cuda.synchronize()
    check(name, precision, whole, e)
    return whole


def check(name, precision, whole, e):
    got = whole.cpu().numpy()[gr.GUARD:-gr.GUARD].astype(np.float64)
    w = e.written
    err, bnd = np.abs(got - e.ref)[w], e.bound[w]
    ratio = float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0
    if ratio > WORST[precision][0]:
        WORST[precision] = (ratio, name)
    print(f"{name} precision {precision}: worst err/bound {ratio:.3f}, max-norm {rel_err(got[w], e.ref[w]):.2e}   "
          f"[file so far: {WORST[precision][0]:.3f} at {WORST[precision][1]}]")
    gr.assert_untouched(whole, w, name)
    assert np.isfinite(got[w]).all(), name
    worst = int(np.argmax(err - bnd))
    assert np.all(err <= bnd), f"{name}: |got - ref| = {err[worst]:.3e} above the bound {bnd[worst]:.3e} (ratio {ratio:.2f})"
    assert rel_err(got[w], e.ref[w]) < MAXNORM[precision], name


def _up4(x):
    return (x + 3) // 4 * 4


# ---- addressing ----
SHAPES = {(0, 0): (150, 131, 170), (0, 1): (127, 200, 120), (1, 0): (129, 128, 80), (1, 1): (200, 127, 40)}


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("tA,tB", TRANSPOSES)
@pytest.mark.parametrize("form", ["padded_ld", "unaligned_base", "odd_ld"])
def test_addressing(form, tA, tB, precision):
    """Leading dimensions above natural; a base that is 4- but not 16-byte aligned under ld % 4 == 0 (the 16-byte loads must be
    given up for the POINTER's sake); an aligned base under ld % 4 != 0 (given up for the ROWS' sake)."""
    M, N, K = SHAPES[(tA, tB)]
    na, nb = (M if tA else K), (K if tB else N)
    if form == "padded_ld":
        kw = dict(lda=na + 4, ldb=nb + 5, ldc=N + 5)
    elif form == "unaligned_base":
        kw = dict(lda=_up4(na) + 4, ldb=_up4(nb) + 8, ldc=_up4(N) + 4, a_off=1, b_off=3, c_off=2)
    else:
        kw = dict(lda=_up4(na) + 1, ldb=_up4(nb) + 3, ldc=_up4(N) + 2)
    run_gemm(f"{form} tA={tA} tB={tB}", M, N, K, precision, transA=bool(tA), transB=bool(tB), with_bias=True, **kw)


# ---- batches ----
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("form", ["positive", "zero_B_interleaved_C", "zero_A", "negative"])
@pytest.mark.parametrize("tA,tB", [(0, 1), (1, 0)])
def test_batch_strides(tA, tB, form, precision):
    M, N, K, batch = 130, 127, 40, 3
    na, ra = ((M, K) if tA else (K, M))                      # row length, storage rows
    nb, rb = ((K, N) if tB else (N, K))
    lda, ldb, ldc = na + 4, nb + 1, N + 3
    if form == "positive":
        kw = dict(strideA=ra * lda + 7, strideB=rb * ldb + 2, strideC=M * ldc + 11)
    elif form == "zero_B_interleaved_C":                    # one weight for every batch; C rows interleaved by batch (the input layer)
        ldc = batch * N
        kw = dict(strideA=ra * lda, strideB=0, strideC=N)
    elif form == "zero_A":
        kw = dict(strideA=0, strideB=rb * ldb, strideC=M * ldc)
    else:
        sa, sb, sc = ra * lda + 5, rb * ldb + 1, M * ldc + 9
        kw = dict(strideA=-sa, strideB=-sb, strideC=-sc, a_off=2 * sa + 1, b_off=2 * sb, c_off=2 * sc + 2)
    run_gemm(f"batch strides {form} tA={tA} tB={tB}", M, N, K, precision, transA=bool(tA), transB=bool(tB), lda=lda, ldb=ldb, ldc=ldc,
             batch=batch, with_bias=True, act=1, **kw)


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("tA,tB", [(1, 1), (0, 0)])
def test_sum_batches(tA, tB, splitk, accumulate, precision):
    M, N, K, batch = 129, 131, 80, 3
    ra, rb = (K if tA else M), (N if tB else K)
    lda, ldb = (M if tA else K) + 4, (K if tB else N) + 4
    run_gemm(f"sum_batches splitk={splitk} acc={accumulate} tA={tA} tB={tB}", M, N, K, precision, transA=bool(tA), transB=bool(tB),
             lda=lda, ldb=ldb, ldc=N + 1, strideA=ra * lda, strideB=rb * ldb, strideC=0, batch=batch, sum_batches=True, splitk=splitk,
             accumulate=accumulate, with_bias=True, with_bias2=True, act=1, alpha=-0.5)


# ---- split-K ----
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("K,splitk", [(40, 4), (9, 2), (170, 3), (120, 2), (170, 7)])
@pytest.mark.parametrize("tA,tB", TRANSPOSES)
def test_split_k_short_and_empty_slabs(tA, tB, K, splitk, precision):
    """Slabs are rounded up to the k-tile (16 exact, 32 bf16x3): K = 40 in four leaves the fourth slab empty in both kernels,
    K = 9 in two the second; K = 170 in three or seven and 120 in two leave a short last slab."""
    M, N = SHAPES[(tA, tB)][:2]
    run_gemm(f"split-K K={K}/{splitk} tA={tA} tB={tB}", M, N, K, precision, transA=bool(tA), transB=bool(tB), splitk=splitk, batch=2,
             strideA=M * K, strideB=N * K, strideC=M * N + 5, with_bias=True, accumulate=True)


# ---- epilogues ----
EPILOGUES = [dict(), dict(with_bias=True), dict(with_bias=True, with_bias2=True), dict(with_bias2=True, act=1),
             dict(with_bias=True, act=1, accumulate=True), dict(accumulate=True), dict(with_bias=True, with_bias2=True, act=1, accumulate=True)]


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("alpha", [-0.5, 0.0, 2.0])
@pytest.mark.parametrize("ep", range(len(EPILOGUES)))
@pytest.mark.parametrize("path", ["plain", "reduce"])
def test_epilogues(path, ep, alpha, precision):
    """The same epilogue in the tile kernels (store_tiles_fast: its straight-line form and its load-then-store form) and in
    gemm_reduce_kernel."""
    M, N, K = 129, 131, 40
    run_gemm(f"epilogue {path} #{ep} alpha={alpha}", M, N, K, precision, seed=ep, transB=True, ldc=N + 3, alpha=alpha,
             splitk=2 if path == "reduce" else 1, **EPILOGUES[ep])


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("tA,tB", [(0, 0), (1, 1)])
def test_dact_epilogue(tA, tB, accumulate, precision):
    """d(leaky_relu) mask from a tensor in C's layout (ldc gaps, batch stride) with exact zeros of both signs."""
    M, N, K, batch = 150, 131, 40, 2
    run_gemm(f"dact acc={accumulate} tA={tA} tB={tB}", M, N, K, precision, transA=bool(tA), transB=bool(tB), ldc=N + 5, batch=batch,
             strideA=M * K, strideB=K * N, strideC=M * (N + 5) + 3, with_dact=True, with_bias=True, accumulate=accumulate, alpha=2.0,
             slope=0.01)


# ---- normalised operands ----
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("splitk", [1, 2])
@pytest.mark.parametrize("operand,trans", [(1, 0), (1, 1), (2, 0), (2, 1)])
@pytest.mark.parametrize("K", [170, 120])
def test_normalised_operand(K, operand, trans, splitk, precision):
    """(x - shift[b]) * scale[b] on load, for both storage orientations of the normalised operand, with M, N and K tails and with
    a short split-K slab.  A padded cell that went through the transform is -shift * scale, about -40 here; it may only ever meet a
    zero of the other operand (k tails) or a row / column that is not stored (M, N tails).  Each batch has its own shift and scale."""
    M, N, batch = 150, 131, 2
    tA, tB = (trans, 1) if operand == 1 else (1, trans)
    ra, rb = (K if tA else M), (N if tB else K)
    lda, ldb = (M if tA else K) + 4, (K if tB else N) + 1
    run_gemm(f"norm operand={operand} trans={trans} K={K} splitk={splitk}", M, N, K, precision, transA=bool(tA), transB=bool(tB),
             lda=lda, ldb=ldb, strideA=ra * lda, strideB=rb * ldb, strideC=M * N, batch=batch, splitk=splitk, norm_operand=operand,
             with_bias=True)


# ---- the call sites' own argument patterns ----
def _site_178(B=3, F=120, T=53, N=256):
    return (T, N, F), dict(transA=True, transB=True, lda=T, ldb=F, ldc=B * N, strideA=F * T, strideB=0, strideC=N, batch=B,
                           with_bias=True, act=1, slope=0.01, norm_operand=1)


def _site_211(accumulate, splitk, B=3, F=120, T=53, N=256):
    return (N, F, T), dict(transA=True, transB=True, lda=B * N, ldb=T, ldc=F, strideA=N, strideB=F * T, strideC=0, batch=B,
                           sum_batches=True, norm_operand=2, accumulate=accumulate, splitk=splitk)


def _site_567(T=6, B=5, H=256):
    G = 8 * H
    return (4 * H, H, (T - 1) * B), dict(transA=True, lda=G, ldb=2 * H, ldc=H, a_off=B * G, b_off=0, strideA=4 * H - B * G,
                                         strideB=B * 2 * H + H, strideC=4 * H * H, batch=2, splitk=1)


CALL_SITES = {
    "functional.py InstNormAffineFn.forward (input layer)": _site_178(),
    "functional.py InstNormAffineFn.backward dW": _site_211(False, 1),
    "functional.py InstNormAffineFn.backward dW into weight.grad": _site_211(True, 1),
    "functional.py InstNormAffineFn.backward dW, split-K 2": _site_211(False, 2),
    "functional.py InstNormAffineFn.backward dW into weight.grad, split-K 2": _site_211(True, 2),
    "functional.py BLSTMLayerFn dW_hh fallback (negative batch stride)": _site_567(),
}


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("site", list(CALL_SITES))
def test_call_site_replicas(site, precision):
    (M, N, K), kw = CALL_SITES[site]
    run_gemm(site, M, N, K, precision, **dict(kw))


# ---- degenerate sizes ----
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (1, 200, 9), (200, 1, 9), (127, 129, 1), (130, 130, 15)])
@pytest.mark.parametrize("tA,tB", TRANSPOSES)
def test_degenerate_sizes(tA, tB, M, N, K, precision):
    run_gemm(f"degenerate {M}x{N}x{K} tA={tA} tB={tB}", M, N, K, precision, transA=bool(tA), transB=bool(tB), with_bias=True, act=1)


# ---- queue mode ----
@pytest.mark.parametrize("mask", [0x00, 0xA5, 0xFF])
@pytest.mark.parametrize("tA,tB", TRANSPOSES)
def test_queue_mode_equals_plain_launch(tA, tB, mask):
    """bf16x3 tiles drawn from a counter, workgroups on `busy` XCDs taking none, an unmasked second launch for the rest: the same bits
    as the plain launch for every mask (nothing here waits on anything)."""
    M, N, K = 150, 131, 170                                 # a ragged two-by-two tile grid
    kw = dict(transA=bool(tA), transB=bool(tB), ldc=N + 3, with_bias=True, act=1, accumulate=True)
    plain = run_gemm(f"queue reference tA={tA} tB={tB}", M, N, K, 1, **dict(kw))
    busy = torch.tensor([(mask >> i) & 1 for i in range(8)], dtype=torch.int32, device=DEV)
    queued = run_gemm(f"queue mask={mask:#04x} tA={tA} tB={tB}", M, N, K, 1, xcc_busy=busy.data_ptr(), **dict(kw))
    assert torch.equal(plain, queued)


# ---- the 4 GiB edge ----
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("M,with_dact", [(130, True), (120, False)])
def test_four_gib_edge(M, with_dact, precision):
    """ldc = 8 600 000.  M = 130: C's span reaches 2^32 bytes, the 64-bit epilogue runs (bias, leaky, leaky' mask, accumulate).
    M = 120: the span is 3.81 GiB, but the 128 rows the last tile touches reach past 4 GiB; addressed with 32-bit offsets, rows 125,
    126 and 127 wrap to elements 1 258 176, 9 858 176 and 18 458 176 of C -- inside the buffer, so the range check lets them through.
    The host decides the addressing mode on the padded row count, which sends this case to the 64-bit epilogue as well."""
    from policy_gradient_asr_amd import hipops
    N, K, ldc = 64, 9, 8_600_000
    span = (M - 1) * ldc + N
    assert (span * 4 >= 2 ** 32) == (M == 130) and (127 * ldc + N) * 4 >= 2 ** 32
    rng = np.random.default_rng(M + precision)
    A = _data(rng, M * K, K); B = _data(rng, K * N, N)
    bias = (rng.standard_normal(N) * 3).astype(np.float32)
    C0 = _data(rng, M * N, N)
    y = None
    if with_dact:
        y = rng.standard_normal(M * N).astype(np.float32)
        pick = rng.random(y.size); y[pick < 0.2] = 0.0; y[pick < 0.1] = -0.0
    e = gr.gemm_expect(A, B, C0, M, N, K, precision=precision, bias=bias, act=1, slope=0.01, accumulate=True, dact_y=y, alpha=2.0)

    def rows(flat):                                          # the M x N elements the call owns
        return torch.as_strided(flat, (M, N), (ldc, 1))
    whole, view = gr.guarded(span, DEV)
    rows(view).copy_(torch.from_numpy(C0.reshape(M, N)))
    yd = None
    if with_dact:
        _, yd = gr.guarded(span, DEV)
        rows(yd).copy_(torch.from_numpy(y.reshape(M, N)))
    hipops.gemm(torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV), view, M, N, K, ldc=ldc, alpha=2.0, bias=torch.from_numpy(bias).to(DEV),
                act=1, slope=0.01, accumulate=True, dact_y=yd, precision=precision, xcc_busy=0)
    torch.cuda.synchronize()
    got = rows(view).cpu().numpy().astype(np.float64).reshape(-1)
    bits = whole.view(torch.int32)
    changed = sum(int((bits[i:i + (1 << 28)] != gr.SENTINEL_BITS).sum()) for i in range(0, bits.numel(), 1 << 28))
    del whole, view, yd, bits
    torch.cuda.empty_cache()
    err = np.abs(got - e.ref)
    ratio = float((err / e.bound).max())
    if ratio > WORST[precision][0]:
        WORST[precision] = (ratio, f"4 GiB edge M={M}")
    print(f"4 GiB edge M={M} precision {precision}: worst err/bound {ratio:.3f}, non-sentinel elements {changed} (M*N = {M * N})")
    assert changed == M * N, f"{changed - M * N} elements outside the M x N output were written"
    assert np.all(err <= e.bound) and rel_err(got, e.ref) < MAXNORM[precision]


# ---- pgasr_colsum_f32 ----
@pytest.mark.parametrize("mode", ["out", "out_out2", "accumulate", "accumulate_out_only"])
@pytest.mark.parametrize("rows", [1, 3, 511, 512, 513, 1500])
def test_colsum(rows, mode):
    """Column sums (the bias gradient behind each of these products) against fp64 with the derived bound (rows + 8) u sum|x|, on
    both sides of the 512-row block and the 64-column tile, dense and with a row gap; out and out2 in guarded buffers."""
    from policy_gradient_asr_amd import hipops
    worst = 0.0
    for cols in (1, 63, 64, 65, 300):
        for ld in (cols, cols + 5):
            rng = np.random.default_rng(rows * 1000 + cols + ld)
            X = _data(rng, rows * ld, ld)
            x = X.reshape(rows, ld)[:, :cols]
            acc = mode.startswith("accumulate")
            outs = []
            for _ in range(1 if mode in ("out", "accumulate_out_only") else 2):
                whole, view = gr.guarded(cols, DEV)
                init = (rng.standard_normal(cols) * 10).astype(np.float32) if acc else None
                if acc:
                    view.copy_(torch.from_numpy(init))
                outs.append((whole, view, init))
            hipops.colsum(torch.from_numpy(X).to(DEV), rows, cols, ld, outs[0][1], outs[1][1] if len(outs) == 2 else None, accumulate=acc)
            torch.cuda.synchronize()
            for whole, view, init in outs:
                want = x.astype(np.float64).sum(0) + (init.astype(np.float64) if acc else 0.0)
                bnd = gr.colsum_bound(x, init)
                err = np.abs(view.cpu().numpy().astype(np.float64) - want)
                gr.assert_untouched(whole, np.ones(cols, dtype=bool), f"colsum {rows}x{cols} ld={ld}")
                worst = max(worst, float((err / bnd).max()))
                assert np.all(err <= bnd), (rows, cols, ld, mode, float((err / bnd).max()))
            if len(outs) == 2 and not acc:
                assert torch.equal(outs[0][1], outs[1][1])
    print(f"colsum rows={rows} {mode}: worst err/bound {worst:.2e}")
