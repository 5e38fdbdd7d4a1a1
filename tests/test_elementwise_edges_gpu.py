"""The small kernels of csrc/optim.hip and csrc/attention.hip against byte and fp64 oracles at their edges: the batch copy
(pgasr_stream_copy, the hand-over of every batch of the timed step), Adam (pgasr_adam_step[_clipped]), the error flag of the
gradient all-reduce (pgasr_error_flag), the decoder's LSTM cell (pgasr_lstm_cell_f32) and the reference's attention context
(pgasr_attention_ctx).  Oracles, bounds and case tables: tests/elementwise_ref.py; none of the bounds comes from a kernel, and
tests/test_elementwise_ref_cpu.py holds plain fp32 arithmetic to half of each.  Every test prints its worst err / bound.

    copy        no tolerance: the destination's bytes are the source's (NaN payloads, -0.0 included) and every byte around the
                destination keeps its fill, at every size where the kernel takes another path (8-deep body, remainder loop,
                byte tail, fewer than 16 bytes), from device and pinned host sources, for 1 .. 1024 workgroups
    Adam        one fp64 step from the fp32 state the kernel was given: p, exp_avg and exp_avg_sq each within E_p, E_m, E_v
    error flag  exactly 0.0 or 1.0 in word 0, nothing else written
    LSTM cell   c', h' within the sensitivity bounds E_c, E_h with K = elementwise_ref.LSTM_K; no NaN where expf overflows
    attention   per entry within (C eps (1 + X) + 2e-6) A + FL with C = elementwise_ref.ATTN_C, finite where the reference's own
                exp is finite (products up to 75, results up to 5e29)

Worst err / bound on an MI355X: NOTES.md 0.33."""
import functools

import numpy as np
import pytest
import torch

import elementwise_ref as er

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 48             # the destination starts 48 bytes into a buffer of fill bytes: a multiple of 16, not of 64


@pytest.fixture(scope="module")
def ops():
    from policy_gradient_asr_amd import hipops
    return hipops


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8)


# ------------------------------------------------------------------------------------------------------------------------
# A. batch copy
# ------------------------------------------------------------------------------------------------------------------------
def _source(src_np, where, dtype):
    t = torch.from_numpy(src_np).view(dtype)
    if where == "device":
        return t.to(DEV)
    pinned = torch.empty(t.shape, dtype=dtype, pin_memory=True)
    pinned.copy_(t)
    return pinned


def _framed(nbytes, dtype=torch.uint8):
    big = torch.full((PAD + nbytes + 64,), er.COPY_FILL, dtype=torch.uint8, device=DEV)
    return big, big[PAD:PAD + nbytes].view(dtype)


def _differing(big, src_np):
    """Bytes of the framed buffer that are not what a perfect copy leaves: the source inside, the fill around it."""
    want = torch.full((big.numel(),), er.COPY_FILL, dtype=torch.uint8)
    want[PAD:PAD + src_np.size] = torch.from_numpy(src_np)
    got = big.cpu()
    return 0 if torch.equal(got, want) else int((got != want).sum())


def _copy_case(ops, nbytes, where, dtype=torch.uint8, workgroups=None):
    src_np = er.copy_source(nbytes, nbytes)
    src = _source(src_np, where, dtype)
    big, dst = _framed(nbytes, dtype)
    assert dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
    out = ops.stream_copy(dst, src) if workgroups is None else ops.stream_copy(dst, src, workgroups=workgroups)
    assert out is dst
    bad = _differing(big, src_np)                            # (.cpu() waits for the kernel: a pinned source lives until here)
    assert bad == 0, (nbytes, where, dtype, workgroups, bad)
    assert torch.equal(_bits(dst), torch.from_numpy(src_np))


@pytest.mark.parametrize("where", ["device", "pinned"])
def test_stream_copy_every_path_bytes_exact(ops, where):
    for nbytes in er.COPY_SIZES:
        _copy_case(ops, nbytes, where)
    print(f"[stream copy] {where} source, {len(er.COPY_SIZES)} sizes of 1 .. {max(er.COPY_SIZES)} bytes, 8 workgroups: 0 bytes differ")


@pytest.mark.parametrize("where", ["device", "pinned"])
def test_stream_copy_workgroup_counts(ops, where):
    for wg, nbytes in er.COPY_WORKGROUP_CASES:
        _copy_case(ops, nbytes, where, workgroups=wg)
    print(f"[stream copy] {where} source, (workgroups, bytes) {er.COPY_WORKGROUP_CASES}: 0 bytes differ")


@pytest.mark.parametrize("where", ["device", "pinned"])
@pytest.mark.parametrize("dtype", [torch.int64, torch.float32])
def test_stream_copy_typed(ops, where, dtype):
    _copy_case(ops, er.COPY_TYPED_BYTES, where, dtype=dtype)
    print(f"[stream copy] {where} source as {dtype}, {er.COPY_TYPED_BYTES} bytes: 0 bytes differ")


def test_stream_copy_back_to_back_on_a_side_stream(ops):
    from policy_gradient_asr_amd import streams
    nbytes = 16385 * 16 + 15
    src_np = er.copy_source(nbytes, 7)
    src = _source(src_np, "pinned", torch.uint8)
    big1, dst1 = _framed(nbytes)
    big2, dst2 = _framed(nbytes)
    main = torch.cuda.current_stream()
    side = streams.side_stream("elementwise_edges_copy")
    assert side.cuda_stream != main.cuda_stream
    side.wait_stream(main)                                   # the fills above ran on the main stream
    with torch.cuda.stream(side):
        ops.stream_copy(dst1, src)                           # host -> device
        ops.stream_copy(dst2, dst1)                          # device -> device, behind it in stream order
    main.wait_stream(side)
    bad = _differing(big1, src_np) + _differing(big2, src_np)
    print(f"[stream copy] two copies back to back on a side stream, {nbytes} bytes: {bad} bytes differ")
    assert bad == 0


def test_stream_copy_refusals(ops):
    from policy_gradient_asr_amd._lib import PgasrError
    dst = torch.zeros(256, dtype=torch.uint8, device=DEV)
    src = torch.ones(256, dtype=torch.uint8, device=DEV)
    with pytest.raises(PgasrError, match="pinned"):
        ops.stream_copy(dst, torch.ones(256, dtype=torch.uint8))                 # a pageable host source never reaches the kernel
    with pytest.raises(PgasrError, match="one dtype and size"):
        ops.stream_copy(dst, src[:255])
    with pytest.raises(PgasrError, match="one dtype and size"):
        ops.stream_copy(dst, src.view(torch.int32))
    with pytest.raises(PgasrError, match="destination on the GPU"):
        ops.stream_copy(torch.empty(256, dtype=torch.uint8, pin_memory=True), src)
    buf = torch.zeros(257, dtype=torch.uint8, device=DEV)
    with pytest.raises(PgasrError, match="status 1"):                            # INVALID_ARG: 16-byte loads need aligned ends
        ops.stream_copy(dst, buf[1:])
    with pytest.raises(PgasrError, match="status 1"):
        ops.stream_copy(buf[1:], src)
    for wg in (0, 1025, -1):
        with pytest.raises(PgasrError, match="status 1"):
            ops.stream_copy(dst, src, workgroups=wg)
    torch.cuda.synchronize()
    assert not dst.any() and not buf.any()                                       # a refused call wrote nothing
    empty = torch.empty(0, dtype=torch.uint8, device=DEV)
    assert ops.stream_copy(empty, torch.empty(0, dtype=torch.uint8, device=DEV)) is empty


# ------------------------------------------------------------------------------------------------------------------------
# B. Adam
# ------------------------------------------------------------------------------------------------------------------------
def _adam_launch(ops, p, g, m, v, step, name, **kw):
    lr, b1, b2, eps, wd = (float(x) for x in er.adam_hyper32(name))
    ops.adam_step(p, g, m, v, step, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, **kw)


def _adam_step_vs_oracle(ops, dp, dm, dv, g, t, name, label, step=None, **kw):
    """One call on the device state (dp, dm, dv) against one fp64 step from that same state at bias-correction count t."""
    p, m, v = (x.cpu().numpy() for x in (dp, dm, dv))
    want = er.adam_oracle(p, g, m, v, t, name)
    er.adam_preconditions(p, g, m, v, want)
    _adam_launch(ops, dp, _dev(g), dm, dv, t if step is None else step, name, **kw)
    p2, m2, v2 = (x.cpu().numpy() for x in (dp, dm, dv))
    r = er.adam_ratios(p2, m2, v2, want)
    print(f"[adam] {label} t={t}: err / bound p {r[0]:.3f} exp_avg {r[1]:.3f} exp_avg_sq {r[2]:.3f}")
    zero, _ = er.adam_index_sets(p.shape[0])
    if zero.size and er.ADAM_HYPER[name][4] == 0:            # g = m = v = 0, no decay: p keeps its bits, the moments stay 0
        assert np.array_equal(p2[zero].view(np.uint32), p[zero].view(np.uint32)) and not m2[zero].any() and not v2[zero].any()
    assert max(r) <= 1.0, (label, t, r)
    return r


@pytest.mark.parametrize("name,p_zero", er.ADAM_CHAINS)
def test_adam_chain_each_call_vs_one_fp64_step(ops, name, p_zero):
    """t = 1, 2, 3, 10, 1000, 20000 at n = 10007 with applied=None (step is t); from p = 0 the first update is held to E_u."""
    dp, dm, dv = (_dev(x) for x in er.adam_state(er.ADAM_CHAIN_N, name, 11, p_zero=p_zero, fresh=True))
    worst = np.zeros(3)
    for k, t in enumerate(er.ADAM_CHAIN_T):
        g = er.adam_grad(dp.cpu().numpy(), dm.cpu().numpy(), name, 100 + k, call=k)
        worst = np.maximum(worst, _adam_step_vs_oracle(ops, dp, dm, dv, g, t, name, f"chain {name} p0={p_zero}"))
    print(f"[adam] chain {name} p0={p_zero}: worst err / bound p {worst[0]:.3f} exp_avg {worst[1]:.3f} exp_avg_sq {worst[2]:.3f}")


@pytest.mark.parametrize("n,t", er.ADAM_SINGLE)
def test_adam_single_call_sizes(ops, n, t):
    """n < 4 (tail only), 4, 5, sizes with a tail behind the quads, and 2^21 + 7: the second pass of the grid-stride loop."""
    worst = np.zeros(3)
    for name in er.ADAM_HYPER:
        p, m, v = er.adam_state(n, name, n)
        g = er.adam_grad(p, m, name, n + 1)
        worst = np.maximum(worst, _adam_step_vs_oracle(ops, _dev(p), _dev(m), _dev(v), g, t, name, f"n={n} {name}"))
    print(f"[adam] n={n}: worst err / bound p {worst[0]:.3f} exp_avg {worst[1]:.3f} exp_avg_sq {worst[2]:.3f}")


def test_adam_guards_and_applied_count(ops):
    """Six calls, step = 1 .. 6, a guard word set on calls 2 and 5: those keep p, m, v bit for bit, the applied words read
    1, 1, 2, 3, 3, 4, and every applied call is the oracle's step at t = the applied count.  Then a clip state whose non-finite
    flag is set skips like a guard, and one with scale 1 is the plain step."""
    name, n = "decay", 1027
    dp, dm, dv = (_dev(x) for x in er.adam_state(n, name, 5))
    applied = torch.zeros(2, dtype=torch.int32, device=DEV)
    guard = torch.zeros(4, dtype=torch.int32, device=DEV)
    counts, worst = [], np.zeros(3)

    def skipped_call(step, **kw):
        before = [_bits(x) for x in (dp, dm, dv)]
        g = er.adam_grad(dp.cpu().numpy(), dm.cpu().numpy(), name, 200 + step, call=step)
        _adam_launch(ops, dp, _dev(g), dm, dv, step, name, applied=applied, **kw)
        assert all(torch.equal(b, _bits(x)) for b, x in zip(before, (dp, dm, dv))), step

    for step in range(1, 7):
        if step in (2, 5):
            guard[1] = 7 if step == 2 else -1
            skipped_call(step, guards=[guard.data_ptr() + 4])
            guard[1] = 0
        else:
            t = (counts[-1] if counts else 0) + 1
            g = er.adam_grad(dp.cpu().numpy(), dm.cpu().numpy(), name, 200 + step, call=step)
            worst = np.maximum(worst, _adam_step_vs_oracle(ops, dp, dm, dv, g, t, name, f"guarded sequence step={step}", step=step,
                                                           guards=[guard.data_ptr(), guard.data_ptr() + 4], applied=applied))
        counts.append(int(applied[step & 1]))
    assert counts == [1, 1, 2, 3, 3, 4], counts
    state = ops.clip_state(DEV)
    state[1] = 1.0
    state.view(torch.int32)[2] = 1                           # nonfinite
    skipped_call(7, clip_state=state)
    assert int(applied[7 & 1]) == 4
    state.view(torch.int32)[2] = 0
    g = er.adam_grad(dp.cpu().numpy(), dm.cpu().numpy(), name, 208, call=8)
    worst = np.maximum(worst, _adam_step_vs_oracle(ops, dp, dm, dv, g, 5, name, "clip state with scale 1, step=8", step=8,
                                                   applied=applied, clip_state=state))
    assert int(applied[8 & 1]) == 5
    print(f"[adam] guards and applied count: worst err / bound p {worst[0]:.3f} exp_avg {worst[1]:.3f} exp_avg_sq {worst[2]:.3f}")


# ------------------------------------------------------------------------------------------------------------------------
# C. error flag
# ------------------------------------------------------------------------------------------------------------------------
def test_error_flag_word():
    from policy_gradient_asr_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    nan_bits = 0x7FC12345
    for w0, w1, want in ((None, None, 0.0), (0, None, 0.0), (1, None, 1.0), (0, 7, 1.0), (-1, 0, 1.0), (None, 3, 1.0)):
        words = torch.tensor([w0 or 0, w1 or 0], dtype=torch.int32, device=DEV)
        out = torch.full((8,), nan_bits, dtype=torch.int32, device=DEV).view(torch.float32)
        _lib.check(lib.pgasr_error_flag(None if w0 is None else words.data_ptr(), None if w1 is None else words.data_ptr() + 4,
                                        out.data_ptr(), stream), "pgasr_error_flag")
        got = out.cpu()
        assert _bits(got[:1]).tolist() == _bits(torch.tensor([want])).tolist(), (w0, w1, got[0])
        assert (got[1:].view(torch.int32) == nan_bits).all(), (w0, w1)
        assert words.tolist() == [w0 or 0, w1 or 0]
    assert lib.pgasr_error_flag(None, None, None, stream) == 1                   # INVALID_ARG
    print("[error flag] 6 word pairs: word 0 exact, 7 NaN words around it untouched")


# ------------------------------------------------------------------------------------------------------------------------
# D. decoder LSTM cell
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", er.LSTM_SHAPES)
def test_lstm_cell_vs_fp64(ops, B, H):
    worst = {"c": 0.0, "h": 0.0}
    for gs, cs in er.LSTM_SCALES:
        gh, xp, c, h = er.lstm_case(B, H, gs, cs)
        want = er.lstm_oracle(gh, xp, c)
        er.lstm_preconditions(gh, xp, c, want)
        for with_out in (False, True):
            dgh, dxp, dc, dh = (_dev(x) for x in (gh, xp, c, h))
            h_out = torch.full((B, H), float("nan"), device=DEV) if with_out else None
            assert ops.lstm_cell(dgh, dxp, dc, dh, h_out) is None
            assert torch.equal(_bits(dgh), _bits(torch.from_numpy(gh))) and torch.equal(_bits(dxp), _bits(torch.from_numpy(xp)))
            got = {"c": dc.cpu().numpy(), "h": dh.cpu().numpy()}            # c and h are updated in place
            if with_out:
                assert torch.equal(_bits(h_out), _bits(dh))
            for key in ("c", "h"):
                assert np.isfinite(got[key]).all(), (B, H, gs, cs, key)      # expf overflows at scale 30: the gate is 0 or 1, never NaN
                ratio = float((np.abs(got[key].astype(np.float64) - want[key]) / want["E_" + key]).max())
                worst[key] = max(worst[key], ratio)
                assert ratio <= 1.0, (B, H, gs, cs, key, with_out, ratio)
            if gs == 30.0:
                assert (np.abs(got["h"]) <= 1.0).all()
    print(f"[lstm cell] B={B} H={H}, K={er.LSTM_K}: worst err / bound c' {worst['c']:.3f} h' {worst['h']:.3f}")


# ------------------------------------------------------------------------------------------------------------------------
# E. attention context
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _attn(case):
    d, e = er.attn_case(*case)
    want = er.attn_oracle(d, e)
    er.attn_preconditions(want)
    return d, e, want


@pytest.mark.parametrize("case", er.ATTN_CASES, ids=lambda c: "L{}-B{}-H{}-T{}-s{}".format(*c[:5]))
def test_attention_ctx_vs_oracle(ops, case):
    d, e, want = _attn(case)
    dd, de = _dev(d), _dev(e)
    got = ops.attention_ctx(dd, de)                          # (L, B, H): NQ = L B rows, row q belongs to utterance q % B
    again = ops.attention_ctx(dd, de)
    assert got.shape == dd.shape and torch.equal(_bits(got), _bits(again))
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - want["c"])         # want["c"][l] = oracle.attn_ref.attention_ctx(d[l], e)
    ratio = float((err / er.attn_bound(want)).max())
    print(f"[attention ctx] L,B,H,T,scale={case[:5]}, C={er.ATTN_C}: worst err / bound {ratio:.3f}, max |d e| {want['X'].max():.1f}, "
          f"max |c| {np.abs(want['c']).max():.2e}, err / max |c| {err.max() / np.abs(want['c']).max():.1e}")
    assert ratio <= 1.0, (case, ratio)


def test_attention_ctx_refusals(ops):
    from policy_gradient_asr_amd._lib import PgasrError
    with pytest.raises(PgasrError, match="status 4"):        # UNSUPPORTED: d and one frame must fit the LDS
        ops.attention_ctx(torch.zeros(1, 8193, device=DEV), torch.zeros(1, 1, 8193, device=DEV))
    with pytest.raises(PgasrError, match="multiple of B"):
        ops.attention_ctx(torch.zeros(3, 64, device=DEV), torch.zeros(2, 5, 64, device=DEV))
    with pytest.raises(PgasrError, match="same H"):
        ops.attention_ctx(torch.zeros(2, 64, device=DEV), torch.zeros(2, 5, 32, device=DEV))
