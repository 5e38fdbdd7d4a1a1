"""The two persistent sweeps of csrc/lstm.hip against fp64 OFF the headline's geometry (tests/lstm_geometry_ref.py: the case table
and the oracle): loaders that read HBM themselves (flags bit 2, B > 64) past every lap of their LDS rings, and staged sweeps with
three and four batch groups past every lap of the helpers' staging rings.  At the layer (functional.blstm_layer) and at the two
sweep entry points; no train step, no concurrent stream (feed-ahead is switched off for this file: the projection runs first).

One run of a (case, mode, flags) is cached on the device and shared by every check that needs it; the oracle is cached per case."""
import pytest
import torch

import lstm_geometry_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("f32", "bf16x3")
G, H = 8 * R.HID, R.HID
GUARD_ROWS = 16           # rows of NaN behind every buffer a sweep writes: a group's rows past B would land there at the last frame
LAYER_KEYS = ("y", "dx") + tuple(f"grad{i}" for i in range(8))
SWEEP_KEYS = ("out", "cbuf", "acts", "dgates", "dbias_part")

_RUNS = {}


def _guarded(T, B, width):
    """A (T,B,width) view of a NaN-filled buffer with GUARD_ROWS more rows behind it -> (view, guard)."""
    full = torch.full(((T * B + GUARD_ROWS) * width,), float("nan"), device=DEV)
    return full[:T * B * width].view(T, B, width), full[T * B * width:]


def _fresh_sweep_workspaces():
    """Forget the cached sweep workspaces (after checking their error words): the next sweep allocates a zeroed one of its own size."""
    from policy_gradient_asr_amd import hipops
    hipops.lstm_assert_no_timeouts()
    for key in [k for k in hipops._ws_cache if k[0].startswith("lstm")]:
        del hipops._ws_cache[key]


def _run(c, mode, flags):
    """Layer forward + backward, then the sequential sweep order of test_dense_lstm_gpu._streamed_case (lstm_pack, gemm,
    lstm_layer_fwd, lstm_layer_bwd(want_dbias=True)) on the same inputs -> dict of device tensors."""
    from policy_gradient_asr_amd import functional as Fh, hipops
    params, x, dy, lengths = R.make_inputs(c)
    T, B = c.T, c.B
    xd, dyd, ln = x.to(DEV), dy.to(DEV), lengths.to(torch.int32).to(DEV)
    prev_flags, prev_feed = hipops.LSTM_FLAGS, Fh.FEED_AHEAD
    hipops.LSTM_FLAGS, Fh.FEED_AHEAD = flags, False
    try:
        with hipops.precision(mode):
            pg = [p.to(DEV).requires_grad_(True) for p in params]
            xg = xd.clone().requires_grad_(True)
            y = Fh.blstm_layer(xg, ln, pg)
            y.backward(dyd)
            torch.cuda.synchronize()
            hipops.lstm_assert_no_timeouts()
            r = {"y": y.detach(), "dx": xg.grad}
            r.update({f"grad{i}": p.grad for i, p in enumerate(pg)})

            wih, bias, pf, pb = hipops.lstm_pack([p.detach().contiguous() for p in pg], R.IN_DIM)
            (gates, g_guard), (out, o_guard), (cbuf, c_guard) = _guarded(T, B, G), _guarded(T, B, 2 * H), _guarded(T, B, 2 * H)
            hipops.gemm(xd, wih, gates, M=T * B, N=G, K=R.IN_DIM, transB=True, bias=bias)
            hipops.lstm_layer_fwd(gates, out, cbuf, pf, ln, T, B)           # gates := saved activations
            r["acts"] = gates.clone()
            _, part = hipops.lstm_layer_bwd(gates, out, cbuf, dyd, pb, ln, T, B, want_dbias=True)      # gates := d(pre-activations)
            torch.cuda.synchronize()
            hipops.lstm_assert_no_timeouts()
            r.update({"out": out, "cbuf": cbuf, "dgates": gates, "dbias_part": part})
            r["guards"] = (g_guard, o_guard, c_guard)
    finally:
        hipops.LSTM_FLAGS, Fh.FEED_AHEAD = prev_flags, prev_feed
    return r


def _cached_run(c, mode, flags):
    key = (R.case_id(c), mode, flags)
    if key not in _RUNS:
        _RUNS[key] = _run(c, mode, flags)
    return _RUNS[key]


def _same_bits(a, b, keys=LAYER_KEYS + SWEEP_KEYS):
    return [k for k in keys if not torch.equal(a[k], b[k])]


def _layer_errors(c, r):
    o = R.oracle(c)
    e = {"out": R.rel_err(r["y"].cpu(), o["y"]), "dx": R.rel_err(r["dx"].cpu(), o["dx"])}
    for i, want in enumerate(o["grads"]):
        e[f"grad{i}"] = R.rel_err(r[f"grad{i}"].cpu(), want)
    return e


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_layer_vs_fp64(c):
    """(a) functional.blstm_layer forward and backward with the flags the case is about: output, dx and the eight parameter gradients
    within 1e-5 ("f32") / 1e-3 ("bf16x3") of fp64 in the max norm, the f32 output the more exact of the two, exact zeros past
    every length."""
    errs = {}
    for mode in MODES:
        r = _cached_run(c, mode, R.native_flags(c))
        errs[mode] = _layer_errors(c, r)
        for b, n in enumerate(c.lens):
            assert torch.all(r["y"][n:, b] == 0)
    worst = {m: max(e.values()) for m, e in errs.items()}
    print(f"[geometry layer] T={c.T} B={c.B} {c.path}: worst rel err vs fp64  f32 {worst['f32']:.2e} (out {errs['f32']['out']:.2e})   "
          f"bf16x3 {worst['bf16x3']:.2e} (out {errs['bf16x3']['out']:.2e})")
    assert worst["f32"] < R.BOUND["f32"], errs["f32"]
    assert worst["bf16x3"] < R.BOUND["bf16x3"], errs["bf16x3"]
    assert errs["f32"]["out"] < errs["bf16x3"]["out"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_sweeps_vs_fp64(c, mode):
    """(b) the two sweep entry points: out, c_t and the saved activations of the forward sweep, d(pre-activations) and the bias
    partial sums (by group and summed) of the backward sweep against fp64 at the same bounds; exact zeros past every length (c_t:
    zero in the reverse direction, the held last state in the forward one); every element of every buffer written, none behind it."""
    r = _cached_run(c, mode, R.native_flags(c))
    o = R.oracle(c)
    T, B = c.T, c.B
    out, cbuf = r["out"].cpu(), r["cbuf"].cpu().view(T, B, 2, H)
    acts, dgates = r["acts"].cpu().view(T, B, 2, H, 4), r["dgates"].cpu().view(T, B, 2, H, 4)
    part = r["dbias_part"].cpu().view(-1, 2, H, 4)
    for name, t in (("out", out), ("cbuf", cbuf), ("acts", acts), ("dgates", dgates), ("dbias_part", part)):
        assert bool(torch.isfinite(t).all()), f"{name}: an element was not written (or is not finite)"
    for guard in r["guards"]:
        assert bool(torch.isnan(guard).all()), "a sweep wrote behind its buffer"
    assert part.shape[0] == (B + 15) // 16
    e = {"out": R.rel_err(out, o["y"]), "c": R.rel_err(cbuf, o["c"]), "acts": R.rel_err(acts, o["acts"]),
         "dgates": R.rel_err(dgates, o["dgates"]), "dbias": R.rel_err(part.double().sum(0), o["dbias"])}
    for i in range(part.shape[0]):
        e[f"dbias_group{i}"] = R.rel_err(part[i], o["dbias_group"][i])
    print(f"[geometry sweeps] T={T} B={B} {c.path} {mode}: " + "  ".join(f"{k} {v:.2e}" for k, v in e.items() if not k.startswith("dbias_group"))
          + f"  dbias by group {max(v for k, v in e.items() if k.startswith('dbias_group')):.2e}")
    assert max(e.values()) < R.BOUND[mode], e
    for b, n in enumerate(c.lens):
        assert not out[n:, b].any() and not acts[n:, b].any() and not dgates[n:, b].any(), b
        assert not cbuf[n:, b, 1].any(), b
        assert torch.equal(cbuf[n:, b, 0], cbuf[n - 1, b, 0].expand(T - n, -1)), b


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", R.BITWISE_CASES, ids=R.case_id)
def test_staging_does_no_arithmetic(c, mode):
    """(c) helpers on (flags 0) against loaders that read HBM themselves (flags 4): loader_issue is an LDS-DMA into the same slot
    either way, so every tensor of the layer and of the sweeps has the same bits; the write-through protocol (flags 1 and 5) as
    well, on one case per family."""
    base = _cached_run(c, mode, 0)
    others = (4,) + ((1, 5) if c in R.WRITE_THROUGH_CASES else ())
    for flags in others:
        assert _same_bits(base, _cached_run(c, mode, flags)) == [], (c.T, c.B, flags)
    # .. and the flags-0 run is itself held to fp64 (the "4" rows are held with flags 4 above, the others with flags 0)
    assert max(_layer_errors(c, base).values()) < R.BOUND[mode]


def test_weight_gradients_of_a_two_frame_sweep_over_sixteen_utterances():
    """What the (2, 16) case found: hipops.lstm_wgrads_ok promises the six-product weight-gradient launch for B % 16 == 0 from
    T = 2 on, but dW_hh is then ONE 16-row k-step and the launch check asked for 32 rows of every kernel, so the "f32" layer
    raised.  The launch on the sweep's own d(pre-activations), against their fp64 products at fp32-GEMM accuracy (2e-6, the
    bound of test_dense_lstm_gpu._streamed_case); the same launch still refuses what it always did."""
    from policy_gradient_asr_amd import hipops, _lib
    c = R.case(2, 16)
    T, B = c.T, c.B
    assert hipops.lstm_wgrads_ok(T, B, R.IN_DIM, 3) and not hipops.lstm_wgrads_ok(T, B, R.IN_DIM, 2) and not hipops.lstm_wgrads_ok(1, B, R.IN_DIM, 3)
    r = _cached_run(c, "f32", R.native_flags(c))
    _, x, _, _ = R.make_inputs(c)
    dwih = torch.full((G, R.IN_DIM), float("nan"), device=DEV)
    dwhh = torch.full((2, 4 * H, H), float("nan"), device=DEV)
    hipops.lstm_wgrads(r["dgates"], x.to(DEV), r["out"], T, B, R.IN_DIM, dwih, dwhh, planes=3)
    torch.cuda.synchronize()
    d64, x64, o64 = r["dgates"].double().cpu(), x.double(), r["out"].double().cpu()
    assert R.rel_err(dwih.cpu(), d64.reshape(T * B, G).t() @ x64.reshape(T * B, R.IN_DIM)) < 2e-6
    assert R.rel_err(dwhh[0].cpu(), d64[1:, :, :4 * H].reshape(-1, 4 * H).t() @ o64[:-1, :, :H].reshape(-1, H)) < 2e-6
    assert R.rel_err(dwhh[1].cpu(), d64[:-1, :, 4 * H:].reshape(-1, 4 * H).t() @ o64[1:, :, H:].reshape(-1, H)) < 2e-6
    with pytest.raises(_lib.PgasrError):          # 16 rows are no k-step of the bf16x3 kernel
        hipops.lstm_wgrads(r["dgates"], x.to(DEV), r["out"], T, B, R.IN_DIM, dwih, dwhh, planes=2)


@pytest.mark.parametrize("mode", MODES)
def test_one_workspace_changing_geometry(mode):
    """(d) The sweep workspaces are cached and only grow, and lstm_prepare_kernel sizes its fill from the CURRENT layout: a smaller
    geometry after a larger one finds the larger one's hello / ready / progress words and exchange slots behind its own.  Sixteen
    clusters, then one pair without helpers, then three staged pairs, then sixteen again, each with the bits it gives on a
    workspace of its own."""
    seq = [(R.case(T, B), flags) for T, B, flags in R.GEOMETRY_SEQUENCE]
    alone = {}
    for c, flags in seq:
        if (c, flags) not in alone:
            _fresh_sweep_workspaces()
            alone[(c, flags)] = _run(c, mode, flags)
    _fresh_sweep_workspaces()
    for i, (c, flags) in enumerate(seq):
        assert _same_bits(alone[(c, flags)], _run(c, mode, flags)) == [], (i, c.T, c.B, flags)
    for (c, flags), r in alone.items():
        assert max(_layer_errors(c, r).values()) < R.BOUND[mode]


def test_fed_and_streamed_sweeps_are_refused_here():
    """(e) No helpers (flags bit 2) or more than two groups: lstm_fed_ok says no, and the fed / streamed entry points raise and
    launch no sweep (every buffer keeps its NaN fill, the counters stay zero).  129 utterances are refused outright."""
    from policy_gradient_asr_amd import hipops, _lib
    params, _, _, _ = R.make_inputs(R.SMALLEST)
    _, _, pf, pb = hipops.lstm_pack([p.to(DEV) for p in params], R.IN_DIM)
    assert hipops.LSTM_FLAGS == 0
    assert hipops.lstm_fed_ok(13, 32) and not hipops.lstm_fed_ok(13, 33) and not hipops.lstm_fed_ok(37, 64) and not hipops.lstm_fed_ok(14, 128)
    for T, B, flags in ((13, 33, 0), (13, 16, 4), (13, 32, 5), (14, 65, 0)):
        hipops.LSTM_FLAGS = flags
        try:
            assert not hipops.lstm_fed_ok(T, B)
            gates, out, cbuf = (torch.full((T, B, w), float("nan"), device=DEV) for w in (G, 2 * H, 2 * H))
            dout = torch.zeros(T, B, 2 * H, device=DEV)
            ln = torch.full((B,), T, dtype=torch.int32, device=DEV)
            fed = torch.zeros(2 * ((T * B + 255) // 256), dtype=torch.int32, device=DEV)
            words = torch.zeros(64, dtype=torch.int32, device=DEV)
            with pytest.raises(_lib.PgasrError):
                hipops.lstm_layer_fwd(gates, out, cbuf, pf, ln, T, B, fed=fed, fed_need=G // 256)
            with pytest.raises(_lib.PgasrError):
                hipops.lstm_layer_bwd(gates, out, cbuf, dout, pb, ln, T, B, fed=fed, fed_need=2 * H // 256)
            with pytest.raises(_lib.PgasrError):
                hipops.lstm_layer_bwd(gates, out, cbuf, dout, pb, ln, T, B, slab=words)
            torch.cuda.synchronize()
            assert all(bool(torch.isnan(t).all()) for t in (gates, out, cbuf)) and not fed.any() and not words.any()
        finally:
            hipops.LSTM_FLAGS = 0
    T, B = 2, R.MAX_B + 1
    gates, out, cbuf = (torch.full((T, B, w), float("nan"), device=DEV) for w in (G, 2 * H, 2 * H))
    ln = torch.full((B,), T, dtype=torch.int32, device=DEV)
    for flags in (0, 4):
        hipops.LSTM_FLAGS = flags
        try:
            with pytest.raises(_lib.PgasrError):
                hipops.lstm_layer_fwd(gates, out, cbuf, pf, ln, T, B)
            with pytest.raises(_lib.PgasrError):
                hipops.lstm_layer_bwd(gates, out, cbuf, torch.zeros(T, B, 2 * H, device=DEV), pb, ln, T, B)
        finally:
            hipops.LSTM_FLAGS = 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (gates, out, cbuf))
    hipops.lstm_assert_no_timeouts()
