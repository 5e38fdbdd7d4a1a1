"""The discrete kernels -- edit distance (csrc/editdist.hip), path collapse, arg-max and per-frame reward-to-go coefficients
(csrc/frame_ops.hip), the Viterbi backtrace (csrc/align.hip) -- against plain oracles at every template instantiation and every
chunk seam.  All comparisons are exact (integers, fp64 bit for bit) except the per-step coefficients, whose three fp32
operations are held to rtol 1e-6 / atol 1e-9 as in test_pg_ctc_loss_per_step_rewards_vs_oracle.

Which case reaches which instantiation.

edit_distance_kernel<J>: J is the smallest power of two >= ceil((col_max + 1) / 64), col_max = R with prefix distances,
max(R, Hy) without.  test_edit_distance_tilings runs every col_max below with prefix (R = col_max, Hy = 70) and without
(R = col_max, Hy = 70, and the swapped R = 70, Hy = col_max):
    col_max   63 -> J = 1      64, 127 -> J = 2     128, 255 -> J = 4     256, 511 -> J = 8
    512, 1023 -> J = 16        1024, 2047 -> J = 32                       2048, 4095 -> J = 64
col_max = 64 J - 1 (63, 127, 255, 511, 1023, 2047, 4095) fills the last lane's last cell.  The headline train step's call
(J = 16, no prefix, operands swapped) is col_max = 1023 in the swapped geometry.

align_fwd_kernel<NSPT>: the smallest of 1, 2, 4, 8 with 2 Lmax + 1 <= 256 NSPT.  test_align_exact_fit has T = L at
    L = 33, 64, 65, 66, 67, 127 -> NSPT = 1     128, 255 -> NSPT = 2     256, 511 -> NSPT = 4     512, 1023 -> NSPT = 8

Mutants these tests were shown to catch are listed in the commit that added this file."""
import functools

import numpy as np
import pytest
import torch

import align_ref
import discrete_ref as D
from oracle import decode_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ops():
    from policy_gradient_asr_amd import hipops
    return hipops


def _err():
    from policy_gradient_asr_amd._lib import PgasrError
    return PgasrError


def _i32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.int32).to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------------------------------
# edit distance
# ------------------------------------------------------------------------------------------------------------------------
def _pack(pairs, R, Hy):
    """[(ref, hyp)] -> zero-padded ref (N,R), ref_len, hyp (N,Hy), hyp_len"""
    N = len(pairs)
    ref, hyp = np.zeros((N, R), np.int32), np.zeros((N, Hy), np.int32)
    rl, hl = np.zeros(N, np.int32), np.zeros(N, np.int32)
    for k, (r, h) in enumerate(pairs):
        rl[k], hl[k] = len(r), len(h)
        ref[k, :len(r)], hyp[k, :len(h)] = r, h
    return ref, rl, hyp, hl


def _ed_run(ref, rl, hyp, hl, want_prefix):
    """one call; dist and (with want_prefix) every prefix distance against D.ed_prefix on the clamped lengths, the wrapper's -1
    fill beyond each row's hypothesis; returns dist"""
    ref, hyp = np.asarray(ref, np.int32), np.asarray(hyp, np.int32)
    (N, R), Hy = ref.shape, hyp.shape[1]
    out = _ops().edit_distance(_i32(ref), _i32(rl), _i32(hyp), _i32(hl), want_prefix=want_prefix)
    d, pre = (out[0].cpu().numpy(), out[1].cpu().numpy()) if want_prefix else (out.cpu().numpy(), None)
    assert d.shape == (N,) and (pre is None or pre.shape == (N, Hy + 1))
    for k in range(N):
        n, m = min(max(int(rl[k]), 0), R), min(max(int(hl[k]), 0), Hy)
        want = D.ed_prefix(ref[k, :n], hyp[k, :m])
        assert d[k] == want[-1], (k, n, m, int(d[k]), int(want[-1]))
        if pre is not None:
            bad = np.nonzero(pre[k, :m + 1] != want)[0]
            assert bad.size == 0, (k, n, m, bad[:8], pre[k, bad[:8]], want[bad[:8]])
            assert (pre[k, m + 1:] == -1).all(), (k, n, m)
    return d


ED_COL_MAX = [63, 64, 127, 128, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 4095]
ED_SHORT = 70


def _cells_per_lane(col_max):
    need, J = (col_max + 64) // 64, 1
    while J < need:
        J *= 2
    return J


@pytest.mark.parametrize("geometry", ["prefix", "plain", "plain_swapped"])
@pytest.mark.parametrize("col_max", ED_COL_MAX)
def test_edit_distance_tilings(col_max, geometry):
    """Every instantiation (module docstring), with and without prefix distances and with the operands swapped; lengths at the
    stride, one short of it, 1, 0, on a lane boundary (J k and J k - 1 cells); planted pairs with a known distance."""
    want_prefix = geometry == "prefix"
    R, Hy = (ED_SHORT, col_max) if geometry == "plain_swapped" else (col_max, ED_SHORT)
    J = _cells_per_lane(col_max)
    assert J in (1, 2, 4, 8, 16, 32, 64) and 64 * J > col_max and (J == 1 or 32 * J <= col_max)
    k = min(41, col_max // J - 1)
    assert 0 < k < 63
    rng = np.random.default_rng(col_max)
    long_lens = [col_max, col_max - 1, 1, 0, col_max, J * k, J * k - 1, int(rng.integers(2, col_max))]
    short_lens = [ED_SHORT, ED_SHORT, ED_SHORT, ED_SHORT, 0, ED_SHORT, ED_SHORT - 1, int(rng.integers(2, ED_SHORT))]
    pairs = []
    for i, (a, b) in enumerate(zip(long_lens, short_lens)):
        alpha = 2 if i in (0, 7) else 4                      # the full-length pair and the last one over 2 symbols, the others over 4
        lo, sh = rng.integers(1, alpha + 1, size=a), rng.integers(1, alpha + 1, size=b)
        pairs.append((sh, lo) if geometry == "plain_swapped" else (lo, sh))
    _ed_run(*_pack(pairs, R, Hy), want_prefix)

    planted = D.planted_pairs(R, Hy, rng)
    pairs = [(r, h) for _, r, h, _ in planted]
    pairs.append((rng.integers(1, 5, size=R), rng.integers(1, 5, size=Hy)))
    # two symbols and nearly equal lengths: the best path shifts back and forth, so insertion moves count in every lane in use
    # (where one side is much the longer, every hypothesis token finds a diagonal and no insertion move is ever needed)
    pairs.append((rng.integers(1, 3, size=min(R, ED_SHORT)), rng.integers(1, 3, size=min(Hy, ED_SHORT) - 1)))
    d = _ed_run(*_pack(pairs, R, Hy), want_prefix)
    for i, (name, _, _, want) in enumerate(planted):
        assert d[i] == want, (name, int(d[i]), want)


def test_edit_distance_long_hypothesis_short_reference():
    """R = 40, Hy = 4095 with prefix distances: J = 1 and 4095 rows, every one of them reported"""
    rng = np.random.default_rng(40)
    R, Hy = 40, 4095
    pairs = [(rng.integers(1, 3, size=R), rng.integers(1, 3, size=Hy)), (rng.integers(1, 5, size=R), rng.integers(1, 5, size=Hy)),
             (rng.integers(1, 5, size=R - 1), rng.integers(1, 5, size=Hy - 1)), (rng.integers(1, 5, size=17), rng.integers(1, 5, size=2049))]
    _ed_run(*_pack(pairs, R, Hy), True)


def test_edit_distance_both_at_the_limit():
    """R = Hy = 4095 without prefix distances: J = 64, all 4096 cells in use, with and without the swap"""
    rng = np.random.default_rng(4095)
    R = Hy = 4095
    pairs = [(rng.integers(1, 3, size=R), rng.integers(1, 3, size=Hy)), (rng.integers(1, 5, size=R), rng.integers(1, 5, size=Hy)),
             (rng.integers(1, 5, size=4000), rng.integers(1, 5, size=Hy)), (rng.integers(1, 5, size=R), rng.integers(1, 5, size=3000))]
    _ed_run(*_pack(pairs, R, Hy), False)


@pytest.mark.parametrize("want_prefix", [True, False])
def test_edit_distance_ignores_padding(want_prefix):
    """the tokens beyond each length are a copy of the other row's tokens at the same positions: read, they lower the distance"""
    rng = np.random.default_rng(7)
    N, R = 6, 100
    ref, hyp = rng.integers(1, 4, size=(N, R)).astype(np.int32), rng.integers(1, 4, size=(N, R)).astype(np.int32)
    rl, hl = rng.integers(10, 91, size=N).astype(np.int32), rng.integers(10, 91, size=N).astype(np.int32)
    rl[0], hl[0], rl[1], hl[1] = 30, 90, 90, 30
    ref_p, hyp_p = ref.copy(), hyp.copy()
    for k in range(N):
        ref_p[k, rl[k]:] = hyp[k, rl[k]:]
        hyp_p[k, hl[k]:] = ref[k, hl[k]:]
    d = _ed_run(ref_p, rl, hyp_p, hl, want_prefix)
    read = [D.ed(ref_p[k], hyp_p[k]) for k in range(N)]
    assert any(read[k] != d[k] for k in range(N))            # the poison is one: reading it changes the answer


@pytest.mark.parametrize("want_prefix", [True, False])
def test_edit_distance_clamps_lengths(want_prefix):
    """ref_len = R + 9 acts as R, hyp_len = -3 and ref_len = -1 as 0 (_ed_run's oracle takes the clamped lengths)"""
    rng = np.random.default_rng(9)
    R, Hy = 50, 60
    ref, hyp = rng.integers(1, 5, size=(5, R)), rng.integers(1, 5, size=(5, Hy))
    rl, hl = np.array([R + 9, 20, -1, R + 9, -1]), np.array([30, -3, 25, Hy + 4, -3])
    d = _ed_run(ref, rl, hyp, hl, want_prefix)
    assert d[1] == 20 and d[2] == 25 and d[4] == 0 and d[0] == D.ed(ref[0], hyp[0, :30]) and d[3] == D.ed(ref[3], hyp[3])


@pytest.mark.parametrize("want_prefix", [True, False])
@pytest.mark.parametrize("R,Hy", [(0, 20), (20, 0), (0, 0)])
def test_edit_distance_zero_strides(R, Hy, want_prefix):
    rng = np.random.default_rng(R + 2 * Hy)
    ref, hyp = rng.integers(1, 5, size=(3, R)), rng.integers(1, 5, size=(3, Hy))
    rl, hl = np.array([R, R // 4, 3]), np.array([Hy, 7, Hy // 2])
    d = _ed_run(ref, rl, hyp, hl, want_prefix)
    assert d.tolist() == [max(min(a, R), min(b, Hy)) for a, b in zip(rl, hl)]


@pytest.mark.parametrize("N", [128, 129])
def test_edit_distance_pair_count(N):
    """both sides of the switch between one reserved compute unit per pair and many waves per unit; R = Hy = 90 (J = 2)"""
    rng = np.random.default_rng(N)
    R = Hy = 90
    ref, hyp = rng.integers(1, 4, size=(N, R)), rng.integers(1, 4, size=(N, Hy))
    rl, hl = rng.integers(0, R + 1, size=N), rng.integers(0, Hy + 1, size=N)
    rl[0], hl[0], rl[N - 1], hl[N - 1] = R, Hy, R, Hy - 1
    d1 = _ed_run(ref, rl, hyp, hl, True)
    d2 = _ed_run(ref, rl, hyp, hl, False)
    assert np.array_equal(d1, d2)


def test_edit_distance_refusals():
    ops, err = _ops(), _err()
    one = _i32([1])
    with pytest.raises(err):
        ops.edit_distance(_i32(np.ones((1, 4096))), one, _i32(np.ones((1, 10))), one, want_prefix=True)
    with pytest.raises(err):
        ops.edit_distance(_i32(np.ones((1, 10))), one, _i32(np.ones((1, 4096))), one, want_prefix=False)
    # with prefix distances only the reference lies across the lanes: any hypothesis stride is accepted
    rng = np.random.default_rng(4096)
    R, Hy = 10, 4096
    pairs = [(rng.integers(1, 4, size=R), rng.integers(1, 4, size=Hy)), (rng.integers(1, 4, size=7), rng.integers(1, 4, size=4095))]
    _ed_run(*_pack(pairs, R, Hy), True)


# ------------------------------------------------------------------------------------------------------------------------
# collapse and arg-max
# ------------------------------------------------------------------------------------------------------------------------
COLLAPSE_T = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]
COLLAPSE_V = 6


def _runs(T, rng, V=COLLAPSE_V, p_new=0.2):
    """random labels held over long runs"""
    lab = rng.integers(0, V, size=T)
    idx = np.where(rng.random(T) < p_new, np.arange(T), 0)
    return lab[np.maximum.accumulate(idx)]


def _collapse_patterns(T, blank, rng):
    nb = np.array([v for v in range(COLLAPSE_V) if v != blank])
    pats = [np.full(T, blank), nb[np.arange(T) % len(nb)], np.full(T, nb[2])]      # all blank; count T; count 1
    for seam in (256, 512):
        if T > seam:
            run = _runs(T, rng)
            run[seam - 5:seam + 5] = blank
            run[seam - 3:seam + 2] = nb[1]                     # one run over frames seam - 1 and seam: one token
            sep = _runs(T, rng)
            sep[seam - 5:seam + 5] = blank
            sep[seam - 2], sep[seam] = nb[3], nb[3]            # label, blank on seam - 1, the same label on the seam: two tokens
            pats += [run, sep]
    pats.append(_runs(T, rng))
    while len(pats) % 3:
        pats.append(_runs(T, rng, p_new=0.5))
    return pats


def _collapse_lengths(T):
    vecs = [[T, 1, 0, T + 5]]
    if T > 512:
        vecs += [[-3, 511, 512, 513], [255, 256, 257, T - 1]]
    elif T > 256:
        vecs += [[-3, 255, 256, 257]]
    else:
        vecs += [[-3, T - 1, T, min(T, 64)]]
    return vecs


@pytest.mark.parametrize("blank", [0, 3, COLLAPSE_V - 1])
@pytest.mark.parametrize("T", COLLAPSE_T)
def test_collapse_at_the_round_seams(T, blank):
    """P = 3 path sets x B = 4 utterances; every pattern under every length; the outputs pre-filled with -7, which must survive
    beyond every count (the whole tensors are compared, so a write into a neighbouring row shows as well)"""
    ops = _ops()
    P, B = 3, 4
    rng = np.random.default_rng(10 * T + blank)
    pats = _collapse_patterns(T, blank, rng)
    for lengths in _collapse_lengths(T):
        for c in range(0, len(pats), P):
            paths = np.stack([np.repeat(pats[c + p][:, None], B, axis=1) for p in range(P)]).astype(np.int32)      # (P,T,B)
            tok = torch.full((P, B, T), -7, dtype=torch.int32, device=DEV)
            tl = torch.full((P, B), -7, dtype=torch.int32, device=DEV)
            got = ops.ctc_collapse(_i32(paths), _i32(lengths), blank=blank, out=(tok, tl))
            assert got[0] is tok and got[1] is tl
            want_tok, want_tl = np.full((P, B, T), -7, np.int32), np.zeros((P, B), np.int32)
            for p in range(P):
                for b in range(B):
                    seq = decode_ref.collapse_path(paths[p, :min(max(lengths[b], 0), T), b], blank)
                    want_tok[p, b, :len(seq)], want_tl[p, b] = seq, len(seq)
            assert np.array_equal(tl.cpu().numpy(), want_tl), (lengths, c, tl.cpu().numpy(), want_tl)
            assert np.array_equal(tok.cpu().numpy(), want_tok), (lengths, c)
            if c == 0 and lengths[0] == T:
                assert want_tl[:, 0].tolist() == [0, T, 1]       # the row filled to its last word, and the two extremes


def test_collapse_seam_counts():
    """the two seam constructions give the counts they were built for (the oracle is applied to what was meant)"""
    rng = np.random.default_rng(3)
    pats = _collapse_patterns(513, 0, rng)
    for seam, (run, sep) in ((256, pats[3:5]), (512, pats[5:7])):
        assert decode_ref.collapse_path(run[seam - 5:seam + 5], 0) == [2]
        assert decode_ref.collapse_path(sep[seam - 5:seam + 5], 0) == [4, 4]
        assert run[seam - 1] == run[seam] == 2 and sep[seam - 1] == 0


def test_argmax_ties_take_the_first():
    """V = 64: exact ties across the halves and quarters of the wave's reduction, signed zeros, rows of -inf"""
    ops = _ops()
    T, B, V = 5, 4, 64
    rng = np.random.default_rng(64)
    x = (-1.0 - rng.random((T * B, V))).astype(np.float32)      # everything else below -1
    ties = [(0, 63), (31, 32), (32, 33), (63, 0), (33, 32), (1, 2, 62), (15, 16, 47, 48)]
    for r, labs in enumerate(ties):
        x[r, list(labs)] = 0.5
    x[7, 40], x[7, 9] = -0.0, 0.0                               # -0.0 == +0.0: label 9 is the first
    x[8, 9], x[8, 40] = -0.0, 0.0
    x[9, :] = -np.inf
    x[10, :] = -np.inf; x[10, V - 1] = -3.0
    x[11, :] = -np.inf; x[11, 0] = -np.inf; x[11, 32] = -7.0; x[11, 33] = -7.0
    x[12, :] = 2.0                                              # every label tied
    want = np.argmax(x, axis=1)
    assert want[:5].tolist() == [0, 31, 32, 0, 32] and want[7] == 9 and want[8] == 9 and want[9] == 0 and want[10] == V - 1
    g, s = ops.frame_argmax_sample(torch.from_numpy(x.reshape(T, B, V)).to(DEV), want_sample=False)
    assert s is None
    assert np.array_equal(g.cpu().numpy().reshape(-1), want), (g.cpu().numpy().reshape(-1), want)


# ------------------------------------------------------------------------------------------------------------------------
# per-step coefficients
# ------------------------------------------------------------------------------------------------------------------------
COEF_T = [1, 63, 64, 65, 128, 129, 200]
COEF_V = 5
LAM = 0.7


def _planted_path(T, Tb, extra, rng):
    """frame labels (T), built by hand: characters start at frames 0, 63, 64, 65 and Tb - 1 (the last valid frame) and at ``extra``
    random frames; a character is held up to the next start or for one frame; consecutive characters differ, so every planted
    frame is a start.  The frames from Tb on carry characters too: they must not count."""
    starts = sorted({s for s in [0, 63, 64, 65, Tb - 1] + rng.integers(0, T, size=extra).tolist() if 0 <= s < T})
    path = np.zeros(T, np.int32)
    for i, s in enumerate(starts):
        end = starts[i + 1] if i + 1 < len(starts) else T
        path[s:(end if rng.random() < 0.5 else s + 1)] = 1 + i % (COEF_V - 1)
    assert D.char_starts(path)[starts].all() and int(D.char_starts(path).sum()) == len(starts)
    return path


@functools.lru_cache(maxsize=None)
def _coef_case(T, in_len, tg_len):
    """hand-built inputs of B = 4 utterances; the greedy set gets 3 extra character starts, the sampled set 9: a carry lost
    between two 64-frame rounds changes G_sample - G_greedy.  prefix (2B, T + 1): D.ed_prefix on the collapsed paths, poisoned
    beyond each row's length."""
    B = len(in_len)
    rng = np.random.default_rng(T)
    paths = np.zeros((2, T, B), np.int32)
    targets = [rng.integers(1, COEF_V, size=n) for n in tg_len]
    tok_len = np.zeros(2 * B, np.int32)
    prefix = np.full((2 * B, T + 1), 10 ** 6, np.int32)
    for w in range(2):
        for b in range(B):
            Tb = min(max(in_len[b], 0), T)
            paths[w, :, b] = _planted_path(T, Tb, 3 + 6 * w, rng)
            hyp = decode_ref.collapse_path(paths[w, :Tb, b], 0)
            tok_len[w * B + b] = len(hyp)
            prefix[w * B + b, :len(hyp) + 1] = D.ed_prefix(targets[b], hyp)
    return paths, np.array(in_len, np.int32), prefix, tok_len, np.array(tg_len, np.int32)


def _coef_check(paths, in_len, prefix, tok_len, tg_len, frame0=True):
    ops = _ops()
    _, T, B = paths.shape
    inv_bg = 1.0 / B
    got = ops.pg_step_coefs(_i32(paths), _i32(in_len), _i32(prefix), _i32(tok_len), _i32(tg_len), LAM, inv_bg).cpu().numpy()
    want = D.step_coefs(paths, in_len, prefix, tok_len, tg_len, LAM, inv_bg)
    print("max |coef|", np.abs(want).max(), "max |diff|", np.abs(got - want).max())
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-9)
    for b in range(B):
        assert (got[min(max(int(in_len[b]), 0), T):, b] == 0).all()
    if frame0:
        dist = prefix[np.arange(2 * B), np.clip(tok_len, 0, prefix.shape[1] - 1)]
        _, _, coef_utt, _ = ops.pg_rewards(_i32(dist), _i32(tg_len), LAM, inv_bg)
        np.testing.assert_allclose(got[0], coef_utt.cpu().numpy(), rtol=1e-6, atol=1e-9)    # no frame: both paths empty, both 0
    return got


# The target lengths are powers of two (and one empty target, divisor 1): -ED / L is then exact in fp32, so frame 0 and
# pg_rewards' utterance coefficient, which round at different places, agree to the last bit of the one rounding either has left;
# with another L the two quotients of pg_rewards would cancel in R_s - R_g and leave more than 1e-6 of their difference.
@pytest.mark.parametrize("T", COEF_T)
def test_step_coefs_planted_starts(T):
    for in_len, tg_len in (((T, T + 7, 0, -2), (8, 0, 4, 16)), ((64, T, max(T - 1, 1), min(T, 65)), (4, 2, 0, 8))):
        case = _coef_case(T, in_len, tg_len)
        got = _coef_check(*case)
        if T >= 63:
            assert np.abs(got).sum() > 0


def test_step_coefs_carry_matters():
    """the planted case is one in which the carried count decides: without it the oracle gives other coefficients"""
    paths, in_len, prefix, tok_len, tg_len = _coef_case(129, (129, 136, 0, -2), (8, 0, 4, 16))
    want = D.step_coefs(paths, in_len, prefix, tok_len, tg_len, LAM, 0.25)
    for t0 in (64, 128):
        st = [int(D.char_starts(paths[w, :t0, 0]).sum()) for w in range(2)]
        assert st[0] != st[1] and min(st) > 0
    assert np.abs(want[64:, 0]).sum() > 0 and np.abs(want[128:, 0]).sum() > 0


def test_step_coefs_prefix_stride_clamps():
    T = 129
    paths, in_len, prefix, tok_len, tg_len = _coef_case(T, (T, T + 7, 0, -2), (8, 0, 4, 16))
    full = _coef_check(paths, in_len, prefix, tok_len, tg_len)
    # the tightest table: the clamp is active on the longest row and changes nothing
    P = int(tok_len.max()) + 1
    tight = _coef_check(paths, in_len, np.ascontiguousarray(prefix[:, :P]), tok_len, tg_len)
    assert np.array_equal(tight, full)
    # a length reported beyond the table: the result of the clamped one
    P = int(tok_len.max()) - 3
    cut = np.ascontiguousarray(prefix[:, :P])
    assert (tok_len > P - 1).any() and (tok_len[tok_len > 0] < P - 1).any()
    over = _coef_check(paths, in_len, cut, tok_len, tg_len, frame0=False)
    clamped = _coef_check(paths, in_len, cut, np.minimum(tok_len, P - 1), tg_len, frame0=False)
    assert np.array_equal(over, clamped) and not np.array_equal(over, full)
    # and a negative one acts as 0
    neg = tok_len.copy(); neg[0] = -4
    zero = tok_len.copy(); zero[0] = 0
    assert np.array_equal(_coef_check(paths, in_len, prefix, neg, tg_len, frame0=False),
                          _coef_check(paths, in_len, prefix, zero, tg_len, frame0=False))


# ------------------------------------------------------------------------------------------------------------------------
# forced alignment at tight fits
# ------------------------------------------------------------------------------------------------------------------------
def _align_check(lp, tokens, il, tl, blank=0):
    """every field against align_ref.align_batch bit for bit, padding included (test_align_gpu._assert_equal restated); for every
    utterance that has an alignment: its frame labels collapse to the transcript, its spans are ascending and disjoint.
    Returns the reference."""
    a = _ops().ctc_forced_align(lp.to(DEV).contiguous(), _i32(tokens), _i32(il), _i32(tl), blank=blank)
    r = align_ref.align_batch(lp.numpy(), tokens, il, tl, blank=blank)
    score, fl, ft = a.score.cpu().numpy(), a.frame_label.cpu().numpy(), a.frame_token.cpu().numpy()
    st, en, tlp = a.token_start.cpu().numpy(), a.token_end.cpu().numpy(), a.token_logp.cpu().numpy()
    assert a.score.dtype == torch.float64 and a.token_logp.dtype == torch.float64 and a.frame_label.dtype == torch.int32
    assert np.array_equal(score, r.score), (score, r.score)
    for name, x, y in (("frame_label", fl, r.frame_label), ("frame_token", ft, r.frame_token), ("token_start", st, r.token_start),
                       ("token_end", en, r.token_end), ("token_logp", tlp, r.token_logp)):
        assert np.array_equal(x, y), (name, np.argwhere(x != y)[:6])
    T, Lmax = lp.shape[0], np.asarray(tokens).shape[1]
    for b in range(len(il)):
        Tb, Lb = min(max(int(il[b]), 0), T), min(max(int(tl[b]), 0), Lmax)
        if not np.isfinite(score[b]) or Tb == 0:
            assert (fl[b] == -1).all() and (ft[b] == -1).all() and (st[b] == -1).all() and (en[b] == -1).all()
            continue
        assert decode_ref.collapse_path(fl[b, :Tb], blank) == [int(t) for t in np.asarray(tokens)[b, :Lb]]
        if Lb:
            s, e = st[b, :Lb], en[b, :Lb]
            assert (s >= 0).all() and (e > s).all() and (s[1:] >= e[:-1]).all() and e[-1] <= Tb
            assert int((e - s).sum()) == int((ft[b] >= 0).sum())
    return r


def _distinct_tokens(B, L, V):
    return np.tile(np.arange(L) % (V - 1) + 1, (B, 1))          # neighbours always differ


def _lp(T, B, V, seed):
    return torch.log_softmax(torch.randn(T, B, V, generator=torch.Generator().manual_seed(seed)), 2)


ALIGN_L = [33, 64, 65, 66, 67, 127, 128, 255, 256, 511, 512, 1023]


@pytest.mark.parametrize("V", [5, 29])
@pytest.mark.parametrize("L", ALIGN_L)
def test_align_exact_fit(L, V):
    """T = L: two states down in every frame, so every 32-frame backtrace block uses its whole 68-byte window; the second
    utterance (L - 1 tokens in T - 1 frames) ends one state pair lower, so the end states 2L, 2L - 1, 2L - 2, 2L - 3 over the L
    of this list take all four byte positions of a word.  Then one and two spare frames: the scores decide where the stay goes.
    L = 1023 is the token limit."""
    for spare in (0, 1, 2):
        T = L + spare
        r = _align_check(_lp(T, 2, V, 1000 * spare + L + V), _distinct_tokens(2, L, V), [T, T - 1], [L, L - 1])
        assert np.isfinite(r.score).all()
        if spare == 0:
            assert (r.frame_token[0] == np.arange(L)).all() and (r.frame_token[1, :L - 1] == np.arange(L - 1)).all()


def test_align_end_states_cover_a_word():
    """the claim of test_align_exact_fit's docstring: the walk starts in every byte position of a word"""
    ends = {(2 * (L - b) - 1) % 4 for L in ALIGN_L for b in (0, 1)} | {(2 * (L - b)) % 4 for L in ALIGN_L for b in (0, 1)}
    assert ends == {0, 1, 2, 3}


@pytest.mark.parametrize("L", [17, 64, 300])
def test_align_repeated_label(L):
    """all tokens equal: only single steps, label and blank alternating, T = 2L - 1 the exact fit; one frame fewer has no alignment"""
    T, V = 2 * L - 1, 5
    tokens = np.full((2, L), 3)
    r = _align_check(_lp(T, 2, V, L), tokens, [T, T - 1], [L, L])
    assert np.isfinite(r.score[0]) and r.score[1] == np.inf and (r.frame_label[1] == -1).all()
    assert r.frame_label[0].tolist() == ([3, 0] * L)[:T]


@pytest.mark.parametrize("T", [96, 97, 128, 129, 161])
def test_align_early_and_late_descent(T):
    """L = 65 with 20 nats added to the blank column on the first T - L frames (utterance 0: the descent is steep and late, at the
    top of the lattice) or on the last T - L frames (utterance 1: steep and early, at the bottom)"""
    L, V = 65, 5
    lp = _lp(T, 2, V, T).clone()
    lp[:T - L, 0, 0] += 20.0
    lp[L:, 1, 0] += 20.0
    r = _align_check(lp, _distinct_tokens(2, L, V), [T, T], [L, L])
    assert np.isfinite(r.score).all()
    # the spare frames are spent on blanks inside the favoured stretch (20 nats each); where the first or last token goes is
    # the scores' choice, so only the steepness is asserted: the other L - 2 tokens and their blanks fit into L + 8 frames
    for b in (0, 1):
        print("utterance", b, "tokens 1 ..", L - 2, "in frames", r.token_start[b, 1], "..", r.token_end[b, L - 2])
        assert r.token_end[b, L - 2] - r.token_start[b, 1] <= L + 8


@pytest.mark.parametrize("V", [5, 29])
@pytest.mark.parametrize("T", [31, 32, 33, 63, 64, 65])
def test_align_backtrace_block_boundaries(T, V):
    L = 12
    tokens = _distinct_tokens(3, L, V)
    r = _align_check(_lp(T, 3, V, T + V), tokens, [T, T - 1, T - 2], [L, L - 1, L])
    assert np.isfinite(r.score).all()


@pytest.mark.parametrize("spare", [1, 31])
def test_align_uniform_rows_tight(spare):
    """uniform rows: every comparison is a tie and the smallest move wins each, at a tight fit"""
    L, V = 64, 5
    T = L + spare
    lp = torch.full((T, 2, V), float(-np.log(np.float32(V))), dtype=torch.float32)
    r = _align_check(lp, _distinct_tokens(2, L, V), [T, T - 1], [L, L - 1])
    assert np.isfinite(r.score).all()


def test_align_token_limit():
    ops = _ops()
    assert ops.ALIGN_MAX_TOKENS == 1023 == max(ALIGN_L)         # accepted: test_align_exact_fit[1023]
    T, V = 8, 5
    with pytest.raises(_err()):
        ops.ctc_forced_align(_lp(T, 1, V, 0).to(DEV), _i32(_distinct_tokens(1, 1024, V)), _i32([T]), _i32([4]))
