"""Spelling subword units into characters on the GPU (csrc/unit_spell.hip; include/pgasr_hip.h, A11-SPELL) and the layers above it,
against tests/unit_spell_ref.py -- the strings joined, split with str.split(" ") and compared by the plain DP.  Integer results are
compared with ==.  The objectives are held to the fp64 oracle (oracle/pg_ref.py's terms through unit_spell_ref.objective, which
differs from pg_ref.pg_objective in the reward alone; tests/mwer_ref.py for MWER) on the DEVICE's discrete choices, with the bounds of
the wide tests: rewards rtol 1e-6, loss 1e-5, d(logits) 1e-4 (max norm) for the sampled objectives (tests/test_wide_pg_gpu.py,
tests/test_wide_seq_gpu.py), loss and d(logits) 1e-5 for MWER (tests/test_wide_seq_gpu.py)."""
import functools

import numpy as np
import pytest
import torch

import mbr_ref
import mwer_ref as MR
import unit_spell_ref as R
from oracle import decode_ref
from pg_harness import DEV, lattice_case, make_batch, oracle_model, rel_err, shards_vs_whole

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from policy_gradient_asr_amd import hipops
    return hipops


def dv(a, dtype=np.int32):
    return torch.tensor(np.asarray(a, dtype=dtype)).to(DEV)


def _spelling(units, alphabet):
    from policy_gradient_asr_amd.units import SubwordUnits, UnitSpelling
    return UnitSpelling(SubwordUnits(units), alphabet)


# ---- 1. the kernel ----
KERNEL_ALPHABET = [" "] + [chr(c) for c in range(ord("a"), ord("z") + 1)] + [chr(c) for c in range(ord("A"), ord("Z") + 1)] + list("0123456")
ROW_LENGTHS = [0, 1, 63, 64, 65, 128, 129, 200, 300, -3]          # the chunk seams, one above the stride, one negative
STRIDE = 200


@functools.lru_cache(maxsize=None)
def kernel_units(V):
    """V - 1 distinct units with spellings of 1, 2 and 7 characters in turn (the index in base 59, padded with spaces: interior
    and leading spaces everywhere) and, from four units on, one of the cap, 64 characters."""
    digits = KERNEL_ALPHABET[1:]
    units = []
    for i in range(V - 1):
        n = (1, 2, 7)[i % 3]
        s = digits[i % 59] if i < 59 else digits[i // 59] + digits[i % 59]
        units.append(s if len(s) >= n else s[:-1] + " " * (n - len(s)) + s[-1])
    if V >= 5:
        units[-1] = ("cap " * 16)[:64]
    assert len(set(units)) == len(units)
    return units


@functools.lru_cache(maxsize=None)
def kernel_case(V):
    """tokens (10, 200) over [0, V) with ids 0, -1, V and V + 5 inside the rows, the lengths of ROW_LENGTHS; rows 2 and 6 hold the
    cap unit several times, so that chunk spans cross multiples of 64 characters by every residue."""
    rng = np.random.RandomState(V)
    tokens = rng.randint(1, V, size=(len(ROW_LENGTHS), STRIDE)).astype(np.int32)
    for n in range(tokens.shape[0]):
        for j, bad in enumerate((0, -1, V, V + 5)):
            tokens[n, (7 + 13 * n + 29 * j) % STRIDE] = bad
            tokens[n, (3 + 31 * j) % 60] = bad
    if V >= 5:
        tokens[2, 5:60:9] = V - 1
        tokens[6, ::17] = V - 1
    return tokens, np.array(ROW_LENGTHS, dtype=np.int32)


def _launch(V, tokens, lengths, out_stride, want_full=True, misalign=0):
    """pgasr_unit_spell itself on a buffer prefilled with -1, with 64 guard words behind the rows: (out, out_len, full_len, guard)."""
    from policy_gradient_asr_amd import _lib
    sp = _spelling(kernel_units(V), KERNEL_ALPHABET)
    off, pool = sp.to(DEV)
    N, stride = tokens.shape
    tk, ln = dv(tokens), dv(lengths)
    buf = torch.full((misalign + N * out_stride + 64,), -1, dtype=torch.int32, device=DEV)
    lens = torch.full((2, N), -7, dtype=torch.int32, device=DEV)
    st = _lib.load().pgasr_unit_spell(tk.data_ptr(), ln.data_ptr(), stride, N, off.data_ptr(), pool.data_ptr(), V,
                                      buf.data_ptr() + 4 * misalign, out_stride, lens[0].data_ptr(),
                                      lens[1].data_ptr() if want_full else 0, torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    return (b[misalign:misalign + N * out_stride].reshape(N, out_stride), lens[0].cpu().numpy(), lens[1].cpu().numpy(),
            np.concatenate((b[:misalign], b[misalign + N * out_stride:])))


@pytest.mark.parametrize("V", [2, 65, 1024])
def test_kernel_rows_lengths_and_zero_tail(V):
    """Whole rows ==, lengths ==, the tail zero on a buffer prefilled with -1, nothing written outside the rows: N around the four
    rows of a workgroup, out_stride at the longest row, one short of it, inside a unit, 1 and 0, full_len given and NULL, and an
    output address that is not 16-byte aligned."""
    tokens, lengths = kernel_case(V)
    units = kernel_units(V)
    _, _, full = R.spell_rows(units, KERNEL_ALPHABET, tokens, lengths, 0)
    longest = int(full.max())
    assert full[0] == 0 and full[-1] == 0 and longest > 64 and (V < 5 or longest > 3 * 64)
    strides = [longest, longest - 1, longest // 2 + 3, 1, 0]
    for N in (1, 3, 4, 5, len(ROW_LENGTHS)):
        rows = slice(len(ROW_LENGTHS) - N, None) if N < 5 else slice(0, N)          # the short N take the long rows too
        tk, ln = tokens[rows], lengths[rows]
        for out_stride in strides if N in (5, len(ROW_LENGTHS)) else strides[:2]:
            want, want_len, want_full = R.spell_rows(units, KERNEL_ALPHABET, tk, ln, out_stride)
            for given, mis in ((True, 0), (False, 0), (True, 1)):
                out, out_len, full_len, guard = _launch(V, tk, ln, out_stride, want_full=given, misalign=mis)
                assert np.array_equal(out, want), (V, N, out_stride, given, mis)
                assert np.array_equal(out_len, want_len) and (guard == -1).all()
                assert np.array_equal(full_len, want_full if given else np.full(N, -7))
    # stride 0: nothing is read, every row is empty and zero
    out, out_len, full_len, guard = _launch(V, tokens[:3, :0], lengths[:3], 5)
    assert not out.any() and not out_len.any() and not full_len.any() and (guard == -1).all()


def test_wrapper_shapes_and_default_stride(ops):
    V = 65
    sp = _spelling(kernel_units(V), KERNEL_ALPHABET)
    tokens, lengths = kernel_case(V)
    tk, ln = dv(tokens[:8].reshape(2, 4, STRIDE)), dv(lengths[:8].reshape(2, 4))
    out, out_len, full_len = ops.unit_spell(tk, ln, sp, want_full=True)
    assert out.shape == (2, 4, min(STRIDE * 64, ops.WORD_MAX_STRIDE)) and out_len.shape == full_len.shape == (2, 4)
    want, want_len, want_full = R.spell_rows(kernel_units(V), KERNEL_ALPHABET, tokens[:8], lengths[:8], out.shape[2])
    assert np.array_equal(out.cpu().numpy().reshape(8, -1), want) and np.array_equal(out_len.cpu().numpy().reshape(8), want_len)
    assert np.array_equal(full_len.cpu().numpy().reshape(8), want_full)
    out2, len2 = ops.unit_spell(tk[0], ln[0], sp, out_stride=50)
    assert np.array_equal(out2.cpu().numpy(), want[:4, :50]) and np.array_equal(len2.cpu().numpy(), np.minimum(want_full[:4], 50))
    from policy_gradient_asr_amd import _lib
    with pytest.raises(_lib.PgasrError):
        ops.unit_spell(tk, ln[0], sp)


# ---- 2. the compositions ----
def _pad(rows, width=None):
    width = max(width or 0, max((len(r) for r in rows), default=0), 1)
    out = np.zeros((len(rows), width), dtype=np.int32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out, np.array([len(r) for r in rows], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def units300():
    return R.random_units(300, 1)


def _random_rows(rng, n, V, lo, hi):
    return [[int(x) for x in rng.randint(1, V, size=rng.randint(lo, hi + 1))] for _ in range(n)]


def test_spelled_edit_distance_counts_and_truncation(ops):
    """Both units on the fixed cases (every pair of them) and on random rows over 300 units: distances, the reference's character
    and word counts, truncated == 0; then a reference of 70 cap units (4480 characters) against the row limit of 4094: the distance
    is the cut row's, and truncated counts it once."""
    sp = _spelling(R.UNITS, R.ALPHABET)
    pairs = [(ref, hyp) for ref, a, b in R.CASES.values() for hyp in (a, b)]
    pairs += [(a, b) for _, a, b in R.CASES.values()]
    ref, rl = _pad([p[0] for p in pairs]); hyp, hl = _pad([p[1] for p in pairs])
    want = [R.distances(R.UNITS, r, h) for r, h in pairs]
    for unit, col, cnt in (("char", 1, 3), ("word", 2, 4)):
        d, c, tr = ops.spelled_edit_distance(dv(ref), dv(rl), dv(hyp), dv(hl), sp, unit=unit)
        assert d.cpu().tolist() == [w[col] for w in want] and c.cpu().tolist() == [w[cnt] for w in want] and int(tr) == 0
    units, alphabet = units300()
    sp = _spelling(units, alphabet)
    rng = np.random.RandomState(5)
    refs = _random_rows(rng, 9, 300, 0, 30)
    hyps = [list(r) for r in refs]
    for h in hyps[:6]:                                       # near the reference: a few units replaced, dropped, inserted
        for _ in range(3):
            k = rng.randint(0, len(h) + 1)
            h[k:k + rng.randint(0, 2)] = [int(rng.randint(1, 300))]
    ref, rl = _pad(refs); hyp, hl = _pad(hyps)
    want = [R.distances(units, r, h) for r, h in zip(refs, hyps)]
    assert len({(w[0], w[1], w[2]) for w in want}) > 3 and any(w[0] != w[1] for w in want)
    for unit, col, cnt in (("char", 1, 3), ("word", 2, 4)):
        d, c, tr = ops.spelled_edit_distance(dv(ref), dv(rl), dv(hyp), dv(hl), sp, unit=unit)
        assert d.cpu().tolist() == [w[col] for w in want] and c.cpu().tolist() == [w[cnt] for w in want] and int(tr) == 0
    # the row limit
    V = 65
    ku = kernel_units(V)
    sp = _spelling(ku, KERNEL_ALPHABET)
    ref, rl = _pad([[V - 1] * 70, [1, 2]]); hyp, hl = _pad([[V - 1, 3, 4], [1, 2]], 70)
    cut = R.text(ku, [V - 1] * 70)[:ops.WORD_MAX_STRIDE]
    assert len(R.text(ku, [V - 1] * 70)) == 4480
    d, c, tr = ops.spelled_edit_distance(dv(ref), dv(rl), dv(hyp), dv(hl), sp, unit="char")
    assert d.cpu().tolist() == [R.levenshtein(cut, R.text(ku, [V - 1, 3, 4])), 0] and c.cpu().tolist() == [4094, len(R.text(ku, [1, 2]))]
    assert int(tr) == 1 and tr.dtype == torch.int32 and tr.is_cuda
    d, c, tr = ops.spelled_edit_distance(dv(ref), dv(rl), dv(hyp), dv(hl), sp, unit="word")
    assert d.cpu().tolist() == [R.levenshtein(cut.split(" "), R.text(ku, [V - 1, 3, 4]).split(" ")), 0] and int(tr) == 1
    assert c.cpu().tolist()[0] == len(cut.split(" "))


def _list_case(N, B, seed, lo=0, hi=12, near=True):
    """An N-best list over 300 units: rows near one base row per utterance (so that the distances differ and are small), count
    below N for one utterance, garbage behind every length."""
    rng = np.random.RandomState(seed)
    stride = hi + 3
    tokens = rng.randint(1, 300, size=(N, B, stride)).astype(np.int32)
    lengths = np.zeros((N, B), dtype=np.int32)
    for b in range(B):
        base = _random_rows(rng, 1, 300, max(lo, hi - 4), hi)[0]
        for n in range(N):
            row = list(base) if near else _random_rows(rng, 1, 300, lo, hi)[0]
            for _ in range(rng.randint(0, 4) if near else 0):
                if row:
                    row[rng.randint(0, len(row))] = int(rng.randint(1, 300))
            if near and n % 5 == 4 and row:
                row.pop(rng.randint(0, len(row)))
            tokens[n, b, :len(row)] = row
            lengths[n, b] = len(row)
    count = np.array([N if b else max(N - 1, 1) for b in range(B)], dtype=np.int32)
    return tokens, lengths, count


def _pair_ref(units, tokens, lengths, count, col):
    N, B = lengths.shape
    dist = np.full((B, N, N), -1, dtype=np.int32)
    for b in range(B):
        for n in range(int(count[b])):
            for m in range(n, int(count[b])):
                d = 0 if n == m else R.distances(units, tokens[n, b, :lengths[n, b]], tokens[m, b, :lengths[m, b]])[col]
                dist[b, n, m] = dist[b, m, n] = d
    return dist


@pytest.mark.parametrize("N", [2, 5, 16])
def test_pair_distances_over_the_spelled_list(ops, N):
    """nbest_pair_distance_spelled over 300 units against the plain DP on the strings, both units; without a spelling the word form
    keeps its refusal, word for word."""
    units, alphabet = units300()
    sp = _spelling(units, alphabet)
    tokens, lengths, count = _list_case(N, 2, 40 + N)
    tk, ln, ct = dv(tokens), dv(lengths), dv(count)
    for unit, col in (("char", 1), ("word", 2)):
        got = ops.nbest_pair_distance_spelled(tk, ln, ct, sp, unit=unit).cpu().numpy()
        want = _pair_ref(units, tokens, lengths, count, col)
        assert np.array_equal(got, want), (N, unit)
        assert want.max() > 0
    with pytest.raises(ValueError) as e:
        ops.nbest_pair_distance(tk, ln, ct, 300, unit="word", delimiter=5)
    assert str(e.value) == ("unit='word': not over 300 > 64 symbols -- a subword unit may span a space, so words cannot be split at a "
                            "delimiter token; take unit='char' (the units are the symbols)")


def test_pair_distances_of_long_rows_take_the_composed_path(ops):
    """Two hypotheses of about 110 units (more than 640 characters, few pairs): the existing length rule sends the spelled list to the
    wave-per-pair kernels; the same distances."""
    units, alphabet = units300()
    sp = _spelling(units, alphabet)
    tokens, lengths, count = _list_case(2, 2, 7, lo=150, hi=160)
    count[:] = 2
    assert min(len(R.text(units, tokens[n, b, :lengths[n, b]])) for n in range(2) for b in range(2)) >= ops.PAIR_DIST_COMPOSED_MIN_LEN
    got = ops.nbest_pair_distance_spelled(dv(tokens), dv(lengths), dv(count), sp, unit="char").cpu().numpy()
    assert np.array_equal(got, _pair_ref(units, tokens, lengths, count, 1))


def test_oracle_counts_and_mbr_over_the_spelled_list(ops):
    """metrics.nbest_oracle(spelling=) and metrics.unit_error_counts against the DP; CTCDecoder.mbr_from_list(risk_unit="word",
    unit_spelling=): the matrix is the reference's and so is the choice (tests/mbr_ref.select_ref); without a spelling it raises."""
    from policy_gradient_asr_amd import metrics
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    units, alphabet = units300()
    sp = _spelling(units, alphabet)
    N, B = 5, 3
    tokens, lengths, count = _list_case(N, B, 91)
    rng = np.random.RandomState(3)
    targets, tg_len = _pad([list(tokens[1, b, :lengths[1, b]]) + [int(rng.randint(1, 300))] for b in range(B)])
    nb = ops.CTCNBest(dv(tokens), dv(lengths), dv(rng.rand(N, B), np.float64), dv(count))
    for unit, col, cnt in (("char", 1, 3), ("word", 2, 4)):
        best, rank, ref_count = metrics.nbest_oracle(dv(targets), dv(tg_len), nb, spelling=sp, unit=unit)
        d = np.array([[R.distances(units, targets[b, :tg_len[b]], tokens[n, b, :lengths[n, b]])[col] if n < count[b] else 1 << 30
                       for b in range(B)] for n in range(N)])
        assert best.cpu().tolist() == d.min(0).tolist() and rank.cpu().tolist() == d.argmin(0).tolist()
        assert ref_count.cpu().tolist() == [R.distances(units, targets[b, :tg_len[b]], [])[cnt] for b in range(B)]
    plain = metrics.nbest_oracle(dv(targets), dv(tg_len), nb)                  # without a spelling: units, two values, as ever
    assert len(plain) == 2 and plain[0].cpu().tolist() == [1] * B
    cd, cl, wd, wc = metrics.unit_error_counts(dv(targets), dv(tg_len), dv(tokens[0]), dv(lengths[0]), sp)
    want = [R.distances(units, targets[b, :tg_len[b]], tokens[0, b, :lengths[0, b]]) for b in range(B)]
    assert [cd.cpu().tolist(), cl.cpu().tolist(), wd.cpu().tolist(), wc.cpu().tolist()] == [[w[i] for w in want] for i in (1, 3, 2, 4)]
    score = np.sort(rng.rand(N, B) * 3.0, axis=0)
    dec = CTCDecoder(["<pad>"] + units)
    md = dec.mbr_from_list(nb, dv(score, np.float64), vocab=300, risk_unit="word", unit_spelling=sp)
    want_dist = _pair_ref(units, tokens, lengths, count, 2)
    want_best, want_risk, _ = mbr_ref.select_ref(want_dist, score, count, 1.0)
    assert np.array_equal(md.dist.cpu().numpy(), want_dist)
    assert md.best.cpu().tolist() == want_best.tolist() and all(mbr_ref.best_within_margin(md.best.cpu().numpy(), want_risk))
    for b in range(B):
        k = int(want_best[b])
        assert md.tokens[b, :int(md.lengths[b])].cpu().tolist() == tokens[k, b, :lengths[k, b]].tolist()      # the unit row is returned
    with pytest.raises(ValueError, match="a subword unit may span a space"):
        dec.mbr_from_list(nb, dv(score, np.float64), vocab=300, risk_unit="word", word_delimiter=5)
    # the error report over spelled strings
    rep = metrics.ErrorReport(sp.char_alphabet, " ", device=DEV)
    refs = [R.text(units, targets[b, :tg_len[b]]) for b in range(B)]
    hyps = [R.text(units, tokens[0, b, :lengths[0, b]]) for b in range(B)]
    rep.add(refs, hyps)
    s = rep.summary(top_k=0)
    assert s["char"]["sub"] + s["char"]["del"] + s["char"]["ins"] == sum(w[1] for w in want)
    assert s["word"]["sub"] + s["word"]["del"] + s["word"]["ins"] == sum(w[2] for w in want) and s["word"]["ref"] == sum(w[4] for w in want)


# ---- 3. the sampled objectives ----
OBJ = dict(T=24, B=3, L=6, in_len=[24, 17, 24], tg_len=[6, 4, 5])
OBJ_VARIANTS = {"K1-hypothesis": (dict(), dict()),
                "K4-leave-one-out-entropy": (dict(num_samples=4, baseline="leave_one_out", entropy_weight=0.1), dict(wide_objectives=True)),
                "K2-sequence": (dict(num_samples=2, score_function="sequence", max_hyp_len=12),
                                dict(wide_objectives=True, wide_sequence=True))}
SPACED = [" "] + list("abcdefgh")            # a small alphabet: one character in nine is a space, most rows hold several words


@functools.lru_cache(maxsize=None)
def _objective_case(V):
    g = torch.Generator().manual_seed(100 + V)
    logits = torch.randn(OBJ["T"], OBJ["B"], V, generator=g) * 2
    targets = torch.randint(1, V, (OBJ["B"], OBJ["L"]), generator=g, dtype=torch.int32)
    units, alphabet = R.random_units(V, V, alphabet=SPACED)
    return logits, targets, np.array(OBJ["in_len"]), np.array(OBJ["tg_len"]), units, alphabet


def _objective_vs_oracle(ops, V, name, unit, wide):
    from policy_gradient_asr_amd.loss import PGCTCLossFn, pg_ctc_loss
    kw, flags = OBJ_VARIANTS[name]
    flags = flags if wide else {}
    K, loo = kw.get("num_samples", 1), kw.get("baseline") == "leave_one_out"
    logits, targets, il, tl, units, alphabet = _objective_case(V)
    sp = _spelling(units, alphabet)
    ild, tld = dv(il), dv(tl)
    z = logits.to(DEV).requires_grad_(True)
    call = dict(lam=1.0, seed=3, offset=1, reward_unit=unit, **kw, **flags)
    loss, nll, R_s, R_b = pg_ctc_loss(z, ild, targets.to(DEV), tld, unit_spelling=sp, **call)
    truncated = PGCTCLossFn.last_spell_truncated
    loss.backward()
    assert truncated.dtype == torch.int32 and truncated.is_cuda and int(truncated) == 0
    # the device's discrete choices, made as the loss section makes them
    lp_dev = ops.log_softmax_rows(logits.to(DEV))
    greedy, paths = ops.frame_sample_multi(lp_dev, K, seed=3, offset=1, want_greedy=True)
    o = R.objective(logits.double().numpy(), il, targets.numpy(), tl, R.spelled_reward(units, unit), paths=paths.cpu().numpy(),
                    greedy_frames=greedy.cpu().numpy(), baseline=kw.get("baseline", "hypothesis"),
                    score_function=kw.get("score_function", "path"), max_hyp_len=kw.get("max_hyp_len"),
                    entropy_weight=kw.get("entropy_weight", 0.0))
    lerr, gerr = abs(float(loss.detach()) - o.loss) / abs(o.loss), rel_err(z.grad.cpu(), o.grad)
    print(f"[unit spelling objective] V={V} {name} {unit}: loss rel err {lerr:.2e}, d(logits) rel err {gerr:.2e}, largest |coef| "
          f"{np.abs(o.coef).max():.2e}")
    assert np.abs(o.coef).max() > 0                                             # the reward term is there
    np.testing.assert_allclose(R_s.cpu().numpy().reshape(K, OBJ["B"]), o.R, rtol=1e-6)
    np.testing.assert_allclose(R_b.cpu().numpy(), o.baselines.mean(axis=0) if loo else o.R_hyp, rtol=1e-6, atol=1e-7)
    assert lerr < 1e-5, (float(loss.detach()), o.loss)
    assert gerr < 1e-4
    if kw.get("score_function") == "sequence":
        assert np.array_equal(PGCTCLossFn.last_sequence_scored.cpu().numpy(), o.scored)
    return call, (z, ild, targets.to(DEV), tld)


@pytest.mark.parametrize("unit", ["char", "word"])
@pytest.mark.parametrize("name", list(OBJ_VARIANTS))
@pytest.mark.parametrize("V", [70, 300])
def test_pg_ctc_loss_with_a_spelling_vs_oracle(ops, V, name, unit):
    """pg_ctc_loss(unit_spelling=) at 70 and 300 units, T = 24, B = 3, against the fp64 oracle with the spelled reward.  The word
    reward without the spelling keeps being refused."""
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    call, (z, ild, tg, tld) = _objective_vs_oracle(ops, V, name, unit, wide=True)
    if unit == "word":
        with pytest.raises(ValueError, match="reward_unit='word' takes an alphabet of at most 64 symbols"):
            pg_ctc_loss(z.detach(), ild, tg, tld, **dict(call, word_delimiter=1))


@pytest.mark.parametrize("name", list(OBJ_VARIANTS))
def test_a_narrow_units_model_takes_the_spelling_too(ops, name):
    """40 units on the narrow kernels with a spelling and the word reward, against the same reference."""
    _objective_vs_oracle(ops, 40, name, "word", wide=False)


def test_the_spelled_rewards_are_not_the_unit_rewards(ops):
    """On the objective's own case the spelled character reward, the spelled word reward and the unit reward differ: a pass that
    spelled nothing would not go unnoticed."""
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    logits, targets, il, tl, units, alphabet = _objective_case(300)
    sp = _spelling(units, alphabet)
    out = {}
    for key, kw in (("unit", {}), ("char", dict(unit_spelling=sp)), ("word", dict(unit_spelling=sp, reward_unit="word"))):
        out[key] = pg_ctc_loss(logits.to(DEV), dv(il), targets.to(DEV), dv(tl), lam=1.0, seed=3, offset=1, **kw)[2].cpu().numpy()
    assert not np.array_equal(out["unit"], out["char"]) and not np.array_equal(out["char"], out["word"])


# ---- 4. MWER ----
def test_mwer_word_risk_over_the_spelled_list_vs_fp64():
    """mwer_ctc_loss_lm(wide_sequence=True, unit_spelling=, risk_unit="word") at 300 units, nbest 4, against mwer_ref's closed form on
    the device's own list with the spelled word distances: loss and d(logits) 1e-5, the statistics as in tests/test_wide_seq_gpu.py.
    The logits lean towards an alignment of the target, so the list holds near misses of different risks.  Without the spelling the
    word risk is refused as ever."""
    from policy_gradient_asr_amd.mwer import MWERLossFn, mwer_ctc_loss_lm
    T_, B_, V, beam, N, L = 60, 4, 300, 8, 4, 6
    units, alphabet = R.random_units(V, 17, alphabet=SPACED)
    sp = _spelling(units, alphabet)
    g = torch.Generator().manual_seed(560)
    logits = (torch.randn(T_, B_, V, generator=g, dtype=torch.float64) * 2).float()
    in_len = torch.tensor([T_, T_ - T_ // 4, T_ // 2, 20], dtype=torch.int32)
    tg_len = torch.tensor([6, 5, 4, 3], dtype=torch.int32)
    targets = torch.randint(1, V, (B_, L), generator=g, dtype=torch.int32)
    for b in range(B_):
        targets[b, int(tg_len[b]):] = 0
        for i in range(int(tg_len[b])):                  # three frames per target unit, a blank frame between two units
            logits[4 * i:4 * i + 3, b, int(targets[b, i])] += 3.0
            logits[4 * i + 3, b, 0] += 3.0
    lg = logits.to(DEV).requires_grad_(True)
    args = (in_len.to(DEV), targets.to(DEV), tg_len.to(DEV))
    out = mwer_ctc_loss_lm(lg, *args, lam=1.0, beam=beam, nbest=N, wide_sequence=True, unit_spelling=sp, risk_unit="word")
    out[0].backward()
    torch.cuda.synchronize()
    assert int(MWERLossFn.last_spell_truncated) == 0
    tokens, lengths, score, count = (t.cpu().numpy() for t in MWERLossFn.last_nbest)
    dist, risk_len = np.zeros((N, B_), dtype=np.int64), np.zeros(B_, dtype=np.int64)
    for b in range(B_):
        y = targets[b, :int(tg_len[b])].tolist()
        for n in range(N):
            _, _, dist[n, b], _, risk_len[b] = R.distances(units, y, tokens[n, b, :lengths[n, b]])
    ref = MR.mwer_closed_form(logits.double().numpy(), in_len.numpy(), targets.numpy(), tg_len.numpy(), tokens, lengths, count,
                              min(T_, 1023), 1.0, B_, dist, risk_len)
    assert any(ref.w.valid[:, b].sum() >= 2 and np.ptp(ref.w.r[ref.w.valid[:, b], b]) > 0 for b in range(B_))
    assert np.abs(ref.w.coef).max() > 0
    unit_dist, _ = MR.risks(targets.numpy(), tg_len.numpy(), tokens, lengths)
    assert not np.array_equal(unit_dist, dist)                                  # the word risk is not the unit risk
    loss, grad = float(out[0].detach()), lg.grad.cpu().double().numpy()
    lerr = abs(loss - ref.loss) / abs(ref.loss)
    gerr = np.abs(grad - ref.grad).max() / np.abs(ref.grad).max()
    print(f"[unit spelling mwer] loss rel err {lerr:.2e}; d(logits) max-norm rel err {gerr:.2e}; largest |coef| {np.abs(ref.w.coef).max():.2e}")
    assert lerr <= 1e-5 and gerr <= 1e-5
    np.testing.assert_allclose(out[1].cpu().numpy(), ref.nll, rtol=1e-5)
    np.testing.assert_allclose(out[2].cpu().numpy(), -ref.w.rbar, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out[3].cpu().numpy(), -ref.w.r[0], rtol=1e-6)
    np.testing.assert_allclose(MWERLossFn.last_posterior.cpu().numpy(), ref.w.p, rtol=0, atol=1e-4)
    np.testing.assert_allclose(MWERLossFn.last_risk.cpu().numpy(), ref.w.r, rtol=1e-6)
    with pytest.raises(ValueError, match="a list of units has no word boundaries of its own"):
        mwer_ctc_loss_lm(logits.to(DEV), *args, lam=1.0, beam=beam, nbest=N, wide_sequence=True, risk_unit="word", word_delimiter=1)


# ---- 5. the trainer and the shards ----
def test_trainer_step_with_the_word_reward_at_300_units(ops, monkeypatch):
    """One PolicyGradientTrainer(wide_alphabet=True, unit_spelling=, reward_unit="word") step of the whole model: the rewards are the
    spelled word rewards of the paths the step drew (recorded from the sampler), last_spell_truncated == 0, the update is finite;
    reward_unit="word" without the spelling is refused at construction as ever."""
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    s = dict(B=4, F=80, T=120, V=300, L=12, lens=[120, 90, 120, 64], tlens=[12, 9, 12, 5])
    units, alphabet = R.random_units(300, 23, alphabet=SPACED)
    sp = _spelling(units, alphabet)
    batch = make_batch(s["B"], s["F"], s["T"], s["V"], s["L"], s["lens"], s["tlens"], 61)
    _, _, m = oracle_model(s["F"], s["V"], 62)
    with pytest.raises(ValueError, match="reward_unit='word' takes an alphabet of at most 64 symbols"):
        PolicyGradientTrainer(m, lam=1.0, seed=3, precision="f32", wide_alphabet=True, reward_unit="word", word_delimiter=1)
    recorded = []
    real = ops.frame_argmax_sample

    def recording(*a, **k):
        out = real(*a, **k)
        recorded.append(out)
        return out
    monkeypatch.setattr(ops, "frame_argmax_sample", recording)
    with ops.precision("f32"):
        tr = PolicyGradientTrainer(m, lam=1.0, seed=3, precision="f32", wide_alphabet=True, reward_unit="word", unit_spelling=sp)
        loss = tr.step(*(t.to(DEV) for t in batch))
        torch.cuda.synchronize()
        ops.lstm_assert_no_timeouts()
    assert len(recorded) == 1 and np.isfinite(float(loss))
    assert tr.last_spell_truncated.dtype == torch.int32 and int(tr.last_spell_truncated) == 0
    greedy, sample = (p.cpu().numpy() for p in recorded[0])
    reward = R.spelled_reward(units, "word")
    _, targets, _, _ = batch
    ys = [targets[b, :s["tlens"][b]].tolist() for b in range(s["B"])]
    want_s = [reward(ys[b], [int(t) for t in decode_ref.collapse_path(sample[:s["lens"][b], b], 0)]) for b in range(s["B"])]
    want_g = [reward(ys[b], [int(t) for t in decode_ref.collapse_path(greedy[:s["lens"][b], b], 0)]) for b in range(s["B"])]
    nll, R_s, R_b = tr.last_stats
    np.testing.assert_allclose(R_s.cpu().numpy(), want_s, rtol=1e-6)
    np.testing.assert_allclose(R_b.cpu().numpy(), want_g, rtol=1e-6)
    assert all(bool(torch.isfinite(q).all()) for q in m.parameters()) and tr.applied_steps() >= 1


def test_shards_sum_to_the_whole_batch_with_the_word_reward():
    """pg_harness.shards_vs_whole at 300 units with four samples, the leave-one-out baseline and the spelled word reward: the same
    rewards bit for bit, d(logits) and loss within 1e-6."""
    from policy_gradient_asr_amd.loss import PGCTCLossFn
    units, alphabet = R.random_units(300, 29, alphabet=SPACED)
    kw = dict(lam=1.0, seed=9, offset=2, num_samples=4, baseline="leave_one_out", wide_objectives=True, reward_unit="word",
              unit_spelling=_spelling(units, alphabet))
    r = shards_vs_whole(kw, lattice_case(150, 4, 300, 12, 77), extra=lambda: PGCTCLossFn.last_spell_truncated.clone())
    assert r.R_s.shape == (4, 4) and float(r.grad.abs().max()) > 0 and bool(torch.isfinite(r.loss))
    assert int(r.extra_whole) == 0 and all(int(t) == 0 for t in r.extra_parts)


# ---- 6. the drivers ----
def test_train_and_predict_drivers_over_spelled_text(tmp_path, capsys):
    """model.train(units_path=, spelled_reward=True, reward_unit="word") for one epoch over 100 units: it runs and the checkpoint
    holds the keyword; without it the word reward is refused as ever.  model.predict(units_path=, spelled=True): the error report
    with greedy decoding, and with the wide search and its second pass mbr_unit="word", the error report and the oracle as a CER over
    spelled text; without spelled=True each refusal stands."""
    import itertools
    import os
    from pg_harness import tiny_corpus
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.model import _read_alphabet, predict, train
    from policy_gradient_asr_amd.units import SubwordUnits
    corpus, out, _ = tiny_corpus(tmp_path)
    base = ["a", "b", "c", "d", " "]
    two = ["".join(q) for q in itertools.product(base, repeat=2)]
    three = ["".join(q) for q in itertools.product(base, repeat=3)]
    upath = str(corpus / "units.txt")
    SubwordUnits(base + two + three[:70]).save(upath)
    _, char2ind = _read_alphabet(upath)
    ds = SyntheticSpeech(32, char2ind, n_feats=20, max_chars=4, seed=1)
    kw = dict(train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=0, units_path=upath, reward_unit="word")
    with pytest.raises(ValueError, match="reward_unit='word' takes an alphabet of at most 64 symbols"):
        train(str(corpus), str(tmp_path / "other"), 1, 16, 0, **kw)
    with pytest.raises(ValueError, match="needs units_path"):
        train(str(corpus), str(tmp_path / "other"), 1, 16, 0, train_dataset=ds, n_feats=20, spelled_reward=True)
    losses, _ = train(str(corpus), str(out), 1, 16, 0, spelled_reward=True, **kw)
    assert len(losses) == 1 and np.isfinite(losses[0])
    st = torch.load(os.path.join(str(out), "checkpoint_last.pth"), map_location="cpu")
    assert st["spelled_reward"] is True and st["wide_alphabet"] is True and st["reward_unit"] == "word"
    pk = dict(test_dataset=SyntheticSpeech(16, char2ind, n_feats=20, max_chars=4, seed=2), n_feats=20, units_path=upath)
    alphabet_txt = str(corpus / "alphabet.txt")
    with pytest.raises(ValueError, match="ErrorReport"):
        predict(None, None, alphabet_txt, str(out), 8, beam_size=0, error_report=True, **pk)
    capsys.readouterr()
    cer, wer = predict(None, None, alphabet_txt, str(out), 8, beam_size=0, error_report=True, spelled=True, **pk)
    assert np.isfinite(cer) and np.isfinite(wer) and "%CER" in capsys.readouterr().out
    assert os.path.exists(os.path.join(str(out), "errors.txt")) and os.path.exists(os.path.join(str(out), "confusions.tsv"))
    wide = dict(beam_size=4, wide_beam=True, wide_second_pass=True, nbest=3, mbr=True, mbr_unit="word")
    with pytest.raises(ValueError, match="a subword unit may span a space"):
        predict(None, None, alphabet_txt, str(out), 8, **wide, **pk)
    with pytest.raises(ValueError, match="error_report"):
        predict(None, None, alphabet_txt, str(out), 8, **dict(wide, mbr_unit="char"), error_report=True, **pk)
    capsys.readouterr()
    cer, wer = predict(None, None, alphabet_txt, str(out), 8, error_report=True, spelled=True, **wide, **pk)
    text = capsys.readouterr().out
    assert np.isfinite(cer) and np.isfinite(wer) and "MBR (word)" in text and "Oracle CER (3-best)" in text and "%WER" in text
    assert len(open(os.path.join(str(out), "mbr.tsv")).read().splitlines()) == 16
    capsys.readouterr()
    predict(None, None, None, str(out), 8, beam_size=4, wide_beam=True, nbest=2, spelled=True, **pk)      # no alphabet file: the units' characters
    assert "Oracle CER (2-best)" in capsys.readouterr().out
