"""csrc/confidence.hip (include/pgasr_hip.h, A10-CONF) against tests/confidence_ref.py, every fp64 word bit for bit, on the inputs
tests/test_confidence_cpu.py proves discriminating; then the layers above it: hipops.edit_ops_slot_mass / nbest_confidence,
CTCDecoder.confidence / decode_words, metrics.hyp_correct and model.predict(word_confidence=True)."""
import math
import os

import numpy as np
import pytest
import torch

import confidence_cases as C
import confidence_ref as R
import editops_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
OK, INVALID, UNSUPPORTED = 0, 1, 4


def _ops():
    from policy_gradient_asr_amd import hipops
    return hipops


def _raw(ops, n_ops, weight, per_group, side, slots, stream=0):
    """The C entry itself, outputs prefilled with NaN / -7: (status, mass, n_slots, left_out) as numpy."""
    from policy_gradient_asr_amd import _lib
    ops_t = torch.from_numpy(np.ascontiguousarray(ops, dtype=np.int8)).to(DEV)
    n_t = torch.from_numpy(np.ascontiguousarray(n_ops, dtype=np.int32)).to(DEV)
    w_t = torch.from_numpy(np.ascontiguousarray(weight, dtype=np.float64)).to(DEV)
    groups = ops.shape[0] // per_group
    mass = torch.full((groups, 4, slots + 1), float("nan"), dtype=torch.float64, device=DEV)
    meta = torch.full((2, groups), -7, dtype=torch.int32, device=DEV)
    st = _lib.load().pgasr_edit_ops_slot_mass(ops_t.data_ptr() if ops.shape[1] else 0, n_t.data_ptr(), ops.shape[1], w_t.data_ptr(),
                                              groups, per_group, side, slots, mass.data_ptr(), meta[0].data_ptr(),
                                              meta[1].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, mass.cpu().numpy(), meta[0].cpu().numpy(), meta[1].cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _check(ops, n_ops, weight, per_group, side, slots):
    want_mass, want_n, want_left = R.slot_mass(ops, n_ops, weight, per_group, side, slots)
    st, mass, n_slots, left = _raw(ops, n_ops, weight, per_group, R.SIDES[side], slots)
    assert st == OK
    assert np.array_equal(n_slots, want_n) and np.array_equal(left, want_left)
    assert np.array_equal(mass, want_mass) and np.array_equal(_bits(mass), _bits(want_mass))     # == on every word, and its bits
    return mass, n_slots, left


@pytest.mark.parametrize("side", ["ref", "hyp"])
def test_operation_string_lengths(side):
    """Strings of exactly 0, 1, 63, 64, 65, 255 .. 257, 511 .. 513, 1023 .. 1025, 1536, 1537 and 1860 operations (every seam of the
    512-operation chunks and of their waves), one group per length in one launch, four pairs a group; the stride and the slot
    count are larger than any group needs."""
    cases = C.length_cases()
    lists, weight = [], []
    for K, pivot, rows, ws, _ in cases:
        group = C.op_lists(pivot, rows, side)
        assert K in [len(o) for o in group]
        lists += group; weight += ws
    ops, n_ops = C.pack_ops(lists, extra=7)
    mass, n_slots, left = _check(ops, n_ops, weight, 4, side, max(len(c[1]) for c in cases) + 2)
    assert n_slots.tolist() == [len(c[1]) for c in cases] and not left.any()
    assert mass[0, :3].sum() == 0 and mass[0, 3, 0] > 0        # the empty pivot: all insertions, into gap 0


@pytest.mark.parametrize("side", ["ref", "hyp"])
@pytest.mark.parametrize("index", range(len(C.GROUP_SHAPES)))
def test_group_shapes(index, side):
    """per_group 1, 2, 16 and 128 at 1 and 5 groups, pivots of 5 .. 70 symbols, slots exactly the longest pivot."""
    pg, G, groups = C.shape_cases()[index]
    lists = [o for pivot, rows, _, _ in groups for o in C.op_lists(pivot, rows, side)]
    weight = [w for _, _, ws, _ in groups for w in ws]
    assert len(lists) == pg * G
    ops, n_ops = C.pack_ops(lists, extra=0)
    _, n_slots, left = _check(ops, n_ops, weight, pg, side, max(len(g[0]) for g in groups))
    assert n_slots.tolist() == [len(g[0]) for g in groups] and not left.any()


def test_pairs_that_take_no_part_or_are_left_out():
    """One launch, 16 pairs a group: weights of 0, NaN, +inf, -inf and a negative one in the middle of a group (and in front: the
    pivot is then the first pair that does take part); n_ops below 0 and above the stride; a pair with another slot count; a
    group where nobody takes part; an empty pivot; garbage behind n_ops."""
    pg, G, groups = C.shape_cases()[5]
    assert (pg, G) == (16, 5)
    lists = [C.op_lists(pivot, rows, "ref") for pivot, rows, _, _ in groups]
    weight = np.asarray([ws for _, _, ws, _ in groups], dtype=np.float64)
    weight[0, [0, 3, 5, 6, 9, 11]] = [0.0, float("nan"), float("inf"), -0.25, -float("inf"), -0.0]
    lists[1][4] = lists[0][2]                                # another pivot's string: (almost surely) another slot count
    assert R.slot_count(lists[1][4], "ref") != len(groups[1][0])
    weight[2, :] = [0.0, float("nan"), -1.0, float("inf")] * 4
    lists[3] = [[3] * k for k in range(16)]                  # an empty pivot: k insertions into gap 0
    flat = [o for group in lists for o in group]
    ops, n_ops = C.pack_ops(flat, extra=9, fill=0)           # "hits" behind every string: they are not to be read
    n_ops[4 * 16 + 1] = -1; n_ops[4 * 16 + 2] = ops.shape[1] + 1; n_ops[4 * 16 + 3] = 2 ** 31 - 1
    slots = max(len(g[0]) for g in groups) + 1
    mass, n_slots, left = _check(ops, n_ops, weight.reshape(-1), 16, "ref", slots)
    assert n_slots.tolist() == [len(groups[0][0]), len(groups[1][0]), -1, 0, len(groups[4][0])]
    assert left.tolist() == [0, 1, 0, 0, 0] and not mass[2].any()
    assert mass[3, 3, 0] > 0 and not mass[3, :3].any()
    # every pair on the other side too, and slots below the pivots' lengths: those groups are left out whole
    ops_h, n_h = C.pack_ops([C.mirror(o) for o in flat], extra=2)
    _check(ops_h, n_h, weight.reshape(-1), 16, "hyp", slots)
    small = sorted(len(g[0]) for g in groups)[2]
    mass, n_slots, left = _check(ops_h, n_h, weight.reshape(-1), 16, "hyp", small)
    for g in (0, 1, 4):
        if len(groups[g][0]) > small:
            assert not mass[g].any() and n_slots[g] == len(groups[g][0]) and left[g] > 0


def test_one_pair_per_group_and_no_operations():
    """per_group = 1 over many groups (hyp_correct's shape), a stride of 0 without an ops pointer, slots = 0."""
    st, mass, n_slots, left = _raw(np.zeros((3, 0), dtype=np.int8), [0, 0, 1], [1.0, 0.0, 1.0], 1, 0, 0)
    assert st == OK and n_slots.tolist() == [0, -1, -1] and not mass.any() and mass.shape == (3, 4, 1) and not left.any()
    lists = [[0, 1, 2, 3, 3, 0], [3, 3], [2, 2], []]
    ops, n_ops = C.pack_ops(lists, extra=0)
    for side in ("ref", "hyp"):
        _check(ops, n_ops, [1.0, 0.5, 0.25, 2.0], 1, side, 4)
        _check(ops, n_ops, [1.0, 0.5, 0.25, 2.0], 1, side, 0)


def test_refusals_of_the_entry():
    ops, n_ops = C.pack_ops([[0, 1]] * 4)
    w = [0.25] * 4
    assert _raw(ops, n_ops, w, 2, 2, 4)[0] == INVALID and _raw(ops, n_ops, w, 2, -1, 4)[0] == INVALID
    assert _raw(ops, n_ops, w, 2, 0, 4096)[0] == UNSUPPORTED and _raw(ops, n_ops, w, 2, 0, 4095)[0] == OK
    wide = np.zeros((1, 8191), dtype=np.int8)
    assert _raw(wide, [2], [1.0], 1, 0, 4)[0] == UNSUPPORTED and _raw(wide[:, :8190], [2], [1.0], 1, 0, 4)[0] == OK
    big = np.zeros((129, 2), dtype=np.int8)
    assert _raw(big, [2] * 129, [1.0] * 129, 129, 0, 4)[0] == UNSUPPORTED
    from policy_gradient_asr_amd import _lib
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.float64, device=DEV)
    p = t.data_ptr()
    good = [p, p, 2, p, 1, 1, 0, 2, p, p, p, 0]
    for null_at in (0, 1, 3, 8, 9, 10):
        args = list(good); args[null_at] = 0
        assert lib.pgasr_edit_ops_slot_mass(*args) == INVALID
    for at, bad in ((4, 0), (5, 0), (2, -1), (7, -1)):
        args = list(good); args[at] = bad
        assert lib.pgasr_edit_ops_slot_mass(*args) == INVALID
    hipops = _ops()
    o, n, wt = (torch.from_numpy(a).to(DEV) for a in (ops, n_ops, np.asarray(w)))
    with pytest.raises(ValueError, match="side"):
        hipops.edit_ops_slot_mass(o, n, wt, 2, side="both")
    with pytest.raises(Exception, match="per_group"):
        hipops.edit_ops_slot_mass(o, n, wt, 3)
    with pytest.raises(Exception, match="float64"):
        hipops.edit_ops_slot_mass(o, n, wt.float(), 2)


def test_wrapper_views_and_slots():
    hipops = _ops()
    pg, G, groups = C.shape_cases()[3]                       # 2 pairs, 5 groups
    lists = [o for pivot, rows, _, _ in groups for o in C.op_lists(pivot, rows, "ref")]
    weight = [w for _, _, ws, _ in groups for w in ws]
    ops, n_ops = C.pack_ops(lists)
    o, n, w = torch.from_numpy(ops).to(DEV), torch.from_numpy(n_ops).to(DEV), torch.tensor(weight, dtype=torch.float64, device=DEV)
    sm = hipops.edit_ops_slot_mass(o, n, w, pg, side="ref", slots=90)
    want, want_n, want_left = R.slot_mass(ops, n_ops, weight, pg, "ref", 90)
    for ch, field in enumerate((sm.hit, sm.sub, sm.gap, sm.other)):
        assert tuple(field.shape) == (G, 91) and np.array_equal(field.cpu().numpy(), want[:, ch])
    assert sm.n_slots.tolist() == want_n.tolist() and sm.left_out.tolist() == want_left.tolist()
    auto = hipops.edit_ops_slot_mass(o, n, w, pg)            # slots read from the device: the longest string bounds every count
    W = auto.hit.shape[1]
    assert W == int(n_ops.max()) + 1 <= 91 and np.array_equal(auto.hit.cpu().numpy(), want[:, 0, :W])


# ---- nbest_confidence on handmade lists ----

def _list_tensors(rows_per_utt, stride, extra_rows=0, fill=1):
    """Lists of token rows per utterance -> tokens (N,B,stride), lengths (N,B), count (B) on the device; rows beyond a list's
    count are filled with ``fill`` and a length that would matter if they were read."""
    B = len(rows_per_utt)
    N = max(len(r) for r in rows_per_utt) + extra_rows
    tokens = np.full((N, B, stride), fill, dtype=np.int32)
    lengths = np.full((N, B), 2, dtype=np.int32)
    count = np.zeros(B, dtype=np.int32)
    for b, rows in enumerate(rows_per_utt):
        count[b] = len(rows)
        for n, r in enumerate(rows):
            tokens[n, b, :len(r)] = r
            lengths[n, b] = len(r)
    return tuple(torch.from_numpy(a).to(DEV) for a in (tokens, lengths, count))


def _posterior(weights_per_utt, N):
    p = np.zeros((N, len(weights_per_utt)), dtype=np.float64)
    for b, ws in enumerate(weights_per_utt):
        p[:len(ws), b] = ws
    return torch.from_numpy(p).to(DEV)


def _hand_lists(sym, space):
    """The hand-worked list at character level, the same list with its letters as words, and a second utterance with another
    pivot, over the symbol ids ``sym`` gives."""
    rows, weights, want = C.hand_case()
    chars = [[sym(c) for c in r] for r in rows]
    spaced = [[sym(c) if c != " " else space for c in " ".join(r)] for r in rows]
    return rows, weights, want, chars, spaced


@pytest.mark.parametrize("V", [29, 300])
def test_nbest_confidence_by_hand(V):
    """The list of the statement's hand-worked case with symbol ids below 29, and with ids up to 299 as a wide search returns
    them: every mass is the short binary fraction written out in tests/confidence_cases.py."""
    hipops = _ops()
    sym = (lambda c: 1 + ord(c) - ord("a")) if V == 29 else (lambda c: 299 - 7 * (ord(c) - ord("a")))
    rows, weights, want, chars, spaced = _hand_lists(sym, 28)
    other = [chars[2], chars[0], chars[3]]                   # a second utterance: pivot "ac" at rank 0, three rows
    tokens, lengths, count = _list_tensors([chars, other], stride=9, extra_rows=2)
    post = _posterior([weights, [0.5, 0.25, 0.25]], tokens.shape[0])
    pivot = torch.tensor([0, 0], dtype=torch.int32, device=DEV)
    c = hipops.nbest_confidence(tokens, lengths, count, post, pivot, vocab=V)
    assert tuple(c.tokens.shape) == (2, 9) and c.lengths.tolist() == [3, 2] and c.tokens[0, :3].tolist() == chars[0]
    assert tuple(c.conf.shape) == (2, 10) and c.left_out.tolist() == [0, 0]
    for field, name in ((c.conf, "conf"), (c.substituted, "substituted"), (c.deleted, "deleted"), (c.inserted, "inserted")):
        assert field[0].tolist() == want[name] + [0.0] * 6, name
    got = R.nbest_confidence(["ac", "abc", "xabcc"], [0.5, 0.25, 0.25], 0, slots=9)
    assert [c.conf[1].tolist(), c.substituted[1].tolist(), c.deleted[1].tolist(), c.inserted[1].tolist()] == [list(x) for x in got[:4]]
    # "ac" HH, "abc" HIH, "xabcc" IHIIH: one x in front of a (1/4), b from both longer rows and a c between a and c (1/4 + 2/4)
    assert c.conf[1, :2].tolist() == [1.0, 1.0] and c.inserted[1, :3].tolist() == [0.25, 0.75, 0.0]
    # another pivot per utterance, a row with posterior 0 and a cap that shuts the longest row out
    pivot = torch.tensor([2, 1], dtype=torch.int32, device=DEV)
    c = hipops.nbest_confidence(tokens, lengths, count, post, pivot, max_hyp_len=4)
    got = R.nbest_confidence(rows[:3], weights[:3], 2, slots=4)
    assert c.lengths.tolist() == [2, 3] and tuple(c.conf.shape) == (2, 5)
    assert [c.conf[0].tolist(), c.substituted[0].tolist(), c.deleted[0].tolist(), c.inserted[0].tolist()] == [list(x) for x in got[:4]]
    if V == 29:
        tokens, lengths, count = _list_tensors([spaced], stride=12)
        c = hipops.nbest_confidence(tokens, lengths, count, _posterior([weights], 4), pivot[:1] * 0, unit="word", delimiter=28, vocab=V)
        assert c.tokens is None and c.lengths.tolist() == [3] and tuple(c.conf.shape) == (1, 14)
        for field, name in ((c.conf, "conf"), (c.substituted, "substituted"), (c.deleted, "deleted"), (c.inserted, "inserted")):
            assert field[0].tolist() == want[name] + [0.0] * 10, name
    else:
        with pytest.raises(ValueError, match="unit='word'"):
            hipops.nbest_confidence(tokens, lengths, count, post, pivot, unit="word", delimiter=28, vocab=V)
        from policy_gradient_asr_amd.CTCdecoder import CTCDecoder, MBRDecoded
        dec = CTCDecoder(["<b>"] + ["u%d" % i for i in range(298)] + [" "], wide_search=True)
        md = MBRDecoded(None, None, pivot, None, post, None, hipops.CTCNBest(tokens, lengths, None, count))
        with pytest.raises(ValueError, match="unit='word'"):
            dec.confidence(md, unit="word")
        assert dec.confidence(md, pivot="map").conf[0].tolist() == want["conf"] + [0.0] * 6


def test_nbest_confidence_refusals_and_chunks():
    hipops = _ops()
    rows, weights, want, chars, _ = _hand_lists(lambda c: 1 + ord(c) - ord("a"), 28)
    tokens, lengths, count = _list_tensors([chars] * 5, stride=9)
    post = _posterior([weights] * 5, 4)
    pivot = torch.zeros(5, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="unit"):
        hipops.nbest_confidence(tokens, lengths, count, post, pivot, unit="syllable")
    with pytest.raises(ValueError, match="delimiter"):
        hipops.nbest_confidence(tokens, lengths, count, post, pivot, unit="word")
    with pytest.raises(Exception, match="float64"):
        hipops.nbest_confidence(tokens, lengths, count, post.float(), pivot)
    with pytest.raises(Exception, match="pivot"):
        hipops.nbest_confidence(tokens, lengths, count, post, pivot[:3])
    # a workspace cap of one utterance's pairs: five chunks, the same words
    per_pair = hipops.edit_ops_workspace_bytes(9, 9, 1)
    c = hipops.nbest_confidence(tokens, lengths, count, post, pivot, max_workspace_bytes=4 * per_pair)
    for b in range(5):
        assert c.conf[b].tolist() == want["conf"] + [0.0] * 6 and c.inserted[b].tolist() == want["inserted"] + [0.0] * 6


# ---- the decoder ----

ALPHABET = ["_", "a", "b", "c", "d", "e", "f", " "]


@pytest.fixture(scope="module")
def decoded():
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    g = torch.Generator().manual_seed(11)
    T, B, V = 40, 3, 8
    logits = 2.5 * torch.randn(T, B, V, generator=g)
    logits[:, :, 7] += 0.5                                   # spaces: several words a row
    lp = torch.log_softmax(logits, 2).to(DEV).contiguous()
    lengths = torch.tensor([40, 33, 25], dtype=torch.int32, device=DEV)
    dec = CTCDecoder(ALPHABET)
    md = dec.mbr_decode(lp, lengths, beam_size=8, nbest=8)
    return dec, lp, lengths, md


@pytest.mark.parametrize("pivot", ["map", "mbr"])
def test_decode_words_end_to_end(decoded, pivot):
    """T = 40, B = 3, V = 8, beam 8, 8-best: decode_words against the statement run on the device's own list and posterior; the
    pivot's own posterior bounds every confidence from below; the spans are align_batch + word_spans on the pivot rows."""
    from policy_gradient_asr_amd.CTCdecoder import word_spans
    dec, lp, lengths, md = decoded
    got = dec.decode_words(lp, lengths, beam_size=8, nbest=8, pivot=pivot)
    nb = md.nbest
    tok, ln, cnt, post = nb.tokens.cpu().numpy(), nb.lengths.cpu().numpy(), nb.count.cpu().tolist(), md.posterior.cpu().numpy()
    piv = md.best.cpu().tolist() if pivot == "mbr" else [0, 0, 0]
    assert len(got) == 3 and min(cnt) >= 2
    ptok = torch.zeros(3, 40, dtype=torch.int32)
    plen = torch.zeros(3, dtype=torch.int32)
    for b in range(3):
        rows = [[int(x) for x in tok[n, b, :ln[n, b]]] if n < cnt[b] else [] for n in range(8)]
        p = [float(x) for x in post[:, b]]
        assert all(p[n] == 0 for n in range(cnt[b], 8)) and abs(sum(p) - 1) < 1e-12
        conf_c = R.nbest_confidence(rows, p, piv[b])[0]
        conf_w = R.nbest_confidence([R.words_of(r, 7) for r in rows], p, piv[b])[0]
        row = rows[piv[b]]
        words = R.words_of(row, 7)
        assert [w[0] for w in got[b]] == ["".join(ALPHABET[k] for k in w) for w in words]
        assert [w[3] for w in got[b]] == conf_w[:len(words)]
        assert [x for w in got[b] for x in w[4]] == [c for c, k in zip(conf_c, row) if k != 7]
        for x in [w[3] for w in got[b]] + [x for w in got[b] for x in w[4]]:
            assert p[piv[b]] <= x <= 1.0 + 1e-12
        ptok[b, :len(row)] = torch.tensor(row, dtype=torch.int32); plen[b] = len(row)
    al = dec.align_batch(lp, ptok.to(DEV), plen.to(DEV), lengths)
    st, en = al.token_start.cpu(), al.token_end.cpu()
    for b in range(3):
        n = int(plen[b])
        spans = word_spans(st[b, :n].tolist(), en[b, :n].tolist(), ptok[b, :n].tolist(), 7)
        assert [(w[1], w[2]) for w in got[b]] == spans
        assert any(s >= 0 for s, _ in spans)
        for (word, s, e, _, _) in got[b]:
            assert (s, e) == (-1, -1) if word == "" else 0 <= s < e <= int(lengths[b])


def test_confidence_pivots_and_refusals(decoded):
    dec, lp, lengths, md = decoded
    a = dec.confidence(md)                                   # pivot="mbr": md.best, the row md.tokens holds
    b = dec.confidence(md, pivot=md.best)
    assert torch.equal(a.conf, b.conf) and torch.equal(a.tokens[:, :md.tokens.shape[1]], md.tokens) and torch.equal(a.lengths, md.lengths)
    w = dec.confidence(md, pivot="map", unit="word")
    assert w.tokens is None and tuple(w.conf.shape) == (3, md.nbest.tokens.shape[2] + 2)
    with pytest.raises(ValueError, match="pivot"):
        dec.confidence(md, pivot="best")
    with pytest.raises(ValueError, match="pivot"):
        dec.confidence(md, pivot=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="unit"):
        dec.confidence(md, unit="phone")
    with pytest.raises(ValueError, match="pivot"):
        dec.decode_words(lp, lengths, beam_size=8, nbest=8, pivot="first")
    with pytest.raises(ValueError, match="risk_unit"):
        dec.decode_words(lp, lengths, beam_size=8, nbest=8, risk_unit="word")
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    with pytest.raises(ValueError, match="word_delimiter"):
        CTCDecoder(ALPHABET[:7]).decode_words(lp[:, :, :7].contiguous(), lengths, beam_size=8, nbest=8)


# ---- metrics ----

def test_hyp_correct_against_the_reference():
    from policy_gradient_asr_amd.metrics import confidence_nce, hyp_correct
    rng = np.random.default_rng(17)
    pairs = [("abc", "xabcc"), ("abc", ""), ("", "ab"), ("ab cd ab", "ab ab cd"), ("a b  c", "a  b c")]
    sym = {c: i + 1 for i, c in enumerate("abcdx ")}
    pairs = [([sym[c] for c in r], [sym[c] for c in h]) for r, h in pairs]
    for n, m in ((40, 37), (64, 70), (130, 129)):
        ref = rng.integers(1, 7, n).tolist()
        pairs.append((ref, C._mutate(rng, ref, m, 6) if m else []))
    R_, Hy = max(len(p[0]) for p in pairs) + 2, max(len(p[1]) for p in pairs) + 3
    ref = np.full((len(pairs), R_), 3, dtype=np.int32); hyp = np.full((len(pairs), Hy), 3, dtype=np.int32)
    for k, (r, h) in enumerate(pairs):
        ref[k, :len(r)] = r; hyp[k, :len(h)] = h
    rl = torch.tensor([len(p[0]) for p in pairs], dtype=torch.int32, device=DEV)
    hl = torch.tensor([len(p[1]) for p in pairs], dtype=torch.int32, device=DEV)
    ref_t, hyp_t = torch.from_numpy(ref).to(DEV), torch.from_numpy(hyp).to(DEV)
    right, n = hyp_correct(ref_t, rl, hyp_t, hl)
    assert tuple(right.shape) == (len(pairs), Hy + 1) and n.tolist() == [len(p[1]) for p in pairs]
    for k, (r, h) in enumerate(pairs):
        assert right[k].tolist() == R.hyp_correct(r, h) + [0.0] * (Hy + 1 - len(h)), k
    right_w, n_w = hyp_correct(ref_t, rl, hyp_t, hl, unit="word", delimiter=6)
    assert tuple(right_w.shape) == (len(pairs), Hy + 2)
    for k, (r, h) in enumerate(pairs):
        want = R.hyp_correct(R.words_of(r, 6), R.words_of(h, 6))
        assert n_w[k].item() == len(want) and right_w[k].tolist() == want + [0.0] * (Hy + 2 - len(want)), k
    with pytest.raises(ValueError, match="delimiter"):
        hyp_correct(ref_t, rl, hyp_t, hl, unit="word")
    # the labels and a device tensor of confidences through the NCE
    keep = torch.arange(Hy + 1, device=DEV).view(1, -1) < n.view(-1, 1)
    labels = right[keep]
    conf = torch.where(labels > 0.5, 0.8, 0.3).to(torch.float64)
    assert abs(confidence_nce(conf, labels) - R.nce(conf.cpu().numpy(), labels.cpu().numpy())) < 1e-12


# ---- model.predict(word_confidence=True) ----

def test_predict_word_confidence(tmp_path, capsys):
    """On the tiny synthetic corpus of the predict tests: words.tsv is well formed, its words are the hypotheses of predicted.txt,
    the NCE line is printed, and everything else is what the call without the flag gives."""
    from policy_gradient_asr_amd.CTCdecoder import collapse_fn
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.model import Seq2Seq, predict
    corpus = tmp_path / "corpus"; out = tmp_path / "run"
    corpus.mkdir(); out.mkdir()
    (corpus / "alphabet.txt").write_text("a\nb\nc\nd\n \n")
    char2ind = {"<pad>": 0, "a": 1, "b": 2, "c": 3, "d": 4, " ": 5}
    dv = SyntheticSpeech(16, char2ind, n_feats=20, seed=2)
    torch.manual_seed(5)
    torch.save(Seq2Seq(alphabet_size=6, n_feats=20).state_dict(), out / "model_best.pth")
    kw = dict(test_dataset=dv, n_feats=20, nbest=4)
    base = predict(None, None, str(corpus / "alphabet.txt"), str(out), 8, **kw)
    base_lines = open(out / "predicted.txt").read()
    base_out = capsys.readouterr().out
    assert not os.path.exists(out / "words.tsv")
    got = predict(None, None, str(corpus / "alphabet.txt"), str(out), 8, word_confidence=True, **kw)
    new_out = capsys.readouterr().out
    assert got == base and open(out / "predicted.txt").read() == base_lines
    assert new_out.splitlines()[:-1] == base_out.splitlines()
    last = new_out.splitlines()[-1]
    assert last.startswith("Confidence (4-best, pivot map) word NCE: ") and "character NCE: " in last
    rows = [ln.split("\t") for ln in open(out / "words.tsv").read().split("\n")[:-1]]
    assert all(len(r) == 6 for r in rows) and sorted({int(r[0]) for r in rows}) == list(range(16))
    hyps = [ln.split("|")[1] for ln in base_lines.splitlines()]
    for u in range(16):
        mine = [r for r in rows if int(r[0]) == u]
        assert [int(r[1]) for r in mine] == list(range(len(mine)))
        assert collapse_fn(" ".join(r[2] for r in mine)) == hyps[u]
        prev = 0
        for _, _, word, s, e, conf in mine:
            s, e, conf = int(s), int(e), float(conf)
            assert 0.0 <= conf <= 1.0 + 1e-9 and math.isfinite(conf)
            if word == "":
                assert (s, e) == (-1, -1)
            elif s >= 0:
                assert prev <= s < e
                prev = e
            else:
                assert (s, e) == (-1, -1)
    # under a frame_stack policy the batch is stacked in the loop: the same hypotheses, spans in INPUT frames as align writes them
    stacked = tmp_path / "stacked"; stacked.mkdir()
    torch.manual_seed(6)
    torch.save(Seq2Seq(alphabet_size=6, n_feats=60).state_dict(), stacked / "model_best.pth")
    base = predict(None, None, str(corpus / "alphabet.txt"), str(stacked), 8, frame_stack=(3, 3), **kw)
    base_lines = open(stacked / "predicted.txt").read()
    assert predict(None, None, str(corpus / "alphabet.txt"), str(stacked), 8, frame_stack=(3, 3), word_confidence=True, **kw) == base
    assert open(stacked / "predicted.txt").read() == base_lines
    for u, _, word, s, e, _ in (ln.split("\t") for ln in open(stacked / "words.tsv").read().split("\n")[:-1]):
        n_in, s, e = dv[int(u)]["feat"].shape[1], int(s), int(e)
        if s >= 0:
            assert s % 3 == 0 and (e % 3 == 0 or e == n_in) and s < e <= n_in
    capsys.readouterr()
    predict(None, None, str(corpus / "alphabet.txt"), str(out), 8, word_confidence=True, confidence_pivot="mbr", mbr=True, **kw)
    assert "pivot mbr" in capsys.readouterr().out.splitlines()[-1]
    with pytest.raises(ValueError, match="nbest >= 2"):
        predict(None, None, str(corpus / "alphabet.txt"), str(out), 8, test_dataset=dv, n_feats=20, word_confidence=True)
    with pytest.raises(ValueError, match="subword"):
        predict(None, None, None, str(out), 8, units_path=str(corpus / "alphabet.txt"), word_confidence=True, **kw)
    with pytest.raises(ValueError, match="confidence_pivot"):
        predict(None, None, str(corpus / "alphabet.txt"), str(out), 8, word_confidence=True, confidence_pivot="top", **kw)
