"""csrc/editops.hip (include/pgasr_hip.h, A10-OPS) and the layers above it against tests/editops_ref.py, bit for bit: counts, the
operation string, n_ops, the -1 tail and the confusion matrix, at every length where the kernel's lane tiling changes, both ways
round, on tie-heavy rows (tests/test_editops_cpu.py proves that another tie rule changes their counts)."""
import os

import numpy as np
import pytest
import torch

import editops_cases as C
import editops_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _ops():
    from policy_gradient_asr_amd import hipops
    return hipops


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _run(ref, rl, hyp, hl, **kw):
    return _ops().edit_ops(_i32(ref), _i32(rl), _i32(hyp), _i32(hl), **kw)


def _check(eo, want):
    counts, ops, n_ops, _ = want
    assert np.array_equal(eo.counts.cpu().numpy(), counts)
    assert np.array_equal(eo.n_ops.cpu().numpy(), n_ops)
    assert np.array_equal(eo.ops.cpu().numpy(), ops)          # the -1 tail included


@pytest.fixture(scope="module")
def length_groups():
    """One launch per longer length (the kernel instantiation follows the longer STRIDE), the reference computed once: the
    strides one and two beyond the longer length."""
    groups = {}
    for n, m, ref, hyp in C.length_cases():
        groups.setdefault(max(n, m), []).append((ref, hyp))
    out = []
    for longer in C.TILING_LENGTHS:
        packed = C.pack(groups[longer], extra_ref=1, extra_hyp=2)
        assert packed[0].shape[1] == longer + 1 and packed[2].shape[1] == longer + 2
        out.append((packed, R.batch(*packed)))
    return out


def test_lengths_where_the_lane_tiling_changes(length_groups):
    """Longer length 0, 1, 63, 64, 65, .., 257, 1024, each both ways round and equal, empty sides included; strides larger than
    the lengths, padding filled with symbols of the rows."""
    for packed, want in length_groups:
        _check(_run(*packed), want)


def test_strides_equal_to_the_lengths(length_groups):
    """The same pairs with the longer stride EQUAL to the longer length: 63, 127, 255 are then the last lengths of their tilings,
    and at 0 both strides are 0 (no row pointer, no workspace, no operation)."""
    for (ref, rl, hyp, hl), (counts, ops, n_ops, _) in length_groups:
        longer = ref.shape[1] - 1
        eo = _run(ref[:, :longer], rl, hyp[:, :longer], hl)
        want_ops = np.full((ref.shape[0], 2 * longer), -1, dtype=np.int8)
        want_ops[:] = ops[:, :2 * longer]
        assert (ops[:, 2 * longer:] == -1).all()
        _check(eo, (counts, want_ops, n_ops, None))


@pytest.mark.parametrize("index", range(len(C.LONG_LENGTHS) * 3))
def test_long_pairs(index):
    """1025, 2049 and 4095: one pair each way round and one with equal lengths (the stride IS the limit at 4095)."""
    n, m, ref, hyp = C.long_cases()[index]
    pad = 0 if max(n, m) == 4095 else 2
    packed = C.pack([(ref, hyp)], extra_ref=pad if n >= m else 3, extra_hyp=pad if m >= n else 3)
    _check(_run(*packed), R.batch(*packed))


def test_lengths_below_zero_and_above_the_stride():
    rng = np.random.default_rng(9)
    ref = rng.integers(0, 4, (6, 70)); hyp = rng.integers(0, 4, (6, 40))
    rl = np.array([-3, 70, 71, 1000, 12, 0]); hl = np.array([5, -1, 40, 41, 2 ** 31 - 1, -2 ** 31])
    want = R.batch(ref, rl, hyp, hl)
    assert want[0][0].tolist() == [0, 0, 0, 5] and want[0][1].tolist() == [0, 0, 70, 0] and want[2][5] == 0
    _check(_run(ref, rl, hyp, hl), want)


@pytest.fixture(scope="module")
def tie_batch():
    cases = [(r, h) for _, r, h in C.tie_cases()]
    packed = C.pack(cases)
    return packed, R.batch(*packed, vocab=29)


def test_tie_heavy_rows(tie_batch):
    packed, want = tie_batch
    eo = _run(*packed)
    _check(eo, want)
    # the transposition: two substitutions, not a deletion and an insertion around a hit
    assert eo.counts[0].tolist() == [0, 2, 0, 0] and eo.ops[0, :3].tolist() == [1, 1, -1]
    # a run against a shorter run: the walk back takes the diagonal first, so the deletions come FIRST in the string
    assert eo.ops[2, :5].tolist() == [2, 2, 0, 0, -1] and eo.ops[3, :5].tolist() == [3, 3, 0, 0, -1]


def test_modes_agree(tie_batch, length_groups):
    hipops = _ops()
    for packed, want in [tie_batch] + length_groups[-3:]:
        args = [_i32(a) for a in packed]
        full = hipops.edit_ops(*args)
        only = hipops.edit_ops(*args, want_ops=False)
        assert only.ops is None and only.n_ops is None
        assert torch.equal(only.counts, full.counts)
        assert torch.equal(full.counts[:, 1:].sum(1).to(torch.int32), hipops.edit_distance(*args))
        assert torch.equal(full.counts.sum(1).to(torch.int32), full.n_ops)


@pytest.mark.parametrize("vocab", [1, 29, 64])
def test_confusion_matrix(vocab):
    """Equals the reference, accumulates across two calls, and symbols outside [0, vocab) -- negative ones too -- are counted in
    counts but stay out of the matrix."""
    hipops = _ops()
    rng = np.random.default_rng(100 + vocab)
    cases = []
    for n, m in ((40, 33), (33, 40), (64, 64), (130, 90), (90, 130), (0, 7), (7, 0), (0, 0), (300, 280)):
        ref, hyp = C._rows(rng, vocab + 3, n, m)
        cases.append(([s - 1 for s in ref], [s - 1 for s in hyp]))          # symbols -1 .. vocab + 1
    packed = C.pack(cases)
    counts, ops, n_ops, cm = R.batch(*packed, vocab=vocab)
    assert 0 < cm.sum() < n_ops.sum()                     # some operations are outside the matrix
    dev_cm = torch.zeros(vocab + 1, vocab + 1, dtype=torch.int64, device=DEV)
    eo = hipops.edit_ops(*[_i32(a) for a in packed], confusion=dev_cm, vocab=vocab)
    _check(eo, (counts, ops, n_ops, None))
    assert np.array_equal(dev_cm.cpu().numpy(), cm)
    hipops.edit_ops(*[_i32(a) for a in packed], want_ops=False, confusion=dev_cm, vocab=vocab)
    assert np.array_equal(dev_cm.cpu().numpy(), 2 * cm)


def test_confusion_of_the_tie_cases(tie_batch):
    packed, want = tie_batch
    cm = torch.zeros(30, 30, dtype=torch.int64, device=DEV)
    _ops().edit_ops(*[_i32(a) for a in packed], confusion=cm, vocab=29)
    assert np.array_equal(cm.cpu().numpy(), want[3])


def test_chunking_gives_the_same_bits(tie_batch):
    hipops = _ops()
    packed, want = tie_batch
    args = [_i32(a) for a in packed]
    per_pair = hipops.edit_ops_workspace_bytes(packed[0].shape[1], packed[2].shape[1], 1)
    N = packed[0].shape[0]
    for pairs in (1, 5, N - 1):
        cm = torch.zeros(30, 30, dtype=torch.int64, device=DEV)
        eo = hipops.edit_ops(*args, confusion=cm, vocab=29, max_workspace_bytes=pairs * per_pair + 3)
        _check(eo, want)
        assert np.array_equal(cm.cpu().numpy(), want[3])
    with pytest.raises(hipops._lib.PgasrError):
        hipops.edit_ops(*args, max_workspace_bytes=per_pair - 1)


def test_words_against_str_split():
    """word_edit_ops against the reference on str.split(" ") of the decoded rows: leading, trailing and double delimiters."""
    hipops = _ops()
    texts = [("ab cd ab", "ab ab cd"), (" ab  cd ", "ab cd"), ("a b c d e", "a c d e f"), ("", "a b"), ("a b", ""), ("  ", " "),
             ("ab cd ef gh", "ab xx ef gh yy"), ("x", "x"), ("the cat sat", "the the cat"), ("b a", "a b")]
    sym = {ch: i + 1 for i, ch in enumerate("abcdefghijklmnopqrstuvwxyz")}
    sym[" "] = 0
    enc = [([sym[c] for c in r], [sym[c] for c in h]) for r, h in texts]
    ref, rl, hyp, hl = C.pack(enc)          # padded with symbols of the rows, delimiters among them
    wo = hipops.word_edit_ops(_i32(ref), _i32(rl), _i32(hyp), _i32(hl), 0)
    counts, ops, n_ops = wo.counts.cpu().numpy(), wo.ops.cpu().numpy(), wo.n_ops.cpu().numpy()
    for k, (r, h) in enumerate(texts):
        rw, hw = r.split(" "), h.split(" ")
        c, o = R.edit_ops(rw, hw)
        assert counts[k].tolist() == c and n_ops[k] == len(o), (r, h)
        assert ops[k, :len(o)].tolist() == o and (ops[k, len(o):] == -1).all()
        assert int(wo.ref_words[k]) == len(rw) and int(wo.hyp_words[k]) == len(hw)
    from policy_gradient_asr_amd import metrics
    cc, wc = metrics.error_counts(_i32(ref), _i32(rl), _i32(hyp), _i32(hl), 0)
    assert torch.equal(wc, wo.counts)
    assert cc.cpu().numpy().tolist() == [R.edit_ops(a, b)[0] for a, b in enc]
    got = metrics.edit_ops_batch([r for r, _ in texts] + [r.split(" ") for r, _ in texts], [h for _, h in texts] + [h.split(" ") for _, h in texts])
    for k, (r, h) in enumerate(texts):
        c, o = R.edit_ops(r, h)
        assert got[k] == (*c, o)
        c, o = R.edit_ops(r.split(" "), h.split(" "))
        assert got[len(texts) + k] == (*c, o)


def test_refusals_launch_nothing():
    """A stride of 4096 and a too-small workspace return their status codes; outputs stay untouched."""
    hipops = _ops()
    lib = hipops._lib.load()
    one = _i32([1])
    with pytest.raises(hipops._lib.PgasrError, match="status 4"):
        hipops.edit_ops(_i32(np.ones((1, 4096))), one, _i32(np.ones((1, 10))), one)
    with pytest.raises(hipops._lib.PgasrError, match="status 4"):
        hipops.edit_ops(_i32(np.ones((1, 10))), one, _i32(np.ones((1, 4096))), one)
    ref, hyp = _i32(np.ones((2, 100))), _i32(np.ones((2, 90)))
    ln = _i32([100, 90])
    counts = torch.full((2, 4), -7, dtype=torch.int32, device=DEV)
    ops = torch.full((2, 190), 55, dtype=torch.int8, device=DEV)
    n_ops = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    need = hipops.edit_ops_workspace_bytes(100, 90, 2)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(ws_ptr, ws_bytes, vocab=0, cm=0, n_ops_ptr=n_ops.data_ptr(), N=2):
        return lib.pgasr_edit_ops(ref.data_ptr(), ln.data_ptr(), 100, hyp.data_ptr(), ln.data_ptr(), 90, N, counts.data_ptr(),
                                  ops.data_ptr(), n_ops_ptr, cm, vocab, ws_ptr, ws_bytes, stream)
    assert call(ws.data_ptr(), need - 1) == 3 and call(0, need) == 3
    assert call(ws.data_ptr(), need, n_ops_ptr=0) == 1 and call(ws.data_ptr(), need, N=0) == 1
    cm = torch.zeros(66, 66, dtype=torch.int64, device=DEV)
    assert call(ws.data_ptr(), need, vocab=65, cm=cm.data_ptr()) == 4 and call(ws.data_ptr(), need, vocab=0, cm=cm.data_ptr()) == 1
    torch.cuda.synchronize()
    assert (counts == -7).all() and (ops == 55).all() and (n_ops == -7).all() and (cm == 0).all()
    assert call(ws.data_ptr(), need) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [[90, 0, 10, 0], [90, 0, 0, 0]] and n_ops.tolist() == [100, 90]
    # over the dirty buffer: the string, then -1 to the end of the row
    assert ops[0].tolist() == [2] * 10 + [0] * 90 + [-1] * 90 and ops[1].tolist() == [0] * 90 + [-1] * 100


# ---- ErrorReport and predict(error_report=True) ----

def _reference_totals(pairs):
    """Sums of the per-utterance reference counts over characters and over str.split(" ") words."""
    ch, wd = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    for ref, hyp in pairs:
        ch += R.edit_ops(ref, hyp)[0]
        wd += R.edit_ops(ref.split(" "), hyp.split(" "))[0]
    return ch, wd


def _totals_line(tag, t):
    h, s, d, i = (int(x) for x in t)
    return "%{} {:.2f} [ {} / {}, {} ins, {} del, {} sub ]".format(tag, 100.0 * (s + d + i) / max(h + s + d, 1), s + d + i, h + s + d, i, d, s)


def test_error_report(tmp_path):
    from policy_gradient_asr_amd.metrics import ErrorReport
    alphabet = ["<pad>", "a", "b", "c", "d", " "]
    pairs = [("ab cd ab", "ab ab cd"), ("a b c d", "a c d d"), ("dab", "dab"), ("ab  cd", "ab cd"), ("", "a"), ("abc", ""),
             ("bad cab", "bad dab cab"), ("a!b", "ab")]
    rep = ErrorReport(alphabet, " ", device=DEV)
    rep.add([p[0] for p in pairs[:5]], [p[1] for p in pairs[:5]])
    rep.add([p[0] for p in pairs[5:]], [p[1] for p in pairs[5:]])
    ch, wd = _reference_totals(pairs)
    s = rep.summary()
    assert s["utterances"] == len(pairs)
    assert [s["char"][k] for k in ("hits", "sub", "del", "ins")] == ch.tolist() and s["char"]["ref"] == sum(len(p[0]) for p in pairs)
    assert [s["word"][k] for k in ("hits", "sub", "del", "ins")] == wd.tolist()
    assert s["cer"] == ch[1:].sum() / (ch[0] + ch[1] + ch[2]) and s["wer"] == wd[1:].sum() / (wd[0] + wd[1] + wd[2])
    # the character confusion matrix on the device against the reference ("!" is outside the alphabet: counted, not entered)
    sym = {c: i for i, c in enumerate(alphabet)}
    cm = np.zeros((7, 7), dtype=np.int64)
    for ref, hyp in pairs:
        r, h = [sym.get(c, 99) for c in ref], [sym.get(c, 99) for c in hyp]
        R.confusion_add(cm, r, h, R.edit_ops(r, h)[1], 6)
    assert np.array_equal(rep.confusion.cpu().numpy(), cm) and cm.sum() == ch.sum() - 1
    rows = rep.confusions()
    assert [r[3] for r in rows] == sorted((r[3] for r in rows), reverse=True)
    assert ("word_ins", "", "dab", 1) in rows and ("char_del", "c", "", int(cm[3, 6])) in rows
    rep.write(str(tmp_path))
    text = open(tmp_path / "errors.txt").read().splitlines()
    assert text[-2:] == [_totals_line("CER", ch), _totals_line("WER", wd)]
    k = text.index("REF: ab CD AB")                  # two substituted words, in upper case
    assert text[k - 1] == "utt 0  char H/S/D/I {} {} {} {}  word H/S/D/I 1 2 0 0".format(*R.edit_ops(*pairs[0])[0])
    assert text[k + 1:k + 3] == ["HYP: ab AB CD", "OPS:    S  S"]
    k = text.index("REF: bad *** cab")               # an inserted word: a run of * on the reference side
    assert text[k + 1:k + 3] == ["HYP: bad dab cab", "OPS:     I"]
    assert sum(1 for ln in text if ln.startswith("REF:")) == len(pairs) == sum(1 for ln in text if ln.startswith("OPS:"))
    tsv = open(tmp_path / "confusions.tsv").read().splitlines()
    assert tsv[0] == "kind\tref\thyp\tcount" and len(tsv) == 1 + len(rows)
    assert [ln.split("\t") for ln in tsv[1:]] == [[r[0], r[1], r[2], str(r[3])] for r in rows]


def test_aligned_lines_are_padded_columns():
    from policy_gradient_asr_amd.metrics import _aligned_lines
    ref, hyp = "the cat sat".split(" "), "the the cat".split(" ")
    assert R.edit_ops(ref, hyp)[1] == [0, 1, 1]                 # the diagonal first: two substitutions
    assert _aligned_lines(ref, hyp, [0, 1, 1]) == ("the CAT SAT", "the THE CAT", "    S   S")
    # another alignment of the pair, for the gap columns
    assert _aligned_lines(ref, hyp, [0, 3, 0, 2]) == ("the *** cat sat", "the the cat ***", "    I       D")


def test_predict_error_report(tmp_path, capsys):
    """predict(error_report=True) on the tiny synthetic dataset of tests/test_drivers_gpu.py: both files exist, the totals line is
    the sum of the reference's per-utterance counts over predicted.txt, and everything else is what the default call gives."""
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.model import Seq2Seq, predict
    corpus = tmp_path / "corpus"; out = tmp_path / "run"
    corpus.mkdir(); out.mkdir()
    (corpus / "alphabet.txt").write_text("a\nb\nc\nd\n \n")
    char2ind = {"<pad>": 0, "a": 1, "b": 2, "c": 3, "d": 4, " ": 5}
    dv = SyntheticSpeech(16, char2ind, n_feats=20, seed=2)
    torch.manual_seed(5)
    torch.save(Seq2Seq(alphabet_size=6, n_feats=20).state_dict(), out / "model_best.pth")
    base = predict(None, None, str(corpus / "alphabet.txt"), str(out), 8, test_dataset=dv, n_feats=20)
    base_lines = open(out / "predicted.txt").read()
    assert not os.path.exists(out / "errors.txt") and not os.path.exists(out / "confusions.tsv")
    base_out = capsys.readouterr().out
    got = predict(None, None, str(corpus / "alphabet.txt"), str(out), 8, test_dataset=dv, n_feats=20, error_report=True)
    new_out = capsys.readouterr().out
    assert got == base and open(out / "predicted.txt").read() == base_lines
    assert os.path.exists(out / "errors.txt") and os.path.exists(out / "confusions.tsv")
    pairs = [tuple(ln.split("|")) for ln in base_lines.splitlines()]
    assert len(pairs) == 16
    ch, wd = _reference_totals(pairs)
    text = open(out / "errors.txt").read().splitlines()
    assert text[-2:] == [_totals_line("CER", ch), _totals_line("WER", wd)]
    assert new_out.splitlines()[:-1] == base_out.splitlines()
    assert new_out.splitlines()[-1] == "Corpus " + "  ".join(text[-2:])
