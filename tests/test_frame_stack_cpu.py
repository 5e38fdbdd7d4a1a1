"""Low-frame-rate input without a GPU: the numpy statement (tests/frame_stack_ref.py) against plain loops, the FrameStack policy
object, its feasibility test against a brute-force CTC check, and the proof that the corpus of the driver test loses no utterance."""
import itertools

import numpy as np
import pytest
import torch

import frame_stack_ref as R
from policy_gradient_asr_amd import hipops
from policy_gradient_asr_amd.features import FrameStack

POLICIES = [(1, 1, 0), (2, 2, 0), (3, 3, 0), (3, 3, 1), (7, 3, 3), (8, 3, 7), (4, 1, 2), (2, 5, 0), (16, 16, 15)]


def _case(B, F, T, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, F, T)).astype(np.float32)
    n = g.integers(0, T + 1, size=B)
    n[0], n[-1] = T, 0
    return x, n


@pytest.mark.parametrize("policy", POLICIES)
def test_reference_equals_the_plain_loops(policy):
    stack, skip, left = policy
    for F, T in ((1, 1), (3, 7), (2, 19)):
        x, n = _case(4, F, T, seed=F * 100 + T)
        out, fmask, n_out = R.frame_stack_ref(x, n, stack, skip, left)
        assert out.shape == (4, stack * F, -(-T // skip)) and out.dtype == np.float32
        assert R.same_bits(out, R.frame_stack_loops(x, n, stack, skip, left))
        assert list(n_out) == [-(-int(v) // skip) for v in n]
        assert np.array_equal(fmask[:, 0, :], (np.arange(out.shape[2])[None, :] < n_out[:, None]).astype(np.float32))


def test_identity_policy_zeroes_the_padding():
    x, n = _case(5, 4, 11, seed=3)
    x[1, :, n[1]:] = np.nan                       # padding is never read into a written value
    out, fmask, n_out = R.frame_stack_ref(x, n, 1, 1, 0)
    want = x.copy()
    for b in range(5):
        want[b, :, n[b]:] = 0.0
    assert R.same_bits(out, want) and list(n_out) == list(n)
    assert np.array_equal(fmask[:, 0, :].sum(1), n)


def test_skip_one_keeps_the_lengths_and_replicates_the_edges():
    x, n = _case(3, 2, 9, seed=5)
    n[1] = 2                                      # stack > n: every tap is clamped to frames 0 and 1
    out, _, n_out = R.frame_stack_ref(x, n, 4, 1, 2)
    assert list(n_out) == list(n)
    assert np.array_equal(out[0, 0:2, 0], x[0, :, 0]) and np.array_equal(out[0, 2:4, 0], x[0, :, 0])      # taps -2, -1 -> frame 0
    assert np.array_equal(out[0, 6:8, 8], x[0, :, 8])                                                      # tap 9 -> frame 8
    assert np.array_equal(out[1, :, 0], np.concatenate([x[1, :, 0]] * 3 + [x[1, :, 1]]))
    assert np.array_equal(out[1, :, 1], np.concatenate([x[1, :, 0]] * 2 + [x[1, :, 1]] * 2))
    assert not out[1, :, 2:].any()


def test_fits_is_ctc_feasibility():
    """L + repeats <= n' against the brute-force reachability check, for every transcript of 1 .. 4 symbols over {1, 2} and every
    frame count 0 .. 8; the padding (id 0) is not counted as a repeat."""
    fs = FrameStack(3, 3, 0)
    rows, lens, frames, want = [], [], [], []
    for L in range(1, 5):
        for labels in itertools.product((1, 2), repeat=L):
            for n in range(0, 9):
                rows.append(list(labels) + [0] * (5 - L)); lens.append(L); frames.append(n)
                want.append(R.ctc_feasible(labels, n))
    trans = torch.tensor(rows)
    got = fs.fits(trans, torch.tensor(lens), torch.tensor(frames, dtype=torch.int32))
    assert got.dtype == torch.bool and got.tolist() == want
    assert any(want) and not all(want)
    assert fs.fits(trans, None, torch.tensor(frames)).tolist() == want          # lengths from the ids != blank


def test_policy_object():
    fs = FrameStack()
    assert (fs.stack, fs.skip, fs.left) == (3, 3, 0) and fs.state() == {"stack": 3, "skip": 3, "left": 0}
    assert FrameStack.from_state(fs.state()) == fs and hash(FrameStack(3, 3)) == hash(fs)
    assert FrameStack(8, 3, 7) != fs and fs != (3, 3, 0)
    assert repr(FrameStack(8, 3, 7)) == "FrameStack(stack=8, skip=3, left=7)"
    assert FrameStack.coerce(None) is None and FrameStack.coerce(fs) is fs
    assert FrameStack.coerce((8, 3)) == FrameStack(8, 3, 0) and FrameStack.coerce([8, 3, 7]) == FrameStack(8, 3, 7)
    assert FrameStack.coerce({"stack": 2, "skip": 2, "left": 1}) == FrameStack(2, 2, 1)
    assert fs.out_feats(80) == 240 and [fs.out_frames(n) for n in (0, 1, 3, 4, 1000)] == [0, 1, 1, 2, 334]
    assert fs.out_frames(torch.tensor([0, 1, 3, 4])).tolist() == [0, 1, 1, 2]
    with pytest.raises(AttributeError, match="immutable"):
        fs.stack = 4
    with pytest.raises(AttributeError, match="immutable"):
        del fs.skip
    for bad in ((0, 1, 0), (17, 1, 0), (3, 0, 0), (3, 17, 0), (3, 3, -1), (3, 3, 3)):
        with pytest.raises(ValueError, match="stack|skip|left"):
            FrameStack(*bad)
    for bad in ((3.0, 3, 0), (3, True, 0), (3, 3, "0")):
        with pytest.raises(TypeError, match="integer"):
            FrameStack(*bad)
    with pytest.raises(ValueError, match="unknown fields"):
        FrameStack.from_state({"stack": 3, "skip": 3, "left": 0, "right": 1})
    for bad in ("3,3", 3, (3,), (3, 3, 0, 0)):
        with pytest.raises(TypeError, match="frame_stack"):
            FrameStack.coerce(bad)


def test_input_span_round_trips():
    """Stacked frame t' is anchored at input frame t'*skip: consecutive stacked spans tile [0, n), and the stacked frames of an input
    span's ends are the span again."""
    for stack, skip, left in POLICIES:
        fs = FrameStack(stack, skip, left)
        for n in (1, 2, skip, skip + 1, 7 * skip - 1, 100):
            m = fs.out_frames(n)
            assert fs.input_span(0, m, n) == (0, n)
            cuts = [0, m // 3, m // 2, m]
            spans = [fs.input_span(a, b, n) for a, b in zip(cuts[:-1], cuts[1:])]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans[:-1], spans[1:]))
            for (s, e), a, b in zip(spans, cuts[:-1], cuts[1:]):
                assert s % skip == 0 and s // skip == a and fs.out_frames(e) == b and e <= n


def test_no_cpu_path():
    from policy_gradient_asr_amd import _lib
    from policy_gradient_asr_amd.data import SyntheticSpeech, collate_custom
    x = torch.zeros(2, 4, 8)
    with pytest.raises(ValueError, match="GPU"):
        hipops.frame_stack(x, stack=3, skip=3)
    with pytest.raises(_lib.PgasrError, match="no CPU path"):
        FrameStack()(x, torch.ones(2, 1, 8))
    ds = SyntheticSpeech(2, {"<pad>": 0, "a": 1, "b": 2}, n_feats=4, seed=0)
    with pytest.raises(ValueError, match="frame_stack"):
        collate_custom([ds[0], ds[1]], frame_stack=(3, 3))
    assert collate_custom([ds[0], ds[1]])["feat"].shape[1] == 4          # the CPU contract without it: as ever


def test_driver_arguments_exist():
    import inspect
    from policy_gradient_asr_amd import model
    for fn in (model.train, model.predict, model.align):
        assert inspect.signature(fn).parameters["frame_stack"].default is None
    assert "pgasr_frame_stack" in __import__("policy_gradient_asr_amd._lib", fromlist=["SIGNATURES"]).SIGNATURES


def test_the_driver_corpus_loses_no_utterance(tmp_path):
    """Every utterance of the driver test's corpus still fits under its policy, so that test cannot pass by dropping data: checked
    with ``fits`` AND with the brute-force alignment check, on the frame counts the policy gives."""
    from pg_harness import tiny_corpus
    fs = FrameStack(*R.DRIVER_POLICY)
    _, _, ds = tiny_corpus(tmp_path, R.DRIVER_UTTERANCES)
    assert len(ds) == R.DRIVER_UTTERANCES
    Lmax = max(len(ds[i]["trans"]) for i in range(len(ds)))
    trans = torch.zeros(len(ds), Lmax, dtype=torch.int64)
    lens, frames = [], []
    for i in range(len(ds)):
        item = ds[i]
        ids = [item["charmap"][c] for c in item["trans"]]
        trans[i, :len(ids)] = torch.tensor(ids)
        lens.append(len(ids)); frames.append(fs.out_frames(item["feat"].shape[1]))
        assert item["feat"].shape[1] >= 4 * len(ids)                     # 4 .. 8 frames per character
        assert R.ctc_feasible(ids, frames[-1])
    fit = fs.fits(trans, torch.tensor(lens), torch.tensor(frames))
    assert int((~fit).sum()) == 0
    assert not all(fs.fits(trans, torch.tensor(lens), torch.tensor(frames) // 4).tolist())      # the check can fail: it does at n'/4
