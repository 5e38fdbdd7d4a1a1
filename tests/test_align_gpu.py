"""CTC forced alignment on the device against the numpy fp64 statement (tests/align_ref.py).  Every comparison is EXACT: the
arithmetic is fp64 max-plus in a fixed order, so any difference is a bug."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import align_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _i32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.int32).to(DEV).contiguous()


def _run(lp, tokens, il, tl, blank=0):
    from policy_gradient_asr_amd import hipops
    return hipops.ctc_forced_align(lp.to(DEV).contiguous(), _i32(tokens), _i32(il), _i32(tl), blank=blank)


def _assert_equal(a, r):
    """device CTCAlignment == reference, bit for bit, padding included"""
    assert np.array_equal(a.score.cpu().numpy(), r.score), (a.score.cpu().numpy(), r.score)
    assert np.array_equal(a.frame_label.cpu().numpy(), r.frame_label)
    assert np.array_equal(a.frame_token.cpu().numpy(), r.frame_token)
    assert np.array_equal(a.token_start.cpu().numpy(), r.token_start)
    assert np.array_equal(a.token_end.cpu().numpy(), r.token_end)
    assert np.array_equal(a.token_logp.cpu().numpy(), r.token_logp)
    assert a.score.dtype == torch.float64 and a.token_logp.dtype == torch.float64 and a.frame_label.dtype == torch.int32


@functools.lru_cache(maxsize=None)
def _variant_case(L):
    """B = 3 ragged utterances of up to L tokens over T = 2L + 40 frames, V = 29: (inputs, device result, reference)"""
    T, B, V = 2 * L + 40, 3, 29
    g = torch.Generator().manual_seed(100 + L)
    lp = torch.log_softmax(torch.randn(T, B, V, generator=g), 2)
    tokens = torch.randint(1, V, (B, L), generator=g).numpy()
    il, tl = np.array([T, T - 5, T - 13]), np.array([L, L - 7, L // 2])
    a = _run(lp, tokens, il, tl)
    r = R.align_batch(lp.numpy(), tokens, il, tl)
    return lp, tokens, il, tl, a, r


@pytest.mark.parametrize("L", [100, 200, 400, 600])       # 1, 2, 4 and 8 lattice states per thread
def test_states_per_thread_variants(L):
    lp, tokens, il, tl, a, r = _variant_case(L)
    assert np.isfinite(r.score).all()
    _assert_equal(a, r)


@pytest.mark.parametrize("L", [100, 200, 400, 600])
def test_invariants_against_existing_kernels(L):
    from policy_gradient_asr_amd import hipops
    lp, tokens, il, tl, a, _ = _variant_case(L)
    B, T = a.frame_label.shape
    # the alignment collapses to the transcript
    tok, n = hipops.ctc_collapse(a.frame_label.t()[None].contiguous(), _i32(il), blank=0)
    tok, n = tok[0].cpu().numpy(), n[0].cpu().numpy()
    for b in range(B):
        assert n[b] == tl[b] and np.array_equal(tok[b, :n[b]], tokens[b, :tl[b]])
    # best path <= sum over paths: score >= nll, up to the lattice's documented fp32-transcendental error
    nll, _ = hipops.ctc_lattice(lp.to(DEV).contiguous(), _i32(tokens), _i32(il), _i32(tl), blank=0)
    score, nll = a.score.cpu().numpy(), nll.cpu().numpy().astype(np.float64)
    print("score - nll:", score - nll)
    assert (score - nll >= -1e-4 * np.maximum(1.0, nll)).all()
    # spans ascending and disjoint; together they are the non-blank frames
    st, en, ft = a.token_start.cpu().numpy(), a.token_end.cpu().numpy(), a.frame_token.cpu().numpy()
    for b in range(B):
        s, e = st[b, :tl[b]], en[b, :tl[b]]
        assert (s >= 0).all() and (e > s).all() and (s[1:] >= e[:-1]).all() and e[-1] <= il[b]
        assert int((e - s).sum()) == int((ft[b] >= 0).sum())


def test_edge_batch():
    T, B, V, Lmax = 24, 8, 5, 6
    g = torch.Generator().manual_seed(5)
    lp = torch.log_softmax(torch.randn(T, B, V, generator=g), 2)
    tokens = np.zeros((B, Lmax), np.int64)
    tokens[1, :2] = [1, 2]
    tokens[3, :1] = [4]
    tokens[4, :3] = [1, 1, 1]               # needs 5 frames
    tokens[5, :3] = [1, 1, 1]
    tokens[6] = [3, 3, 1, 4, 2, 2]
    tokens[7, :4] = [2, 9, -3, 3]           # labels outside [0,V): aligned as blanks
    #              no frames  no frames  all blank  one frame  too short  exact fit  clamped lengths  bad labels
    il = np.array([0,         0,         10,        1,         4,         5,         30,              12])
    tl = np.array([0,         2,         0,         1,         3,         3,         9,               4])
    a = _run(lp, tokens, il, tl)
    r = R.align_batch(lp.numpy(), tokens, il, tl)
    _assert_equal(a, r)
    s = a.score.cpu().numpy()
    assert s[0] == 0.0 and s[1] == np.inf and s[4] == np.inf and np.isfinite(s[[2, 3, 5, 6, 7]]).all()
    fl, ft = a.frame_label.cpu().numpy(), a.frame_token.cpu().numpy()
    assert (fl[[0, 1, 4]] == -1).all() and (ft[[0, 1, 4]] == -1).all()            # nothing to report
    assert (fl[2, :10] == 0).all() and (fl[2, 10:] == -1).all() and fl[3, 0] == 4
    assert fl[5, :5].tolist() == [1, 0, 1, 0, 1] and (fl[6] >= 0).all()
    assert (a.token_start.cpu().numpy()[4] == -1).all() and (a.token_logp.cpu().numpy()[4] == 0).all()
    assert a.token_start.cpu().numpy()[5, :3].tolist() == [0, 2, 4] and a.token_end.cpu().numpy()[5].tolist() == [1, 3, 5, -1, -1, -1]
    assert ft[7, :12].max() == 3 and set(fl[7, :12].tolist()) <= {0, 2, 3}
    # want_spans=False: the same score and frame labels, nothing else
    from policy_gradient_asr_amd import hipops
    b = hipops.ctc_forced_align(lp.to(DEV).contiguous(), _i32(tokens), _i32(il), _i32(tl), want_spans=False)
    assert torch.equal(b.score, a.score) and torch.equal(b.frame_label, a.frame_label) and b.token_start is None


def test_tie_rule_on_the_device():
    """the literal paths of tests/test_align_cpu.py: uniform rows, the smallest move wins every tie"""
    lp = torch.full((7, 2, 3), -math.log(3.0), dtype=torch.float32)
    a = _run(lp, [[1, 2], [1, 1]], [7, 7], [2, 2])
    assert a.frame_label.cpu().tolist() == [[1, 2, 0, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0, 0]]
    _assert_equal(a, R.align_batch(lp.numpy(), np.array([[1, 2], [1, 1]]), [7, 7], [2, 2]))


@pytest.mark.parametrize("V,blank", [(6, 5), (64, 0)])
def test_other_blank_and_widest_alphabet(V, blank):
    T, B, L = 30, 2, 8
    g = torch.Generator().manual_seed(V)
    lp = torch.log_softmax(torch.randn(T, B, V, generator=g), 2)
    tokens = torch.randint(0 if blank else 1, V - 1 if blank else V, (B, L), generator=g).numpy()
    il, tl = [T, T - 4], [L, L - 3]
    a = _run(lp, tokens, il, tl, blank=blank)
    r = R.align_batch(lp.numpy(), tokens, il, tl, blank=blank)
    assert np.isfinite(r.score).all()
    _assert_equal(a, r)


def test_greedy_identity_at_the_headline_size():
    """The best path of all is the per-frame arg-max, and it is an alignment of its own collapse: aligning the greedy hypotheses
    must give back the arg-max labels and -sum_t max lp (added in ascending t).  Runs the 8-states-per-thread variant and the
    backtrace at its longest."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.CTCdecoder import greedy_decode
    T, B, V = 1000, 32, 29
    lp = torch.log_softmax(torch.randn(T, B, V, generator=torch.Generator().manual_seed(1234)), 2)
    top = lp.topk(2, dim=2).values
    assert float((top[..., 0] - top[..., 1]).min()) > 0.0            # every frame's maximum is unique
    lpd = lp.to(DEV).contiguous()
    hyp, hl = greedy_decode(lpd)
    assert int(hl.max()) <= hipops.ALIGN_MAX_TOKENS and int(hl.min()) > 0      # every hypothesis fits (912 .. 945 tokens)
    il = torch.full((B,), T, dtype=torch.int32, device=DEV)
    a = hipops.ctc_forced_align(lpd, hyp[:, :hipops.ALIGN_MAX_TOKENS].contiguous(), il, hl.contiguous())
    assert torch.equal(a.frame_label.cpu(), lp.argmax(2).t().to(torch.int32))
    want = -np.cumsum(top[..., 0].double().numpy(), axis=0)[-1]                 # (B), sequential over t
    assert np.array_equal(a.score.cpu().numpy(), want)
    # every token's span is one run of its label, and the spans' log-probs add up to the non-blank part of the score
    ft = a.frame_token.cpu().numpy()
    assert (np.diff(ft, axis=1)[(ft[:, 1:] >= 0) & (ft[:, :-1] >= 0)] >= 0).all()
    assert int(ft.max()) == int(hl.max()) - 1


def test_model_align(tmp_path):
    """model.align on a tiny synthetic corpus: alignments.tsv with one line per reference character, spans inside the utterance"""
    from pg_harness import tiny_corpus
    from policy_gradient_asr_amd.model import Seq2Seq, align
    corpus, out, ds = tiny_corpus(tmp_path, n=16)
    out.mkdir()
    torch.manual_seed(0)
    torch.save(Seq2Seq(alphabet_size=6, n_feats=20).state_dict(), out / "model_best.pth")
    scores = align(None, None, str(corpus / "alphabet.txt"), str(out), 8, test_dataset=ds, n_feats=20)
    assert len(scores) == 16 and all(math.isfinite(s) and s > 0 for s in scores)
    path = out / "alignments.tsv"
    assert os.path.exists(path)
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    assert len(rows) == sum(len(it["trans"]) for it in ds.items)
    k = 0
    for u, it in enumerate(ds.items):
        frames, prev_end = it["feat"].shape[1], 0
        for j, ch in enumerate(it["trans"]):
            uu, jj, sym, s0, s1, mean = rows[k]; k += 1
            assert (int(uu), int(jj), sym) == (u, j, ch)
            assert prev_end <= int(s0) < int(s1) <= frames and float(mean) <= 0.0
            prev_end = int(s1)
