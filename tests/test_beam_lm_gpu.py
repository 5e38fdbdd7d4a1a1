"""Language-model fusion of the CTC prefix beam search on the device (csrc/beam.hip, LM = true) against the plain-Python fused
search of tests/beam_lm_ref.py: hypotheses token for token; scores to 1e-9 relative on the exact (fp64) path and 1e-6 on the fp32
path, whose cases carry a margin condition (tests/test_beam_lm_cpu.py); zero weights and no table against the search as it was."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lm(table, order, blank=0):
    from policy_gradient_asr_amd.lm import CharNgramLM
    return CharNgramLM(table, order, blank=blank)


# (T, V, beam, order, blank, alpha, beta, exact zeros)
EXACT_CASES = [
    (60, 4, 16, 1, 0, 1.0, 0.5, False),
    (50, 29, 5, 2, 0, 0.5, 0.0, False),
    (120, 29, 16, 3, 0, 0.7, 1.2, True),
    (40, 29, 100, 3, 0, 0.5, 1.0, False),
    (25, 29, 128, 2, 0, 0.8, 0.3, True),
    (300, 29, 5, 4, 0, 0.4, 0.8, False),
    (60, 48, 16, 3, 0, 0.6, 0.6, False),
    (30, 64, 5, 4, 63, 0.3, 0.9, False),
    (40, 64, 16, 2, 5, 1.0, 0.0, True),
    (80, 29, 1, 3, 0, 0.5, 0.5, False),
    (20, 4, 128, 4, 2, 0.9, 0.4, False),
    (1, 29, 16, 3, 0, 0.8, 0.5, False),
]


@pytest.mark.parametrize("T,V,beam,order,blank,alpha,beta,zeros", EXACT_CASES)
def test_exact_path_matches_the_fused_reference(T, V, beam, order, blank, alpha, beta, zeros):
    """CTCDecoder.decode on fp64 probabilities: tokens identical, score 1e-9 relative (fp64 device math; no margin condition)."""
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    rng = np.random.default_rng(7 * T + V + beam + order)
    logits = rng.normal(size=(T, V)) * rng.choice([0.3, 2.0, 5.0], size=(T, 1))
    logits[:, blank] += 1.5
    probs = np.exp(logits - logits.max(axis=1, keepdims=True))
    if zeros and T >= 8:
        probs[3, [s for s in range(V) if s != blank][:2]] = 0.0            # zero probabilities (log p = -inf)
        probs[5, :] = 0.0; probs[5, (blank + 2) % V] = 1.0
    probs = probs / probs.sum(axis=1, keepdims=True)
    table = R.random_table(V, order, blank, seed=T + order)
    dec = CTCDecoder(list(range(V)), lm=_lm(table, order, blank), lm_alpha=alpha, lm_beta=beta)
    got, score = dec.decode(probs, beam_size=beam, blank=blank)
    want, wscore, gap = R.fused_prefix_beam_search(probs, table, order, alpha, beta, beam_size=beam, blank=blank)
    print(f"exact T={T} V={V} beam={beam} order={order}: score {score!r} reference {wscore!r} gap {gap:.3e}")
    assert got == want
    assert score == pytest.approx(wscore, rel=1e-9)
    # a per-call override: lm=None is the acoustic search
    plain, pscore = dec.decode(probs, beam_size=beam, blank=blank, lm=None)
    assert (plain, pytest.approx(pscore, rel=1e-9)) == R.fused_prefix_beam_search(probs, None, 0, 0, 0, beam_size=beam, blank=blank)[:2]


@pytest.mark.parametrize("case", R.FAST_CASES, ids=lambda c: "T%d-V%d-K%d-n%d-b%d-s%d" % (c[0], c[1], c[2], c[3], c[4], c[7]))
def test_fast_path_matches_the_fused_reference(case):
    """decode_batch on fp32 log-probs with ragged lengths (0 and 1 among them): tokens identical, score 1e-6 relative; the
    collapse=True output is the plain output with adjacent duplicates removed."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    T, V, beam, order, blank, alpha, beta, seed = case
    lp, lens, table = R.fast_case_inputs(case)
    lm = _lm(table, order, blank)
    d_lp, d_len = torch.from_numpy(lp).to(DEV), torch.from_numpy(lens).to(DEV)
    dec = CTCDecoder(list(range(V)), lm=lm, lm_alpha=alpha, lm_beta=beta)
    tok, tl, score = dec.decode_batch(d_lp, d_len, beam_size=beam, blank=blank)
    ctok, ctl, cscore = hipops.ctc_beam_search(d_lp, d_len, beam=beam, blank=blank, collapse=True, lm=lm, lm_alpha=alpha, lm_beta=beta)
    assert torch.equal(score, cscore)
    for b in range(R.FAST_B):
        n = int(lens[b])
        want, wscore, gap = R.fused_prefix_beam_search(logp=lp[:n, b].astype(np.float64), table=table, order=order, alpha=alpha,
                                                       beta=beta, beam_size=beam, blank=blank)
        got = list(tok[b, :tl[b]].cpu().numpy())
        print(f"fast {case} b={b} n={n}: score {float(score[b])!r} reference {wscore!r} gap {gap:.3e}")
        assert got == list(want), (b, n)
        assert float(score[b]) == pytest.approx(wscore, rel=1e-6), (b, n)
        assert int(tok[b, tl[b]:].abs().sum()) == 0
        dedup = [x for i, x in enumerate(got) if i == 0 or x != got[i - 1]]
        assert list(ctok[b, :ctl[b]].cpu().numpy()) == dedup
        assert int(ctok[b, ctl[b]:].abs().sum()) == 0


@pytest.mark.parametrize("T,B,V,beam,order,blank", [(120, 4, 29, 16, 3, 0), (80, 3, 64, 5, 2, 63), (200, 3, 29, 100, 3, 0), (60, 4, 4, 16, 4, 0)])
def test_zero_weights_are_the_search_without_lm_bit_for_bit(T, B, V, beam, order, blank):
    """alpha = beta = 0 with a table: x + 0.0 == x, so tokens, lengths and scores equal the same kernel's without an LM."""
    from policy_gradient_asr_amd import hipops
    rng = np.random.default_rng(T + V)
    lp32 = R.log_softmax32(rng.normal(size=(T, B, V)) * 2.0)
    lens = torch.tensor([T] + [max(0, T - 9 * b) for b in range(1, B)], dtype=torch.int32, device=DEV)
    lm = _lm(R.random_table(V, order, blank, seed=3), order, blank)
    for lp in (torch.from_numpy(lp32).to(DEV), torch.from_numpy(lp32).double().to(DEV)):
        a = hipops.ctc_beam_search(lp, lens, beam=beam, blank=blank, generic=True)
        z = hipops.ctc_beam_search(lp, lens, beam=beam, blank=blank, lm=lm, lm_alpha=0.0, lm_beta=0.0)
        assert torch.equal(a[0], z[0]) and torch.equal(a[1], z[1]) and torch.equal(a[2], z[2])
        w = hipops.ctc_beam_search(lp, lens, beam=beam, blank=blank, lm=lm, lm_alpha=0.5, lm_beta=0.5)
        assert not torch.equal(a[2], w[2])                  # and the weights do reach the kernel


def test_no_table_through_the_new_entry_point_is_the_old_one():
    """lm=None goes through pgasr_ctc_beam_search_lm with a NULL table: the same kernels as pgasr_ctc_beam_search, the single-wave
    dispatch at beam 16 included."""
    from policy_gradient_asr_amd import hipops, _lib
    lib = _lib.load()
    T, B, V, beam = 200, 6, 29, 16
    rng = np.random.default_rng(11)
    lp = torch.from_numpy(R.log_softmax32(rng.normal(size=(T, B, V)) * 2.0)).to(DEV)
    lens = torch.tensor([200, 150, 1, 0, 77, 200], dtype=torch.int32, device=DEV)
    for flags in (0, 1, 2):
        new = hipops.ctc_beam_search(lp, lens, beam=beam, collapse=bool(flags & 1), generic=bool(flags & 2))
        tokens = torch.zeros(B, T, dtype=torch.int32, device=DEV)
        tl = torch.empty(B, dtype=torch.int32, device=DEV)
        score = torch.empty(B, dtype=torch.float64, device=DEV)
        ws = torch.empty(lib.pgasr_beam_workspace_bytes(T, B, V, beam), dtype=torch.uint8, device=DEV)
        st = lib.pgasr_ctc_beam_search(lp.data_ptr(), 0, lp.stride(0), lp.stride(1), lens.data_ptr(), T, B, V, beam, 0, flags,
                                       tokens.data_ptr(), tl.data_ptr(), score.data_ptr(), ws.data_ptr(), ws.numel(),
                                       torch.cuda.current_stream().cuda_stream)
        assert st == 0
        torch.cuda.synchronize()
        assert torch.equal(new[0], tokens) and torch.equal(new[1], tl) and torch.equal(new[2], score)
    # the single-wave kernel and the general one are different code: where they differ in the last bits of a score, the LM-less new
    # entry point must side with the dispatch of the old one
    a = hipops.ctc_beam_search(lp, lens, beam=beam)
    g = hipops.ctc_beam_search(lp, lens, beam=beam, generic=True)
    torch.testing.assert_close(a[2], g[2], rtol=1e-6, atol=1e-6)


def test_constructed_flip():
    """Frames acoustically balanced between symbols 1 and 2 (1 slightly ahead); the LM strongly prefers 2.  The hypothesis changes
    with alpha > 0 and not with alpha = 0 -- on the exact and on the fp32 path, and as the reference search says."""
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    T, V = 9, 3
    probs = np.zeros((T, V))
    probs[:] = [0.9, 0.05, 0.05]
    probs[2] = [0.1, 0.46, 0.44]
    table = np.array([0.0, np.log(0.02), np.log(0.98)], dtype=np.float32)
    lm = _lm(table, 1)
    dec = CTCDecoder(["-", "a", "b"], lm=lm, lm_alpha=0.0, lm_beta=0.0)
    no_lm = CTCDecoder(["-", "a", "b"]).decode(probs, beam_size=8)[0]
    assert no_lm == (1,)
    assert dec.decode(probs, beam_size=8)[0] == no_lm                                   # alpha = 0: unchanged
    assert dec.decode(probs, beam_size=8, lm_alpha=1.0)[0] == (2,)                      # the LM's choice
    assert R.fused_prefix_beam_search(probs, table, 1, 1.0, 0.0, beam_size=8)[0] == (2,)
    lp = torch.from_numpy(np.log(probs)).float().view(T, 1, V).to(DEV)
    t0, l0, _ = dec.decode_batch(lp, None, beam_size=8)
    t1, l1, _ = dec.decode_batch(lp, None, beam_size=8, lm_alpha=1.0)
    assert t0[0, :l0[0]].tolist() == [1] and t1[0, :l1[0]].tolist() == [2]
    # an order-2 LM that only dislikes "a" after "a": the flip happens at the second character
    probs2 = probs.copy(); probs2[6] = probs[2]
    t2 = np.zeros((3, 3), dtype=np.float32); t2[:, 1:] = np.log(0.5); t2[1, 1], t2[1, 2] = np.log(0.02), np.log(0.98)
    d2 = CTCDecoder(["-", "a", "b"], lm=_lm(t2, 2), lm_alpha=1.0)
    assert d2.decode(probs2, beam_size=8, lm_alpha=0.0)[0] == (1, 1)
    assert d2.decode(probs2, beam_size=8)[0] == (1, 2) == R.fused_prefix_beam_search(probs2, t2, 2, 1.0, 0.0, beam_size=8)[0]


def test_headline_shape():
    """T = 1000, B = 32, V = 29, beam 16, order 3: runs, finite scores, two calls bit-identical, and two utterances cut to 150
    frames match the reference search (their margins are checked in tests/test_beam_lm_cpu.py)."""
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    T, B, V, beam, order, blank, alpha, beta, seed = R.HEADLINE
    lp, table = R.headline_inputs()
    dec = CTCDecoder(list(range(V)), lm=_lm(table, order, blank), lm_alpha=alpha, lm_beta=beta)
    d_lp = torch.from_numpy(lp).to(DEV)
    a = dec.decode_batch(d_lp, None, beam_size=beam)
    b = dec.decode_batch(d_lp, None, beam_size=beam)
    assert torch.isfinite(a[2]).all() and (a[1] >= 0).all() and (a[1] <= T).all()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for u in (0, 13, 31):
        seq = a[0][u, :a[1][u]]
        assert ((seq >= 1) & (seq < V)).all()
    cut = torch.from_numpy(np.ascontiguousarray(lp[:R.HEADLINE_CUT][:, list(R.HEADLINE_CHECK)])).to(DEV)
    tok, tl, score = dec.decode_batch(cut, None, beam_size=beam)
    for i, u in enumerate(R.HEADLINE_CHECK):
        want, wscore, gap = R.fused_prefix_beam_search(logp=lp[:R.HEADLINE_CUT, u].astype(np.float64), table=table, order=order,
                                                       alpha=alpha, beta=beta, beam_size=beam, blank=blank)
        print(f"headline utterance {u}: score {float(score[i])!r} reference {wscore!r} gap {gap:.3e}")
        assert list(tok[i, :tl[i]].cpu().numpy()) == list(want)
        assert float(score[i]) == pytest.approx(wscore, rel=1e-6)


def test_lm_must_match_the_search():
    from policy_gradient_asr_amd import hipops
    lp = torch.log_softmax(torch.randn(10, 2, 29, device=DEV), 2)
    with pytest.raises(ValueError):
        hipops.ctc_beam_search(lp, None, beam=5, lm=_lm(R.random_table(28, 2, 0, 0), 2))              # another alphabet
    with pytest.raises(ValueError):
        hipops.ctc_beam_search(lp, None, beam=5, blank=0, lm=_lm(R.random_table(29, 2, 3, 0), 2, 3))  # another blank


def test_predict_with_lm(tmp_path):
    """predict() on a tiny SyntheticSpeech model with lm_path: runs and writes predictions; with zero weights CER / WER are those
    of the run without lm_path."""
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.lm import CharNgramLM
    from policy_gradient_asr_amd.model import build_lm, predict, train
    corpus = tmp_path / "corpus"; out = tmp_path / "run"
    corpus.mkdir()
    (corpus / "alphabet.txt").write_text("a\nb\nc\nd\n \n")
    char2ind = {"<pad>": 0, "a": 1, "b": 2, "c": 3, "d": 4, " ": 5}
    ds = SyntheticSpeech(48, char2ind, n_feats=20, seed=1)
    dv = SyntheticSpeech(16, char2ind, n_feats=20, seed=2)
    train(str(corpus), str(out), 6, 16, 0, train_dataset=ds, dev_dataset=dv, n_feats=20, lam=0.0, lr=3e-3, log_every=0)
    lm = build_lm(str(corpus), order=3, train_dataset=ds)
    lm_path = str(corpus / "lm.npz")
    assert os.path.exists(lm_path) and lm.order == 3 and lm.vocab == 6
    back = CharNgramLM.load(lm_path)
    assert np.array_equal(back.table, lm.table)
    assert np.array_equal(lm.table, CharNgramLM.from_text([it["trans"] for it in ds.items], char2ind, order=3).table)
    alphabet = str(corpus / "alphabet.txt")
    base = predict(None, None, alphabet, str(out), 8, test_dataset=dv, n_feats=20)
    zero = predict(None, None, alphabet, str(out), 8, test_dataset=dv, n_feats=20, lm_path=lm_path, lm_alpha=0.0, lm_beta=0.0)
    assert zero == base
    cer, wer = predict(None, None, alphabet, str(out), 8, test_dataset=dv, n_feats=20, lm_path=lm_path, lm_alpha=0.5, lm_beta=0.5)
    lines = open(out / "predicted.txt").read().splitlines()
    assert len(lines) == 16 and all("|" in ln for ln in lines)
    assert 0.0 <= cer and np.isfinite(wer)
