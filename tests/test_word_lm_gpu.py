"""The word n-gram LM of the second pass on the device (csrc/word_lm.hip): pgasr_nbest_word_lm_score against the plain statement of
tests/word_lm_ref.py on every word of its three outputs (==), pgasr_nbest_combine_rank against the formula and the stable rank
(==), and the host layer end to end: ``CTCDecoder.rescore(word_lm=)``, ``mbr_decode(word_lm=)`` and ``predict``.
The lists are synthetic token rows; tests/test_word_lm_cpu.py asserts the premises of every generated case."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import word_lm_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(*arrays):
    return tuple(torch.from_numpy(np.array(a)).to(DEV) for a in arrays)          # a copy: the shared cases are read-only


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_scores_equal_the_reference_on_every_word(order):
    from policy_gradient_asr_amd import hipops
    lm = W.model(order)
    ref = W.Ref(lm)
    for name in W.LISTS:
        tokens, lengths, count = W.list_case(name)
        want = W.list_ref(ref, tokens, lengths, count, W.DELIM)
        tk, ln, cn = _dev(tokens, lengths, count)
        got = hipops.nbest_word_lm_score(tk, ln, cn, lm, W.DELIM)
        assert [g.dtype for g in got] == [torch.float64, torch.int32, torch.int32]
        for g, w, what in zip(got, want, ("word_logp", "n_words", "n_oov")):
            g = g.cpu().numpy()
            bad = np.argwhere(g != w)
            assert bad.size == 0, (name, what, len(bad), [(tuple(i), g[tuple(i)], w[tuple(i)]) for i in bad[:6]])
        # the host's own statement says the same, bit for bit
        for n in range(min(int(count[0]), 8)):
            L = min(int(lengths[n, 0]), W.STRIDE)
            assert lm.logp_sentence(tokens[n, 0, :L]) == (want[0][n, 0], want[1][n, 0], want[2][n, 0])


def test_rows_at_the_stride_limit():
    """tok_stride = 4096, the documented limit: a full row of 2048 one-letter words, and a row of one letter."""
    from policy_gradient_asr_amd import hipops
    lm = W.model(5)
    ref = W.Ref(lm)
    S = hipops.WORD_LM_MAX_STRIDE
    tokens = np.full((2, 1, S), W.DELIM, dtype=np.int32)
    tokens[0, 0, 0::2] = np.random.default_rng(2).integers(2, W.V, size=S // 2)
    tokens[1, 0, 0] = 2
    lengths, count = np.array([[S], [1]], dtype=np.int32), np.array([2], dtype=np.int32)
    want = W.list_ref(ref, tokens, lengths, count, W.DELIM)
    assert want[1][0, 0] == S // 2
    got = hipops.nbest_word_lm_score(*_dev(tokens, lengths, count), lm, W.DELIM)
    for g, w in zip(got, want):
        assert (g.cpu().numpy() == w).all()
    from policy_gradient_asr_amd import _lib
    with pytest.raises(_lib.PgasrError):
        hipops.nbest_word_lm_score(*_dev(np.zeros((1, 1, S + 1), dtype=np.int32), lengths[:1], count), lm, W.DELIM)


@pytest.mark.parametrize("alpha,beta", [(0.7, 1.3), (0.0, 0.0), (-0.25, 0.0)])
def test_combine_rank_equals_the_formula_and_the_stable_rank(alpha, beta):
    from policy_gradient_asr_amd import hipops
    base, logp, nw, count = W.combine_case()
    want_total, want_order = W.combine_ref(base, logp, nw, count, alpha, beta)
    order, total = hipops.nbest_combine_rank(*_dev(base, logp, nw, count), word_alpha=alpha, word_beta=beta)
    assert (total.cpu().numpy() == want_total).all()
    assert (order.cpu().numpy() == want_order).all()
    if alpha == 0.0 and beta == 0.0:
        keep = np.isfinite(base) & (np.arange(base.shape[0])[:, None] < count[None, :])
        assert (total.cpu().numpy()[keep] == base[keep]).all()
    # N = 128 and N = 1
    rng = np.random.default_rng(9)
    for N in (128, 1):
        b2 = np.round(rng.normal(0, 3, size=(N, 2)), 0); l2 = -np.round(rng.uniform(0, 9, size=(N, 2)), 0)
        n2 = rng.integers(0, 4, size=(N, 2)).astype(np.int32); c2 = np.array([N, N // 2], dtype=np.int32)
        wt, wo = W.combine_ref(b2, l2, n2, c2, 0.5, 0.25)                  # small integers and dyadic weights: many exact ties
        o, t = hipops.nbest_combine_rank(*_dev(b2, l2, n2, c2), word_alpha=0.5, word_beta=0.25)
        assert (t.cpu().numpy() == wt).all() and (o.cpu().numpy() == wo).all()


def _random_case():
    T, B = 40, 3
    g = torch.Generator().manual_seed(4)
    lp = torch.log_softmax(2.0 * torch.randn(T, B, W.V, generator=g), 2).to(DEV)
    lengths = torch.tensor([40, 31, 17], dtype=torch.int32, device=DEV)
    return lp, lengths


def test_rescore_with_a_word_lm_end_to_end():
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder, NBestRescored, NBestRescoredWords
    lm = W.model(3)
    ref = W.Ref(lm)
    dec = CTCDecoder(W.ALPHABET)
    lp, lengths = _random_case()
    nb = dec.decode_batch(lp, lengths, beam_size=8, nbest=6)
    plain = dec.rescore(lp, lengths, nb)
    assert type(plain) is NBestRescored
    rs = dec.rescore(lp, lengths, nb, word_lm=lm, word_lm_alpha=0.6, word_lm_beta=0.4)
    assert type(rs) is NBestRescoredWords and rs._fields[:7] == plain._fields
    tokens, ln, count = nb.tokens.cpu().numpy(), nb.lengths.cpu().numpy(), nb.count.cpu().numpy()
    want = W.list_ref(ref, tokens, ln, count, W.DELIM)
    assert (rs.word_logp.cpu().numpy() == want[0]).all() and (rs.n_words.cpu().numpy() == want[1]).all()
    assert (rs.n_oov.cpu().numpy() == want[2]).all() and want[1].max() >= 2
    total, order = W.combine_ref(plain.total.cpu().numpy(), want[0], want[1], count, 0.6, 0.4)
    assert (rs.total.cpu().numpy() == total).all() and (rs.order.cpu().numpy() == order).all()
    assert (rs.am == plain.am).all() and (rs.lm_logp == plain.lm_logp).all()
    first = order[:, 0]
    for b in range(3):
        assert int(rs.best_len[b]) == ln[first[b], b] and (rs.best_tokens[b].cpu().numpy() == tokens[first[b], b]).all()
    # weights of zero: what rescore returns without a word LM, bit for bit
    zero = dec.rescore(lp, lengths, nb, word_lm=lm)
    assert (zero.total == plain.total).all() and (zero.order == plain.order).all() and (zero.best_tokens == plain.best_tokens).all()
    # the explicit delimiter is the default's
    again = dec.rescore(lp, lengths, nb, word_lm=lm, word_lm_alpha=0.6, word_lm_beta=0.4, word_delimiter=W.DELIM)
    assert (again.total == rs.total).all()


def test_the_word_lm_prefers_the_hypothesis_made_of_words():
    """Frames that spell 'ab c' and then slightly prefer 'e' to 'd': the first pass and the exact CTC likelihood rank 'ab ce' first,
    'ce' is no word of the vocabulary, and the word LM moves 'ab cd' to rank 0."""
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    lm = W.model(3)
    dec = CTCDecoder(W.ALPHABET)
    spell = W.enc("ab c")
    probs = np.full((5, W.V), 0.01)
    for t, s in enumerate(spell):
        probs[t, s] = 1.0
    probs[4, W.CHAR2IND["e"]], probs[4, W.CHAR2IND["d"]] = 0.50, 0.42
    probs /= probs.sum(axis=1, keepdims=True)
    lp = torch.from_numpy(np.log(probs).astype(np.float32)).to(DEV).view(5, 1, W.V)
    nb = dec.decode_batch(lp, None, beam_size=8, nbest=4)
    texts = ["".join(W.ALPHABET[k] for k in nb.tokens[r, 0, :int(nb.lengths[r, 0])].tolist()) for r in range(int(nb.count[0]))]
    assert texts[0] == "ab ce" and "ab cd" in texts
    plain = dec.rescore(lp, None, nb)
    assert int(plain.order[0, 0]) == 0
    rs = dec.rescore(lp, None, nb, word_lm=lm, word_lm_alpha=1.0)
    assert int(rs.n_oov[0, 0]) == 1 and int(rs.n_oov[texts.index("ab cd"), 0]) == 0
    assert int(rs.order[0, 0]) == texts.index("ab cd")
    assert W.enc("ab cd") == rs.best_tokens[0, :int(rs.best_len[0])].tolist()


def test_mbr_decode_takes_its_posterior_from_the_word_lm_totals():
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    lm = W.model(2)
    dec = CTCDecoder(W.ALPHABET)
    lp, lengths = _random_case()
    md = dec.mbr_decode(lp, lengths, beam_size=8, nbest=6, word_lm=lm, word_lm_alpha=0.8, word_lm_beta=0.3)
    rs = dec.rescore(lp, lengths, md.nbest, word_lm=lm, word_lm_alpha=0.8, word_lm_beta=0.3)
    want = dec.mbr_from_list(md.nbest, rs.total, vocab=W.V)
    assert (md.posterior == want.posterior).all() and (md.best == want.best).all() and (md.risk == want.risk).all()
    # the statement of the posterior itself: the softmax of -total over each list
    t = rs.total.cpu().numpy()
    p = np.exp(-(t - t.min(axis=0)))
    p /= p.sum(axis=0)
    assert md.posterior.cpu().numpy() == pytest.approx(p, rel=1e-12)
    without = dec.mbr_decode(lp, lengths, beam_size=8, nbest=6)
    assert not (without.posterior == md.posterior).all()


def test_predict_with_a_word_lm(tmp_path):
    """predict(rescore_word_lm_path=) on a tiny SyntheticSpeech model: nbest.tsv gains word_logp, n_words and n_oov, and only then."""
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.lm import WordNgramLM
    from policy_gradient_asr_amd.model import build_lm, build_word_lm, predict, train
    corpus = tmp_path / "corpus"; out = tmp_path / "run"
    corpus.mkdir()
    (corpus / "alphabet.txt").write_text("a\nb\nc\nd\n \n")
    char2ind = {"<pad>": 0, "a": 1, "b": 2, "c": 3, "d": 4, " ": 5}
    ds = SyntheticSpeech(32, char2ind, n_feats=20, seed=1)
    dv = SyntheticSpeech(8, char2ind, n_feats=20, seed=2)
    train(str(corpus), str(out), 2, 16, 0, train_dataset=ds, dev_dataset=dv, n_feats=20, lam=0.0, lr=3e-3, log_every=0)
    wlm = build_word_lm(str(corpus), order=3, train_dataset=ds)
    assert os.path.exists(corpus / "word_lm.npz") and wlm.delimiter == 5
    alphabet = str(corpus / "alphabet.txt")
    predict(None, None, alphabet, str(out), 8, test_dataset=dv, n_feats=20, nbest=4)
    assert all(len(ln.split("\t")) == 5 for ln in open(out / "nbest.tsv").read().splitlines())
    cer, wer = predict(None, None, alphabet, str(out), 8, test_dataset=dv, n_feats=20, nbest=4,
                       rescore_word_lm_path=str(corpus / "word_lm.npz"), rescore_word_alpha=0.5, rescore_word_beta=0.5)
    assert 0.0 <= cer and np.isfinite(wer)
    rows = [ln.split("\t") for ln in open(out / "nbest.tsv").read().splitlines()]
    assert rows and all(len(r) == 8 for r in rows)
    loaded = WordNgramLM.load(str(corpus / "word_lm.npz"))
    for u, r, score, total, text, word_logp, n_words, n_oov in rows:
        assert np.isfinite(float(total)) and int(n_words) == len(text.split()) and 0 <= int(n_oov) <= int(n_words)
        assert float(word_logp) <= 0.0
    # with the character LM and MBR on top
    build_lm(str(corpus), order=2, train_dataset=ds)
    cer, wer = predict(None, None, alphabet, str(out), 8, test_dataset=dv, n_feats=20, nbest=4, rescore_lm_path=str(corpus / "lm.npz"),
                       rescore_alpha=0.3, rescore_word_lm_path=str(corpus / "word_lm.npz"), rescore_word_alpha=0.5, mbr=True)
    assert np.isfinite(cer) and all(len(ln.split("\t")) == 8 for ln in open(out / "nbest.tsv").read().splitlines())
    assert loaded.order == 3
    with pytest.raises(ValueError):
        predict(None, None, alphabet, str(out), 8, test_dataset=dv, n_feats=20, rescore_word_lm_path=str(corpus / "word_lm.npz"))
