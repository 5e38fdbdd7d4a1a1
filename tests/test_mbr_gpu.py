"""Minimum-Bayes-risk decoding on the device (csrc/mbr.hip): the pairwise distances of pgasr_nbest_pair_dist against the DP of
tests/mbr_ref.py on every word of the output (==), the composed path of ``hipops.nbest_pair_distance`` against both, the selection
of pgasr_mbr_select against its numpy statement (1e-12 relative; == where scale = 0 makes it exact), and the host layer end to end.
The lists are synthetic token rows; tests/test_mbr_cpu.py asserts the premises of every generated case."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as R  # noqa: E402
import mbr_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(*arrays):
    return tuple(torch.from_numpy(np.array(a)).to(DEV) for a in arrays)          # a copy: the shared cases are read-only


@pytest.mark.parametrize("name", [c[0] for c in M.PAIR_CASES])
def test_pair_distances_equal_the_dp_on_every_word(name):
    from policy_gradient_asr_amd import hipops
    tokens, lengths, count, V, Lmax, want = M.pair_case(name)
    tk, ln, cn = _dev(tokens, lengths, count)
    got = hipops._pair_distance_kernel(tk, ln, cn, V, Lmax).cpu().numpy()          # pgasr_nbest_pair_dist itself
    assert got.dtype == np.int32 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, len(bad), [(tuple(i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:8]])
    # the public call, whichever path it picks for the size; max_hyp_len=None reads the longest valid hypothesis from the device
    assert (hipops.nbest_pair_distance(tk, ln, cn, V, max_hyp_len=Lmax).cpu().numpy() == want).all()
    if Lmax == M.LMAX and count.max() > 0:
        assert (hipops.nbest_pair_distance(tk, ln, cn, V).cpu().numpy() == want).all()


def test_composed_path_equals_the_dp_and_the_kernel():
    from policy_gradient_asr_amd import hipops
    # one hypothesis of 1025 tokens: over the kernel's limit, so the whole list takes the composed path
    rng = np.random.default_rng(3)
    rows = [[int(x) for x in rng.integers(0, 29, size=L)] for L in (1025, 64, 0, 513)]
    rows.append(rows[0][:500] + rows[0][520:])
    tokens, lengths, count = M._pack([rows], [5], 29, rng)
    want = M.pair_dist_ref(tokens, lengths, count, 29, 1025)
    tk, ln, cn = _dev(tokens, lengths, count)
    got = hipops.nbest_pair_distance(tk, ln, cn, 29).cpu().numpy()
    assert (got == want).all() and want[0, 0, 4] == 20 and (want >= 0).all()
    # at lengths <= 1024 the composed path gives the kernel's matrix, -1 entries included; a cap above the limit forces it
    for name in ("n3", "n17-v2", "n16-edges", "symbol-ge-v", "n2", "over-lmax"):
        tokens, lengths, count, V, Lmax, want = M.pair_case(name)
        tk, ln, cn = _dev(tokens, lengths, count)
        kernel = hipops._pair_distance_kernel(tk, ln, cn, V, Lmax)
        composed = hipops._pair_distance_composed(tk, ln, cn, V, Lmax, "char", None)
        assert torch.equal(kernel, composed) and (kernel.cpu().numpy() == want).all(), name
        if Lmax == M.LMAX:
            assert torch.equal(hipops.nbest_pair_distance(tk, ln, cn, V, max_hyp_len=1025), kernel), name


def test_word_distances_equal_the_helper():
    from policy_gradient_asr_amd import hipops
    tokens, lengths, count, d = M.word_case()
    tk, ln, cn = _dev(tokens, lengths, count)
    want = M.word_pair_dist_ref(tokens, lengths, count, d, M.LMAX)
    got = hipops.nbest_pair_distance(tk, ln, cn, 6, unit="word", delimiter=d).cpu().numpy()
    assert (got == want).all()
    capped = hipops.nbest_pair_distance(tk, ln, cn, 6, max_hyp_len=40, unit="word", delimiter=d).cpu().numpy()
    assert (capped == M.word_pair_dist_ref(tokens, lengths, count, d, 40)).all() and (capped[1, 4, :] == -1).all()
    with pytest.raises(ValueError):
        hipops.nbest_pair_distance(tk, ln, cn, 6, unit="word")


def _select(case):
    from policy_gradient_asr_amd import hipops
    dist, score, count, scale = case
    d, s, c = _dev(dist.astype(np.int32), score, count)
    best, risk, post = hipops.mbr_select(d, s, c, scale=scale)
    return best.cpu().numpy(), risk.cpu().numpy(), post.cpu().numpy(), M.select_ref(dist, score, count, scale)


def _close(got, want):
    fin = np.isfinite(want)
    assert (np.isfinite(got) == fin).all() and (got[~fin] == want[~fin]).all()                  # inf == inf
    assert (np.abs(got[fin] - want[fin]) <= 1e-12 * np.abs(want[fin])).all(), float(np.abs(got[fin] - want[fin]).max())


@pytest.mark.parametrize("case", ["general", "large", "other"])
def test_selection_against_the_helper(case):
    best, risk, post, (rbest, rrisk, rpost) = _select(getattr(M, "select_" + case)())
    print(case, "max |posterior - ref| =", float(np.abs(post - rpost).max()), "best =", best.tolist(), "ref =", rbest.tolist())
    assert all(M.best_within_margin(best, rrisk)), (best, rbest)
    _close(post, rpost); _close(risk, rrisk)
    assert (post[rpost == 0] == 0).all()


def test_selection_is_exact_at_scale_zero_and_first_wins_ties():
    best, risk, post, (rbest, rrisk, rpost) = _select(M.select_exact())
    assert (post == rpost).all() and (risk == rrisk).all() and (best == rbest).all(), (best, rbest)


def _lm(V, seed):
    from policy_gradient_asr_amd.lm import CharNgramLM
    return CharNgramLM(R.random_table(V, 2, 0, seed), 2, blank=0)


@pytest.mark.parametrize("unit", ["char", "word"])
@pytest.mark.parametrize("with_lm", [False, True], ids=["nolm", "lm"])
def test_mbr_decode_end_to_end(with_lm, unit):
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    T, B, V, beam, N = 40, 3, 8, 8, 8
    rng = np.random.default_rng(21)
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, B, V)).astype(np.float32) * 2.0), dim=-1).to(DEV)
    lens = torch.tensor([40, 33, 17], dtype=torch.int32, device=DEV)
    dec = CTCDecoder(list("abcdefg"))
    kw = {"lm": _lm(V, 4), "lm_alpha": 0.7, "lm_beta": 0.3} if with_lm else {"lm": None}
    delim = 5 if unit == "word" else None
    md = dec.mbr_decode(lp, lens, beam_size=beam, nbest=N, risk_unit=unit, word_delimiter=delim, posterior_scale=0.8, **kw)
    nb = md.nbest
    tokens, lengths, count = nb.tokens.cpu().numpy(), nb.lengths.cpu().numpy(), nb.count.cpu().numpy()
    assert tokens.shape == (N, B, T) and (count >= 2).all()
    total = dec.rescore(lp, lens, nb, **kw).total.cpu().numpy()                  # the device's own totals feed the helper
    want = M.pair_dist_ref(tokens, lengths, count, V, T) if unit == "char" else M.word_pair_dist_ref(tokens, lengths, count, delim, T)
    assert (md.dist.cpu().numpy() == want).all()
    rbest, rrisk, rpost = M.select_ref(want, total, count, 0.8)
    best = md.best.cpu().numpy()
    assert all(M.best_within_margin(best, rrisk)), (best, rbest)
    _close(md.posterior.cpu().numpy(), rpost); _close(md.risk.cpu().numpy(), rrisk)
    out_tok, out_len = md.tokens.cpu().numpy(), md.lengths.cpu().numpy()
    for b in range(B):
        assert out_len[b] == lengths[best[b], b] and (out_tok[b] == tokens[best[b], b]).all()
    # a list the caller holds, scored by the first pass: the same path through mbr_from_list
    m2 = dec.mbr_from_list(nb, nb.score, vocab=V, risk_unit=unit, word_delimiter=delim, posterior_scale=0.0, max_hyp_len=T)
    b2, r2, _ = M.select_ref(want, nb.score.cpu().numpy(), count, 0.0)
    assert all(M.best_within_margin(m2.best.cpu().numpy(), r2))


def test_predict_writes_mbr_tsv_and_leaves_the_default_alone(tmp_path, capsys):
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.model import train, predict
    corpus = tmp_path / "corpus"; out = tmp_path / "run"
    corpus.mkdir()
    (corpus / "alphabet.txt").write_text("a\nb\nc\nd\n \n")
    char2ind = {"<pad>": 0, "a": 1, "b": 2, "c": 3, "d": 4, " ": 5}
    ds = SyntheticSpeech(32, char2ind, n_feats=20, seed=1)
    dv = SyntheticSpeech(16, char2ind, n_feats=20, seed=2)
    train(str(corpus), str(out), 2, 16, 0, train_dataset=ds, dev_dataset=dv, n_feats=20, lam=0.0, lr=3e-3, log_every=0)
    args = (None, None, str(corpus / "alphabet.txt"), str(out), 8)
    predict(*args, test_dataset=dv, n_feats=20, nbest=4)
    plain = open(out / "predicted.txt", "rb").read()
    assert not os.path.exists(out / "mbr.tsv")
    predict(*args, test_dataset=dv, n_feats=20, nbest=4, mbr=False)
    assert open(out / "predicted.txt", "rb").read() == plain and not os.path.exists(out / "mbr.tsv")
    capsys.readouterr()
    for unit in ("char", "word"):
        cer, wer = predict(*args, test_dataset=dv, n_feats=20, nbest=4, mbr=True, mbr_unit=unit, mbr_scale=0.5)
        lines = open(out / "mbr.tsv").read().splitlines()
        assert len(lines) == 16 and [int(ln.split("\t")[0]) for ln in lines] == list(range(16))
        for ln in lines:
            _, rank, chosen, first = ln.split("\t")
            assert 0 <= int(rank) < 4 and 0.0 <= float(chosen) <= float(first) + 1e-6       # the choice is never worse than rank 0
        assert len(open(out / "predicted.txt").read().splitlines()) == 16 and np.isfinite(cer) and np.isfinite(wer)
        assert "MAP CER" in capsys.readouterr().out
    with pytest.raises(ValueError):
        predict(*args, test_dataset=dv, n_feats=20, mbr=True)
