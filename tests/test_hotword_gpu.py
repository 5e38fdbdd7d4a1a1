"""Hotword biasing on the device (csrc/beam.hip BIAS = true, csrc/hotword.hip) against the plain-Python search with the bias' bonus
(tests/hotword_ref.py): hypotheses token for token, scores to 1e-6 relative on the fp32 path (cases with a margin condition:
tests/test_hotword_cpu.py) and 1e-9 on the exact path; weight 0 against the search without a bias, bit for bit; the N-best lists;
the second pass against ``score_sequence`` with ==; and one constructed utterance end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as L  # noqa: E402
import hotword_ref as H  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lm(table, order, blank):
    from policy_gradient_asr_amd.lm import CharNgramLM
    return None if table is None else CharNgramLM(table, order, blank=blank)


def _kw(case, table, bias):
    T, V, beam, blank, order, gamma, kind, seed = case
    return dict(beam=beam, blank=blank, lm=_lm(table, order, blank), lm_alpha=H.ALPHA if order else 0.0,
                lm_beta=H.BETA if order else 0.0, bias=bias, bias_weight=gamma)


@pytest.mark.parametrize("case", H.CASES, ids=H.case_id)
def test_fast_path_matches_the_biased_reference(case):
    """fp32 log-probs with ragged lengths (0 and 1 among them): the 1-best token for token, score 1e-6 relative; the N-best list at
    N = min(beam, 16) row for row; row 0 of the list bit-equal to the 1-best entry point."""
    from policy_gradient_asr_amd import hipops
    lp, lens, table, bias, _ = H.case_inputs(case)
    ref = H.case_reference(case)
    N = H.nbest_of(case)
    d_lp, d_len = torch.from_numpy(lp).to(DEV), torch.from_numpy(lens).to(DEV)
    tok, tl, score = hipops.ctc_beam_search(d_lp, d_len, **_kw(case, table, bias))
    nb = hipops.ctc_beam_search_nbest(d_lp, d_len, nbest=N, **_kw(case, table, bias))
    assert torch.equal(nb.tokens[0], tok) and torch.equal(nb.lengths[0], tl) and torch.equal(nb.score[0], score)
    ntok, nlen, nsc, ncnt = nb.tokens.cpu().numpy(), nb.lengths.cpu().numpy(), nb.score.cpu().numpy(), nb.count.cpu().numpy()
    for b in range(H.B):
        hyps, gap = ref[b]
        got = list(tok[b, :tl[b]].cpu().numpy())
        print(f"{H.case_id(case)} b={b}: score {float(score[b])!r} reference {hyps[0][1]!r} gap {gap:.3e}")
        assert got == list(hyps[0][0]), b
        assert float(score[b]) == pytest.approx(hyps[0][1], rel=1e-6), b
        assert int(tok[b, tl[b]:].abs().sum()) == 0
        assert int(ncnt[b]) == len(hyps)
        for r, (want, wscore) in enumerate(hyps):
            assert list(ntok[r, b, :nlen[r, b]]) == list(want), (b, r)
            assert not ntok[r, b, nlen[r, b]:].any()
            assert (nsc[r, b] == wscore) if np.isinf(wscore) else (nsc[r, b] == pytest.approx(wscore, rel=1e-6)), (b, r)
        for r in range(len(hyps), N):
            assert nlen[r, b] == 0 and nsc[r, b] == np.inf and not ntok[r, b].any()


@pytest.mark.parametrize("case", [H.CASES[i] for i in H.EXACT_CASES], ids=H.case_id)
def test_exact_path_matches_the_biased_reference(case):
    """The same inputs as fp64 on the exact instantiation: tokens identical, score 1e-9 relative, as the exact LM kernel is held."""
    from policy_gradient_asr_amd import hipops
    lp, lens, table, bias, _ = H.case_inputs(case)
    ref = H.case_reference(case)
    d_lp, d_len = torch.from_numpy(lp).double().to(DEV), torch.from_numpy(lens).to(DEV)
    tok, tl, score = hipops.ctc_beam_search(d_lp, d_len, **_kw(case, table, bias))
    nb = hipops.ctc_beam_search_nbest(d_lp, d_len, nbest=H.nbest_of(case), **_kw(case, table, bias))
    assert torch.equal(nb.tokens[0], tok) and torch.equal(nb.lengths[0], tl) and torch.equal(nb.score[0], score)
    for b in range(H.B):
        hyps, gap = ref[b]
        print(f"exact {H.case_id(case)} b={b}: score {float(score[b])!r} reference {hyps[0][1]!r} gap {gap:.3e}")
        assert list(tok[b, :tl[b]].cpu().numpy()) == list(hyps[0][0]), b
        assert float(score[b]) == pytest.approx(hyps[0][1], rel=1e-9), b
        for r, (want, wscore) in enumerate(hyps):
            assert list(nb.tokens[r, b, :nb.lengths[r, b]].cpu().numpy()) == list(want), (b, r)
            if np.isfinite(wscore):
                assert float(nb.score[r, b]) == pytest.approx(wscore, rel=1e-9), (b, r)


@pytest.mark.parametrize("case", [H.CASES[2], H.CASES[7], H.CASES[3]], ids=H.case_id)
@pytest.mark.parametrize("f64", [False, True])
def test_zero_weight_is_the_search_without_a_bias_bit_for_bit(case, f64):
    """bias_weight = 0: every output word (tokens, lengths, scores, count) equals the workgroup kernel's without a bias -- with and
    without an LM, for the 1-best and for N = 16 -- and the weight does reach the kernel."""
    from policy_gradient_asr_amd import hipops
    lp, lens, table, bias, _ = H.case_inputs(case)
    kw = _kw(case, table, bias)
    d_lp, d_len = torch.from_numpy(lp).to(DEV), torch.from_numpy(lens).to(DEV)
    if f64:
        d_lp = d_lp.double()
    plain = {k: v for k, v in kw.items() if k not in ("bias", "bias_weight")}
    zero = dict(kw, bias_weight=0.0)
    a = hipops.ctc_beam_search(d_lp, d_len, generic=True, **plain)
    z = hipops.ctc_beam_search(d_lp, d_len, **zero)
    assert all(torch.equal(x, y) for x, y in zip(a, z))
    w = hipops.ctc_beam_search(d_lp, d_len, **kw)
    assert not torch.equal(a[2], w[2])
    a = hipops.ctc_beam_search_nbest(d_lp, d_len, nbest=16, **plain)
    z = hipops.ctc_beam_search_nbest(d_lp, d_len, nbest=16, **zero)
    assert all(torch.equal(x, y) for x, y in zip(a, z))


@pytest.mark.parametrize("order", [0, 2])
def test_the_edge_of_the_lds_check_is_accepted_with_a_bias(order):
    """beam 128, V 32 -- 4096 candidates, the largest sort the 160 KB check admits -- runs with a bias table as it does without."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.lm import HotwordBias
    T, Bn, V, beam = 12, 2, 32, 128
    rng = np.random.default_rng(3)
    lp = torch.from_numpy(L.log_softmax32(rng.normal(size=(T, Bn, V)) * 2.0)).to(DEV)
    bias = HotwordBias(rng.integers(1, V, size=(20, 3)).tolist(), V)
    lm = _lm(L.random_table(V, order, 0, 1), order, 0) if order else None
    kw = dict(beam=beam, lm=lm, lm_alpha=0.5 if order else 0.0, lm_beta=0.5 if order else 0.0)
    a = hipops.ctc_beam_search(lp, None, generic=True, **kw)
    z = hipops.ctc_beam_search(lp, None, bias=bias, bias_weight=0.0, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, z))
    w = hipops.ctc_beam_search(lp, None, bias=bias, bias_weight=1.0, **kw)
    nb = hipops.ctc_beam_search_nbest(lp, None, nbest=128, bias=bias, bias_weight=1.0, **kw)
    assert torch.isfinite(w[2]).all() and torch.equal(nb.score[0], w[2]) and torch.equal(nb.tokens[0], w[0])
    assert not torch.equal(a[2], w[2])


@pytest.mark.parametrize("V", [29, 300, 1024])
@pytest.mark.parametrize("N", [1, 16, 128])
def test_second_pass_equals_score_sequence(N, V):
    """nbest_bias_score == score_sequence with ==: stride > the longest row, lengths 0, rows beyond count zero, rows holding the blank
    and ids >= V (and a negative one), phrases planted so that matches happen."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.lm import HotwordBias
    rng = np.random.default_rng(1000 * N + V)
    Bn, stride = 3, 44
    phrases = [tuple(rng.integers(1, V, size=int(rng.integers(1, 6))).tolist()) for _ in range(40)]
    phrases += [phrases[0] + phrases[1], phrases[1][-1:] + phrases[2], (1, 1, 2), (1, 2), (2, 1, 1, 3)]
    bias = HotwordBias(phrases, V, boost=0.75, weights=rng.uniform(0.1, 3.0, size=len(phrases)).tolist(), partial=0.5)
    tokens = rng.integers(1, V, size=(N, Bn, stride)).astype(np.int32)
    lengths = rng.integers(0, 38, size=(N, Bn)).astype(np.int32)
    lengths[0, 0] = 0
    lengths[N - 1, 1] = 37
    for n in range(N):
        for b in range(Bn):
            for _ in range(3):
                p = phrases[int(rng.integers(len(phrases)))]
                i = int(rng.integers(0, 30))
                tokens[n, b, i:i + len(p)] = p
    tokens[0, 1, 3], tokens[0, 1, 5], tokens[0, 1, 7] = 0, V, -1          # the blank, an id >= V, a negative id
    tokens[N - 1, 2, 2], tokens[N - 1, 2, 9] = 0, V + 7
    lengths[0, 1] = max(lengths[0, 1], 12)
    lengths[N - 1, 2] = max(lengths[N - 1, 2], 12)
    count = np.array([N, max(N - 3, 1), (N + 1) // 2], dtype=np.int32)
    got = hipops.nbest_bias_score(torch.from_numpy(tokens).to(DEV), torch.from_numpy(lengths).to(DEV), torch.from_numpy(count).to(DEV),
                                  bias).cpu().numpy()
    nonzero = 0
    for n in range(N):
        for b in range(Bn):
            want = bias.score_sequence(tokens[n, b, :lengths[n, b]].tolist()) if n < count[b] else 0.0
            assert got[n, b] == want, (n, b, got[n, b], want)
            nonzero += want != 0.0
    assert nonzero >= min(N, 3)


def test_rescore_with_a_bias_over_a_wide_list():
    """A list of ``ctc_beam_search_wide`` at V = 300: rescore(bias=) total == earlier total - bias_weight * B(y) and its order is
    the stable ascending rank of that total; the bias field is score_sequence."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    from policy_gradient_asr_amd.lm import HotwordBias
    T, Bn, V, beam, N, w = 30, 3, 300, 8, 8, 0.7
    rng = np.random.default_rng(17)
    logits = rng.normal(size=(T, Bn, V)) * 3.0
    logits[:, :, 0] += 2.0
    lp = torch.from_numpy(L.log_softmax32(logits)).to(DEV)
    lens = torch.tensor([T, T - 9, 1], dtype=torch.int32, device=DEV)
    nb = hipops.ctc_beam_search_wide(lp, lens, beam=beam, nbest=N)
    rows = [[nb.tokens[r, b, :nb.lengths[r, b]].tolist() for r in range(int(nb.count[b]))] for b in range(Bn)]

    def own(b, r):       # the tokens around the first place where row r leaves row 0: a phrase the better rows do not hold
        y, y0 = rows[b][r], rows[b][0]
        i = next((k for k in range(min(len(y), len(y0))) if y[k] != y0[k]), min(len(y), len(y0)))
        return tuple(y[max(0, i - 1):i + 2])

    phrases = [own(0, 2), own(0, 5), own(1, 3), own(2, 6)]
    bias = HotwordBias([p for p in phrases if p] + rng.integers(1, V, size=(30, 3)).tolist(), V)
    dec = CTCDecoder(list(range(V)), wide_search=True)
    base = dec.rescore(lp, lens, nb, acoustic="first_pass")
    rs = dec.rescore(lp, lens, nb, acoustic="first_pass", bias=bias, bias_weight=w)
    assert rs._fields == base._fields + ("bias",) and torch.equal(rs.am, base.am)
    total, order, bsc = rs.total.cpu().numpy(), rs.order.cpu().numpy(), rs.bias.cpu().numpy()
    base_total = base.total.cpu().numpy()
    moved = 0
    for b in range(Bn):
        want = []
        for r in range(N):
            if r < len(rows[b]):
                B_y = bias.score_sequence(rows[b][r])
                assert bsc[r, b] == B_y
                want.append(float(base_total[r, b]) - w * B_y)
            else:
                assert bsc[r, b] == 0.0
                want.append(float("inf"))
            assert total[r, b] == want[r], (b, r)
        n = len(rows[b])
        assert list(order[b]) == sorted(range(n), key=lambda r: want[r]) + list(range(n, N))      # sorted() is stable
        moved += list(order[b]) != list(base.order[b].cpu().numpy())
        first = int(order[b, 0])
        assert rs.best_tokens[b, :rs.best_len[b]].tolist() == rows[b][first]
    assert moved >= 2
    md = dec.mbr_decode(lp, lens, beam_size=beam, nbest=N, acoustic="first_pass", bias=bias, bias_weight=w, max_hyp_len=T)
    assert torch.equal(md.nbest.tokens, nb.tokens) and md.tokens.shape == (Bn, T)


def test_hotword_end_to_end():
    """A (T = 40, V = 29) utterance whose acoustics say "kuznetzova": with the hotword "kuznetsova" the decoder returns it, without
    it does not; decode_batch (fp32) and the N-best form agree."""
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    alphabet = ["<pad>"] + list("abcdefghijklmnopqrstuvwxyz' ")
    ind = {c: i for i, c in enumerate(alphabet)}
    word, heard = "kuznetsova", "kuznetzova"
    T, V = 40, len(alphabet)
    assert V == 29
    probs = 0.002 * np.exp(np.random.default_rng(3).normal(size=(T, V)) * 1.5)      # uneven background: no cut is decided by < 2e-3
    probs[:, 0] = 1.0
    for k, (c, h) in enumerate(zip(word, heard)):
        for t in (4 * k, 4 * k + 1):
            probs[t, 0] = 0.002
            if c == h:
                probs[t, ind[c]] = 1.0
            else:
                probs[t, ind[h]], probs[t, ind[c]] = 0.55, 0.45
    probs /= probs.sum(axis=1, keepdims=True)
    text = lambda toks: "".join(alphabet[t] for t in toks)
    assert text(CTCDecoder(alphabet).decode(probs, beam_size=16)[0]) == heard
    dec = CTCDecoder(alphabet, hotwords=[word])
    assert text(dec.decode(probs, beam_size=16)[0]) == word
    assert text(dec.decode(probs, beam_size=16, nbest=4)[0][0]) == word
    lp = torch.from_numpy(np.log(probs)).float().view(T, 1, V).to(DEV)
    tok, tl, _ = dec.decode_batch(lp, None, beam_size=16)
    assert text(tok[0, :tl[0]].tolist()) == word
    dec.set_hotwords(None)
    tok, tl, _ = dec.decode_batch(lp, None, beam_size=16)
    assert text(tok[0, :tl[0]].tolist()) == heard
    dec.set_hotwords([word], 0.0)                            # weight 0: the acoustic answer
    assert text(dec.decode(probs, beam_size=16)[0]) == heard
