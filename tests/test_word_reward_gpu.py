"""The word-level (WER) reward: word ids and word edit distances against str.split(" ") and the reference Levenshtein, the rewards
with a separate normaliser against numpy, whole f32 trainer steps with reward_unit="word" against the fp64 torch-CPU model, shard
identity, ragged batches, the default's bits, the train() driver and metrics.edit_counts."""
import numpy as np
import pytest
import torch

from oracle import decode_ref, pg_ref
from pg_harness import D, DEV, spaced_batch, spaced_lattice_case, shards_vs_whole, tiny_corpus, trainer_step_vs_oracle

pytestmark = pytest.mark.gpu
CHARS = "abcdefghijklmnopqrstuvwxyz'"


def decode(seq):
    return "".join(" " if int(t) == D else CHARS[int(t) - 1] for t in seq)


def split_words(seq):
    return pg_ref.split_words(seq, D)


def lev(a, b):
    """Levenshtein distance of two int sequences, numpy row DP (left chain as a prefix minimum): for the long word lists."""
    a = np.asarray(a, dtype=np.int64); b = np.asarray(b, dtype=np.int64)
    j = np.arange(len(a) + 1)
    row = j.copy()
    for i, tok in enumerate(b, 1):
        x = np.empty_like(row)
        x[0] = i
        x[1:] = np.minimum(row[1:] + 1, row[:-1] + (a != tok))
        row = np.minimum.accumulate(x - j) + j
    return int(row[-1])


def expected(ref, hyp):
    """(ref ids, hyp ids, word edit distance) of one pair as the header defines them."""
    wr, wh = split_words(ref), split_words(hyp)
    first = {}
    for i, w in enumerate(wr + wh):
        first.setdefault(w, i + 1)
    ri, hi = [first[w] for w in wr], [first[w] for w in wh]
    d = decode_ref.edit_dist(wr, wh)[0] if len(wr) * len(wh) <= 40000 else lev(ri, hi)
    return ri, hi, d


def run_pairs(pairs, stride=None):
    """word_ids + word_edit_distance of the pairs in ONE launch each; rows padded with delimiters past their lengths."""
    from policy_gradient_asr_amd import hipops
    N = len(pairs)
    R = stride or max(1, max(len(r) for r, _ in pairs))
    H = stride or max(1, max(len(h) for _, h in pairs))
    ref = torch.full((N, R), D, dtype=torch.int32); hyp = torch.full((N, H), D, dtype=torch.int32)
    rl = torch.zeros(N, dtype=torch.int32); hl = torch.zeros(N, dtype=torch.int32)
    for i, (r, h) in enumerate(pairs):
        ref[i, :len(r)] = torch.tensor(r, dtype=torch.int32); hyp[i, :len(h)] = torch.tensor(h, dtype=torch.int32)
        rl[i], hl[i] = len(r), len(h)
    args = (ref.to(DEV), rl.to(DEV), hyp.to(DEV), hl.to(DEV), D)
    ri, rw, hi, hw = hipops.word_ids(*args)
    dist, rw2, hw2 = hipops.word_edit_distance(*args)
    again = hipops.word_ids(*args)
    torch.cuda.synchronize()
    assert torch.equal(rw, rw2) and torch.equal(hw, hw2)
    for a, b_, n in ((ri, again[0], rw), (hi, again[2], hw)):          # deterministic
        for i in range(N):
            assert torch.equal(a[i, :int(n[i])], b_[i, :int(n[i])])
    return ri.cpu(), rw.cpu(), hi.cpu(), hw.cpu(), dist.cpu()


def check_pairs(pairs, stride=None):
    ri, rw, hi, hw, dist = run_pairs(pairs, stride)
    for i, (r, h) in enumerate(pairs):
        assert [decode(w) for w in split_words(r)] == decode(r).split(" ")          # the restatement is str.split
        eri, ehi, ed = expected(r, h)
        assert (int(rw[i]), int(hw[i])) == (len(eri), len(ehi)), i
        assert ri[i, :len(eri)].tolist() == eri, i
        assert hi[i, :len(ehi)].tolist() == ehi, i
        assert int(dist[i]) == ed, (i, int(dist[i]), ed)


def _rand_seq(rng, n, density, alpha):
    s = rng.integers(1, alpha + 1, size=n)
    s[rng.random(n) < density] = D
    return s.tolist()


def _mutate(rng, s, rate=0.05, alpha=27):
    s = list(s)
    for k in range(len(s)):
        if rng.random() < rate:
            s[k] = int(rng.integers(1, alpha + 1)) if rng.random() < 0.7 else D
    return s


@pytest.mark.parametrize("density", [0.0, 0.03, 0.18, 0.6, 1.0])
def test_word_ids_and_distance_random_pairs(density):
    """100 pairs per delimiter density (500 in all), lengths 0..1200; small alphabets so that words repeat, and hypotheses
    mutated from their reference so that most words are shared."""
    rng = np.random.default_rng(int(density * 1000) + 7)
    pairs = []
    for i in range(100):
        alpha = 3 if i % 2 else 27
        n = int(rng.integers(0, 1201)) if i % 4 else int(rng.integers(0, 40))
        r = _rand_seq(rng, n, density, alpha)
        h = _mutate(rng, r, alpha=alpha) if i % 3 else _rand_seq(rng, int(rng.integers(0, 1201)), density, alpha)
        pairs.append((r, h))
    check_pairs(pairs)


def test_word_ids_hand_cases():
    E = D
    rng = np.random.default_rng(1)
    distinct = [[int(a), int(b)] for a in range(1, 28) for b in range(1, 28)][:500]      # 500 distinct words of two tokens
    order = rng.permutation(len(distinct))
    many = sum(([*w, E] for w in distinct), [])[:-1]
    many_shuffled = sum(([*distinct[k], E] for k in order[:400]), [])[:-1]
    long_word = [int(t) for t in rng.integers(1, 28, size=300)]
    cases = [
        ([], []),                                            # one empty word each
        ([], [E]),                                           # one empty word against two
        ([E], []),
        ([E, 1, 2, E], [1, 2]),                              # leading and trailing delimiters
        ([1, E, E, 2, E], [E, 1, E, 2]),                     # doubled delimiters
        ([1, 2, E, 1, 2, E, 1, 2], [1, 2, E, 3, E, 1, 2]),   # repeated words
        ([1, E, 2, E, 3], [3, E, 2, E, 1]),                  # the same words reordered
        (many, many_shuffled),                               # many distinct words of equal length
        ([1, 2], [1, 2, 3]),                                 # prefixes
        ([1, 2, E, 1, 2, 3], [1, 2, 3, E, 1, 2]),
        ([1, 2, 3], [1, 2]),
        (long_word + [E] + long_word[:-1], long_word[:-1] + [E] + long_word),     # long words (cooperative confirmation)
        ([E] * 50, [E] * 49),
    ]
    check_pairs(cases)


def test_word_ids_at_the_stride_limit():
    from policy_gradient_asr_amd import _lib, hipops
    rng = np.random.default_rng(2)
    r = _rand_seq(rng, 4094, 0.18, 27)
    same = [5] * 4094
    check_pairs([(r, _mutate(rng, r)), (same, same), (r, same)], stride=4094)
    z = torch.zeros(1, 4095, dtype=torch.int32, device=DEV)
    n = torch.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.PgasrError):
        hipops.word_ids(z, n, z, n, D)


@pytest.mark.parametrize("mode", ["hypothesis", "leave_one_out"])
def test_rewards_with_word_normaliser_vs_numpy(mode):
    from policy_gradient_asr_amd import hipops
    B, K, lam, Bg = 37, 5, 0.7, 64
    rng = np.random.default_rng(9)
    H = 1 if mode == "hypothesis" else 0
    dist = rng.integers(0, 12, size=(H + K) * B).astype(np.int32)
    tg_len = rng.integers(0, 60, size=B).astype(np.int32)
    n_words = rng.integers(1, 12, size=B).astype(np.int32)
    d_, t_, w_ = (torch.from_numpy(a).to(DEV) for a in (dist, tg_len, n_words))
    R_b, R_s, coef, us = hipops.pg_rewards_multi(d_, t_, K, lam, 1.0 / Bg, baseline=mode, reward_lengths=w_)
    f = np.float32
    Wf = n_words.astype(f)
    R = -(dist[H * B:].reshape(K, B).astype(f)) / Wf
    if mode == "hypothesis":
        bk = np.broadcast_to(-(dist[:B].astype(f)) / Wf, (K, B))
    else:
        S = np.zeros(B, dtype=f)
        for k in range(K):
            S = (S + R[k]).astype(f)
        bk = ((S[None] - R) / f(K - 1)).astype(f)
    scale = (f(lam) * f(1.0 / Bg)) / f(K)
    np.testing.assert_array_equal(R_s.cpu().numpy(), R)                             # R normalised by the word count
    np.testing.assert_allclose(coef.cpu().numpy(), scale * (R - bk), rtol=2e-7, atol=1e-12)
    R64 = -dist[H * B:].reshape(K, B) / n_words
    b64 = np.broadcast_to(-dist[:B] / n_words, R64.shape) if H else (R64.sum(axis=0, keepdims=True) - R64) / (K - 1)
    np.testing.assert_allclose(coef.cpu().numpy(), lam / (Bg * K) * (R64 - b64), rtol=1e-5, atol=1e-8)
    # utt_scale stays on the character counts: the bits of the character path
    _, _, _, us_c = hipops.pg_rewards_multi(d_, t_, K, lam, 1.0 / Bg, baseline=mode)
    assert torch.equal(us, us_c)
    # reward_lengths = target_lengths: pg_rewards_multi's bits, and with K = 1 / hypothesis pg_rewards'
    same = hipops.pg_rewards_multi(d_, t_, K, lam, 1.0 / Bg, baseline=mode, reward_lengths=t_.clone())
    ref = hipops.pg_rewards_multi(d_, t_, K, lam, 1.0 / Bg, baseline=mode)
    assert all(torch.equal(a, b) for a, b in zip(same, ref))
    if mode == "hypothesis":
        d1 = d_[:2 * B].contiguous()
        one = hipops.pg_rewards_multi(d1, t_, 1, lam, 1.0 / Bg, reward_lengths=t_.clone())
        R_g, R_s1, c1, u1 = hipops.pg_rewards(d1, t_, lam, 1.0 / Bg)
        assert torch.equal(one[0], R_g) and torch.equal(one[1][0], R_s1) and torch.equal(one[2][0], c1) and torch.equal(one[3], u1)


def _word_step_vs_oracle(reward_baseline, beam, K, seed=61):
    """One lambda = 1 trainer step (f32 mode, reward_unit="word") against the torch-CPU model in FP64 on the same weights:
    rewards exact, loss within 1e-5, every parameter gradient within 1e-4 (max norm)."""
    r = trainer_step_vs_oracle(dict(reward_decoder="beam" if beam else "greedy", beam_size=beam or 16, num_samples=K,
                                    reward_baseline=reward_baseline, reward_unit="word", word_delimiter=D),
                               dict(num_samples=K, baseline=reward_baseline, beam=beam, reward_unit="word", word_delimiter=D),
                               word=True, seed=seed, label=f"[word step] K={K} {reward_baseline} beam={beam}")
    tr = r.trainer
    assert all(s_.shape == (4,) for s_ in tr.last_stats) and tr.last_sample_rewards.shape == (K, 4)
    chars = pg_ref.pg_objective(*r.args, **dict(r.kw, reward_unit="char", paths=r.oracle.paths, beam=0))
    assert (np.abs(r.oracle.R - chars.R) > 1e-6).any()          # the word rewards are not the character rewards


@pytest.mark.parametrize("baseline,beam,K", [("hypothesis", 0, 1), ("hypothesis", 16, 1), ("hypothesis", 0, 4),
                                             ("leave_one_out", 0, 4)])
def test_word_reward_step_vs_oracle(baseline, beam, K):
    _word_step_vs_oracle(baseline, beam, K)


@pytest.mark.parametrize("K,baseline", [(1, "hypothesis"), (4, "leave_one_out")])
def test_word_reward_shards_reproduce_the_whole_batch(K, baseline):
    """Two pg_ctc_loss calls on the halves of a batch (global_batch, sample_base set) give the whole batch's word rewards and logits
    gradient (the coefficients times the paths)."""
    T, B, V, L = 150, 8, 29, 14
    kw = dict(lam=1.0, seed=11, offset=4, num_samples=K, baseline=baseline, reward_unit="word", word_delimiter=D)
    shards_vs_whole(kw, spaced_lattice_case(T, B, V, L, 78))


def test_word_reward_ragged_batch():
    """Padded (empty) utterances get R = 0 -- one empty word against one empty word --, and the real rows are the un-padded batch's;
    the trainer's padded step gives the un-padded step's word rewards."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    from policy_gradient_asr_amd.model import Seq2Seq, weights
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    T, B, V, L, P = 90, 5, 29, 12, 3
    logits, targets, in_len, tg_len = spaced_lattice_case(T, B, V, L, 5)
    for K, baseline in ((1, "hypothesis"), (4, "leave_one_out")):
        kw = dict(lam=1.0, seed=2, offset=3, num_samples=K, baseline=baseline, reward_unit="word", word_delimiter=D)
        _, _, R_s, R_b = pg_ctc_loss(logits.float().to(DEV), in_len.to(DEV), targets.to(DEV), tg_len.to(DEV), **kw)
        lp = torch.cat((logits.float(), torch.zeros(T, P, V)), dim=1).to(DEV)
        il = torch.cat((in_len, torch.zeros(P, dtype=torch.int32))).to(DEV)
        tg = torch.cat((targets, torch.zeros(P, L, dtype=torch.int32))).to(DEV)
        tl = torch.cat((tg_len, torch.zeros(P, dtype=torch.int32))).to(DEV)
        _, _, Rp_s, Rp_b = pg_ctc_loss(lp, il, tg, tl, global_batch=B, sample_base=0, **kw)
        assert torch.equal(Rp_s[..., :B], R_s) and torch.equal(Rp_b[:B], R_b)
        assert (Rp_s[..., B:] == 0).all() and (Rp_b[B:] == 0).all()

    F, T, L = 80, 60, 6
    lens = [T - (3 * b) % 17 for b in range(B)]
    x, targets, fmask, tmask = spaced_batch(B, F, T, V, L, lens, [max(1, L - b % 4) for b in range(B)], 8)
    batch = [v.to(DEV) for v in (x, targets, fmask, tmask)]
    res = {}
    for pad in (False, True):
        torch.manual_seed(0)
        m = Seq2Seq(V, n_feats=F); m.apply(weights); m = m.to(DEV).eval()
        tr = PolicyGradientTrainer(m, lam=1.0, seed=4, precision="f32", reward_unit="word", word_delimiter=D)
        tr.pad_ragged_batches = pad
        loss = tr.compute_gradients(*batch)
        torch.cuda.synchronize()
        hipops.lstm_assert_no_timeouts()
        res[pad] = (float(loss), [s_.clone() for s_ in tr.last_stats])
    assert torch.equal(res[True][1][1], res[False][1][1]) and torch.equal(res[True][1][2], res[False][1][2])
    assert abs(res[True][0] - res[False][0]) <= 1e-6 * abs(res[False][0])


def test_default_reward_unit_is_char_bit_for_bit():
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.model import Seq2Seq, weights
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    B, F, T, V, L = 16, 80, 80, 29, 10
    x, targets, fmask, tmask = spaced_batch(B, F, T, V, L, [T - b for b in range(B)], [L - b % 3 for b in range(B)], 12)
    batch = [v.to(DEV) for v in (x, targets, fmask, tmask)]
    out = []
    for kw in ({}, {"reward_unit": "char"}):
        torch.manual_seed(0)
        m = Seq2Seq(V, n_feats=F); m.apply(weights); m = m.to(DEV).eval()
        tr = PolicyGradientTrainer(m, lam=1.0, seed=4, precision="f32", **kw)
        loss = tr.compute_gradients(*batch)
        torch.cuda.synchronize()
        hipops.lstm_assert_no_timeouts()
        out.append((loss.detach().clone(), [s_.clone() for s_ in tr.last_stats], tr.gflat.clone()))
    (l0, s0, g0), (l1, s1, g1) = out
    assert torch.equal(l0, l1) and all(torch.equal(a, b) for a, b in zip(s0, s1)) and torch.equal(g0, g1)


def test_word_reward_argument_checks():
    from policy_gradient_asr_amd.model import Seq2Seq
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    m = Seq2Seq(29, n_feats=80).to(DEV)
    for kw in ({"reward_unit": "bpe", "word_delimiter": D}, {"reward_unit": "word"}, {"reward_unit": "word", "word_delimiter": 0},
               {"reward_unit": "word", "word_delimiter": 29}, {"reward_unit": "word", "word_delimiter": -2},
               {"reward_unit": "word", "word_delimiter": D, "reward_mode": "per_step"}):
        with pytest.raises(ValueError):
            PolicyGradientTrainer(m, **kw)
    tr = PolicyGradientTrainer(m, reward_unit="word", word_delimiter=D)
    x = torch.zeros(2, 80, 4095, device=DEV)
    fmask = torch.ones(2, 4095, device=DEV)
    t = torch.ones(2, 3, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="4094"):
        tr.compute_gradients(x, t, fmask, torch.ones_like(t))


def test_train_driver_records_reward_unit(tmp_path, capsys):
    """model.train(reward_unit="word"): trains with the alphabet's " " as the delimiter, records the unit in the checkpoint, warns on
    a resume with another unit; an alphabet without " " is refused."""
    from policy_gradient_asr_amd.model import train
    corpus, out, ds = tiny_corpus(tmp_path)
    l1, _ = train(str(corpus), str(out), 2, 16, 0, train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=0, reward_unit="word")
    assert len(l1) == 2 and all(np.isfinite(l1))
    st = torch.load(out / "checkpoint_last.pth", map_location="cpu")
    assert st["reward_unit"] == "word"
    capsys.readouterr()
    train(str(corpus), str(out), 3, 16, 0, train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=0)
    assert "reward_unit=char" in capsys.readouterr().out
    nospace = tmp_path / "nospace"
    nospace.mkdir()
    (nospace / "alphabet.txt").write_text("a\nb\nc\nd\n")
    with pytest.raises(ValueError, match="alphabet.txt"):
        train(str(nospace), str(tmp_path / "run2"), 1, 16, 0, train_dataset=ds, n_feats=20, log_every=0, reward_unit="word")


def test_edit_counts_agree_with_evaluate():
    from policy_gradient_asr_amd import metrics
    rng = np.random.default_rng(4)
    B, L, T = 24, 60, 200
    tg = torch.zeros(B, L, dtype=torch.int32); tok = torch.zeros(B, T, dtype=torch.int32)
    tl = torch.zeros(B, dtype=torch.int32); kl = torch.zeros(B, dtype=torch.int32)
    refs, hyps = [], []
    for b in range(B):
        r = _rand_seq(rng, int(rng.integers(1, L + 1)), 0.18, 27 if b % 2 else 4)
        h = _mutate(rng, r, 0.1)[:T] if b % 3 else _rand_seq(rng, int(rng.integers(0, T + 1)), 0.18, 27)
        tg[b, :len(r)] = torch.tensor(r, dtype=torch.int32); tl[b] = len(r)
        tok[b, :len(h)] = torch.tensor(h, dtype=torch.int32); kl[b] = len(h)
        refs.append(decode(r)); hyps.append(decode(h))
    cd, cl, wd, wc = metrics.edit_counts(tg.to(DEV), tl.to(DEV), tok.to(DEV), kl.to(DEV), D)
    assert all(t_.dtype == torch.int32 and t_.is_cuda and t_.shape == (B,) for t_ in (cd, cl, wd, wc))
    cd, cl, wd, wc = (t_.cpu().tolist() for t_ in (cd, cl, wd, wc))
    for b in range(B):
        cer, wer = metrics.evaluate(refs[b], hyps[b])
        assert cd[b] / cl[b] == cer and wd[b] / wc[b] == wer, b
        assert (cd[b], wd[b], wc[b]) == (decode_ref.edit_dist(refs[b], hyps[b])[0],
                                         decode_ref.edit_dist(refs[b].split(" "), hyps[b].split(" "))[0], len(refs[b].split(" ")))
