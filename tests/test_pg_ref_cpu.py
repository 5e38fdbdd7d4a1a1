"""oracle/pg_ref.py, the fp64 statement the GPU train steps are held to, against torch autograd of the same loss (no GPU)."""
import numpy as np
import pytest
import torch

from oracle import decode_ref, pg_ref
from pg_harness import rel_err

T, B, V, L, D = 40, 4, 7, 6, 6                     # D: the word delimiter of the word-reward configurations
IN_LEN, TG_LEN = np.array([40, 31, 40, 17]), np.array([6, 4, 0, 3])          # one empty target
SEED, OFFSET = 3, 1

CONFIGS = {
    "default": {},
    "K4_hypothesis": dict(num_samples=4),
    "K4_leave_one_out": dict(num_samples=4, baseline="leave_one_out"),
    "K4_beam4": dict(num_samples=4, beam=4),
    "sequence_leave_one_out": dict(num_samples=4, baseline="leave_one_out", score_function="sequence"),
    "sequence_capped": dict(num_samples=4, baseline="leave_one_out", score_function="sequence", max_hyp_len="median"),
    "word_leave_one_out": dict(num_samples=4, baseline="leave_one_out", reward_unit="word", word_delimiter=D),
    "word_sequence": dict(num_samples=4, baseline="leave_one_out", reward_unit="word", word_delimiter=D, score_function="sequence"),
    "per_step": dict(per_step=True),
}


def _case():
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(T, B, V, generator=g, dtype=torch.float64) * 2
    logits[:, :, 0] += 1.5
    targets = torch.randint(1, V - 1, (B, L), generator=g)
    targets[0, 2] = targets[1, 1] = targets[3, 0] = D                      # a delimiter inside, inside, and leading
    return logits.numpy(), targets.numpy()


def _torch_objective(logits, targets, o, kw):
    """The loss rebuilt from log_softmax, F.ctc_loss, gathers and the entropy sum; the oracle's coef, paths and hyps are constants."""
    z = torch.tensor(logits, requires_grad=True)
    lp = torch.log_softmax(z, 2)
    il, tl = torch.from_numpy(IN_LEN), torch.from_numpy(TG_LEN)
    mask = torch.arange(T)[:, None] < il[None, :]
    nll = torch.nn.functional.ctc_loss(lp, torch.from_numpy(targets), il, tl, blank=0, reduction="none")
    loss = (nll / (tl.clamp(min=1) * B)).sum()
    coef = torch.from_numpy(o.coef)
    for k in range(o.paths.shape[0]):
        picked = lp.gather(2, torch.from_numpy(o.paths[k])[..., None])[..., 0] * mask
        if kw.get("per_step"):
            loss = loss - (coef * picked).sum()
            continue
        term = -picked.sum(0)
        if kw.get("score_function") == "sequence":
            hl = torch.tensor([len(h) for h in o.hyps[k]])
            ht = torch.zeros(B, T, dtype=torch.long)
            for b in range(B):
                ht[b, :hl[b]] = torch.tensor(o.hyps[k][b], dtype=torch.long)
            seq = torch.from_numpy(o.scored[k])
            nll_h = torch.nn.functional.ctc_loss(lp, ht, il, torch.where(seq, hl, 0), blank=0, reduction="none")
            term = torch.where(seq, nll_h, term)
        loss = loss + (coef[k] * term).sum()
    beta = kw.get("entropy_weight", 0.0)
    H = -(lp.exp() * lp).sum(2) * mask
    loss = loss - (beta / (B * il.clamp(min=1).double()) * H.sum(0)).sum()
    loss.backward()
    return float(loss.detach()), z.grad.numpy()


@pytest.mark.parametrize("beta", [0.0, 2.0])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_pg_objective_vs_torch_autograd(name, beta):
    """loss and grad of every configuration against torch autograd in fp64: 1e-11 relative (max norm for the gradient), about 300
    times the fp64 noise of this shape and eight orders below any missing term.  Measured: loss <= 7.7e-16, gradient <= 1.8e-14."""
    logits, targets = _case()
    kw = dict(CONFIGS[name], lam=0.7, seed=SEED, offset=OFFSET, entropy_weight=beta)
    if kw.get("max_hyp_len") == "median":
        lens = [len(h) for row in pg_ref.pg_objective(logits, IN_LEN, targets, TG_LEN, **dict(kw, max_hyp_len=None)).hyps for h in row]
        kw["max_hyp_len"] = int(np.median(lens))
    o = pg_ref.pg_objective(logits, IN_LEN, targets, TG_LEN, **kw)
    K = kw.get("num_samples", 1)
    assert o.coef.shape == ((T, B) if kw.get("per_step") else (K, B)) and np.abs(o.coef).max() > 0          # no vacuous term
    assert o.R.shape == o.baselines.shape == o.scored.shape == (K, B) and o.paths.shape == (K, T, B)
    assert o.grad.shape == (T, B, V) and o.nll.shape == o.ent_mean.shape == (B,)
    if kw.get("score_function") != "sequence":
        assert not o.scored.any()
    elif name == "sequence_capped":
        assert o.scored.any() and not o.scored.all()
    else:
        assert o.scored.all()
    if kw.get("reward_unit") == "word":
        chars = pg_ref.pg_objective(logits, IN_LEN, targets, TG_LEN, **dict(kw, reward_unit="char"))
        assert (np.abs(o.R - chars.R) > 1e-6).any() and np.array_equal(o.nll, chars.nll)
    w_loss, w_grad = _torch_objective(logits, targets, o, kw)
    e_loss, e_grad = abs(o.loss - w_loss) / abs(w_loss), rel_err(o.grad, w_grad)
    print(f"[pg_ref] {name} beta={beta}: loss rel err {e_loss:.2e}, gradient rel err {e_grad:.2e}")
    assert e_loss < 1e-11 and e_grad < 1e-11


def test_an_infeasible_target_adds_nothing_to_the_loss():
    logits, targets = _case()
    il = IN_LEN.copy(); il[3] = 2                                           # three characters do not fit two frames
    o = pg_ref.pg_objective(logits, il, targets, TG_LEN, lam=0.0)
    assert np.isinf(o.nll[3]) and np.isfinite(o.loss) and (o.grad[:, 3] == 0).all()
    assert o.loss == (o.nll[:3] / (np.maximum(TG_LEN[:3], 1) * B)).sum()


def test_sampler_forms():
    logits, _ = _case()
    paths, cdf, u = pg_ref.sample_paths(logits, 4, SEED, OFFSET)
    one = decode_ref.sample_paths(logits, seed=SEED, offset=OFFSET)
    assert np.array_equal(pg_ref.sample_paths(logits, 1, SEED, OFFSET)[0][0], one[0]) and np.array_equal(paths[0], one[0])
    assert np.array_equal(u[0], one[2]) and np.array_equal(cdf, one[1])
    assert (paths[0] != paths[1]).mean() > 0.3                              # distinct draws
    # ids = base + arange against the stride of the whole batch: the whole batch's columns
    for base in (0, 2):
        ids = base + np.arange(2)
        assert np.array_equal(pg_ref.sampler_uniforms(T, ids, 4, SEED, OFFSET, B), u[:, :, base:base + 2])
        half = pg_ref.sample_paths(logits[:, base:base + 2], 4, SEED, OFFSET, ids=ids, stride=B)[0]
        assert np.array_equal(half, paths[:, :, base:base + 2])
    perm = [2, 0, 3, 1]
    assert np.array_equal(pg_ref.sample_paths(logits[:, perm], 4, SEED, OFFSET, ids=perm, stride=B)[0], paths[:, :, perm])


@pytest.mark.parametrize("name", ["K4_beam4", "per_step", "word_sequence"])
def test_overrides_reproduce_the_result(name):
    """The oracle's own paths, arg-max frames and baseline hypotheses handed back in: the same result exactly; other paths, another."""
    logits, targets = _case()
    kw = dict(CONFIGS[name], lam=0.7, entropy_weight=2.0)
    o = pg_ref.pg_objective(logits, IN_LEN, targets, TG_LEN, seed=SEED, offset=OFFSET, **kw)
    over = dict(paths=o.paths if name != "per_step" else o.paths[0], greedy_frames=np.argmax(logits, axis=2))
    if name == "K4_beam4":
        lp = np.log(np.exp(logits) / np.exp(logits).sum(axis=2, keepdims=True))
        over["hypotheses"] = []
        for b in range(B):
            hyp, _ = decode_ref.prefix_beam_search(np.exp(lp[:IN_LEN[b], b]), beam_size=4)
            over["hypotheses"].append([h for i, h in enumerate(hyp) if i == 0 or h != hyp[i - 1]])
    again = pg_ref.pg_objective(logits, IN_LEN, targets, TG_LEN, seed=99, offset=7, **kw, **over)        # the seed is not read
    assert again.loss == o.loss and np.array_equal(again.grad, o.grad) and np.array_equal(again.coef, o.coef)
    assert np.array_equal(again.R, o.R) and np.array_equal(again.baselines, o.baselines)
    other = pg_ref.pg_objective(logits, IN_LEN, targets, TG_LEN, seed=99, offset=7, **kw)
    assert not np.array_equal(other.paths, o.paths) and other.loss != o.loss
    if name == "K4_beam4":                                                  # a hypothesis of one's own is what the baseline scores
        over["hypotheses"] = [[] for _ in range(B)]
        empty = pg_ref.pg_objective(logits, IN_LEN, targets, TG_LEN, **kw, **over)
        np.testing.assert_array_equal(empty.R_hyp, -TG_LEN / np.maximum(TG_LEN, 1))


def test_split_words_is_str_split():
    for row in ([], [D], [D, 1, 2, D], [1, D, D, 2, D], [1, 2, 3]):
        text = "".join(" " if t == D else "abcde"[t - 1] for t in row)
        assert ["".join("abcde"[t - 1] for t in w) for w in pg_ref.split_words(row, D)] == text.split(" ")
