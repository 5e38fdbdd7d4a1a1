"""Plumbing shared by the GPU test modules of the policy-gradient objective: batches and lattice cases, the trainers of the
accumulation tests, one trainer step against the fp64 oracle (oracle/model_ref.py forward and backward around
oracle/pg_ref.pg_objective), the shard identity and the corpus of the train-driver tests.  A plain module: no test, no fixture."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import ctc_ref, decode_ref, model_ref, pg_ref

DEV = "cuda:0"
D = 28                                   # the word delimiter of the V = 29 cases: ids 1..27 letters, 28 = " "


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


# ---- batches and lattice cases ----
def make_batch(B, F, T, V, L, lens, tlens, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, F, T, generator=g)
    fmask = torch.zeros(B, T)
    for b, n in enumerate(lens):
        fmask[b, :n] = 1; x[b, :, n:] = 0
    targets = torch.randint(1, V, (B, L), generator=g)
    tmask = torch.zeros(B, L, dtype=torch.int64)
    for b, n in enumerate(tlens):
        tmask[b, :n] = 1; targets[b, n:] = 0
    return x, targets, fmask, tmask


def spaced_batch(B, F, T, V, L, lens, tlens, seed):
    """make_batch's batch with about 18 % of the target symbols replaced by the delimiter."""
    x, targets, fmask, tmask = make_batch(B, F, T, V, L, lens, tlens, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    sp = (torch.rand(B, L, generator=g) < 0.18) & (tmask > 0)
    targets[sp] = D
    return x, targets, fmask, tmask


def lattice_case(T, B, V, L, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(T, B, V, generator=g, dtype=torch.float64) * 2
    targets = torch.randint(1, V, (B, L), generator=g, dtype=torch.int32)
    in_len = torch.tensor([T - 37 * (b % 4) for b in range(B)], dtype=torch.int32)
    tg_len = torch.tensor([L - 3 * (b % 3) for b in range(B)], dtype=torch.int32)
    return logits, targets, in_len, tg_len


def spaced_lattice_case(T, B, V, L, seed):
    logits, targets, in_len, tg_len = lattice_case(T, B, V, L, seed)
    g = torch.Generator().manual_seed(seed + 1)
    targets[torch.rand(B, L, generator=g) < 0.18] = D
    return logits, targets, in_len, tg_len


def sampled_case(T, B, V, K, seed=44, philox=11, offset=4, in_len=None, blank_path=None):
    """lattice_case's logits and targets, K paths per utterance from the device sampler, their collapsed hypotheses.
    blank_path = (k, b): that sample is replaced by the all-blank path (an empty hypothesis)."""
    from policy_gradient_asr_amd import hipops
    logits, targets, il, tg_len = lattice_case(T, B, V, 14, seed)
    if in_len is not None:
        il = torch.tensor(in_len, dtype=torch.int32)
    lp = hipops.log_softmax_rows(logits.float().to(DEV))
    _, paths = hipops.frame_sample_multi(lp, K, seed=philox, offset=offset)
    if blank_path is not None:
        paths[blank_path[0], :, blank_path[1]] = 0
    ild = il.to(DEV)
    tokens, tok_len = hipops.ctc_collapse(paths, ild)
    torch.cuda.synchronize()
    # the device's collapse is the oracle's
    pn, tn, ln = paths.cpu().numpy(), tokens.cpu().numpy(), tok_len.cpu().numpy()
    for k in range(K):
        for b in range(B):
            want = decode_ref.collapse_path(pn[k, :int(il[b]), b])
            assert list(tn[k, b, :ln[k, b]]) == list(want)
    return dict(lp=lp, lg=lp.double().cpu().numpy(), targets=targets, in_len=il, tg_len=tg_len, paths=paths, tokens=tokens,
                tok_len=tok_len, T=T, B=B, V=V, K=K)


def fused_grad_ref(c, coef, scale, Lh):
    """fp64: the target part, then the oracle's K capped sequence terms on the device's paths (pg_ref.score_terms: per sample the
    hypothesis' CTC gradient where it is sequence-scored, the path term where it is not)."""
    lg, il = c["lg"], c["in_len"].numpy()
    _, g_ctc = ctc_ref.ctc_loss_and_grad(lg, c["targets"].numpy(), il, c["tg_len"].numpy())
    _, g_pg, _, scored = pg_ref.score_terms(lg, il, c["paths"].cpu().numpy(), coef.double().numpy(), "sequence", Lh)
    assert np.array_equal(scored, c["tok_len"].cpu().numpy() <= Lh)
    return g_ctc * scale.double().numpy()[None, :, None] + g_pg


# ---- the accumulation tests' batch (F, T, V, L = 80, 60, 29, 6) and trainers ----
ACC_F, ACC_T, ACC_V, ACC_L = 80, 60, 29, 6


def _lens(B):
    return [ACC_T - (3 * b) % 17 for b in range(B)], [max(1, ACC_L - b % 4) for b in range(B)]


def _batch(B, seed=8):
    lens, tlens = _lens(B)
    return tuple(v.to(DEV) for v in make_batch(B, ACC_F, ACC_T, ACC_V, ACC_L, lens, tlens, seed)), lens


def _trainer(precision="f32", train=False, **kw):
    from policy_gradient_asr_amd.model import Seq2Seq, weights
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    torch.manual_seed(0)
    m = Seq2Seq(ACC_V, n_feats=ACC_F); m.apply(weights); m = m.to(DEV)
    m = m.train() if train else m.eval()
    kw.setdefault("seed", 4)
    return PolicyGradientTrainer(m, lam=1.0, precision=precision, **kw)


def _rows(batch, idx):
    idx = torch.as_tensor(idx, device=DEV)
    return tuple(t.index_select(0, idx).contiguous() for t in batch)


def _slices(sizes):
    out, o = [], 0
    for n in sizes:
        out.append(list(range(o, o + n)))
        o += n
    return out


# ---- one trainer step against the fp64 oracle ----
def load_params(m, p):
    """The oracle's parameters (model_ref.init_params names) into a Seq2Seq."""
    m.load_state_dict({("encoder." + k if not k.startswith("head.") else k): v for k, v in p.items()}, strict=True)
    return m


def oracle_model(F, V, seed, head_gain=1.0):
    """(params, fp64 leaf params, Seq2Seq on the device loaded with them); head_gain multiplies the head's weight and bias."""
    from policy_gradient_asr_amd.model import Seq2Seq
    p = model_ref.init_params(n_feats=F, vocab=V, seed=seed)
    p = {k: (v * head_gain if k.startswith("head.") else v) for k, v in p.items()}
    pr = {k: v.double().requires_grad_(True) for k, v in p.items()}
    return p, pr, load_params(Seq2Seq(V, n_feats=F), p).to(DEV).eval()


def param_errs(m, want):
    """rel_err of every parameter gradient of the device model against ``want`` (oracle names -> gradients)."""
    errs = {}
    for k, v in m.named_parameters():
        rk = k[len("encoder."):] if k.startswith("encoder.") else k
        errs[rk] = rel_err(v.grad.cpu(), want[rk])
    return errs


def step_batch(B=4, word=False, seed=51):
    """The batch of the step-vs-oracle tests: F, T, V = 80, 120, 29, the last B of four ragged utterances; returns
    (x, targets, fmask, tmask), lens, tlens."""
    lens = [120, 90, 120, 64][-B:]
    if word:
        tlens = [16, 11, 14, 7][-B:]
        return spaced_batch(B, 80, 120, 29, 16, lens, tlens, seed), lens, tlens
    tlens = [12, 9, 12, 5][-B:]
    return make_batch(B, 80, 120, 29, 12, lens, tlens, seed), lens, tlens


def oracle_step(pr, batch, lens, tlens, **objective_kw):
    """The fp64 side of a step (no GPU): the torch-CPU model's logits on fp64 leaf params pr, pg_ref.pg_objective on them with the
    sampler address of a trainer's first step (seed 3, offset 1), its gradient back-propagated.  Returns oracle (the pg_objective
    result), args (logits, lengths, targets), kw (the keywords), grads (parameter gradients) and backprop(d_logits) -> gradients."""
    x, targets, fmask, _ = batch
    logits_ref = model_ref.head_logits_torch(pr, model_ref.encoder_forward_torch(pr, x.double(), fmask, packed=True))
    args = (logits_ref.detach().numpy(), np.array(lens), targets.numpy(), np.array(tlens))
    kw = dict(lam=1.0, seed=3, offset=1, **objective_kw)
    o = pg_ref.pg_objective(*args, **kw)

    def backprop(d_logits):
        for v in pr.values():
            v.grad = None
        logits_ref.backward(torch.from_numpy(d_logits), retain_graph=True)
        return {k: v.grad.clone() for k, v in pr.items()}

    return SimpleNamespace(oracle=o, args=args, kw=kw, grads=backprop(o.grad), backprop=backprop)


def trainer_step_vs_oracle(trainer_kw, objective_kw, *, B=4, word=False, head_gain=1.0, seed, tol_loss=1e-5, tol_grad=1e-4, label):
    """One lambda = 1 trainer step (f32 mode, eval-mode dropout) on step_batch against oracle_step on the same weights: rewards exact
    (rtol 1e-6), loss within tol_loss, every parameter gradient within tol_grad (max norm).  The device makes its discrete choices
    on its logits, the oracle on its own.  Returns oracle_step's result with trainer and errs (per parameter) added."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    batch, lens, tlens = step_batch(B, word, seed)
    p, pr, m = oracle_model(80, 29, seed + 1, head_gain)
    tr = PolicyGradientTrainer(m, lam=1.0, seed=3, precision="f32", **trainer_kw)
    loss = tr.compute_gradients(*(t.to(DEV) for t in batch))
    nll, R_s, R_b = tr.last_stats
    R_all = tr.last_sample_rewards
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    r = oracle_step(pr, batch, lens, tlens, **objective_kw)
    o = r.oracle
    np.testing.assert_allclose(R_all.cpu().numpy(), o.R, rtol=1e-6)
    np.testing.assert_allclose(R_s.cpu().numpy(), o.R.mean(axis=0), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(R_b.cpu().numpy(), o.baselines.mean(axis=0), rtol=1e-6, atol=1e-7)
    lerr = abs(float(loss) - o.loss) / abs(o.loss)
    assert lerr < tol_loss, (float(loss), o.loss)
    r.trainer, r.errs = tr, param_errs(m, r.grads)
    worst = max(r.errs, key=r.errs.get)
    print(f"{label}: loss rel err {lerr:.2e}; worst parameter gradient {worst} {r.errs[worst]:.2e}")
    assert r.errs[worst] < tol_grad, (worst, r.errs[worst])
    return r


# ---- two shards against the whole batch ----
def shards_vs_whole(kw, case, extra=None):
    """Two pg_ctc_loss calls on the halves of ``case`` (logits, targets, in_len, tg_len; global_batch and sample_base set) against
    one call on the whole batch: the same rewards bit for bit, logits gradient and loss within 1e-6.  ``extra()`` is read after
    every call (a PGCTCLossFn.last_* capture).  Returns loss, R_s, R_b and grad of the whole batch, extra_whole, extra_parts."""
    from policy_gradient_asr_amd.loss import pg_ctc_loss
    logits, targets, in_len, tg_len = case
    B, half = logits.shape[1], logits.shape[1] // 2
    lg = logits.float().to(DEV)
    tg, il, tl = targets.to(DEV), in_len.to(DEV), tg_len.to(DEV)
    whole = lg.clone().requires_grad_(True)
    loss, nll, R_s, R_b = pg_ctc_loss(whole, il, tg, tl, **kw)
    extra_whole = extra() if extra else None
    loss.backward()
    grads, total, extra_parts = [], 0.0, []
    for h in range(2):
        sl = slice(half * h, half * h + half)
        part = lg[:, sl].contiguous().requires_grad_(True)
        l_h, _, Rs_h, Rb_h = pg_ctc_loss(part, il[sl].contiguous(), tg[sl].contiguous(), tl[sl].contiguous(), global_batch=B,
                                         sample_base=half * h, **kw)
        if extra:
            extra_parts.append(extra())
        l_h.backward()
        grads.append(part.grad)
        total += float(l_h.detach())
        assert torch.equal(Rs_h, R_s[..., sl]) and torch.equal(Rb_h, R_b[sl])
    diff = (torch.cat(grads, dim=1) - whole.grad).abs().max()
    assert float(diff) <= 1e-6 * float(whole.grad.abs().max()), float(diff)
    loss = loss.detach()
    assert abs(total - float(loss)) <= 1e-6 * abs(float(loss))
    return SimpleNamespace(loss=loss, R_s=R_s, R_b=R_b, grad=whole.grad, lg=lg, tg=tg, il=il, tl=tl, extra_whole=extra_whole,
                           extra_parts=extra_parts)


# ---- the train driver's corpus ----
def tiny_corpus(tmp_path, n=32):
    """(corpus dir with the five-symbol alphabet.txt, run dir, SyntheticSpeech of n utterances with 20 features)."""
    from policy_gradient_asr_amd.data import SyntheticSpeech
    corpus = tmp_path / "corpus"; out = tmp_path / "run"
    corpus.mkdir()
    (corpus / "alphabet.txt").write_text("a\nb\nc\nd\n \n")
    char2ind = {"<pad>": 0, "a": 1, "b": 2, "c": 3, "d": 4, " ": 5}
    return corpus, out, SyntheticSpeech(n, char2ind, n_feats=20, seed=1)
