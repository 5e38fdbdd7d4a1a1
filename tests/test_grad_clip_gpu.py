"""Gradient clipping by global norm on the device: the norm kernel against torch-CPU fp64, the clipped Adam against
``clip_grad_norm_`` + torch's Adam, and the trainer with ``max_grad_norm`` (bit-equal to the unclipped step where nothing is
clipped, the kernel-level oracle where something is, the non-finite guard, two RCCL ranks)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from policy_gradient_asr_amd.train_step import FLAG_PAD, PolicyGradientTrainer
from pg_harness import make_batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAT_WORDS = 4787229        # parameters of Seq2Seq(29, n_feats=80): the trainer's flat size minus FLAG_PAD (checked below)


def _bits(x):
    return int(np.asarray(x, dtype=np.float32).reshape(()).view(np.int32))


def _ulps(a, b):
    """Distance in fp32 ulps of two positive finite fp32 numbers."""
    return abs(_bits(a) - _bits(b))


def _want_norm(g_cpu):
    """float32(sqrt(float64 sum of squares)) on the CPU -- the oracle of the norm."""
    return np.float32(float(g_cpu.double().pow(2).sum().sqrt()))


def _want_scale(norm32, max_norm):
    """clip_grad_norm_'s arithmetic in fp32, applied to an fp32 norm."""
    with np.errstate(over="ignore"):
        return np.minimum(np.float32(1.0), np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6)))


def _buffer(n, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g, dtype=torch.float64)
    if kind == "wide":          # magnitudes spread log-uniformly over 1e-20 .. 1e+15
        x = x * 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 35.0 - 20.0)
    elif kind == "tiny":        # every square (1e-40) is below the smallest normal fp32
        x = x * 1e-20
    elif kind == "big":
        x = x * 1e15
    return x.float()


def _state_words(state):
    f = state.cpu()
    i = f.view(torch.int32)
    return {"norm": f[0].numpy(), "scale": f[1].numpy(), "nonfinite": int(i[2]), "n_clipped": int(i[4]), "n_nonfinite": int(i[5])}


def test_flat_size_constant():
    from policy_gradient_asr_amd.model import Seq2Seq
    assert sum(p.numel() for p in Seq2Seq(29, n_feats=80).parameters()) == FLAT_WORDS


@pytest.mark.parametrize("n", [1, 3, 4, 1023, 65537, FLAT_WORDS])
@pytest.mark.parametrize("kind", ["wide", "tiny", "big"])
def test_norm_kernel_vs_fp64(n, kind):
    """norm within ONE fp32 ulp of float32(sqrt(fp64 sum)): the squares are exact in fp64 and the fp64 summation error is
    <= n 2^-53 relative, far below half an fp32 ulp, so only the final rounding (and its double rounding through the fp64 root)
    is left.  scale is the fp32 formula on the kernel's own norm; a second launch gives the same bits; the counts advance."""
    from policy_gradient_asr_amd import hipops
    g_cpu = _buffer(n, kind, seed=n % 1000 + len(kind))
    want = _want_norm(g_cpu)
    assert np.isfinite(want) and want > 0
    g = g_cpu.to(DEV)
    state = hipops.clip_state(g.device)
    expect_clipped = 0
    for max_norm in (float(want) * 0.5, float(want) * 2.0, float("inf"), float(want) * 0.25):
        hipops.grad_norm_clip(g, max_norm, state)
        w = _state_words(state)
        print(f"n={n} {kind}: norm {float(w['norm']):.9g} want {float(want):.9g} ulps {_ulps(w['norm'], want)} max {max_norm:.6g} scale {float(w['scale']):.9g}")
        assert _ulps(w["norm"], want) <= 1
        # max_norm travels as an fp32 argument
        assert _bits(w["scale"]) == _bits(_want_scale(w["norm"], np.float32(max_norm)))
        assert w["nonfinite"] == 0
        clipped = bool(_want_scale(want, np.float32(max_norm)) < 1.0)      # the bounds are factors of two away from the norm: no edge case
        assert (float(w["scale"]) < 1.0) == clipped and (clipped or _bits(w["scale"]) == _bits(1.0))
        expect_clipped += clipped
        assert (w["n_clipped"], w["n_nonfinite"]) == (expect_clipped, 0)
        again = hipops.grad_norm_clip(g, max_norm)                     # a fresh state: same bits
        w2 = _state_words(again)
        assert _bits(w2["norm"]) == _bits(w["norm"]) and _bits(w2["scale"]) == _bits(w["scale"])
        assert (w2["n_clipped"], w2["n_nonfinite"]) == (int(clipped), 0)


@pytest.mark.parametrize("n", [65537, FLAT_WORDS])        # both leave a tail of one word behind the last quad
@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")])
def test_norm_kernel_flags_non_finite_elements(n, value):
    from policy_gradient_asr_amd import hipops
    assert n % 4 == 1
    g = _buffer(n, "wide", seed=5).to(DEV)
    state = hipops.clip_state(g.device)
    hipops.grad_norm_clip(g, 1.0, state)
    assert _state_words(state)["nonfinite"] == 0
    before = _state_words(state)["n_clipped"]
    for k, pos in enumerate((0, n // 2, n - 1), 1):       # first, a middle and the last (tail) element
        bad = g.clone()
        bad[pos] = value
        hipops.grad_norm_clip(bad, 1.0, state)
        w = _state_words(state)
        assert w["nonfinite"] == 1 and float(w["scale"]) == 0.0 and not np.isfinite(w["norm"]), (pos, w)
        assert (w["n_clipped"], w["n_nonfinite"]) == (before, k)        # a skipped step is not a clipped one
    hipops.grad_norm_clip(g, 1.0, state)                  # a clean gradient clears the flag; the counts stay
    w = _state_words(state)
    assert w["nonfinite"] == 0 and w["n_nonfinite"] == 3 and np.isfinite(w["norm"])


def test_clipped_adam_kernel_matches_torch():
    """test_adam_kernel_matches_torch's loop with clip_grad_norm_ in it; the gradients' norms alternate around the bound."""
    from policy_gradient_asr_amd import hipops
    g = torch.Generator().manual_seed(0)
    bound = 10.0                # randn(10007) * 0.1 has norm ~ 10
    p0 = torch.randn(10007, generator=g)
    grads = [torch.randn(10007, generator=g) * 0.1 * f for f in (0.5, 2.0, 0.8, 3.0, 1.5)]
    ref = torch.nn.Parameter(p0.clone()); opt = torch.optim.Adam([ref], lr=5e-4)
    p = p0.clone().to(DEV); m = torch.zeros_like(p); v = torch.zeros_like(p)
    state = hipops.clip_state(p.device)
    clipped = []
    for i, gr in enumerate(grads):
        ref.grad = gr.clone()
        norm = float(torch.nn.utils.clip_grad_norm_([ref], bound))
        opt.step()
        gd = gr.to(DEV)
        twin = [t.clone() for t in (p, m, v)]
        hipops.grad_norm_clip(gd, bound, state)
        hipops.adam_step(p, gd, m, v, i + 1, lr=5e-4, clip_state=state)
        w = _state_words(state)
        assert float(w["norm"]) == pytest.approx(norm, rel=1e-6)
        clipped.append(float(w["scale"]) < 1.0)
        assert clipped[-1] == (norm > bound)
        if not clipped[-1]:     # scale == 1: the bits of the unclipped kernel
            assert _bits(w["scale"]) == _bits(1.0)
            hipops.adam_step(twin[0], gd, twin[1], twin[2], i + 1, lr=5e-4)
            for a, b in zip(twin, (p, m, v)):
                assert torch.equal(a, b)
        torch.testing.assert_close(p.cpu(), ref.detach(), rtol=1e-5, atol=1e-7)
        # the first moment is linear in the scale (the update itself is nearly invariant to it)
        torch.testing.assert_close(m.cpu(), opt.state[ref]["exp_avg"], rtol=1e-5, atol=1e-7)
    assert clipped == [False, True, False, True, True]
    assert (w["n_clipped"], w["n_nonfinite"]) == (3, 0)


def test_clipped_adam_skips_a_non_finite_gradient():
    from policy_gradient_asr_amd import hipops
    g = torch.Generator().manual_seed(1)
    p = torch.randn(10007, generator=g).to(DEV); m = torch.rand(10007, generator=g).to(DEV); v = torch.rand(10007, generator=g).to(DEV)
    gr = (torch.randn(10007, generator=g) * 0.1).to(DEV)
    applied = torch.zeros(2, dtype=torch.int32, device=DEV)
    state = hipops.clip_state(p.device)
    hipops.grad_norm_clip(gr, 1.0, state)
    hipops.adam_step(p, gr, m, v, 1, applied=applied, clip_state=state)
    assert applied.tolist() == [0, 1]
    snap = [t.clone() for t in (p, m, v)]
    bad = gr.clone(); bad[77] = float("nan")
    hipops.grad_norm_clip(bad, 1.0, state)
    assert _state_words(state)["nonfinite"] == 1
    hipops.adam_step(p, bad, m, v, 2, applied=applied, clip_state=state)
    for a, b in zip(snap, (p, m, v)):
        assert torch.equal(a, b)                          # parameters and moments untouched
    assert applied.tolist() == [1, 1]                     # the call's word holds the count BEFORE it: not advanced
    hipops.grad_norm_clip(gr, 1.0, state)
    hipops.adam_step(p, gr, m, v, 3, applied=applied, clip_state=state)
    assert applied.tolist() == [1, 2] and not torch.equal(snap[0], p) and bool(torch.isfinite(p).all())


# ---- the trainer ----
def _trainer_and_batch(max_grad_norm, precision, cls=PolicyGradientTrainer, B=20, T=60):
    """The mid-size train-mode trainer of tests/test_train_step_gpu.py (_trainer_and_batch), with a precision and a bound."""
    from policy_gradient_asr_amd.model import Seq2Seq, weights
    F, V, L = 80, 29, 6
    x, targets, fmask, tmask = make_batch(B, F, T, V, L, [T] * (B // 2) + [T - 19] * (B - B // 2), [6] * B, 3)
    torch.manual_seed(0)
    m = Seq2Seq(V, n_feats=F); m.apply(weights); m = m.to(DEV).train()
    tr = cls(m, lr=1e-3, lam=1.0, seed=5, precision=precision, max_grad_norm=max_grad_norm)
    return tr, tuple(t.to(DEV) for t in (x, targets, fmask, tmask))


def _run(tr, batch, steps):
    out = []
    for _ in range(steps):
        loss = tr.step(*batch)
        torch.cuda.synchronize()
        out.append((loss.clone(), tr.gflat.clone(), tr.flat.clone()))
    return out


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_trainer_with_an_infinite_bound_gives_the_unclipped_bits_and_measures_the_norm(mode):
    tr0, batch = _trainer_and_batch(None, mode)
    assert tr0.last_grad_norm is None and tr0.clip_state is None
    plain = _run(tr0, batch, 3)
    tr1, batch = _trainer_and_batch(float("inf"), mode)
    for i in range(3):
        loss = tr1.step(*batch)
        torch.cuda.synchronize()
        assert torch.equal(loss, plain[i][0]) and torch.equal(tr1.gflat, plain[i][1]) and torch.equal(tr1.flat, plain[i][2])
        want = _want_norm(tr1.gflat[FLAG_PAD:].cpu())
        got = tr1.last_grad_norm.cpu().numpy()
        print(f"{mode} step {i + 1}: last_grad_norm {float(got):.9g} fp64 {float(want):.9g} ulps {_ulps(got, want)}")
        assert tr1.last_grad_norm.dim() == 0 and tr1.last_grad_norm.is_cuda
        assert _ulps(got, want) <= 1
    assert tr1.clip_counts() == (0, 0) and tr1.applied_steps() == 3


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_trainer_clips_the_first_step_like_the_kernel_level_oracle(mode):
    """The bound is half the MEASURED norm of the first step, so no gradient magnitude is assumed: step 1 is clipped, gflat keeps
    the unclipped gradient, and parameters and first moment are clip_grad_norm_ + torch's Adam applied to that gradient."""
    tr0, batch = _trainer_and_batch(float("inf"), mode)
    p0 = tr0.flat[FLAG_PAD:].cpu().clone()
    tr0.step(*batch)
    torch.cuda.synchronize()
    n0 = float(tr0.last_grad_norm)
    g1 = tr0.gflat.clone()
    tr, batch = _trainer_and_batch(n0 / 2, mode)
    assert torch.equal(tr.flat[FLAG_PAD:].cpu(), p0)
    tr.step(*batch)
    torch.cuda.synchronize()
    print(f"{mode}: first-step norm {n0:.9g}, bound {n0 / 2:.9g}, counts {tr.clip_counts()}")
    assert tr.clip_counts()[0] >= 1 and tr.clip_counts()[1] == 0 and tr.applied_steps() == 1
    assert float(tr.last_grad_norm) == n0
    assert torch.equal(tr.gflat, g1)                      # Adam reads scale * g; the buffer keeps the reduced gradient itself
    ref = torch.nn.Parameter(p0.clone()); opt = torch.optim.Adam([ref], lr=1e-3)
    ref.grad = g1[FLAG_PAD:].cpu().clone()
    torch.nn.utils.clip_grad_norm_([ref], n0 / 2)
    opt.step()
    torch.testing.assert_close(tr.flat[FLAG_PAD:].cpu(), ref.detach(), rtol=1e-5, atol=1e-7)
    # The parameters hardly notice the scale (Adam's first update is lr * g / (|g| + eps)); the first moment, 0.1 * scale * g, does.
    # torch's fp32 norm of 4.79 M words on the CPU is itself off by ~1e-4 relative (measured: 1.7e-4 on a vector of this length),
    # so the moment is compared with the rule evaluated in fp64 instead: scale = min(1, max / (norm64 + 1e-6)), fp32 rounding only.
    g64 = g1[FLAG_PAD:].double().cpu()
    scale = min(1.0, (n0 / 2) / (float(g64.norm()) + 1e-6))
    m_want = (0.1 * scale * g64).float()
    assert 0.49 < scale < 0.51
    torch.testing.assert_close(tr.exp_avg[FLAG_PAD:].cpu(), m_want, rtol=1e-5, atol=1e-7 * float(m_want.abs().max()))
    # .. and torch's own clipped first moment agrees to the accuracy of its norm
    torch.testing.assert_close(tr.exp_avg[FLAG_PAD:].cpu(), opt.state[ref]["exp_avg"], rtol=1e-3, atol=1e-7 * float(m_want.abs().max()))


class PoisonedTrainer(PolicyGradientTrainer):
    """Writes an inf into the reduced gradient of its SECOND step, between backward and the update (reduce_rest is what every step
    calls just before the update)."""
    poison_call = 1

    def reduce_rest(self):
        super().reduce_rest()
        if self.nstep == self.poison_call:
            self.gflat[FLAG_PAD + 12345] = float("inf")


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_trainer_skips_a_non_finite_gradient_and_goes_on(mode):
    tr, batch = _trainer_and_batch(float("inf"), mode, cls=PoisonedTrainer)
    tr.step(*batch)
    torch.cuda.synchronize()
    assert tr.applied_steps() == 1 and tr.clip_counts() == (0, 0)
    snap = [t.clone() for t in (tr.flat, tr.exp_avg, tr.exp_avg_sq)]
    tr.step(*batch)                                       # the poisoned one
    torch.cuda.synchronize()
    assert tr.nstep == 2 and tr.applied_steps() == 1 and tr.clip_counts() == (0, 1)
    assert not np.isfinite(float(tr.last_grad_norm))
    for a, b in zip(snap, (tr.flat, tr.exp_avg, tr.exp_avg_sq)):
        assert torch.equal(a[FLAG_PAD:], b[FLAG_PAD:])
    tr.step(*batch)
    torch.cuda.synchronize()
    assert tr.nstep == 3 and tr.applied_steps() == 2 and tr.clip_counts() == (0, 1)
    assert np.isfinite(float(tr.last_grad_norm)) and bool(torch.isfinite(tr.flat).all())
    # bias correction with the APPLIED count (2), not the call count (3): replay the update on the host
    b1, b2, lr, eps = 0.9, 0.999, tr.lr, 1e-8
    g = tr.gflat[FLAG_PAD:].double().cpu()
    m = snap[1][FLAG_PAD:].double().cpu() * b1 + (1 - b1) * g
    v = snap[2][FLAG_PAD:].double().cpu() * b2 + (1 - b2) * g * g
    p = snap[0][FLAG_PAD:].double().cpu()
    want = p - lr * (m / (1 - b1 ** 2)) / ((v / (1 - b2 ** 2)).sqrt() + eps)
    wrong = p - lr * (m / (1 - b1 ** 3)) / ((v / (1 - b2 ** 3)).sqrt() + eps)
    got = tr.flat[FLAG_PAD:].double().cpu()
    assert float((got - want).abs().max() / want.abs().max()) < 1e-5
    assert float((got - want).abs().max()) < 0.2 * float((wrong - want).abs().max())


def test_two_rccl_ranks_clip_alike(tmp_path):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL does not take two ranks on one device)")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import grad_clip_rccl_worker as gw
    dev = torch.device("cuda", 0)
    # the bound: half the global-batch gradient's norm, measured by one process holding the whole batch
    batch = [t.to(dev) for t in gw.w.make_batch(16, 80, 60, 29, 6)]
    probe = gw.build(dev, 1, 0, float("inf"))
    probe.step(*batch)
    torch.cuda.synchronize()
    n0 = float(probe.last_grad_norm)
    bound = n0 / 2
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    worker = os.path.join(ROOT, "tests", "grad_clip_rccl_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", str(port), str(tmp_path), repr(bound)]) for r in range(2)]
    try:
        for p in procs:
            assert p.wait(timeout=600) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    res = [torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(2)]
    assert all(r["world"] == 2 for r in res)
    assert torch.equal(res[0]["flat"], res[1]["flat"])                          # replicas bit-identical after two clipped steps
    assert torch.equal(res[0]["norms"].view(torch.int32), res[1]["norms"].view(torch.int32))
    assert res[0]["counts"] == res[1]["counts"] == (2, 0) and res[0]["applied"] == res[1]["applied"] == 2
    assert float(res[0]["norms"][0]) == pytest.approx(n0, rel=1e-5)             # the norm of the SUMMED gradient
    assert all(bool(torch.isfinite(r["flat"]).all()) for r in res)


def test_train_driver_passes_the_bound_logs_the_norm_and_records_it(tmp_path, capsys):
    """model.train(max_grad_norm=...): the trainer gets the bound, the log lines carry the norm and the counts, the checkpoint
    records it and a resume with another value warns; with None the lines are the old ones."""
    from policy_gradient_asr_amd.data import SyntheticSpeech
    from policy_gradient_asr_amd.model import train
    corpus = tmp_path / "corpus"; out = tmp_path / "run"
    corpus.mkdir()
    (corpus / "alphabet.txt").write_text("a\nb\nc\nd\n \n")
    char2ind = {"<pad>": 0, "a": 1, "b": 2, "c": 3, "d": 4, " ": 5}
    ds = SyntheticSpeech(48, char2ind, n_feats=20, seed=1)
    kw = dict(train_dataset=ds, n_feats=20, lam=0.0, lr=3e-3, log_every=1)
    l1, _ = train(str(corpus), str(out), 2, 16, 0, max_grad_norm=0.5, **kw)
    text = capsys.readouterr().out
    assert text.count(" Grad norm: ") == 6 and "Clipped steps: " in text and "Skipped (non-finite gradient): 0" in text
    assert all(np.isfinite(l1)) and torch.load(out / "checkpoint_last.pth")["max_grad_norm"] == 0.5
    train(str(corpus), str(out), 3, 16, 0, max_grad_norm=None, **kw)
    text = capsys.readouterr().out
    assert "Warning: resuming with max_grad_norm=None but the checkpoint was written with 0.5" in text
    assert "Grad norm" not in text and "Clipped steps" not in text and text.count("Step ") == 3
    with pytest.raises(ValueError):
        train(str(corpus), str(tmp_path / "other"), 1, 16, 0, max_grad_norm=-1.0, **kw)
