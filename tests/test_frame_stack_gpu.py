"""Low-frame-rate input on the device (csrc/frame_stack.hip, hipops.frame_stack, features.FrameStack): the kernel against the numpy
statement bit for bit, its refusals, shards, one train step on stacked input against the fp64 oracle, and the drivers."""
import os

import numpy as np
import pytest
import torch

import frame_stack_ref as R
from pg_harness import DEV, make_batch, oracle_model, oracle_step, param_errs, tiny_corpus

pytestmark = pytest.mark.gpu

TILE = 64                   # csrc/frame_stack.hip: output frames per workgroup
POLICIES = [(1, 1, 0), (2, 2, 0), (3, 3, 0), (3, 3, 1), (7, 3, 3), (8, 3, 7), (4, 1, 2), (2, 5, 0), (16, 16, 15)]
INVALID_ARG = 1


def _lengths(T, stack, skip):
    """Ragged frame counts: 0, 1, T, one with n % skip != 0 (where T allows), one below the stack (every tap clamped), T - 1, one
    inside the last tile."""
    odd = next((n for n in range(T, 0, -1) if n % skip), T)
    return [min(max(v, 0), T) for v in (0, 1, T, odd, stack - 1, T - 1, T - T // 3)]


def _nan_padded(B, F, T, lens, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, F, T, generator=g)
    for b, n in enumerate(lens):
        x[b, :, n:] = float("nan")          # a frame at or beyond n is never read into a written value
    return x


def _run_entry(x_dev, lens, stack, skip, left):
    """The C entry on NaN / -1 prefilled outputs: every word must be written."""
    from policy_gradient_asr_amd import _lib
    lib = _lib.load()
    B, F, T = x_dev.shape
    Tout = -(-T // skip)
    out = torch.full((B, stack * F, Tout), float("nan"), device=DEV)
    fm = torch.full((B, 1, Tout), float("nan"), device=DEV)
    n_out = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    n_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    st = lib.pgasr_frame_stack(x_dev.data_ptr(), n_dev.data_ptr(), B, F, T, stack, skip, left, Tout, out.data_ptr(), fm.data_ptr(),
                               n_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == 0, st
    torch.cuda.synchronize()
    return out.cpu().numpy(), fm.cpu().numpy(), n_out.cpu().numpy()


@pytest.mark.parametrize("policy", POLICIES, ids=lambda p: "x".join(map(str, p)))
def test_kernel_equals_the_reference_bit_for_bit(policy):
    """F in {1, 5, 80} x T in {1, 2, 63, 64, 65, 257} and the T that give T' = tile - 1, tile, tile + 1; outputs prefilled with NaN, the
    input's padding filled with NaN, ragged lengths.  Odd T: rows that are not 16-byte aligned (the one-float path); T % 4 == 0: the
    16-byte path, whose span begins below its first frame."""
    stack, skip, left = policy
    Ts = sorted({1, 2, 63, 64, 65, 257, (TILE - 1) * skip, TILE * skip, TILE * skip + 1})
    assert {-(-T // skip) for T in Ts} >= {TILE - 1, TILE, TILE + 1}
    for F in (1, 5, 80):
        for T in Ts:
            lens = _lengths(T, stack, skip)
            x = _nan_padded(len(lens), F, T, lens, seed=F * 1000 + T)
            out, fm, n_out = _run_entry(x.to(DEV), lens, stack, skip, left)
            want, want_fm, want_n = R.frame_stack_ref(x.numpy(), lens, stack, skip, left)
            assert not np.isnan(want).any()
            assert R.same_bits(out, want), (F, T)
            assert R.same_bits(fm, want_fm) and np.array_equal(n_out, want_n), (F, T)


def test_every_tap_clamped_and_misaligned_base():
    """stack > n for every utterance (all taps clamp to the few real frames), and a T % 4 == 0 batch whose base address is 4 bytes
    past a 16-byte boundary (the one-float path at an aligned T) next to the same batch aligned: the same bits."""
    lens = [1, 2, 3, 0]
    x = _nan_padded(4, 5, 12, lens, seed=9)
    out, _, n_out = _run_entry(x.to(DEV), lens, 8, 3, 7)
    want, _, want_n = R.frame_stack_ref(x.numpy(), lens, 8, 3, 7)
    assert R.same_bits(out, want) and np.array_equal(n_out, want_n)
    lens = [256, 100, 255, 7]
    x = _nan_padded(4, 5, 256, lens, seed=10)
    buf = torch.empty(x.numel() + 1, device=DEV)
    shifted = buf[1:].view(4, 5, 256)
    shifted.copy_(x)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    want = R.frame_stack_ref(x.numpy(), lens, 3, 3, 1)[0]
    assert R.same_bits(_run_entry(shifted, lens, 3, 3, 1)[0], want)
    assert R.same_bits(_run_entry(x.to(DEV), lens, 3, 3, 1)[0], want)


def test_wrapper_and_policy_object():
    """hipops.frame_stack with lengths, with the front end's fmask (lengths taken on the device) and with neither; the policy object
    returns the same tensors; NaN and inf in real frames travel unchanged."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.features import FrameStack
    lens = [130, 0, 77, 129]
    g = torch.Generator().manual_seed(4)
    x = torch.randn(4, 7, 130, generator=g)
    x[0, 3, 5], x[2, 0, 76], x[3, 6, 0] = float("nan"), float("inf"), -0.0
    fmask = torch.zeros(4, 1, 130)
    for b, n in enumerate(lens):
        fmask[b, 0, :n] = 1
    want, want_fm, want_n = R.frame_stack_ref(x.numpy(), lens, 3, 3, 0)
    xd = x.to(DEV)
    for kw in ({"lengths": torch.tensor(lens, dtype=torch.int32, device=DEV)}, {"fmask": fmask.to(DEV)}, {"fmask": fmask[:, 0].to(DEV)}):
        out, fm, n_out = hipops.frame_stack(xd, stack=3, skip=3, left=0, **kw)
        assert out.shape == (4, 21, 44) and fm.shape == (4, 1, 44) and n_out.dtype == torch.int32
        assert R.same_bits(out.cpu().numpy(), want) and R.same_bits(fm.cpu().numpy(), want_fm)
        assert np.array_equal(n_out.cpu().numpy(), want_n)
    out, fm, n_out = hipops.frame_stack(xd, stack=2, skip=5)
    assert R.same_bits(out.cpu().numpy(), R.frame_stack_ref(x.numpy(), [130] * 4, 2, 5, 0)[0]) and n_out.tolist() == [26] * 4
    fs = FrameStack(3, 3, 0)
    f2, m2 = fs(xd, fmask.to(DEV))
    assert R.same_bits(f2.cpu().numpy(), want) and R.same_bits(m2.cpu().numpy(), want_fm)
    f3, _ = fs(xd, lens)
    assert torch.equal(f3.view(torch.int32), f2.view(torch.int32))
    assert bool(fs.fits(torch.tensor([[1, 1, 2]], device=DEV), None, torch.tensor([4], device=DEV))[0])
    assert not bool(fs.fits(torch.tensor([[1, 1, 2]], device=DEV), None, torch.tensor([3], device=DEV))[0])


def test_refusals():
    """Every limit of the C entry (PGASR_ERR_INVALID_ARG, nothing launched: the pointers are never touched) and of the wrapper."""
    from policy_gradient_asr_amd import _lib, hipops
    lib = _lib.load()
    x = torch.zeros(2, 4, 9, device=DEV)
    n = torch.tensor([9, 4], dtype=torch.int32, device=DEV)
    out = torch.zeros(2, 64, 9, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def entry(xp=x.data_ptr(), np_=n.data_ptr(), B=2, F=4, T=9, stack=3, skip=3, left=0, Tout=3, op=out.data_ptr()):
        return lib.pgasr_frame_stack(xp, np_, B, F, T, stack, skip, left, Tout, op, None, None, st)

    assert entry() == 0                                          # the accepted call the refusals are variations of
    for kw in (dict(xp=None), dict(np_=None), dict(op=None), dict(op=x.data_ptr()), dict(B=0), dict(F=0), dict(T=0),
               dict(stack=0), dict(stack=17, Tout=3), dict(skip=0), dict(skip=17, Tout=1), dict(left=-1), dict(left=3),
               dict(stack=16, left=16), dict(stack=16, F=4096), dict(B=65536), dict(Tout=2), dict(Tout=4), dict(skip=2, Tout=4)):
        assert entry(**kw) == INVALID_ARG, kw
    assert entry(stack=16, skip=16, left=15, Tout=1) == 0 and entry(skip=2, Tout=5) == 0
    torch.cuda.synchronize()

    for bad, why in ((x.double(), "float32"), (x.cpu(), "GPU"), (x.transpose(1, 2), "contiguous"), (x[0], r"\(B,F,T\)"),
                     (x[:, :, :0], "empty")):
        with pytest.raises(ValueError, match=why):
            hipops.frame_stack(bad, stack=3, skip=3)
    for kw, why in ((dict(stack=0), "stack"), (dict(stack=17), "stack"), (dict(skip=0), "skip"), (dict(skip=17), "skip"),
                    (dict(left=-1), "left"), (dict(left=3), "left"), (dict(lengths=n.long()), "lengths"), (dict(lengths=n.cpu()), "lengths"),
                    (dict(lengths=n[:1]), "lengths"), (dict(lengths=n, fmask=torch.ones(2, 9, device=DEV)), "not both"),
                    (dict(fmask=torch.ones(2, 8, device=DEV)), "fmask"), (dict(fmask=torch.ones(2, 9)), "fmask")):
        with pytest.raises(ValueError, match=why):
            hipops.frame_stack(x, **{"stack": 3, "skip": 3, **kw})
    with pytest.raises(ValueError, match="output rows"):
        hipops.frame_stack(torch.zeros(1, 4096, 1, device=DEV), stack=16, skip=1)
    with pytest.raises(ValueError, match="utterances per call"):
        hipops.frame_stack(torch.zeros(65536, 1, 1, device=DEV), stack=1, skip=1)
    with pytest.raises(TypeError, match="integer"):
        hipops.frame_stack(x, stack=3.0, skip=3)


def test_shards_reproduce_the_whole_batch():
    """The two halves of a batch, each cut to its own longest utterance, give the whole batch's rows over their frames and zeros
    beyond: a row depends on nothing but its own utterance."""
    from policy_gradient_asr_amd import hipops
    lens = [200, 131, 97, 64]
    x, _, fmask, _ = make_batch(4, 80, 200, 29, 4, lens, [4, 4, 4, 4], seed=21)
    whole, wm, wn = hipops.frame_stack(x.to(DEV), fmask=fmask.to(DEV), stack=8, skip=3, left=7)
    for sl in (slice(0, 2), slice(2, 4)):
        Th = max(lens[sl])
        part, pm, pn = hipops.frame_stack(x[sl, :, :Th].contiguous().to(DEV), fmask=fmask[sl, :Th].contiguous().to(DEV), stack=8,
                                          skip=3, left=7)
        Tp = part.shape[2]
        assert Tp == -(-Th // 3) and torch.equal(pn, wn[sl])
        assert torch.equal(part.view(torch.int32), whole[sl, :, :Tp].view(torch.int32)) and torch.equal(pm, wm[sl, :, :Tp])
        assert not whole[sl, :, Tp:].any()


def test_train_step_on_stacked_input_against_the_fp64_oracle():
    """One lambda = 1 step at F = 240, T' = 40: pg_harness's ragged batch stacked (3, 3, 0) -- on the device for the trainer, by the
    reference for the oracle -- then the harness's step-vs-oracle comparison with its own bounds: rewards exact, loss within 1e-5,
    every parameter gradient within 1e-4 in max norm."""
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.features import FrameStack
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    seed = 83
    lens, tlens = [120, 90, 120, 64], [12, 9, 12, 5]
    x, targets, fmask, tmask = make_batch(4, 80, 120, 29, 12, lens, tlens, seed)
    fs = FrameStack(3, 3, 0)
    xs, fms = fs(x.to(DEV), fmask.to(DEV))
    want, want_fm, n_out = R.frame_stack_ref(x.numpy(), lens, 3, 3, 0)
    assert xs.shape == (4, 240, 40) and R.same_bits(xs.cpu().numpy(), want) and list(n_out) == [40, 30, 40, 22]
    assert bool(fs.fits(targets, torch.tensor(tlens), torch.from_numpy(n_out)).all())
    p, pr, m = oracle_model(240, 29, seed + 1)
    tr = PolicyGradientTrainer(m, lam=1.0, seed=3, precision="f32")
    loss = tr.compute_gradients(xs, targets.to(DEV), fms.squeeze(1), tmask.to(DEV))
    nll, R_s, R_b = tr.last_stats
    torch.cuda.synchronize()
    hipops.lstm_assert_no_timeouts()
    r = oracle_step(pr, (torch.from_numpy(want), targets, torch.from_numpy(want_fm[:, 0]), tmask), [int(v) for v in n_out], tlens)
    o = r.oracle
    np.testing.assert_allclose(tr.last_sample_rewards.cpu().numpy(), o.R, rtol=1e-6)
    np.testing.assert_allclose(R_s.cpu().numpy(), o.R.mean(axis=0), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(R_b.cpu().numpy(), o.baselines.mean(axis=0), rtol=1e-6, atol=1e-7)
    lerr = abs(float(loss) - o.loss) / abs(o.loss)
    errs = param_errs(m, r.grads)
    worst = max(errs, key=errs.get)
    print(f"stacked step F=240 T'=40: loss rel err {lerr:.2e}; worst parameter gradient {worst} {errs[worst]:.2e}")
    assert lerr < 1e-5, (float(loss), o.loss)
    assert errs[worst] < 1e-4, (worst, errs[worst])


def test_drivers_carry_the_policy(tmp_path, capsys):
    """model.train(frame_stack=) for one epoch on the tiny corpus, a resume, predict and align with the policy from the checkpoint,
    and the refusals of a conflicting policy.  The corpus loses no utterance under this policy (tests/test_frame_stack_cpu.py)."""
    from policy_gradient_asr_amd.data import collate_custom
    from policy_gradient_asr_amd.features import FrameStack
    from policy_gradient_asr_amd.model import align, predict, train
    fs = FrameStack(*R.DRIVER_POLICY)
    corpus, out, ds = tiny_corpus(tmp_path, R.DRIVER_UTTERANCES)
    b = collate_custom([ds[0], ds[1], ds[2]], device=DEV, frame_stack=fs)
    T = max(ds[i]["feat"].shape[1] for i in range(3))
    assert b["feat"].shape == (3, 20 * fs.stack, fs.out_frames(T)) and b["fmask"].shape == (3, 1, fs.out_frames(T))
    assert b["fmask"].sum((1, 2)).tolist() == [fs.out_frames(ds[i]["feat"].shape[1]) for i in range(3)]
    kw = dict(train_dataset=ds, n_feats=20, lam=1.0, lr=3e-3, log_every=0)
    l1, _ = train(str(corpus), str(out), 1, 16, 0, frame_stack=R.DRIVER_POLICY, **kw)
    assert len(l1) == 1 and np.isfinite(l1[0])
    assert "does not fit their stacked frames (zero weight): 0" in capsys.readouterr().out
    st = torch.load(out / "checkpoint_last.pth", map_location="cpu")
    assert st["frame_stack"] == fs.state() and st["model"]["encoder.input_layer.weight"].shape == (512, 60)
    with pytest.raises(ValueError, match="frame_stack"):
        train(str(corpus), str(out), 2, 16, 0, frame_stack=(3, 3), **kw)
    with pytest.raises(ValueError, match="frame_stack"):
        train(str(corpus), str(out), 2, 16, 0, **kw)
    l2, _ = train(str(corpus), str(out), 2, 16, 0, frame_stack=fs, **kw)
    assert len(l2) == 2 and l2[0] == pytest.approx(l1[0]) and np.isfinite(l2[1])
    assert "Resumed from epoch 1" in capsys.readouterr().out

    alphabet = str(corpus / "alphabet.txt")
    pk = dict(test_dataset=ds, n_feats=20)
    with pytest.raises(ValueError, match="frame_stack"):
        predict(None, None, alphabet, str(out), 16, beam_size=0, frame_stack=(3, 3), **pk)
    with pytest.raises(ValueError, match="frame_stack"):
        align(None, None, alphabet, str(out), 16, frame_stack=(2, 2), **pk)
    cer, wer = predict(None, None, alphabet, str(out), 16, beam_size=0, **pk)           # the policy comes from the checkpoint
    assert np.isfinite(cer) and np.isfinite(wer) and len(open(out / "predicted.txt").read().splitlines()) == len(ds)
    assert predict(None, None, alphabet, str(out), 16, beam_size=0, frame_stack=fs, **pk) == (cer, wer)

    scores = align(None, None, alphabet, str(out), 16, **pk)
    assert len(scores) == len(ds) and all(np.isfinite(scores))                          # every transcript fits: every one aligns
    rows = [ln.split("\t") for ln in open(out / "alignments.tsv").read().splitlines()]
    assert len(rows) == sum(len(ds[i]["trans"]) for i in range(len(ds)))
    for u in range(len(ds)):
        n = ds[u]["feat"].shape[1]
        spans = [(int(r[3]), int(r[4])) for r in rows if int(r[0]) == u]
        assert len(spans) == len(ds[u]["trans"])
        prev = 0
        for s, e in spans:
            assert s % fs.skip == 0 and (e % fs.skip == 0 or e == n) and prev <= s < e <= n, (u, spans, n)
            prev = e
    assert os.path.exists(out / "model_best.pth")
