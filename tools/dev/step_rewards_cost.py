"""What per-step rewards with K samples cost (csrc/step_rewards.hip and the per-frame form of the multi-sample gradient pass of
csrc/ctc.hip; header section A12-STEP; NOTES.md 0.37).  Shape: T = 1000, B = 32, L = 60, N(0,1) * 2 logits, random targets.

  kernels   each launch alone:
              coefs_K{1,4,16}_{hyp,loo}  pgasr_pg_step_coefs_multi on the paths of the device's sampler at V = 29, their collapsed forms
                                   and per-prefix distances; beside it coefs_single (pgasr_pg_step_coefs, K = 1: the parent has it too)
                                   and lattice (the CTC lattice call the coefficient launch runs beside, on the other stream).  The
                                   coefficient kernel's inputs (2 MB of paths, 2 MB of distances at K = 16) are NOT rotated: in the step
                                   the kernels just before it wrote them.
              grad_utt_V, grad_frame_V   the multi-sample gradient pass at K = 4 without tails with per-utterance (K,B) and per-frame
                                   (K,T,B) coefficients on the same inputs, V in {29, 128, 256, 1024}.  With --parent-lib the
                                   per-utterance pass is timed with the other build too, in a process of its own.  Every call of a
                                   window takes the next of n row buffers, n chosen so that the buffers together exceed twice the
                                   256 MiB Infinity Cache.
  step      the whole train step (PolicyGradientTrainer, f32, train mode, F = 80) with num_samples = 4 and the leave-one-out
            baseline, with and without reward_mode="per_step", at V = 29 and V = 256, each in a process of its own.
  parent    the default step at V = 29 with this tree's library and, with --parent-lib, the other build, in alternating child
            processes: the new entries must not move the step that does not use them.

Every measurement runs in a child process under a time limit (--limit seconds each; the parent process never touches the GPU and
starts nothing after a child that failed or was killed).  A child warms every configuration up, then times --repeats (5) windows
of back-to-back calls between two device events and reports the median, minimum and maximum.  One JSON line at the end.  Not
imported by bench.py or the package."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

T, B, L, F = 1000, 32, 60, 80
GRAD_V = (29, 128, 256, 1024)
CACHE = 256 << 20            # Infinity Cache


def _summary(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def _windows(fn, calls, repeats, warm):
    import torch
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(calls):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


def _drop_missing_entries():
    """An older build lacks the entry points added since: bind what it has."""
    import ctypes
    from policy_gradient_asr_amd import _lib
    have = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
        del _lib.SIGNATURES[name]


def kernels_worker(args):
    import torch
    from policy_gradient_asr_amd import _lib, hipops
    if args.older_lib:
        _drop_missing_entries()
    if not torch.cuda.is_available():
        raise SystemExit("step_rewards_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    res = {"device": torch.cuda.get_device_name(0), "lib": _lib.LIB_PATH, "shape": {"T": T, "B": B, "L": L}}
    il = torch.full((B,), T, dtype=torch.int32, device=dev)
    tl = torch.full((B,), L, dtype=torch.int32, device=dev)
    us = torch.full((B,), 1.0 / (B * L), device=dev)

    def timed(name, fn):
        ms = _windows(fn, args.calls, args.repeats, args.warm)
        res[name] = _summary(ms)
        print(f"{name:22s}: median {statistics.median(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f})", flush=True)

    # (i) the coefficient launch, at V = 29
    V = 29
    lp = hipops.log_softmax_rows((torch.randn(T, B, V, generator=g) * 2).to(dev))
    targets = torch.randint(1, V, (B, L), generator=g, dtype=torch.int32).to(dev)
    rows = torch.empty(17, T, B, dtype=torch.int32, device=dev)
    hipops.frame_sample_multi(lp, 16, seed=3, out=(rows[0], rows[1:]))
    tokens, tok_len = hipops.ctc_collapse(rows, il)
    _, prefix = hipops.edit_distance(targets.repeat(17, 1), tl.repeat(17), tokens.view(17 * B, T), tok_len.view(17 * B), want_prefix=True)
    timed("lattice", lambda i: hipops.ctc_lattice(lp, targets, il, tl))
    timed("coefs_single", lambda i: hipops.pg_step_coefs(rows[:2], il, prefix[:2 * B], tok_len[:2].reshape(-1), tl, 1.0, 1.0 / B))
    if not args.older_lib:
        for K in (1, 4, 16):
            timed(f"coefs_K{K}_hyp", lambda i, K=K: hipops.pg_step_coefs_multi(rows[:K + 1], il, prefix[:(K + 1) * B],
                                                                                tok_len[:K + 1].reshape(-1), tl, K, 1.0, 1.0 / B))
            if K > 1:
                timed(f"coefs_K{K}_loo", lambda i, K=K: hipops.pg_step_coefs_multi(rows[1:K + 1], il, prefix[B:(K + 1) * B],
                                                                                    tok_len[1:K + 1].reshape(-1), tl, K, 1.0, 1.0 / B,
                                                                                    baseline="leave_one_out"))
    del lp

    # (ii) the gradient pass at K = 4 with per-utterance and per-frame coefficients
    K = 4
    for V in GRAD_V:
        row_bytes = T * B * V * 4
        n = max(2, -(-2 * CACHE // row_bytes) + 1)
        base = (torch.randn(T, B, V, generator=g) * 2).to(dev)
        lps = [hipops.log_softmax_rows(base.clone()) for _ in range(n)]      # n copies: one lattice fits every one of them
        targets = torch.randint(1, V, (B, L), generator=g, dtype=torch.int32).to(dev)
        _, paths = hipops.frame_sample_multi(lps[0], K, seed=3)
        _, handle = hipops.ctc_lattice(lps[0], targets, il, tl)
        utt = (torch.linspace(-1, 1, K * B, device=dev) / B).view(K, B).contiguous()
        timed(f"grad_utt_V{V}", lambda i: hipops.ctc_grad_from_lattice_multi(lps[i % n], il, tl, handle, us, utt, paths))
        if not args.older_lib:
            frames = (torch.linspace(-1, 1, K * T * B, device=dev) / B).view(K, T, B).contiguous()
            timed(f"grad_frame_V{V}", lambda i: hipops.ctc_grad_from_lattice_multi(lps[i % n], il, tl, handle, us, frames, paths))
        del lps, base
        torch.cuda.empty_cache()
    print(json.dumps({"kernels": res}))


def step_worker(args):
    import torch
    from policy_gradient_asr_amd import _lib, hipops
    if args.older_lib:
        _drop_missing_entries()
    from policy_gradient_asr_amd.model import Seq2Seq, weights
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    if not torch.cuda.is_available():
        raise SystemExit("step_rewards_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    V, K = args.vocab, args.samples
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(0)
    m = Seq2Seq(V, n_feats=F); m.apply(weights); m = m.to(dev).train()
    kw = {"wide_alphabet": True} if V > 64 else {}
    if K > 1:
        kw.update(num_samples=K, reward_baseline="leave_one_out", **({"wide_objectives": True} if V > 64 else {}))
    if args.per_step:
        kw.update(reward_mode="per_step", step_objectives=True)
    tr = PolicyGradientTrainer(m, lam=1.0, seed=3, precision="f32", **kw)
    x = torch.randn(B, F, T, generator=g).to(dev)
    targets = torch.randint(1, V, (B, L), generator=g).to(dev)
    fmask = torch.ones(B, T, device=dev)
    tmask = torch.ones(B, L, dtype=torch.int64, device=dev)
    ms = _windows(lambda i: tr.step(x, targets, fmask, tmask), args.calls, args.repeats, args.warm)
    hipops.lstm_assert_no_timeouts()
    print(f"step V={V} K={K} per_step={bool(args.per_step)} lib={os.path.basename(_lib.LIB_PATH)}: median {statistics.median(ms):.4f} ms "
          f"(min {min(ms):.4f}, max {max(ms):.4f})", flush=True)
    print(json.dumps({"step": {"V": V, "K": K, "per_step": bool(args.per_step), "lib": _lib.LIB_PATH, "ms_per_step": _summary(ms)}}))


def _child(argv, limit, lib=None):
    env = dict(os.environ)
    env.pop("PGASR_HIP_LIB", None)
    if lib:
        env["PGASR_HIP_LIB"] = lib
        argv = argv + ["--older-lib"]
    cmd = [sys.executable, os.path.abspath(__file__)] + argv
    try:
        p = subprocess.run(cmd, timeout=limit, env=env, stdout=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"step_rewards_cost.py: a measuring child ran past {limit} s and was killed; nothing else was started")
    sys.stdout.write(p.stdout)
    sys.stdout.flush()
    if p.returncode != 0:
        raise SystemExit(f"step_rewards_cost.py: a measuring child ended with status {p.returncode}; nothing else was started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40, help="calls per timed window of a kernel")
    ap.add_argument("--step-calls", type=int, default=20, help="steps per timed window")
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds each measuring child may take")
    ap.add_argument("--parent-lib", default=None, help="another build of libpgasr_hip.so (the parent commit's) to compare with")
    ap.add_argument("--step-vocabs", default="29,256", help="alphabet sizes of the K = 4 leave-one-out steps")
    ap.add_argument("--alternations", type=int, default=2, help="this / parent process pairs of the default step")
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: kernels, step, parent")
    ap.add_argument("--worker", choices=("kernels", "step"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--vocab", type=int, default=29, help=argparse.SUPPRESS)
    ap.add_argument("--samples", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--per-step", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--older-lib", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker == "kernels":
        return kernels_worker(args)
    if args.worker == "step":
        return step_worker(args)
    skip = set(filter(None, args.skip.split(",")))
    parent = os.path.abspath(args.parent_lib) if args.parent_lib else None
    common = ["--repeats", str(args.repeats), "--warm", str(args.warm)]
    kernels = ["--worker", "kernels", "--calls", str(args.calls)] + common
    step = ["--worker", "step", "--calls", str(args.step_calls)] + common
    out = {}
    if "kernels" not in skip:
        out["kernels"] = _child(kernels, args.limit)["kernels"]
        if parent:
            out["kernels_parent"] = _child(kernels, args.limit, parent)["kernels"]
    if "step" not in skip:
        out["step"] = {}
        for V in (int(v) for v in args.step_vocabs.split(",")):
            for per_step in (False, True):
                r = _child(step + ["--vocab", str(V), "--samples", "4"] + (["--per-step"] if per_step else []), args.limit)
                out["step"][f"V{V}_K4_loo_{'per_step' if per_step else 'utterance'}"] = r["step"]["ms_per_step"]
    if "parent" not in skip:
        runs = out["step_V29_default"] = {"this": []}
        libs = [("this", None)] + ([("parent", parent)] if parent else [])
        for name, _ in libs:
            runs.setdefault(name, [])
        for _ in range(args.alternations):      # alternating processes: this, parent, this, parent, ..
            for name, lib in libs:
                runs[name].append(_child(step + ["--vocab", "29"], args.limit, lib)["step"]["ms_per_step"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
