"""What the wide policy-gradient kernels cost (csrc/wide_pg.hip and the multi-sample wide gradient pass of csrc/ctc.hip; header
section A12-WIDE; NOTES.md 0.31).  Shape: T = 1000, B = 32, L = 60, V in {128, 256, 1024}, N(0,1) * 2 logits, random targets.

  kernels   each launch alone beside the bytes it must move, as a share of the 8 TB/s HBM peak:
              grad_wide            pgasr_ctc_grad_from_lattice_wide with one sampled path (the default wide objective's pass): one
                                   row read, one written.  Timed with this tree's library and, with --parent-lib, with another build
                                   (the parent commit's) in a process of its own, on the same inputs.
              grad_multi_K1        the new pass with K = 1 and no tails on the same inputs: the same bytes.
              grad_multi_K{4,16}_{ent,kl}   the new pass with the entropy tail (one row read, one written) and with both tails (one
                                   more row read).
              sample_K{1,4,16}, argmax_sample   the K-draw sampler beside the single-sample one: one row read.
              entropy, kl          the statistics kernels: one row read, two with the reference.
            Every call of a window takes the next of n row buffers, n chosen so that the buffers together exceed twice the 256 MiB
            Infinity Cache: no call finds its rows in a cache.
  step      the whole train step (PolicyGradientTrainer(wide_alphabet=True), f32, train mode, F = 80) at --step-vocab: the default
            objective, and num_samples = 4 with the leave-one-out baseline (wide_objectives=True), each in a process of its own.
  parent    the default step at V = 29 and the default wide step at --step-vocab with this tree's library and, with --parent-lib, the
            other build, in alternating child processes: the new entries must not move the steps that do not use them.

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
WIDE_V = (128, 256, 1024)
HBM_PEAK = 8.0e12            # bytes / s
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
        raise SystemExit("wide_pg_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    res = {"device": torch.cuda.get_device_name(0), "lib": _lib.LIB_PATH, "shape": {"T": T, "B": B, "L": L}, "V": {}}
    for V in WIDE_V:
        row_bytes = T * B * V * 4
        n = max(2, -(-2 * CACHE // row_bytes) + 1)
        base = (torch.randn(T, B, V, generator=g) * 2).to(dev)
        lps = [hipops.log_softmax_rows(base.clone()) for _ in range(n)]      # n copies: one lattice fits every one of them
        ref = hipops.log_softmax_rows((torch.randn(T, B, V, generator=g) * 2).to(dev))
        refs = [ref.clone() for _ in range(n)]
        targets = torch.randint(1, V, (B, L), generator=g, dtype=torch.int32).to(dev)
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        tl = torch.full((B,), L, dtype=torch.int32, device=dev)
        us = torch.full((B,), 1.0 / (B * L), device=dev)
        coef = torch.linspace(-1, 1, B, device=dev) / B
        _, path = hipops.frame_argmax_sample(lps[0], seed=3, want_greedy=False)
        _, handle = hipops.ctc_lattice(lps[0], targets, il, tl)         # one lattice serves every gradient window (same shapes)
        configs = {"grad_wide": (lambda i: hipops.ctc_grad_from_lattice(lps[i % n], il, tl, handle, utt_scale=us, pg_coef=coef,
                                                                       pg_path=path), 2 * row_bytes)}
        if not args.older_lib:
            _, paths = hipops.frame_sample_multi(lps[0], 16, seed=3)
            coefs = (torch.linspace(-1, 1, 16 * B, device=dev) / B).view(16, B).contiguous()
            _, es = hipops.frame_entropy(lps[0], il, 0.1, 1.0 / B)
            _, ks = hipops.frame_kl(lps[0], refs[0], il, 0.1, 1.0 / B)

            def multi(K, ent, kl):
                pk, ck = paths[:K].contiguous(), coefs[:K].contiguous()
                return lambda i: hipops.ctc_grad_from_lattice_multi(lps[i % n], il, tl, handle, us, ck, pk, ent_scale=es if ent else None,
                                                                    ref_log_probs=refs[i % n] if kl else None, kl_scale=ks if kl else None)
            configs["grad_multi_K1"] = (multi(1, False, False), 2 * row_bytes)
            for K in (4, 16):
                configs[f"grad_multi_K{K}_ent"] = (multi(K, True, False), 2 * row_bytes)
                configs[f"grad_multi_K{K}_kl"] = (multi(K, True, True), 3 * row_bytes)
            configs["argmax_sample"] = (lambda i: hipops.frame_argmax_sample(lps[i % n], seed=3, offset=i), row_bytes)
            for K in (1, 4, 16):
                configs[f"sample_K{K}"] = (lambda i, K=K: hipops.frame_sample_multi(lps[i % n], K, seed=3, offset=i), row_bytes)
            configs["entropy"] = (lambda i: hipops.frame_entropy(lps[i % n], il, 0.1, 1.0 / B), row_bytes)
            configs["kl"] = (lambda i: hipops.frame_kl(lps[i % n], refs[i % n], il, 0.1, 1.0 / B), 2 * row_bytes)
        entry = res["V"][str(V)] = {"row_tensor_bytes": row_bytes, "buffers": n}
        for name, (fn, nbytes) in configs.items():
            ms = _windows(fn, args.calls, args.repeats, args.warm)
            entry[name] = {"ms_per_call": _summary(ms), "bytes": nbytes,
                           "share_of_hbm_peak": round(nbytes / (statistics.median(ms) * 1e-3) / HBM_PEAK, 3)}
            print(f"V={V:5d} {name:20s}: median {statistics.median(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f})  "
                  f"{entry[name]['share_of_hbm_peak'] * 100:.0f} % of HBM peak", flush=True)
        del lps, refs
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
        raise SystemExit("wide_pg_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    V, K = args.vocab, args.samples
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(0)
    m = Seq2Seq(V, n_feats=F); m.apply(weights); m = m.to(dev).train()
    kw = {"wide_alphabet": True} if V > 64 else {}
    if K > 1:
        kw.update(num_samples=K, reward_baseline="leave_one_out", **({"wide_objectives": True} if V > 64 else {}))
    tr = PolicyGradientTrainer(m, lam=1.0, seed=3, precision="f32", **kw)
    x = torch.randn(B, F, T, generator=g).to(dev)
    targets = torch.randint(1, V, (B, L), generator=g).to(dev)
    fmask = torch.ones(B, T, device=dev)
    tmask = torch.ones(B, L, dtype=torch.int64, device=dev)
    ms = _windows(lambda i: tr.step(x, targets, fmask, tmask), args.calls, args.repeats, args.warm)
    hipops.lstm_assert_no_timeouts()
    print(f"step V={V} K={K} lib={os.path.basename(_lib.LIB_PATH)}: median {statistics.median(ms):.4f} ms (min {min(ms):.4f}, "
          f"max {max(ms):.4f})", flush=True)
    print(json.dumps({"step": {"V": V, "K": K, "lib": _lib.LIB_PATH, "ms_per_step": _summary(ms)}}))


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
        raise SystemExit(f"wide_pg_cost.py: a measuring child ran past {limit} s and was killed; nothing else was started")
    sys.stdout.write(p.stdout)
    sys.stdout.flush()
    if p.returncode != 0:
        raise SystemExit(f"wide_pg_cost.py: a measuring child ended with status {p.returncode}; nothing else was started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40, help="calls per timed window of a kernel")
    ap.add_argument("--step-calls", type=int, default=20, help="steps per timed window")
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds each measuring child may take")
    ap.add_argument("--parent-lib", default=None, help="another build of libpgasr_hip.so (the parent commit's) to compare with")
    ap.add_argument("--step-vocab", type=int, default=300, help="alphabet size of the wide steps")
    ap.add_argument("--alternations", type=int, default=2, help="this / parent process pairs per compared step")
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: kernels, step, parent")
    ap.add_argument("--worker", choices=("kernels", "step"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--vocab", type=int, default=29, help=argparse.SUPPRESS)
    ap.add_argument("--samples", type=int, default=1, help=argparse.SUPPRESS)
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
        # the K = 1 wide step is timed by the parent part below (its "this" runs); alone only when that part is left out
        out["step"] = {f"V{args.step_vocab}_K{K}": _child(step + ["--vocab", str(args.step_vocab), "--samples", str(K)],
                                                        args.limit)["step"]["ms_per_step"]
                       for K in ((4,) if "parent" not in skip else (1, 4))}
    if "parent" not in skip:
        for V in (29, args.step_vocab):
            runs = out[f"step_V{V}"] = {"this": []}
            libs = [("this", None)] + ([("parent", parent)] if parent else [])
            for name, _ in libs:
                runs.setdefault(name, [])
            for _ in range(args.alternations):      # alternating processes: this, parent, this, parent, ..
                for name, lib in libs:
                    runs[name].append(_child(step + ["--vocab", str(V)], args.limit, lib)["step"]["ms_per_step"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
