"""What the wide-alphabet kernels cost (csrc/wide_vocab.hip and the wide pair of csrc/ctc.hip; NOTES.md 0.25).
Shape: T = 1000, B = 32, L = 60, V in {128, 256, 1024}, N(0,1) * 2 logits, random targets.

  kernels   each of the four launches alone -- log-softmax, arg-max + sample, the lattice call (label lists + the two sweeps) and the
            gradient pass -- beside the bytes it must move: T*B*V*4 read, and written where it writes a row (log-softmax, gradient),
            as a share of the 8 TB/s HBM peak.  The lattice is a latency chain of T frames, not a streaming kernel: its bytes are
            listed, its share says nothing.  Every call of a window takes the next of n row buffers, n chosen so that the buffers
            together exceed twice the 256 MiB Infinity Cache: no call finds its rows in a cache.
  step      the whole default train step (PolicyGradientTrainer(wide_alphabet=True), f32, train mode, F = 80) at the same V.
  parent    the default step at V = 29 with this tree's library and, with --parent-lib, with another build of the library (the
            parent commit's), in alternating child processes: the new entries must not move the step that does not use them.

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


def kernels_worker(args):
    import torch
    from policy_gradient_asr_amd import hipops
    if not torch.cuda.is_available():
        raise SystemExit("wide_vocab_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    res = {"device": torch.cuda.get_device_name(0), "shape": {"T": T, "B": B, "L": L}, "V": {}}
    for V in WIDE_V:
        row_bytes = T * B * V * 4
        n = max(2, -(-2 * CACHE // row_bytes) + 1)
        base = (torch.randn(T, B, V, generator=g) * 2).to(dev)
        logits = [base.clone() for _ in range(n)]          # n copies of one tensor: the lattice in the workspace fits every one of them
        lps = [hipops.log_softmax_rows(z) for z in logits]
        targets = torch.randint(1, V, (B, L), generator=g, dtype=torch.int32).to(dev)
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        tl = torch.full((B,), L, dtype=torch.int32, device=dev)
        us = torch.full((B,), 1.0 / (B * L), device=dev)
        coef = torch.linspace(-1, 1, B, device=dev) / B
        _, path = hipops.frame_argmax_sample(lps[0], seed=3, want_greedy=False)
        _, handle = hipops.ctc_lattice(lps[0], targets, il, tl)         # one lattice serves every gradient window (same shapes)
        configs = {
            "log_softmax": (lambda i: hipops.log_softmax_rows(logits[i % n]), 2 * row_bytes),
            "argmax_sample": (lambda i: hipops.frame_argmax_sample(lps[i % n], seed=3, offset=i), row_bytes),
            "lattice": (lambda i: hipops.ctc_lattice(lps[i % n], targets, il, tl), None),
            "grad": (lambda i: hipops.ctc_grad_from_lattice(lps[i % n], il, tl, handle, utt_scale=us, pg_coef=coef, pg_path=path),
                     2 * row_bytes),
        }
        entry = res["V"][str(V)] = {"row_tensor_bytes": row_bytes, "buffers": n}
        for name, (fn, nbytes) in configs.items():
            ms = _windows(fn, args.calls, args.repeats, args.warm)
            e = entry[name] = {"ms_per_call": _summary(ms)}
            if nbytes is not None:
                e["bytes"] = nbytes
                e["share_of_hbm_peak"] = round(nbytes / (statistics.median(ms) * 1e-3) / HBM_PEAK, 3)
            print(f"V={V:5d} {name:14s}: median {statistics.median(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f})"
                  + (f"  {e['share_of_hbm_peak'] * 100:.0f} % of HBM peak" if nbytes is not None else ""), flush=True)
        del logits, lps
        torch.cuda.empty_cache()
    print(json.dumps({"kernels": res}))


def step_worker(args):
    import ctypes
    import torch
    from policy_gradient_asr_amd import _lib, hipops
    if args.older_lib:
        # an older build lacks the entry points added since: bind what it has (the V = 29 step calls none of the others)
        have = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
            del _lib.SIGNATURES[name]
    from policy_gradient_asr_amd.model import Seq2Seq, weights
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    if not torch.cuda.is_available():
        raise SystemExit("wide_vocab_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    V = args.vocab
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(0)
    m = Seq2Seq(V, n_feats=F); m.apply(weights); m = m.to(dev).train()
    tr = PolicyGradientTrainer(m, lam=1.0, seed=3, precision="f32", **({"wide_alphabet": True} if V > 64 else {}))
    x = torch.randn(B, F, T, generator=g).to(dev)
    targets = torch.randint(1, V, (B, L), generator=g).to(dev)
    fmask = torch.ones(B, T, device=dev)
    tmask = torch.ones(B, L, dtype=torch.int64, device=dev)
    ms = _windows(lambda i: tr.step(x, targets, fmask, tmask), args.calls, args.repeats, args.warm)
    hipops.lstm_assert_no_timeouts()
    print(f"step V={V} lib={os.path.basename(_lib.LIB_PATH)}: median {statistics.median(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f})",
          flush=True)
    print(json.dumps({"step": {"V": V, "lib": _lib.LIB_PATH, "ms_per_step": _summary(ms)}}))


def _child(argv, limit, env=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + argv
    try:
        p = subprocess.run(cmd, timeout=limit, env=env, stdout=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"wide_vocab_cost.py: a measuring child ran past {limit} s and was killed; nothing else was started")
    sys.stdout.write(p.stdout)
    sys.stdout.flush()
    if p.returncode != 0:
        raise SystemExit(f"wide_vocab_cost.py: a measuring child ended with status {p.returncode}; nothing else was started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40, help="calls per timed window of a kernel")
    ap.add_argument("--step-calls", type=int, default=20, help="steps per timed window")
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds each measuring child may take")
    ap.add_argument("--parent-lib", default=None, help="another build of libpgasr_hip.so to time the V = 29 step with")
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: kernels, step, parent")
    ap.add_argument("--worker", choices=("kernels", "step"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--vocab", type=int, default=29, help=argparse.SUPPRESS)
    ap.add_argument("--older-lib", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker == "kernels":
        return kernels_worker(args)
    if args.worker == "step":
        return step_worker(args)
    skip = set(filter(None, args.skip.split(",")))
    common = ["--repeats", str(args.repeats), "--warm", str(args.warm)]
    out = {}
    if "kernels" not in skip:
        out.update(_child(["--worker", "kernels", "--calls", str(args.calls)] + common, args.limit))
    step = ["--worker", "step", "--calls", str(args.step_calls)] + common
    if "step" not in skip:
        out["step"] = {str(V): _child(step + ["--vocab", str(V)], args.limit)["step"]["ms_per_step"] for V in WIDE_V}
    if "parent" not in skip:
        runs = {"this": []}
        libs = [("this", None)]
        if args.parent_lib:
            libs.append(("parent", os.path.abspath(args.parent_lib)))
            runs["parent"] = []
        for _ in range(3):                      # alternating processes: this, parent, this, parent, ..
            for name, lib in libs:
                env = dict(os.environ)
                env.pop("PGASR_HIP_LIB", None)
                if lib:
                    env["PGASR_HIP_LIB"] = lib
                runs[name].append(_child(step + ["--vocab", "29"] + (["--older-lib"] if lib else []), args.limit, env)["step"]["ms_per_step"])
        out["step_V29"] = runs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
