"""What the wide sequence-level kernels cost (the hypothesis label lists and the gradient pass over K+1 lattices of csrc/ctc.hip;
header section A13-WIDE; NOTES.md 0.32).  Shape: T = 1000, B = 32, L = 60, max_hyp_len = 300, K = N in {4, 16}, N(0,1) * 2 logits,
random targets, random hypotheses of 40 .. 300 tokens (mean 170) given directly -- the cost of the two kernels does not depend on
where a list comes from.

  kernels   each launch alone, at V = 64 (the new entries with one label per lane, wide=True) and at V in {128, 256, 1024}:
              hyp_lattice_K{4,16}   pgasr_ctc_hyp_lattice_wide: the label-list kernel and the K*B alpha / beta sweeps.
              grad_nbest_K{4,16}    pgasr_ctc_grad_from_lattices_seq_wide without a path tensor (MWER).
              grad_seq_K{4,16}      .. with sampled paths and no tail; grad_seq_K4_kl with both tails (one more row read).
            Beside a gradient pass stand the bytes it must move -- the row read, the row written (and the reference row), and the
            alpha / beta words of the K + 1 lattices it walks -- as a share of the 8 TB/s HBM peak.  Every call of a window takes
            the next of n row buffers, n chosen so that the buffers together exceed twice the 256 MiB Infinity Cache.
            With --parent-lib the V = 64 inputs are also timed with the other build's NARROW entries (pgasr_ctc_hyp_lattice,
            pgasr_ctc_grad_from_lattices_nbest, _seq) in a process of its own: the yardstick of the NV = 1 instantiations.
  step      the whole train step (f32, train mode, F = 80) at --step-vocab: MWERTrainer(wide_sequence=True, beam_size=16, nbest=4,
            max_hyp_len=300) beside PolicyGradientTrainer(wide_alphabet=True)'s default step, each in a process of its own.
  parent    the default wide step at --step-vocab with this tree's library and, with --parent-lib, the other build, in alternating
            child processes: the new entries must not move a step that does not use them.

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

T, B, L, F, LH = 1000, 32, 60, 80, 300
ALL_V = (64, 128, 256, 1024)
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
        raise SystemExit("wide_seq_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    wide = not args.older_lib               # the other build is asked for its narrow entries (V = 64 only)
    res = {"device": torch.cuda.get_device_name(0), "lib": _lib.LIB_PATH, "shape": {"T": T, "B": B, "L": L, "Lh": LH}, "V": {}}
    for V in ((64,) if args.older_lib else ALL_V):
        row_bytes = T * B * V * 4
        n = max(2, -(-2 * CACHE // row_bytes) + 1)
        base = (torch.randn(T, B, V, generator=g) * 2).to(dev)
        lps = [hipops.log_softmax_rows(base.clone()) for _ in range(n)]      # n copies: one set of lattices fits every one of them
        ref = hipops.log_softmax_rows((torch.randn(T, B, V, generator=g) * 2).to(dev))
        refs = [ref.clone() for _ in range(n)]
        targets = torch.randint(1, V, (B, L), generator=g, dtype=torch.int32).to(dev)
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        tl = torch.full((B,), L, dtype=torch.int32, device=dev)
        us = torch.full((B,), 1.0 / (B * L), device=dev)
        hyp_len = torch.randint(40, LH + 1, (16, B), generator=g, dtype=torch.int32)
        hyp = torch.randint(1, V, (16, B, T), generator=g, dtype=torch.int32)
        hyp[torch.arange(T)[None, None, :] >= hyp_len[:, :, None]] = 0
        hyp, hyp_len = hyp.to(dev), hyp_len.to(dev)
        coefs = (torch.linspace(-1, 1, 16 * B, device=dev) / B).view(16, B).contiguous()
        paths = torch.randint(0, V, (16, T, B), generator=g, dtype=torch.int32).to(dev)
        _, handle = hipops.ctc_lattice(lps[0], targets, il, tl, wide=wide)
        _, es = hipops.frame_entropy(lps[0], il, 0.1, 1.0 / B)
        _, ks = hipops.frame_kl(lps[0], refs[0], il, 0.1, 1.0 / B)
        entry = res["V"][str(V)] = {"row_tensor_bytes": row_bytes, "buffers": n}
        for K in (4, 16):
            hk, lk, ck, pk = hyp[:K].contiguous(), hyp_len[:K].contiguous(), coefs[:K].contiguous(), paths[:K].contiguous()
            # what a pass reads of the lattices: alpha and beta of the 2 len + 1 states of every lattice, at every frame
            walk = 2 * 4 * T * (B * (2 * L + 1) + int((2 * lk.long() + 1).sum()))
            configs = {f"hyp_lattice_K{K}": (lambda i, hk=hk, lk=lk: hipops.ctc_hyp_lattice(lps[i % n], hk, lk, il, LH, wide=wide), 0)}
            hh = hipops.ctc_hyp_lattice(lps[0], hk, lk, il, LH, wide=wide)[1]
            configs[f"grad_nbest_K{K}"] = (lambda i, hh=hh, lk=lk, ck=ck: hipops.ctc_grad_from_lattices_nbest(
                lps[i % n], il, tl, handle, hh, us, ck, lk, wide=wide), 2 * row_bytes + walk)
            configs[f"grad_seq_K{K}"] = (lambda i, hh=hh, lk=lk, ck=ck, pk=pk: hipops.ctc_grad_from_lattices_seq(
                lps[i % n], il, tl, handle, hh, us, ck, pk, lk, wide=wide), 2 * row_bytes + walk)
            if K == 4 and not args.older_lib:
                configs["grad_seq_K4_kl"] = (lambda i, hh=hh, lk=lk, ck=ck, pk=pk: hipops.ctc_grad_from_lattices_seq(
                    lps[i % n], il, tl, handle, hh, us, ck, pk, lk, ent_scale=es, ref_log_probs=refs[i % n], kl_scale=ks, wide=wide),
                    3 * row_bytes + walk)
            for name, (fn, nbytes) in configs.items():
                # the gradient windows read the lattices of the LAST ctc_hyp_lattice call of this K: time the lattice first
                ms = _windows(fn, args.calls if nbytes else max(4, args.calls // 4), args.repeats, args.warm)
                entry[name] = {"ms_per_call": _summary(ms)}
                share = ""
                if nbytes:
                    entry[name].update(bytes=nbytes, lattice_bytes=walk,
                                       share_of_hbm_peak=round(nbytes / (statistics.median(ms) * 1e-3) / HBM_PEAK, 3))
                    share = f"  {entry[name]['share_of_hbm_peak'] * 100:.0f} % of HBM peak ({nbytes / 1e6:.0f} MB, {walk / 1e6:.0f} of them lattice words)"
                print(f"V={V:5d} {name:18s}: median {statistics.median(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}){share}", flush=True)
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
        raise SystemExit("wide_seq_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    V = args.vocab
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(0)
    m = Seq2Seq(V, n_feats=F); m.apply(weights); m = m.to(dev).train()
    if args.mwer:
        from policy_gradient_asr_amd.mwer import MWERTrainer
        tr = MWERTrainer(m, lam=1.0, seed=3, precision="f32", beam_size=16, nbest=4, max_hyp_len=LH, wide_sequence=True)
    else:
        tr = PolicyGradientTrainer(m, lam=1.0, seed=3, precision="f32", **({"wide_alphabet": True} if V > 64 else {}))
    x = torch.randn(B, F, T, generator=g).to(dev)
    targets = torch.randint(1, V, (B, L), generator=g).to(dev)
    fmask = torch.ones(B, T, device=dev)
    tmask = torch.ones(B, L, dtype=torch.int64, device=dev)
    ms = _windows(lambda i: tr.step(x, targets, fmask, tmask), args.calls, args.repeats, args.warm)
    hipops.lstm_assert_no_timeouts()
    what = "mwer" if args.mwer else "default"
    print(f"step V={V} {what} lib={os.path.basename(_lib.LIB_PATH)}: median {statistics.median(ms):.4f} ms (min {min(ms):.4f}, "
          f"max {max(ms):.4f})", flush=True)
    print(json.dumps({"step": {"V": V, "objective": what, "lib": _lib.LIB_PATH, "ms_per_step": _summary(ms)}}))


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
        raise SystemExit(f"wide_seq_cost.py: a measuring child ran past {limit} s and was killed; nothing else was started")
    sys.stdout.write(p.stdout)
    sys.stdout.flush()
    if p.returncode != 0:
        raise SystemExit(f"wide_seq_cost.py: a measuring child ended with status {p.returncode}; nothing else was started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40, help="calls per timed window of a gradient pass (a quarter of it for the lattices)")
    ap.add_argument("--step-calls", type=int, default=20, help="steps per timed window")
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds each measuring child may take")
    ap.add_argument("--parent-lib", default=None, help="another build of libpgasr_hip.so (the parent commit's) to compare with")
    ap.add_argument("--step-vocab", type=int, default=256, help="alphabet size of the wide steps")
    ap.add_argument("--alternations", type=int, default=2, help="this / parent process pairs of the compared step")
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: kernels, step, parent")
    ap.add_argument("--worker", choices=("kernels", "step"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--vocab", type=int, default=256, help=argparse.SUPPRESS)
    ap.add_argument("--mwer", action="store_true", help=argparse.SUPPRESS)
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
    step = ["--worker", "step", "--calls", str(args.step_calls), "--vocab", str(args.step_vocab)] + common
    out = {}
    if "kernels" not in skip:
        out["kernels"] = _child(kernels, args.limit)["kernels"]
        if parent:
            out["kernels_parent"] = _child(kernels, args.limit, parent)["kernels"]
    if "step" not in skip:
        out["step_mwer"] = _child(step + ["--mwer"], args.limit)["step"]["ms_per_step"]
    if "parent" not in skip:
        runs = out[f"step_V{args.step_vocab}"] = {"this": []}
        libs = [("this", None)] + ([("parent", parent)] if parent else [])
        for name, _ in libs:
            runs.setdefault(name, [])
        for _ in range(args.alternations):      # alternating processes: this, parent, this, parent, ..
            for name, lib in libs:
                runs[name].append(_child(step, args.limit, lib)["step"]["ms_per_step"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
