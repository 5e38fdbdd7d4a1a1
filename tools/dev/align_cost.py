"""What a forced alignment (pgasr_ctc_forced_align, NOTES.md 0.11) costs at the headline shape B = 32, T = 1000, V = 29:

  targets : L = 100 random transcripts (the 1-state-per-thread forward kernel);
  greedy  : the greedy hypotheses of the same random rows, L ~ 930 (the 8-states-per-thread kernel, the longest backtrace);
  lattice : the yardstick, hipops.ctc_lattice (alpha and beta sweeps in parallel) on the `targets` inputs.

Each case runs in a child process of its own under a time limit (--limit seconds); the first failure ends the run.  A timing is
the time between two HIP events around --calls back-to-back calls, divided by the calls; the median, minimum and maximum of
--repeats such windows are printed, `align` with the spans and `align_nospans` without the third launch.  There is no pass/fail
bar.  The three kernels apart: run one case under `rocprofv3 --kernel-trace --stats -- python tools/dev/align_cost.py --child greedy`.
Not imported by bench.py or the package."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CASES = ("targets", "greedy", "lattice")


def child(case, repeats, calls):
    sys.path.insert(0, ROOT)
    import torch
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.CTCdecoder import greedy_decode
    if not torch.cuda.is_available():
        raise SystemExit("align_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    T, B, V, L = 1000, 32, 29, 100
    g = torch.Generator().manual_seed(1234)
    lp = torch.log_softmax(torch.randn(T, B, V, generator=g), 2).to(dev).contiguous()
    il = torch.full((B,), T, dtype=torch.int32, device=dev)
    if case == "greedy":
        hyp, tl = greedy_decode(lp)
        tokens, tl = hyp[:, :hipops.ALIGN_MAX_TOKENS].contiguous(), tl.contiguous()
    else:
        tokens = torch.randint(1, V, (B, L), generator=g).to(torch.int32).to(dev)
        tl = torch.full((B,), L, dtype=torch.int32, device=dev)
    runs = {"lattice": lambda: hipops.ctc_lattice(lp, tokens, il, tl)} if case == "lattice" else {
        "align": lambda: hipops.ctc_forced_align(lp, tokens, il, tl),
        "align_nospans": lambda: hipops.ctc_forced_align(lp, tokens, il, tl, want_spans=False)}
    out = {"case": case, "L_max": int(tl.max()), "L_min": int(tl.min()), "device": torch.cuda.get_device_name(0)}
    for name, fn in runs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / calls)
        out[name] = {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=CASES, default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed window")
    ap.add_argument("--limit", type=int, default=120, help="seconds a case may take")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.repeats, args.calls)
    for case in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--repeats", str(args.repeats),
                            "--calls", str(args.calls)], timeout=args.limit)
        if r.returncode != 0:
            raise SystemExit(f"case {case} ended with status {r.returncode}: nothing further is run")


if __name__ == "__main__":
    main()
