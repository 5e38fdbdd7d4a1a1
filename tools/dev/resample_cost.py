"""What sample-rate conversion / speed perturbation (pgasr_resample, NOTES.md) costs at the headline batch, B = 32 utterances of 10 s:

  48k   : 480000 samples at 48 kHz -> 16 kHz, ratio 1/3 (39 taps): 61 MB read, 20 MB written;
  speed : 160000 samples at 16 kHz at speed 0.9, ratio 10/9 (15 taps, 10 phases): 20 MB read, 23 MB written.

Per case: `resample`, the one launch, and `logmel80_rest`, the rest of LogMel(80) on the batch it produced (padding copy, framing, DFT,
mel, dB, stacking).  The launch rotates over --sets input / output buffer pairs (default 6: ~0.5 GB, more than the 256 MiB Infinity
Cache), so its bytes come from HBM, not from the previous call's cache lines; `hbm_fraction` is (bytes read + written) / time over the
8.0 TB/s peak -- the kernel is memory-bound, the least time is bytes over bandwidth.
Each case runs in a child process of its own under a time limit (--limit seconds); the first failure ends the run.  A timing is the
time between two HIP events around --calls back-to-back calls, divided by the calls; the median, minimum and maximum of --repeats
such windows are printed.  There is no pass/fail bar.  Not imported by bench.py or the package."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CASES = {"48k": (1, 3, 480000), "speed": (10, 9, 160000)}
HBM_PEAK = 8.0e12


def timed(fn, repeats, calls):
    import torch
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
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def child(case, repeats, calls, sets):
    sys.path.insert(0, ROOT)
    import torch
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.features import LogMel, resample_length
    if not torch.cuda.is_available():
        raise SystemExit("resample_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    L, M, n = CASES[case]
    B = 32
    g = torch.Generator(device=dev).manual_seed(1234)
    n_in = torch.full((B,), n, dtype=torch.int32, device=dev)
    n_out = resample_length(n, L, M)
    waves = [0.1 * torch.randn(B, n, generator=g, device=dev) for _ in range(sets)]
    outs = [torch.empty(B, (n_out + 3) // 4 * 4, dtype=torch.float32, device=dev) for _ in range(sets)]
    lens = torch.empty(B, dtype=torch.int32, device=dev)
    turn = [0]

    def launch():
        k = turn[0] = (turn[0] + 1) % sets
        hipops.resample(waves[k], n_in, [(L, M)], out=outs[k], n_out=lens)
    out = {"case": case, "ratio": f"{L}/{M}", "B": B, "n_in": n, "n_out": n_out, "device": torch.cuda.get_device_name(0)}
    out["resample"] = timed(launch, repeats, calls)
    moved = 4 * B * (n + outs[0].shape[1])
    out["bytes_read"], out["bytes_written"] = 4 * B * n, 4 * B * outs[0].shape[1]
    out["resample"]["hbm_fraction"] = round(moved / (out["resample"]["median_us"] * 1e-6) / HBM_PEAK, 3)
    fe = LogMel(80, dev)
    rows = [outs[0][b, :n_out] for b in range(B)]
    out["logmel80_rest"] = timed(lambda: fe(rows), repeats, max(calls // 4, 1))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=tuple(CASES), default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=40, help="back-to-back calls per timed window")
    ap.add_argument("--sets", type=int, default=6, help="buffer pairs the launch rotates over")
    ap.add_argument("--limit", type=int, default=120, help="seconds a case may take")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.repeats, args.calls, args.sets)
    for case in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--repeats", str(args.repeats),
                            "--calls", str(args.calls), "--sets", str(args.sets)], timeout=args.limit)
        if r.returncode != 0:
            raise SystemExit(f"case {case} ended with status {r.returncode}: nothing further is run")


if __name__ == "__main__":
    main()
