"""What the edit-operation alignment costs beside the distance alone (csrc/editops.hip against csrc/editdist.hip; NOTES.md 0.24).
Shapes: N = 32 and N = 1024 pairs of ~100 symbols (strides 112 / 128), and N = 32 pairs of ~930 symbols (strides 960 / 1000),
V = 29; the hypothesis is an edited copy of the reference (about 12 % deletions, 15 % substitutions, 10 % insertions), so the walk
back has all four operations.  Per shape, four times:

  (distance)  pgasr_edit_distance -- editdist.hip is not touched by the alignment work, so this is the parent commit's kernel;
  (counts)    pgasr_edit_ops with counts only: the forward pass with its 2-bit stores, and the walk back;
  (ops)       the same with the operation string and n_ops;
  (confusion) the same with the operation string and the 30 x 30 confusion matrix.

The measurement runs in ONE child process under a time limit (--limit seconds; the parent never touches the GPU and starts nothing
after a child that failed or was killed).  In it every configuration is warmed up, then every repeat (--repeats 5) times a window of
back-to-back calls (--calls 200) between two device events, the order reversed every other repeat; the median of the windows is
reported, with the workspace bytes and that counts agree with the distance.  One JSON line at the end.  Not imported by bench.py or
the package."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

V = 29
SHAPES = (("N32_L100", 32, 100, 112, 128), ("N1024_L100", 1024, 100, 112, 128), ("N32_L930", 32, 930, 960, 1000))


def make_pairs(rng, N, L, R, Hy):
    import numpy as np
    ref = rng.integers(1, V, (N, R)).astype(np.int32); hyp = rng.integers(1, V, (N, Hy)).astype(np.int32)
    rl = np.zeros(N, dtype=np.int32); hl = np.zeros(N, dtype=np.int32)
    for k in range(N):
        n = int(rng.integers(L - L // 10, min(L + L // 10, R) + 1))
        out = []
        for s in ref[k, :n].tolist():
            u = rng.random()
            if u < 0.12:
                continue
            out.append(int(rng.integers(1, V)) if u < 0.27 else s)
            if u > 0.9:
                out.append(int(rng.integers(1, V)))
        out = out[:Hy]
        hyp[k, :len(out)] = out
        rl[k], hl[k] = n, len(out)
    return ref, rl, hyp, hl


def worker(args):
    import numpy as np
    import torch
    from policy_gradient_asr_amd import hipops
    if not torch.cuda.is_available():
        raise SystemExit("editops_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20240611)
    result = {"device": torch.cuda.get_device_name(0), "V": V, "repeats": args.repeats, "calls_per_window": args.calls, "shapes": {}}
    for name, N, L, R, Hy in SHAPES:
        ref, rl, hyp, hl = (torch.from_numpy(a).to(dev) for a in make_pairs(rng, N, L, R, Hy))
        cm = torch.zeros(V + 1, V + 1, dtype=torch.int64, device=dev)
        configs = {
            "distance": lambda: hipops.edit_distance(ref, rl, hyp, hl),
            "counts": lambda: hipops.edit_ops(ref, rl, hyp, hl, want_ops=False),
            "ops": lambda: hipops.edit_ops(ref, rl, hyp, hl),
            "confusion": lambda: hipops.edit_ops(ref, rl, hyp, hl, confusion=cm, vocab=V),
        }
        names = list(configs)
        calls = max(args.calls // (8 if L > 500 else 1), 5)

        def window(name, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                configs[name]()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / calls          # ms per call

        for n_ in names:
            window(n_, min(args.warm, calls))
        times = {n_: [] for n_ in names}
        for r in range(args.repeats):
            for n_ in (names if r % 2 == 0 else names[::-1]):
                times[n_].append(window(n_, calls))
        eo = configs["ops"]()
        entry = result["shapes"][name] = {
            "pairs": N, "strides": [R, Hy], "mean_ref_len": round(float(rl.float().mean().item()), 1),
            "mean_hyp_len": round(float(hl.float().mean().item()), 1), "mean_ops": round(float(eo.n_ops.float().mean().item()), 1),
            "workspace_bytes": hipops.edit_ops_workspace_bytes(R, Hy, N), "calls_per_window": calls,
            "counts_agree_with_distance": bool(torch.equal(eo.counts[:, 1:].sum(1).to(torch.int32), configs["distance"]())),
            "ms_per_call": {}}
        for n_ in names:
            v = times[n_]
            entry["ms_per_call"][n_] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            print(f"{name:11s} {n_:9s}: median {statistics.median(v):.4f} ms  (min {min(v):.4f}, max {max(v):.4f})", flush=True)
        base = entry["ms_per_call"]["distance"]["median"]
        entry["over_distance"] = {n_: round(entry["ms_per_call"][n_]["median"] / base, 2) for n_ in names[1:]}
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window (an eighth of it at ~930 symbols)")
    ap.add_argument("--warm", type=int, default=5, help="warm-up calls per configuration")
    ap.add_argument("--limit", type=int, default=240, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(args.repeats), "--calls", str(args.calls),
           "--warm", str(args.warm)]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"editops_cost.py: the measuring child ran past {args.limit} s and was killed; nothing else was started")
    sys.exit(rc)


if __name__ == "__main__":
    main()
