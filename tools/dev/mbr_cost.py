"""What minimum-Bayes-risk decoding adds to an N-best search (csrc/mbr.hip; NOTES.md 0.20).  Headline shape: T = 1000 (--frames), B = 32, V = 29,
beam = N in {16, 64, 128} (--sizes), fp32 log-probs peaked enough that the lists are near-equal strings; the lists come from the
workgroup-per-utterance search (``ctc_beam_search_nbest``).  Per N, three times:

  (kernel)   pgasr_nbest_pair_dist (one lane per pair, bit-vector recurrence), the cap given -- the path hipops.nbest_pair_distance
             takes but for few pairs of long hypotheses;
  (composed) the same matrix on the composed path: the unordered pairs expanded in chunks through pgasr_edit_distance (one wave
             per pair) -- the baseline, what the parent commit could do;
  (select)   hipops.mbr_select on that matrix.

The measurement runs in ONE child process under a time limit (--limit seconds; the parent never touches the GPU and starts nothing
after a child that failed or was killed).  In it every configuration is warmed up, then every repeat (--repeats 5) times a window of
back-to-back calls (--calls 20; the composed path --composed-calls 2) between two device events, the order reversed every other
repeat; the median of the windows is reported, and that the two paths gave the same matrix.  One JSON line at the end.  Not imported
by bench.py or the package."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

B, V = 32, 29


def worker(args):
    import numpy as np
    import torch
    from policy_gradient_asr_amd import _lib, hipops
    if not torch.cuda.is_available():
        raise SystemExit("mbr_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(424246)
    T, SIZES = args.frames, tuple(int(x) for x in args.sizes.split(","))
    logits = rng.normal(size=(T, B, V)) * 4.0
    m = logits.max(axis=-1, keepdims=True)
    lp = torch.from_numpy((logits - (m + np.log(np.exp(logits - m).sum(axis=-1, keepdims=True)))).astype(np.float32)).to(dev)
    result = {"shape": {"T": T, "B": B, "V": V}, "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "calls_per_window": args.calls, "composed_calls_per_window": args.composed_calls, "sizes": {}}
    for n in SIZES:
        try:
            nb = hipops.ctc_beam_search_nbest(lp, None, beam=n, nbest=n)
        except _lib.PgasrError as e:                     # a refusal of the search at this size: reported, not measured
            result["sizes"]["N%d" % n] = {"refused": str(e)}
            continue
        longest = int(nb.lengths.max().item())
        dist = hipops._pair_distance_kernel(nb.tokens, nb.lengths, nb.count, V, longest)
        composed = hipops._pair_distance_composed(nb.tokens, nb.lengths, nb.count, V, longest, "char", None)
        configs = {
            "kernel": (args.calls, lambda: hipops._pair_distance_kernel(nb.tokens, nb.lengths, nb.count, V, longest)),
            "composed": (args.composed_calls, lambda: hipops._pair_distance_composed(nb.tokens, nb.lengths, nb.count, V, longest, "char", None)),
            "select": (args.calls, lambda: hipops.mbr_select(dist, nb.score, nb.count, scale=1.0)),
        }
        names = list(configs)

        def window(name, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                configs[name][1]()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / calls          # ms per call

        for name in names:
            window(name, min(args.warm, configs[name][0]))
        times = {name: [] for name in names}
        for r in range(args.repeats):
            for name in (names if r % 2 == 0 else names[::-1]):
                times[name].append(window(name, configs[name][0]))
        entry = result["sizes"]["N%d" % n] = {"pairs": B * n * (n - 1) // 2, "longest_hypothesis": longest,
                                              "mean_hypothesis": round(float(nb.lengths.float().mean().item()), 1),
                                              "paths_agree": bool(torch.equal(dist, composed)), "ms_per_call": {}}
        for name in names:
            v = times[name]
            entry["ms_per_call"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            print(f"N={n:3d} {name:9s}: median {statistics.median(v):.4f} ms  (min {min(v):.4f}, max {max(v):.4f})", flush=True)
        entry["composed_over_kernel"] = round(entry["ms_per_call"]["composed"]["median"] / entry["ms_per_call"]["kernel"]["median"], 2)
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000, help="T: frames per utterance (the hypotheses are about 0.93 T long)")
    ap.add_argument("--sizes", default="16,64,128", help="list sizes N (= beam), comma separated")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--composed-calls", type=int, default=2, help="calls per timed window of the composed path")
    ap.add_argument("--warm", type=int, default=3, help="warm-up calls per configuration")
    ap.add_argument("--limit", type=int, default=240, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(args.repeats), "--calls", str(args.calls),
           "--composed-calls", str(args.composed_calls), "--warm", str(args.warm), "--frames", str(args.frames), "--sizes", args.sizes]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"mbr_cost.py: the measuring child ran past {args.limit} s and was killed; nothing else was started")
    sys.exit(rc)


if __name__ == "__main__":
    main()
