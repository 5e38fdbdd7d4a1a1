"""What the exact wide prefix beam search costs (csrc/beam_wide.hip; NOTES.md 0.19).  Shape: T = 1000, B = 32, beam 16, fp32
log-probs, blank 0; rows are PEAKED (logits 5 N(0,1)) or FLAT (logits 0.3 N(0,1)), the two ends of what a model emits.

  (w)  ctc_beam_search_wide at V = 128 / 256 / 1024 and N = 1 / 16, with the share of frames that took the counting selection;
  (c)  the same with counting=True at V = 1024, N = 16: what the counting selection costs when every frame takes it;
  (n)  at V = 64, the wide entry against ctc_beam_search_nbest without ``fast`` (the workgroup-per-utterance kernel of csrc/beam.hip)
       on the same inputs and the same library, N = 16, with a bit-for-bit comparison of their outputs;
  (g)  the greedy decode (CTCdecoder.greedy_decode) at V = 1024, for scale.

The measurement runs in ONE child process under a time limit (--limit seconds; the parent never touches the GPU and starts nothing
after a child that failed or was killed).  In it every configuration is warmed up, then every repeat (--repeats 5) times --calls (3)
back-to-back calls of every configuration in turn between two device events, the order reversed every other repeat; medians of
the windows are reported.  No bar is set.  One JSON line at the end.  Not imported by bench.py or the package."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

T, B, BEAM = 1000, 32, 16
WIDTHS = (128, 256, 1024)
SIZES = (1, 16)
ROWS = {"peaked": 5.0, "flat": 0.3}


def worker(args):
    import numpy as np
    import torch
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.CTCdecoder import greedy_decode
    if not torch.cuda.is_available():
        raise SystemExit("beam_wide_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")

    def rows(V, kind):
        rng = np.random.default_rng(424245 + V)
        logits = rng.normal(size=(T, B, V)) * ROWS[kind]
        m = logits.max(axis=-1, keepdims=True)
        return torch.from_numpy((logits - (m + np.log(np.exp(logits - m).sum(axis=-1, keepdims=True)))).astype(np.float32)).to(dev)

    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    configs, share = {}, {}
    for kind in ROWS:
        for V in WIDTHS:
            lp = rows(V, kind)
            for n in SIZES:
                configs[f"w_V{V}_{kind}_n{n}"] = lambda lp=lp, n=n: hipops.ctc_beam_search_wide(lp, None, beam=BEAM, nbest=n)
            _, frames = hipops.ctc_beam_search_wide(lp, None, beam=BEAM, nbest=1, stats=True)
            share[f"V{V}_{kind}"] = round(float(frames.sum()) / (T * B), 5)
            if V == 1024:
                configs[f"c_V1024_{kind}_n16"] = lambda lp=lp: hipops.ctc_beam_search_wide(lp, None, beam=BEAM, nbest=16, counting=True)
                configs[f"g_V1024_{kind}"] = lambda lp=lp: greedy_decode(lp, lens)
        lp64 = rows(64, kind)
        configs[f"n_V64_{kind}_wide"] = lambda lp=lp64: hipops.ctc_beam_search_wide(lp, None, beam=BEAM, nbest=16)
        configs[f"n_V64_{kind}_narrow"] = lambda lp=lp64: hipops.ctc_beam_search_nbest(lp, None, beam=BEAM, nbest=16)
        a, b = configs[f"n_V64_{kind}_wide"](), configs[f"n_V64_{kind}_narrow"]()
        share[f"V64_{kind}_equal_bits"] = bool(torch.equal(a.tokens, b.tokens) and torch.equal(a.lengths, b.lengths)
                                               and torch.equal(a.count, b.count) and torch.equal(a.score.view(torch.int64), b.score.view(torch.int64)))
    names = list(configs)

    def window(name, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            configs[name]()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls          # ms per call

    for name in names:
        window(name, args.warm)
    times = {name: [] for name in names}
    for r in range(args.repeats):
        for name in (names if r % 2 == 0 else names[::-1]):
            times[name].append(window(name, args.calls))
    result = {"shape": {"T": T, "B": B, "beam": BEAM}, "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "calls_per_window": args.calls, "counting_share": share, "configs": {}}
    for name in names:
        v = times[name]
        e = result["configs"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        print(f"{name:24s}: median {e['median']:.3f} ms  (min {e['min']:.3f}, max {e['max']:.3f})", flush=True)
    for kind in ROWS:
        result[f"wide_over_narrow_V64_{kind}"] = round(result["configs"][f"n_V64_{kind}_wide"]["median"]
                                                       / result["configs"][f"n_V64_{kind}_narrow"]["median"], 3)
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed window")
    ap.add_argument("--warm", type=int, default=1, help="warm-up calls per configuration")
    ap.add_argument("--limit", type=int, default=400, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(args.repeats), "--calls", str(args.calls),
           "--warm", str(args.warm)]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"beam_wide_cost.py: the measuring child ran past {args.limit} s and was killed; nothing else was started")
    sys.exit(rc)


if __name__ == "__main__":
    main()
