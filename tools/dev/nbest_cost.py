"""What N-best emission costs the CTC beam search (csrc/beam.hip, NBEST = true; NOTES.md 0.13), and whether adding it left the 1-best
kernel alone.  Headline shape: T = 1000, B = 32, V = 29, beam 16, fp32 log-probs, no language model.

  (a) ctc_beam_search(generic=True) of a library built from the PARENT commit (--parent-lib; e.g. `git worktree add /tmp/parent HEAD~1 &&
      make -C /tmp/parent/policy_gradient_asr_amd/csrc`);
  (b) ctc_beam_search(generic=True) of this tree's library: the same kernel text, so (b) against (a) is the box;
  (n1, n4, n16) ctc_beam_search_nbest at N = 1, 4, 16 of this tree's library: the same search with the N-best tail.

The measurement runs in ONE child process under a time limit (--limit seconds; the parent never touches the GPU and starts nothing
after a child that failed or was killed).  In it every configuration is warmed up, then every repeat (--repeats 5) times --calls (20)
back-to-back calls of every configuration in turn between two device events, the order reversed every other repeat.  No bar is set:
the tail's cost is reported as n_k minus b.  One JSON line at the end.  Not imported by bench.py or the package."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

T, B, V, BEAM = 1000, 32, 29, 16
SIZES = (1, 4, 16)


def worker(args):
    import numpy as np
    import torch
    from policy_gradient_asr_amd import _lib, hipops
    if not torch.cuda.is_available():
        raise SystemExit("nbest_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    libs = {"new": _lib.load()}
    if args.parent_lib:
        lib = C.CDLL(args.parent_lib)
        for name, (res, argtypes) in _lib.SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, argtypes
        assert lib.pgasr_abi_version() == 7 and not hasattr(lib, "pgasr_ctc_beam_search_nbest"), "--parent-lib already has the N-best entry"
        libs["parent"] = lib
    rng = np.random.default_rng(424245)
    logits = rng.normal(size=(T, B, V)) * 2.0
    m = logits.max(axis=-1, keepdims=True)
    lp = torch.from_numpy((logits - (m + np.log(np.exp(logits - m).sum(axis=-1, keepdims=True)))).astype(np.float32)).to(dev)
    configs = {}
    if "parent" in libs:
        configs["a_parent_1best"] = ("parent", lambda: hipops.ctc_beam_search(lp, None, beam=BEAM, generic=True))
    configs["b_new_1best"] = ("new", lambda: hipops.ctc_beam_search(lp, None, beam=BEAM, generic=True))
    for n in SIZES:
        configs["n%d" % n] = ("new", lambda n=n: hipops.ctc_beam_search_nbest(lp, None, beam=BEAM, nbest=n))
    names = list(configs)

    def window(name, calls):
        lib, fn = configs[name]
        _lib._lib = libs[lib]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls          # ms per call

    try:
        for name in names:
            window(name, args.warm)
        times = {name: [] for name in names}
        for r in range(args.repeats):
            for name in (names if r % 2 == 0 else names[::-1]):
                times[name].append(window(name, args.calls))
    finally:
        _lib._lib = libs["new"]
    one = hipops.ctc_beam_search(lp, None, beam=BEAM, generic=True)
    nb = hipops.ctc_beam_search_nbest(lp, None, beam=BEAM, nbest=16)
    same = bool(torch.equal(nb.tokens[0], one[0]) and torch.equal(nb.lengths[0], one[1]) and torch.equal(nb.score[0], one[2]))
    result = {"shape": {"T": T, "B": B, "V": V, "beam": BEAM}, "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "calls_per_window": args.calls, "row0_equals_1best": same, "configs": {}}
    for name in names:
        v = times[name]
        e = result["configs"][name] = {"ms_per_call": [round(x, 4) for x in v], "median": round(statistics.median(v), 4),
                                       "min": round(min(v), 4), "max": round(max(v), 4)}
        print(f"{name:15s}: median {e['median']:.3f} ms  (min {e['min']:.3f}, max {e['max']:.3f})", flush=True)
    b_med = result["configs"]["b_new_1best"]["median"]
    for n in SIZES:
        result["n%d_minus_b_ms" % n] = round(result["configs"]["n%d" % n]["median"] - b_med, 4)
    if "parent" in libs:
        a = result["configs"]["a_parent_1best"]
        result["b_over_a"] = round(b_med / a["median"], 4)
        result["b_inside_spread_of_a"] = bool(a["min"] <= b_med <= a["max"])
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libpgasr_hip.so built from the parent commit; without it (a) is not measured")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--warm", type=int, default=3, help="warm-up calls per configuration")
    ap.add_argument("--limit", type=int, default=240, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(args.repeats), "--calls", str(args.calls),
           "--warm", str(args.warm)] + (["--parent-lib", args.parent_lib] if args.parent_lib else [])
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"nbest_cost.py: the measuring child ran past {args.limit} s and was killed; nothing else was started")
    sys.exit(rc)


if __name__ == "__main__":
    main()
