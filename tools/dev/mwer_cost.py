"""What MWER training over N-best lists costs (mwer.MWERTrainer, csrc/beam.hip's single-wave N-best tail; NOTES.md 0.15), and whether
adding it left the default step alone.

Part 1, the search.  Headline shape: T = 1000, B = 32, V = 29, beam 16, fp32 log-probs, no language model, one library (this tree's):
  (s1)          ctc_beam_search(...) in its default dispatch: the single-wave kernel's 1-best tail;
  (f1, f4, f16) ctc_beam_search_nbest(fast=True) at N = 1, 4, 16: the same kernel with the N-best tail;
  (g1, g4, g16) ctc_beam_search_nbest(...) at N = 1, 4, 16: the workgroup-per-utterance kernel, the call of before.
The one bar: f16 must be faster than g16, else the dispatch is not taking the new kernel.

Part 2, the step.  Headline step: B = 32, T = 1000, F = 80, V = 29, "f32", train mode, lam = 1:
  (a) the default PolicyGradientTrainer step, a library built from the PARENT commit (--parent-lib; e.g. `git worktree add /tmp/parent
      HEAD~1 && make -C /tmp/parent/policy_gradient_asr_amd/csrc`);
  (b) the same step, this tree's library: the same kernel text, so (b) against (a) is the box;
  (m) the MWERTrainer step at nbest = 4, beam_size = 16, this tree's library.
No bar: (m) minus (b) is reported.

The measurement runs in ONE child process under a time limit (--limit seconds; the parent never touches the GPU and starts nothing
after a child that failed or was killed).  Every configuration is warmed up, then every repeat times a window of back-to-back calls
or steps of every configuration in turn between two device events, the order reversed every other repeat.  One JSON line at the
end.  Not imported by bench.py or the package."""
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


def measure(configs, use, warm, repeats, n):
    """configs: name -> (library, fn).  Returns name -> [ms per call] over the repeats."""
    import torch
    names = list(configs)

    def window(name, calls):
        lib, fn = configs[name]
        use(lib)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    for name in names:
        window(name, warm)
    times = {name: [] for name in names}
    for r in range(repeats):
        for name in (names if r % 2 == 0 else names[::-1]):
            times[name].append(window(name, n))
    return times


def summary(times):
    out = {}
    for name, v in times.items():
        e = out[name] = {"ms": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "min": round(min(v), 4),
                         "max": round(max(v), 4)}
        print(f"{name:16s}: median {e['median']:.3f} ms  (min {e['min']:.3f}, max {e['max']:.3f})", flush=True)
    return out


def worker(args):
    import numpy as np
    import torch
    import bench
    from policy_gradient_asr_amd import _lib, hipops
    from policy_gradient_asr_amd.model import Seq2Seq, weights
    from policy_gradient_asr_amd.mwer import MWERTrainer
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    if not torch.cuda.is_available():
        raise SystemExit("mwer_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    libs = {"new": _lib.load()}
    if args.parent_lib:
        lib = C.CDLL(args.parent_lib)
        for name, (res, argtypes) in _lib.SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, argtypes
        assert lib.pgasr_abi_version() == 7 and not hasattr(lib, "pgasr_mwer_weights"), "--parent-lib already has the MWER entries"
        libs["parent"] = lib

    def use(name):
        _lib._lib = libs[name]

    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats}
    try:
        # ---- part 1: the search ----
        rng = np.random.default_rng(424245)
        logits = rng.normal(size=(T, B, V)) * 2.0
        m = logits.max(axis=-1, keepdims=True)
        lp = torch.from_numpy((logits - (m + np.log(np.exp(logits - m).sum(axis=-1, keepdims=True)))).astype(np.float32)).to(dev)
        configs = {"s1_1best": ("new", lambda: hipops.ctc_beam_search(lp, None, beam=BEAM))}
        for n in SIZES:
            configs["f%d_fast" % n] = ("new", lambda n=n: hipops.ctc_beam_search_nbest(lp, None, beam=BEAM, nbest=n, fast=True))
        for n in SIZES:
            configs["g%d_workgroup" % n] = ("new", lambda n=n: hipops.ctc_beam_search_nbest(lp, None, beam=BEAM, nbest=n))
        search = summary(measure(configs, use, args.warm, args.repeats, args.calls))
        one = hipops.ctc_beam_search(lp, None, beam=BEAM)
        nb = hipops.ctc_beam_search_nbest(lp, None, beam=BEAM, nbest=16, fast=True)
        result["search"] = {"shape": {"T": T, "B": B, "V": V, "beam": BEAM}, "calls_per_window": args.calls, "configs": search,
                            "row0_equals_1best": bool(torch.equal(nb.tokens[0], one[0]) and torch.equal(nb.lengths[0], one[1])
                                                      and torch.equal(nb.score[0], one[2]))}
        for n in SIZES:
            result["search"]["f%d_minus_s1_ms" % n] = round(search["f%d_fast" % n]["median"] - search["s1_1best"]["median"], 4)
        result["search"]["f16_faster_than_g16"] = bool(search["f16_fast"]["median"] < search["g16_workgroup"]["median"])

        # ---- part 2: the step ----
        def trainer(cls, **kw):
            torch.manual_seed(0)
            model = Seq2Seq(bench.V, n_feats=bench.F)
            model.apply(weights)
            return cls(model.to(dev).train(), lr=5e-4, lam=1.0, seed=1234, precision="f32", **kw)

        default, mwer = trainer(PolicyGradientTrainer), trainer(MWERTrainer, nbest=4, beam_size=16)
        batch = [t.to(dev) for t in bench.synth_batch(100)]
        configs = {}
        if "parent" in libs:
            configs["a_parent_default"] = ("parent", lambda: default.step(*batch))
        configs["b_new_default"] = ("new", lambda: default.step(*batch))
        configs["m_new_mwer"] = ("new", lambda: mwer.step(*batch))
        step = summary(measure(configs, use, args.warm, args.repeats, args.steps))
        hipops.lstm_assert_no_timeouts()
        result["step"] = {"shape": {"B": batch[0].shape[0], "T": batch[0].shape[2], "F": bench.F, "V": bench.V}, "nbest": 4, "beam_size": 16,
                          "steps_per_window": args.steps, "configs": step,
                          "m_minus_b_ms": round(step["m_new_mwer"]["median"] - step["b_new_default"]["median"], 4),
                          "m_over_b": round(step["m_new_mwer"]["median"] / step["b_new_default"]["median"], 4)}
        if "parent" in libs:
            a = step["a_parent_default"]
            result["step"]["b_over_a"] = round(step["b_new_default"]["median"] / a["median"], 4)
            result["step"]["b_inside_spread_of_a"] = bool(a["min"] <= step["b_new_default"]["median"] <= a["max"])
    finally:
        use("new")
    print(json.dumps(result))
    sys.exit(0 if result["search"]["f16_faster_than_g16"] else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libpgasr_hip.so built from the parent commit; without it (a) is not measured")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="search calls per timed window")
    ap.add_argument("--steps", type=int, default=20, help="train steps per timed window")
    ap.add_argument("--warm", type=int, default=3, help="warm-up calls / steps per configuration")
    ap.add_argument("--limit", type=int, default=300, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(args.repeats), "--calls", str(args.calls),
           "--steps", str(args.steps), "--warm", str(args.warm)] + (["--parent-lib", args.parent_lib] if args.parent_lib else [])
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"mwer_cost.py: the measuring child ran past {args.limit} s and was killed; nothing else was started")
    sys.exit(rc)


if __name__ == "__main__":
    main()
