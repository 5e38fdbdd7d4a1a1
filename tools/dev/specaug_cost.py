"""What SpecAugment masking on the device (features.SpecAugment, NOTES.md 0.12) costs in front of the train step, and whether adding
the kernel to the library left the step alone.  Headline step: B = 32, T = 1000, F = 80, V = 29, "f32", train mode, greedy hypothesis, lam = 1.

  (a) no masking, a library built from the PARENT commit (--parent-lib; e.g. `git worktree add /tmp/parent HEAD~1 &&
      make -C /tmp/parent/policy_gradient_asr_amd/csrc`);
  (b) no masking, this tree's library;
  (c) every step's batch masked first with SpecAugment() (2 x 27 rows, 2 x 100 frames, row-mean fill; seed and offset as a trainer
      integration would pass them: the trainer's seed, nstep + 1) on the step's stream, this tree's library.

All configurations run in ONE process on one trainer (the host layer looks its library up per call: `_lib._lib` is swapped between
configurations), and every repeat runs all of them in turn, so old and new alternate in the same call.  Each timing is --steps (20)
back-to-back steps between two device events, after --warm (5) warm-up steps of every configuration.  (b) against (a) is a pass/fail
bar: the median of (b)'s repeats must lie inside the run-to-run spread (min .. max) of (a)'s own repeats -- the kernels are the same,
so anything else is the box.  (c) has no bar: (c) minus (b), and minus (a) where it was measured, is reported.  The expectation is
one extra read and write of the 10 MB feature tensor.  One JSON line at the end.  Not imported by bench.py or the package."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from policy_gradient_asr_amd import _lib, hipops  # noqa: E402
from policy_gradient_asr_amd.features import SpecAugment  # noqa: E402
from policy_gradient_asr_amd.model import Seq2Seq, weights  # noqa: E402
from policy_gradient_asr_amd.train_step import PolicyGradientTrainer  # noqa: E402

CONFIGS = {   # name -> (library, policy)
    "a_parent_off": ("parent", None),
    "b_new_off": ("new", None),
    "c_new_on": ("new", SpecAugment()),
}


def bind(path):
    """A library bound like _lib.load() binds the product's, without the entries it does not have (the parent's)."""
    lib = C.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    assert lib.pgasr_abi_version() == 7
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libpgasr_hip.so built from the parent commit; without it (a) is not measured")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="steps per timed window")
    ap.add_argument("--warm", type=int, default=5, help="warm-up steps per configuration")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("specaug_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    libs = {"new": _lib.load()}
    if args.parent_lib:
        libs["parent"] = bind(args.parent_lib)
        assert not hasattr(libs["parent"], "pgasr_spec_augment"), "--parent-lib already has the SpecAugment entry"
    names = [n for n in CONFIGS if CONFIGS[n][0] in libs]

    torch.manual_seed(0)
    model = Seq2Seq(bench.V, n_feats=bench.F)
    model.apply(weights)
    model = model.to(dev).train()
    trainer = PolicyGradientTrainer(model, lr=5e-4, lam=1.0, seed=1234, precision="f32")
    batch = [t.to(dev) for t in bench.synth_batch(100)]

    lengths = batch[2].sum(1).to(torch.int32).contiguous()
    state = {"policy": None}

    def use(name):
        lib, state["policy"] = CONFIGS[name]
        _lib._lib = libs[lib]

    def window(n):
        policy = state["policy"]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            x = batch[0] if policy is None else policy(batch[0], lengths, trainer.seed, trainer.nstep + 1)
            trainer.step(x, *batch[1:])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n          # ms per step

    try:
        for name in names:
            use(name)
            window(args.warm)
        hipops.lstm_assert_no_timeouts()
        times = {name: [] for name in names}
        for r in range(args.repeats):
            for name in (names if r % 2 == 0 else names[::-1]):
                use(name)
                times[name].append(window(args.steps))
        hipops.lstm_assert_no_timeouts()
    finally:
        _lib._lib = libs["new"]

    result = {"shape": {"B": batch[0].shape[0], "T": batch[0].shape[2], "F": bench.F, "V": bench.V},
              "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "steps_per_window": args.steps,
              "policy": CONFIGS["c_new_on"][1].state(), "configs": {}}
    for name in names:
        v = times[name]
        e = result["configs"][name] = {"ms_per_step": [round(x, 4) for x in v], "median": round(statistics.median(v), 4),
                                       "min": round(min(v), 4), "max": round(max(v), 4)}
        print(f"{name:13s}: median {e['median']:.3f} ms  (min {e['min']:.3f}, max {e['max']:.3f})", flush=True)
    cfg = result["configs"]
    result["c_minus_b_ms"] = round(cfg["c_new_on"]["median"] - cfg["b_new_off"]["median"], 4)
    if "parent" in libs:
        a, b_med = cfg["a_parent_off"], cfg["b_new_off"]["median"]
        result["b_inside_spread_of_a"] = bool(a["min"] <= b_med <= a["max"])
        result["b_over_a"] = round(b_med / a["median"], 4)
        result["c_minus_a_ms"] = round(cfg["c_new_on"]["median"] - a["median"], 4)
    else:
        result["b_inside_spread_of_a"] = "not measured"
    print(f"(b) inside the spread of (a): {result['b_inside_spread_of_a']};  (c) minus (b): {result['c_minus_b_ms']:+.3f} ms", flush=True)
    print(json.dumps(result))
    sys.exit(0 if result["b_inside_spread_of_a"] is not False else 1)


if __name__ == "__main__":
    main()
