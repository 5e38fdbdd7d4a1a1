"""What the KL penalty towards a frozen reference policy (kl_weight, NOTES.md 0.16) costs the train step, and whether adding it left
the default step alone.  Headline step: B = 32, T = 1000, F = 80, V = 29, "f32", train mode, greedy hypothesis, lam = 1.

  (a) kl_weight = 0, a library built from the PARENT commit (--parent-lib; e.g. `git worktree add /tmp/parent HEAD~1 &&
      make -C /tmp/parent/policy_gradient_asr_amd/csrc`);
  (b) kl_weight = 0, this tree's library;
  (c) kl_weight > 0 with a reference model of the policy's shape (other weights), K = 1 and K = 4, this tree's library -- each beside
      its own weight-0 twin, so that (c) is read against the same objective without the term.  (c) minus its twin is the reference's
      eval forward (three sweeps and their projections, before the policy's), the KL launch under the lattice, and the second row read
      and wave sum of the gradient pass.

Both libraries are loaded into ONE process (the host layer looks its library up per call: `_lib._lib` is swapped between
configurations) and every repeat runs all configurations in turn, so old and new alternate in the same call.  Each timing is a
window of at least --window seconds of back-to-back steps between two device events, after a warm-up of every configuration.
(b) against (a) is a pass/fail bar: the median of (b)'s repeats must lie inside the run-to-run spread (min .. max) of (a)'s own
repeats -- the kernels are the same, so anything else is the box.  (c) has no bar: (c) minus its twin is reported.  One JSON line
at the end.  Not imported by bench.py or the package."""
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
from policy_gradient_asr_amd.model import Seq2Seq, weights  # noqa: E402
from policy_gradient_asr_amd.train_step import PolicyGradientTrainer  # noqa: E402

WEIGHT = 0.1
CONFIGS = {   # name -> (library, num_samples, kl_weight)
    "a_parent_k1_w0": ("parent", 1, 0.0),
    "b_new_k1_w0": ("new", 1, 0.0),
    "c_k1": ("new", 1, WEIGHT),
    "k4_w0": ("new", 4, 0.0),
    "c_k4": ("new", 4, WEIGHT),
}
TWINS = {"c_k1": "b_new_k1_w0", "c_k4": "k4_w0"}


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
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--warm", type=int, default=4, help="warm-up steps per configuration")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kl_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    libs = {"new": _lib.load()}
    if args.parent_lib:
        libs["parent"] = bind(args.parent_lib)
        assert not hasattr(libs["parent"], "pgasr_frame_kl"), "--parent-lib already has the KL entries"
    names = [n for n in CONFIGS if CONFIGS[n][0] in libs]

    def make(seed):
        torch.manual_seed(seed)
        m = Seq2Seq(bench.V, n_feats=bench.F)
        m.apply(weights)
        return m.to(dev)

    model, reference = make(0).train(), make(1)
    trainer = PolicyGradientTrainer(model, lr=5e-4, lam=1.0, seed=1234, precision="f32", kl_reference=reference)
    batch = [t.to(dev) for t in bench.synth_batch(100)]

    def use(name):
        lib, k, w = CONFIGS[name]
        _lib._lib = libs[lib]
        trainer.num_samples, trainer.kl_weight = k, w

    def window(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            trainer.step(*batch)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n          # ms per step

    try:
        calls = {}
        for name in names:                          # warm-up, and the number of steps that fills a window
            use(name)
            window(args.warm)
            calls[name] = max(3, int(args.window * 1e3 / window(args.warm)) + 1)
        hipops.lstm_assert_no_timeouts()
        times = {name: [] for name in names}
        for r in range(args.repeats):
            for name in (names if r % 2 == 0 else names[::-1]):
                use(name)
                times[name].append(window(calls[name]))
        hipops.lstm_assert_no_timeouts()
    finally:
        _lib._lib = libs["new"]

    result = {"shape": {"B": batch[0].shape[0], "T": batch[0].shape[2], "F": bench.F, "V": bench.V},
              "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "window_s": args.window, "kl_weight": WEIGHT,
              "configs": {}}
    for name in names:
        v = times[name]
        result["configs"][name] = {"ms_per_step": [round(x, 4) for x in v], "median": round(statistics.median(v), 4),
                                   "min": round(min(v), 4), "max": round(max(v), 4), "steps_per_window": calls[name]}
        e = result["configs"][name]
        print(f"{name:16s}: median {e['median']:.3f} ms  (min {e['min']:.3f}, max {e['max']:.3f}; {e['steps_per_window']} steps per "
              f"window)", flush=True)
    cfg = result["configs"]
    if "parent" in libs:
        a, b_med = cfg["a_parent_k1_w0"], cfg["b_new_k1_w0"]["median"]
        result["b_inside_spread_of_a"] = bool(a["min"] <= b_med <= a["max"])
        result["b_over_a"] = round(b_med / a["median"], 4)
    else:
        result["b_inside_spread_of_a"] = "not measured"
    for c, twin in TWINS.items():
        result[f"{c}_minus_twin_ms"] = round(cfg[c]["median"] - cfg[twin]["median"], 4)
        result[f"{c}_over_twin"] = round(cfg[c]["median"] / cfg[twin]["median"], 4)
    print(f"(b) inside the spread of (a): {result['b_inside_spread_of_a']};  (c) minus its weight-0 twin: "
          + ", ".join(f"{c} {result[f'{c}_minus_twin_ms']:+.3f} ms" for c in TWINS), flush=True)
    print(json.dumps(result))
    sys.exit(0 if result["b_inside_spread_of_a"] is not False else 1)


if __name__ == "__main__":
    main()
