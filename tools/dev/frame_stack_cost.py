"""What low-frame-rate input (features.FrameStack, NOTES.md 0.41) costs and what it buys, on the MI355X.

  kernel   pgasr_frame_stack alone at B = 32, F = 80, T = 1000 for (stack, skip, left) = (3, 3, 0) and (8, 3, 7): --launches (200)
           back-to-back launches between two device events, every launch on the next of --buffers (24) input / output pairs so that
           the working set (24 x (10.2 + 10.3 .. 27.4) MB) lies past the 256 MiB Infinity Cache; median of --repeats (5) windows,
           beside the bytes the call must move (x once, out once, the two small outputs) and the time those take at the 8.0 TB/s
           HBM peak.  A window measures launches back to back, so it is bounded below by the launch rate of the stream; the kernel's
           own duration comes from a trace (`rocprofv3 --kernel-trace --stats -- python tools/dev/frame_stack_cost.py --only kernel`).
  step     the default train step ("f32", train mode, greedy hypothesis, lam = 1; B = 32, V = 29, 100 target symbols) on the SAME
           audio three ways: (T = 1000, F = 80) as it is, (T' = 334, F = 240) behind FrameStack(3, 3, 0) and (T' = 500, F = 160)
           behind FrameStack(2, 2, 0) -- each with a model of its own width, the stacking launch INSIDE the timed window (it is part
           of what such a step costs).  Every repeat runs the three in turn (the order reversed every other repeat), --steps (20)
           steps per window after --warm (5) warm-up steps each; medians of --repeats (5) windows, and utterances / s from them.

One JSON line at the end.  Not imported by bench.py or the package."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from policy_gradient_asr_amd import hipops  # noqa: E402
from policy_gradient_asr_amd.features import FrameStack  # noqa: E402
from policy_gradient_asr_amd.model import Seq2Seq, weights  # noqa: E402
from policy_gradient_asr_amd.train_step import PolicyGradientTrainer  # noqa: E402

HBM_PEAK_TBS = 8.0
KERNEL_POLICIES = ((3, 3, 0), (8, 3, 7))
STEP_CONFIGS = {"T1000_F80": None, "T334_F240": FrameStack(3, 3, 0), "T500_F160": FrameStack(2, 2, 0)}


def summary(v, digits=4):
    return {"windows": [round(x, digits) for x in v], "median": round(statistics.median(v), digits), "min": round(min(v), digits),
            "max": round(max(v), digits)}


def kernel_cost(args, dev):
    B, F, T = bench.B_PER_GPU, bench.F, bench.T
    lengths = torch.full((B,), T, dtype=torch.int32, device=dev)
    xs = [torch.randn(B, F, T, device=dev) for _ in range(args.buffers)]
    out = {}
    for stack, skip, left in KERNEL_POLICIES:
        Tout = -(-T // skip)
        moved = 4 * (B * F * T + B * stack * F * Tout + B * Tout + 2 * B)          # x, out, fmask_out, n_frames and n_out
        lib = hipops._lib.load()
        outs = [torch.empty(B, stack * F, Tout, device=dev) for _ in range(args.buffers)]
        fm = torch.empty(B, 1, Tout, device=dev)
        n_out = torch.empty(B, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def window(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(n):
                k = i % args.buffers
                rc = lib.pgasr_frame_stack(xs[k].data_ptr(), lengths.data_ptr(), B, F, T, stack, skip, left, Tout, outs[k].data_ptr(),
                                           fm.data_ptr(), n_out.data_ptr(), st)
                assert rc == 0, rc
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n          # us per launch

        window(args.buffers)                              # every buffer touched once, code object loaded
        us = [window(args.launches) for _ in range(args.repeats)]
        e = out["x".join(map(str, (stack, skip, left)))] = summary(us, 3)
        e.update(bytes_moved=moved, working_set_mb=round(args.buffers * moved / 1e6, 1), us_at_hbm_peak=round(moved / (HBM_PEAK_TBS * 1e6), 3),
                 tb_per_s_back_to_back=round(moved / (e["median"] * 1e6), 3))
        print(f"kernel {stack},{skip},{left}: median {e['median']:.2f} us per back-to-back launch (min {e['min']:.2f}, max {e['max']:.2f}); "
              f"{moved / 1e6:.2f} MB = {e['us_at_hbm_peak']:.2f} us at {HBM_PEAK_TBS} TB/s", flush=True)
        del outs
    return out


def step_cost(args, dev):
    batch = [t.to(dev) for t in bench.synth_batch(100)]
    x, targets, fmask, tmask = batch
    runs = {}
    for name, policy in STEP_CONFIGS.items():
        torch.manual_seed(0)
        model = Seq2Seq(bench.V, n_feats=bench.F if policy is None else policy.out_feats(bench.F))
        model.apply(weights)
        runs[name] = (policy, PolicyGradientTrainer(model.to(dev).train(), lr=5e-4, lam=1.0, seed=1234, precision="f32"))

    def window(name, n):
        policy, trainer = runs[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            if policy is None:
                trainer.step(x, targets, fmask, tmask)
            else:
                xs, fms = policy(x, fmask)
                trainer.step(xs, targets, fms.squeeze(1), tmask)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n          # ms per step

    names = list(STEP_CONFIGS)
    for name in names:
        window(name, args.warm)
    hipops.lstm_assert_no_timeouts()
    times = {name: [] for name in names}
    for r in range(args.repeats):
        for name in (names if r % 2 == 0 else names[::-1]):
            times[name].append(window(name, args.steps))
    hipops.lstm_assert_no_timeouts()
    out = {}
    for name in names:
        e = out[name] = summary(times[name])
        e["utterances_per_s"] = round(x.shape[0] / (e["median"] * 1e-3), 1)
        e["over_T1000_F80"] = round(e["median"] / statistics.median(times[names[0]]), 4)
        print(f"step {name:10s}: median {e['median']:.3f} ms (min {e['min']:.3f}, max {e['max']:.3f}) = {e['utterances_per_s']:.0f} utterances/s, "
              f"{e['over_T1000_F80']:.3f} x the T = 1000 step", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("kernel", "step"), default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200, help="kernel launches per timed window")
    ap.add_argument("--buffers", type=int, default=24, help="input / output pairs the launches rotate over")
    ap.add_argument("--steps", type=int, default=20, help="train steps per timed window")
    ap.add_argument("--warm", type=int, default=5, help="warm-up steps per configuration")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_stack_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    result = {"shape": {"B": bench.B_PER_GPU, "T": bench.T, "F": bench.F, "V": bench.V}, "device": torch.cuda.get_device_name(0),
              "repeats": args.repeats}
    if args.only != "step":
        result["kernel_us"] = kernel_cost(args, dev)
    if args.only != "kernel":
        result["step_ms"] = step_cost(args, dev)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
