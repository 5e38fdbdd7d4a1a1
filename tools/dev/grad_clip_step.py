"""Gradient clipping: what ``max_grad_norm`` costs the train step (NOTES.md 0.04).

Headline step (B = 32, T = 1000, F = 80, V = 29, f32, train mode, inputs resident in HBM) with ``max_grad_norm=None`` against a
finite bound (BOUND, default 1.0: every step of a freshly initialised model is clipped) and against float("inf") (measure and
guard, never scale).  One trainer per configuration on identically initialised models; the configurations are timed in alternating
rounds (ROUNDS x STEPS steps each, after WARM steps) so that drift of the box falls on all of them alike.

  python tools/dev/grad_clip_step.py [out.json]        (ROUNDS=7 STEPS=30 WARM=4 BOUND=1.0)
  MODE=trace python tools/dev/grad_clip_step.py         (a few clipped steps, for rocprofv3 --kernel-trace --stats)
Not imported by bench.py or the package."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from policy_gradient_asr_amd import hipops  # noqa: E402
from policy_gradient_asr_amd.model import Seq2Seq, weights  # noqa: E402
from policy_gradient_asr_amd.train_step import FLAG_PAD, PolicyGradientTrainer  # noqa: E402


def make_trainer(dev, bound):
    torch.manual_seed(0)
    model = Seq2Seq(bench.V, n_feats=bench.F)
    model.apply(weights)
    model = model.to(dev).train()
    return PolicyGradientTrainer(model, lr=5e-4, lam=1.0, seed=1234, precision="f32", max_grad_norm=bound)


def main():
    dev = torch.device("cuda:0")
    rounds, steps, warm = (int(os.environ.get(k, d)) for k, d in (("ROUNDS", 7), ("STEPS", 30), ("WARM", 4)))
    bound = float(os.environ.get("BOUND", "1.0"))
    batch = [t.to(dev) for t in bench.synth_batch(100)]

    def run(tr, n):
        for _ in range(n):
            tr.step(*batch)

    if os.environ.get("MODE") == "trace":
        tr = make_trainer(dev, bound)
        run(tr, warm + steps)
        torch.cuda.synchronize()
        hipops.lstm_assert_no_timeouts()
        print("clip counts", tr.clip_counts(), "last norm", float(tr.last_grad_norm),
              "norm bytes", 4 * (tr.gflat.numel() - FLAG_PAD))
        return

    trainers = {"none": make_trainer(dev, None), "clip": make_trainer(dev, bound), "inf": make_trainer(dev, float("inf"))}
    names = list(trainers)
    ms = {n: [] for n in names}
    for n in names:
        run(trainers[n], warm)
    torch.cuda.synchronize()
    for r in range(rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            run(trainers[n], warm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(trainers[n], steps)
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) / steps * 1e3)
    hipops.lstm_assert_no_timeouts()
    out = {}
    for n in names:
        tr = trainers[n]
        out[n] = {"max_grad_norm": tr.max_grad_norm, "ms_per_step_median": statistics.median(ms[n]), "ms_per_step_rounds": ms[n],
                  "clip_counts": tr.clip_counts(), "calls": tr.nstep, "applied": tr.applied_steps(),
                  "last_grad_norm": None if tr.last_grad_norm is None else float(tr.last_grad_norm)}
        print(f"{n:5s} max_grad_norm={tr.max_grad_norm}  step {out[n]['ms_per_step_median']:7.3f} ms "
              f"(rounds {min(ms[n]):.3f} .. {max(ms[n]):.3f})  clipped/skipped {out[n]['clip_counts']} of {tr.nstep} calls, "
              f"last norm {out[n]['last_grad_norm']}", flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else None
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        json.dump({"rounds": rounds, "steps": steps, "warm": warm, "bound": bound, "device": torch.cuda.get_device_name(0),
                   "configs": out}, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
