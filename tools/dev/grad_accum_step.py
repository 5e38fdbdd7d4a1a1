"""Gradient accumulation: what ``step_accumulated`` costs and saves against ``step`` (NOTES.md 0.05).

Headline shape (T = 1000, F = 80, V = 29, f32, train mode, inputs resident in HBM), one trainer per configuration on identically
initialised models, timed in alternating rounds (ROUNDS x STEPS units each, after WARM units) so that drift of the box falls on
all of them alike.  A unit is what one configuration does for its utterances:
  (a) step_32        one step() of B = 32                     against  acc_1x32      step_accumulated([that batch])
  (b) step_4x32      four step() calls, four batches of 32    against  acc_4x32      one step_accumulated of the four
  (c) step_64        one step() of B = 64 (sequential order)  against  acc_2x32      one step_accumulated of 2 x 32
  (d) acc_4x32_ids   (b)'s accumulated step with explicit utt_ids (the id-addressed sampler inside the lattice window)
Printed per configuration: ms per unit (median round; range) and microseconds per utterance.

  python tools/dev/grad_accum_step.py [out.json]        (ROUNDS=7 STEPS=30 WARM=4)
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
from policy_gradient_asr_amd.train_step import PolicyGradientTrainer  # noqa: E402


def make_trainer(dev):
    torch.manual_seed(0)
    model = Seq2Seq(bench.V, n_feats=bench.F)
    model.apply(weights)
    model = model.to(dev).train()
    return PolicyGradientTrainer(model, lr=5e-4, lam=1.0, seed=1234, precision="f32")


def main():
    dev = torch.device("cuda:0")
    rounds, steps, warm = (int(os.environ.get(k, d)) for k, d in (("ROUNDS", 7), ("STEPS", 30), ("WARM", 4)))
    b32 = [tuple(t.to(dev) for t in bench.synth_batch(100 + i, lengths=[bench.T] * 32)) for i in range(4)]
    b64 = tuple(torch.cat((p, q), dim=0) for p, q in zip(b32[0], b32[1]))
    ids = [list(range(127 - 32 * j, 95 - 32 * j, -1)) for j in range(4)]       # a permutation of 0 .. 127: explicit, not the default rule

    def four_steps(tr):
        for b in b32:
            tr.step(*b)

    # name -> (utterances per unit, the unit)
    units = {
        "step_32": (32, lambda tr: tr.step(*b32[0])),
        "acc_1x32": (32, lambda tr: tr.step_accumulated(b32[:1])),
        "step_4x32": (128, four_steps),
        "acc_4x32": (128, lambda tr: tr.step_accumulated(b32)),
        "acc_4x32_ids": (128, lambda tr: tr.step_accumulated(b32, utt_ids=ids)),
        "step_64": (64, lambda tr: tr.step(*b64)),
        "acc_2x32": (64, lambda tr: tr.step_accumulated(b32[:2])),
    }
    names = list(units)
    trainers = {n: make_trainer(dev) for n in names}
    ms = {n: [] for n in names}

    def run(n, k):
        for _ in range(k):
            units[n][1](trainers[n])

    for n in names:
        run(n, warm)
    torch.cuda.synchronize()
    for r in range(rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            run(n, warm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(n, steps)
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) / steps * 1e3)
    hipops.lstm_assert_no_timeouts()
    out = {}
    for n in names:
        tr, utts = trainers[n], units[n][0]
        med = statistics.median(ms[n])
        out[n] = {"utterances_per_unit": utts, "ms_per_unit_median": med, "ms_per_unit_rounds": ms[n],
                  "us_per_utterance_median": med * 1e3 / utts, "optimizer_steps": tr.nstep, "applied": tr.applied_steps()}
        print(f"{n:13s} {utts:4d} utterances  {med:8.3f} ms per unit (rounds {min(ms[n]):.3f} .. {max(ms[n]):.3f})  "
              f"{med * 1e3 / utts:7.2f} us per utterance  ({tr.nstep} optimizer steps, {out[n]['applied']} applied)", flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else None
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        json.dump({"rounds": rounds, "steps": steps, "warm": warm, "device": torch.cuda.get_device_name(0), "configs": out},
                  open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
