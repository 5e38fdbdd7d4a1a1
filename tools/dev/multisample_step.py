"""Multi-sample REINFORCE: what K sampled paths per utterance cost the train step (NOTES.md, "Multi-sample REINFORCE").

Headline step (B = 32, T = 1000, f32, greedy hypothesis) at the default (K = 1), K = 4 against the greedy hypothesis and K = 4
with the leave-one-out baseline; configs[4] (beam-16 hypothesis, lengths U[500,1000] bucketed) at the default against K = 4
leave-one-out.  One trainer, inputs resident in HBM; the configurations are timed in alternating rounds (ROUNDS x STEPS steps each,
after WARM steps) so that drift of the box falls on all of them alike; per configuration the median round and the loss-section
phase of the step (last forward sweep end -> first backward sweep start, hipops.profile_phases).

  python tools/dev/multisample_step.py [out.json]        (ROUNDS=5 STEPS=30 WARM=4)
  MODE=trace CONFIG=k4_loo python tools/dev/multisample_step.py   (a few steps of one configuration, for rocprofv3 --kernel-trace)
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

CONFIGS = {   # name -> (workload, reward_decoder, num_samples, reward_baseline)
    "default": ("headline", "greedy", 1, "hypothesis"),
    "k4_greedy": ("headline", "greedy", 4, "hypothesis"),
    "k4_loo": ("headline", "greedy", 4, "leave_one_out"),
    "c4_default": ("bucketed", "beam", 1, "hypothesis"),
    "c4_k4_loo": ("bucketed", "beam", 4, "leave_one_out"),
}


def main():
    dev = torch.device("cuda:0")
    rounds, steps, warm = (int(os.environ.get(k, d)) for k, d in (("ROUNDS", 5), ("STEPS", 30), ("WARM", 4)))
    torch.manual_seed(0)
    model = Seq2Seq(bench.V, n_feats=bench.F)
    model.apply(weights)
    model = model.to(dev).train()
    trainer = PolicyGradientTrainer(model, lr=5e-4, lam=1.0, seed=1234, precision="f32")
    batches = {"headline": [[t.to(dev) for t in bench.synth_batch(100)]],
               "bucketed": [[t.to(dev) for t in bench.synth_batch(1000 + 17 * i, lens)]
                            for i, lens in enumerate(bench.bucketed_pool(0, 1, n_batches=8, seed=0))]}
    counter = [0]

    def use(name):
        work, dec, k, base = CONFIGS[name]
        trainer.reward_decoder, trainer.beam_size = dec, 16
        trainer.num_samples, trainer.reward_baseline = k, base
        return batches[work]

    def run(bs, n, marks=None):
        for _ in range(n):
            b = bs[counter[0] % len(bs)]
            counter[0] += 1
            if marks is not None:
                e0 = torch.cuda.Event(enable_timing=True); e0.record()
            trainer.step(*b)
            if marks is not None:
                e1 = torch.cuda.Event(enable_timing=True); e1.record()
                marks.append((e0, e1))

    if os.environ.get("MODE") == "trace":
        bs = use(os.environ.get("CONFIG", "k4_loo"))
        run(bs, warm + steps)
        torch.cuda.synchronize()
        hipops.lstm_assert_no_timeouts()
        return

    names = list(CONFIGS)
    ms = {n: [] for n in names}
    for n in names:                                    # every shape and decoder warmed before the first timed round
        run(use(n), warm)
    torch.cuda.synchronize()
    for r in range(rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            bs = use(n)
            run(bs, warm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(bs, steps)
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) / steps * 1e3)
    hipops.lstm_assert_no_timeouts()
    phases = {}
    for n in names:
        bs = use(n)
        run(bs, warm)
        marks = []
        hipops.profile_reset(True, only=("lstm_",))
        run(bs, 10, marks)
        phases[n] = hipops.profile_phases(marks)
        hipops.profile_reset(False)
    out = {}
    for n in names:
        work, dec, k, base = CONFIGS[n]
        out[n] = {"workload": work, "reward_decoder": dec, "num_samples": k, "reward_baseline": base,
                  "ms_per_step_median": statistics.median(ms[n]), "ms_per_step_rounds": ms[n],
                  "loss_section_ms": (phases[n] or {}).get("loss_section"), "phases_ms": phases[n]}
        print(f"{n:12s} {work:9s} {dec:6s} K={k} {base:13s} step {statistics.median(ms[n]):7.3f} ms "
              f"(rounds {min(ms[n]):.3f} .. {max(ms[n]):.3f})  loss section "
              f"{out[n]['loss_section_ms'] if out[n]['loss_section_ms'] is None else round(out[n]['loss_section_ms'], 4)} ms",
              flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else None
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        json.dump({"rounds": rounds, "steps": steps, "warm": warm, "device": torch.cuda.get_device_name(0), "configs": out},
                  open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
