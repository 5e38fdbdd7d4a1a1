"""Word-level reward: what reward_unit="word" costs the train step against the default character reward (NOTES.md 0.03).

Headline step (B = 32, T = 1000, f32) at K = 1 (greedy hypothesis) and K = 4 (leave-one-out), configs[4] (beam-16 hypothesis,
lengths U[500,1000] bucketed) at K = 1, each with reward_unit "char" and "word".  Both units score the SAME batches: bench.py's
synthetic batches with about 18 % of the target symbols replaced by the delimiter (V - 1, the alphabet's " ").  One trainer, inputs
resident in HBM; the configurations are timed in alternating rounds (ROUNDS x STEPS steps each, after WARM steps); per configuration the
median round and the loss-section phase of the step (last forward sweep end -> first backward sweep start, hipops.profile_phases).

  python tools/dev/word_reward_step.py [out.json]        (ROUNDS=5 STEPS=30 WARM=4)
  MODE=trace CONFIG=word_k4_loo python tools/dev/word_reward_step.py   (a few steps of one configuration, for rocprofv3 --kernel-trace)
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

DELIM = bench.V - 1
CONFIGS = {   # name -> (workload, reward_decoder, num_samples, reward_baseline, reward_unit)
    "char_k1": ("headline", "greedy", 1, "hypothesis", "char"),
    "word_k1": ("headline", "greedy", 1, "hypothesis", "word"),
    "char_k4_loo": ("headline", "greedy", 4, "leave_one_out", "char"),
    "word_k4_loo": ("headline", "greedy", 4, "leave_one_out", "word"),
    "c4_char_k1": ("bucketed", "beam", 1, "hypothesis", "char"),
    "c4_word_k1": ("bucketed", "beam", 1, "hypothesis", "word"),
}


def spaced(batch, seed):
    """bench.synth_batch's batch with ~18 % of the valid target symbols set to the delimiter."""
    x, targets, fmask, tmask = batch
    g = torch.Generator().manual_seed(seed)
    sp = (torch.rand(targets.shape, generator=g) < 0.18) & (tmask > 0)
    targets = targets.clone()
    targets[sp] = DELIM
    return [x, targets, fmask, tmask]


def main():
    dev = torch.device("cuda:0")
    rounds, steps, warm = (int(os.environ.get(k, d)) for k, d in (("ROUNDS", 5), ("STEPS", 30), ("WARM", 4)))
    torch.manual_seed(0)
    model = Seq2Seq(bench.V, n_feats=bench.F)
    model.apply(weights)
    model = model.to(dev).train()
    trainer = PolicyGradientTrainer(model, lr=5e-4, lam=1.0, seed=1234, precision="f32")
    batches = {"headline": [[t.to(dev) for t in spaced(bench.synth_batch(100), 1)]],
               "bucketed": [[t.to(dev) for t in spaced(bench.synth_batch(1000 + 17 * i, lens), 2 + i)]
                            for i, lens in enumerate(bench.bucketed_pool(0, 1, n_batches=8, seed=0))]}
    counter = [0]

    def use(name):
        work, dec, k, base, unit = CONFIGS[name]
        trainer.reward_decoder, trainer.beam_size = dec, 16
        trainer.num_samples, trainer.reward_baseline = k, base
        trainer.reward_unit, trainer.word_delimiter = unit, (DELIM if unit == "word" else None)
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
        bs = use(os.environ.get("CONFIG", "word_k4_loo"))
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
        work, dec, k, base, unit = CONFIGS[n]
        ls = (phases[n] or {}).get("loss_section")
        out[n] = {"workload": work, "reward_decoder": dec, "num_samples": k, "reward_baseline": base, "reward_unit": unit,
                  "ms_per_step_median": statistics.median(ms[n]), "ms_per_step_rounds": ms[n], "loss_section_ms": ls,
                  "phases_ms": phases[n]}
        print(f"{n:12s} {work:9s} {dec:6s} K={k} {base:13s} {unit:4s} step {statistics.median(ms[n]):7.3f} ms "
              f"(rounds {min(ms[n]):.3f} .. {max(ms[n]):.3f})  loss section {ls if ls is None else round(ls, 4)} ms", flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else None
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        json.dump({"rounds": rounds, "steps": steps, "warm": warm, "device": torch.cuda.get_device_name(0), "configs": out},
                  open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
