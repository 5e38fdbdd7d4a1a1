"""Sequence-level REINFORCE (score_function="sequence"): what it costs the train step and what it buys (NOTES.md 0.06).

Headline shape (B = 32, T = 1000, V = 29, f32, train mode, inputs resident), K = 4, leave-one-out and greedy-hypothesis baselines:
score_function="path" against "sequence" at max_hyp_len=None and at max_hyp_len = 2 L = 200, timed in alternating rounds (ROUNDS x
STEPS steps after WARM) with the learning rate at 0 so that the model -- and with it the hypothesis lengths -- stays what it is:
once freshly initialised (hypotheses of ~0.9 T tokens, the worst case) and once after TRAIN_STEPS steps on learnable batches (every
target symbol is a noisy code held for 10 frames, data.SyntheticSpeech's recipe at the headline shape; hypotheses near the target
length).  Per configuration the median round, the loss-section phase (hipops.profile_phases), the peak device memory of a step and
the share of samples that took the sequence term.

  python tools/dev/seq_score_step.py [out.json]          (ROUNDS=3 STEPS=15 WARM=3 TRAIN_STEPS=80)
  MODE=trace CONFIG=seq_loo STATE=fresh|trained python tools/dev/seq_score_step.py     (a few steps, for rocprofv3 --kernel-trace)
  MODE=variance OFFSETS=256 python tools/dev/seq_score_step.py [out.json]
      the REINFORCE part of d(logits) on the trained model's fixed logits over OFFSETS sampler offsets, both score functions:
      (a) share of the TOP coordinates (largest |mean|) whose two means agree within three standard errors,
      (b) the ratio of the summed per-coordinate variances, sequence over path.
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
from policy_gradient_asr_amd.loss import pg_ctc_loss  # noqa: E402
from policy_gradient_asr_amd.model import Seq2Seq, weights  # noqa: E402
from policy_gradient_asr_amd.train_step import PolicyGradientTrainer  # noqa: E402

L = bench.T // 10
CONFIGS = {   # name -> (reward_baseline, score_function, max_hyp_len)
    "path_loo": ("leave_one_out", "path", None),
    "seq_loo": ("leave_one_out", "sequence", None),
    "seq_loo_cap": ("leave_one_out", "sequence", 2 * L),
    "path_greedy": ("hypothesis", "path", None),
    "seq_greedy": ("hypothesis", "sequence", None),
    "seq_greedy_cap": ("hypothesis", "sequence", 2 * L),
}
K = 4


def learnable_batch(seed, dev):
    """bench.synth_batch's shapes with features the targets can be read from: symbol i of utterance b is a fixed random code plus
    noise, held for 10 frames."""
    g = torch.Generator().manual_seed(seed)
    proto = torch.randn(bench.V, bench.F, generator=torch.Generator().manual_seed(12345))
    B, T = bench.B_PER_GPU, bench.T
    targets = torch.randint(1, bench.V, (B, L), generator=g)
    x = proto[targets].repeat_interleave(T // L, dim=1).transpose(1, 2).contiguous()       # (B,F,T)
    x = x + 0.3 * torch.randn(x.shape, generator=g)
    return [x.to(dev), targets.to(dev), torch.ones(B, T, device=dev), torch.ones(B, L, dtype=torch.int64, device=dev)]


def main():
    dev = torch.device("cuda:0")
    rounds, steps, warm, train_steps = (int(os.environ.get(k, d)) for k, d in (("ROUNDS", 3), ("STEPS", 15), ("WARM", 3),
                                                                                ("TRAIN_STEPS", 80)))
    torch.manual_seed(0)
    model = Seq2Seq(bench.V, n_feats=bench.F)
    model.apply(weights)
    model = model.to(dev).train()
    trainer = PolicyGradientTrainer(model, lr=1e-3, lam=1.0, seed=1234, precision="f32", num_samples=K,
                                    reward_baseline="leave_one_out")
    pool = [learnable_batch(100 + i, dev) for i in range(4)]
    counter = [0]

    def use(name):
        trainer.reward_baseline, trainer.score_function, trainer.max_hyp_len = CONFIGS[name]

    def run(n, marks=None):
        for _ in range(n):
            b = pool[counter[0] % len(pool)]
            counter[0] += 1
            if marks is not None:
                e0 = torch.cuda.Event(enable_timing=True); e0.record()
            trainer.step(*b)
            if marks is not None:
                e1 = torch.cuda.Event(enable_timing=True); e1.record()
                marks.append((e0, e1))

    def train():
        use("path_loo")
        trainer.lr = 1e-3
        run(train_steps)
        trainer.lr = 0.0
        torch.cuda.synchronize()

    mode = os.environ.get("MODE", "time")
    if mode == "trace":
        if os.environ.get("STATE", "fresh") == "trained":
            train()
        trainer.lr = 0.0
        use(os.environ.get("CONFIG", "seq_loo"))
        run(warm + steps)
        torch.cuda.synchronize()
        hipops.lstm_assert_no_timeouts()
        return
    if mode == "variance":
        train()
        out = variance(model, pool[0], int(os.environ.get("OFFSETS", 256)))
        if len(sys.argv) > 1:
            os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
            json.dump(out, open(sys.argv[1], "w"), indent=1)
        return

    out = {}
    trainer.lr = 0.0
    for state in ("fresh", "trained"):
        if state == "trained":
            train()
        names = list(CONFIGS)
        ms = {n: [] for n in names}
        for n in names:
            use(n); run(warm)
        torch.cuda.synchronize()
        for r in range(rounds):
            for n in (names if r % 2 == 0 else names[::-1]):
                use(n)
                run(warm)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(steps)
                torch.cuda.synchronize()
                ms[n].append((time.perf_counter() - t0) / steps * 1e3)
        hipops.lstm_assert_no_timeouts()
        for n in names:
            use(n)
            run(warm)
            marks = []
            hipops.profile_reset(True, only=("lstm_",))
            run(8, marks)
            phases = hipops.profile_phases(marks)
            hipops.profile_reset(False)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base_mem = torch.cuda.memory_allocated()
            run(2)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated()
            scored = trainer.last_sequence_scored
            hyp_ws = sum(v.numel() for k_, v in hipops._ws_cache.items() if k_[0] == "ctc_hyp")
            base, sf, cap = CONFIGS[n]
            out[f"{state}/{n}"] = {
                "state": state, "reward_baseline": base, "score_function": sf, "max_hyp_len": cap,
                "ms_per_step_median": statistics.median(ms[n]), "ms_per_step_rounds": ms[n],
                "loss_section_ms": (phases or {}).get("loss_section"), "phases_ms": phases,
                "peak_memory_bytes": peak, "allocated_before_bytes": base_mem, "hyp_workspace_cached_bytes": hyp_ws,
                "sequence_scored_share": None if scored is None else float(scored.float().mean()),
                "mean_reward": float(trainer.last_sample_rewards.mean())}
            print(f"{state:8s} {n:15s} step {statistics.median(ms[n]):7.3f} ms (rounds {min(ms[n]):.3f} .. {max(ms[n]):.3f})  "
                  f"loss section {(phases or {}).get('loss_section', float('nan')):.4f} ms  peak {peak / 2**30:.3f} GiB "
                  f"(hyp workspace cached {hyp_ws / 2**30:.3f} GiB)  scored {out[f'{state}/{n}']['sequence_scored_share']}  "
                  f"mean R {out[f'{state}/{n}']['mean_reward']:.3f}", flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        json.dump({"rounds": rounds, "steps": steps, "warm": warm, "train_steps": train_steps, "K": K,
                   "device": torch.cuda.get_device_name(0), "configs": out}, open(sys.argv[1], "w"), indent=1)


def variance(model, batch, offsets, top=2000):
    """Mean and variance per coordinate of the REINFORCE part of d(logits) over sampler offsets, path- against sequence-level."""
    x, targets, fmask, tmask = batch
    model.eval()
    with torch.no_grad():
        logits, in_len = model.logits(x, fmask)
    logits = logits.detach().clone()
    tg, tl = targets.to(torch.int32).contiguous(), tmask.sum(1).to(torch.int32).contiguous()

    def grad(**kw):
        z = logits.clone().requires_grad_(True)
        res = pg_ctc_loss(z, in_len, tg, tl, seed=77, **kw)
        res[0].backward()
        return z.grad.double(), res

    g_ctc, _ = grad(lam=0.0)
    out = {"offsets": offsets, "K": K, "top": top}
    for base in ("leave_one_out", "hypothesis"):
        stats = {}
        for sf in ("path", "sequence"):
            s1 = torch.zeros_like(g_ctc); s2 = torch.zeros_like(g_ctc)
            lens = []
            for o in range(offsets):
                g, res = grad(lam=1.0, offset=o + 1, num_samples=K, baseline=base, score_function=sf)
                d = g - g_ctc
                s1 += d; s2 += d * d
                if o == 0:
                    out[f"{base}/mean_reward"] = float(res[2].mean())
            mean = s1 / offsets
            var = (s2 / offsets - mean * mean).clamp_min(0) * offsets / (offsets - 1)
            stats[sf] = (mean, var)
        (mp, vp), (ms_, vs) = stats["path"], stats["sequence"]
        se = ((vp + vs) / offsets).sqrt()
        idx = (mp.abs() + ms_.abs()).flatten().topk(top).indices
        agree = ((mp - ms_).abs().flatten()[idx] <= 3 * se.flatten()[idx]).double().mean()
        ratio = float(vs.sum() / vp.sum())
        out[base] = {"share_of_top_means_within_3_se": float(agree), "variance_ratio_sequence_over_path": ratio,
                     "summed_variance_path": float(vp.sum()), "summed_variance_sequence": float(vs.sum()),
                     "mean_norm_path": float(mp.norm()), "mean_norm_sequence": float(ms_.norm()),
                     "mean_difference_norm": float((mp - ms_).norm())}
        print(f"[variance] K={K} {base}: {float(agree) * 100:.1f} % of the {top} largest means agree within 3 s.e.; summed variance "
              f"sequence / path = {ratio:.4f} ({float(vs.sum()):.4e} / {float(vp.sum()):.4e}); |mean| path {float(mp.norm()):.3e} "
              f"sequence {float(ms_.norm()):.3e} difference {float((mp - ms_).norm()):.3e}; mean reward {out[f'{base}/mean_reward']:.3f}",
              flush=True)
    return out


if __name__ == "__main__":
    main()
