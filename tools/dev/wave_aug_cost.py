"""What noise and reverberation augmentation (pgasr_reverb, pgasr_wave_power, pgasr_wave_mix; NOTES.md 0.22) costs at the headline
batch, B = 32 utterances of 10 s at 16 kHz (160000 samples each: 20 MB per batch):

  rir2000 / rir8000 / rir16000 : `reverb` with every row filtered by a response of that many taps (0.125 / 0.5 / 1 s).  The kernel is
      bound by its fp64 multiply-adds, B * n * K of them less the edges; `fma_fraction` is that count / time over the chip's fp64
      vector rate, 256 CUs x 4 SIMDs x 16 lanes per clock x 2.4 GHz = 3.93e13 per second.
  stream  : the three powers (dry, wet, the wrapped noise segment) and the mix, each alone; `hbm_fraction` is bytes / time over 8.0 TB/s.
  chain   : the whole of features.WaveAugment (8000-tap responses, noise on every row) at rir_prob 0.5 and 1.0, draws and uploads
      included, and `logmel80_rest`, the rest of LogMel(80) on the same batch.

The launches rotate over --sets buffer pairs (default 8: ~330 MB, more than the 256 MiB Infinity Cache), so their bytes come from HBM.
Each case runs in a child process of its own under a time limit (--limit seconds); the first failure ends the run.  A timing is the
time between two HIP events around --calls back-to-back calls, divided by the calls; the median, minimum and maximum of --repeats
such windows are printed.  The headline step time is bench.py's: this stage sits in front of the framing and runs nothing of the
train step.  There is no pass/fail bar.  Not imported by bench.py or the package."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CASES = ("rir2000", "rir8000", "rir16000", "stream", "chain")
B, N = 32, 160000
HBM_PEAK, FMA_PEAK = 8.0e12, 256 * 4 * 16 * 2.4e9


def timed(fn, repeats, calls):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1) / calls)
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def fma_count(n, K, d):
    """Multiply-adds of one row: the (i, k) pairs with 0 <= i + d - k < n."""
    return sum(max(0, min(n, n + k - d) - max(0, k - d)) for k in range(K))


def child(case, repeats, calls, sets):
    sys.path.insert(0, ROOT)
    import torch
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.features import LogMel, NoiseBank, RirBank, WaveAugment
    if not torch.cuda.is_available():
        raise SystemExit("wave_aug_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1234)
    n = torch.full((B,), N, dtype=torch.int32, device=dev)
    waves = [0.1 * torch.randn(B, N, generator=g, device=dev) for _ in range(sets)]
    outs = [torch.empty(B, N, dtype=torch.float32, device=dev) for _ in range(sets)]
    turn = [0]

    def rotate():
        turn[0] = (turn[0] + 1) % sets
        return turn[0]

    def rir_bank(K, count=4):
        t = torch.arange(K, dtype=torch.float32)
        hs = [torch.randn(K, generator=torch.Generator().manual_seed(r)) * torch.exp(-6.0 * t / K) for r in range(count)]
        for h in hs:
            h[K // 100] = 4.0                               # the direct path, a little into the response
        return RirBank(hs, device=dev)

    out = {"case": case, "B": B, "n": N, "device": torch.cuda.get_device_name(0)}
    if case.startswith("rir"):
        K = int(case[3:])
        bank = rir_bank(K)
        idx = (torch.arange(B, device=dev) % len(bank)).to(torch.int32)

        def launch():
            k = rotate()
            hipops.reverb(waves[k], n, bank.wave, bank.len_dev, bank.delay_dev, idx, out=outs[k])
        out["taps"], out["delays"] = K, bank.delays
        out["reverb"] = timed(launch, repeats, max(calls // 4, 1))
        fmas = sum(fma_count(N, K, bank.delays[b % len(bank)]) for b in range(B))
        out["fmas"] = fmas
        out["reverb"]["fma_fraction"] = round(fmas / (out["reverb"]["median_us"] * 1e-6) / FMA_PEAK, 3)
    elif case == "stream":
        noise = NoiseBank([0.3 * torch.randn(m, generator=torch.Generator().manual_seed(m)) for m in (48000, 160000, 400000)], device=dev)
        nidx = (torch.arange(B, device=dev) % 3).to(torch.int32)
        start = (torch.arange(B, device=dev) * 977).to(torch.int32)
        period = noise.len_dev[nidx.long()]
        p = torch.empty(B, dtype=torch.float64, device=dev)
        out["power_signal"] = timed(lambda: hipops.wave_power(waves[rotate()], n, out=p), repeats, calls)
        out["power_signal"]["hbm_fraction"] = round(4 * B * N / (out["power_signal"]["median_us"] * 1e-6) / HBM_PEAK, 3)
        pn = torch.empty(B, dtype=torch.float64, device=dev)
        out["power_noise"] = timed(lambda: hipops.wave_power(noise.wave, n, row=nidx, start=start, period=period, out=pn), repeats, calls)
        amp = torch.full((B,), 10.0 ** -0.5, dtype=torch.float64, device=dev)

        def launch():
            k = rotate()
            hipops.wave_mix(waves[k], n, p, p, pn, amp, noise.wave, noise.len_dev, nidx, start, out=outs[k])
        out["mix"] = timed(launch, repeats, calls)
        out["mix"]["hbm_fraction"] = round(3 * 4 * B * N / (out["mix"]["median_us"] * 1e-6) / HBM_PEAK, 3)
    else:
        noise = NoiseBank([0.3 * torch.randn(m, generator=torch.Generator().manual_seed(m)) for m in (48000, 160000, 400000)], device=dev)
        bank = rir_bank(8000)
        ids = list(range(B))
        for prob in (0.5, 1.0):
            aug = WaveAugment(noise=noise, snr_db=(5.0, 20.0), noise_prob=1.0, rir=bank, rir_prob=prob)
            out[f"reverberated_rows_at_{prob}"] = int((aug.draws(ids, 7, 0)["rir_idx"] >= 0).sum())

            def launch(aug=aug):
                k = rotate()
                aug(waves[k], n, ids, 7, 0, out=outs[k])
            out[f"chain_rir_prob_{prob}"] = timed(launch, repeats, max(calls // 4, 1))
        fe = LogMel(80, dev)
        rows = [waves[0][b] for b in range(B)]
        out["logmel80_rest"] = timed(lambda: fe(rows), repeats, max(calls // 4, 1))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=CASES, default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=40, help="back-to-back calls per timed window (a quarter of it for the long launches)")
    ap.add_argument("--sets", type=int, default=8, help="buffer pairs the launches rotate over")
    ap.add_argument("--limit", type=int, default=120, help="seconds a case may take")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.repeats, args.calls, args.sets)
    for case in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--repeats", str(args.repeats),
                            "--calls", str(args.calls), "--sets", str(args.sets)], timeout=args.limit)
        if r.returncode != 0:
            raise SystemExit(f"case {case} ended with status {r.returncode}: nothing further is run")


if __name__ == "__main__":
    main()
