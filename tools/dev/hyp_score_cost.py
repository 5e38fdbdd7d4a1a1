"""What the lattice-free CTC scorer costs (csrc/hyp_score.hip; NOTES.md 0.27).  T = 1000 (--frames), B = 32, fp32 log-probs, lists of
near-equal hypotheses made on the host (one base row per utterance, a few substitutions per list row):

  narrow  V = 29, hypotheses of ~930 symbols, N in {16, 64, 128}: ``hipops.ctc_hyp_score``; at N = 16 also ``hipops.ctc_hyp_lattice``
          on the same inputs in the same process (its code is the parent commit's) with the workspace it takes;
  wide    V in {256, 1024}, hypotheses of ~300 units, N in {16, 128}: the scorer, the composed pair-distance path on the same
          lists, and at the sizes of --mbr-sizes the whole ``CTCDecoder.mbr_decode`` (search, scorer, distances, selection) on the
          same log-probs.

The measurement runs in ONE child process under a time limit (--limit seconds; the parent never touches the GPU and starts nothing
after a child that failed or was killed).  Every configuration is warmed up, then every repeat (--repeats 5) times a window of
back-to-back calls between two device events, the order of the configurations reversed every other repeat and the log-probs and
token buffers rotated over --copies copies from call to call; the median of the windows is reported with their minimum and
maximum.  One JSON line at the end.  Not imported by bench.py or the package."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

B = 32


def lattice_bytes(T, N, Lh):
    """pgasr_ctc_hyp_lattice's two sweeps: 2 * N * B * T * roundup64(2 * Lh + 1) * 4 (the per-pair tables are < 2 % more)."""
    return 2 * N * B * T * ((2 * Lh + 1 + 63) // 64 * 64) * 4


def make_list(rng, N, V, L, edits=4):
    """tokens (N,B,L) int32, lengths (N,B): per utterance one random base row without the blank 0, every other row the base with a
    few substitutions and up to two symbols dropped from its end."""
    import numpy as np
    tokens = np.zeros((N, B, L), dtype=np.int32)
    lengths = np.zeros((N, B), dtype=np.int32)
    for b in range(B):
        base = rng.integers(1, V, size=L)
        for n in range(N):
            row = base.copy()
            if n:
                row[rng.integers(0, L, size=edits)] = rng.integers(1, V, size=edits)
            ln = L - (n % 3)
            tokens[n, b, :ln] = row[:ln]
            lengths[n, b] = ln
    return tokens, lengths


def worker(args):
    import numpy as np
    import torch
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    if not torch.cuda.is_available():
        raise SystemExit("hyp_score_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(424247)
    T = args.frames
    in_len = torch.full((B,), T, dtype=torch.int32, device=dev)
    result = {"shape": {"T": T, "B": B}, "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "copies": args.copies,
              "cases": {}}

    def log_probs(V, scale):
        out = []
        for _ in range(args.copies):
            z = torch.from_numpy(rng.normal(size=(T, B, V)).astype(np.float32) * scale).to(dev)
            out.append(torch.log_softmax(z, dim=-1).contiguous())
        return out

    def measure(tag, configs):
        """configs: name -> (calls per window, f(i) with i the running call index)"""
        names = list(configs)
        counter = {n: 0 for n in names}

        def window(name, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                configs[name][1](counter[name])
                counter[name] += 1
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / calls          # ms per call

        for name in names:
            window(name, min(args.warm, configs[name][0]))
        times = {name: [] for name in names}
        for r in range(args.repeats):
            for name in (names if r % 2 == 0 else names[::-1]):
                times[name].append(window(name, configs[name][0]))
        out = {}
        for name in names:
            v = times[name]
            out[name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                         "calls_per_window": configs[name][0]}
            print(f"{tag} {name:9s}: median {statistics.median(v):.4f} ms  (min {min(v):.4f}, max {max(v):.4f})", flush=True)
        return out

    def lists(N, V, L):
        out = []
        for _ in range(args.copies):
            tok, ln = make_list(rng, N, V, L)
            out.append((torch.from_numpy(tok).to(dev), torch.from_numpy(ln).to(dev)))
        return out

    # ---- narrow: V = 29, ~930 symbols ----
    V, L = 29, int(0.93 * T)
    lps = log_probs(V, 2.0)
    for N in (int(x) for x in args.narrow_sizes.split(",")):
        ls = lists(N, V, L)
        score = lambda i: hipops.ctc_hyp_score(lps[i % args.copies], ls[i % args.copies][0], ls[i % args.copies][1], in_len, L)
        configs = {"score": (args.calls, score)}
        entry = {"V": V, "N": N, "hypothesis_length": L, "scorer_workspace_bytes": 0, "lattice_workspace_bytes": lattice_bytes(T, N, L)}
        if N <= hipops.MAX_SAMPLES:
            configs["lattice"] = (args.calls, lambda i: hipops.ctc_hyp_lattice(lps[i % args.copies], ls[i % args.copies][0],
                                                                               ls[i % args.copies][1], in_len, L))
            a = score(0).cpu().numpy()
            b = hipops.ctc_hyp_lattice(lps[0], ls[0][0], ls[0][1], in_len, L)[0].double().cpu().numpy()
            entry["finite_rows"] = int(np.isfinite(a).sum())
            entry["max_rel_dev_scorer_vs_lattice"] = float(np.nanmax(np.abs(a - b) / np.abs(a))) if np.isfinite(a).any() else None
            entry["lattice_workspace_bytes_allocated"] = hipops.ctc_hyp_workspace_bytes(T, B, V, N, L)
        entry["ms_per_call"] = measure(f"narrow V={V} N={N:3d}", configs)
        result["cases"][f"narrow_V{V}_N{N}"] = entry
        del ls
        hipops._ws_cache.clear()
        torch.cuda.empty_cache()
    del lps

    # ---- wide: V = 256 / 1024, ~300 units ----
    L = int(0.3 * T)
    mbr_sizes = tuple(int(x) for x in args.mbr_sizes.split(",") if x)
    for V in (int(x) for x in args.wide_vocabs.split(",")):
        lps = log_probs(V, 5.0)
        dec = CTCDecoder(list(range(V)), wide_search=True)
        for N in (int(x) for x in args.wide_sizes.split(",")):
            ls = lists(N, V, L)
            count = torch.full((B,), N, dtype=torch.int32, device=dev)
            configs = {
                "score": (args.calls, lambda i: hipops.ctc_hyp_score(lps[i % args.copies], ls[i % args.copies][0], ls[i % args.copies][1],
                                                                      in_len, L)),
                "composed": (args.composed_calls, lambda i: hipops._pair_distance_composed(ls[i % args.copies][0], ls[i % args.copies][1],
                                                                                           count, V, L, "char", None)),
            }
            entry = {"V": V, "N": N, "hypothesis_length": L, "pairs": B * N * (N - 1) // 2, "scorer_workspace_bytes": 0,
                     "lattice_workspace_bytes": lattice_bytes(T, N, L)}
            if N in mbr_sizes:
                configs["mbr_decode"] = (args.mbr_calls, lambda i: dec.mbr_decode(lps[i % args.copies], in_len, beam_size=N, nbest=N))
                md = dec.mbr_decode(lps[0], in_len, beam_size=N, nbest=N)
                entry["mbr_mean_hypothesis"] = round(float(md.nbest.lengths.float().mean().item()), 1)
            entry["ms_per_call"] = measure(f"wide   V={V} N={N:3d}", configs)
            result["cases"][f"wide_V{V}_N{N}"] = entry
            del ls
            torch.cuda.empty_cache()
        del lps
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000, help="T: frames per utterance")
    ap.add_argument("--narrow-sizes", default="16,64,128", help="list sizes N at V = 29, comma separated")
    ap.add_argument("--wide-sizes", default="16,128", help="list sizes N at the wide vocabularies")
    ap.add_argument("--wide-vocabs", default="256,1024")
    ap.add_argument("--mbr-sizes", default="16", help="list sizes at which the whole mbr_decode is timed too (empty: none)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--copies", type=int, default=3, help="copies of the inputs the calls rotate over")
    ap.add_argument("--calls", type=int, default=4, help="calls per timed window")
    ap.add_argument("--composed-calls", type=int, default=1, help="calls per timed window of the composed pair-distance path")
    ap.add_argument("--mbr-calls", type=int, default=1, help="calls per timed window of mbr_decode")
    ap.add_argument("--warm", type=int, default=2, help="warm-up calls per configuration")
    ap.add_argument("--limit", type=int, default=420, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker"]
    for k, v in vars(args).items():
        if k not in ("worker", "limit"):
            cmd += ["--" + k.replace("_", "-"), str(v)]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"hyp_score_cost.py: the measuring child ran past {args.limit} s and was killed; nothing else was started")
    sys.exit(rc)


if __name__ == "__main__":
    main()
