"""What a word n-gram LM adds to second-pass rescoring (csrc/word_lm.hip; NOTES.md 0.23).  Headline shape: B = 32, V = 29, lists of
N in {16, 128} (--sizes) hypotheses of ~930 symbols (T = 1000 frames) in rows of 1000 tokens; models of order 3 and 5 (--orders)
with 10^5 words and ~10^6 n-grams (--words, --ngrams), synthetic: random spellings, a Zipf stream of words whose windows of every
order are the stored n-grams (so every context is stored), random logp / bow.  The hypotheses are stretches of that stream with one
word in ten replaced by a random word and one in fifty by a string outside the vocabulary, so the back-off rule is walked at
every depth.  Per (order, N), four times:

  (score)    pgasr_nbest_word_lm_score on the list;
  (combine)  pgasr_nbest_combine_rank on its outputs;
  (rescore)  the existing pgasr_nbest_rescore on the same list with an order-3 character table -- for scale;
  (host)     the loop a user would otherwise run: the list copied to the host and ``WordNgramLM.logp_sentence`` per hypothesis
             (one pass, wall clock).

The measurement runs in ONE child process under a time limit (--limit seconds; the parent never touches the GPU and starts nothing
after a child that failed or was killed).  In it every device configuration is warmed up, then every repeat (--repeats 5) times a
window of back-to-back calls (--calls 20) between two device events, the calls rotating over three copies of the list, the order
reversed every other repeat; the median of the windows is reported, and that device and host agree bit for bit.  One JSON line at
the end.  Not imported by bench.py or the package."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

B, V, STRIDE, DELIM = 32, 29, 1000, 1


def synthetic_model(np, order, n_words, n_ngrams, rng):
    from policy_gradient_asr_amd.lm import N_RESERVED, WordNgramLM
    spell = set()
    while len(spell) < n_words:
        k = int(rng.integers(2, 11))
        spell.add(bytes(rng.integers(2, V, size=k).astype(np.uint8)))
    spell = sorted(spell)
    off = np.zeros(N_RESERVED + n_words + 1, dtype=np.int64)
    off[N_RESERVED + 1:] = np.cumsum([len(s) for s in spell])
    pool = np.frombuffer(b"".join(spell), dtype=np.uint8)
    total = N_RESERVED + n_words
    S = max(order, (n_ngrams - total) // max(order - 1, 1))
    p = 1.0 / np.arange(1, n_words + 1)
    stream = (N_RESERVED + rng.permutation(n_words)[rng.choice(n_words, size=S, p=p / p.sum())]).astype(np.int32)
    ngrams = [np.arange(total, dtype=np.int32)[:, None]]
    for k in range(2, order + 1):
        ngrams.append(np.unique(np.lib.stride_tricks.sliding_window_view(stream, k), axis=0).astype(np.int32))
    logp = [(-rng.uniform(0.1, 12.0, size=g.shape[0])).astype(np.float32) for g in ngrams]
    bow = [(-rng.uniform(0.0, 3.0, size=g.shape[0])).astype(np.float32) for g in ngrams]
    return WordNgramLM(pool, off, ngrams, logp, bow, blank=0, delimiter=DELIM), stream


def hypotheses(np, lm, stream, N, rng):
    tokens = np.zeros((N, B, STRIDE), dtype=np.int32)
    lengths = np.zeros((N, B), dtype=np.int32)
    for n in range(N):
        for b in range(B):
            at = int(rng.integers(0, max(1, stream.size - 400)))
            row = []
            for w in stream[at:at + 400]:
                r = rng.random()
                if r < 0.02:
                    s = bytes(rng.integers(2, V, size=12).astype(np.uint8))
                elif r < 0.12:
                    s = lm.spellings[int(rng.integers(3, lm.n_words))]
                else:
                    s = lm.spellings[int(w)]
                if len(row) + len(s) + 1 > 930:
                    break
                row += list(s) + [DELIM]
            tokens[n, b, :len(row) - 1] = row[:-1]
            lengths[n, b] = len(row) - 1
    return tokens, lengths


def worker(args):
    import numpy as np
    import torch
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.lm import CharNgramLM
    if not torch.cuda.is_available():
        raise SystemExit("word_lm_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(424247)
    char_lm = CharNgramLM(np.log(rng.dirichlet(np.ones(V), size=(V, V))).astype(np.float32), 3)
    result = {"shape": {"B": B, "V": V, "stride": STRIDE}, "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "calls_per_window": args.calls, "runs": {}}
    for order in (int(x) for x in args.orders.split(",")):
        t0 = time.perf_counter()
        lm, stream = synthetic_model(np, order, args.words, args.ngrams, rng)
        lm.device_tables(dev)
        built = time.perf_counter() - t0
        for N in (int(x) for x in args.sizes.split(",")):
            tokens, lengths = hypotheses(np, lm, stream, N, rng)
            copies = [(torch.from_numpy(tokens).to(dev), torch.from_numpy(lengths).to(dev)) for _ in range(3)]
            count = torch.full((B,), N, dtype=torch.int32, device=dev)
            am = torch.from_numpy(rng.uniform(50.0, 90.0, size=(N, B))).to(dev)
            word_logp, n_words, n_oov = hipops.nbest_word_lm_score(copies[0][0], copies[0][1], count, lm, DELIM)
            turn = [0]

            def rotated():
                turn[0] = (turn[0] + 1) % 3
                return copies[turn[0]]

            configs = {
                "score": lambda: hipops.nbest_word_lm_score(*rotated(), count, lm, DELIM),
                "combine": lambda: hipops.nbest_combine_rank(am, word_logp, n_words, count, word_alpha=0.5, word_beta=0.5),
                "rescore": lambda: hipops.nbest_rescore(*rotated(), count, am, V, lm=char_lm, lm_alpha=0.5, lm_beta=0.5),
            }
            names = list(configs)

            def window(name, calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    configs[name]()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / calls          # ms per call

            for name in names:
                window(name, args.warm)
            times = {name: [] for name in names}
            for r in range(args.repeats):
                for name in (names if r % 2 == 0 else names[::-1]):
                    times[name].append(window(name, args.calls))
            lm.logp_sentence([])                            # the host's dict of n-grams is made on the first query: not timed
            t0 = time.perf_counter()
            tk, ln = copies[0][0].cpu().numpy(), copies[0][1].cpu().numpy()
            host = [[lm.logp_sentence(tk[n, b, :ln[n, b]]) for b in range(B)] for n in range(N)]
            host_ms = (time.perf_counter() - t0) * 1e3
            got = (word_logp.cpu().numpy(), n_words.cpu().numpy(), n_oov.cpu().numpy())
            agree = all(host[n][b] == (got[0][n, b], got[1][n, b], got[2][n, b]) for n in range(N) for b in range(B))
            entry = result["runs"]["order%d-N%d" % (order, N)] = {
                "words": lm.n_words, "ngrams": int(sum(g.shape[0] for g in lm.ngrams)), "model_build_s": round(built, 1),
                "hypotheses": N * B, "mean_symbols": round(float(ln.mean()), 1), "mean_words": round(float(got[1].mean()), 1),
                "oov_share": round(float(got[2].sum() / max(got[1].sum(), 1)), 4), "device_equals_host": bool(agree),
                "host_loop_ms": round(host_ms, 1), "ms_per_call": {}}
            for name in names:
                v = times[name]
                entry["ms_per_call"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                print(f"order {order} N={N:3d} {name:8s}: median {statistics.median(v):.4f} ms  (min {min(v):.4f}, max {max(v):.4f})",
                      flush=True)
            print(f"order {order} N={N:3d} host loop: {host_ms:.1f} ms, equal to the device: {agree}", flush=True)
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--orders", default="3,5", help="model orders, comma separated")
    ap.add_argument("--sizes", default="16,128", help="list sizes N, comma separated")
    ap.add_argument("--words", type=int, default=100000)
    ap.add_argument("--ngrams", type=int, default=1000000, help="stored n-grams of all orders (approximately)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--warm", type=int, default=3, help="warm-up calls per configuration")
    ap.add_argument("--limit", type=int, default=420, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--orders", args.orders, "--sizes", args.sizes, "--words", str(args.words),
           "--ngrams", str(args.ngrams), "--repeats", str(args.repeats), "--calls", str(args.calls), "--warm", str(args.warm)]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"word_lm_cost.py: the measuring child ran past {args.limit} s and was killed; nothing else was started")
    sys.exit(rc)


if __name__ == "__main__":
    main()
