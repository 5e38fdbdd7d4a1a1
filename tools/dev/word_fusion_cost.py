"""What fusing the word n-gram model and its lexicon into the first pass costs (csrc/beam.hip WORDS = true; NOTES.md 0.43), and whether
adding it left the kernels without it alone.

Headline shape T = 1000, B = 32, V = 29, beam 16, fp32 log-probs whose frames follow sentences of lexicon words, for N = 1 and N = 16:
  (u)    the workgroup-per-utterance N-best search without a model, of this tree's library and, with --parent-lib, of a library built
         from the PARENT commit (`git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/policy_gradient_asr_amd/csrc`): the same
         kernel text, so the two must agree within the run's own window-to-window spread, and their outputs are compared bit for bit;
  (lm)   the same search with a dense order-3 character model -- the yardstick: one fused table gather per candidate;
  (wK)   ``hipops.ctc_beam_search_words`` with a word model of order K = 3 and 5 over ~1e5 words (random spellings of 2 .. 7 letters,
         1e5 random n-grams per order above the unigrams), finalize and eos on.

The measurement runs in ONE child process under a time limit (--limit seconds; the parent process never touches the GPU and starts
nothing after a child that failed or was killed).  In it every configuration is warmed up, then every repeat (--repeats 5) times
--calls back-to-back calls of every configuration in turn between two device events, the order reversed every other repeat and the
inputs rotated over --inputs (4) different batches call by call.  No bar is set.  One JSON line at the end.  Not imported by bench.py
or the package."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

T, B, V, BEAM = 1000, 32, 29, 16
NBESTS = (1, 16)
ORDERS = (3, 5)
N_WORDS, N_GRAMS = 100000, 100000
DELIM = 28
ALPHA, BETA, OOV = 0.5, 2.0, -3.0
LM_ALPHA, LM_BETA = 0.6, 0.8


def random_word_lm(rng, order):
    """A ``lm.WordNgramLM`` over N_WORDS random spellings with N_GRAMS random n-grams per order above the unigrams, every context
    stored; log-probabilities and back-off weights are random (the cost does not depend on their values)."""
    import numpy as np
    from policy_gradient_asr_amd.lm import EOS, UNK, BOS, WordNgramLM
    words = set()
    while len(words) < N_WORDS:
        for row, n in zip(rng.integers(1, DELIM, size=(N_WORDS, 7)), rng.integers(2, 8, size=N_WORDS)):
            words.add(bytes(row[:n].tolist()))
    words = sorted(words)[:N_WORDS]
    val = lambda: (float(-rng.uniform(1.0, 12.0)), float(-rng.uniform(0.0, 2.0)))
    grams = [{(w,): val() for w in words}]
    grams[0].update({(BOS,): (-99.0 * 2.302585092994046, -0.5), (EOS,): val(), (UNK,): val()})
    prev = [(w,) for w in words] + [(BOS,), (UNK,)]
    for k in range(2, order + 1):
        cur = {}
        starts = [p for p in prev if k == 2 or BOS not in p[1:]]
        for i in rng.integers(0, len(starts), size=N_GRAMS):
            w = words[int(rng.integers(len(words)))] if rng.random() < 0.95 else EOS
            cur[starts[int(i)] + (w,)] = val()
        grams.append(cur)
        prev = [g for g in cur if g[-1] != EOS]
    return WordNgramLM._build(grams, order, 0, DELIM), [tuple(w) for w in words]


def worker(args):
    import numpy as np
    import torch
    from policy_gradient_asr_amd import _lib, hipops
    from policy_gradient_asr_amd.lm import CharNgramLM, WordFusion
    if not torch.cuda.is_available():
        raise SystemExit("word_fusion_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    libs = {"new": _lib.load()}
    if args.parent_lib:
        lib = C.CDLL(args.parent_lib)
        for name, (res, argtypes) in _lib.SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, argtypes
        assert lib.pgasr_abi_version() == 7 and not hasattr(lib, "pgasr_ctc_beam_search_words"), "--parent-lib already has the word fusion"
        libs["parent"] = lib
    rng = np.random.default_rng(424251)
    fusions = {}
    for order in ORDERS:
        lm, words = random_word_lm(rng, order)
        f = fusions[order] = WordFusion(lm, V, DELIM, blank=0, oov_penalty=OOV)
        f.device_tables(dev)
        print(f"order {order}: {lm.n_words} words, {sum(g.shape[0] for g in lm.ngrams)} n-grams, {f.n_states} trie states", flush=True)

    def log_probs():      # noise under sentences of lexicon words, a token every 1 .. 3 frames
        logits = rng.normal(size=(T, B, V)) * 2.0
        logits[:, :, 0] += 2.0
        for b in range(B):
            t = 0
            while t < T:
                for tok in words[int(rng.integers(len(words)))] + (DELIM,):
                    if t < T:
                        logits[t, b, tok] += 5.0
                    t += int(rng.integers(1, 4))
        m = logits.max(axis=-1, keepdims=True)
        return torch.from_numpy((logits - (m + np.log(np.exp(logits - m).sum(axis=-1, keepdims=True)))).astype(np.float32)).to(dev)

    lps = [log_probs() for _ in range(args.inputs)]
    z = rng.standard_normal((V,) * 3, dtype=np.float32) * np.float32(2.0)
    z[..., 0] = -np.inf
    m = z.max(axis=-1, keepdims=True)
    tab = z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))
    tab[..., 0] = 0.0
    lm3 = CharNgramLM(np.ascontiguousarray(tab, dtype=np.float32), 3)
    lm3.device_table(dev)
    turn = [0]

    def lp():
        turn[0] += 1
        return lps[turn[0] % len(lps)]

    configs = {}
    for n in NBESTS:
        configs["u_n%d_new" % n] = ("new", lambda n=n: hipops.ctc_beam_search_nbest(lp(), None, beam=BEAM, nbest=n))
        if "parent" in libs:
            configs["u_n%d_parent" % n] = ("parent", lambda n=n: hipops.ctc_beam_search_nbest(lp(), None, beam=BEAM, nbest=n))
        configs["lm_n%d" % n] = ("new", lambda n=n: hipops.ctc_beam_search_nbest(lp(), None, beam=BEAM, nbest=n, lm=lm3, lm_alpha=LM_ALPHA,
                                                                                 lm_beta=LM_BETA))
        for order in ORDERS:
            configs["w%d_n%d" % (order, n)] = ("new", lambda n=n, f=fusions[order]: hipops.ctc_beam_search_words(
                lp(), None, beam=BEAM, nbest=n, fusion=f, alpha=ALPHA, beta=BETA))
    names = list(configs)

    def window(name, calls):
        lib, fn = configs[name]
        _lib._lib = libs[lib]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls          # ms per call

    equal = {}
    try:
        for name in names:
            window(name, args.warm)
        times = {name: [] for name in names}
        for r in range(args.repeats):
            for name in (names if r % 2 == 0 else names[::-1]):
                times[name].append(window(name, args.calls))
        if "parent" in libs:      # bit-equality of the call without a model, this library against the parent's, on every input
            for n in NBESTS:
                ok = True
                for x in lps:
                    _lib._lib = libs["new"]
                    a = hipops.ctc_beam_search_nbest(x, None, beam=BEAM, nbest=n)
                    _lib._lib = libs["parent"]
                    b = hipops.ctc_beam_search_nbest(x, None, beam=BEAM, nbest=n)
                    ok = ok and all(torch.equal(p, q) for p, q in zip(a, b))
                equal["n%d" % n] = bool(ok)
    finally:
        _lib._lib = libs["new"]
    nb = hipops.ctc_beam_search_words(lps[0], None, beam=BEAM, nbest=1, fusion=fusions[ORDERS[0]], alpha=ALPHA, beta=BETA)
    rows = [nb.tokens[0, b, :nb.lengths[0, b]].tolist() for b in range(B)]
    result = {"shape": {"T": T, "B": B, "V": V, "beam": BEAM}, "device": torch.cuda.get_device_name(0),
              "repeats": args.repeats, "calls_per_window": args.calls, "inputs": args.inputs,
              "trie_states": {str(k): f.n_states for k, f in fusions.items()},
              "words_per_best_row": round(sum(r.count(DELIM) for r in rows) / B, 1), "configs": {}}
    for name in names:
        v = times[name]
        e = result["configs"][name] = {"ms_per_call": [round(x, 4) for x in v], "median": round(statistics.median(v), 4),
                                       "min": round(min(v), 4), "max": round(max(v), 4)}
        print(f"{name:16s}: median {e['median']:.3f} ms  (min {e['min']:.3f}, max {e['max']:.3f})", flush=True)
    med = lambda n: result["configs"][n]["median"]
    for n in NBESTS:
        u = med("u_n%d_new" % n)
        result["lm_minus_u_ms_n%d" % n] = round(med("lm_n%d" % n) - u, 4)
        for order in ORDERS:
            result["w%d_minus_u_ms_n%d" % (order, n)] = round(med("w%d_n%d" % (order, n)) - u, 4)
        if "parent" in libs:
            cn, cp = result["configs"]["u_n%d_new" % n], result["configs"]["u_n%d_parent" % n]
            result["u_n%d_new_over_parent" % n] = round(cn["median"] / cp["median"], 4)
            result["u_n%d_new_inside_spread_of_parent" % n] = bool(cp["min"] <= cn["median"] <= cp["max"])
    if equal:
        result["unfused_bit_equal_to_parent"] = equal
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libpgasr_hip.so built from the parent commit; without it the parent is not measured")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=8, help="calls per timed window")
    ap.add_argument("--warm", type=int, default=2, help="warm-up calls per configuration")
    ap.add_argument("--inputs", type=int, default=4, help="different input batches, rotated call by call")
    ap.add_argument("--limit", type=int, default=400, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(args.repeats), "--calls", str(args.calls),
           "--warm", str(args.warm), "--inputs", str(args.inputs)] + (["--parent-lib", args.parent_lib] if args.parent_lib else [])
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"word_fusion_cost.py: the measuring child ran past {args.limit} s and was killed; nothing else was started")
    sys.exit(rc)


if __name__ == "__main__":
    main()
