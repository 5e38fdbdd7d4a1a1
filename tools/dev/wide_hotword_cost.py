"""What hotword biasing inside the wide beam search costs (csrc/beam_wide.hip with a WideBias; NOTES.md 0.39), and whether adding it
left the search without a bias alone.  Shape: T = 1000, B = 32, beam 16, fp32 log-probs, blank 0; rows are PEAKED (logits 5 N(0,1)) or
FLAT (logits 0.3 N(0,1)) as in beam_wide_cost.py / unit_lm_cost.py; V = 128 / 256 / 1024.

  (w)    ctc_beam_search_wide without a bias, 1-best, of this tree's library and, with --parent-lib, of a library built from the
         PARENT commit in the same process and in neighbouring windows: the same kernel text, so the two must agree within the
         parent's own window-to-window spread, and their outputs are compared bit for bit on every input;
  (bS)   the search with a bias automaton of S ~ 150 and S >= 12000 states (25 and 2100 random phrases of length 7, weight 1), at
         1-best and at N = 16;
  (lm)   the search with a unit LM of order 3 (estimated as in unit_lm_cost.py from --sentences random unit sequences) -- the
         yardstick, NOTES.md 0.29 -- and (lmb) the LM and the large automaton together.
The share of frames that took the counting selection is reported for every configuration.

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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

T, B, BEAM, NBEST = 1000, 32, 16, 16
WIDTHS = (128, 256, 1024)
ROWS = {"peaked": 5.0, "flat": 0.3}
PHRASES = ((150, 25), (12000, 2100))      # (about / at least this many states, from this many random phrases of length 7)
ORDER, ALPHA, BETA, GAMMA = 3, 0.5, 0.5, 1.0


def worker(args):
    import numpy as np
    import torch
    from policy_gradient_asr_amd import _lib, hipops
    from policy_gradient_asr_amd.lm import HotwordBias, UnitNgramLM
    from unit_lm_cost import sentences
    if not torch.cuda.is_available():
        raise SystemExit("wide_hotword_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    libs = {"new": _lib.load()}
    if args.parent_lib:
        lib = C.CDLL(args.parent_lib)
        for name, (res, argtypes) in _lib.SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, argtypes
        assert lib.pgasr_abi_version() == 7 and not hasattr(lib, "pgasr_ctc_beam_search_wide_bias"), "--parent-lib already has the wide bias"
        libs["parent"] = lib
    rng = np.random.default_rng(424251)

    def rows(V, kind):
        logits = rng.normal(size=(T, B, V)) * ROWS[kind]
        m = logits.max(axis=-1, keepdims=True)
        return torch.from_numpy((logits - (m + np.log(np.exp(logits - m).sum(axis=-1, keepdims=True)))).astype(np.float32)).to(dev)

    turn = [0]
    configs, inputs, states, share = {}, {}, {}, {}
    for V in WIDTHS:
        lm = UnitNgramLM.from_transcripts(sentences(V, args.sentences, 7 + V), V, order=ORDER)
        lm.device_tables(dev)
        biases = {}
        for about, n in PHRASES:
            hb = HotwordBias(rng.integers(1, V, size=(n, 7)).tolist(), V)
            hb.device_table(dev)
            biases[about] = hb
            states[f"V{V}_b{about}"] = hb.n_states
        assert biases[12000].n_states >= 12000
        print(f"V={V}: LM of {lm.n_ngrams} n-grams, automata of {[hb.n_states for hb in biases.values()]} states", flush=True)
        for kind in ROWS:
            lps = inputs[V, kind] = [rows(V, kind) for _ in range(args.inputs)]

            def lp(lps=lps):
                turn[0] += 1
                return lps[turn[0] % len(lps)]
            tag = f"V{V}_{kind}"
            lmkw = dict(unit_lm=lm, lm_alpha=ALPHA, lm_beta=BETA)
            calls = {"w": {}, "lm": lmkw, "lmb12000": dict(lmkw, bias=biases[12000], bias_weight=GAMMA)}
            for about, hb in biases.items():
                calls[f"b{about}"] = dict(bias=hb, bias_weight=GAMMA)
                calls[f"b{about}_n{NBEST}"] = dict(bias=hb, bias_weight=GAMMA, nbest=NBEST)
            if "parent" in libs:
                configs[f"w_parent_{tag}"] = ("parent", lambda lp=lp: hipops.ctc_beam_search_wide(lp(), None, beam=BEAM, nbest=1))
            for name, kw in calls.items():
                kw = dict(dict(beam=BEAM, nbest=1), **kw)
                configs[f"{name}_{tag}"] = ("new", lambda lp=lp, kw=kw: hipops.ctc_beam_search_wide(lp(), None, **kw))
                _, frames = hipops.ctc_beam_search_wide(lps[0], None, stats=True, **kw)
                share[f"{name}_{tag}"] = round(float(frames.sum()) / (T * B), 5)
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
        if "parent" in libs:      # bit-equality of the call without a bias, this library against the parent's, on every input
            for (V, kind), lps in inputs.items():
                ok = True
                for x in lps:
                    _lib._lib = libs["new"]
                    a = hipops.ctc_beam_search_wide(x, None, beam=BEAM, nbest=NBEST)
                    _lib._lib = libs["parent"]
                    b = hipops.ctc_beam_search_wide(x, None, beam=BEAM, nbest=NBEST)
                    ok = ok and all(torch.equal(p, q) for p, q in zip(a[:2] + (a.count,), b[:2] + (b.count,)))
                    ok = ok and torch.equal(a.score.view(torch.int64), b.score.view(torch.int64))
                equal[f"V{V}_{kind}"] = bool(ok)
    finally:
        _lib._lib = libs["new"]
    result = {"shape": {"T": T, "B": B, "beam": BEAM, "nbest": NBEST, "order": ORDER, "alpha": ALPHA, "beta": BETA, "gamma": GAMMA},
              "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "calls_per_window": args.calls, "inputs": args.inputs,
              "sentences": args.sentences, "states": states, "counting_share": share, "configs": {}, "ratios": {}}
    for name in names:
        v = times[name]
        e = result["configs"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        print(f"{name:28s}: median {e['median']:.3f} ms  (min {e['min']:.3f}, max {e['max']:.3f})", flush=True)
    med = lambda n: result["configs"][n]["median"]
    for V in WIDTHS:
        for kind in ROWS:
            tag = f"V{V}_{kind}"
            r = result["ratios"][tag] = {n: round(med(f"{n}_{tag}") / med(f"w_{tag}"), 4)
                                         for n in ("lm", "lmb12000", "b150", "b12000", f"b150_n{NBEST}", f"b12000_n{NBEST}")}
            if "parent" in libs:
                cn, cp = result["configs"][f"w_{tag}"], result["configs"][f"w_parent_{tag}"]
                r["w_over_parent"] = round(cn["median"] / cp["median"], 4)
                r["w_inside_spread_of_parent"] = bool(cp["min"] <= cn["median"] <= cp["max"])
            print(tag, r, flush=True)
    if equal:
        result["unbiased_bit_equal_to_parent"] = equal
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libpgasr_hip.so built from the parent commit; without it the parent is not measured")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed window")
    ap.add_argument("--warm", type=int, default=1, help="warm-up calls per configuration")
    ap.add_argument("--inputs", type=int, default=4, help="different input batches, rotated call by call")
    ap.add_argument("--sentences", type=int, default=5000, help="random unit sequences the LM is estimated from")
    ap.add_argument("--limit", type=int, default=540, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(args.repeats), "--calls", str(args.calls),
           "--warm", str(args.warm), "--inputs", str(args.inputs), "--sentences", str(args.sentences)] \
        + (["--parent-lib", os.path.abspath(args.parent_lib)] if args.parent_lib else [])
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"wide_hotword_cost.py: the measuring child ran past {args.limit} s and was killed; nothing else was started")
    sys.exit(rc)


if __name__ == "__main__":
    main()
