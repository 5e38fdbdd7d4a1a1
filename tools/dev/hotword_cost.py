"""What hotword biasing costs (csrc/beam.hip BIAS = true, csrc/hotword.hip; NOTES.md 0.38), and whether adding it left the kernels
without a bias alone.

First pass, headline shape T = 1000, B = 32, V = 29, beam 16, fp32 log-probs, for the 1-best and for N = 16:
  (u)    the workgroup-per-utterance search without a bias, of this tree's library and, with --parent-lib, of a library built from the
         PARENT commit (`git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/policy_gradient_asr_amd/csrc`): the same kernel
         text, so the two must agree within the run's own window-to-window spread, and their outputs are compared bit for bit;
  (lm)   the same search with a dense order-3 language model -- the yardstick: what one fused table gather per candidate costs;
  (bS)   the search with a bias automaton of S ~ 1e2, 1e4 and 1e5 states (random phrases of length 8: 20, 1500 and 15500 of them).
Second pass, B = 32, N = 16 and N = 128, rows of ~930 symbols over V = 29 and of ~300 units over V = 256:
  (s)    hipops.nbest_bias_score, beside the host loop of HotwordBias.score_sequence over the same N * B rows (one pass, wall clock).

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
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

T, B, V, BEAM, NBEST = 1000, 32, 29, 16, 16
STATES = ((100, 20), (10000, 1500), (100000, 15500))      # (about this many states, from this many random phrases of length 8)
ALPHA, BETA, GAMMA = 0.6, 0.8, 1.0


def worker(args):
    import numpy as np
    import torch
    from policy_gradient_asr_amd import _lib, hipops
    from policy_gradient_asr_amd.lm import CharNgramLM, HotwordBias
    if not torch.cuda.is_available():
        raise SystemExit("hotword_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    libs = {"new": _lib.load()}
    if args.parent_lib:
        lib = C.CDLL(args.parent_lib)
        for name, (res, argtypes) in _lib.SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, argtypes
        assert lib.pgasr_abi_version() == 7 and not hasattr(lib, "pgasr_ctc_beam_search_bias"), "--parent-lib already has the bias"
        libs["parent"] = lib
    rng = np.random.default_rng(424249)

    def log_probs():
        logits = rng.normal(size=(T, B, V)) * 2.0
        m = logits.max(axis=-1, keepdims=True)
        return torch.from_numpy((logits - (m + np.log(np.exp(logits - m).sum(axis=-1, keepdims=True)))).astype(np.float32)).to(dev)

    lps = [log_probs() for _ in range(args.inputs)]
    z = rng.standard_normal((V,) * 3, dtype=np.float32) * np.float32(2.0)
    z[..., 0] = -np.inf
    m = z.max(axis=-1, keepdims=True)
    tab = z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))
    tab[..., 0] = 0.0
    lm = CharNgramLM(np.ascontiguousarray(tab, dtype=np.float32), 3)
    lm.device_table(dev)
    biases = {}
    for about, n in STATES:
        hb = HotwordBias(rng.integers(1, V, size=(n, 8)).tolist(), V)
        hb.device_table(dev)
        biases[about] = hb
    turn = [0]

    def lp():
        turn[0] += 1
        return lps[turn[0] % len(lps)]

    configs = {
        "u_1best_new": ("new", lambda: hipops.ctc_beam_search(lp(), None, beam=BEAM, generic=True)),
        "u_nbest_new": ("new", lambda: hipops.ctc_beam_search_nbest(lp(), None, beam=BEAM, nbest=NBEST)),
        "lm_1best": ("new", lambda: hipops.ctc_beam_search(lp(), None, beam=BEAM, lm=lm, lm_alpha=ALPHA, lm_beta=BETA)),
        "lm_nbest": ("new", lambda: hipops.ctc_beam_search_nbest(lp(), None, beam=BEAM, nbest=NBEST, lm=lm, lm_alpha=ALPHA, lm_beta=BETA)),
    }
    if "parent" in libs:
        configs["u_1best_parent"] = ("parent", lambda: hipops.ctc_beam_search(lp(), None, beam=BEAM, generic=True))
        configs["u_nbest_parent"] = ("parent", lambda: hipops.ctc_beam_search_nbest(lp(), None, beam=BEAM, nbest=NBEST))
    for about, hb in biases.items():
        configs["b%d_1best" % about] = ("new", lambda hb=hb: hipops.ctc_beam_search(lp(), None, beam=BEAM, bias=hb, bias_weight=GAMMA))
        configs["b%d_nbest" % about] = ("new", lambda hb=hb: hipops.ctc_beam_search_nbest(lp(), None, beam=BEAM, nbest=NBEST, bias=hb,
                                                                                           bias_weight=GAMMA))
    configs["b10000_lm_1best"] = ("new", lambda: hipops.ctc_beam_search(lp(), None, beam=BEAM, lm=lm, lm_alpha=ALPHA, lm_beta=BETA,
                                                                      bias=biases[10000], bias_weight=GAMMA))
    # ---- second pass: lists of random rows with phrases of the automaton planted in them ----
    second = {}
    for name, v2, length in (("chars930", 29, 930), ("units300", 256, 300)):
        hb = HotwordBias(rng.integers(1, v2, size=(1500, 6)).tolist(), v2)
        hb.device_table(dev)
        for n in (16, 128):
            stride = length + 70
            sets = []
            for _ in range(args.inputs):
                tok = rng.integers(1, v2, size=(n, B, stride)).astype(np.int32)
                ln = rng.integers(length - 60, length + 60, size=(n, B)).astype(np.int32)
                for p in range(0, length - 10, 37):
                    tok[:, :, p:p + 6] = np.asarray(hb.phrases[int(rng.integers(len(hb.phrases)))], dtype=np.int32)
                sets.append((tok, ln, torch.from_numpy(tok).to(dev), torch.from_numpy(ln).to(dev)))
            cnt = torch.full((B,), n, dtype=torch.int32, device=dev)
            key = "s_%s_n%d" % (name, n)
            second[key] = (hb, sets, cnt)

            def call(hb=hb, sets=sets, cnt=cnt):
                turn[0] += 1
                s = sets[turn[0] % len(sets)]
                return hipops.nbest_bias_score(s[2], s[3], cnt, hb)
            configs[key] = ("new", call)
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
            for kind, fn in (("1best", lambda x: hipops.ctc_beam_search(x, None, beam=BEAM, generic=True)),
                             ("nbest", lambda x: hipops.ctc_beam_search_nbest(x, None, beam=BEAM, nbest=NBEST))):
                ok = True
                for x in lps:
                    _lib._lib = libs["new"]
                    a = fn(x)
                    _lib._lib = libs["parent"]
                    b = fn(x)
                    ok = ok and all(torch.equal(p, q) for p, q in zip(a, b))
                equal[kind] = bool(ok)
    finally:
        _lib._lib = libs["new"]
    result = {"shape": {"T": T, "B": B, "V": V, "beam": BEAM, "nbest": NBEST}, "device": torch.cuda.get_device_name(0),
              "repeats": args.repeats, "calls_per_window": args.calls, "inputs": args.inputs,
              "states": {str(k): hb.n_states for k, hb in biases.items()}, "configs": {}}
    for name in names:
        v = times[name]
        e = result["configs"][name] = {"ms_per_call": [round(x, 4) for x in v], "median": round(statistics.median(v), 4),
                                       "min": round(min(v), 4), "max": round(max(v), 4)}
        print(f"{name:22s}: median {e['median']:.3f} ms  (min {e['min']:.3f}, max {e['max']:.3f})", flush=True)
    med = lambda n: result["configs"][n]["median"]
    for kind in ("1best", "nbest"):
        u = med("u_%s_new" % kind)
        result["lm_minus_u_ms_" + kind] = round(med("lm_" + kind) - u, 4)
        for about in biases:
            result["b%d_minus_u_ms_%s" % (about, kind)] = round(med("b%d_%s" % (about, kind)) - u, 4)
        if "parent" in libs:
            cn, cp = result["configs"]["u_%s_new" % kind], result["configs"]["u_%s_parent" % kind]
            result["u_%s_new_over_parent" % kind] = round(cn["median"] / cp["median"], 4)
            result["u_%s_new_inside_spread_of_parent" % kind] = bool(cp["min"] <= cn["median"] <= cp["max"])
    if equal:
        result["unbiased_bit_equal_to_parent"] = equal
    # ---- the host loop beside the second pass: one pass over the first input set of each configuration ----
    host = result["host_score_sequence_ms"] = {}
    for key, (hb, sets, cnt) in second.items():
        tok, ln = sets[0][0], sets[0][1]
        rows = [tok[n, b, :ln[n, b]].tolist() for n in range(tok.shape[0]) for b in range(B)]
        t0 = time.perf_counter()
        want = [hb.score_sequence(y) for y in rows]
        host[key] = round((time.perf_counter() - t0) * 1e3, 2)
        got = hipops.nbest_bias_score(sets[0][2], sets[0][3], cnt, hb).cpu().numpy().reshape(-1)
        assert list(got) == want, key
        print(f"{key:22s}: host loop {host[key]:.1f} ms for {len(rows)} rows, device equal", flush=True)
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
        raise SystemExit(f"hotword_cost.py: the measuring child ran past {args.limit} s and was killed; nothing else was started")
    sys.exit(rc)


if __name__ == "__main__":
    main()
