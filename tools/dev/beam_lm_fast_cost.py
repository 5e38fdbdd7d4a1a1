"""What language-model fusion costs in the single-wave CTC beam search (csrc/beam.hip, sb::beam_small_kernel<.., LM = true>; NOTES.md
0.17), and whether adding it left the no-LM kernel alone.  Headline shape: T = 1000, B = 32, V = 29, beam 16, fp32 log-probs; table
orders 3 (24 389 words) and 5 (20.5 M words, 82 MB: the gathers come from HBM).

  (a_nK) ctc_beam_search(lm=) on the workgroup-per-utterance kernel, order K;
  (b_nK) ctc_beam_search(lm=, fast_lm=True): the single-wave kernel with the LM term, order K;
  (c)    ctc_beam_search() -- the single-wave kernel without an LM -- of this tree's library and, with --parent-lib, of a library built
         from the PARENT commit (e.g. `git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/policy_gradient_asr_amd/csrc`): the
         same kernel text, so the two must agree within the run's own repeat-to-repeat spread.

The measurement runs in ONE child process under a time limit (--limit seconds; the parent never touches the GPU and starts nothing
after a child that failed or was killed).  In it every configuration is warmed up, then every repeat (--repeats 5) times --calls (20)
back-to-back calls of every configuration in turn between two device events, the order reversed every other repeat.  No bar is set:
(b) is reported against (a) and (c).  Then, with --steps > 0, the MWERTrainer step at nbest 4, beam 16 without an LM and with the table
of either order (tools/dev/mwer_cost.py's window: B = 32, T = 1000, F = 80, "f32", train mode, 20 steps per window).  One JSON line at the end.  Not imported by bench.py or the package."""
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
ORDERS = (3, 5)
ALPHA, BETA = 0.6, 0.8


def random_table(order, seed):
    """Per context a log-softmax over the non-blank symbols of 2 * N(0,1) logits, fp32; blank (0) column 0."""
    import numpy as np
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((V,) * order, dtype=np.float32) * np.float32(2.0)
    z[..., 0] = -np.inf
    m = z.max(axis=-1, keepdims=True)
    t = z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))
    t[..., 0] = 0.0
    return np.ascontiguousarray(t, dtype=np.float32)


def worker(args):
    import numpy as np
    import torch
    from policy_gradient_asr_amd import _lib, hipops
    from policy_gradient_asr_amd.lm import CharNgramLM
    if not torch.cuda.is_available():
        raise SystemExit("beam_lm_fast_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    libs = {"new": _lib.load()}
    if args.parent_lib:
        lib = C.CDLL(args.parent_lib)
        for name, (res, argtypes) in _lib.SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, argtypes
        assert lib.pgasr_abi_version() == 7 and not hasattr(lib, "pgasr_beam_lm_single_wave_ok"), "--parent-lib already has the single-wave LM"
        libs["parent"] = lib
    rng = np.random.default_rng(424247)
    logits = rng.normal(size=(T, B, V)) * 2.0
    m = logits.max(axis=-1, keepdims=True)
    lp = torch.from_numpy((logits - (m + np.log(np.exp(logits - m).sum(axis=-1, keepdims=True)))).astype(np.float32)).to(dev)
    lms = {k: CharNgramLM(random_table(k, 40 + k), k) for k in ORDERS}
    for lm in lms.values():
        lm.device_table(dev)
    configs = {}
    for k in ORDERS:
        assert hipops.beam_lm_single_wave_ok(T, V, BEAM, False, k)
        configs["a_workgroup_lm_n%d" % k] = ("new", lambda k=k: hipops.ctc_beam_search(lp, None, beam=BEAM, lm=lms[k], lm_alpha=ALPHA, lm_beta=BETA))
        configs["b_single_wave_lm_n%d" % k] = ("new", lambda k=k: hipops.ctc_beam_search(lp, None, beam=BEAM, lm=lms[k], lm_alpha=ALPHA,
                                                                                        lm_beta=BETA, fast_lm=True))
    configs["c_new_nolm"] = ("new", lambda: hipops.ctc_beam_search(lp, None, beam=BEAM))
    if "parent" in libs:
        configs["c_parent_nolm"] = ("parent", lambda: hipops.ctc_beam_search(lp, None, beam=BEAM))
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

    try:
        for name in names:
            window(name, args.warm)
        times = {name: [] for name in names}
        for r in range(args.repeats):
            for name in (names if r % 2 == 0 else names[::-1]):
                times[name].append(window(name, args.calls))
    finally:
        _lib._lib = libs["new"]
    agree = {}
    for k in ORDERS:
        a, b = configs["a_workgroup_lm_n%d" % k][1](), configs["b_single_wave_lm_n%d" % k][1]()
        agree["n%d" % k] = int((a[1] == b[1]).sum().item())          # utterances on which the two kernels return equally long hypotheses
    result = {"shape": {"T": T, "B": B, "V": V, "beam": BEAM}, "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "calls_per_window": args.calls, "equal_length_utterances_of_%d" % B: agree, "configs": {}}
    for name in names:
        v = times[name]
        e = result["configs"][name] = {"ms_per_call": [round(x, 4) for x in v], "median": round(statistics.median(v), 4),
                                       "min": round(min(v), 4), "max": round(max(v), 4)}
        print(f"{name:22s}: median {e['median']:.3f} ms  (min {e['min']:.3f}, max {e['max']:.3f})", flush=True)
    med = lambda n: result["configs"][n]["median"]
    for k in ORDERS:
        result["b_over_a_n%d" % k] = round(med("b_single_wave_lm_n%d" % k) / med("a_workgroup_lm_n%d" % k), 4)
        result["b_minus_c_ms_n%d" % k] = round(med("b_single_wave_lm_n%d" % k) - med("c_new_nolm"), 4)
    if "parent" in libs:
        cn, cp = result["configs"]["c_new_nolm"], result["configs"]["c_parent_nolm"]
        result["c_new_over_parent"] = round(cn["median"] / cp["median"], 4)
        result["c_spread_ms"] = {"new": round(cn["max"] - cn["min"], 4), "parent": round(cp["max"] - cp["min"], 4)}
        result["c_new_inside_spread_of_parent"] = bool(cp["min"] <= cn["median"] <= cp["max"])
    if args.steps > 0:
        # ---- the MWER step at nbest 4, beam 16 with and without the LM (tools/dev/mwer_cost.py's window: B = 32, T = 1000, F = 80, "f32", train mode) ----
        import bench
        from policy_gradient_asr_amd.model import Seq2Seq, weights
        from policy_gradient_asr_amd.mwer import MWERTrainer

        def trainer(**kw):
            torch.manual_seed(0)
            model = Seq2Seq(bench.V, n_feats=bench.F)
            model.apply(weights)
            return MWERTrainer(model.to(dev).train(), lr=5e-4, lam=1.0, seed=1234, precision="f32", nbest=4, beam_size=16, **kw)

        plain = trainer()
        fused = {k: trainer(lm=lms[k], lm_alpha=ALPHA, lm_beta=BETA) for k in ORDERS}
        batch = [t.to(dev) for t in bench.synth_batch(100)]
        configs = {"m_mwer": ("new", lambda: plain.step(*batch))}
        for k in ORDERS:
            configs["m_mwer_lm_n%d" % k] = ("new", lambda k=k: fused[k].step(*batch))
        names = list(configs)
        for name in names:
            window(name, args.warm)
        times = {name: [] for name in names}
        for r in range(args.repeats):
            for name in (names if r % 2 == 0 else names[::-1]):
                times[name].append(window(name, args.steps))
        hipops.lstm_assert_no_timeouts()
        step = result["mwer_step"] = {"steps_per_window": args.steps, "nbest": 4, "beam_size": 16, "configs": {}}
        for name in names:
            v = times[name]
            e = step["configs"][name] = {"ms_per_step": [round(x, 4) for x in v], "median": round(statistics.median(v), 4),
                                         "min": round(min(v), 4), "max": round(max(v), 4)}
            print(f"{name:22s}: median {e['median']:.3f} ms  (min {e['min']:.3f}, max {e['max']:.3f})", flush=True)
        for k in ORDERS:
            step["lm_minus_plain_ms_n%d" % k] = round(step["configs"]["m_mwer_lm_n%d" % k]["median"] - step["configs"]["m_mwer"]["median"], 4)
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libpgasr_hip.so built from the parent commit; without it (c) of the parent is not measured")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--steps", type=int, default=20, help="MWER train steps per timed window (0: the search only)")
    ap.add_argument("--warm", type=int, default=3, help="warm-up calls per configuration")
    ap.add_argument("--limit", type=int, default=400, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(args.repeats), "--calls", str(args.calls),
           "--steps", str(args.steps), "--warm", str(args.warm)] + (["--parent-lib", args.parent_lib] if args.parent_lib else [])
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"beam_lm_fast_cost.py: the measuring child ran past {args.limit} s and was killed; nothing else was started")
    sys.exit(rc)


if __name__ == "__main__":
    main()
