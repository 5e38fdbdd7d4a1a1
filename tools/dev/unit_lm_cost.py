"""What the back-off unit n-gram LM costs (lm.UnitNgramLM; csrc/beam_wide.hip with a model, csrc/unit_lm.hip; NOTES.md 0.29).  Shape:
T = 1000, B = 32, beam 16, fp32 log-probs, blank 0; rows are PEAKED (logits 5 N(0,1)) or FLAT (logits 0.3 N(0,1)) as in
beam_wide_cost.py; V = 128 / 256 / 1024; models of order 3 and 5 estimated (Witten-Bell, ``from_transcripts``) from --sentences random
unit sequences of 20 .. 60 units -- Zipf-distributed units, every other one drawn from a fixed successor table of its predecessor, so
that n-grams repeat as they do in text; the number of stored n-grams is reported.

  (f)  ctc_beam_search_wide(unit_lm=, lm_alpha=0.5, lm_beta=0.5), N = 1, beside (w) the call without a model on the same inputs, with
       the share of frames that took the counting selection in each;
  (p)  with --parent-lib PATH (a libpgasr_hip.so built from the parent commit): pgasr_ctc_beam_search_wide of THAT library on the same
       inputs, in the same process and the same interleaved windows as (w), so the two differ by the library alone;
  (s)  nbest_unit_lm_score at N = 16 and N = 128 (lists of B x N random sequences of 100 .. 300 units, order 5, V = 1024), beside the
       host loop of ``logp_sequence`` over the same lists (wall clock, once).

The measurement runs in ONE child process under a time limit (--limit seconds; the parent never touches the GPU and starts nothing
after a child that failed or was killed).  Every configuration is warmed up, then every repeat (--repeats 5) times --calls (3)
back-to-back calls of every configuration in turn between two device events, the order reversed every other repeat; medians of
the windows are reported.  No bar is set.  One JSON line at the end.  Not imported by bench.py or the package."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

T, B, BEAM = 1000, 32, 16
WIDTHS = (128, 256, 1024)
ORDERS = (3, 5)
ROWS = {"peaked": 5.0, "flat": 0.3}
ALPHA, BETA = 0.5, 0.5


def sentences(V, n, seed, lo=20, hi=60):
    import numpy as np
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, V)
    p /= p.sum()
    follow = rng.choice(np.arange(1, V), size=V, p=p)
    out = []
    for _ in range(n):
        y = rng.choice(np.arange(1, V), size=int(rng.integers(lo, hi + 1)), p=p)
        tied = rng.random(y.size) < 0.5
        for i in range(1, y.size):
            if tied[i]:
                y[i] = follow[y[i - 1]]
        out.append(y.tolist())
    return out


def worker(args):
    import numpy as np
    import torch
    from policy_gradient_asr_amd import hipops
    from policy_gradient_asr_amd.lm import UnitNgramLM
    if not torch.cuda.is_available():
        raise SystemExit("unit_lm_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        parent.pgasr_beam_wide_workspace_bytes.restype = ctypes.c_size_t
        parent.pgasr_ctc_beam_search_wide.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p] \
            + [ctypes.c_int] * 7 + [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_void_p]

    def rows(V, kind):
        rng = np.random.default_rng(424245 + V)
        logits = rng.normal(size=(T, B, V)) * ROWS[kind]
        m = logits.max(axis=-1, keepdims=True)
        return torch.from_numpy((logits - (m + np.log(np.exp(logits - m).sum(axis=-1, keepdims=True)))).astype(np.float32)).to(dev)

    def parent_call(lp, V):
        ws = torch.empty(parent.pgasr_beam_wide_workspace_bytes(T, B, V, BEAM), dtype=torch.uint8, device=dev)
        tok = torch.empty(1, B, T, dtype=torch.int32, device=dev)
        ln, cnt = torch.empty(1, B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        sc = torch.empty(1, B, dtype=torch.float64, device=dev)

        def call():
            st = parent.pgasr_ctc_beam_search_wide(lp.data_ptr(), 0, lp.stride(0), lp.stride(1), None, T, B, V, BEAM, 0, 0, 1, tok.data_ptr(), T,
                                                   ln.data_ptr(), sc.data_ptr(), cnt.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                                   torch.cuda.current_stream().cuda_stream)
            assert st == 0, st
            return tok, ln, sc
        return call

    models, built = {}, {}
    for V in WIDTHS:
        sents = sentences(V, args.sentences, 7 + V)
        for order in ORDERS:
            t0 = time.perf_counter()
            models[V, order] = UnitNgramLM.from_transcripts(sents, V, order=order)
            models[V, order].device_tables(dev)
            built[f"V{V}_n{order}"] = {"ngrams": models[V, order].n_ngrams, "build_s": round(time.perf_counter() - t0, 2)}
            print(f"model V={V} order={order}: {built[f'V{V}_n{order}']}", flush=True)
    configs, share = {}, {}
    for kind in ROWS:
        for V in WIDTHS:
            lp = rows(V, kind)
            configs[f"w_V{V}_{kind}"] = lambda lp=lp: hipops.ctc_beam_search_wide(lp, None, beam=BEAM, nbest=1)
            _, frames = hipops.ctc_beam_search_wide(lp, None, beam=BEAM, nbest=1, stats=True)
            share[f"w_V{V}_{kind}"] = round(float(frames.sum()) / (T * B), 5)
            if parent is not None:
                configs[f"p_V{V}_{kind}"] = parent_call(lp, V)
                a, b = configs[f"p_V{V}_{kind}"](), configs[f"w_V{V}_{kind}"]()
                share[f"p_V{V}_{kind}_equal_bits"] = bool(torch.equal(a[0], b.tokens) and torch.equal(a[1], b.lengths)
                                                           and torch.equal(a[2].view(torch.int64), b.score.view(torch.int64)))
            for order in ORDERS:
                kw = dict(beam=BEAM, nbest=1, unit_lm=models[V, order], lm_alpha=ALPHA, lm_beta=BETA)
                configs[f"f_V{V}_{kind}_n{order}"] = lambda lp=lp, kw=kw: hipops.ctc_beam_search_wide(lp, None, **kw)
                _, frames = hipops.ctc_beam_search_wide(lp, None, stats=True, **kw)
                share[f"f_V{V}_{kind}_n{order}"] = round(float(frames.sum()) / (T * B), 5)
    host = {}
    for N in (16, 128):
        seqs = sentences(1024, N * B, 99 + N, lo=100, hi=300)
        tok = np.zeros((N, B, 300), dtype=np.int32)
        ln = np.zeros((N, B), dtype=np.int32)
        for i, y in enumerate(seqs):
            tok[i // B, i % B, :len(y)] = y
            ln[i // B, i % B] = len(y)
        dt, dl, dc = torch.from_numpy(tok).to(dev), torch.from_numpy(ln).to(dev), torch.full((B,), N, dtype=torch.int32, device=dev)
        m = models[1024, 5]
        configs[f"s_N{N}"] = lambda dt=dt, dl=dl, dc=dc, m=m: hipops.nbest_unit_lm_score(dt, dl, dc, m)
        got = configs[f"s_N{N}"]().cpu().numpy()
        m.logp_sequence(seqs[0][:2])                   # the host's table is built on first use: not part of the loop's time
        t0 = time.perf_counter()
        want = np.array([m.logp_sequence(y) for y in seqs]).reshape(N, B)
        host[f"N{N}"] = {"host_loop_ms": round(1e3 * (time.perf_counter() - t0), 1), "equal_bits": bool((got == want).all())}
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
    result = {"shape": {"T": T, "B": B, "beam": BEAM, "alpha": ALPHA, "beta": BETA}, "device": torch.cuda.get_device_name(0),
              "repeats": args.repeats, "calls_per_window": args.calls, "sentences": args.sentences, "models": built,
              "counting_share": share, "second_pass_host": host, "configs": {}}
    for name in names:
        v = times[name]
        e = result["configs"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        print(f"{name:24s}: median {e['median']:.3f} ms  (min {e['min']:.3f}, max {e['max']:.3f})", flush=True)
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed window")
    ap.add_argument("--warm", type=int, default=1, help="warm-up calls per configuration")
    ap.add_argument("--sentences", type=int, default=20000, help="random unit sequences each model is estimated from")
    ap.add_argument("--parent-lib", default=None, help="a libpgasr_hip.so of the parent commit, for (p)")
    ap.add_argument("--limit", type=int, default=900, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(args.repeats), "--calls", str(args.calls),
           "--warm", str(args.warm), "--sentences", str(args.sentences)]
    if args.parent_lib:
        cmd += ["--parent-lib", os.path.abspath(args.parent_lib)]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"unit_lm_cost.py: the measuring child ran past {args.limit} s and was killed; nothing else was started")
    sys.exit(rc)


if __name__ == "__main__":
    main()
