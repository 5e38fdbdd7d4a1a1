"""What spelling unit rows into character rows costs (csrc/unit_spell.hip; NOTES.md 0.34).

  kernel    pgasr_unit_spell alone on two shapes -- 160 rows of 1000 units (K = 4, B = 32, T = 1000: the rows of a train step, about
            a quarter of each row filled, as collapsed paths are) and 4096 full rows of 300 units -- over 1023 units of 1 .. 8
            characters (mean 4.5, a 20 KB pool), beside the bytes it must move: the units read, the whole output rows written (the
            zero tail included), as a share of the 8 TB/s HBM peak.  Every call of a window takes the next of n (input, output) buffer
            pairs, n chosen so that the pairs together exceed twice the 256 MiB Infinity Cache: no call finds its rows in a cache.
  step      the V = 256 wide train step (PolicyGradientTrainer(wide_alphabet=True), f32, train mode, F = 80, T = 1000, B = 32) with
            unit_spelling= and reward_unit="word" beside the default wide step, on the same library, in alternating child processes.
  parent    the default V = 29 and V = 256 steps with this tree's library and, with --parent-lib, with another build of the
            library (the parent commit's), in alternating child processes: the new entry must not move a step that does not use it.

Every measurement runs in a child process under a time limit (--limit seconds each; the parent process never touches the GPU and
starts nothing after a child that failed or was killed).  A child warms every configuration up, then times --repeats (5) windows
of back-to-back calls between two device events and reports the median, minimum and maximum.  One JSON line at the end.  Not
imported by bench.py or the package."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

T, B, L, F = 1000, 32, 60, 80
HBM_PEAK = 8.0e12            # bytes / s
CACHE = 256 << 20            # Infinity Cache
SHAPES = {"160x1000": (160, 1000, 0.25), "4096x300": (4096, 300, 1.0)}      # rows, stride, filled share of a row


def _summary(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def _windows(fn, calls, repeats, warm):
    import torch
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(calls):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


def _spelling(V, seed=1):
    """V - 1 distinct units over " " and 26 letters: the single characters, then random strings of 2 .. 8 characters."""
    import random
    from policy_gradient_asr_amd.units import SubwordUnits, UnitSpelling
    rnd = random.Random(seed)
    alphabet = [" "] + [chr(97 + i) for i in range(26)]
    units = list(alphabet[:V - 1])
    have = set(units)
    while len(units) < V - 1:
        u = "".join(rnd.choice(alphabet) for _ in range(rnd.randint(2, 8)))
        if u not in have:
            units.append(u); have.add(u)
    return UnitSpelling(SubwordUnits(units), alphabet)


def kernel_worker(args):
    import torch
    from policy_gradient_asr_amd import _lib, hipops
    if not torch.cuda.is_available():
        raise SystemExit("unit_spell_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    sp = _spelling(1024)
    off, pool = sp.to(dev)
    g = torch.Generator().manual_seed(7)
    res = {"device": torch.cuda.get_device_name(0), "units": sp.vocab - 1, "pool_bytes": 4 * len(sp.chars), "shapes": {}}
    for name, (N, stride, fill) in SHAPES.items():
        out_stride = min(stride * sp.max_unit_chars, hipops.WORD_MAX_STRIDE)
        pair_bytes = N * (stride + out_stride) * 4
        n = max(2, -(-2 * CACHE // pair_bytes) + 1)
        lengths = torch.full((N,), int(stride * fill), dtype=torch.int32).to(dev)
        tokens = [torch.randint(1, sp.vocab, (N, stride), generator=g, dtype=torch.int32).to(dev) for _ in range(n)]
        outs = [torch.empty(N, out_stride, dtype=torch.int32, device=dev) for _ in range(n)]
        lens = torch.empty(2, N, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def fn(i):
            st = lib.pgasr_unit_spell(tokens[i % n].data_ptr(), lengths.data_ptr(), stride, N, off.data_ptr(), pool.data_ptr(), sp.vocab,
                                      outs[i % n].data_ptr(), out_stride, lens[0].data_ptr(), lens[1].data_ptr(), stream)
            assert st == 0
        ms = _windows(fn, args.calls, args.repeats, args.warm)
        full = lens[1].cpu()
        nbytes = N * int(stride * fill) * 4 + N * out_stride * 4
        e = res["shapes"][name] = {"rows": N, "stride": stride, "units_per_row": int(stride * fill), "out_stride": out_stride,
                                   "mean_chars_per_row": float(full.float().mean()), "truncated_rows": int((full > out_stride).sum()),
                                   "buffers": n, "bytes": nbytes, "ms_per_call": _summary(ms),
                                   "share_of_hbm_peak": round(nbytes / (statistics.median(ms) * 1e-3) / HBM_PEAK, 4)}
        print(f"{name}: median {statistics.median(ms):.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}), {nbytes / 1e6:.1f} MB, "
              f"{e['share_of_hbm_peak'] * 100:.1f} % of HBM peak", flush=True)
        del tokens, outs
        torch.cuda.empty_cache()
    print(json.dumps({"kernel": res}))


def step_worker(args):
    import ctypes
    import torch
    from policy_gradient_asr_amd import _lib, hipops
    if args.older_lib:
        # an older build lacks the entry points added since: bind what it has (the default steps call none of the others)
        have = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
            del _lib.SIGNATURES[name]
    from policy_gradient_asr_amd.model import Seq2Seq, weights
    from policy_gradient_asr_amd.train_step import PolicyGradientTrainer
    if not torch.cuda.is_available():
        raise SystemExit("unit_spell_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    V = args.vocab
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(0)
    m = Seq2Seq(V, n_feats=F); m.apply(weights); m = m.to(dev).train()
    kw = {"wide_alphabet": True} if V > 64 else {}
    if args.spelled:
        kw.update(unit_spelling=_spelling(V), reward_unit="word")
    tr = PolicyGradientTrainer(m, lam=1.0, seed=3, precision="f32", **kw)
    x = torch.randn(B, F, T, generator=g).to(dev)
    targets = torch.randint(1, V, (B, L), generator=g).to(dev)
    fmask = torch.ones(B, T, device=dev)
    tmask = torch.ones(B, L, dtype=torch.int64, device=dev)
    ms = _windows(lambda i: tr.step(x, targets, fmask, tmask), args.calls, args.repeats, args.warm)
    hipops.lstm_assert_no_timeouts()
    extra = {}
    if args.spelled:
        extra["truncated_rows_last_step"] = int(tr.last_spell_truncated)
    print(f"step V={V} spelled={bool(args.spelled)} lib={os.path.basename(_lib.LIB_PATH)}: median {statistics.median(ms):.4f} ms "
          f"(min {min(ms):.4f}, max {max(ms):.4f})", flush=True)
    print(json.dumps({"step": {"V": V, "spelled": bool(args.spelled), "lib": _lib.LIB_PATH, "ms_per_step": _summary(ms), **extra}}))


def _child(argv, limit, env=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + argv
    try:
        p = subprocess.run(cmd, timeout=limit, env=env, stdout=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"unit_spell_cost.py: a measuring child ran past {limit} s and was killed; nothing else was started")
    sys.stdout.write(p.stdout)
    sys.stdout.flush()
    if p.returncode != 0:
        raise SystemExit(f"unit_spell_cost.py: a measuring child ended with status {p.returncode}; nothing else was started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40, help="calls per timed window of the kernel")
    ap.add_argument("--step-calls", type=int, default=20, help="steps per timed window")
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds of the step comparisons")
    ap.add_argument("--limit", type=int, default=240, help="seconds each measuring child may take")
    ap.add_argument("--parent-lib", default=None, help="another build of libpgasr_hip.so to time the default steps with")
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: kernel, step, parent")
    ap.add_argument("--worker", choices=("kernel", "step"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--vocab", type=int, default=29, help=argparse.SUPPRESS)
    ap.add_argument("--spelled", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--older-lib", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker == "kernel":
        return kernel_worker(args)
    if args.worker == "step":
        return step_worker(args)
    skip = set(filter(None, args.skip.split(",")))
    common = ["--repeats", str(args.repeats), "--warm", str(args.warm)]
    out = {}
    if "kernel" not in skip:
        out.update(_child(["--worker", "kernel", "--calls", str(args.calls)] + common, args.limit))
    step = ["--worker", "step", "--calls", str(args.step_calls)] + common
    if "step" not in skip:
        runs = {"default": [], "spelled_word": []}
        for _ in range(args.rounds):                      # alternating processes: default, spelled, default, spelled, ..
            runs["default"].append(_child(step + ["--vocab", "256"], args.limit)["step"]["ms_per_step"])
            runs["spelled_word"].append(_child(step + ["--vocab", "256", "--spelled"], args.limit)["step"]["ms_per_step"])
        out["step_V256"] = runs
    if "parent" not in skip:
        libs = [("this", None)] + ([("parent", os.path.abspath(args.parent_lib))] if args.parent_lib else [])
        for V in (29, 256):
            runs = {name: [] for name, _ in libs}
            for _ in range(args.rounds):                  # alternating processes: this, parent, this, parent, ..
                for name, lib in libs:
                    env = dict(os.environ)
                    env.pop("PGASR_HIP_LIB", None)
                    if lib:
                        env["PGASR_HIP_LIB"] = lib
                    runs[name].append(_child(step + ["--vocab", str(V)] + (["--older-lib"] if lib else []), args.limit, env)["step"]["ms_per_step"])
            out[f"default_step_V{V}"] = runs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
