"""What the language-model term costs the workgroup-per-utterance beam kernel (csrc/beam.hip), and whether adding it left the
LM-less instantiations alone.  T = 1000, B = 32, V = 29, fp32 log-probs, beam 5 and 16, the general kernel forced (flags bit 1):

  (a) no LM, a library built from the PARENT commit (--parent-lib; e.g. `git worktree add /tmp/parent HEAD~1 &&
      make -C /tmp/parent/policy_gradient_asr_amd/csrc`), through pgasr_ctc_beam_search;
  (b) no LM, this tree's library, through pgasr_ctc_beam_search;
  (c) with an LM of order 2, 3, 4 (random tables), this tree's library, through pgasr_ctc_beam_search_lm.

Both libraries are loaded into ONE process and every repeat runs a, b, c2, c3, c4 in turn, so old and new alternate in the same
call.  Each timing is a window of at least --window seconds of back-to-back calls between two device events, after a warm-up of
every configuration.  (b) against (a) is a pass/fail bar: the median of (b)'s repeats must lie inside the run-to-run spread
(min .. max) of (a)'s own repeats.  (c) has no bar: (c)/(b) is reported per order.  One JSON line at the end."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
from policy_gradient_asr_amd import _lib  # noqa: E402

DEV = "cuda:0"
T, B, V = 1000, 32, 29
BASE_ARGS = _lib.SIGNATURES["pgasr_ctc_beam_search"][1]


def bind(path, with_lm):
    lib = C.CDLL(path)
    lib.pgasr_beam_workspace_bytes.restype = C.c_size_t
    lib.pgasr_beam_workspace_bytes.argtypes = [C.c_int] * 4
    lib.pgasr_ctc_beam_search.restype = C.c_int
    lib.pgasr_ctc_beam_search.argtypes = BASE_ARGS
    if with_lm:
        lib.pgasr_ctc_beam_search_lm.restype, lib.pgasr_ctc_beam_search_lm.argtypes = _lib.SIGNATURES["pgasr_ctc_beam_search_lm"]
    return lib


def random_table(order, gen):
    z = torch.randn((V,) * order, generator=gen) * 2.0
    z[..., 0] = -float("inf")
    t = torch.log_softmax(z, -1)
    t[..., 0] = 0.0
    return t.contiguous().to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libpgasr_hip.so built from the parent commit; without it (a) is not measured")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beam_lm_cost.py needs the MI355X: nothing is measured without it")

    new = bind(_lib.LIB_PATH, True)
    old = bind(args.parent_lib, False) if args.parent_lib else None
    gen = torch.Generator().manual_seed(0)
    lp = torch.log_softmax(torch.randn(T, B, V, generator=gen) * 2, 2).to(DEV)
    tables = {n: random_table(n, gen) for n in (2, 3, 4)}
    tokens = torch.zeros(B, T, dtype=torch.int32, device=DEV)
    tl = torch.empty(B, dtype=torch.int32, device=DEV)
    score = torch.empty(B, dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    result = {"shape": {"T": T, "B": B, "V": V}, "repeats": args.repeats, "window_s": args.window, "beams": {}}

    for beam in (5, 16):
        ws = torch.empty(new.pgasr_beam_workspace_bytes(T, B, V, beam), dtype=torch.uint8, device=DEV)
        base = (lp.data_ptr(), 0, lp.stride(0), lp.stride(1), None, T, B, V, beam, 0, 2, tokens.data_ptr(), tl.data_ptr(),
                score.data_ptr(), ws.data_ptr(), ws.numel(), stream)

        def call_plain(lib):
            def f():
                st = lib.pgasr_ctc_beam_search(*base)
                assert st == 0, st
            return f

        def call_lm(order):
            def f():
                st = new.pgasr_ctc_beam_search_lm(*base, tables[order].data_ptr(), order, 0.5, 0.5)
                assert st == 0, st
            return f

        configs = {}
        if old is not None:
            configs["a_parent_no_lm"] = call_plain(old)
        configs["b_new_no_lm"] = call_plain(new)
        for n in (2, 3, 4):
            configs[f"c_lm_order{n}"] = call_lm(n)

        def window(f, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                f()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n          # ms per call

        # the LM-less results of the two libraries must be the same bits before their times are compared
        outs = {}
        for name, f in configs.items():
            f(); torch.cuda.synchronize()
            outs[name] = (tokens.clone(), tl.clone(), score.clone())
        if old is not None:
            assert all(torch.equal(x, y) for x, y in zip(outs["a_parent_no_lm"], outs["b_new_no_lm"])), "parent and new differ without LM"
        calls = {}
        for name, f in configs.items():              # warm-up, and the number of calls that fills a window
            per = window(f, 3)
            calls[name] = max(3, int(args.window * 1e3 / per) + 1)
        times = {name: [] for name in configs}
        for _ in range(args.repeats):
            for name, f in configs.items():
                times[name].append(window(f, calls[name]))
        entry = {name: {"ms_per_call": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "min": round(min(v), 4),
                        "max": round(max(v), 4), "calls_per_window": calls[name]} for name, v in times.items()}
        b_med = entry["b_new_no_lm"]["median"]
        if old is not None:
            a = entry["a_parent_no_lm"]
            entry["b_inside_spread_of_a"] = bool(a["min"] <= b_med <= a["max"])
            entry["b_over_a"] = round(b_med / a["median"], 4)
        else:
            entry["b_inside_spread_of_a"] = "not measured"
        for n in (2, 3, 4):
            entry[f"c{n}_over_b"] = round(entry[f"c_lm_order{n}"]["median"] / b_med, 4)
        result["beams"][str(beam)] = entry
        for name in configs:
            e = entry[name]
            print(f"beam {beam:2d} {name:16s}: median {e['median']:.3f} ms  (min {e['min']:.3f}, max {e['max']:.3f}; "
                  f"{e['calls_per_window']} calls per window)", flush=True)
        print(f"beam {beam:2d} (b) inside the spread of (a): {entry['b_inside_spread_of_a']};  (c)/(b): "
              + ", ".join(f"order {n}: {entry[f'c{n}_over_b']:.3f}" for n in (2, 3, 4)), flush=True)
    print(json.dumps(result))
    ok = all(e["b_inside_spread_of_a"] is not False for e in result["beams"].values())
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
