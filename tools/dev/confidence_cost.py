"""What N-best confidences cost beside the decoding they annotate (csrc/confidence.hip; NOTES.md 0.44).  Headline shape: T = 1000
(--frames), B = 32, V = 29, beam = N in {16, 128} (--sizes), fp32 log-probs peaked enough that the lists are near-equal strings of
about 0.93 T symbols; the lists come from the workgroup-per-utterance search (``ctc_beam_search_nbest``).  Per N, four times:

  (slot_mass)  pgasr_edit_ops_slot_mass alone, on the operation strings of the B * N (pivot, row) pairs, side "ref";
  (confidence) the whole hipops.nbest_confidence call at character level: the pairs expanded in chunks, pgasr_edit_ops on them
               (one wave per pair, about 235 KB of workspace a pair at this length) and the launch above per chunk;
  (mbr)        CTCDecoder.mbr_from_list on the same lists (pair distances and selection), the cap given: what produced the
               posterior the confidences weight;
  (search)     the N-best search itself.

Inputs are rotated: every call of a window takes the next of as many device copies of its inputs as make 288 MB, so that no call
finds its operands in the 256 MB Infinity Cache because the call before left them there.  The measurement runs in ONE child process
under a time limit (--limit seconds; the parent never touches the GPU and starts nothing after a child that failed or was killed).
In it every configuration is warmed up, then every repeat (--repeats 5) times a window of back-to-back calls between two device
events, the order reversed every other repeat; the median of the windows is reported, with the share of the confidence call that is
the new kernel.  One JSON line at the end.  Not imported by bench.py or the package."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

B, V = 32, 29
ROTATE_BYTES = 288 << 20


def worker(args):
    import numpy as np
    import torch
    from policy_gradient_asr_amd import _lib, hipops
    from policy_gradient_asr_amd.CTCdecoder import CTCDecoder
    if not torch.cuda.is_available():
        raise SystemExit("confidence_cost.py needs the MI355X: nothing is measured without it")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(424246)
    T, SIZES = args.frames, tuple(int(x) for x in args.sizes.split(","))
    logits = rng.normal(size=(T, B, V)) * 4.0
    m = logits.max(axis=-1, keepdims=True)
    lp = torch.from_numpy((logits - (m + np.log(np.exp(logits - m).sum(axis=-1, keepdims=True)))).astype(np.float32)).to(dev)
    dec = CTCDecoder(["<b>"] + [chr(ord("a") + i) for i in range(26)] + ["'", " "])
    result = {"shape": {"T": T, "B": B, "V": V}, "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "sizes": {}}
    for n in SIZES:
        try:
            nb = hipops.ctc_beam_search_nbest(lp, None, beam=n, nbest=n)
        except _lib.PgasrError as e:                     # a refusal of the search at this size: reported, not measured
            result["sizes"]["N%d" % n] = {"refused": str(e)}
            continue
        longest = int(nb.lengths.max().item())
        md = dec.mbr_from_list(nb, nb.score, vocab=V, max_hyp_len=longest)
        pivot = torch.zeros(B, dtype=torch.int32, device=dev)
        S = nb.tokens.shape[2]
        # the operation strings of all pairs, as nbest_confidence builds them chunk by chunk
        ref = nb.tokens[0].unsqueeze(1).expand(B, n, S).reshape(B * n, S).contiguous()
        rl = nb.lengths[0].unsqueeze(1).expand(B, n).reshape(B * n).contiguous()
        hyp = nb.tokens.permute(1, 0, 2).reshape(B * n, S).contiguous()
        hl = nb.lengths.t().reshape(B * n).contiguous()
        eo = hipops.edit_ops(ref, rl, hyp, hl, want_ops=True)
        weight = md.posterior.t().contiguous().view(-1)
        del ref, hyp
        copies = max(2, -(-ROTATE_BYTES // eo.ops.numel()))
        ops_copies = [eo.ops.clone() for _ in range(copies)]
        tok_copies = [nb.tokens.clone() for _ in range(max(2, -(-ROTATE_BYTES // (nb.tokens.numel() * 4))))]
        turn = {"slot_mass": 0, "confidence": 0}

        def slot_mass():
            turn["slot_mass"] += 1
            return hipops.edit_ops_slot_mass(ops_copies[turn["slot_mass"] % len(ops_copies)], eo.n_ops, weight, n, side="ref", slots=S)

        def confidence():
            turn["confidence"] += 1
            return hipops.nbest_confidence(tok_copies[turn["confidence"] % len(tok_copies)], nb.lengths, nb.count, md.posterior, pivot,
                                           max_hyp_len=longest)

        whole, alone = confidence(), slot_mass()
        agree = bool(torch.equal(whole.conf[:, :longest + 1], alone.hit[:, :longest + 1]))
        configs = {
            "slot_mass": (args.calls, slot_mass),
            "confidence": (args.slow_calls, confidence),
            "mbr": (args.slow_calls, lambda: dec.mbr_from_list(nb, nb.score, vocab=V, max_hyp_len=longest)),
            "search": (1, lambda: hipops.ctc_beam_search_nbest(lp, None, beam=n, nbest=n)),
        }
        names = list(configs)

        def window(name, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                configs[name][1]()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / calls          # ms per call

        for name in names:
            window(name, min(args.warm, configs[name][0]))
        times = {name: [] for name in names}
        for r in range(args.repeats):
            for name in (names if r % 2 == 0 else names[::-1]):
                times[name].append(window(name, configs[name][0]))
        entry = result["sizes"]["N%d" % n] = {"pairs": B * n, "longest_hypothesis": longest,
                                              "mean_hypothesis": round(float(nb.lengths.float().mean().item()), 1),
                                              "ops_stride": int(eo.ops.shape[1]), "rotated_copies": {"ops": len(ops_copies), "tokens": len(tok_copies)},
                                              "kernel_agrees_with_call": agree, "ms_per_call": {}}
        for name in names:
            v = times[name]
            entry["ms_per_call"][name] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            print(f"N={n:3d} {name:10s}: median {statistics.median(v):.4f} ms  (min {min(v):.4f}, max {max(v):.4f})", flush=True)
        med = {k: entry["ms_per_call"][k]["median"] for k in names}
        entry["slot_mass_share_of_confidence"] = round(med["slot_mass"] / med["confidence"], 4)
        entry["confidence_over_mbr"] = round(med["confidence"] / med["mbr"], 2)
        entry["confidence_over_search"] = round(med["confidence"] / med["search"], 3)
        del ops_copies, tok_copies
        torch.cuda.empty_cache()
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000, help="T: frames per utterance (the hypotheses are about 0.93 T long)")
    ap.add_argument("--sizes", default="16,128", help="list sizes N (= beam), comma separated")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window of the new launch")
    ap.add_argument("--slow-calls", type=int, default=2, help="calls per timed window of the whole call and of mbr_from_list")
    ap.add_argument("--warm", type=int, default=2, help="warm-up calls per configuration")
    ap.add_argument("--limit", type=int, default=420, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(args.repeats), "--calls", str(args.calls),
           "--slow-calls", str(args.slow_calls), "--warm", str(args.warm), "--frames", str(args.frames), "--sizes", args.sizes]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f"confidence_cost.py: the measuring child ran past {args.limit} s and was killed; nothing else was started")
    sys.exit(rc)


if __name__ == "__main__":
    main()
