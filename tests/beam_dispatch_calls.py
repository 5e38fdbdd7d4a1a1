"""The dispatch matrix of the beam searches: every combination of keywords that picks another kernel family, instantiation or argument
tail, on tiny seeded inputs.  ``run_all()`` makes the calls on the GPU and returns {name: the bytes of every output word};
tools/dev/beam_dispatch_record.py stores that for ANOTHER commit's library in tests/golden/beam_dispatch_parent.npz and
tests/test_beam_dispatch_gpu.py compares the current library with it, bit for bit.

Narrow calls go through hipops: T = 12, B = 3, lengths (12, 7, 1); V 29 and 40 (the single-wave kernel's two symbols-per-lane
instantiations); beam 4 and 17 (17 is just above that kernel's 16: the fast flags must change nothing); fp32 and fp64; with and without a
dense order-2 LM and a two-phrase hotword automaton at weight 1.5.  Combinations the wrappers refuse by name (a bias with fast /
fast_lm) are left out.  hipops never calls pgasr_ctc_beam_search itself, so a few raw calls of it follow.  The wide calls run at V = 80,
beam 4 on a case of tests/wide_hotword_ref.py's recipe (that module's model and automaton builders on a shape smaller than any of its
own cases), with and without a list, the unit model and the automaton.
"""
import itertools

import numpy as np

import beam_lm_ref as R
import wide_hotword_ref as WH

T, B, LENGTHS = 12, 3, (12, 7, 1)
NBEST, BIAS_WEIGHT, LM_ALPHA, LM_BETA = 3, 1.5, 0.7, 0.3
WIDE_CASE = (12, 80, 4, 0, 3, 2, 1.5, "mixed", 0)        # (T, V, beam, blank, B, unit-LM order, gamma, kind, seed) as wide_hotword_ref.CASES


def narrow_inputs(V, f64):
    rng = np.random.default_rng(1009 * V + 7)
    logits = rng.normal(size=(T, B, V)) * rng.choice([0.3, 2.0, 5.0], size=(T, B, 1))
    logits[:, :, 0] += 1.5
    if not f64:
        return R.log_softmax32(logits)
    m = logits.max(axis=-1, keepdims=True)
    return logits - (m + np.log(np.exp(logits - m).sum(axis=-1, keepdims=True)))


def _bools(n):
    return itertools.product((False, True), repeat=n)


def _cat(*tensors):
    return b"".join(t.detach().cpu().contiguous().numpy().tobytes() for t in tensors)


def run_all():
    import torch
    from policy_gradient_asr_amd import _lib, hipops
    from policy_gradient_asr_amd.lm import CharNgramLM, HotwordBias
    dev = torch.device("cuda:0")
    lens = torch.tensor(LENGTHS, dtype=torch.int32, device=dev)
    out = {}
    for V, f64 in itertools.product((29, 40), (False, True)):
        lp = torch.from_numpy(narrow_inputs(V, f64)).to(dev)
        lms = {"nolm": None, "lm": CharNgramLM(R.random_table(V, 2, 0, seed=V), 2, blank=0)}
        biases = {"nobias": None, "bias": HotwordBias([(3, 5, 7), (5, 2)], V, blank=0, boost=1.0, partial=1.0)}
        for beam, (ln, lm), (bn, bias) in itertools.product((4, 17), lms.items(), biases.items()):
            kw = dict(beam=beam, blank=0, lm=lm, lm_alpha=LM_ALPHA, lm_beta=LM_BETA)
            if bias is not None:
                kw.update(bias=bias, bias_weight=BIAS_WEIGHT)
            tag = f"V{V}-{'f64' if f64 else 'f32'}-K{beam}-{ln}-{bn}"
            for collapse, generic, fast_lm in _bools(3):
                if bias is None or not fast_lm:
                    out[f"best-{tag}-c{collapse:d}g{generic:d}l{fast_lm:d}"] = _cat(
                        *hipops.ctc_beam_search(lp, lens, collapse=collapse, generic=generic, fast_lm=fast_lm, **kw))
            for collapse, fast, fast_lm in _bools(3):
                if bias is None or not (fast or fast_lm):
                    out[f"list-{tag}-c{collapse:d}f{fast:d}l{fast_lm:d}"] = _cat(
                        *hipops.ctc_beam_search_nbest(lp, lens, nbest=NBEST, collapse=collapse, fast=fast, fast_lm=fast_lm, **kw))
        # the entry without a model, which hipops reaches only through pgasr_ctc_beam_search_lm
        lib = _lib.load()
        for beam, flags in itertools.product((4, 17), (0, 1, 2)):
            ws = torch.empty(lib.pgasr_beam_workspace_bytes(T, B, V, beam), dtype=torch.uint8, device=dev)
            tok, tl = torch.zeros(B, T, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
            score = torch.empty(B, dtype=torch.float64, device=dev)
            st = lib.pgasr_ctc_beam_search(lp.data_ptr(), int(f64), lp.stride(0), lp.stride(1), lens.data_ptr(), T, B, V, beam, 0, flags,
                                           tok.data_ptr(), tl.data_ptr(), score.data_ptr(), ws.data_ptr(), ws.numel(),
                                           torch.cuda.current_stream().cuda_stream)
            assert st == 0
            out[f"raw-V{V}-{'f64' if f64 else 'f32'}-K{beam}-flags{flags}"] = _cat(tok, tl, score)
    wlp, wlens, wbias, _ = WH.case_inputs(WIDE_CASE)
    unit = WH.case_model(WIDE_CASE)[1]
    lens_w = torch.from_numpy(np.asarray(wlens, dtype=np.int32)).to(dev)
    for f64 in (False, True):
        lp = torch.from_numpy(np.array(wlp, dtype=np.float64 if f64 else np.float32)).to(dev)
        for nbest, with_lm, with_bias, collapse in itertools.product((None, NBEST), *[(False, True)] * 3):
            if f64 and not (with_lm and with_bias):
                continue
            kw = dict(beam=WIDE_CASE[2], nbest=nbest, blank=WIDE_CASE[3], collapse=collapse)
            if with_lm:
                kw.update(unit_lm=unit, lm_alpha=WH.ALPHA, lm_beta=WH.BETA)
            if with_bias:
                kw.update(bias=wbias, bias_weight=WIDE_CASE[6])
            out[f"wide-{'f64' if f64 else 'f32'}-n{nbest}-lm{with_lm:d}-bias{with_bias:d}-c{collapse:d}"] = _cat(*hipops.ctc_beam_search_wide(lp, lens_w, **kw))
    torch.cuda.synchronize()
    return out


def pack(results):
    """{name: bytes} as three arrays: names, offsets (len + 1) and the words."""
    names = sorted(results)
    sizes = [len(results[n]) for n in names]
    return dict(names=np.array(names), offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                words=np.frombuffer(b"".join(results[n] for n in names), dtype=np.uint8))


def unpack(doc):
    off = doc["offsets"]
    return {str(n): doc["words"][off[i]:off[i + 1]].tobytes() for i, n in enumerate(doc["names"])}
