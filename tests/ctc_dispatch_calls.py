"""The dispatch matrix of the CTC loss section: every combination of entry, alphabet size and optional term that picks another kernel
family, instantiation or argument tail, on tiny seeded inputs.  ``run_all()`` makes the calls on the GPU and returns
{name: SHA-256 of the status and every output word}; tools/dev/ctc_dispatch_record.py stores that for ANOTHER commit's library in
tests/golden/ctc_dispatch_parent.npz and tests/test_ctc_dispatch_gpu.py compares the current library with it, bit for bit.

T = 6, B = 3: eighteen rows, so the last workgroup of four waves is partial.  input_lengths (6, 0, 4), target_lengths (3, 2, 0) with
Lmax = 4, K = 2, Lh = 3 with one sampled hypothesis of length 4 (it takes the path fallback) and one N-best row of length 0.  V 5 and
64 go through the narrow entries, V 40 .. 1024 through the wide ones: every NV of PGASR_WIDE_DISPATCH and both values of V % vector
width.  The calls go through the hipops wrappers; a few raw calls of the narrow ``_ent`` / ``_kl`` entries with NULL tails follow (the
forwarding chain).
"""
import hashlib

import numpy as np

T, B, LMAX, K, LH, STRIDE = 6, 3, 4, 2, 3, 4
INPUT_LENGTHS, TARGET_LENGTHS = (6, 0, 4), (3, 2, 0)
HYP_LEN = ((3, 2, 4), (1, 3, 2))            # (K,B): pair (0,2) is over Lh
NBEST_LEN = ((3, 0, 2), (1, 3, 2))          # (N,B): pair (0,1) is the empty hypothesis
NARROW_V, WIDE_V = (5, 64), (40, 65, 128, 130, 260, 1022, 1024)
TAILS = ("none", "ent", "kl", "both")


def inputs(V):
    """Host arrays of one alphabet size, by name."""
    rng = np.random.default_rng(7919 * V + 3)

    def log_softmax(x):
        x = x - x.max(axis=-1, keepdims=True)
        return (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)

    tok = lambda *shape: rng.integers(1, V, size=shape).astype(np.int32)      # noqa: E731
    f32 = lambda *shape: rng.normal(size=shape).astype(np.float32)            # noqa: E731
    d = dict(lp=log_softmax(rng.normal(size=(T, B, V)) * 2.0), ref=log_softmax(rng.normal(size=(T, B, V))),
             targets=tok(B, LMAX), il=np.array(INPUT_LENGTHS, np.int32), tl=np.array(TARGET_LENGTHS, np.int32),
             utt=np.abs(f32(B)) + 0.25, coef_b=f32(B), coef_tb=f32(T, B), coef_kb=f32(K, B), coef_ktb=f32(K, T, B),
             path=rng.integers(0, V, size=(T, B)).astype(np.int32), paths=rng.integers(0, V, size=(K, T, B)).astype(np.int32),
             hyp=tok(K, B, STRIDE), hyp_len=np.array(HYP_LEN, np.int32), nbest_len=np.array(NBEST_LEN, np.int32),
             ent=np.abs(f32(B)) * 0.1, kl=np.abs(f32(B)) * 0.2)
    d["coef_tb_const"] = np.broadcast_to(d["coef_b"], (T, B)).copy()
    d["coef_ktb_const"] = np.broadcast_to(d["coef_kb"][:, None, :], (K, T, B)).copy()
    return d


def digest(status, *tensors):
    h = hashlib.sha256(np.int32(status).tobytes())
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _tails(d, which):
    return {"none": {}, "ent": dict(ent_scale=d["ent"]), "kl": dict(ref_log_probs=d["ref"], kl_scale=d["kl"]),
            "both": dict(ent_scale=d["ent"], ref_log_probs=d["ref"], kl_scale=d["kl"])}[which]


def _shifted(t):
    """The tensor's values one float past a 16-byte boundary: a contiguous view that no vector access may take."""
    import torch
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    return out


def run_all():
    import torch
    from policy_gradient_asr_amd import _lib, hipops
    dev = torch.device("cuda:0")
    out = {}
    for V, wide in [(v, False) for v in NARROW_V] + [(v, True) for v in WIDE_V]:
        d = {k: torch.from_numpy(v).to(dev) for k, v in inputs(V).items()}
        lp, il, tl, utt = d["lp"], d["il"], d["tl"], d["utt"]
        tag = f"{'wide' if wide else 'narrow'}-V{V}"
        nll, grad = hipops.ctc_loss_grad(lp, d["targets"], il, tl, utt_scale=utt, need_grad=False, wide=wide)
        out[f"loss-{tag}-nograd"] = digest(0, nll)
        nll, grad = hipops.ctc_loss_grad(lp, d["targets"], il, tl, utt_scale=utt, pg_coef=d["coef_b"], pg_path=d["path"], wide=wide)
        out[f"loss-{tag}-grad"] = digest(0, nll, grad)
        nll, handle = hipops.ctc_lattice(lp, d["targets"], il, tl, wide=wide)
        out[f"lattice-{tag}"] = digest(0, nll)
        for tail in TAILS if not wide else TAILS[:1]:                # the wide single-path pass has no optional terms
            for form, coef in (("nopg", None), ("utt", "coef_b"), ("frame", "coef_tb"), ("frameconst", "coef_tb_const")):
                pg = {} if coef is None else dict(pg_coef=d[coef], pg_path=d["path"])
                out[f"one-{tag}-{form}-{tail}"] = digest(0, hipops.ctc_grad_from_lattice(lp, il, tl, handle, utt, wide=wide, **pg, **_tails(d, tail)))
        for tail in TAILS:
            for form, coef in (("multi", "coef_kb"), ("steps", "coef_ktb"), ("stepsconst", "coef_ktb_const")):
                out[f"{form}-{tag}-{tail}"] = digest(0, hipops.ctc_grad_from_lattice_multi(lp, il, tl, handle, utt, d[coef], d["paths"], wide=wide,
                                                                                          **_tails(d, tail)))
        hyp_nll, hyp_handle = hipops.ctc_hyp_lattice(lp, d["hyp"], d["hyp_len"], il, LH, wide=wide)
        out[f"hyp-{tag}-seq"] = digest(0, hyp_nll)
        for tail in TAILS:
            out[f"seq-{tag}-{tail}"] = digest(0, hipops.ctc_grad_from_lattices_seq(lp, il, tl, handle, hyp_handle, utt, d["coef_kb"], d["paths"],
                                                                                 d["hyp_len"], wide=wide, **_tails(d, tail)))
        if wide:        # the KL tail's one `vec`: log_probs off the vector boundary, then ref_log_probs alone
            for what, lp_x, ref_x in (("lpshift", _shifted(lp), d["ref"]), ("refshift", lp, _shifted(d["ref"]))):
                kl = dict(ref_log_probs=ref_x, kl_scale=d["kl"])
                out[f"multi-{tag}-kl-{what}"] = digest(0, hipops.ctc_grad_from_lattice_multi(lp_x, il, tl, handle, utt, d["coef_kb"], d["paths"],
                                                                                           wide=True, **kl))
                out[f"steps-{tag}-kl-{what}"] = digest(0, hipops.ctc_grad_from_lattice_multi(lp_x, il, tl, handle, utt, d["coef_ktb"], d["paths"],
                                                                                           wide=True, **kl))
                out[f"seq-{tag}-kl-{what}"] = digest(0, hipops.ctc_grad_from_lattices_seq(lp_x, il, tl, handle, hyp_handle, utt, d["coef_kb"],
                                                                                        d["paths"], d["hyp_len"], wide=True, **kl))
        else:           # the forwarding chain: X_ent with ent_scale NULL and X_kl with every tail NULL are X
            out.update(_raw_chain(_lib.load(), tag, d, V, handle, hyp_handle))
        # after the last pass over the sampled hypotheses' lattices: the N-best ones take their place in the cached workspace
        nb_nll, nb_handle = hipops.ctc_hyp_lattice(lp, d["hyp"], d["nbest_len"], il, LH, wide=wide)
        out[f"hyp-{tag}-nbest"] = digest(0, nb_nll)
        out[f"nbest-{tag}-none"] = digest(0, hipops.ctc_grad_from_lattices_nbest(lp, il, tl, handle, nb_handle, utt, d["coef_kb"], d["nbest_len"],
                                                                               wide=wide))
    torch.cuda.synchronize()
    return out


def _raw_chain(lib, tag, d, V, handle, hyp_handle):
    import torch
    p = lambda t: 0 if t is None else t.data_ptr()      # noqa: E731
    ws, Lmax, blank = handle
    hws, _, Lh = hyp_handle
    st = torch.cuda.current_stream().cuda_stream
    head = [p(d["lp"]), p(d["il"]), p(d["tl"]), T, B, V, Lmax, blank, p(d["utt"])]
    mids = {"one": [p(d["coef_b"]), p(d["path"]), 0], "multi": [K, p(d["coef_kb"]), p(d["paths"])],
            "seq": [K, p(d["coef_kb"]), p(d["paths"]), p(d["hyp_len"]), Lh]}
    names = {"one": "pgasr_ctc_grad_from_lattice", "multi": "pgasr_ctc_grad_from_lattice_multi", "seq": "pgasr_ctc_grad_from_lattices_seq"}
    out = {}
    for form, mid in mids.items():
        two = [p(hws), hws.numel()] if form == "seq" else []
        for suffix, nulls in (("_ent", [0]), ("_kl", [0, 0, 0]), ("_kl", [p(d["ent"]), 0, 0])):
            grad = torch.empty_like(d["lp"])
            status = getattr(lib, names[form] + suffix)(*head, *mid, *nulls, p(grad), p(ws), ws.numel(), *two, st)
            out[f"raw-{tag}-{form}{suffix}-{'ent' if nulls[0] else 'null'}"] = digest(status, grad)
    return out


def pack(results):
    """{name: hex digest} as two arrays: the sorted names and their digests, 32 bytes each."""
    names = sorted(results)
    return dict(names=np.array(names), digests=np.array([list(bytes.fromhex(results[n])) for n in names], dtype=np.uint8))


def unpack(doc):
    return {str(n): bytes(row).hex() for n, row in zip(doc["names"], doc["digests"])}
