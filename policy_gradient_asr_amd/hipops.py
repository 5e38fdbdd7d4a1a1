"""Tensor-level wrappers over the C ABI (one function per entry point of
include/pgasr_hip.h).  torch is used for device memory and the current stream only.
Every wrapper requires CUDA(HIP) tensors and raises otherwise -- no CPU fallback."""
import collections
import ctypes
import os

import torch

_os_environ_get = os.environ.get

from . import _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _req(t, dtype, name):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.PgasrError(f"{name} must live on the GPU (got {t.device}); there is no CPU path")
    if t.dtype != dtype:
        raise _lib.PgasrError(f"{name} must be {dtype} (got {t.dtype})")
    if not t.is_contiguous():
        raise _lib.PgasrError(f"{name} must be contiguous")
    return t


def _p(t):
    return 0 if t is None else t.data_ptr()


_ws_cache = {}

# ---- optional per-kernel timing with HIP events on the launch stream (used by bench.py) ----
_prof_on = False
_prof_events = []


_prof_only = None


def profile_reset(enable, only=None):
    """only: iterable of name prefixes to time (None = every instrumented launch); an event pair costs a few
    microseconds of stream time, so bench.py times just the kernels its roofline is about inside the timed region."""
    global _prof_on, _prof_only
    _prof_on = bool(enable)
    _prof_only = tuple(only) if only else None
    _prof_events.clear()


def profile_pause(paused):
    """Stop / resume recording without dropping what was collected (bench.py instruments every n-th step: each event
    record costs the stream ~5 us)."""
    global _prof_on
    _prof_on = not paused


def profile_collect():
    """name -> (total ms, launches); synchronises."""
    torch.cuda.synchronize()
    out = {}
    for name, e0, e1 in _prof_events:
        ms, n = out.get(name, (0.0, 0))
        out[name] = (ms + e0.elapsed_time(e1), n + 1)
    return out


def profile_phases(step_marks):
    """Mean phases of a train step from the HIP events of its six sweeps (``profile_reset(True, only=("lstm_",))``) and one
    (start, end) event pair per step, all on the main stream: front end (step start -> first forward sweep), forward (first
    forward sweep start -> last forward sweep end, gaps included), loss section (-> first backward sweep), backward sweeps, tail
    (last backward sweep end -> end of the step's Adam).  Synchronises."""
    torch.cuda.synchronize()
    sweeps = [(n, a, b) for n, a, b in _prof_events if n.startswith("lstm_")]
    if not step_marks or len(sweeps) != 6 * len(step_marks):
        return None
    acc = {"front_end": 0.0, "forward_sweeps": 0.0, "loss_section": 0.0, "backward_sweeps": 0.0, "tail": 0.0}
    per_sweep = [0.0] * 6      # launch order: forward layers 1..3, backward layers 3..1
    for i, (s0, s1) in enumerate(step_marks):
        sw = sweeps[6 * i:6 * i + 6]
        if [n for n, _, _ in sw] != ["lstm_fwd_kernel"] * 3 + ["lstm_bwd_kernel"] * 3:
            return None
        acc["front_end"] += s0.elapsed_time(sw[0][1])
        acc["forward_sweeps"] += sw[0][1].elapsed_time(sw[2][2])
        acc["loss_section"] += sw[2][2].elapsed_time(sw[3][1])
        acc["backward_sweeps"] += sw[3][1].elapsed_time(sw[5][2])
        acc["tail"] += sw[5][2].elapsed_time(s1)
        for j in range(6):
            per_sweep[j] += sw[j][1].elapsed_time(sw[j][2])
    out = {k: v / len(step_marks) for k, v in acc.items()}
    out["sweeps_in_launch_order"] = [v / len(step_marks) for v in per_sweep]
    return out


class _timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.on = _prof_on and self.name is not None and (_prof_only is None or self.name.startswith(_prof_only))
        if self.on:
            self.e0 = torch.cuda.Event(enable_timing=True); self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *a):
        if self.on:
            self.e1.record()
            _prof_events.append((self.name, self.e0, self.e1))
        return False


def _workspace(nbytes, device, tag):
    key = (tag, device, torch.cuda.current_stream().cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        # sweep workspaces start zeroed: their first word is a STICKY error flag (lstm_assert_no_timeouts)
        alloc = torch.zeros if tag.startswith("lstm") else torch.empty
        buf = alloc(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


# ---- alphabets of 65 .. 1024 symbols (include/pgasr_hip.h, A5-WIDE / A9-WIDE / A12-WIDE / A13-WIDE) ----
MAX_VOCAB_NARROW = 64            # one label per lane: every entry point without a _wide form
MAX_VOCAB_WIDE = 1024            # PGASR_MAX_VOCAB_WIDE: log-softmax, arg-max / sample, CTC lattice and gradient pass; the K-draw
                                 # sampler, the entropy and KL statistics and the multi-sample gradient pass with their tails


def _wide(V, wide, what):
    """Which entry a wrapper with a ``_wide`` form takes: by V (wide=None), or the caller's choice -- the wide kernels take V <= 64
    too, which is how the tests compare the two."""
    if wide is None:
        wide = V > MAX_VOCAB_NARROW
    if not wide and V > MAX_VOCAB_NARROW:
        raise _lib.PgasrError(f"{what}: V = {V} > {MAX_VOCAB_NARROW} needs the wide entry")
    return bool(wide)


def _ctc_call(log_probs, targets, input_lengths, target_lengths, blank, utt_scale=None, pg_coef=None, pg_path=None, need_grad=False,
              wide=None):
    """``pgasr_ctc_loss_grad`` (V > 64: ``pgasr_ctc_loss_grad_wide``, the same arguments and workspace) for ``ctc_loss_grad`` and
    ``ctc_lattice``: (nll, grad or None, lattice handle)."""
    lib = _lib.load()
    _req(log_probs, torch.float32, "log_probs")
    T, B, V = log_probs.shape
    _req(targets, torch.int32, "targets"); _req(input_lengths, torch.int32, "input_lengths")
    _req(target_lengths, torch.int32, "target_lengths")
    _req(utt_scale, torch.float32, "utt_scale"); _req(pg_coef, torch.float32, "pg_coef")
    _req(pg_path, torch.int32, "pg_path")
    Lmax = targets.shape[1] if targets.dim() == 2 else 0
    if Lmax == 0:
        targets = torch.zeros(B, 1, dtype=torch.int32, device=log_probs.device)
    nbytes = lib.pgasr_ctc_workspace_bytes(T, B, V, Lmax)
    ws = _workspace(nbytes, log_probs.device, "ctc")
    nll = torch.empty(B, dtype=torch.float32, device=log_probs.device)
    grad = torch.empty_like(log_probs) if need_grad else None
    entry = "pgasr_ctc_loss_grad" + ("_wide" if _wide(V, wide, "ctc_loss_grad") else "")
    st = getattr(lib, entry)(_p(log_probs), _p(targets), _p(input_lengths), _p(target_lengths),
                             T, B, V, Lmax, blank, _p(utt_scale), _p(pg_coef), _p(pg_path),
                             _p(nll), _p(grad), _p(ws), ws.numel(), _stream())
    _lib.check(st, entry)
    return nll, grad, (ws, Lmax, blank)


def ctc_loss_grad(log_probs, targets, input_lengths, target_lengths, blank=0, utt_scale=None,
                  pg_coef=None, pg_path=None, need_grad=True, wide=None):
    """log_probs (T,B,V) fp32, V <= MAX_VOCAB_WIDE; targets (B,Lmax) int32; lengths int32.
    Returns (nll (B,), grad_logits (T,B,V) or None).  wide: None = the wide kernels when V > 64 (``_wide``)."""
    return _ctc_call(log_probs, targets, input_lengths, target_lengths, blank, utt_scale, pg_coef, pg_path, need_grad, wide)[:2]


def ctc_lattice(log_probs, targets, input_lengths, target_lengths, blank=0, wide=None):
    """First half of ``ctc_loss_grad``: alpha/beta lattice only.  Returns (nll (B,), handle); the handle goes to
    ``ctc_grad_from_lattice`` (which may run on another stream once this one's work is ordered before it)."""
    nll, _, handle = _ctc_call(log_probs, targets, input_lengths, target_lengths, blank, wide=wide)
    return nll, handle


def _coef_per_frame(pg_coef, T, B):
    """pg_coef (B,): one coefficient per utterance; (T,B): one per frame (pg_step_coefs)."""
    if pg_coef is None or pg_coef.numel() == B and pg_coef.dim() == 1:
        return 0
    if tuple(pg_coef.shape) != (T, B):
        raise _lib.PgasrError(f"pg_coef must be (B,) or (T,B) = ({B},) / ({T},{B}); got {tuple(pg_coef.shape)}")
    return 1


def _tail(log_probs, ent_scale, ref_log_probs, kl_scale):
    """The optional terms of a gradient pass, checked: 0 = none, 1 = the entropy term, 2 = the KL term (with or without entropy).
    ent_scale (B) fp32 (``frame_entropy``): adds ent_scale_b p (ln p + H) in the same pass.
    ref_log_probs (T,B,V), kl_scale (B) fp32 (``frame_kl``), both or neither: adds kl_scale_b p (ln p - lnq - KL) after it."""
    B = log_probs.shape[1]
    if ent_scale is not None:
        _req(ent_scale, torch.float32, "ent_scale")
        if tuple(ent_scale.shape) != (B,):
            raise _lib.PgasrError(f"ent_scale must be ({B},); got {tuple(ent_scale.shape)}")
    if ref_log_probs is None and kl_scale is None:
        return 0 if ent_scale is None else 1
    if ref_log_probs is None or kl_scale is None:
        raise _lib.PgasrError("the KL term takes ref_log_probs and kl_scale together")
    _req(ref_log_probs, torch.float32, "ref_log_probs"); _req(kl_scale, torch.float32, "kl_scale")
    if ref_log_probs.shape != log_probs.shape or tuple(kl_scale.shape) != (B,):
        raise _lib.PgasrError(f"ref_log_probs must be {tuple(log_probs.shape)} and kl_scale ({B},); got "
                              f"{tuple(ref_log_probs.shape)} and {tuple(kl_scale.shape)}")
    return 2


# how many of (ent_scale, ref_log_probs, kl_scale) a narrow family's entry takes, by ``_tail``'s number: X, X_ent, X_kl (ent_scale
# NULL there when it is None).  A wide entry takes all three as nullable pointers.
_TAIL_ENTRY = (("", 0), ("_ent", 1), ("_kl", 3))


def _grad_pass(entry, log_probs, input_lengths, target_lengths, handle, utt_scale, mid, hyp_handle=None, label=None,
               nullable_tails=False, ent_scale=None, ref_log_probs=None, kl_scale=None):
    """Every ``ctc_grad_from_lattice*`` wrapper: entry(log-probs, lengths, shapes, blank, utt_scale, *mid, *tails, grad, workspace,
    [hypothesis workspace,] stream) into a fresh (T,B,V) gradient.  mid: what the entry point takes between utt_scale and the tails,
    by name, tensors as tensors (``*coef`` fp32, the others int32); label: the launch's ``_timed`` name; nullable_tails: the entry
    takes ent_scale, ref_log_probs and kl_scale as three nullable pointers, else it is the first of a narrow family whose ``_ent`` /
    ``_kl`` form the terms select (``_TAIL_ENTRY``).  hyp_handle: ``ctc_hyp_lattice``'s, for the entries with two workspaces."""
    lib = _lib.load()
    ws, Lmax, blank = handle
    T, B, V = log_probs.shape
    _req(log_probs, torch.float32, "log_probs"); _req(utt_scale, torch.float32, "utt_scale")
    for name, a in mid.items():
        if not isinstance(a, int):
            _req(a, torch.float32 if name.endswith("coef") else torch.int32, name)
    ws_tail = ()
    if hyp_handle is not None:
        hws, K, Lh = hyp_handle
        _req(input_lengths, torch.int32, "input_lengths"); _req(target_lengths, torch.int32, "target_lengths")
        if input_lengths.numel() != B or target_lengths.numel() != B or (utt_scale is not None and utt_scale.numel() != B):
            raise _lib.PgasrError(f"input_lengths, target_lengths and utt_scale must hold {B} utterances")
        # the handles say nothing of T and B: the lattices must at least fit the workspaces they name
        need = lib.pgasr_ctc_workspace_bytes(T, B, V, Lmax)
        need_h = getattr(lib, "pgasr_ctc_hyp_workspace_bytes" + ("_wide" if entry.endswith("_wide") else ""))(T, B, V, K, Lh)
        if need_h == 0 or ws.numel() < need or hws.numel() < need_h:
            raise _lib.PgasrError(f"the lattice handles were not made for log_probs {tuple(log_probs.shape)} with K = {K}, Lh = {Lh}: "
                                  f"workspaces of {ws.numel()} and {hws.numel()} bytes, {need} and {need_h} needed")
        ws_tail = (_p(hws), hws.numel())
    tail = _tail(log_probs, ent_scale, ref_log_probs, kl_scale)
    suffix, ntail = ("", 3) if nullable_tails else _TAIL_ENTRY[tail]
    grad = torch.empty_like(log_probs)
    with _timed(label):
        st = getattr(lib, entry + suffix)(_p(log_probs), _p(input_lengths), _p(target_lengths), T, B, V, Lmax, blank, _p(utt_scale),
                                          *(a if isinstance(a, int) else _p(a) for a in mid.values()),
                                          *(_p(a) for a in (ent_scale, ref_log_probs, kl_scale)[:ntail]),
                                          _p(grad), _p(ws), ws.numel(), *ws_tail, _stream())
    _lib.check(st, entry + suffix)
    return grad


def _loss_value(entry, log_probs, paths, paths_name, input_lengths, nll, utt_scale, pg_coef, K=(), mid=(), tail=()):
    """The three ``pg_loss_value*`` wrappers: entry(log_probs, paths, *K, input_lengths, nll, utt_scale, pg_coef, *mid, T, B, V,
    *tail, terms, stream) -> terms (B,) fp32."""
    lib = _lib.load()
    T, B, V = log_probs.shape
    _req(log_probs, torch.float32, "log_probs"); _req(paths, torch.int32, paths_name); _req(nll, torch.float32, "nll")
    _req(utt_scale, torch.float32, "utt_scale"); _req(pg_coef, torch.float32, "pg_coef")
    terms = torch.empty(B, dtype=torch.float32, device=log_probs.device)
    st = getattr(lib, entry)(_p(log_probs), _p(paths), *K, _p(input_lengths), _p(nll), _p(utt_scale), _p(pg_coef), *mid,
                             T, B, V, *tail, _p(terms), _stream())
    _lib.check(st, entry)
    return terms


def ctc_grad_from_lattice(log_probs, input_lengths, target_lengths, handle, utt_scale=None, pg_coef=None, pg_path=None,
                          ent_scale=None, ref_log_probs=None, kl_scale=None, wide=None):
    """ent_scale (B): add the entropy term of ``frame_entropy`` in the same pass (``_grad_pass``), here and in the two wrappers below.
    ref_log_probs (T,B,V), kl_scale (B): add the KL term of ``frame_kl`` after it, likewise.
    V > 64 (or wide=True): ``pgasr_ctc_grad_from_lattice_wide``, which has no entropy or KL form."""
    T, B, V = log_probs.shape
    tail = "_wide" if _wide(V, wide, "ctc_grad_from_lattice") else ""
    if tail and (ent_scale is not None or ref_log_probs is not None or kl_scale is not None):
        raise _lib.PgasrError(f"ctc_grad_from_lattice: the entropy and KL terms take at most {MAX_VOCAB_NARROW} symbols (V = {V}); "
                              f"ctc_grad_from_lattice_multi has them for wide rows")
    return _grad_pass("pgasr_ctc_grad_from_lattice" + tail, log_probs, input_lengths, target_lengths, handle, utt_scale,
                      dict(pg_coef=pg_coef, pg_path=pg_path, per_frame=_coef_per_frame(pg_coef, T, B)), ent_scale=ent_scale,
                      ref_log_probs=ref_log_probs, kl_scale=kl_scale)


def frame_kl(log_probs, ref_log_probs, input_lengths, kl_weight=0.0, inv_global_batch=1.0, wide=None):
    """The KL of the frame policy from a frozen reference policy (``pgasr_frame_kl``): log_probs, ref_log_probs (T,B,V) fp32,
    input_lengths (B) int32 -> (kl_mean (B), kl_scale (B)) fp32 in one launch: kl_mean[b] = the MEAN over the utterance's own frames of
    KL(p || q) = sum_v p (ln p - max(ln q, -104)) (nats; 0 for an empty utterance, not clamped at 0), kl_scale[b] =
    kl_weight * inv_global_batch / max(T_b,1), what the gradient passes take as ``kl_scale``.  Deterministic; symbols with p = 0 add
    exactly 0 and a zero reference probability costs the floor, never inf.
    V > 64 (or wide=True): ``pgasr_frame_kl_wide``, the same arguments and sums."""
    lib = _lib.load()
    _req(log_probs, torch.float32, "log_probs"); _req(ref_log_probs, torch.float32, "ref_log_probs")
    _req(input_lengths, torch.int32, "input_lengths")
    if log_probs.dim() != 3 or ref_log_probs.shape != log_probs.shape or input_lengths.numel() != log_probs.shape[1]:
        raise _lib.PgasrError("frame_kl wants log_probs and ref_log_probs (T,B,V) and input_lengths (B,)")
    T, B, V = log_probs.shape
    out = torch.empty(2, B, dtype=torch.float32, device=log_probs.device)
    entry = "pgasr_frame_kl_wide" if _wide(V, wide, "frame_kl") else "pgasr_frame_kl"
    with _timed("frame_kl_kernel"):
        st = getattr(lib, entry)(_p(log_probs), _p(ref_log_probs), _p(input_lengths), T, B, V, float(kl_weight),
                                 float(inv_global_batch), out[0].data_ptr(), out[1].data_ptr(), _stream())
    _lib.check(st, entry)
    return out[0], out[1]


def frame_entropy(log_probs, input_lengths, entropy_weight=0.0, inv_global_batch=1.0, wide=None):
    """The entropy of the frame policy (``pgasr_frame_entropy``): log_probs (T,B,V) fp32, input_lengths (B) int32 ->
    (ent_mean (B), ent_scale (B)) fp32 in one launch: ent_mean[b] = the MEAN over the utterance's own frames of
    H = -sum_v p ln p (nats; 0 for an empty utterance), ent_scale[b] = entropy_weight * inv_global_batch / max(T_b,1), what the
    gradient passes take as ``ent_scale``.  Deterministic; -inf entries add exactly 0.
    V > 64 (or wide=True): ``pgasr_frame_entropy_wide``, the same arguments and sums."""
    lib = _lib.load()
    _req(log_probs, torch.float32, "log_probs"); _req(input_lengths, torch.int32, "input_lengths")
    if log_probs.dim() != 3 or input_lengths.numel() != log_probs.shape[1]:
        raise _lib.PgasrError("frame_entropy wants log_probs (T,B,V) and input_lengths (B,)")
    T, B, V = log_probs.shape
    out = torch.empty(2, B, dtype=torch.float32, device=log_probs.device)
    entry = "pgasr_frame_entropy_wide" if _wide(V, wide, "frame_entropy") else "pgasr_frame_entropy"
    with _timed("frame_entropy_kernel"):
        st = getattr(lib, entry)(_p(log_probs), _p(input_lengths), T, B, V, float(entropy_weight), float(inv_global_batch),
                                 out[0].data_ptr(), out[1].data_ptr(), _stream())
    _lib.check(st, entry)
    return out[0], out[1]


def pg_rewards(dist, target_lengths, lam, inv_global_batch):
    """dist (2B,) int32 [greedy..., sampled...] -> (R_greedy, R_sample, pg_coef, utt_scale), each (B,) fp32."""
    lib = _lib.load()
    _req(dist, torch.int32, "dist"); _req(target_lengths, torch.int32, "target_lengths")
    B = target_lengths.numel()
    if dist.numel() != 2 * B:
        raise _lib.PgasrError("pg_rewards wants 2*B distances")
    out = torch.empty(4, B, dtype=torch.float32, device=dist.device)
    st = lib.pgasr_pg_rewards(_p(dist), _p(target_lengths), B, float(lam), float(inv_global_batch),
                              out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), _stream())
    _lib.check(st, "pgasr_pg_rewards")
    return out[0], out[1], out[2], out[3]


def pg_loss_value(log_probs, path, input_lengths, nll, utt_scale, pg_coef):
    """Per-utterance value of the objective (see include/pgasr_hip.h); sum() it for the loss."""
    T, B, _ = log_probs.shape
    return _loss_value("pgasr_pg_loss_value", log_probs, path, "path", input_lengths, nll, utt_scale, pg_coef,
                       tail=(_coef_per_frame(pg_coef, T, B),))


# ---- multi-sample REINFORCE (include/pgasr_hip.h: K sampled paths per utterance, hypothesis or leave-one-out baseline) ----
MAX_SAMPLES = 16                 # PGASR_MAX_SAMPLES
BASELINES = {"hypothesis": 0, "leave_one_out": 1}


def ctc_grad_from_lattice_multi(log_probs, input_lengths, target_lengths, handle, utt_scale, pg_coef, pg_paths, ent_scale=None,
                                ref_log_probs=None, kl_scale=None, wide=None):
    """``ctc_grad_from_lattice`` with K sampled paths: pg_paths (K,T,B) int32, pg_coef (K,B) fp32; the K REINFORCE terms are
    added in k order after the CTC part, in the same pass.
    V > 64 (or wide=True): ``pgasr_ctc_grad_from_lattice_multi_wide``, ONE entry that takes ent_scale, ref_log_probs and kl_scale as
    nullable pointers where the narrow family has three.
    pg_coef (K,T,B), one coefficient per sample and frame (``pg_step_coefs_multi``): ``pgasr_ctc_grad_from_lattice_multi_steps``, one
    entry for every V <= 1024 with nullable tails (the form is chosen by the shape, as ``_coef_per_frame`` does for one path)."""
    T, B, V = log_probs.shape
    K = pg_paths.shape[0]
    # one coefficient per sample and frame (pg_step_coefs_multi): ONE entry for every V, which picks the kernel family by V
    steps = pg_paths.dim() == 3 and tuple(pg_paths.shape[1:]) == (T, B) and tuple(pg_coef.shape) == (K, T, B)
    if not steps and (pg_paths.dim() != 3 or tuple(pg_paths.shape[1:]) != (T, B) or tuple(pg_coef.shape) != (K, B)):
        raise _lib.PgasrError(f"ctc_grad_from_lattice_multi wants pg_paths (K,{T},{B}) and pg_coef (K,{B}) or (K,{T},{B})")
    tail = "_wide" if _wide(V, wide, "ctc_grad_from_lattice_multi") else ""
    return _grad_pass("pgasr_ctc_grad_from_lattice_multi" + ("_steps" if steps else tail), log_probs, input_lengths, target_lengths,
                      handle, utt_scale, dict(K=K, pg_coef=pg_coef, pg_paths=pg_paths), nullable_tails=steps or bool(tail),
                      ent_scale=ent_scale, ref_log_probs=ref_log_probs, kl_scale=kl_scale)


def pg_rewards_multi(dist, target_lengths, num_samples, lam, inv_global_batch, baseline="hypothesis", reward_lengths=None):
    """dist ((H+K)*B,) int32: [hypothesis row (H = 1, baseline "hypothesis" only), sample 0, .., sample K-1] x B ->
    (R_baseline (B), R_sample (K,B), pg_coef (K,B), utt_scale (B)) fp32.
    reward_lengths (B,) int32: normalise the rewards by these (the word counts of the word-level reward) instead of target_lengths,
    which keep normalising utt_scale (pgasr_pg_rewards_multi_ex)."""
    lib = _lib.load()
    _req(dist, torch.int32, "dist"); _req(target_lengths, torch.int32, "target_lengths")
    _req(reward_lengths, torch.int32, "reward_lengths")
    if baseline not in BASELINES:
        raise ValueError(f"baseline must be one of {sorted(BASELINES)}")
    B, K = target_lengths.numel(), int(num_samples)
    H = 1 if baseline == "hypothesis" else 0
    if dist.numel() != (H + K) * B:
        raise _lib.PgasrError(f"pg_rewards_multi wants {(H + K)} x B distances")
    if reward_lengths is not None and reward_lengths.numel() != B:
        raise _lib.PgasrError(f"pg_rewards_multi wants reward_lengths of {B} utterances")
    out = torch.empty(2 * K + 2, B, dtype=torch.float32, device=dist.device)
    R_b, R_s, coef, utt_scale = out[0], out[1:K + 1], out[K + 1:2 * K + 1], out[2 * K + 1]
    if reward_lengths is None:
        st = lib.pgasr_pg_rewards_multi(_p(dist), _p(target_lengths), B, K, BASELINES[baseline], float(lam), float(inv_global_batch),
                                        R_b.data_ptr(), R_s.data_ptr(), coef.data_ptr(), utt_scale.data_ptr(), _stream())
        _lib.check(st, "pgasr_pg_rewards_multi")
    else:
        st = lib.pgasr_pg_rewards_multi_ex(_p(dist), _p(reward_lengths), _p(target_lengths), B, K, BASELINES[baseline], float(lam),
                                           float(inv_global_batch), R_b.data_ptr(), R_s.data_ptr(), coef.data_ptr(),
                                           utt_scale.data_ptr(), _stream())
        _lib.check(st, "pgasr_pg_rewards_multi_ex")
    return R_b, R_s, coef, utt_scale


def pg_loss_value_multi(log_probs, paths, input_lengths, nll, utt_scale, pg_coef):
    """Per-utterance value of the multi-sample objective, paths (K,T,B), pg_coef (K,B) -- or (K,T,B), one coefficient per sample and
    frame (``pgasr_pg_loss_value_multi_steps``); sum() it for the loss."""
    T, B, _ = log_probs.shape
    K = paths.shape[0]
    if paths.dim() == 3 and tuple(paths.shape[1:]) == (T, B) and tuple(pg_coef.shape) == (K, T, B):
        # one coefficient per sample and frame (pg_step_coefs_multi)
        return _loss_value("pgasr_pg_loss_value_multi_steps", log_probs, paths, "paths", input_lengths, nll, utt_scale, pg_coef, K=(K,))
    if paths.dim() != 3 or tuple(paths.shape[1:]) != (T, B) or tuple(pg_coef.shape) != (K, B):
        raise _lib.PgasrError(f"pg_loss_value_multi wants paths (K,{T},{B}) and pg_coef (K,{B}) or (K,{T},{B})")
    return _loss_value("pgasr_pg_loss_value_multi", log_probs, paths, "paths", input_lengths, nll, utt_scale, pg_coef, K=(K,))


# ---- sequence-level REINFORCE (include/pgasr_hip.h: the score function of a sample is the CTC likelihood of its hypothesis) ----
SCORE_FUNCTIONS = ("path", "sequence")
MAX_HYP_LEN = 1023               # the lattice's 2L+1 <= 2048 states


def hyp_len_cap(T, max_hyp_len=None):
    """Lh = min(T, MAX_HYP_LEN, max_hyp_len if given): hypotheses of at most Lh tokens are sequence-scored."""
    return min(int(T), MAX_HYP_LEN) if max_hyp_len is None else min(int(T), MAX_HYP_LEN, int(max_hyp_len))


def ctc_hyp_workspace_bytes(T, B, V, K, Lh, wide=None):
    """Bytes of the K*B hypothesis lattices: 2 * K*B*T * roundup64(2*Lh+1) * 4 plus the per-pair tables.
    V > 64 (or wide=True): ``pgasr_ctc_hyp_workspace_bytes_wide``, the same layout for V <= 1024."""
    tail = "_wide" if _wide(V, wide, "ctc_hyp_workspace_bytes") else ""
    return int(getattr(_lib.load(), "pgasr_ctc_hyp_workspace_bytes" + tail)(T, B, V, K, Lh))


def ctc_hyp_lattice(log_probs, hyp_tokens, hyp_len, input_lengths, Lh, blank=0, wide=None):
    """The CTC lattices of the K sampled hypotheses of every utterance over the SAME log-prob rows: log_probs (T,B,V),
    hyp_tokens (K,B,stride) / hyp_len (K,B) int32 as ``ctc_collapse`` returns them.  Pairs with hyp_len > Lh are skipped.
    Returns (hyp_nll (K,B) fp32 -- 0 for a skipped pair --, handle); the handle goes to ``ctc_grad_from_lattices_seq``.
    The lattices live in a cached workspace of ``ctc_hyp_workspace_bytes(T, B, V, K, Lh)`` bytes (tag "ctc_hyp").
    V > 64 (or wide=True): ``pgasr_ctc_hyp_lattice_wide`` (include/pgasr_hip.h, A13-WIDE) -- the same sweeps, arguments and
    workspace, the label lists built for V <= 1024."""
    lib = _lib.load()
    _req(log_probs, torch.float32, "log_probs"); _req(hyp_tokens, torch.int32, "hyp_tokens")
    _req(hyp_len, torch.int32, "hyp_len"); _req(input_lengths, torch.int32, "input_lengths")
    T, B, V = log_probs.shape
    if hyp_tokens.dim() != 3 or hyp_tokens.shape[1] != B or tuple(hyp_len.shape) != (hyp_tokens.shape[0], B):
        raise _lib.PgasrError(f"ctc_hyp_lattice wants hyp_tokens (K,{B},stride) and hyp_len (K,{B})")
    K, stride, Lh = hyp_tokens.shape[0], hyp_tokens.shape[2], int(Lh)
    tail = "_wide" if _wide(V, wide, "ctc_hyp_lattice") else ""
    nbytes = getattr(lib, "pgasr_ctc_hyp_workspace_bytes" + tail)(T, B, V, K, Lh)
    ws = _workspace(nbytes, log_probs.device, "ctc_hyp")
    hyp_nll = torch.empty(K, B, dtype=torch.float32, device=log_probs.device)
    with _timed("ctc_hyp_lattice_kernel"):
        st = getattr(lib, "pgasr_ctc_hyp_lattice" + tail)(_p(log_probs), _p(hyp_tokens), stride, _p(hyp_len), _p(input_lengths), T, B, V,
                                                          K, Lh, blank, _p(hyp_nll), _p(ws), ws.numel(), _stream())
    _lib.check(st, "pgasr_ctc_hyp_lattice" + tail)
    return hyp_nll, (ws, K, Lh)


def ctc_hyp_score(log_probs, hyp_tokens, hyp_len, input_lengths, Lh, count=None, blank=0):
    """The exact CTC -log p(y|x) of every hypothesis of an N-best list, forward sweep only (pgasr_ctc_hyp_score; include/pgasr_hip.h,
    A12-SCORE): log_probs (T,B,V) fp32 with V <= 1024, hyp_tokens (N,B,stride) / hyp_len (N,B) int32 as ``ctc_beam_search_nbest`` /
    ``ctc_beam_search_wide`` return them, N <= 128, count (B) int32 or None (every row).  Returns nll (N,B) float64: +inf for a row
    beyond count, a hypothesis longer than Lh (or than stride), a token that is the blank or outside [0,V), and where no alignment
    exists.  No workspace, one launch, no host synchronisation; fp64 throughout (``ctc_hyp_lattice``'s nll is fp32)."""
    lib = _lib.load()
    _req(log_probs, torch.float32, "log_probs"); _req(hyp_tokens, torch.int32, "hyp_tokens")
    _req(hyp_len, torch.int32, "hyp_len"); _req(input_lengths, torch.int32, "input_lengths"); _req(count, torch.int32, "count")
    if log_probs.dim() != 3:
        raise _lib.PgasrError("ctc_hyp_score wants log_probs (T,B,V)")
    T, B, V = log_probs.shape
    if hyp_tokens.dim() != 3 or hyp_tokens.shape[1] != B or tuple(hyp_len.shape) != (hyp_tokens.shape[0], B) \
            or input_lengths.numel() != B or (count is not None and count.numel() != B):
        raise _lib.PgasrError(f"ctc_hyp_score wants hyp_tokens (N,{B},stride), hyp_len (N,{B}), input_lengths ({B}) and count ({B})")
    N, stride = hyp_tokens.shape[0], hyp_tokens.shape[2]
    nll = torch.empty(N, B, dtype=torch.float64, device=log_probs.device)
    with _timed("ctc_hyp_score_kernel"):
        st = lib.pgasr_ctc_hyp_score(_p(log_probs), _p(hyp_tokens), stride, _p(hyp_len), _p(count), _p(input_lengths), T, B, V, N,
                                     int(Lh), int(blank), _p(nll), _stream())
    _lib.check(st, "pgasr_ctc_hyp_score")
    return nll


def ctc_grad_from_lattices_seq(log_probs, input_lengths, target_lengths, handle, hyp_handle, utt_scale, pg_coef, pg_paths, hyp_len,
                               ent_scale=None, ref_log_probs=None, kl_scale=None, wide=None):
    """One gradient pass over the target lattice (``ctc_lattice``'s handle) and the K*B hypothesis lattices (``ctc_hyp_lattice``'s):
    utt_scale (softmax - occ_target) + sum_k pg_coef[k,b] * (hyp_len[k,b] <= Lh ? softmax - occ_hyp : softmax - onehot(pg_paths[k,t,b])),
    the K terms in k order.  pg_paths (K,T,B) int32, pg_coef (K,B) fp32, hyp_len (K,B) int32.
    V > 64 (or wide=True): ``pgasr_ctc_grad_from_lattices_seq_wide``, ONE entry that takes ent_scale, ref_log_probs and kl_scale as
    nullable pointers where the narrow family has three."""
    hws, K, Lh = hyp_handle
    T, B, V = log_probs.shape
    _req(hyp_len, torch.int32, "hyp_len")
    if tuple(pg_paths.shape) != (K, T, B) or tuple(pg_coef.shape) != (K, B) or tuple(hyp_len.shape) != (K, B):
        raise _lib.PgasrError(f"ctc_grad_from_lattices_seq wants pg_paths ({K},{T},{B}), pg_coef and hyp_len ({K},{B})")
    tail = "_wide" if _wide(V, wide, "ctc_grad_from_lattices_seq") else ""
    return _grad_pass("pgasr_ctc_grad_from_lattices_seq" + tail, log_probs, input_lengths, target_lengths, handle, utt_scale,
                      dict(K=K, pg_coef=pg_coef, pg_paths=pg_paths, hyp_len=hyp_len, Lh=Lh), hyp_handle=hyp_handle,
                      label=f"ctc_grad_seq{tail}_kernel", nullable_tails=bool(tail), ent_scale=ent_scale, ref_log_probs=ref_log_probs,
                      kl_scale=kl_scale)


def pg_loss_value_seq(log_probs, paths, input_lengths, nll, utt_scale, pg_coef, hyp_nll, hyp_len, Lh):
    """Per-utterance value of the sequence-level objective: nll_b utt_scale_b + sum_k pg_coef[k,b] * (hyp_len[k,b] <= Lh ?
    hyp_nll[k,b] : -sum_t log p(paths[k,t,b])); sum() it for the loss."""
    T, B, _ = log_probs.shape
    _req(hyp_nll, torch.float32, "hyp_nll"); _req(hyp_len, torch.int32, "hyp_len")
    K = paths.shape[0]
    if paths.dim() != 3 or tuple(paths.shape[1:]) != (T, B) or any(tuple(t_.shape) != (K, B) for t_ in (pg_coef, hyp_nll, hyp_len)):
        raise _lib.PgasrError(f"pg_loss_value_seq wants paths (K,{T},{B}) and pg_coef, hyp_nll, hyp_len (K,{B})")
    return _loss_value("pgasr_pg_loss_value_seq", log_probs, paths, "paths", input_lengths, nll, utt_scale, pg_coef, K=(K,),
                       mid=(_p(hyp_nll), _p(hyp_len), int(Lh)))


FUSED_HEAD = _os_environ_get("PGASR_FUSED_HEAD", "1") != "0"


def head_logsoftmax_ok(K, V):
    return FUSED_HEAD and V <= 32 and K % 64 == 0 and K <= 1024


def head_logsoftmax(x, weight, bias, want_logits=True):
    """x (rows,K) @ weight (V,K)^T + bias -> (logits or None, log_probs), both (rows,V): the CTC head as one exact-fp32 kernel."""
    lib = _lib.load()
    _req(x, torch.float32, "x"); _req(weight, torch.float32, "weight"); _req(bias, torch.float32, "bias")
    rows, K = x.shape
    V = weight.shape[0]
    logits = torch.empty(rows, V, dtype=torch.float32, device=x.device) if want_logits else None
    lp = torch.empty(rows, V, dtype=torch.float32, device=x.device)
    with _timed("head_logsoftmax"):
        st = lib.pgasr_head_logsoftmax(_p(x), rows, K, x.stride(0), _p(weight), _p(bias), V, _p(logits), _p(lp), _stream())
    _lib.check(st, "pgasr_head_logsoftmax")
    return logits, lp


def pg_step_coefs(paths, input_lengths, prefix_dist, token_lengths, target_lengths, lam, inv_global_batch, blank=0):
    """Per-frame REINFORCE coefficients (T,B) from the per-step rewards (policy_grad.py:10-15; include/pgasr_hip.h):
    paths (2,T,B) greedy then sampled frame labels, prefix_dist (2B, P) / token_lengths (2B) of their collapsed forms."""
    lib = _lib.load()
    _req(paths, torch.int32, "paths"); _req(prefix_dist, torch.int32, "prefix_dist"); _req(token_lengths, torch.int32, "token_lengths")
    _req(input_lengths, torch.int32, "input_lengths"); _req(target_lengths, torch.int32, "target_lengths")
    two, T, B = paths.shape
    if two != 2 or prefix_dist.shape[0] != 2 * B or token_lengths.numel() != 2 * B or target_lengths.numel() != B:
        raise _lib.PgasrError("pg_step_coefs wants paths (2,T,B), prefix_dist (2B,P), token_lengths (2B,), target_lengths (B,)")
    coef = torch.empty(T, B, dtype=torch.float32, device=paths.device)
    st = lib.pgasr_pg_step_coefs(_p(paths), _p(input_lengths), _p(prefix_dist), prefix_dist.shape[1], _p(token_lengths),
                                 _p(target_lengths), T, B, int(blank), float(lam), float(inv_global_batch), _p(coef), _stream())
    _lib.check(st, "pgasr_pg_step_coefs")
    return coef


def pg_step_coefs_multi(paths, input_lengths, prefix_dist, token_lengths, target_lengths, num_samples, lam, inv_global_batch,
                        baseline="hypothesis", blank=0):
    """Per-frame REINFORCE coefficients (K,T,B) of K sampled paths (``pgasr_pg_step_coefs_multi``; include/pgasr_hip.h, A12-STEP):
    paths (P,T,B) frame labels -- the greedy path then the K samples (baseline "hypothesis", P = K + 1), or the K samples
    ("leave_one_out", P = K) --, prefix_dist (P*B, stride) / token_lengths (P*B) of their collapsed forms.  K = 1 with the hypothesis
    baseline gives ``pg_step_coefs``' words as (1,T,B)."""
    lib = _lib.load()
    _req(paths, torch.int32, "paths"); _req(prefix_dist, torch.int32, "prefix_dist"); _req(token_lengths, torch.int32, "token_lengths")
    _req(input_lengths, torch.int32, "input_lengths"); _req(target_lengths, torch.int32, "target_lengths")
    if baseline not in BASELINES:
        raise ValueError(f"baseline must be one of {sorted(BASELINES)}")
    K = int(num_samples)
    P = K + (1 if baseline == "hypothesis" else 0)
    if (paths.dim() != 3 or paths.shape[0] != P or prefix_dist.dim() != 2 or prefix_dist.shape[0] != P * paths.shape[2]
            or token_lengths.numel() != P * paths.shape[2] or target_lengths.numel() != paths.shape[2]
            or input_lengths.numel() != paths.shape[2]):
        raise _lib.PgasrError(f"pg_step_coefs_multi wants paths ({P},T,B), prefix_dist ({P}*B,stride), token_lengths ({P}*B,), "
                              f"input_lengths and target_lengths (B,)")
    _, T, B = paths.shape
    coef = torch.empty(K, T, B, dtype=torch.float32, device=paths.device)
    st = lib.pgasr_pg_step_coefs_multi(_p(paths), _p(input_lengths), _p(prefix_dist), prefix_dist.shape[1], _p(token_lengths),
                                       _p(target_lengths), T, B, K, BASELINES[baseline], int(blank), float(lam),
                                       float(inv_global_batch), _p(coef), _stream())
    _lib.check(st, "pgasr_pg_step_coefs_multi")
    return coef


def _check_utt_ids(utt_ids, B, T, batch_stride, device, what):
    """The id form's arguments: (B) int32 on the scores' device, a global batch >= 1 whose counters fit Philox word 0."""
    _req(utt_ids, torch.int32, "utt_ids")
    if utt_ids.dim() != 1 or utt_ids.numel() != B or utt_ids.device != device:
        raise _lib.PgasrError(f"{what}: utt_ids must be ({B},) int32 on {device}")
    if int(batch_stride) < 1:
        raise ValueError(f"{what}: utt_ids needs batch_stride, the global batch (>= 1)")
    if T * int(batch_stride) > 2 ** 32:
        raise ValueError(f"{what}: T * batch_stride = {T} * {int(batch_stride)} > 2^32: the sampler's counter word is 32 bits")


def frame_argmax_sample(scores, seed=0, offset=0, want_greedy=True, want_sample=True, batch_stride=0, batch_offset=0, utt_ids=None,
                        wide=None):
    """batch_stride / batch_offset: the GLOBAL batch and this shard's first utterance in it (data parallel: N ranks with
    one seed then draw what one process holding the whole batch draws); 0 / 0 = the local batch is the whole batch.
    utt_ids (B) int32 on the device, with batch_stride: row b's global index instead of batch_offset + b (an id < 0 or >=
    batch_stride: a row beyond the global batch; pgasr_frame_argmax_sample_ids).
    V > 64 (or wide=True): ``pgasr_frame_argmax_sample_wide``, one entry for both addressings, the same draws."""
    lib = _lib.load()
    _req(scores, torch.float32, "scores")
    T, B, V = scores.shape
    if utt_ids is not None:
        _check_utt_ids(utt_ids, B, T, batch_stride, scores.device, "frame_argmax_sample")
    g = torch.empty(T, B, dtype=torch.int32, device=scores.device) if want_greedy else None
    s = torch.empty(T, B, dtype=torch.int32, device=scores.device) if want_sample else None
    if _wide(V, wide, "frame_argmax_sample"):
        with _timed("frame_argmax_sample_wide"):
            st = lib.pgasr_frame_argmax_sample_wide(_p(scores), T, B, V, int(seed) & (2 ** 64 - 1), int(offset) & 0xFFFFFFFF,
                                                    int(batch_stride), 0 if utt_ids is not None else int(batch_offset), _p(utt_ids),
                                                    _p(g), _p(s), _stream())
        _lib.check(st, "pgasr_frame_argmax_sample_wide")
        return g, s
    if utt_ids is not None:
        with _timed("frame_argmax_sample"):
            st = lib.pgasr_frame_argmax_sample_ids(_p(scores), T, B, V, int(seed) & (2 ** 64 - 1), int(offset) & 0xFFFFFFFF,
                                                   int(batch_stride), _p(utt_ids), _p(g), _p(s), _stream())
        _lib.check(st, "pgasr_frame_argmax_sample_ids")
        return g, s
    with _timed("frame_argmax_sample"):
        st = lib.pgasr_frame_argmax_sample(_p(scores), T, B, V, int(seed) & (2 ** 64 - 1), int(offset) & 0xFFFFFFFF,
                                           int(batch_stride), int(batch_offset), _p(g), _p(s), _stream())
    _lib.check(st, "pgasr_frame_argmax_sample")
    return g, s


def frame_sample_multi(scores, num_samples, seed=0, offset=0, want_greedy=False, batch_stride=0, batch_offset=0, out=None,
                       utt_ids=None, wide=None):
    """K draws per frame (include/pgasr_hip.h, pgasr_frame_sample_multi): returns (greedy (T,B) or None, samples (K,T,B)) int32.
    Draw 0 is ``frame_argmax_sample``'s sample; batch_stride / batch_offset / utt_ids as there.  out = (greedy or None, samples) to
    write into (contiguous int32).
    V > 64 (or wide=True): ``pgasr_frame_sample_multi_wide``, one entry for both addressings, the same draws."""
    lib = _lib.load()
    _req(scores, torch.float32, "scores")
    T, B, V = scores.shape
    K = int(num_samples)
    if utt_ids is not None:
        _check_utt_ids(utt_ids, B, T, batch_stride, scores.device, "frame_sample_multi")
    if out is not None:
        g, s = out
        _req(g, torch.int32, "out greedy"); _req(s, torch.int32, "out samples")
        if tuple(s.shape) != (K, T, B) or (g is not None and tuple(g.shape) != (T, B)):
            raise _lib.PgasrError(f"frame_sample_multi: out tensors must be ({T},{B}) and ({K},{T},{B}) int32")
    else:
        g = torch.empty(T, B, dtype=torch.int32, device=scores.device) if want_greedy else None
        s = torch.empty(K, T, B, dtype=torch.int32, device=scores.device)
    if _wide(V, wide, "frame_sample_multi"):
        with _timed("frame_sample_multi_wide"):
            st = lib.pgasr_frame_sample_multi_wide(_p(scores), T, B, V, K, int(seed) & (2 ** 64 - 1), int(offset) & 0xFFFFFFFF,
                                                   int(batch_stride), 0 if utt_ids is not None else int(batch_offset), _p(utt_ids),
                                                   _p(g), _p(s), _stream())
        _lib.check(st, "pgasr_frame_sample_multi_wide")
        return g, s
    if utt_ids is not None:
        with _timed("frame_sample_multi"):
            st = lib.pgasr_frame_sample_multi_ids(_p(scores), T, B, V, K, int(seed) & (2 ** 64 - 1), int(offset) & 0xFFFFFFFF,
                                                  int(batch_stride), _p(utt_ids), _p(g), _p(s), _stream())
        _lib.check(st, "pgasr_frame_sample_multi_ids")
        return g, s
    with _timed("frame_sample_multi"):
        st = lib.pgasr_frame_sample_multi(_p(scores), T, B, V, K, int(seed) & (2 ** 64 - 1), int(offset) & 0xFFFFFFFF,
                                          int(batch_stride), int(batch_offset), _p(g), _p(s), _stream())
    _lib.check(st, "pgasr_frame_sample_multi")
    return g, s


def batch_prep(fmask, tmask, targets):
    """The collated batch (model.py:227-230) -> (in_len (B) int32, tg_len (B) int32, targets (B,L) int32) in one launch."""
    lib = _lib.load()
    _req(fmask, torch.float32, "fmask"); _req(tmask, torch.int64, "tmask"); _req(targets, torch.int64, "targets")
    B, T = fmask.shape
    L = targets.shape[1]
    if tuple(tmask.shape) != (B, L) or targets.shape[0] != B:
        raise _lib.PgasrError("batch_prep: fmask (B,T), tmask (B,L), targets (B,L)")
    dev = fmask.device
    in_len = torch.empty(B, dtype=torch.int32, device=dev)
    tg_len = torch.empty(B, dtype=torch.int32, device=dev)
    tg32 = torch.empty(B, L, dtype=torch.int32, device=dev)
    _lib.check(lib.pgasr_batch_prep(_p(fmask), B, T, _p(tmask), _p(targets), L, _p(in_len), _p(tg_len), _p(tg32), _stream()), "pgasr_batch_prep")
    return in_len, tg_len, tg32


SPECAUG_FILLS = {"row_mean": 0, "zero": 1}      # PGASR_SPECAUG_FILL_*
SPECAUG_MAX_MASKS = 8                           # csrc/specaug.hip: masks of a kind


def spec_augment(x, lengths, policy, seed, offset, utt_ids=None, batch_offset=0, out=None, want_masks=False):
    """SpecAugment masking of x (B,F,T) fp32 (include/pgasr_hip.h, A0-AUG): ``policy`` holds freq_masks, freq_width, time_masks,
    time_width, time_ratio and fill (features.SpecAugment); lengths (B) int32 on the device.  The intervals are a function of
    (seed, offset, the row's global utterance index): utt_ids (B) int32 on the device, or batch_offset + b.  Returns the masked
    tensor -- a new one, ``out`` (contiguous fp32 of x's shape), or x itself with ``out=x`` -- and with ``want_masks`` also the
    (B, freq_masks + time_masks, 2) int32 tensor of (start, width), frequency masks first.  No host synchronisation."""
    lib = _lib.load()
    _req(x, torch.float32, "x"); _req(lengths, torch.int32, "lengths"); _req(utt_ids, torch.int32, "utt_ids"); _req(out, torch.float32, "out")
    if x.dim() != 3 or lengths.dim() != 1 or lengths.numel() != x.shape[0] or lengths.device != x.device:
        raise _lib.PgasrError("spec_augment wants x (B,F,T) and lengths (B) on one device")
    B, F, T = x.shape
    if utt_ids is not None and (utt_ids.dim() != 1 or utt_ids.numel() != B or utt_ids.device != x.device):
        raise _lib.PgasrError(f"spec_augment: utt_ids must be ({B},) int32 on {x.device}")
    if out is None:
        out = torch.empty_like(x)
    elif tuple(out.shape) != (B, F, T) or out.device != x.device:
        raise _lib.PgasrError(f"spec_augment: out must be ({B},{F},{T}) fp32 on {x.device}")
    if policy.fill not in SPECAUG_FILLS:
        raise ValueError(f"spec_augment: fill must be one of {sorted(SPECAUG_FILLS)} (got {policy.fill!r})")
    nF, nT = int(policy.freq_masks), int(policy.time_masks)
    ratio = 1.0 if policy.time_ratio is None else float(policy.time_ratio)
    masks = torch.empty(B, nF + nT, 2, dtype=torch.int32, device=x.device) if want_masks else None
    with _timed("spec_augment"):
        st = lib.pgasr_spec_augment(_p(x), _p(lengths), _p(utt_ids), int(batch_offset), B, F, T, nF, int(policy.freq_width), nT,
                                    int(policy.time_width), ratio, SPECAUG_FILLS[policy.fill], int(seed) & (2 ** 64 - 1),
                                    int(offset) & 0xFFFFFFFF, _p(out), _p(masks), _stream())
    _lib.check(st, "pgasr_spec_augment")
    return (out, masks) if want_masks else out


FRAME_STACK_MAX, FRAME_STACK_MAX_ROWS, FRAME_STACK_MAX_BATCH = 16, 65535, 65535      # csrc/frame_stack.hip: stack and skip; stack * F; B


def frame_stack_check(stack, skip, left, what="frame_stack"):
    """(stack, skip, left) as python ints; TypeError / ValueError with the reason unless they lie within the kernel's limits
    (include/pgasr_hip.h, A0-LFR): 1 <= stack, skip <= 16, 0 <= left < stack."""
    import numbers
    for k, v in (("stack", stack), ("skip", skip), ("left", left)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise TypeError(f"{what}: {k} must be an integer (got {v!r})")
    stack, skip, left = int(stack), int(skip), int(left)
    if not 1 <= stack <= FRAME_STACK_MAX:
        raise ValueError(f"{what}: stack must lie in [1, {FRAME_STACK_MAX}] (got {stack})")
    if not 1 <= skip <= FRAME_STACK_MAX:
        raise ValueError(f"{what}: skip must lie in [1, {FRAME_STACK_MAX}] (got {skip})")
    if not 0 <= left < stack:
        raise ValueError(f"{what}: left must lie in [0, stack = {stack}) (got {left})")
    return stack, skip, left


def frame_stack(x, lengths=None, fmask=None, stack=3, skip=3, left=0):
    """Low-frame-rate input (include/pgasr_hip.h, A0-LFR): x (B,F,T) fp32 -> (out (B, stack*F, Tout) fp32, fmask_out (B,1,Tout) fp32,
    n_out (B) int32) with Tout = ceil(T / skip), n_out = ceil(n / skip) and
        out[b, j*F + f, t'] = x[b, f, clamp(t'*skip + j - left, 0, n-1)]  for t' < n_out[b],  0 beyond.
    The frame counts n are ``lengths`` (B) int32 on the device, or the sum of ``fmask`` (B,1,T) / (B,T) (1 / 0; taken on the device),
    or T for every row where both are None.  One launch, no host synchronisation.  A wrong dtype, device, layout or a value beyond
    the limits (1 <= stack, skip <= 16, 0 <= left < stack, stack * F <= 65535, B <= 65535) raises a ValueError that says which."""
    stack, skip, left = frame_stack_check(stack, skip, left)
    if not isinstance(x, torch.Tensor) or x.dim() != 3:
        raise ValueError("frame_stack: x must be a (B,F,T) tensor")
    if not x.is_cuda:
        raise ValueError(f"frame_stack: x must live on the GPU (got {x.device}); there is no CPU path")
    if x.dtype != torch.float32:
        raise ValueError(f"frame_stack: x must be torch.float32 (got {x.dtype})")
    if not x.is_contiguous():
        raise ValueError("frame_stack: x must be contiguous")
    B, F, T = x.shape
    if B < 1 or F < 1 or T < 1:
        raise ValueError(f"frame_stack: x must not be empty (got {tuple(x.shape)})")
    if stack * F > FRAME_STACK_MAX_ROWS:
        raise ValueError(f"frame_stack: stack * F = {stack * F} output rows; at most {FRAME_STACK_MAX_ROWS}")
    if B > FRAME_STACK_MAX_BATCH:
        raise ValueError(f"frame_stack: B = {B}; at most {FRAME_STACK_MAX_BATCH} utterances per call")
    if lengths is not None and fmask is not None:
        raise ValueError("frame_stack: give lengths or fmask, not both")
    if fmask is not None:
        if not isinstance(fmask, torch.Tensor) or fmask.device != x.device or fmask.shape[0] != B or fmask.numel() != B * T:
            raise ValueError(f"frame_stack: fmask must be ({B},1,{T}) or ({B},{T}) on {x.device}")
        lengths = fmask.reshape(B, T).sum(dim=1).to(torch.int32)          # on the device: no host synchronisation
    elif lengths is None:
        lengths = torch.full((B,), T, dtype=torch.int32, device=x.device)
    elif not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int32 or lengths.device != x.device \
            or lengths.dim() != 1 or lengths.numel() != B or not lengths.is_contiguous():
        raise ValueError(f"frame_stack: lengths must be a contiguous ({B},) torch.int32 tensor on {x.device}")
    Tout = (T + skip - 1) // skip
    out = torch.empty(B, stack * F, Tout, dtype=torch.float32, device=x.device)
    fmask_out = torch.empty(B, 1, Tout, dtype=torch.float32, device=x.device)
    n_out = torch.empty(B, dtype=torch.int32, device=x.device)
    lib = _lib.load()
    with _timed("frame_stack"):
        st = lib.pgasr_frame_stack(_p(x), _p(lengths), B, F, T, stack, skip, left, Tout, _p(out), _p(fmask_out), _p(n_out), _stream())
    _lib.check(st, "pgasr_frame_stack")
    return out, fmask_out, n_out


RESAMPLE_MAX_LM, RESAMPLE_MAX_FACTOR, RESAMPLE_MAX_RATIOS = 1024, 16, 8      # csrc/resample.hip

_resample_tables = {}


def _resample_tables_for(ratios, device):
    """(descriptors (n,4) int32 numpy, tables fp32, bases int32 on the device) of a tuple of reduced ratios; built once per device."""
    import numpy as np
    from .features import resample_filter
    key = (str(device), ratios)
    hit = _resample_tables.get(key)
    if hit is None:
        desc, hs, bs, off = [], [], [], 0
        for L, M in ratios:
            h, base, _ = resample_filter(L, M)
            desc.append((L, M, h.shape[1], off))
            pad = -h.size % 4                                  # every table starts on a 16-byte boundary
            hs += [h.reshape(-1), np.zeros(pad, dtype=np.float32)]
            bs.append(base)
            off += h.size + pad
        hit = _resample_tables[key] = (np.ascontiguousarray(np.array(desc, dtype=np.int32)),
                                       torch.from_numpy(np.concatenate(hs)).to(device),
                                       torch.from_numpy(np.concatenate(bs)).to(device))
    return hit


def resample(wave, n_in, ratios, ratio_idx=None, out=None, n_out=None):
    """Sample-rate conversion of wave (B, in_stride) fp32 (include/pgasr_hip.h, A0-RS): row b, n_in[b] samples long (n_in (B) int32 on
    the device), is resampled by ratios[ratio_idx[b]] = (L, M), output rate / input rate, reduced (ratio_idx (B) int32 on the device;
    None: every row takes ratios[0]; at most 8 ratios).  Returns (out (B, out_stride) fp32, zero beyond each row's length, n_out (B)
    int32 = ceil(n_in * L / M)); ``out``: a contiguous fp32 (B, out_stride) tensor with out_stride >= the length the largest ratio
    gives in_stride samples (default: just that, rounded up to 4).  One launch, no host synchronisation."""
    lib = _lib.load()
    _req(wave, torch.float32, "wave"); _req(n_in, torch.int32, "n_in"); _req(ratio_idx, torch.int32, "ratio_idx")
    _req(out, torch.float32, "out"); _req(n_out, torch.int32, "n_out")
    if wave.dim() != 2 or n_in.dim() != 1 or n_in.numel() != wave.shape[0] or n_in.device != wave.device:
        raise _lib.PgasrError("resample wants wave (B, in_stride) and n_in (B) on one device")
    B, in_stride = wave.shape
    ratios = tuple((int(L), int(M)) for L, M in ratios)
    if not 1 <= len(ratios) <= RESAMPLE_MAX_RATIOS:
        raise _lib.PgasrError(f"resample takes 1 .. {RESAMPLE_MAX_RATIOS} ratios per call (got {len(ratios)})")
    if ratio_idx is not None and (ratio_idx.dim() != 1 or ratio_idx.numel() != B or ratio_idx.device != wave.device):
        raise _lib.PgasrError(f"resample: ratio_idx must be ({B},) int32 on {wave.device}")
    desc, tables, bases = _resample_tables_for(ratios, wave.device)
    if out is None:
        need = max((in_stride * L + M - 1) // M for L, M in ratios)
        out = torch.empty(B, (need + 3) // 4 * 4, dtype=torch.float32, device=wave.device)
    elif out.dim() != 2 or out.shape[0] != B or out.device != wave.device:
        raise _lib.PgasrError(f"resample: out must be ({B}, out_stride) fp32 on {wave.device}")
    if n_out is None:
        n_out = torch.empty(B, dtype=torch.int32, device=wave.device)
    elif n_out.dim() != 1 or n_out.numel() != B or n_out.device != wave.device:
        raise _lib.PgasrError(f"resample: n_out must be ({B},) int32 on {wave.device}")
    with _timed("resample"):
        st = lib.pgasr_resample(_p(wave), in_stride, _p(n_in), B, _p(ratio_idx), len(ratios), desc.ctypes.data, _p(tables), _p(bases),
                                _p(out), out.shape[1], _p(n_out), _stream())
    _lib.check(st, "pgasr_resample")
    return out, n_out


REVERB_TILE, REVERB_CHUNK, REVERB_MAX_TAPS = 2048, 512, 16384      # csrc/wave_aug.hip (pgasr_reverb_limits)


def _rows_i32(t, B, device, what, name):
    _req(t, torch.int32, name)
    if t is not None and (t.dim() != 1 or t.numel() != B or t.device != device):
        raise _lib.PgasrError(f"{what}: {name} must be ({B},) int32 on {device}")


def reverb(wave, n, rirs, rir_len, rir_delay, rir_idx, out=None):
    """Convolution of wave (B, stride) fp32 with room impulse responses (include/pgasr_hip.h, A0-WA): row b, n[b] samples long (n (B)
    int32 on the device), is filtered with row rir_idx[b] of the bank rirs (R, rir_stride) fp32, rir_len (R) taps, direct path at
    rir_delay (R) (all int32 on the device); a row with rir_idx[b] < 0 is copied.  The output is as long as the input and zero beyond
    it.  ``out``: a contiguous fp32 tensor of wave's shape that shares no memory with it.  One launch, no host synchronisation."""
    lib = _lib.load()
    _req(wave, torch.float32, "wave"); _req(n, torch.int32, "n"); _req(rirs, torch.float32, "rirs"); _req(out, torch.float32, "out")
    if wave.dim() != 2 or n.dim() != 1 or n.numel() != wave.shape[0] or n.device != wave.device:
        raise _lib.PgasrError("reverb wants wave (B, stride) and n (B) on one device")
    B, stride = wave.shape
    if rirs.dim() != 2 or rirs.device != wave.device:
        raise _lib.PgasrError(f"reverb: rirs must be (R, rir_stride) fp32 on {wave.device}")
    R = rirs.shape[0]
    _rows_i32(rir_len, R, wave.device, "reverb", "rir_len"); _rows_i32(rir_delay, R, wave.device, "reverb", "rir_delay")
    _rows_i32(rir_idx, B, wave.device, "reverb", "rir_idx")
    if rir_len is None or rir_delay is None or rir_idx is None:
        raise _lib.PgasrError("reverb wants rir_len, rir_delay and rir_idx")
    if out is None:
        out = torch.empty_like(wave)
    elif tuple(out.shape) != (B, stride) or out.device != wave.device:
        raise _lib.PgasrError(f"reverb: out must be ({B}, {stride}) fp32 on {wave.device}")
    if out.untyped_storage().data_ptr() == wave.untyped_storage().data_ptr():
        lo, hi = sorted(((out.data_ptr(), out.numel()), (wave.data_ptr(), wave.numel())))
        if lo[0] + 4 * lo[1] > hi[0]:
            raise _lib.PgasrError("reverb: out must not alias wave")
    with _timed("reverb"):
        st = lib.pgasr_reverb(_p(wave), stride, _p(n), B, _p(rirs), rirs.shape[1], R, _p(rir_len), _p(rir_delay), _p(rir_idx), _p(out),
                              _stream())
    _lib.check(st, "pgasr_reverb")
    return out


def wave_power(src, n, row=None, start=None, period=None, out=None):
    """power[b] = sum over i < n[b] of src[row[b], (start[b] + i) mod period[b]]^2 in fp64, in a fixed order (A0-WA): (B) fp64 on the
    device.  src (rows, stride) fp32; n, row, start, period: (B) int32 on the device.  row None: row b; period None: no wrap (start
    must be None too).  One launch, no host synchronisation."""
    lib = _lib.load()
    _req(src, torch.float32, "src"); _req(n, torch.int32, "n"); _req(out, torch.float64, "out")
    if src.dim() != 2 or n.dim() != 1 or n.device != src.device:
        raise _lib.PgasrError("wave_power wants src (rows, stride) and n (B) on one device")
    B = n.numel()
    for t, name in ((row, "row"), (start, "start"), (period, "period")):
        _rows_i32(t, B, src.device, "wave_power", name)
    if row is None and src.shape[0] < B:
        raise _lib.PgasrError(f"wave_power: src has {src.shape[0]} rows for {B} lengths and no row index")
    if start is not None and period is None:
        raise _lib.PgasrError("wave_power: start needs a period")
    if out is None:
        out = torch.empty(B, dtype=torch.float64, device=src.device)
    elif out.dim() != 1 or out.numel() != B or out.device != src.device:
        raise _lib.PgasrError(f"wave_power: out must be ({B},) fp64 on {src.device}")
    with _timed("wave_power"):
        st = lib.pgasr_wave_power(_p(src), src.shape[1], src.shape[0], _p(n), B, _p(row), _p(start), _p(period), _p(out), _stream())
    _lib.check(st, "pgasr_wave_power")
    return out


def wave_mix(wave, n, p_dry=None, p_wet=None, p_noise=None, amp=None, noise=None, noise_len=None, noise_idx=None, noise_start=None,
             gains=None, out=None):
    """out[b, i] = fp32(a_b wave[b, i] + g_b noise[noise_idx[b], (noise_start[b] + i) mod noise_len]) for i < n[b], zero beyond (A0-WA).
    With ``gains`` (B, 2) fp32 = (a, g) given they are used as they are; else they are formed on the device from the powers p_dry,
    p_wet, p_noise and amp = 10^(-snr / 20) (each (B) fp64 on the device): a restores the dry level after reverberation, g sets the
    signal-to-noise ratio.  Returns (out, gains); ``out=wave`` mixes in place.  noise (Rn, noise_stride) fp32, noise_len (Rn),
    noise_idx / noise_start (B) int32 on the device; a row with noise_idx < 0 takes no noise.  One launch, no host synchronisation."""
    lib = _lib.load()
    _req(wave, torch.float32, "wave"); _req(n, torch.int32, "n"); _req(noise, torch.float32, "noise"); _req(out, torch.float32, "out")
    _req(gains, torch.float32, "gains")
    if wave.dim() != 2 or n.dim() != 1 or n.numel() != wave.shape[0] or n.device != wave.device:
        raise _lib.PgasrError("wave_mix wants wave (B, stride) and n (B) on one device")
    B, stride = wave.shape
    dev = wave.device
    given = gains is not None
    if given:
        if tuple(gains.shape) != (B, 2) or gains.device != dev:
            raise _lib.PgasrError(f"wave_mix: gains must be ({B}, 2) fp32 on {dev}")
    else:
        gains = torch.empty(B, 2, dtype=torch.float32, device=dev)
        for t, name in ((p_dry, "p_dry"), (p_wet, "p_wet"), (p_noise, "p_noise"), (amp, "amp")):
            _req(t, torch.float64, name)
            if t is not None and (t.dim() != 1 or t.numel() != B or t.device != dev):
                raise _lib.PgasrError(f"wave_mix: {name} must be ({B},) fp64 on {dev}")
        if p_dry is None or p_wet is None or (noise is not None and (p_noise is None or amp is None)):
            raise _lib.PgasrError("wave_mix wants gains, or p_dry and p_wet (with noise: p_noise and amp too)")
    nstride = nrows = 0
    if noise is not None:
        if noise.dim() != 2 or noise.device != dev:
            raise _lib.PgasrError(f"wave_mix: noise must be (Rn, noise_stride) fp32 on {dev}")
        nrows, nstride = noise.shape
        _rows_i32(noise_len, nrows, dev, "wave_mix", "noise_len"); _rows_i32(noise_idx, B, dev, "wave_mix", "noise_idx")
        _rows_i32(noise_start, B, dev, "wave_mix", "noise_start")
        if noise_len is None or noise_idx is None:
            raise _lib.PgasrError("wave_mix: noise needs noise_len and noise_idx")
    if out is None:
        out = torch.empty_like(wave)
    elif tuple(out.shape) != (B, stride) or out.device != dev:
        raise _lib.PgasrError(f"wave_mix: out must be ({B}, {stride}) fp32 on {dev}")
    with _timed("wave_mix"):
        st = lib.pgasr_wave_mix(_p(wave), stride, _p(n), B, _p(p_dry), _p(p_wet), _p(p_noise), _p(amp), _p(noise), nstride, nrows,
                                _p(noise_len), _p(noise_idx), _p(noise_start), _p(gains), 1 if given else 0, _p(out), _stream())
    _lib.check(st, "pgasr_wave_mix")
    return out, gains


def ctc_collapse(paths, lengths, blank=0, out=None):
    """paths (P,T,B) int32 -> tokens (P,B,T) int32, token_lengths (P,B) int32.
    out = (tokens, token_lengths) to write into (contiguous, zero-filled tokens)."""
    lib = _lib.load()
    _req(paths, torch.int32, "paths"); _req(lengths, torch.int32, "lengths")
    P, T, B = paths.shape
    if out is not None:
        tokens, tl = out
        _req(tokens, torch.int32, "out tokens"); _req(tl, torch.int32, "out lengths")
        if tokens.numel() != P * B * T or tl.numel() != P * B:
            raise _lib.PgasrError("ctc_collapse: out tensors must hold (P,B,T) and (P,B) int32")
    else:
        tokens = torch.zeros(P, B, T, dtype=torch.int32, device=paths.device)
        tl = torch.empty(P, B, dtype=torch.int32, device=paths.device)
    st = lib.pgasr_ctc_collapse(_p(paths), _p(lengths), P, T, B, blank, _p(tokens), _p(tl), _stream())
    _lib.check(st, "pgasr_ctc_collapse")
    return tokens, tl


CTCAlignment = collections.namedtuple("CTCAlignment", "score frame_label frame_token token_start token_end token_logp")
ALIGN_MAX_TOKENS = 1023      # csrc/align.hip: 2 * Lmax + 1 <= 2048 lattice states


def ctc_forced_align(log_probs, tokens, input_lengths, token_lengths, blank=0, want_spans=True):
    """The best single CTC alignment (Viterbi, fp64 max-plus) of tokens (B,Lmax) int32 to log_probs (T,B,V) fp32; lengths (B) int32.
    Returns ``CTCAlignment`` of device tensors, no host synchronisation: score (B) fp64 = -log p of the best path (+inf: no
    alignment), frame_label (B,T) int32 (-1 beyond the utterance), and with ``want_spans`` frame_token (B,T) int32 (token index,
    -1 on blank frames), token_start / token_end (B,Lmax) int32 (first and one-past-last frame, -1 beyond the transcript),
    token_logp (B,Lmax) fp64 (sum of the token's frame log-probs); else None in their places.  Labels must lie in [0,V) and differ
    from blank: one that does not is aligned as a blank."""
    lib = _lib.load()
    _req(log_probs, torch.float32, "log_probs"); _req(tokens, torch.int32, "tokens")
    _req(input_lengths, torch.int32, "input_lengths"); _req(token_lengths, torch.int32, "token_lengths")
    if log_probs.dim() != 3:
        raise _lib.PgasrError("ctc_forced_align wants log_probs (T,B,V)")
    T, B, V = log_probs.shape
    if tokens.dim() != 2 or tokens.shape[0] != B or tokens.shape[1] < 1 or input_lengths.numel() != B or token_lengths.numel() != B:
        raise _lib.PgasrError(f"ctc_forced_align wants tokens ({B},Lmax >= 1) and lengths ({B})")
    Lmax, dev = tokens.shape[1], log_probs.device
    nbytes = lib.pgasr_ctc_align_workspace_bytes(T, B, Lmax)
    ws = _workspace(nbytes, dev, "align")
    score = torch.empty(B, dtype=torch.float64, device=dev)
    frame_label = torch.empty(B, T, dtype=torch.int32, device=dev)
    frame_token = token_start = token_end = token_logp = None
    if want_spans:
        frame_token = torch.empty(B, T, dtype=torch.int32, device=dev)
        token_start = torch.empty(B, Lmax, dtype=torch.int32, device=dev)
        token_end = torch.empty(B, Lmax, dtype=torch.int32, device=dev)
        token_logp = torch.empty(B, Lmax, dtype=torch.float64, device=dev)
    with _timed("ctc_forced_align"):
        st = lib.pgasr_ctc_forced_align(_p(log_probs), _p(tokens), _p(input_lengths), _p(token_lengths), T, B, V, Lmax, int(blank),
                                        _p(score), _p(frame_label), _p(frame_token), _p(token_start), _p(token_end), _p(token_logp),
                                        _p(ws), ws.numel(), _stream())
    _lib.check(st, "pgasr_ctc_forced_align")
    return CTCAlignment(score, frame_label, frame_token, token_start, token_end, token_logp)


def edit_distance(ref, ref_len, hyp, hyp_len, want_prefix=False):
    """ref (N,R) int32, hyp (N,Hy) int32 -> dist (N,) int32 [, prefix (N,Hy+1) int32]."""
    lib = _lib.load()
    _req(ref, torch.int32, "ref"); _req(hyp, torch.int32, "hyp")
    _req(ref_len, torch.int32, "ref_len"); _req(hyp_len, torch.int32, "hyp_len")
    N, R = ref.shape
    Hy = hyp.shape[1]
    dist = torch.empty(N, dtype=torch.int32, device=ref.device)
    prefix = torch.full((N, Hy + 1), -1, dtype=torch.int32, device=ref.device) if want_prefix else None
    st = lib.pgasr_edit_distance(_p(ref) if R else 0, _p(ref_len), R, _p(hyp) if Hy else 0, _p(hyp_len), Hy,
                                 N, _p(dist), _p(prefix), _stream())
    _lib.check(st, "pgasr_edit_distance")
    return (dist, prefix) if want_prefix else dist


WORD_MAX_STRIDE = 4094           # PGASR_WORD_MAX_STRIDE


def word_ids(ref, ref_len, hyp, hyp_len, delimiter):
    """Words = the runs between ``delimiter`` tokens (str.split(" ") on the decoded rows).  ref (N,R), hyp (N,Hy) int32 ->
    (ref_ids (N,R+1), ref_words (N,), hyp_ids (N,Hy+1), hyp_words (N,)) int32: per word 1 + the index of its first occurrence in
    the pair's ref words ++ hyp words (entries past a row's word count are not written), and the word counts."""
    lib = _lib.load()
    _req(ref, torch.int32, "ref"); _req(hyp, torch.int32, "hyp")
    _req(ref_len, torch.int32, "ref_len"); _req(hyp_len, torch.int32, "hyp_len")
    N, R = ref.shape
    Hy = hyp.shape[1]
    dev = ref.device
    ref_ids = torch.empty(N, R + 1, dtype=torch.int32, device=dev)
    hyp_ids = torch.empty(N, Hy + 1, dtype=torch.int32, device=dev)
    counts = torch.empty(2, N, dtype=torch.int32, device=dev)
    st = lib.pgasr_word_ids(_p(ref) if R else 0, _p(ref_len), R, _p(hyp) if Hy else 0, _p(hyp_len), Hy, N, int(delimiter),
                            _p(ref_ids), counts[0].data_ptr(), _p(hyp_ids), counts[1].data_ptr(), _stream())
    _lib.check(st, "pgasr_word_ids")
    return ref_ids, counts[0], hyp_ids, counts[1]


def word_edit_distance(ref, ref_len, hyp, hyp_len, delimiter):
    """Word-level Levenshtein distance of N token-row pairs: ``word_ids`` then ``edit_distance`` on the id rows.
    Returns (dist (N,), ref_words (N,), hyp_words (N,)) int32."""
    ref_ids, ref_words, hyp_ids, hyp_words = word_ids(ref, ref_len, hyp, hyp_len, delimiter)
    return edit_distance(ref_ids, ref_words, hyp_ids, hyp_words), ref_words, hyp_words


SPELL_MAX_UNIT_CHARS = 64        # PGASR_SPELL_MAX_UNIT_CHARS


def unit_spell(tokens, lengths, spelling, out_stride=None, want_full=False):
    """Rows of subword units -> rows of character ids (pgasr_unit_spell; include/pgasr_hip.h, A11-SPELL): tokens (N,stride) or
    (P,B,T) int32 with lengths (N,) or (P,B), ``spelling`` a ``units.UnitSpelling``.  Returns (chars, char_len[, full_len]) int32 with
    the rows' leading shape: chars (.., out_stride) is the concatenation of the units' spellings cut at out_stride and zero behind
    char_len = min(full_len, out_stride).  out_stride: None = min(stride * spelling.max_unit_chars, WORD_MAX_STRIDE), which keeps every
    spelled row within pgasr_word_ids' and pgasr_edit_distance's limits.  One launch, no host synchronisation."""
    lib = _lib.load()
    _req(tokens, torch.int32, "tokens"); _req(lengths, torch.int32, "lengths")
    if tokens.dim() < 2 or tuple(lengths.shape) != tuple(tokens.shape[:-1]):
        raise _lib.PgasrError("unit_spell wants tokens (.., stride) and lengths of the leading shape")
    if spelling.max_unit_chars > SPELL_MAX_UNIT_CHARS:
        raise ValueError(f"a unit of {spelling.max_unit_chars} characters: pgasr_unit_spell takes at most {SPELL_MAX_UNIT_CHARS}")
    lead, stride = tuple(tokens.shape[:-1]), tokens.shape[-1]
    N = lengths.numel()
    if out_stride is None:
        out_stride = min(stride * spelling.max_unit_chars, WORD_MAX_STRIDE)
    out_stride = int(out_stride)
    if out_stride < 0:
        raise ValueError(f"out_stride must be >= 0 (got {out_stride})")
    dev = tokens.device
    off, pool = spelling.to(dev)
    out = torch.empty(lead + (out_stride,), dtype=torch.int32, device=dev)
    lens = torch.empty((2 if want_full else 1,) + lead, dtype=torch.int32, device=dev)
    with _timed("unit_spell"):
        st = lib.pgasr_unit_spell(_p(tokens) if stride else 0, _p(lengths), stride, N, _p(off), _p(pool), spelling.vocab,
                                  _p(out) if out_stride else 0, out_stride, lens[0].data_ptr(),
                                  lens[1].data_ptr() if want_full else 0, _stream())
    _lib.check(st, "pgasr_unit_spell")
    return (out, lens[0], lens[1]) if want_full else (out, lens[0])


def spelled_edit_distance(ref, ref_len, hyp, hyp_len, spelling, unit="char"):
    """The edit distance of N pairs of unit rows over their SPELLED text: both sides through ``unit_spell``, then ``edit_distance``
    (unit="char") or ``word_edit_distance`` at the spelling's " " (unit="word").  Returns (dist (N,), ref_count (N,), truncated)
    int32 on the device: ref_count the reference's spelled length or word count, truncated the number of rows, of either side, whose
    spelling was cut at the output stride (a 0-d tensor; nothing synchronises on it)."""
    if unit not in ("char", "word"):
        raise ValueError(f"unit must be 'char' or 'word' (got {unit!r})")
    delim = spelling.word_delimiter() if unit == "word" else None
    rc, rl, rf = unit_spell(ref, ref_len, spelling, want_full=True)
    hc, hl, hf = unit_spell(hyp, hyp_len, spelling, want_full=True)
    truncated = ((rf > rl).sum() + (hf > hl).sum()).to(torch.int32)
    if unit == "char":
        return edit_distance(rc, rl, hc, hl), rl, truncated
    dist, ref_words, _ = word_edit_distance(rc, rl, hc, hl, delim)
    return dist, ref_words, truncated


EditOps = collections.namedtuple("EditOps", "counts ops n_ops")
WordEditOps = collections.namedtuple("WordEditOps", "counts ops n_ops ref_words hyp_words")
EDIT_OPS_MAX_VOCAB = 64          # csrc/editops.hip: the confusion matrix


def edit_ops_workspace_bytes(ref_stride, hyp_stride, N):
    """Bytes of workspace one ``pgasr_edit_ops`` launch over N pairs of these strides needs (host only, no GPU)."""
    return int(_lib.load().pgasr_edit_ops_workspace_bytes(int(ref_stride), int(hyp_stride), int(N)))


def edit_ops(ref, ref_len, hyp, hyp_len, want_ops=True, confusion=None, vocab=None, max_workspace_bytes=256 << 20):
    """The canonical optimal alignment of N (reference, hypothesis) pairs (include/pgasr_hip.h, A10-OPS): diagonal before deletion
    before insertion on the walk back.  ref (N,R), hyp (N,Hy) int32 rows of arbitrary symbols with lengths (N) int32, on the GPU.
    Returns ``EditOps`` of device tensors: counts (N,4) int32 = hits, substitutions, deletions, insertions; with ``want_ops`` ops
    (N,R+Hy) int8 -- 0 hit, 1 substitution, 2 deletion, 3 insertion, left to right, -1 from n_ops on -- and n_ops (N) int32, else
    None in their places.  confusion: None, or a (vocab+1, vocab+1) int64 device matrix the kernel ADDS into ([r][h] hits and
    substitutions, [r][vocab] deletions, [vocab][h] insertions; symbols outside [0, vocab) are left out), vocab <= 64.
    N is split into chunks so that no launch needs more than ``max_workspace_bytes`` of workspace (the cached "edit_ops" buffer);
    a cap below one pair's workspace raises.  Current stream, no host synchronisation."""
    lib = _lib.load()
    _req(ref, torch.int32, "ref"); _req(hyp, torch.int32, "hyp")
    _req(ref_len, torch.int32, "ref_len"); _req(hyp_len, torch.int32, "hyp_len")
    if ref.dim() != 2 or hyp.dim() != 2 or hyp.shape[0] != ref.shape[0] or ref_len.numel() != ref.shape[0] or hyp_len.numel() != ref.shape[0]:
        raise _lib.PgasrError("edit_ops wants ref (N,R), hyp (N,Hy) and lengths (N)")
    N, R = ref.shape
    Hy = hyp.shape[1]
    dev = ref.device
    if confusion is not None:
        _req(confusion, torch.int64, "confusion")
        if vocab is None or int(vocab) < 1 or tuple(confusion.shape) != (int(vocab) + 1, int(vocab) + 1):
            raise _lib.PgasrError("edit_ops: confusion must be (vocab+1, vocab+1) int64 with vocab >= 1 given")
    vocab = 0 if confusion is None else int(vocab)
    counts = torch.empty(N, 4, dtype=torch.int32, device=dev)
    ops = torch.empty(N, R + Hy, dtype=torch.int8, device=dev) if want_ops else None
    n_ops = torch.empty(N, dtype=torch.int32, device=dev) if want_ops else None
    if N == 0:
        return EditOps(counts, ops, n_ops)
    per_pair = int(lib.pgasr_edit_ops_workspace_bytes(R, Hy, 1))
    if per_pair > int(max_workspace_bytes):
        raise _lib.PgasrError(f"edit_ops: one pair of strides {R} / {Hy} needs {per_pair} bytes of workspace, above "
                              f"max_workspace_bytes = {int(max_workspace_bytes)}")
    chunk = N if per_pair == 0 else max(1, min(N, int(max_workspace_bytes) // per_pair))
    nbytes = int(lib.pgasr_edit_ops_workspace_bytes(R, Hy, chunk))
    ws = _workspace(nbytes, dev, "edit_ops")
    with _timed("edit_ops"):
        for a in range(0, N, chunk):
            b = min(N, a + chunk)
            st = lib.pgasr_edit_ops(ref[a:b].data_ptr() if R else 0, ref_len[a:b].data_ptr(), R,
                                    hyp[a:b].data_ptr() if Hy else 0, hyp_len[a:b].data_ptr(), Hy, b - a,
                                    counts[a:b].data_ptr(), ops[a:b].data_ptr() if want_ops and R + Hy else 0,
                                    n_ops[a:b].data_ptr() if want_ops else 0, _p(confusion), vocab, _p(ws), ws.numel(), _stream())
            _lib.check(st, "pgasr_edit_ops")
    return EditOps(counts, ops, n_ops)


def word_edit_ops(ref, ref_len, hyp, hyp_len, delimiter, want_ops=True, max_workspace_bytes=256 << 20):
    """Word-level alignment of N token-row pairs: ``word_ids`` then ``edit_ops`` on the id rows (words are the runs between
    ``delimiter`` tokens, as str.split(" ") cuts the decoded rows).  Returns ``WordEditOps``: counts (N,4), ops (N,R+Hy+2) / n_ops
    as ``edit_ops`` gives them over words, and the word counts ref_words / hyp_words (N) int32."""
    ref_ids, ref_words, hyp_ids, hyp_words = word_ids(ref, ref_len, hyp, hyp_len, delimiter)
    eo = edit_ops(ref_ids, ref_words, hyp_ids, hyp_words, want_ops=want_ops, max_workspace_bytes=max_workspace_bytes)
    return WordEditOps(eo.counts, eo.ops, eo.n_ops, ref_words, hyp_words)


SlotMass = collections.namedtuple("SlotMass", "hit sub gap other n_slots left_out")
NBestConfidence = collections.namedtuple("NBestConfidence", "tokens lengths conf substituted deleted inserted left_out")
SLOT_MASS_MAX_SLOTS = 4095       # csrc/confidence.hip (and ops_stride <= 8190)
SLOT_MASS_MAX_PER_GROUP = 128
_SLOT_SIDES = {"ref": 0, "hyp": 1}


def _slot_mass_launch(ops, n_ops, ops_stride, weight, groups, per_group, side, slots, mass, n_slots, left_out):
    with _timed("edit_ops_slot_mass"):
        st = _lib.load().pgasr_edit_ops_slot_mass(_p(ops) if ops_stride else 0, _p(n_ops), ops_stride, _p(weight), groups, per_group,
                                                  side, slots, _p(mass), _p(n_slots), _p(left_out), _stream())
    _lib.check(st, "pgasr_edit_ops_slot_mass")


def edit_ops_slot_mass(ops, n_ops, weight, per_group, side="ref", slots=None):
    """Per-position masses of groups of operation strings (pgasr_edit_ops_slot_mass; include/pgasr_hip.h, A10-CONF): ops (P,stride)
    int8 / n_ops (P) int32 as ``edit_ops(want_ops=True)`` returns them, weight (P) float64, pair p = g * per_group + n in group g,
    per_group <= 128.  side="ref" indexes slots by reference position (own gap operation: the deletion, other: the insertion),
    side="hyp" by hypothesis position (own: insertion, other: deletion).  Returns ``SlotMass``: hit / sub / gap / other
    (groups, slots+1) float64 views of one tensor -- per slot the weight of the participating pairs (weight finite and > 0) with a
    hit / a substitution / the own gap operation there, in ascending pair order, and per gap the weighted count of other operations
    --, n_slots (groups) int32 the slot count of the group's first participating pair (-1: none) and left_out (groups) int32 the
    participating pairs with another slot count or more than ``slots``.  slots: None reads the largest possible count from the
    device (ONE host synchronisation); a number avoids it.  One launch."""
    _req(ops, torch.int8, "ops"); _req(n_ops, torch.int32, "n_ops"); _req(weight, torch.float64, "weight")
    if side not in _SLOT_SIDES:
        raise ValueError(f"side must be 'ref' or 'hyp' (got {side!r})")
    per_group = int(per_group)
    if ops.dim() != 2 or per_group < 1 or ops.shape[0] % per_group or n_ops.numel() != ops.shape[0] or weight.numel() != ops.shape[0]:
        raise _lib.PgasrError("edit_ops_slot_mass wants ops (P,stride), n_ops (P) and weight (P) with P a multiple of per_group")
    P, stride = ops.shape
    if P == 0:
        raise _lib.PgasrError("edit_ops_slot_mass: no pairs")
    if slots is None:
        slots = min(int(n_ops.clamp(0, stride).max().item()), SLOT_MASS_MAX_SLOTS)
    slots = int(slots)
    if slots < 0:
        raise ValueError(f"slots must be >= 0 (got {slots})")
    groups = P // per_group
    dev = ops.device
    mass = torch.empty(groups, 4, slots + 1, dtype=torch.float64, device=dev)
    meta = torch.empty(2, groups, dtype=torch.int32, device=dev)
    _slot_mass_launch(ops, n_ops, stride, weight, groups, per_group, _SLOT_SIDES[side], slots, mass, meta[0], meta[1])
    return SlotMass(mass[:, 0], mass[:, 1], mass[:, 2], mass[:, 3], meta[0], meta[1])


def nbest_confidence(tokens, lengths, count, posterior, pivot, unit="char", delimiter=None, max_hyp_len=None,
                     max_workspace_bytes=256 << 20, vocab=None):
    """N-best confidences (Wessel et al. 2001): every hypothesis of a list aligned to the chosen one, the confidence of a position
    being the posterior mass of the hypotheses that agree with it there.  tokens (N,B,stride) / lengths (N,B) / count (B) int32 as
    the N-best searches return them (narrow or wide), posterior (N,B) float64 as ``mbr_select`` returns it (rows with 0 take no
    part), pivot (B) int32 the chosen row of every utterance.  The B * N pairs (pivot row of b, row n of b) are expanded in bounded
    chunks of whole utterances through ``edit_ops(want_ops=True)`` -- the canonical alignment, pivot as the reference -- and
    ``pgasr_edit_ops_slot_mass`` with side="ref"; unit="word" runs ``word_ids`` first and aligns the id rows (words split at the
    token ``delimiter`` as str.split(" ") cuts them).  vocab: the number of symbols, if the caller knows it: unit="word" over more
    than 64 raises ValueError, because a subword unit may hold a space.
    max_hyp_len: None, or a cap on the rows' length: a longer row takes no part, and neither does a list whose pivot is longer.
    Returns ``NBestConfidence``: tokens (B,L) / lengths (B) int32 the pivot rows (unit="word": tokens None, lengths the pivots'
    word counts), and (B,L+1) float64 conf (hit mass), substituted, deleted (the mass of hypotheses
    without a partner for the position) and inserted (per gap j, in front of position j, the expected number of extra symbols);
    left_out (B) int32 as ``edit_ops_slot_mass`` counts it.  conf + substituted + deleted is the participating mass at every
    position.  No host synchronisation."""
    lib = _lib.load()
    _req(tokens, torch.int32, "tokens"); _req(lengths, torch.int32, "lengths"); _req(count, torch.int32, "count")
    _req(posterior, torch.float64, "posterior"); _req(pivot, torch.int32, "pivot")
    if tokens.dim() != 3 or tuple(lengths.shape) != tuple(tokens.shape[:2]) or count.numel() != tokens.shape[1] \
            or tuple(posterior.shape) != tuple(lengths.shape) or pivot.numel() != tokens.shape[1]:
        raise _lib.PgasrError("nbest_confidence wants tokens (N,B,stride), lengths (N,B), count (B), posterior (N,B) and pivot (B)")
    if unit not in ("char", "word"):
        raise ValueError(f"unit must be 'char' or 'word' (got {unit!r})")
    if unit == "word" and (delimiter is None or int(delimiter) < 0):
        raise ValueError("unit='word' needs delimiter, the token id of the alphabet's ' ' symbol")
    if unit == "word" and vocab is not None and int(vocab) > MAX_VOCAB_NARROW:
        raise ValueError(f"unit='word': not over {int(vocab)} > {MAX_VOCAB_NARROW} symbols -- a subword unit may hold a space, so words "
                         f"cannot be split at a delimiter token; take unit='char' (the units are the symbols)")
    N, B, stride = tokens.shape
    if N < 1 or N > SLOT_MASS_MAX_PER_GROUP:
        raise _lib.PgasrError(f"nbest_confidence takes 1 <= N <= {SLOT_MASS_MAX_PER_GROUP} hypotheses per utterance (got {N})")
    if max_hyp_len is not None and int(max_hyp_len) < 0:
        raise ValueError(f"max_hyp_len must be >= 0 (got {max_hyp_len})")
    cap = stride if max_hyp_len is None else min(stride, int(max_hyp_len))
    S = max(1, cap)
    dev = tokens.device
    piv = pivot.long().clamp(0, N - 1)
    cols = torch.arange(B, device=dev)
    ln = lengths.clamp(0, stride)
    rows = torch.arange(N, device=dev).view(N, 1) < count.clamp(0, N).view(1, B)
    valid = rows & (ln <= cap)
    valid = valid & valid[piv, cols].view(1, B)
    ln = torch.where(valid, ln, torch.zeros_like(ln))
    weight = torch.where(valid, posterior, torch.zeros_like(posterior)).t().contiguous()            # (B,N): pair b * N + n
    piv_tok = tokens[piv, cols, :S].contiguous()                                                     # (B,S)
    piv_len = ln[piv, cols].contiguous()
    L = S + 1 if unit == "word" else S                      # word rows: a row of S tokens has at most S + 1 words
    ops_stride = 2 * L
    if L > SLOT_MASS_MAX_SLOTS:
        raise _lib.PgasrError(f"nbest_confidence: rows of {S} tokens exceed the limit of {SLOT_MASS_MAX_SLOTS} positions")
    mass = torch.empty(B, 4, L + 1, dtype=torch.float64, device=dev)
    meta = torch.empty(2, B, dtype=torch.int32, device=dev)
    n_words = torch.empty(B, dtype=torch.int32, device=dev) if unit == "word" else None
    per_pair = int(lib.pgasr_edit_ops_workspace_bytes(L, L, 1))
    by_ws = int(max_workspace_bytes) // max(per_pair * N, 1)
    by_rows = PAIR_DIST_CHUNK_ELEMS // ((2 if unit == "char" else 4) * (S + 1) * N)
    step = max(1, min(B, by_ws, by_rows))                   # utterances per chunk
    with _timed("nbest_confidence"):
        for b0 in range(0, B, step):
            b1 = min(B, b0 + step)
            G = b1 - b0
            ref = piv_tok[b0:b1].unsqueeze(1).expand(G, N, S).reshape(G * N, S)
            rl = piv_len[b0:b1].unsqueeze(1).expand(G, N).reshape(G * N).contiguous()
            hyp = tokens[:, b0:b1, :S].permute(1, 0, 2).reshape(G * N, S)
            hl = ln[:, b0:b1].t().reshape(G * N).contiguous()
            if unit == "word":
                ref, rl, hyp, hl = word_ids(ref.contiguous(), rl, hyp.contiguous(), hl, int(delimiter))
                n_words[b0:b1] = rl.view(G, N)[:, 0]
            eo = edit_ops(ref.contiguous(), rl, hyp.contiguous(), hl, want_ops=True, max_workspace_bytes=max_workspace_bytes)
            _slot_mass_launch(eo.ops, eo.n_ops, ops_stride, weight[b0:b1], G, N, 0, L, mass[b0:b1], meta[0, b0:b1], meta[1, b0:b1])
    if unit == "word":
        return NBestConfidence(None, n_words, mass[:, 0], mass[:, 1], mass[:, 2], mass[:, 3], meta[1])
    return NBestConfidence(piv_tok, piv_len, mass[:, 0], mass[:, 1], mass[:, 2], mass[:, 3], meta[1])


def reinforce_grad(scores, path, coef, lengths, out=None, accumulate=False):
    lib = _lib.load()
    _req(scores, torch.float32, "scores"); _req(path, torch.int32, "path")
    _req(coef, torch.float32, "coef"); _req(lengths, torch.int32, "lengths")
    T, B, V = scores.shape
    if out is None:
        if accumulate:
            raise _lib.PgasrError("accumulate=True needs an output tensor")
        out = torch.empty_like(scores)
    _req(out, torch.float32, "out")
    st = lib.pgasr_reinforce_grad(_p(scores), _p(path), _p(coef), _p(lengths), T, B, V, int(bool(accumulate)),
                                  _p(out), _stream())
    _lib.check(st, "pgasr_reinforce_grad")
    return out


# ------------------------------------------------------------------------------------------
# dense contractions
# ------------------------------------------------------------------------------------------
GEMM_XCC_BUSY_PTR = 0   # device address of a sweep's 8 busy counters (0 = plain launch); set around side-stream GEMMs
GEMM_PRECISION = 0   # the model's GEMMs: 0 = fp32-faithful (six-product / exact fp32 MFMA; the default mode "f32"), 1 = bf16x3 split MFMA
LSTM_PLANES = 3      # bf16 planes per fp32 operand in the recurrent sweeps: 3 = hi/mid/lo, 6 products (default, "f32"); 2 = hi/lo, 3 products

# The arithmetic of the whole path is a MODE of the host layer:
#   "bf16x3": (opt-in) every dense product = 3 bf16 MFMA terms of a 2-plane split (~16 operand bits), fp32 accumulate; the input
#             affine (whose sign feeds leaky_relu') on the exact fp32 MFMA.  Within north_star's 1e-3 bar; ~20 % faster.
#   "f32":    (the DEFAULT since round 5) the reference's arithmetic (torch fp32: nn.Linear / nn.LSTM, model.py:38-44): every fp32 operand of a big product
#             as THREE bf16 planes and the product as SIX MFMA terms (every term down to 2^-24) -- the recurrent sweeps
#             (lstm.hip NP = 3) and, since round 4, the hoisted W_ih products and the weight gradients too (gemm_x6.hip), so the
#             mode runs the same feed-ahead and streamed orders as "bf16x3"; the small products (input affine, CTC head) on
#             the exact fp32 MFMA (v_mfma_f32_32x32x2_f32).
PRECISION_MODES = {"bf16x3": (1, 2), "f32": (0, 3)}
_precision = "f32"


def set_precision(mode):
    global GEMM_PRECISION, LSTM_PLANES, _precision
    if mode not in PRECISION_MODES:
        raise ValueError(f"precision mode must be one of {sorted(PRECISION_MODES)}")
    GEMM_PRECISION, LSTM_PLANES = PRECISION_MODES[mode]
    _precision = mode


def get_precision():
    return _precision


class precision:
    """``with hipops.precision("f32"): ...`` -- the mode for everything launched inside."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = _precision
        set_precision(self.mode)
        return self

    def __exit__(self, *a):
        set_precision(self.prev)
        return False


def gemm(A, B, C, M, N, K, transA=False, transB=False, lda=None, ldb=None, ldc=None, alpha=1.0,
         strideA=0, strideB=0, strideC=0, batch=1, sum_batches=False, splitk=1, bias=None, bias2=None,
         act=0, slope=0.01, accumulate=False, dact_y=None, norm_operand=0, shift=None, scale=None,
         a_off=0, b_off=0, c_off=0, precision=None, xcc_busy=None):
    """Raw strided GEMM on device tensors (element offsets a_off/b_off/c_off into A/B/C).
    See include/pgasr_hip.h for the contract."""
    lib = _lib.load()
    if precision is None:
        precision = GEMM_PRECISION
    for t, nm in ((A, "A"), (B, "B"), (C, "C"), (bias, "bias"), (bias2, "bias2"), (dact_y, "dact_y"),
                  (shift, "shift"), (scale, "scale")):
        if t is not None:
            if not t.is_cuda or t.dtype != torch.float32:
                raise _lib.PgasrError(f"gemm operand {nm} must be a float32 GPU tensor")
    lda = lda if lda is not None else (M if transA else K)
    ldb = ldb if ldb is not None else (K if transB else N)
    ldc = ldc if ldc is not None else N
    nbytes = lib.pgasr_gemm_workspace_bytes(M, N, batch, splitk, int(sum_batches))
    ws = _workspace(nbytes, C.device, "gemm")
    with _timed("gemm_f32"):
      st = lib.pgasr_gemm_f32(int(transA), int(transB), M, N, K, float(alpha),
                            A.data_ptr() + 4 * a_off, lda, int(strideA), B.data_ptr() + 4 * b_off, ldb, int(strideB),
                            C.data_ptr() + 4 * c_off, ldc, int(strideC), batch, int(sum_batches), splitk,
                            _p(bias), _p(bias2), act, float(slope), int(accumulate), _p(dact_y),
                            norm_operand, _p(shift), _p(scale), int(precision), int(GEMM_XCC_BUSY_PTR if xcc_busy is None else xcc_busy), _p(ws), ws.numel() if ws is not None else 0, _stream())
    _lib.check(st, "pgasr_gemm_f32")
    return C


X6_PACKED = _os_environ_get("PGASR_X6_PACKED", "1") != "0"     # three-plane weights as ONE buffer in the six-product kernel's LDS-image order


class X6Pack:
    """The three-plane weight operand of the six-product kernels, packed tile by tile (``pgasr_pack_x6w_planes``)."""
    __slots__ = ("pack", "N", "K")

    def __init__(self, pack, N, K):
        self.pack, self.N, self.K = pack, N, K

    def __len__(self):
        return 3

    def __iter__(self):          # tensors to keep alive / to hold across streams
        return iter((self.pack,))


def split_planes(w, transpose=False, planes=None, packed=None):
    """fp32 matrix (rows, cols) -> bf16 planes (int16 storage) of shape (rows, cols), or (cols, rows) with ``transpose``: the
    pre-split weight operand of ``gemm_x3w``.  planes = 2: (hi, lo), the bf16x3 kernels' operand; 3: (hi, mid, lo), the
    six-product kernels' (precision mode "f32"); None: what the current precision mode uses."""
    lib = _lib.load()
    _req(w, torch.float32, "w")
    if w.dim() != 2 or w.stride(1) != 1:
        raise _lib.PgasrError("split_planes wants a row-major 2-D tensor")
    planes = LSTM_PLANES if planes is None else int(planes)
    if planes not in (2, 3):
        raise _lib.PgasrError("split_planes: 2 or 3 planes")
    rows, cols = w.shape
    shape = (cols, rows) if transpose else (rows, cols)
    if planes == 3 and (X6_PACKED if packed is None else packed) and shape[0] % 256 == 0 and shape[1] % 16 == 0:
        pack = torch.empty(shape[0] * shape[1] * 6, dtype=torch.uint8, device=w.device)
        _lib.check(lib.pgasr_pack_x6w_planes(w.data_ptr(), rows, cols, w.stride(0), int(transpose), pack.data_ptr(), _stream()), "pgasr_pack_x6w_planes")
        return X6Pack(pack, shape[0], shape[1])
    out = tuple(torch.empty(shape, dtype=torch.int16, device=w.device) for _ in range(planes))
    if planes == 3:
        st = lib.pgasr_split_bf16_planes3(w.data_ptr(), rows, cols, w.stride(0), int(transpose), *[t.data_ptr() for t in out], _stream())
    else:
        st = lib.pgasr_split_bf16_planes(w.data_ptr(), rows, cols, w.stride(0), int(transpose), *[t.data_ptr() for t in out], _stream())
    _lib.check(st, "pgasr_split_bf16_planes")
    return out


def gemm_x3w_ok(M, N, K, lda=None, planes=2):
    """Shapes the LDS-DMA kernels take (else use ``gemm``): planes = 2 the bf16x3 kernels, 3 the six-product ones."""
    lda = K if lda is None else lda
    if planes == 3:
        Mp = (M + 255) // 256 * 256       # the kernel addresses whole 256-row tiles with 32-bit offsets (x6w_shape_ok, gemm_x6.hip)
        return K % 16 == 0 and K >= 64 and N % 256 == 0 and lda % 4 == 0 and M > 0 and Mp * max(N, lda) * 4 < 2 ** 32
    Mp = (M + 255) // 256 * 256           # the same rule for the two-plane kernels' epilogue (256-row tiles, ldc = N; pgasr_gemm_x3w_f32)
    return K % 32 == 0 and N % 128 == 0 and lda % 4 == 0 and M > 0 and Mp * N * 4 < 2 ** 32


def _plane_ptrs(planes):
    """(hi, mid, lo) device addresses for the six-product entry points: a pack travels as hi with mid = lo = NULL."""
    if isinstance(planes, X6Pack):
        return planes.pack.data_ptr(), None, None
    return tuple(t.data_ptr() for t in planes)


def _check_planes(planes, N, K, what):
    if isinstance(planes, X6Pack):
        if (planes.N, planes.K) != (N, K) or not planes.pack.is_cuda:
            raise _lib.PgasrError(f"{what}: packed planes are for a ({planes.N}, {planes.K}) weight, the product wants ({N}, {K})")
        return
    if len(planes) not in (2, 3):
        raise _lib.PgasrError(f"{what}: planes must be a (hi, lo) or (hi, mid, lo) tuple")
    for t in planes:
        if tuple(t.shape) != (N, K) or t.dtype != torch.int16 or not t.is_contiguous() or not t.is_cuda:
            raise _lib.PgasrError(f"{what} planes must be contiguous int16 (N, K) GPU tensors")


def gemm_x3w(A, planes, C, M, N, K, lda=None, ldc=None, bias=None, dact_y=None, slope=0.01):
    """C[M,N] = A[M,K] @ W[N,K]^T (+bias) (*leaky'(dact_y)); W given as ``split_planes`` output: two planes -> the bf16x3
    kernels (three products), three planes -> the fp32-faithful six-product kernel (gemm_x6.hip)."""
    lib = _lib.load()
    for t, nm in ((A, "A"), (C, "C"), (bias, "bias"), (dact_y, "dact_y")):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise _lib.PgasrError(f"gemm_x3w operand {nm} must be a float32 GPU tensor")
    _check_planes(planes, N, K, "gemm_x3w")
    with _timed("gemm_x6c" if len(planes) == 3 else "gemm_x3c"):
        if len(planes) == 3:
            st = lib.pgasr_gemm_x6w_f32(M, N, K, A.data_ptr(), K if lda is None else lda, *_plane_ptrs(planes),
                                        C.data_ptr(), N if ldc is None else ldc, _p(bias), _p(dact_y), float(slope), _stream())
        else:
            st = lib.pgasr_gemm_x3w_f32(M, N, K, A.data_ptr(), K if lda is None else lda, planes[0].data_ptr(), planes[1].data_ptr(),
                                        C.data_ptr(), N if ldc is None else ldc, _p(bias), _p(dact_y), float(slope), _stream())
    _lib.check(st, "pgasr_gemm_x6w_f32" if len(planes) == 3 else "pgasr_gemm_x3w_f32")
    return C


def colsum(X, rows, cols, ld, out, out2=None, accumulate=False):
    lib = _lib.load()
    nbytes = lib.pgasr_colsum_workspace_bytes(rows, cols)
    ws = _workspace(nbytes, X.device, "colsum")
    st = lib.pgasr_colsum_f32(_p(X), rows, cols, ld, _p(out), _p(out2), int(accumulate), _p(ws), ws.numel(), _stream())
    _lib.check(st, "pgasr_colsum_f32")
    return out


def instnorm_stats(x, eps=1e-5):
    lib = _lib.load()
    _req(x, torch.float32, "x")
    B, F, T = x.shape
    mean = torch.empty(B, dtype=torch.float32, device=x.device)
    rstd = torch.empty(B, dtype=torch.float32, device=x.device)
    _lib.check(lib.pgasr_instnorm_stats(_p(x), B, F, T, float(eps), _p(mean), _p(rstd), _stream()), "pgasr_instnorm_stats")
    return mean, rstd


def log_softmax_rows(logits, wide=None):
    """log_softmax over the last dimension, V <= MAX_VOCAB_WIDE; V > 64 (or wide=True): ``pgasr_log_softmax_rows_wide``."""
    lib = _lib.load()
    _req(logits, torch.float32, "logits")
    V = logits.shape[-1]
    out = torch.empty_like(logits)
    entry = "pgasr_log_softmax_rows_wide" if _wide(V, wide, "log_softmax_rows") else "pgasr_log_softmax_rows"
    _lib.check(getattr(lib, entry)(_p(logits), logits.numel() // V, V, _p(out), _stream()), entry)
    return out


# ------------------------------------------------------------------------------------------
# LSTM layer
# ------------------------------------------------------------------------------------------
HID = 256


def lstm_pack(params, in_dim):
    """params: 8 tensors (w_ih, w_hh, b_ih, b_hh) x (fwd, rev) -> (wih_perm, bias_perm, pack_f, pack_b)."""
    lib = _lib.load()
    dev = params[0].device
    for t in params:
        _req(t, torch.float32, "lstm parameter")
    wih_perm = torch.empty(2 * 4 * HID, in_dim, dtype=torch.float32, device=dev)
    bias_perm = torch.empty(2 * 4 * HID, dtype=torch.float32, device=dev)
    nb = lib.pgasr_lstm_pack_bytes(0, LSTM_PLANES)
    pack_f = torch.empty(nb, dtype=torch.uint8, device=dev)
    pack_b = torch.empty(nb, dtype=torch.uint8, device=dev)
    st = lib.pgasr_lstm_pack_weights(*[_p(t) for t in params], in_dim, _p(wih_perm), _p(bias_perm),
                                     _p(pack_f), _p(pack_b), LSTM_PLANES, _stream())
    _lib.check(st, "pgasr_lstm_pack_weights")
    return wih_perm, bias_perm, pack_f, pack_b


def _lstm_flags(pack):
    """Sweep flags for a W_hh pack made by ``lstm_pack``: the pack's size says how many planes it holds."""
    planes = 3 if pack.numel() == _lib.load().pgasr_lstm_pack_bytes(0, 3) else 2
    return LSTM_FLAGS | (2 if planes == 3 else 0)


def lstm_unpack_grads(dwih_perm, dbias_perm, dwhh_perm, in_dim, grads, accumulate=False):
    lib = _lib.load()
    st = lib.pgasr_lstm_unpack_grads(_p(dwih_perm), _p(dbias_perm), _p(dwhh_perm), in_dim,
                                     *[_p(g) for g in grads], int(accumulate), _stream())
    _lib.check(st, "pgasr_lstm_unpack_grads")


_lstm_err_checks = []


def _lstm_ws(T, B, backward, device):
    lib = _lib.load()
    nbytes = lib.pgasr_lstm_workspace_bytes(T, B, int(backward))
    return _workspace(nbytes, device, "lstm_bwd" if backward else "lstm_fwd")


import os as _os
LSTM_FLAGS = int(_os.environ.get("PGASR_LSTM_FLAGS", "0"), 0)   # bit 0: force the write-through (cross-XCD) hand-off protocol; bits 8..: diagnostics


def lstm_layer_fwd(gates, out, cbuf, pack_f, lengths, T, B, fed=None, fed_need=0, out_drop=None, drop=None):
    """fed: int32 (2, ceil(T*B/256)) finished-tile counters of a ``gemm_x3w_feed`` that is launched AFTER this call on
    another stream and fills ``gates`` while the sweep runs (zeroed by the caller before this call).
    out_drop + drop = (p, seed, offset): the sweep also writes dropout(out) -- the next layer's input -- there."""
    lib = _lib.load()
    ws = _lstm_ws(T, B, False, gates.device)
    p, seed, offset = drop if (drop is not None and out_drop is not None) else (0.0, 0, 0)
    if out_drop is not None:
        _req(out_drop, torch.float32, "out_drop")
        if out_drop.numel() != out.numel() or drop is None:
            raise _lib.PgasrError("lstm_layer_fwd: out_drop must have out's size and come with drop = (p, seed, offset)")
    dargs = (_p(out_drop), float(p), int(seed) & (2 ** 64 - 1), int(offset) & 0xFFFFFFFF)
    with _timed("lstm_fwd_kernel"):
        if fed is None:
            st = lib.pgasr_lstm_layer_fwd(_p(gates), _p(out), _p(cbuf), _p(pack_f), _p(lengths), T, B, _lstm_flags(pack_f), *dargs,
                                          _p(ws), ws.numel(), _stream())
        else:
            if fed.dtype != torch.int32 or not fed.is_cuda or fed.numel() < 2 * ((T * B + 255) // 256):
                raise _lib.PgasrError("lstm_layer_fwd: fed must be an int32 GPU tensor of 2 * ceil(T*B/256) words")
            st = lib.pgasr_lstm_layer_fwd_fed(_p(gates), _p(out), _p(cbuf), _p(pack_f), _p(lengths), T, B, _lstm_flags(pack_f),
                                              _p(fed), int(fed_need), *dargs, _p(ws), ws.numel(), _stream())
    _lib.check(st, "pgasr_lstm_layer_fwd_fed" if fed is not None else "pgasr_lstm_layer_fwd")
    return ws


def lstm_fed_ok(T, B):
    """Can a forward sweep of this shape be fed by a concurrent projection GEMM (B <= 32, helpers on)?"""
    return bool(_lib.load().pgasr_lstm_fed_ok(T, B, LSTM_FLAGS))


def x3w_feed_col_tiles(N, planes=2):
    """Column tiles per direction half that ``gemm_x3w_feed`` counts per row tile for an N-column product: the
    ``fed_need`` of the sweep it feeds (0: not a feedable width).  planes: of the W operand (2 / 3, see ``gemm_x3w``)."""
    lib = _lib.load()
    return int(lib.pgasr_gemm_x6w_feed_col_tiles(int(N)) if planes == 3 else lib.pgasr_gemm_x3w_feed_col_tiles(int(N)))


# Tile groups of a feeding GEMM computed IN FRONT of the fed sweep, on its own stream (pgasr_gemm_x3w_feed_f32 phase 1).
# Off by default -- measured round 3 on one box, 40 + 100 steps each: the fed sweeps get shorter (forward 1.15 / 1.11 / 1.09 ->
# 1.10 / 1.08 / 1.06 ms, backward 1.27 -> 1.23-1.25: they no longer sit ~40 us on their first rows) but the head launch itself
# takes the ~30 us it saves, on the same critical stream: 8.49 ms per step without, 8.53 / 8.50 / 8.60 with 2 / 4 / 1 groups.
FEED_HEAD_GROUPS = int(_os_environ_get("PGASR_FEED_HEAD", "0"))


# Six-product feeds (round 5): their K-split head can be a launch of its own (``gemm_x3w_feed(phase=1 / 2, ctrl=...)``,
# pgasr_gemm_x6w_feed_phase_f32) -- right behind the previous sweep instead of behind the consuming sweep's registration, gate and memset
# (the feed otherwise starts ~40 us after the previous sweep's end).  Wired into BLSTMLayerFn twice and measured (tools/dev/r5_side_head.sh, f32
# step, A/B/A/B on one box each): head on the feeding stream 10.00 / 9.90 ms against 9.67 / 9.75 (gate and persistent launch queue behind the
# head kernel: the whole tiles start ~40 us later and the sweep waits for those); head on a stream of its own with caller-zeroed queue words
# 9.79 / 9.785 (9.76 with four or six forward groups in the head) against 9.77 / 9.72 -- nothing.  The wiring was taken out again; the entry
# point stays, covered by test_gemm_x6w_feed_graded_head (same bits as the single launch).


def x3w_feed_head_items(N, K, groups=None, planes=2):
    """Work items of a feed's HEAD launch IN FRONT of the sweep on the sweep's stream (0: this shape / tile structure has none; the
    six-product feeds have none of that kind)."""
    groups = FEED_HEAD_GROUPS if groups is None else groups
    if planes == 3:
        return 0
    return int(_lib.load().pgasr_gemm_x3w_feed_head_items(int(N), int(K), int(groups))) if groups > 0 else 0


def gemm_x3w_feed(A, planes, C, M, N, K, bias, busy_ptr, tiles_done, order=0, phase=0, ws=None, ctrl=None):
    """``gemm_x3w`` in feed-ahead mode on the CURRENT stream (see include/pgasr_hip.h, pgasr_gemm_x3w_feed_f32).
    phase 1 (head, on the sweep's stream in front of the sweep) returns the workspace that the phase-2 call (rest, on
    the feeding stream) must be given as ``ws``: both work on one queue."""
    lib = _lib.load()
    for t, nm in ((A, "A"), (C, "C"), (bias, "bias")):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise _lib.PgasrError(f"gemm_x3w_feed operand {nm} must be a float32 GPU tensor")
    _check_planes(planes, N, K, "gemm_x3w_feed")
    if tiles_done.dtype != torch.int32 or tiles_done.numel() < 2 * ((M + 255) // 256):
        raise _lib.PgasrError("gemm_x3w_feed: tiles_done must hold 2 * ceil(M/256) int32 words")
    if len(planes) == 3:
        if phase == 2 and ws is None:
            raise _lib.PgasrError("gemm_x3w_feed: phase 2 continues the queue of a phase-1 call: pass its workspace")
        if ws is None:
            ws = _workspace(lib.pgasr_gemm_x6w_feed_workspace_bytes(), C.device, "x6w_feed")
        with _timed("gemm_feed_x6c"):        # on the feeding stream: the time includes what the persistent workgroups wait for the sweep
            if ctrl is not None and (ctrl.dtype != torch.int32 or ctrl.numel() < 256 or not ctrl.is_contiguous()):
                raise _lib.PgasrError("gemm_x3w_feed: ctrl = 256 zeroed int32 words")
            st = lib.pgasr_gemm_x6w_feed_phase_f32(M, N, K, A.data_ptr(), K, *_plane_ptrs(planes), C.data_ptr(), N, _p(bias),
                                                   busy_ptr, tiles_done.data_ptr(), int(order), int(phase), _p(ctrl), _p(ws), ws.numel(), _stream())
        _lib.check(st, "pgasr_gemm_x6w_feed_phase_f32")
        return ws if phase == 1 else C
    if ws is None:
        ws = _workspace(lib.pgasr_gemm_x3w_feed_workspace_bytes(), C.device, "x3w_feed")
    with _timed("gemm_feed_x3w"):
        st = lib.pgasr_gemm_x3w_feed_f32(M, N, K, A.data_ptr(), K, planes[0].data_ptr(), planes[1].data_ptr(), C.data_ptr(), N, _p(bias),
                                         busy_ptr, tiles_done.data_ptr(), int(order), int(phase), FEED_HEAD_GROUPS if phase else 0,
                                         _p(ws), ws.numel(), _stream())
    _lib.check(st, "pgasr_gemm_x3w_feed_f32")
    return ws if phase == 1 else C


def lstm_layer_bwd(gates, out, cbuf, dout, pack_b, lengths, T, B, want_dbias=False, fed=None, fed_need=0, drop=None, slab=None):
    """gates := d(pre-activation gates).  want_dbias: also returns the (ceil(B/16), 2*4H) per-group bias-gradient
    partial sums the sweep accumulates on the way (sum its rows).
    fed: counters of a ``gemm_x3w_feed(order=1)`` launched AFTER this call that fills ``dout`` while the sweep runs;
    drop = (p, seed, offset): dout arrives without that dropout mask, the sweep's helpers apply it.
    slab: STREAMED sweep -- int32 tensor of 2 * ceil(B/16) words, zeroed by the caller, in which the sweep counts the time
    slabs (``lstm_wgrad_slabs(T)``) whose dgates rows consumers on other XCDs may read (``lstm_wgrads(slab=...)``)."""
    lib = _lib.load()
    ws = _lstm_ws(T, B, True, gates.device)
    part = torch.empty((B + 15) // 16, 2 * 4 * HID, dtype=torch.float32, device=gates.device) if want_dbias else None
    with _timed("lstm_bwd_kernel"):
        if slab is not None:
            words = slab
            if words.dtype != torch.int32 or not words.is_cuda or words.numel() < 2 * ((B + 15) // 16):
                raise _lib.PgasrError("lstm_layer_bwd: slab_done must be an int32 GPU tensor of 2 * ceil(B/16) words")
            p, seed, offset = drop if drop is not None else (0.0, 0, 0)
            st = lib.pgasr_lstm_layer_bwd_streamed(_p(gates), _p(out), _p(cbuf), _p(dout), _p(pack_b), _p(lengths), T, B, _lstm_flags(pack_b),
                                                   _p(part), _p(fed), int(fed_need), float(p), int(seed), int(offset),
                                                   _p(words), _p(ws), ws.numel(), _stream())
        elif fed is None:
            st = lib.pgasr_lstm_layer_bwd(_p(gates), _p(out), _p(cbuf), _p(dout), _p(pack_b), _p(lengths), T, B, _lstm_flags(pack_b),
                                          _p(part), _p(ws), ws.numel(), _stream())
        else:
            if fed.dtype != torch.int32 or not fed.is_cuda or fed.numel() < 2 * ((T * B + 255) // 256):
                raise _lib.PgasrError("lstm_layer_bwd: fed must be an int32 GPU tensor of 2 * ceil(T*B/256) words")
            p, seed, offset = drop if drop is not None else (0.0, 0, 0)
            st = lib.pgasr_lstm_layer_bwd_fed(_p(gates), _p(out), _p(cbuf), _p(dout), _p(pack_b), _p(lengths), T, B, _lstm_flags(pack_b),
                                              _p(part), _p(fed), int(fed_need), float(p), int(seed), int(offset),
                                              _p(ws), ws.numel(), _stream())
    _lib.check(st, "pgasr_lstm_layer_bwd")
    return (ws, part) if want_dbias else ws


def lstm_wgrad_slabs(T):
    """Frame boundaries 0 = h_0 < .. < h_n = T of the time slabs the weight-gradient products are summed over."""
    import ctypes
    lib = _lib.load()
    n = lib.pgasr_lstm_wgrad_slabs(int(T), None, 0)          # the count alone
    edges = (ctypes.c_int * (n + 1))()
    lib.pgasr_lstm_wgrad_slabs(int(T), ctypes.addressof(edges), n + 1)
    return [int(edges[i]) for i in range(n + 1)]


def lstm_wgrads_ok(T, B, in_dim, planes=None):
    """Shapes ``lstm_wgrads`` takes (the 256 x 256 TN kernels: both products in one launch): the time slabs of the sum must be whole
    k-steps of the kernel -- 16 rows for the six-product kernel of gemm_x6.hip (planes = 3, mode "f32": B % 16 == 0), 32 rows for
    gemm_c256.hip's bf16x3 kernel (planes = 2: B % 32 == 0).  planes = None: the current precision mode's."""
    planes = LSTM_PLANES if planes is None else int(planes)
    return T >= 2 and in_dim % 256 == 0 and B > 0 and B % (16 if planes == 3 else 32) == 0 and T * B * 2048 * 4 < 2 ** 31


def lstm_wgrads(dgates, x, out, T, B, in_dim, dwih, dwhh, busy_ptr=0, slab=None, err_ws=None, planes=None):
    """dwih (2*4H, in_dim) = dgates^T x and dwhh (2, 4H, H) = dgates[d]^T h_prev(d) in one launch, summed over the time slabs
    of ``lstm_wgrad_slabs(T)``.  slab: the slab_done words of the STREAMED sweep that is still writing ``dgates`` on another
    stream; err_ws: that sweep's workspace (its error word is set if a wait gives up).
    planes: 2 = bf16x3 products, 3 = the fp32-faithful six-product arithmetic; None = the current precision mode's."""
    lib = _lib.load()
    planes = LSTM_PLANES if planes is None else int(planes)
    for t_, nm in ((dgates, "dgates"), (x, "x"), (out, "out"), (dwih, "dwih"), (dwhh, "dwhh")):
        _req(t_, torch.float32, nm)
    nbytes = lib.pgasr_lstm_wgrads_workspace_bytes(T, in_dim)
    ws = _workspace(nbytes, dgates.device, "gemm")
    err_ptr = 0
    if err_ws is not None:
        import ctypes
        off = ctypes.c_size_t(0)
        _lib.check(lib.pgasr_lstm_error_offset(B, 1, ctypes.byref(off)), "pgasr_lstm_error_offset")
        err_ptr = err_ws.data_ptr() + off.value
    with _timed("gemm_t6" if planes == 3 else "gemm_t256"):      # streamed (slab != None): includes the waits for the sweep's slabs
        st = lib.pgasr_lstm_wgrads_streamed(_p(dgates), _p(x), _p(out), T, B, in_dim, _p(dwih), _p(dwhh), int(busy_ptr),
                                            _p(slab), err_ptr, planes, _p(ws), ws.numel(), _stream())
    _lib.check(st, "pgasr_lstm_wgrads_streamed")


def lstm_check_error(ws, B, backward):
    """Host-side check (synchronises): raises if a persistent sweep timed out."""
    import ctypes
    lib = _lib.load()
    off = ctypes.c_size_t(0)
    _lib.check(lib.pgasr_lstm_error_offset(B, int(backward), ctypes.byref(off)), "pgasr_lstm_error_offset")
    flag = int(ws[off.value:off.value + 4].view(torch.int32).item())
    if flag != 0:
        raise _lib.PgasrError("persistent LSTM sweep timed out waiting for its cluster (status 5)")


def lstm_assert_no_timeouts():
    """Host-side check of EVERY sweep workspace this process has used (synchronises the current stream): a persistent
    sweep that gave up on a bounded wait -- its cluster, its helpers or the GEMM feeding it never showed up -- leaves
    its sticky error word set and its results are invalid.  ``pgasr_lstm_status`` turns the word into
    PGASR_ERR_TIMEOUT, which is raised here.  Call it wherever the host synchronises anyway (the loss print every
    ``log_every`` steps, before a checkpoint is written, at the end of a benchmark); between two calls the guarded
    Adam (``lstm_error_words``) keeps invalid gradients away from the parameters."""
    lib = _lib.load()
    for key, ws in list(_ws_cache.items()):
        if not key[0].startswith("lstm"):
            continue
        st = lib.pgasr_lstm_status(ws.data_ptr(), ws.numel(), 1, int(key[0] == "lstm_bwd"), _stream())
        if st == _lib.TIMEOUT:
            raise _lib.PgasrError(f"persistent LSTM sweep timed out (status {st}: {lib.pgasr_status_string(st).decode()}) "
                                  f"in workspace {key[0]!r}; its outputs and every gradient since are invalid")
        _lib.check(st, "pgasr_lstm_status")


def lstm_error_words(device):
    """Device addresses of the sticky error words of the sweep workspaces used on the CURRENT stream (at most two:
    forward, backward) -- the guards of ``adam_step``."""
    return [w.data_ptr() for w in lstm_error_word_tensors(device)]


def lstm_error_word_tensors(device):
    """The same words as int32 (1,) views, forward workspace first.  The word's place inside a workspace comes from the library
    (``pgasr_lstm_error_offset``: the same call ``lstm_wgrads`` and ``lstm_check_error`` use), not from an assumption here."""
    import ctypes
    lib = _lib.load()
    cur = torch.cuda.current_stream().cuda_stream
    out = []
    for tag, backward in (("lstm_fwd", 0), ("lstm_bwd", 1)):
        ws = _ws_cache.get((tag, device, cur))
        if ws is None:
            continue
        off = ctypes.c_size_t(0)
        _lib.check(lib.pgasr_lstm_error_offset(1, backward, ctypes.byref(off)), "pgasr_lstm_error_offset")
        out.append(ws[off.value:off.value + 4].view(torch.int32))
    return out


# ------------------------------------------------------------------------------------------
# attention context of the reference's seq2seq decoder (model.py:58-94)
# ------------------------------------------------------------------------------------------
def attention_ctx(dec, enc):
    """dec (NQ,H) or (L,B,H) decoder states (row q belongs to utterance q % B), enc (B,T,H) -> ctx with dec's shape:
    Attention.forward of the reference as executed (include/pgasr_hip.h, pgasr_attention_ctx)."""
    lib = _lib.load()
    _req(dec, torch.float32, "dec"); _req(enc, torch.float32, "enc")
    if enc.dim() != 3 or dec.shape[-1] != enc.shape[2]:
        raise _lib.PgasrError("attention_ctx: enc (B,T,H) and dec (..., H) with the same H (model.py:69: the bmm output is (H,H))")
    B, T, H = enc.shape
    NQ = dec.numel() // H
    if NQ % B:
        raise _lib.PgasrError("attention_ctx: dec must hold a multiple of B rows")
    ctx = torch.empty_like(dec)
    _lib.check(lib.pgasr_attention_ctx(_p(dec), _p(enc), NQ, B, T, H, _p(ctx), _stream()), "pgasr_attention_ctx")
    return ctx


def lstm_cell(gh, xp, c, h, h_out=None):
    """One step of the decoder's LSTM cell in place (include/pgasr_hip.h, pgasr_lstm_cell_f32): gh, xp (B,4H) contiguous,
    c, h (B,H) updated, h_out (B,H) optional copy of the new h (the decoder's output row)."""
    lib = _lib.load()
    for n, t in (("gh", gh), ("xp", xp), ("c", c), ("h", h)):
        _req(t, torch.float32, n)
    B, H = c.shape
    if gh.shape != (B, 4 * H) or xp.shape != (B, 4 * H) or h.shape != (B, H) or not (gh.is_contiguous() and xp.is_contiguous() and c.is_contiguous() and h.is_contiguous()):
        raise _lib.PgasrError("lstm_cell: gh, xp (B,4H) and c, h (B,H), all contiguous")
    if h_out is not None:
        _req(h_out, torch.float32, "h_out")
        if h_out.shape != (B, H) or not h_out.is_contiguous():
            raise _lib.PgasrError("lstm_cell: h_out (B,H) contiguous")
    _lib.check(lib.pgasr_lstm_cell_f32(_p(gh), _p(xp), _p(c), _p(h), _p(h_out), B, H, _stream()),
               "pgasr_lstm_cell_f32")


# ------------------------------------------------------------------------------------------
# prefix beam search
# ------------------------------------------------------------------------------------------
def beam_lm_single_wave_ok(T, V, beam, is_f64, lm_order):
    """Whether ``fast_lm=True`` takes the single-wave kernel's LM instantiations for this shape (pgasr_beam_lm_single_wave_ok: a
    table, fp32 log-probs, beam <= 16, V <= 64, T * beam <= 24576, T <= 4096).  Host only: no device is touched."""
    return bool(_lib.load().pgasr_beam_lm_single_wave_ok(int(T), int(V), int(beam), int(bool(is_f64)), int(lm_order)))


def _search_inputs(log_probs, lengths):
    """The checks the three search wrappers share; returns (T, B, V)."""
    if not log_probs.is_cuda or log_probs.dtype not in (torch.float32, torch.float64):
        raise _lib.PgasrError("log_probs must be a float32/float64 GPU tensor")
    if log_probs.stride(2) != 1:
        raise _lib.PgasrError("log_probs must be contiguous in its last dimension")
    T, B, V = log_probs.shape
    _req(lengths, torch.int32, "lengths")
    return T, B, V


def _nbest_outputs(N, B, T, dev):
    """tokens (N,B,T), lengths (N,B), score (N,B), count (B), uninitialised: the N-best kernels write every word."""
    N = max(N, 0)
    return (torch.empty(N, B, T, dtype=torch.int32, device=dev), torch.empty(N, B, dtype=torch.int32, device=dev),
            torch.empty(N, B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev))


def _lm_table(lm, V, blank, device):
    if lm is None:
        return None, 0
    if lm.vocab != V or lm.blank != int(blank):
        raise ValueError(f"the LM is over {lm.vocab} symbols with blank {lm.blank}; the search has {V} symbols and blank {int(blank)}")
    return lm.device_table(device), lm.order


def _bias_table(bias, V, blank, device, fast_lm=False, fast=False):
    """The bias keywords of the search wrappers: (table tensor, states) of a ``lm.HotwordBias``.  Refusals need no device."""
    from .lm import HotwordBias
    if not isinstance(bias, HotwordBias):
        raise ValueError("bias: a lm.HotwordBias is wanted (never raw tensors)")
    if bias.vocab != V or bias.blank != int(blank):
        raise ValueError(f"bias: the hotwords are over {bias.vocab} symbols with blank {bias.blank}; the call has {V} symbols and "
                         f"blank {int(blank)}")
    if fast_lm:
        raise ValueError("fast_lm: the single-wave kernel has no hotword bias; search with fast_lm=False")
    if fast:
        raise ValueError("fast: the single-wave kernel has no hotword bias; search with fast=False")
    return bias.device_table(device), bias.n_states


def _search_head(log_probs, lengths, T, B, V, beam, blank):
    """The leading C arguments of every search entry, up to the flags."""
    return (_p(log_probs), int(log_probs.dtype == torch.float64), log_probs.stride(0), log_probs.stride(1), _p(lengths), T, B, V,
            int(beam), int(blank))


def ctc_beam_search(log_probs, lengths=None, beam=5, blank=0, collapse=False, out=None, generic=False,
                    lm=None, lm_alpha=0.0, lm_beta=0.0, fast_lm=False, bias=None, bias_weight=0.0):
    """log_probs (T,B,V) fp32 or fp64 natural-log probabilities on the GPU.
    Returns (tokens (B,T) int32, token_lengths (B) int32, score (B) float64 = -log p).
    collapse: the returned tokens have gone through collapse_fn (adjacent duplicates removed, CTCdecoder.py:119-131),
    the form policy_grad.py:8 scores.  out = (tokens, token_lengths) to write into (tokens zero-filled).
    generic: never take the single-wave small-beam kernel (testing).
    lm: None (default: the acoustic search, the kernels and bits it always had) or a ``lm.CharNgramLM`` over the same V symbols and
    blank: every extension by a non-blank s gets ``lm_alpha * ln p_lm(s | context) + lm_beta`` added (pgasr_ctc_beam_search_lm in
    include/pgasr_hip.h).  The returned score is then a FUSED score, not a negative log-likelihood.  With an LM every call takes the
    workgroup-per-utterance kernel, unless
    fast_lm: the call takes the single-wave kernel with the LM term where ``beam_lm_single_wave_ok`` says so (an LM, fp32, beam <= 16,
    V <= 64, T * beam <= 24576, T <= 4096): the same algebra, several times faster; its scores agree with the workgroup kernel's to
    ~1e-7 relative, its hypotheses wherever no two candidates are closer than that.  Without an LM or outside those limits the flag
    changes nothing.
    bias: None (default: the calls above, launch for launch) or a ``lm.HotwordBias`` over the same V symbols and blank: every
    extension by a non-blank s also gets ``bias_weight * bonus(state of the prefix, s)`` added (pgasr_ctc_beam_search_bias;
    include/pgasr_hip.h, A7-BIAS), with or without ``lm``.  Such a call always takes the workgroup-per-utterance kernel -- fast_lm=True
    with it raises --, and bias_weight = 0 returns the words of that kernel without a bias (``generic=True`` without an LM)."""
    if bias is not None:
        bias_table, bias_states = _bias_table(bias, log_probs.shape[-1], blank, log_probs.device, fast_lm=fast_lm)
    lib = _lib.load()
    T, B, V = _search_inputs(log_probs, lengths)
    lm_table, lm_order = _lm_table(lm, V, blank, log_probs.device)
    nbytes = lib.pgasr_beam_workspace_bytes(T, B, V, beam)
    ws = _workspace(nbytes, log_probs.device, "beam")
    if out is not None:
        tokens, tl = out
        _req(tokens, torch.int32, "out tokens"); _req(tl, torch.int32, "out lengths")
        if tokens.numel() != B * T or tl.numel() != B:
            raise _lib.PgasrError("ctc_beam_search: out tensors must hold (B,T) and (B) int32")
    else:
        tokens = torch.zeros(B, T, dtype=torch.int32, device=log_probs.device)
        tl = torch.empty(B, dtype=torch.int32, device=log_probs.device)
    score = torch.empty(B, dtype=torch.float64, device=log_probs.device)
    # one entry point with and without a language model: without a table it IS pgasr_ctc_beam_search
    entry, label, extra = "pgasr_ctc_beam_search_lm", "beam_search", ()
    if bias is not None:
        entry, label, extra = "pgasr_ctc_beam_search_bias", "beam_search_bias", (_p(bias_table), bias_states, float(bias_weight))
    # fast_lm with a bias has raised by name in _bias_table: the bias entry never sees bit 4 (it would refuse it as unsupported)
    with _timed(label):
        st = getattr(lib, entry)(*_search_head(log_probs, lengths, T, B, V, beam, blank),
                                 int(bool(collapse)) | (2 if generic else 0) | (16 if fast_lm else 0),
                                 _p(tokens), _p(tl), _p(score), _p(ws), ws.numel(), _stream(),
                                 _p(lm_table), lm_order, float(lm_alpha), float(lm_beta), *extra)
    _lib.check(st, entry)
    return tokens, tl, score


CTCNBest = collections.namedtuple("CTCNBest", "tokens lengths score count")
NBEST_RESCORE_MAX = 128          # csrc/nbest.hip: hypotheses per utterance


def ctc_beam_search_nbest(log_probs, lengths=None, beam=5, nbest=1, blank=0, collapse=False, lm=None, lm_alpha=0.0, lm_beta=0.0,
                          fast=False, fast_lm=False, bias=None, bias_weight=0.0):
    """The first ``nbest`` entries of the search's final beam (pgasr_ctc_beam_search_nbest): log_probs (T,B,V) fp32 or fp64 as
    ``ctc_beam_search`` takes them, 1 <= nbest <= beam.  Returns ``CTCNBest`` of device tensors, no host synchronisation:
    tokens (N,B,T) int32 (zero behind each hypothesis), lengths (N,B) int32, score (N,B) float64 = -logsumexp(p_blank, p_nonblank)
    of the entry (a FUSED score with ``lm``), count (B) int32 = min(nbest, size of the final beam).  Rank order is the search's own:
    score ascending (probability descending), first touch among equals (with blank != 0 two entries of exactly equal score -- in
    practice of probability zero -- can swap against the reference: include/pgasr_hip.h, A7-NBEST).  Rows beyond count: length 0, score +inf, tokens zero.
    collapse: collapse_fn on each hypothesis separately -- rows that become equal strings are NOT merged.
    Without ``fast`` every call takes the workgroup-per-utterance kernel (fp64 math for fp64 input, the fast path for fp32): row 0 is bit for bit
    ``ctc_beam_search(generic=True)``, or ``ctc_beam_search(lm=...)`` with a language model.  (N,B,T) is the (K,B,stride) layout
    ``ctc_hyp_lattice`` takes.
    fast: the call may take the single-wave kernel of the train step, exactly where ``ctc_beam_search`` takes it by default (no LM,
    fp32, beam <= 16, V <= 64, T * beam <= 24576, T <= 4096); row 0 is then bit for bit ``ctc_beam_search(...)``.  Anywhere else
    the flag changes nothing.
    fast_lm: with ``lm``, the call takes the single-wave kernel's LM instantiations where ``beam_lm_single_wave_ok`` says so (the
    limits of ``fast`` with a table); row 0 is then bit for bit ``ctc_beam_search(lm=..., fast_lm=True)``.  Without an LM or outside
    the limits the flag changes nothing; ``fast`` without it keeps a call with an LM on the workgroup kernel.
    bias / bias_weight: a ``lm.HotwordBias`` as ``ctc_beam_search`` takes it (pgasr_ctc_beam_search_nbest_bias); row 0 is then bit
    for bit ``ctc_beam_search(bias=...)``.  Not with ``fast`` or ``fast_lm`` (ValueError)."""
    if bias is not None:
        bias_table, bias_states = _bias_table(bias, log_probs.shape[-1], blank, log_probs.device, fast_lm=fast_lm, fast=fast)
    lib = _lib.load()
    T, B, V = _search_inputs(log_probs, lengths)
    lm_table, lm_order = _lm_table(lm, V, blank, log_probs.device)
    N, dev = int(nbest), log_probs.device
    ws = _workspace(lib.pgasr_beam_workspace_bytes(T, B, V, int(beam)), dev, "beam")
    tokens, tl, score, count = _nbest_outputs(N, B, T, dev)
    entry, label, extra = "pgasr_ctc_beam_search_nbest", "beam_search_nbest", ()
    if bias is not None:
        entry, label = "pgasr_ctc_beam_search_nbest_bias", "beam_search_nbest_bias"
        extra = (_p(bias_table), bias_states, float(bias_weight))
    # fast / fast_lm with a bias have raised by name in _bias_table: the bias entry never sees bits 3 and 4
    with _timed(label):
        st = getattr(lib, entry)(*_search_head(log_probs, lengths, T, B, V, beam, blank),
                                 int(bool(collapse)) | (8 if fast else 0) | (16 if fast_lm else 0), N, _p(tokens), T, _p(tl), _p(score),
                                 _p(count), _p(ws), ws.numel(), _stream(), _p(lm_table), lm_order, float(lm_alpha), float(lm_beta), *extra)
    _lib.check(st, entry)
    return CTCNBest(tokens, tl, score, count)


def ctc_beam_search_words(log_probs, lengths=None, beam=5, nbest=1, blank=0, collapse=False, fusion=None, alpha=0.0, beta=0.0,
                          finalize=True, eos=True):
    """The N-best search with a word n-gram model and its lexicon fused into it (pgasr_ctc_beam_search_words; include/pgasr_hip.h,
    A7-WORDFUSE): log_probs (T,B,V) fp32 or fp64 as ``ctc_beam_search_nbest`` takes them, 1 <= nbest <= beam, ``fusion`` a
    ``lm.WordFusion`` over the same V <= 64 symbols and blank.  Every extension by a non-blank s gets ``fusion.bonus(prefix, s, alpha,
    beta)`` added: the lexicon's ``oov_penalty`` on the way out of the lexicon, and ``alpha * ln p(word | history) + beta`` at every
    word end.  Returns ``CTCNBest`` of device tensors, no host synchronisation; the scores are FUSED scores.
    finalize (default): every entry of the final beam also gets ``fusion.final(prefix, alpha, beta, eos)`` -- the bonus of its pending
    word and, with ``eos``, ``alpha * ln p(</s> | history)`` --, and the list is the final beam ranked again with it (equal totals in
    the search's order).  finalize=False: the search's own list, nothing added (``eos`` is then not consulted).
    Always the workgroup-per-utterance kernel; the 1-best is row 0 at nbest = 1.  alpha = beta = 0 with a fusion of oov_penalty 0 and
    eos=False returns every word of ``ctc_beam_search_nbest`` bit for bit."""
    from .lm import WordFusion
    if not isinstance(fusion, WordFusion):
        raise ValueError("fusion: a lm.WordFusion is wanted (never raw tensors)")
    V = log_probs.shape[-1]
    if fusion.vocab != V or fusion.blank != int(blank):
        raise ValueError(f"fusion: the lexicon is over {fusion.vocab} symbols with blank {fusion.blank}; the call has {V} symbols and "
                         f"blank {int(blank)}")
    alpha, beta = float(alpha), float(beta)
    for name, x in (("alpha", alpha), ("beta", beta)):
        if x != x or x in (float("inf"), -float("inf")):
            raise ValueError(f"{name}: a finite weight is wanted (got {x!r})")
    lib = _lib.load()
    T, B, V = _search_inputs(log_probs, lengths)
    N, dev = int(nbest), log_probs.device
    tabs = fusion.device_tables(dev)
    ws = _workspace(lib.pgasr_beam_workspace_bytes(T, B, V, int(beam)), dev, "beam")
    tokens, tl, score, count = _nbest_outputs(N, B, T, dev)
    with _timed("beam_search_words"):
        st = lib.pgasr_ctc_beam_search_words(*_search_head(log_probs, lengths, T, B, V, beam, blank), int(bool(collapse)), N, _p(tokens), T,
                                             _p(tl), _p(score), _p(count), _p(ws), ws.numel(), _stream(), None, 0, 0.0, 0.0,
                                             _p(tabs.trie), fusion.n_states, _p(tabs.node_word), ctypes.byref(tabs.word_lm.struct),
                                             fusion.delimiter, alpha, beta, (1 if finalize else 0) | (2 if eos else 0))
    _lib.check(st, "pgasr_ctc_beam_search_words")
    return CTCNBest(tokens, tl, score, count)


MAX_VOCAB_SEARCH_WIDE = 1024     # csrc/beam_wide.hip: the exact prefix beam search over rows of up to 1024 symbols


BIAS_SCORE_MAX_VOCAB = 1024      # csrc/hotword.hip


def nbest_bias_score(tokens, lengths, count, bias):
    """A hotword bias over N-best lists (pgasr_nbest_bias_score; include/pgasr_hip.h, A7-BIAS): tokens (N,B,stride) / lengths (N,B) /
    count (B) int32 as the searches return them (narrow or wide), ``bias`` a ``lm.HotwordBias``.  Returns bias_score (N,B) float64, no
    host synchronisation: per hypothesis what ``bias.score_sequence`` returns, bit for bit -- the fp64 sum of the fp32 bonuses in token
    order; 0 in the rows beyond count.  A blank or an id outside the vocabulary adds nothing.  N <= 128, at most 1024 symbols."""
    from .lm import HotwordBias
    if not isinstance(bias, HotwordBias):
        raise ValueError("bias: a lm.HotwordBias is wanted (never raw tensors)")
    lib = _lib.load()
    _req(tokens, torch.int32, "tokens"); _req(lengths, torch.int32, "lengths"); _req(count, torch.int32, "count")
    if tokens.dim() != 3 or tuple(lengths.shape) != tuple(tokens.shape[:2]) or count.numel() != tokens.shape[1]:
        raise _lib.PgasrError("nbest_bias_score wants tokens (N,B,stride), lengths (N,B) and count (B)")
    N, B, stride = tokens.shape
    table = bias.device_table(tokens.device)
    out = torch.empty(N, B, dtype=torch.float64, device=tokens.device)
    with _timed("nbest_bias_score"):
        st = lib.pgasr_nbest_bias_score(_p(tokens), _p(lengths), _p(count), N, B, stride, bias.vocab, _p(table), bias.n_states,
                                        _p(out), _stream())
    _lib.check(st, "pgasr_nbest_bias_score")
    return out


def _unit_lm_check(unit_lm, V, blank):
    """Refusals that need no device: the model's type, its vocabulary and its blank."""
    if not hasattr(unit_lm, "device_tables") or not hasattr(unit_lm, "logp_sequence"):
        raise ValueError("unit_lm: a lm.UnitNgramLM is wanted")
    if unit_lm.vocab != V or unit_lm.blank != int(blank):
        raise ValueError(f"unit_lm: the model is over {unit_lm.vocab} symbols with blank {unit_lm.blank}; the call has {V} symbols and "
                         f"blank {int(blank)}")


def ctc_beam_search_wide(log_probs, lengths=None, beam=5, nbest=None, blank=0, collapse=False, counting=False, stats=False,
                         unit_lm=None, lm_alpha=0.0, lm_beta=0.0, bias=None, bias_weight=0.0):
    """The exact prefix beam search over rows of up to MAX_VOCAB_SEARCH_WIDE = 1024 symbols (pgasr_ctc_beam_search_wide; narrower
    rows are taken too): log_probs (T,B,V) fp32 or fp64 as ``ctc_beam_search`` takes them, beam <= 128, no language model.
    nbest=None (default): the triple of ``ctc_beam_search`` -- tokens (B,T) int32, token_lengths (B) int32, score (B) float64.
    nbest=N, 1 <= N <= beam: ``CTCNBest`` as ``ctc_beam_search_nbest`` returns it -- tokens (N,B,T), lengths (N,B), score (N,B),
    count (B) --, rank order score ascending, first touch among equals, without the exception noted there.
    No host synchronisation.  collapse: collapse_fn on each hypothesis separately.
    counting: every frame takes the counting selection instead of the threshold list (the same result bit for bit; tests, timing).
    stats: the counting-frames tensor (B) int32 -- frames of each utterance that took the counting selection -- is returned as one
    more value behind the result.
    unit_lm: None (default: the acoustic search, the kernels and bits it always had) or a ``lm.UnitNgramLM`` over the same V symbols
    and blank: every extension by a non-blank s gets ``lm_alpha * ln p_lm(s | context) + lm_beta`` added (pgasr_ctc_beam_search_wide_lm;
    include/pgasr_hip.h, A7-WIDE-LM) and the returned score is a FUSED score.  lm_alpha = lm_beta = 0 returns the words of the call
    without a model.
    bias: None (default: the calls above, launch for launch) or a ``lm.HotwordBias`` over the same V symbols and blank: every
    extension by a non-blank s also gets ``bias_weight * bonus(state of the prefix, s)`` added inside the search
    (pgasr_ctc_beam_search_wide_bias; include/pgasr_hip.h, A7-WIDE-BIAS), with or without ``unit_lm``; the returned score is a FUSED
    score.  bias_weight = 0 returns the words of the call without a bias."""
    if unit_lm is not None:
        _unit_lm_check(unit_lm, log_probs.shape[-1], blank)
    if bias is not None:
        bias_table, bias_states = _bias_table(bias, log_probs.shape[-1], blank, log_probs.device)
    lib = _lib.load()
    T, B, V = _search_inputs(log_probs, lengths)
    N, dev = (1 if nbest is None else int(nbest)), log_probs.device
    if unit_lm is None:
        entry, label, ws_bytes, lm_args = "pgasr_ctc_beam_search_wide", "beam_search_wide", lib.pgasr_beam_wide_workspace_bytes, ()
    else:
        entry, label, ws_bytes = "pgasr_ctc_beam_search_wide_lm", "beam_search_wide_lm", lib.pgasr_beam_wide_lm_workspace_bytes
        lm_args = (ctypes.byref(unit_lm.device_tables(dev).struct), float(lm_alpha), float(lm_beta))
    if bias is not None:     # one entry for both: the model's arguments (NULL tables without one), then the automaton's
        entry, label = "pgasr_ctc_beam_search_wide_bias", "beam_search_wide_bias"
        lm_args = (lm_args or (None, 0.0, 0.0)) + (_p(bias_table), bias_states, float(bias_weight))
    ws = _workspace(ws_bytes(T, B, V, int(beam)), dev, "beam_wide")
    tokens, tl, score, count = _nbest_outputs(N, B, T, dev)
    frames = torch.empty(B, dtype=torch.int32, device=dev) if stats else None
    with _timed(label):
        st = getattr(lib, entry)(*_search_head(log_probs, lengths, T, B, V, beam, blank), int(bool(collapse)) | (32 if counting else 0), N,
                                 _p(tokens), T, _p(tl), _p(score), _p(count), _p(frames), _p(ws), ws.numel(), _stream(), *lm_args)
    _lib.check(st, entry)
    res = (tokens[0], tl[0], score[0]) if nbest is None else CTCNBest(tokens, tl, score, count)
    return (res, frames) if stats else res


def mwer_weights(dist, risk_len, target_lengths, hyp_nll, hyp_len, count, nll, Lh, lam, inv_global_batch):
    """Posterior, risks and gradient coefficients of MWER over an N-best list (pgasr_mwer_weights; include/pgasr_hip.h, A13-MWER):
    dist (N,B) int32 (word) edit distances, risk_len (B) int32 what normalises them, target_lengths (B) int32, hyp_nll (N,B) fp32 the
    exact CTC nll of every hypothesis, hyp_len (N,B) / count (B) int32 the list's, nll (B) fp32 the target's.
    Returns (p (N,B), r (N,B), coef (N,B), utt_scale (B), rbar (B), terms (B)) fp32; one launch, no host synchronisation."""
    lib = _lib.load()
    _req(dist, torch.int32, "dist"); _req(risk_len, torch.int32, "risk_len"); _req(target_lengths, torch.int32, "target_lengths")
    _req(hyp_nll, torch.float32, "hyp_nll"); _req(hyp_len, torch.int32, "hyp_len"); _req(count, torch.int32, "count")
    _req(nll, torch.float32, "nll")
    if hyp_nll.dim() != 2:
        raise _lib.PgasrError("mwer_weights wants hyp_nll (N,B)")
    N, B = hyp_nll.shape
    if dist.numel() != N * B or tuple(hyp_len.shape) != (N, B) or any(t_.numel() != B for t_ in (risk_len, target_lengths, count, nll)):
        raise _lib.PgasrError(f"mwer_weights wants dist, hyp_nll, hyp_len ({N},{B}) and risk_len, target_lengths, count, nll ({B},)")
    out = torch.empty(3 * N + 3, B, dtype=torch.float32, device=hyp_nll.device)
    p, r, coef, rest = out[:N], out[N:2 * N], out[2 * N:3 * N], out[3 * N:]
    st = lib.pgasr_mwer_weights(_p(dist), _p(risk_len), _p(target_lengths), _p(hyp_nll), _p(hyp_len), _p(count), _p(nll), N, B, int(Lh),
                                float(lam), float(inv_global_batch), p.data_ptr(), r.data_ptr(), coef.data_ptr(),
                                rest[0].data_ptr(), rest[1].data_ptr(), rest[2].data_ptr(), _stream())
    _lib.check(st, "pgasr_mwer_weights")
    return p, r, coef, rest[0], rest[1], rest[2]


def ctc_grad_from_lattices_nbest(log_probs, input_lengths, target_lengths, handle, hyp_handle, utt_scale, coef, hyp_len, wide=None):
    """``ctc_grad_from_lattices_seq`` without sampled paths (pgasr_ctc_grad_from_lattices_nbest): utt_scale (softmax - occ_target) +
    sum_n coef[n,b] (softmax - occ_{y_n}) over the N*B hypothesis lattices of ``ctc_hyp_lattice``, the N terms in n order.  coef (N,B)
    fp32; hyp_len (N,B) int32 is the tensor ``ctc_hyp_lattice`` was given.
    V > 64 (or wide=True): ``pgasr_ctc_grad_from_lattices_seq_wide`` without a path tensor, its N-best form."""
    hws, N, Lh = hyp_handle
    T, B, V = log_probs.shape
    _req(hyp_len, torch.int32, "hyp_len")
    if tuple(coef.shape) != (N, B) or tuple(hyp_len.shape) != (N, B):
        raise _lib.PgasrError(f"ctc_grad_from_lattices_nbest wants coef and hyp_len ({N},{B})")
    if _wide(V, wide, "ctc_grad_from_lattices_nbest"):
        return _grad_pass("pgasr_ctc_grad_from_lattices_seq_wide", log_probs, input_lengths, target_lengths, handle, utt_scale,
                          dict(K=N, pg_coef=coef, pg_paths=None, hyp_len=hyp_len, Lh=Lh), hyp_handle=hyp_handle,
                          label="ctc_grad_seq_wide_kernel", nullable_tails=True)
    return _grad_pass("pgasr_ctc_grad_from_lattices_nbest", log_probs, input_lengths, target_lengths, handle, utt_scale,
                      dict(N=N, coef=coef, hyp_len=hyp_len, Lh=Lh), hyp_handle=hyp_handle, label="ctc_grad_nbest_kernel")


def nbest_rescore(tokens, lengths, count, am, vocab, blank=0, lm=None, am_weight=1.0, lm_alpha=0.0, lm_beta=0.0):
    """Second pass over N-best lists (pgasr_nbest_rescore): tokens (N,B,stride) / lengths (N,B) / count (B) int32 as
    ``ctc_beam_search_nbest`` returns them, am (N,B) float64 acoustic scores (lower is better), ``vocab`` the number of symbols.
    Returns (order (B,N) int32, total (N,B) float64, lm_logp (N,B) float64), no host synchronisation:
    lm_logp = the hypothesis' log-probability under ``lm`` (0 without one), total = am_weight * am - lm_alpha * lm_logp -
    lm_beta * length (lower is better; +inf for a non-finite am and for rows beyond count), order[b] = the stable ascending
    rank of total over the utterance's count hypotheses (ties keep the list's order), then the remaining rows.  N <= 128."""
    lib = _lib.load()
    _req(tokens, torch.int32, "tokens"); _req(lengths, torch.int32, "lengths"); _req(count, torch.int32, "count")
    _req(am, torch.float64, "am")
    if tokens.dim() != 3 or tuple(lengths.shape) != tuple(tokens.shape[:2]) or tuple(am.shape) != tuple(tokens.shape[:2]) \
            or count.numel() != tokens.shape[1]:
        raise _lib.PgasrError("nbest_rescore wants tokens (N,B,stride), lengths (N,B), am (N,B) and count (B)")
    N, B, stride = tokens.shape
    lm_table, lm_order = _lm_table(lm, int(vocab), blank, tokens.device)
    order = torch.empty(B, N, dtype=torch.int32, device=tokens.device)
    total = torch.empty(N, B, dtype=torch.float64, device=tokens.device)
    lm_logp = torch.empty(N, B, dtype=torch.float64, device=tokens.device)
    with _timed("nbest_rescore"):
        st = lib.pgasr_nbest_rescore(_p(tokens), stride, _p(lengths), _p(count), _p(am), N, B, int(vocab), int(blank),
                                     _p(lm_table), lm_order, float(am_weight), float(lm_alpha), float(lm_beta),
                                     _p(lm_logp), _p(total), _p(order), _stream())
    _lib.check(st, "pgasr_nbest_rescore")
    return order, total, lm_logp


WORD_LM_MAX_STRIDE = 4096        # csrc/word_lm.hip: the row of tokens, its words and their scores live in 64 KB of LDS


def nbest_word_lm_score(tokens, lengths, count, word_lm, delimiter):
    """A word n-gram LM over N-best lists (pgasr_nbest_word_lm_score; include/pgasr_hip.h, A7-WORDLM): tokens (N,B,stride) /
    lengths (N,B) / count (B) int32 as ``ctc_beam_search_nbest`` returns them, ``word_lm`` a ``lm.WordNgramLM``, ``delimiter`` the
    token id that separates words.  Returns (word_logp (N,B) float64, n_words (N,B) int32, n_oov (N,B) int32), no host
    synchronisation: per hypothesis what ``word_lm.logp_sentence`` returns, bit for bit; zeros in the rows beyond count.
    N <= 128, stride <= WORD_LM_MAX_STRIDE."""
    lib = _lib.load()
    _req(tokens, torch.int32, "tokens"); _req(lengths, torch.int32, "lengths"); _req(count, torch.int32, "count")
    if tokens.dim() != 3 or tuple(lengths.shape) != tuple(tokens.shape[:2]) or count.numel() != tokens.shape[1]:
        raise _lib.PgasrError("nbest_word_lm_score wants tokens (N,B,stride), lengths (N,B) and count (B)")
    if not hasattr(word_lm, "device_tables"):
        raise _lib.PgasrError("nbest_word_lm_score wants a lm.WordNgramLM")
    N, B, stride = tokens.shape
    tables = word_lm.device_tables(tokens.device)
    out = torch.empty(2, N, B, dtype=torch.int32, device=tokens.device)
    word_logp = torch.empty(N, B, dtype=torch.float64, device=tokens.device)
    with _timed("nbest_word_lm_score"):
        st = lib.pgasr_nbest_word_lm_score(_p(tokens), stride, _p(lengths), _p(count), N, B, int(delimiter), ctypes.byref(tables.struct),
                                           _p(word_logp), out[0].data_ptr(), out[1].data_ptr(), _stream())
    _lib.check(st, "pgasr_nbest_word_lm_score")
    return word_logp, out[0], out[1]


def nbest_unit_lm_score(tokens, lengths, count, unit_lm):
    """A back-off unit n-gram LM over N-best lists (pgasr_nbest_unit_lm_score; include/pgasr_hip.h, A7-WIDE-LM): tokens (N,B,stride) /
    lengths (N,B) / count (B) int32 as the searches return them, ``unit_lm`` a ``lm.UnitNgramLM``.  Returns lm_logp (N,B) float64, no
    host synchronisation: per hypothesis what ``unit_lm.logp_sequence`` returns, bit for bit; 0 in the rows beyond count, -inf for a
    row holding the blank or a symbol outside the model's vocabulary.  N <= 128."""
    _unit_lm_check(unit_lm, getattr(unit_lm, "vocab", 0), getattr(unit_lm, "blank", 0))
    lib = _lib.load()
    _req(tokens, torch.int32, "tokens"); _req(lengths, torch.int32, "lengths"); _req(count, torch.int32, "count")
    if tokens.dim() != 3 or tuple(lengths.shape) != tuple(tokens.shape[:2]) or count.numel() != tokens.shape[1]:
        raise _lib.PgasrError("nbest_unit_lm_score wants tokens (N,B,stride), lengths (N,B) and count (B)")
    N, B, stride = tokens.shape
    tables = unit_lm.device_tables(tokens.device)
    lm_logp = torch.empty(N, B, dtype=torch.float64, device=tokens.device)
    with _timed("nbest_unit_lm_score"):
        st = lib.pgasr_nbest_unit_lm_score(_p(tokens), stride, _p(lengths), _p(count), N, B, unit_lm.vocab, unit_lm.blank,
                                           ctypes.byref(tables.struct), _p(lm_logp), _stream())
    _lib.check(st, "pgasr_nbest_unit_lm_score")
    return lm_logp


def nbest_combine_rank(base, word_logp, n_words, count, word_alpha=0.0, word_beta=0.0):
    """A word LM's score on top of an earlier pass (pgasr_nbest_combine_rank): base, word_logp (N,B) float64, n_words (N,B) int32,
    count (B) int32.  Returns (order (B,N) int32, total (N,B) float64), no host synchronisation:
    total = base - word_alpha * word_logp - word_beta * n_words (lower is better; +inf for a non-finite base and for rows beyond
    count), order as ``nbest_rescore`` ranks.  N <= 128."""
    lib = _lib.load()
    _req(base, torch.float64, "base"); _req(word_logp, torch.float64, "word_logp"); _req(n_words, torch.int32, "n_words")
    _req(count, torch.int32, "count")
    if base.dim() != 2 or tuple(word_logp.shape) != tuple(base.shape) or tuple(n_words.shape) != tuple(base.shape) \
            or count.numel() != base.shape[1]:
        raise _lib.PgasrError("nbest_combine_rank wants base, word_logp, n_words (N,B) and count (B)")
    N, B = base.shape
    order = torch.empty(B, N, dtype=torch.int32, device=base.device)
    total = torch.empty(N, B, dtype=torch.float64, device=base.device)
    with _timed("nbest_combine_rank"):
        st = lib.pgasr_nbest_combine_rank(_p(base), _p(word_logp), _p(n_words), _p(count), N, B, float(word_alpha), float(word_beta),
                                          _p(total), _p(order), _stream())
    _lib.check(st, "pgasr_nbest_combine_rank")
    return order, total


PAIR_DIST_MAX_LEN = 1024         # csrc/mbr.hip: 16 blocks of 64 pattern positions
PAIR_DIST_CHUNK_ELEMS = 1 << 24  # the composed path: int32 words of expanded rows per chunk of pairs (64 MB)
# Where the composed path is the faster one (MI355X, tools/dev/mbr_cost.py, NOTES.md 0.20): few pairs of long hypotheses.  A lane of
# the bit-vector kernel walks its pair alone, 1.3 - 1.7 ms at 930 symbols however few pairs there are; a wave per pair takes 0.97 /
# 1.19 ms there for 192 / 896 pairs (B = 32, N = 4 / 8).  From 16 hypotheses per list, or at 232 symbols, the kernel wins at every
# size measured.
PAIR_DIST_COMPOSED_MAX_PAIRS = 1024
PAIR_DIST_COMPOSED_MIN_LEN = 640


def _pair_distance_composed(tokens, lengths, count, vocab, cap, unit, delimiter):
    """The unordered pairs of every list through the wave-per-pair kernels (``edit_distance`` / ``word_edit_distance``), expanded in
    chunks of at most PAIR_DIST_CHUNK_ELEMS words, scattered into (B,N,N) with pgasr_nbest_pair_dist's -1 convention."""
    N, B, stride = tokens.shape
    dev = tokens.device
    S = max(1, min(stride, int(cap)))                       # a valid hypothesis has no token behind min(stride, cap)
    ln = lengths.clamp(0, stride)
    valid = (torch.arange(N, device=dev).view(N, 1) < count.clamp(0, N).view(1, B)) & (ln <= int(cap))       # (N,B)
    ln = torch.where(valid, ln, torch.zeros_like(ln))
    dist = torch.full((B, N, N), -1, dtype=torch.int32, device=dev)
    diag = torch.arange(N, device=dev)
    dist[:, diag, diag] = torch.where(valid.t(), 0, -1).to(torch.int32)
    P = N * (N - 1) // 2
    if P == 0:
        return dist
    iu = torch.triu_indices(N, N, offset=1, device=dev)      # (2,P): n < m
    words_per_pair = (2 if unit == "char" else 4) * (S + 1)
    step = max(1, PAIR_DIST_CHUNK_ELEMS // words_per_pair)
    flat = dist.view(-1)
    for q0 in range(0, B * P, step):
        q = torch.arange(q0, min(q0 + step, B * P), device=dev)
        b, pr = q // P, q % P
        n, m = iu[0, pr], iu[1, pr]
        ref, hyp = tokens[n, b, :S].contiguous(), tokens[m, b, :S].contiguous()
        rl, hl = ln[n, b].contiguous(), ln[m, b].contiguous()
        if unit == "char":
            # pgasr_nbest_pair_dist's rule: a symbol outside [0, vocab) matches nothing, not even itself
            ref = torch.where((ref >= 0) & (ref < int(vocab)), ref, torch.full_like(ref, -1))
            hyp = torch.where((hyp >= 0) & (hyp < int(vocab)), hyp, torch.full_like(hyp, -2))
            d = edit_distance(ref, rl, hyp, hl)
        else:
            d = word_edit_distance(ref, rl, hyp, hl, int(delimiter))[0]
        d = torch.where(valid[n, b] & valid[m, b], d, torch.full_like(d, -1))
        flat[(b * N + n) * N + m] = d
        flat[(b * N + m) * N + n] = d
    return dist


def nbest_pair_distance(tokens, lengths, count, vocab, max_hyp_len=None, unit="char", delimiter=None):
    """The edit distances inside each N-best list: tokens (N,B,stride) / lengths (N,B) / count (B) int32 as ``ctc_beam_search_nbest``
    returns them, ``vocab`` the number of symbols.  Returns dist (B,N,N) int32: dist[b,n,m] = dist[b,m,n] = the Levenshtein distance of
    hypotheses n and m of utterance b, 0 on the diagonal, and -1 wherever n or m lies beyond count[b] or is longer than the cap (its own
    diagonal included).  N <= 128.
    unit="char" (default): the list's own units -- characters, or the subword units of a wide alphabet --, by pgasr_nbest_pair_dist
        (Myers' bit-vector algorithm, one lane per pair, one launch; vocab <= 64); a symbol outside [0, vocab) matches nothing, not
        even itself.  Lists whose cap exceeds 1024 take the composed path: the unordered pairs expanded in bounded chunks through
        ``edit_distance`` (one wave per pair), the same result -- and so do at most PAIR_DIST_COMPOSED_MAX_PAIRS pairs with a cap
        from PAIR_DIST_COMPOSED_MIN_LEN, where that path measured faster, and every list over more than 64 symbols (up to 1024).
    unit="word": words split at the token ``delimiter`` as str.split(" ") cuts them (``word_edit_distance`` on the composed path);
        vocab <= 64 only (ValueError above: a subword unit may span a space).
    max_hyp_len: the cap.  None: the longest hypothesis of the lists, read from the device (ONE host synchronisation, as in
        ``CTCDecoder.rescore``; unit="word" needs none) -- nothing is over it.  A number avoids the synchronisation.
    A list of subword units is counted in characters or words of its text by ``nbest_pair_distance_spelled``."""
    _lib.load()
    _req(tokens, torch.int32, "tokens"); _req(lengths, torch.int32, "lengths"); _req(count, torch.int32, "count")
    if tokens.dim() != 3 or tuple(lengths.shape) != tuple(tokens.shape[:2]) or count.numel() != tokens.shape[1]:
        raise _lib.PgasrError("nbest_pair_distance wants tokens (N,B,stride), lengths (N,B) and count (B)")
    if unit not in ("char", "word"):
        raise ValueError(f"unit must be 'char' or 'word' (got {unit!r})")
    if unit == "word" and (delimiter is None or int(delimiter) < 0):
        raise ValueError("unit='word' needs delimiter, the token id of the alphabet's ' ' symbol")
    wide = int(vocab) > MAX_VOCAB_NARROW
    if wide and unit == "word":
        raise ValueError(f"unit='word': not over {int(vocab)} > {MAX_VOCAB_NARROW} symbols -- a subword unit may span a space, so words "
                         f"cannot be split at a delimiter token; take unit='char' (the units are the symbols)")
    N, B, stride = tokens.shape
    if N < 1 or N > NBEST_RESCORE_MAX:
        raise _lib.PgasrError(f"nbest_pair_distance takes 1 <= N <= {NBEST_RESCORE_MAX} hypotheses per utterance (got {N})")
    if max_hyp_len is not None:
        cap = int(max_hyp_len)
        if cap < 0:
            raise ValueError(f"max_hyp_len must be >= 0 (got {max_hyp_len})")
    elif unit == "word":
        cap = stride
    else:
        rows = torch.arange(N, device=tokens.device).view(N, 1) < count.view(1, B)
        cap = int((lengths.clamp(0, stride) * rows).max().item())
    few_and_long = B * N * (N - 1) // 2 <= PAIR_DIST_COMPOSED_MAX_PAIRS and cap >= PAIR_DIST_COMPOSED_MIN_LEN
    if unit == "word" or wide or cap > PAIR_DIST_MAX_LEN or few_and_long:
        with _timed("nbest_pair_dist_composed"):
            return _pair_distance_composed(tokens, lengths, count, vocab, cap, unit, delimiter)
    return _pair_distance_kernel(tokens, lengths, count, vocab, cap)


def nbest_pair_distance_spelled(tokens, lengths, count, spelling, max_hyp_len=None, unit="char"):
    """``nbest_pair_distance`` over the SPELLED text of a list of subword units (``nbest_pair_distance``'s own parameter list is
    fixed, so the spelling has an entry of its own): the list is spelled first (``unit_spell``, one launch) and is then a list over
    at most 64 character ids that takes the paths there by its rules -- unit="char" counts the characters of the text (the
    bit-vector kernel or the composed path, by the length rule), unit="word" its words, split at the spelling's " " (the composed
    word path).  max_hyp_len caps the spelled rows."""
    if unit not in ("char", "word"):
        raise ValueError(f"unit must be 'char' or 'word' (got {unit!r})")
    delimiter = spelling.word_delimiter() if unit == "word" else None
    _req(tokens, torch.int32, "tokens"); _req(lengths, torch.int32, "lengths")
    if tokens.dim() != 3 or tuple(lengths.shape) != tuple(tokens.shape[:2]):
        raise _lib.PgasrError("nbest_pair_distance_spelled wants tokens (N,B,stride), lengths (N,B) and count (B)")
    chars, char_len = unit_spell(tokens, lengths, spelling)
    return nbest_pair_distance(chars, char_len, count, spelling.n_symbols, max_hyp_len=max_hyp_len, unit=unit, delimiter=delimiter)


def _pair_distance_kernel(tokens, lengths, count, vocab, cap):
    """pgasr_nbest_pair_dist itself: one launch, no host synchronisation; cap <= 1024, vocab <= 64."""
    N, B, stride = tokens.shape
    dist = torch.empty(B, N, N, dtype=torch.int32, device=tokens.device)      # the kernel writes every word
    with _timed("nbest_pair_dist"):
        st = _lib.load().pgasr_nbest_pair_dist(_p(tokens), stride, _p(lengths), _p(count), N, B, int(vocab), int(cap), _p(dist),
                                               _stream())
    _lib.check(st, "pgasr_nbest_pair_dist")
    return dist


def mbr_select(dist, score, count, scale=1.0):
    """Minimum-Bayes-risk selection over N-best lists (pgasr_mbr_select; include/pgasr_hip.h, A7-MBR): dist (B,N,N) int32 as
    ``nbest_pair_distance`` returns it (or any matrix in that layout), score (N,B) float64 with lower better, count (B) int32.
    Returns (best (B) int32, risk (N,B) float64, posterior (N,B) float64), no host synchronisation: posterior = the softmax of
    -scale * score over the valid rows (n < count, finite score, dist[b,n,n] >= 0; 0 elsewhere), risk[n] = sum_m posterior[m] *
    dist[n,m] (+inf where not valid), best = the first row of least risk (0 when no row is valid).  scale = 0: a uniform posterior."""
    lib = _lib.load()
    _req(dist, torch.int32, "dist"); _req(score, torch.float64, "score"); _req(count, torch.int32, "count")
    if dist.dim() != 3 or dist.shape[1] != dist.shape[2] or tuple(score.shape) != (dist.shape[1], dist.shape[0]) \
            or count.numel() != dist.shape[0]:
        raise _lib.PgasrError("mbr_select wants dist (B,N,N), score (N,B) and count (B)")
    B, N, _ = dist.shape
    dev = dist.device
    out = torch.empty(2, N, B, dtype=torch.float64, device=dev)
    best = torch.empty(B, dtype=torch.int32, device=dev)
    with _timed("mbr_select"):
        st = lib.pgasr_mbr_select(_p(dist), _p(score), _p(count), N, B, float(scale), out[1].data_ptr(), out[0].data_ptr(), _p(best),
                                  _stream())
    _lib.check(st, "pgasr_mbr_select")
    return best, out[0], out[1]


# ------------------------------------------------------------------------------------------
# dropout / Adam
# ------------------------------------------------------------------------------------------
def dropout(x, p, seed, offset, out=None, dact_y=None, slope=0.01):
    """Inverted dropout; with ``dact_y`` the result is also multiplied by leaky'(dact_y) (fused backward)."""
    lib = _lib.load()
    _req(x, torch.float32, "x"); _req(dact_y, torch.float32, "dact_y")
    if dact_y is not None and dact_y.numel() != x.numel():
        raise _lib.PgasrError("dropout: dact_y must have x's size")
    if out is None:
        out = torch.empty_like(x)
    _lib.check(lib.pgasr_dropout(_p(x), _p(out), x.numel(), float(p), int(seed) & (2 ** 64 - 1),
                                 int(offset) & 0xFFFFFFFF, _p(dact_y), float(slope), _stream()), "pgasr_dropout")
    return out


def stream_copy(dst, src, workgroups=8):
    """dst (GPU tensor) <- src: a GPU tensor or a PINNED host tensor (mapped into the device's address space), same
    dtype and element count, both contiguous.  A kernel on the current stream; never blocks the host."""
    lib = _lib.load()
    if not dst.is_cuda or not dst.is_contiguous() or not src.is_contiguous() or dst.dtype != src.dtype or dst.numel() != src.numel():
        raise _lib.PgasrError("stream_copy: contiguous tensors of one dtype and size, destination on the GPU")
    if not src.is_cuda and not src.is_pinned():
        raise _lib.PgasrError("stream_copy: a host source must be pinned (device-mapped) memory")
    nbytes = dst.numel() * dst.element_size()
    if nbytes == 0:
        return dst
    _lib.check(lib.pgasr_stream_copy(src.data_ptr(), dst.data_ptr(), nbytes, int(workgroups), _stream()), "pgasr_stream_copy")
    return dst


CLIP_STATE_WORDS = 8    # PGASR_CLIP_STATE_BYTES / 4: norm, scale (fp32); nonfinite, pad, n_clipped, n_nonfinite (int32); 2 spare


def clip_state(device):
    """A zeroed clip state for ``grad_norm_clip`` / ``adam_step(clip_state=...)``: fp32 (8,); ``state[0]`` is the norm, ``state[1]`` the
    scale, ``clip_state_counts`` reads the integer words."""
    return torch.zeros(CLIP_STATE_WORDS, dtype=torch.float32, device=device)


def clip_state_counts(state):
    """(nonfinite, n_clipped, n_nonfinite) of a clip state (synchronises)."""
    w = state.view(torch.int32).tolist()
    return w[2], w[4], w[5]


def grad_norm_clip(grad, max_norm, state=None):
    """Global L2 norm of the flat fp32 gradient ``grad`` and what clip_grad_norm_ derives from it (``pgasr_grad_norm_clip``): writes
    norm, scale = min(1, max_norm / (norm + 1e-6)) and the non-finite flag into ``state`` (``clip_state``; a new one when None) and
    advances its counts.  Nothing is scaled here: ``adam_step(clip_state=state)`` applies the scale.  Returns the state."""
    lib = _lib.load()
    _req(grad, torch.float32, "grad")
    if state is None:
        state = clip_state(grad.device)
    _req(state, torch.float32, "state")
    if state.numel() != CLIP_STATE_WORDS:
        raise _lib.PgasrError(f"grad_norm_clip: state must hold {CLIP_STATE_WORDS} words (hipops.clip_state)")
    n = grad.numel()
    nbytes = lib.pgasr_grad_norm_ws_bytes(n)
    ws = _workspace(nbytes, grad.device, "grad_norm")
    with _timed("grad_norm_kernel"):
        _lib.check(lib.pgasr_grad_norm_clip(_p(grad), n, float(max_norm), _p(ws), nbytes, _p(state), _stream()), "pgasr_grad_norm_clip")
    return state


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, guards=(),
              applied=None, clip_state=None):
    """guards: up to two device addresses of int32 words (``lstm_error_words``, or the word of the gradient buffer that
    carried the error flag through the all-reduce); the update is skipped while one is set.
    applied: int32 (2,) GPU tensor, zeroed once: the count of updates really applied lives there (bias correction then
    ignores skipped calls); ``step`` stays the 1-based count of calls.
    clip_state: a state ``grad_norm_clip`` has written for this gradient on the current stream: the gradient enters as
    scale * g, and a non-finite gradient skips the update like a set guard (``pgasr_adam_step_clipped``)."""
    lib = _lib.load()
    for t, nm in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _req(t, torch.float32, nm)
    _req(applied, torch.int32, "applied")
    if applied is not None and applied.numel() != 2:
        raise _lib.PgasrError("adam_step: applied must hold two int32 words")
    g = list(guards)[:2] + [0, 0]
    if clip_state is not None:
        _req(clip_state, torch.float32, "clip_state")
        if clip_state.numel() != CLIP_STATE_WORDS:
            raise _lib.PgasrError(f"adam_step: clip_state must hold {CLIP_STATE_WORDS} words (hipops.clip_state)")
        _lib.check(lib.pgasr_adam_step_clipped(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), int(step),
                                               float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                               g[0], g[1], _p(applied), _p(clip_state), _stream()), "pgasr_adam_step_clipped")
        return
    _lib.check(lib.pgasr_adam_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), int(step),
                                   float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                   g[0], g[1], _p(applied), _stream()), "pgasr_adam_step")


def lstm_busy_ptr(T, B, backward, device, stream=None):
    """Device address of the per-XCD busy counters inside the sweep workspace used on ``stream``
    (default: current stream) -- the hint queue-mode GEMMs read."""
    import ctypes
    lib = _lib.load()
    off = ctypes.c_size_t(0)
    _lib.check(lib.pgasr_lstm_busy_offset(B, int(backward), ctypes.byref(off)), "pgasr_lstm_busy_offset")
    if stream is None:
        ws = _lstm_ws(T, B, backward, device)
    else:
        with torch.cuda.stream(stream):
            ws = _lstm_ws(T, B, backward, device)
    return ws.data_ptr() + off.value


_concurrent = {}
STRICT_CONCURRENCY = False   # bench.py: raise instead of quietly running the (slower) sequential order


def streams_concurrent(other):
    """True iff kernels on ``other`` run while a kernel of the CURRENT stream is resident (probed once per stream pair,
    synchronises).  The feed-ahead GEMMs need this: with serialised kernels (counter-collecting profilers,
    HIP_LAUNCH_BLOCKING, one hardware queue) a fed sweep would wait for a GEMM that cannot start."""
    main = torch.cuda.current_stream()
    key = (main.cuda_stream, other.cuda_stream)
    if key not in _concurrent:
        lib = _lib.load()
        words = torch.zeros(2, dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()))
        torch.cuda.synchronize()
        _lib.check(lib.pgasr_stream_probe(words.data_ptr(), 200000, _stream()), "pgasr_stream_probe")
        with torch.cuda.stream(other):
            words[0:1].fill_(1)
        torch.cuda.synchronize()
        _concurrent[key] = bool(int(words[1].item()) == 1)
        if not _concurrent[key] and STRICT_CONCURRENCY:
            raise _lib.PgasrError("kernels of different streams do not run concurrently here (serialising profiler / launch-blocking "
                                  "mode / one hardware queue): the feed-ahead GEMMs would fall back to the sequential order; set "
                                  "PGASR_ALLOW_SEQUENTIAL=1 to benchmark that order knowingly")
        if not _concurrent[key]:
            import warnings
            warnings.warn("policy_gradient_asr_amd: kernels of different streams do not run concurrently here "
                          "(serialising profiler / launch-blocking mode / one hardware queue): feed-ahead GEMMs are off")
    return _concurrent[key]


GATE_OPENED_ON_BUSY, GATE_OPENED_ON_PUBLICATION, GATE_TIMED_OUT = 1, 2, 3     # report[0] of pgasr_stream_gate_report


def stream_gate(words_ptr, count=8, timeout_us=60, need=0, running=None, report=None):
    """Hold the current stream until a sweep has registered in the busy counters at ``words_ptr``; need > 0: until ``need``
    clusters have (consumers that wait for the sweep's publications: all of its workgroups must be resident first) -- or until
    the first word of ``running`` (the streamed sweep's slab_done words) is non-zero: the sweep is under way or already over.
    report (need > 0; int32 tensor of >= 2 words): the gate writes how it left (GATE_*) and the microseconds it held the stream."""
    lib = _lib.load()
    if need > 0 and report is not None:
        _req(report, torch.int32, "report")
        if report.numel() < 2:
            raise _lib.PgasrError("report needs two int32 words")
        _lib.check(lib.pgasr_stream_gate_report(words_ptr, count, int(need), _p(running), timeout_us, _p(report), _stream()),
                   "pgasr_stream_gate_report")
    elif need > 0:
        _lib.check(lib.pgasr_stream_gate_sum(words_ptr, count, int(need), _p(running), timeout_us, _stream()), "pgasr_stream_gate_sum")
    else:
        _lib.check(lib.pgasr_stream_gate(words_ptr, count, timeout_us, _stream()), "pgasr_stream_gate")
