"""The train-step body of model.py:225-239 for the CTC + policy-gradient objective, one process
per GPU, gradients all-reduced over RCCL (replaces nn.DataParallel, model.py:201).

Parameters and gradients live in two flat fp32 buffers (nn.Parameters are views), so the
data-parallel exchange is ONE all-reduce of the whole gradient (19.15 MB at F=80,V=29) and the
optimizer is one Adam over the flat buffer.  Utterances are independent through forward, CTC,
decode, reward and REINFORCE gradient, so the gradient all-reduce is the only collective; the loss
is normalised by the GLOBAL batch so 1-GPU and N-GPU gradients agree to fp32 rounding.
"""
import copy
import os
import threading

import torch
import torch.distributed as dist

# Leading fp32 words of both flat buffers (256 bytes: the parameters keep their alignment).  Word 0 of the GRADIENT
# buffer carries the step's error flag through the gradient all-reduce: every rank writes 1.0 there when one of its
# sweeps timed out, the SUM is > 0 on every rank, and the guarded Adam of every rank reads that word -- all replicas skip
# the update or none does (the rank-local guard let replicas diverge, and let the other ranks apply a reduced gradient
# that contained the failed rank's garbage).
FLAG_PAD = 64
_step_lock = threading.Lock()     # the host layer keeps per-process state (grad_overlap, held tensors): one step at a time


def flatten_parameters(model, pad=0):
    """Re-point every parameter (and its .grad) at a slice of one flat buffer (``pad`` leading words stay free)."""
    params = [p for p in model.parameters()]
    dev = params[0].device
    total = pad + sum(p.numel() for p in params)
    flat = torch.zeros(total, dtype=torch.float32, device=dev)
    gflat = torch.zeros(total, dtype=torch.float32, device=dev)
    off = pad
    with torch.no_grad():
        for p in params:
            n = p.numel()
            flat[off:off + n].copy_(p.data.view(-1))
            p.data = flat[off:off + n].view_as(p.data)
            p.grad = gflat[off:off + n].view_as(p.data)
            off += n
    return flat, gflat


def shard_slice(global_batch, rank, world):
    """Contiguous B/N utterances per rank (global_batch must divide evenly)."""
    if global_batch % world:
        raise ValueError("global batch must be a multiple of the world size")
    per = global_batch // world
    return slice(rank * per, (rank + 1) * per)


def balance_by_frames(lengths, world):
    """Variable-T batches (BASELINE config 5): assign utterances to ranks so that every rank gets
    the same COUNT and nearly the same total number of frames (ranks then reach the all-reduce
    together).  Greedy longest-first into the lightest non-full rank.  Returns a list of index
    lists, one per rank."""
    n = len(lengths)
    if n % world:
        raise ValueError("batch must be a multiple of the world size")
    per = n // world
    order = sorted(range(n), key=lambda i: -int(lengths[i]))
    loads = [0] * world
    out = [[] for _ in range(world)]
    for i in order:
        r = min((r for r in range(world) if len(out[r]) < per), key=lambda r: loads[r])
        out[r].append(i)
        loads[r] += int(lengths[i])
    return out


def check_max_grad_norm(max_grad_norm):
    """None (no clipping), or a real number > 0 (``float("inf")``: measure and guard, never scale) -> None or float."""
    if max_grad_norm is None:
        return None
    import numbers
    if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, numbers.Real):
        raise ValueError(f"max_grad_norm must be None or a real number > 0 (got {max_grad_norm!r})")
    v = float(max_grad_norm)
    if not v > 0:        # <= 0 and NaN
        raise ValueError(f"max_grad_norm must be None or a real number > 0 (got {max_grad_norm!r})")
    return v


def default_utt_ids(sizes, rank, world):
    """The ids an accumulated step gives its rows when the caller names none: row b of micro-batch j (``sizes[j]`` real utterances
    per rank) on ``rank`` is utterance ``world * off_j + rank * sizes[j] + b`` of the global batch, ``off_j = sum(sizes[:j])`` --
    micro-batch j is a contiguous slice of the global batch, sharded contiguously over the ranks.  Over all ranks and micro-batches
    the ids are a bijection onto [0, world * sum(sizes)).  Returns one list of ints per micro-batch."""
    out, off = [], 0
    for n in sizes:
        base = world * off + rank * n
        out.append(list(range(base, base + n)))
        off += n
    return out


def check_utt_ids(utt_ids, sizes, world):
    """``utt_ids`` of an accumulated step: one host sequence of integers per micro-batch, ``sizes[j]`` of them for micro-batch j,
    pairwise distinct over the whole step and each in [0, world * sum(sizes)).  Returns them as lists of int."""
    import numbers
    if isinstance(utt_ids, torch.Tensor) or not hasattr(utt_ids, "__len__"):
        raise ValueError("utt_ids must be a sequence of host integer sequences, one per micro-batch")
    if len(utt_ids) != len(sizes):
        raise ValueError(f"utt_ids names {len(utt_ids)} micro-batches, the step has {len(sizes)}")
    total = world * sum(sizes)
    seen, out = set(), []
    for j, (ids, n) in enumerate(zip(utt_ids, sizes)):
        ids = ids.tolist() if isinstance(ids, torch.Tensor) else list(ids)
        if len(ids) != n:
            raise ValueError(f"utt_ids[{j}] holds {len(ids)} ids for a micro-batch of {n} utterances")
        for i in ids:
            if isinstance(i, bool) or not isinstance(i, numbers.Integral):
                raise ValueError(f"utt_ids[{j}]: {i!r} is not an integer")
            if not 0 <= i < total:
                raise ValueError(f"utt_ids[{j}]: id {i} outside [0, {total}) = world x the step's utterances per rank")
            if i in seen:
                raise ValueError(f"utt_ids[{j}]: id {i} occurs twice in one step (two utterances would share their sampler counters)")
            seen.add(i)
        out.append([int(i) for i in ids])
    return out


class MicroBatch:
    """What ``forward_loss`` may want to know about the micro-batch it is running (``DataParallelStep._micro``; None outside
    an accumulated step): its index, how many the step has, the real utterances per rank in the micro-batches before it, and
    the caller's ids for its rows (a list of int, or None for the default rule)."""
    __slots__ = ("index", "count", "offset", "ids")

    def __init__(self, index, count, offset, ids):
        self.index, self.count, self.offset, self.ids = index, count, offset, ids


class DataParallelStep:
    """zero_grad -> forward_loss -> backward -> all-reduce(sum) -> [clip by global norm] -> Adam, on flat buffers.
    Subclasses provide ``forward_loss(batch, global_batch) -> scalar loss`` already divided by the
    GLOBAL batch size, so the summed gradient is the global-batch gradient."""

    def __init__(self, model, lr=5e-4, world_size=1, process_group=None, precision=None, max_grad_norm=None, wide_alphabet=False):
        """wide_alphabet: False (default) -- an alphabet of more than 64 symbols is refused, as ever; True -- up to 1024 symbols
        (hipops.MAX_VOCAB_WIDE) on the wide kernels, which run the default objective alone (loss.check_options).
        precision: "f32" (the library default: the reference's arithmetic, torch fp32 -- every big product as six bf16 MFMA terms
        of three-plane operands, exact to 2^-24: three-plane sweeps, six-product W_ih projections / input and weight gradients,
        gemm_x6.hip; the small products on the exact fp32 MFMA) or "bf16x3" (opt-in: 3-term products of two-plane operands, within
        the 1e-3 bar, ~20 % faster) -- hipops.PRECISION_MODES; None = whatever mode is set when a step runs.
        max_grad_norm: None (default: the step as it always was) or a bound > 0 on the L2 norm of the REDUCED gradient
        (torch.nn.utils.clip_grad_norm_ between backward and the update: g := g * min(1, max / (norm + 1e-6))), measured over
        gflat[FLAG_PAD:] after the last all-reduce -- the same numbers on every rank, so replicas stay bit-identical -- and applied
        inside the Adam kernel; a gradient that holds an inf or NaN skips the update on every rank (parameters and moments untouched,
        not counted by ``applied_steps``).  float("inf") measures and guards without ever scaling.  No host synchronisation:
        ``last_grad_norm`` / ``clip_counts()`` read the result."""
        self.max_grad_norm = check_max_grad_norm(max_grad_norm)
        self.wide_alphabet = bool(wide_alphabet)
        if precision is not None:
            from . import hipops
            if precision not in hipops.PRECISION_MODES:
                raise ValueError(f"precision must be one of {sorted(hipops.PRECISION_MODES)} or None")
        self.precision = precision
        self.model = model
        self.world = world_size
        self.pg = process_group
        self.flat, self.gflat = flatten_parameters(model, FLAG_PAD)
        self.flat_param = torch.nn.Parameter(self.flat)
        self.flat_param.grad = self.gflat
        # Adam(lr=5e-4) is the reference's commented choice (model.py:207)
        self.lr = lr
        if self.flat.is_cuda:
            self.exp_avg = torch.zeros_like(self.flat)
            self.exp_avg_sq = torch.zeros_like(self.flat)
            self.applied = torch.zeros(2, dtype=torch.int32, device=self.flat.device)   # updates really applied (pgasr_adam_step)
            self.opt = None
        else:   # CPU is only the gloo plumbing test: torch's Adam
            self.opt = torch.optim.Adam([self.flat_param], lr=lr)
            self.applied_cpu = 0
        # clipping: the device-resident state of pgasr_grad_norm_clip (norm, scale, non-finite flag, counts); on the CPU plumbing
        # path a 0-d tensor and two host counts
        self.clip_state = None
        self.last_grad_norm = None          # 0-d tensor: the pre-clip norm of the last step's reduced gradient (reading it synchronises)
        self._clip_counts_cpu = [0, 0]
        if self.max_grad_norm is not None and self.flat.is_cuda:
            from . import hipops
            self.clip_state = hipops.clip_state(self.flat.device)
            self.last_grad_norm = self.clip_state[0]
            self._clip_grad = self.gflat[FLAG_PAD:]     # what the norm is taken over: not the flag word and its pad
        self.nstep = 0                      # CALLS of step() (seeds the sampler / dropout offsets); see applied_steps()
        self.collective = self.world > 1    # tests set this on a 1-rank group to exercise the plumbing
        self._early = None                  # (split, work) of an all-reduce issued during backward
        self._micro = None                  # the running micro-batch of an accumulated step (MicroBatch), else None
        self._hold_collectives = False      # True while a micro-batch that is not the step's last runs: nothing is exchanged
        if self.world > 1:
            dist.broadcast(self.flat, src=0, group=self.pg)   # identical replicas

    def param_offset(self, name):
        """Offset in the flat buffers of the parameter called ``name`` (model.named_parameters() order)."""
        off = FLAG_PAD
        for n, p in self.model.named_parameters():
            if n == name:
                return off
            off += p.numel()
        raise KeyError(name)

    def reduce_upper(self, split):
        """Start the all-reduce of gflat[split:] now (its gradients are complete on the CURRENT stream) and leave
        gflat[:split] to ``reduce_rest``: two buckets, the first one hidden under what is left of backward.
        Every rank must call it at the same point of its step (collectives are matched by order)."""
        if not self.collective or self._early is not None or self._hold_collectives:
            return          # (an accumulated step exchanges around its LAST micro-batch only)
        # The blocking form on purpose: issued under the weight-gradient side stream it makes only THAT stream wait for the
        # collective (the caller's stream joins the side stream before Adam anyway).  With async_op=True the whole step ran
        # 9.0 -> 12.6 ms on a 1-rank RCCL group -- every phase slower, forward sweeps of the next step included, host enqueue
        # time unchanged (bench.py, PGASR_BENCH_SOLO_COLLECTIVE=1); a dummy kernel in the same place and the blocking
        # form both cost nothing.
        dist.all_reduce(self.gflat[split:], op=dist.ReduceOp.SUM, group=self.pg)
        self._early = (split, None)

    def reduce_rest(self):
        if not self.collective:
            return
        if self._early is None:
            dist.all_reduce(self.gflat, op=dist.ReduceOp.SUM, group=self.pg)
            return
        split, work = self._early
        self._early = None
        if work is not None:
            work.wait()                 # the current stream waits for the first bucket
        if split > 0:
            dist.all_reduce(self.gflat[:split], op=dist.ReduceOp.SUM, group=self.pg)

    def forward_loss(self, batch, global_batch):  # pragma: no cover - abstract
        raise NotImplementedError

    def write_local_error_flag(self):
        """Word 0 of the gradient buffer := 1.0 iff THIS rank's step produced invalid gradients (a persistent sweep gave up on a bounded
        wait; the words are sticky), else 0.0 -- one small launch on the current stream (``pgasr_error_flag``).  Returns False where
        there is nothing to report (CPU plumbing, no sweep workspace yet)."""
        if not self.flat.is_cuda:
            return False
        from . import _lib, hipops
        words = hipops.lstm_error_word_tensors(self.flat.device)
        if not words:
            return False
        lib = _lib.load()
        _lib.check(lib.pgasr_error_flag(words[0].data_ptr(), words[1].data_ptr() if len(words) > 1 else None, self.gflat.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream), "pgasr_error_flag")
        return True

    def applied_steps(self):
        """Number of Adam updates really applied (synchronises): ``nstep`` minus the updates the guard skipped."""
        if self.opt is not None:
            return self.applied_cpu
        return int(self.applied[self.nstep & 1].item())

    def clip_counts(self):
        """(steps whose gradient was scaled down, steps skipped for a non-finite gradient) so far (synchronises); (0, 0)
        without ``max_grad_norm``."""
        if self.clip_state is None:
            return tuple(self._clip_counts_cpu)
        from . import hipops
        _, n_clipped, n_nonfinite = hipops.clip_state_counts(self.clip_state)
        return n_clipped, n_nonfinite

    def set_applied_steps(self, n):
        """Checkpoint resume: the bias correction continues from ``n`` applied updates."""
        if self.opt is not None:
            self.applied_cpu = int(n)
        else:
            self.applied.fill_(int(n))

    def backward(self, loss):
        loss.backward()

    def step(self, *batch, utt_ids=None):
        """One optimizer step on one batch.  utt_ids: None, or one host integer per row -- the row's index in the GLOBAL batch
        (world x B utterances), for shards that are not contiguous slices of it (``balance_by_frames``); see ``step_accumulated``."""
        if utt_ids is not None:
            return self.step_accumulated([batch], utt_ids=[utt_ids])
        return self._locked(self._step, batch)

    def compute_gradients(self, *batch, utt_ids=None):
        """The step WITHOUT its exchange and update: zero_grad -> forward_loss -> backward in the step's own orders (fed sweeps,
        streamed weight gradients, side streams), gradients left in ``gflat`` (the parameters' ``.grad`` views), every side stream
        joined.  Returns the detached local loss.  What the full-size parity tests compare with the oracle.  Every call zeroes
        ``gflat`` and draws with the same sampler offset: to accumulate micro-batches use ``accumulate_gradients`` /
        ``step_accumulated``.  utt_ids as in ``step``."""
        if utt_ids is not None:
            return self.accumulate_gradients([batch], utt_ids=[utt_ids])
        return self._locked(self._gradients, batch).detach()

    def step_accumulated(self, micro_batches, utt_ids=None):
        """ONE optimizer step over a sequence of micro-batches, each the tuple that ``step()`` takes: the batch a step sees is then
        bounded by time, not by what one call takes.
          - ``gflat`` is zeroed once; every micro-batch runs forward_loss -> backward in the step's own orders and adds to it.
          - Every micro-batch's loss is normalised by global_batch = world x (the sum of the micro-batches' real utterances), so
            the accumulated gradient IS the global batch's gradient: no rescaling pass follows.
          - Collectives are issued around the LAST micro-batch only (the early bucket during its backward, the rest after it).
          - The error flag, the global-norm clip (if any) and the Adam update run once, after the last micro-batch, on the
            accumulated and reduced gradient; ``nstep``, Adam's bias correction and ``applied_steps()`` advance by one.
          - The step lock is held across the whole call; tensors a micro-batch keeps alive across streams are released when the
            next one begins, so the peak memory is that of the largest micro-batch plus the flat buffers.
        Returns the sum of the micro-batches' detached losses (the global-batch loss of this rank; added on the device).
        utt_ids: None, or one sequence of host integers per micro-batch: the index of every row in the global batch of
        world x sum(B_j) utterances -- pairwise distinct, checked on the host (ValueError).  A trainer that samples addresses its
        draws by them.  None: ``default_utt_ids``.
        world > 1: every rank must pass the same number of micro-batches with the same sizes (the normalisation and the order
        of the collectives assume it; a rank cannot see the others' sizes, so only an empty sequence or an empty micro-batch
        raises ValueError here).
        The identity with ONE process that holds the whole global batch holds for micro-batches padded to one common T: the
        encoder's instance norm runs over the whole padded (F, T) plane, so an utterance's activations depend on the T its
        batch is padded to.  Micro-batches of different T (a bucketing loader's) are valid training, but their sum is not the
        gradient of any single padded batch."""
        return self._locked(self._step_accumulated, (micro_batches, utt_ids))

    def accumulate_gradients(self, micro_batches, utt_ids=None):
        """``step_accumulated`` WITHOUT its exchange and update, as ``compute_gradients`` is to ``step``: the accumulated local
        gradient is left in ``gflat``, every side stream joined.  Returns the summed detached local loss."""
        return self._locked(self._accumulate, (micro_batches, utt_ids), hold_last=True)

    def _locked(self, fn, batch, **kw):
        from . import streams
        # every side stream of the step is joined into the calling stream by the time backward() returns, so tensors that
        # cross streams are kept alive until the next step begins instead of being handed to record_stream (streams.hold)
        if not _step_lock.acquire(blocking=False):
            raise RuntimeError("policy_gradient_asr_amd: one train step at a time per process (the host layer's overlap / "
                               "stream state is process-global); a second trainer may only step between the steps of the first")
        try:
            with streams.managed_step():
                if self.precision is not None and self.flat.is_cuda:
                    from . import hipops
                    with hipops.precision(self.precision):
                        return fn(*batch, **kw)
                return fn(*batch, **kw)
        finally:
            _step_lock.release()

    def _gradients(self, *batch):
        local_b = batch[0].shape[0]
        self.gflat.zero_()
        loss = self.forward_loss(batch, local_b * self.world)
        self.backward(loss)
        return loss

    def _check_micro_batches(self, micro_batches, utt_ids):
        """-> (list of batch tuples, their sizes, ids per micro-batch or Nones); ValueError on what cannot be one step."""
        if isinstance(micro_batches, torch.Tensor) or not hasattr(micro_batches, "__len__"):
            raise ValueError("micro_batches must be a sequence of batches, each the tuple that step() takes")
        mbs = [tuple(mb) for mb in micro_batches]
        if not mbs:
            raise ValueError("step_accumulated needs at least one micro-batch")
        for j, mb in enumerate(mbs):
            if not mb or not isinstance(mb[0], torch.Tensor) or mb[0].dim() < 1 or mb[0].shape[0] < 1:
                raise ValueError(f"micro-batch {j} is empty: every rank must pass the same micro-batch sizes, each >= 1")
        sizes = [mb[0].shape[0] for mb in mbs]
        ids = check_utt_ids(utt_ids, sizes, self.world) if utt_ids is not None else [None] * len(mbs)
        return mbs, sizes, ids

    def _accumulate(self, micro_batches, utt_ids, hold_last=False):
        """gflat := the sum of the micro-batches' gradients of the global-batch loss.  hold_last: the last micro-batch exchanges
        nothing either (accumulate_gradients)."""
        from . import streams
        mbs, sizes, ids = self._check_micro_batches(micro_batches, utt_ids)
        global_batch = self.world * sum(sizes)
        self.gflat.zero_()
        total, off = None, 0
        try:
            for j, mb in enumerate(mbs):
                if j:
                    streams.release()       # backward() joined every side stream: as between two steps
                self._micro = MicroBatch(j, len(mbs), off, ids[j])
                self._hold_collectives = hold_last or j + 1 < len(mbs)
                loss = self.forward_loss(mb, global_batch)
                self.backward(loss)
                loss = loss.detach()
                total = loss if total is None else total + loss
                del loss
                off += sizes[j]
        finally:
            self._micro = None
            self._hold_collectives = False
        return total

    def _step_accumulated(self, micro_batches, utt_ids):
        return self._finish(self._accumulate(micro_batches, utt_ids))

    def _step(self, *batch):
        return self._finish(self._gradients(*batch))

    def _finish(self, loss):
        """The once-per-step tail: error flag -> the rest of the exchange -> [clip] -> Adam, on the reduced gradient in gflat."""
        if self.collective:
            # the error flag travels with the last gradient bucket (word 0, see FLAG_PAD): SUM > 0 on every rank iff any
            # rank's gradients are invalid
            self.write_local_error_flag()
        self.reduce_rest()
        self.nstep += 1
        if self.opt is None:
            from . import hipops
            # a sweep that timed out in this step (or an earlier one: the words are sticky) left invalid gradients:
            # the update is skipped on the device -- on every rank, since the guard is the reduced flag -- and does not
            # count for the bias correction; the host raises at its next check (hipops.lstm_assert_no_timeouts)
            guards = [self.gflat.data_ptr()] if self.collective else hipops.lstm_error_words(self.flat.device)
            if self.clip_state is not None:
                # both buckets are in: the norm of the reduced gradient (not of the flag word and its pad), on the critical
                # stream between the last all-reduce and Adam, which reads scale and the non-finite flag from the state
                hipops.grad_norm_clip(self._clip_grad, self.max_grad_norm, self.clip_state)
            hipops.adam_step(self.flat, self.gflat, self.exp_avg, self.exp_avg_sq, self.nstep, lr=self.lr,
                             guards=guards, applied=self.applied, clip_state=self.clip_state)
        else:
            # CPU plumbing (gloo tests): the same rules, checked on the host
            flagged = self.collective and float(self.gflat[0]) > 0
            scale = 1.0
            if self.max_grad_norm is not None:
                norm = self.gflat[FLAG_PAD:].double().norm().float()
                self.last_grad_norm = norm
                if not bool(torch.isfinite(norm)):
                    self._clip_counts_cpu[1] += 1
                    flagged = True
                else:
                    scale = float(torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0))
                    self._clip_counts_cpu[0] += scale < 1.0
            if not flagged:
                if scale < 1.0:         # Adam sees scale * g; gflat keeps the unclipped gradient, as on the device
                    self.flat_param.grad = self.gflat * scale
                    self.opt.step()
                    self.flat_param.grad = self.gflat
                else:
                    self.opt.step()
                self.applied_cpu += 1
        return loss.detach()


class PolicyGradientTrainer(DataParallelStep):
    """step(x, targets, fmask, tmask): x (B,F,T) fp32; targets (B,L) int (pad 0); fmask (B,T);
    tmask (B,L) -- the collate_custom batch (data.py:107-116) after model.py:227-230's squeeze.
    Returns the detached local loss (no host sync).
    ONE trainer steps at a time per process: the overlap / stream / held-tensor state of the host layer (functional.grad_overlap,
    streams) is process-global and guarded by a step lock -- a second trainer may step between the steps of the first, a concurrent
    ``step()`` raises RuntimeError.
    Data parallel: the sampler addresses its draws by global utterance index, which makes N ranks sample exactly what one process
    holding the whole batch samples.  By default a rank's rows are taken for a CONTIGUOUS shard of the global batch
    (``shard_slice``): row b is utterance ``rank * local_B + b``.  Shards that are not contiguous (``balance_by_frames``: variable
    lengths, configs[4]) name their rows' global indices with ``utt_ids`` -- ``step(..., utt_ids=parts[rank])`` -- and keep the
    identity.
    ``step_accumulated(micro_batches, utt_ids=None)`` is one optimizer step over several such batches (DataParallelStep): every
    micro-batch samples with the same offset ``nstep + 1`` and distinct ids -- by default ``default_utt_ids``, micro-batch j a contiguous
    slice of the global batch --, and ``last_stats`` / ``last_sample_rewards`` hold the micro-batches' statistics concatenated in call
    order (real rows only), and so do ``last_sequence_scored``, ``last_entropy`` and ``last_kl``."""

    def __init__(self, model, lr=5e-4, lam=1.0, seed=0, blank=0, world_size=1, process_group=None, rank=0,
                 reward_decoder="greedy", beam_size=16, precision=None, reward_mode="utterance", num_samples=1,
                 reward_baseline="hypothesis", reward_unit="char", word_delimiter=None, max_grad_norm=None,
                 score_function="path", max_hyp_len=None, entropy_weight=0.0, kl_weight=0.0, kl_reference=None, wide_alphabet=False,
                 wide_objectives=False, wide_sequence=False, unit_spelling=None, step_objectives=False, hotwords=None):
        """wide_alphabet: opt in to alphabets of 65 .. 1024 symbols (subword units).  MAX_VOCAB becomes 1024, and such a model takes
        the default objective alone: reward_decoder="greedy", reward_mode="utterance", num_samples=1, reward_baseline="hypothesis",
        reward_unit="char", score_function="path", entropy_weight=0, kl_weight=0 -- anything else raises here and before every
        step (loss.check_options).  False (default): a model of more than 64 symbols is refused by ``step`` as ever.
        wide_objectives: with wide_alphabet=True (else ValueError), opt in to num_samples 1 .. MAX_SAMPLES, either reward_baseline,
        entropy_weight and kl_weight / kl_reference for such a model too, in any combination, on the wide kernels of A12-WIDE;
        reward_decoder="beam", reward_mode="per_step" (without step_objectives), reward_unit="word" and score_function="sequence" stay
        refused there.  The default objective keeps its launches and bits with or without it.
        wide_sequence: with wide_alphabet=True (else ValueError), opt in to score_function="sequence" for such a model, on the wide
        kernels of A13-WIDE: num_samples=1 against the greedy hypothesis, or together with whatever wide_objectives=True admits.  Set
        max_hyp_len for unit models (the workspace formula below: 2.1 GB at K = 4, B = 32, T = 1000 with the default cap).
        reward_decoder="beam", reward_mode="per_step" (without step_objectives) and reward_unit="word" stay refused there.
        reward_mode: "utterance" (default) -- one reward R = -ED / |y| per utterance, the sum of the reference's per-step rewards
        (policy_grad.py:10-15) up to a constant the baseline removes; "per_step" -- the per-step rewards themselves, as rewards-to-go
        per frame against the greedy path's reward-to-go at the same frame (loss.PGCTCLossFn; greedy baseline only).
        reward_decoder: which hypothesis the self-critical baseline reward comes from -- "greedy" (best path) or
        "beam": the reference's own reward definition (policy_grad.py:6-8: prefix beam search -> collapse_fn ->
        edit distance), decoded on the device with ``beam_size`` (BASELINE config 5: 16; the reference passes 5).
        num_samples: sampled paths per utterance (1 .. MAX_SAMPLES; multi-sample REINFORCE, loss.PGCTCLossFn).
        reward_baseline: "hypothesis" (default) -- every sample's reward against the reward_decoder hypothesis'; "leave_one_out" --
        against the mean reward of the utterance's other samples (num_samples >= 2; no greedy or beam decode runs).
        ``last_stats`` stays (nll, R_s, R_b), each (B,): R_s averaged over the samples, R_b the baseline averaged over them;
        ``last_sample_rewards`` holds every sample's reward, (num_samples, B).
        reward_unit: "char" (default) -- R = -ED / |y| over characters; "word" -- R = -WED / W(y) over words, split at the token
        ``word_delimiter`` (the alphabet's " "; not the blank) like str.split(" "), for every sample and baseline reward (the CTC term
        stays normalised by the character count; not with reward_mode="per_step"; T <= MAX_WORD_FRAMES).
        max_grad_norm: clip the reduced gradient to this global L2 norm inside the step and skip non-finite gradients
        (DataParallelStep; None = off); ``last_grad_norm`` and ``clip_counts()`` report.
        score_function: "path" (default) -- the REINFORCE term scores a sample by its frame path, log p(pi_k | x); "sequence" -- by
        the CTC likelihood of its collapsed hypothesis, log p(y_k | x) over all alignments: the same expected gradient with no larger
        variance (loss.PGCTCLossFn; any num_samples, baseline, reward_decoder and reward_unit; not with reward_mode="per_step").
        max_hyp_len ("sequence" only): hypotheses of more tokens keep the path-level term; None = min(T, MAX_HYP_LEN).  It bounds the
        hypothesis-lattice workspace, 2 * K*B*T * roundup64(2*Lh+1) * 4 bytes.  ``last_sequence_scored``: (num_samples, B) bool on the
        device, which samples took the sequence term in the last step (None with "path"); reading it synchronises.
        entropy_weight: beta >= 0 (default 0: off, the step as it was), entropy regularisation of the frame policy against collapse:
        the loss gains -beta / global_batch times every utterance's MEAN frame entropy (nats), so beta is in loss units per nat per
        frame and does not grow with T (loss.PGCTCLossFn; with every other setting, reward_mode="per_step" included).
        ``last_entropy``: (B,) mean frame entropy of the last step's real utterances, on the device (None with weight 0); nothing
        synchronises until it is read.
        kl_weight: gamma >= 0 (default 0: off, the step as it was -- no reference forward, no launch), a KL penalty towards the frozen
        reference policy ``kl_reference``, the anchor of an RL fine-tune of a pretrained model: the loss gains gamma / global_batch
        times every utterance's MEAN frame KL(p || q) in nats, so gamma is in loss units per nat per frame (loss.PGCTCLossFn; with every
        other setting).  kl_reference: a module with ``Seq2Seq.logits`` and the model's alphabet, not the trained model and sharing no
        parameter storage with it, or "initial" for a deep copy of ``model`` as it stands at construction; required when gamma > 0.
        The trainer puts it in eval() with requires_grad_(False) and never updates it.  Every step its logits are computed on the
        padded batch under no_grad, in the trainer's precision, on the calling stream and BEFORE the policy's forward (the two
        models' sweeps never run beside each other), which costs one eval forward per step.  ``last_kl``: (B,) mean frame KL of the
        last step's real utterances, on the device (None with weight 0).
        unit_spelling: None (default: the step as it was) or the ``units.UnitSpelling`` of the model's subword units: the rewards are
        counted on the spelled TEXT -- reward_unit="char" its characters, "word" its words, split at the spelling's " " (give no
        word_delimiter) -- with every setting the alphabet's size admits except reward_mode="per_step"; above 64 symbols it is what
        admits reward_unit="word" (loss.PGCTCLossFn).  ``last_spell_truncated``: how many rows of the last step were cut at the
        4094-character row limit, a 0-d int32 on the device (None without a spelling); nothing synchronises until it is read.
        step_objectives: False (default: the step, and every refusal, as it was) or True -- reward_mode="per_step" then takes
        num_samples 1 .. MAX_SAMPLES, either reward_baseline, entropy_weight, kl_weight, shards and micro-batches: per-FRAME
        coefficients from the rewards-to-go of all K sampled paths against the greedy path's or the other samples' at the same frame
        (loss.PGCTCLossFn, A12-STEP).  With wide_alphabet=True it admits per_step above 64 symbols with num_samples=1, the hypothesis
        baseline and no entropy or KL term; the rest there needs wide_objectives=True as well.  reward_decoder="beam",
        score_function="sequence", reward_unit="word" and unit_spelling stay refused with reward_mode="per_step"; with
        reward_mode="utterance" the keyword changes nothing.
        hotwords: must stay None -- there is no hotword bias during training (the in-step search of reward_decoder="beam" is the
        single-wave kernel); anything else raises a ValueError that says so.  Bias the decoder: CTCDecoder(hotwords=)."""
        from .loss import check_kl_weight
        kl_weight = check_kl_weight(kl_weight)
        if hotwords is not None:
            raise ValueError("hotwords: there is no hotword bias during training -- the in-step search of reward_decoder='beam' is the "
                             "single-wave kernel, which has none; bias the decoder (CTCDecoder(hotwords=))")
        if isinstance(kl_reference, str):
            if kl_reference != "initial":
                raise ValueError(f"kl_reference must be a module with Seq2Seq.logits or 'initial' (got {kl_reference!r})")
            kl_reference = copy.deepcopy(model)          # before the parameters move into the trainer's flat buffer
        super().__init__(model, lr=lr, world_size=world_size, process_group=process_group, precision=precision,
                         max_grad_norm=max_grad_norm, wide_alphabet=wide_alphabet)
        if self.wide_alphabet:
            from . import hipops
            self.MAX_VOCAB = hipops.MAX_VOCAB_WIDE
        self.wide_objectives = bool(wide_objectives)
        if self.wide_objectives and not self.wide_alphabet:
            raise ValueError("wide_objectives=True opens objectives for alphabets of more than 64 symbols: it needs wide_alphabet=True")
        self.step_objectives = bool(step_objectives)
        self.wide_sequence = bool(wide_sequence)
        if self.wide_sequence and not self.wide_alphabet:
            raise ValueError("wide_sequence=True opens the sequence-level objectives for alphabets of more than 64 symbols: it needs "
                             "wide_alphabet=True")
        if reward_decoder not in ("greedy", "beam"):
            raise ValueError("reward_decoder must be 'greedy' or 'beam'")
        if reward_mode not in ("utterance", "per_step"):
            raise ValueError("reward_mode must be 'utterance' or 'per_step'")
        if reward_mode == "per_step" and reward_decoder != "greedy":
            raise ValueError("per-step rewards need the frame-aligned greedy baseline (reward_decoder='greedy')")
        self.reward_decoder, self.beam_size, self.reward_mode = reward_decoder, int(beam_size), reward_mode
        self.blank = blank
        self.num_samples, self.reward_baseline = num_samples, reward_baseline
        self.reward_unit, self.word_delimiter = reward_unit, word_delimiter
        self.unit_spelling, self.last_spell_truncated = unit_spelling, None
        self.score_function, self.max_hyp_len = score_function, max_hyp_len
        self.entropy_weight = entropy_weight
        self.kl_weight, self.kl_reference = kl_weight, None
        opt = self._checked_options()
        self.num_samples, self.max_hyp_len, self.entropy_weight = opt.num_samples, opt.max_hyp_len, opt.entropy_weight
        self.last_entropy = self.last_kl = None
        if kl_reference is not None:
            self.kl_reference = self._frozen_reference(kl_reference)
        self._check_kl_reference()
        self.word_delimiter = None if word_delimiter is None else int(word_delimiter)
        self.last_sequence_scored = None
        self.lam = lam
        # ONE sampling seed for all ranks: a rank addresses its draws by GLOBAL utterance index (contiguous shards: rank *
        # local batch), so N ranks sample exactly the paths of one process holding the whole batch -- the N-rank REINFORCE
        # gradient equals the single-process one, like the CTC part (tests/test_dp_rccl_gpu.py, lambda = 1)
        self.seed = seed
        self.rank = rank
        if hasattr(model, "encoder"):
            model.encoder.dropout_seed = 0x5EED + 104729 * rank
        self._one = None
        self.last_stats = None
        self.last_sample_rewards = None
        self.overlap_weight_grads = True
        # A batch whose size the fast orders do not take (feed-ahead: B <= 32; streamed weight gradients: B % 16 == 0 in "f32", B % 32
        # == 0 in "bf16x3") is padded with EMPTY utterances (no frames, no target) up to the next such size: the last, ragged batch of an
        # epoch (model.py:221-222 leaves it as it comes) then runs the same orders as every other batch.  An empty utterance adds nothing
        # to the loss or to any gradient (CTC of nothing against nothing is 0, its rewards are 0, the sweeps skip it), the loss keeps
        # its normalisation by the REAL batch, the sampler its addressing; a 16-utterance group costs a sweep the same full or not.
        self.pad_ragged_batches = True
        # N > 1: the gradients of the head and of BLSTM layers 1, 2 (2/3 of the bytes) are all-reduced under the tail
        # of backward (the first layer's three GEMMs and the affine gradients), the rest after it
        self.early_reduce = os.environ.get("PGASR_EARLY_REDUCE", "1") != "0"
        try:
            self.upper_split = self.param_offset("encoder.blstm.weight_ih_l1")
        except KeyError:
            self.upper_split = None

    MAX_LOCAL_BATCH = 128      # pgasr_lstm_layer_fwd/bwd: at most 16 clusters of 16 utterances are co-resident
    MAX_VOCAB = 64             # CTC lattice / frame kernels: one wave per (t, b) row
    MAX_SAMPLES = 16           # multi-sample kernels: sampled paths per utterance (PGASR_MAX_SAMPLES)
    MAX_WORD_FRAMES = 4094     # word-level reward: token rows of at most PGASR_WORD_MAX_STRIDE (frames, target symbols)
    MAX_HYP_LEN = 1023         # sequence-level score: hypotheses of at most this many tokens (2L+1 <= 2048 lattice states)

    def _frozen_reference(self, ref):
        """``ref`` as the frozen reference policy of the KL term: checked against the trained model, in eval mode, without gradients."""
        if not callable(getattr(ref, "logits", None)) or not isinstance(ref, torch.nn.Module):
            raise ValueError("kl_reference must be a module with Seq2Seq.logits(x, fmask, lengths), or 'initial'")
        if ref is self.model:
            raise ValueError("kl_reference is the trained model itself: the KL from a policy to itself is 0; pass a frozen copy "
                             "(kl_reference='initial' deep-copies the model as it stands)")
        own = {p.untyped_storage().data_ptr() for p in self.model.parameters()}
        if any(p.untyped_storage().data_ptr() in own for p in ref.parameters()):
            raise ValueError("kl_reference shares parameter storage with the trained model: the optimizer would move the reference")
        vocab, ref_vocab = (getattr(getattr(m, "head", None), "out_features", None) for m in (self.model, ref))
        if vocab != ref_vocab:
            raise ValueError(f"kl_reference has an alphabet of {ref_vocab} symbols, the model one of {vocab}")
        ref.eval()
        ref.requires_grad_(False)
        for p in ref.parameters():
            p.grad = None
        return ref

    def _check_kl_reference(self):
        if self.kl_weight > 0 and self.kl_reference is None:
            raise ValueError("kl_weight > 0 needs kl_reference: the frozen reference policy (a module with Seq2Seq.logits, or 'initial')")

    def _reference_log_probs(self, x, fmask, in_len):
        """The frozen reference's log-probs (T,B,V) for the padded batch: its eval forward under no_grad on the calling stream, in the
        precision of the running step, complete before the policy's forward starts.  It uses its own encoder's counters (eval mode
        draws no dropout mask) and leaves grad_overlap as it found it: a feed stream it left unjoined is joined here."""
        from . import hipops
        from .functional import grad_overlap
        key = grad_overlap._key()
        unjoined = grad_overlap._feed_unjoined.get(key, False)
        ref = self.kl_reference
        if ref.training:
            ref.eval()
        with torch.no_grad():
            z, _ = ref.logits(x, fmask, in_len)
            lp = getattr(z, "log_probs", None)
            if lp is None or getattr(z, "log_probs_version", None) != z._version or lp.shape != z.shape or not lp.is_contiguous():
                lp = hipops.log_softmax_rows(z.contiguous())
        if not unjoined and grad_overlap._feed_unjoined.pop(key, False):
            torch.cuda.current_stream().wait_stream(grad_overlap.second_side_stream())
        return lp.detach()

    def _checked_options(self, frames=None, symbols=None):
        """This trainer's loss settings as they stand now, through the loss's own check (loss.check_options)."""
        from .loss import PGOptions, check_options
        vocab = getattr(getattr(self.model, "head", None), "out_features", None)
        opt = PGOptions(blank=self.blank, per_step=self.reward_mode == "per_step", num_samples=self.num_samples,
                        beam=self.beam_size if self.reward_decoder == "beam" else 0, baseline=self.reward_baseline, reward_unit=self.reward_unit, word_delimiter=self.word_delimiter,
                        score_function=self.score_function, max_hyp_len=self.max_hyp_len, entropy_weight=self.entropy_weight,
                        kl_weight=self.kl_weight, unit_spelling=getattr(self, "unit_spelling", None))
        return check_options(opt, vocab=vocab, frames=frames, symbols=symbols, wide_check=self.wide_alphabet,
                             wide_objectives=getattr(self, "wide_objectives", False),
                             wide_sequence=getattr(self, "wide_sequence", False),
                             step_objectives=getattr(self, "step_objectives", False))

    def _check_limits(self, x, targets):
        """The kernels' compiled-in limits, stated where the caller can read them (otherwise the first symptom is a
        PGASR_ERR_UNSUPPORTED from deep inside the step)."""
        if x.dim() != 3 or targets.dim() != 2:
            raise ValueError("step(x, targets, fmask, tmask): x (B,F,T), targets (B,L)")
        if x.shape[0] > self.MAX_LOCAL_BATCH:
            raise ValueError(f"local batch {x.shape[0]} > {self.MAX_LOCAL_BATCH}: the persistent LSTM sweeps keep at most 16 "
                             "clusters of 16 utterances resident on the chip; use more ranks or smaller batches")
        vocab = getattr(getattr(self.model, "head", None), "out_features", None)
        if vocab is not None and vocab > self.MAX_VOCAB:
            raise ValueError(f"alphabet of {vocab} symbols > {self.MAX_VOCAB}: the CTC / sampling kernels hold one frame's scores in one wave"
                             + ("" if self.wide_alphabet else "; wide_alphabet=True takes up to 1024 symbols with the default objective"))
        if self.reward_decoder == "beam" and self.beam_size > 128:
            raise ValueError("beam_size > 128 is not supported by pgasr_ctc_beam_search")
        self._checked_options(frames=x.shape[2], symbols=targets.shape[1])
        self._check_kl_reference()

    def staging_stream(self):
        """The stream on which the NEXT batch is to be staged into HBM once ``step()`` has returned (model.py:227-230's
        ``.to(device)``, taken off the critical path): the loss section's side stream.  Work queued there now runs beside
        this step's backward pass, is ordered after everything of the step before it (so the buffers of step k-1 are
        free) and needs no stream of its own -- an extra stream whose first packet waits for an event shares a hardware
        queue with one of the step's streams and holds up the GEMMs queued behind it (measured: 9.7 -> 13.8 ms)."""
        from .loss import PGCTCLossFn
        main = torch.cuda.current_stream()
        side = PGCTCLossFn._lattice_streams.get(main.cuda_stream)
        if side is None:
            from . import streams
            side = streams.side_stream("loss_section")
            PGCTCLossFn._lattice_streams[main.cuda_stream] = side
        return side

    def _upper_grads_issued(self, swept):
        """Called from the first BLSTM layer's backward once its sweep has been launched: every gradient of
        gflat[upper_split:] has been issued on the side stream by then.  The collective is ordered after them AND
        after the sweep (``swept``): a collective kernel never runs beside a sweep's latency chain."""
        from .functional import grad_overlap
        side = grad_overlap.side_stream()
        s3 = grad_overlap._sides3.get(grad_overlap._key()) if grad_overlap._streamed_unjoined.get(grad_overlap._key()) else None
        with torch.cuda.stream(side):
            side.wait_event(swept)
            if s3 is not None:
                side.wait_stream(s3)      # streamed sweeps: the upper layers' weight gradients were issued THERE (the first layer's are not yet)
            self.reduce_upper(self.upper_split)

    def backward(self, loss):
        """Weight-gradient GEMMs run on a side stream under the next layer's backward sweep."""
        from .functional import grad_overlap
        from .loss import PGCTCLossFn
        grad_overlap.enabled = self.overlap_weight_grads
        early = (self.collective and self.early_reduce and self.overlap_weight_grads and self.upper_split is not None
                 and not self._hold_collectives)       # an accumulated step exchanges around its last micro-batch only
        grad_overlap.upper_grads_hook = self._upper_grads_issued if early else None
        if self._one is None or self._one.device != loss.device:
            self._one = torch.ones((), dtype=loss.dtype, device=loss.device)
        PGCTCLossFn.unit_seed_ptr = self._one.data_ptr()   # the seed gradient below IS 1: no fill, no 3.7 MB multiply on the chain
        try:
            loss.backward(gradient=self._one)
        except BaseException:
            grad_overlap._deferred.clear()      # do not let finish() mask the error with its own complaint
            raise
        finally:
            PGCTCLossFn.unit_seed_ptr = None
            grad_overlap.enabled = False
            grad_overlap.upper_grads_hook = None
            grad_overlap.finish()

    def _padded(self, x, targets, fmask, tmask):
        """The batch with empty utterances appended up to the next size the fast orders take (see ``pad_ragged_batches``)."""
        from . import hipops
        B = x.shape[0]
        q = 16 if hipops.LSTM_PLANES == 3 else 32
        Bp = -(-B // q) * q
        if not (self.pad_ragged_batches and x.is_cuda and Bp != B and Bp <= 32 and targets.dim() == 2 and fmask.dim() == 2):
            return x, targets, fmask, tmask
        n = Bp - B
        grow = lambda t_: torch.cat((t_, t_.new_zeros((n,) + tuple(t_.shape[1:]))), dim=0)
        return grow(x), grow(targets), grow(fmask), grow(tmask)

    def forward_loss(self, batch, global_batch):
        from .loss import PGCTCLossFn, pg_ctc_loss
        x, targets, fmask, tmask = batch
        from . import hipops
        self._check_limits(x, targets)
        real_b = x.shape[0]
        x, targets, fmask, tmask = self._padded(x, targets, fmask, tmask)
        padded = x.shape[0] != real_b
        if (fmask.dtype == torch.float32 and tmask.dtype == torch.int64 and targets.dtype == torch.int64 and targets.dim() == 2
                and targets.shape[1] > 0 and fmask.is_contiguous() and tmask.is_contiguous() and targets.is_contiguous()):
            in_len, tg_len, tg = hipops.batch_prep(fmask, tmask, targets)       # the collate_custom dtypes: one launch
        else:
            in_len = None
            tg_len = tmask.sum(dim=1).to(torch.int32).contiguous()
            tg = targets.to(torch.int32).contiguous()
        kl = {}
        if self.kl_weight > 0:
            # the frozen reference's sweep first, whole, then the policy's: weight 0 runs neither this forward nor the KL launch
            kl = {"kl_weight": self.kl_weight, "ref_log_probs": self._reference_log_probs(x, fmask, in_len)}
        logits, in_len = self.model.logits(x, fmask, in_len)
        sample_base, sample_ids = self._sample_addressing(real_b, x.shape[0], x.device)
        loss, nll, R_s, R_g = pg_ctc_loss(logits, in_len, tg, tg_len, lam=self.lam, seed=self.seed,
                                          offset=self.nstep + 1, global_batch=global_batch, blank=self.blank,
                                          beam=self.beam_size if self.reward_decoder == "beam" else 0,
                                          sample_base=sample_base,
                                          per_step=self.reward_mode == "per_step", num_samples=self.num_samples,
                                          baseline=self.reward_baseline, reward_unit=self.reward_unit,
                                          word_delimiter=self.word_delimiter, sample_ids=sample_ids,
                                          score_function=self.score_function, max_hyp_len=self.max_hyp_len,
                                          entropy_weight=self.entropy_weight, **kl,
                                          **({"wide_objectives": True} if self.wide_objectives else {}),
                                          **({"wide_sequence": True} if self.wide_sequence else {}),
                                          **({"step_objectives": True} if self.step_objectives else {}),
                                          **({"unit_spelling": self.unit_spelling} if self.unit_spelling is not None else {}))
        self.last_spell_truncated = PGCTCLossFn.last_spell_truncated      # 0-d int32, None without a spelling
        scored = PGCTCLossFn.last_sequence_scored                # (K,B) bool, None with score_function="path"
        self.last_sequence_scored = scored[:, :real_b] if (padded and scored is not None) else scored
        ent = PGCTCLossFn.last_entropy                           # (B,) mean frame entropy, None with entropy_weight = 0
        self.last_entropy = ent[:real_b] if (padded and ent is not None) else ent
        klm = PGCTCLossFn.last_kl                                # (B,) mean frame KL from the reference, None with kl_weight = 0
        self.last_kl = klm[:real_b] if (padded and klm is not None) else klm
        R_all = R_s if R_s.dim() == 2 else R_s.view(1, -1)       # (K,B): every sample's reward
        if R_s.dim() == 2:
            R_s = R_s.mean(dim=0)
        self.last_sample_rewards = R_all[:, :real_b] if padded else R_all
        self.last_stats = (nll[:real_b], R_s[:real_b], R_g[:real_b]) if padded else (nll, R_s, R_g)
        if self._micro is not None and self._micro.count > 1:
            self._micro_stats.append((self.last_stats, self.last_sample_rewards, self.last_sequence_scored, self.last_entropy,
                                      self.last_kl, self.last_spell_truncated))
        return loss

    def _sample_addressing(self, real_b, padded_b, device):
        """(sample_base, sample_ids) of the running batch for pg_ctc_loss: how the sampler addresses its rows' draws.
        No ids from the caller: the rows are utterances base .. base + real_b - 1 of the global batch, base = world * (real
        utterances per rank in the micro-batches before this one) + rank * real_b (``default_utt_ids``), passed as ``sample_base``
        -- no id tensor, no copy, nothing at all (-1) for a lone batch on one rank.  The id form is taken where the caller names
        ids (uploaded from pinned memory, no synchronisation) and where base + b would hand a PADDED row the counters of a real
        utterance of the next rank or micro-batch (world > 1, or more than one micro-batch): padded rows then carry id -1
        (the ids are built on the device).  A padded lone batch on one rank keeps ``sample_base``: base + b >= the global batch
        there, which the sampler already treats as beyond it."""
        mb = self._micro
        n_micro = mb.count if mb is not None else 1
        padded = padded_b != real_b
        if mb is not None and mb.ids is not None:
            host = torch.tensor(mb.ids + [-1] * (padded_b - real_b), dtype=torch.int32)
            if device.type == "cuda":
                host = host.pin_memory()
            return -1, host.to(device, non_blocking=True)
        base = self.world * (mb.offset if mb is not None else 0) + self.rank * real_b
        if padded and (self.world > 1 or n_micro > 1):
            ids = torch.arange(base, base + padded_b, dtype=torch.int32, device=device)
            ids[real_b:] = -1
            return -1, ids
        return (base if (self.world > 1 or padded or n_micro > 1) else -1), None

    def _accumulate(self, micro_batches, utt_ids, hold_last=False):
        self._micro_stats = []
        try:
            loss = super()._accumulate(micro_batches, utt_ids, hold_last=hold_last)
            if len(self._micro_stats) > 1:
                # the micro-batches' statistics in call order, real rows only
                self.last_stats = tuple(torch.cat([m[0][i] for m in self._micro_stats]) for i in range(3))
                self.last_sample_rewards = torch.cat([m[1] for m in self._micro_stats], dim=1)
                if self.score_function == "sequence":
                    self.last_sequence_scored = torch.cat([m[2] for m in self._micro_stats], dim=1)
                if self.entropy_weight > 0:
                    self.last_entropy = torch.cat([m[3] for m in self._micro_stats])
                if self.kl_weight > 0:
                    self.last_kl = torch.cat([m[4] for m in self._micro_stats])
                if self.unit_spelling is not None:
                    self.last_spell_truncated = torch.stack([m[5] for m in self._micro_stats]).sum().to(torch.int32)
        finally:
            self._micro_stats = []
        return loss
