"""MWER training over the N-best list of the in-step beam search (Prabhavalkar et al., arXiv:1712.01818).

The other standard form of expected-risk training beside the sampled objectives of ``loss.PGCTCLossFn``: the model's probability is
renormalised over the N hypotheses the decoder actually returns, and the expected (word) edit distance under that distribution is
minimised.  Nothing is sampled: no sampling variance, no sampler addressing.  The lists are the ones ``CTCDecoder.decode_batch(nbest=)``
and ``rescore`` consume.  Semantics of the kernels: include/pgasr_hip.h, section A13-MWER.

This module adds nothing to the code the default train step runs: ``train_step.py`` and ``loss.py`` do not know it.
"""
import dataclasses
import math

import torch

from . import hipops
from . import streams
from .loss import PGCTCLossFn, _check_score, _check_spelling, _check_unit, _spelled_distances, _word_distances
from .train_step import PolicyGradientTrainer

MAX_NBEST = hipops.MAX_SAMPLES       # PGASR_MAX_SAMPLES: entries per utterance the weights and gradient kernels take


@dataclasses.dataclass(frozen=True)
class MWEROptions:
    """Everything of a ``mwer_ctc_loss`` call that is not a tensor."""
    lam: float = 1.0
    beam: int = 16
    nbest: int = 4
    global_batch: int = 1
    blank: int = 0
    risk_unit: str = "char"
    word_delimiter: object = None
    max_hyp_len: object = None
    lm: object = None              # a lm.CharNgramLM: the N-best list comes from the LM-fused search (the posterior does not change)
    lm_alpha: float = 0.0
    lm_beta: float = 0.0


@dataclasses.dataclass(frozen=True)
class MWERWideOptions(MWEROptions):
    """The options of a ``wide_sequence=True`` call: ``MWEROptions`` keeps its fields (a call without the keyword has the options it
    always had), these two come with the keyword."""
    wide: bool = True              # more than 64 symbols are taken (the wide search and the A13-WIDE kernels)
    unit_lm: object = None         # a lm.UnitNgramLM: the list comes from the wide search fused with it (lm_alpha / lm_beta its weights)


@dataclasses.dataclass(frozen=True)
class MWERSpelledOptions(MWERWideOptions):
    """The options of a ``unit_spelling=`` call: the risk is counted on the spelled text of the units (``wide`` says whether
    wide_sequence=True came with it)."""
    unit_spelling: object = None   # a units.UnitSpelling


MAX_BEAM_WIDE = 128                  # pgasr_ctc_beam_search_wide


def _wide_fields(opt):
    """(wide, unit_lm) of either options class: ``MWEROptions`` has neither field and reads (False, None)."""
    return (bool(opt.wide), opt.unit_lm) if isinstance(opt, MWERWideOptions) else (False, None)


def _wide_list(opt, vocab):
    """Does the list come from the wide search?  With wide_sequence=True, above 64 symbols or with a unit LM (which only that search
    fuses); at most 64 symbols without one, the fast single-wave list as ever."""
    wide, unit_lm = _wide_fields(opt)
    return wide and (unit_lm is not None or (vocab is not None and int(vocab) > hipops.MAX_VOCAB_NARROW))


def check_mwer_options(opt, vocab=None, frames=None, symbols=None):
    """Made before any kernel runs.  Returns the options with their integers as ints.  With a spelling (``MWERSpelledOptions``) the
    risk is counted on the spelled text, so risk_unit="word" is admitted above 64 symbols too and takes no word_delimiter."""
    wide, unit_lm = _wide_fields(opt)
    spelling = getattr(opt, "unit_spelling", None)
    for name in ("beam", "nbest"):
        v = getattr(opt, name)
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name} must be an integer (got {v!r})")
    if not 1 <= opt.nbest <= opt.beam:
        raise ValueError(f"nbest {opt.nbest} outside 1 .. beam = {opt.beam}: the list is the head of the search's final beam")
    if opt.nbest > MAX_NBEST:
        raise ValueError(f"nbest {opt.nbest} > {MAX_NBEST}: the MWER kernels take at most {MAX_NBEST} hypotheses per utterance")
    if opt.lm is not None:
        if wide and vocab is not None and int(vocab) > hipops.MAX_VOCAB_NARROW:
            raise ValueError(f"lm= is a dense character LM over at most {hipops.MAX_VOCAB_NARROW} symbols (got {int(vocab)}): above that "
                             f"give unit_lm=, a lm.UnitNgramLM, which the wide beam search fuses")
        if opt.lm.blank != int(opt.blank) or (vocab is not None and opt.lm.vocab != int(vocab)):
            raise ValueError(f"the LM is over {opt.lm.vocab} symbols with blank {opt.lm.blank}; the search has "
                             f"{'its own' if vocab is None else int(vocab)} symbols and blank {int(opt.blank)}")
        for name in ("lm_alpha", "lm_beta"):
            if not math.isfinite(float(getattr(opt, name))):
                raise ValueError(f"{name} must be finite (got {getattr(opt, name)!r})")
    if unit_lm is not None:
        if not wide:
            raise ValueError("unit_lm= is fused by the wide beam search: it needs wide_sequence=True")
        if opt.lm is not None:
            raise ValueError("lm= and unit_lm= are two language models for one search: give one")
        if vocab is not None:
            hipops._unit_lm_check(unit_lm, int(vocab), opt.blank)
        for name in ("lm_alpha", "lm_beta"):
            if not math.isfinite(float(getattr(opt, name))):
                raise ValueError(f"{name} must be finite (got {getattr(opt, name)!r})")
    if vocab is not None and int(vocab) > hipops.MAX_VOCAB_NARROW:
        if not wide:
            raise ValueError(f"MWER over an alphabet of {int(vocab)} symbols needs wide_sequence=True: without it the beam search and "
                             f"the N-best kernels hold one symbol per lane, at most {hipops.MAX_VOCAB_NARROW}")
        if int(vocab) > hipops.MAX_VOCAB_WIDE:
            raise ValueError(f"alphabet of {int(vocab)} symbols > {hipops.MAX_VOCAB_WIDE}: the wide kernels hold at most 16 symbols per lane")
        if opt.risk_unit == "word" and spelling is None:
            raise ValueError(f"risk_unit='word' takes an alphabet of at most {hipops.MAX_VOCAB_NARROW} symbols (got {int(vocab)}): a "
                             f"subword unit may span a space, so a list of units has no word boundaries of its own "
                             f"(hipops.nbest_pair_distance's reason); use risk_unit='char', the unit error rate")
    if _wide_list(opt, vocab) and opt.beam > MAX_BEAM_WIDE:
        raise ValueError(f"beam {opt.beam} > {MAX_BEAM_WIDE}: the wide beam search keeps at most {MAX_BEAM_WIDE} prefixes")
    if spelling is not None:
        _check_spelling(spelling, opt.risk_unit, opt.word_delimiter, vocab=vocab)
    else:
        _check_unit(opt.risk_unit, opt.word_delimiter, blank=opt.blank, vocab=vocab)
    _check_score("sequence", opt.max_hyp_len)
    if spelling is None and opt.risk_unit == "word" and frames is not None and max(frames, symbols or 0) > hipops.WORD_MAX_STRIDE:
        raise ValueError(f"the word-level risk takes at most {hipops.WORD_MAX_STRIDE} frames and target symbols per utterance "
                         f"(pgasr_word_ids); got T = {frames}")
    return dataclasses.replace(opt, beam=int(opt.beam), nbest=int(opt.nbest),
                               max_hyp_len=None if opt.max_hyp_len is None else int(opt.max_hyp_len))


def _lm_fields(lm, lm_alpha, lm_beta):
    """The options' LM fields; without an LM the weights are not part of them, so the options are the ones of a call without these arguments."""
    return {} if lm is None else {"lm": lm, "lm_alpha": float(lm_alpha), "lm_beta": float(lm_beta)}


def _options(wide_sequence, unit_lm, lm, lm_alpha, lm_beta, unit_spelling=None, **fields):
    """``MWEROptions`` as ever, or with the keyword ``MWERWideOptions`` (the unit LM and its weights among them); with a spelling
    ``MWERSpelledOptions``."""
    if unit_spelling is not None:
        if unit_lm is not None and not wide_sequence:
            raise ValueError("unit_lm= is fused by the wide beam search: it needs wide_sequence=True")
        weights = {} if unit_lm is None else {"lm_alpha": float(lm_alpha), "lm_beta": float(lm_beta)}
        return MWERSpelledOptions(**fields, wide=bool(wide_sequence), unit_lm=unit_lm, unit_spelling=unit_spelling,
                                  **{**weights, **_lm_fields(lm, lm_alpha, lm_beta)})
    if not wide_sequence:
        if unit_lm is not None:
            raise ValueError("unit_lm= is fused by the wide beam search: it needs wide_sequence=True")
        return MWEROptions(**fields, **_lm_fields(lm, lm_alpha, lm_beta))
    weights = {} if unit_lm is None else {"lm_alpha": float(lm_alpha), "lm_beta": float(lm_beta)}
    return MWERWideOptions(**fields, unit_lm=unit_lm, **{**weights, **_lm_fields(lm, lm_alpha, lm_beta)})


class MWERLossFn(torch.autograd.Function):
    """loss = sum_b [ nll_b / (Bg max(L_b,1))  +  lam / Bg * sum_n p[n,b] r[n,b] ]

    over the first ``nbest`` entries y_n of the width-``beam`` prefix beam search's final beam (raw prefixes, no collapse_fn: distinct
    label sequences, each with a well-defined CTC likelihood), with
        valid(n,b) := n < count_b  and  |y_n| <= Lh  and  nll(y_n | x_b) finite           Lh = min(T, 1023, max_hyp_len if given)
        p[n,b]     =  softmax over the valid n of -nll(y_n | x_b), the EXACT CTC likelihood (not the first-pass beam score)
        r[n,b]     =  ED(y_b, y_n) / max(L_b,1), or WED / W(y_b) with risk_unit = "word"
        d(logits)  =  utt_scale_b (softmax - occ_target) + sum_n coef[n,b] (softmax - occ_{y_n}),
        coef[n,b]  =  -lam / Bg * p[n,b] (r[n,b] - rbar_b)
    ``MWERWideOptions`` (wide_sequence=True) with more than 64 symbols: the list is ``ctc_beam_search_wide``'s (beam <= 128; with ``opt.unit_lm``
    the search fused with that back-off unit LM), the lattices and the gradient pass are the A13-WIDE entries; char risk only.
    With ``opt.lm`` the list is the final beam of the LM-FUSED search (every extension by s gets lm_alpha * ln p_lm(s | context) + lm_beta,
    ``ctc_beam_search_nbest(lm=, fast=True, fast_lm=True)``: the single-wave kernel with the LM term): the hypotheses the model is
    decoded to at test time.  The LM only chooses which hypotheses are in the list; p, r and the gradient are formed as above.
    Stream layout of ``PGCTCLossFn``: the target lattice stays on the calling stream; N-best search, hypothesis lattices, (word) edit
    distance and the weights run on its side stream and are joined before the one gradient pass.
    ``MWERLossFn.last_nbest``: the ``CTCNBest`` of the last call; ``MWERLossFn.last_posterior``: p (N,B) fp32, 0 where not valid;
    ``MWERLossFn.last_risk``: r (N,B) fp32.
    Returns (loss, nll (B), expected_reward (B) = -rbar, top_reward (B) = -r[0]), the last three detached."""

    last_nbest = None
    last_posterior = None
    last_risk = None           # r (N,B) fp32 of the last call
    last_spell_truncated = None    # 0-d int32: rows of the last unit_spelling call whose spelling was cut at the row limit

    @staticmethod
    def forward(ctx, logits, in_len, targets, tg_len, log_probs, opt):
        T, B, V = logits.shape
        N, blank = opt.nbest, opt.blank
        wd = opt.word_delimiter if opt.risk_unit == "word" else None
        sp = getattr(opt, "unit_spelling", None)
        MWERLossFn.last_spell_truncated = None
        Lh = hipops.hyp_len_cap(T, opt.max_hyp_len)
        inv_gb = 1.0 / float(opt.global_batch)
        lp = log_probs
        if lp is None or lp.shape != logits.shape or not lp.is_contiguous():
            lp = hipops.log_softmax_rows(logits.contiguous())
        main = torch.cuda.current_stream()
        side = PGCTCLossFn._lattice_streams.setdefault(main.cuda_stream, None) or streams.side_stream("loss_section")
        PGCTCLossFn._lattice_streams[main.cuda_stream] = side
        side.wait_stream(main)
        with torch.cuda.stream(side):
            if _wide_list(opt, V):
                # wide_sequence=True above 64 symbols (or with a unit LM): the exact wide search's list; everything behind it is the
                # sequence of calls below, whose wrappers take the A13-WIDE entries by V
                fused = {} if opt.unit_lm is None else {"unit_lm": opt.unit_lm, "lm_alpha": float(opt.lm_alpha), "lm_beta": float(opt.lm_beta)}
                nb = hipops.ctc_beam_search_wide(lp, in_len, beam=opt.beam, nbest=N, blank=blank, collapse=False, **fused)
            else:
                fused = {} if opt.lm is None else {"lm": opt.lm, "lm_alpha": float(opt.lm_alpha), "lm_beta": float(opt.lm_beta), "fast_lm": True}
                nb = hipops.ctc_beam_search_nbest(lp, in_len, beam=opt.beam, nbest=N, blank=blank, collapse=False, fast=True, **fused)
            # a hypothesis over the cap gets the EMPTY hypothesis' lattice (rows beyond count have length 0 already): every lattice
            # the gradient pass reads was really computed, and meets a coefficient of 0
            lat_len = torch.where(nb.lengths > Lh, torch.zeros_like(nb.lengths), nb.lengths)
            hyp_nll, hyp_lattice = hipops.ctc_hyp_lattice(lp, nb.tokens, lat_len, in_len, Lh, blank=blank)
            if sp is not None:
                # the risk over the spelled text: r = ED(chars) / C(y) or WED / W(y)
                dist, risk_len, MWERLossFn.last_spell_truncated = _spelled_distances(targets, tg_len, nb.tokens, nb.lengths, N, sp,
                                                                                    opt.risk_unit)
            elif wd is not None:
                dist, risk_len = _word_distances(targets, tg_len, nb.tokens, nb.lengths, N, wd)
            else:
                dist = hipops.edit_distance(targets.repeat(N, 1), tg_len.repeat(N), nb.tokens.view(N * B, T), nb.lengths.view(N * B))
                risk_len = tg_len
        nll, lattice = hipops.ctc_lattice(lp, targets, in_len, tg_len, blank=blank)
        with torch.cuda.stream(side):
            side.wait_stream(main)                   # the weights form the loss terms from the target's nll
            p, r, coef, utt_scale, rbar, terms = hipops.mwer_weights(dist, risk_len, tg_len, hyp_nll, nb.lengths, nb.count, nll, Lh,
                                                                     opt.lam, inv_gb)
        main.wait_stream(side)
        for t_ in ((nb.tokens, nb.lengths, nb.score, nb.count, lat_len, hyp_nll, dist, p, r, coef, utt_scale, rbar, terms)
                   + ((MWERLossFn.last_spell_truncated,) if sp is not None else ())):
            streams.hold(t_, main)
        MWERLossFn.last_nbest, MWERLossFn.last_posterior, MWERLossFn.last_risk = nb, p, r
        grad = hipops.ctc_grad_from_lattices_nbest(lp, in_len, tg_len, lattice, hyp_lattice, utt_scale, coef, lat_len)
        loss = terms.sum()
        expected, top = -rbar, -r[0]
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(nll, expected, top)
        ctx.set_materialize_grads(False)
        return loss, nll, expected, top

    @staticmethod
    def backward(ctx, g, *unused):
        (grad,) = ctx.saved_tensors
        # the trainer's backward registers its unit seed with PGCTCLossFn: the same shortcut, the same counter
        if PGCTCLossFn.unit_seed_ptr is not None and g.data_ptr() == PGCTCLossFn.unit_seed_ptr and g.numel() == 1:
            PGCTCLossFn.unit_hits += 1
        else:
            grad = grad * g
        return (grad,) + (None,) * (len(ctx.needs_input_grad) - 1)


def mwer_ctc_loss(logits, in_len, targets, tg_len, lam=1.0, beam=16, nbest=4, global_batch=None, blank=0, risk_unit="char",
                  word_delimiter=None, max_hyp_len=None, log_probs=None):
    """CTC + lam * MWER over the ``nbest`` best hypotheses of the width-``beam`` prefix beam search (see ``MWERLossFn``).
    logits (T,B,V) fp32 on the GPU, in_len / tg_len (B) int32, targets (B,L) int32.  1 <= nbest <= beam, nbest <= 16.
    risk_unit: "char" (default) -- r = ED / |y|; "word" -- r = WED / W(y), words split at the token ``word_delimiter``.
    max_hyp_len: hypotheses of more tokens are left out of the list's posterior (None: min(T, 1023)); it bounds the hypothesis-lattice
    workspace, 2 * nbest*B*T * roundup64(2*Lh+1) * 4 bytes.
    log_probs: log_softmax(logits) if the caller already has it (picked up from ``logits.log_probs`` when not given).
    Returns (loss, nll (B), expected_reward (B) = -rbar, top_reward (B) = -r[0]).  The list is the acoustic search's;
    ``mwer_ctc_loss_lm`` takes it from the search fused with a language model, and (``wide_sequence=True``) takes alphabets of 65 ..
    1024 symbols: this function keeps its parameter list."""
    return mwer_ctc_loss_lm(logits, in_len, targets, tg_len, None, lam=lam, beam=beam, nbest=nbest, global_batch=global_batch, blank=blank,
                            risk_unit=risk_unit, word_delimiter=word_delimiter, max_hyp_len=max_hyp_len, log_probs=log_probs)


def mwer_ctc_loss_lm(logits, in_len, targets, tg_len, lm=None, lm_alpha=0.0, lm_beta=0.0, lam=1.0, beam=16, nbest=4, global_batch=None,
                     blank=0, risk_unit="char", word_delimiter=None, max_hyp_len=None, log_probs=None, wide_sequence=False,
                     unit_lm=None, unit_spelling=None):
    """``mwer_ctc_loss`` over the N-best list of the LM-FUSED search: ``lm`` a ``lm.CharNgramLM`` over the same V symbols and blank, its
    weights lm_alpha / lm_beta as ``CTCDecoder`` takes them (``MWERLossFn``; the list comes from the single-wave kernel's LM
    instantiation where its limits allow).  The posterior over the list stays the exact CTC likelihood.  ``lm=None`` is
    ``mwer_ctc_loss``: the options and the calls it always made.  (A function of its own because ``mwer_ctc_loss`` keeps its
    parameter list.)
    wide_sequence: opt-in for an alphabet of 65 .. 1024 symbols (V <= 64 without unit_lm: the call as it was, bit for bit) -- the list
    is ``hipops.ctc_beam_search_wide``'s (beam <= 128, nbest <= 16), risk_unit "char" only; unit_lm: a ``lm.UnitNgramLM`` that search is
    fused with, weighted by lm_alpha / lm_beta -- above 64 symbols ``lm`` (dense, character-level) is refused in its favour.  Set
    max_hyp_len for unit models: the default cap takes 2.1 GB of lattices at nbest = 4, B = 32, T = 1000.
    unit_spelling: None (default: the call as it was) or the ``units.UnitSpelling`` of the alphabet's subword units -- the distances
    and the risk normaliser come from the spelled text of targets and hypotheses (``pgasr_unit_spell``): risk_unit="char" is
    r = ED(chars) / max(C(y),1), "word" r = WED / W(y) with words split at the spelling's " " (no word_delimiter), admitted above 64
    symbols too.  ``MWERLossFn.last_spell_truncated``: the rows cut at the 4094-character row limit (0-d int32 on the device)."""
    if logits.dim() != 3:
        raise ValueError("mwer_ctc_loss: logits (T,B,V)")
    T, B, V = logits.shape
    opt = check_mwer_options(_options(wide_sequence, unit_lm, lm, lm_alpha, lm_beta, unit_spelling, lam=float(lam), beam=beam, nbest=nbest,
                                      global_batch=int(global_batch or B), blank=int(blank), risk_unit=risk_unit,
                                      word_delimiter=word_delimiter, max_hyp_len=max_hyp_len),
                             vocab=V, frames=T, symbols=targets.shape[1] if targets.dim() == 2 else 0)
    for name, t_ in (("logits", logits), ("in_len", in_len), ("targets", targets), ("tg_len", tg_len)):
        if not t_.is_cuda:
            raise hipops._lib.PgasrError(f"{name} must live on the GPU (got {t_.device}); there is no CPU path")
    if log_probs is None:
        log_probs = getattr(logits, "log_probs", None)
        if log_probs is not None and getattr(logits, "log_probs_version", None) != logits._version:
            log_probs = None
    return MWERLossFn.apply(logits, in_len, targets, tg_len, log_probs, opt)


class MWERTrainer(PolicyGradientTrainer):
    """``PolicyGradientTrainer`` with the MWER objective: only ``forward_loss`` differs, so ``step``, ``compute_gradients``,
    ``step_accumulated``, clipping, shards and RCCL work as in the parent.  Nothing is sampled, so ``utt_ids`` and the sampler's
    addressing play no part: a shard or micro-batch contributes its own utterances' terms, normalised by the global batch.
    ``last_stats`` = (nll, expected reward -rbar, top-hypothesis reward -r[0]), each (B,); ``last_sample_rewards`` = -r, (nbest, B);
    ``last_posterior`` (nbest, B), 0 where an entry is not in the list's posterior.
    lm / lm_alpha / lm_beta: None (default) or a ``lm.CharNgramLM`` and its weights -- the N-best lists then come from the LM-fused search
    (the standard MWER setting, arXiv:1712.01818 section 3: train on the lists the model is decoded to); ``mwer_options`` holds the checked options.
    wide_sequence=True: an alphabet of 65 .. 1024 subword units -- MAX_VOCAB becomes 1024, the lists come from ``ctc_beam_search_wide``
    (beam_size <= 128, nbest <= 16), with ``unit_lm`` (a ``lm.UnitNgramLM``, weights lm_alpha / lm_beta) from that search fused with it;
    risk_unit="char" and no dense ``lm`` above 64 symbols.  Set max_hyp_len for unit models (2.1 GB of lattices at nbest = 4, B = 32,
    T = 1000 with the default cap).  ``wide_alphabet=True`` without it keeps being refused.
    unit_spelling: a ``units.UnitSpelling`` -- the risk is counted on the spelled text (characters, or words with risk_unit="word", which
    this admits above 64 symbols; no word_delimiter); ``last_spell_truncated`` as in the parent."""

    _FIXED = {"num_samples": 1, "reward_baseline": "hypothesis", "score_function": "path", "reward_mode": "utterance",
              "reward_decoder": "greedy", "entropy_weight": 0.0}

    def __init__(self, model, lr=5e-4, lam=1.0, seed=0, blank=0, world_size=1, process_group=None, rank=0, precision=None,
                 max_grad_norm=None, beam_size=16, nbest=4, risk_unit="char", word_delimiter=None, max_hyp_len=None, lm=None, lm_alpha=0.0,
                 lm_beta=0.0, wide_sequence=False, unit_lm=None, unit_spelling=None, **sampled):
        wide_sequence = bool(wide_sequence)
        if sampled.pop("hotwords", None) is not None:
            raise ValueError("hotwords: MWERTrainer trains on unbiased N-best lists -- there is no hotword bias during training; bias "
                             "the decoder (CTCDecoder(hotwords=))")
        if sampled.pop("wide_alphabet", False) and not wide_sequence:
            raise ValueError("MWERTrainer takes an alphabet of at most 64 symbols: the beam search and the N-best kernels hold one "
                             "symbol per lane (wide_alphabet=True is PolicyGradientTrainer's default objective only)")
        for k, v in sampled.items():
            if k not in self._FIXED:
                raise TypeError(f"MWERTrainer got an unexpected keyword argument {k!r}")
            if isinstance(v, bool) or v != self._FIXED[k]:
                raise ValueError(f"MWERTrainer samples nothing: {k}={v!r} has no meaning here (an entropy bonus for MWER is not built)")
        vocab = getattr(getattr(model, "head", None), "out_features", None)
        opt = check_mwer_options(_options(wide_sequence, unit_lm, lm, lm_alpha, lm_beta, unit_spelling, blank=int(blank), beam=beam_size, nbest=nbest,
                                          risk_unit=risk_unit, word_delimiter=word_delimiter, max_hyp_len=max_hyp_len), vocab=vocab)
        # wide_sequence=True lifts MAX_VOCAB to 1024 itself: the parent's wide_alphabet, whose default objective is not run here
        super().__init__(model, lr=lr, lam=lam, seed=seed, blank=blank, world_size=world_size, process_group=process_group, rank=rank,
                         precision=precision, max_grad_norm=max_grad_norm,
                         **({"wide_alphabet": True, "wide_sequence": True} if wide_sequence else {}))
        self.beam_size, self.nbest = opt.beam, opt.nbest
        self.risk_unit, self.mwer_max_hyp_len = risk_unit, opt.max_hyp_len
        self.risk_delimiter = None if word_delimiter is None else int(word_delimiter)
        self.mwer_lm, self.mwer_lm_alpha, self.mwer_lm_beta = opt.lm, opt.lm_alpha, opt.lm_beta
        self.mwer_unit_lm = _wide_fields(opt)[1]
        self.mwer_options = opt
        self.mwer_unit_spelling = unit_spelling
        self.last_posterior = None

    def _list_fields(self):
        """What ``mwer_ctc_loss_lm`` takes beyond the call it always got: nothing without an LM and without wide_sequence."""
        if not self.wide_sequence:
            return _lm_fields(self.mwer_lm, self.mwer_lm_alpha, self.mwer_lm_beta)
        fields = {"wide_sequence": True, "unit_lm": self.mwer_unit_lm}
        if self.mwer_lm is not None or self.mwer_unit_lm is not None:
            fields.update(lm=self.mwer_lm, lm_alpha=self.mwer_lm_alpha, lm_beta=self.mwer_lm_beta)
        return fields

    def forward_loss(self, batch, global_batch):
        x, targets, fmask, tmask = batch
        self._check_limits(x, targets)
        real_b = x.shape[0]
        x, targets, fmask, tmask = self._padded(x, targets, fmask, tmask)
        padded = x.shape[0] != real_b
        if (fmask.dtype == torch.float32 and tmask.dtype == torch.int64 and targets.dtype == torch.int64 and targets.dim() == 2
                and targets.shape[1] > 0 and fmask.is_contiguous() and tmask.is_contiguous() and targets.is_contiguous()):
            in_len, tg_len, tg = hipops.batch_prep(fmask, tmask, targets)
        else:
            in_len = None
            tg_len = tmask.sum(dim=1).to(torch.int32).contiguous()
            tg = targets.to(torch.int32).contiguous()
        logits, in_len = self.model.logits(x, fmask, in_len)
        loss, nll, expected, top = mwer_ctc_loss_lm(logits, in_len, tg, tg_len, lam=self.lam, beam=self.beam_size, nbest=self.nbest,
                                                    global_batch=global_batch, blank=self.blank, risk_unit=self.risk_unit,
                                                    word_delimiter=self.risk_delimiter, max_hyp_len=self.mwer_max_hyp_len,
                                                    **self._list_fields(),
                                                    **({} if self.mwer_unit_spelling is None else {"unit_spelling": self.mwer_unit_spelling}))
        self.last_spell_truncated = MWERLossFn.last_spell_truncated
        post = MWERLossFn.last_posterior
        R_all = -MWERLossFn.last_risk                            # (N,B): every entry's reward
        self.last_posterior = post[:, :real_b] if padded else post
        self.last_sample_rewards = R_all[:, :real_b] if padded else R_all
        self.last_stats = (nll[:real_b], expected[:real_b], top[:real_b]) if padded else (nll, expected, top)
        if self._micro is not None and self._micro.count > 1:
            self._micro_stats.append((self.last_stats, self.last_sample_rewards, None, None))
        return loss
