"""Losses of the path.

``customNLLLoss`` keeps the reference's name, constructor and call signature (loss.py:5-17),
including its quirk that a falsy ignore_index (None or 0) ignores nothing.  ``PGCTCLossFn`` is
the spec'd objective the reference lacks: CTC + lambda * REINFORCE with a
self-critical (greedy) baseline, computed by the HIP kernels in one fused gradient pass.
"""
import dataclasses
import numbers

import torch
import torch.nn as nn

from . import hipops
from . import streams


class customNLLLoss(nn.Module):
    """sum_i mean_b( -inp[i, b, target[b, i]] ) for inp (L,B,V) log-probs, target (B,L)."""

    def __init__(self, ignore_index=None):
        super().__init__()
        self.ignore_index = ignore_index

    def forward(self, inp, target):
        L, B, V = inp.shape
        tgt = target.t().unsqueeze(-1).long()                 # (L,B,1)
        picked = -inp.gather(2, tgt).squeeze(-1)              # (L,B)
        if self.ignore_index:                                 # loss.py:9: falsy -> ignore nothing
            keep = (target.t() != self.ignore_index).to(inp.dtype)
            return ((picked * keep).sum(dim=1) / keep.sum(dim=1)).sum()
        return picked.mean(dim=1).sum()


class PGCTCLossFn(torch.autograd.Function):
    """loss = (1/Bg) sum_b [ nll_b / max(L_b,1)  -  lam * (R_s,b - R_g,b) * sum_{t<T_b} log p(pi_t,b) ]

    pi ~ softmax(logits) per frame (Philox, seed-addressable), R = -ED(y, collapse(path)) / max(L,1)
    for the sampled (R_s) path and for the baseline hypothesis (R_g): the greedy best path (beam = 0), or -- the
    reference's own reward definition, policy_grad.py:6-8 -- the prefix-beam-search hypothesis of width ``beam``
    after collapse_fn.  Bg = global batch (all ranks).  The reward is the utterance-level R = -ED / |y|: the
    reference's per-step r_t (policy_grad.py:10-15) telescope to |y| - ED(y, yhat), i.e. to the
    same R up to the constant |y| that the baseline subtracts; the per-t values themselves are available from
    policy_grad.rewards_all_t, and the gradient uses their sum (one coefficient per utterance).
    ``per_step = True`` (opt-in) puts the per-step rewards themselves into the gradient, as rewards-to-go: the coefficient of
    frame t becomes lam/Bg (G_s(t) - G_g(t)) / max(L,1) with G(t) = ED(y, yhat[:c(t)]) - ED(y, yhat) the sum of the rewards of the
    characters that start at frames >= t (c(t) = characters started before t), for the sampled path and -- the baseline -- for the
    greedy path at the same frame (``pgasr_pg_step_coefs``); frame 0 carries the utterance coefficient.  Greedy baseline only (a
    beam hypothesis has no frame alignment).
    ``num_samples = K > 1`` or ``baseline = "leave_one_out"`` (multi-sample REINFORCE, include/pgasr_hip.h): K paths pi_k per
    utterance, draw k of frame t from Philox counter (t*Bg + b_global, offset, 0, k) -- draw 0 is the single-sample draw --, rewards
    R_k = -ED(y_b, collapse(pi_k)) / max(L_b,1) and per sample a baseline b_k:
      "hypothesis" (default): R_g, the reward of the greedy or beam hypothesis as above;
      "leave_one_out": (S - R_k) / (K-1) with S = sum_j R_j in j order, fp32 (K >= 2; the greedy argmax and the beam search are skipped).
        loss = sum_b [ nll_b / (Bg max(L_b,1))  -  sum_k lam / (Bg K) (R_k - b_k) sum_{t<T_b} log p(pi_k,t,b) ]
    and d(logits) adds the K REINFORCE terms in k order after the CTC part.  K = 1 with the hypothesis baseline is the objective
    above, on the single-path kernels.  per_step takes K = 1 only, unless step_objectives is set (below).  The baseline of an
    utterance uses that utterance's samples alone, so data-parallel ranks exchange nothing for it.
    ``step_objectives = True`` (opt-in; False, the default, is every call, refusal and bit above): per_step with num_samples 1..16,
    either baseline, entropy_weight, kl_weight and the shard addressings, and with alphabets of 65 .. 1024 symbols
    (include/pgasr_hip.h, A12-STEP).  Path rows of utterance b: P = K + 1 with the hypothesis baseline -- the greedy path, then the K
    samples --, P = K with leave one out.  For row w with collapsed length n_w, D_w[i] = ED(y_b, yhat_w[:i]) and c_w(t) the characters
    started at frames < t (a character starts at t < T_b where the label is not blank and t = 0 or the label differs from that at
    t - 1), clipped to n_w, the reward-to-go is the integer G_w(t) = D_w[c_w(t)] - D_w[n_w], and in fp32
        kf_b         = ((lam / Bg) / K) / max(L_b,1)
        coef[k,t,b]  = kf_b (G_k(t) - G_greedy(t))                                          "hypothesis"
                     = kf_b (G_k(t) - (S(t) - G_k(t)) / (K-1)),  S(t) = sum_j G_j(t)        "leave_one_out"     0 for t >= T_b
        loss         = sum_b nll_b utt_scale_b - sum_k sum_b sum_{t<T_b} coef[k,t,b] log p(pi_k[t,b])    + the entropy and KL terms
        d(logits)    = utt_scale_b (softmax - occ) + sum_k coef[k,t,b] (softmax - onehot(pi_k[t,b]))  in k order, then the two tails
    Frame 0 carries the utterance-level pg_coef[k,b] in exact arithmetic; either baseline of a frame depends on the other rows alone, so
    the estimator is unbiased.  R_s (K,B), R_b (B) and utt_scale are the multi-sample call's (``pgasr_pg_rewards_multi``, whose (K,B)
    coefficients are not used).  K = 1 with the hypothesis baseline and no entropy or KL term above 64 symbols keeps the per_step
    launches and bits above; every other call samples, collapses and scores as a multi-sample call and takes
    ``pgasr_pg_step_coefs_multi`` (side stream, after the edit distance), ``pgasr_ctc_grad_from_lattice_multi_steps`` and
    ``pgasr_pg_loss_value_multi_steps``; with leave one out no greedy arg-max runs.  Above 64 symbols K > 1, leave one out, entropy and
    KL need wide_objectives=True as well.  beam > 0, score_function="sequence", reward_unit="word" and unit_spelling stay refused.
    ``reward_unit = "word"`` (opt-in): every reward above -- sample, hypothesis and the leave-one-out baselines -- is the word-level
    R = -WED(y, yhat) / W(y), words being the runs between ``word_delimiter`` tokens exactly as str.split(" ") cuts the decoded string
    (n delimiters give n + 1 words, empty ones included), WED the Levenshtein distance over the word lists and W(y) >= 1 the target's
    word count; the word step (pgasr_word_ids) runs on the side stream between collapse and edit distance.  The CTC term keeps
    utt_scale = 1 / (Bg max(L_chars,1)).  Not with per_step (character-level only).
    ``score_function = "sequence"`` (opt-in; the default "path" is everything above, launch for launch): the reward depends on the
    HYPOTHESIS y_k = collapse(pi_k) alone, so the score function of sample k becomes the CTC likelihood of its hypothesis,
    log p(y_k | x) = -nll(y_k) summed over all its alignments, instead of log p(pi_k | x) -- the same expectation (E[grad log p(pi|x) |
    y] = grad log p(y|x)), no larger variance (sampled expected risk / MWER).  With rewards, baselines, pg_coef[k,b] = lam / (Bg K)
    (R_k - b_k) and utt_scale_b = 1 / (Bg max(L_b,1)) exactly as above (any num_samples, either baseline, greedy or beam hypothesis,
    char or word reward) and a length cap Lh = min(T, 1023, max_hyp_len if given):
        seq(k,b)  :=  |y_k,b| <= Lh
        loss      =  sum_b [ nll_b utt_scale_b
                             + sum_k pg_coef[k,b] * ( seq(k,b) ?  nll(y_k,b | x_b)  :  -sum_{t<T_b} log p(pi_k[t,b]) ) ]
        d(logits) =  utt_scale_b (softmax - occ_target)
                     + sum_k pg_coef[k,b] * ( seq(k,b) ?  (softmax - occ_{y_k})  :  (softmax - onehot(pi_k[t,b])) )     in k order
    occ_y is the CTC posterior occupancy of y's lattice over the utterance's own T_b frames.  A hypothesis longer than the cap keeps
    the path-level term: the choice depends on y alone, so the mixture is still unbiased and a long sample never fails; a hypothesis
    nll of +inf contributes nothing, as for targets.  The hypothesis lattices take 2 * K*B*T * roundup64(2*Lh+1) * 4 bytes of cached
    workspace (B = 32, T = 1000, K = 4: 2.1 GB at Lh = 1000, 0.46 GB with max_hyp_len = 200; hipops.ctc_hyp_workspace_bytes).  Always
    the multi-sample kernels (K = 1 included); not with per_step (frame-aligned coefficients have no sequence form).
    ``PGCTCLossFn.last_sequence_scored``: (K,B) bool on the device, which samples of the last call took the sequence term (None after
    a "path" call).
    ``entropy_weight = beta > 0`` (opt-in; 0, the default, is every objective above launch for launch and bit for bit): entropy
    regularisation of the frame policy, the exploration side -- nothing above keeps the per-frame distributions from collapsing to
    one-hot rows, after which every sample is the greedy path, R_k - b_k = 0 and the REINFORCE term is silent.  With
    H_{t,b} = -sum_v p_v ln p_v (nats, 0 ln 0 := 0) and ent_scale_b = beta / (Bg max(T_b,1)):
        loss      += -sum_b ent_scale_b sum_{t<T_b} H_{t,b}
        d(logits) += ent_scale_b p_v (ln p_v + H_{t,b})     for t < T_b, 0 beyond
    The bonus is the utterance's MEAN frame entropy, so beta is in loss units per nat per frame and does not grow with T.  It does
    not depend on targets, rewards, samples or the score function (any other option, per_step included, takes it), an utterance whose
    target nll is +inf still gets it, an empty utterance adds nothing, and nothing in it is sampled, so shards and micro-batches need
    no addressing for it.  ``pgasr_frame_entropy`` runs on the side stream beside the lattice; the gradient passes add the term in the
    pass that writes d(logits) (their ``_ent`` entries).  ``PGCTCLossFn.last_entropy``: (B,) mean frame entropy per utterance of the
    last call, detached, on the device (None after a call with weight 0); ``metrics.frame_entropy`` is the same kernel for monitoring.
    ``kl_weight = gamma > 0`` with ``ref_log_probs`` (opt-in; 0, the default, is every objective above launch for launch and bit for
    bit, whether or not a reference tensor is given): a KL penalty towards a frozen reference policy q, the anchor of an RL
    fine-tune of a pretrained model -- the ``lam`` mix holds the policy near the targets, not near the model it started from.  The
    reverse KL(p || q) of KL-regularised policy optimisation, per frame, with lnq_v = max(ref_log_probs[t,b,v], -104) (just under
    ln 2^-149: a zero reference probability costs a large finite penalty, never inf or NaN) and kl_scale_b = gamma / (Bg max(T_b,1)):
        KL_{t,b}   = sum_v p_v (ln p_v - lnq_v)              nats; a symbol with p_v = 0 adds exactly 0
        loss      += sum_b kl_scale_b sum_{t<T_b} KL_{t,b}
        d(logits) += kl_scale_b p_v (ln p_v - lnq_v - KL_{t,b})     for t < T_b, 0 beyond
    A mean over the utterance's own frames like the entropy bonus, so gamma is in loss units per nat per frame.  It depends on the
    two log-prob tensors and the lengths alone: with every other option (per_step and entropy_weight included), nothing sampled, no
    addressing for shards and micro-batches (slice ref_log_probs as the logits are sliced), and an utterance with an infeasible
    target still gets it.  ref_log_probs is one more tensor input without a gradient: fp32, contiguous, detached, of the logits' shape
    and device.  ``pgasr_frame_kl`` runs on the side stream after the entropy launch, under the lattice; the gradient passes add the
    term after the entropy term in the pass that writes d(logits) (their ``_kl`` entries).  ``PGCTCLossFn.last_kl``: (B,) mean frame KL
    per utterance of the last call, detached, on the device (None after a call with weight 0; not clamped at 0, it can read -1e-7
    where the policies agree); ``metrics.frame_kl`` is the same kernel for monitoring.
    ``unit_spelling`` (opt-in; None, the default, is every objective above launch for launch): for a model of subword units, whose
    units may hold spaces, every reward above is counted on the spelled TEXT -- targets (once) and collapsed paths go through
    ``pgasr_unit_spell`` on the side stream between collapse and the distance, and R = -ED(chars) / max(C(y),1) for reward_unit="char",
    -WED / W(y) for "word" with words split at the spelling's " ".  utt_scale stays on the unit counts, the unit rows still feed the
    hypothesis lattices of score_function="sequence".  Not with per_step.  ``PGCTCLossFn.last_spell_truncated``: how many rows were
    cut at the 4094-character row limit, a 0-d int32 on the device that nothing synchronises on (None after a call without).
    Returns (loss, stats) where stats = (nll (B), R_s (B), R_g (B)) detached; with K > 1, (nll (B), R_s (K,B), R_b (B)) where
    R_b is the baseline averaged over k (R_g for "hypothesis")."""

    _lattice_streams = {}      # one side stream per calling stream
    # The trainer seeds loss.backward() with ITS OWN tensor of value 1 and registers that tensor's address here: only when
    # the incoming gradient IS that tensor (nothing between this function's output and the seed scaled it) is the
    # 3.7 MB multiply skipped.  Any other g -- a subclass that scales the loss, gradient accumulation with 1/k, a second
    # trainer -- takes grad * g.
    unit_seed_ptr = None
    unit_hits = 0              # how often the shortcut was taken (tests)
    last_sequence_scored = None    # (K,B) bool: the samples of the last score_function="sequence" call that were sequence-scored
    last_entropy = None            # (B,) fp32: mean frame entropy per utterance of the last entropy_weight > 0 call
    last_kl = None                 # (B,) fp32: mean frame KL(p || reference) per utterance of the last kl_weight > 0 call
    last_spell_truncated = None    # 0-d int32: rows of the last unit_spelling call whose spelling was cut at the row limit
    @staticmethod
    def forward(ctx, logits, in_len, targets, tg_len, log_probs, sample_ids, opt, ref_log_probs=None):
        """opt: the ``PGOptions`` of the call, checked by ``pg_ctc_loss``; ref_log_probs: read only when opt.kl_weight > 0."""
        T, B, V = logits.shape
        PGCTCLossFn.last_sequence_scored = PGCTCLossFn.last_entropy = PGCTCLossFn.last_kl = PGCTCLossFn.last_spell_truncated = None
        K, beam, blank = opt.num_samples, opt.beam, opt.blank
        beta, gamma = opt.entropy_weight, opt.kl_weight
        ent_mean = ent_scale = kl_mean = kl_scale = None
        loo = opt.baseline == "leave_one_out"
        wd = opt.word_delimiter if opt.reward_unit == "word" else None
        sp = opt.unit_spelling
        Lh = hipops.hyp_len_cap(T, opt.max_hyp_len) if opt.score_function == "sequence" else None     # the hypothesis-length cap
        # Kernel family: the single-path kernels (per_step's (T,B) coefficients included) for the one configuration they were
        # written for, the multi-sample kernels -- K = 1 included -- for every other, their _seq pair when Lh is set.
        single = K == 1 and not loo and Lh is None
        # Above 64 symbols the single-path gradient pass has no entropy or KL form: such a call samples, collapses and scores as a
        # single-path call does and takes the multi-sample pass and loss value with K = 1 (samples = sample[None], coef[None]).
        single_pass = single and not (V > hipops.MAX_VOCAB_NARROW and (beta > 0 or gamma > 0))
        # step_objectives: per-step rewards of every configuration but the one the single-path per-step kernels were written for
        # take the multi-sample family with (K,T,B) coefficients, K = 1 included
        steps = opt.per_step and opt.step_objectives and not single_pass
        single = single and not steps
        greedy_row = not loo and beam == 0      # the greedy path is sampled along and collapsed as row 0
        P = K + (0 if loo else 1)               # path sets that are collapsed and scored: [hypothesis,] sample 0 .. K-1
        inv_gb = 1.0 / float(opt.global_batch)
        dev = logits.device
        # log-probs the head kernel already produced for exactly this tensor (model.Seq2Seq.logits), else one pass over the logits
        lp = log_probs
        if lp is None or lp.shape != logits.shape or not lp.is_contiguous():
            lp = hipops.log_softmax_rows(logits.contiguous())
        # The alpha/beta lattice (96 workgroups, a serial chain of T frames, ~0.27 ms at T=1000) is the long pole of this
        # section and stays on the CALLING stream; sampling, collapse, (beam search,) (the K*B hypothesis lattices,) edit
        # distance and the reward arithmetic (~0.13 ms with the greedy baseline) run beside it on a side stream -- no third
        # stream -- and are joined before the gradient pass.  (Round 1 had it the other way round: two cross-stream hops then
        # sat on the critical chain.)
        main = torch.cuda.current_stream()
        side = PGCTCLossFn._lattice_streams.setdefault(main.cuda_stream, None) or streams.side_stream("loss_section")
        PGCTCLossFn._lattice_streams[main.cuda_stream] = side
        # sample_base >= 0: this shard's first utterance in the GLOBAL batch -- the draws are then addressed globally
        # sample_ids: the global index of every row instead (micro-batches of an accumulated step, shards that are not contiguous)
        if sample_ids is not None:
            lay = {"batch_stride": opt.global_batch, "utt_ids": sample_ids}
        else:
            lay = {"batch_stride": opt.global_batch, "batch_offset": opt.sample_base} if opt.sample_base >= 0 else {}
        side.wait_stream(main)
        with torch.cuda.stream(side):
            if beta > 0:
                # the policy's entropy needs the log-probs alone: first on the side stream, under the lattice
                ent_mean, ent_scale = hipops.frame_entropy(lp, in_len, beta, inv_gb)
                PGCTCLossFn.last_entropy = ent_mean
            if gamma > 0:
                # .. and so does the KL from the reference, whose log-probs the caller finished on the calling stream
                kl_mean, kl_scale = hipops.frame_kl(lp, ref_log_probs, in_len, gamma, inv_gb)
                PGCTCLossFn.last_kl = kl_mean
            # samples (K,T,B); paths = what one collapse takes: [greedy,] samples
            if single:
                greedy, sample = hipops.frame_argmax_sample(lp, seed=opt.seed, offset=opt.offset, want_greedy=greedy_row, **lay)
                samples = sample[None]
                paths = torch.stack((greedy, sample), dim=0) if greedy_row else samples
            elif greedy_row:
                paths = torch.empty(P, T, B, dtype=torch.int32, device=dev)
                hipops.frame_sample_multi(lp, K, seed=opt.seed, offset=opt.offset, out=(paths[0], paths[1:]), **lay)
                samples = paths[1:]
            else:
                # leave-one-out: the baseline comes from the other samples, no greedy argmax and no beam search
                _, samples = hipops.frame_sample_multi(lp, K, seed=opt.seed, offset=opt.offset, **lay)
                paths = samples
            if beam > 0 and not loo:
                # baseline hypothesis = prefix beam search + collapse_fn (policy_grad.py:6-8), row 0 of the token buffers
                tokens = torch.zeros(P, B, T, dtype=torch.int32, device=dev)
                tok_len = torch.empty(P, B, dtype=torch.int32, device=dev)
                hipops.ctc_beam_search(lp, in_len, beam=beam, blank=blank, collapse=True, out=(tokens[0], tok_len[0]))
                hipops.ctc_collapse(samples, in_len, blank=blank, out=(tokens[1:], tok_len[1:]))
            else:
                tokens, tok_len = hipops.ctc_collapse(paths, in_len, blank=blank)     # (P,B,T), (P,B)
            if Lh is not None:
                hyp_len = tok_len[P - K:]                     # the K samples' rows (row 0 may be the baseline hypothesis)
                hyp_nll, hyp_lattice = hipops.ctc_hyp_lattice(lp, tokens[P - K:], hyp_len, in_len, Lh, blank=blank)
                PGCTCLossFn.last_sequence_scored = scored = hyp_len <= Lh
            n_words = prefix = None
            if sp is not None:
                # reward over the spelled text: R = -ED / C(y) or -WED / W(y); the CTC term's utt_scale stays on the unit counts
                dist, n_words, PGCTCLossFn.last_spell_truncated = _spelled_distances(targets, tg_len, tokens, tok_len, P, sp,
                                                                                     opt.reward_unit)
            elif wd is not None:
                # word-level reward: R = -WED / W(y), the CTC term's utt_scale stays on the character counts
                dist, n_words = _word_distances(targets, tg_len, tokens, tok_len, P, wd)
            else:
                dist = hipops.edit_distance(targets.repeat(P, 1), tg_len.repeat(P), tokens.view(P * B, T), tok_len.view(P * B),
                                            want_prefix=opt.per_step)
                if opt.per_step:
                    dist, prefix = dist
            if single and wd is None and sp is None:
                R_b, R_s, coef, utt_scale = hipops.pg_rewards(dist, tg_len, opt.lam, inv_gb)
            else:
                R_b, R_s, coef, utt_scale = hipops.pg_rewards_multi(dist, tg_len, K, opt.lam, inv_gb, baseline=opt.baseline,
                                                                    reward_lengths=n_words)
                if single:
                    R_s, coef = R_s[0], coef[0]
                elif steps and K == 1:
                    R_s = R_s[0]
            if steps:
                coef = hipops.pg_step_coefs_multi(paths, in_len, prefix, tok_len.view(P * B), tg_len, K, opt.lam, inv_gb,
                                                  baseline=opt.baseline, blank=blank)
            elif opt.per_step:
                coef = hipops.pg_step_coefs(paths, in_len, prefix, tok_len.view(2 * B), tg_len, opt.lam, inv_gb, blank=blank)
        nll, lattice = hipops.ctc_lattice(lp, targets, in_len, tg_len, blank=blank)
        main.wait_stream(side)
        for t_ in ((samples, R_b, R_s, coef, utt_scale) + ((tok_len, hyp_nll, scored) if Lh is not None else ())
                   + ((ent_mean, ent_scale) if beta > 0 else ()) + ((kl_mean, kl_scale, ref_log_probs) if gamma > 0 else ())
                   + ((PGCTCLossFn.last_spell_truncated,) if sp is not None else ())):
            streams.hold(t_, main)
        ent = {"ent_scale": ent_scale} if beta > 0 else {}        # weight 0: the calls as they were
        if gamma > 0:
            ent.update(ref_log_probs=ref_log_probs, kl_scale=kl_scale)
        if single_pass:
            grad = hipops.ctc_grad_from_lattice(lp, in_len, tg_len, lattice, utt_scale=utt_scale, pg_coef=coef, pg_path=sample, **ent)
            terms = hipops.pg_loss_value(lp, sample, in_len, nll, utt_scale, coef)
        elif single:
            grad = hipops.ctc_grad_from_lattice_multi(lp, in_len, tg_len, lattice, utt_scale, coef[None], samples, **ent)
            terms = hipops.pg_loss_value_multi(lp, samples, in_len, nll, utt_scale, coef[None])
        elif Lh is None:
            grad = hipops.ctc_grad_from_lattice_multi(lp, in_len, tg_len, lattice, utt_scale, coef, samples, **ent)
            terms = hipops.pg_loss_value_multi(lp, samples, in_len, nll, utt_scale, coef)
        else:
            grad = hipops.ctc_grad_from_lattices_seq(lp, in_len, tg_len, lattice, hyp_lattice, utt_scale, coef, samples, hyp_len, **ent)
            terms = hipops.pg_loss_value_seq(lp, samples, in_len, nll, utt_scale, coef, hyp_nll, hyp_len, Lh)
        if beta > 0:
            terms = torch.sub(terms, ent_mean, alpha=beta * inv_gb)      # - beta / Bg * (mean frame entropy), on the device
        if gamma > 0:
            terms = torch.add(terms, kl_mean, alpha=gamma * inv_gb)      # + gamma / Bg * (mean frame KL), on the device
        loss = terms.sum()
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(nll, R_s, R_b)
        ctx.set_materialize_grads(False)        # no zero-filled gradients for the three statistics
        return loss, nll, R_s, R_b

    @staticmethod
    def backward(ctx, g, *unused):
        (grad,) = ctx.saved_tensors
        if PGCTCLossFn.unit_seed_ptr is not None and g.data_ptr() == PGCTCLossFn.unit_seed_ptr and g.numel() == 1:
            PGCTCLossFn.unit_hits += 1
        else:
            grad = grad * g
        return (grad,) + (None,) * (len(ctx.needs_input_grad) - 1)      # the logits' gradient; no other input has one


REWARD_UNITS = ("char", "word")


def _word_distances(targets, tg_len, tokens, tok_len, P, delimiter):
    """Word edit distances of the P x B (target, collapsed path) pairs and the targets' word counts (B,), both int32."""
    B, T = tokens.shape[1], tokens.shape[2]
    dist, ref_words, _ = hipops.word_edit_distance(targets.repeat(P, 1), tg_len.repeat(P), tokens.view(P * B, T),
                                                   tok_len.view(P * B), delimiter)
    return dist, ref_words[:B]


def _spelled_distances(targets, tg_len, tokens, tok_len, P, spelling, unit):
    """Distances of the P x B (target, collapsed path) pairs over their spelled text -- characters, or words split at the spelling's
    " " --, the targets' spelled lengths or word counts (B,), and the number of rows cut at the row limit (0-d), all int32.  The
    targets are spelled once, not P times."""
    B, T = tokens.shape[1], tokens.shape[2]
    tc, tl, tf = hipops.unit_spell(targets, tg_len, spelling, want_full=True)
    hc, hl, hf = hipops.unit_spell(tokens, tok_len, spelling, want_full=True)
    truncated = ((tf > tl).sum() + (hf > hl).sum()).to(torch.int32)
    ref, ref_len, hyp, hyp_len = tc.repeat(P, 1), tl.repeat(P), hc.view(P * B, hc.shape[2]), hl.view(P * B)
    if unit == "word":
        dist, ref_words, _ = hipops.word_edit_distance(ref, ref_len, hyp, hyp_len, spelling.word_delimiter("reward_unit='word'"))
        return dist, ref_words[:B], truncated
    return hipops.edit_distance(ref, ref_len, hyp, hyp_len), tl, truncated


@dataclasses.dataclass(frozen=True)
class PGOptions:
    """Everything of a ``pg_ctc_loss`` call that is not a tensor: ONE input of ``PGCTCLossFn`` beside the tensors."""
    lam: float = 1.0
    seed: int = 0
    offset: int = 0
    global_batch: int = 1
    blank: int = 0
    beam: int = 0
    sample_base: int = -1
    per_step: bool = False
    num_samples: int = 1
    baseline: str = "hypothesis"
    reward_unit: str = "char"
    word_delimiter: object = None
    score_function: str = "path"
    max_hyp_len: object = None
    entropy_weight: float = 0.0
    kl_weight: float = 0.0
    unit_spelling: object = None
    step_objectives: bool = False


def check_options(opt, vocab=None, frames=None, symbols=None, sample_ids=None, wide_check=True, wide_objectives=False,
                  wide_sequence=False, step_objectives=False):
    """The one check of a ``PGOptions`` -- by ``pg_ctc_loss`` per call, by ``PolicyGradientTrainer`` at construction and before
    every step --, made before any kernel runs and where the caller can read the reason.  vocab, frames (T) and symbols (the
    targets' row length) are checked against where they are known.  Returns the options with their integers as ints.
    An alphabet of 65 .. 1024 symbols (hipops.MAX_VOCAB_WIDE) takes the default objective alone -- CTC + single-sample REINFORCE
    against the greedy hypothesis (``_check_wide``); wide_check=False leaves that rule to the caller (a trainer without
    ``wide_alphabet`` refuses such a model itself).  wide_objectives=True (opt-in) admits the multi-sample, leave-one-out, entropy
    and KL objectives for such an alphabet as well; at most 64 symbols it changes nothing.  wide_sequence=True (opt-in) admits
    score_function="sequence" there (A13-WIDE), alone or with what wide_objectives=True admits; at most 64 symbols it changes nothing.
    step_objectives=True (opt-in, here or in ``opt``) admits per_step with num_samples 1..16, either baseline, entropy_weight, kl_weight
    and the shard addressings (A12-STEP), and above 64 symbols per_step with K = 1, the greedy baseline and no tails -- K > 1, leave one
    out, entropy and KL there need wide_objectives=True as well; beam, score_function="sequence", reward_unit="word" and unit_spelling
    stay refused with per_step.  Without per_step it changes nothing."""
    steps = bool(step_objectives) or bool(opt.step_objectives)
    _check_score(opt.score_function, opt.max_hyp_len, opt.per_step)
    if sample_ids is not None and opt.sample_base >= 0:
        raise ValueError("sample_ids and sample_base >= 0 are two addressings of the same draws: give one")
    if opt.per_step and opt.beam > 0:
        raise ValueError("per-step rewards need the frame-aligned greedy baseline (beam = 0)")
    _check_samples(opt.num_samples, opt.baseline, opt.per_step and not steps)
    if opt.unit_spelling is not None:
        _check_spelling(opt.unit_spelling, opt.reward_unit, opt.word_delimiter, opt.per_step, vocab=vocab)
    else:
        _check_unit(opt.reward_unit, opt.word_delimiter, opt.per_step, blank=opt.blank, vocab=vocab)
    if opt.unit_spelling is None and opt.reward_unit == "word" and frames is not None and max(frames, symbols or 0) > hipops.WORD_MAX_STRIDE:
        raise ValueError(f"the word-level reward takes at most {hipops.WORD_MAX_STRIDE} frames and target symbols per utterance "
                         f"(pgasr_word_ids); got T = {frames}")
    if wide_check and vocab is not None and vocab > hipops.MAX_VOCAB_NARROW:
        try:
            _check_wide(opt, vocab, wide_objectives=bool(wide_objectives), wide_sequence=bool(wide_sequence), step_objectives=steps)
        except ValueError as e:
            if not steps:
                raise
            raise ValueError(str(e).replace(", no per-step rewards", "")) from None      # they are what the keyword opens
    return dataclasses.replace(opt, num_samples=int(opt.num_samples), step_objectives=steps,
                               max_hyp_len=None if opt.max_hyp_len is None else int(opt.max_hyp_len),
                               entropy_weight=check_entropy_weight(opt.entropy_weight), kl_weight=check_kl_weight(opt.kl_weight))


WIDE_OBJECTIVES = ("num_samples", "baseline", "entropy_weight", "kl_weight")      # what wide_objectives=True opens above 64 symbols


def _check_wide(opt, vocab, wide_objectives=False, wide_sequence=False, step_objectives=False):
    """An alphabet of more than 64 symbols: the wide kernels cover log-softmax, arg-max / sample, the CTC lattice and its gradient
    pass with one sampled path -- the default objective.  Every other option runs kernels that hold one symbol per lane.
    wide_objectives=True (opt-in): the K-draw sampler, the entropy and KL statistics and the multi-sample gradient pass have wide
    forms too (include/pgasr_hip.h, A12-WIDE), so num_samples 1..16, either baseline, entropy_weight and kl_weight are admitted in
    any combination; the beam reward search, the sequence score function, the word reward and per-step rewards stay refused.
    wide_sequence=True (opt-in): the hypothesis lattices and the gradient pass over K+1 lattices have wide forms (A13-WIDE), so
    score_function="sequence" (with max_hyp_len) is admitted -- with K = 1 against the greedy hypothesis, or with whatever
    wide_objectives=True admits beside it; the beam reward search, the word reward and per-step rewards stay refused.
    step_objectives=True (opt-in): per-step rewards are admitted (A12-STEP) -- alone with K = 1, the greedy baseline and no tails, on
    the single-path wide kernels; K > 1, leave one out, entropy and KL beside them need wide_objectives=True as well."""
    if vocab > hipops.MAX_VOCAB_WIDE:
        raise ValueError(f"alphabet of {vocab} symbols > {hipops.MAX_VOCAB_WIDE}: the wide kernels hold at most 16 symbols per lane")
    entropy, kl = check_entropy_weight(opt.entropy_weight), check_kl_weight(opt.kl_weight)
    for name, given, ok in (("baseline", opt.baseline, opt.baseline == "hypothesis"),
                            ("num_samples", opt.num_samples, int(opt.num_samples) == 1),
                            ("beam", opt.beam, opt.beam == 0),
                            ("score_function", opt.score_function, opt.score_function == "path"),
                            ("entropy_weight", opt.entropy_weight, entropy == 0.0),
                            ("kl_weight", opt.kl_weight, kl == 0.0),
                            ("reward_unit", opt.reward_unit, opt.reward_unit == "char" or opt.unit_spelling is not None),
                            ("per_step", opt.per_step, not opt.per_step or step_objectives)):
        if ok or (wide_objectives and name in WIDE_OBJECTIVES) or (wide_sequence and name == "score_function"):
            continue
        if step_objectives and opt.per_step and name in WIDE_OBJECTIVES:
            raise ValueError(f"{name}={given!r} with per-step rewards takes an alphabet of at most {hipops.MAX_VOCAB_NARROW} symbols (got "
                             f"{vocab}): above the 64-symbol limit step_objectives=True alone opens per_step with num_samples=1, "
                             f"baseline='hypothesis', entropy_weight=0 and kl_weight=0; num_samples 1..{hipops.MAX_SAMPLES}, "
                             f"baseline='leave_one_out', entropy_weight and kl_weight need wide_objectives=True as well")
        if wide_sequence:
            rest = (f"wide_objectives=True opens num_samples 1..{hipops.MAX_SAMPLES}, baseline='leave_one_out', entropy_weight and "
                    f"kl_weight" if wide_objectives else
                    "num_samples > 1, baseline='leave_one_out', entropy_weight and kl_weight need wide_objectives=True as well")
            raise ValueError(f"{name}={given!r} takes an alphabet of at most {hipops.MAX_VOCAB_NARROW} symbols (got {vocab}): above the "
                             f"64-symbol limit wide_sequence=True opens score_function='sequence' (with max_hyp_len); {rest}; "
                             f"nothing else -- beam=0, reward_unit='char', no per-step rewards")
        if wide_objectives:
            raise ValueError(f"{name}={given!r} takes an alphabet of at most {hipops.MAX_VOCAB_NARROW} symbols (got {vocab}): above the "
                             f"64-symbol limit wide_objectives=True opens num_samples 1..{hipops.MAX_SAMPLES}, "
                             f"baseline='leave_one_out', entropy_weight and kl_weight, and nothing else -- beam=0, "
                             f"score_function='path', reward_unit='char', no per-step rewards")
        if not ok:
            raise ValueError(f"{name}={given!r} takes an alphabet of at most {hipops.MAX_VOCAB_NARROW} symbols (got {vocab}): above the "
                             f"64-symbol limit only the default objective runs -- num_samples=1, baseline='hypothesis', beam=0, "
                             f"score_function='path', entropy_weight=0, kl_weight=0, reward_unit='char', no per-step rewards")


def check_entropy_weight(entropy_weight):
    """The weight of the entropy bonus, in loss units per nat per frame: a finite real number >= 0 -> float."""
    if isinstance(entropy_weight, bool) or not isinstance(entropy_weight, numbers.Real):
        raise ValueError(f"entropy_weight must be a real number >= 0 (got {entropy_weight!r})")
    v = float(entropy_weight)
    if not (v >= 0.0 and v != float("inf")):        # negative, NaN, inf
        raise ValueError(f"entropy_weight must be finite and >= 0: it weighs the mean frame entropy, in loss units per nat per frame "
                         f"(got {entropy_weight!r})")
    return v


def check_kl_weight(kl_weight):
    """The weight of the KL penalty towards the reference policy, in loss units per nat per frame: a finite real number >= 0 -> float."""
    if isinstance(kl_weight, bool) or not isinstance(kl_weight, numbers.Real):
        raise ValueError(f"kl_weight must be a real number >= 0 (got {kl_weight!r})")
    v = float(kl_weight)
    if not (v >= 0.0 and v != float("inf")):        # negative, NaN, inf
        raise ValueError(f"kl_weight must be finite and >= 0: it weighs the mean frame KL from the reference policy, in loss units per "
                         f"nat per frame (got {kl_weight!r})")
    return v


def _check_reference(ref_log_probs, logits):
    """The reference log-probs of a kl_weight > 0 call, checked before any kernel runs."""
    if ref_log_probs is None:
        raise ValueError("kl_weight > 0 needs ref_log_probs, the frozen reference policy's log-probs for this batch")
    if not isinstance(ref_log_probs, torch.Tensor) or ref_log_probs.dtype != torch.float32:
        raise ValueError(f"ref_log_probs must be an fp32 tensor (got {getattr(ref_log_probs, 'dtype', type(ref_log_probs))})")
    if ref_log_probs.shape != logits.shape:
        raise ValueError(f"ref_log_probs must have the logits' shape {tuple(logits.shape)} (got {tuple(ref_log_probs.shape)})")
    if ref_log_probs.device != logits.device:
        raise ValueError(f"ref_log_probs must be on the logits' device {logits.device} (got {ref_log_probs.device})")
    if not ref_log_probs.is_contiguous():
        raise ValueError("ref_log_probs must be contiguous")
    if ref_log_probs.requires_grad:
        raise ValueError("ref_log_probs must be detached: the reference policy is frozen and the term has no gradient towards it")


def _check_unit(reward_unit, word_delimiter, per_step=False, blank=None, vocab=None):
    if reward_unit not in REWARD_UNITS:
        raise ValueError(f"reward_unit must be one of {REWARD_UNITS} (got {reward_unit!r})")
    if reward_unit != "word":
        return
    if word_delimiter is None:
        raise ValueError("reward_unit='word' needs word_delimiter, the token id of the alphabet's ' ' symbol")
    if isinstance(word_delimiter, bool) or int(word_delimiter) != word_delimiter or word_delimiter < 0:
        raise ValueError(f"word_delimiter must be a token id >= 0 (got {word_delimiter!r})")
    if blank is not None and word_delimiter == blank:
        raise ValueError(f"word_delimiter {word_delimiter} is the CTC blank: a collapsed path never holds it")
    if vocab is not None and word_delimiter >= vocab:
        raise ValueError(f"word_delimiter {word_delimiter} is outside the alphabet of {vocab} symbols")
    if per_step:
        raise ValueError("per-step rewards are character-level: reward_mode='per_step' does not take reward_unit='word'")


def _check_spelling(unit_spelling, reward_unit, word_delimiter, per_step=False, vocab=None):
    """A reward over the spelled text of subword units (``units.UnitSpelling``): "char" counts its characters, "word" its words."""
    if reward_unit not in REWARD_UNITS:
        raise ValueError(f"reward_unit must be one of {REWARD_UNITS} (got {reward_unit!r})")
    if not all(hasattr(unit_spelling, a) for a in ("offsets", "chars", "max_unit_chars", "delimiter", "to")):
        raise ValueError(f"unit_spelling must be a units.UnitSpelling (got {type(unit_spelling).__name__})")
    if word_delimiter is not None:
        raise ValueError("unit_spelling brings its own word delimiter, the id of ' ' in the spelled text: give no word_delimiter")
    if per_step:
        raise ValueError("per-step rewards are counted on the frame-aligned units: per_step does not take unit_spelling")
    if vocab is not None and unit_spelling.vocab != vocab:
        raise ValueError(f"unit_spelling spells {unit_spelling.vocab} symbols (units and blank), the output layer has {vocab}")
    if unit_spelling.max_unit_chars > hipops.SPELL_MAX_UNIT_CHARS:
        raise ValueError(f"unit_spelling has a unit of {unit_spelling.max_unit_chars} characters: pgasr_unit_spell takes at most "
                         f"{hipops.SPELL_MAX_UNIT_CHARS}")
    if reward_unit == "word":
        unit_spelling.word_delimiter("reward_unit='word'")


def _check_score(score_function, max_hyp_len, per_step=False):
    if score_function not in hipops.SCORE_FUNCTIONS:
        raise ValueError(f"score_function must be one of {hipops.SCORE_FUNCTIONS} (got {score_function!r})")
    if max_hyp_len is not None:
        if isinstance(max_hyp_len, bool) or not isinstance(max_hyp_len, numbers.Integral) or max_hyp_len < 0:
            raise ValueError(f"max_hyp_len must be None or an integer >= 0 (got {max_hyp_len!r})")
        if score_function != "sequence":
            raise ValueError("max_hyp_len caps the hypotheses that score_function='sequence' scores: it has no meaning with 'path'")
    if score_function == "sequence" and per_step:
        raise ValueError("per-step rewards have frame-aligned coefficients, which have no sequence form: score_function='sequence' "
                         "does not take reward_mode='per_step'")


def _check_samples(num_samples, baseline, per_step=False):
    if baseline not in hipops.BASELINES:
        raise ValueError(f"baseline must be one of {sorted(hipops.BASELINES)} (got {baseline!r})")
    if isinstance(num_samples, bool) or int(num_samples) != num_samples:
        raise ValueError(f"num_samples must be an integer (got {num_samples!r})")
    if not 1 <= num_samples <= hipops.MAX_SAMPLES:
        raise ValueError(f"num_samples {num_samples} outside 1 .. {hipops.MAX_SAMPLES}: the multi-sample kernels take at most "
                         f"{hipops.MAX_SAMPLES} paths per utterance")
    if baseline == "leave_one_out" and num_samples < 2:
        raise ValueError("the leave-one-out baseline needs num_samples >= 2 (the other samples' rewards)")
    if per_step and num_samples > 1:
        raise ValueError("per-step rewards take one sampled path (num_samples = 1)")


def pg_ctc_loss(logits, in_len, targets, tg_len, lam=1.0, seed=0, offset=0, global_batch=None, blank=0, beam=0, sample_base=-1,
                per_step=False, log_probs=None, num_samples=1, baseline="hypothesis", reward_unit="char", word_delimiter=None,
                sample_ids=None, score_function="path", max_hyp_len=None, entropy_weight=0.0, kl_weight=0.0, ref_log_probs=None,
                wide_objectives=False, wide_sequence=False, unit_spelling=None, step_objectives=False):
    """beam > 0: the baseline reward comes from the prefix-beam-search hypothesis of that width (see PGCTCLossFn).
    num_samples / baseline: multi-sample REINFORCE (see PGCTCLossFn); with num_samples > 1 the third returned tensor is R_s (K,B).
    reward_unit: "char" (default) or "word" -- the word-level reward R = -WED / W(y) with words split at the token
    ``word_delimiter`` (see PGCTCLossFn); not with per_step.
    sample_base >= 0 (data parallel): index of this shard's first utterance in the global batch; the sampled paths are
    then those of the single-process global batch with the same seed.
    sample_ids (B) int32 on the device, instead of sample_base >= 0: the index of EVERY row in the global batch (``global_batch`` is
    the stride) -- for shards or micro-batches that are not contiguous slices of it; an id < 0 marks a row beyond the global batch
    (a padded, empty utterance).
    score_function: "path" (default) or "sequence" -- score every sample by the CTC likelihood of its collapsed hypothesis instead of
    its frame path (see PGCTCLossFn); max_hyp_len caps the hypotheses so scored (None: min(T, 1023)), longer ones keep the path term.
    entropy_weight: beta >= 0, the weight of the entropy bonus on the frame policy -- the loss gains -beta / Bg times every utterance's
    MEAN frame entropy, so beta is in loss units per nat per frame and does not grow with T (see PGCTCLossFn); 0 (default): off, the
    call as it was.  With every other option.
    kl_weight: gamma >= 0, the weight of the KL penalty towards a frozen reference policy whose log-probs for this batch are
    ref_log_probs (T,B,V) fp32, contiguous, detached, on the logits' device -- the loss gains gamma / Bg times every utterance's MEAN
    frame KL(p || q), so gamma is in loss units per nat per frame (see PGCTCLossFn).  With gamma > 0 the tensor is required; 0
    (default): off, the tensor is ignored and the call is as it was, so a schedule may anneal gamma to 0.  With every other option.
    wide_objectives: opt-in for an alphabet of 65 .. 1024 symbols -- num_samples 1..16, either baseline, entropy_weight and kl_weight
    then run there too, on the wide kernels of A12-WIDE (``_check_wide``); beam, score_function="sequence", reward_unit="word" and
    per_step (without step_objectives) stay refused.  False (default) and at most 64 symbols: every call as it was.
    wide_sequence: opt-in for an alphabet of 65 .. 1024 symbols -- score_function="sequence" then runs there, on the wide kernels of
    A13-WIDE: K = 1 against the greedy hypothesis, or together with whatever wide_objectives=True admits.  Set max_hyp_len for unit
    models: the hypothesis lattices take 2 * K*B*T * roundup64(2*Lh+1) * 4 bytes (2.1 GB at K = 4, B = 32, T = 1000 with the
    default cap).  beam, reward_unit="word" and per_step (without step_objectives) stay refused.  False (default) and at most 64
    symbols: every call as it was.
    unit_spelling: None (default: every call as it was) or the ``units.UnitSpelling`` of a subword alphabet -- the rewards are then
    counted on the spelled TEXT of targets and hypotheses (``pgasr_unit_spell`` on the side stream, between collapse and the distance):
    reward_unit="char" is R = -ED(chars) / max(C(y),1), "word" is R = -WED / W(y) with words split at the spelling's " " (no
    word_delimiter); utt_scale stays on the unit counts.  With every option the alphabet's size admits except per_step; above 64
    symbols it is what admits reward_unit="word".  Spelled rows are cut at 4094 characters; ``PGCTCLossFn.last_spell_truncated`` counts
    the rows cut (0-d int32 on the device, None after a call without a spelling).
    step_objectives: opt-in for per_step beyond one sampled path -- num_samples 1..16, either baseline, entropy_weight, kl_weight,
    sample_ids / sample_base / global_batch, and alphabets of 65 .. 1024 symbols (K = 1, the greedy baseline and no tails there; the
    rest with wide_objectives=True as well): per-FRAME coefficients from the rewards-to-go of all K paths (see PGCTCLossFn, A12-STEP).
    beam, score_function="sequence", reward_unit="word" and unit_spelling stay refused with per_step.  False (default), or without
    per_step: every call, refusal and bit as it was.
    log_probs: log_softmax(logits) if the caller already has it (the head kernel's by-product, ``logits.log_probs`` of
    Seq2Seq.logits -- picked up from that attribute when not given)."""
    T, B, V = logits.shape
    opt = check_options(PGOptions(lam=float(lam), seed=int(seed), offset=int(offset), global_batch=int(global_batch or B),
                                  blank=int(blank), beam=int(beam), sample_base=int(sample_base), per_step=bool(per_step),
                                  num_samples=num_samples, baseline=baseline, reward_unit=reward_unit, word_delimiter=word_delimiter,
                                  score_function=score_function, max_hyp_len=max_hyp_len, entropy_weight=entropy_weight,
                                  kl_weight=kl_weight, unit_spelling=unit_spelling, step_objectives=bool(step_objectives)),
                        vocab=V, frames=T, symbols=targets.shape[1] if targets.dim() == 2 else 0, sample_ids=sample_ids,
                        wide_objectives=wide_objectives, wide_sequence=wide_sequence)
    if log_probs is None:
        # the by-product is valid only for the tensor as the head kernel wrote it: any in-place edit since bumps _version
        log_probs = getattr(logits, "log_probs", None)
        if log_probs is not None and getattr(logits, "log_probs_version", None) != logits._version:
            log_probs = None
    if opt.kl_weight > 0:
        _check_reference(ref_log_probs, logits)
        return PGCTCLossFn.apply(logits, in_len, targets, tg_len, log_probs, sample_ids, opt, ref_log_probs)
    return PGCTCLossFn.apply(logits, in_len, targets, tg_len, log_probs, sample_ids, opt)


class CTCLoss(nn.Module):
    """CTC-only objective ('mean' reduction: per-utterance nll / max(L,1), mean over the batch)."""

    def __init__(self, blank=0):
        super().__init__()
        self.blank = blank

    def forward(self, logits, in_len, targets, tg_len, global_batch=None):
        loss, _, _, _ = pg_ctc_loss(logits, in_len, targets, tg_len, lam=0.0, global_batch=global_batch,
                                    blank=self.blank)
        return loss
