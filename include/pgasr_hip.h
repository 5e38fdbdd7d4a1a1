/*
 * pgasr_hip.h -- C ABI of libpgasr_hip.so, the MI355X (gfx950) implementation of the
 * acoustic-model policy-gradient training hot path of ana-kuznetsova/Policy-Gradient-ASR.
 *
 * The reference is pure Python on torch.nn (no FFI of its own), so each
 * entry point below names the reference call site whose arithmetic it replaces; the Python
 * host layer (the policy_gradient_asr_amd package) binds these with ctypes and keeps the reference's
 * module-level names and signatures on top.
 *
 * Conventions (all entry points):
 *   - return value: PGASR_OK (0) or a pgasr_status code; no exceptions cross the ABI;
 *   - every pointer is a DEVICE pointer owned by the caller unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work (no sync, no
 *     hipMalloc): workspaces are sized by the *_workspace_bytes queries and caller-allocated;
 *   - no global mutable state: re-entrant per stream;
 *   - tensors are dense, row-major, fp32 unless said otherwise; activations are TIME-MAJOR
 *     (T,B,C) so that one recurrent / CTC step touches one contiguous (B,C) slab;
 *   - blank = pad = index 0 is the reference's convention (CTCdecoder.py:41, data.py:99) and
 *     is passed explicitly as `blank`.
 */
#ifndef PGASR_HIP_H
#define PGASR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pgasr_status {
    PGASR_OK = 0,
    PGASR_ERR_INVALID_ARG = 1,   /* null pointer, negative size, shape the kernel cannot take */
    PGASR_ERR_LAUNCH = 2,        /* hipLaunch / runtime error (hipGetLastError != success) */
    PGASR_ERR_WORKSPACE = 3,     /* workspace null or too small */
    PGASR_ERR_UNSUPPORTED = 4,   /* size beyond a compiled-in limit (see each function) */
    PGASR_ERR_TIMEOUT = 5        /* a bounded in-kernel wait gave up (persistent LSTM) */
} pgasr_status;

/* 4 (round 3): pgasr_adam_step(guards, applied), pgasr_lstm_pack_weights(planes), the feed phases, and the streamed order:
 * pgasr_lstm_wgrad_slabs, pgasr_lstm_layer_bwd_streamed, pgasr_lstm_wgrads_streamed(+_workspace_bytes), pgasr_stream_gate_sum.
 * 7 (round 5): pgasr_stream_gate_report, pgasr_lstm_cell_f32, pgasr_gemm_x6w_feed_phase_f32 / _head_items; the sampler's counters for
 * utterances beyond the global batch.  Added since without a version change: the multi-sample entries (pgasr_frame_sample_multi,
 * pgasr_ctc_grad_from_lattice_multi, pgasr_pg_rewards_multi, pgasr_pg_loss_value_multi), the word-reward entries (pgasr_word_ids,
 * pgasr_pg_rewards_multi_ex), the gradient-clipping entries (pgasr_grad_norm_ws_bytes, pgasr_grad_norm_clip,
 * pgasr_adam_step_clipped), the id-addressed samplers (pgasr_frame_argmax_sample_ids, pgasr_frame_sample_multi_ids) and the
 * sequence-level score function (pgasr_ctc_hyp_workspace_bytes, pgasr_ctc_hyp_lattice, pgasr_ctc_grad_from_lattices_seq,
 * pgasr_pg_loss_value_seq) and the entropy regularisation (pgasr_frame_entropy, pgasr_ctc_grad_from_lattice_ent,
 * pgasr_ctc_grad_from_lattice_multi_ent, pgasr_ctc_grad_from_lattices_seq_ent), forced alignment (pgasr_ctc_forced_align),
 * SpecAugment masking (pgasr_spec_augment), the N-best entries (pgasr_ctc_beam_search_nbest, pgasr_nbest_rescore) and MWER training
 * over them (pgasr_mwer_weights, pgasr_ctc_grad_from_lattices_nbest), and the KL penalty towards a frozen reference policy
 * (pgasr_frame_kl, pgasr_ctc_grad_from_lattice_kl, pgasr_ctc_grad_from_lattice_multi_kl, pgasr_ctc_grad_from_lattices_seq_kl),
 * sample-rate conversion / speed perturbation (pgasr_resample), and minimum-Bayes-risk decoding over N-best lists
 * (pgasr_nbest_pair_dist, pgasr_mbr_select), and waveform augmentation (pgasr_reverb_limits, pgasr_reverb, pgasr_wave_power,
 * pgasr_wave_mix), and edit-operation alignment (pgasr_edit_ops_workspace_bytes, pgasr_edit_ops), and the wide-alphabet entries
 * (pgasr_log_softmax_rows_wide, pgasr_frame_argmax_sample_wide, pgasr_ctc_loss_grad_wide, pgasr_ctc_grad_from_lattice_wide), and
 * spelling rows of subword units into characters (pgasr_unit_spell), and the slot masses behind N-best confidences
 * (pgasr_edit_ops_slot_mass). */
#define PGASR_ABI_VERSION 7

int pgasr_abi_version(void);
const char* pgasr_status_string(int status);

/* ------------------------------------------------------------------------------------------
 * A5  CTC loss + gradient.  The reference has no call site; the oracle is
 * torch.nn.functional.ctc_loss composed with log_softmax.  Conventions from CTCdecoder.py:41
 * (blank=0) and data.py:99 (targets padded with 0).
 *
 *   log_probs   (T,B,V) fp32 log-softmax outputs
 *   targets     (B,Lmax) int32, first target_lengths[b] entries valid
 *   nll         (B) fp32: -log p(target_b | x_b); +inf when no alignment exists
 *   grad_logits (T,B,V) fp32: d(sum_b utt_scale[b]*nll_b)/d(logits) = utt_scale[b] *
 *               (softmax - posterior occupancy); zero for t >= input_lengths[b] and for
 *               utterances whose nll is +inf.  utt_scale may be NULL (= 1).
 *   If pg_coef and pg_path are non-NULL the REINFORCE term of pgasr_reinforce_grad is
 *   added in the same pass (A12):  + pg_coef[b] * (softmax - onehot(pg_path[t,b])).
 *   log_probs may hold -inf (a symbol of probability exactly 0 at that frame, e.g. a masked vocabulary): such a symbol has
 *   occupancy 0 and gradient entry 0 -- in this entry and in every gradient pass below -- and a target that needs it at every
 *   frame has no alignment (nll = +inf, zero gradient).  Held to the fp64 oracle by tests/test_ctc_numerics_gpu.py.
 *   Limits: 2*Lmax+1 <= 2048, V <= 64.
 * ---------------------------------------------------------------------------------------- */
size_t pgasr_ctc_workspace_bytes(int T, int B, int V, int Lmax);
int pgasr_ctc_loss_grad(const float* log_probs, const int32_t* targets,
                        const int32_t* input_lengths, const int32_t* target_lengths,
                        int T, int B, int V, int Lmax, int blank,
                        const float* utt_scale, const float* pg_coef, const int32_t* pg_path,
                        float* nll, float* grad_logits,
                        void* workspace, size_t workspace_bytes, void* stream);

/* The gradient pass of pgasr_ctc_loss_grad on its own, over the lattice that an earlier
 * pgasr_ctc_loss_grad(..., grad_logits = NULL, ...) call with the same T, B, V, Lmax left in `workspace`
 * (so the lattice can run on another stream beside the kernels that produce pg_coef).
 * pg_coef_per_frame != 0: pg_coef is (T,B), one coefficient per frame (pgasr_pg_step_coefs), instead of (B,). */
int pgasr_ctc_grad_from_lattice(const float* log_probs, const int32_t* input_lengths,
                                const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                const float* utt_scale, const float* pg_coef, const int32_t* pg_path,
                                int pg_coef_per_frame, float* grad_logits, void* workspace, size_t workspace_bytes,
                                void* stream);

/* Rewards and gradient coefficients (policy_grad.py:4-16 intent):
 *   dist [2B]: edit distances of the greedy paths, then of the sampled paths (pgasr_edit_distance);
 *   R = -dist / max(L,1);  pg_coef = lam * inv_global_batch * (R_sample - R_greedy);
 *   utt_scale = inv_global_batch / max(L,1).
 * pgasr_pg_loss_value: terms[b] = nll[b]*utt_scale[b] - pg_coef[b] * sum_{t<input_lengths[b]} log_probs[t,b,path[t,b]]
 *   (pg_coef and path both NULL: CTC only); the objective's value is sum_b terms[b].  Deterministic.
 *   pg_coef_per_frame != 0: pg_coef is (T,B) and the second term is sum_t pg_coef[t,b] * log_probs[t,b,path[t,b]].
 * pgasr_pg_step_coefs: per-frame coefficients from the PER-STEP rewards of policy_grad.py:10-15 (the reference computes r_t and
 *   never consumes it; this is the build's use of it, opt-in).  With yhat the collapsed path, d(i) = ED(y, yhat[:i]) and
 *   rho_j = d(j-1) - d(j) the reward of character j (reference: r_1 = rho_1 + rho_2, r_t = rho_{t+1} for t >= 2), the reward-to-go
 *   of frame t is G(t) = d(c(t)) - d(|yhat|), c(t) = characters that start in frames < t, and
 *     coef[t,b] = lam * inv_global_batch * (G_sample(t) - G_greedy(t)) / max(L_b,1)   for t < input_lengths[b], else 0
 *   (baseline = the greedy path's reward-to-go at the same frame; coef[0,b] is pgasr_pg_rewards' pg_coef[b]).
 *   paths (2,T,B) = greedy then sampled frame labels; prefix_dist (2B, prefix_stride) and token_lengths (2B) = the per-prefix
 *   distances and lengths of their collapsed forms (pgasr_edit_distance with prefix_dist, pgasr_ctc_collapse). */
int pgasr_pg_rewards(const int32_t* dist, const int32_t* target_lengths, int B, float lam,
                     float inv_global_batch, float* R_greedy, float* R_sample, float* pg_coef,
                     float* utt_scale, void* stream);
int pgasr_pg_loss_value(const float* log_probs, const int32_t* path, const int32_t* input_lengths,
                        const float* nll, const float* utt_scale, const float* pg_coef,
                        int T, int B, int V, int pg_coef_per_frame, float* terms, void* stream);
int pgasr_pg_step_coefs(const int32_t* paths, const int32_t* input_lengths, const int32_t* prefix_dist, int prefix_stride,
                        const int32_t* token_lengths, const int32_t* target_lengths, int T, int B, int blank,
                        float lam, float inv_global_batch, float* coef, void* stream);

/* ------------------------------------------------------------------------------------------
 * A12  multi-sample REINFORCE ("greedy reward, self-critical, or batch mean").  K = 1..PGASR_MAX_SAMPLES sampled
 * paths pi_k per utterance, rewards R_k = -ED(y, collapse(pi_k)) / max(L,1), and per sample a baseline b_k:
 *   PGASR_BASELINE_HYPOTHESIS:     b_k = R_hyp, the reward of one greedy or beam hypothesis;
 *   PGASR_BASELINE_LEAVE_ONE_OUT:  b_k = (S - R_k) / (K-1), S = sum_j R_j in j order, fp32 (K >= 2; needs no decode).
 *   pg_coef[k,b] = lam * inv_global_batch / K * (R_k - b_k)
 *   objective    = sum_b [ nll_b utt_scale_b - sum_k pg_coef[k,b] sum_{t<T_b} log p(pi_k[t,b]) ]
 *   d(logits)    = utt_scale_b (softmax - occupancy) + sum_k pg_coef[k,b] (softmax - onehot(pi_k[t,b])), the K terms in k order.
 * K = 1 with the hypothesis baseline is the single-sample objective above (pgasr_pg_rewards, pgasr_ctc_grad_from_lattice).
 * K < 1 or K > PGASR_MAX_SAMPLES: PGASR_ERR_INVALID_ARG.
 *
 * pgasr_frame_sample_multi: pgasr_frame_argmax_sample with K draws per frame from one softmax; draw k uses Philox word 0 of
 *   counter (t*ctr_stride+ctr_base+b, offset, 0, k) (third word 1 beyond the global batch, as there), so draw 0 is
 *   pgasr_frame_argmax_sample's sample bit for bit.  sample_paths (K,T,B) int32; greedy_path (T,B) or NULL.
 * pgasr_ctc_grad_from_lattice_multi: pgasr_ctc_grad_from_lattice's gradient pass with pg_paths (K,T,B) and pg_coef (K,B).
 * pgasr_pg_rewards_multi: dist = [hypothesis row (HYPOTHESIS only), sample 0, .., sample K-1] x B edit distances (pgasr_edit_distance);
 *   R_baseline (B) = b_k averaged over k in k order (= R_hyp for HYPOTHESIS), R_sample (K,B), pg_coef (K,B), utt_scale (B) as
 *   pgasr_pg_rewards'.
 * pgasr_pg_loss_value_multi: terms[b] = nll[b]*utt_scale[b] - sum_k pg_coef[k,b] * sum_{t<input_lengths[b]} log_probs[t,b,paths[k,t,b]];
 *   each path's sum in pgasr_pg_loss_value's fixed order, the K products added in k order.  Deterministic.
 * ---------------------------------------------------------------------------------------- */
#define PGASR_MAX_SAMPLES 16
#define PGASR_BASELINE_HYPOTHESIS 0
#define PGASR_BASELINE_LEAVE_ONE_OUT 1
int pgasr_frame_sample_multi(const float* scores, int T, int B, int V, int K,
                             uint64_t seed, uint32_t offset, int ctr_stride, int ctr_base,
                             int32_t* greedy_path, int32_t* sample_paths, void* stream);
int pgasr_ctc_grad_from_lattice_multi(const float* log_probs, const int32_t* input_lengths,
                                      const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                      const float* utt_scale, int K, const float* pg_coef, const int32_t* pg_paths,
                                      float* grad_logits, void* workspace, size_t workspace_bytes, void* stream);
int pgasr_pg_rewards_multi(const int32_t* dist, const int32_t* target_lengths, int B, int K, int baseline,
                           float lam, float inv_global_batch, float* R_baseline, float* R_sample, float* pg_coef,
                           float* utt_scale, void* stream);
int pgasr_pg_loss_value_multi(const float* log_probs, const int32_t* paths, int K, const int32_t* input_lengths,
                              const float* nll, const float* utt_scale, const float* pg_coef,
                              int T, int B, int V, float* terms, void* stream);

/* ------------------------------------------------------------------------------------------
 * A12  sequence-level REINFORCE (sampled expected risk / MWER; opt-in beside the path-level score function above).  The reward of
 * sample k depends on its HYPOTHESIS y_k = collapse(pi_k) alone, so the score function log p(pi_k | x) may be replaced by the CTC
 * likelihood of the hypothesis, log p(y_k | x) = -nll(y_k) summed over all its alignments: the same expectation, no larger variance.
 * With K sampled paths, hyp_tokens (K,B,hyp_stride) / hyp_len (K,B) exactly as pgasr_ctc_collapse leaves them, pg_coef (K,B),
 * utt_scale (B) as above and a length cap Lh:
 *     seq(k,b)  :=  hyp_len[k,b] <= Lh
 *     objective =  sum_b [ nll_b utt_scale_b
 *                          + sum_k pg_coef[k,b] * ( seq(k,b) ?  nll(y_k,b | x_b)  :  -sum_{t<T_b} log p(pi_k[t,b]) ) ]
 *     d(logits) =  utt_scale_b (softmax - occ_target)
 *                  + sum_k pg_coef[k,b] * ( seq(k,b) ? (softmax - occ_{y_k}) : (softmax - onehot(pi_k[t,b])) ),  the K terms in k order
 * occ_y = posterior occupancy of y's CTC lattice over the utterance's own T_b frames.  A hypothesis longer than the cap keeps the
 * path-level term (the choice depends on y alone: the mixture stays unbiased); a hypothesis nll of +inf contributes nothing.
 *
 * pgasr_ctc_hyp_workspace_bytes: the K*B hypothesis lattices, 2 * K*B*T * roundup64(2*Lh+1) * 4 bytes plus per-pair tables (row
 *   maxima, nll, label lists); 0 for arguments the entry points below reject.
 * pgasr_ctc_hyp_lattice: alpha / beta / label lists of the pairs (k,b) with hyp_len <= Lh, every pair over log-prob row b of the one
 *   (T,B,V) tensor and frames t < input_lengths[b]; pgasr_ctc_loss_grad's lattice numerics, run-to-run reproducible.  hyp_nll (K,B):
 *   nll(y_k,b | x_b), 0 for a skipped pair.  hyp_stride >= max(Lh, 1).
 * pgasr_ctc_grad_from_lattices_seq: the gradient above in one pass over the target lattice in `workspace` (pgasr_ctc_loss_grad with
 *   grad_logits = NULL, same T, B, V, Lmax) and the hypothesis lattices in `hyp_workspace` (same T, B, V, K, Lh).
 * pgasr_pg_loss_value_seq: terms[b] of the objective; path sums in pgasr_pg_loss_value's fixed order, the K products in k order.
 * K outside 1..PGASR_MAX_SAMPLES, Lh < 0, null pointers: PGASR_ERR_INVALID_ARG.  2*Lh+1 > 2048 or V > 64: PGASR_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------- */
size_t pgasr_ctc_hyp_workspace_bytes(int T, int B, int V, int K, int Lh);
int pgasr_ctc_hyp_lattice(const float* log_probs, const int32_t* hyp_tokens, int hyp_stride, const int32_t* hyp_len,
                          const int32_t* input_lengths, int T, int B, int V, int K, int Lh, int blank,
                          float* hyp_nll, void* hyp_workspace, size_t hyp_workspace_bytes, void* stream);
int pgasr_ctc_grad_from_lattices_seq(const float* log_probs, const int32_t* input_lengths, const int32_t* target_lengths,
                                     int T, int B, int V, int Lmax, int blank, const float* utt_scale,
                                     int K, const float* pg_coef, const int32_t* pg_paths, const int32_t* hyp_len, int Lh,
                                     float* grad_logits, void* workspace, size_t workspace_bytes,
                                     void* hyp_workspace, size_t hyp_workspace_bytes, void* stream);
int pgasr_pg_loss_value_seq(const float* log_probs, const int32_t* paths, int K, const int32_t* input_lengths,
                            const float* nll, const float* utt_scale, const float* pg_coef,
                            const float* hyp_nll, const int32_t* hyp_len, int Lh,
                            int T, int B, int V, float* terms, void* stream);

/* ------------------------------------------------------------------------------------------
 * A12  entropy regularisation of the frame policy (opt-in; the exploration side of the REINFORCE objectives above).  With
 * beta >= 0, T_b = input_lengths[b] clamped to [0, T] and H[t,b] = -sum_v p_v ln p_v in nats (p = exp(log_probs[t,b,:]), 0 ln 0 := 0):
 *     ent_mean[b]  = (1 / max(T_b,1)) sum_{t<T_b} H[t,b]            the utterance's MEAN frame entropy; 0 for an empty utterance
 *     ent_scale[b] = beta * inv_global_batch / max(T_b,1)
 *     objective   += -sum_b beta * inv_global_batch * ent_mean[b]   =  -sum_b ent_scale[b] sum_{t<T_b} H[t,b]
 *     d(logits)[t,b,v] += ent_scale[b] * p_v * (ln p_v + H[t,b])    for t < T_b, 0 beyond
 * The bonus is a mean over the utterance's own frames, so beta is in loss units per nat per frame and does not grow with T.  It
 * depends on the log-probs and lengths alone: not on targets, rewards, samples or the score function, and an utterance whose target
 * nll is +inf still gets it.
 *
 * pgasr_frame_entropy: both vectors in one launch, no host round trip (as pgasr_pg_rewards leaves utt_scale).  One workgroup per
 *   utterance; the sums over v (wave butterfly) and over t (16 strided partial sums in fp64, added in order) have a fixed order, so
 *   the result is run-to-run reproducible.  -inf entries and symbols whose p underflows add exactly 0.  beta = 0 is the monitoring
 *   call (ent_scale = 0).  V <= 64 (else PGASR_ERR_UNSUPPORTED), any T; beta < 0 or NaN, inv_global_batch <= 0, null pointers:
 *   PGASR_ERR_INVALID_ARG.
 * pgasr_ctc_grad_from_lattice_ent / _multi_ent / pgasr_ctc_grad_from_lattices_seq_ent: the three gradient passes above with the
 *   entropy term added in the same pass, after the REINFORCE terms: one wave sum per row and one fma per lane.  ent_scale (B) sits
 *   before grad_logits; every other argument is the entry's without the suffix.  ent_scale = NULL runs that entry's own kernel (the
 *   same bits); lanes >= V and symbols with p = 0 contribute exactly 0.
 * ---------------------------------------------------------------------------------------- */
int pgasr_frame_entropy(const float* log_probs, const int32_t* input_lengths, int T, int B, int V,
                        float beta, float inv_global_batch, float* ent_mean, float* ent_scale, void* stream);
int pgasr_ctc_grad_from_lattice_ent(const float* log_probs, const int32_t* input_lengths,
                                    const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                    const float* utt_scale, const float* pg_coef, const int32_t* pg_path,
                                    int pg_coef_per_frame, const float* ent_scale, float* grad_logits,
                                    void* workspace, size_t workspace_bytes, void* stream);
int pgasr_ctc_grad_from_lattice_multi_ent(const float* log_probs, const int32_t* input_lengths,
                                          const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                          const float* utt_scale, int K, const float* pg_coef, const int32_t* pg_paths,
                                          const float* ent_scale, float* grad_logits, void* workspace, size_t workspace_bytes,
                                          void* stream);
int pgasr_ctc_grad_from_lattices_seq_ent(const float* log_probs, const int32_t* input_lengths, const int32_t* target_lengths,
                                         int T, int B, int V, int Lmax, int blank, const float* utt_scale,
                                         int K, const float* pg_coef, const int32_t* pg_paths, const int32_t* hyp_len, int Lh,
                                         const float* ent_scale, float* grad_logits, void* workspace, size_t workspace_bytes,
                                         void* hyp_workspace, size_t hyp_workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A12  KL penalty towards a frozen reference policy (opt-in; the anchor of an RL fine-tune of a pretrained model).  With gamma >= 0,
 * p = exp(log_probs[t,b,:]) the trained policy, T_b = input_lengths[b] clamped to [0, T] and the reference's log-probs floored,
 * lnq_v = max(ref_log_probs[t,b,v], PGASR_KL_LOG_FLOOR) -- just under ln 2^-149, so a zero reference probability costs a large finite
 * penalty, never inf or NaN:
 *     KL[t,b]     = sum_v p_v (ln p_v - lnq_v)                      nats; a symbol with p_v = 0 adds exactly 0 (no 0 * inf)
 *     kl_mean[b]  = (1 / max(T_b,1)) sum_{t<T_b} KL[t,b]            0 for an empty utterance; NOT clamped at 0
 *     kl_scale[b] = gamma * inv_global_batch / max(T_b,1)
 *     objective  += sum_b gamma * inv_global_batch * kl_mean[b]
 *     d(logits)[t,b,v] += kl_scale[b] * p_v * (ln p_v - lnq_v - KL[t,b])     for t < T_b, 0 beyond
 * The reverse KL(p || q) of KL-regularised policy optimisation, as a mean over the utterance's own frames: gamma is in loss units per
 * nat per frame, like beta above.  It depends on the two log-prob tensors and the lengths alone; nothing is sampled.
 *
 * pgasr_frame_kl: pgasr_frame_entropy's launch with a second row load -- one workgroup per utterance, fixed summation order over v
 *   and t (fp64 carries), so two calls give equal bits; both vectors in one launch.  ref_log_probs == log_probs gives exactly 0.
 *   gamma = 0 is the monitoring call (kl_scale = 0).  gamma < 0 or NaN, inv_global_batch <= 0, T, B or V <= 0, null pointers:
 *   PGASR_ERR_INVALID_ARG; V > 64: PGASR_ERR_UNSUPPORTED; all checked before any pointer is touched.
 * pgasr_ctc_grad_from_lattice_kl / _multi_kl / pgasr_ctc_grad_from_lattices_seq_kl: the _ent entries above with ref_log_probs
 *   (T,B,V) and kl_scale (B) between ent_scale and grad_logits.  The KL term is added in the pass that writes the row, after the
 *   REINFORCE terms and after the entropy term (ent_scale may be NULL: KL alone): a second row read, a second wave sum, one fma per
 *   lane.  Both NULL runs exactly what the _ent entry runs for that ent_scale (the same bits); exactly one NULL is
 *   PGASR_ERR_INVALID_ARG; every other check is the _ent entry's.
 * ---------------------------------------------------------------------------------------- */
#define PGASR_KL_LOG_FLOOR (-104.0f)
int pgasr_frame_kl(const float* log_probs, const float* ref_log_probs, const int32_t* input_lengths, int T, int B, int V,
                   float gamma, float inv_global_batch, float* kl_mean, float* kl_scale, void* stream);
int pgasr_ctc_grad_from_lattice_kl(const float* log_probs, const int32_t* input_lengths,
                                   const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                   const float* utt_scale, const float* pg_coef, const int32_t* pg_path,
                                   int pg_coef_per_frame, const float* ent_scale, const float* ref_log_probs,
                                   const float* kl_scale, float* grad_logits,
                                   void* workspace, size_t workspace_bytes, void* stream);
int pgasr_ctc_grad_from_lattice_multi_kl(const float* log_probs, const int32_t* input_lengths,
                                         const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                         const float* utt_scale, int K, const float* pg_coef, const int32_t* pg_paths,
                                         const float* ent_scale, const float* ref_log_probs, const float* kl_scale,
                                         float* grad_logits, void* workspace, size_t workspace_bytes, void* stream);
int pgasr_ctc_grad_from_lattices_seq_kl(const float* log_probs, const int32_t* input_lengths, const int32_t* target_lengths,
                                        int T, int B, int V, int Lmax, int blank, const float* utt_scale,
                                        int K, const float* pg_coef, const int32_t* pg_paths, const int32_t* hyp_len, int Lh,
                                        const float* ent_scale, const float* ref_log_probs, const float* kl_scale,
                                        float* grad_logits, void* workspace, size_t workspace_bytes,
                                        void* hyp_workspace, size_t hyp_workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A5-VIT  CTC forced alignment (Viterbi): the best single alignment of a KNOWN label sequence, its score, and the frames each token
 * occupies (csrc/align.hip).  Max-plus in fp64 with a fixed order: the outputs are bit-identical to tests/align_ref.py.
 * log_probs (T,B,V) fp32 contiguous, natural log; tokens (B,Lmax) int32; T_b = input_lengths[b] clamped to [0,T], L_b =
 * token_lengths[b] clamped to [0,Lmax].  States s = 0 .. 2 L_b: even states are blank, state 2i+1 is token i.  label(s) is blank or
 * tok[i]; a label outside [0,V) is TREATED AS BLANK (defensive: valid labels are the caller's duty).
 *     delta_0(0) = lp[0][blank], delta_0(1) = lp[0][tok_0], -inf elsewhere
 *     delta_t(s) = max(c0, c1, c2) + (double)lp[t][label(s)],   c0 = delta_{t-1}(s), c1 = delta_{t-1}(s-1),
 *                  c2 = delta_{t-1}(s-2) only for odd s >= 3 with tok[i] != tok[i-1]
 *     backpointer: the smallest move wins a tie -- 1 only if c1 > c0, 2 only if c2 > max(c0, c1)
 *     end state:   2 L_b, unless L_b > 0 and delta(2 L_b - 1) > delta(2 L_b)
 * Outputs, row b (the value beyond the real lengths in parentheses):
 *     score (B) fp64        -delta_{T_b-1}(end); +inf when no alignment exists; T_b = 0: 0 when L_b = 0, else +inf
 *     frame_label (B,T)     label of the state occupied at each frame (-1)
 *     frame_token (B,T)     i on a frame in state 2i+1, -1 on a blank frame (-1)                                  [may be NULL]
 *     token_start/_end (B,Lmax)  first frame and one-past-last frame in state 2i+1 (-1)                          [may be NULL]
 *     token_logp (B,Lmax) fp64   sum of (double)lp[t][label(2i+1)] over the token's frames, ascending t (0)       [may be NULL]
 *   When score is +inf every per-frame and per-token value of that utterance is -1 / 0.
 * pgasr_ctc_align_workspace_bytes: the backpointers, one byte per (b,t,state) with the states rounded up to 64, plus two small
 *   tables; 0 for sizes the entry point rejects.  No GPU needed.
 * Checked before any HIP call: null required pointers, T/B/V/Lmax <= 0, blank outside [0,V): PGASR_ERR_INVALID_ARG;
 * 2*Lmax+1 > 2048: PGASR_ERR_UNSUPPORTED; workspace NULL or short: PGASR_ERR_WORKSPACE.  Any V, any T.  No host synchronisation.
 * ---------------------------------------------------------------------------------------- */
size_t pgasr_ctc_align_workspace_bytes(int T, int B, int Lmax);
int pgasr_ctc_forced_align(const float* log_probs, const int32_t* tokens, const int32_t* input_lengths,
                           const int32_t* token_lengths, int T, int B, int V, int Lmax, int blank,
                           double* score, int32_t* frame_label, int32_t* frame_token,
                           int32_t* token_start, int32_t* token_end, double* token_logp,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A11  word-level (WER) reward, opt-in: R = -WED(y, yhat) / W(y), where a word is a run of tokens between delimiters -- exactly
 * Python's str.split(" ") on the decoded string (n delimiters give n + 1 words, empty words included; an empty row is one empty
 * word) --, WED the Levenshtein distance over the two word lists and W(y) >= 1 the reference's word count.
 * pgasr_word_ids: N pairs in pgasr_edit_distance's layout (ref (N,ref_stride) with ref_len (N), hyp (N,hyp_stride) with hyp_len
 *   (N)) and the delimiter token d >= 0 ->
 *     ref_ids (N, ref_stride+1), hyp_ids (N, hyp_stride+1): per word, 1 + the index of its first occurrence in the pair's
 *       (ref words ++ hyp words) -- two words of one pair get the same id iff their tokens are equal (confirmed on the tokens);
 *       entries past the word count are not written;
 *     ref_words (N), hyp_words (N): the word counts.
 *   WED = pgasr_edit_distance(ref_ids, ref_words, ref_stride+1, hyp_ids, hyp_words, hyp_stride+1, ...).  One launch, deterministic,
 *   no workspace.  N <= 0 or d < 0: PGASR_ERR_INVALID_ARG; a stride above PGASR_WORD_MAX_STRIDE: PGASR_ERR_UNSUPPORTED (the id rows
 *   must stay within pgasr_edit_distance's 4095).
 * pgasr_pg_rewards_multi_ex: pgasr_pg_rewards_multi with R normalised by max(reward_lengths, 1) (e.g. the word counts) and utt_scale
 *   by max(target_lengths, 1) (the character counts of the CTC term).  reward_lengths == target_lengths gives
 *   pgasr_pg_rewards_multi's bits, and with K = 1 and the hypothesis baseline pgasr_pg_rewards'.
 * ---------------------------------------------------------------------------------------- */
#define PGASR_WORD_MAX_STRIDE 4094
int pgasr_word_ids(const int32_t* ref, const int32_t* ref_len, int ref_stride,
                   const int32_t* hyp, const int32_t* hyp_len, int hyp_stride, int N, int delimiter,
                   int32_t* ref_ids, int32_t* ref_words, int32_t* hyp_ids, int32_t* hyp_words, void* stream);
int pgasr_pg_rewards_multi_ex(const int32_t* dist, const int32_t* reward_lengths, const int32_t* target_lengths, int B, int K,
                              int baseline, float lam, float inv_global_batch, float* R_baseline, float* R_sample,
                              float* pg_coef, float* utt_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * A11-SPELL  spelling rows of subword units into rows of characters, opt-in: a unit of a 65 .. 1024-symbol alphabet may hold a
 * space, so a unit row has no word boundaries of its own and its unit edit distance depends on the unit inventory.  The spelled row
 * is a row over at most 64 character ids, which pgasr_word_ids, pgasr_edit_distance, pgasr_nbest_pair_dist and pgasr_edit_ops take
 * as it is: WER and CER of the text for a subword model.
 *   spell_off (V+1) int32, spell_chars int32: unit id v in [0, V) spells spell_chars[spell_off[v] .. spell_off[v+1]), at most
 *     PGASR_SPELL_MAX_UNIT_CHARS characters (the host checks the table; a longer entry is read up to the cap); id 0, the blank /
 *     pad, has an empty spelling.
 *   Row n reads tokens[n, i] for i < clamp(lengths[n], 0, stride).  A token outside [0, V) and a token with an empty spelling
 *     contribute nothing.  full_len[n] (may be NULL) = the length of the concatenated spellings, out_len[n] = min(full_len[n],
 *     out_stride), out[n, :out_len[n]] = the concatenation cut at out_stride characters (the cut may fall inside a unit), and
 *     out[n, out_len[n] : out_stride] is written as 0: the output need not be initialised.
 *   One launch, one wave per row; no workspace, no atomics, no host synchronisation; deterministic.
 *   N <= 0, stride < 0, out_stride < 0, V < 1, a missing required pointer: PGASR_ERR_INVALID_ARG; stride > 2^24:
 *   PGASR_ERR_UNSUPPORTED (full_len stays an int32).
 * ---------------------------------------------------------------------------------------- */
#define PGASR_SPELL_MAX_UNIT_CHARS 64
int pgasr_unit_spell(const int32_t* tokens, const int32_t* lengths, int stride, int N,
                     const int32_t* spell_off, const int32_t* spell_chars, int V,
                     int32_t* out, int out_stride, int32_t* out_len, int32_t* full_len /* may be NULL */, void* stream);

/* ------------------------------------------------------------------------------------------
 * A4  the CTC head as one kernel (model.py:52-55 as the build's Seq2Seq uses it): logits = x W^T + bias, log_probs = log_softmax.
 *   x (rows, K) fp32 with row stride ldx, W (V, K) row-major, bias (V) or NULL; logits / log_probs (rows, V), either may be NULL.
 *   Exact fp32 arithmetic (v_mfma_f32_32x32x2_f32) in every precision mode; one pass over x.  V <= 32, K % 64 == 0, K <= 1024.
 * ---------------------------------------------------------------------------------------- */
int pgasr_head_logsoftmax(const float* x, long long rows, int K, int ldx, const float* W, const float* bias, int V,
                          float* logits, float* log_probs, void* stream);

/* ------------------------------------------------------------------------------------------
 * A9 / A12  per-frame best label and sampled label.
 *   scores (T,B,V) fp32 logits or log-probs (softmax is shift invariant).
 *   greedy_path[t,b] = argmax_v scores[t,b,v], first max wins  (oracle: numpy argmax)
 *   sample_path[t,b] ~ softmax(scores[t,b,:]) by inverse CDF with
 *        u = (philox4x32_10(ctr=(t*ctr_stride+ctr_base+b, offset,0,0), key=(seed_lo,seed_hi)).x >> 8) * 2^-24
 *        k = min(#{v : cdf_v <= u * total}, V - 1), cdf the inclusive fp32 lane scan of e_v = exp(score_v - max).  A draw never
 *        returns a label with e_v == 0 (score -inf, or more than about 87 under the maximum): such a k moves to the nearest label
 *        above it with e > 0, or to the last label with e > 0 if there is none above; a k with e_k > 0 is returned as counted.
 *        (The scan adds each lane's prefix in its own order, so a flat stretch of the cdf is flat to an ulp only.)  The same
 *        rule holds for every draw of pgasr_frame_sample_multi and for the wide samplers (A9-WIDE, A12-WIDE).
 *   ctr_stride = 0 means B (counter t*B+b, the single-process layout); a data-parallel rank passes the GLOBAL batch as
 *   ctr_stride and its first utterance's global index as ctr_base (0 <= ctr_base < ctr_stride), so that N ranks with one
 *   seed draw what one process holding the whole batch draws.  Utterances with ctr_base + b >= ctr_stride lie BEYOND the global batch
 *   (ABI 7: the empty utterances a ragged batch is padded with) and draw from a disjoint domain, ctr = (t*B+b, offset, 1, 0).
 *   Either output may be NULL.  V <= 64.
 * ---------------------------------------------------------------------------------------- */
int pgasr_frame_argmax_sample(const float* scores, int T, int B, int V,
                              uint64_t seed, uint32_t offset, int ctr_stride, int ctr_base,
                              int32_t* greedy_path, int32_t* sample_path, void* stream);

/* The two samplers with the draws addressed by an explicit global utterance index per row instead of ctr_base + b (gradient
 * accumulation over micro-batches, shards that are not contiguous slices of the global batch).  utt_ids (B) int32 on the device.
 *   0 <= utt_ids[b] < ctr_stride: row b draws from Philox counter (t*ctr_stride + utt_ids[b], offset, 0, k);
 *   utt_ids[b] < 0 or >= ctr_stride: the row lies beyond the global batch (a padded, empty utterance) and draws from the disjoint
 *     domain (t*B + b, offset, 1, k) of the entry points above.
 * With utt_ids[b] = ctr_base + b the outputs are those of pgasr_frame_argmax_sample / pgasr_frame_sample_multi bit for bit (one kernel
 * body serves both).  Checked before any launch: utt_ids NULL or ctr_stride < 1 (there is no "0 means B" here): PGASR_ERR_INVALID_ARG;
 * K outside 1 .. PGASR_MAX_SAMPLES: PGASR_ERR_INVALID_ARG; V > 64: PGASR_ERR_UNSUPPORTED; (long long)T * ctr_stride > 2^32:
 * PGASR_ERR_UNSUPPORTED (counter word 0 is 32 bits; the entry points above truncate silently). */
int pgasr_frame_argmax_sample_ids(const float* scores, int T, int B, int V, uint64_t seed, uint32_t offset,
                                  int ctr_stride, const int32_t* utt_ids,
                                  int32_t* greedy_path, int32_t* sample_path, void* stream);
int pgasr_frame_sample_multi_ids(const float* scores, int T, int B, int V, int K, uint64_t seed, uint32_t offset,
                                 int ctr_stride, const int32_t* utt_ids,
                                 int32_t* greedy_path, int32_t* sample_paths, void* stream);

/* ------------------------------------------------------------------------------------------
 * A9  CTC collapse of frame paths: drop repeats, then drop blank, per utterance, for frames
 * t < lengths[b].  paths (P,T,B) int32 (P stacked path sets, e.g. greedy and sampled);
 * tokens (P,B,T) int32, token_lengths (P,B) int32.  Bit-exact against
 * oracle.decode_ref.collapse_path.
 * ---------------------------------------------------------------------------------------- */
/* A0  the collated batch of data.py:107-116 made ready for the kernels in one launch: fmask (B,T) fp32 1/0 -> in_len (B)
 * (model.py:52: lengths = mask.sum(1)); tmask (B,L) int64 1/0 -> tg_len (B) (data.py:101); targets (B,L) int64 -> int32. */
int pgasr_batch_prep(const float* fmask, int B, int T, const long long* tmask, const long long* targets, int L,
                     int32_t* in_len, int32_t* tg_len, int32_t* targets32, void* stream);
int pgasr_ctc_collapse(const int32_t* paths, const int32_t* lengths, int P, int T, int B,
                       int blank, int32_t* tokens, int32_t* token_lengths, void* stream);

/* ------------------------------------------------------------------------------------------
 * A10  batched Levenshtein distance (metrics.py:4-21: sub = ins = del = 1).
 *   ref (N,ref_stride) int32 with ref_len (N); hyp (N,hyp_stride) int32 with hyp_len (N);
 *   dist[n] = ED(ref_n, hyp_n).  If prefix_dist != NULL it is (N,hyp_stride+1) and receives
 *   ED(ref_n, hyp_n[:i]) for i = 0..hyp_len[n] -- the quantity policy_grad.py:11-15
 *   differences to form r_t.  Limit: sequence lengths <= 4095.
 * ---------------------------------------------------------------------------------------- */
int pgasr_edit_distance(const int32_t* ref, const int32_t* ref_len, int ref_stride,
                        const int32_t* hyp, const int32_t* hyp_len, int hyp_stride,
                        int N, int32_t* dist, int32_t* prefix_dist, void* stream);

/* ------------------------------------------------------------------------------------------
 * A10-OPS  edit-operation alignment (csrc/editops.hip): WHICH edits make up the distance of A10 -- hits, substitutions, deletions
 * and insertions per pair, the operation string, and a confusion matrix.  Inputs as for pgasr_edit_distance: int32 rows of
 * arbitrary int32 symbols (word-id rows of pgasr_word_ids included), lengths clamped to [0, stride].
 *   The alignment is contractual, because almost every pair has several optimal ones and S / D / I differ between them.  With
 *   D[i][j] the Levenshtein matrix over reference prefix i and hypothesis prefix j, walk back from (n, m); at (i, j) take
 *     the diagonal   if i, j > 0 and D[i-1][j-1] + (ref[i-1] != hyp[j-1]) == D[i][j],
 *     else deletion  if i > 0 and D[i-1][j] + 1 == D[i][j]      (a reference symbol with no partner),
 *     else insertion                                            (a hypothesis symbol with no partner).
 *   The result does not depend on which sequence the kernel lays across its lanes.
 *   counts (N,4) int32, required: hits, substitutions, deletions, insertions.  H + S + D = n, H + S + I = m, S + D + I = the distance.
 *   ops (N, ref_stride + hyp_stride) int8 or NULL (counts only): the operations left to right, 0 = hit, 1 = substitution,
 *     2 = deletion, 3 = insertion; every entry from n_ops[n] on is written as -1, so the buffer may be uninitialised.
 *   n_ops (N) int32: the length of the string (H + S + D + I); required with ops, else optional.
 *   confusion: NULL, or an int64 matrix (vocab+1) x (vocab+1), 1 <= vocab <= 64, that the kernel ADDS into: [r][h] every hit and
 *     substitution, [r][vocab] deletions of r, [vocab][h] insertions of h.  An operation that involves a symbol outside
 *     [0, vocab) is counted in counts and left out of the matrix.  Integer adds: the sums do not depend on their order.
 *   workspace: pgasr_edit_ops_workspace_bytes(ref_stride, hyp_stride, N) bytes, 4-byte aligned: the 2-bit choice of every DP
 *     cell, min(stride) rows of 64 * J cells, J = ceil((max(stride) + 1) / 64) rounded up to a power of two, a quarter byte each
 *     (3 KB per pair at 100 x 100, 4 MB at 4095 x 4095).
 *     The query is host-only and needs no GPU; it returns 0 for sizes the kernel refuses.
 *   Checked before any HIP call, in this order: null ref_len / hyp_len / counts, N <= 0, a negative stride, a null row pointer
 *   with a positive stride, ops without n_ops, confusion with vocab < 1 -> PGASR_ERR_INVALID_ARG; the longer stride above 4095,
 *   confusion with vocab > 64 -> PGASR_ERR_UNSUPPORTED; a workspace that is NULL or too small -> PGASR_ERR_WORKSPACE.
 *   One launch, one wave per pair, no host synchronisation.
 * ---------------------------------------------------------------------------------------- */
size_t pgasr_edit_ops_workspace_bytes(int ref_stride, int hyp_stride, int N);
int pgasr_edit_ops(const int32_t* ref, const int32_t* ref_len, int ref_stride,
                   const int32_t* hyp, const int32_t* hyp_len, int hyp_stride, int N,
                   int32_t* counts, int8_t* ops, int32_t* n_ops, long long* confusion, int vocab,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A10-CONF  slot masses of operation strings (csrc/confidence.hip): the reduction behind N-best confidences (Wessel et al.,
 * IEEE Trans. SAP 9(3), 2001).  Align every hypothesis of a list to the chosen one with pgasr_edit_ops; the confidence of a
 * position of the chosen row is the posterior mass of the hypotheses whose alignment has a hit there.  Because the alignment
 * is the contractual one of A10-OPS, the result is a pure function of operation strings and weights.
 *   ops (groups * per_group, ops_stride) int8, n_ops (groups * per_group) int32: what pgasr_edit_ops writes (0 hit, 1 substitution,
 *     2 deletion, 3 insertion, left to right; entries from n_ops on are not read).  Pair p = g * per_group + n belongs to group g.
 *     A byte outside 0 .. 3 in front of n_ops is skipped.
 *   side = 0: slots are reference positions; operations 0, 1, 2 consume a slot, 2 is the side's own gap operation, 3 the "other"
 *     one.  side = 1: slots are hypothesis positions; 0, 1, 3 consume a slot, 3 is the own gap operation, 2 the other one.
 *     The slot of a slot-consuming operation is the number of slot-consuming operations in front of it; the gap of an "other"
 *     operation is the number of slot-consuming operations in front of it, 0 .. the slot count.
 *   weight (groups * per_group) fp64.  A pair takes part iff its weight is finite and > 0 and 0 <= n_ops <= ops_stride.
 *   n_slots[g]: the slot count of the group's first participating pair (the pivot's length), -1 if none takes part.  A
 *     participating pair whose slot count differs from n_slots[g] or exceeds `slots` is left out and counted in left_out[g].
 *   mass (groups, 4, slots + 1) fp64, every word written (nothing needs initialising):
 *     [g][0][i] = sum over the participating pairs n that are not left out, ascending, of w_n where the operation on slot i is a hit,
 *     [g][1][i] the same for substitutions, [g][2][i] for the own gap operation;
 *     [g][3][j] = sum over those n, ascending, of w_n * (double)k_n(j), k_n(j) the number of "other" operations of pair n in gap j:
 *       one product and one addition per pair and gap, and only where k_n(j) > 0;
 *     every cell at or behind n_slots[g] is exactly 0, except [g][3][n_slots[g]], the last gap.
 *   fp64, every product and sum rounded once, in the stated order; no floating-point atomics.  One launch, one workgroup per
 *   group, (slots + 1) * 36 bytes of LDS; no workspace, no host synchronisation.
 *   Checked before any HIP call: a null n_ops / weight / mass / n_slots / left_out, ops null with ops_stride > 0, groups or
 *   per_group < 1, ops_stride or slots < 0, side outside {0, 1} -> PGASR_ERR_INVALID_ARG; ops_stride > 8190, slots > 4095,
 *   per_group > 128, groups * per_group >= 2^31 -> PGASR_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------- */
int pgasr_edit_ops_slot_mass(const int8_t* ops, const int32_t* n_ops, int ops_stride,
                             const double* weight, int groups, int per_group, int side, int slots,
                             double* mass, int32_t* n_slots, int32_t* left_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * A12  REINFORCE gradient on the logits:
 *   grad[t,b,v] (+)= coef[b] * (softmax(scores[t,b,:])[v] - (v == path[t,b])),  t < lengths[b]
 *   and 0 (or unchanged when accumulate != 0) for t >= lengths[b].
 * ---------------------------------------------------------------------------------------- */
int pgasr_reinforce_grad(const float* scores, const int32_t* path, const float* coef,
                         const int32_t* lengths, int T, int B, int V, int accumulate,
                         float* grad, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense contractions (A1-A4 and their gradients).  fp32 in, fp32 accumulate on the matrix cores
 * (v_mfma_f32_32x32x2_f32, bit-equal to an fmaf chain).
 *
 *   C[b] (M x N, ldc) = epilogue( alpha * opA(A[b]) * opB(B[b]) )     b = 0..batch-1
 *   opA(A) = A (M x K row-major, lda) or, transA != 0, A stored K x M;  opB likewise (transB != 0:
 *   B stored N x K, i.e. torch's Linear weight layout).
 *   sum_batches != 0: the batch results are summed into the single C (partial slabs in workspace,
 *   reduced in index order); splitk > 1 splits K the same way.  workspace bytes:
 *   pgasr_gemm_workspace_bytes.  epilogue: + bias[n] + bias2[n]; act 1 = leaky_relu(slope)
 *   (model.py:50); dact_y != NULL multiplies by d leaky_relu evaluated on dact_y (same layout as C);
 *   accumulate != 0 adds to C.  norm_operand 1/2 applies (x - shift[b]) * scale[b] to A/B while
 *   the tile is loaded: the per-utterance InstanceNorm2d of model.py:37,48 fused into the affine.
 *   precision 0: exact fp32 MFMA.  precision 1: each operand element is split into bf16 hi+lo while
 *   staged and the product is hi*hi + hi*lo + lo*hi on the bf16 MFMA with fp32 accumulation
 *   (~1e-6 relative; ~5x the fp32 matrix rate).  precision 2 (ABI 5): the fp32-faithful six-product arithmetic of
 *   pgasr_gemm_x6w_f32 (three bf16 planes per operand) -- only for the weight-gradient shaped products the 256 x 256 TN
 *   kernel takes (transA, !transB, split-K or batch sums, M, N % 256 == 0, K and the K-slabs % 32 == 0), else
 *   PGASR_ERR_UNSUPPORTED.
 *   xcc_busy (NULL = plain launch; precision 1 only): device array of 8 words, e.g. the busy counters a
 *   persistent LSTM sweep keeps in its workspace (pgasr_lstm_busy_offset).  Tiles are then drawn from a
 *   global queue and a workgroup that RUNS on XCD i (HW_REG_XCC_ID) with xcc_busy[i] != 0 takes none; an
 *   unmasked second launch picks up any leftovers.  Keeps a GEMM off the XCDs of a concurrent sweep; the
 *   result is complete and identical for any placement.
 *   workspace: always >= pgasr_gemm_workspace_bytes (>= 256: tile counter + partial slabs).
 *   Leading dimensions (elements) are at least the row they stride: lda >= (transA ? M : K), ldb >= (transB ? K : N),
 *   ldc >= N, else PGASR_ERR_INVALID_ARG; batch strides may be zero or negative.  Also PGASR_ERR_INVALID_ARG, all before any
 *   launch: null A/B/C, a size, batch or splitk < 1, norm_operand outside 0..2 or without shift/scale, act outside 0..1,
 *   precision outside 0..2, dact_y together with splitk > 1 or sum_batches.  Only rows < M and columns < N of each C[b] are
 *   written; an output whose last 128-row tile would reach 4 GiB (ceil128(M) rows of ldc, or of N in a partial slab) keeps
 *   64-bit addressing in the epilogue.
 * ---------------------------------------------------------------------------------------- */
size_t pgasr_gemm_workspace_bytes(int M, int N, int batch, int splitk, int sum_batches);
int pgasr_gemm_f32(int transA, int transB, int M, int N, int K, float alpha,
                   const float* A, int lda, long long strideA,
                   const float* B, int ldb, long long strideB,
                   float* C, int ldc, long long strideC,
                   int batch, int sum_batches, int splitk,
                   const float* bias, const float* bias2, int act, float slope, int accumulate,
                   const float* dact_y, int norm_operand, const float* shift, const float* scale,
                   int precision, const unsigned* xcc_busy, void* workspace, size_t workspace_bytes, void* stream);

/* Activation x weight GEMM with the weight PRE-SPLIT into bf16 hi/lo planes (csrc/gemm_dma.hip):
 *   C[M,N] = A[M,K] * W[N,K]^T (+ bias[n]) (* (dact_y[m,n] > 0 ? 1 : slope))
 * Replaces the same torch calls as pgasr_gemm_f32 for the two big shapes of the path: the LSTM input
 * projections (model.py:39-44) and their input gradients.  Same 3-term bf16 split / fp32 accumulate as
 * pgasr_gemm_f32(precision=1); tiles are moved by LDS-DMA three stages deep.
 * pgasr_split_bf16_planes: src (rows x cols fp32, leading dim ld) -> dense planes hi, lo of
 *   (rows x cols) bf16, or (cols x rows) when transpose != 0; x = hi + lo to ~2^-17 relative.
 * pgasr_gemm_x3w_f32 needs K % 32 == 0, N % 128 == 0, lda % 4 == 0 and 16-byte aligned A / planes, else
 *   PGASR_ERR_UNSUPPORTED (use pgasr_gemm_f32), and so does ceil256(M)*ldc*4 >= 2^32 (whole 256-row tiles are addressed with
 *   32-bit offsets).  N % 256 == 0 takes the 256 x 256 tile (128 x 128 per wave, 4 waves).  dact_y (optional) has C's shape and leading dim. */
int pgasr_split_bf16_planes(const float* src, int rows, int cols, int ld, int transpose,
                            unsigned short* hi, unsigned short* lo, void* stream);
int pgasr_gemm_x3w_f32(int M, int N, int K, const float* A, int lda, const unsigned short* Whi,
                       const unsigned short* Wlo, float* C, int ldc, const float* bias,
                       const float* dact_y, float slope, void* stream);
/* The same product FEEDING a forward LSTM sweep that is already running (csrc/gemm_dma.hip, FEED kernel): the input
 * projection leaves the step's critical path.  Persistent workgroups on the XCDs the sweep leaves free draw
 * 256 x 256 tiles (256 x 128 when N % 512 != 0) in the order the sweep consumes rows (rows are (t, b) time-major; N = the two directions' column
 * halves: row tile i of direction 0 together with row tile last-i of direction 1), store C write-through and count
 * finished tiles in tiles_done[2][ceil(M/256)] (zeroed by the caller BEFORE the sweep is launched; a word is
 * complete at pgasr_gemm_x3w_feed_col_tiles(N) = the column tiles of one direction half: the consumer's fed_need).  xcc_busy = the sweep's busy counters (pgasr_lstm_busy_offset): workgroups on a busy XCD
 * take no tile, a second unmasked launch picks up any rest.  workspace >= 1024 bytes; with
 * pgasr_gemm_x3w_feed_workspace_bytes() (32 MB) the first 16 tile groups -- the ones the sweep is waiting for -- are
 * computed as four parallel K-quarters and summed in index order by the last arrival (a tile otherwise takes one CU
 * K/32 x 1.7 us).  A tile's result is ONE fp32 accumulation chain over K, except those first tiles of a feed with
 * K >= 1024 and K % 128 == 0, which are ((q0 + q1) + q2) + q3 over K-quarters accumulated from zero.  To get the same
 * bits from the sequential order of the same product, call THIS function before the (plain) sweep with xcc_busy = NULL:
 * the decomposition depends on the arguments only, never on which workgroup computes what.  (On the 256 x 128 tile
 * -- N % 512 != 0 -- every x3w product with such a K, pgasr_gemm_x3w_f32's too, is the quarter sum.)
 * Call order on the host:
 * zero tiles_done -> pgasr_lstm_layer_fwd_fed (stream S) -> pgasr_stream_gate + this call (another stream that
 * waits for the zeroing).  order 0: rows in the order a forward sweep consumes them; 1: a backward sweep's (the
 * product is then the input gradient of the layer above, feeding pgasr_lstm_layer_bwd_fed).  Needs N % 256 == 0 on top of pgasr_gemm_x3w_f32's conditions and ceil256(M)*ldc*4 < 2^31. */
/* phase 0: the whole feed in one call (queue zeroed here, two persistent launches).  phase 1 (HEAD) + phase 2 (REST) split it:
 * phase 1 zeroes the queue and computes the first head_groups tile groups -- pgasr_gemm_x3w_feed_head_items(N, K, head_groups)
 * work items, one per workgroup, no XCD mask -- and is meant for the SWEEP'S OWN stream, in front of the sweep launch, so
 * that the rows of the sweep's first steps are in memory when it starts (they are what a fed sweep otherwise waits ~50-70 us
 * for: stream gate + launch + first tiles); phase 2, on the feeding stream and ordered behind phase 1, continues the SAME
 * queue (same workspace, not zeroed again) with the persistent launches.  The decomposition -- and so the bits -- is the
 * same as phase 0's.  head_items == 0: no head for this shape (use phase 0). */
size_t pgasr_gemm_x3w_feed_workspace_bytes(void);
int pgasr_gemm_x3w_feed_col_tiles(int N);
int pgasr_gemm_x3w_feed_head_items(int N, int K, int groups);
int pgasr_gemm_x3w_feed_f32(int M, int N, int K, const float* A, int lda, const unsigned short* Whi,
                            const unsigned short* Wlo, float* C, int ldc, const float* bias,
                            const unsigned* xcc_busy, unsigned* tiles_done, int order, int phase, int head_groups,
                            void* workspace, size_t workspace_bytes, void* stream);

/* The two weight-gradient products of one BLSTM layer (model.py:39-44; torch autograd's dW_ih, dW_hh) in ONE queue-mode
 * launch of the 256 x 256 TN kernel:
 *   dwih_perm (2*4H x in_dim) = dgates^T x                   (K = T*B rows of the (t, b)-major tensors)
 *   dwhh_perm (2 x 4H x H)    = dgates[d]^T h_prev(d)        (K = (T-1)*B rows; prev = t-1 for d = 0, t+1 for d = 1; h = out)
 * bf16x3 arithmetic (as pgasr_gemm_f32 precision 1); every 256 x 256 tile is the sum of its partial products over the time
 * slabs of pgasr_lstm_wgrad_slabs(T) in the order a backward sweep completes them (direction 0: [h_j, h_j+1) from the top
 * down; direction 1: the mirror image) -- a function of the shapes only, so every mode gives the same bits.
 * slab_done != NULL: dgates belongs to a backward sweep that is STILL RUNNING (pgasr_lstm_layer_bwd_streamed on another
 * stream, launched before this call); the work items then wait for the slab_done words that cover their rows and read
 * dgates with agent-scope loads.  slab_done == NULL: dgates is complete (the sequential order, same bits).
 * xcc_busy (optional): the sweep's busy counters (workgroups on its XCDs take no item; a second unmasked launch picks up
 * any rest).  err_word (optional): set to 1 when a wait gives up after 3 s -- pass the sweep workspace's error word.
 * Needs in_dim % 256 == 0, B % 32 == 0, T >= 2 and 16-byte aligned tensors, else PGASR_ERR_UNSUPPORTED (use pgasr_gemm_f32
 * behind the sweep). */
/* planes (ABI 5): 2 = the bf16x3 arithmetic above; 3 = the fp32-faithful six-product arithmetic of pgasr_gemm_x6w_f32 (csrc/gemm_x6.hip:
 * 16-deep steps, three planes per operand), same slabs, same order, same gate. */
size_t pgasr_lstm_wgrads_workspace_bytes(int T, int in_dim);
int pgasr_lstm_wgrads_streamed(const float* dgates, const float* x, const float* out, int T, int B, int in_dim,
                               float* dwih_perm, float* dwhh_perm, const unsigned* xcc_busy,
                               const unsigned* slab_done, int* err_word, int planes,
                               void* workspace, size_t workspace_bytes, void* stream);

/* The same two roles of W_ih (input projection, input gradient: model.py:39-44) in the REFERENCE'S arithmetic -- torch fp32 -- at
 * bf16 MFMA rate (csrc/gemm_x6.hip; the host layer's "f32" precision mode): every fp32 operand as THREE bf16 planes
 * (x = hi + mid + lo to 2^-24) and every product as the SIX terms hh + hm + mh + hl + lh + mm (all terms >= 2^-24 of the product),
 * fp32 accumulate.  256 x 256 tile, 16-deep steps.
 * pgasr_split_bf16_planes3: like pgasr_split_bf16_planes with the third plane.
 * pgasr_gemm_x6w_f32: C[M,N] = A[M,K] * W[N,K]^T (+ bias[n]) (* (dact_y[m,n] > 0 ? 1 : slope)); needs K % 16 == 0, K >= 64,
 *   N % 256 == 0, lda % 4 == 0, 16-byte aligned A / planes, M*ldc*4 < 2^32 and M*lda*4 < 2^32, else PGASR_ERR_UNSUPPORTED
 *   (use pgasr_gemm_f32 precision 0).  One fp32 accumulation chain over K per tile.
 * pgasr_gemm_x6w_feed_f32: the product FEEDING a sweep that is already running -- contract, call order, tiles_done / xcc_busy /
 *   order / workspace exactly as pgasr_gemm_x3w_feed_f32 (phase 0; there is no head launch), N % 512 == 0, M*ldc*4 < 2^31;
 *   fed_need of the consumer = pgasr_gemm_x6w_feed_col_tiles(N) = N / 512.  With pgasr_gemm_x6w_feed_workspace_bytes() the first
 *   tiles of a K >= 1024 (K % 64 == 0) feed are fixed-order sums ((q0 + q1) + q2) + q3 of K-quarters computed in parallel; called
 *   with xcc_busy = NULL before a plain sweep it is the sequential order of the same product with the same bits. */
/* pgasr_pack_x6w_planes: the same three planes PACKED tile by tile in the kernel's own LDS-image order,
 *   pack[N/256][K/16][plane 3][8 KB]  (N*K*6 bytes; N = rows, K = cols of the weight as the GEMM sees it; transpose as above),
 * so that a W piece of a step is 1 KB of consecutive bytes (8 full cache lines per LDS-DMA instruction instead of 32 quarter lines of a
 * row-major plane).  Needs N % 256 == 0, K % 16 == 0.  pgasr_gemm_x6w_f32 / _feed_f32 take a pack as Whi with Wmid = Wlo = NULL. */
int pgasr_pack_x6w_planes(const float* src, int rows, int cols, int ld, int transpose, void* pack, void* stream);
int pgasr_split_bf16_planes3(const float* src, int rows, int cols, int ld, int transpose,
                             unsigned short* hi, unsigned short* mid, unsigned short* lo, void* stream);
int pgasr_gemm_x6w_f32(int M, int N, int K, const float* A, int lda, const unsigned short* Whi,
                       const unsigned short* Wmid, const unsigned short* Wlo, float* C, int ldc, const float* bias,
                       const float* dact_y, float slope, void* stream);
size_t pgasr_gemm_x6w_feed_workspace_bytes(void);
int pgasr_gemm_x6w_feed_col_tiles(int N);
int pgasr_gemm_x6w_feed_f32(int M, int N, int K, const float* A, int lda, const unsigned short* Whi,
                            const unsigned short* Wmid, const unsigned short* Wlo, float* C, int ldc, const float* bias,
                            const unsigned* xcc_busy, unsigned* tiles_done, int order,
                            void* workspace, size_t workspace_bytes, void* stream);
/* The same feed in two launches (round 5).  phase 0: as pgasr_gemm_x6w_feed_f32.  phase 1, the HEAD: the queue head is zeroed and the
 * pgasr_gemm_x6w_feed_head_items(M, N, K) K-split items at the front of the queue (the tile groups the consumer takes first) are computed
 * one per workgroup, without an XCD mask -- to be issued on the feeding stream right behind the PREVIOUS sweep, before the consuming sweep
 * has registered its XCDs (its launch, registration, the gate and the memset are then off the first rows' path).  phase 2, the rest: no
 * memset, the persistent passes continue the same queue (same workspace, same arguments).  A phased feed needs the full
 * pgasr_gemm_x6w_feed_workspace_bytes(); head_items == 0 (no split head for this shape): PGASR_ERR_UNSUPPORTED for phases 1 and 2.
 * ctrl (optional): 256 words zeroed by the CALLER for this feed -- the queue and arrival counters live there instead of the workspace's
 * first KB and no phase issues a memset, so phases 1 and 2 may be issued on two streams (the head right behind the previous sweep, the rest
 * behind the consuming sweep's registration) and draw from the one queue side by side.
 * The decomposition -- hence every bit of C -- is that of phase 0. */
int pgasr_gemm_x6w_feed_head_items(int M, int N, int K);
int pgasr_gemm_x6w_feed_phase_f32(int M, int N, int K, const float* A, int lda, const unsigned short* Whi,
                                  const unsigned short* Wmid, const unsigned short* Wlo, float* C, int ldc, const float* bias,
                                  const unsigned* xcc_busy, unsigned* tiles_done, int order, int phase, unsigned* ctrl,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* The reference's attention context (model.py:58-94, Attention.forward, AS EXECUTED -- csrc/attention.hip):
 *   ctx[q,k] = sum_i e[b,i,k] * (sum_r exp(d[q,r] e[b,i,k])) / (sum_k' exp(d[q,k] e[b,i,k'])),   b = q % B
 * dec (NQ x H) decoder states -- NQ = L * B rows in (step, utterance) order, or just B rows for one step --, enc (B x T x H) encoder
 * outputs, ctx (NQ x H).  The denominator is the reference's own: model.py:73 divides the (H,H) outer-product matrix by its row
 * sums lined up with the LAST axis (entry [r,k] by row k's sum).  Every encoder frame counts (no mask), H_dec == H_enc.  fp32,
 * exponent maxima taken out exactly.  A defined function for parity, not a hot kernel (2 H exponentials per output and frame). */
int pgasr_attention_ctx(const float* dec, const float* enc, int NQ, int B, int T, int H, float* ctx, void* stream);

/* One step of the decoder's one-layer LSTM (model.py:104,111, Decoder's nn.LSTM(128 -> hidden); gate order i, f, g, o):
 *   g = gh + xp;  c <- sigmoid(g_f) c + sigmoid(g_i) tanh(g_g);  h <- sigmoid(g_o) tanh(c);  h_out <- h (may be NULL)
 * gh (B x 4H) = h_{t-1} W_hh^T (pgasr_gemm_f32, exact mode), xp (B x 4H) = x_t W_ih^T + b_ih + b_hh, c and h (B x H) in place.
 * Forward only, like the reference's decoder. */
int pgasr_lstm_cell_f32(const float* gh, const float* xp, float* c, float* h, float* h_out, int B, int H, void* stream);

/* Column sums of X (rows x cols, leading dim ld >= cols) -> out[cols] (and out2[cols] if non-NULL): the bias gradients.
 * accumulate != 0 adds to out / out2.  Rows are summed in blocks of 512 (four interleaved chains each), the blocks in index order:
 * deterministic.  Null X / out, rows or cols < 1, ld < cols: PGASR_ERR_INVALID_ARG; workspace NULL or below
 * pgasr_colsum_workspace_bytes: PGASR_ERR_WORKSPACE; both before any launch. */
size_t pgasr_colsum_workspace_bytes(int rows, int cols);
int pgasr_colsum_f32(const float* X, int rows, int cols, int ld, float* out, float* out2, int accumulate,
                     void* workspace, size_t workspace_bytes, void* stream);

/* A1: per-utterance mean and 1/sqrt(var+eps) over all F*T values of x (B,F,T), biased variance,
 * padding included (model.py:37,48; nn.InstanceNorm2d on (B,1,F,T)). */
int pgasr_instnorm_stats(const float* x, int B, int F, int T, float eps, float* mean, float* rstd,
                         void* stream);

/* A4: row-wise log_softmax of logits (rows, V), V <= 64 (the commented head of model.py:166-167;
 * consumer contract model.py:323). */
int pgasr_log_softmax_rows(const float* logits, long long rows, int V, float* log_probs, void* stream);

/* ------------------------------------------------------------------------------------------
 * A3  bidirectional LSTM layer, H = 256 per direction (model.py:39-44), packed-sequence semantics
 * of model.py:52-55: per-utterance lengths, the reverse direction starts at each utterance's own
 * last frame, outputs are zero past the length.
 *
 * pgasr_lstm_pack_weights: torch-layout parameters of the two directions (weight_ih (4H,in),
 *   weight_hh (4H,H), bias_ih, bias_hh (4H); gate rows i|f|g|o) ->
 *     wih_perm (2*4H, in) and bias_perm (2*4H) in column order dir*4H + unit*4 + gate
 *     (bias_perm = bias_ih + bias_hh), and the two register-resident bf16 W_hh packs
 *     (pgasr_lstm_pack_bytes(which, planes) each) the sweeps load once.  planes = 2: every fp32 weight as bf16 hi + lo
 *     (products hi*hi + hi*lo + lo*hi: ~16 operand bits, the default); planes = 3: hi + mid + lo for the fp32-faithful
 *     sweeps (flags bit 1 below; the reference's nn.LSTM is fp32, model.py:39-44): six products, every term down to
 *     2^-24 of the product.
 * pgasr_lstm_layer_fwd: gates (T,B,2,H,4) holds xproj = X * wih_perm^T + bias_perm on entry and
 *   the activations (i,f,g,o) on exit; out (T,B,2H) = h; cbuf (T,B,2,H) = c.  Every row t < T, b < B is written, none
 *   beyond; past an utterance's length out and the activations are 0 and cbuf is the state as it stands there: the last
 *   frame's in the forward direction, 0 in the reverse one (tests/test_lstm_geometry_gpu.py).
 * pgasr_lstm_layer_bwd: dout (T,B,2H) -> gates overwritten in place by d(pre-activation gates), 0 past each length;
 *   the caller forms dX = dgates * wih_perm, dW_ih = dgates^T X, dW_hh = dgates^T h_prev with
 *   pgasr_gemm_f32 and maps them back with pgasr_lstm_unpack_grads.  dbias_part (optional, 16-byte aligned,
 *   ceil(B/16) x 2*4H floats): per 16-utterance group, the sum over t of dgates in gates' column order -- the bias
 *   gradient is the sum of its rows (saves a 262 MB column-sum pass over dgates at B=32,T=1000).
 * The sweeps are persistent kernels: 16 compute workgroups (+ 4 helper workgroups that stage the coming steps'
 * HBM rows in an L2-resident ring inside the workspace) per (direction, 16-utterance group) that hand
 * h_t / partial dh sums to each other through global memory every step (self-validating words; plain
 * stores when the cluster is verified to share an XCD, write-through stores otherwise).
 * flags bit 0: force the write-through protocol (testing the placement-independent path); bit 1: three-plane
 * (fp32-faithful) arithmetic -- the W_hh pack must have been made with planes = 3; bit 2: no helper
 * workgroups (the loaders read HBM themselves: slower, but two processes can then share one GPU's XCDs).
 * All workgroups of a sweep wait for each other and must be co-resident: with helpers a sweep takes 20 of an XCD's 32
 * CUs per cluster, so run ONE sweep at a time per GPU (other kernels beside it are fine: they finish on their own) or
 * set bit 2.  Every wait is bounded (3 s): a sweep that cannot make progress sets the error word and returns.
 * Limit: B <= 128.  workspace (pgasr_lstm_workspace_bytes) holds exchange buffers and an
 * error word (offset: pgasr_lstm_error_offset) that is set when a bounded wait times out.
 * ---------------------------------------------------------------------------------------- */
size_t pgasr_lstm_pack_bytes(int which, int planes);
int pgasr_lstm_pack_weights(const float* w_ih_f, const float* w_hh_f, const float* b_ih_f, const float* b_hh_f,
                            const float* w_ih_r, const float* w_hh_r, const float* b_ih_r, const float* b_hh_r,
                            int in_dim, float* wih_perm, float* bias_perm,
                            void* whh_pack_fwd, void* whh_pack_bwd, int planes, void* stream);
int pgasr_lstm_unpack_grads(const float* dwih_perm, const float* dbias_perm, const float* dwhh_perm, int in_dim,
                            float* dw_ih_f, float* dw_hh_f, float* db_ih_f, float* db_hh_f,
                            float* dw_ih_r, float* dw_hh_r, float* db_ih_r, float* db_hh_r,
                            int accumulate, void* stream);
size_t pgasr_lstm_workspace_bytes(int T, int B, int backward);
/* Byte offset of the workspace's error word: set to 1 when a bounded wait inside a sweep gives up (results invalid).
 * The word is STICKY -- no launch clears it: zero the first 16 bytes of a workspace once after allocating it. */
int pgasr_lstm_error_offset(int B, int backward, size_t* offset);
/* How a time-out reaches the caller: the launch calls themselves are asynchronous and return PGASR_OK; the sweep sets
 * the sticky word.  pgasr_lstm_status synchronises `stream`, reads the word and returns PGASR_ERR_TIMEOUT when it is
 * set (PGASR_OK otherwise); pgasr_adam_step takes the words' device addresses as guards and skips the update while
 * one is set, so invalid gradients never reach the parameters between two host-side checks. */
int pgasr_lstm_status(const void* workspace, size_t workspace_bytes, int B, int backward, void* stream);
/* out[0] = 1.0f if *word0 or *word1 (sweep error words; either may be NULL) is non-zero, else 0.0f -- the flag a data-parallel rank writes
 * into word 0 of its gradient buffer before the last all-reduce, so that every replica skips the Adam update together (one launch). */
int pgasr_error_flag(const int32_t* word0, const int32_t* word1, float* out, void* stream);
int pgasr_lstm_busy_offset(int B, int backward, size_t* offset);   /* 8 per-XCD busy counters (hint for pgasr_gemm_f32) */
/* Holds `stream` until any of words[0..count) is non-zero or timeout_us (<= 100000) has passed: put in front of
 * GEMMs that are to run BESIDE a sweep, so that the sweep's workgroups are dispatched first (a large grid
 * enqueued ahead of the sweep delays it by the whole GEMM).  A hint only: never affects results. */
int pgasr_stream_gate(const unsigned* words, int count, int timeout_us, void* stream);
/* The same for consumers that WAIT for the sweep (pgasr_lstm_wgrads_streamed): holds `stream` until the counters add up to
 * `need` = the sweep's clusters, 2 * ceil(B/16) -- all of its workgroups are then resident; workgroups that poll for the
 * sweep's publications must not take CUs the sweep still needs.  running (optional): the sweep's slab_done words -- a
 * non-zero first word also opens the gate (the sweep has published, i.e. it is under way or already OVER: a gate that
 * comes late would otherwise sit out its whole time-out on counters that have gone back to zero). */
int pgasr_stream_gate_sum(const unsigned* words, int count, int need, const unsigned* running, int timeout_us, void* stream);
/* pgasr_stream_gate_sum that also says how it left (ABI 7): report[0] = 1 opened on the busy counters, 2 opened on a publication
 * (`running`), 3 timed out; report[1] = microseconds the gate held the stream.  report may be NULL. */
int pgasr_stream_gate_report(const unsigned* words, int count, int need, const unsigned* running, int timeout_us,
                             unsigned* report, void* stream);
/* One wave on `stream` waits (at most timeout_us <= 1e6) for words[0] != 0 and then writes words[1] = 1 if it saw it, else
 * 0.  Set words[0] from ANOTHER stream after this call: words[1] tells whether the two streams really run concurrently
 * (they do not under kernel-serialising profilers / launch-blocking modes / a single hardware queue).  The fed sweeps
 * below REQUIRE that concurrency; callers probe once per stream pair and otherwise use the sequential order. */
int pgasr_stream_probe(unsigned* words, int timeout_us, void* stream);
/* out_drop (optional, with drop_p in (0,1)): the sweep also writes dropout(out) there -- nn.LSTM's inter-layer dropout
 * (model.py:42), i.e. the NEXT layer's input, with exactly pgasr_dropout(out, drop_p, drop_seed, drop_offset)'s mask;
 * out itself stays un-dropped (the backward pass needs h_t).  NULL / 0: no second output. */
int pgasr_lstm_layer_fwd(float* gates, float* out, float* cbuf, const void* whh_pack_fwd,
                         const int32_t* lengths, int T, int B, int flags,
                         float* out_drop, float drop_p, uint64_t drop_seed, uint32_t drop_offset,
                         void* workspace, size_t workspace_bytes, void* stream);
/* pgasr_lstm_layer_fwd whose gates rows are produced WHILE it runs by pgasr_gemm_x3w_feed_f32 (launched after this
 * call on another stream): fed = that call's tiles_done, fed_need = 8H/256 column tiles per direction.  The helper
 * workgroups wait for a step's row tile(s) before they stage its rows and read them with agent-scope loads.
 * PGASR_ERR_UNSUPPORTED when no XCD would be left for the GEMM (B > 32) or helpers are off (flags bit 2):
 * pgasr_lstm_fed_ok(T, B, flags) != 0 says beforehand whether this call is possible. */
int pgasr_lstm_layer_fwd_fed(float* gates, float* out, float* cbuf, const void* whh_pack_fwd,
                             const int32_t* lengths, int T, int B, int flags, const unsigned* fed, int fed_need,
                             float* out_drop, float drop_p, uint64_t drop_seed, uint32_t drop_offset,
                             void* workspace, size_t workspace_bytes, void* stream);
int pgasr_lstm_fed_ok(int T, int B, int flags);
/* Backward counterpart: dout (= the input gradient of the layer above) is produced while the sweep runs by
 * pgasr_gemm_x3w_feed_f32(order = 1); fed_need = 2H/256.  drop_p != 0: dout arrives WITHOUT the inter-layer dropout
 * mask (model.py:42) and the helper workgroups apply pgasr_dropout(drop_p, drop_seed, drop_offset)'s mask to the rows
 * they stage -- the separate dropout pass between the layers disappears. */
int pgasr_lstm_layer_bwd_fed(float* gates, const float* out, const float* cbuf, const float* dout,
                             const void* whh_pack_bwd, const int32_t* lengths, int T, int B, int flags,
                             float* dbias_part, const unsigned* fed, int fed_need, float drop_p, uint64_t drop_seed,
                             uint32_t drop_offset, void* workspace, size_t workspace_bytes, void* stream);
int pgasr_lstm_layer_bwd(float* gates, const float* out, const float* cbuf, const float* dout,
                         const void* whh_pack_bwd, const int32_t* lengths, int T, int B, int flags,
                         float* dbias_part, void* workspace, size_t workspace_bytes, void* stream);
/* STREAMED backward sweep (round 3): the sweep publishes its progress so that the SAME layer's weight-gradient products
 * (pgasr_lstm_wgrads_streamed, on another stream, launched after this call) consume its d(pre-activation) rows while it
 * runs, instead of waiting for its end.  The products are sums over n = pgasr_lstm_wgrad_slabs(T, edges, max) TIME slabs
 * 0 = h_0 < h_1 < .. < h_n = T (sizes 16, 24, 32, 40, 48, 64, 80, 104, 128, 128 .. frames: small where a sweep ends); sweep step s is
 * frame T-1-s for direction 0 and frame s for direction 1, so for both directions the sweep steps < T - h_(n-k) complete
 * the first k slabs of the direction's order.  slab_done[c], c = 2 * (16-utterance group) + direction (2 * ceil(B/16)
 * words, zeroed by the caller BEFORE this launch), counts those publications k = 1..n: the rows are then in memory and
 * readable with agent-scope loads from any XCD.  The rows leave the storer waves as ordinary stores; one extra
 * ("flusher") workgroup per cluster waits until every member's stores of a slab are acknowledged, writes the XCD's L2
 * back (agent-scope release) and then publishes the count -- nothing on the sweep's dependent chain (measured: 1.4 us
 * of sweep time per publication).  fed == NULL: dout is complete (as pgasr_lstm_layer_bwd); else as
 * pgasr_lstm_layer_bwd_fed.  Conditions as for the fed sweeps (pgasr_lstm_fed_ok), else PGASR_ERR_UNSUPPORTED. */
int pgasr_lstm_wgrad_slabs(int T, int* edges, int max_edges);
int pgasr_lstm_layer_bwd_streamed(float* gates, const float* out, const float* cbuf, const float* dout,
                                  const void* whh_pack_bwd, const int32_t* lengths, int T, int B, int flags,
                                  float* dbias_part, const unsigned* fed, int fed_need, float drop_p, uint64_t drop_seed,
                                  uint32_t drop_offset, unsigned* slab_done,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A7  CTC prefix beam search (CTCdecoder.py:41-116), one workgroup per utterance.
 *   log_probs: natural-log probabilities, element (t,b,v) at log_probs[t*stride_t + b*stride_b + v],
 *              fp32 (is_f64 = 0: fp64 score carries, fp32 exp/log on differences, ~1e-7 relative) or
 *              fp64 (is_f64 != 0: exact fp64 math; the drop-in CTCDecoder.decode passes
 *              numpy's log of its probability matrix, like CTCdecoder.py:55);
 *   lengths (B) frames per utterance (NULL = T); beam <= 128, V <= 64, beam*V LDS-limited.
 *   out_tokens (B,T) best prefix, out_len (B), out_score (B) = -logsumexp(p_blank, p_nonblank)
 *   of that prefix (CTCdecoder.py:115-116).  Candidate order, prefix merging and the stable
 *   descending sort (ties -> first insertion) follow the reference exactly (held on inputs whose exact ties decide the
 *   output, for every kernel behind A7, A7-LM and A7-NBEST: tests/test_beam_ties_gpu.py); scores are fp64.
 *   flags bit 0: out_tokens / out_len are given AFTER collapse_fn (adjacent duplicate symbols removed,
 *   CTCdecoder.py:119-131) -- the string policy_grad.py:8 and model.py:326 score; bit 1: never take the
 *   single-wave kernel.  fp32 input with beam <= 16, V <= 64 (8 symbols per lane up to 32, 16 beyond) and T * beam <= 24576 (the reward hypothesis inside
 *   the train step) runs as ONE WAVE per utterance with the prefix trie in LDS (no workspace traffic); the scores
 *   of the two fp32 kernels agree to ~1e-7 relative, their hypotheses wherever no two candidates are closer than that.
 * ---------------------------------------------------------------------------------------- */
size_t pgasr_beam_workspace_bytes(int T, int B, int V, int beam);
int pgasr_ctc_beam_search(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                          const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                          int32_t* out_tokens, int32_t* out_len, double* out_score,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A7-LM  The same search fused with a character n-gram language model (Hannun/Maas, arXiv:1408.2873; the place the reference
 * marks at its extension step, CTCdecoder.py:90-96).  Arguments of pgasr_ctc_beam_search, the same workspace function, plus:
 *   lm_table: dense fp32 device table of natural-log probabilities of shape (V,)*lm_order, C order:
 *             lm_table[c_1, .., c_{n-1}, s] = ln p(s | c_1 .. c_{n-1}), c_{n-1} the most recent symbol.  blank never occurs inside a
 *             prefix and serves as the start pad: the context of a prefix shorter than n-1 is left-padded with blank.  The column
 *             s == blank is never read.  Every entry that can be read must be finite (the caller's duty; the Python layer checks it).
 *   lm_order: n >= 1;  V^n <= 2^25 entries (128 MiB: order 5 at V = 29, order 4 at V = 64), beyond that PGASR_ERR_UNSUPPORTED --
 *             a table is never truncated.
 *   lm_alpha, lm_beta: every term that enters a prefix by an extension with a non-blank s gets
 *             w = lm_alpha * (double)lm_table[ctx(prefix), s] + lm_beta  added -- (p_b + p) + w, (p_nb + p) + w -- also where the
 *             extension merges into a prefix already in the beam.  The blank update and the repeat branch that keeps the prefix
 *             (CTCdecoder.py:103-106) are unchanged; there is no end-of-sentence term.  Candidate order, first-touch ties and the
 *             stable descending sort are those of pgasr_ctc_beam_search; the ranking key logsumexp(p_b, p_nb) includes the bonuses.
 *   out_score = -logsumexp(p_blank, p_nonblank) of the best entry: with a language model a FUSED score, not a negative log-likelihood.
 *   lm_table == NULL and lm_order == 0: exactly pgasr_ctc_beam_search (the same kernels, the single-wave dispatch included).
 *   With a table every call without flags bit 4 takes the workgroup-per-utterance kernel; the LM arithmetic is
 *   fp64 for fp32 and fp64 log_probs alike; lm_alpha = lm_beta = 0 gives the no-LM result of that kernel bit for bit.
 *   flags bit 4 (value 16, "single-wave LM"), here and on pgasr_ctc_beam_search_nbest: with a table, the call takes the single-wave
 *             kernel's LM instantiations (the same algebra on that kernel's lane layout: the table words of a frame are gathered at
 *             its top, 8 or 16 consecutive words per lane, and parked in LDS for the winners) when ALL of these hold: a table is
 *             given, fp32 log_probs, beam <= 16, V <= 64, T * beam <= 24576, T <= 4096 -- pgasr_beam_lm_single_wave_ok says so
 *             beforehand.  The bit is an explicit choice and is not overridden by bit 1.  Scores agree with the workgroup kernel's to
 *             ~1e-7 relative (both carry fp64 sums with fp32 exp/log on differences), hypotheses wherever no two candidates are
 *             closer than that; lm_alpha = lm_beta = 0 gives the no-LM result of the single-wave kernel bit for bit.  Without a
 *             table or outside those limits the bit changes nothing, and without the bit every call is what it was, bit for bit --
 *             bit 3 of pgasr_ctc_beam_search_nbest with a table included, which stays on the workgroup kernel.  Every refusal is
 *             the same with the bit.
 *   Checked before any HIP call: lm_order < 0, lm_order > 0 with a NULL table, a table with lm_order == 0, non-finite weights
 *   -> PGASR_ERR_INVALID_ARG; the size cap -> PGASR_ERR_UNSUPPORTED.
 * pgasr_beam_lm_single_wave_ok: 1 where flags bit 4 takes the single-wave kernel for (T, V, beam, is_f64, lm_order) -- lm_order > 0 with
 *   V^lm_order <= 2^25, is_f64 == 0 and the four limits above --, else 0.  Host only: no HIP call.
 * ---------------------------------------------------------------------------------------- */
int pgasr_beam_lm_single_wave_ok(int T, int V, int beam, int is_f64, int lm_order);
int pgasr_ctc_beam_search_lm(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                             const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                             int32_t* out_tokens, int32_t* out_len, double* out_score,
                             void* workspace, size_t workspace_bytes, void* stream,
                             const float* lm_table, int lm_order, double lm_alpha, double lm_beta);

/* ------------------------------------------------------------------------------------------
 * A7-NBEST  The same search returning the first `nbest` entries of its final beam instead of the best one: the reference's
 * sorted(...)[:nbest] of the last frame (CTCdecoder.py:110-113) -- score descending, first touch among equals; the kernel's own sort,
 * no second one.  One exception to "first touch", which a list exposes beyond rank 0: with blank != 0 an entry's unchanged ("stay")
 * candidate and its own repeat extension can carry the same first-touch time, and where their scores are EXACTLY equal -- in
 * practice two entries of probability zero -- the kernel may rank the stay first where the reference ranks the extension first.
 * Arguments of pgasr_ctc_beam_search_lm (a NULL table with lm_order 0: the acoustic search), plus:
 *   nbest:      rows to return, 1 <= nbest <= beam.
 *   out_tokens: (nbest, B, tok_stride) int32, tok_stride >= T; out_len, out_score: (nbest, B); out_count: (B).  This is the
 *               (K, B, stride) layout pgasr_ctc_hyp_lattice takes, so a list goes there without a copy.
 *   count[b] = min(nbest, entries of utterance b's final beam).  Row r < count[b]: the prefix of rank r in out_tokens[r, b, :len],
 *               zeros behind it, out_score[r, b] = -logsumexp(p_blank, p_nonblank) of that entry (+inf for an entry of probability
 *               zero).  Rows r >= count[b]: length 0, score +inf, tokens zero.  lengths[b] == 0: count 1, the empty prefix, score -0.0.
 *               The kernel writes every word of the four outputs: they need no initialisation.
 *   flags bit 0: collapse_fn is applied to every hypothesis separately; rows that become equal strings are NOT merged and keep
 *               their own scores.  Bit 1 is ignored: without bit 3 every call takes the workgroup-per-utterance kernel -- exact fp64
 *               math for fp64 input, fp32 exp/log on differences for fp32 input, with or without a table.  Row 0 is therefore, bit for
 *               bit, what pgasr_ctc_beam_search_lm returns from that kernel (flags bit 1 set, or a table given).
 *   flags bit 3 (value 8, "fast"): the call may take the single-wave kernel of the train step, exactly where the 1-best dispatch of
 *               pgasr_ctc_beam_search would: no table, fp32 input, beam <= 16, V <= 64, T * beam <= 24576, T <= 4096.  Row 0 is
 *               then, bit for bit, what pgasr_ctc_beam_search returns by default; the list is that kernel's final beam in its rank
 *               order, lane r of the wave walking entry r's ancestors through the trie in LDS.  Outside those conditions the bit
 *               changes nothing: the call is the call without it, launch for launch.  Every refusal below is the same with the bit.
 *   flags bit 4 (value 16, "single-wave LM"): as on pgasr_ctc_beam_search_lm -- with a table and inside the limits there the list is
 *               the final beam of the single-wave kernel's LM instantiation, and row 0 is, bit for bit, what pgasr_ctc_beam_search_lm
 *               returns with bit 4.  Bit 3 is not needed for it and, alone, keeps a call with a table on the workgroup kernel.
 *   Every ancestor walk ends after lengths[b] steps at the latest, whatever the node store holds.
 *   Checked before any HIP call, in this order: the search's argument checks, its limits and the LM's checks as in
 *   pgasr_ctc_beam_search_lm; nbest < 1, nbest > beam, tok_stride < T, a NULL output -> PGASR_ERR_INVALID_ARG; then the
 *   workspace (pgasr_beam_workspace_bytes) -> PGASR_ERR_WORKSPACE.  No host synchronisation.
 * ---------------------------------------------------------------------------------------- */
int pgasr_ctc_beam_search_nbest(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                                const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                                int nbest, int32_t* out_tokens, int tok_stride, int32_t* out_len, double* out_score,
                                int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream,
                                const float* lm_table, int lm_order, double lm_alpha, double lm_beta);

/* ------------------------------------------------------------------------------------------
 * A7-WIDE  The same search over rows of up to 1024 symbols (subword units): the reference's CTCDecoder.decode (CTCdecoder.py:41-116)
 * over all V symbols, no heuristic symbol pruning, returning the first `nbest` entries of the final beam in the layout and with the
 * conventions of pgasr_ctc_beam_search_nbest (nbest = 1: the 1-best search).  A kernel of its own (csrc/beam_wide.hip; the score
 * forms, the rank key, the trie and the result tail are the A7 workgroup kernel's, both from csrc/beam_core.h): one
 * workgroup of 256 threads per utterance, a beam x V bitmap for the merge test, the hash-consed trie with 10-bit symbols, and a
 * top-`beam` SELECTION in place of the sort of all beam * V candidates -- a threshold (the beam-th largest of 2 * beam candidates that
 * certainly exist), a list of the candidates at or above it (2048 items), a bitonic sort of that list; a frame whose list overflows
 * takes a counting selection instead (radix passes over the 64-bit score image and the touch time with an LDS histogram, keys
 * recomputed per pass, until exactly `beam` are kept).  Both rank by the same unique key (score image, touch time), so both return
 * what the sort of everything would.
 *   log_probs, strides, lengths, blank, out_tokens (nbest, B, tok_stride), out_len / out_score (nbest, B), out_count (B): as A7-NBEST.
 *               Every word of the outputs is written; rows r >= count[b]: length 0, score +inf, tokens zero; lengths[b] == 0: count 1,
 *               the empty prefix, score -0.0.  fp32 input: fp64 carries with fp32 exp/log on differences; fp64 input: exact fp64
 *               math; both in the argument order of the A7 kernels, so that for V <= 64 every output word equals
 *               pgasr_ctc_beam_search_nbest's (no table, flags bit 3 clear) bit for bit wherever no two candidates tie exactly.
 *   Tie order: score descending, then first touch in the reference's loop nest (symbol-major, rank-minor; within one (symbol, entry)
 *               iteration the extension is touched before the kept prefix).  The exception A7-NBEST documents (an entry's stay
 *               candidate against its own repeat extension at exactly equal score) does NOT apply here: the touch time carries
 *               one more bit that orders the two as the reference does.
 *   flags bit 0: collapse_fn per hypothesis, as A7-NBEST.  Bit 5 (value 32): every frame takes the counting selection (the same
 *               result bit for bit; for tests and measurements).  Any other bit: PGASR_ERR_INVALID_ARG.
 *   out_counting_frames: (B) int32 or NULL: the number of frames of each utterance that took the counting selection.
 *   Limits: 1 <= V <= 1024 (narrow rows are accepted), beam <= 128, 1 <= nbest <= beam, tok_stride >= T; node ids are 22 bits
 *               (a trie node is parent << 10 | symbol in one word): T * beam + 1 >= 2^22 -> PGASR_ERR_UNSUPPORTED.
 *   Every loop is bounded: hash probes by the table size, ancestor walks by lengths[b], radix passes by the key width (12).
 *   Checked before any HIP call, in this order: NULL log_probs / out_tokens / out_len / out_score, T, B, V, beam <= 0, blank outside
 *   [0, V) -> PGASR_ERR_INVALID_ARG; V > 1024 or beam > 128 -> PGASR_ERR_UNSUPPORTED; unknown flag bits, nbest < 1, nbest > beam,
 *   tok_stride < T, NULL out_count -> PGASR_ERR_INVALID_ARG; the workspace (pgasr_beam_wide_workspace_bytes; 0 for T, B or
 *   beam <= 0) -> PGASR_ERR_WORKSPACE; the node-id width -> PGASR_ERR_UNSUPPORTED.  No host synchronisation.
 * ---------------------------------------------------------------------------------------- */
size_t pgasr_beam_wide_workspace_bytes(int T, int B, int V, int beam);
int pgasr_ctc_beam_search_wide(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                               const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                               int nbest, int32_t* out_tokens, int tok_stride, int32_t* out_len, double* out_score,
                               int32_t* out_count, int32_t* out_counting_frames,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A7-WIDE-LM  A back-off n-gram language model over the acoustic units themselves (order 1 .. 5, V <= 1024 symbols, sparse): fusion
 * inside the A7-WIDE search, and the model's score of every hypothesis of an N-best list (csrc/beam_wide.hip, csrc/unit_lm.hip,
 * csrc/unit_lm.h; the host model, its packing and its own statement of the query: lm.UnitNgramLM).
 * The model.  blank never occurs inside a prefix: it is the start-of-sentence symbol, exactly one of it (ARPA's <s>).  The context of
 *   a prefix y is the last order-1 symbols of (blank,) + y, shorter near the start.  Stored k-grams are (c_1 .. c_{k-1}, s), s != blank,
 *   blank only as c_1; each has logp and, below the top order, bow (natural log, fp32).  Every one of the V-1 unigrams is stored, and
 *   the context of every stored n-gram is stored.  The query lp32(h, s), contractual on the host and on the device:
 *     acc = 0.0 (fp64); if (h, s) is stored: return (float)(acc + (double)logp[h, s]); else acc += (double)bow[h] where h is stored,
 *     drop the oldest symbol of h, and again -- sums from the longest context to the shortest, one rounding to fp32 at the end.
 * pgasr_unit_lm_tables: device pointers and sizes, a plain struct in HOST memory passed by pointer and read before the launch.
 *   A STATE is a stored context: state 0 the empty one, then every stored k-gram with k < order (the unigram of symbol c, <s> = blank
 *   included, is state 1 + c).  states (n_states) x 16 bytes {float bow, int32 back-off state, int32 first successor, int32 one past
 *   the last}; the back-off state is the longest proper suffix of the context that is a state.  A SUCCESSOR is a stored n-gram listed
 *   behind its context: succ (n_succ) x 16 bytes {int32 symbol, float logp, int32 next state, 0}, the successors of one state
 *   consecutive and ascending in the symbol; state 0 lists all V-1 unigrams.  next state = the longest suffix of context + symbol, of
 *   at most order-1 symbols, that is a state.  start = the state of the empty prefix: (blank,) from order 2 on.  Walking the back-off
 *   states instead of dropping one symbol at a time is the same query: a context that is no state has no bow and, by closure, no
 *   successor.
 * pgasr_ctc_beam_search_wide_lm: pgasr_ctc_beam_search_wide with the model fused in, A7-LM's algebra word for word: every term that
 *   enters a prefix by an extension with a non-blank s gets w = __dadd_rn(__dmul_rn(lm_alpha, (double)lp32(ctx(prefix), s)), lm_beta)
 *   added -- (p_b + p) + w, (p_nb + p) + w --, also where the extension of parent i by last(j) merges into entry j's stay candidate
 *   (with the parent's context); the blank update and the repeat branch that keeps the prefix are unchanged.  fp64 for fp32 and fp64
 *   input alike.  Candidates, touch times, both selections, the trie and the result tail are A7-WIDE's; out_score is a FUSED score.
 *   lm_alpha = lm_beta = 0 returns pgasr_ctc_beam_search_wide's words bit for bit; for V <= 64 and a model with a dense form every
 *   output word equals pgasr_ctc_beam_search_nbest's with that table (flags bits 3 and 4 clear) wherever no two candidates tie.
 *   Each beam entry owns a dense row of its state in the workspace (lp32(state, s) and the next state for every s; 2 * beam rows per
 *   utterance; a staying entry keeps its row, an extension winner's row is filled from the successor lists of its back-off chain,
 *   shortest context first), so a candidate costs one fp32 load.  Every loop is bounded: the chain by the order, a list by its length,
 *   the rest as A7-WIDE.
 *   Checked before any HIP call, in this order: A7-WIDE's checks up to and including the flags / nbest / tok_stride / out_count group;
 *   then the model -- tables, states or succ NULL -> PGASR_ERR_INVALID_ARG; order outside 1 .. 5, vocab > 1024, n_succ > 2^24, n_states >
 *   2^24 + 1 -> PGASR_ERR_UNSUPPORTED; vocab != V, blank != the call's, n_states < 1, n_succ < V - 1, start outside the states, a weight
 *   that is not finite -> PGASR_ERR_INVALID_ARG --; then the trie's part of the workspace -> PGASR_ERR_WORKSPACE, the node-id width ->
 *   PGASR_ERR_UNSUPPORTED, the whole workspace (pgasr_beam_wide_lm_workspace_bytes) -> PGASR_ERR_WORKSPACE.  No host synchronisation.
 * pgasr_nbest_unit_lm_score:
 *   tokens (N, B, tok_stride) int32, len (N, B), count (B): a list as pgasr_ctc_beam_search_nbest writes it (len is clamped to
 *   [0, tok_stride], count to [0, N]); nothing behind a hypothesis' length is read.  For n < count[b]:
 *     out_lm_logp[n, b] fp64 = sum_i (double)lp32(ctx(y_<i), y_i), one addition per token in index order; no end-of-sentence term.
 *   A symbol outside [0, V) or equal to blank gives -inf (no table word is read for it).  Rows n >= count[b]: 0.  Totals and ranks:
 *   pgasr_nbest_combine_rank with word_logp = out_lm_logp and n_words = len is A7-RESCORE's formula with the same roundings.
 *   Checked before any HIP call, in this order: N < 1, N > 128, V > 1024 -> PGASR_ERR_UNSUPPORTED; a NULL pointer, B < 1,
 *   tok_stride < 1, V < 1, blank outside [0, V) -> PGASR_ERR_INVALID_ARG; the model as above.  One launch, one thread per
 *   hypothesis, no workspace, no host synchronisation.
 * ---------------------------------------------------------------------------------------- */
typedef struct pgasr_unit_lm_tables {
    const void* states;
    const void* succ;
    int32_t order, vocab, blank, n_states, n_succ, start;
} pgasr_unit_lm_tables;
size_t pgasr_beam_wide_lm_workspace_bytes(int T, int B, int V, int beam);
int pgasr_ctc_beam_search_wide_lm(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                                  const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                                  int nbest, int32_t* out_tokens, int tok_stride, int32_t* out_len, double* out_score,
                                  int32_t* out_count, int32_t* out_counting_frames,
                                  void* workspace, size_t workspace_bytes, void* stream,
                                  const pgasr_unit_lm_tables* tables, double lm_alpha, double lm_beta);
int pgasr_nbest_unit_lm_score(const int32_t* tokens, int tok_stride, const int32_t* len, const int32_t* count,
                              int N, int B, int V, int blank, const pgasr_unit_lm_tables* tables, double* out_lm_logp,
                              void* stream);

/* ------------------------------------------------------------------------------------------
 * A7-BIAS  Hotword (contextual phrase) biasing: the A7 / A7-LM / A7-NBEST search with a weighted automaton over the token rows, and the
 * automaton's score of every hypothesis of an N-best list (csrc/beam.hip BIAS = true, csrc/hotword.hip; the builder and the host
 * statement of the query: lm.HotwordBias).
 * The meaning.  For a list of phrases p (token-id rows without the blank) with weights w(p), the bias of a token row y is
 *     B(y) = sum_p (occurrences of p in y, overlapping ones included) * w(p)
 *            + partial * boost * (length of the longest suffix of y that is a PROPER prefix of some phrase);
 *   the second term is pending credit: it rewards a hypothesis for being on the way into a phrase and is taken back by the transition
 *   that leaves the phrase.
 * bias_table: S * V 8-byte little-endian words {int32 next; float32 bonus} on the device, word (q, s) at q * V + s: the Aho-Corasick
 *   machine of the phrase trie (state 0 the root, states in breadth-first order, children in symbol order; dense goto with the failure
 *   links resolved), bonus[q, s] = out(next) + pend(next) - pend(q) formed in fp64 and rounded once to fp32, so that the sum of the
 *   bonuses along y is B(y).  The blank's column is next = q, bonus = 0.  bias_states = S >= 1; S * V <= 2^24 words (128 MiB).  A next
 *   outside [0, S) read from the table is taken as state 0: no table content gives an address outside the S * V words.
 * pgasr_ctc_beam_search_bias / pgasr_ctc_beam_search_nbest_bias: the arguments of pgasr_ctc_beam_search_lm / _nbest, then the table,
 *   S and bias_weight.  A7-LM's algebra line for line.  An entry carries bst = the state of its prefix (a stay inherits it, an
 *   extension by s takes next[bst_j V + s]) and bwi = bst(parent prefix) V + last, the word of its own last emission, which is the
 *   merged term of its stay candidate (parent i extended by last(j)).  Every term that enters a prefix by an extension with a
 *   non-blank s gets w added, with these roundings, for fp32 and fp64 log_probs alike:
 *       wb = __dmul_rn(bias_weight, (double)bonus);
 *       with a language model  w = __dadd_rn(__dadd_rn(__dmul_rn(lm_alpha, (double)lm_word), lm_beta), wb);   without  w = wb;
 *       then (p_b + p) + w and (p_nb + p) + w.
 *   The blank update and the repeat branch that keeps the prefix are unchanged; candidate order, first-touch ties and the sort are
 *   A7's; out_score is a FUSED score.  bias_weight = 0 returns the words of the same kernel without a table bit for bit.
 *   With a table every call takes the workgroup-per-utterance kernel (fp64 input: exact math; fp32: fp32 exp/log on differences),
 *   and every (beam, V) that kernel accepts without a table it accepts with one.  flags bits 3 and 4 (the single-wave kernel) with a
 *   table -> PGASR_ERR_UNSUPPORTED: the call is refused, never run differently.
 *   bias_table == NULL and bias_states == 0: exactly pgasr_ctc_beam_search_lm / pgasr_ctc_beam_search_nbest, every dispatch included.
 *   Checked before any HIP call, behind the language model's checks: a NULL table with bias_states != 0, a table with bias_states < 1,
 *   bias_states * V > 2^24, a bias_weight that is not finite -> PGASR_ERR_INVALID_ARG; then the flag refusal above.
 * pgasr_nbest_bias_score: tokens (N, B, tok_stride) int32, len (N, B), count (B): a list as pgasr_ctc_beam_search_nbest or
 *   pgasr_ctc_beam_search_wide writes it (len is clamped to [0, tok_stride], count to [0, N]).  For n < count[b]:
 *     out[n, b] fp64 = sum_i (double)bonus[q_i, y_i], q_0 = 0, q_{i+1} = next[q_i, y_i], one addition per token in index order;
 *   a token outside [0, V) leaves state and sum unchanged (and so does the blank, by its column).  Rows n >= count[b]: 0.
 *   N <= 128, V <= 1024, else PGASR_ERR_UNSUPPORTED; a NULL pointer, B < 1, tok_stride < 1, V < 1, bias_states < 1, bias_states * V >
 *   2^24 -> PGASR_ERR_INVALID_ARG; all before any HIP call.  One launch, one lane per hypothesis with its tokens staged ahead of the
 *   state chain, no workspace, no host synchronisation.  Totals and ranks: pgasr_nbest_combine_rank with word_logp = out,
 *   word_alpha = bias_weight, word_beta = 0.
 * ---------------------------------------------------------------------------------------- */
int pgasr_ctc_beam_search_bias(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                               const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                               int32_t* out_tokens, int32_t* out_len, double* out_score,
                               void* workspace, size_t workspace_bytes, void* stream,
                               const float* lm_table, int lm_order, double lm_alpha, double lm_beta,
                               const void* bias_table, int bias_states, double bias_weight);
int pgasr_ctc_beam_search_nbest_bias(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                                     const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                                     int nbest, int32_t* out_tokens, int tok_stride, int32_t* out_len, double* out_score,
                                     int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream,
                                     const float* lm_table, int lm_order, double lm_alpha, double lm_beta,
                                     const void* bias_table, int bias_states, double bias_weight);
int pgasr_nbest_bias_score(const int32_t* tokens, const int32_t* len, const int32_t* count, int N, int B, int tok_stride, int V,
                           const void* bias_table, int bias_states, double* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * A7-WIDE-BIAS  Hotword biasing inside the A7-WIDE search: rows of up to 1024 symbols, with or without the unit model of A7-WIDE-LM
 * (csrc/beam_wide.hip, the WideBias argument of beam_wide_kernel).  The first pass itself is biased, so a rare phrase the acoustic
 * search would drop from the beam stays in it; a second pass (pgasr_nbest_bias_score) can only re-rank rows that are in the list.
 *   The arguments of pgasr_ctc_beam_search_wide_lm up to and including stream; then tables (NULL: no model), lm_alpha, lm_beta as
 *   there; then bias_table, bias_states, bias_weight: the automaton of A7-BIAS in its one layout -- S * V words {int32 next; float32
 *   bonus}, word (q, s) at q * V + s, what lm.HotwordBias.device_table holds and the A7-BIAS entries read.
 *   The meaning is A7-BIAS's, line for line, on A7-WIDE's candidates.  An entry carries the state of its prefix (the root, 0, for the
 *   empty prefix; a stay inherits it, an extension by s takes next[state_j V + s]) and the bonus of its own last emission,
 *   bonus[state(parent prefix), last], which is the bias part of the merged term of its stay candidate.  Every term that enters a
 *   prefix by an extension with a non-blank s gets w added, with these roundings, for fp32 and fp64 log_probs alike:
 *       wb = __dmul_rn(bias_weight, (double)bonus);
 *       with a model  w = __dadd_rn(__dadd_rn(__dmul_rn(lm_alpha, (double)lp32(ctx(prefix), s)), lm_beta), wb);   without  w = wb;
 *       then (p_b + p) + w and (p_nb + p) + w.
 *   The blank update and the repeat branch that keeps the prefix are unchanged.  Candidates, touch times, both selections, the trie
 *   and the result tail are A7-WIDE's; bonuses can be negative, so the threshold's extension candidate of an entry is the symbol of
 *   largest log-prob + w with its own w in its image, as in A7-WIDE-LM.  out_score is a FUSED score.  A next outside [0, S) read from
 *   the table is taken as state 0 and every index is formed from the clamped state: no table content gives an address outside the
 *   S * V words.  No loop is added: everything is bounded as in A7-WIDE.  For V <= 64 (and a model with a dense form) every output
 *   word equals pgasr_ctc_beam_search_nbest_bias's wherever no two candidates tie.
 *   Dispatch: tables == NULL, bias_table == NULL and bias_states == 0 is exactly pgasr_ctc_beam_search_wide; tables != NULL without a
 *   bias is exactly pgasr_ctc_beam_search_wide_lm; bias_weight = 0 with a table returns the words of the same call without a table
 *   bit for bit.
 *   Workspace: pgasr_beam_wide_workspace_bytes without a model, pgasr_beam_wide_lm_workspace_bytes with one; the bias needs none.
 *   Checked before any HIP call, in this order: A7-WIDE's checks up to and including the flags / nbest / tok_stride / out_count group;
 *   the model's checks as in A7-WIDE-LM when tables != NULL; then the bias -- a NULL table with bias_states != 0, a table with
 *   bias_states < 1, bias_states * V > 2^24, a bias_weight that is not finite -> PGASR_ERR_INVALID_ARG --; then the workspace and the
 *   node-id width as in A7-WIDE / A7-WIDE-LM.  No host synchronisation.
 * ---------------------------------------------------------------------------------------- */
int pgasr_ctc_beam_search_wide_bias(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                                    const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                                    int nbest, int32_t* out_tokens, int tok_stride, int32_t* out_len, double* out_score,
                                    int32_t* out_count, int32_t* out_counting_frames,
                                    void* workspace, size_t workspace_bytes, void* stream,
                                    const pgasr_unit_lm_tables* tables, double lm_alpha, double lm_beta,
                                    const void* bias_table, int bias_states, double bias_weight);

/* ------------------------------------------------------------------------------------------
 * A7-RESCORE Second pass over N-best lists: an n-gram LM score of every hypothesis, a weighted total and its rank.
 *   tokens (N, B, tok_stride) int32, len (N, B), count (B): a list as pgasr_ctc_beam_search_nbest writes it (len is clamped to
 *   [0, tok_stride], count to [0, N]); am (N, B) fp64: the caller's acoustic score, lower is better.
 *   lm_table / lm_order: a table as pgasr_ctc_beam_search_lm takes it, or NULL / 0 (lm_logp = 0).  For n < count[b]:
 *     lm_logp[n, b] = sum_i (double)lm_table[ctx(y_<i), y_i]   (the last lm_order-1 symbols, left-padded with blank; fp64 sum)
 *     total[n, b]   = ((am_weight * am) + -(lm_alpha * lm_logp)) + -(lm_beta * len),  every product and sum rounded once.
 *   A non-finite am, or a total that is not a number, gives total = +inf.  A symbol outside [0, V) gives lm_logp = -inf and
 *   total = +inf (no table word is read for it).  Rows n >= count[b]: lm_logp = 0, total = +inf.
 *   order (B, N) int32: order[b, :count[b]] = the stable ascending rank of total (ties keep the list's order), then the rows
 *   n >= count[b] in index order.
 *   N <= 128, V <= 64, V^lm_order <= 2^25 (else PGASR_ERR_UNSUPPORTED: a table is never truncated); NULL pointers, N < 1, B < 1,
 *   tok_stride < 1, blank outside [0, V), a table without an order or the reverse, non-finite weights: PGASR_ERR_INVALID_ARG.
 *   All checked before any HIP call.  One launch, one workgroup per utterance, no workspace, no host synchronisation.
 * ---------------------------------------------------------------------------------------- */
int pgasr_nbest_rescore(const int32_t* tokens, int tok_stride, const int32_t* len, const int32_t* count, const double* am,
                        int N, int B, int V, int blank, const float* lm_table, int lm_order,
                        double am_weight, double lm_alpha, double lm_beta,
                        double* out_lm_logp, double* out_total, int32_t* out_order, void* stream);

/* ------------------------------------------------------------------------------------------
 * A7-MBR  Minimum-Bayes-risk decoding over N-best lists (the inference-side counterpart of A13-MWER): the edit distances inside each
 * list, and the hypothesis of least expected distance under the list's renormalised posterior.
 * pgasr_nbest_pair_dist:
 *   tokens (N, B, tok_stride) int32, len (N, B), count (B): a list as pgasr_ctc_beam_search_nbest writes it (len is clamped to
 *   [0, tok_stride], count to [0, N]); nothing behind a hypothesis' length is read.  dist (B, N, N) int32; the kernel writes every
 *   word of it.  For n, m < count[b] with len[n,b] <= Lmax and len[m,b] <= Lmax:
 *     dist[b,n,m] = dist[b,m,n] = the Levenshtein distance of the two hypotheses (sub = ins = del = 1), 0 on the diagonal.
 *   Every other entry is -1: a row beyond count, a hypothesis longer than Lmax -- its row, its column and its own diagonal.
 *   A symbol outside [0, V) matches nothing, not even itself (the search never emits one): two equal rows holding one such
 *   symbol are at distance 1.
 *   Myers' bit-vector recurrence in blocks of 64 pattern positions, one lane per pair, each unordered pair once (csrc/mbr.hip).
 *   Checked before any HIP call, in this order: N < 1, N > 128, V < 1, V > 64, Lmax outside [0, 1024] -> PGASR_ERR_UNSUPPORTED;
 *   a NULL pointer, B < 1, tok_stride < 1 -> PGASR_ERR_INVALID_ARG.  One launch, no workspace, no host synchronisation.
 * pgasr_mbr_select:
 *   dist (B, N, N) int32 as above, or any caller-made matrix in that layout (word distances); score (N, B) fp64, lower is better
 *   (the exact CTC -log p, the first-pass score or a rescored total); scale: the posterior temperature, finite and >= 0.
 *     valid(n,b)      := n < count[b]  and  score[n,b] finite  and  dist[b,n,n] >= 0
 *     m_b              = min over valid n of score[n,b]
 *     w[n,b]           = exp(-(scale * (score[n,b] - m_b)))
 *     posterior[n,b]   = w[n,b] / sum_valid w, the sum in n order                      0 where not valid
 *     risk[n,b]        = sum over valid m of posterior[m,b] * dist[b,n,m], in m order  +inf where not valid
 *     best[b]          = the first valid n of least risk                               0 when no n is valid
 *   Every product and every sum is rounded once (no contraction into fused multiply-adds); scale = 0 gives the uniform posterior
 *   over the valid rows.  posterior, risk (N, B) fp64, best (B) int32.  risk[best[b], b] is the expected number of errors of the
 *   chosen hypothesis under the list's posterior.
 *   Checked before any HIP call: N < 1 or N > 128 -> PGASR_ERR_UNSUPPORTED; a NULL pointer, B < 1, a scale that is negative or
 *   not finite -> PGASR_ERR_INVALID_ARG.  One launch, one workgroup per utterance, fp64, no host synchronisation.
 * ---------------------------------------------------------------------------------------- */
int pgasr_nbest_pair_dist(const int32_t* tokens, int tok_stride, const int32_t* len, const int32_t* count,
                          int N, int B, int V, int Lmax, int32_t* dist, void* stream);
int pgasr_mbr_select(const int32_t* dist, const double* score, const int32_t* count, int N, int B, double scale,
                     double* posterior, double* risk, int32_t* best, void* stream);

/* ------------------------------------------------------------------------------------------
 * A7-WORDLM  A back-off word n-gram language model (ARPA form, order 1 .. 5) over N-best lists: the log-probability of every
 * hypothesis' word sequence, and a weighted total with its rank on top of an earlier pass' total (csrc/word_lm.hip; the host
 * model, its packing and its own statement of the query: lm.WordNgramLM).
 * The model.  A word is 1 .. 32 token ids in [0, 255], without the delimiter; word ids 0, 1, 2 are <s>, </s>, <unk> and have no
 *   spelling.  Every stored n-gram has logp and, below the top order, bow (natural log, fp32).  With h the last order-1 words
 *   (<s>-padded at the sentence start, a word outside the vocabulary replaced by <unk>):
 *     score(w | h) = logp(h, w) if that n-gram is stored, else (bow(h) if h is stored else 0) + score(w | h without its oldest word),
 *   ending at the unigram, which every vocabulary entry has.  Every fp32 is widened to fp64; one word's score starts from 0 and
 *   adds the back-off weights from the longest context to the shortest, then the found logp; a sentence's word_logp is the sum
 *   of its words' scores in word order, one addition per word, then the score of </s>.  An empty sentence scores score(</s> | <s>).
 *   The words of a hypothesis are its maximal runs of tokens other than `delimiter` (str.split(): no empty words).
 * pgasr_word_lm_tables: device pointers and sizes, a plain struct in HOST memory passed by pointer and read before the launch.
 *   word_pool (pool_bytes) bytes, word_off (n_words + 1) int32: the spelling of word i is word_pool[word_off[i] .. word_off[i+1]).
 *   word_slots (word_cap) int32: a word id or -1.  A word is looked up from slot hash_word(spelling) & (word_cap - 1) on, slot by
 *     slot, until its spelling equals a slot's word byte for byte (found) or a slot is empty (not in the vocabulary): a hash match
 *     alone never decides.  hash_word: FNV-1a over the bytes (offset 2166136261, prime 16777619), then h ^= h >> 16;
 *     h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16, in wrapping 32 bits.
 *   uni_logp, uni_bow (n_words) fp32: the unigrams at the word's id.  The entry index of a unigram is the word id.
 *   ngram_slots (ngram_cap) x 16 bytes {int32 ctx, int32 word, float logp, float bow}, ctx = -1 in an empty slot: the n-grams of
 *     all orders >= 2 in one table.  ctx is the entry index of the n-gram's context (all its words but the last); the entry index
 *     of the n-gram in slot s is n_words + s.  Looked up from slot hash_ngram(ctx, word) & (ngram_cap - 1) on until both ctx and
 *     word are equal or a slot is empty.  hash_ngram: x = ctx * 2^32 + word; x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27;
 *     x *= 0x94D049BB133111EB; x ^= x >> 31, in wrapping 64 bits.
 *   word_cap and ngram_cap are powers of two and at most half their slots are taken, so every probe ends.
 * pgasr_nbest_word_lm_score:
 *   tokens (N, B, tok_stride) int32, len (N, B), count (B): a list as pgasr_ctc_beam_search_nbest writes it (len is clamped to
 *   [0, tok_stride], count to [0, N]); nothing behind a hypothesis' length is read.  For n < count[b]:
 *     out_word_logp[n, b] fp64 = the sentence's word_logp,  out_n_words[n, b] int32 = its words (</s> not counted),
 *     out_n_oov[n, b] int32 = its words outside the vocabulary.   Rows n >= count[b]: 0, 0, 0.
 *   A word of more than 32 tokens, or with a token outside [0, 255], is outside the vocabulary without a look at the tables.  The
 *   blank is not special here: no spelling holds it (the host model refuses one), so a word with a blank in it is not found.
 *   Checked before any HIP call: tables NULL -> PGASR_ERR_INVALID_ARG; order outside 1 .. 5, N < 1, N > 128, tok_stride >
 *   PGASR_WORD_LM_MAX_STRIDE, n_words > 2^22, ngram_cap > 2^25 (2^24 n-grams) -> PGASR_ERR_UNSUPPORTED; a NULL pointer, B < 1,
 *   tok_stride < 1, n_words < 3, a capacity that is no power of two, more than word_cap / 2 spelled words, pool_bytes < 0 or above
 *   32 bytes per spelled word -> PGASR_ERR_INVALID_ARG.  One launch, one workgroup per hypothesis, no workspace, no host
 *   synchronisation.
 * pgasr_nbest_combine_rank:
 *   base, word_logp (N, B) fp64, n_words (N, B) int32, count (B).  For n < count[b]:
 *     total[n, b] = (base + -(word_alpha * word_logp)) + -(word_beta * n_words),  every product and sum rounded once.
 *   A non-finite base, or a total that is not a number, gives total = +inf; rows n >= count[b]: total = +inf.  order (B, N) int32 as
 *   pgasr_nbest_rescore ranks: the stable ascending rank of total over the first count[b] rows (ties keep the list's order), then
 *   the rows beyond count in index order.  word_alpha = word_beta = 0 returns base bit for bit where it is finite.
 *   Checked before any HIP call: N < 1 or N > 128 -> PGASR_ERR_UNSUPPORTED; a NULL pointer, B < 1, a weight that is not finite ->
 *   PGASR_ERR_INVALID_ARG.  One launch, one workgroup per utterance, no host synchronisation.
 * ---------------------------------------------------------------------------------------- */
#define PGASR_WORD_LM_MAX_STRIDE 4096
typedef struct pgasr_word_lm_tables {
    const unsigned char* word_pool;
    const int32_t* word_off;
    const int32_t* word_slots;
    const float* uni_logp;
    const float* uni_bow;
    const void* ngram_slots;
    int32_t order, n_words, word_cap, ngram_cap, pool_bytes, reserved;
} pgasr_word_lm_tables;
int pgasr_nbest_word_lm_score(const int32_t* tokens, int tok_stride, const int32_t* len, const int32_t* count,
                              int N, int B, int delimiter, const pgasr_word_lm_tables* tables,
                              double* out_word_logp, int32_t* out_n_words, int32_t* out_n_oov, void* stream);
int pgasr_nbest_combine_rank(const double* base, const double* word_logp, const int32_t* n_words, const int32_t* count,
                             int N, int B, double word_alpha, double word_beta, double* out_total, int32_t* out_order,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * A7-WORDFUSE  The word n-gram model of A7-WORDLM and its lexicon inside the first pass: the A7 / A7-NBEST search with a per-extension
 * bonus from a lexicon trie and, at every word end, from the word model (csrc/beam.hip WORDS = true; the builder and the host statement
 * of every term: lm.WordFusion).  A second pass (pgasr_nbest_word_lm_score) can only re-rank rows that survived a search that knew
 * nothing about words; here the hypothesis the word model prefers stays in the beam.
 * The meaning.  d = `delimiter`, a token other than the blank.  The lexicon is the model's vocabulary (word ids 3 and up, 1 .. 32 tokens
 *   each, no d, no blank) as a trie: state 0 the root, the nodes in breadth-first order with children in symbol order, and ONE sink for
 *   everything outside the lexicon, the LAST state (trie_states - 1).  For a prefix y: u(y) = the tokens behind its last d (the pending
 *   word, maybe empty), hist(y) = the ids of its completed words, cut as str.split() cuts them (no empty words), a word outside the
 *   lexicon being <unk>.  Every term that enters a prefix by an extension with a non-blank s gets w = bonus(y, s) added exactly where
 *   A7-LM adds its term, (p_b + p) + w and (p_nb + p) + w; the blank update and the repeat branch are unchanged.
 *     s != d:  w = (double)trie[q V + s].bonus and the state becomes trie[q V + s].next: 0.0 into a child node; oov_penalty (fp32, <= 0,
 *              may be -inf: the hard lexicon constraint) from a trie node into the sink; 0.0 inside the sink.
 *     s == d:  u empty (q = 0): w = 0.0, nothing changes.  Otherwise word = node_word[q] (the word's id at a terminal node, <unk> = 2
 *              elsewhere) and  w = __dadd_rn(__dmul_rn(alpha, score(hist, word)), beta), score the fp64 back-off query of A7-WORDLM;
 *              for a node that is neither terminal nor the sink, w = __dadd_rn(w, (double)trie[q V + d].bonus) -- that word holds
 *              oov_penalty there and 0 elsewhere; the sink was charged on the way in.  The state becomes 0, the word joins hist.
 *   Finalisation (flags2 bit 0).  After the last frame every entry of the final beam gets fin(y): 0.0, or the d-bonus of its pending
 *   word where u is not empty; with flags2 bit 1 (eos) fin = __dadd_rn(fin, __dmul_rn(alpha, score(hist', </s>))), hist' with the pending
 *   word in it.  The final beam is ranked again by lse(p_b, p_nb) + fin, descending, equal totals in the search's order, and the rows and
 *   out_score = -(lse + fin) come from that ranking.  Without bit 0 the list is the search's own and no fin is added.  The bonuses
 *   along a row y plus fin(y) with eos equal alpha * word_logp + beta * n_words + oov_penalty * n_oov of pgasr_nbest_word_lm_score.
 *   alpha = beta = oov_penalty = 0 without eos: every output word of pgasr_ctc_beam_search_nbest's workgroup kernel, bit for bit.
 * pgasr_ctc_beam_search_words: the arguments of pgasr_ctc_beam_search_nbest, all of them (a dense character table beside the word model
 *   is out of scope: lm_table must be NULL and lm_order 0, anything else -> PGASR_ERR_UNSUPPORTED), then
 *   trie: trie_states * V words {int32 next; float32 bonus}, word (q, s) at q * V + s, the layout of A7-BIAS; the columns of the blank
 *     and of d hold next = q / 0 and are read for the bonus of d only.  A next outside [0, trie_states) is taken as state 0.
 *   node_word (trie_states) int32; an id outside [0, n_words) is taken as <unk>.   tables: the model, as A7-WORDLM passes it (the
 *     unigram arrays and ngram_slots are read; the spellings are in the trie).   delimiter, alpha, beta, flags2.
 *   An entry carries its trie state, the entry indices of its last 1 .. order-1 words as contexts, own = the w of its own last emission
 *   (the merged term of its stay candidate) and dlm = the bonus d would get; the thread that writes an extension winner makes the one
 *   back-off query (at most order-1 independent probes), so the model costs O(beam) probes per frame.
 *   fp32 and fp64 log_probs, the workgroup-per-utterance kernel, N-best form (the 1-best is row 0 at nbest = 1).  Accepted (beam, V):
 *   beam <= 128, V <= 64 and a power-of-two sort of beam * V candidates within 160 KB of LDS with 72 bytes of word state per entry --
 *   beam * V <= 4096 (128 x 32, 64 x 64) is accepted, beyond that PGASR_ERR_UNSUPPORTED before any HIP call, as without a model.
 *   Checked before any HIP call, behind the checks of pgasr_ctc_beam_search_nbest (V > 64 or beam > 128 -> PGASR_ERR_UNSUPPORTED):
 *   trie, node_word, tables or one of the tables' unigram / n-gram pointers NULL, trie_states < 1, trie_states * V > 2^24, an alpha or
 *   beta that is not finite, n_words < 3, an ngram_cap that is no power of two, delimiter outside [0, V) or equal to blank, unknown
 *   flags2 bits -> PGASR_ERR_INVALID_ARG; order outside 1 .. 5, n_words > 2^22, ngram_cap > 2^25, a character table, flags bits 3 and 4 (the
 *   single-wave kernel has no word model) -> PGASR_ERR_UNSUPPORTED; then the workspace (pgasr_beam_workspace_bytes).  No host synchronisation.
 * ---------------------------------------------------------------------------------------- */
int pgasr_ctc_beam_search_words(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                                const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                                int nbest, int32_t* out_tokens, int tok_stride, int32_t* out_len, double* out_score,
                                int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream,
                                const float* lm_table, int lm_order, double lm_alpha, double lm_beta,
                                const void* trie, int trie_states, const int32_t* node_word, const pgasr_word_lm_tables* tables,
                                int delimiter, double alpha, double beta, int flags2);

/* ------------------------------------------------------------------------------------------
 * A13-MWER  Minimum word error rate training over the N-best list of the beam search (Prabhavalkar et al., arXiv:1712.01818): the
 * model's probability renormalised over the N hypotheses the decoder returns, and the expected risk under that distribution.
 * Nothing is sampled.  With a list as pgasr_ctc_beam_search_nbest writes it WITHOUT collapse (raw prefixes are distinct label
 * sequences), hyp_nll (N,B) = the exact -log p(y_n | x) of pgasr_ctc_hyp_lattice (not the first-pass beam score, which lacks the
 * pruned mass), dist (N,B) the (word) edit distances to the target and risk_len (B) the target's characters (or words):
 *     valid(n,b) := n < count[b]  and  hyp_len[n,b] <= Lh  and  hyp_nll[n,b] finite
 *     m_b        =  min over valid n of hyp_nll[n,b]
 *     p[n,b]     =  exp(-(hyp_nll[n,b] - m_b)) / sum_valid exp(-(hyp_nll - m_b))              0 where not valid
 *     r[n,b]     =  dist[n,b] / max(risk_len[b], 1)
 *     rbar[b]    =  sum_n p[n,b] r[n,b]
 *     coef[n,b]  =  -lam * inv_global_batch * p[n,b] * (r[n,b] - rbar[b])                     the factor of d nll_n / d logits
 *     utt_scale[b] = inv_global_batch / max(target_lengths[b], 1)                             as pgasr_pg_rewards leaves it
 *     terms[b]   =  nll[b] * utt_scale[b] + lam * inv_global_batch * rbar[b]                  the CTC part as pgasr_pg_loss_value forms it
 *     objective  =  sum_b terms[b]
 *     d(logits)  =  utt_scale_b (softmax - occ_target) + sum_n coef[n,b] (softmax - occ_{y_n}),  the N terms in n order
 * sum_n coef[n,b] = 0.  No valid entry: p = coef = 0, rbar = 0.
 *
 * pgasr_mwer_weights: all six outputs (fp32; p, r, coef (N,B); utt_scale, rbar, terms (B)) in one launch, one thread per utterance,
 *   fp64 arithmetic with the sums in n order: run-to-run reproducible, no host synchronisation.  N outside 1..PGASR_MAX_SAMPLES,
 *   B < 1, Lh < 0, null pointers, lam or inv_global_batch not finite, inv_global_batch <= 0: PGASR_ERR_INVALID_ARG before any HIP call.
 * pgasr_ctc_grad_from_lattices_nbest: pgasr_ctc_grad_from_lattices_seq without a path tensor (its kernel with the path branch
 *   compiled out): the gradient above in one pass over the target lattice in `workspace` and the N*B hypothesis lattices in
 *   `hyp_workspace` (pgasr_ctc_hyp_lattice with K = N, same T, B, V, Lh and the SAME hyp_len).  A pair with hyp_len > Lh has no
 *   lattice and adds nothing; give pgasr_ctc_hyp_lattice and this entry a length of 0 for every pair that is over the cap or beyond
 *   count, so that every lattice in the workspace is really computed (the empty hypothesis') and meets a coefficient of 0.
 *   Checks and limits as pgasr_ctc_grad_from_lattices_seq, before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int pgasr_mwer_weights(const int32_t* dist, const int32_t* risk_len, const int32_t* target_lengths, const float* hyp_nll,
                       const int32_t* hyp_len, const int32_t* count, const float* nll, int N, int B, int Lh,
                       float lam, float inv_global_batch, float* p, float* r, float* coef, float* utt_scale,
                       float* rbar, float* terms, void* stream);
int pgasr_ctc_grad_from_lattices_nbest(const float* log_probs, const int32_t* input_lengths, const int32_t* target_lengths,
                                       int T, int B, int V, int Lmax, int blank, const float* utt_scale,
                                       int N, const float* coef, const int32_t* hyp_len, int Lh,
                                       float* grad_logits, void* workspace, size_t workspace_bytes,
                                       void* hyp_workspace, size_t hyp_workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A0-AUG  SpecAugment (Park et al., arXiv:1904.08779): time / frequency masking of a feature batch on the device.
 *   x (B,F,T) fp32 contiguous, zero beyond each utterance's length; lengths (B) int32 (clamped to [0,T]); out (B,F,T), may equal x.
 *   id_b = utt_ids[b] (utt_ids (B) int32 on the device), or batch_offset + b where utt_ids is NULL: the utterance's index in the
 *   GLOBAL batch, so a rank, a shard or a micro-batch masks exactly what one process holding the whole batch masks.
 *   Every mask interval of utterance b comes from ONE Philox4x32-10 block:
 *        w = philox4x32_10(ctr = (id_b, offset, dom, m), key = (seed lo32, seed hi32)),   m = the mask's index,
 *        dom = 2 for the n_freq frequency masks, 3 for the n_time time masks (the samplers use 0 and 1 in that word: one seed
 *        serves both without overlap);
 *        span = F, W = min(freq_width, F)                                                       (frequency mask)
 *        span = len_b, W = min(time_width, len_b, (int)fmul_rn(time_ratio, (float)len_b))       (time mask: one fp32 multiply,
 *                                                                                                then truncation)
 *        width = ((w[0] >> 8) * (W + 1)) >> 24            uniform on 0 .. W
 *        start = ((w[1] >> 8) * (span - width + 1)) >> 24  uniform on 0 .. span - width          (64-bit integers, no float)
 *   out[b,f,t] = the fill value where t < len_b and (f lies in a frequency interval of b or t in a time interval of b), else
 *   x[b,f,t]: frames t >= len_b are copied (the padding stays zero), and so is every row with len_b <= 0 or id_b < 0 (id_b < 0: a
 *   padded, empty utterance; it has no intervals).  fill_mode PGASR_SPECAUG_FILL_ZERO: 0.0f; PGASR_SPECAUG_FILL_ROW_MEAN: the mean of
 *   the ORIGINAL x[b,f,0:len_b] (masked frames included), summed in fp64 in a fixed order (two runs give the same bits), divided by
 *   len_b in fp64, rounded to fp32.
 *   masks: NULL, or (B, n_freq + n_time, 2) int32: (start, width) of every interval, frequency masks first (0, 0 where id_b < 0).
 *   One launch, no workspace, no atomics, no host synchronisation; any B, F, T (16-byte accesses where T % 4 == 0 and x, out are
 *   16-byte aligned).  Checked before any pointer is touched or anything is launched: x, lengths or out NULL, B / F / T < 1, a negative
 *   count or width, time_ratio outside (0,1] or NaN, an unknown fill_mode: PGASR_ERR_INVALID_ARG; more than 8 masks of a kind:
 *   PGASR_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------- */
#define PGASR_SPECAUG_FILL_ROW_MEAN 0
#define PGASR_SPECAUG_FILL_ZERO 1
int pgasr_spec_augment(const float* x, const int32_t* lengths, const int32_t* utt_ids /* NULL: id = batch_offset + b */,
                       int batch_offset, int B, int F, int T, int n_freq, int freq_width, int n_time, int time_width,
                       float time_ratio, int fill_mode, unsigned long long seed, unsigned offset,
                       float* out /* may equal x */, int32_t* masks /* NULL or (B, n_freq + n_time, 2): start, width */,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * A0-LFR  Low-frame-rate input (Sak et al., Interspeech 2015; Pundak & Sainath, Interspeech 2016): stack `stack` neighbouring frames
 *   of a feature batch and keep every `skip`-th one, on the device (csrc/frame_stack.hip; in numpy: tests/frame_stack_ref.py).
 *   x (B,F,T) fp32 contiguous; n_frames (B) int32 on the device, clamped to [0,T]; out (B, stack*F, Tout) fp32, not x.
 *   With n = n_frames[b], n' = ceil(n / skip) and Tout = ceil(T / skip):
 *        out[b, j*F + f, t'] = x[b, f, clamp(t'*skip + j - left, 0, n-1)]     for t' < n',  j = 0 .. stack-1
 *        out[b, j*F + f, t'] = 0.0f                                            for n' <= t' < Tout
 *   The rows are offset-major (j), feature-minor (f), as in Kaldi's splice; `left` of the stack's frames lie in front of the anchor
 *   frame t'*skip.  The edges replicate the first / last real frame; an utterance of 0 frames gives all zeros and n' = 0.
 *   fmask_out: NULL, or (B,1,Tout) fp32 = (t' < n');  n_out: NULL, or (B) int32 = n'.
 *   Pure data movement: the result equals the statement above bit for bit, whatever x holds (NaN and inf included); a frame at or
 *   beyond n is never read, so x need not be zero (or even finite) there.
 *   One launch, no workspace, no atomics, no host synchronisation; any T and any alignment (16-byte loads where T % 4 == 0 and x is
 *   16-byte aligned).  Checked before any pointer is touched or anything is launched, PGASR_ERR_INVALID_ARG: x, n_frames or out
 *   NULL, out == x, B / F / T < 1, stack or skip outside [1, 16], left outside [0, stack), stack * F > 65535, B > 65535,
 *   Tout != ceil(T / skip).
 * ---------------------------------------------------------------------------------------- */
int pgasr_frame_stack(const float* x, const int32_t* n_frames, int B, int F, int T, int stack, int skip, int left, int Tout,
                      float* out, float* fmask_out /* NULL or (B,1,Tout) */, int32_t* n_out /* NULL or (B) */, void* stream);

/* ------------------------------------------------------------------------------------------
 * A0-RS  Sample-rate conversion and speed perturbation (Ko et al., Interspeech 2015) of a waveform batch on the device: one
 *   polyphase Hann-windowed sinc filter (the function of torchaudio's default "sinc_interp_hann" resampler, 6 zero crossings,
 *   rolloff 0.99).  A conversion is a reduced ratio L / M = output rate / input rate; speed factor f = p / q is the ratio q / p.
 *   Per ratio (all in fp64, h then rounded to fp32):
 *        fc = 0.99 * min(1, L / M);  half = ceil(6 / fc);  W = 2 * half + 1 taps
 *        base_j = (j * M) / L (integer),  frac_j = j * M / L - base_j                            for each phase j = 0 .. L-1
 *        t = fc * ((k - half) - frac_j);  h[j][k] = fc * sinc(t) * cos(pi * t / 12)^2 if |t| < 6, else 0    (sinc(t) = sin(pi t) / (pi t))
 *   wave (B, in_stride) fp32; n_in (B) int32 on the device, clamped to [0, in_stride]; out (B, out_stride) fp32, not wave.
 *   Row b takes ratio r = ratio_idx[b] (ratio_idx (B) int32 on the device; NULL: every row takes ratio 0):
 *        n_out[b] = ceil(n_in[b] * L / M)                                                        (64-bit integers)
 *        out[b, i * L + j] = fp32( sum_{k = 0 .. W-1} fp64(h[j][k]) * fp64(wave[b, i * M + base_j - half + k]) )
 *   summed in ascending k in an fp64 accumulator that starts at +0.0; a tap whose sample lies outside [0, n_in[b]) is skipped and
 *   never read.  A product of two fp32 numbers is exact in fp64, so the result equals a numpy loop over k bit for bit, and two runs
 *   give the same bits.  out[b, n] = 0.0f for n_out[b] <= n < out_stride.  Ratio 1/1 copies the bits of wave[b, 0:n_in[b]].  A row
 *   with n_in[b] <= 0, or with ratio_idx[b] outside [0, n_ratios), is zeros and n_out[b] = 0.
 *   ratio_desc: HOST memory, (n_ratios, 4) int32: L, M, W, and the offset in words of the ratio's h[L][W] in `tables` (device,
 *   fp32); `bases` (device, int32) holds base_j of ratio 0, then of ratio 1, ..: L_r words each, with no gaps.
 *   One launch, no workspace, no atomics, no host synchronisation: a workgroup stages the input span of a tile of consecutive
 *   outputs in LDS (16-byte loads where in_stride % 4 == 0 and wave is 16-byte aligned) and the ratio's table beside it where
 *   L * W <= 5632 words.  Checked before any device pointer is touched or anything is launched: a NULL pointer (ratio_idx excepted),
 *   out == wave, B / in_stride / out_stride / n_ratios < 1: PGASR_ERR_INVALID_ARG; n_ratios > 8: PGASR_ERR_UNSUPPORTED; then per
 *   descriptor L or M < 1 or gcd(L, M) != 1: PGASR_ERR_INVALID_ARG; L or M > 1024, or L / M outside [1/16, 16] (so W <= 195):
 *   PGASR_ERR_UNSUPPORTED; a W that is not the W of L / M, or a negative offset: PGASR_ERR_INVALID_ARG; last, out_stride below
 *   the largest ceil(in_stride * L / M) of the ratios: PGASR_ERR_INVALID_ARG.
 * ---------------------------------------------------------------------------------------- */
int pgasr_resample(const float* wave, int in_stride, const int32_t* n_in, int B,
                   const int32_t* ratio_idx /* NULL: all 0 */, int n_ratios, const int32_t* ratio_desc /* host */,
                   const float* tables, const int32_t* bases, float* out, int out_stride, int32_t* n_out /* written */,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * A0-WA  Waveform augmentation on the device (csrc/wave_aug.hip; in numpy: tests/wave_aug_ref.py): convolution with a room impulse
 *   response and additive noise at a drawn signal-to-noise ratio (the Kaldi / ESPnet "noise + RIR" recipe; Ko et al., ICASSP 2017).
 *   Waveforms are fp32 rows (B, stride) with lengths n (B) int32 on the device, clamped to [0, stride]; every intermediate is fp64.
 *   A product of two fp32 numbers is exact in fp64, so a fused multiply-add and a multiply followed by an add give the same bits.
 *   Bit statements hold for finite samples and taps.  Each call is launches on `stream` only: no workspace, no atomics, no host
 *   synchronisation, 16-byte accesses where the stride is a multiple of 4 and the bases are 16-byte aligned; two runs give the same bits.
 *
 * pgasr_reverb: rirs (n_rirs, rir_stride) fp32; row r has K = rir_len[r] taps (clamped to [0, min(rir_stride, max_taps)]) and its
 *   direct path at d = rir_delay[r] (clamped to [0, K-1]): the first index of max |h|, found by whoever builds the bank.
 *   With r = rir_idx[b] in [0, n_rirs), for 0 <= i < n_b:
 *        out[b, i] = fp32( sum_{k = 0 .. K-1} fp64(h[k]) * fp64(wave[b, i + d - k]) )
 *   summed in ascending k in an fp64 accumulator that starts at +0.0; a term whose sample index lies outside [0, n_b) is skipped and
 *   the sample never read.  The output is as long as the input: out[b, i] = 0.0f for n_b <= i < stride.  A row with rir_idx[b]
 *   outside [0, n_rirs) is copied bit for bit (zero beyond n_b).  out must not be wave (PGASR_ERR_INVALID_ARG, as are a NULL pointer
 *   and B / stride / rir_stride / n_rirs < 1).  A workgroup computes a tile of `tile` outputs and stages `chunk` taps at a time:
 *   pgasr_reverb_limits reports both and max_taps (>= 16000: one second at 16 kHz); any of its pointers may be NULL.
 *
 * pgasr_wave_power: power[b] = sum_{i < n_b} fp64(src[row_b, (start_b + i) mod period_b])^2, fp64, in a fixed order that depends on
 *   n_b alone: the value does not depend on what else is in the batch.  src (src_rows, src_stride) fp32.  row NULL: row_b = b (then
 *   src_rows >= B); period NULL: no wrap -- start must be NULL too, period_b = src_stride and n_b is clamped to it; else period_b is
 *   clamped to src_stride, start_b is reduced mod period_b, and n_b may exceed period_b (the segment wraps, several times if need be).
 *   0 where n_b <= 0, row_b lies outside [0, src_rows) or period_b < 1.  power: (B) fp64, written.
 *
 * pgasr_wave_mix: for i < n_b
 *        out[b, i] = fp32( fp64(a_b) * fp64(wave[b, i]) + fp64(g_b) * fp64(noise[r_b, (s_b + i) mod m_b]) ),   0.0f for n_b <= i < stride,
 *   r_b = noise_idx[b], m_b = noise_len[r_b] (clamped to noise_stride), s_b = noise_start[b] mod m_b (noise_start NULL: 0).  Where
 *   g_b = 0 the noise is not read and the term is dropped: out = fp32(fp64(a_b) * fp64(wave)), with a_b = 1 the bits of the input.
 *   A row takes no noise (g_b = 0) where noise is NULL, r_b lies outside [0, noise_rows), m_b < 1 or n_b < 1.
 *   gains (B, 2) fp32 holds (a_b, g_b).  gains_given != 0: they are read (g_b still 0 for a row that takes no noise).  Else they
 *   are formed from p_dry, p_wet, p_noise and amp (each (B) fp64; amp_b = 10^(-snr_b / 20), computed on the host) and written:
 *        a_b = fp32( sqrt(p_dry / p_wet) )                     the dry signal's level, restored after the reverberation;
 *                                                               1 where a power is 0 or the result is no finite positive fp32
 *        g_b = fp32( amp_b * sqrt((fp64(a_b)^2 * p_wet) / p_noise) )    0 where a power or amp_b is 0, the row takes no noise, or the
 *                                                               result is no finite positive fp32: never inf or NaN
 *   every fp64 operation rounded once, in the order written.  The gains are fp32 so that a sum of squares whose last bits differ
 *   does not change the output (the idiom of SpecAugment's row mean).  out may equal wave.
 * ---------------------------------------------------------------------------------------- */
int pgasr_reverb_limits(int* tile, int* chunk, int* max_taps);
int pgasr_reverb(const float* wave, int stride, const int32_t* n, int B, const float* rirs, int rir_stride, int n_rirs,
                 const int32_t* rir_len, const int32_t* rir_delay, const int32_t* rir_idx, float* out /* not wave */, void* stream);
int pgasr_wave_power(const float* src, int src_stride, int src_rows, const int32_t* n, int B, const int32_t* row /* NULL: b */,
                     const int32_t* start /* NULL: 0 */, const int32_t* period /* NULL: no wrap */, double* power, void* stream);
int pgasr_wave_mix(const float* wave, int stride, const int32_t* n, int B, const double* p_dry, const double* p_wet,
                   const double* p_noise, const double* amp, const float* noise /* NULL: none */, int noise_stride, int noise_rows,
                   const int32_t* noise_len, const int32_t* noise_idx, const int32_t* noise_start, float* gains /* (B,2) */,
                   int gains_given, float* out /* may equal wave */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Elementwise pieces of the train step.
 * pgasr_dropout: inverted dropout y = keep ? x/(1-p) : 0 (nn.Dropout, model.py:45,51 p=0.5; LSTM
 *   inter-layer dropout model.py:42 p=0.3).  keep is a pure function of (seed, offset, element
 *   index) (Philox4x32-10 on counter (index/4, offset), word index%4 >= p*2^32), so the backward
 *   pass re-applies the SAME call to the gradient instead of storing a mask.  x == y allowed.
 *   dact_y (optional, n elements): the result is also multiplied by (dact_y > 0 ? 1 : slope) -- the backward
 *   of F.leaky_relu (model.py:50) fused into the backward of the dropout that follows it (model.py:51).
 * pgasr_adam_step: torch.optim.Adam update (model.py:207, lr=5e-4) on flat fp32 buffers;
 *   step is the 1-based count of CALLS.  guard0 / guard1 (optional, device int32 words, e.g. the sweep workspaces'
 *   error words, or -- data parallel -- the word of the gradient buffer that carried every rank's error flag through
 *   the all-reduce, so that all replicas skip together): the update is skipped -- parameters and moments untouched --
 *   while either is != 0.  applied (optional, two device int32 words, zeroed once by the owner): the number of updates
 *   really applied, kept on the device in ping-pong fashion (word (step-1)&1 is read, word step&1 written); the bias
 *   correction then uses that count + 1 instead of `step`, so a skipped update does not shift it.  NULL: `step` is used.
 * ---------------------------------------------------------------------------------------- */
int pgasr_dropout(const float* x, float* y, unsigned long long n, float p, uint64_t seed, uint32_t offset,
                  const float* dact_y, float slope, void* stream);
/* A0 batch hand-over (model.py:227-230, `.to(device)`): copies `bytes` from src to dst (both 16-byte aligned) with
 * `workgroups` (<= 1024) streaming workgroups on `stream`.  src may be pinned host memory that is mapped into the
 * device's address space (hipHostMalloc, PyTorch's pinned tensors): the launch never blocks the host, and on a stream of
 * its own the copy runs beside the train step instead of in front of it. */
int pgasr_stream_copy(const void* src, void* dst, unsigned long long bytes, int workgroups, void* stream);
int pgasr_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, unsigned long long n,
                    int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                    const int32_t* guard0, const int32_t* guard1, int32_t* applied, void* stream);
/* Gradient clipping by global norm (torch.nn.utils.clip_grad_norm_) and a non-finite guard, on the device (csrc/optim.hip).
 * The clip state is PGASR_CLIP_STATE_BYTES of device memory, 16-byte aligned, zeroed once by its owner:
 *   float norm; float scale; int32 nonfinite; int32 pad; int32 n_clipped; int32 n_nonfinite; int32 pad2[2];
 * pgasr_grad_norm_clip(grad, n, max_norm, ws, ws_bytes, state, stream): over the n fp32 words of grad (16-byte aligned)
 *   norm      = sqrt(sum g^2), squares and sums in fp64 (the square of an fp32 is exact there), rounded to fp32 once;
 *   scale     = min(1, max_norm / (norm + 1e-6f)) in fp32 -- clip_grad_norm_'s arithmetic; exactly 1.0f when nothing is clipped;
 *   nonfinite = 1 iff the sum is not finite, i.e. some element is inf or NaN; scale is then 0;
 *   n_nonfinite += nonfinite; n_clipped += (scale < 1 and the sum is finite) -- running counts, kept on the device.
 *   max_norm must be > 0; +inf is allowed and means "measure and guard, never scale".
 *   The result is a function of (grad, n) only: a grid derived from n, fixed orders inside a lane, a wave and a workgroup (no
 *   floating-point atomics), one fp64 partial per workgroup parked in ws, and a second one-wave launch that adds the partials in a
 *   fixed order (stream order is its only synchronisation: ws needs no initialisation and holds nothing between calls).  The same
 *   gradient gives the same 32 bits of norm and scale, run to run and rank to rank.
 *   ws: pgasr_grad_norm_ws_bytes(n) bytes (at most 8 KB), 8-byte aligned.
 *   n == 0, a null or misaligned pointer, max_norm not > 0 (NaN included) or ws_bytes too small: PGASR_ERR_INVALID_ARG, nothing launched.
 * pgasr_adam_step_clipped: pgasr_adam_step with g := state.scale * g (rounded on its own: scale == 1.0f gives pgasr_adam_step's bits)
 *   and state.nonfinite != 0 as one more guard -- the update is skipped, parameters and moments untouched, applied not advanced.
 *   clip_state: a state pgasr_grad_norm_clip has written on the same stream (null or misaligned: PGASR_ERR_INVALID_ARG). */
#define PGASR_CLIP_STATE_BYTES 32
size_t pgasr_grad_norm_ws_bytes(unsigned long long n);
int pgasr_grad_norm_clip(const float* grad, unsigned long long n, float max_norm, void* ws, size_t ws_bytes,
                         void* state, void* stream);
int pgasr_adam_step_clipped(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, unsigned long long n,
                            int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                            const int32_t* guard0, const int32_t* guard1, int32_t* applied, const void* clip_state,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * N3  feature front end (data.py:44-79): MFCC(40) + delta + delta-delta of torchaudio's defaults
 *   (16 kHz, n_fft 400, hop 200, periodic Hann, reflect-centred frames, power spectrum, 128 HTK mel bands,
 *   10*log10 floored at the utterance's max - top_db, orthonormal DCT-II; 5-tap delta filter with replicate
 *   padding).  The DFT / mel / DCT contractions are pgasr_gemm_f32 calls made by the host between these:
 *   pgasr_feat_frames:  wave (B rows of wave_stride samples), n_samples (B), n_frames (B) = 1 + n_samples/200
 *                       -> frames (B*Tmax, 400), windowed, zero rows past an utterance's frames
 *   pgasr_feat_power:   spec (rows, 402) = [re(201) | im(201)] -> power (rows, 201)
 *   pgasr_feat_db:      in place on mel (B, Tmax, n_mels)
 *   pgasr_feat_deltas_stack: mfcc (B, Tmax, n_mfcc) -> feat (B, 3*n_mfcc, Tmax) zero padded (the reference's
 *                       batch layout, data.py:71-79), fmask (B, 1, Tmax) (optional)
 *   Preconditions the calls cannot check (the lengths live on the device): 200 < n_samples[b] <= wave_stride -- the reflect
 *   index of a shorter utterance leaves its row (features._FrontEnd refuses it with a ValueError); 1 <= n_frames[b] <= Tmax.
 *   Checked, PGASR_ERR_INVALID_ARG before any launch: null pointers (fmask alone may be NULL), B, Tmax, wave_stride, rows,
 *   n_mels, n_mfcc, C <= 0, B or n_mfcc / C > 65535 in the two stacking calls (grid dimensions), B * Tmax > 2^31 - 1 in
 *   pgasr_feat_frames, top_db not > 0 (NaN included).
 *   Rows t >= n_frames[b] are never read: pgasr_feat_frames / _deltas_stack / _stack write zeros there whatever the input row
 *   holds, pgasr_feat_db leaves them as they are and takes its maximum over the utterance's own n_frames[b] * n_mels cells.
 *   A delta is (2 (x[t+2] - x[t-2]) + (x[t+1] - x[t-1])) / 10 with the indices clamped to [0, n_frames[b] - 1]: exactly 0 over
 *   a constant stretch, so both deltas of a one-frame utterance are exactly 0.
 * ---------------------------------------------------------------------------------------- */
int pgasr_feat_frames(const float* wave, const int32_t* n_samples, const int32_t* n_frames, int B,
                      long long wave_stride, int Tmax, float* frames, void* stream);
int pgasr_feat_power(const float* spec, long long rows, float* power, void* stream);
int pgasr_feat_db(float* mel, const int32_t* n_frames, int B, int Tmax, int n_mels, float top_db, void* stream);
int pgasr_feat_deltas_stack(const float* mfcc, const int32_t* n_frames, int B, int Tmax, int n_mfcc,
                            float* feat, float* fmask, void* stream);
/* x (B x Tmax x C) -> feat (B x C x Tmax), 0 past n_frames[b], and fmask (B x 1 x Tmax): the layout of data.py:64-79 for a front
 * end without deltas -- the 80-band log-mel features (F = 80 of the benchmark; features.LogMel). */
int pgasr_feat_stack(const float* x, const int32_t* n_frames, int B, int Tmax, int C, float* feat, float* fmask, void* stream);

/* ------------------------------------------------------------------------------------------
 * A5-WIDE / A9-WIDE  alphabets of up to PGASR_MAX_VOCAB_WIDE = 1024 symbols (subword units): the four kernels that hold a (t,b)
 * row of scores in one wave, for rows of 1 <= V <= 1024 fp32 values.  One wave per row as before, lane l holding the
 * NV = ceil(V / 64) (rounded up to 1, 2, 4, 8 or 16) consecutive labels l*NV .. l*NV + NV - 1 in registers.  The entries above keep
 * what they accept (V <= 64) and what they launch; these take any V in the range, V <= 64 included.  Every sum is taken in a fixed
 * order: two calls give the same bits.  Checked before any HIP call: V <= 0, T, B or rows <= 0, a blank outside [0, V), a missing
 * required pointer -> PGASR_ERR_INVALID_ARG; V > 1024, and for the CTC pair 2 * Lmax + 1 > 2048 -> PGASR_ERR_UNSUPPORTED.
 *   pgasr_log_softmax_rows_wide: pgasr_log_softmax_rows.  Row maximum, exp of the differences and their sum in fp32.
 *   pgasr_frame_argmax_sample_wide: pgasr_frame_argmax_sample and, with utt_ids != NULL, pgasr_frame_argmax_sample_ids (ctr_base is
 *     then ignored, ctr_stride >= 1 is required and T * ctr_stride must fit counter word 0, else PGASR_ERR_UNSUPPORTED).  The
 *     arg-max takes the first maximum.  The sample uses the same Philox counter, key and u, the domain for rows beyond the global
 *     batch included: k = min(#{v : cdf_v <= u * total}, V - 1) with the inclusive cdf of exp(score - max) in label order (a
 *     sequential prefix over the lane's labels on top of the wave scan of the lane totals; with V <= 64 the narrow kernel's cdf),
 *     moved off a label whose exp(score - max) is 0 by the rule of A9 / A12.
 *   pgasr_ctc_loss_grad_wide, pgasr_ctc_grad_from_lattice_wide: pgasr_ctc_loss_grad and pgasr_ctc_grad_from_lattice, argument for
 *     argument, on the same workspace (pgasr_ctc_workspace_bytes, same format: either pair may run the gradient pass over the
 *     other's lattice).  The alpha / beta sweeps are the same kernel, so nll has the same bits; the label lists and the gradient
 *     pass utt_scale_b (softmax - occupancy) + pg_coef (softmax - onehot(pg_path)) are kernels of their own.  A symbol of
 *     probability exactly 0 has occupancy 0 and gradient entry 0, rows t >= input_lengths[b] are written as zeros, an utterance
 *     without an alignment (nll = +inf) gets no CTC part.
 * ---------------------------------------------------------------------------------------- */
#define PGASR_MAX_VOCAB_WIDE 1024
int pgasr_log_softmax_rows_wide(const float* logits, long long rows, int V, float* log_probs, void* stream);
int pgasr_frame_argmax_sample_wide(const float* scores, int T, int B, int V, uint64_t seed, uint32_t offset,
                                   int ctr_stride, int ctr_base, const int32_t* utt_ids /* may be NULL */,
                                   int32_t* greedy_path /* may be NULL */, int32_t* sample_path /* may be NULL */, void* stream);
int pgasr_ctc_loss_grad_wide(const float* log_probs, const int32_t* targets,
                             const int32_t* input_lengths, const int32_t* target_lengths,
                             int T, int B, int V, int Lmax, int blank,
                             const float* utt_scale, const float* pg_coef, const int32_t* pg_path,
                             float* nll, float* grad_logits,
                             void* workspace, size_t workspace_bytes, void* stream);
int pgasr_ctc_grad_from_lattice_wide(const float* log_probs, const int32_t* input_lengths,
                                     const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                     const float* utt_scale, const float* pg_coef, const int32_t* pg_path,
                                     int pg_coef_per_frame, float* grad_logits, void* workspace, size_t workspace_bytes,
                                     void* stream);

/* ------------------------------------------------------------------------------------------
 * A12-WIDE  The multi-sample, entropy and KL objectives (A12) for rows of 1 <= V <= 1024 symbols: the four kernels of those
 * objectives that hold one symbol per lane, on the rows of A5-WIDE / A9-WIDE (lane l holding NV consecutive labels).  Everything
 * else the objectives run (collapse, edit distance, pgasr_pg_rewards_multi, pgasr_pg_loss_value_multi, the lattice) never looks at
 * V.  The narrow entries keep what they accept (V <= 64) and what they launch.  Every sum is taken in a fixed order -- a lane's
 * NV terms in label order, then one wave butterfly; frames in t order -- so two calls give the same bits, and with V <= 64 the
 * operations are the narrow kernel's, one for one.  Checked before any HIP call, with the narrow twins' codes: a missing required
 * pointer, T, B or V <= 0, K outside 1..PGASR_MAX_SAMPLES, a blank outside [0, V) -> PGASR_ERR_INVALID_ARG; V > 1024,
 * 2 * Lmax + 1 > 2048 -> PGASR_ERR_UNSUPPORTED; a workspace that is missing or too small -> PGASR_ERR_WORKSPACE.
 *   pgasr_frame_sample_multi_wide: pgasr_frame_sample_multi and, with utt_ids != NULL, pgasr_frame_sample_multi_ids (ctr_base is
 *     then ignored, ctr_stride >= 1 is required and T * ctr_stride must fit counter word 0, else PGASR_ERR_UNSUPPORTED).  The
 *     row's maximum, cdf and total are pgasr_frame_argmax_sample_wide's and are formed once; draw k uses Philox word 0 of counter
 *     (t*ctr_stride + id, offset, 0 or 1, k), the same u and the same min(#{v : cdf_v <= u * total}, V - 1), moved off a label
 *     of probability 0 by the same rule.  Draw 0 is pgasr_frame_argmax_sample_wide's sample and greedy_path its arg-max, bit for
 *     bit.
 *   pgasr_frame_entropy_wide, pgasr_frame_kl_wide: pgasr_frame_entropy and pgasr_frame_kl, argument for argument: one workgroup of
 *     16 waves per utterance, frames added in t order with fp64 carries.  p = 0 adds exactly 0; the reference's log-probability is
 *     floored at PGASR_KL_LOG_FLOOR; q = p gives exactly 0.
 *   pgasr_ctc_grad_from_lattice_multi_wide: pgasr_ctc_grad_from_lattice_multi, _multi_ent and _multi_kl in one entry, on the
 *     workspace of pgasr_ctc_loss_grad or pgasr_ctc_loss_grad_wide (same format: either lattice serves).  One wave per (t,b) row,
 *     one write: the CTC part of pgasr_ctc_grad_from_lattice_wide, then pg_coef[k,b] (softmax - onehot(pg_paths[k,t,b])) in k
 *     order, then ent_scale_b p (ln p + H) when ent_scale is given, then kl_scale_b p (ln p - lnq - KL) when ref_log_probs and
 *     kl_scale are (both or neither, else PGASR_ERR_INVALID_ARG); a KL term of 0 leaves the entry as it is.  Rows t >=
 *     input_lengths[b] are written as zeros, nll = +inf gives no CTC part, log p = -inf gives occupancy 0, gradient entry 0 and
 *     entropy and KL terms 0, never NaN.  The pass without tails holds no code of them.
 * ---------------------------------------------------------------------------------------- */
int pgasr_frame_sample_multi_wide(const float* scores, int T, int B, int V, int K, uint64_t seed, uint32_t offset,
                                  int ctr_stride, int ctr_base, const int32_t* utt_ids /* may be NULL */,
                                  int32_t* greedy_path /* may be NULL */, int32_t* sample_paths /* (K,T,B) */, void* stream);
int pgasr_frame_entropy_wide(const float* log_probs, const int32_t* input_lengths, int T, int B, int V,
                             float beta, float inv_global_batch, float* ent_mean, float* ent_scale, void* stream);
int pgasr_frame_kl_wide(const float* log_probs, const float* ref_log_probs, const int32_t* input_lengths, int T, int B, int V,
                        float gamma, float inv_global_batch, float* kl_mean, float* kl_scale, void* stream);
int pgasr_ctc_grad_from_lattice_multi_wide(const float* log_probs, const int32_t* input_lengths,
                                           const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                           const float* utt_scale, int K, const float* pg_coef, const int32_t* pg_paths,
                                           const float* ent_scale /* may be NULL */, const float* ref_log_probs /* may be NULL */,
                                           const float* kl_scale /* may be NULL */, float* grad_logits,
                                           void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A12-SCORE  Lattice-free CTC scorer (csrc/hyp_score.hip): the exact -log p(y | x) of every hypothesis of an N-best list, one fp64
 * number per hypothesis.  The forward sweep of pgasr_ctc_hyp_lattice alone, with its rows kept in LDS: no workspace, nothing
 * written but the result, so none of the lattice's limits (K <= 16, V <= 64) and none of its 2*K*B*T*roundup64(2*Lh+1)*4 bytes.
 *   log_probs (T,B,V) fp32; hyp_tokens (N,B,hyp_stride) / hyp_len (N,B) int32 as pgasr_ctc_beam_search_nbest and _wide write
 *   them; count (B) int32, clamped to [0,N], or NULL: every row; input_lengths (B) int32.  out_nll (N,B) fp64, every word written.
 *   With len = max(hyp_len[n,b], 0) and Tb = clamp(input_lengths[b], 0, T), in this order:
 *     n >= count[b]                                     -> +inf, no work
 *     len > Lh or len > hyp_stride                      -> +inf, no work (nothing behind len is ever read)
 *     a token outside [0,V) or equal to blank           -> +inf (every gather index is brought into the row first: garbage tokens
 *                                                          never cause a read outside log_probs)
 *     Tb == 0                                           -> 0 for len == 0, +inf otherwise
 *     else  -log sum_alignments prod_t p_t              the alpha recurrence of A5 over the 2*len+1 states, ending in the sum of
 *                                                          alpha[S-1] and alpha[S-2]; +inf when no alignment exists (len +
 *                                                          repeats > Tb, symbols of probability 0).
 *   Arithmetic: the linear domain, every alpha an fp64 fraction with an int32 binary exponent of its own (nothing underflows; each
 *   frame rounds a few times at 2^-53), exp(log_prob) in fp64, one fp64 log at the end: within 1e-9 relative of the log-domain
 *   recurrence in fp64 (tests/hyp_score_ref.py), where pgasr_ctc_hyp_lattice's fp32 nll is within 1e-5.  A likelihood below
 *   2^-(2^30) (an nll above 7.4e8 nats) reads +inf.
 *   Never NaN for inputs that are finite or -inf.  No atomics: two calls give the same bits.  Every frame loop is bounded by Tb,
 *   every state loop by 2*len+1.  One launch, one workgroup per (utterance, hypothesis), no host synchronisation.
 *   Checked before any HIP call: a NULL pointer (count excepted), T, B, N or hyp_stride < 1, Lh < 0, V < 1, blank outside [0,V) ->
 *   PGASR_ERR_INVALID_ARG; then V > 1024, N > 128, 2*Lh+1 > 2048 (or N*B >= 2^31) -> PGASR_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------------- */
int pgasr_ctc_hyp_score(const float* log_probs, const int32_t* hyp_tokens, int hyp_stride, const int32_t* hyp_len,
                        const int32_t* count /* NULL: every row */, const int32_t* input_lengths,
                        int T, int B, int V, int N, int Lh, int blank, double* out_nll, void* stream);

/* ------------------------------------------------------------------------------------------
 * A13-WIDE  The sequence-level score function and MWER over N-best lists (A13-MWER) for rows of 1 <= V <= 1024 symbols: the two
 * kernels of those objectives that hold one symbol per lane -- the label lists of the K*B hypothesis lattices and the gradient
 * pass over K+1 lattices -- on the rows of A5-WIDE.  The sweeps are the narrow entry's kernel (the lattice never looks at V beyond
 * addressing a row), so with V <= 64 hyp_nll and every alpha / beta word have pgasr_ctc_hyp_lattice's bits; collapse, edit
 * distance, pgasr_mwer_weights, pgasr_pg_rewards_multi and pgasr_pg_loss_value_seq never look at V.  The narrow entries keep what
 * they accept (V <= 64) and what they launch.
 *   pgasr_ctc_hyp_workspace_bytes_wide: pgasr_ctc_hyp_workspace_bytes for V <= 1024 (the same layout; 0 where the arguments are
 *     refused).
 *   pgasr_ctc_hyp_lattice_wide: pgasr_ctc_hyp_lattice, argument for argument.  The label -> states lists of pair p = k*B + b are
 *     built from row p of hyp_tokens and hyp_len[p] by integer counts, a scan over V + 1 counts and slot = offset + rank among
 *     earlier equal tokens, so each list ascends in s.  A pair with hyp_len > Lh has no lattice; its nll reads 0.
 *   pgasr_ctc_grad_from_lattices_seq_wide: pgasr_ctc_grad_from_lattices_seq, _seq_ent, _seq_kl and, with pg_paths == NULL,
 *     pgasr_ctc_grad_from_lattices_nbest in one entry, on the workspaces of pgasr_ctc_loss_grad[_wide] and
 *     pgasr_ctc_hyp_lattice[_wide] (same formats).  One wave per (t,b) row, one write: the target part of
 *     pgasr_ctc_grad_from_lattice_multi_wide; then for k = 0 .. K-1 in k order pg_coef[k,b] (softmax - occ_{y_k}) from lattice (k,b)
 *     where hyp_len[k,b] <= Lh, else pg_coef[k,b] (softmax - onehot(pg_paths[k,t,b])) -- nothing when pg_paths is NULL --; then
 *     ent_scale_b p (ln p + H) when ent_scale is given; then kl_scale_b p (ln p - lnq - KL) when ref_log_probs and kl_scale are
 *     (both or neither, else PGASR_ERR_INVALID_ARG).  The N-best form takes no tails (ent_scale or kl_scale with pg_paths == NULL
 *     -> PGASR_ERR_INVALID_ARG).  Rows t >= input_lengths[b] are written as zeros, a lattice whose nll is +inf adds nothing,
 *     log p = -inf gives occupancy 0 and gradient entry 0, never NaN.  Fixed summation order: the same bits every call, and with
 *     V <= 64 the narrow kernels' sums in their order.
 * Checked before any HIP call, with the narrow twins' codes: a missing required pointer, T, B or V <= 0, Lh < 0, K outside
 * 1..PGASR_MAX_SAMPLES, a blank outside [0, V), hyp_stride < max(1, Lh) -> PGASR_ERR_INVALID_ARG; V > 1024, 2 * Lh + 1 > 2048,
 * 2 * Lmax + 1 > 2048 -> PGASR_ERR_UNSUPPORTED; a workspace that is missing or too small -> PGASR_ERR_WORKSPACE.
 * ---------------------------------------------------------------------------------------- */
size_t pgasr_ctc_hyp_workspace_bytes_wide(int T, int B, int V, int K, int Lh);
int pgasr_ctc_hyp_lattice_wide(const float* log_probs, const int32_t* hyp_tokens, int hyp_stride, const int32_t* hyp_len,
                               const int32_t* input_lengths, int T, int B, int V, int K, int Lh, int blank,
                               float* hyp_nll, void* hyp_workspace, size_t hyp_workspace_bytes, void* stream);
int pgasr_ctc_grad_from_lattices_seq_wide(const float* log_probs, const int32_t* input_lengths, const int32_t* target_lengths,
                                          int T, int B, int V, int Lmax, int blank, const float* utt_scale,
                                          int K, const float* pg_coef, const int32_t* pg_paths /* NULL: the N-best form */,
                                          const int32_t* hyp_len, int Lh, const float* ent_scale /* may be NULL */,
                                          const float* ref_log_probs /* may be NULL */, const float* kl_scale /* may be NULL */,
                                          float* grad_logits, void* workspace, size_t workspace_bytes,
                                          void* hyp_workspace, size_t hyp_workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A12-STEP  Per-step rewards (pgasr_pg_step_coefs) with K sampled paths, either baseline, both tails and rows of 1 <= V <= 1024
 * symbols: the reward-to-go of every frame goes into the multi-sample REINFORCE term in place of one coefficient per utterance.
 * Path rows of utterance b: the hypothesis baseline has P = K + 1 rows, the greedy path first, then the K samples; leave one out
 * has P = K rows.  For row w with collapsed length n_w and D_w[i] = ED(y_b, yhat_w[:i]) (pgasr_edit_distance's prefix row):
 *   a character starts at frame t when t < T_b, the label is not blank, and t = 0 or the label differs from the label at t - 1;
 *   c_w(t) = characters started at frames < t, clipped to n_w;      G_w(t) = D_w[c_w(t)] - D_w[n_w]      an integer
 *   kf_b   = ((lam * inv_global_batch) / K) / max(L_b,1)            fp32, in this order
 *   PGASR_BASELINE_HYPOTHESIS:     coef[k,t,b] = kf_b * (G_k(t) - G_greedy(t))
 *   PGASR_BASELINE_LEAVE_ONE_OUT:  coef[k,t,b] = kf_b * (G_k(t) - (S(t) - G_k(t)) / (K-1)),  S(t) = sum_j G_j(t) an exact integer
 *   coef[k,t,b] = 0 for t >= T_b.  In exact arithmetic coef[k,0,b] is pgasr_pg_rewards_multi's pg_coef[k,b]; the leave-one-out
 *   coefficients of a frame sum to 0 over k.  Either baseline is a function of the OTHER rows at the same frame, so the estimator
 *   stays unbiased.
 *   objective  = sum_b nll_b utt_scale_b - sum_k sum_b sum_{t<T_b} coef[k,t,b] log p(pi_k[t,b])      (+ the entropy and KL terms)
 *   d(logits)[t,b,:] = utt_scale_b (softmax - occupancy) + sum_k coef[k,t,b] (softmax - onehot(pi_k[t,b])) in k order, then the
 *   entropy tail, then the KL tail.  R_sample, R_baseline and utt_scale come from pgasr_pg_rewards_multi as in any multi-sample call;
 *   its (K,B) coefficients are not used.
 *
 * pgasr_pg_step_coefs_multi: paths (P,T,B) int32 frame labels; prefix_dist (P*B, prefix_stride) and token_lengths (P*B) int32 of
 *   their collapsed forms, row w*B + b; coef (K,T,B) fp32, every word written.  One workgroup of 16 waves per utterance, each wave a
 *   64-frame chunk of a 1024-frame pass: per (row, chunk) start counts by ballot, one scan per row for the carries, then each lane
 *   forms all K coefficients of its frame from the P integers it holds.  Deterministic.  With K = 1 and the hypothesis baseline
 *   the output is pgasr_pg_step_coefs' (T,B) words bit for bit.  Checked before any launch: a NULL pointer, T or B <= 0,
 *   prefix_stride < 1, blank < 0, K outside 1..PGASR_MAX_SAMPLES, an unknown baseline, leave one out with K < 2 ->
 *   PGASR_ERR_INVALID_ARG.
 * pgasr_ctc_grad_from_lattice_multi_steps: pgasr_ctc_grad_from_lattice_multi[_ent,_kl] and _multi_wide with pg_coef (K,T,B), read
 *   at k*T*B + t*B + b: ONE entry for 1 <= V <= 1024 with nullable tails, on the workspace of pgasr_ctc_loss_grad or
 *   pgasr_ctc_loss_grad_wide.  V <= 64 runs the narrow kernels' body, V > 64 the wide kernels' -- a compile-time switch of each,
 *   so coefficients that are constant over t give the per-utterance entries' bits, and K = 1 without tails at V <= 64 gives
 *   pgasr_ctc_grad_from_lattice's with pg_coef_per_frame.  Argument checks and codes of pgasr_ctc_grad_from_lattice_multi_wide.
 * pgasr_pg_loss_value_multi_steps: terms[b] = nll[b]*utt_scale[b] - sum_k sum_{t<input_lengths[b]} pg_coef[k,t,b] *
 *   log_probs[t,b,paths[k,t,b]]; each path's sum in pgasr_pg_loss_value's fixed per-frame order, the K sums added in k order.  Any V.
 * ---------------------------------------------------------------------------------------- */
int pgasr_pg_step_coefs_multi(const int32_t* paths, const int32_t* input_lengths, const int32_t* prefix_dist, int prefix_stride,
                              const int32_t* token_lengths, const int32_t* target_lengths, int T, int B, int K, int baseline,
                              int blank, float lam, float inv_global_batch, float* coef, void* stream);
int pgasr_ctc_grad_from_lattice_multi_steps(const float* log_probs, const int32_t* input_lengths,
                                            const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                            const float* utt_scale, int K, const float* pg_coef /* (K,T,B) */,
                                            const int32_t* pg_paths, const float* ent_scale /* may be NULL */,
                                            const float* ref_log_probs /* may be NULL */, const float* kl_scale /* may be NULL */,
                                            float* grad_logits, void* workspace, size_t workspace_bytes, void* stream);
int pgasr_pg_loss_value_multi_steps(const float* log_probs, const int32_t* paths, int K, const int32_t* input_lengths,
                                    const float* nll, const float* utt_scale, const float* pg_coef /* (K,T,B) */,
                                    int T, int B, int V, float* terms, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PGASR_HIP_H */
