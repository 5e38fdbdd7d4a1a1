"""ctypes binding of libpgasr_hip.so (the C ABI declared in include/pgasr_hip.h).

There is NO fallback: if the shared library is missing or a call returns a non-zero
status this module raises.  Nothing here imports ``oracle``.
"""
import ctypes as C
import os

# Import order matters: PyTorch bundles its own HIP runtime (torch/lib/libamdhip64.so).  Loading this
# library first would pull in the system ROCm runtime as well, and kernels launched through one
# runtime on memory/streams owned by the other fail.  With torch loaded first the library's
# libamdhip64.so.7 dependency resolves to the runtime torch already mapped: ONE runtime per process.
import torch  # noqa: F401  (must precede CDLL below)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PGASR_HIP_LIB", os.path.join(_HERE, "libpgasr_hip.so"))   # override: diagnostic builds

c_f32p = C.c_void_p   # device pointers travel as integers (tensor.data_ptr())
c_i32p = C.c_void_p
c_ptr = C.c_void_p

# The nine beam-search entries share their argument list piece by piece (include/pgasr_hip.h, A7-*)
_S_HEAD = [c_ptr, C.c_int, C.c_longlong, C.c_longlong, c_i32p] + [C.c_int] * 6   # log_probs, is_f64, strides, lengths, T, B, V, beam, blank, flags
_S_BEST = [c_i32p, c_i32p, c_ptr]                                    # out_tokens, out_len, out_score
_S_LIST = [C.c_int, c_i32p, C.c_int, c_i32p, c_ptr, c_i32p]          # nbest, out_tokens, tok_stride, out_len, out_score, out_count
_S_WS = [c_ptr, C.c_size_t, c_ptr]                                   # workspace, workspace_bytes, stream
_S_LM = [c_f32p, C.c_int, C.c_double, C.c_double]                    # lm_table, lm_order, lm_alpha, lm_beta
_S_UNIT_LM = [c_ptr, C.c_double, C.c_double]                         # tables, lm_alpha, lm_beta
_S_BIAS = [c_ptr, C.c_int, C.c_double]                               # bias_table, bias_states, bias_weight
_S_WORDS = [c_ptr, C.c_int, c_i32p, c_ptr, C.c_int, C.c_double, C.c_double, C.c_int]   # trie, trie_states, node_word, tables, delimiter, alpha, beta, flags2
_S_WIDE = _S_HEAD + _S_LIST + [c_i32p] + _S_WS                       # ... out_counting_frames

# The CTC loss section's gradient, loss and hypothesis-lattice entries likewise (include/pgasr_hip.h, A5 / A12 / A13 and their -WIDE forms):
# head, one policy-gradient group, [the hypothesis group,] [the tails,] output + workspace(s) + stream
_G_HEAD = [c_f32p, c_i32p, c_i32p] + [C.c_int] * 5 + [c_f32p]        # log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale
_G_ONE = [c_f32p, c_i32p, C.c_int]                                   # pg_coef, pg_path, pg_coef_per_frame
_G_MULTI = [C.c_int, c_f32p, c_i32p]                                 # K, pg_coef, pg_paths
_G_NBEST = [C.c_int, c_f32p]                                         # N, coef
_G_HYP = [c_i32p, C.c_int]                                           # hyp_len, Lh
_G_ENT = [c_f32p]                                                    # ent_scale
_G_KL = [c_f32p, c_f32p, c_f32p]                                     # ent_scale (nullable), ref_log_probs, kl_scale
_G_OUT = [c_f32p] + _S_WS                                            # grad_logits, workspace, workspace_bytes, stream
_G_OUT2 = [c_f32p, c_ptr, C.c_size_t] + _S_WS                        # grad_logits, workspace, its bytes, hyp_workspace, its bytes, stream
_G_LOSS = [c_f32p, c_i32p] + _G_HEAD[1:] + [c_f32p, c_i32p, c_f32p] + _G_OUT       # log_probs, targets, <head>, pg_coef, pg_path, nll, <out>
_G_HYP_LATTICE = [c_f32p, c_i32p, C.c_int, c_i32p, c_i32p] + [C.c_int] * 6 + [c_f32p] + _S_WS   # log_probs, hyp_tokens, hyp_stride, hyp_len,
                                                                     # input_lengths, T, B, V, K, Lh, blank, hyp_nll, hyp_workspace, bytes, stream

# name -> (restype, argtypes).  Mirrors include/pgasr_hip.h one to one.
SIGNATURES = {
    "pgasr_abi_version": (C.c_int, []),
    "pgasr_status_string": (C.c_char_p, [C.c_int]),
    "pgasr_ctc_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "pgasr_ctc_loss_grad": (C.c_int, _G_LOSS),
    "pgasr_ctc_grad_from_lattice": (C.c_int, _G_HEAD + _G_ONE + _G_OUT),
    "pgasr_pg_rewards": (C.c_int, [c_i32p, c_i32p, C.c_int, C.c_float, C.c_float, c_f32p, c_f32p, c_f32p, c_f32p, c_ptr]),
    "pgasr_pg_loss_value": (C.c_int, [c_f32p, c_i32p, c_i32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      c_f32p, c_ptr]),
    "pgasr_head_logsoftmax": (C.c_int, [c_f32p, C.c_longlong, C.c_int, C.c_int, c_f32p, c_f32p, C.c_int, c_f32p, c_f32p, c_ptr]),
    "pgasr_pg_step_coefs": (C.c_int, [c_i32p, c_i32p, c_i32p, C.c_int, c_i32p, c_i32p, C.c_int, C.c_int, C.c_int,
                                      C.c_float, C.c_float, c_f32p, c_ptr]),
    "pgasr_frame_argmax_sample": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_int, C.c_int,
                                            c_i32p, c_i32p, c_ptr]),
    "pgasr_frame_sample_multi": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_int, C.c_int,
                                           c_i32p, c_i32p, c_ptr]),
    "pgasr_frame_argmax_sample_ids": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_int, c_i32p,
                                                c_i32p, c_i32p, c_ptr]),
    "pgasr_frame_sample_multi_ids": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_int, c_i32p,
                                               c_i32p, c_i32p, c_ptr]),
    "pgasr_ctc_grad_from_lattice_multi": (C.c_int, _G_HEAD + _G_MULTI + _G_OUT),
    "pgasr_pg_rewards_multi": (C.c_int, [c_i32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, c_f32p, c_f32p, c_f32p,
                                         c_f32p, c_ptr]),
    "pgasr_pg_loss_value_multi": (C.c_int, [c_f32p, c_i32p, C.c_int, c_i32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int,
                                            c_f32p, c_ptr]),
    "pgasr_ctc_hyp_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "pgasr_ctc_hyp_lattice": (C.c_int, _G_HYP_LATTICE),
    "pgasr_ctc_hyp_score": (C.c_int, [c_f32p, c_i32p, C.c_int, c_i32p, c_i32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, c_ptr, c_ptr]),
    "pgasr_ctc_grad_from_lattices_seq": (C.c_int, _G_HEAD + _G_MULTI + _G_HYP + _G_OUT2),
    "pgasr_pg_loss_value_seq": (C.c_int, [c_f32p, c_i32p, C.c_int, c_i32p, c_f32p, c_f32p, c_f32p, c_f32p, c_i32p, C.c_int,
                                          C.c_int, C.c_int, C.c_int, c_f32p, c_ptr]),
    "pgasr_frame_entropy": (C.c_int, [c_f32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, c_f32p, c_f32p, c_ptr]),
    "pgasr_ctc_grad_from_lattice_ent": (C.c_int, _G_HEAD + _G_ONE + _G_ENT + _G_OUT),
    "pgasr_ctc_grad_from_lattice_multi_ent": (C.c_int, _G_HEAD + _G_MULTI + _G_ENT + _G_OUT),
    "pgasr_ctc_grad_from_lattices_seq_ent": (C.c_int, _G_HEAD + _G_MULTI + _G_HYP + _G_ENT + _G_OUT2),
    "pgasr_ctc_align_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "pgasr_ctc_forced_align": (C.c_int, [c_f32p, c_i32p, c_i32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         c_ptr, c_i32p, c_i32p, c_i32p, c_i32p, c_ptr, c_ptr, C.c_size_t, c_ptr]),
    "pgasr_frame_kl": (C.c_int, [c_f32p, c_f32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, c_f32p, c_f32p, c_ptr]),
    "pgasr_ctc_grad_from_lattice_kl": (C.c_int, _G_HEAD + _G_ONE + _G_KL + _G_OUT),
    "pgasr_ctc_grad_from_lattice_multi_kl": (C.c_int, _G_HEAD + _G_MULTI + _G_KL + _G_OUT),
    "pgasr_ctc_grad_from_lattices_seq_kl": (C.c_int, _G_HEAD + _G_MULTI + _G_HYP + _G_KL + _G_OUT2),
    "pgasr_word_ids": (C.c_int, [c_i32p, c_i32p, C.c_int, c_i32p, c_i32p, C.c_int, C.c_int, C.c_int, c_i32p, c_i32p, c_i32p, c_i32p,
                                 c_ptr]),
    "pgasr_pg_rewards_multi_ex": (C.c_int, [c_i32p, c_i32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, c_f32p, c_f32p,
                                            c_f32p, c_f32p, c_ptr]),
    "pgasr_unit_spell": (C.c_int, [c_i32p, c_i32p, C.c_int, C.c_int, c_i32p, c_i32p, C.c_int, c_i32p, C.c_int, c_i32p, c_i32p, c_ptr]),
    "pgasr_batch_prep": (C.c_int, [c_f32p, C.c_int, C.c_int, c_ptr, c_ptr, C.c_int, c_i32p, c_i32p, c_i32p, c_ptr]),
    "pgasr_ctc_collapse": (C.c_int, [c_i32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_int, c_i32p, c_i32p, c_ptr]),
    "pgasr_edit_distance": (C.c_int, [c_i32p, c_i32p, C.c_int, c_i32p, c_i32p, C.c_int, C.c_int,
                                      c_i32p, c_i32p, c_ptr]),
    "pgasr_edit_ops_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "pgasr_edit_ops": (C.c_int, [c_i32p, c_i32p, C.c_int, c_i32p, c_i32p, C.c_int, C.c_int,
                                 c_i32p, c_ptr, c_i32p, c_ptr, C.c_int, c_ptr, C.c_size_t, c_ptr]),
    "pgasr_edit_ops_slot_mass": (C.c_int, [c_ptr, c_i32p, C.c_int, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int,
                                           c_ptr, c_i32p, c_i32p, c_ptr]),
    "pgasr_reinforce_grad": (C.c_int, [c_f32p, c_i32p, c_f32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                       c_f32p, c_ptr]),
    "pgasr_beam_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "pgasr_ctc_beam_search": (C.c_int, _S_HEAD + _S_BEST + _S_WS),
    "pgasr_ctc_beam_search_lm": (C.c_int, _S_HEAD + _S_BEST + _S_WS + _S_LM),
    "pgasr_beam_lm_single_wave_ok": (C.c_int, [C.c_int] * 5),
    "pgasr_ctc_beam_search_nbest": (C.c_int, _S_HEAD + _S_LIST + _S_WS + _S_LM),
    "pgasr_ctc_beam_search_bias": (C.c_int, _S_HEAD + _S_BEST + _S_WS + _S_LM + _S_BIAS),
    "pgasr_ctc_beam_search_nbest_bias": (C.c_int, _S_HEAD + _S_LIST + _S_WS + _S_LM + _S_BIAS),
    "pgasr_ctc_beam_search_words": (C.c_int, _S_HEAD + _S_LIST + _S_WS + _S_LM + _S_WORDS),
    "pgasr_nbest_bias_score": (C.c_int, [c_i32p, c_i32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr, C.c_int, c_ptr, c_ptr]),
    "pgasr_beam_wide_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "pgasr_ctc_beam_search_wide": (C.c_int, _S_WIDE),
    "pgasr_beam_wide_lm_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "pgasr_ctc_beam_search_wide_lm": (C.c_int, _S_WIDE + _S_UNIT_LM),
    "pgasr_ctc_beam_search_wide_bias": (C.c_int, _S_WIDE + _S_UNIT_LM + _S_BIAS),
    "pgasr_nbest_unit_lm_score": (C.c_int, [c_i32p, C.c_int, c_i32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr, c_ptr,
                                            c_ptr]),
    "pgasr_nbest_rescore": (C.c_int, [c_i32p, C.c_int, c_i32p, c_i32p, c_ptr, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, C.c_int,
                                      C.c_double, C.c_double, C.c_double, c_ptr, c_ptr, c_i32p, c_ptr]),
    "pgasr_nbest_pair_dist": (C.c_int, [c_i32p, C.c_int, c_i32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_int, c_i32p, c_ptr]),
    "pgasr_mbr_select": (C.c_int, [c_i32p, c_ptr, c_i32p, C.c_int, C.c_int, C.c_double, c_ptr, c_ptr, c_i32p, c_ptr]),
    "pgasr_nbest_word_lm_score": (C.c_int, [c_i32p, C.c_int, c_i32p, c_i32p, C.c_int, C.c_int, C.c_int, c_ptr, c_ptr, c_i32p, c_i32p,
                                            c_ptr]),
    "pgasr_nbest_combine_rank": (C.c_int, [c_ptr, c_ptr, c_i32p, c_i32p, C.c_int, C.c_int, C.c_double, C.c_double, c_ptr, c_i32p,
                                           c_ptr]),
    "pgasr_mwer_weights": (C.c_int, [c_i32p, c_i32p, c_i32p, c_f32p, c_i32p, c_i32p, c_f32p, C.c_int, C.c_int, C.c_int,
                                     C.c_float, C.c_float, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_ptr]),
    "pgasr_ctc_grad_from_lattices_nbest": (C.c_int, _G_HEAD + _G_NBEST + _G_HYP + _G_OUT2),
    "pgasr_dropout": (C.c_int, [c_f32p, c_f32p, C.c_ulonglong, C.c_float, C.c_uint64, C.c_uint32, c_f32p, C.c_float, c_ptr]),
    "pgasr_spec_augment": (C.c_int, [c_f32p, c_i32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_float, C.c_int, C.c_ulonglong, C.c_uint, c_f32p, c_i32p, c_ptr]),
    "pgasr_frame_stack": (C.c_int, [c_f32p, c_i32p] + [C.c_int] * 7 + [c_f32p, c_f32p, c_i32p, c_ptr]),
    "pgasr_resample": (C.c_int, [c_f32p, C.c_int, c_i32p, C.c_int, c_i32p, C.c_int, c_ptr, c_f32p, c_i32p, c_f32p, C.c_int, c_i32p,
                                 c_ptr]),
    "pgasr_reverb_limits": (C.c_int, [C.POINTER(C.c_int)] * 3),
    "pgasr_reverb": (C.c_int, [c_f32p, C.c_int, c_i32p, C.c_int, c_f32p, C.c_int, C.c_int, c_i32p, c_i32p, c_i32p, c_f32p, c_ptr]),
    "pgasr_wave_power": (C.c_int, [c_f32p, C.c_int, C.c_int, c_i32p, C.c_int, c_i32p, c_i32p, c_i32p, c_ptr, c_ptr]),
    "pgasr_wave_mix": (C.c_int, [c_f32p, C.c_int, c_i32p, C.c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_f32p, C.c_int, C.c_int,
                                 c_i32p, c_i32p, c_i32p, c_f32p, C.c_int, c_f32p, c_ptr]),
    "pgasr_stream_copy": (C.c_int, [c_ptr, c_ptr, C.c_ulonglong, C.c_int, c_ptr]),
    "pgasr_adam_step": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_ulonglong, C.c_int, C.c_float, C.c_float,
                                  C.c_float, C.c_float, C.c_float, c_i32p, c_i32p, c_i32p, c_ptr]),
    "pgasr_adam_step_clipped": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, C.c_ulonglong, C.c_int, C.c_float, C.c_float,
                                          C.c_float, C.c_float, C.c_float, c_i32p, c_i32p, c_i32p, c_ptr, c_ptr]),
    "pgasr_grad_norm_ws_bytes": (C.c_size_t, [C.c_ulonglong]),
    "pgasr_grad_norm_clip": (C.c_int, [c_f32p, C.c_ulonglong, C.c_float, c_ptr, C.c_size_t, c_ptr, c_ptr]),
    "pgasr_gemm_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "pgasr_gemm_f32": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                 c_f32p, C.c_int, C.c_longlong, c_f32p, C.c_int, C.c_longlong,
                                 c_f32p, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                 c_f32p, c_f32p, C.c_int, C.c_float, C.c_int,
                                 c_f32p, C.c_int, c_f32p, c_f32p, C.c_int, c_ptr, c_ptr, C.c_size_t, c_ptr]),
    "pgasr_split_bf16_planes": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr, c_ptr, c_ptr]),
    "pgasr_gemm_x3w_f32": (C.c_int, [C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, c_ptr, c_ptr, c_f32p, C.c_int,
                                     c_f32p, c_f32p, C.c_float, c_ptr]),
    "pgasr_gemm_x3w_feed_workspace_bytes": (C.c_size_t, []),
    "pgasr_gemm_x3w_feed_col_tiles": (C.c_int, [C.c_int]),
    "pgasr_gemm_x3w_feed_head_items": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "pgasr_gemm_x3w_feed_f32": (C.c_int, [C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, c_ptr, c_ptr, c_f32p, C.c_int,
                                          c_f32p, c_ptr, c_ptr, C.c_int, C.c_int, C.c_int, c_ptr, C.c_size_t, c_ptr]),
    "pgasr_feat_frames": (C.c_int, [c_f32p, c_i32p, c_i32p, C.c_int, C.c_longlong, C.c_int, c_f32p, c_ptr]),
    "pgasr_feat_power": (C.c_int, [c_f32p, C.c_longlong, c_f32p, c_ptr]),
    "pgasr_feat_db": (C.c_int, [c_f32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_float, c_ptr]),
    "pgasr_feat_deltas_stack": (C.c_int, [c_f32p, c_i32p, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_ptr]),
    "pgasr_feat_stack": (C.c_int, [c_f32p, c_i32p, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_ptr]),
    "pgasr_colsum_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "pgasr_colsum_f32": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, C.c_int,
                                   c_ptr, C.c_size_t, c_ptr]),
    "pgasr_instnorm_stats": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_float, c_f32p, c_f32p, c_ptr]),
    "pgasr_log_softmax_rows": (C.c_int, [c_f32p, C.c_longlong, C.c_int, c_f32p, c_ptr]),
    "pgasr_log_softmax_rows_wide": (C.c_int, [c_f32p, C.c_longlong, C.c_int, c_f32p, c_ptr]),
    "pgasr_frame_argmax_sample_wide": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_int, C.c_int,
                                                 c_i32p, c_i32p, c_i32p, c_ptr]),
    "pgasr_ctc_loss_grad_wide": (C.c_int, _G_LOSS),
    "pgasr_ctc_grad_from_lattice_wide": (C.c_int, _G_HEAD + _G_ONE + _G_OUT),
    "pgasr_frame_sample_multi_wide": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_int, C.c_int,
                                                c_i32p, c_i32p, c_i32p, c_ptr]),
    "pgasr_frame_entropy_wide": (C.c_int, [c_f32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, c_f32p, c_f32p, c_ptr]),
    "pgasr_frame_kl_wide": (C.c_int, [c_f32p, c_f32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, c_f32p, c_f32p,
                                      c_ptr]),
    "pgasr_ctc_grad_from_lattice_multi_wide": (C.c_int, _G_HEAD + _G_MULTI + _G_KL + _G_OUT),
    "pgasr_ctc_hyp_workspace_bytes_wide": (C.c_size_t, [C.c_int] * 5),
    "pgasr_ctc_hyp_lattice_wide": (C.c_int, _G_HYP_LATTICE),
    "pgasr_ctc_grad_from_lattices_seq_wide": (C.c_int, _G_HEAD + _G_MULTI + _G_HYP + _G_KL + _G_OUT2),
    "pgasr_pg_step_coefs_multi": (C.c_int, [c_i32p, c_i32p, c_i32p, C.c_int, c_i32p, c_i32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_float, C.c_float, c_f32p, c_ptr]),
    "pgasr_ctc_grad_from_lattice_multi_steps": (C.c_int, _G_HEAD + _G_MULTI + _G_KL + _G_OUT),
    "pgasr_pg_loss_value_multi_steps": (C.c_int, [c_f32p, c_i32p, C.c_int, c_i32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int,
                                                  C.c_int, c_f32p, c_ptr]),
    "pgasr_lstm_pack_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "pgasr_lstm_pack_weights": (C.c_int, [c_f32p] * 8 + [C.c_int, c_f32p, c_f32p, c_ptr, c_ptr, C.c_int, c_ptr]),
    "pgasr_lstm_unpack_grads": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int] + [c_f32p] * 8 + [C.c_int, c_ptr]),
    "pgasr_lstm_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "pgasr_lstm_error_offset": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "pgasr_lstm_busy_offset": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "pgasr_lstm_status": (C.c_int, [c_ptr, C.c_size_t, C.c_int, C.c_int, c_ptr]),
    "pgasr_stream_gate": (C.c_int, [c_ptr, C.c_int, C.c_int, c_ptr]),
    "pgasr_stream_gate_sum": (C.c_int, [c_ptr, C.c_int, C.c_int, c_ptr, C.c_int, c_ptr]),
    "pgasr_stream_gate_report": (C.c_int, [c_ptr, C.c_int, C.c_int, c_ptr, C.c_int, c_ptr, c_ptr]),
    "pgasr_stream_probe": (C.c_int, [c_ptr, C.c_int, c_ptr]),
    "pgasr_lstm_layer_fwd": (C.c_int, [c_f32p, c_f32p, c_f32p, c_ptr, c_i32p, C.c_int, C.c_int, C.c_int,
                                       c_f32p, C.c_float, C.c_uint64, C.c_uint32, c_ptr, C.c_size_t, c_ptr]),
    "pgasr_lstm_layer_fwd_fed": (C.c_int, [c_f32p, c_f32p, c_f32p, c_ptr, c_i32p, C.c_int, C.c_int, C.c_int, c_ptr, C.c_int,
                                           c_f32p, C.c_float, C.c_uint64, C.c_uint32, c_ptr, C.c_size_t, c_ptr]),
    "pgasr_lstm_fed_ok": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "pgasr_lstm_layer_bwd_fed": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_ptr, c_i32p, C.c_int, C.c_int, C.c_int,
                                           c_f32p, c_ptr, C.c_int, C.c_float, C.c_uint64, C.c_uint32, c_ptr, C.c_size_t, c_ptr]),
    "pgasr_lstm_layer_bwd": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_ptr, c_i32p, C.c_int, C.c_int, C.c_int,
                                       c_f32p, c_ptr, C.c_size_t, c_ptr]),
    "pgasr_lstm_wgrad_slabs": (C.c_int, [C.c_int, c_i32p, C.c_int]),
    "pgasr_lstm_layer_bwd_streamed": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_ptr, c_i32p, C.c_int, C.c_int, C.c_int,
                                                c_f32p, c_ptr, C.c_int, C.c_float, C.c_uint64, C.c_uint32, c_ptr,
                                                c_ptr, C.c_size_t, c_ptr]),
    "pgasr_lstm_wgrads_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "pgasr_lstm_wgrads_streamed": (C.c_int, [c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, c_f32p, c_f32p, c_ptr,
                                             c_ptr, c_ptr, C.c_int, c_ptr, C.c_size_t, c_ptr]),
    "pgasr_error_flag": (C.c_int, [c_i32p, c_i32p, c_f32p, c_ptr]),
    "pgasr_attention_ctx": (C.c_int, [c_f32p, c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_f32p, c_ptr]),
    "pgasr_lstm_cell_f32": (C.c_int, [c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, C.c_int, C.c_int, c_ptr]),
    "pgasr_pack_x6w_planes": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr, c_ptr]),
    "pgasr_split_bf16_planes3": (C.c_int, [c_f32p, C.c_int, C.c_int, C.c_int, C.c_int, c_ptr, c_ptr, c_ptr, c_ptr]),
    "pgasr_gemm_x6w_f32": (C.c_int, [C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, c_ptr, c_ptr, c_ptr, c_f32p, C.c_int,
                                     c_f32p, c_f32p, C.c_float, c_ptr]),
    "pgasr_gemm_x6w_feed_workspace_bytes": (C.c_size_t, []),
    "pgasr_gemm_x6w_feed_col_tiles": (C.c_int, [C.c_int]),
    "pgasr_gemm_x6w_feed_f32": (C.c_int, [C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, c_ptr, c_ptr, c_ptr, c_f32p, C.c_int,
                                          c_f32p, c_ptr, c_ptr, C.c_int, c_ptr, C.c_size_t, c_ptr]),
    "pgasr_gemm_x6w_feed_head_items": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "pgasr_gemm_x6w_feed_phase_f32": (C.c_int, [C.c_int, C.c_int, C.c_int, c_f32p, C.c_int, c_ptr, c_ptr, c_ptr, c_f32p, C.c_int,
                                                c_f32p, c_ptr, c_ptr, C.c_int, C.c_int, c_ptr, c_ptr, C.c_size_t, c_ptr]),
}


class WordLMTables(C.Structure):
    """pgasr_word_lm_tables (include/pgasr_hip.h, A7-WORDLM): device addresses and sizes, a host struct passed with C.byref."""
    _fields_ = [("word_pool", C.c_void_p), ("word_off", C.c_void_p), ("word_slots", C.c_void_p), ("uni_logp", C.c_void_p),
                ("uni_bow", C.c_void_p), ("ngram_slots", C.c_void_p), ("order", C.c_int32), ("n_words", C.c_int32),
                ("word_cap", C.c_int32), ("ngram_cap", C.c_int32), ("pool_bytes", C.c_int32), ("reserved", C.c_int32)]


class UnitLMTables(C.Structure):
    """pgasr_unit_lm_tables (include/pgasr_hip.h, A7-WIDE-LM): device addresses and sizes, a host struct passed with C.byref."""
    _fields_ = [("states", C.c_void_p), ("succ", C.c_void_p), ("order", C.c_int32), ("vocab", C.c_int32), ("blank", C.c_int32),
                ("n_states", C.c_int32), ("n_succ", C.c_int32), ("start", C.c_int32)]


class PgasrError(RuntimeError):
    pass


TIMEOUT = 5     # PGASR_ERR_TIMEOUT


_lib = None


def load():
    """Load the library once; raise (never fall back) if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PgasrError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C policy_gradient_asr_amd/csrc`.  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.pgasr_abi_version() != 7:
        raise PgasrError("libpgasr_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        msg = load().pgasr_status_string(status).decode()
        raise PgasrError(f"{what} failed: status {status} ({msg})")
