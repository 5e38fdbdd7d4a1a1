// Per-step rewards with K sampled paths (include/pgasr_hip.h, A12-STEP): the per-frame coefficients of the multi-sample REINFORCE
// term (pgasr_pg_step_coefs_multi) and the value of that objective (pgasr_pg_loss_value_multi_steps).  The gradient pass that
// consumes the coefficients is ctc.hip's (pgasr_ctc_grad_from_lattice_multi_steps).
#include "common.h"

namespace {

// Path rows of utterance b: [greedy (hypothesis baseline only), sample 0, .., sample K-1], P = K + 1 or K of them.  Row w has the
// collapsed length n_w and the per-prefix distances D_w[i] = ED(y_b, yhat_w[:i]); a character starts at frame t when t < T_b, the
// label is not blank and (t = 0 or the label differs from the one before); c_w(t) = starts at frames < t, clipped to n_w;
//   G_w(t) = D_w[c_w(t)] - D_w[n_w]                                                      an integer
//   kf_b   = ((lam * inv_bg) / K) / max(L_b,1)                                           fp32, in this order
//   coef[k,t,b] = kf_b * (G_k(t) - G_greedy(t))                                          hypothesis
//               = kf_b * (G_k(t) - (S(t) - G_k(t)) / (K-1)),  S(t) = sum_j G_j(t)        leave one out; S an exact integer
// and 0 for t >= T_b.  pg_step_coef_kernel walks T in 64-frame chunks with one wave and a serial carry per row; with up to 17 rows
// that chain would be 8 times its length.  Here an utterance has a workgroup of STEP_WAVES waves and wave v takes frames
// t0 + 64 v .. t0 + 64 v + 63 of a pass (t0 = 0, STEP_SPAN, ..): per row one ballot gives the lane's count of starts before it in
// the chunk and the chunk's total, the totals go to LDS, P threads turn them into exclusive offsets (one scan of STEP_WAVES
// entries per row, carrying the running total into the next pass), and then every lane holds the P integers G_w(t) of ITS frame
// in registers (loops over rows unrolled to STEP_PMAX under a uniform guard: no scratch), forms S(t) and stores the K
// coefficients of the frame.  coef is (K,T,B) and a workgroup owns one b, so a wave's store covers 64 frames of one utterance,
// B floats apart, as pg_step_coef_kernel's does; the B workgroups of a frame fill its B-float line between them.
constexpr int STEP_WAVES = 16;
constexpr int STEP_SPAN = 64 * STEP_WAVES;               // frames a workgroup covers in one pass
constexpr int STEP_PMAX = PGASR_MAX_SAMPLES + 1;         // path rows: the greedy row and K samples

template <bool LOO>
__global__ __launch_bounds__(64 * STEP_WAVES) void pg_step_coefs_multi_kernel(
    const int32_t* __restrict__ paths, const int32_t* __restrict__ in_len, const int32_t* __restrict__ prefix, int pstride,
    const int32_t* __restrict__ tok_len, const int32_t* __restrict__ tg_len, int T, int B, int K, int blank, float lam, float inv_bg,
    float* __restrict__ coef) {
    __shared__ int cnt[STEP_PMAX][STEP_WAVES];      // starts of (row, chunk) in this pass, then the starts before the chunk
    __shared__ int run[STEP_PMAX];                  // starts of the row in earlier passes
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int P = LOO ? K : K + 1;
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    const int L = tg_len[b];
    const float kf = ((lam * inv_bg) / (float)K) / (float)(L > 1 ? L : 1);
    const size_t TB = (size_t)T * B;
    if (tid < STEP_PMAX) run[tid] = 0;
    for (int t0 = 0; t0 < T; t0 += STEP_SPAN) {
        const int t = t0 + tid;
        int c[STEP_PMAX];
#pragma unroll
        for (int w = 0; w < STEP_PMAX; ++w) {
            c[w] = 0;
            if (w < P) {
                const int32_t* p = paths + (size_t)w * TB;
                const int cur = t < Tb ? p[(size_t)t * B + b] : blank;
                const int prev = (t > 0 && t < Tb) ? p[(size_t)(t - 1) * B + b] : blank;
                const bool start = t < Tb && cur != blank && (t == 0 || cur != prev);
                const unsigned long long m = __ballot(start);
                c[w] = __popcll(m & ((1ull << lane) - 1ull));
                if (lane == 0) cnt[w][wv] = __popcll(m);
            }
        }
        __syncthreads();
        if (tid < P) {
            int r = run[tid];
#pragma unroll
            for (int i = 0; i < STEP_WAVES; ++i) {
                const int x = cnt[tid][i];
                cnt[tid][i] = r;
                r += x;
            }
            run[tid] = r;
        }
        __syncthreads();
        int G[STEP_PMAX], S = 0;
#pragma unroll
        for (int w = 0; w < STEP_PMAX; ++w) {
            G[w] = 0;
            if (w < P) {
                const int32_t* pd = prefix + ((size_t)w * B + b) * pstride;
                int n = tok_len[(size_t)w * B + b];
                n = n < 0 ? 0 : (n > pstride - 1 ? pstride - 1 : n);
                int cc = cnt[w][wv] + c[w];
                cc = cc > n ? n : cc;
                G[w] = pd[cc] - pd[n];
                S += G[w];
            }
        }
        if (t < T) {
#pragma unroll
            for (int k = 0; k < PGASR_MAX_SAMPLES; ++k) {
                if (k < K) {
                    float v = 0.f;
                    if (t < Tb) {
                        if (LOO) {
                            const float g = (float)G[k];
                            v = kf * (g - (float)(S - G[k]) / (float)(K - 1));
                        } else {
                            v = kf * ((float)G[k + 1] - (float)G[0]);
                        }
                    }
                    coef[(size_t)k * TB + (size_t)t * B + b] = v;
                }
            }
        }
        __syncthreads();      // the next pass overwrites cnt
    }
}

// Value of the per-step multi-sample objective per utterance:
//   terms[b] = nll_b utt_scale_b - sum_k sum_{t < T_b} coef[k,t,b] log p(paths[k,t,b])
// pg_loss_value_multi_kernel with (K,T,B) coefficients: per path block_path_logprob_sum's per-frame form in its fixed order, the K
// sums added in k order (deterministic).  Any V: it only addresses a row.
__global__ __launch_bounds__(256) void pg_loss_value_multi_steps_kernel(const float* __restrict__ lp, const int32_t* __restrict__ paths,
                                                                        int K, const int32_t* __restrict__ in_len,
                                                                        const float* __restrict__ nll, const float* __restrict__ utt_scale,
                                                                        const float* __restrict__ coef, int T, int B, int V,
                                                                        float* __restrict__ terms) {
    __shared__ float red[256];
    const int b = blockIdx.x;
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    const size_t TB = (size_t)T * B;
    float acc = 0.f;
    for (int k = 0; k < K; ++k)
        acc += block_path_logprob_sum(lp, paths + (size_t)k * TB, coef + (size_t)k * TB, Tb, b, B, V, red);
    if (threadIdx.x == 0) terms[b] = nll[b] * utt_scale[b] - acc;
}

}  // namespace

extern "C" int pgasr_pg_step_coefs_multi(const int32_t* paths, const int32_t* input_lengths, const int32_t* prefix_dist,
                                         int prefix_stride, const int32_t* token_lengths, const int32_t* target_lengths, int T, int B,
                                         int K, int baseline, int blank, float lam, float inv_global_batch, float* coef, void* stream) {
    if (!paths || !input_lengths || !prefix_dist || !token_lengths || !target_lengths || !coef) return PGASR_ERR_INVALID_ARG;
    if (T <= 0 || B <= 0 || prefix_stride < 1 || blank < 0) return PGASR_ERR_INVALID_ARG;
    if (K < 1 || K > PGASR_MAX_SAMPLES) return PGASR_ERR_INVALID_ARG;
    if (baseline != PGASR_BASELINE_HYPOTHESIS && baseline != PGASR_BASELINE_LEAVE_ONE_OUT) return PGASR_ERR_INVALID_ARG;
    if (baseline == PGASR_BASELINE_LEAVE_ONE_OUT && K < 2) return PGASR_ERR_INVALID_ARG;
    if (baseline == PGASR_BASELINE_LEAVE_ONE_OUT)
        PGASR_LAUNCH_KERNEL(pg_step_coefs_multi_kernel<true>, dim3(B), dim3(64 * STEP_WAVES), 0, (hipStream_t)stream,
                           paths, input_lengths, prefix_dist, prefix_stride, token_lengths, target_lengths, T, B, K, blank, lam,
                           inv_global_batch, coef);
    else
        PGASR_LAUNCH_KERNEL(pg_step_coefs_multi_kernel<false>, dim3(B), dim3(64 * STEP_WAVES), 0, (hipStream_t)stream,
                           paths, input_lengths, prefix_dist, prefix_stride, token_lengths, target_lengths, T, B, K, blank, lam,
                           inv_global_batch, coef);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

extern "C" int pgasr_pg_loss_value_multi_steps(const float* log_probs, const int32_t* paths, int K, const int32_t* input_lengths,
                                               const float* nll, const float* utt_scale, const float* pg_coef,
                                               int T, int B, int V, float* terms, void* stream) {
    if (!log_probs || !paths || !pg_coef || !input_lengths || !nll || !utt_scale || !terms) return PGASR_ERR_INVALID_ARG;
    if (T <= 0 || B <= 0 || V <= 0 || K < 1 || K > PGASR_MAX_SAMPLES) return PGASR_ERR_INVALID_ARG;
    PGASR_LAUNCH_KERNEL(pg_loss_value_multi_steps_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream,
                       log_probs, paths, K, input_lengths, nll, utt_scale, pg_coef, T, B, V, terms);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
