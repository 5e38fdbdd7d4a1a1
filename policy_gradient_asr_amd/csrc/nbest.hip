// Second-pass rescoring of N-best lists on gfx950 (pgasr_nbest_rescore; semantics in include/pgasr_hip.h, section A7-RESCORE).
//
// One launch, one workgroup of four waves per utterance.  A wave takes hypotheses n = wave, wave + 4, .. of the utterance:
//   * the hypothesis is read 64 tokens at a time (one coalesced load of the wave) into the wave's own LDS strip, behind the last 32
//     tokens of the chunk before -- an n-gram context reaches back at most 24 symbols (V^n <= 2^25, V >= 2);
//   * lane i forms the table index of token i from the strip (lm.py's context rule: the last order-1 symbols, left-padded with
//     blank), gathers the fp32 word and adds it to its own fp64 partial sum; the 64 partial sums meet in a fixed butterfly;
//   * total = am_weight * am - lm_alpha * lm_logp - lm_beta * len with each product and each sum rounded once, in that order
//     (no contraction into fused multiply-adds), so tests/nbest_ref.py repeats it in numpy.
// Then thread n < N ranks hypothesis n among the utterance's totals in LDS: stable ascending, ties keep first-pass order.
// A few gathers per token and at most 128 x 128 compares per utterance: latency work, nothing for the matrix units.
#include "common.h"
#include <cmath>

namespace {

constexpr int NR_THREADS = 256;
constexpr int NR_WAVES = NR_THREADS / 64;
constexpr int NR_NMAX = 128;
constexpr int NR_VMAX = 64;                               // as the search (csrc/beam.hip)
constexpr long long NR_LM_MAX_ENTRIES = 1ll << 25;        // as the search: V^n <= 2^25 words
constexpr int NR_HIST = 32;                               // tokens of the previous chunk kept in front of the current one (order - 1 <= 24)

__global__ __launch_bounds__(NR_THREADS) void nbest_rescore_kernel(
    const int32_t* __restrict__ tokens, int tok_stride, const int32_t* __restrict__ len, const int32_t* __restrict__ count,
    const double* __restrict__ am, int N, int B, int V, int blank, const float* __restrict__ table, int order,
    double am_weight, double lm_alpha, double lm_beta, double* __restrict__ out_lm, double* __restrict__ out_total,
    int32_t* __restrict__ out_order) {
    __shared__ volatile int s_tok[NR_WAVES][NR_HIST + 64];
    __shared__ double s_total[NR_NMAX];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int cnt = count[b]; cnt = cnt < 0 ? 0 : (cnt > N ? N : cnt);

    for (int n = wave; n < N; n += NR_WAVES) {
        double lm_sum = 0.0, total = INFINITY;
        if (n < cnt) {                                     // wave-uniform
            int L = len[(size_t)n * B + b]; L = L < 0 ? 0 : (L > tok_stride ? tok_stride : L);
            const int32_t* tk = tokens + ((size_t)n * B + b) * tok_stride;
            double part = 0.0;
            bool bad = false;                              // a symbol outside [0, V): no table word to read
            if (order > 0) {
                if (lane < NR_HIST) s_tok[wave][lane] = blank;          // before the first token: the start pad
                for (int base = 0; base < L; base += 64) {
                    const int i = base + lane;
                    const int s = i < L ? tk[i] : blank;
                    s_tok[wave][NR_HIST + lane] = s;                    // DS operations of one wave execute in issue order
                    if (i < L) {
                        long long idx = 0;
                        bool ok = s >= 0 && s < V;
                        for (int k = order - 1; k >= 1; --k) {
                            const int c = s_tok[wave][NR_HIST + lane - k];
                            ok = ok && c >= 0 && c < V;
                            idx = idx * V + c;
                        }
                        idx = idx * V + s;
                        if (ok) part += (double)table[idx]; else bad = true;
                    }
                    const int carry = s_tok[wave][64 + lane % NR_HIST];      // the chunk's last 32 tokens become the history
                    if (lane < NR_HIST) s_tok[wave][lane] = carry;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
            bad = __any(bad);
            lm_sum = part;
            const double a = am[(size_t)n * B + b];
            if (!bad && std::isfinite(a)) {
                // Plain operators under contract(off), not __dmul_rn / __dadd_rn: this compiler inlines those as plain operators and then
                // fuses them into v_fma_f64 (HIP's default -ffp-contract=fast); the pragma, which works on the operators written in its
                // own block, is what keeps the five roundings of the statement.
#pragma clang fp contract(off)
                const double t1 = am_weight * a, t2 = lm_alpha * lm_sum, t3 = lm_beta * (double)L;
                total = (t1 + -t2) + -t3;
                if (total != total) total = INFINITY;
            }
            if (bad) lm_sum = -INFINITY;
        }
        if (lane == 0) {
            s_total[n] = total;
            out_lm[(size_t)n * B + b] = lm_sum;
            out_total[(size_t)n * B + b] = total;
        }
    }
    __syncthreads();
    if (tid < N) {
        int rank = tid;                                    // rows beyond count follow in index order
        if (tid < cnt) {
            const double mine = s_total[tid];
            rank = 0;
            for (int m = 0; m < cnt; ++m) {
                const double x = s_total[m];
                rank += (x < mine || (x == mine && m < tid)) ? 1 : 0;
            }
        }
        out_order[(size_t)b * N + rank] = tid;
    }
}

// MWER over an N-best list (pgasr_mwer_weights; semantics in include/pgasr_hip.h, section A13-MWER): the posterior over the list's valid
// entries from their exact CTC nll, the risks, the expected risk and the gradient coefficients.  One thread per utterance, fp64, the
// sums in n order: two calls give the same bits.  N <= PGASR_MAX_SAMPLES entries, read three times; nothing here is worth a wave.
__global__ __launch_bounds__(64) void mwer_weights_kernel(
    const int32_t* __restrict__ dist, const int32_t* __restrict__ risk_len, const int32_t* __restrict__ tg_len,
    const float* __restrict__ hyp_nll, const int32_t* __restrict__ hyp_len, const int32_t* __restrict__ count,
    const float* __restrict__ nll, int N, int B, int Lh, double lam, double inv_gb,
    float* __restrict__ p_out, float* __restrict__ r_out, float* __restrict__ coef, float* __restrict__ utt_scale,
    float* __restrict__ rbar_out, float* __restrict__ terms) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int cnt = count[b];
    const int rl = risk_len[b];
    const double den = (double)(rl > 1 ? rl : 1);
    unsigned valid = 0u;
    double m = INFINITY;
    for (int n = 0; n < N; ++n) {
        const size_t i = (size_t)n * B + b;
        const float h = hyp_nll[i];
        const bool ok = n < cnt && hyp_len[i] <= Lh && h == h && h != INFINITY && h != -INFINITY;
        if (ok) { valid |= 1u << n; m = fmin(m, (double)h); }
    }
    double z = 0.0;
    for (int n = 0; n < N; ++n)
        if (valid >> n & 1u) z += exp(-((double)hyp_nll[(size_t)n * B + b] - m));
    double rbar = 0.0;
    for (int n = 0; n < N; ++n) {
        const size_t i = (size_t)n * B + b;
        const double p = (valid >> n & 1u) ? exp(-((double)hyp_nll[i] - m)) / z : 0.0;
        const double r = (double)dist[i] / den;
        rbar += p * r;
        p_out[i] = (float)p;
        r_out[i] = (float)r;
    }
    for (int n = 0; n < N; ++n) {
        const size_t i = (size_t)n * B + b;
        const double p = (valid >> n & 1u) ? exp(-((double)hyp_nll[i] - m)) / z : 0.0;
        const double r = (double)dist[i] / den;
        coef[i] = (valid >> n & 1u) ? (float)(-lam * inv_gb * p * (r - rbar)) : 0.f;
    }
    const int L = tg_len[b];
    const float us = (float)inv_gb / (float)(L > 1 ? L : 1);      // as pgasr_pg_rewards leaves it
    utt_scale[b] = us;
    rbar_out[b] = (float)rbar;
    terms[b] = (float)((double)(nll[b] * us) + lam * inv_gb * rbar);       // the CTC part as pgasr_pg_loss_value forms it: one fp32 product
}

}  // namespace

extern "C" int pgasr_mwer_weights(const int32_t* dist, const int32_t* risk_len, const int32_t* target_lengths, const float* hyp_nll,
                                  const int32_t* hyp_len, const int32_t* count, const float* nll, int N, int B, int Lh,
                                  float lam, float inv_global_batch, float* p, float* r, float* coef, float* utt_scale,
                                  float* rbar, float* terms, void* stream) {
    if (!dist || !risk_len || !target_lengths || !hyp_nll || !hyp_len || !count || !nll) return PGASR_ERR_INVALID_ARG;
    if (!p || !r || !coef || !utt_scale || !rbar || !terms) return PGASR_ERR_INVALID_ARG;
    if (N < 1 || N > PGASR_MAX_SAMPLES || B <= 0 || Lh < 0) return PGASR_ERR_INVALID_ARG;
    if (!std::isfinite(lam) || !std::isfinite(inv_global_batch) || !(inv_global_batch > 0.f)) return PGASR_ERR_INVALID_ARG;
    PGASR_LAUNCH_KERNEL(mwer_weights_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, dist, risk_len, target_lengths,
                       hyp_nll, hyp_len, count, nll, N, B, Lh, (double)lam, (double)inv_global_batch, p, r, coef, utt_scale, rbar, terms);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

extern "C" int pgasr_nbest_rescore(const int32_t* tokens, int tok_stride, const int32_t* len, const int32_t* count, const double* am,
                                   int N, int B, int V, int blank, const float* lm_table, int lm_order,
                                   double am_weight, double lm_alpha, double lm_beta,
                                   double* out_lm_logp, double* out_total, int32_t* out_order, void* stream) {
    if (!tokens || !len || !count || !am || !out_lm_logp || !out_total || !out_order) return PGASR_ERR_INVALID_ARG;
    if (N < 1 || B <= 0 || V <= 0 || tok_stride < 1 || blank < 0 || blank >= V) return PGASR_ERR_INVALID_ARG;
    if (lm_order < 0 || (lm_order > 0) != (lm_table != nullptr)) return PGASR_ERR_INVALID_ARG;
    if (!std::isfinite(am_weight) || !std::isfinite(lm_alpha) || !std::isfinite(lm_beta)) return PGASR_ERR_INVALID_ARG;
    if (N > NR_NMAX || V > NR_VMAX) return PGASR_ERR_UNSUPPORTED;
    long long entries = 1;
    for (int k = 0; k < lm_order; ++k) {
        entries *= V;
        if (entries > NR_LM_MAX_ENTRIES) return PGASR_ERR_UNSUPPORTED;      // refused, never truncated
    }
    if (lm_order - 1 > NR_HIST - 8) return PGASR_ERR_UNSUPPORTED;           // the history strip; V >= 2 bounds the order by 25 already
    PGASR_LAUNCH_KERNEL(nbest_rescore_kernel, dim3(B), dim3(NR_THREADS), 0, (hipStream_t)stream, tokens, tok_stride, len, count, am,
                       N, B, V, blank, lm_table, lm_order, am_weight, lm_alpha, lm_beta, out_lm_logp, out_total, out_order);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
