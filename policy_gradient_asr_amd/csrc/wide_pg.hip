// The policy-gradient row kernels for alphabets of up to 1024 symbols on gfx950 (header section A12-WIDE): K inverse-CDF draws per
// (t,b) row, and the per-utterance entropy and KL statistics of the frame policy.  Rows are held as in wide_vocab.hip: one wave per
// row, lane l owning the NV consecutive labels l*NV .. l*NV + NV - 1 (wide_rows.h).  Every reduction is a sequential pass over the
// lane's own values in label order followed by ONE wave butterfly or scan of the 64 lane results, and frames are added in t order:
// a fixed order, so two calls give the same bits.  With NV = 1 the operations are those of frame_sample_multi_kernel,
// frame_entropy_kernel and frame_kl_kernel, one for one.  (The multi-sample gradient pass of this section lives in ctc.hip, beside
// the workspace it reads.)
#include "wide_rows.h"

namespace {

// frame_sample_multi_kernel for wide rows.  The row's maximum, inclusive cdf and total are frame_argmax_sample_wide_kernel's and are
// formed once; lane j < K runs the Philox block of draw j (counter word 3 = j), and each draw is resolved against the same cdf by
// NV ballots -- the count is an integer, so its order does not matter.  Draw 0's counter, u, threshold and count are those of
// frame_argmax_sample_wide_kernel: its sample bit for bit.
template <int NV>
__global__ __launch_bounds__(256) void frame_sample_multi_wide_kernel(
    const float* __restrict__ scores, long long rows, int B, int V, int vec, int K, uint32_t k0, uint32_t k1,
    uint32_t offset, int ctr_stride, int ctr_base, const int32_t* __restrict__ utt_ids, int32_t* __restrict__ greedy,
    int32_t* __restrict__ samples) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    float x[NV];
    wide_row_load<NV>(scores + r * V, V, lane, vec != 0, -INFINITY, x);
    const int v0 = lane * NV;
    float bv = x[0]; int bi = (v0 < V) ? v0 : 0x7fffffff;
#pragma unroll
    for (int i = 1; i < NV; ++i)
        if (v0 + i < V && x[i] > bv) { bv = x[i]; bi = v0 + i; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (greedy && lane == 0) greedy[r] = bi;
    float c[NV];          // inclusive prefix within the lane
    float run = 0.f;
    unsigned pm = 0;      // the lane's labels with e > 0
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float e = (v0 + i < V) ? __expf(x[i] - bv) : 0.f;
        run = (i == 0) ? e : run + e;
        c[i] = run;
        pm |= (e > 0.f ? 1u : 0u) << i;
    }
    float scan = run;     // inclusive scan of the lane totals, in lane order
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(scan, o, 64);
        if (lane >= o) scan += up;
    }
    const float total = __shfl(scan, 63, 64);
    float excl = __shfl_up(scan, 1, 64);
    if (lane == 0) excl = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) c[i] = (NV == 1) ? scan : excl + c[i];      // the cdf of frame_argmax_sample_wide_kernel
    const int bg_ = utt_ids ? utt_ids[r % B] : ctr_base + (int)(r % B);     // as in frame_argmax_sample_kernel
    const bool outside = (unsigned)bg_ >= (unsigned)ctr_stride;
    const long long ctr = outside ? (long long)r : (r / B) * (long long)ctr_stride + bg_;
    uint32_t rnd[4];
    philox4x32_10((uint32_t)ctr, offset, outside ? 1u : 0u, (uint32_t)lane, k0, k1, rnd);
    const float u = (float)(rnd[0] >> 8) * (1.0f / 16777216.0f);
    int mine = 0;
    for (int j = 0; j < K; ++j) {
        const float thr = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(u), j)) * total;
        int n = 0;
#pragma unroll
        for (int i = 0; i < NV; ++i) n += __popcll(__ballot(v0 + i < V && c[i] <= thr));
        if (n > V - 1) n = V - 1;
        n = wide_sample_skip_zero<NV>(n, pm, lane);
        if (lane == j) mine = n;
    }
    if (lane < K) samples[(size_t)lane * rows + r] = mine;
}

inline bool counter_fits(int T, int ctr_stride) { return (long long)T * ctr_stride <= (1ll << 32); }

// The statistics kernels keep frame_entropy_kernel's shape: one workgroup of WAVES waves per utterance, wave w adding the frames
// w, w + WAVES, .. in t order with an fp64 carry, wave 0 lane 0 adding the partial sums in w order.  FPT frames of a wave are
// loaded together so that their loads are in flight at once; fewer for the widest rows, which fill the registers by themselves.
// The grouping does not change the order of the additions.
constexpr int STAT_WAVES = 16;
template <int NV> constexpr int stat_fpt() { return NV <= 4 ? 4 : (NV == 8 ? 2 : 1); }
constexpr float KL_LOG_FLOOR = PGASR_KL_LOG_FLOOR;

// -H of the row in this wave's registers: p ln p added in label order within the lane, then one wave_sum.  p = 0 adds exactly 0.
template <int NV>
__device__ __forceinline__ float wide_row_plogp(const float (&lpv)[NV]) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float sm = __expf(lpv[i]);
        const float plp = sm > 0.f ? sm * lpv[i] : 0.f;
        s = (i == 0) ? plp : s + plp;
    }
    return wave_sum(s);
}

template <int NV>
__global__ __launch_bounds__(64 * STAT_WAVES) void frame_entropy_wide_kernel(
    const float* __restrict__ lp, const int32_t* __restrict__ in_len, int T, int B, int V, int vec, float beta, float inv_gb,
    float* __restrict__ ent_mean, float* __restrict__ ent_scale) {
    constexpr int FPT = stat_fpt<NV>();
    __shared__ double part[STAT_WAVES];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    double acc = 0.0;
    for (int t0 = w; t0 < Tb; t0 += FPT * STAT_WAVES) {
        float lpv[FPT][NV];
#pragma unroll
        for (int f = 0; f < FPT; ++f) {
            const int t = t0 + f * STAT_WAVES;
            if (t < Tb) {
                wide_row_load<NV>(lp + ((size_t)t * B + b) * V, V, lane, vec != 0, -INFINITY, lpv[f]);
            } else {
#pragma unroll
                for (int i = 0; i < NV; ++i) lpv[f][i] = -INFINITY;       // a frame >= T_b reads as p = 0 everywhere: H = 0
            }
        }
#pragma unroll
        for (int f = 0; f < FPT; ++f) acc += (double)(-wide_row_plogp<NV>(lpv[f]));
    }
    if (lane == 0) part[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < STAT_WAVES; ++i) s += part[i];
        const float n = (float)(Tb > 0 ? Tb : 1);
        ent_mean[b] = (float)(s / (double)n);
        ent_scale[b] = beta * inv_gb / n;
    }
}

template <int NV>
__global__ __launch_bounds__(64 * STAT_WAVES) void frame_kl_wide_kernel(
    const float* __restrict__ lp, const float* __restrict__ ref_lp, const int32_t* __restrict__ in_len, int T, int B, int V, int vec,
    float gamma, float inv_gb, float* __restrict__ kl_mean, float* __restrict__ kl_scale) {
    constexpr int FPT = stat_fpt<NV>();
    __shared__ double part[STAT_WAVES];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    double acc = 0.0;
    for (int t0 = w; t0 < Tb; t0 += FPT * STAT_WAVES) {
        float lpv[FPT][NV], lqv[FPT][NV];
#pragma unroll
        for (int f = 0; f < FPT; ++f) {
            const int t = t0 + f * STAT_WAVES;
            if (t < Tb) {
                const size_t o = ((size_t)t * B + b) * V;
                wide_row_load<NV>(lp + o, V, lane, vec != 0, -INFINITY, lpv[f]);
                wide_row_load<NV>(ref_lp + o, V, lane, vec != 0, 0.f, lqv[f]);
            } else {
#pragma unroll
                for (int i = 0; i < NV; ++i) { lpv[f][i] = -INFINITY; lqv[f][i] = 0.f; }     // p = 0 everywhere: KL = 0
            }
        }
#pragma unroll
        for (int f = 0; f < FPT; ++f) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const float sm = __expf(lpv[f][i]);
                const float d = sm > 0.f ? sm * (lpv[f][i] - fmaxf(lqv[f][i], KL_LOG_FLOOR)) : 0.f;
                s = (i == 0) ? d : s + d;
            }
            acc += (double)wave_sum(s);
        }
    }
    if (lane == 0) part[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < STAT_WAVES; ++i) s += part[i];
        const float n = (float)(Tb > 0 ? Tb : 1);
        kl_mean[b] = (float)(s / (double)n);
        kl_scale[b] = gamma * inv_gb / n;
    }
}

}  // namespace

extern "C" int pgasr_frame_sample_multi_wide(const float* scores, int T, int B, int V, int K, uint64_t seed, uint32_t offset,
                                             int ctr_stride, int ctr_base, const int32_t* utt_ids,
                                             int32_t* greedy_path, int32_t* sample_paths, void* stream) {
    if (!scores || !sample_paths || T <= 0 || B <= 0 || V <= 0) return PGASR_ERR_INVALID_ARG;
    if (K < 1 || K > PGASR_MAX_SAMPLES) return PGASR_ERR_INVALID_ARG;
    if (utt_ids) {
        if (ctr_stride < 1) return PGASR_ERR_INVALID_ARG;
        ctr_base = 0;
    } else {
        if (ctr_stride == 0) ctr_stride = B;              // the single-process layout: counter = t * B + b
        if (ctr_stride <= 0 || ctr_base < 0 || ctr_base >= ctr_stride) return PGASR_ERR_INVALID_ARG;
    }
    if (V > PGASR_WIDE_VMAX || (utt_ids && !counter_fits(T, ctr_stride))) return PGASR_ERR_UNSUPPORTED;
    const long long rows = (long long)T * B;
    const unsigned blocks = (unsigned)((rows + 3) / 4);
#define PGASR_CALL(NV) PGASR_LAUNCH_KERNEL(frame_sample_multi_wide_kernel<NV>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, \
                                           scores, rows, B, V, wide_vec_ok<NV>(scores, scores, V) ? 1 : 0, K,                    \
                                           (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), offset, ctr_stride, ctr_base, \
                                           utt_ids, greedy_path, sample_paths)
    PGASR_WIDE_DISPATCH(V, PGASR_CALL);
#undef PGASR_CALL
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

extern "C" int pgasr_frame_entropy_wide(const float* log_probs, const int32_t* input_lengths, int T, int B, int V,
                                        float beta, float inv_global_batch, float* ent_mean, float* ent_scale, void* stream) {
    if (!log_probs || !input_lengths || !ent_mean || !ent_scale) return PGASR_ERR_INVALID_ARG;
    if (T <= 0 || B <= 0 || V <= 0 || !(beta >= 0.f) || !(inv_global_batch > 0.f)) return PGASR_ERR_INVALID_ARG;
    if (V > PGASR_WIDE_VMAX) return PGASR_ERR_UNSUPPORTED;
#define PGASR_CALL(NV) PGASR_LAUNCH_KERNEL(frame_entropy_wide_kernel<NV>, dim3(B), dim3(64 * STAT_WAVES), 0, (hipStream_t)stream, \
                                           log_probs, input_lengths, T, B, V, wide_vec_ok<NV>(log_probs, log_probs, V) ? 1 : 0,    \
                                           beta, inv_global_batch, ent_mean, ent_scale)
    PGASR_WIDE_DISPATCH(V, PGASR_CALL);
#undef PGASR_CALL
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

extern "C" int pgasr_frame_kl_wide(const float* log_probs, const float* ref_log_probs, const int32_t* input_lengths, int T, int B,
                                   int V, float gamma, float inv_global_batch, float* kl_mean, float* kl_scale, void* stream) {
    if (!log_probs || !ref_log_probs || !input_lengths || !kl_mean || !kl_scale) return PGASR_ERR_INVALID_ARG;
    if (T <= 0 || B <= 0 || V <= 0 || !(gamma >= 0.f) || !(inv_global_batch > 0.f)) return PGASR_ERR_INVALID_ARG;
    if (V > PGASR_WIDE_VMAX) return PGASR_ERR_UNSUPPORTED;
#define PGASR_CALL(NV) PGASR_LAUNCH_KERNEL(frame_kl_wide_kernel<NV>, dim3(B), dim3(64 * STAT_WAVES), 0, (hipStream_t)stream,      \
                                           log_probs, ref_log_probs, input_lengths, T, B, V,                                      \
                                           wide_vec_ok<NV>(log_probs, ref_log_probs, V) ? 1 : 0, gamma, inv_global_batch, kl_mean, \
                                           kl_scale)
    PGASR_WIDE_DISPATCH(V, PGASR_CALL);
#undef PGASR_CALL
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
