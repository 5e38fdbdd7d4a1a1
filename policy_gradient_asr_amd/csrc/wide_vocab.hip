// Row kernels for alphabets of up to 1024 symbols on gfx950 (header section A9-WIDE): log-softmax and argmax / inverse-CDF sample
// of (t,b) rows of V <= 1024 scores.  One wave per row as in frame_ops.hip, but lane l holds the NV = ceil(V / 64) (rounded up to
// 1, 2, 4, 8 or 16) CONSECUTIVE labels l*NV .. l*NV + NV - 1 in registers (wide_rows.h): a lane's loads are one or more 16-byte
// vectors where the row's alignment allows, a wave's loads cover one contiguous span, and every reduction is a sequential pass over
// the lane's own values followed by ONE wave butterfly or scan of the 64 lane results -- a fixed order, so two runs give the
// same bits.  HBM-bound streaming kernels: T*B*V*4 bytes read, and written where a row is written.
#include "wide_rows.h"

namespace {

// log_softmax of one row per wave: maximum, exp of the differences and their sum in fp32
template <int NV>
__global__ __launch_bounds__(256) void log_softmax_rows_wide_kernel(const float* __restrict__ x, long long rows, int V, int vec,
                                                                    float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    float v[NV];
    wide_row_load<NV>(x + r * V, V, lane, vec != 0, -INFINITY, v);
    float m = v[0];
#pragma unroll
    for (int i = 1; i < NV; ++i) m = fmaxf(m, v[i]);
    const float mx = wave_max(m);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (lane * NV + i < V) ? __expf(v[i] - mx) : 0.f;      // label order within the lane
    const float lse = mx + __logf(wave_sum(s));
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] -= lse;
    wide_row_store<NV>(y + r * V, V, lane, vec != 0, v);
}

// frame_argmax_sample_kernel for wide rows: the same Philox counter, key and u; first maximum wins; k = #{v : cdf_v <= u * total}
// clamped to V - 1, the inclusive cdf in label order: a sequential prefix over the lane's labels on top of the exclusive wave scan
// of the lane totals.  With NV = 1 the cdf IS frame_argmax_sample_kernel's scan, operation for operation.
template <int NV>
__global__ __launch_bounds__(256) void frame_argmax_sample_wide_kernel(
    const float* __restrict__ scores, long long rows, int B, int V, int vec, uint32_t k0, uint32_t k1,
    uint32_t offset, int ctr_stride, int ctr_base, const int32_t* __restrict__ utt_ids, int32_t* __restrict__ greedy,
    int32_t* __restrict__ sample) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    float x[NV];
    wide_row_load<NV>(scores + r * V, V, lane, vec != 0, -INFINITY, x);
    const int v0 = lane * NV;
    // the lane's first maximum, then (value, index) pairs across the wave: the smaller index wins a tie
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
    if (sample) {
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
        uint32_t rnd[4];
        // counter addressing as in frame_argmax_sample_kernel: t * ctr_stride + global utterance index, rows beyond the global
        // batch in the disjoint domain (third counter word 1)
        const int bg_ = utt_ids ? utt_ids[r % B] : ctr_base + (int)(r % B);
        const bool outside = (unsigned)bg_ >= (unsigned)ctr_stride;
        const long long ctr = outside ? (long long)r : (r / B) * (long long)ctr_stride + bg_;
        philox4x32_10((uint32_t)ctr, offset, outside ? 1u : 0u, 0u, k0, k1, rnd);
        const float u = (float)(rnd[0] >> 8) * (1.0f / 16777216.0f);
        const float thr = u * total;
        int n = 0;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const float cdf = (NV == 1) ? scan : excl + c[i];
            n += (v0 + i < V && cdf <= thr) ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if (n > V - 1) n = V - 1;
        n = wide_sample_skip_zero<NV>(n, pm, lane);
        if (lane == 0) sample[r] = n;
    }
}

inline bool counter_fits(int T, int ctr_stride) { return (long long)T * ctr_stride <= (1ll << 32); }

}  // namespace

extern "C" int pgasr_log_softmax_rows_wide(const float* logits, long long rows, int V, float* log_probs, void* stream) {
    if (!logits || !log_probs || rows <= 0 || V <= 0) return PGASR_ERR_INVALID_ARG;
    if (V > PGASR_WIDE_VMAX) return PGASR_ERR_UNSUPPORTED;
    const unsigned blocks = (unsigned)((rows + 3) / 4);
#define PGASR_CALL(NV) PGASR_LAUNCH_KERNEL(log_softmax_rows_wide_kernel<NV>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, \
                                           logits, rows, V, wide_vec_ok<NV>(logits, log_probs, V) ? 1 : 0, log_probs)
    PGASR_WIDE_DISPATCH(V, PGASR_CALL);
#undef PGASR_CALL
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

extern "C" int pgasr_frame_argmax_sample_wide(const float* scores, int T, int B, int V, uint64_t seed, uint32_t offset,
                                              int ctr_stride, int ctr_base, const int32_t* utt_ids,
                                              int32_t* greedy_path, int32_t* sample_path, void* stream) {
    if (!scores || T <= 0 || B <= 0 || V <= 0) return PGASR_ERR_INVALID_ARG;
    if (utt_ids) {
        if (ctr_stride < 1) return PGASR_ERR_INVALID_ARG;
        ctr_base = 0;
    } else {
        if (ctr_stride == 0) ctr_stride = B;              // the single-process layout: counter = t * B + b
        if (ctr_stride <= 0 || ctr_base < 0 || ctr_base >= ctr_stride) return PGASR_ERR_INVALID_ARG;
    }
    // the id form checks that t * ctr_stride + id fits counter word 0, as pgasr_frame_argmax_sample_ids does
    if (V > PGASR_WIDE_VMAX || (utt_ids && !counter_fits(T, ctr_stride))) return PGASR_ERR_UNSUPPORTED;
    if (!greedy_path && !sample_path) return PGASR_OK;
    const long long rows = (long long)T * B;
    const unsigned blocks = (unsigned)((rows + 3) / 4);
#define PGASR_CALL(NV) PGASR_LAUNCH_KERNEL(frame_argmax_sample_wide_kernel<NV>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, \
                                           scores, rows, B, V, wide_vec_ok<NV>(scores, scores, V) ? 1 : 0,                        \
                                           (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), offset, ctr_stride, ctr_base,  \
                                           utt_ids, greedy_path, sample_path)
    PGASR_WIDE_DISPATCH(V, PGASR_CALL);
#undef PGASR_CALL
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
