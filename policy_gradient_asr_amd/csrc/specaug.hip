// SpecAugment (Park et al. 2019) time / frequency masking of a feature batch for gfx950 (pgasr_spec_augment; the masking function
// is stated in include/pgasr_hip.h, section A0-AUG, and in numpy in tests/specaug_ref.py).
//
// One launch, one 256-thread workgroup per (b, f) row of T contiguous floats (a grid-stride loop over the B * F rows):
//   1. threads 0 .. n_freq + n_time - 1 each run the ONE Philox block of their mask and put (start, width) into LDS -- at most 16
//      blocks, recomputed per row instead of read from a table a first launch would have to write (no second launch, no workspace);
//      the workgroup of row f = 0 also writes them to `masks`.
//   2. a row that some mask touches and that is filled with its mean: the sum of x[b, f, 0:len] in fp64 -- every thread adds its own
//      elements in ascending t, a butterfly over the wave, the four wave sums added in wave order -- a fixed order, so two runs
//      give the same bits.  No atomics anywhere.
//   3. the row is streamed from x to out with the masked cells replaced; 16-byte loads and stores where T % 4 == 0 and both
//      pointers are 16-byte aligned (every row then is), one float per thread otherwise.  The second read of a row the mean was
//      taken over comes from the cache.  out == x: a row no mask touches is left alone; every other row is read completely (the
//      barriers of the sum) before its first store, and rows do not depend on each other.
#include "common.h"
#include <limits.h>

namespace {

constexpr int SA_THREADS = 256;
constexpr int SA_MAX_MASKS = 8;          // of a kind
constexpr int SA_MAX_BLOCKS = 8192;      // workgroups of a launch; the rows beyond are taken by the grid-stride loop

// the sum of v over the workgroup in a fixed order; every thread returns it, and `red` is free again on return
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return r;
}

struct TimeMasks {
    int start[SA_MAX_MASKS], width[SA_MAX_MASKS];     // absent masks: width 0
    __device__ __forceinline__ bool hit(int t) const {
        bool h = false;
#pragma unroll
        for (int m = 0; m < SA_MAX_MASKS; ++m) h |= (unsigned)(t - start[m]) < (unsigned)width[m];
        return h;
    }
};

template <bool VEC>
__global__ __launch_bounds__(SA_THREADS) void spec_augment_kernel(
    const float* x, const int32_t* __restrict__ lengths, const int32_t* __restrict__ utt_ids, int batch_offset,
    int B, int F, int T, int n_freq, int freq_width, int n_time, int time_width, float time_ratio, int fill_mode,
    uint32_t k0, uint32_t k1, uint32_t offset, float* out, int32_t* __restrict__ masks) {
    __shared__ int s_start[2 * SA_MAX_MASKS], s_width[2 * SA_MAX_MASKS];
    __shared__ double red[SA_THREADS / 64];
    const int tid = threadIdx.x;
    const int nM = n_freq + n_time;
    const size_t rows = (size_t)B * F;
    for (size_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int b = (int)(row / F), f = (int)(row - (size_t)b * F);
        int len = lengths[b];
        len = len < 0 ? 0 : (len > T ? T : len);
        const long long id = utt_ids ? (long long)utt_ids[b] : (long long)batch_offset + b;
        if (tid < nM) {
            int start = 0, width = 0;                 // id < 0 (a padded, empty utterance): no mask at all
            if (id >= 0) {
                const bool fm = tid < n_freq;
                const int m = fm ? tid : tid - n_freq;
                const int span = fm ? F : len;
                int W;
                if (fm) {
                    W = freq_width < F ? freq_width : F;
                } else {
                    const float wr = __fmul_rn(time_ratio, (float)len);        // one fp32 multiply, then truncation
                    const int wi = wr >= 2147483648.f ? INT_MAX : (int)wr;
                    W = time_width < len ? time_width : len;
                    W = wi < W ? wi : W;
                }
                uint32_t w[4];
                philox4x32_10((uint32_t)id, offset, fm ? 2u : 3u, (uint32_t)m, k0, k1, w);
                width = (int)(((uint64_t)(w[0] >> 8) * ((uint64_t)W + 1)) >> 24);                      // uniform on 0 .. W
                start = (int)(((uint64_t)(w[1] >> 8) * ((uint64_t)(span - width) + 1)) >> 24);         // uniform on 0 .. span - width
            }
            s_start[tid] = start; s_width[tid] = width;
            if (masks && f == 0) {
                masks[((size_t)b * nM + tid) * 2] = start;
                masks[((size_t)b * nM + tid) * 2 + 1] = width;
            }
        }
        __syncthreads();
        bool frow = false;                   // the whole row lies in a frequency mask
        for (int m = 0; m < n_freq; ++m) frow |= (unsigned)(f - s_start[m]) < (unsigned)s_width[m];
        TimeMasks tm;
        bool any_time = false;
#pragma unroll
        for (int m = 0; m < SA_MAX_MASKS; ++m) {
            tm.start[m] = m < n_time ? s_start[n_freq + m] : 0;
            tm.width[m] = m < n_time ? s_width[n_freq + m] : 0;
            any_time |= tm.width[m] > 0;
        }
        const bool touched = len > 0 && (frow || any_time);      // the same in every thread of the workgroup
        const float* xr = x + row * (size_t)T;
        float* orow = out + row * (size_t)T;

        float fill = 0.f;
        if (touched && fill_mode == PGASR_SPECAUG_FILL_ROW_MEAN) {
            double s = 0.0;
            if (VEC) {
                const float4* x4 = (const float4*)xr;
                for (int i = tid; 4 * i < len; i += SA_THREADS) {
                    const float4 v = x4[i];
                    const int t = 4 * i;
                    s += (double)v.x;
                    if (t + 1 < len) s += (double)v.y;
                    if (t + 2 < len) s += (double)v.z;
                    if (t + 3 < len) s += (double)v.w;
                }
            } else {
                for (int t = tid; t < len; t += SA_THREADS) s += (double)xr[t];
            }
            fill = (float)(block_sum_f64(s, red) / (double)len);
        }

        if (touched || out != x) {
            if (VEC) {
                const float4* x4 = (const float4*)xr;
                float4* o4 = (float4*)orow;
                const int n4 = T >> 2;
                for (int i = tid; i < n4; i += SA_THREADS) {
                    float4 v = x4[i];
                    const int t = 4 * i;
                    if (touched && t < len) {
                        if (frow || tm.hit(t)) v.x = fill;
                        if (t + 1 < len && (frow || tm.hit(t + 1))) v.y = fill;
                        if (t + 2 < len && (frow || tm.hit(t + 2))) v.z = fill;
                        if (t + 3 < len && (frow || tm.hit(t + 3))) v.w = fill;
                    }
                    o4[i] = v;
                }
            } else {
                for (int t = tid; t < T; t += SA_THREADS) {
                    float v = xr[t];
                    if (touched && t < len && (frow || tm.hit(t))) v = fill;
                    orow[t] = v;
                }
            }
        }
        __syncthreads();        // the interval table is rewritten for the next row
    }
}

}  // namespace

extern "C" int pgasr_spec_augment(const float* x, const int32_t* lengths, const int32_t* utt_ids, int batch_offset,
                                  int B, int F, int T, int n_freq, int freq_width, int n_time, int time_width,
                                  float time_ratio, int fill_mode, unsigned long long seed, unsigned offset,
                                  float* out, int32_t* masks, void* stream) {
    if (!x || !lengths || !out) return PGASR_ERR_INVALID_ARG;
    if (B < 1 || F < 1 || T < 1) return PGASR_ERR_INVALID_ARG;
    if (n_freq < 0 || n_time < 0 || freq_width < 0 || time_width < 0) return PGASR_ERR_INVALID_ARG;
    if (!(time_ratio > 0.f && time_ratio <= 1.f)) return PGASR_ERR_INVALID_ARG;      // NaN included
    if (fill_mode != PGASR_SPECAUG_FILL_ROW_MEAN && fill_mode != PGASR_SPECAUG_FILL_ZERO) return PGASR_ERR_INVALID_ARG;
    if (n_freq > SA_MAX_MASKS || n_time > SA_MAX_MASKS) return PGASR_ERR_UNSUPPORTED;
    if (n_freq + n_time == 0 && out == x) return PGASR_OK;                           // the identity, in place
    const size_t rows = (size_t)B * F;
    const int grid = (int)(rows < (size_t)SA_MAX_BLOCKS ? rows : (size_t)SA_MAX_BLOCKS);
    const bool vec = T % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (vec)
        PGASR_LAUNCH_KERNEL(spec_augment_kernel<true>, dim3(grid), dim3(SA_THREADS), 0, st, x, lengths, utt_ids, batch_offset,
                            B, F, T, n_freq, freq_width, n_time, time_width, time_ratio, fill_mode, k0, k1, (uint32_t)offset, out, masks);
    else
        PGASR_LAUNCH_KERNEL(spec_augment_kernel<false>, dim3(grid), dim3(SA_THREADS), 0, st, x, lengths, utt_ids, batch_offset,
                            B, F, T, n_freq, freq_width, n_time, time_width, time_ratio, fill_mode, k0, k1, (uint32_t)offset, out, masks);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
