// Waveform augmentation for gfx950: reverberation (pgasr_reverb), signal / noise power (pgasr_wave_power) and the level-restoring
// additive-noise mix (pgasr_wave_mix).  The functions are stated in include/pgasr_hip.h, section A0-WA, and in numpy in
// tests/wave_aug_ref.py.  All three are opt-in stages in front of the framing; nothing of the train step runs here.
//
// pgasr_reverb is a direct-form FIR in fp64: y[i] = fp32( sum_k f64(h[k]) * f64(x[i + d - k]) ), ascending k.  One 256-thread
// workgroup per tile of WA_TILE consecutive outputs of one row; the row's impulse response goes through LDS in chunks of WA_CHUNK
// taps together with the input span the chunk needs (WA_TILE + WA_CHUNK - 1 samples, zero outside [0, n)), both converted to fp64
// ONCE while they are staged, so the loop is fp64 FMAs and LDS reads only:
//   - thread t owns the WA_PER consecutive outputs 8 t .. 8 t + 7 of the tile: their accumulators and a sliding window of x stay in
//     registers.  Tap k reads ONE new x (the window moves down by one sample per tap) and h[k], a broadcast read, and feeds
//     WA_PER FMAs: 2 LDS reads per 8 FMAs.  The loop is unrolled by 8 taps, so the window's rotation is register renaming.
//   - the span is stored with one pad word per 8 (element j at j + j / 8): lane t reads 8-byte word 9 t + c, which covers the 64 banks
//     exactly once per 32 lanes (MI355X_MICROARCH.md, LDS: ds_read_b64, bank = (a / 4) mod 64).
//   - a staged zero (x outside [0, n), h beyond K in the last block of 8 taps) adds +-0.0 to an accumulator that starts at +0.0 and
//     therefore never is -0.0: the bits are those of skipping the term (the argument at the top of resample.hip).  This needs finite
//     h and x; the bank builder and the readers give nothing else.
//   - a chunk whose whole span lies outside [0, n) is skipped, and a row stops at its own K.
// 16-byte loads where the stride is a multiple of 4 and the base 16-byte aligned (the span starts on a multiple of 4 samples); a
// sample outside [0, n) is never loaded.  No workspace, no atomics; two runs give the same bits.
//
// pgasr_wave_power: one 1024-thread workgroup per row, one pass.  Element i belongs to thread (i / 4) % 1024, which adds its squares
// in ascending i (fp64 FMA; the square of an fp32 is exact); the 1024 partial sums are added in a fixed tree.  The order depends on
// n alone: the same samples give the same bits whatever else is in the batch, and whatever the alignment.
// pgasr_wave_mix: one pass, 4 elements per thread; the gains are formed in fp64 by every workgroup of a row from the three powers
// and rounded to fp32 before use (tile 0 of the row records them), or taken as given.
#include "common.h"

namespace {

constexpr int WA_THREADS = 256;
constexpr int WA_PER = 8;                          // consecutive outputs of a thread
constexpr int WA_TILE = WA_THREADS * WA_PER;       // 2048 outputs of a workgroup
constexpr int WA_CHUNK = 512;                      // taps staged at a time
constexpr int WA_MAX_TAPS = 16384;                 // the cap on taps: 1.024 s at 16 kHz
constexpr int WA_SPAN = WA_TILE + WA_CHUNK + 8;    // staged samples: tile + chunk - 1, + 3 for the 4-sample alignment, rounded up
constexpr int WA_SPAN_PAD = WA_SPAN + WA_SPAN / 8; // with one pad word per 8: 23.1 KB of fp64, + 4 KB of taps

__device__ __forceinline__ int wa_pos(int j) { return j + (j >> 3); }

// The taps kk = 0 .. kc-1 of one staged chunk for the thread's outputs ob .. ob + 7 (ob a multiple of 8).  With top = ob + SH +
// WA_CHUNK-1, tap kk + u of output ob + p reads staged sample X(p - u), X(q) = top - kk + q, kept in ring[q & 7]: each tap loads
// X(-u) alone.  top & 7 = R is the same for every thread and kk advances by 8, so wa_pos(top - kk - u) = wa_pos(top) - 9 kk / 8 - u -
// (u > R): the reads' offsets are immediates and the loop holds no address arithmetic beyond one subtraction per 8 taps.
template <int SH>
__device__ __forceinline__ void fir_chunk(const double* s_x, const double* s_h, int ob, int kc, double (&acc)[WA_PER]) {
    constexpr int R = (SH + WA_CHUNK - 1) & 7;
    const double* px = s_x + wa_pos(ob + SH + WA_CHUNK - 1);
    double ring[WA_PER];
#pragma unroll
    for (int q = 1; q < WA_PER; ++q) ring[q] = px[q + ((R + q) >> 3)];
    for (int kk = 0; kk < kc; kk += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            ring[(8 - u) & 7] = px[-u - (u > R ? 1 : 0)];
            const double hk = s_h[kk + u];
#pragma unroll
            for (int p = 0; p < WA_PER; ++p) acc[p] = fma(hk, ring[(p - u + 8) & 7], acc[p]);
        }
        px -= 9;
    }
}

template <bool VEC>
__global__ __launch_bounds__(WA_THREADS) void reverb_kernel(
    const float* __restrict__ wave, int stride, const int32_t* __restrict__ n_len, const float* __restrict__ rirs, int rir_stride,
    int n_rirs, const int32_t* __restrict__ rir_len, const int32_t* __restrict__ rir_delay, const int32_t* __restrict__ rir_idx,
    float* __restrict__ out, int tiles) {
    __shared__ __attribute__((aligned(16))) double s_x[WA_SPAN_PAD];
    __shared__ __attribute__((aligned(16))) double s_h[WA_CHUNK];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int t0 = tile * WA_TILE;                               // < stride: tiles = ceil(stride / WA_TILE)
    const int t1 = t0 + WA_TILE < stride ? t0 + WA_TILE : stride;
    const float* xr = wave + (size_t)b * stride;
    float* orow = out + (size_t)b * stride;
    int n = n_len[b];
    n = n < 0 ? 0 : (n > stride ? stride : n);
    const int c1 = n < t1 ? n : t1;                              // outputs [t0, c1) carry samples, [c1, t1) are zero
    const int r = rir_idx[b];
    if (r < 0 || r >= n_rirs) {                                  // no impulse response: the bits of the input
        for (int i = t0 + tid; i < t1; i += WA_THREADS) orow[i] = i < c1 ? xr[i] : 0.f;
        return;
    }
    if (c1 > t0) {
        int K = rir_len[r];
        K = K < 0 ? 0 : (K > rir_stride ? rir_stride : K);
        K = K > WA_MAX_TAPS ? WA_MAX_TAPS : K;
        int d = rir_delay[r];
        d = d < 0 ? 0 : (d >= K ? (K > 0 ? K - 1 : 0) : d);
        const float* h = rirs + (size_t)r * rir_stride;
        double acc[WA_PER];
#pragma unroll
        for (int p = 0; p < WA_PER; ++p) acc[p] = 0.0;
        const int ob = tid * WA_PER;                             // the thread's first output, relative to t0
        for (int k0 = 0; k0 < K; k0 += WA_CHUNK) {
            // taps k0 + kk, kk = 0 .. WA_CHUNK-1, of outputs t0 + o, o = 0 .. WA_TILE-1, read x[base + o + (WA_CHUNK-1 - kk)]
            const int base = t0 + d - k0 - (WA_CHUNK - 1);
            if (base + WA_TILE + WA_CHUNK - 2 < 0) break;        // this chunk and every later one lie in front of the row
            if (base >= n) continue;                             // behind the row's end (a long delay): nothing to add
            const int s0 = base & ~3;                            // rounds down, also below zero
            const int sh = base - s0;                            // 0 .. 3: staged sample j is x[s0 + j]
            __syncthreads();                                     // the previous chunk has been read
            if (VEC) {
                for (int q = tid; 4 * q < WA_SPAN; q += WA_THREADS) {
                    const int g = s0 + 4 * q;
                    float4 v;
                    if (g >= 0 && g + 3 < n) {
                        v = *(const float4*)(xr + g);
                    } else {
                        v.x = (g >= 0 && g < n) ? xr[g] : 0.f;
                        v.y = (g + 1 >= 0 && g + 1 < n) ? xr[g + 1] : 0.f;
                        v.z = (g + 2 >= 0 && g + 2 < n) ? xr[g + 2] : 0.f;
                        v.w = (g + 3 >= 0 && g + 3 < n) ? xr[g + 3] : 0.f;
                    }
                    const int j = wa_pos(4 * q);                 // 4 q .. 4 q + 3 share their pad offset
                    s_x[j] = (double)v.x; s_x[j + 1] = (double)v.y; s_x[j + 2] = (double)v.z; s_x[j + 3] = (double)v.w;
                }
            } else {
                for (int q = tid; q < WA_SPAN; q += WA_THREADS) {
                    const int g = s0 + q;
                    s_x[wa_pos(q)] = (g >= 0 && g < n) ? (double)xr[g] : 0.0;
                }
            }
            for (int q = tid; q < WA_CHUNK; q += WA_THREADS) s_h[q] = k0 + q < K ? (double)h[k0 + q] : 0.0;
            __syncthreads();
            const int kc = K - k0 < WA_CHUNK ? K - k0 : WA_CHUNK;          // taps of this chunk; the last block of 8 is zero padded
            switch (sh) {                                        // the span's alignment is uniform: it fixes the pad offsets
                case 0: fir_chunk<0>(s_x, s_h, ob, kc, acc); break;
                case 1: fir_chunk<1>(s_x, s_h, ob, kc, acc); break;
                case 2: fir_chunk<2>(s_x, s_h, ob, kc, acc); break;
                default: fir_chunk<3>(s_x, s_h, ob, kc, acc); break;
            }
        }
        // 8 consecutive fp32 per thread: two 16-byte stores where the row allows
        const int i0 = t0 + ob;
        if (VEC && i0 + WA_PER <= c1) {
            float4 lo, hi;
            lo.x = (float)acc[0]; lo.y = (float)acc[1]; lo.z = (float)acc[2]; lo.w = (float)acc[3];
            hi.x = (float)acc[4]; hi.y = (float)acc[5]; hi.z = (float)acc[6]; hi.w = (float)acc[7];
            *(float4*)(orow + i0) = lo;
            *(float4*)(orow + i0 + 4) = hi;
        } else {
#pragma unroll
            for (int p = 0; p < WA_PER; ++p)
                if (i0 + p < c1) orow[i0 + p] = (float)acc[p];
        }
    }
    const int z0 = c1 > t0 ? c1 : t0;
    for (int i = z0 + tid; i < t1; i += WA_THREADS) orow[i] = 0.f;
}

constexpr int WP_THREADS = 1024;

template <bool VEC>
__global__ __launch_bounds__(WP_THREADS) void wave_power_kernel(
    const float* __restrict__ src, int src_stride, int src_rows, const int32_t* __restrict__ n_len, const int32_t* __restrict__ row,
    const int32_t* __restrict__ start, const int32_t* __restrict__ period, double* __restrict__ power) {
    __shared__ double s_p[WP_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int rb = row ? row[b] : b;
    int n = n_len[b];
    n = n < 0 ? 0 : n;
    int m = period ? period[b] : src_stride;
    m = m > src_stride ? src_stride : m;
    if (rb < 0 || rb >= src_rows || m < 1) n = 0;                // no such row, or an empty one: 0
    const bool wraps = period != nullptr;
    if (!wraps && n > src_stride) n = src_stride;
    const float* xr = src + (size_t)(rb < 0 || rb >= src_rows ? 0 : rb) * src_stride;
    unsigned s = 0;
    if (wraps && start) {
        const int sb = start[b];
        s = sb < 0 ? 0u : (unsigned)sb % (unsigned)m;
    }
    double acc = 0.0;
    for (unsigned i = 4u * tid; i < (unsigned)n; i += 4u * WP_THREADS) {       // unsigned: i may pass 2^31 behind the last element
        if (!wraps) {
            if (VEC && i + 3 < (unsigned)n) {
                const float4 v = *(const float4*)(xr + i);
                acc = fma((double)v.x, (double)v.x, acc); acc = fma((double)v.y, (double)v.y, acc);
                acc = fma((double)v.z, (double)v.z, acc); acc = fma((double)v.w, (double)v.w, acc);
            } else {
                for (unsigned e = 0; e < 4 && i + e < (unsigned)n; ++e) {
                    const double v = (double)xr[i + e];
                    acc = fma(v, v, acc);
                }
            }
        } else {
            unsigned j = (s + i) % (unsigned)m;                  // s < m <= 2^31 - 1, i < 2^31: no overflow
            for (unsigned e = 0; e < 4 && i + e < (unsigned)n; ++e) {
                const double v = (double)xr[j];
                acc = fma(v, v, acc);
                j = j + 1 == (unsigned)m ? 0u : j + 1;
            }
        }
    }
    s_p[tid] = acc;
    __syncthreads();
    for (int w = WP_THREADS / 2; w > 0; w >>= 1) {               // a fixed tree: s_p[t] += s_p[t + w]
        if (tid < w) s_p[tid] += s_p[tid + w];
        __syncthreads();
    }
    if (tid == 0) power[b] = s_p[0];
}

constexpr int WM_THREADS = 256;
constexpr int WM_TILE = WM_THREADS * 4;

// a = fp32(sqrt(P_dry / P_wet)), 1 where P_wet = 0 or the quotient is no finite fp32; g = fp32(amp * sqrt(a^2 P_wet / P_noise)), 0
// where a power or amp is 0, the row takes no noise or the result is no finite fp32.  Each fp64 operation is rounded once.
__device__ __forceinline__ void wave_gains(double p_dry, double p_wet, double p_noise, double amp, bool noisy, float& a, float& g) {
    a = 1.f;
    if (p_wet > 0.0 && p_dry > 0.0) {
        const float t = (float)sqrt(p_dry / p_wet);
        if (t > 0.f && t < INFINITY) a = t;
    }
    g = 0.f;
    if (noisy && p_wet > 0.0 && p_noise > 0.0 && amp > 0.0) {
        const double aa = (double)a * (double)a;
        const double q = (aa * p_wet) / p_noise;
        const float t = (float)(amp * sqrt(q));
        if (t > 0.f && t < INFINITY) g = t;
    }
}

template <bool VEC>
__global__ __launch_bounds__(WM_THREADS) void wave_mix_kernel(
    const float* wave, int stride, const int32_t* __restrict__ n_len, const double* __restrict__ p_dry,
    const double* __restrict__ p_wet, const double* __restrict__ p_noise, const double* __restrict__ amp,
    const float* __restrict__ noise, int noise_stride, int noise_rows, const int32_t* __restrict__ noise_len,
    const int32_t* __restrict__ noise_idx, const int32_t* __restrict__ noise_start, float* gains, int gains_given, float* out,
    int tiles) {
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const float* xr = wave + (size_t)b * stride;
    float* orow = out + (size_t)b * stride;
    int n = n_len[b];
    n = n < 0 ? 0 : (n > stride ? stride : n);
    int rn = (noise && noise_idx) ? noise_idx[b] : -1;
    int m = 0;
    if (rn >= 0 && rn < noise_rows) {
        m = noise_len[rn];
        m = m > noise_stride ? noise_stride : m;
    }
    const bool noisy = m >= 1 && n >= 1;
    float a, g;
    if (gains_given) {
        a = gains[2 * b];
        g = noisy ? gains[2 * b + 1] : 0.f;
    } else {
        wave_gains(p_dry[b], p_wet[b], noisy ? p_noise[b] : 0.0, amp ? amp[b] : 0.0, noisy, a, g);
        if (tile == 0 && tid == 0) { gains[2 * b] = a; gains[2 * b + 1] = g; }
    }
    const double ad = (double)a, gd = (double)g;
    const int i = tile * WM_TILE + 4 * tid;
    if (i >= stride) return;
    float x[4], y[4];
    if (VEC && i + 3 < n) {
        const float4 v = *(const float4*)(xr + i);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = i + e < n ? xr[i + e] : 0.f;
    }
    if (g != 0.f) {                                              // g = 0: the noise is not read and the term is dropped
        const float* nr = noise + (size_t)rn * noise_stride;
        const int sb = noise_start ? noise_start[b] : 0;
        unsigned j = ((sb < 0 ? 0u : (unsigned)sb % (unsigned)m) + (unsigned)i) % (unsigned)m;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float z = i + e < n ? nr[j] : 0.f;
            y[e] = (float)fma(ad, (double)x[e], gd * (double)z);
            j = j + 1 == (unsigned)m ? 0u : j + 1;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = (float)(ad * (double)x[e]);
    }
    if (VEC && i + 3 < stride) {
        float4 v;
        v.x = i < n ? y[0] : 0.f; v.y = i + 1 < n ? y[1] : 0.f; v.z = i + 2 < n ? y[2] : 0.f; v.w = i + 3 < n ? y[3] : 0.f;
        *(float4*)(orow + i) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i + e < stride) orow[i + e] = i + e < n ? y[e] : 0.f;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int pgasr_reverb_limits(int* tile, int* chunk, int* max_taps) {
    if (tile) *tile = WA_TILE;
    if (chunk) *chunk = WA_CHUNK;
    if (max_taps) *max_taps = WA_MAX_TAPS;
    return PGASR_OK;
}

extern "C" int pgasr_reverb(const float* wave, int stride, const int32_t* n, int B, const float* rirs, int rir_stride, int n_rirs,
                            const int32_t* rir_len, const int32_t* rir_delay, const int32_t* rir_idx, float* out, void* stream) {
    if (!wave || !n || !rirs || !rir_len || !rir_delay || !rir_idx || !out) return PGASR_ERR_INVALID_ARG;
    if (out == wave) return PGASR_ERR_INVALID_ARG;
    if (B < 1 || stride < 1 || rir_stride < 1 || n_rirs < 1) return PGASR_ERR_INVALID_ARG;
    if (stride > 2147483647 - 2 * WA_MAX_TAPS - WA_TILE) return PGASR_ERR_UNSUPPORTED;        // sample indices stay in 32 bits
    const long long tiles = ((long long)stride + WA_TILE - 1) / WA_TILE;
    if (tiles * B > 2147483647LL) return PGASR_ERR_UNSUPPORTED;
    const bool vec = stride % 4 == 0 && aligned16(wave) && aligned16(out);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(tiles * B));
    if (vec)
        PGASR_LAUNCH_KERNEL(reverb_kernel<true>, grid, dim3(WA_THREADS), 0, st, wave, stride, n, rirs, rir_stride, n_rirs, rir_len,
                            rir_delay, rir_idx, out, (int)tiles);
    else
        PGASR_LAUNCH_KERNEL(reverb_kernel<false>, grid, dim3(WA_THREADS), 0, st, wave, stride, n, rirs, rir_stride, n_rirs, rir_len,
                            rir_delay, rir_idx, out, (int)tiles);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

extern "C" int pgasr_wave_power(const float* src, int src_stride, int src_rows, const int32_t* n, int B, const int32_t* row,
                                const int32_t* start, const int32_t* period, double* power, void* stream) {
    if (!src || !n || !power) return PGASR_ERR_INVALID_ARG;
    if (B < 1 || src_stride < 1 || src_rows < 1) return PGASR_ERR_INVALID_ARG;
    if (!row && src_rows < B) return PGASR_ERR_INVALID_ARG;
    if (start && !period) return PGASR_ERR_INVALID_ARG;
    const bool vec = src_stride % 4 == 0 && aligned16(src);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        PGASR_LAUNCH_KERNEL(wave_power_kernel<true>, dim3(B), dim3(WP_THREADS), 0, st, src, src_stride, src_rows, n, row, start, period,
                            power);
    else
        PGASR_LAUNCH_KERNEL(wave_power_kernel<false>, dim3(B), dim3(WP_THREADS), 0, st, src, src_stride, src_rows, n, row, start, period,
                            power);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

extern "C" int pgasr_wave_mix(const float* wave, int stride, const int32_t* n, int B, const double* p_dry, const double* p_wet,
                              const double* p_noise, const double* amp, const float* noise, int noise_stride, int noise_rows,
                              const int32_t* noise_len, const int32_t* noise_idx, const int32_t* noise_start, float* gains,
                              int gains_given, float* out, void* stream) {
    if (!wave || !n || !gains || !out) return PGASR_ERR_INVALID_ARG;
    if (B < 1 || stride < 1) return PGASR_ERR_INVALID_ARG;
    if (stride > 2147483647 - WM_TILE) return PGASR_ERR_UNSUPPORTED;
    if (noise && (!noise_len || !noise_idx || noise_stride < 1 || noise_rows < 1)) return PGASR_ERR_INVALID_ARG;
    if (!gains_given && (!p_dry || !p_wet || (noise && (!p_noise || !amp)))) return PGASR_ERR_INVALID_ARG;
    const long long tiles = ((long long)stride + WM_TILE - 1) / WM_TILE;
    if (tiles * B > 2147483647LL) return PGASR_ERR_UNSUPPORTED;
    const bool vec = stride % 4 == 0 && aligned16(wave) && aligned16(out);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(tiles * B));
    if (vec)
        PGASR_LAUNCH_KERNEL(wave_mix_kernel<true>, grid, dim3(WM_THREADS), 0, st, wave, stride, n, p_dry, p_wet, p_noise, amp, noise,
                            noise_stride, noise_rows, noise_len, noise_idx, noise_start, gains, gains_given, out, (int)tiles);
    else
        PGASR_LAUNCH_KERNEL(wave_mix_kernel<false>, grid, dim3(WM_THREADS), 0, st, wave, stride, n, p_dry, p_wet, p_noise, amp, noise,
                            noise_stride, noise_rows, noise_len, noise_idx, noise_start, gains, gains_given, out, (int)tiles);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
