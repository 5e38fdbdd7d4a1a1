// Sample-rate conversion / speed perturbation of a waveform batch for gfx950 (pgasr_resample; the resampling function is stated in
// include/pgasr_hip.h, section A0-RS, and in numpy in tests/resample_ref.py): a polyphase Hann-windowed sinc filter, ratio L / M.
//
// One launch, one 256-thread workgroup per tile of consecutive outputs of one utterance.  Output n = i * L + j reads the W inputs
// from pos(n) - half on, pos(n) = i * M + base_j = floor(n * M / L): pos is monotone in n, so a tile [n0, n1) needs ONE contiguous
// input span, pos(n0) - half .. pos(n1 - 1) + half.  The tile size of a ratio is chosen on the host so that the span fits RS_SPAN
// words of LDS (downsampling by 16 still gets 256 outputs per tile):
//   1. the span is staged in LDS, zero outside [0, n_in) -- 16-byte loads where in_stride % 4 == 0 and the batch is 16-byte aligned
//      (the span starts on a multiple of 4 samples), never a load of a sample outside [0, n_in); the ratio's table h[L][W] is staged
//      beside it where it fits RS_TABLE words (160 x 35 does), else it is read through L2.
//   2. thread t computes outputs n0 + t, n0 + t + 256, ..: W multiply-adds in ascending tap order in fp64, rounded to fp32 once.  A
//      staged zero adds +-0.0 to an accumulator that starts at +0.0 and so never is -0.0: the bits are those of skipping the tap.
//      Lanes walk the span with stride M / L and the table with stride W (odd): neither piles onto an LDS bank.
//   3. outputs n_out <= n < out_stride of the tile are written as 0.0f; the workgroup of tile 0 writes n_out[b].
// Ratio 1/1 copies the bits.  No workspace, no atomics, no host synchronisation; a run is reproducible bit for bit.
#include "common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_RATIOS = 8;
constexpr int RS_MAX_LM = 1024;          // L, M after reduction
constexpr int RS_MAX_FACTOR = 16;        // 1/16 <= L / M <= 16
constexpr int RS_PER_THREAD = 4;         // outputs of a thread
constexpr int RS_MAX_TILE = RS_THREADS * RS_PER_THREAD;
constexpr int RS_SPAN = 4608;            // words of LDS for a tile's input span: 256 outputs at 1/16 need 255 * 16 + 195 + 4
constexpr int RS_TABLE = 5632;           // words of LDS for a ratio's table; with the span 40 KB, four workgroups per CU
constexpr double RS_ZEROS = 6.0, RS_ROLLOFF = 0.99;

struct RsRatio { int L, M, W, half, tile, tab_off, base_off, staged; };
struct RsRatios { RsRatio r[RS_MAX_RATIOS]; };

template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(
    const float* __restrict__ wave, int in_stride, const int32_t* __restrict__ n_in, const int32_t* __restrict__ ratio_idx,
    int n_ratios, RsRatios ratios, const float* __restrict__ tables, const int32_t* __restrict__ bases,
    float* __restrict__ out, int out_stride, int32_t* __restrict__ n_out, int tiles) {
    __shared__ __attribute__((aligned(16))) float s_x[RS_SPAN];
    __shared__ float s_h[RS_TABLE];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    float* orow = out + (size_t)b * out_stride;
    const int ri = ratio_idx ? ratio_idx[b] : 0;
    if (ri < 0 || ri >= n_ratios) {               // no such ratio: an empty row
        for (long long n = (long long)tile * RS_MAX_TILE + tid; n < out_stride && n < (long long)(tile + 1) * RS_MAX_TILE; n += RS_THREADS)
            orow[n] = 0.f;
        if (tile == 0 && tid == 0) n_out[b] = 0;
        return;
    }
    const RsRatio R = ratios.r[ri];
    const long long n0 = (long long)tile * R.tile;
    if (n0 >= out_stride) return;
    int len = n_in[b];
    len = len < 0 ? 0 : (len > in_stride ? in_stride : len);
    const int nout = (int)(((long long)len * R.L + R.M - 1) / R.M);        // <= out_stride (checked on the host for in_stride)
    if (tile == 0 && tid == 0) n_out[b] = nout;
    const int t0 = (int)n0;
    const int t1 = (int)(n0 + R.tile < out_stride ? n0 + R.tile : out_stride);      // the tile's outputs [t0, t1)
    const int c1 = nout < t1 ? nout : t1;                                           // .. of which [t0, c1) are computed
    const float* xr = wave + (size_t)b * in_stride;

    if (R.L == 1 && R.M == 1) {                   // the bits of the input
        for (int n = t0 + tid; n < t1; n += RS_THREADS) orow[n] = n < c1 ? xr[n] : 0.f;
        return;
    }
    if (c1 > t0) {
        const int32_t* bj = bases + R.base_off;
        const float* tab = tables + R.tab_off;
        // pos(n) = (n / L) * M + base[n % L]
        const int pos0 = (t0 / R.L) * R.M + bj[t0 % R.L];
        const int posl = ((c1 - 1) / R.L) * R.M + bj[(c1 - 1) % R.L];
        const int s0 = (pos0 - R.half) & ~3;                      // rounds down, also below zero
        const int span = posl + R.half + 1 - s0;                  // <= RS_SPAN by the host's choice of R.tile
        if (VEC) {
            for (int q = tid; 4 * q < span; q += RS_THREADS) {
                const int g = s0 + 4 * q;
                float4 v;
                if (g >= 0 && g + 3 < len) {
                    v = *(const float4*)(xr + g);
                } else {
                    v.x = (g >= 0 && g < len) ? xr[g] : 0.f;
                    v.y = (g + 1 >= 0 && g + 1 < len) ? xr[g + 1] : 0.f;
                    v.z = (g + 2 >= 0 && g + 2 < len) ? xr[g + 2] : 0.f;
                    v.w = (g + 3 >= 0 && g + 3 < len) ? xr[g + 3] : 0.f;
                }
                *(float4*)(s_x + 4 * q) = v;
            }
        } else {
            for (int q = tid; q < span; q += RS_THREADS) {
                const int g = s0 + q;
                s_x[q] = (g >= 0 && g < len) ? xr[g] : 0.f;
            }
        }
        if (R.staged)
            for (int q = tid; q < R.L * R.W; q += RS_THREADS) s_h[q] = tab[q];
        __syncthreads();
        // the thread's outputs t0 + tid + 256 r side by side: RS_PER_THREAD independent accumulators, each summed in ascending k
        int xo[RS_PER_THREAD], ho[RS_PER_THREAD];
        double acc[RS_PER_THREAD];
#pragma unroll
        for (int r = 0; r < RS_PER_THREAD; ++r) {
            const int n = t0 + tid + r * RS_THREADS;
            const bool live = n < c1;
            const int i = live ? n / R.L : 0, j = live ? n - i * R.L : 0;
            xo[r] = live ? i * R.M + bj[j] - R.half - s0 : 0;         // an idle slot reads taps 0 .. W-1 of the span and of phase 0
            ho[r] = j * R.W;
            acc[r] = 0.0;
        }
        if (R.staged && RS_THREADS % R.L == 0) {          // outputs 256 apart share their phase (1/3, 1/2, 2/1, ..): one table read per tap
            const float* h = s_h + ho[0];
            for (int k = 0; k < R.W; ++k) {
                const double hk = (double)h[k];
#pragma unroll
                for (int r = 0; r < RS_PER_THREAD; ++r) acc[r] = fma(hk, (double)s_x[xo[r] + k], acc[r]);
            }
        } else if (R.staged) {
            for (int k = 0; k < R.W; ++k)
#pragma unroll
                for (int r = 0; r < RS_PER_THREAD; ++r) acc[r] = fma((double)s_h[ho[r] + k], (double)s_x[xo[r] + k], acc[r]);
        } else {
            for (int k = 0; k < R.W; ++k)
#pragma unroll
                for (int r = 0; r < RS_PER_THREAD; ++r) acc[r] = fma((double)tab[ho[r] + k], (double)s_x[xo[r] + k], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < RS_PER_THREAD; ++r) {
            const int n = t0 + tid + r * RS_THREADS;
            if (n < c1) orow[n] = (float)acc[r];
        }
    }
    const int z0 = c1 > t0 ? c1 : t0;
    for (int n = z0 + tid; n < t1; n += RS_THREADS) orow[n] = 0.f;
}

int gcd_int(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

// half = ceil(Z / fc), fc = rolloff * min(1, L / M): the same double operations as features.resample_filter
int filter_half(int L, int M) {
    const double fc = RS_ROLLOFF * (L < M ? (double)L / (double)M : 1.0);
    return (int)ceil(RS_ZEROS / fc);
}

}  // namespace

extern "C" int pgasr_resample(const float* wave, int in_stride, const int32_t* n_in, int B, const int32_t* ratio_idx, int n_ratios,
                              const int32_t* ratio_desc, const float* tables, const int32_t* bases, float* out, int out_stride,
                              int32_t* n_out, void* stream) {
    if (!wave || !n_in || !ratio_desc || !tables || !bases || !out || !n_out) return PGASR_ERR_INVALID_ARG;
    if (out == wave) return PGASR_ERR_INVALID_ARG;
    if (B < 1 || in_stride < 1 || out_stride < 1 || n_ratios < 1) return PGASR_ERR_INVALID_ARG;
    if (n_ratios > RS_MAX_RATIOS) return PGASR_ERR_UNSUPPORTED;
    RsRatios rs;
    long long need = 0, tiles = 1;
    int base_off = 0;
    for (int r = 0; r < n_ratios; ++r) {
        const int L = ratio_desc[4 * r], M = ratio_desc[4 * r + 1], W = ratio_desc[4 * r + 2], off = ratio_desc[4 * r + 3];
        if (L < 1 || M < 1 || gcd_int(L, M) != 1) return PGASR_ERR_INVALID_ARG;
        if (L > RS_MAX_LM || M > RS_MAX_LM || L > (long long)RS_MAX_FACTOR * M || M > (long long)RS_MAX_FACTOR * L)
            return PGASR_ERR_UNSUPPORTED;
        const int half = filter_half(L, M);
        if (W != 2 * half + 1 || off < 0) return PGASR_ERR_INVALID_ARG;
        int tile = (int)((long long)(RS_SPAN - W - 4) * L / M) / RS_THREADS * RS_THREADS;
        tile = tile < RS_THREADS ? RS_THREADS : (tile > RS_MAX_TILE ? RS_MAX_TILE : tile);
        if (((long long)(tile - 1) * M + L - 1) / L + W + 3 > RS_SPAN) return PGASR_ERR_UNSUPPORTED;     // cannot happen within the limits
        rs.r[r] = RsRatio{L, M, W, half, tile, off, base_off, L * W <= RS_TABLE ? 1 : 0};
        base_off += L;
        const long long n = ((long long)in_stride * L + M - 1) / M;
        need = n > need ? n : need;
        const long long t = ((long long)out_stride + tile - 1) / tile;
        tiles = t > tiles ? t : tiles;
    }
    for (int r = n_ratios; r < RS_MAX_RATIOS; ++r) rs.r[r] = RsRatio{1, 1, 0, 0, RS_MAX_TILE, 0, 0, 0};
    if (out_stride < need) return PGASR_ERR_INVALID_ARG;
    // a row without a ratio is zeroed in tiles of RS_MAX_TILE, no larger than any ratio's: `tiles` covers it
    if (tiles * (long long)B > 2147483647LL) return PGASR_ERR_UNSUPPORTED;
    const bool vec = in_stride % 4 == 0 && ((uintptr_t)wave & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(tiles * B));
    if (vec)
        PGASR_LAUNCH_KERNEL(resample_kernel<true>, grid, dim3(RS_THREADS), 0, st, wave, in_stride, n_in, ratio_idx, n_ratios, rs,
                            tables, bases, out, out_stride, n_out, (int)tiles);
    else
        PGASR_LAUNCH_KERNEL(resample_kernel<false>, grid, dim3(RS_THREADS), 0, st, wave, in_stride, n_in, ratio_idx, n_ratios, rs,
                            tables, bases, out, out_stride, n_out, (int)tiles);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
