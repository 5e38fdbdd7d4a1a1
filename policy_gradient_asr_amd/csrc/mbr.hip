// Minimum-Bayes-risk decoding over N-best lists on gfx950 (pgasr_nbest_pair_dist, pgasr_mbr_select; semantics in
// include/pgasr_hip.h, section A7-MBR).
//
// pgasr_nbest_pair_dist: the N x N Levenshtein distances inside each list, by Myers' bit-vector algorithm in Hyyro's block form
// (Myers, JACM 46(3) 1999; Hyyro, Nordic J. Computing 10(1) 2003).  One launch, one single-wave workgroup per (group of patterns,
// utterance):
//   * a wave holds 64 / TPP patterns with TPP lanes each (TPP = the power of two >= floor(N/2), so N = 16 packs eight patterns into
//     a wave and N = 128 gives every pattern a whole one; at most 8 patterns, which bounds the LDS at 8 * V * W words = 64 KB);
//   * the match masks Peq[c][w] of a pattern are built once, from one coalesced load and V ballots per 64-token chunk, and stay in
//     LDS for all lanes of the pattern;
//   * lane k of pattern n carries the pair (n, (n + k + 1) mod N): every unordered pair once, the same number of pairs per
//     pattern (the circular schedule), and writes dist[n][m] and dist[m][n]; its Pv / Mv of all blocks stay in registers, the
//     kernel body being instantiated on 1 / 2 / 4 / 8 / 16 blocks and chosen per wave from the longest pattern it runs;
//   * a lane reads its text four symbols ahead of the step that uses them and requests all masks of a step before the chain of
//     blocks waits for the first; nothing is exchanged between lanes in the loop.
// The score of a pattern with fewer blocks than the instantiation is taken where its last symbol lies (block (m-1)/64, bit
// (m-1)%64); the blocks above that one compute on masks of zeros and feed nothing back (carries only travel upwards), and a
// wave-uniform bound skips the blocks no pattern of the wave reaches.
//
// pgasr_mbr_select: one launch, one workgroup of 128 threads per utterance, fp64.  The sums of the statement are serial in index
// order (thread n owns risk[n]), every product and sum rounded once: tests/mbr_ref.py repeats them in numpy.
#include "common.h"
#include <cmath>

namespace {

constexpr int MB_NMAX = 128;
constexpr int MB_VMAX = 64;                               // as the search (csrc/beam.hip)
constexpr int MB_LMAX = 1024;                             // 16 blocks of 64 pattern positions
constexpr int MB_PPW_MAX = 8;                             // patterns per wave: 8 * 64 symbols * 16 blocks * 8 B = 64 KB of LDS at the limits

typedef unsigned long long u64;

// One text symbol against a pattern of up to W blocks (the recurrence of the header, hin carried as the two bits hp / hn).
template <int W>
__device__ __forceinline__ void myers_step(u64 (&Pv)[W], u64 (&Mv)[W], int& score, const u64* __restrict__ peq, int Ws, int V, int c,
                                           int wcap, int wl, u64 topmask) {
    const bool inr = (unsigned)c < (unsigned)V;           // a symbol outside [0, V) matches nothing
    const u64* row = peq + (size_t)(inr ? c : 0) * Ws;
    u64 eq[W];                                             // every mask of the step is requested before the chain waits for the first
#pragma unroll
    for (int w = 0; w < W; ++w) eq[w] = row[w < wcap ? w : 0];                 // a block past wcap: block 0 again, in bounds and not used
    u64 hp = 1ull, hn = 0ull;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        if (w >= wcap) continue;                           // wave-uniform; no break: a loop with a run-time trip count would index Pv / Mv dynamically
        u64 Eq = inr ? eq[w] : 0ull;
        const u64 pv = Pv[w], mv = Mv[w];
        const u64 Xv = Eq | mv;
        Eq |= hn;
        const u64 Xh = (((Eq & pv) + pv) ^ pv) | Eq;
        u64 Ph = mv | ~(Xh | pv);
        u64 Mh = pv & Xh;
        const u64 tm = (w == wl) ? topmask : 0ull;
        score += (int)((Ph & tm) != 0ull) - (int)((Mh & tm) != 0ull);
        const u64 hp_out = Ph >> 63, hn_out = Mh >> 63;
        Ph = (Ph << 1) | hp;
        Mh = (Mh << 1) | hn;
        Pv[w] = Mh | ~(Xv | Ph);
        Mv[w] = Ph & Xv;
        hp = hp_out; hn = hn_out;
    }
}

template <int W>
__device__ __forceinline__ int myers_pair(const u64* __restrict__ peq, int Ws, int V, const int32_t* __restrict__ text, int tlen,
                                          int tmax, int m, int wcap) {
    u64 Pv[W], Mv[W];
#pragma unroll
    for (int w = 0; w < W; ++w) { Pv[w] = ~0ull; Mv[w] = 0ull; }
    int score = m;
    const int wl = (m - 1) >> 6;                           // m == 0: -1, no block adds to the score; the caller returns the text's length
    const u64 topmask = 1ull << ((m - 1) & 63);
    int c0 = 0 < tlen ? text[0] : -1, c1 = 1 < tlen ? text[1] : -1, c2 = 2 < tlen ? text[2] : -1, c3 = 3 < tlen ? text[3] : -1;
    for (int i = 0; i < tmax; i += 4) {                    // tmax: wave-uniform
        const int n0 = i + 4 < tlen ? text[i + 4] : -1, n1 = i + 5 < tlen ? text[i + 5] : -1;
        const int n2 = i + 6 < tlen ? text[i + 6] : -1, n3 = i + 7 < tlen ? text[i + 7] : -1;
        if (i < tlen) myers_step<W>(Pv, Mv, score, peq, Ws, V, c0, wcap, wl, topmask);
        if (i + 1 < tlen) myers_step<W>(Pv, Mv, score, peq, Ws, V, c1, wcap, wl, topmask);
        if (i + 2 < tlen) myers_step<W>(Pv, Mv, score, peq, Ws, V, c2, wcap, wl, topmask);
        if (i + 3 < tlen) myers_step<W>(Pv, Mv, score, peq, Ws, V, c3, wcap, wl, topmask);
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
    return score;
}

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int x = __shfl_xor(v, o, 64); v = x > v ? x : v; }
    return __builtin_amdgcn_readfirstlane(v);              // every lane holds the maximum: hand it to the scalar unit
}

// grid (B, ceil(N / ppw)), 64 threads; dynamic LDS: ppw * V * Ws words of 8 bytes, Ws = max(1, ceil(Lmax / 64)).
__global__ __launch_bounds__(64) void nbest_pair_dist_kernel(
    const int32_t* __restrict__ tokens, int tok_stride, const int32_t* __restrict__ len, const int32_t* __restrict__ count,
    int N, int B, int V, int Lmax, int Ws, int tpp, int ppw, int32_t* __restrict__ dist) {
    extern __shared__ u64 s_peq[];                         // [slot][symbol][block]
    const int b = blockIdx.x, first = blockIdx.y * ppw, lane = threadIdx.x;
    int cnt = count[b]; cnt = cnt < 0 ? 0 : (cnt > N ? N : cnt);
    const int half = N >> 1;
    const int slot = lane / tpp, k = lane % tpp + 1;
    const int n = first + slot;

    // this lane's pattern n and text m = n + k (mod N)
    const bool has_pat = slot < ppw && n < N;
    const bool has_pair = has_pat && k <= half && !((N & 1) == 0 && k == half && n >= half);
    const int m = has_pair ? (n + k) % N : (has_pat ? n : 0);
    int Ln = 0, Lm = 0;
    bool vn = false, vm = false;
    if (has_pat) {
        Ln = len[(size_t)n * B + b]; Ln = Ln < 0 ? 0 : (Ln > tok_stride ? tok_stride : Ln);
        vn = n < cnt && Ln <= Lmax;
    }
    if (has_pair) {
        Lm = len[(size_t)m * B + b]; Lm = Lm < 0 ? 0 : (Lm > tok_stride ? tok_stride : Lm);
        vm = m < cnt && Lm <= Lmax;
    }
    const bool run = has_pair && vn && vm;

    // the match masks of the wave's valid patterns; the blocks behind a pattern's length are zeros
    const int wcap = (wave_max_i32(run ? Ln : 0) + 63) >> 6;             // blocks the longest pattern of a running pair needs
    for (int s = 0; s < ppw; ++s) {                                     // wave-uniform
        const int pn = first + s;
        if (pn >= cnt) break;
        int L = len[(size_t)pn * B + b]; L = L < 0 ? 0 : (L > tok_stride ? tok_stride : L);
        if (L > Lmax) continue;
        const int32_t* tk = tokens + ((size_t)pn * B + b) * tok_stride;
        for (int w = 0; w < wcap; ++w) {
            const int i = w * 64 + lane;
            const int t = i < L ? tk[i] : -1;
            u64 mine = 0ull;
            for (int v = 0; v < V; ++v) {
                const u64 mk = __ballot(t == v);
                if (lane == v) mine = mk;
            }
            if (lane < V) s_peq[((size_t)s * V + lane) * Ws + w] = mine;
        }
    }
    __syncthreads();

    int d = -1;
    if (run) d = Ln == 0 ? Lm : Ln;                       // an empty pattern: the text's length; an empty text: the pattern's
    const int tlen = run && Ln > 0 ? Lm : 0;
    const int tmax = wave_max_i32(tlen);
    if (tmax > 0) {
        const u64* peq = s_peq + (size_t)(slot < ppw ? slot : 0) * V * Ws;
        const int32_t* text = tokens + ((size_t)m * B + b) * tok_stride;
        int sc;
        if (wcap <= 1) sc = myers_pair<1>(peq, Ws, V, text, tlen, tmax, Ln, wcap);
        else if (wcap <= 2) sc = myers_pair<2>(peq, Ws, V, text, tlen, tmax, Ln, wcap);
        else if (wcap <= 4) sc = myers_pair<4>(peq, Ws, V, text, tlen, tmax, Ln, wcap);
        else if (wcap <= 8) sc = myers_pair<8>(peq, Ws, V, text, tlen, tmax, Ln, wcap);
        else sc = myers_pair<16>(peq, Ws, V, text, tlen, tmax, Ln, wcap);
        if (run && Ln > 0) d = sc;
    }
    int32_t* out = dist + (size_t)b * N * N;
    if (has_pair) {
        out[(size_t)n * N + m] = d;
        out[(size_t)m * N + n] = d;
    }
    if (has_pat && k == 1) out[(size_t)n * N + n] = vn ? 0 : -1;
}

__global__ __launch_bounds__(MB_NMAX) void mbr_select_kernel(
    const int32_t* __restrict__ dist, const double* __restrict__ score, const int32_t* __restrict__ count, int N, int B, double scale,
    double* __restrict__ posterior, double* __restrict__ risk, int32_t* __restrict__ best) {
    __shared__ double s_score[MB_NMAX], s_w[MB_NMAX], s_p[MB_NMAX], s_risk[MB_NMAX];
    __shared__ int s_valid[MB_NMAX];
    const int b = blockIdx.x, n = threadIdx.x;
    int cnt = count[b]; cnt = cnt < 0 ? 0 : (cnt > N ? N : cnt);
    const int32_t* d = dist + (size_t)b * N * N;
    bool valid = false;
    double s = INFINITY;
    if (n < N) {
        s = score[(size_t)n * B + b];
        valid = n < cnt && std::isfinite(s) && d[(size_t)n * N + n] >= 0;
    }
    s_score[n] = s;
    s_valid[n] = valid ? 1 : 0;
    __syncthreads();
    double mn = INFINITY;
    for (int j = 0; j < N; ++j)
        if (s_valid[j]) mn = fmin(mn, s_score[j]);
    double w = 0.0;
    if (valid) {
        // plain operators under contract(off): see csrc/nbest.hip
#pragma clang fp contract(off)
        const double diff = s - mn;
        const double t = scale * diff;
        w = exp(-t);
    }
    s_w[n] = w;
    __syncthreads();
    double z = 0.0;
    for (int j = 0; j < N; ++j)
        if (s_valid[j]) z += s_w[j];
    const double p = valid ? w / z : 0.0;
    s_p[n] = p;
    __syncthreads();
    double r = INFINITY;
    if (valid) {
#pragma clang fp contract(off)
        double acc = 0.0;
        for (int j = 0; j < N; ++j)
            if (s_valid[j]) {
                const double term = s_p[j] * (double)d[(size_t)n * N + j];
                acc = acc + term;
            }
        r = acc;
    }
    s_risk[n] = r;
    if (n < N) {
        posterior[(size_t)n * B + b] = p;
        risk[(size_t)n * B + b] = r;
    }
    __syncthreads();
    if (n == 0) {
        int arg = 0;
        bool found = false;
        double least = INFINITY;
        for (int j = 0; j < N; ++j)
            if (s_valid[j] && (!found || s_risk[j] < least)) { found = true; least = s_risk[j]; arg = j; }
        best[b] = arg;
    }
}

}  // namespace

extern "C" int pgasr_nbest_pair_dist(const int32_t* tokens, int tok_stride, const int32_t* len, const int32_t* count,
                                     int N, int B, int V, int Lmax, int32_t* dist, void* stream) {
    if (N < 1 || N > MB_NMAX || V < 1 || V > MB_VMAX || Lmax < 0 || Lmax > MB_LMAX) return PGASR_ERR_UNSUPPORTED;
    if (!tokens || !len || !count || !dist || B < 1 || tok_stride < 1) return PGASR_ERR_INVALID_ARG;
    const int half = N / 2;
    int tpp = 1;
    while (tpp < half) tpp *= 2;                           // lanes per pattern: 1 .. 64
    int ppw = 64 / tpp;
    if (ppw > MB_PPW_MAX) ppw = MB_PPW_MAX;
    if (ppw > N) ppw = N;
    const int Ws = Lmax > 0 ? (Lmax + 63) / 64 : 1;
    const size_t lds = (size_t)ppw * V * Ws * sizeof(u64);
    PGASR_LAUNCH_KERNEL(nbest_pair_dist_kernel, dim3(B, (N + ppw - 1) / ppw), dim3(64), lds, (hipStream_t)stream, tokens, tok_stride,
                       len, count, N, B, V, Lmax, Ws, tpp, ppw, dist);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

extern "C" int pgasr_mbr_select(const int32_t* dist, const double* score, const int32_t* count, int N, int B, double scale,
                                double* posterior, double* risk, int32_t* best, void* stream) {
    if (N < 1 || N > MB_NMAX) return PGASR_ERR_UNSUPPORTED;
    if (!dist || !score || !count || !posterior || !risk || !best || B < 1) return PGASR_ERR_INVALID_ARG;
    if (!std::isfinite(scale) || scale < 0.0) return PGASR_ERR_INVALID_ARG;
    PGASR_LAUNCH_KERNEL(mbr_select_kernel, dim3(B), dim3(MB_NMAX), 0, (hipStream_t)stream, dist, score, count, N, B, scale, posterior,
                       risk, best);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
