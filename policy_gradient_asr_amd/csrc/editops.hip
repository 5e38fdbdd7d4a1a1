// Edit-operation alignment for gfx950 (include/pgasr_hip.h, A10-OPS): per (reference, hypothesis) pair the hit / substitution /
// deletion / insertion counts, the left-to-right operation string and a confusion matrix, under ONE contractual tie rule.
//
// One wave per pair, four pairs per workgroup.  Three phases per wave:
//
//  (1) forward: the register-row DP of editdist.hip (J consecutive cells per lane, min-plus prefix scan per row; the longer
//      sequence lies across the lanes, the shorter one is the serial chain).  After a row every lane has up, diagonal, left and
//      new of its cells (the left neighbour of a lane's first cell is exc + j0 - 1, which the scan has already produced), so it
//      emits a 2-bit choice per cell: 0 diagonal hit, 3 diagonal substitution, 1 left, 2 up.  The contract prefers the diagonal,
//      then the DELETION (a step back in the reference), then the insertion; a deletion is "left" when the reference lies across
//      the lanes and "up" after the swap, so the second test follows the swap.
//      The codes go to the workspace a quarter byte per cell, in words a lane fills by itself -- no shuffle: for J < 16 a word is a
//      tile of J columns x 16/J rows (one coalesced 256-byte store per 16/J rows), for J >= 16 a word is 16 columns of one row.
//  (2) backtrace: a dependent walk of at most n + m steps, held in scalar registers.  The 64 lanes fetch a WINDOW of 64 code
//      words -- 32 x 32 cells ending at the current cell -- in one memory round trip; every step then picks its word with
//      v_readlane.  The walk leaves a window after at least 17 steps, so a pair costs at most (n + m) / 17 + 1 dependent loads.
//      A step is ~50 scalar instructions and no branch but the window test (code -> operation and code -> step are look-ups in
//      constants).  The operations come out reversed and are packed, sixteen to a word, into the wave's 2 KB of LDS.
//  (3) output: the operation string turned left to right (coalesced byte stores, -1 from n_ops on), substitutions and deletions
//      counted off it by all lanes (hits and insertions follow from H + S + D = n, H + S + I = m), n_ops, and the
//      confusion matrix: each lane takes a contiguous piece of the string, a wave scan of the pieces' reference / hypothesis
//      symbol counts gives its start, and the entries are added to an LDS-private int32 matrix that the workgroup flushes once,
//      non-zero entries only, with 64-bit vector atomics.
#include "common.h"
#include <type_traits>

namespace {

constexpr int EO_BIG = 0x3fffffff;
constexpr int EO_WAVES = 4;            // pairs per workgroup
constexpr int EO_MAX_VOCAB = 64;
constexpr int EO_MAX_LEN = 4095;
constexpr int EO_REV_WORDS = 512;      // 2 * 4095 operations, sixteen to a word

// cells per lane for the longer stride, as editdist.hip picks them
inline int eo_cells_per_lane(int col_max) {
    const int need = (col_max + 1 + 63) / 64;
    int J = 1;
    while (J < need) J <<= 1;
    return J;
}

// code words of one pair: rows_max rows of 64 * J cells; always a multiple of 64 words, so pairs never share a 256-byte line
inline size_t eo_pair_words(int J, int rows_max) {
    if (J < 16) {
        const int TR = 16 / J;
        return (size_t)((rows_max + TR - 1) / TR) * 64;
    }
    return (size_t)rows_max * (J / 16) * 64;
}

template <int J>
__global__ __launch_bounds__(64 * EO_WAVES) void edit_ops_kernel(
    const int32_t* __restrict__ ref, const int32_t* __restrict__ ref_len, int ref_stride,
    const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len, int hyp_stride, int N,
    int32_t* __restrict__ counts, int8_t* __restrict__ ops, int32_t* __restrict__ n_ops,
    unsigned long long* __restrict__ confusion, int vocab, uint32_t* __restrict__ ws, size_t pair_words) {
    constexpr int TC = J < 16 ? J : 16;        // columns of a code word
    constexpr int TR = 16 / TC;                // rows of a code word
    constexpr int WPL = J < 16 ? 1 : J / 16;   // words per lane and row (J >= 16)
    constexpr int WC = 32 / TC;                // window: WC x WR words = 32 x 32 cells
    constexpr int WR = 64 / WC;
    __shared__ uint32_t rev_all[EO_WAVES][EO_REV_WORDS];
    __shared__ int cm[(EO_MAX_VOCAB + 1) * (EO_MAX_VOCAB + 1)];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pair = blockIdx.x * EO_WAVES + wave;
    const int V1 = vocab + 1;
    if (confusion) {
        for (int e = threadIdx.x; e < V1 * V1; e += 64 * EO_WAVES) cm[e] = 0;
        __syncthreads();
    }

    if (pair < N) {
        int n = ref_len[pair]; n = n < 0 ? 0 : (n > ref_stride ? ref_stride : n);
        int m = hyp_len[pair]; m = m < 0 ? 0 : (m > hyp_stride ? hyp_stride : m);
        const int32_t* r0 = ref + (size_t)pair * ref_stride;
        const int32_t* h0 = hyp + (size_t)pair * hyp_stride;
        const int32_t* r = r0;
        const int32_t* h = h0;
        // the longer sequence across the lanes (columns), the shorter one down the rows; the tie rule follows the swap
        const bool swapped = m > n;
        if (swapped) { r = h0; h = r0; const int tn = n; n = m; m = tn; }
        uint32_t* w = ws + (size_t)pair * pair_words;

        // ---- (1) forward ----
        const int j0 = lane * J;
        int rt[J];    // column token left of cell j; unused for j == 0 or j > n
        int prev[J];  // dp[i-1][j]
#pragma unroll
        for (int q = 0; q < J; ++q) {
            const int j = j0 + q;
            rt[q] = (j >= 1 && j <= n) ? r[j - 1] : -1;
            prev[q] = (j <= n) ? j : EO_BIG;
        }
        // the row loop once per way round (the choice is wave-uniform): the second test and its two codes are then compile-time
        auto forward = [&](auto swapped_t) {
        constexpr bool SW = decltype(swapped_t)::value;
        constexpr uint32_t second_hit = SW ? 2 : 1, second_miss = SW ? 1 : 2;
        uint32_t acc = 0;
        int hn = (m > 0) ? h[0] : 0;
        for (int i = 1; i <= m; ++i) {
            const int tok = hn;
            if (i < m) hn = h[i];
            const int left_prev = __shfl_up(prev[J - 1], 1, 64);  // dp[i-1][j0-1]
            int y[J];
            int diag = left_prev;
#pragma unroll
            for (int q = 0; q < J; ++q) {
                const int j = j0 + q;
                int x;
                if (j == 0) x = i;
                else if (j > n) x = EO_BIG;
                else x = min(prev[q] + 1, diag + (rt[q] != tok ? 1 : 0));
                diag = prev[q];
                y[q] = (q == 0) ? x : min(x, y[q - 1] + 1);
            }
            // exclusive cross-lane prefix-min of z = y[J-1] - (j0 + J - 1)
            int inc = y[J - 1] - (j0 + J - 1);
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(inc, o, 64);
                if (lane >= o) inc = min(inc, up);
            }
            int exc = __shfl_up(inc, 1, 64);
            if (lane == 0) exc = EO_BIG;
            const int rr = (i - 1) & (TR - 1);
            int dg = left_prev;          // dp[i-1][j-1]
            int lf = exc + j0 - 1;       // dp[i][j-1]: min over the lanes before of (x[k] - k), plus j0 - 1 (lane 0: column 0, unused)
            uint32_t cw = 0;
#pragma unroll
            for (int q = 0; q < J; ++q) {
                const int j = j0 + q;
                int v = y[q];
                if (exc < EO_BIG / 2) v = min(v, exc + j);
                const int up = prev[q];
                const int neq = rt[q] != tok ? 1 : 0;
                uint32_t code;
                if (dg + neq == v) code = neq ? 3u : 0u;
                else code = ((SW ? up : lf) + 1 == v) ? second_hit : second_miss;
                const int nv = (j <= n) ? v : EO_BIG;
                dg = up; lf = nv; prev[q] = nv;
                if (J < 16) {
                    acc |= code << ((rr * TC + q) * 2);
                } else {
                    cw |= code << ((q & 15) * 2);
                    if ((q & 15) == 15) { w[((size_t)(i - 1) * WPL + q / 16) * 64 + lane] = cw; cw = 0; }
                }
            }
            if (J < 16 && (rr == TR - 1 || i == m)) { w[(size_t)((i - 1) / TR) * 64 + lane] = acc; acc = 0; }
        }
        };
        if (swapped) forward(std::true_type{}); else forward(std::false_type{});
        // the wave reads back what other lanes of it stored
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

        // ---- (2) backtrace: (row, col) and every choice are wave-uniform ----
        uint32_t* rev = rev_all[wave];
        int row = __builtin_amdgcn_readfirstlane(m), col = __builtin_amdgcn_readfirstlane(n);
        // code -> operation: 0 hit, 3 substitution, left / up a deletion or an insertion by the swap; the step back in row / column
        const uint32_t op_left = swapped ? 3 : 2, op_up = swapped ? 2 : 3;
        const uint32_t op_lut = (op_left << 2) | (op_up << 4) | (1u << 6);
        int ga = -1, ta = 0;
        uint32_t win = 0;
        int K = 0;
        uint32_t oacc = 0;                            // scalar; every lane stores the same word (no exec juggling on the chain)
        auto emit = [&](uint32_t op) {
            oacc |= op << ((K & 15) * 2);
            ++K;
            if ((K & 15) == 0) { rev[(K >> 4) - 1] = oacc; oacc = 0; }
        };
        while (row > 0 && col > 0) {
            const int g = (row - 1) / TR, t = col / TC;     // tile row, tile column
            int wr = ga - g, wc = ta - t;
            if (ga < 0 || wr >= WR || wc >= WC) {
                ga = g; ta = t; wr = 0; wc = 0;
                const int g2 = ga - lane / WC, t2 = ta - lane % WC;
                win = 0;
                if (g2 >= 0 && t2 >= 0)
                    win = J < 16 ? w[(size_t)g2 * 64 + t2] : w[((size_t)g2 * WPL + t2 % WPL) * 64 + t2 / WPL];
            }
            const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)win, wr * WC + wc);
            const int bit = ((((row - 1) & (TR - 1)) * TC) + (col & (TC - 1))) * 2;
            const uint32_t code = (word >> bit) & 3u;
            emit((op_lut >> (code * 2)) & 3u);        // table look-ups in a constant, not branches: the chain is serial
            row -= (0xdu >> code) & 1u;               // every code but "left"
            col -= (0xbu >> code) & 1u;               // every code but "up"
        }
        while (col > 0) { emit(op_left); --col; }
        while (row > 0) { emit(op_up); --row; }
        if ((K & 15) != 0) rev[K >> 4] = oacc;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();

        // ---- (3) output ----
        auto op_at = [&](int k) {                     // k-th operation from the left
            const int t = K - 1 - k;
            return (int)((rev[t >> 4] >> ((t & 15) * 2)) & 3u);
        };
        const int ops_stride = ops ? ref_stride + hyp_stride : 0;
        int8_t* o = ops + (size_t)pair * ops_stride;
        int n_sub = 0, n_del = 0;
        for (int k = lane; k < max(K, ops_stride); k += 64) {
            int v = -1;
            if (k < K) { v = op_at(k); n_sub += v == 1; n_del += v == 2; }
            if (k < ops_stride) o[k] = (int8_t)v;
        }
#pragma unroll
        for (int x = 32; x > 0; x >>= 1) { n_sub += __shfl_xor(n_sub, x, 64); n_del += __shfl_xor(n_del, x, 64); }
        if (lane == 0) {
            const int n_ref = swapped ? m : n, n_hyp = swapped ? n : m;
            const int n_hit = n_ref - n_sub - n_del;          // H + S + D = n, H + S + I = m
            int32_t* c = counts + (size_t)pair * 4;
            c[0] = n_hit; c[1] = n_sub; c[2] = n_del; c[3] = n_hyp - n_hit - n_sub;
            if (n_ops) n_ops[pair] = K;
        }
        if (confusion) {
            const int ch = (K + 63) / 64;
            const int k0 = min(K, lane * ch), k1 = min(K, k0 + ch);
            int ci = 0, cj = 0;                       // reference / hypothesis symbols this lane's piece consumes
            for (int k = k0; k < k1; ++k) { const int op = op_at(k); ci += op != 3; cj += op != 2; }
            int si = ci, sj = cj;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int ui = __shfl_up(si, o, 64), uj = __shfl_up(sj, o, 64);
                if (lane >= o) { si += ui; sj += uj; }
            }
            int i = si - ci, j = sj - cj;
            for (int k = k0; k < k1; ++k) {
                const int op = op_at(k);
                const int a = op != 3 ? r0[i] : vocab, b = op != 2 ? h0[j] : vocab;
                i += op != 3; j += op != 2;
                if (a >= 0 && a <= vocab && b >= 0 && b <= vocab && (op == 3 || a < vocab) && (op == 2 || b < vocab))
                    atomicAdd(&cm[a * V1 + b], 1);
            }
        }
    }

    if (confusion) {
        __syncthreads();
        for (int e = threadIdx.x; e < V1 * V1; e += 64 * EO_WAVES) {
            const int v = cm[e];
            if (v) atomicAdd(confusion + e, (unsigned long long)v);
        }
    }
}

}  // namespace

extern "C" size_t pgasr_edit_ops_workspace_bytes(int ref_stride, int hyp_stride, int N) {
    if (ref_stride < 0 || hyp_stride < 0 || N <= 0) return 0;
    const int col_max = ref_stride > hyp_stride ? ref_stride : hyp_stride;
    const int rows_max = ref_stride > hyp_stride ? hyp_stride : ref_stride;
    if (col_max > EO_MAX_LEN) return 0;
    return (size_t)N * eo_pair_words(eo_cells_per_lane(col_max), rows_max) * sizeof(uint32_t);
}

extern "C" int pgasr_edit_ops(const int32_t* ref, const int32_t* ref_len, int ref_stride,
                              const int32_t* hyp, const int32_t* hyp_len, int hyp_stride, int N,
                              int32_t* counts, int8_t* ops, int32_t* n_ops, long long* confusion, int vocab,
                              void* workspace, size_t workspace_bytes, void* stream) {
    if (!ref_len || !hyp_len || !counts || N <= 0 || ref_stride < 0 || hyp_stride < 0) return PGASR_ERR_INVALID_ARG;
    if ((ref_stride > 0 && !ref) || (hyp_stride > 0 && !hyp)) return PGASR_ERR_INVALID_ARG;
    if (ops && !n_ops) return PGASR_ERR_INVALID_ARG;
    if (confusion && vocab < 1) return PGASR_ERR_INVALID_ARG;
    const int col_max = ref_stride > hyp_stride ? ref_stride : hyp_stride;
    const int rows_max = ref_stride > hyp_stride ? hyp_stride : ref_stride;
    if (col_max > EO_MAX_LEN) return PGASR_ERR_UNSUPPORTED;
    if (confusion && vocab > EO_MAX_VOCAB) return PGASR_ERR_UNSUPPORTED;
    const int J = eo_cells_per_lane(col_max);
    const size_t pair_words = eo_pair_words(J, rows_max);
    const size_t need = (size_t)N * pair_words * sizeof(uint32_t);
    if (need > 0 && (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 3) != 0)) return PGASR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((N + EO_WAVES - 1) / EO_WAVES), block(64 * EO_WAVES);
#define EO_LAUNCH(JJ)                                                                                              \
    PGASR_LAUNCH_KERNEL(edit_ops_kernel<JJ>, grid, block, 0, st, ref, ref_len, ref_stride, hyp, hyp_len, hyp_stride, N, \
                        counts, ops, n_ops, (unsigned long long*)confusion, confusion ? vocab : 0, (uint32_t*)workspace, pair_words)
    switch (J) {
        case 1: EO_LAUNCH(1); break;
        case 2: EO_LAUNCH(2); break;
        case 4: EO_LAUNCH(4); break;
        case 8: EO_LAUNCH(8); break;
        case 16: EO_LAUNCH(16); break;
        case 32: EO_LAUNCH(32); break;
        default: EO_LAUNCH(64); break;
    }
#undef EO_LAUNCH
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
