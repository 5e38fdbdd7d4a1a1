// Lattice-free CTC scorer for gfx950 (include/pgasr_hip.h, A12-SCORE): the exact -log p(y | x) of every hypothesis of an N-best
// list, one fp64 number per hypothesis, no workspace.
//
// It is the forward half of ctc.hip's ctc_lattice_body: one workgroup of 256 threads per (utterance, hypothesis) pair, the two
// alpha rows in LDS with two guard cells on each side, one LDS-only barrier per frame, the next frame's emissions gathered one
// frame ahead, a states-per-thread variant picked per pair from its own length.  What the lattice needs for the gradient is gone:
// no storer wave, no beta sweep, no label lists, nothing written but the result.  That lifts the limits the lattice's roles
// impose: any V <= 1024 (the label lists held V <= 64), any N <= 128 (the workspace held K <= 16).
//
// Numerics.  The lattice's lse3 takes exp and log in fp32 on the differences to the maximum, ~1e-7 absolute per frame: right for a
// gradient, and what holds its nll to 1e-5 relative.  A score that re-ranks hypotheses whose likelihoods differ in the sixth digit
// is held to 1e-9 relative against an fp64 statement instead (tests/hyp_score_ref.py).  The first version here was that lse3 with
// fp64 exp and log: three exp and a log of ~40 fp64 instructions each per state and frame, 5.8 ms where the lattice call takes 3.2
// (NOTES.md 0.27) -- bound by the fp64 issue rate, not by latency.  So the sweep runs in the LINEAR domain instead, which needs no
// logarithm per state and one exponential, off the dependent chain:
//     alpha_t(s) = p_t(s) * (alpha_{t-1}(s) + alpha_{t-1}(s-1) + [skip] alpha_{t-1}(s-2))
// with every alpha an fp64 fraction and an int32 binary exponent of its own (f * 2^e, re-normalised every frame), so nothing
// ever underflows however far a state lies below its row's maximum: ctc.hip's round-5 note names that as what a linear lattice
// with one exponent per lane runs into.  p_t(s) = exp(lp) is split the same way, exp(r) * 2^k with |r| <= ln2 / 2, before the
// frame's barrier.  Each step rounds a few times at 2^-53 relative; the one log is taken by thread 0 at the end.
// A value below 2^-(2^30) is flushed to zero: an nll above 7.4e8 nats reads +inf.
//
// Grid: b major, n minor.  All hypotheses of one utterance gather from the same (T, V) slab of log_probs, so workgroups that
// are neighbours in the dispatch order share its cache lines (a frame row is 4 KB at V = 1024).
#include "common.h"

namespace {

constexpr int HS_THREADS = 256;
constexpr int HS_SPT = 8;                        // states per thread -> 2 * Lh + 1 <= 2048
constexpr int HS_SMAX = HS_THREADS * HS_SPT;
constexpr int HS_NMAX = 128;                     // rows of a list (pgasr_nbest_rescore's limit)
constexpr int HS_EZERO = -(1 << 30);             // the exponent of zero: below every exponent a non-zero value may carry
constexpr int HS_EMAX = 1 << 30;

// exp(lp) = f * 2^e with f in (0.70, 1.42); (0, HS_EZERO) for lp = -inf.  k = rint(x / ln2), r = x - k ln2 in two steps
// (Cody-Waite), exp(r) by its Taylor series to r^13 (|r| <= 0.3466: the remainder is below 1e-17 relative).  The two clamps only
// bite on log-probs no softmax produces (|x| > 7e8, where k and r stop being exact); they keep f finite and e in range there.
__device__ __forceinline__ void exp_split(float lp, double& f, int& e) {
    const double x = (double)lp;
    double k = rint(x * 1.4426950408889634);
    k = fmin(fmax(k, (double)HS_EZERO), (double)HS_EMAX);
    double r = fma(-k, 6.93147180369123816490e-01, x);
    r = fma(-k, 1.90821492927058770002e-10, r);
    r = fmin(fmax(r, -0.35), 0.35);
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    const bool zero = (lp == -INFINITY);
    f = zero ? 0.0 : p;
    e = zero ? HS_EZERO : (int)k;
}

// f * 2^e -> fraction in [0.5, 1) and exponent; zero, and anything at or below 2^HS_EZERO, becomes (0, HS_EZERO)
__device__ __forceinline__ void renorm(double v, long long e, double& f, int& eo) {
    const double m = __builtin_amdgcn_frexp_mant(v);
    long long E = e + (long long)__builtin_amdgcn_frexp_exp(v);
    E = E > HS_EMAX ? HS_EMAX : E;
    const bool zero = (v == 0.0) || E <= HS_EZERO;
    f = zero ? 0.0 : m;
    eo = zero ? HS_EZERO : (int)E;
}

// LDS-only barrier: __syncthreads() would also drain vmcnt, the emission prefetch of the next frame
#define ROW_BARRIER() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); \
                           asm volatile("" ::: "memory"); } while (0)

// The alpha sweep of ONE hypothesis over its utterance's Tb frames; thread 0 writes the result.  lpb = log_probs + b * V (frame t
// at lpb + t * fstride), tgt the hypothesis' Lb tokens (nothing behind them is read), rf / re the kernel's LDS blocks of at
// least 2 * (NSPT * HS_THREADS + 4) fractions and exponents.  Bounds: every gather index is a label in [0, V) (a token outside it
// selects the blank and makes the result +inf), every frame index is below Tb <= T, every token index below Lb <= hyp_stride,
// every row position is s + 2 - {0, 1, 2} with s < NSPT * HS_THREADS.
template <int NSPT>
__device__ __forceinline__ void hyp_score_body(const float* __restrict__ lpb, size_t fstride, const int32_t* __restrict__ tgt,
                                               int Tb, int Lb, int V, int blank, double* __restrict__ rf, int* __restrict__ re,
                                               double* __restrict__ out) {
    const int tid = threadIdx.x;
    const int S = 2 * Lb + 1;
    constexpr int ROW = NSPT * HS_THREADS + 4;      // position p = s + 2
    for (int i = tid; i < 2 * ROW; i += HS_THREADS) { rf[i] = 0.0; re[i] = HS_EZERO; }

    int lab[NSPT];
    bool skip[NSPT];
    int bad = 0;
#pragma unroll
    for (int j = 0; j < NSPT; ++j) {
        const int s = tid + j * HS_THREADS;
        lab[j] = blank; skip[j] = false;
        if (s < S && (s & 1)) {
            const int c = tgt[s >> 1];
            if (c < 0 || c >= V || c == blank) bad = 1;
            else lab[j] = c;
            if (s >= 3) skip[j] = (c != tgt[(s >> 1) - 1]);
        }
    }
    if (__syncthreads_or(bad)) {                    // uniform: a token that is the blank or no symbol at all
        if (tid == 0) *out = INFINITY;
        return;
    }
    if (Tb == 0) {
        if (tid == 0) *out = (Lb == 0) ? 0.0 : INFINITY;
        return;
    }

#pragma unroll
    for (int j = 0; j < NSPT; ++j) {                // frame 0: states 0 and 1
        const int s = tid + j * HS_THREADS;
        if (s < S && s <= 1) {
            double pf; int pe;
            exp_split(lpb[lab[j]], pf, pe);
            renorm(pf, pe, rf[s + 2], re[s + 2]);
        }
    }
    int cur = 0;
    float lpn[NSPT];
#pragma unroll
    for (int j = 0; j < NSPT; ++j) lpn[j] = 0.f;
    if (Tb > 1) {
        const float* lpt = lpb + fstride;
#pragma unroll
        for (int j = 0; j < NSPT; ++j) lpn[j] = lpt[lab[j]];
    }
    for (int t = 1; t < Tb; ++t) {
        double pf[NSPT];
        int pe[NSPT];
#pragma unroll
        for (int j = 0; j < NSPT; ++j) exp_split(lpn[j], pf[j], pe[j]);       // this frame's emissions: off the dependent chain
        if (t + 1 < Tb) {                           // the next frame's: in flight across the barrier
            const float* lpt = lpb + (size_t)(t + 1) * fstride;
#pragma unroll
            for (int j = 0; j < NSPT; ++j) lpn[j] = lpt[lab[j]];
        }
        ROW_BARRIER();
        const double* fc = rf + cur * ROW;
        const int* ec = re + cur * ROW;
        double* fn = rf + (cur ^ 1) * ROW;
        int* en = re + (cur ^ 1) * ROW;
#pragma unroll
        for (int j = 0; j < NSPT; ++j) {
            // no test on the chain: all three neighbours are read (guard cells), a state that may not skip selects zero, and a
            // thread past S writes zero
            const int s = tid + j * HS_THREADS;
            const int p = s + 2;
            const double f0 = fc[p], f1 = fc[p - 1], f2 = skip[j] ? fc[p - 2] : 0.0;
            const int e0 = ec[p], e1 = ec[p - 1], e2 = skip[j] ? ec[p - 2] : HS_EZERO;
            const int em = max(e0, max(e1, e2));
            const double sum = ldexp(f0, e0 - em) + ldexp(f1, e1 - em) + ldexp(f2, e2 - em);      // differences >= -2^31: no overflow
            double fo; int eo;
            renorm(sum * pf[j], (long long)em + pe[j], fo, eo);
            fn[p] = (s < S) ? fo : 0.0;
            en[p] = (s < S) ? eo : HS_EZERO;
        }
        cur ^= 1;
    }
    __syncthreads();
    if (tid == 0) {
        const double* fc = rf + cur * ROW;
        const int* ec = re + cur * ROW;
        const double fa = fc[S - 1 + 2], fb = (S > 1) ? fc[S - 2 + 2] : 0.0;
        const int ea = ec[S - 1 + 2], eb = (S > 1) ? ec[S - 2 + 2] : HS_EZERO;
        const int em = max(ea, eb);
        const double sum = ldexp(fa, ea - em) + ldexp(fb, eb - em);
        *out = (sum == 0.0) ? INFINITY : -fma((double)em, 6.93147180559945286227e-01, log(sum));
    }
}
#undef ROW_BARRIER

// grid (B * N): blockIdx.x = b * N + n, pair p = n * B + b in the list's (N, B) layout.  NMAX = the states-per-thread variant that
// holds 2 * Lh + 1 states and sizes the LDS blocks; a pair whose own 2 * len + 1 fits a smaller variant runs that one (a uniform
// branch per workgroup, read from hyp_len on the device: no host synchronisation).
template <int NMAX>
__global__ __launch_bounds__(HS_THREADS) void ctc_hyp_score_kernel(
    const float* __restrict__ lp, const int32_t* __restrict__ hyp, int hyp_stride, const int32_t* __restrict__ hyp_len,
    const int32_t* __restrict__ count, const int32_t* __restrict__ in_len, int T, int B, int V, int N, int Lh, int blank,
    double* __restrict__ out_nll) {
    __shared__ double rf[2 * (NMAX * HS_THREADS + 4)];
    __shared__ int re[2 * (NMAX * HS_THREADS + 4)];
    const int b = blockIdx.x / N, n = blockIdx.x - b * N;
    const size_t p = (size_t)n * B + b;
    int cnt = N;
    if (count) { cnt = count[b]; cnt = cnt < 0 ? 0 : (cnt > N ? N : cnt); }
    int len = 0;
    bool scored = n < cnt;
    if (scored) {
        len = hyp_len[p]; len = len < 0 ? 0 : len;
        scored = len <= Lh && len <= hyp_stride;
    }
    if (!scored) {                                  // beyond the list, or longer than the launch holds: no work
        if (threadIdx.x == 0) out_nll[p] = INFINITY;
        return;
    }
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    const int S = 2 * len + 1;
    const float* lpb = lp + (size_t)b * V;
    const size_t fstride = (size_t)B * V;
    const int32_t* tgt = hyp + p * (size_t)hyp_stride;
#define PGASR_SCORE_BODY(NS) hyp_score_body<NS>(lpb, fstride, tgt, Tb, len, V, blank, rf, re, out_nll + p)
    if constexpr (NMAX == 1) {
        PGASR_SCORE_BODY(1);
    } else if constexpr (NMAX == 2) {
        if (S <= HS_THREADS) PGASR_SCORE_BODY(1); else PGASR_SCORE_BODY(2);
    } else if constexpr (NMAX == 4) {
        if (S <= HS_THREADS) PGASR_SCORE_BODY(1); else if (S <= 2 * HS_THREADS) PGASR_SCORE_BODY(2); else PGASR_SCORE_BODY(4);
    } else {
        if (S <= HS_THREADS) PGASR_SCORE_BODY(1); else if (S <= 2 * HS_THREADS) PGASR_SCORE_BODY(2);
        else if (S <= 4 * HS_THREADS) PGASR_SCORE_BODY(4); else PGASR_SCORE_BODY(8);
    }
#undef PGASR_SCORE_BODY
}

}  // namespace

extern "C" int pgasr_ctc_hyp_score(const float* log_probs, const int32_t* hyp_tokens, int hyp_stride, const int32_t* hyp_len,
                                   const int32_t* count, const int32_t* input_lengths, int T, int B, int V, int N, int Lh, int blank,
                                   double* out_nll, void* stream) {
    if (!log_probs || !hyp_tokens || !hyp_len || !input_lengths || !out_nll) return PGASR_ERR_INVALID_ARG;
    if (T < 1 || B < 1 || N < 1 || hyp_stride < 1 || Lh < 0 || V < 1 || blank < 0 || blank >= V) return PGASR_ERR_INVALID_ARG;
    if (V > PGASR_MAX_VOCAB_WIDE || N > HS_NMAX || 2 * (long long)Lh + 1 > HS_SMAX) return PGASR_ERR_UNSUPPORTED;
    if ((long long)N * B > 0x7fffffffLL) return PGASR_ERR_UNSUPPORTED;       // one workgroup per pair in grid.x
    const int Smax = 2 * Lh + 1;
    hipStream_t st = (hipStream_t)stream;
#define PGASR_HYP_SCORE(NMAX) PGASR_LAUNCH_KERNEL(ctc_hyp_score_kernel<NMAX>, dim3((unsigned)(N * B)), dim3(HS_THREADS), 0, st, \
                        log_probs, hyp_tokens, hyp_stride, hyp_len, count, input_lengths, T, B, V, N, Lh, blank, out_nll)
    if (Smax <= HS_THREADS) PGASR_HYP_SCORE(1);
    else if (Smax <= 2 * HS_THREADS) PGASR_HYP_SCORE(2);
    else if (Smax <= 4 * HS_THREADS) PGASR_HYP_SCORE(4);
    else PGASR_HYP_SCORE(8);
#undef PGASR_HYP_SCORE
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
