// CTC loss and gradient for gfx950.
//
// Two launches:
//   ctc_lattice_kernel : grid (B,3).  y=0 sweeps alpha forward in time, y=1 sweeps beta
//       backward, y=2 builds the label->states lists.  One workgroup per utterance and
//       direction, one lattice state per thread (strided when S > 256), one barrier per
//       frame, the previous row double-buffered in LDS.  The recursion is a serial chain of
//       T dependent steps, so this kernel is latency bound, not HBM bound.
//   ctc_grad_kernel    : one wave per (t,b): posterior occupancy per label from alpha+beta,
//       grad = scale_b * (softmax - occupancy) [+ REINFORCE term], fully parallel over T*B.
//
// Measured and NOT kept (round 3): a barrier-free lattice for S <= 256 -- one state per lane, neighbours by DPP wave_shr:1 /
// wave_shl:1, the four compute waves as a pipeline that hands only its two edge states per frame through an LDS ring with
// frame counters (prefetched a frame ahead), the storer following the counters four frames at a time.  Bit-identical, and
// no faster: 268-298 us against 272.  Switching its parts off one by one (diagnostic flags) showed why: without the
// neighbour exchange 278 us, without the storer 280, with the emissions prefetched 16 frames ahead 268, with cached
// emissions 283 -- and with ALL of these AND lse3 removed still 239 us, 0.24 us = ~570 cycles per frame for ~60 dependent
// instructions of one wave per SIMD.  The frame is bound by the dependent-issue latency of a single wave's instruction
// chain, not by the barrier, the LDS round trip, the emission loads or the stores; more waves do not shorten a chain.
//
// Measured and NOT kept (round 5, commit cdcbccd): a LINEAR-domain lattice for S <= 256 -- one compute wave per utterance and direction,
// four adjacent states per lane, alpha_t(s) = p_t(s) (alpha_{t-1}(s) + alpha_{t-1}(s-1) + [skip] alpha_{t-1}(s-2)) as two additions and a
// multiplication per state instead of an lse3, neighbours by DPP wave_shr / wave_shl, block floating point with one binary exponent per
// lane (re-based on the neighbour's when that is far above), a feeder wave turning log-probs into probabilities 32 frames at a time, three
// storer waves writing the same workspace format, a redo in log space when fp32's range empties the lattice.  Bit-for-bit the same nll to
// eight digits and all CTC tests green -- and 0.31 us per frame in fp64 (fp64 vector instructions issue at half rate), 0.31 in fp32 with
// per-frame renormalisation, 0.36 with exponents frozen for four frames, against 0.27 for the kernel below.  In-kernel clocks: 709 cycles per
// frame at 2.4 GHz for ~45 vector instructions, 490 with every LDS access removed: once more (see the round-3 note above) a frame of ONE
// wave costs the dependent-issue latency of its chain, ~13-20 cycles per dependent instruction, plus an LDS round trip -- shortening the
// arithmetic does not shorten that.  The lattice stays at 0.27 us per frame.
//
// Numerics: alpha/beta are kept in fp64 (adds/max are native fp64 VALU ops) while exp/log
// run in fp32 on the *differences* to the row maximum, which are O(1..50): absolute error
// per step ~1e-7 instead of the ~2e-4 ulp an fp32 log-space value of magnitude 3000 has at
// T=1000.  Sums over states are taken in a fixed order (wave butterfly, then list order), so
// results are run-to-run reproducible.
#include <type_traits>

#include "common.h"
#include "wide_rows.h"

namespace {

constexpr int CTC_THREADS = 256;
constexpr int CTC_SPT = 8;                        // states per thread -> S <= 2048
constexpr int CTC_SMAX = CTC_THREADS * CTC_SPT;   // 2048
constexpr int CTC_VMAX = 64;

struct CtcWs {
    // The lattice leaves the chip as fp32 OFFSETS from the row maximum plus one fp64 maximum per row (round 2): the rows
    // live in fp64 in LDS while the recursion runs (values reach -3000 at T = 1000, where fp32 resolves 2.4e-4), but
    // within a row only states within ~100 of the maximum carry any posterior mass, and there an fp32 offset resolves
    // < 1e-5.  Halves the lattice traffic of the round-1 fp64 spill (229 -> ~105 MB per step at B=32, T=1000, S=201).
    float* alpha;      // [B][T][SP]     alpha_t(s) - amax[t]   (-inf stays -inf); SP = Smax rounded up to 64: the storer
    float* beta;       // [B][T][SP]     beta_t(s)  - bmax[t]      writes whole 64-state groups, no bounds test per state
    int SP;
    double* amax;      // [B][T]         row maxima (0 for a row that is -inf everywhere)
    double* bmax;      // [B][T]
    double* nll64;     // [B]
    int32_t* lab_off;  // [B][V+1]   offsets into lab_states, per label
    int32_t* lab_states;  // [B][Smax] odd (non-blank) states grouped by label, ascending s
};

__host__ __device__ inline size_t ctc_ws_layout(int T, int B, int V, int Smax, CtcWs* ws, char* base) {
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const int SP = (Smax + 63) / 64 * 64;
    size_t a = take((size_t)B * T * SP * sizeof(float));
    size_t b = take((size_t)B * T * SP * sizeof(float));
    size_t am = take((size_t)B * T * sizeof(double));
    size_t bm = take((size_t)B * T * sizeof(double));
    size_t n = take((size_t)B * sizeof(double));
    size_t lo = take((size_t)B * (V + 1) * sizeof(int32_t));
    size_t ls = take((size_t)B * Smax * sizeof(int32_t));
    if (ws) {
        ws->alpha = (float*)(base + a); ws->beta = (float*)(base + b);
        ws->amax = (double*)(base + am); ws->bmax = (double*)(base + bm); ws->SP = SP;
        ws->nll64 = (double*)(base + n); ws->lab_off = (int32_t*)(base + lo);
        ws->lab_states = (int32_t*)(base + ls);
    }
    return off;
}

// max over the 64 lanes of a wave, in all lanes: DPP row rotations + four readlanes (a butterfly of ds_bpermute pairs costs
// six LDS-crossbar round trips, more than a lattice frame lasts)
template <int CTRL> __device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float wave_max_f32_all(float m) {
    m = fmaxf(m, dpp_f32<0x128>(m)); m = fmaxf(m, dpp_f32<0x124>(m));     // row_ror:8, :4
    m = fmaxf(m, dpp_f32<0x122>(m)); m = fmaxf(m, dpp_f32<0x121>(m));     // row_ror:2, :1 -> every lane holds its row's maximum
    const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 0)), b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 16));
    const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 32)), d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 48));
    return fmaxf(fmaxf(a, b), fmaxf(c, d));
}

// log(exp(a0)+exp(a1)+exp(a2)) with fp64 carries and fp32 transcendentals.
__device__ __forceinline__ double lse3(double a0, double a1, double a2) {
    const double m = fmax(fmax(a0, a1), a2);
    // no branch on the all -inf row (a select at the end instead): every taken branch on the T-step chain refills the
    // instruction buffer.  mz keeps the differences finite-or--inf when m = -inf.
    const double mz = (m == -INFINITY) ? 0.0 : m;
    const float s = __builtin_amdgcn_exp2f(1.4426950408889634f * (float)(a0 - mz)) + __builtin_amdgcn_exp2f(1.4426950408889634f * (float)(a1 - mz)) +
                    __builtin_amdgcn_exp2f(1.4426950408889634f * (float)(a2 - mz));
    // s is in [1, 3]: the bare v_log_f32 (log2) needs none of __logf's denormal / range fix-ups, which sat on the chain
    const double r = m + (double)(0.6931471805599453f * __builtin_amdgcn_logf(s));
    return (m == -INFINITY) ? -INFINITY : r;
}

// label -> states lists for the gradient pass (grid row y = 2 of the lattice launch)
__device__ __forceinline__ void ctc_labels_body(const int32_t* __restrict__ targets, const int32_t* __restrict__ tg_len,
                                                int V, int Lmax, int Smax, int blank, CtcWs ws) {
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    int Lb = tg_len[b]; Lb = Lb < 0 ? 0 : (Lb > Lmax ? Lmax : Lb);
    const int32_t* tgt = targets + (size_t)b * Lmax;
        // label -> list of odd states carrying it (ascending s).  One thread per label.
        __shared__ int cnt[CTC_VMAX + 1];
        if (tid <= V) cnt[tid] = 0;
        __syncthreads();
        if (tid < V) {
            int c = 0;
            if (tid != blank)
                for (int i = 0; i < Lb; ++i) c += (tgt[i] == tid);
            cnt[tid + 1] = c;
        }
        __syncthreads();
        if (tid == 0) {
            int run = 0;
            for (int v = 0; v <= V; ++v) { run += cnt[v]; cnt[v] = run; }  // cnt[v] = start of label v
            // after the loop cnt[v] holds the inclusive sum up to v; shift handled below
        }
        __syncthreads();
        // cnt[v] now = sum_{u<=v} count_u where count stored at u+1 => cnt[v] = start of label v
        if (tid <= V) ws.lab_off[(size_t)b * (V + 1) + tid] = cnt[tid];
        if (tid < V && tid != blank) {
            int w = cnt[tid];
            for (int i = 0; i < Lb; ++i)
                if (tgt[i] == tid) ws.lab_states[(size_t)b * Smax + (w++)] = 2 * i + 1;
        }
}

// LDS-only barrier: __syncthreads() would also drain vmcnt (the storer's stores, the emission prefetch)
#define ROW_BARRIER() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); \
                           asm volatile("" ::: "memory"); } while (0)

// The alpha (ROLE 0) or beta (ROLE 1) sweep of ONE label sequence over one utterance's frames: the body of both
// ctc_lattice_kernel (the targets) and ctc_hyp_lattice_kernel (the sampled hypotheses).  The caller resolves everything that
// depends on how its lattices are addressed: lpb = log_probs + b*V (frame t of the utterance at lpb + t*fstride), tgt / Tb / Lb
// the label row and the clamped lengths, out / outmax this lattice's alpha or beta rows [T][SP] and row references [T],
// nll64 / nll_out where ROLE 0 leaves the sequence's nll, rows the kernel's LDS block of 2 * (NSPT * CTC_THREADS + 4) doubles.
// NSPT = states per thread, a compile-time constant: the common case S <= 256 (L <= 127) runs with no per-state
// loop or bound checks on the T-step chain (measured 492 -> see DESIGN.md at T=1000, S=201).
template <int NSPT, int ROLE>
__device__ __forceinline__ void ctc_lattice_body(
    const float* __restrict__ lpb, size_t fstride, const int32_t* __restrict__ tgt, int Tb, int Lb, int V, int blank,
    float* __restrict__ out, int SP, double* __restrict__ outmax, double* __restrict__ nll64, float* __restrict__ nll_out,
    double* __restrict__ rows) {
    constexpr int role = ROLE;          // compile-time: the frame loop carries no direction test
    const int tid = threadIdx.x;
    const int S = 2 * Lb + 1;

    // row buffers: position p = s + 2, two guard cells of -inf on each side
    constexpr int ROW = NSPT * CTC_THREADS + 4;
    auto row = [&](int i) { return rows + i * ROW; };      // the two row buffers
    // Wave 4 is the STORER: it copies each finished row from LDS to the alpha/beta array.  With the store in the
    // compute threads the chain waited every step for the store's write acknowledgement: hipcc must use vmcnt(0)
    // for the emission prefetch as soon as a store is also outstanding (loads and stores retire out of order
    // with respect to each other) -- 391 us against 492 us before the NSPT template, see DESIGN.md.
    const bool storer = tid >= CTC_THREADS;
    for (int i = tid; i < 2 * ROW; i += CTC_THREADS + 64) rows[i] = -INFINITY;

    // per-thread state descriptors
    int lab[NSPT];
    bool skip[NSPT];   // alpha: may come from s-2 ; beta: may go to s+2
#pragma unroll
    for (int j = 0; j < NSPT; ++j) {
        const int s = storer ? S : tid + j * CTC_THREADS;       // the storer owns no state
        lab[j] = blank; skip[j] = false;
        if (s < S && (s & 1)) lab[j] = tgt[s >> 1];
        if (role == 0) {
            if (s < S && (s & 1) && s >= 3) skip[j] = (tgt[s >> 1] != tgt[(s >> 1) - 1]);
        } else {
            if (s + 2 < S && (s & 1)) skip[j] = (tgt[(s >> 1) + 1] != tgt[s >> 1]);
        }
        if (lab[j] < 0 || lab[j] >= V) lab[j] = blank;  // defensive: never index outside the row
    }
    __syncthreads();

    // the storer wave's row write: maximum over the row (fixed butterfly order), then fp32 offsets
    double m_ref = 0.0;          // the storer's current reference (refreshed every 4th row)
    auto store_row = [&](const double* rc, int t_row, bool refresh) {
        // Branch-free: the storer lane keeps 64-strided states in registers -- cells past S hold the -inf the rows were
        // initialised with, and the output rows are padded to whole 64-state groups -- so the only waits are the LDS reads.
        // (It sits at the same per-frame barrier as the compute waves: a slower storer would set the frame time.)
        constexpr int NG = NSPT * 4;
        const int ls = tid - CTC_THREADS;
        const int ng = (S + 63) >> 6;           // 64-state groups that hold states (wave-uniform)
        double v[NG];
#pragma unroll
        for (int i = 0; i < NG; ++i) v[i] = rc[ls + 64 * i + 2];
        // The reference of a row need not be its maximum, only NEAR it: offsets are formed in fp64 against whatever
        // reference is stored with the row.  It is refreshed every 4th row (a row maximum moves by one frame's log-prob
        // per frame, a few units; even 4 x 88 keeps the fp32 offset's resolution at 3e-5), and the wave reduction runs on
        // fp32 DPP maxima -- so three rows out of four cost the storer four reads, four subtractions and four stores.
        if (refresh) {
            double ml = -INFINITY;
#pragma unroll
            for (int i = 0; i < NG; ++i) ml = fmax(ml, v[i]);
            const double mw = (double)wave_max_f32_all((float)ml);
            m_ref = (mw == -INFINITY) ? 0.0 : mw;
        }
        const double m = m_ref;
        float* o = out + (size_t)t_row * SP + ls;
#pragma unroll
        for (int i = 0; i < NG; ++i)
            if (i < ng) o[64 * i] = (float)(v[i] - m);
        if (ls == 0) outmax[t_row] = m;
    };
    if (Tb == 0) {
        if (role == 0 && tid == 0) {
            const double v = (Lb == 0) ? 0.0 : INFINITY;
            *nll64 = v; *nll_out = (float)v;
        }
        return;
    }

    const int t0 = (role == 0) ? 0 : Tb - 1;
    const int dt = (role == 0) ? 1 : -1;

    // frame t0
    {
        const float* lpt = lpb + (size_t)t0 * fstride;
#pragma unroll
        for (int j = 0; j < NSPT; ++j) {
            const int s = storer ? S : tid + j * CTC_THREADS;
            if (s < S) {
                double v = -INFINITY;
                if (role == 0) { if (s <= 1) v = (double)lpt[lab[j]]; }
                else           { if (s >= S - 2) v = (double)lpt[lab[j]]; }
                row(0)[s + 2] = v;
            }
        }
    }
    int cur = 0;
    if (storer) {
        // its own loop (same number of barriers): nothing in this path ever waits for a store
        for (int k = 1; k < Tb; ++k) {
            ROW_BARRIER();
            store_row(row(cur), t0 + (k - 1) * dt, ((k - 1) & 3) == 0);      // row(cur) = frame t0 + (k-1)*dt, stable until the next barrier
            cur ^= 1;
        }
    } else {
        float lpn[NSPT];
#pragma unroll
        for (int j = 0; j < NSPT; ++j) lpn[j] = 0.f;
        if (Tb > 1) {
            const float* lpt = lpb + (size_t)(t0 + dt) * fstride;
#pragma unroll
            for (int j = 0; j < NSPT; ++j) lpn[j] = lpt[lab[j]];
        }
        for (int k = 1; k < Tb; ++k) {
            const int t = t0 + k * dt;
            float lpc[NSPT];
#pragma unroll
            for (int j = 0; j < NSPT; ++j) lpc[j] = lpn[j];
            if (k + 1 < Tb) {  // prefetch the next frame's emissions: off the dependent chain
                const float* lpt = lpb + (size_t)(t + dt) * fstride;
#pragma unroll
                for (int j = 0; j < NSPT; ++j) lpn[j] = lpt[lab[j]];
            }
            ROW_BARRIER();
            const double* rc = row(cur);
            double* rn = row(cur ^ 1);
#pragma unroll
            for (int j = 0; j < NSPT; ++j) {
                // no test on the chain: all three neighbours are read (guard cells on both sides), a state that may not
                // skip and a thread past S select -inf
                const int s = tid + j * CTC_THREADS;
                const int p = s + 2;
                const double a0 = rc[p];
                const double a1 = rc[role == 0 ? p - 1 : p + 1];
                const double a2r = rc[role == 0 ? p - 2 : p + 2];
                const double a2 = skip[j] ? a2r : -INFINITY;
                const double v = lse3(a0, a1, a2) + (double)lpc[j];
                rn[p] = (s < S) ? v : -INFINITY;
            }
            cur ^= 1;
        }
    }
    {                    // the last frame's row (the only one when Tb == 1)
        __syncthreads();
        if (storer) store_row(row(cur), t0 + (Tb - 1) * dt, ((Tb - 1) & 3) == 0);
    }
    if (role == 0) {
        __syncthreads();
        if (tid == 0) {
            const double* rc = row(cur);
            const double ll = lse3(rc[S - 1 + 2], (S > 1) ? rc[S - 2 + 2] : -INFINITY, -INFINITY);
            *nll64 = -ll;
            *nll_out = (float)(-ll);
        }
    }
}
#undef ROW_BARRIER

// grid (B,3): y = 0 alpha, y = 1 beta, y = 2 the label -> states lists; one LDS block serves whichever sweep the workgroup runs
template <int NSPT>
__global__ __launch_bounds__(CTC_THREADS + 64) void ctc_lattice_kernel(
    const float* __restrict__ lp, const int32_t* __restrict__ targets,
    const int32_t* __restrict__ in_len, const int32_t* __restrict__ tg_len,
    int T, int B, int V, int Lmax, int Smax, int blank, CtcWs ws, float* __restrict__ nll_out, int role_base) {
    __shared__ double rows[2 * (NSPT * CTC_THREADS + 4)];
    const int b = blockIdx.x;
    const int role = blockIdx.y + role_base;      // one uniform branch per workgroup, none per frame
    if (role >= 2) { ctc_labels_body(targets, tg_len, V, Lmax, Smax, blank, ws); return; }
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    int Lb = tg_len[b]; Lb = Lb < 0 ? 0 : (Lb > Lmax ? Lmax : Lb);
    const float* lpb = lp + (size_t)b * V;
    const size_t fstride = (size_t)B * V;
    const int32_t* tgt = targets + (size_t)b * Lmax;
    float* out = (role == 0 ? ws.alpha : ws.beta) + (size_t)b * T * ws.SP;
    double* outmax = (role == 0 ? ws.amax : ws.bmax) + (size_t)b * T;
    if (role == 0) ctc_lattice_body<NSPT, 0>(lpb, fstride, tgt, Tb, Lb, V, blank, out, ws.SP, outmax, ws.nll64 + b, nll_out + b, rows);
    else           ctc_lattice_body<NSPT, 1>(lpb, fstride, tgt, Tb, Lb, V, blank, out, ws.SP, outmax, ws.nll64 + b, nll_out + b, rows);
}

// The CTC part of one (t,b) row's gradient, utt_scale_b * (softmax - occupancy) in this lane (0 when no alignment exists);
// lpv / sm = this lane's log-prob / probability.  The one occupancy routine of the three gradient kernels below: b names the
// lattice in ws, so ctc_grad_seq_kernel calls it once more per sequence-scored hypothesis with the pair index and its workspace.
// (ctc_grad_kernel once kept these lines inline: stand-alone at B = 32, T = 1000 that form ran 31.2 us against 31.8 us with the
// call, and the step cannot tell them apart -- trace means 67.6 / 72.1 us inline, 71.3 us with the call; NOTES.md 0.07.)
__device__ __forceinline__ float ctc_grad_row(float lpv, float sm, int lane, int t, int b, int T, int V, int Lb, int Smax, int blank,
                                              CtcWs ws, const float* __restrict__ utt_scale) {
    float g = 0.f;
    const double nll = ws.nll64[b];
    if (nll != INFINITY) {
        const int S = 2 * Lb + 1;
        const float* al = ws.alpha + ((size_t)b * T + t) * ws.SP;
        const float* be = ws.beta + ((size_t)b * T + t) * ws.SP;
        // log occupancy of state s = (alpha offset + beta offset) + [row maxima + nll - log p]: the bracket is O(10)
        const double cst = ws.amax[(size_t)b * T + t] + ws.bmax[(size_t)b * T + t] + nll;
        // A symbol of probability exactly 0 at this frame (log p = -inf, a masked vocabulary) has occupancy 0: every state that
        // carries it holds alpha = beta = -inf, and the constant would read +inf -- -inf + inf = NaN, for the blank in all lanes
        // through wave_sum.  A select on the constant: exp(-inf + 0) = 0.  A finite log p keeps its bits.
        // blank occupancy: even states, all lanes, fixed butterfly order
        const float lpb = __shfl(lpv, blank, 64);
        const float cb = (lpb == -INFINITY) ? 0.f : (float)(cst - (double)lpb);
        float accb = 0.f;
        for (int s = 2 * lane; s < S; s += 128)
            accb += __expf((al[s] + be[s]) + cb);
        accb = wave_sum(accb);
        float occ = accb;
        if (lane < V && lane != blank) {
            const int32_t* lo = ws.lab_off + (size_t)b * (V + 1);
            const int32_t* ls = ws.lab_states + (size_t)b * Smax;
            float acc = 0.f;
            const float cl = (lpv == -INFINITY) ? 0.f : (float)(cst - (double)lpv);
            for (int i = lo[lane]; i < lo[lane + 1]; ++i) {
                const int s = ls[i];
                acc += __expf((al[s] + be[s]) + cl);
            }
            occ = acc;
        }
        const float sc = utt_scale ? utt_scale[b] : 1.f;
        g = sc * (sm - occ);
    }
    return g;
}

// ---- entropy regularisation of the frame policy (pgasr_frame_entropy and the *_ent gradient entries) ----
// H_{t,b} = -sum_v p_v ln p_v (nats) of row (t,b), from the row's log p and p as the gradient kernels hold them: one lane per symbol,
// lanes >= V with p = 0.  A symbol with p = 0 (ln p = -inf, or an exp that underflowed) adds exactly 0: no 0 * -inf.  One wave_sum in
// its fixed butterfly order; every lane returns p ln p of its own symbol and the row's H.
__device__ __forceinline__ float row_entropy(float lpv, float sm, float* plp) {
    *plp = sm > 0.f ? sm * lpv : 0.f;
    return -wave_sum(*plp);
}

// d(-ent_scale_b H_{t,b}) / d(logits) = ent_scale_b p (ln p + H), in the pass that writes the row: one wave_sum, one fma per lane.
// The three gradient kernels are templated <bool ENT, class... Ent>: the ENT instantiation takes ONE more argument after grad,
// `const float* ent_scale` (B), and adds this term last; the ENT = false instantiation has the argument list -- and the kernarg
// layout, implicit arguments included -- it had before the term existed.  (An empty struct in that place moved the implicit
// arguments by 8 bytes.)
__device__ __forceinline__ float ctc_entropy_grad(float lpv, float sm, int b, const float* __restrict__ ent_scale) {
    float plp;
    const float H = row_entropy(lpv, sm, &plp);
    return sm > 0.f ? ent_scale[b] * fmaf(sm, H, plp) : 0.f;
}

// ent_mean[b] = (1 / max(T_b,1)) sum_{t<T_b} H_{t,b} and ent_scale[b] = beta * inv_global_batch / max(T_b,1).  One workgroup of
// ENT_WAVES waves per utterance: wave w adds the entropies of frames w, w + ENT_WAVES, .. in t order (fp64 carries), wave 0 lane 0 adds
// the ENT_WAVES partial sums in w order -- a fixed order over v and t, so two calls give the same bits.
constexpr int ENT_WAVES = 16;
__global__ __launch_bounds__(64 * ENT_WAVES) void frame_entropy_kernel(
    const float* __restrict__ lp, const int32_t* __restrict__ in_len, int T, int B, int V, float beta, float inv_gb,
    float* __restrict__ ent_mean, float* __restrict__ ent_scale) {
    __shared__ double part[ENT_WAVES];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    double acc = 0.0;
    // four of the wave's frames per trip: their loads are in flight together, their entropies added in t order
    for (int t0 = w; t0 < Tb; t0 += 4 * ENT_WAVES) {
        float lpv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = t0 + i * ENT_WAVES;
            lpv[i] = (lane < V && t < Tb) ? lp[((size_t)t * B + b) * V + lane] : -INFINITY;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float plp;
            acc += (double)row_entropy(lpv[i], __expf(lpv[i]), &plp);      // a frame >= T_b reads as p = 0 everywhere: H = 0
        }
    }
    if (lane == 0) part[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < ENT_WAVES; ++i) s += part[i];
        const float n = (float)(Tb > 0 ? Tb : 1);
        ent_mean[b] = (float)(s / (double)n);
        ent_scale[b] = beta * inv_gb / n;
    }
}

// ---- KL penalty towards a frozen reference policy (pgasr_frame_kl and the *_kl gradient entries) ----
// KL_{t,b} = sum_v p_v (ln p_v - lnq_v) (nats) of row (t,b): the reverse KL(p || q) of the trained policy p against the reference's
// log-probs, lnq_v = max(ref_log_probs, PGASR_KL_LOG_FLOOR) -- a zero reference probability under a live policy symbol costs a large
// finite penalty, never inf or NaN.  A symbol with p = 0 adds exactly 0 (no 0 * inf), and q = p gives exactly 0 in every lane.  One
// wave_sum in its fixed butterfly order; every lane returns p (ln p - lnq) of its own symbol and the row's KL.
constexpr float KL_LOG_FLOOR = PGASR_KL_LOG_FLOOR;
__device__ __forceinline__ float row_kl(float lpv, float sm, float lqv, float* d) {
    *d = sm > 0.f ? sm * (lpv - fmaxf(lqv, KL_LOG_FLOOR)) : 0.f;
    return wave_sum(*d);
}

// The KL form of the three gradient kernels: their Ent pack holds three pointers, (ent_scale, ref_log_probs, kl_scale), with
// ent_scale nullable (one uniform branch per row).  After the entropy term it adds
// d(kl_scale_b KL_{t,b}) / d(logits) = kl_scale_b p (ln p - lnq - KL): a second row read, a second wave_sum, one fma per lane.  A lane
// whose term is 0 leaves g as it is, sign of zero included, so a reference equal to the policy gives the bits of the pass without it.
__device__ __forceinline__ float ctc_entropy_kl_grad(float g, float lpv, float sm, int lane, int V, int b, size_t o,
                                                     const float* __restrict__ ent_scale, const float* __restrict__ ref_lp,
                                                     const float* __restrict__ kl_scale) {
    if (ent_scale != nullptr) g += ctc_entropy_grad(lpv, sm, b, ent_scale);
    const float lqv = (lane < V) ? ref_lp[o + lane] : 0.f;
    float d;
    const float kl = row_kl(lpv, sm, lqv, &d);
    const float term = kl_scale[b] * fmaf(-sm, kl, d);
    return term != 0.f ? g + term : g;
}

// kl_mean[b] = (1 / max(T_b,1)) sum_{t<T_b} KL_{t,b} and kl_scale[b] = gamma * inv_global_batch / max(T_b,1): frame_entropy_kernel's
// structure with a second row load -- one workgroup of ENT_WAVES waves per utterance, wave w adds the KLs of frames w, w + ENT_WAVES, ..
// in t order (fp64 carries), wave 0 lane 0 adds the partial sums in w order, so two calls give the same bits.  Not clamped at 0.
__global__ __launch_bounds__(64 * ENT_WAVES) void frame_kl_kernel(
    const float* __restrict__ lp, const float* __restrict__ ref_lp, const int32_t* __restrict__ in_len, int T, int B, int V,
    float gamma, float inv_gb, float* __restrict__ kl_mean, float* __restrict__ kl_scale) {
    __shared__ double part[ENT_WAVES];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    double acc = 0.0;
    // four of the wave's frames per trip: their eight loads are in flight together, their KLs added in t order
    for (int t0 = w; t0 < Tb; t0 += 4 * ENT_WAVES) {
        float lpv[4], lqv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = t0 + i * ENT_WAVES;
            const bool live = lane < V && t < Tb;
            const size_t o = ((size_t)t * B + b) * V + lane;
            lpv[i] = live ? lp[o] : -INFINITY;
            lqv[i] = live ? ref_lp[o] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float d;
            acc += (double)row_kl(lpv[i], __expf(lpv[i]), lqv[i], &d);      // a frame >= T_b reads as p = 0 everywhere: KL = 0
        }
    }
    if (lane == 0) part[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < ENT_WAVES; ++i) s += part[i];
        const float n = (float)(Tb > 0 ? Tb : 1);
        kl_mean[b] = (float)(s / (double)n);
        kl_scale[b] = gamma * inv_gb / n;
    }
}

// The tail of a gradient kernel's row: nothing (ENT = false), the entropy term (one pointer in the pack) or entropy and KL (three).
template <bool ENT, class... Ent>
__device__ __forceinline__ float ctc_grad_tail(float g, float lpv, float sm, int lane, int V, int b, size_t o, Ent... ent) {
    static_assert(ENT ? (sizeof...(Ent) == 1 || sizeof...(Ent) == 3) : sizeof...(Ent) == 0,
                  "no pointer, ent_scale, or (ent_scale, ref_log_probs, kl_scale)");
    if constexpr (sizeof...(Ent) == 3) return ctc_entropy_kl_grad(g, lpv, sm, lane, V, b, o, ent...);
    else if constexpr (ENT) return g + ctc_entropy_grad(lpv, sm, b, ent...);
    else return g;
}

// one wave per (t,b)
template <bool ENT, class... Ent>
__global__ __launch_bounds__(256) void ctc_grad_kernel(
    const float* __restrict__ lp, const int32_t* __restrict__ in_len, const int32_t* __restrict__ tg_len,
    int T, int B, int V, int Lmax, int Smax, int blank, CtcWs ws,
    const float* __restrict__ utt_scale, const float* __restrict__ pg_coef,
    const int32_t* __restrict__ pg_path, int coef_per_frame, float* __restrict__ grad, Ent... ent_scale) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= (long long)T * B) return;
    const int t = (int)(w / B), b = (int)(w % B);
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    int Lb = tg_len[b]; Lb = Lb < 0 ? 0 : (Lb > Lmax ? Lmax : Lb);
    const size_t o = ((size_t)t * B + b) * V;
    if (t >= Tb) { if (lane < V) grad[o + lane] = 0.f; return; }

    const float lpv = (lane < V) ? lp[o + lane] : 0.f;
    const float sm = (lane < V) ? __expf(lpv) : 0.f;
    float g = ctc_grad_row(lpv, sm, lane, t, b, T, V, Lb, Smax, blank, ws, utt_scale);
    if (pg_coef != nullptr && pg_path != nullptr) {
        const int k = pg_path[(size_t)t * B + b];
        g += pg_coef[coef_per_frame ? (size_t)t * B + b : (size_t)b] * (sm - (lane == k ? 1.f : 0.f));
    }
    g = ctc_grad_tail<ENT>(g, lpv, sm, lane, V, b, o, ent_scale...);
    if (lane < V) grad[o + lane] = g;
}

// Multi-sample REINFORCE (pgasr_ctc_grad_from_lattice_multi): the CTC part above, then the K terms
// pg_coef[k,b] * (softmax - onehot(pg_paths[k,t,b])) added in k order.  One wave per (t,b), one pass over the gradient;
// K = 1 is ctc_grad_kernel's per-utterance expression.
// STEPS (pgasr_ctc_grad_from_lattice_multi_steps, A12-STEP): pg_coef is (K,T,B), one coefficient per sample and FRAME, read at
// k*T*B + t*B + b; everything else is the same line.  A compile-time switch, so the STEPS = false instantiations keep the instruction
// text they had before it existed (their symbols gained the parameter; per-kernel disassembly compared, NOTES.md 0.37).  One
// __device__ body called by two kernels did not keep it: the registers came out differently.
template <bool ENT, bool STEPS, class... Ent>
__global__ __launch_bounds__(256) void ctc_grad_multi_kernel(
    const float* __restrict__ lp, const int32_t* __restrict__ in_len, const int32_t* __restrict__ tg_len,
    int T, int B, int V, int Lmax, int Smax, int blank, CtcWs ws,
    const float* __restrict__ utt_scale, int K, const float* __restrict__ pg_coef,
    const int32_t* __restrict__ pg_paths, float* __restrict__ grad, Ent... ent_scale) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= (long long)T * B) return;
    const int t = (int)(w / B), b = (int)(w % B);
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    int Lb = tg_len[b]; Lb = Lb < 0 ? 0 : (Lb > Lmax ? Lmax : Lb);
    const size_t o = ((size_t)t * B + b) * V;
    if (t >= Tb) { if (lane < V) grad[o + lane] = 0.f; return; }

    const float lpv = (lane < V) ? lp[o + lane] : 0.f;
    const float sm = (lane < V) ? __expf(lpv) : 0.f;
    float g = ctc_grad_row(lpv, sm, lane, t, b, T, V, Lb, Smax, blank, ws, utt_scale);
    const size_t TB = (size_t)T * B;
    for (int k = 0; k < K; ++k) {
        const int pk = pg_paths[k * TB + (size_t)t * B + b];
        g += pg_coef[STEPS ? k * TB + (size_t)t * B + b : (size_t)k * B + b] * (sm - (lane == pk ? 1.f : 0.f));
    }
    g = ctc_grad_tail<ENT>(g, lpv, sm, lane, V, b, o, ent_scale...);
    if (lane < V) grad[o + lane] = g;
}


// ---- sequence-level REINFORCE (pgasr_ctc_hyp_lattice, pgasr_ctc_grad_from_lattices_seq, pgasr_pg_loss_value_seq) ----
// The score function of sample k is the CTC likelihood of its HYPOTHESIS y_k = collapse(pi_k), not of the sampled frame path:
//   loss      = sum_b [ nll_b utt_scale_b + sum_k pg_coef[k,b] * ( seq(k,b) ? nll(y_k,b | x_b) : -sum_{t<T_b} log p(pi_k[t,b]) ) ]
//   d(logits) = utt_scale_b (softmax - occ_target)
//               + sum_k pg_coef[k,b] * ( seq(k,b) ? (softmax - occ_{y_k}) : (softmax - onehot(pi_k[t,b])) )         in k order
// with seq(k,b) := |y_k,b| <= Lh (a longer hypothesis keeps the path-level term: the choice depends on y alone, so the mixture is
// unbiased).  occ_y = posterior occupancy of y's lattice over the utterance's own T_b frames; a hypothesis whose nll is +inf
// contributes nothing, as for targets.  The K*B hypothesis lattices live in a workspace of their own, a CtcWs for the "batch" of
// pairs p = k*B + b with Smax = 2*Lh+1; every pair reads log-prob row b of the ONE (T,B,V) tensor.
//
// ctc_hyp_lattice_kernel runs ctc_lattice_body on them: it owns one LDS block for whichever states-per-thread variant the
// pair's REAL length selects and addresses the pair's rows.
//
// grid (K*B, 3): pair p = k*B + b; y = 0 alpha, y = 1 beta, y = 2 the label -> states lists.  NMAX = the states-per-thread variant
// that holds 2*Lh+1 states; a pair whose own 2*len+1 fits a smaller variant runs that one (a uniform branch per workgroup, read
// from hyp_len on the device: no host synchronisation), so hypotheses near the target length do not pay for the cap.
template <int NMAX>
__global__ __launch_bounds__(CTC_THREADS + 64) void ctc_hyp_lattice_kernel(
    const float* __restrict__ lp, const int32_t* __restrict__ hyp, int hyp_stride, const int32_t* __restrict__ hyp_len,
    const int32_t* __restrict__ in_len, int T, int B, int V, int Lh, int Smax, int blank, CtcWs ws, float* __restrict__ hyp_nll) {
    __shared__ double rows[2 * (NMAX * CTC_THREADS + 4)];
    const int p = blockIdx.x, b = p % B, role = blockIdx.y;
    const int len = hyp_len[p];
    if (len > Lh) {            // path-scored sample: no lattice; its nll reads 0
        if (role == 0 && threadIdx.x == 0) { ws.nll64[p] = 0.0; hyp_nll[p] = 0.f; }
        return;
    }
    if (role == 2) { ctc_labels_body(hyp, hyp_len, V, hyp_stride, Smax, blank, ws); return; }
    const int Lb = len < 0 ? 0 : len;
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    const int S = 2 * Lb + 1;
    const float* lpb = lp + (size_t)b * V;
    const size_t fstride = (size_t)B * V;
    const int32_t* tgt = hyp + (size_t)p * hyp_stride;
    float* out = (role == 0 ? ws.alpha : ws.beta) + (size_t)p * T * ws.SP;
    double* outmax = (role == 0 ? ws.amax : ws.bmax) + (size_t)p * T;
#define PGASR_HYP_BODY(N) do { \
        if (role == 0) ctc_lattice_body<N, 0>(lpb, fstride, tgt, Tb, Lb, V, blank, out, ws.SP, outmax, ws.nll64 + p, hyp_nll + p, rows); \
        else           ctc_lattice_body<N, 1>(lpb, fstride, tgt, Tb, Lb, V, blank, out, ws.SP, outmax, ws.nll64 + p, hyp_nll + p, rows); \
    } while (0)
    if constexpr (NMAX == 1) {
        PGASR_HYP_BODY(1);
    } else if constexpr (NMAX == 2) {
        if (S <= CTC_THREADS) PGASR_HYP_BODY(1); else PGASR_HYP_BODY(2);
    } else if constexpr (NMAX == 4) {
        if (S <= CTC_THREADS) PGASR_HYP_BODY(1); else if (S <= 2 * CTC_THREADS) PGASR_HYP_BODY(2); else PGASR_HYP_BODY(4);
    } else {
        if (S <= CTC_THREADS) PGASR_HYP_BODY(1); else if (S <= 2 * CTC_THREADS) PGASR_HYP_BODY(2);
        else if (S <= 4 * CTC_THREADS) PGASR_HYP_BODY(4); else PGASR_HYP_BODY(8);
    }
#undef PGASR_HYP_BODY
}

// One wave per (t,b), one pass, one write: the target part, then sample k = 0..K-1 in k order -- the sequence term from lattice
// (k,b) where hyp_len[k,b] <= Lh (ctc_grad_row over the hypothesis workspace, scale pg_coef[k,b]), else ctc_grad_multi_kernel's path term.
// PATHS = false (pgasr_ctc_grad_from_lattices_nbest, MWER over N-best lists): there are no sampled paths -- the path branch is compiled
// out, pg_paths is not read, and a pair with hyp_len > Lh adds nothing.  The PATHS = true instantiations are the code they were.
template <bool ENT, bool PATHS, class... Ent>
__global__ __launch_bounds__(256) void ctc_grad_seq_kernel(
    const float* __restrict__ lp, const int32_t* __restrict__ in_len, const int32_t* __restrict__ tg_len,
    int T, int B, int V, int Lmax, int Smax, int blank, CtcWs ws,
    const float* __restrict__ utt_scale, int K, const float* __restrict__ pg_coef,
    const int32_t* __restrict__ pg_paths, const int32_t* __restrict__ hyp_len, int Lh, int Smax_h, CtcWs hws,
    float* __restrict__ grad, Ent... ent_scale) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= (long long)T * B) return;
    const int t = (int)(w / B), b = (int)(w % B);
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    int Lb = tg_len[b]; Lb = Lb < 0 ? 0 : (Lb > Lmax ? Lmax : Lb);
    const size_t o = ((size_t)t * B + b) * V;
    if (t >= Tb) { if (lane < V) grad[o + lane] = 0.f; return; }

    const float lpv = (lane < V) ? lp[o + lane] : 0.f;
    const float sm = (lane < V) ? __expf(lpv) : 0.f;
    float g = ctc_grad_row(lpv, sm, lane, t, b, T, V, Lb, Smax, blank, ws, utt_scale);
    const size_t TB = (size_t)T * B;
    for (int k = 0; k < K; ++k) {
        const int p = k * B + b;
        const int len = hyp_len[p];
        if (len <= Lh) {
            // pair p's lattice; the per-pair scale is pg_coef[p]
            g += ctc_grad_row(lpv, sm, lane, t, p, T, V, len < 0 ? 0 : len, Smax_h, blank, hws, pg_coef);
        } else if constexpr (PATHS) {
            const int pk = pg_paths[k * TB + (size_t)t * B + b];
            g += pg_coef[p] * (sm - (lane == pk ? 1.f : 0.f));
        }
    }
    g = ctc_grad_tail<ENT>(g, lpv, sm, lane, V, b, o, ent_scale...);
    if (lane < V) grad[o + lane] = g;
}

// terms[b] = nll_b utt_scale_b + sum_k coef[k,b] * ( hyp_len[k,b] <= Lh ? hyp_nll[k,b] : -sum_{t<T_b} log p(paths[k,t,b]) ): the path
// sums in block_path_logprob_sum's fixed order, the K products added in k order; a +inf hypothesis nll adds nothing.
__global__ __launch_bounds__(256) void pg_loss_value_seq_kernel(const float* __restrict__ lp, const int32_t* __restrict__ paths, int K,
                                                                const int32_t* __restrict__ in_len, const float* __restrict__ nll,
                                                                const float* __restrict__ utt_scale, const float* __restrict__ coef,
                                                                const float* __restrict__ hyp_nll, const int32_t* __restrict__ hyp_len,
                                                                int Lh, int T, int B, int V, float* __restrict__ terms) {
    __shared__ float red[256];
    const int b = blockIdx.x;
    const int Tb = min(in_len[b], T);
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
        const size_t p = (size_t)k * B + b;
        if (hyp_len[p] <= Lh) {               // uniform over the workgroup
            const float hn = hyp_nll[p];
            if (hn != INFINITY) acc -= coef[p] * hn;
            continue;
        }
        acc += coef[p] * block_path_logprob_sum(lp, paths + (size_t)k * T * B, nullptr, Tb, b, B, V, red);
    }
    if (threadIdx.x == 0) terms[b] = nll[b] * utt_scale[b] - acc;
}

// ---- what the entry points below share: argument checks, workspace binding, the description of a gradient call ----
// vmax: CTC_VMAX for the one-label-per-lane kernels, PGASR_WIDE_VMAX for the wide ones
static int ctc_args_ok(int T, int B, int V, int Lmax, int blank, int vmax) {
    if (T <= 0 || B <= 0 || V <= 0 || Lmax < 0 || blank < 0 || blank >= V) return PGASR_ERR_INVALID_ARG;
    if (2 * (long long)Lmax + 1 > CTC_SMAX || V > vmax) return PGASR_ERR_UNSUPPORTED;
    return PGASR_OK;
}

static int ctc_hyp_args_ok(int T, int B, int V, int K, int Lh, int vmax) {
    if (T <= 0 || B <= 0 || V <= 0 || Lh < 0) return PGASR_ERR_INVALID_ARG;
    if (K < 1 || K > PGASR_MAX_SAMPLES) return PGASR_ERR_INVALID_ARG;
    if (2 * (long long)Lh + 1 > CTC_SMAX || V > vmax) return PGASR_ERR_UNSUPPORTED;
    if ((long long)K * B > 0x7fffffffLL / 4) return PGASR_ERR_UNSUPPORTED;
    return PGASR_OK;
}

// lays *ws out over the caller's workspace of N lattices; false when that is missing or too small
static bool ctc_ws_bind(int T, int N, int V, int Smax, CtcWs* ws, void* workspace, size_t workspace_bytes) {
    const size_t need = ctc_ws_layout(T, N, V, Smax, ws, (char*)workspace);
    return workspace && workspace_bytes >= need;
}

// Everything a gradient pass can take, group by group: an entry point fills the groups its signature has and leaves the rest zero.
struct GradHead { const float* log_probs; const int32_t *input_lengths, *target_lengths; int T, B, V, Lmax, blank; const float* utt_scale; };
struct GradPg   { int K; const float* pg_coef; const int32_t* pg_paths; int coef_per_frame; };   // one path: K = 1, the flag 0 or 1
struct GradHyp  { const int32_t* hyp_len; int Lh; void* hyp_workspace; size_t hyp_workspace_bytes; };
struct GradTail { const float *ent_scale, *ref_log_probs, *kl_scale; };     // the tail rule of include/pgasr_hip.h
struct GradCall : GradHead, GradPg, GradHyp, GradTail { float* grad_logits; void* workspace; size_t workspace_bytes; void* stream; };

// What follows the target part: one sampled path (optional; its coefficient per utterance or per frame), K paths, K paths with
// per-frame coefficients (K,T,B), K hypothesis lattices with the path fallback, N hypothesis lattices alone.
enum GradForm { GRAD_ONE, GRAD_MULTI, GRAD_STEPS, GRAD_SEQ, GRAD_NBEST };

// TAIL as the kernels number it: 0 = none, 1 = entropy, 2 = entropy (nullable) and KL.  f(integral_constant<int, TAIL>) for the call's.
template <int N> using Int = std::integral_constant<int, N>;
template <class F>
static int ctc_with_tail(const GradTail& t, F f) { return t.kl_scale ? f(Int<2>{}) : t.ent_scale ? f(Int<1>{}) : f(Int<0>{}); }

// A gradient pass of the one-label-per-lane kernels: one wave per (t,b) row, four rows per workgroup.  Every gradient kernel starts
// with the same arguments up to utt_scale; `rest` is what follows them.
template <class Kernel, class... Rest>
static int ctc_launch_grad(Kernel kernel, const GradCall& c, const CtcWs& ws, Rest... rest) {
    const long long waves = (long long)c.T * c.B;
    const int wpb = 4;
    const unsigned blocks = (unsigned)((waves + wpb - 1) / wpb);
    PGASR_LAUNCH_KERNEL(kernel, dim3(blocks), dim3(64 * wpb), 0, (hipStream_t)c.stream, c.log_probs, c.input_lengths, c.target_lengths,
                       c.T, c.B, c.V, c.Lmax > 0 ? c.Lmax : 1, 2 * c.Lmax + 1, c.blank, ws, c.utt_scale, rest...);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

// ... with the tail the kernels take as a pack of pointers: none, (ent_scale), or (ent_scale, ref_log_probs, kl_scale).  The one
// place that names the narrow instantiations; the N-best form exists without a tail only.
template <int TAIL, class... Ent>
static int ctc_grad_narrow(const GradCall& c, GradForm form, const CtcWs& ws, const CtcWs& hws, Ent... ent) {
    static_assert(sizeof...(Ent) == (TAIL == 2 ? 3 : TAIL), "the pack is the tail");
    constexpr bool ENT = TAIL != 0;
    const int Smax_h = 2 * c.Lh + 1;
    switch (form) {
    case GRAD_ONE:
        return ctc_launch_grad(ctc_grad_kernel<ENT, Ent...>, c, ws, c.pg_coef, c.pg_paths, c.coef_per_frame, c.grad_logits, ent...);
    case GRAD_MULTI:
        return ctc_launch_grad(ctc_grad_multi_kernel<ENT, false, Ent...>, c, ws, c.K, c.pg_coef, c.pg_paths, c.grad_logits, ent...);
    case GRAD_STEPS:
        return ctc_launch_grad(ctc_grad_multi_kernel<ENT, true, Ent...>, c, ws, c.K, c.pg_coef, c.pg_paths, c.grad_logits, ent...);
    case GRAD_SEQ:
        return ctc_launch_grad(ctc_grad_seq_kernel<ENT, true, Ent...>, c, ws, c.K, c.pg_coef, c.pg_paths, c.hyp_len, c.Lh, Smax_h, hws,
                               c.grad_logits, ent...);
    case GRAD_NBEST:
        if constexpr (TAIL == 0)
            return ctc_launch_grad(ctc_grad_seq_kernel<false, false>, c, ws, c.K, c.pg_coef, c.pg_paths, c.hyp_len, c.Lh, Smax_h, hws,
                                   c.grad_logits);
    }
    return PGASR_ERR_INVALID_ARG;
}

// ---- alphabets of up to 1024 symbols (pgasr_ctc_loss_grad_wide, pgasr_ctc_grad_from_lattice_wide; header section A5-WIDE) ----
// The lattice is V-agnostic (V only addresses a row): the wide entries launch ctc_lattice_kernel with grid (B,2) -- roles 0 and 1 --
// and build the label -> states lists with the kernel below, in the workspace format of ctc_labels_body, for any V <= 1024.
// One workgroup per utterance.  Counting the labels is integer work (LDS atomics: the counts do not depend on the order); the
// offsets are a block scan over V + 1 counts; entry i of the target goes to slot lab_off[label] + #{j < i : target[j] == label},
// so every list is in ascending s whatever order the threads run in.
__global__ __launch_bounds__(256) void ctc_labels_wide_kernel(const int32_t* __restrict__ targets, const int32_t* __restrict__ tg_len,
                                                              int V, int Lmax, int Smax, int blank, CtcWs ws) {
    constexpr int CH = (PGASR_WIDE_VMAX + 1 + 255) / 256;      // counts per thread in the scan (5)
    __shared__ int tg[CTC_SMAX / 2];                           // the target row, L <= 1023
    __shared__ int cnt[256 * CH];                              // counts, then offsets
    __shared__ int wtot[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int Lb = tg_len[b]; Lb = Lb < 0 ? 0 : (Lb > Lmax ? Lmax : Lb);
    if (Lb > CTC_SMAX / 2) Lb = CTC_SMAX / 2;                  // defensive: the entry points refuse 2 * Lmax + 1 > 2048
    const int32_t* tgt = targets + (size_t)b * Lmax;
    for (int i = tid; i < 256 * CH; i += 256) cnt[i] = 0;
    for (int i = tid; i < Lb; i += 256) tg[i] = tgt[i];
    __syncthreads();
    for (int i = tid; i < Lb; i += 256) {
        const int l = tg[i];
        if (l != blank && (unsigned)l < (unsigned)V) atomicAdd(&cnt[l], 1);
    }
    __syncthreads();
    // exclusive scan of cnt[0 .. V]: thread i owns entries i*CH .. i*CH + CH - 1
    int loc[CH], sum = 0;
#pragma unroll
    for (int j = 0; j < CH; ++j) { loc[j] = cnt[tid * CH + j]; sum += loc[j]; }
    int inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wtot[wid] = inc;
    __syncthreads();
    int run = inc - sum;
    for (int w = 0; w < wid; ++w) run += wtot[w];
#pragma unroll
    for (int j = 0; j < CH; ++j) { cnt[tid * CH + j] = run; run += loc[j]; }
    __syncthreads();
    for (int v = tid; v <= V; v += 256) ws.lab_off[(size_t)b * (V + 1) + v] = cnt[v];
    for (int i = tid; i < Lb; i += 256) {
        const int l = tg[i];
        if (l == blank || (unsigned)l >= (unsigned)V) continue;
        int rank = 0;
        for (int j = 0; j < i; ++j) rank += (tg[j] == l);
        ws.lab_states[(size_t)b * Smax + cnt[l] + rank] = 2 * i + 1;
    }
}

// The gradient pass for wide rows: one wave per (t,b), lane l holding labels l*NV .. l*NV + NV - 1 (wide_rows.h).
//   grad = utt_scale_b (softmax - occupancy) [+ pg_coef (softmax - onehot(pg_path))],  zero rows at t >= T_b.
// Occupancy is ctc_grad_row's walk with NV labels per lane: the lane reads lab_off[l*NV .. l*NV + NV] and adds up each of its
// labels' lists in list order -- the order, the constants and the selects of ctc_grad_row, so a row of V <= 64 gets that routine's
// sums -- and the blank's occupancy (even states) is its strided sum with one butterfly.  Fixed order, no atomics: the same bits
// every run.  A symbol with log p = -inf has occupancy 0 and gradient entry 0, never NaN (the selects on the constant).  The
// offsets are V + 1 more words per row, as many bytes as the row at V = 1024, but they are the utterance's 4 KB for all its T
// rows and come from L2, not from HBM; walking the at most L target entries instead would need the targets, which
// pgasr_ctc_grad_from_lattice's signature does not carry (NOTES.md).
constexpr int CTC_WIDE_WPB = 4;      // waves (rows) per workgroup
template <int NV>
__global__ __launch_bounds__(64 * CTC_WIDE_WPB) void ctc_grad_wide_kernel(
    const float* __restrict__ lp, const int32_t* __restrict__ in_len,
    const int32_t* __restrict__ tg_len, int T, int B, int V, int vec, int Lmax, int Smax, int blank, CtcWs ws,
    const float* __restrict__ utt_scale, const float* __restrict__ pg_coef,
    const int32_t* __restrict__ pg_path, int coef_per_frame, float* __restrict__ grad) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * CTC_WIDE_WPB + (threadIdx.x >> 6);
    if (w >= (long long)T * B) return;
    const int t = (int)(w / B), b = (int)(w % B);
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    int Lb = tg_len[b]; Lb = Lb < 0 ? 0 : (Lb > Lmax ? Lmax : Lb);
    const size_t o = ((size_t)t * B + b) * V;
    const int v0 = lane * NV;
    float g[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) g[i] = 0.f;
    if (t >= Tb) {
        wide_row_store<NV>(grad + o, V, lane, vec != 0, g);
        return;
    }
    float lpv[NV], sm[NV];
    wide_row_load<NV>(lp + o, V, lane, vec != 0, 0.f, lpv);
#pragma unroll
    for (int i = 0; i < NV; ++i) sm[i] = (v0 + i < V) ? __expf(lpv[i]) : 0.f;

    const double nll = ws.nll64[b];
    if (nll != INFINITY) {            // uniform over the wave
        const int S = 2 * Lb + 1;
        const float* al = ws.alpha + ((size_t)b * T + t) * ws.SP;
        const float* be = ws.beta + ((size_t)b * T + t) * ws.SP;
        const double cst = ws.amax[(size_t)b * T + t] + ws.bmax[(size_t)b * T + t] + nll;
        const float lpb = lp[o + blank];
        const float cb = (lpb == -INFINITY) ? 0.f : (float)(cst - (double)lpb);
        float accb = 0.f;
        for (int s = 2 * lane; s < S; s += 128)
            accb += __expf((al[s] + be[s]) + cb);
        accb = wave_sum(accb);
        const int32_t* lo = ws.lab_off + (size_t)b * (V + 1);
        const int32_t* ls = ws.lab_states + (size_t)b * Smax;
        const float sc = utt_scale ? utt_scale[b] : 1.f;
        int off[NV + 1];
#pragma unroll
        for (int i = 0; i <= NV; ++i) off[i] = (v0 + i <= V) ? lo[v0 + i] : 0;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = v0 + i;
            if (v < V) {
                float occ = accb;
                if (v != blank) {
                    float acc = 0.f;
                    const float cl = (lpv[i] == -INFINITY) ? 0.f : (float)(cst - (double)lpv[i]);
                    for (int j = off[i]; j < off[i + 1]; ++j) {
                        const int s = ls[j];
                        acc += __expf((al[s] + be[s]) + cl);
                    }
                    occ = acc;
                }
                g[i] = sc * (sm[i] - occ);
            }
        }
    }
    if (pg_coef != nullptr && pg_path != nullptr) {
        const int k = pg_path[(size_t)t * B + b];
        const float c = pg_coef[coef_per_frame ? (size_t)t * B + b : (size_t)b];
#pragma unroll
        for (int i = 0; i < NV; ++i) g[i] += c * (sm[i] - (v0 + i == k ? 1.f : 0.f));
    }
    wide_row_store<NV>(grad + o, V, lane, vec != 0, g);
}

// ---- the multi-sample gradient pass for wide rows, with the entropy and KL tails (pgasr_ctc_grad_from_lattice_multi_wide; A12-WIDE) ----
// ctc_grad_multi_kernel with NV labels per lane: the CTC part of ctc_grad_wide_kernel, then the K terms
// pg_coef[k,b] (softmax - onehot(pg_paths[k,t,b])) in k order, then ent_scale_b p (ln p + H), then kl_scale_b p (ln p - lnq - KL)
// under ctc_entropy_kl_grad's rule that a zero term leaves g untouched.  H and KL add the lane's NV terms in label order before the
// one wave_sum.  TAIL: 0 = none, 1 = entropy, 2 = entropy (nullable) and KL; the plain pass holds no code of the tails.  With NV = 1
// every sum is ctc_grad_multi_kernel's, in its order.
// The label offsets are read outer-first: lane l reads lab_off[v0] and lab_off[min(v0 + NV, V)], the bounds of the concatenated lists
// of ALL its labels, and reads the NV - 1 offsets between them only when the two differ.  A lane none of whose labels occurs in the
// target -- with L labels over V / NV groups, most lanes at V >= 256 -- does two loads where ctc_grad_wide_kernel does NV + 1, and
// every label's (empty) sum is the 0 the walk would have given: the summation order is unchanged.
// STEPS: pg_coef (K,T,B) as in ctc_grad_multi_kernel, the same compile-time switch.
template <int NV, int TAIL, bool STEPS>
__global__ __launch_bounds__(64 * CTC_WIDE_WPB) void ctc_grad_multi_wide_kernel(
    const float* __restrict__ lp, const int32_t* __restrict__ in_len,
    const int32_t* __restrict__ tg_len, int T, int B, int V, int vec, int Lmax, int Smax, int blank, CtcWs ws,
    const float* __restrict__ utt_scale, int K, const float* __restrict__ pg_coef, const int32_t* __restrict__ pg_paths,
    const float* __restrict__ ent_scale, const float* __restrict__ ref_lp, const float* __restrict__ kl_scale,
    float* __restrict__ grad) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * CTC_WIDE_WPB + (threadIdx.x >> 6);
    if (w >= (long long)T * B) return;
    const int t = (int)(w / B), b = (int)(w % B);
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    int Lb = tg_len[b]; Lb = Lb < 0 ? 0 : (Lb > Lmax ? Lmax : Lb);
    const size_t o = ((size_t)t * B + b) * V;
    const int v0 = lane * NV;
    float g[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) g[i] = 0.f;
    if (t >= Tb) {
        wide_row_store<NV>(grad + o, V, lane, vec != 0, g);
        return;
    }
    float lpv[NV], sm[NV];
    wide_row_load<NV>(lp + o, V, lane, vec != 0, 0.f, lpv);
#pragma unroll
    for (int i = 0; i < NV; ++i) sm[i] = (v0 + i < V) ? __expf(lpv[i]) : 0.f;

    const double nll = ws.nll64[b];
    if (nll != INFINITY) {            // uniform over the wave
        const int S = 2 * Lb + 1;
        const float* al = ws.alpha + ((size_t)b * T + t) * ws.SP;
        const float* be = ws.beta + ((size_t)b * T + t) * ws.SP;
        const double cst = ws.amax[(size_t)b * T + t] + ws.bmax[(size_t)b * T + t] + nll;
        const float lpb = lp[o + blank];
        const float cb = (lpb == -INFINITY) ? 0.f : (float)(cst - (double)lpb);
        float accb = 0.f;
        for (int s = 2 * lane; s < S; s += 128)
            accb += __expf((al[s] + be[s]) + cb);
        accb = wave_sum(accb);
        const int32_t* lo = ws.lab_off + (size_t)b * (V + 1);
        const int32_t* ls = ws.lab_states + (size_t)b * Smax;
        const float sc = utt_scale ? utt_scale[b] : 1.f;
        const int vend = (v0 + NV < V) ? v0 + NV : V;
        const int lo0 = (v0 < V) ? lo[v0] : 0;
        const int lo1 = (v0 < V) ? lo[vend] : 0;
        int off[NV + 1];
#pragma unroll
        for (int i = 0; i <= NV; ++i) off[i] = lo0;                       // no label of this lane in the target: every list is empty
        if (lo0 != lo1) {
#pragma unroll
            for (int i = 1; i < NV; ++i) off[i] = (v0 + i <= V) ? lo[v0 + i] : 0;
            off[NV] = lo1;            // read by label v0 + NV - 1 alone, which exists only when vend = v0 + NV
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = v0 + i;
            if (v < V) {
                float occ = accb;
                if (v != blank) {
                    float acc = 0.f;
                    const float cl = (lpv[i] == -INFINITY) ? 0.f : (float)(cst - (double)lpv[i]);
                    for (int j = off[i]; j < off[i + 1]; ++j) {
                        const int s = ls[j];
                        acc += __expf((al[s] + be[s]) + cl);
                    }
                    occ = acc;
                }
                g[i] = sc * (sm[i] - occ);
            }
        }
    }
    const size_t TB = (size_t)T * B;
    for (int k = 0; k < K; ++k) {
        const int pk = pg_paths[k * TB + (size_t)t * B + b];
        const float c = pg_coef[STEPS ? k * TB + (size_t)t * B + b : (size_t)k * B + b];
#pragma unroll
        for (int i = 0; i < NV; ++i) g[i] += c * (sm[i] - (v0 + i == pk ? 1.f : 0.f));
    }
    if constexpr (TAIL >= 1) {
        if (TAIL == 1 || ent_scale != nullptr) {
            float plp[NV], s = 0.f;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                plp[i] = sm[i] > 0.f ? sm[i] * lpv[i] : 0.f;
                s = (i == 0) ? plp[i] : s + plp[i];
            }
            const float H = -wave_sum(s);
            const float es = ent_scale[b];
#pragma unroll
            for (int i = 0; i < NV; ++i) g[i] += sm[i] > 0.f ? es * fmaf(sm[i], H, plp[i]) : 0.f;
        }
    }
    if constexpr (TAIL == 2) {
        float d[NV];
        wide_row_load<NV>(ref_lp + o, V, lane, vec != 0, 0.f, d);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            d[i] = sm[i] > 0.f ? sm[i] * (lpv[i] - fmaxf(d[i], KL_LOG_FLOOR)) : 0.f;
            s = (i == 0) ? d[i] : s + d[i];
        }
        const float kl = wave_sum(s);
        const float ks = kl_scale[b];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const float term = ks * fmaf(-sm[i], kl, d[i]);
            g[i] = term != 0.f ? g[i] + term : g[i];
        }
    }
    wide_row_store<NV>(grad + o, V, lane, vec != 0, g);
}

// ---- sequence-level REINFORCE and N-best MWER for wide rows (pgasr_ctc_hyp_lattice_wide, pgasr_ctc_grad_from_lattices_seq_wide; A13-WIDE) ----
// The hypothesis lattices are V-agnostic like the target's: the wide entry launches ctc_hyp_lattice_kernel with grid (K*B, 2) -- the
// sweeps alone -- and builds the label -> states lists of pair p = k*B + b with the kernel below: ctc_labels_wide_kernel's counts
// (LDS atomics), block scan over V + 1 counts and slot = offset + rank among earlier equal tokens, over row p of hyp_tokens at
// hyp_stride with the length hyp_len[p].  A pair with hyp_len > Lh has no lattice and no lists, as in the lattice roles.  A kernel
// of its own beside ctc_labels_wide_kernel, whose text stays what it was.
__global__ __launch_bounds__(256) void ctc_hyp_labels_wide_kernel(const int32_t* __restrict__ hyp, int hyp_stride,
                                                                  const int32_t* __restrict__ hyp_len, int V, int Lh, int Smax, int blank,
                                                                  CtcWs ws) {
    constexpr int CH = (PGASR_WIDE_VMAX + 1 + 255) / 256;      // counts per thread in the scan (5)
    __shared__ int tg[CTC_SMAX / 2];                           // the hypothesis row, L <= 1023
    __shared__ int cnt[256 * CH];                              // counts, then offsets
    __shared__ int wtot[4];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int len = hyp_len[p];
    if (len > Lh) return;                                      // path-scored sample: uniform over the workgroup
    int Lb = len < 0 ? 0 : len;
    if (Lb > hyp_stride) Lb = hyp_stride;                      // ctc_labels_body's clamp to the row
    if (Lb > CTC_SMAX / 2) Lb = CTC_SMAX / 2;                  // defensive: the entry points refuse 2 * Lh + 1 > 2048
    const int32_t* tgt = hyp + (size_t)p * hyp_stride;
    for (int i = tid; i < 256 * CH; i += 256) cnt[i] = 0;
    for (int i = tid; i < Lb; i += 256) tg[i] = tgt[i];
    __syncthreads();
    for (int i = tid; i < Lb; i += 256) {
        const int l = tg[i];
        if (l != blank && (unsigned)l < (unsigned)V) atomicAdd(&cnt[l], 1);
    }
    __syncthreads();
    // exclusive scan of cnt[0 .. V]: thread i owns entries i*CH .. i*CH + CH - 1
    int loc[CH], sum = 0;
#pragma unroll
    for (int j = 0; j < CH; ++j) { loc[j] = cnt[tid * CH + j]; sum += loc[j]; }
    int inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wtot[wid] = inc;
    __syncthreads();
    int run = inc - sum;
    for (int w = 0; w < wid; ++w) run += wtot[w];
#pragma unroll
    for (int j = 0; j < CH; ++j) { cnt[tid * CH + j] = run; run += loc[j]; }
    __syncthreads();
    for (int v = tid; v <= V; v += 256) ws.lab_off[(size_t)p * (V + 1) + v] = cnt[v];
    for (int i = tid; i < Lb; i += 256) {
        const int l = tg[i];
        if (l == blank || (unsigned)l >= (unsigned)V) continue;
        int rank = 0;
        for (int j = 0; j < i; ++j) rank += (tg[j] == l);
        ws.lab_states[(size_t)p * Smax + cnt[l] + rank] = 2 * i + 1;      // cnt[l] + rank < Lb <= Lh < Smax
    }
}

// scale_n (softmax - occupancy) of lattice n of ws for one (t,b) row of NV labels per lane: ctc_grad_row with wide rows.  r[i] is
// label v0 + i's value, 0 for every label when the lattice's nll is +inf (no alignment) and for labels past V.  The walk of
// ctc_grad_multi_wide_kernel: the blank's strided sum and one butterfly, every label's list in list order, the selects that give a
// log p = -inf occupancy 0, the label offsets read outer-first.  lpb = the row's log p(blank); scale NULL reads as 1.
template <int NV>
__device__ __forceinline__ void ctc_grad_row_wide(const float (&lpv)[NV], const float (&sm)[NV], float lpb, int lane, int t, int n, int T,
                                                  int V, int Lb, int Smax, int blank, const CtcWs& ws, const float* __restrict__ scale,
                                                  float (&r)[NV]) {
    const int v0 = lane * NV;
#pragma unroll
    for (int i = 0; i < NV; ++i) r[i] = 0.f;
    const double nll = ws.nll64[n];
    if (nll != INFINITY) {            // uniform over the wave
        const int S = 2 * Lb + 1;
        const float* al = ws.alpha + ((size_t)n * T + t) * ws.SP;
        const float* be = ws.beta + ((size_t)n * T + t) * ws.SP;
        const double cst = ws.amax[(size_t)n * T + t] + ws.bmax[(size_t)n * T + t] + nll;
        const float cb = (lpb == -INFINITY) ? 0.f : (float)(cst - (double)lpb);
        float accb = 0.f;
        for (int s = 2 * lane; s < S; s += 128)
            accb += __expf((al[s] + be[s]) + cb);
        accb = wave_sum(accb);
        const int32_t* lo = ws.lab_off + (size_t)n * (V + 1);
        const int32_t* ls = ws.lab_states + (size_t)n * Smax;
        const float sc = scale ? scale[n] : 1.f;
        const int vend = (v0 + NV < V) ? v0 + NV : V;
        const int lo0 = (v0 < V) ? lo[v0] : 0;
        const int lo1 = (v0 < V) ? lo[vend] : 0;
        int off[NV + 1];
#pragma unroll
        for (int i = 0; i <= NV; ++i) off[i] = lo0;                       // no label of this lane in the sequence: every list is empty
        if (lo0 != lo1) {
#pragma unroll
            for (int i = 1; i < NV; ++i) off[i] = (v0 + i <= V) ? lo[v0 + i] : 0;
            off[NV] = lo1;            // read by label v0 + NV - 1 alone, which exists only when vend = v0 + NV
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = v0 + i;
            if (v < V) {
                float occ = accb;
                if (v != blank) {
                    float acc = 0.f;
                    const float cl = (lpv[i] == -INFINITY) ? 0.f : (float)(cst - (double)lpv[i]);
                    for (int j = off[i]; j < off[i + 1]; ++j) {
                        const int s = ls[j];
                        acc += __expf((al[s] + be[s]) + cl);
                    }
                    occ = acc;
                }
                r[i] = sc * (sm[i] - occ);
            }
        }
    }
}

// ctc_grad_seq_kernel with NV labels per lane: the target part, then pair (k,b) for k = 0 .. K-1 in k order -- the sequence term from
// lattice (k,b) of the hypothesis workspace where hyp_len[k,b] <= Lh (scale pg_coef[k,b]), else, when PATHS, the path term
// pg_coef[k,b] (softmax - onehot(pg_paths[k,t,b])) --, then the tails of ctc_grad_multi_wide_kernel (TAIL: 0 none, 1 entropy,
// 2 entropy (nullable) and KL).  PATHS = false (the N-best form, MWER): pg_paths is not read and a pair over the cap adds nothing.
// One wave per (t,b), one pass, one write; rows t >= T_b are written as zeros.  With NV = 1 every sum is ctc_grad_seq_kernel's, in
// its order.
template <int NV, bool PATHS, int TAIL>
__global__ __launch_bounds__(64 * CTC_WIDE_WPB) void ctc_grad_seq_wide_kernel(
    const float* __restrict__ lp, const int32_t* __restrict__ in_len,
    const int32_t* __restrict__ tg_len, int T, int B, int V, int vec, int Lmax, int Smax, int blank, CtcWs ws,
    const float* __restrict__ utt_scale, int K, const float* __restrict__ pg_coef, const int32_t* __restrict__ pg_paths,
    const int32_t* __restrict__ hyp_len, int Lh, int Smax_h, CtcWs hws,
    const float* __restrict__ ent_scale, const float* __restrict__ ref_lp, const float* __restrict__ kl_scale,
    float* __restrict__ grad) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * CTC_WIDE_WPB + (threadIdx.x >> 6);
    if (w >= (long long)T * B) return;
    const int t = (int)(w / B), b = (int)(w % B);
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    int Lb = tg_len[b]; Lb = Lb < 0 ? 0 : (Lb > Lmax ? Lmax : Lb);
    const size_t o = ((size_t)t * B + b) * V;
    const int v0 = lane * NV;
    float g[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) g[i] = 0.f;
    if (t >= Tb) {
        wide_row_store<NV>(grad + o, V, lane, vec != 0, g);
        return;
    }
    float lpv[NV], sm[NV];
    wide_row_load<NV>(lp + o, V, lane, vec != 0, 0.f, lpv);
#pragma unroll
    for (int i = 0; i < NV; ++i) sm[i] = (v0 + i < V) ? __expf(lpv[i]) : 0.f;
    const float lpb = lp[o + blank];

    // (One copy of the walk for all K + 1 lattices, the workspace chosen per trip, was tried: the choice between the two CtcWs put
    // them into 136 bytes of scratch and saved no register.  Two copies, none in scratch.)
    ctc_grad_row_wide<NV>(lpv, sm, lpb, lane, t, b, T, V, Lb, Smax, blank, ws, utt_scale, g);
    const size_t TB = (size_t)T * B;
    for (int k = 0; k < K; ++k) {
        const int p = k * B + b;
        const int len = hyp_len[p];
        if (len <= Lh) {              // uniform over the wave
            float r[NV];
            ctc_grad_row_wide<NV>(lpv, sm, lpb, lane, t, p, T, V, len < 0 ? 0 : len, Smax_h, blank, hws, pg_coef, r);
#pragma unroll
            for (int i = 0; i < NV; ++i) g[i] += r[i];
        } else if constexpr (PATHS) {
            const int pk = pg_paths[k * TB + (size_t)t * B + b];
            const float c = pg_coef[p];
#pragma unroll
            for (int i = 0; i < NV; ++i) g[i] += c * (sm[i] - (v0 + i == pk ? 1.f : 0.f));
        }
    }
    if constexpr (TAIL >= 1) {
        if (TAIL == 1 || ent_scale != nullptr) {
            float plp[NV], s = 0.f;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                plp[i] = sm[i] > 0.f ? sm[i] * lpv[i] : 0.f;
                s = (i == 0) ? plp[i] : s + plp[i];
            }
            const float H = -wave_sum(s);
            const float es = ent_scale[b];
#pragma unroll
            for (int i = 0; i < NV; ++i) g[i] += sm[i] > 0.f ? es * fmaf(sm[i], H, plp[i]) : 0.f;
        }
    }
    if constexpr (TAIL == 2) {
        float d[NV];
        wide_row_load<NV>(ref_lp + o, V, lane, vec != 0, 0.f, d);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            d[i] = sm[i] > 0.f ? sm[i] * (lpv[i] - fmaxf(d[i], KL_LOG_FLOOR)) : 0.f;
            s = (i == 0) ? d[i] : s + d[i];
        }
        const float kl = wave_sum(s);
        const float ks = kl_scale[b];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const float term = ks * fmaf(-sm[i], kl, d[i]);
            g[i] = term != 0.f ? g[i] + term : g[i];
        }
    }
    wide_row_store<NV>(grad + o, V, lane, vec != 0, g);
}

// ---- the host side of every gradient pass ----
// A gradient pass of the wide kernels: CTC_WIDE_WPB rows per workgroup, the kernel's NV by V, and ONE `vec` for the launch -- the row
// loads of log_probs and (KL tail only) ref_log_probs and the row store must all be aligned.  pick(Int<NV>) is the kernel; they all
// start with the same arguments up to utt_scale, `rest` is what follows them.
template <int TAIL, class Pick, class... Rest>
static int ctc_launch_grad_wide(const GradCall& c, const CtcWs& ws, Pick pick, Rest... rest) {
    const long long waves = (long long)c.T * c.B;
    const unsigned blocks = (unsigned)((waves + CTC_WIDE_WPB - 1) / CTC_WIDE_WPB);
#define PGASR_CALL(NV) do {                                                                                                            \
        const bool vec = wide_vec_ok<NV>(c.log_probs, c.grad_logits, c.V) &&                                                            \
                         (TAIL < 2 || wide_vec_ok<NV>(c.ref_log_probs, c.ref_log_probs, c.V));                                          \
        auto kernel = pick(Int<NV>{});                                                                                                  \
        PGASR_LAUNCH_KERNEL(kernel, dim3(blocks), dim3(64 * CTC_WIDE_WPB), 0, (hipStream_t)c.stream, c.log_probs, c.input_lengths,      \
                           c.target_lengths, c.T, c.B, c.V, vec ? 1 : 0, c.Lmax > 0 ? c.Lmax : 1, 2 * c.Lmax + 1, c.blank, ws,          \
                           c.utt_scale, rest...);                                                                                       \
    } while (0)
    PGASR_WIDE_DISPATCH(c.V, PGASR_CALL);
#undef PGASR_CALL
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

// The one place that names the wide instantiations.  The single-path pass and the N-best form exist without a tail only; the tail
// pointers a TAIL does not use are NULL in the call (ctc_grad_run), and reach the kernel so.
template <int TAIL>
static int ctc_grad_wide(const GradCall& c, GradForm form, const CtcWs& ws, const CtcWs& hws) {
    const int Smax_h = 2 * c.Lh + 1;
    switch (form) {
    case GRAD_ONE:
        if constexpr (TAIL == 0)
            return ctc_launch_grad_wide<0>(c, ws, [](auto nv) { return ctc_grad_wide_kernel<decltype(nv)::value>; },
                                           c.pg_coef, c.pg_paths, c.coef_per_frame, c.grad_logits);
        break;
    case GRAD_MULTI:
        return ctc_launch_grad_wide<TAIL>(c, ws, [](auto nv) { return ctc_grad_multi_wide_kernel<decltype(nv)::value, TAIL, false>; },
                                          c.K, c.pg_coef, c.pg_paths, c.ent_scale, c.ref_log_probs, c.kl_scale, c.grad_logits);
    case GRAD_STEPS:
        return ctc_launch_grad_wide<TAIL>(c, ws, [](auto nv) { return ctc_grad_multi_wide_kernel<decltype(nv)::value, TAIL, true>; },
                                          c.K, c.pg_coef, c.pg_paths, c.ent_scale, c.ref_log_probs, c.kl_scale, c.grad_logits);
    case GRAD_SEQ:
        return ctc_launch_grad_wide<TAIL>(c, ws, [](auto nv) { return ctc_grad_seq_wide_kernel<decltype(nv)::value, true, TAIL>; },
                                          c.K, c.pg_coef, c.pg_paths, c.hyp_len, c.Lh, Smax_h, hws, c.ent_scale, c.ref_log_probs,
                                          c.kl_scale, c.grad_logits);
    case GRAD_NBEST:
        if constexpr (TAIL == 0)
            return ctc_launch_grad_wide<0>(c, ws, [](auto nv) { return ctc_grad_seq_wide_kernel<decltype(nv)::value, false, 0>; },
                                           c.K, c.pg_coef, c.pg_paths, c.hyp_len, c.Lh, Smax_h, hws, c.ent_scale, c.ref_log_probs,
                                           c.kl_scale, c.grad_logits);
        break;
    }
    return PGASR_ERR_INVALID_ARG;
}

// Every exported gradient pass: the checks, the workspace(s), the tail, the launch.  vmax is the limit the entry promises
// (CTC_VMAX or PGASR_WIDE_VMAX); rows of at most CTC_VMAX symbols of the per-frame multi-sample entry, which promises the wide limit,
// run the one-label-per-lane kernel.  All refusals for bad values come before those for unsupported sizes.
static int ctc_grad_run(const GradCall& c, GradForm form, int vmax) {
    const bool hyp = form == GRAD_SEQ || form == GRAD_NBEST;
    if (!c.log_probs || !c.input_lengths || !c.target_lengths || !c.grad_logits) return PGASR_ERR_INVALID_ARG;
    if ((c.ref_log_probs == nullptr) != (c.kl_scale == nullptr)) return PGASR_ERR_INVALID_ARG;
    if (form == GRAD_ONE ? (c.pg_coef == nullptr) != (c.pg_paths == nullptr) : !c.pg_coef || (form != GRAD_NBEST && !c.pg_paths))
        return PGASR_ERR_INVALID_ARG;
    if (hyp && !c.hyp_len) return PGASR_ERR_INVALID_ARG;
    if (form == GRAD_NBEST && (c.ent_scale || c.kl_scale)) return PGASR_ERR_INVALID_ARG;      // the N-best form has no tails
    int ok = PGASR_OK;
    if (hyp) {
        if (c.Lmax < 0 || c.blank < 0 || c.blank >= c.V) return PGASR_ERR_INVALID_ARG;
        ok = ctc_hyp_args_ok(c.T, c.B, c.V, c.K, c.Lh, vmax);
    } else if (form != GRAD_ONE && (c.K < 1 || c.K > PGASR_MAX_SAMPLES)) {
        return PGASR_ERR_INVALID_ARG;
    }
    if (ok == PGASR_OK) ok = ctc_args_ok(c.T, c.B, c.V, c.Lmax, c.blank, vmax);
    if (ok != PGASR_OK) return ok;
    CtcWs ws, hws{};
    if (!ctc_ws_bind(c.T, c.B, c.V, 2 * c.Lmax + 1, &ws, c.workspace, c.workspace_bytes)) return PGASR_ERR_WORKSPACE;
    if (hyp && !ctc_ws_bind(c.T, c.K * c.B, c.V, 2 * c.Lh + 1, &hws, c.hyp_workspace, c.hyp_workspace_bytes)) return PGASR_ERR_WORKSPACE;
    const bool narrow = vmax <= CTC_VMAX || (form == GRAD_STEPS && c.V <= CTC_VMAX);
    return ctc_with_tail(c, [&](auto tail) {
        constexpr int TAIL = decltype(tail)::value;
        if (!narrow) return ctc_grad_wide<TAIL>(c, form, ws, hws);
        if constexpr (TAIL == 2) return ctc_grad_narrow<2>(c, form, ws, hws, c.ent_scale, c.ref_log_probs, c.kl_scale);
        else if constexpr (TAIL == 1) return ctc_grad_narrow<1>(c, form, ws, hws, c.ent_scale);
        else return ctc_grad_narrow<0>(c, form, ws, hws);
    });
}

// The target lattice into ws: the sweeps with the states-per-thread variant that holds Smax.  Narrow: grid (B,3), whose third row
// builds the label lists.  Wide: ctc_labels_wide_kernel first, then the sweeps alone, grid (B,2).
static int ctc_launch_lattice(const GradCall& c, const int32_t* targets, float* nll, const CtcWs& ws, bool wide) {
    const int Lmax1 = c.Lmax > 0 ? c.Lmax : 1, Smax = 2 * c.Lmax + 1;
    hipStream_t st = (hipStream_t)c.stream;
    if (wide) {
        PGASR_LAUNCH_KERNEL(ctc_labels_wide_kernel, dim3(c.B), dim3(256), 0, st, targets, c.target_lengths, c.V, Lmax1, Smax, c.blank, ws);
        PGASR_CHECK_LAUNCH();
    }
    // Lmax == 0 still needs a valid targets row pointer; Lmax>=1 is the caller's job.
    // (a single-wave register-resident variant was measured SLOWER: 850 us vs 492 us at S=201 --
    // one wave's fp64 VALU issue rate, not the barrier, is then the limit)
#define PGASR_LATTICE(NSPT) PGASR_LAUNCH_KERNEL(ctc_lattice_kernel<NSPT>, dim3(c.B, wide ? 2 : 3), dim3(CTC_THREADS + 64), 0, st, c.log_probs, \
                        targets, c.input_lengths, c.target_lengths, c.T, c.B, c.V, Lmax1, Smax, c.blank, ws, nll, 0)
    if (Smax <= CTC_THREADS) PGASR_LATTICE(1);
    else if (Smax <= 2 * CTC_THREADS) PGASR_LATTICE(2);
    else if (Smax <= 4 * CTC_THREADS) PGASR_LATTICE(4);
    else PGASR_LATTICE(8);
#undef PGASR_LATTICE
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

// pgasr_ctc_loss_grad and _wide: the lattice, then (grad_logits given) the single-path pass with a per-utterance coefficient
static int ctc_loss_grad_run(const GradCall& c, const int32_t* targets, float* nll, int vmax) {
    if (!c.log_probs || !targets || !c.input_lengths || !c.target_lengths || !nll) return PGASR_ERR_INVALID_ARG;
    if ((c.pg_coef == nullptr) != (c.pg_paths == nullptr)) return PGASR_ERR_INVALID_ARG;
    int ok = ctc_args_ok(c.T, c.B, c.V, c.Lmax, c.blank, vmax);
    if (ok != PGASR_OK) return ok;
    CtcWs ws;
    if (!ctc_ws_bind(c.T, c.B, c.V, 2 * c.Lmax + 1, &ws, c.workspace, c.workspace_bytes)) return PGASR_ERR_WORKSPACE;
    ok = ctc_launch_lattice(c, targets, nll, ws, vmax > CTC_VMAX);
    return ok != PGASR_OK || !c.grad_logits ? ok : ctc_grad_run(c, GRAD_ONE, vmax);
}

// pgasr_ctc_hyp_lattice and _wide: the K*B hypothesis lattices, the ladder and the two families as in ctc_launch_lattice
static int ctc_hyp_lattice_run(const float* log_probs, const int32_t* hyp_tokens, int hyp_stride, const int32_t* hyp_len,
                               const int32_t* input_lengths, int T, int B, int V, int K, int Lh, int blank, float* hyp_nll,
                               void* hyp_workspace, size_t hyp_workspace_bytes, void* stream, int vmax) {
    if (!log_probs || !hyp_tokens || !hyp_len || !input_lengths || !hyp_nll) return PGASR_ERR_INVALID_ARG;
    if (blank < 0 || blank >= V || hyp_stride < 1 || hyp_stride < Lh) return PGASR_ERR_INVALID_ARG;
    const int ok = ctc_hyp_args_ok(T, B, V, K, Lh, vmax);
    if (ok != PGASR_OK) return ok;
    const int Smax = 2 * Lh + 1;
    const bool wide = vmax > CTC_VMAX;
    CtcWs ws;
    if (!ctc_ws_bind(T, K * B, V, Smax, &ws, hyp_workspace, hyp_workspace_bytes)) return PGASR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (wide) {
        PGASR_LAUNCH_KERNEL(ctc_hyp_labels_wide_kernel, dim3(K * B), dim3(256), 0, st, hyp_tokens, hyp_stride, hyp_len, V, Lh, Smax, blank, ws);
        PGASR_CHECK_LAUNCH();
    }
#define PGASR_HYP_LATTICE(NMAX) PGASR_LAUNCH_KERNEL(ctc_hyp_lattice_kernel<NMAX>, dim3(K * B, wide ? 2 : 3), dim3(CTC_THREADS + 64), 0, st, \
                        log_probs, hyp_tokens, hyp_stride, hyp_len, input_lengths, T, B, V, Lh, Smax, blank, ws, hyp_nll)
    if (Smax <= CTC_THREADS) PGASR_HYP_LATTICE(1);
    else if (Smax <= 2 * CTC_THREADS) PGASR_HYP_LATTICE(2);
    else if (Smax <= 4 * CTC_THREADS) PGASR_HYP_LATTICE(4);
    else PGASR_HYP_LATTICE(8);
#undef PGASR_HYP_LATTICE
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

}  // namespace

// ---- the exported entries: each fills a GradCall group by group ({head}, {policy gradient}, {hypotheses}, {tail}, output,
// workspace, stream) and names its form and V limit.  The narrow X -> X_ent -> X_kl chains forward with NULL tails. ----
extern "C" size_t pgasr_ctc_workspace_bytes(int T, int B, int V, int Lmax) {
    if (T <= 0 || B <= 0 || V <= 0 || Lmax < 0) return 0;
    return ctc_ws_layout(T, B, V, 2 * Lmax + 1, nullptr, nullptr);
}

extern "C" int pgasr_ctc_loss_grad(const float* log_probs, const int32_t* targets,
                                   const int32_t* input_lengths, const int32_t* target_lengths,
                                   int T, int B, int V, int Lmax, int blank,
                                   const float* utt_scale, const float* pg_coef, const int32_t* pg_path,
                                   float* nll, float* grad_logits,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    return ctc_loss_grad_run({{log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale}, {1, pg_coef, pg_path, 0}, {}, {},
                              grad_logits, workspace, workspace_bytes, stream}, targets, nll, CTC_VMAX);
}

// Second half of pgasr_ctc_loss_grad on its own: the gradient pass over a lattice that an earlier
// pgasr_ctc_loss_grad(..., grad_logits = NULL, ...) call with the SAME shapes left in `workspace`.
// Lets the host run the lattice (a 64-workgroup serial chain) on one stream beside the sampling /
// decode / edit-distance kernels whose rewards the gradient needs.
extern "C" int pgasr_ctc_grad_from_lattice(const float* log_probs, const int32_t* input_lengths,
                                           const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                           const float* utt_scale, const float* pg_coef, const int32_t* pg_path,
                                           int pg_coef_per_frame, float* grad_logits, void* workspace, size_t workspace_bytes,
                                           void* stream) {
    return pgasr_ctc_grad_from_lattice_ent(log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale, pg_coef, pg_path,
                                           pg_coef_per_frame, nullptr, grad_logits, workspace, workspace_bytes, stream);
}

extern "C" int pgasr_ctc_grad_from_lattice_ent(const float* log_probs, const int32_t* input_lengths,
                                               const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                               const float* utt_scale, const float* pg_coef, const int32_t* pg_path,
                                               int pg_coef_per_frame, const float* ent_scale, float* grad_logits,
                                               void* workspace, size_t workspace_bytes, void* stream) {
    return pgasr_ctc_grad_from_lattice_kl(log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale, pg_coef, pg_path,
                                          pg_coef_per_frame, ent_scale, nullptr, nullptr, grad_logits, workspace, workspace_bytes, stream);
}

extern "C" int pgasr_ctc_grad_from_lattice_kl(const float* log_probs, const int32_t* input_lengths,
                                              const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                              const float* utt_scale, const float* pg_coef, const int32_t* pg_path,
                                              int pg_coef_per_frame, const float* ent_scale, const float* ref_log_probs,
                                              const float* kl_scale, float* grad_logits,
                                              void* workspace, size_t workspace_bytes, void* stream) {
    return ctc_grad_run({{log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale},
                         {1, pg_coef, pg_path, pg_coef_per_frame ? 1 : 0}, {}, {ent_scale, ref_log_probs, kl_scale},
                         grad_logits, workspace, workspace_bytes, stream}, GRAD_ONE, CTC_VMAX);
}

// pgasr_ctc_grad_from_lattice with K sampled paths per utterance (multi-sample REINFORCE): pg_paths (K,T,B), pg_coef (K,B).
extern "C" int pgasr_ctc_grad_from_lattice_multi(const float* log_probs, const int32_t* input_lengths,
                                                 const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                                 const float* utt_scale, int K, const float* pg_coef, const int32_t* pg_paths,
                                                 float* grad_logits, void* workspace, size_t workspace_bytes, void* stream) {
    return pgasr_ctc_grad_from_lattice_multi_ent(log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale, K, pg_coef,
                                                 pg_paths, nullptr, grad_logits, workspace, workspace_bytes, stream);
}

extern "C" int pgasr_ctc_grad_from_lattice_multi_ent(const float* log_probs, const int32_t* input_lengths,
                                                     const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                                     const float* utt_scale, int K, const float* pg_coef, const int32_t* pg_paths,
                                                     const float* ent_scale, float* grad_logits, void* workspace,
                                                     size_t workspace_bytes, void* stream) {
    return pgasr_ctc_grad_from_lattice_multi_kl(log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale, K, pg_coef,
                                                pg_paths, ent_scale, nullptr, nullptr, grad_logits, workspace, workspace_bytes, stream);
}

extern "C" int pgasr_ctc_grad_from_lattice_multi_kl(const float* log_probs, const int32_t* input_lengths,
                                                    const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                                    const float* utt_scale, int K, const float* pg_coef, const int32_t* pg_paths,
                                                    const float* ent_scale, const float* ref_log_probs, const float* kl_scale,
                                                    float* grad_logits, void* workspace, size_t workspace_bytes, void* stream) {
    return ctc_grad_run({{log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale}, {K, pg_coef, pg_paths, 0}, {},
                         {ent_scale, ref_log_probs, kl_scale}, grad_logits, workspace, workspace_bytes, stream}, GRAD_MULTI, CTC_VMAX);
}

// ---- the frame policy's entropy: ent_mean (B) for monitoring and the loss value, ent_scale (B) for the *_ent gradient passes ----
extern "C" int pgasr_frame_entropy(const float* log_probs, const int32_t* input_lengths, int T, int B, int V,
                                   float beta, float inv_global_batch, float* ent_mean, float* ent_scale, void* stream) {
    if (!log_probs || !input_lengths || !ent_mean || !ent_scale) return PGASR_ERR_INVALID_ARG;
    if (T <= 0 || B <= 0 || V <= 0 || !(beta >= 0.f) || !(inv_global_batch > 0.f)) return PGASR_ERR_INVALID_ARG;
    if (V > CTC_VMAX) return PGASR_ERR_UNSUPPORTED;
    PGASR_LAUNCH_KERNEL(frame_entropy_kernel, dim3(B), dim3(64 * ENT_WAVES), 0, (hipStream_t)stream,
                       log_probs, input_lengths, T, B, V, beta, inv_global_batch, ent_mean, ent_scale);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

// ---- the KL of the frame policy from a frozen reference: kl_mean (B) for monitoring and the loss value, kl_scale (B) for the *_kl passes ----
extern "C" int pgasr_frame_kl(const float* log_probs, const float* ref_log_probs, const int32_t* input_lengths, int T, int B, int V,
                              float gamma, float inv_global_batch, float* kl_mean, float* kl_scale, void* stream) {
    if (!log_probs || !ref_log_probs || !input_lengths || !kl_mean || !kl_scale) return PGASR_ERR_INVALID_ARG;
    if (T <= 0 || B <= 0 || V <= 0 || !(gamma >= 0.f) || !(inv_global_batch > 0.f)) return PGASR_ERR_INVALID_ARG;
    if (V > CTC_VMAX) return PGASR_ERR_UNSUPPORTED;
    PGASR_LAUNCH_KERNEL(frame_kl_kernel, dim3(B), dim3(64 * ENT_WAVES), 0, (hipStream_t)stream,
                       log_probs, ref_log_probs, input_lengths, T, B, V, gamma, inv_global_batch, kl_mean, kl_scale);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

// ---- sequence-level REINFORCE: the K*B hypothesis lattices and the passes over K+1 lattices (see the kernels' comment) ----
extern "C" size_t pgasr_ctc_hyp_workspace_bytes(int T, int B, int V, int K, int Lh) {
    if (ctc_hyp_args_ok(T, B, V, K, Lh, CTC_VMAX) != PGASR_OK) return 0;
    return ctc_ws_layout(T, K * B, V, 2 * Lh + 1, nullptr, nullptr);
}

extern "C" int pgasr_ctc_hyp_lattice(const float* log_probs, const int32_t* hyp_tokens, int hyp_stride, const int32_t* hyp_len,
                                     const int32_t* input_lengths, int T, int B, int V, int K, int Lh, int blank,
                                     float* hyp_nll, void* hyp_workspace, size_t hyp_workspace_bytes, void* stream) {
    return ctc_hyp_lattice_run(log_probs, hyp_tokens, hyp_stride, hyp_len, input_lengths, T, B, V, K, Lh, blank, hyp_nll, hyp_workspace,
                               hyp_workspace_bytes, stream, CTC_VMAX);
}

extern "C" int pgasr_ctc_grad_from_lattices_seq(const float* log_probs, const int32_t* input_lengths, const int32_t* target_lengths,
                                                int T, int B, int V, int Lmax, int blank, const float* utt_scale,
                                                int K, const float* pg_coef, const int32_t* pg_paths, const int32_t* hyp_len, int Lh,
                                                float* grad_logits, void* workspace, size_t workspace_bytes,
                                                void* hyp_workspace, size_t hyp_workspace_bytes, void* stream) {
    return pgasr_ctc_grad_from_lattices_seq_ent(log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale, K, pg_coef,
                                                pg_paths, hyp_len, Lh, nullptr, grad_logits, workspace, workspace_bytes,
                                                hyp_workspace, hyp_workspace_bytes, stream);
}

extern "C" int pgasr_ctc_grad_from_lattices_seq_ent(const float* log_probs, const int32_t* input_lengths, const int32_t* target_lengths,
                                                    int T, int B, int V, int Lmax, int blank, const float* utt_scale,
                                                    int K, const float* pg_coef, const int32_t* pg_paths, const int32_t* hyp_len, int Lh,
                                                    const float* ent_scale, float* grad_logits, void* workspace, size_t workspace_bytes,
                                                    void* hyp_workspace, size_t hyp_workspace_bytes, void* stream) {
    return pgasr_ctc_grad_from_lattices_seq_kl(log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale, K, pg_coef,
                                               pg_paths, hyp_len, Lh, ent_scale, nullptr, nullptr, grad_logits, workspace, workspace_bytes,
                                               hyp_workspace, hyp_workspace_bytes, stream);
}

extern "C" int pgasr_ctc_grad_from_lattices_seq_kl(const float* log_probs, const int32_t* input_lengths, const int32_t* target_lengths,
                                                   int T, int B, int V, int Lmax, int blank, const float* utt_scale,
                                                   int K, const float* pg_coef, const int32_t* pg_paths, const int32_t* hyp_len, int Lh,
                                                   const float* ent_scale, const float* ref_log_probs, const float* kl_scale,
                                                   float* grad_logits, void* workspace, size_t workspace_bytes,
                                                   void* hyp_workspace, size_t hyp_workspace_bytes, void* stream) {
    return ctc_grad_run({{log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale}, {K, pg_coef, pg_paths, 0},
                         {hyp_len, Lh, hyp_workspace, hyp_workspace_bytes}, {ent_scale, ref_log_probs, kl_scale},
                         grad_logits, workspace, workspace_bytes, stream}, GRAD_SEQ, CTC_VMAX);
}

// MWER over N-best lists: the sequence pass without a path tensor.  Every pair (n,b) adds coef[n,b] (softmax - occ_{y_n}) from its
// hypothesis lattice, in n order, after the target part; hyp_len is what pgasr_ctc_hyp_lattice was given (0 for a pair that is not
// in the list or over the cap, whose coefficient is 0 and whose lattice -- the empty hypothesis' -- was really computed).
extern "C" int pgasr_ctc_grad_from_lattices_nbest(const float* log_probs, const int32_t* input_lengths, const int32_t* target_lengths,
                                                  int T, int B, int V, int Lmax, int blank, const float* utt_scale,
                                                  int N, const float* coef, const int32_t* hyp_len, int Lh,
                                                  float* grad_logits, void* workspace, size_t workspace_bytes,
                                                  void* hyp_workspace, size_t hyp_workspace_bytes, void* stream) {
    return ctc_grad_run({{log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale}, {N, coef, nullptr, 0},
                         {hyp_len, Lh, hyp_workspace, hyp_workspace_bytes}, {}, grad_logits, workspace, workspace_bytes, stream},
                        GRAD_NBEST, CTC_VMAX);
}

extern "C" int pgasr_pg_loss_value_seq(const float* log_probs, const int32_t* paths, int K, const int32_t* input_lengths,
                                       const float* nll, const float* utt_scale, const float* pg_coef,
                                       const float* hyp_nll, const int32_t* hyp_len, int Lh,
                                       int T, int B, int V, float* terms, void* stream) {
    if (!log_probs || !paths || !input_lengths || !nll || !utt_scale || !pg_coef || !hyp_nll || !hyp_len || !terms)
        return PGASR_ERR_INVALID_ARG;
    if (T <= 0 || B <= 0 || V <= 0 || Lh < 0) return PGASR_ERR_INVALID_ARG;
    if (K < 1 || K > PGASR_MAX_SAMPLES) return PGASR_ERR_INVALID_ARG;
    PGASR_LAUNCH_KERNEL(pg_loss_value_seq_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream,
                       log_probs, paths, K, input_lengths, nll, utt_scale, pg_coef, hyp_nll, hyp_len, Lh, T, B, V, terms);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

// ---- A5-WIDE: pgasr_ctc_loss_grad / pgasr_ctc_grad_from_lattice for 1 <= V <= 1024 (same workspace, same lattice kernel) ----
extern "C" int pgasr_ctc_loss_grad_wide(const float* log_probs, const int32_t* targets,
                                        const int32_t* input_lengths, const int32_t* target_lengths,
                                        int T, int B, int V, int Lmax, int blank,
                                        const float* utt_scale, const float* pg_coef, const int32_t* pg_path,
                                        float* nll, float* grad_logits,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    return ctc_loss_grad_run({{log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale}, {1, pg_coef, pg_path, 0}, {}, {},
                              grad_logits, workspace, workspace_bytes, stream}, targets, nll, PGASR_WIDE_VMAX);
}

extern "C" int pgasr_ctc_grad_from_lattice_wide(const float* log_probs, const int32_t* input_lengths,
                                                const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                                const float* utt_scale, const float* pg_coef, const int32_t* pg_path,
                                                int pg_coef_per_frame, float* grad_logits, void* workspace, size_t workspace_bytes,
                                                void* stream) {
    return ctc_grad_run({{log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale},
                         {1, pg_coef, pg_path, pg_coef_per_frame ? 1 : 0}, {}, {}, grad_logits, workspace, workspace_bytes, stream},
                        GRAD_ONE, PGASR_WIDE_VMAX);
}

// ---- A12-WIDE: pgasr_ctc_grad_from_lattice_multi with its entropy and KL forms in one entry, for 1 <= V <= 1024 ----
extern "C" int pgasr_ctc_grad_from_lattice_multi_wide(const float* log_probs, const int32_t* input_lengths,
                                                      const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                                      const float* utt_scale, int K, const float* pg_coef, const int32_t* pg_paths,
                                                      const float* ent_scale, const float* ref_log_probs, const float* kl_scale,
                                                      float* grad_logits, void* workspace, size_t workspace_bytes, void* stream) {
    return ctc_grad_run({{log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale}, {K, pg_coef, pg_paths, 0}, {},
                         {ent_scale, ref_log_probs, kl_scale}, grad_logits, workspace, workspace_bytes, stream}, GRAD_MULTI, PGASR_WIDE_VMAX);
}

// ---- A12-STEP: the multi-sample gradient pass with per-frame coefficients pg_coef (K,T,B), ONE entry for 1 <= V <= 1024 ----
// V <= 64 runs ctc_grad_multi_kernel (one label per lane) over the lattice pgasr_ctc_loss_grad left, V > 64
// ctc_grad_multi_wide_kernel's over pgasr_ctc_loss_grad_wide's -- the workspace layout is the same --, so coefficients that are
// constant over t give the bits of the per-utterance entries a caller would have taken for that V.
extern "C" int pgasr_ctc_grad_from_lattice_multi_steps(const float* log_probs, const int32_t* input_lengths,
                                                       const int32_t* target_lengths, int T, int B, int V, int Lmax, int blank,
                                                       const float* utt_scale, int K, const float* pg_coef, const int32_t* pg_paths,
                                                       const float* ent_scale, const float* ref_log_probs, const float* kl_scale,
                                                       float* grad_logits, void* workspace, size_t workspace_bytes, void* stream) {
    return ctc_grad_run({{log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale}, {K, pg_coef, pg_paths, 1}, {},
                         {ent_scale, ref_log_probs, kl_scale}, grad_logits, workspace, workspace_bytes, stream}, GRAD_STEPS, PGASR_WIDE_VMAX);
}

// ---- A13-WIDE: the hypothesis lattices and the pass over K+1 lattices for 1 <= V <= 1024 (same workspaces, same sweep kernel) ----
extern "C" size_t pgasr_ctc_hyp_workspace_bytes_wide(int T, int B, int V, int K, int Lh) {
    if (ctc_hyp_args_ok(T, B, V, K, Lh, PGASR_WIDE_VMAX) != PGASR_OK) return 0;
    return ctc_ws_layout(T, K * B, V, 2 * Lh + 1, nullptr, nullptr);
}

extern "C" int pgasr_ctc_hyp_lattice_wide(const float* log_probs, const int32_t* hyp_tokens, int hyp_stride, const int32_t* hyp_len,
                                          const int32_t* input_lengths, int T, int B, int V, int K, int Lh, int blank,
                                          float* hyp_nll, void* hyp_workspace, size_t hyp_workspace_bytes, void* stream) {
    return ctc_hyp_lattice_run(log_probs, hyp_tokens, hyp_stride, hyp_len, input_lengths, T, B, V, K, Lh, blank, hyp_nll, hyp_workspace,
                               hyp_workspace_bytes, stream, PGASR_WIDE_VMAX);
}

// pgasr_ctc_grad_from_lattices_seq, _seq_ent, _seq_kl and (pg_paths NULL) pgasr_ctc_grad_from_lattices_nbest in one entry
extern "C" int pgasr_ctc_grad_from_lattices_seq_wide(const float* log_probs, const int32_t* input_lengths, const int32_t* target_lengths,
                                                     int T, int B, int V, int Lmax, int blank, const float* utt_scale,
                                                     int K, const float* pg_coef, const int32_t* pg_paths, const int32_t* hyp_len, int Lh,
                                                     const float* ent_scale, const float* ref_log_probs, const float* kl_scale,
                                                     float* grad_logits, void* workspace, size_t workspace_bytes,
                                                     void* hyp_workspace, size_t hyp_workspace_bytes, void* stream) {
    return ctc_grad_run({{log_probs, input_lengths, target_lengths, T, B, V, Lmax, blank, utt_scale}, {K, pg_coef, pg_paths, 0},
                         {hyp_len, Lh, hyp_workspace, hyp_workspace_bytes}, {ent_scale, ref_log_probs, kl_scale},
                         grad_logits, workspace, workspace_bytes, stream}, pg_paths ? GRAD_SEQ : GRAD_NBEST, PGASR_WIDE_VMAX);
}
