// CTC forced alignment (Viterbi) for gfx950: the best single alignment of a known label sequence, its score, and the frames
// every token occupies (pgasr_ctc_forced_align; semantics in include/pgasr_hip.h, section A5-VIT).
//
// Three launches, one workgroup per utterance each:
//   align_fwd_kernel<NSPT> : the max-plus recursion over the utterance's frames.  ctc.hip's lattice structure -- 256 compute
//       threads with NSPT states each, the previous row double-buffered in LDS (fp64), one LDS-only barrier per frame, the next
//       frame's emissions prefetched off the chain -- with max3 + one add in place of lse3 + one add.  The compute threads put
//       their backpointer (0 stay, 1 step, 2 skip) into a second, double-buffered LDS row of bytes; the STORER wave copies every
//       finished byte row to the global [B][T][SP] array, so no compute wave has a store outstanding inside the frame loop (what
//       that costs: the comment at the storer in ctc.hip).  delta itself never leaves the chip: only the last row decides.
//   align_back_kernel      : the backtrace, one wave.  The state moves down by at most 2 per frame, so the backpointers of the
//       BT_F frames that end at state s lie in states [s - 2 BT_F, s]: the wave fetches that window of all BT_F frames with
//       independent loads (ceil(BT_F * BT_WW / 64) per lane, one memory round trip), every lane walks the block in LDS (all lanes
//       read the same byte: a broadcast), lane f keeps the state of the block's f-th frame and writes that frame's outputs.
//       T / BT_F round trips instead of T.
//   align_spans_kernel     : one thread per frame finds the token boundaries (into LDS), one thread per token writes its span and
//       adds its own frames' log-probs in ascending t.
//
// Numerics: fp64 max and add only, in a fixed order -- bit-identical to the numpy statement in tests/align_ref.py.
#include "common.h"

namespace {

constexpr int AL_THREADS = 256;
constexpr int AL_SPT = 8;                        // states per thread -> S <= 2048
constexpr int AL_SMAX = AL_THREADS * AL_SPT;
constexpr int AL_LMAX = (AL_SMAX - 1) / 2;       // 1023
constexpr int BT_F = 32;                         // frames per backtrace block
constexpr int BT_WW = 2 * BT_F / 4 + 1;          // 4-byte words that hold states [s - 2 BT_F, s] from a word boundary on
constexpr int BT_LOADS = (BT_F * BT_WW + 63) / 64;

struct AlignWs {
    uint32_t* bp;        // [B][T][SPW] words of four one-byte backpointers, state s in byte s & 3 of word s >> 2; row t = 0 is never written or read
    int SPW;             // SP / 4, SP = Smax rounded up to 64
    int32_t* end_state;  // [B] the state the best alignment ends in, -1 when there is none (or no frame)
    int32_t* ftok;       // [B][T] frame_token (the spans are cut from it whether or not the caller wants it)
};

__host__ __device__ inline size_t align_ws_layout(int T, int B, int Lmax, AlignWs* ws, char* base) {
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
    const int SP = (2 * Lmax + 1 + 63) / 64 * 64;
    const size_t p = take((size_t)B * T * SP);
    const size_t e = take((size_t)B * sizeof(int32_t));
    const size_t f = take((size_t)B * T * sizeof(int32_t));
    if (ws) {
        ws->bp = (uint32_t*)(base + p); ws->SPW = SP / 4;
        ws->end_state = (int32_t*)(base + e); ws->ftok = (int32_t*)(base + f);
    }
    return off;
}

// LDS-only barrier (as in ctc.hip): __syncthreads() would also drain vmcnt (the storer's stores, the emission prefetch)
#define ROW_BARRIER() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); \
                           asm volatile("" ::: "memory"); } while (0)

// grid (B), AL_THREADS compute threads + one storer wave
template <int NSPT>
__global__ __launch_bounds__(AL_THREADS + 64) void align_fwd_kernel(
    const float* __restrict__ lp, const int32_t* __restrict__ tokens, const int32_t* __restrict__ in_len,
    const int32_t* __restrict__ tk_len, int T, int B, int V, int Lmax, int blank, AlignWs ws, double* __restrict__ score) {
    // row buffers: position p = s + 2, two guard cells of -inf on each side; then the two backpointer rows (bytes)
    constexpr int ROW = NSPT * AL_THREADS + 4;
    constexpr int BPROW = NSPT * AL_THREADS;             // bytes
    __shared__ double lds[2 * ROW + 2 * BPROW / 8];
    double* rows = lds;
    unsigned char* bprows = (unsigned char*)(lds + 2 * ROW);
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    int Lb = tk_len[b]; Lb = Lb < 0 ? 0 : (Lb > Lmax ? Lmax : Lb);
    const int S = 2 * Lb + 1;
    const float* lpb = lp + (size_t)b * V;
    const size_t fstride = (size_t)B * V;
    const int32_t* tgt = tokens + (size_t)b * Lmax;
    auto row = [&](int i) { return rows + i * ROW; };
    const bool storer = tid >= AL_THREADS;
    for (int i = tid; i < 2 * ROW; i += AL_THREADS + 64) rows[i] = -INFINITY;

    int lab[NSPT];
    bool skip[NSPT];     // may come from s - 2
#pragma unroll
    for (int j = 0; j < NSPT; ++j) {
        const int s = storer ? S : tid + j * AL_THREADS;       // the storer owns no state
        lab[j] = blank; skip[j] = false;
        if (s < S && (s & 1)) lab[j] = tgt[s >> 1];
        if (s < S && (s & 1) && s >= 3) skip[j] = (tgt[s >> 1] != tgt[(s >> 1) - 1]);
        if (lab[j] < 0 || lab[j] >= V) lab[j] = blank;  // defensive: never index outside the row
    }
    __syncthreads();

    if (Tb == 0) {
        if (tid == 0) { score[b] = (Lb == 0) ? 0.0 : INFINITY; ws.end_state[b] = -1; }
        return;
    }

    // the storer wave's copy of one finished backpointer row: word w = ls + 64 i of the LDS row to the same word of row t_row
    uint32_t* bpg = ws.bp + (size_t)b * T * ws.SPW;
    const int SPW = ws.SPW;
    auto store_bp = [&](const unsigned char* br, int t_row) {
        const int ls = tid - AL_THREADS;
        const uint32_t* src = (const uint32_t*)br;
        uint32_t v[NSPT];
#pragma unroll
        for (int i = 0; i < NSPT; ++i) v[i] = src[ls + 64 * i];
        uint32_t* o = bpg + (size_t)t_row * SPW;
#pragma unroll
        for (int i = 0; i < NSPT; ++i)
            if (ls + 64 * i < SPW) o[ls + 64 * i] = v[i];      // SPW <= 64 NSPT: every word that holds a state is written
    };

    // frame 0
#pragma unroll
    for (int j = 0; j < NSPT; ++j) {
        const int s = storer ? S : tid + j * AL_THREADS;
        if (s < S && s <= 1) row(0)[s + 2] = (double)lpb[lab[j]];
    }
    int cur = 0;
    if (storer) {
        // its own loop (same number of barriers): after barrier k the backpointer row of frame k - 1 is complete and stays
        // untouched until barrier k + 1 (the compute threads write frame k's into the other buffer)
        for (int k = 1; k < Tb; ++k) {
            ROW_BARRIER();
            if (k >= 2) store_bp(bprows + ((k - 1) & 1) * BPROW, k - 1);
        }
    } else {
        float lpn[NSPT];
#pragma unroll
        for (int j = 0; j < NSPT; ++j) lpn[j] = 0.f;
        if (Tb > 1) {
            const float* lpt = lpb + fstride;
#pragma unroll
            for (int j = 0; j < NSPT; ++j) lpn[j] = lpt[lab[j]];
        }
        for (int k = 1; k < Tb; ++k) {
            float lpc[NSPT];
#pragma unroll
            for (int j = 0; j < NSPT; ++j) lpc[j] = lpn[j];
            if (k + 1 < Tb) {  // prefetch the next frame's emissions: off the dependent chain
                const float* lpt = lpb + (size_t)(k + 1) * fstride;
#pragma unroll
                for (int j = 0; j < NSPT; ++j) lpn[j] = lpt[lab[j]];
            }
            ROW_BARRIER();
            const double* rc = row(cur);
            double* rn = row(cur ^ 1);
            unsigned char* bw = bprows + (k & 1) * BPROW;
#pragma unroll
            for (int j = 0; j < NSPT; ++j) {
                // no test on the chain: all three neighbours are read (guard cells), a state that may not skip selects -inf
                const int s = tid + j * AL_THREADS;
                const int p = s + 2;
                const double c0 = rc[p];
                const double c1 = rc[p - 1];
                const double c2r = rc[p - 2];
                const double c2 = skip[j] ? c2r : -INFINITY;
                // the smallest move wins a tie: 1 only if c1 > c0, 2 only if c2 > max(c0, c1)
                const double m01 = (c1 > c0) ? c1 : c0;
                const int k01 = (c1 > c0) ? 1 : 0;
                const double m = (c2 > m01) ? c2 : m01;
                const int kk = (c2 > m01) ? 2 : k01;
                rn[p] = (s < S) ? m + (double)lpc[j] : -INFINITY;
                bw[s] = (unsigned char)((s < S) ? kk : 0);
            }
            cur ^= 1;
        }
    }
    __syncthreads();
    if (storer && Tb >= 2) store_bp(bprows + ((Tb - 1) & 1) * BPROW, Tb - 1);
    if (tid == 0) {
        const double* rc = row(cur);
        int e = S - 1;
        double d = rc[S - 1 + 2];
        if (S > 1 && rc[S - 2 + 2] > d) { e = S - 2; d = rc[S - 2 + 2]; }
        score[b] = -d;                                        // -(-inf) = +inf: no alignment
        ws.end_state[b] = (d == -INFINITY) ? -1 : e;
    }
}
#undef ROW_BARRIER

// grid (B), one wave
__global__ __launch_bounds__(64) void align_back_kernel(
    const int32_t* __restrict__ tokens, const int32_t* __restrict__ in_len, int T, int V, int Lmax, int blank, AlignWs ws,
    int32_t* __restrict__ frame_label, int32_t* __restrict__ frame_token) {
    __shared__ uint32_t tile[BT_LOADS * 64];
    const int b = blockIdx.x, lane = threadIdx.x;
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    const int end = ws.end_state[b];
    if (end < 0) Tb = 0;                    // no alignment: every frame reads -1
    int32_t* fl = frame_label + (size_t)b * T;
    int32_t* ft = ws.ftok + (size_t)b * T;
    int32_t* fto = frame_token ? frame_token + (size_t)b * T : nullptr;
    for (int t = Tb + lane; t < T; t += 64) {
        fl[t] = -1; ft[t] = -1;
        if (fto) fto[t] = -1;
    }
    if (Tb == 0) return;
    const int32_t* tgt = tokens + (size_t)b * Lmax;
    const uint32_t* bpg = ws.bp + (size_t)b * T * ws.SPW;
    const int SPW = ws.SPW;
    const unsigned char* tb = (const unsigned char*)tile;
    int s = end;                            // the state at frame t_hi, the same in every lane
    for (int t_hi = Tb - 1; t_hi >= 0; t_hi -= BT_F) {
        const int w0 = (s > 2 * BT_F ? s - 2 * BT_F : 0) >> 2;
        uint32_t v[BT_LOADS];
#pragma unroll
        for (int i = 0; i < BT_LOADS; ++i) {        // independent loads: one round trip for the whole block
            const int e = lane + 64 * i, f = e / BT_WW, j = e - f * BT_WW;
            const int t = t_hi - f, w = w0 + j;
            v[i] = 0;
            if (f < BT_F && t >= 1 && w < SPW) v[i] = bpg[(size_t)t * SPW + w];
        }
#pragma unroll
        for (int i = 0; i < BT_LOADS; ++i) tile[lane + 64 * i] = v[i];
        __syncthreads();
        int mine = 0;
        for (int f = 0; f < BT_F && f <= t_hi; ++f) {
            if (lane == f) mine = s;
            if (f < t_hi) {                 // frame t_hi - f >= 1 has a backpointer
                int k = tb[(f * BT_WW) * 4 + (s - 4 * w0)];
                k = k > 2 ? 2 : k;
                s = s - k < 0 ? 0 : s - k;
            }
        }
        __syncthreads();                    // the tile is free again
        if (lane < BT_F && lane <= t_hi) {
            const int t = t_hi - lane;
            int lab = blank, i = -1;
            if (mine & 1) {
                i = mine >> 1;
                lab = tgt[i];
                if (lab < 0 || lab >= V) lab = blank;
            }
            fl[t] = lab; ft[t] = i;
            if (fto) fto[t] = i;
        }
    }
}

// grid (B), 256 threads
__global__ __launch_bounds__(AL_THREADS) void align_spans_kernel(
    const float* __restrict__ lp, const int32_t* __restrict__ tokens, const int32_t* __restrict__ in_len,
    int T, int B, int V, int Lmax, int blank, AlignWs ws,
    int32_t* __restrict__ token_start, int32_t* __restrict__ token_end, double* __restrict__ token_logp) {
    __shared__ int st[AL_LMAX + 1], en[AL_LMAX + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    int Tb = in_len[b]; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    if (ws.end_state[b] < 0) Tb = 0;
    for (int i = tid; i < Lmax; i += AL_THREADS) { st[i] = -1; en[i] = -1; }
    __syncthreads();
    const int32_t* ft = ws.ftok + (size_t)b * T;
    for (int t = tid; t < Tb; t += AL_THREADS) {
        const int i = ft[t];
        if (i >= 0 && i < Lmax) {
            const int prev = t > 0 ? ft[t - 1] : -1, next = t + 1 < Tb ? ft[t + 1] : -1;
            if (prev != i) st[i] = t;
            if (next != i) en[i] = t + 1;
        }
    }
    __syncthreads();
    const int32_t* tgt = tokens + (size_t)b * Lmax;
    for (int i = tid; i < Lmax; i += AL_THREADS) {
        const int t0 = st[i], t1 = en[i];
        const size_t o = (size_t)b * Lmax + i;
        if (token_start) token_start[o] = t0;
        if (token_end) token_end[o] = t1;
        if (token_logp) {
            double acc = 0.0;
            if (t0 >= 0) {
                int lab = tgt[i];
                if (lab < 0 || lab >= V) lab = blank;
                for (int t = t0; t < t1; ++t) acc += (double)lp[((size_t)t * B + b) * V + lab];
            }
            token_logp[o] = acc;
        }
    }
}

}  // namespace

extern "C" size_t pgasr_ctc_align_workspace_bytes(int T, int B, int Lmax) {
    if (T <= 0 || B <= 0 || Lmax <= 0 || Lmax > AL_LMAX) return 0;
    return align_ws_layout(T, B, Lmax, nullptr, nullptr);
}

extern "C" int pgasr_ctc_forced_align(const float* log_probs, const int32_t* tokens, const int32_t* input_lengths,
                                      const int32_t* token_lengths, int T, int B, int V, int Lmax, int blank,
                                      double* score, int32_t* frame_label, int32_t* frame_token,
                                      int32_t* token_start, int32_t* token_end, double* token_logp,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!log_probs || !tokens || !input_lengths || !token_lengths || !score || !frame_label) return PGASR_ERR_INVALID_ARG;
    if (T <= 0 || B <= 0 || V <= 0 || Lmax <= 0 || blank < 0 || blank >= V) return PGASR_ERR_INVALID_ARG;
    if (2 * (long long)Lmax + 1 > AL_SMAX) return PGASR_ERR_UNSUPPORTED;
    AlignWs ws;
    const size_t need = align_ws_layout(T, B, Lmax, &ws, (char*)workspace);
    if (!workspace || workspace_bytes < need) return PGASR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int Smax = 2 * Lmax + 1;
#define PGASR_ALIGN_FWD(NSPT) PGASR_LAUNCH_KERNEL(align_fwd_kernel<NSPT>, dim3(B), dim3(AL_THREADS + 64), 0, st, \
                        log_probs, tokens, input_lengths, token_lengths, T, B, V, Lmax, blank, ws, score)
    if (Smax <= AL_THREADS) PGASR_ALIGN_FWD(1);
    else if (Smax <= 2 * AL_THREADS) PGASR_ALIGN_FWD(2);
    else if (Smax <= 4 * AL_THREADS) PGASR_ALIGN_FWD(4);
    else PGASR_ALIGN_FWD(8);
#undef PGASR_ALIGN_FWD
    PGASR_CHECK_LAUNCH();
    PGASR_LAUNCH_KERNEL(align_back_kernel, dim3(B), dim3(64), 0, st,
                       tokens, input_lengths, T, V, Lmax, blank, ws, frame_label, frame_token);
    PGASR_CHECK_LAUNCH();
    if (token_start || token_end || token_logp) {
        PGASR_LAUNCH_KERNEL(align_spans_kernel, dim3(B), dim3(AL_THREADS), 0, st,
                           log_probs, tokens, input_lengths, T, B, V, Lmax, blank, ws, token_start, token_end, token_logp);
        PGASR_CHECK_LAUNCH();
    }
    return PGASR_OK;
}
