// What the two workgroup-per-utterance CTC prefix beam searches share: beam_search_kernel (beam.hip, rows of up to 64 symbols, every
// candidate sorted) and beam_wide_kernel (beam_wide.hip, up to 1024 symbols, a top-`beam` selection).  Both rank candidates by the same
// key, keep prefixes in the same hash-consed trie and write the same N-best tail, and their tests compare them word for word; each of
// those pieces exists once, here.  A real difference is one template parameter: SYM_BITS (symbol bits of a packed trie node: 8 / 10),
// THREADS (workgroup size), FAST (fp32 exp/log on the differences).  The single-wave kernel (namespace sb in beam.hip) shares none of
// this: its table and its tail are a different design.
#pragma once
#include "common.h"
#include <cmath>

namespace beam_core {

// ---- scores: CTCdecoder.py:31-39 with 2 or 3 arguments (argument order preserved) ----
__device__ __forceinline__ double lse2(double a, double b) {
    const double m = fmax(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + log(exp(a - m) + exp(b - m));
}
__device__ __forceinline__ double lse3(double a, double b, double c) {
    const double m = fmax(fmax(a, b), c);
    if (m == -INFINITY) return -INFINITY;
    return m + log((exp(a - m) + exp(b - m)) + exp(c - m));
}

// Fast variants (fp32 device log-probs, training-time rewards): fp64 carries, fp32 exp/log on the
// differences to the maximum -- the software fp64 transcendentals dominate the exact path (28 ms
// vs ~1/4 of that for T=1000, beam 16, 32 utterances).  Scores differ from the exact path by
// ~1e-7 relative, so only exact score ties could rank differently.
template <bool FAST> __device__ __forceinline__ double lse2x(double a, double b) {
    if (!FAST) return lse2(a, b);
    const double m = fmax(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + (double)__logf(__expf((float)(a - m)) + __expf((float)(b - m)));
}
template <bool FAST> __device__ __forceinline__ double lse3x(double a, double b, double c) {
    if (!FAST) return lse3(a, b, c);
    const double m = fmax(fmax(a, b), c);
    if (m == -INFINITY) return -INFINITY;
    return m + (double)__logf((__expf((float)(a - m)) + __expf((float)(b - m))) + __expf((float)(c - m)));
}

// ---- rank: (score descending, first-touch time ascending), the reference's stable sort over dict insertion order (:110-113) ----
// order-preserving map double -> u64 (ascending)
__device__ __forceinline__ unsigned long long ordered_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

struct SortItem { unsigned long long key; unsigned time; unsigned cand; };   // key = ~ordered(score): ascending sort = score descending

__device__ __forceinline__ bool item_less(const SortItem& a, const SortItem& b) {
    return a.key < b.key || (a.key == b.key && a.time < b.time);
}

// Bitonic sort of P (a power of two) items in LDS; the caller has synchronised after filling them, and the sort ends with a barrier.
// Element i is handled by thread i % THREADS, so all elements of a 64-aligned group belong to one
// wave: a pass with partner distance j2 < 64 exchanges only inside a wave (LDS accesses of one
// wave are ordered) and needs a workgroup barrier only next to a cross-wave pass.
template <int THREADS> __device__ __forceinline__ void bitonic_sort(SortItem* items, int P, int tid) {
    bool prev_cross = false;
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
        for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            const bool cross = j2 >= 64;
            if (cross || prev_cross) __syncthreads();
            for (int i = tid; i < P; i += THREADS) {
                const int l = i ^ j2;
                if (l > i) {
                    const SortItem x = items[i], y = items[l];
                    const bool up = ((i & k2) == 0);
                    if (item_less(y, x) == up) { items[i] = y; items[l] = x; }
                }
            }
            prev_cross = cross;
        }
    }
    __syncthreads();
}

// ---- prefix identity: a per-utterance trie in the global workspace, hash-consed so that one prefix has ONE id ----
template <int SYM_BITS> struct TrieWs {
    static constexpr unsigned SYM_MASK = (1u << SYM_BITS) - 1u;
    static constexpr long long MAX_NODES = 1ll << (32 - SYM_BITS);      // parent << SYM_BITS | symbol is one 32-bit word
    unsigned long long* table;   // [B][H] open addressing: (key + 1) << 32 | node id; 0 = empty
    unsigned* nodes;             // [B][NN] parent << SYM_BITS | symbol; node 0 = root
    int H, NN;
};

template <int SYM_BITS>
__host__ __device__ inline size_t trie_ws_layout(int T, int B, int beam, TrieWs<SYM_BITS>* ws, char* base) {
    const long long nn = (long long)T * beam + 1;
    long long H = 1024;
    while (H < 2 * nn) H <<= 1;
    size_t off = 0;
    const size_t t_off = off; off += (size_t)B * (size_t)H * sizeof(unsigned long long);
    off = (off + 255) / 256 * 256;
    const size_t n_off = off; off += (size_t)B * (size_t)nn * sizeof(unsigned);
    off = (off + 255) / 256 * 256;
    if (ws) {
        ws->table = (unsigned long long*)(base + t_off);
        ws->nodes = (unsigned*)(base + n_off);
        ws->H = (int)H; ws->NN = (int)nn;
    }
    return off;
}

// The canonical node of (parent id, symbol) in one utterance's table / nodes: look up, else create (the next id of *counter, a
// workgroup-shared word).  At most H probes, and no store past the NN nodes whatever *counter holds; 0 (the root) if none was placed --
// which cannot happen while the table holds at most T * beam + 1 <= H / 2 keys.
template <int SYM_BITS>
__device__ __forceinline__ int trie_find_or_create(unsigned long long* table, unsigned* nodes, int H, int NN, int* counter, int parent, int sym) {
    const unsigned hmask = (unsigned)H - 1u;
    const unsigned keyv = ((unsigned)parent << SYM_BITS) | (unsigned)sym;
    unsigned h = (keyv * 2654435761u) & hmask;
    int node = -1;
    bool placed = false;
    for (int probe = 0; probe < H && !placed; ++probe) {
        const unsigned long long slot = table[h];
        if (slot == 0ull) {
            if (node < 0) { node = atomicAdd(counter, 1); if (node < NN) nodes[node] = keyv; }
            const unsigned long long want = ((unsigned long long)(keyv + 1u) << 32) | (unsigned)node;
            const unsigned long long old = atomicCAS(&table[h], 0ull, want);
            if (old == 0ull) placed = true;
            else if ((unsigned)(old >> 32) == keyv + 1u) { node = (int)(unsigned)old; placed = true; }   // cannot happen within a frame
        } else if ((unsigned)(slot >> 32) == keyv + 1u) { node = (int)(unsigned)slot; placed = true; }
        h = (h + 1u) & hmask;
    }
    return placed ? node : 0;
}

// ---- N-best result: the final beam is ranked (the last frame's sort IS sorted(...)[:N], CTCdecoder.py:110-113), so row r is entry r ----
// Thread r walks the ancestors of entry r: the chains are independent and run side by side, one chain's latency in all.  A walk ends at
// the root, after Tb steps (a prefix has at most one symbol per frame) or at an id outside the node store, whatever nodes[] holds.
// out_tokens (N, B, S), out_len / out_score (N, B): the (K, B, stride) layout of pgasr_ctc_hyp_lattice.  id / pb / pnb: the final beam
// of nb entries; hlen: N <= THREADS words of LDS, free after the frame loop.  Called by every thread of the workgroup.
template <int SYM_BITS, int THREADS, bool FAST>
__device__ __forceinline__ void nbest_tail(const unsigned* nodes, int NN, int Tb, int b, int tid, int N, int S, int collapse, int nb,
                                           const int* id, const double* pb, const double* pnb, int* hlen,
                                           int32_t* __restrict__ out_tokens, int32_t* __restrict__ out_len,
                                           double* __restrict__ out_score, int32_t* __restrict__ out_count) {
    const int B = (int)gridDim.x;
    const int count = N < nb ? N : nb;
    if (tid < N) {
        int n = 0;
        double sc = INFINITY;                  // rows beyond count: length 0, score +inf, tokens zero
        if (tid < count) {
            int32_t* o = out_tokens + ((size_t)tid * B + b) * S;
            const int head = id[tid];
            for (int v = head; v > 0 && v < NN && n < Tb; v = (int)(nodes[v] >> SYM_BITS)) ++n;
            int v = head;
            for (int k = n - 1; k >= 0; --k) { const unsigned w = nodes[v]; o[k] = (int32_t)(w & TrieWs<SYM_BITS>::SYM_MASK); v = (int)(w >> SYM_BITS); }
            if (collapse) {      // collapse_fn on this hypothesis alone: rows that become equal strings stay separate rows
                int w = 0;
                for (int i = 0; i < n; ++i) if (i == 0 || o[i] != o[i - 1]) { const int32_t x = o[i]; o[w++] = x; }
                n = w;
            }
            sc = -lse2x<FAST>(pb[tid], pnb[tid]);
        }
        hlen[tid] = n;
        out_len[(size_t)tid * B + b] = n;
        out_score[(size_t)tid * B + b] = sc;
    }
    if (tid == 0) out_count[b] = count;
    __threadfence_block();
    __syncthreads();
    for (int r = 0; r < N; ++r) {              // zero tails (and whole rows beyond count), coalesced
        int32_t* o = out_tokens + ((size_t)r * B + b) * S;
        for (int i = hlen[r] + tid; i < S; i += THREADS) o[i] = 0;
    }
}

// ---- host: the argument checks every entry point of the two searches makes, in the order and with the statuses they have always had ----
// `own()` runs the entry's own checks (the language model's arguments, the flag mask, the list's) where they stand: behind the limits,
// before the workspace.  No HIP call.  PGASR_OK with *ws laid out in `workspace`.
template <int SYM_BITS, class Own>
inline int beam_check_args(const void* log_probs, const int32_t* out_tokens, const int32_t* out_len, const double* out_score,
                           int T, int B, int V, int beam, int blank, int vmax, int kmax, Own&& own,
                           void* workspace, size_t workspace_bytes, TrieWs<SYM_BITS>* ws) {
    if (!log_probs || !out_tokens || !out_len || !out_score) return PGASR_ERR_INVALID_ARG;
    if (T <= 0 || B <= 0 || V <= 0 || beam <= 0 || blank < 0 || blank >= V) return PGASR_ERR_INVALID_ARG;
    if (V > vmax || beam > kmax) return PGASR_ERR_UNSUPPORTED;
    if (const int st = own()) return st;
    const size_t need = trie_ws_layout(T, B, beam, ws, (char*)workspace);
    if (!workspace || workspace_bytes < need) return PGASR_ERR_WORKSPACE;
    if ((long long)T * beam + 1 >= TrieWs<SYM_BITS>::MAX_NODES) return PGASR_ERR_UNSUPPORTED;
    return PGASR_OK;
}

}  // namespace beam_core
