// Exact CTC prefix beam search for rows of up to 1024 symbols on gfx950 (CTCdecoder.py:41-116; include/pgasr_hip.h, A7-WIDE).
//
// The kernels of beam.hip lay one symbol per lane, pack a trie node as parent << 8 | symbol and SORT all beam * V candidates of a
// frame: at V = 1024, beam = 128 that is 131072 candidates, which neither fit the LDS nor are worth sorting -- at most `beam` survive.
// This kernel keeps that file's algebra (the same candidates, the same log-sum-exp calls in the same argument order, so the scores
// are the same bits) and replaces the sort by a top-`beam` SELECTION that returns exactly what the sort would.  What the two have in
// common is not restated here: the log-sum-exp forms, the rank key and its bitonic sort, the trie (workspace layout, find-or-create)
// and the N-best result tail are those of beam_core.h, which both files include.
//
//   * one workgroup of 256 threads per utterance, frames a serial chain; the frame's V log-probs and the beam state (p_b, p_nb, node
//     id, last symbol, parent id, the parent's position) live in LDS;
//   * prefix identity is the hash-consed trie of beam.hip in the global workspace with 10-bit symbols (node = parent << 10 | symbol);
//     only the winners of a frame insert nodes;
//   * "the extension of entry i by s already sits in the beam" is bit (i, s) of a beam x V bitmap in LDS, rebuilt every frame; such an
//     extension is no candidate of its own: its mass goes into that entry's stay candidate in the reference's update order;
//   * every candidate has the unique rank key (score image, touch time): score image = the order-preserving u64 map of its fp64 total,
//     touch time = 2 * (symbol * nb + rank) + (0: the extension touched first in that iteration of the reference's loop nest, 1: the
//     kept prefix touched second) -- the position of the candidate's FIRST touch in the reference's dict, so (score descending, time
//     ascending) is the reference's stable sort, the stay-against-own-repeat pair included;
//   * selection: a threshold theta = the beam-th largest score image among 2 * nb candidates that certainly exist (every stay, every
//     entry's extension by the frame's best symbol that is neither merged nor its own repeat) -- nothing below theta can enter the
//     beam; all candidates >= theta are appended to an LDS list of WIDE_CAP items and sorted by the bitonic sort of beam.hip.  If the
//     list overflows (or flags bit 5 forces it) a COUNTING selection finds the exact (score image, time) of rank beam - 1 by radix
//     passes over the 96-bit key with an LDS histogram, most significant digit first, keys recomputed in every pass; the candidates
//     at or above that cut -- exactly min(beam, all) by uniqueness of the key -- are then listed and sorted.  Both paths rank by the
//     same key, so both are exact and equal.
// Every loop is bounded by construction: hash probes by the table size, ancestor walks by lengths[b], radix passes by the key width.
// With a back-off unit n-gram model (pgasr_ctc_beam_search_wide_lm) the same kernel fuses its scores in; see WideLm below.  With a
// hotword automaton (pgasr_ctc_beam_search_wide_bias) it adds the phrase bonuses, with or without the model; see WideBias.
#include "common.h"
#include "beam_core.h"
#include "bias_table.h"
#include "unit_lm.h"
#include <cmath>
#include <type_traits>

namespace {

using namespace beam_core;

constexpr int WIDE_KMAX = 128;
constexpr int WIDE_VMAX = 1024;
constexpr int WIDE_THREADS = 256;
constexpr int WIDE_CAP = 2048;                       // items of the candidate list: a frame with more candidates >= theta takes the counting selection
constexpr int WIDE_SYM_BITS = 10;                    // a trie node is parent << 10 | symbol, so node ids are 22 bits
using WideWs = TrieWs<WIDE_SYM_BITS>;
constexpr int WIDE_RADIX_PASSES = 12;                // 8 digits of the score image, 4 of the touch time
constexpr unsigned WIDE_STAY = 0x80000000u;          // cand: WIDE_STAY | entry, else entry * V + symbol

// p_nb of the extension of an entry (p_b, p_nb) by a symbol of log-prob ps (:90-96); rep: the symbol repeats the entry's last one
template <bool FAST> __device__ __forceinline__ double wide_ext(double pbj, double pnbj, double ps, bool rep) {
    return rep ? lse2x<FAST>(-INFINITY, pbj + ps) : lse3x<FAST>(-INFINITY, pbj + ps, pnbj + ps);
}

// LDS: fixed layout for the largest shape (all offsets multiples of 16)
struct WideLds {
    SortItem items[WIDE_CAP];                   // 32 KB candidate list
    double frame[WIDE_VMAX];                    // the frame's log-probs
    unsigned bitmap[WIDE_KMAX * (WIDE_VMAX / 32)];      // bit (i, s): the extension of entry i by s sits in the beam
    unsigned long long tkeys[2 * WIDE_KMAX];    // the 2 * nb score images the threshold is formed from
    double pb[2][WIDE_KMAX], pnb[2][WIDE_KMAX]; // beam state, double-buffered
    double st_pb[WIDE_KMAX], st_pnb[WIDE_KMAX]; // the stay candidate of every entry
    unsigned long long st_img[WIDE_KMAX];
    int id[2][WIDE_KMAX], last[2][WIDE_KMAX], par[2][WIDE_KMAX];
    int pidx[WIDE_KMAX];                        // position of the entry's parent in the beam, -1 if it is not there
    unsigned st_time[WIDE_KMAX];
    unsigned hist[256];
    unsigned long long theta, cut_hi;
    unsigned cut_lo;
    int nb, nodes, total, done, need, counting;
};

// Fusion of a back-off unit n-gram model (LM = true, pgasr_ctc_beam_search_wide_lm; include/pgasr_hip.h, A7-WIDE-LM): A7-LM's algebra --
// every term that enters a prefix by an extension with a non-blank s gets w = alpha * (double)lp32(ctx(prefix), s) + beta added, the
// merged term of a stay candidate with its parent's context -- over the packed tables of lm.UnitNgramLM.  A back-off chain per candidate
// would be a divergent pointer chase over up to 131072 candidates a frame, so every beam entry owns a dense ROW of its LM state in the
// global workspace: lp[s] = lp32(state, s) and next[s] = the state after s, V words each.
//   * 2 * K rows per utterance, reached through a per-entry slot: an entry that stays keeps its row; only a winner that is an extension
//     takes a free one (the rows of the stay winners are marked, the e-th extension takes the e-th unmarked row);
//   * the workgroup fills the new rows level by level: thread r walks its winner's back-off chain once (at most `order` states) and
//     keeps the top-down prefix sums of the bows -- the contractual order --, then the states' successor lists are scattered over the
//     rows as float32(sum + logp), the empty context (all V-1 unigrams, kept in LDS for the whole call) first, the longest context
//     last, a barrier between levels; the lists are sorted by symbol, so the reads are coalesced;
//   * a candidate then costs one fp32 load of an L2-resident row beside the frame's log-prob -- the words of entry j + 1 are loaded
//     while entry j's candidates are scored --; a winner's new state is next[s].
// The threshold's extension candidate of an entry is the one of largest frame[s] + w: a candidate that exists, its image with its own
// w in it, so theta stays a valid lower bound.  The model's arguments are a parameter pack behind the kernel's own, empty without a model
// (LM = false): those instantiations keep their argument list and carry none of this.
constexpr int WIDE_LM_ORDER_MAX = 5;
template <bool LM> struct WideLm {};
template <> struct WideLm<true> {
    const int4* states;      // (n_states) {bow bits, back-off state, first successor, one past the last}; state 0 = the empty context
    const int4* succ;        // (n_succ) {symbol, logp bits, next state, 0}, a state's successors consecutive and ascending in the symbol
    int n_states, n_succ, start, order;
    float* rows;             // [B][2 K][2][V]: lp, then next (as int)
    double alpha, beta;
};
struct WideLmLds {
    double acc[WIDE_KMAX][WIDE_LM_ORDER_MAX];   // acc[r][p]: the bows of chain[r][0 .. p-1], summed in that order
    int chain[WIDE_KMAX][WIDE_LM_ORDER_MAX];    // the back-off chain of winner r's state, the state itself first, state 0 last
    int depth[WIDE_KMAX];
    int st[2][WIDE_KMAX], row[2][WIDE_KMAX];    // an entry's LM state and the slot of its row
    float own[2][WIDE_KMAX];                    // lp32(ctx(parent prefix), last): the word of the entry's own last emission
    int isext[WIDE_KMAX];
    int used[2 * WIDE_KMAX];
    float uni_lp[WIDE_VMAX];                    // the successors of the empty context by symbol: every row starts from these
    int uni_next[WIDE_VMAX];
    unsigned long long freemask[WIDE_THREADS / 64], extmask[WIDE_THREADS / 64];
};
constexpr size_t WIDE_LM_LDS_OFFSET = (sizeof(WideLds) + 15) / 16 * 16;

// Hotword (contextual phrase) biasing (pgasr_ctc_beam_search_wide_bias; include/pgasr_hip.h, A7-WIDE-BIAS): A7-BIAS's algebra on this
// kernel's candidates, over the dense automaton of lm.HotwordBias -- S * V 8-byte words {int32 next; float bonus}, word (q, s) at
// q V + s, the layout beam.hip and hotword.hip read.  The table IS the row of every state, so nothing is cached or filled:
//   * an entry carries st = the automaton state of its prefix (the root, 0, for the empty one; always inside [0, S): a next outside
//     is taken as 0 where it is read) and own = the bonus of its own last emission, bonus[st(parent prefix), last];
//   * every term that enters a prefix by an extension with a non-blank s gets w added: wb = __dmul_rn(weight, (double)bonus), w = wb
//     without a model and __dadd_rn(__dadd_rn(__dmul_rn(alpha, (double)lp32), beta), wb) with one; the merged term of a stay candidate
//     gets the entry's own w, from `own`;
//   * a candidate (entry j, symbol s) reads word st_j V + s, consecutive lanes consecutive words, entry j + 1's while entry j's are
//     scored; bonuses can be negative (leaving a phrase takes the pending credit back), so the threshold's extension candidate is the
//     symbol of largest frame[s] + w, as with the model;
//   * the thread that writes an extension winner re-reads its word -- one independent 8-byte load in front of trie_find_or_create --
//     for the new state and the new own bonus.
using bias_table::BiasWord;
struct WideBias {
    const BiasWord* table;   // S * V words
    int n_states;            // S
    double weight;
};
struct WideNoBias {};
struct WideBiasLds {
    int st[2][WIDE_KMAX];                       // the automaton state of the entry's prefix
    float own[2][WIDE_KMAX];                    // bonus[st(parent prefix), last]: the bonus of the entry's own last emission
};
constexpr size_t WIDE_LM_BIAS_LDS_OFFSET = (WIDE_LM_LDS_OFFSET + sizeof(WideLmLds) + 15) / 16 * 16;

template <bool FAST> __device__ __forceinline__ double wide_ext_w(double pbj, double pnbj, double ps, bool rep, double w) {
    const double eb = (pbj + ps) + w, en = (pnbj + ps) + w;
    return rep ? lse2x<FAST>(-INFINITY, eb) : lse3x<FAST>(-INFINITY, eb, en);
}

// LmArg: nothing (the search of A7-WIDE: its argument list, and with it its code, is what it was without a model), WideLm<true>,
// WideBias, or WideLm<true> and WideBias in that order
template <typename X, typename... A> constexpr bool wide_has = (std::is_same<X, A>::value || ...);
__device__ __forceinline__ WideLm<false> wide_lm_of() { return {}; }
__device__ __forceinline__ WideLm<false> wide_lm_of(const WideBias&) { return {}; }
template <typename... R> __device__ __forceinline__ const WideLm<true>& wide_lm_of(const WideLm<true>& lm, const R&...) { return lm; }
__device__ __forceinline__ WideNoBias wide_bias_of() { return {}; }
__device__ __forceinline__ WideNoBias wide_bias_of(const WideLm<true>&) { return {}; }
__device__ __forceinline__ const WideBias& wide_bias_of(const WideBias& bias) { return bias; }
__device__ __forceinline__ const WideBias& wide_bias_of(const WideLm<true>&, const WideBias& bias) { return bias; }

// w of a term: the model's word and the automaton's bonus, each where there is one (A7-LM / A7-BIAS: the roundings are contractual)
template <typename Lm, typename Bs> __device__ __forceinline__ double wide_w(const Lm& lm, const Bs& bias, float word, float bonus) {
    constexpr bool LM = std::is_same<Lm, WideLm<true>>::value, BIAS = std::is_same<Bs, WideBias>::value;
    static_assert(LM || BIAS, "a term without a model has no w");
    if constexpr (LM && BIAS) return __dadd_rn(__dadd_rn(__dmul_rn(lm.alpha, (double)word), lm.beta), __dmul_rn(bias.weight, (double)bonus));
    else if constexpr (LM) return __dadd_rn(__dmul_rn(lm.alpha, (double)word), lm.beta);
    else return __dmul_rn(bias.weight, (double)bonus);
}

template <typename TIn, bool FAST, typename... LmArg>
__global__ __launch_bounds__(WIDE_THREADS) void beam_wide_kernel(
    const TIn* __restrict__ lp, long long stride_t, long long stride_b, const int32_t* __restrict__ lengths,
    int T, int V, int K, int blank, int collapse, int force_counting, WideWs ws, int nbest, int tok_stride,
    int32_t* __restrict__ out_tokens, int32_t* __restrict__ out_len, double* __restrict__ out_score,
    int32_t* __restrict__ out_count, int32_t* __restrict__ out_counting, const LmArg... lmarg) {
    constexpr bool LM = wide_has<WideLm<true>, LmArg...>, BIAS = wide_has<WideBias, LmArg...>;
    [[maybe_unused]] const auto& lm = wide_lm_of(lmarg...);
    [[maybe_unused]] const auto& bias = wide_bias_of(lmarg...);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    WideLds& L = *reinterpret_cast<WideLds*>(smem);
    [[maybe_unused]] WideLmLds& M = *reinterpret_cast<WideLmLds*>(smem + WIDE_LM_LDS_OFFSET);
    [[maybe_unused]] WideBiasLds& H = *reinterpret_cast<WideBiasLds*>(smem + (LM ? WIDE_LM_BIAS_LDS_OFFSET : WIDE_LM_LDS_OFFSET));
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int Tb = lengths ? lengths[b] : T; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    const int W = (V + 31) >> 5;                          // bitmap words per entry

    unsigned long long* table = ws.table + (size_t)b * ws.H;
    unsigned* nodes = ws.nodes + (size_t)b * ws.NN;

    if (tid == 0) {
        L.nb = 1; L.nodes = 1; L.counting = 0;
        L.id[0][0] = 0; L.last[0][0] = -1; L.par[0][0] = -1; L.pb[0][0] = 0.0; L.pnb[0][0] = -INFINITY;
        nodes[0] = 0xFFFFFFFFu;
        if constexpr (LM) { M.st[0][0] = lm.start; M.own[0][0] = 0.0f; M.isext[0] = 1; }
        if constexpr (BIAS) { H.st[0][0] = 0; H.own[0][0] = 0.0f; }               // state 0 is the automaton's root
    }
    __syncthreads();
    [[maybe_unused]] float* lmrows = nullptr;
    // the rows of the extension winners among the n entries of buffer `buf` (M.isext; M.st set, the stay winners' M.row set): take
    // free slots, walk the chains, scatter the lists.  Called by every thread; ends with a barrier.
    [[maybe_unused]] auto fill_rows = [&](int buf, int n) {
        if constexpr (LM) {
            M.used[tid] = 0;                                                      // 2 * WIDE_KMAX == WIDE_THREADS
            __syncthreads();
            const bool ext = tid < n && M.isext[tid];
            if (tid < n && !ext) M.used[M.row[buf][tid]] = 1;
            __syncthreads();
            const unsigned long long fm = __ballot(tid < 2 * K && !M.used[tid]), em = __ballot(ext);
            if (lane == 0) { M.freemask[wave] = fm; M.extmask[wave] = em; }
            __syncthreads();
            if (ext) {
                int e = __popcll(M.extmask[wave] & ((1ull << lane) - 1ull));      // rank among the extension winners
                for (int w = 0; w < wave; ++w) e += __popcll(M.extmask[w]);
                int slot = 0;                                                     // the e-th free slot: at most K are marked, so one exists
                for (int w = 0; w < WIDE_THREADS / 64; ++w) {
                    unsigned long long m = M.freemask[w];
                    const int c = __popcll(m);
                    if (e >= c) { e -= c; continue; }
                    for (int k = 0; k < e; ++k) m &= m - 1ull;
                    slot = 64 * w + __ffsll((long long)m) - 1;
                    break;
                }
                M.row[buf][tid] = slot;
                int s = M.st[buf][tid];
                s = (s < 0 || s >= lm.n_states) ? 0 : s;
                double a = 0.0;
                int d = 0;
                for (; d < WIDE_LM_ORDER_MAX; ++d) {                              // top-down: the state itself, then ever shorter contexts
                    if (d == WIDE_LM_ORDER_MAX - 1) s = 0;                        // a chain has at most `order` states; never walk past that
                    M.chain[tid][d] = s; M.acc[tid][d] = a;
                    if (s == 0) { ++d; break; }
                    const int4 rec = lm.states[s];
                    a = a + (double)__int_as_float(rec.x);
                    s = (rec.y < 0 || rec.y >= lm.n_states) ? 0 : rec.y;
                }
                M.depth[tid] = d;
            }
            __syncthreads();
            for (int r = wave; r < n; r += WIDE_THREADS / 64) {                   // the empty context: all V-1 unigrams, from LDS
                if (!M.isext[r]) continue;
                const double a = M.acc[r][M.depth[r] - 1];
                float* rl = lmrows + (size_t)M.row[buf][r] * 2 * V;
                int* rn = reinterpret_cast<int*>(rl + V);
                for (int s = lane; s < V; s += 64) { rl[s] = (float)(a + (double)M.uni_lp[s]); rn[s] = M.uni_next[s]; }
            }
            __syncthreads();
            for (int q = 1; q < lm.order; ++q) {                                  // level q above the empty context
                for (int r = wave; r < n; r += WIDE_THREADS / 64) {
                    if (!M.isext[r] || q >= M.depth[r]) continue;
                    const int p = M.depth[r] - 1 - q;
                    const int4 rec = lm.states[M.chain[r][p]];
                    const double a = M.acc[r][p];
                    const int lo = rec.z < 0 ? 0 : rec.z, hi = rec.w > lm.n_succ ? lm.n_succ : rec.w;
                    float* rl = lmrows + (size_t)M.row[buf][r] * 2 * V;
                    int* rn = reinterpret_cast<int*>(rl + V);
                    for (int i = lo + lane; i < hi; i += 64) {
                        const int4 e = lm.succ[i];
                        if ((unsigned)e.x < (unsigned)V) { rl[e.x] = (float)(a + (double)__int_as_float(e.y)); rn[e.x] = e.z; }
                    }
                }
                __syncthreads();
            }
        }
    };
    if constexpr (LM) {
        lmrows = lm.rows + (size_t)b * 2 * K * 2 * V;
        for (int s = tid; s < WIDE_VMAX; s += WIDE_THREADS) { M.uni_lp[s] = -INFINITY; M.uni_next[s] = 0; }
        __syncthreads();
        const int4 root = lm.states[0];
        const int lo = root.z < 0 ? 0 : root.z, hi = root.w > lm.n_succ ? lm.n_succ : root.w;
        for (int i = lo + tid; i < hi; i += WIDE_THREADS) {
            const int4 e = lm.succ[i];
            if ((unsigned)e.x < (unsigned)V) { M.uni_lp[e.x] = __int_as_float(e.y); M.uni_next[e.x] = e.z; }
        }
        __syncthreads();
        fill_rows(0, 1);
    }
    int cur = 0;
    for (int t = 0; t < Tb; ++t) {
        const int nb = L.nb;
        const int* cid = L.id[cur]; const int* clast = L.last[cur]; const int* cpar = L.par[cur];
        const double* cpb = L.pb[cur]; const double* cpnb = L.pnb[cur];

        // ---- A: the frame, an empty bitmap, the parents' positions ----
        for (int s = tid; s < V; s += WIDE_THREADS) L.frame[s] = (double)lp[(long long)t * stride_t + (long long)b * stride_b + s];
        for (int i = tid; i < nb * W; i += WIDE_THREADS) L.bitmap[i] = 0u;
        if (tid < nb) {
            int f = -1;
            for (int i = 0; i < nb; ++i) if (cid[i] == cpar[tid]) f = i;
            L.pidx[tid] = f;
        }
        __syncthreads();
        if (tid < nb && L.pidx[tid] >= 0) atomicOr(&L.bitmap[L.pidx[tid] * W + (clast[tid] >> 5)], 1u << (clast[tid] & 31));
        __syncthreads();

        // ---- B: stay candidates (:78-82, :90-96 merged, :103-106), as in beam.hip; the threshold's 2 * nb score images ----
        if (tid < nb) {
            const int j = tid;
            const double fb = L.frame[blank];
            const double npb = lse3x<FAST>(-INFINITY, cpb[j] + fb, cpnb[j] + fb);
            double npnb = -INFINITY;
            unsigned time = 2u * (unsigned)(blank * nb + j);
            const int lj = clast[j];
            if (lj >= 0 && lj != blank) {
                const double pl = L.frame[lj];
                const int i = L.pidx[j];
                const double own = cpnb[j] + pl;                                  // repeat branch (:103-106): touched second in iteration (lj, j)
                const unsigned t_own = 2u * (unsigned)(lj * nb + j) + 1u;
                time = t_own < time ? t_own : time;
                if (i >= 0) {
                    double e1 = cpb[i] + pl, e2 = cpnb[i] + pl;                   // extension of parent i by lj (:90-96): touched first in iteration (lj, i)
                    if constexpr (LM || BIAS) {                                   // with the parent's context / state: the entry's own word
                        float word = 0.0f, bonus = 0.0f;
                        if constexpr (LM) word = M.own[cur][j];
                        if constexpr (BIAS) bonus = H.own[cur][j];
                        const double w = wide_w(lm, bias, word, bonus);
                        e1 += w; e2 += w;
                    }
                    const bool rep = (clast[i] == lj);
                    if (i < j) {
                        npnb = rep ? lse2x<FAST>(npnb, e1) : lse3x<FAST>(npnb, e1, e2);
                        npnb = lse2x<FAST>(npnb, own);
                    } else {
                        npnb = lse2x<FAST>(npnb, own);
                        npnb = rep ? lse2x<FAST>(npnb, e1) : lse3x<FAST>(npnb, e1, e2);
                    }
                    const unsigned t_ext = 2u * (unsigned)(lj * nb + i);
                    time = t_ext < time ? t_ext : time;
                } else {
                    npnb = lse2x<FAST>(npnb, own);
                }
            }
            const unsigned long long img = ordered_key(lse2x<FAST>(npb, npnb));
            L.st_pb[j] = npb; L.st_pnb[j] = npnb; L.st_img[j] = img; L.st_time[j] = time;
            L.tkeys[j] = img;
        }
        // wave w takes entries w, w + 4, ..: the best log-prob among the symbols that are a candidate of their own for this entry
        for (int j = wave; j < nb; j += WIDE_THREADS / 64) {
            double best = -INFINITY;
            bool found = false;
            const int lj = clast[j];
            if constexpr (LM || BIAS) {  // the symbol of largest frame[s] + w (the lowest such s): that candidate's image, its w included
                [[maybe_unused]] const float* rl = nullptr;
                [[maybe_unused]] const BiasWord* bt = nullptr;
                if constexpr (LM) rl = lmrows + (size_t)M.row[cur][j] * 2 * V;
                if constexpr (BIAS) bt = bias.table + (size_t)H.st[cur][j] * V;      // st < S: below S V words
                auto w_of = [&](int s) {
                    float word = 0.0f, bonus = 0.0f;
                    if constexpr (LM) word = rl[s];
                    if constexpr (BIAS) bonus = bt[s].bonus;
                    return wide_w(lm, bias, word, bonus);
                };
                int bs = -1;
                for (int s = lane; s < V; s += 64) {
                    if (s == blank || s == lj || ((L.bitmap[j * W + (s >> 5)] >> (s & 31)) & 1u)) continue;
                    const double v = L.frame[s] + w_of(s);
                    if (bs < 0 || v > best) { best = v; bs = s; }
                }
                if (bs < 0) best = -INFINITY;
                const bool any = __ballot(bs >= 0) != 0ull;
                double top = best;
                for (int o = 32; o > 0; o >>= 1) top = fmax(top, __shfl_xor(top, o));
                const unsigned long long who = __ballot(bs >= 0 && best == top);
                const int s1 = __shfl(bs, who ? __ffsll((long long)who) - 1 : 0);
                if (lane == 0) {
                    unsigned long long img = 0ull;
                    if (any && s1 >= 0) {                                         // s1 < 0: every sum is NaN or none compares equal -- no bound from this entry
                        const double w = w_of(s1);
                        img = ordered_key(lse2x<FAST>(-INFINITY, wide_ext_w<FAST>(cpb[j], cpnb[j], L.frame[s1], false, w)));
                    }
                    L.tkeys[nb + j] = img;
                }
                continue;
            }
            for (int s = lane; s < V; s += 64) {
                if (s == blank || s == lj || ((L.bitmap[j * W + (s >> 5)] >> (s & 31)) & 1u)) continue;
                const double v = L.frame[s];
                best = found ? fmax(best, v) : v;
                found = true;
            }
            const bool any = __ballot(found) != 0ull;
            if (!found) best = -INFINITY;
            for (int o = 32; o > 0; o >>= 1) best = fmax(best, __shfl_xor(best, o));
            if (lane == 0)
                L.tkeys[nb + j] = any ? ordered_key(lse2x<FAST>(-INFINITY, wide_ext<FAST>(cpb[j], cpnb[j], best, false))) : 0ull;
        }
        for (int i = 2 * nb + tid; i < 2 * WIDE_KMAX; i += WIDE_THREADS) L.tkeys[i] = 0ull;       // 0 is below every real image
        if (tid == 0) { L.total = 0; L.theta = 0ull; }
        __syncthreads();

        // ---- C: theta = the K-th largest of the 2 * nb images (0 if there are fewer than K): the slot whose value v has fewer than K
        //      images above it and at least K at or above it ----
        {
            const unsigned long long mine = L.tkeys[tid];                         // 2 * WIDE_KMAX == WIDE_THREADS
            int gt = 0, ge = 0;
            for (int i = 0; i < 2 * WIDE_KMAX; ++i) { const unsigned long long x = L.tkeys[i]; gt += x > mine; ge += x >= mine; }
            if (gt < K && K <= ge) L.theta = mine;                                // every such slot holds the same value
        }
        __syncthreads();

        // every candidate of the frame, visited by all threads in step (the appends are wave-aggregated): f(valid, image, time, cand)
        auto for_each_candidate = [&](auto&& f) {
            if constexpr (LM || BIAS) {  // the same visits; entry j + 1's words are loaded while entry j's candidates are scored
                constexpr int NV = WIDE_VMAX / WIDE_THREADS;
                [[maybe_unused]] float wn[NV], bn[NV];
                auto load_words = [&](int j) {
                    if constexpr (LM) {
                        const float* rl = lmrows + (size_t)M.row[cur][j] * 2 * V;
#pragma unroll
                        for (int k = 0; k < NV; ++k) { const int s = k * WIDE_THREADS + tid; wn[k] = s < V ? rl[s] : 0.0f; }
                    }
                    if constexpr (BIAS) {
                        const BiasWord* bt = bias.table + (size_t)H.st[cur][j] * V;
#pragma unroll
                        for (int k = 0; k < NV; ++k) { const int s = k * WIDE_THREADS + tid; bn[k] = s < V ? bt[s].bonus : 0.0f; }
                    }
                };
                if (nb > 0) load_words(0);
                for (int j = 0; j < nb; ++j) {
                    const double pbj = cpb[j], pnbj = cpnb[j];
                    const int lj = clast[j];
                    [[maybe_unused]] float wc[NV], bc[NV];
#pragma unroll
                    for (int k = 0; k < NV; ++k) {
                        if constexpr (LM) wc[k] = wn[k];
                        if constexpr (BIAS) bc[k] = bn[k];
                    }
                    if (j + 1 < nb) load_words(j + 1);
#pragma unroll
                    for (int k = 0; k < NV; ++k) {
                        if (k * WIDE_THREADS >= V) break;
                        const int s = k * WIDE_THREADS + tid;
                        bool valid = s < V && s != blank;
                        if (valid) valid = !((L.bitmap[j * W + (s >> 5)] >> (s & 31)) & 1u);
                        unsigned long long img = 0ull;
                        if (valid) {
                            float word = 0.0f, bonus = 0.0f;
                            if constexpr (LM) word = wc[k];
                            if constexpr (BIAS) bonus = bc[k];
                            const double w = wide_w(lm, bias, word, bonus);
                            img = ordered_key(lse2x<FAST>(-INFINITY, wide_ext_w<FAST>(pbj, pnbj, L.frame[s], s == lj, w)));
                        }
                        f(valid, img, 2u * (unsigned)(s * nb + j), (unsigned)(j * V + s));
                    }
                }
            } else
            for (int j = 0; j < nb; ++j) {
                const double pbj = cpb[j], pnbj = cpnb[j];
                const int lj = clast[j];
                for (int s0 = 0; s0 < V; s0 += WIDE_THREADS) {
                    const int s = s0 + tid;
                    bool valid = s < V && s != blank;
                    if (valid) valid = !((L.bitmap[j * W + (s >> 5)] >> (s & 31)) & 1u);
                    unsigned long long img = 0ull;
                    if (valid) img = ordered_key(lse2x<FAST>(-INFINITY, wide_ext<FAST>(pbj, pnbj, L.frame[s], s == lj)));
                    f(valid, img, 2u * (unsigned)(s * nb + j), (unsigned)(j * V + s));
                }
            }
            const bool valid = tid < nb;
            f(valid, valid ? L.st_img[tid] : 0ull, valid ? L.st_time[tid] : 0u, WIDE_STAY | (unsigned)tid);
        };
        // list every candidate at or above the cut (hi, lo) of the key (image, ~time)
        auto collect = [&](unsigned long long chi, unsigned clo) {
            for_each_candidate([&](bool valid, unsigned long long img, unsigned time, unsigned cand) {
                const bool want = valid && (img > chi || (img == chi && ~time >= clo));
                const unsigned long long m = __ballot(want);
                if (m == 0ull) return;
                const int leader = __ffsll((long long)m) - 1;
                int base = 0;
                if (lane == leader) base = atomicAdd(&L.total, __popcll(m));
                base = __shfl(base, leader);
                const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
                if (want && pos < WIDE_CAP) { SortItem it; it.key = ~img; it.time = time; it.cand = cand; L.items[pos] = it; }
            });
        };

        bool counting = force_counting != 0;
        if (!counting) {
            collect(L.theta, 0u);
            __syncthreads();
            counting = L.total > WIDE_CAP;
        }
        if (counting) {
            // ---- D: counting selection: the key of rank K - 1, digit by digit from the top ----
            if (tid == 0) { L.cut_hi = 0ull; L.cut_lo = 0u; L.need = K; L.done = 0; L.counting += 1; }
            for (int p = 0; p < WIDE_RADIX_PASSES; ++p) {
                L.hist[tid] = 0u;                                                 // 256 bins, 256 threads
                __syncthreads();
                const unsigned long long phi = L.cut_hi;
                const unsigned plo = L.cut_lo;
                for_each_candidate([&](bool valid, unsigned long long img, unsigned time, unsigned) {
                    const unsigned lo = ~time;
                    bool match; unsigned d;
                    if (p < 8) {
                        match = (p == 0) || ((img >> (64 - 8 * p)) == (phi >> (64 - 8 * p)));
                        d = (unsigned)(img >> (56 - 8 * p)) & 255u;
                    } else {
                        const int q = p - 8;
                        match = (img == phi) && (q == 0 || (lo >> (32 - 8 * q)) == (plo >> (32 - 8 * q)));
                        d = (lo >> (24 - 8 * q)) & 255u;
                    }
                    const bool in = valid && match;
                    const unsigned long long m = __ballot(in);
                    if (m == 0ull) return;
                    const int leader = __ffsll((long long)m) - 1;
                    const unsigned d0 = (unsigned)__shfl((int)d, leader);
                    if (__ballot(in && d != d0) == 0ull) {                        // one bin for the whole wave (flat rows): one atomic
                        if (lane == leader) atomicAdd(&L.hist[d0], (unsigned)__popcll(m));
                    } else if (in) atomicAdd(&L.hist[d], 1u);
                });
                __syncthreads();
                if (tid == 0) {
                    const int need = L.need;
                    int cum = 0, d = 255;
                    for (; d >= 0; --d) { cum += (int)L.hist[d]; if (cum >= need) break; }
                    if (d < 0) {                                                  // fewer than `need` candidates in all (first pass only): keep every one
                        L.cut_hi = 0ull; L.cut_lo = 0u; L.done = 1;
                    } else {
                        if (p < 8) L.cut_hi = phi | ((unsigned long long)d << (56 - 8 * p));
                        else L.cut_lo = plo | ((unsigned)d << (24 - 8 * (p - 8)));
                        L.need = need - (cum - (int)L.hist[d]);
                        if (cum == need) L.done = 1;                              // the whole bin is kept: the cut is the bin's lower edge
                    }
                }
                __syncthreads();
                if (L.done) break;
            }
            if (tid == 0) L.total = 0;
            __syncthreads();
            collect(L.cut_hi, L.cut_lo);
            __syncthreads();
        }
        // ---- E: bitonic sort of the list ----
        int total = L.total; total = total > WIDE_CAP ? WIDE_CAP : total;         // the counting selection lists at most K <= WIDE_CAP
        int P = 2; while (P < total) P <<= 1;
        for (int i = total + tid; i < P; i += WIDE_THREADS) { SortItem it; it.key = ~0ull; it.time = 0xFFFFFFFFu; it.cand = 0xFFFFFFFFu; L.items[i] = it; }
        __syncthreads();
        bitonic_sort<WIDE_THREADS>(L.items, P, tid);
        // ---- F: new beam: the first min(K, total) items ----
        const int nxt = cur ^ 1;
        const int nnew = total < K ? total : K;
        if (tid < nnew) {
            const SortItem it = L.items[tid];
            if (it.cand & WIDE_STAY) {
                const int j = (int)(it.cand & ~WIDE_STAY);
                L.pb[nxt][tid] = L.st_pb[j]; L.pnb[nxt][tid] = L.st_pnb[j];
                L.id[nxt][tid] = cid[j]; L.last[nxt][tid] = clast[j]; L.par[nxt][tid] = cpar[j];
                if constexpr (LM) { M.st[nxt][tid] = M.st[cur][j]; M.row[nxt][tid] = M.row[cur][j]; M.own[nxt][tid] = M.own[cur][j]; M.isext[tid] = 0; }
                if constexpr (BIAS) { H.st[nxt][tid] = H.st[cur][j]; H.own[nxt][tid] = H.own[cur][j]; }
            } else {
                const int j = (int)it.cand / V, s = (int)it.cand - j * V;
                L.pb[nxt][tid] = -INFINITY;
                if constexpr (LM || BIAS) {  // the candidate's score as its key had it; its word becomes the entry's own, next[s] its state
                    [[maybe_unused]] const float* rl = nullptr;
                    [[maybe_unused]] BiasWord bw = {0, 0.0f};
                    float word = 0.0f;
                    if constexpr (BIAS) bw = bias.table[(size_t)H.st[cur][j] * V + s];      // st < S: below S V words
                    if constexpr (LM) { rl = lmrows + (size_t)M.row[cur][j] * 2 * V; word = rl[s]; }
                    const double w = wide_w(lm, bias, word, bw.bonus);
                    L.pnb[nxt][tid] = wide_ext_w<FAST>(cpb[j], cpnb[j], L.frame[s], s == clast[j], w);
                    if constexpr (LM) { M.st[nxt][tid] = reinterpret_cast<const int*>(rl + V)[s]; M.own[nxt][tid] = word; M.isext[tid] = 1; }
                    if constexpr (BIAS) {
                        H.st[nxt][tid] = ((unsigned)bw.next < (unsigned)bias.n_states) ? bw.next : 0;
                        H.own[nxt][tid] = bw.bonus;
                    }
                } else
                L.pnb[nxt][tid] = wide_ext<FAST>(cpb[j], cpnb[j], L.frame[s], s == clast[j]);
                // canonical node for (id[j], s): look up, else create
                L.id[nxt][tid] = trie_find_or_create<WIDE_SYM_BITS>(table, nodes, ws.H, ws.NN, &L.nodes, cid[j], s);
                L.last[nxt][tid] = s; L.par[nxt][tid] = cid[j];
            }
        }
        if (tid == 0) L.nb = nnew;
        __syncthreads();
        if constexpr (LM) fill_rows(nxt, nnew);
        cur = nxt;
    }
    // ---- result: row r is entry r of the final, ranked beam; L.pidx is free after the frame loop ----
    nbest_tail<WIDE_SYM_BITS, WIDE_THREADS, FAST>(nodes, ws.NN, Tb, b, tid, nbest, tok_stride, collapse, L.nb, L.id[cur], L.pb[cur], L.pnb[cur],
                                                  L.pidx, out_tokens, out_len, out_score, out_count);
    if (tid == 0 && out_counting) out_counting[b] = L.counting;
}

// the row cache behind the trie in the workspace: [B][2 beam][2][V] words
inline size_t wide_lm_ws_layout(int T, int B, int V, int beam, WideWs* ws, float** rows, char* base) {
    size_t off = trie_ws_layout<WIDE_SYM_BITS>(T, B, beam, ws, base);
    if (rows) *rows = (float*)(base + off);
    off += (size_t)B * 2 * (size_t)beam * 2 * (size_t)V * sizeof(float);
    return (off + 255) / 256 * 256;
}

static_assert(2 * WIDE_KMAX == WIDE_THREADS, "one threshold slot and one histogram bin per thread");
static_assert(WIDE_LM_BIAS_LDS_OFFSET + sizeof(WideBiasLds) <= 160 * 1024, "LDS");

// the model's checks (A7-WIDE-LM), then its kernel arguments but for the rows
inline int wide_lm_check(WideLm<true>* lm, const pgasr_unit_lm_tables* tables, int V, int blank, double lm_alpha, double lm_beta) {
    if (const int st = unit_lm::check_tables(tables, V, blank, lm_alpha, lm_beta)) return st;
    lm->states = (const int4*)tables->states; lm->succ = (const int4*)tables->succ;
    lm->n_states = tables->n_states; lm->n_succ = tables->n_succ; lm->start = tables->start; lm->order = tables->order;
    lm->alpha = lm_alpha; lm->beta = lm_beta;
    return PGASR_OK;
}

inline float** wide_rows_of() { return nullptr; }
inline float** wide_rows_of(WideBias&) { return nullptr; }
template <typename... R> inline float** wide_rows_of(WideLm<true>& lm, R&...) { return &lm.rows; }

// The host side of all entries.  The checks are pgasr_ctc_beam_search_nbest's in its order and with its status codes, lm_check()
// (the models') where that entry checks its flags, then the room for a model's row cache behind the trie; nothing touches HIP until
// every check has passed.  Then the hash table is cleared and beam_wide_kernel<TIn, FAST, LmArg...> launched.  LmArg: nothing, the
// WideLm<true> and / or the WideBias that lm_check() fills in; the model's rows are set here.
template <typename LmCheck, typename... LmArg>
int wide_search(const void* log_probs, int is_f64, long long stride_t, long long stride_b, const int32_t* lengths, int T, int B, int V,
                int beam, int blank, int flags, int nbest, int32_t* out_tokens, int tok_stride, int32_t* out_len, double* out_score,
                int32_t* out_count, int32_t* out_counting_frames, void* workspace, size_t workspace_bytes, void* stream,
                LmCheck&& lm_check, LmArg&... lm) {
    constexpr bool LM = wide_has<WideLm<true>, LmArg...>, BIAS = wide_has<WideBias, LmArg...>;
    WideWs ws;
    if (const int st = beam_check_args(log_probs, out_tokens, out_len, out_score, T, B, V, beam, blank, WIDE_VMAX, WIDE_KMAX,
                                       [&] {
                                           const bool bad = (flags & ~(1 | 32)) || nbest < 1 || nbest > beam || tok_stride < T || !out_count;
                                           return bad ? (int)PGASR_ERR_INVALID_ARG : lm_check();
                                       },
                                       workspace, workspace_bytes, &ws)) return st;
    if constexpr (LM)
        if (workspace_bytes < wide_lm_ws_layout(T, B, V, beam, &ws, wide_rows_of(lm...), (char*)workspace)) return PGASR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws.table, 0, (size_t)B * ws.H * sizeof(unsigned long long), st) != hipSuccess) return PGASR_ERR_LAUNCH;
    constexpr size_t lds_lm = LM ? WIDE_LM_LDS_OFFSET + sizeof(WideLmLds) : sizeof(WideLds);
    constexpr size_t lds = ((BIAS ? (LM ? WIDE_LM_BIAS_LDS_OFFSET : WIDE_LM_LDS_OFFSET) + sizeof(WideBiasLds) : lds_lm) + 15) / 16 * 16;
#define WIDE_LAUNCH(TIN, FAST)                                                                                                    \
    {                                                                                                                             \
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&beam_wide_kernel<TIN, FAST, LmArg...>),                          \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                          \
        PGASR_LAUNCH_KERNEL((beam_wide_kernel<TIN, FAST, LmArg...>), dim3(B), dim3(WIDE_THREADS), lds, st, (const TIN*)log_probs, \
                           stride_t, stride_b, lengths, T, V, beam, blank, flags & 1, (flags & 32) ? 1 : 0, ws, nbest, tok_stride, \
                           out_tokens, out_len, out_score, out_count, out_counting_frames, lm...);                                \
    }
    if (is_f64) WIDE_LAUNCH(double, false) else WIDE_LAUNCH(float, true)
#undef WIDE_LAUNCH
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

}  // namespace

extern "C" size_t pgasr_beam_wide_workspace_bytes(int T, int B, int V, int beam) {
    (void)V;
    if (T <= 0 || B <= 0 || beam <= 0) return 0;
    return trie_ws_layout<WIDE_SYM_BITS>(T, B, beam, nullptr, nullptr);
}

extern "C" int pgasr_ctc_beam_search_wide(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                                          const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                                          int nbest, int32_t* out_tokens, int tok_stride, int32_t* out_len, double* out_score,
                                          int32_t* out_count, int32_t* out_counting_frames,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    return wide_search(log_probs, is_f64, stride_t, stride_b, lengths, T, B, V, beam, blank, flags, nbest, out_tokens, tok_stride,
                       out_len, out_score, out_count, out_counting_frames, workspace, workspace_bytes, stream,
                       [] { return (int)PGASR_OK; });
}

extern "C" size_t pgasr_beam_wide_lm_workspace_bytes(int T, int B, int V, int beam) {
    if (T <= 0 || B <= 0 || V <= 0 || beam <= 0) return 0;
    return wide_lm_ws_layout(T, B, V, beam, nullptr, nullptr, nullptr);
}

extern "C" int pgasr_ctc_beam_search_wide_lm(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                                             const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                                             int nbest, int32_t* out_tokens, int tok_stride, int32_t* out_len, double* out_score,
                                             int32_t* out_count, int32_t* out_counting_frames,
                                             void* workspace, size_t workspace_bytes, void* stream,
                                             const pgasr_unit_lm_tables* tables, double lm_alpha, double lm_beta) {
    WideLm<true> lm;
    return wide_search(log_probs, is_f64, stride_t, stride_b, lengths, T, B, V, beam, blank, flags, nbest, out_tokens, tok_stride,
                       out_len, out_score, out_count, out_counting_frames, workspace, workspace_bytes, stream,
                       [&] {
                           return wide_lm_check(&lm, tables, V, blank, lm_alpha, lm_beta);
                       },
                       lm);
}


// A7-WIDE-BIAS: the search with a hotword automaton, with or without the unit model; without a table it is one of the two entries above
extern "C" int pgasr_ctc_beam_search_wide_bias(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                                               const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                                               int nbest, int32_t* out_tokens, int tok_stride, int32_t* out_len, double* out_score,
                                               int32_t* out_count, int32_t* out_counting_frames,
                                               void* workspace, size_t workspace_bytes, void* stream,
                                               const pgasr_unit_lm_tables* tables, double lm_alpha, double lm_beta,
                                               const void* bias_table, int bias_states, double bias_weight) {
    if (!bias_table && bias_states == 0) {
        if (!tables)
            return pgasr_ctc_beam_search_wide(log_probs, is_f64, stride_t, stride_b, lengths, T, B, V, beam, blank, flags, nbest, out_tokens,
                                              tok_stride, out_len, out_score, out_count, out_counting_frames, workspace, workspace_bytes, stream);
        return pgasr_ctc_beam_search_wide_lm(log_probs, is_f64, stride_t, stride_b, lengths, T, B, V, beam, blank, flags, nbest, out_tokens,
                                             tok_stride, out_len, out_score, out_count, out_counting_frames, workspace, workspace_bytes,
                                             stream, tables, lm_alpha, lm_beta);
    }
    WideLm<true> lm;
    WideBias bias;
    const auto check = [&] {
        if (tables)
            if (const int st = wide_lm_check(&lm, tables, V, blank, lm_alpha, lm_beta)) return st;
        if (!bias_table::usable(bias_table, bias_states, V) || !std::isfinite(bias_weight)) return (int)PGASR_ERR_INVALID_ARG;
        bias.table = (const BiasWord*)bias_table; bias.n_states = bias_states; bias.weight = bias_weight;
        return (int)PGASR_OK;
    };
    if (tables)
        return wide_search(log_probs, is_f64, stride_t, stride_b, lengths, T, B, V, beam, blank, flags, nbest, out_tokens, tok_stride,
                           out_len, out_score, out_count, out_counting_frames, workspace, workspace_bytes, stream, check, lm, bias);
    return wide_search(log_probs, is_f64, stride_t, stride_b, lengths, T, B, V, beam, blank, flags, nbest, out_tokens, tok_stride,
                       out_len, out_score, out_count, out_counting_frames, workspace, workspace_bytes, stream, check, bias);
}
