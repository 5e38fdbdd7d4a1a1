// CTC prefix beam search on gfx950 (CTCdecoder.py:41-116, Hannun's algorithm in log space).
//
// One workgroup per utterance; frames are a serial chain, the work inside a frame is parallel:
//   * beam entries are nodes of a per-utterance trie (parent id, symbol), hash-consed through a
//     (parent,symbol) -> id table in global memory so that one prefix has ONE id for the whole
//     utterance; "extension of entry i by s equals existing entry e" is then the exact integer test
//     parent(e) == id(i) && last(e) == s  (the reference merges by tuple equality, :88,:100);
//   * every (entry j, symbol s) pair is one candidate: s == blank keeps prefix j ("stay"), any other
//     s extends it unless that extension already sits in the beam, in which case its mass is added to
//     that entry's stay candidate in the reference's update order (:90-96, :103-106);
//   * candidates are ranked by a bitonic sort in LDS on (score descending, first-touch time
//     ascending) -- the reference's stable sort over dict insertion order (:110-113), whose loop nest
//     is symbol-major / rank-minor (:68,:74).
// Scores are fp64 (log-sum-exp exactly as CTCdecoder.py:31-39: max, sum of exps in argument order,
// log); this is integer/latency work, not MFMA work.
// The log-sum-exp forms, the rank key and its sort, the trie (workspace layout, find-or-create) and the N-best result tail are shared
// with the wide search (beam_wide.hip) and live in beam_core.h; the single-wave kernel further down (namespace sb) uses none of them.
#include "common.h"
#include "beam_core.h"
#include "bias_table.h"
#include "word_ngram.h"
#include <cmath>
#include <type_traits>

namespace {

using namespace beam_core;

constexpr int BEAM_KMAX = 128;
constexpr int BEAM_VMAX = 64;
constexpr int BEAM_THREADS = 256;
constexpr int BEAM_SYM_BITS = 8;                      // a trie node is parent << 8 | symbol
using BeamWs = TrieWs<BEAM_SYM_BITS>;

// Language-model fusion (LM = true; Hannun/Maas arXiv:1408.2873, the reference's "*NB* this would be a good place to include an LM
// score" at the extension step): a dense fp32 table of natural-log probabilities, table[c_1 .. c_{n-1}, s] = ln p(s | c_1 .. c_{n-1}),
// c_{n-1} the most recent symbol, contexts shorter than n-1 left-padded with blank.  Every term that enters a prefix by an extension with a
// non-blank s (:90-96) gets  w = alpha * (double)table[ctx(prefix), s] + beta  added: (p_b + p) + w, (p_nb + p) + w.  The blank update
// (:78-82) and the repeat branch that keeps the prefix (:103-106) are unchanged.
//   * an entry carries ctx = index of its last n-1 symbols (stay: inherited; extension by s: (ctx V + s) mod V^(n-1)) and lmi = the
//     table index ctx(parent prefix) V + last of its own last emission.  The merged term of entry j's stay candidate, "extension of
//     parent i by last(j)", uses parent i's context -- a function of the prefix alone, so its table word IS table[lmi_j], known without
//     waiting for pidx;
//   * candidate (j, s) reads table[ctx_j V + s]: consecutive candidates of one entry read consecutive words.  The loads of a thread's
//     first BEAM_LM_PRE candidates and of the entries' own words are issued at the top of the frame (ctx is known as soon as the new
//     beam is written) and parked in the thread's own, not yet written sort items until the candidate loop, so they are in flight
//     beside the frame's log-probs and waited for once; candidates beyond BEAM_LM_PRE * 256 load in place;
//   * w is computed in fp64 without contraction (__dmul_rn, __dadd_rn) in the exact and the fast instantiation alike.
// The arguments are an empty struct for LM = false: those instantiations carry none of this.
constexpr int BEAM_LM_PRE = 4;
constexpr long long BEAM_LM_MAX_ENTRIES = 1ll << 25;      // V^n <= 2^25 words (128 MiB): order 5 at V = 29, order 4 at V = 64
template <bool LM> struct BeamLm {};
template <> struct BeamLm<true> {
    const float* table;      // V^n words
    int ctx_mod;             // V^(n-1)
    int ctx0;                // the all-blank context (the root's)
    double alpha, beta;
};

// N-best emission (NBEST = true, pgasr_ctc_beam_search_nbest): the search is the same; only the result tail differs.  Its extra arguments ride
// behind the language model's, so the kernels without it keep their argument list (and their code: NOTES.md 0.13).
template <bool LM> struct BeamNbest : BeamLm<LM> {
    int nbest;               // rows to write, 1 <= nbest <= K
    int tok_stride;          // out_tokens is (nbest, B, tok_stride), tok_stride >= T
    int32_t* out_count;      // (B) min(nbest, entries of the final beam)
};

// Hotword (contextual phrase) biasing (BIAS = true, pgasr_ctc_beam_search_bias / _nbest_bias; include/pgasr_hip.h, A7-BIAS; the host
// builder: lm.HotwordBias).  An n-gram context is the special case next = (ctx V + s) mod V^(n-1) of a deterministic automaton; a phrase
// list compiles to such an automaton too (Aho-Corasick with weighted transitions), and the algebra is A7-LM's line for line:
//   * the table holds S * V 8-byte words {int32 next; float bonus}, word (q, s) at q V + s: consecutive candidates of one entry read
//     consecutive words;
//   * an entry carries bst = the automaton state of its prefix (stay: inherited; extension by s: next[bst V + s]) and bwi = bst(parent
//     prefix) V + last, the word of its own last emission -- the merged term of its stay candidate, known without pidx;
//   * every term that enters a prefix by a non-blank extension gets w added: wb = __dmul_rn(weight, (double)bonus), w = wb without a
//     language model and __dadd_rn(__dadd_rn(__dmul_rn(alpha, tv), beta), wb) with one; the blank update and the repeat branch are unchanged;
//   * the bonuses of a thread's first BEAM_LM_PRE candidates and of the entries' own words are gathered at the top of the frame, beside
//     the language model's, and parked in the `time` word of the thread's own, not yet written sort items;
//   * the thread that writes entry r of the new beam re-reads its winner's word for `next` -- one independent 8-byte load beside
//     trie_find_or_create, instead of 4 K V bytes of LDS --; a next outside [0, S) is taken as state 0, so every index stays below S V.
// The arguments ride behind the others in the last parameter: the BIAS = false instantiations keep their argument list and their code.
using bias_table::BiasWord;
template <bool LM, bool NBEST> using BeamTail = typename std::conditional<NBEST, BeamNbest<LM>, BeamLm<LM>>::type;
template <bool LM, bool NBEST> struct BeamBiased : BeamTail<LM, NBEST> {
    const BiasWord* btable;  // S * V words
    int bstates;             // S
    double bweight;
};

// Word fusion (WORDS = true, pgasr_ctc_beam_search_words; include/pgasr_hip.h, A7-WORDFUSE states every term; the host model:
// lm.WordFusion): the lexicon of a word n-gram model as a trie in the bias table's layout, and the model itself at every word end.
//   * an entry carries wst = the trie state of its pending word, wcx = the entry indices of its last 1 .. order-1 completed words as
//     contexts (a unigram's is its word id, an n-gram's n_words + slot, -1 where the model does not store it; word_lm.hip's step 4),
//     own = the w of its own last emission -- inherited on a stay; the merged term of its stay candidate, known without pidx -- and
//     dlm = the bonus the delimiter would get, alpha score(hist, word of wst) + beta (+ oov_penalty at a non-terminal node);
//   * candidate (j, s) reads dlm[j] for the delimiter and one trie word otherwise (consecutive candidates of one entry read consecutive
//     words; the first BEAM_LM_PRE per thread are gathered at the top of the frame and parked like the bias' bonuses);
//   * the thread that writes an extension winner does the model's work: one trie word and, for a symbol, the back-off query of the
//     new node's word under the inherited contexts -- at most order-1 probes that do not depend on each other (word_lm.hip's step 5) --
//     or, for the delimiter, the same probes to advance the contexts.  O(beam) probes per frame, never O(beam V);
//   * finalisation: every final entry gets fin = its dlm (and alpha score(hist', </s>) with eos); a bitonic sort of the at most 128
//     entries on (lse + fin, search rank) puts the beam in its final order in front of nbest_tail.
// N-best form only, no dense table and no bias beside it; the arguments ride in the last parameter.
using word_ngram::NgramSlot;
constexpr int BEAM_WCTX = word_ngram::WL_MAX_ORDER - 1;      // contexts per entry
constexpr size_t BEAM_WORDS_ENTRY_BYTES = 2 * (2 * sizeof(double) + (1 + BEAM_WCTX) * sizeof(int));      // own, dlm, wst, wcx, double-buffered: 72
struct BeamWords : BeamNbest<false> {
    const BiasWord* trie;    // S * V words
    const int32_t* node_word;      // S
    const NgramSlot* slots; const float* uni_logp; const float* uni_bow;
    int tstates, order, n_words, ngram_cap, delim, finalize, eos;
    double alpha, beta;
};

// the slots of (wcx[m], word), m < order-1, as independent probes: hit[m] the slot's content, at[m] its index or -1
__device__ __forceinline__ void words_probe(const BeamWords& a, const int (&cx)[BEAM_WCTX], int word, int (&at)[BEAM_WCTX], NgramSlot (&hit)[BEAM_WCTX]) {
#pragma unroll
    for (int m = 0; m < BEAM_WCTX; ++m) {
        at[m] = -1;
        hit[m] = NgramSlot{-1, 0, 0.0f, 0.0f};
        if (m < a.order - 1 && cx[m] >= 0) at[m] = word_ngram::ngram_find(a.slots, a.ngram_cap, cx[m], word, hit[m]);
    }
}
// score(hist, word): from 0.0 the back-off weights of the stored contexts, longest first, until one holds the word; then its logp
__device__ __forceinline__ double words_score(const BeamWords& a, const int (&cx)[BEAM_WCTX], int word) {
    int at[BEAM_WCTX]; NgramSlot hit[BEAM_WCTX];
    words_probe(a, cx, word, at, hit);
    double acc = 0.0;
    bool found = false;
#pragma unroll
    for (int m = BEAM_WCTX - 1; m >= 0; --m) {
        if (m < a.order - 1 && cx[m] >= 0 && !found) {
            if (at[m] >= 0) { acc += (double)hit[m].logp; found = true; }
            else acc += (double)(cx[m] < a.n_words ? a.uni_bow[cx[m]] : a.slots[cx[m] - a.n_words].bow);
        }
    }
    if (!found) acc += (double)a.uni_logp[word];
    return acc;
}
// hist + word: the context of m + 1 words is the n-gram (context of m words, word)
__device__ __forceinline__ void words_advance(const BeamWords& a, int (&cx)[BEAM_WCTX], int word) {
    int at[BEAM_WCTX]; NgramSlot hit[BEAM_WCTX];
    words_probe(a, cx, word, at, hit);
#pragma unroll
    for (int m = BEAM_WCTX - 1; m >= 1; --m) cx[m] = (m < a.order - 1 && at[m - 1] >= 0) ? a.n_words + at[m - 1] : -1;
    cx[0] = a.order > 1 ? word : -1;
}
__device__ __forceinline__ int words_word(const BeamWords& a, int q) {
    const int w = a.node_word[q];
    return ((unsigned)w < (unsigned)a.n_words) ? w : word_ngram::WL_UNK;
}
// the bonus of the delimiter behind trie state q != 0
__device__ __forceinline__ double words_dbonus(const BeamWords& a, int V, const int (&cx)[BEAM_WCTX], int q) {
    const int word = words_word(a, q);
    double w = __dadd_rn(__dmul_rn(a.alpha, words_score(a, cx, word)), a.beta);
    if (word == word_ngram::WL_UNK && q != a.tstates - 1) w = __dadd_rn(w, (double)a.trie[q * V + a.delim].bonus);
    return w;
}

template <typename TIn, bool FAST, bool LM, bool NBEST = false, bool BIAS = false, bool WORDS = false>
__global__ __launch_bounds__(BEAM_THREADS) void beam_search_kernel(
    const TIn* __restrict__ lp, long long stride_t, long long stride_b, const int32_t* __restrict__ lengths,
    int T, int V, int K, int blank, int collapse, BeamWs ws, int32_t* __restrict__ out_tokens, int32_t* __restrict__ out_len,
    double* __restrict__ out_score,
    const typename std::conditional<WORDS, BeamWords, typename std::conditional<BIAS, BeamBiased<LM, NBEST>, BeamTail<LM, NBEST>>::type>::type lm) {
    static_assert(!WORDS || (NBEST && !LM && !BIAS), "word fusion: the N-best form, no dense table, no bias");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    int Tb = lengths ? lengths[b] : T; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);

    int P = 1; while (P < K * V) P <<= 1;                 // sort size
    // LDS carve-up (all offsets multiples of 16)
    SortItem* items = reinterpret_cast<SortItem*>(smem);                                   // P
    double* c_pb = reinterpret_cast<double*>(smem + (size_t)P * sizeof(SortItem));          // K*V
    double* c_pnb = c_pb + (size_t)K * V;                                                   // K*V
    double* pb = c_pnb + (size_t)K * V;        // [2][K]
    double* pnb = pb + 2 * K;                  // [2][K]
    double* frame = pnb + 2 * K;               // V log-probs of the current frame
    int* id = reinterpret_cast<int*>(frame + BEAM_VMAX);   // [2][K]
    int* last = id + 2 * K;                    // [2][K]
    int* par = last + 2 * K;                   // [2][K]
    int* pidx = par + 2 * K;                   // [K]
    int* s_ctl = pidx + K;                     // [4]: nb, node counter
    int* ctx = s_ctl + 4;                      // LM only: [2][K] context index
    int* lmi = ctx + 2 * K;                    // LM only: [2][K] table index of the entry's own last emission
    float* ptv = reinterpret_cast<float*>(lmi + 2 * K);    // LM only: [K] table[lmi] of the current beam
    int* bst = s_ctl + 4 + (LM ? 5 * K : 0);   // BIAS only: [2][K] automaton state of the entry's prefix
    int* bwi = bst + 2 * K;                    // BIAS only: [2][K] table index of the entry's own last emission
    float* pbv = reinterpret_cast<float*>(bwi + 2 * K);    // BIAS only: [K] bonus of table[bwi] of the current beam
    // WORDS only, from the next multiple of 8 bytes on: own, dlm [2][K] fp64; wst [2][K]; wcx [2][K][BEAM_WCTX]
    double* wown = reinterpret_cast<double*>(smem + ((reinterpret_cast<unsigned char*>(s_ctl + 4) - smem + 7) & ~(ptrdiff_t)7));
    double* wdlm = wown + 2 * K;
    int* wst = reinterpret_cast<int*>(wdlm + 2 * K);
    int* wcx = wst + 2 * K;
    short* cb = reinterpret_cast<short*>(WORDS ? wcx + 2 * K * BEAM_WCTX : (BIAS ? bst + 5 * K : (LM ? s_ctl + 4 + 5 * K : s_ctl + 4)));       // [K][V] child-in-beam table
#define s_nb s_ctl[0]
#define s_nodes s_ctl[1]

    unsigned long long* table = ws.table + (size_t)b * ws.H;
    unsigned* nodes = ws.nodes + (size_t)b * ws.NN;

    if (tid == 0) {
        s_nb = 1; s_nodes = 1;
        id[0] = 0; last[0] = -1; par[0] = -1; pb[0] = 0.0; pnb[0] = -INFINITY;
        nodes[0] = 0xFFFFFFFFu;
        if constexpr (LM) { ctx[0] = lm.ctx0; lmi[0] = 0; }      // the root has no emission of its own: lmi is never used (last < 0)
        if constexpr (BIAS) { bst[0] = 0; bwi[0] = 0; }          // state 0 is the automaton's root; bwi likewise unused while last < 0
        if constexpr (WORDS) {                                   // the empty prefix: the trie's root, a history of <s>
            wst[0] = 0; wown[0] = 0.0; wdlm[0] = 0.0;
            int e = word_ngram::WL_BOS;
            for (int m = 0; m < BEAM_WCTX; ++m) {
                if (m > 0 && e >= 0) { NgramSlot hit; const int at = word_ngram::ngram_find(lm.slots, lm.ngram_cap, e, word_ngram::WL_BOS, hit); e = at < 0 ? -1 : lm.n_words + at; }
                wcx[m] = m < lm.order - 1 ? e : -1;
            }
        }
    }
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < Tb; ++t) {
        const int nb = s_nb;
        const int* cid = id + cur * K; const int* clast = last + cur * K; const int* cpar = par + cur * K;
        const double* cpb = pb + cur * K; const double* cpnb = pnb + cur * K;
        [[maybe_unused]] const int* cctx = ctx + cur * K;
        [[maybe_unused]] float lmv[BEAM_LM_PRE], lmp = 0.0f;
        if constexpr (LM) {      // issue the gathers first: nothing below depends on them until the candidate loop
#pragma unroll
            for (int k = 0; k < BEAM_LM_PRE; ++k) {
                const int c = tid + k * BEAM_THREADS;
                lmv[k] = 0.0f;
                if (c < nb * V) { const int j = c / V, s = c % V; if (s != blank) lmv[k] = lm.table[cctx[j] * V + s]; }
            }
            if (tid < nb && last[cur * K + tid] >= 0) lmp = lm.table[lmi[cur * K + tid]];
        }
        [[maybe_unused]] const int* cbst = bst + cur * K;
        [[maybe_unused]] float bv[BEAM_LM_PRE], bvp = 0.0f;
        if constexpr (BIAS) {    // the bonuses likewise
#pragma unroll
            for (int k = 0; k < BEAM_LM_PRE; ++k) {
                const int c = tid + k * BEAM_THREADS;
                bv[k] = 0.0f;
                if (c < nb * V) { const int j = c / V, s = c % V; if (s != blank) bv[k] = lm.btable[cbst[j] * V + s].bonus; }
            }
            if (tid < nb && last[cur * K + tid] >= 0) bvp = lm.btable[bwi[cur * K + tid]].bonus;
        }
        [[maybe_unused]] const int* cwst = wst + cur * K;
        [[maybe_unused]] float wv[BEAM_LM_PRE];
        if constexpr (WORDS) {   // the trie words likewise; the delimiter's term is dlm, already in LDS
#pragma unroll
            for (int k = 0; k < BEAM_LM_PRE; ++k) {
                const int c = tid + k * BEAM_THREADS;
                wv[k] = 0.0f;
                if (c < nb * V) { const int j = c / V, s = c % V; if (s != blank && s != lm.delim) wv[k] = lm.trie[cwst[j] * V + s].bonus; }
            }
        }
        if (tid < V) frame[tid] = (double)lp[(long long)t * stride_t + (long long)b * stride_b + tid];
        for (int i = tid; i < nb * V; i += BEAM_THREADS) cb[i] = -1;
        if (tid < nb) {
            int f = -1;
            for (int i = 0; i < nb; ++i) if (cid[i] == cpar[tid]) f = i;
            pidx[tid] = f;
        }
        if constexpr (LM) {      // park them: items[c] is this thread's own word until it writes candidate c
#pragma unroll
            for (int k = 0; k < BEAM_LM_PRE; ++k) {
                const int c = tid + k * BEAM_THREADS;
                if (c < P) items[c].cand = __float_as_uint(lmv[k]);
            }
            if (tid < nb) ptv[tid] = lmp;
        }
        if constexpr (BIAS) {
#pragma unroll
            for (int k = 0; k < BEAM_LM_PRE; ++k) {
                const int c = tid + k * BEAM_THREADS;
                if (c < P) items[c].time = __float_as_uint(bv[k]);
            }
            if (tid < nb) pbv[tid] = bvp;
        }
        if constexpr (WORDS) {
#pragma unroll
            for (int k = 0; k < BEAM_LM_PRE; ++k) {
                const int c = tid + k * BEAM_THREADS;
                if (c < P) items[c].time = __float_as_uint(wv[k]);
            }
        }
        __syncthreads();
        if (tid < nb && pidx[tid] >= 0) cb[pidx[tid] * V + clast[tid]] = (short)tid;
        __syncthreads();
        // ---- candidates: c = j*V + s ----
        const int C = nb * V;
        for (int c = tid; c < P; c += BEAM_THREADS) {
            SortItem it; it.key = ~0ull; it.time = 0xFFFFFFFFu; it.cand = 0xFFFFFFFFu;   // padding sorts last
            if (c < C) {
                const int j = c / V, s = c % V;
                double npb = -INFINITY, npnb = -INFINITY;
                unsigned time = 0xFFFFFFFFu;
                bool alive = true;
                if (s == blank) {
                    // prefix j unchanged.  blank update (:78-82)
                    npb = lse3x<FAST>(-INFINITY, cpb[j] + frame[blank], cpnb[j] + frame[blank]);
                    time = (unsigned)(blank * nb + j);
                    const int lj = clast[j];
                    if (lj >= 0 && lj != blank) {
                        const double pl = frame[lj];
                        const int i = pidx[j];
                        // two possible non-blank updates, applied in loop order (symbol lj, rank i vs j)
                        const double own = cpnb[j] + pl;                              // repeat branch (:103-106)
                        if (i >= 0) {
                            double e1 = cpb[i] + pl, e2 = cpnb[i] + pl;               // extension of parent i by lj (:90-96)
                            if constexpr (WORDS) {
                                const double w = wown[cur * K + j];
                                e1 += w; e2 += w;
                            } else
                            if constexpr (BIAS) {
                                const double wb = __dmul_rn(lm.bweight, (double)pbv[j]);
                                double w = wb;
                                if constexpr (LM) w = __dadd_rn(__dadd_rn(__dmul_rn(lm.alpha, (double)ptv[j]), lm.beta), wb);
                                e1 += w; e2 += w;
                            } else
                            if constexpr (LM) {
                                const double w = __dadd_rn(__dmul_rn(lm.alpha, (double)ptv[j]), lm.beta);
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
                            const unsigned tt = (unsigned)(lj * nb + (i < j ? i : j));
                            time = tt < time ? tt : time;
                        } else {
                            npnb = lse2x<FAST>(npnb, own);
                            const unsigned tt = (unsigned)(lj * nb + j);
                            time = tt < time ? tt : time;
                        }
                    }
                } else if (cb[j * V + s] >= 0) {
                    alive = false;          // merged into an existing entry's stay candidate
                } else {
                    const double ps = frame[s];
                    if constexpr (WORDS) {
                        double w;
                        if (s == lm.delim) w = wdlm[cur * K + j];
                        else w = (double)((c < BEAM_LM_PRE * BEAM_THREADS) ? __uint_as_float(items[c].time) : lm.trie[cwst[j] * V + s].bonus);
                        const double eb = (cpb[j] + ps) + w, en = (cpnb[j] + ps) + w;
                        npnb = (s != clast[j]) ? lse3x<FAST>(-INFINITY, eb, en) : lse2x<FAST>(-INFINITY, eb);
                    } else
                    if constexpr (BIAS) {
                        const bool pre = c < BEAM_LM_PRE * BEAM_THREADS;
                        const float bon = pre ? __uint_as_float(items[c].time) : lm.btable[cbst[j] * V + s].bonus;
                        const double wb = __dmul_rn(lm.bweight, (double)bon);
                        double w = wb;
                        if constexpr (LM) {
                            const float tv = pre ? __uint_as_float(items[c].cand) : lm.table[cctx[j] * V + s];
                            w = __dadd_rn(__dadd_rn(__dmul_rn(lm.alpha, (double)tv), lm.beta), wb);
                        }
                        const double eb = (cpb[j] + ps) + w, en = (cpnb[j] + ps) + w;
                        npnb = (s != clast[j]) ? lse3x<FAST>(-INFINITY, eb, en) : lse2x<FAST>(-INFINITY, eb);
                    } else
                    if constexpr (LM) {
                        const float tv = (c < BEAM_LM_PRE * BEAM_THREADS) ? __uint_as_float(items[c].cand) : lm.table[cctx[j] * V + s];
                        const double w = __dadd_rn(__dmul_rn(lm.alpha, (double)tv), lm.beta);
                        const double eb = (cpb[j] + ps) + w, en = (cpnb[j] + ps) + w;
                        npnb = (s != clast[j]) ? lse3x<FAST>(-INFINITY, eb, en) : lse2x<FAST>(-INFINITY, eb);
                    } else
                    npnb = (s != clast[j]) ? lse3x<FAST>(-INFINITY, cpb[j] + ps, cpnb[j] + ps) : lse2x<FAST>(-INFINITY, cpb[j] + ps);
                    time = (unsigned)(s * nb + j);
                }
                if (alive) {
                    c_pb[c] = npb; c_pnb[c] = npnb;
                    it.key = ~ordered_key(lse2x<FAST>(npb, npnb));
                    it.time = time; it.cand = (unsigned)c;
                }
            }
            items[c] = it;
        }
        __syncthreads();
        bitonic_sort<BEAM_THREADS>(items, P, tid);
        // ---- new beam ----
        const int nxt = cur ^ 1;
        int* nid = id + nxt * K; int* nlast = last + nxt * K; int* npar = par + nxt * K;
        double* nbpb = pb + nxt * K; double* nbpnb = pnb + nxt * K;
        if (tid < K) {
            const SortItem it = items[tid];
            if (it.cand != 0xFFFFFFFFu) {
                const int c = (int)it.cand, j = c / V, s = c % V;
                nbpb[tid] = c_pb[c]; nbpnb[tid] = c_pnb[c];
                if constexpr (LM) {
                    const int e = cctx[j] * V + s;
                    ctx[nxt * K + tid] = (s == blank) ? cctx[j] : e % lm.ctx_mod;
                    lmi[nxt * K + tid] = (s == blank) ? lmi[cur * K + j] : e;
                }
                if constexpr (BIAS) {
                    const int e = cbst[j] * V + s;                          // cbst[j] < S: below S V words
                    int nx = cbst[j];
                    if (s != blank) { nx = lm.btable[e].next; nx = ((unsigned)nx < (unsigned)lm.bstates) ? nx : 0; }
                    bst[nxt * K + tid] = nx;
                    bwi[nxt * K + tid] = (s == blank) ? bwi[cur * K + j] : e;
                }
                if constexpr (WORDS) {
                    const int q = cwst[j];                                  // < S: below S V words
                    int nq = q;
                    double nown = wown[cur * K + j], ndlm = wdlm[cur * K + j];
                    int cx[BEAM_WCTX];
#pragma unroll
                    for (int m = 0; m < BEAM_WCTX; ++m) cx[m] = wcx[(cur * K + j) * BEAM_WCTX + m];
                    if (s != blank) {
                        if (s == lm.delim) {                                // a word end (q != 0), or a delimiter behind none
                            nown = ndlm;                                    // dlm is 0.0 at the root
                            if (q != 0) { words_advance(lm, cx, words_word(lm, q)); nq = 0; ndlm = 0.0; }
                        } else {
                            const BiasWord tw = lm.trie[q * V + s];
                            nq = ((unsigned)tw.next < (unsigned)lm.tstates) ? tw.next : 0;
                            nown = (double)tw.bonus;
                            ndlm = nq != 0 ? words_dbonus(lm, V, cx, nq) : 0.0;
                        }
                    }
                    wst[nxt * K + tid] = nq; wown[nxt * K + tid] = nown; wdlm[nxt * K + tid] = ndlm;
#pragma unroll
                    for (int m = 0; m < BEAM_WCTX; ++m) wcx[(nxt * K + tid) * BEAM_WCTX + m] = cx[m];
                }
                if (s == blank) { nid[tid] = cid[j]; nlast[tid] = clast[j]; npar[tid] = cpar[j]; }
                else {
                    // canonical node for (id[j], s): look up, else create
                    nid[tid] = trie_find_or_create<BEAM_SYM_BITS>(table, nodes, ws.H, ws.NN, &s_nodes, cid[j], s);
                    nlast[tid] = s; npar[tid] = cid[j];
                }
            }
        }
        if (tid == 0) {
            int cnt = 0;
            for (int r = 0; r < K && r < P; ++r) if (items[r].cand != 0xFFFFFFFFu) ++cnt;
            s_nb = cnt;
        }
        __syncthreads();
        cur = nxt;
    }
    if constexpr (WORDS) {
        if (lm.finalize) {
            // ---- finalisation: total = lse + fin per final entry, the beam ranked again on (total, search rank); items, c_pb, c_pnb are free ----
            const int nb = s_nb, nxt = cur ^ 1;
            double* tot = c_pb;            // [nb] by search rank
            double* stot = c_pnb;          // [nb] by final rank
            if (tid < nb) {
                const int e = cur * K + tid, q = wst[e];
                int cx[BEAM_WCTX];
#pragma unroll
                for (int m = 0; m < BEAM_WCTX; ++m) cx[m] = wcx[e * BEAM_WCTX + m];
                double fin = 0.0;
                if (q != 0) fin = wdlm[e];
                if (lm.eos) {
                    if (q != 0) words_advance(lm, cx, words_word(lm, q));
                    fin = __dadd_rn(fin, __dmul_rn(lm.alpha, words_score(lm, cx, word_ngram::WL_EOS)));
                }
                tot[tid] = lse2x<FAST>(pb[e], pnb[e]) + fin;
            }
            __syncthreads();
            int Pf = 1; while (Pf < nb) Pf <<= 1;          // <= the frame loop's P: inside items
            for (int i = tid; i < Pf; i += BEAM_THREADS) {
                SortItem it; it.key = ~0ull; it.time = 0xFFFFFFFFu; it.cand = 0xFFFFFFFFu;
                if (i < nb) { it.key = ~ordered_key(tot[i]); it.time = (unsigned)i; it.cand = (unsigned)i; }
                items[i] = it;
            }
            __syncthreads();
            bitonic_sort<BEAM_THREADS>(items, Pf, tid);
            if (tid < nb) {
                const int r = cur * K + (int)items[tid].cand;
                id[nxt * K + tid] = id[r]; pb[nxt * K + tid] = pb[r]; pnb[nxt * K + tid] = pnb[r];
                stot[tid] = tot[items[tid].cand];
            }
            __syncthreads();
            nbest_tail<BEAM_SYM_BITS, BEAM_THREADS, FAST>(nodes, ws.NN, Tb, b, tid, lm.nbest, lm.tok_stride, collapse, nb, id + nxt * K, pb + nxt * K,
                                                          pnb + nxt * K, pidx, out_tokens, out_len, out_score, lm.out_count);
            if (tid < lm.nbest && tid < nb) out_score[(size_t)tid * gridDim.x + b] = -stot[tid];      // the thread that wrote -lse there
            return;
        }
    }
    if constexpr (NBEST) {
        // ---- N-best result: row r is entry r of the final, ranked beam; pidx is free after the frame loop ----
        nbest_tail<BEAM_SYM_BITS, BEAM_THREADS, FAST>(nodes, ws.NN, Tb, b, tid, lm.nbest, lm.tok_stride, collapse, s_nb, id + cur * K, pb + cur * K,
                                                      pnb + cur * K, pidx, out_tokens, out_len, out_score, lm.out_count);
        return;
    }
    // ---- result: walk the best entry's ancestors ----
    if (tid == 0) {
        const int best = id[cur * K];
        int n = 0;
        for (int v = best; v > 0; v = (int)(nodes[v] >> BEAM_SYM_BITS)) ++n;
        out_len[b] = n;
        int32_t* o = out_tokens + (size_t)b * T;
        int k = n - 1;
        for (int v = best; v > 0; v = (int)(nodes[v] >> BEAM_SYM_BITS)) o[k--] = (int32_t)(nodes[v] & BeamWs::SYM_MASK);
        if (collapse) {      // collapse_fn (CTCdecoder.py:119-131): adjacent duplicates removed
            int w = 0;
            for (int i = 0; i < n; ++i) if (i == 0 || o[i] != o[i - 1]) { const int32_t x = o[i]; o[w++] = x; }
            for (int i = w; i < n; ++i) o[i] = 0;
            out_len[b] = w;
        }
        out_score[b] = -lse2x<FAST>(pb[cur * K], pnb[cur * K]);
    }
}

#undef s_nb
#undef s_nodes

inline size_t beam_lds_bytes(int K, int V, bool lm, bool bias = false, bool words = false) {
    int P = 1; while (P < K * V) P <<= 1;
    size_t n = (size_t)P * sizeof(SortItem);
    n += (size_t)2 * K * V * sizeof(double);          // c_pb, c_pnb
    n += (size_t)4 * K * sizeof(double);              // pb, pnb double-buffered
    n += (size_t)BEAM_VMAX * sizeof(double);          // frame
    n += (size_t)(6 * K + K + 4) * sizeof(int);       // id,last,par (x2), pidx, control words
    if (lm) n += (size_t)(5 * K) * sizeof(int);       // ctx, lmi (x2), ptv
    if (bias) n += (size_t)(5 * K) * sizeof(int);     // bst, bwi (x2), pbv: at most 2560 bytes, and the largest shape without them is 150032
    if (words) n += (size_t)K * BEAM_WORDS_ENTRY_BYTES + 8;       // own, dlm, wst, wcx (x2) behind an 8-byte boundary: 9224 bytes at beam 128, 159256 in all at 128 x 32
    n += (size_t)K * V * sizeof(short);               // cb
    return (n + 15) / 16 * 16;
}


// =====================================================================================================================
// Small-beam search for the training path (reward hypothesis of policy_grad.py:6-8 inside the train step):
// fp32 device log-probs, beam <= 16, V <= 64, T * beam <= 24576 and T <= 4096.  ONE WAVE per utterance, no workgroup barrier, no
// LDS sort: the generic kernel above spends 24 us per frame in 45 LDS bitonic passes with barriers (24 ms for T = 1000);
// a frame here is ~800 wave instructions.
//
//   lane = (q = lane / 16, j = lane % 16): entry j's state (p_b, p_nb, total, node id, last symbol, parent id) is
//     replicated in the four 16-lane rows; lane (q, j) owns the candidates (entry j, symbol SPL q + i), i < SPL = 8 (V <= 32; 16 for
//     V <= 64, round 5: same kernel, twice the candidates per lane, a 63-exchange network; 4.5-4.9 ms for 32 x T = 1000 at beam 16 against
//     3.2-4.1 at V <= 32 and 45 ms on the generic kernel, tools/dev/r5_beam_v64.py) -- the slot
//     of the blank symbol holds entry j's "stay" candidate (prefix unchanged).
//   scores: the same algebra as CTCdecoder.py:74-106 with the per-entry total lse(p_b, p_nb) factored out (an
//     extension is total_j + log p(s), or p_b_j + log p(s) for a repeat of the last symbol; a stay collects blank,
//     repeat and -- when entry j's parent i is in the beam -- the merged extension of i by last(j)); fp64 carries,
//     fp32 exp/log on differences (like the generic fp32 path: ~1e-7 relative, so exact ties aside both rank alike).
//   prefix identity: hash-consed trie in LDS.  A node's id IS its slot in one 32768-word open-addressing table whose
//     word holds (parent id << 8 | symbol) + 1 -- table and node store in one array -- and, in bits 25..29, the beam
//     position + 1 of the entry that currently carries that prefix: "is my parent in the beam, where?" is one LDS
//     read, "which of my children are in the beam" one LDS atomic-or per entry.
//   top-K: every candidate becomes a unique 64-bit key = order-preserving image of (score - best total) with the low
//     17 mantissa bits replaced by [first-touch order of the reference's loop nest (:68,:74), slot, entry]: descending
//     key order IS the reference's stable sort (:110-113).  Each lane sorts its 8 keys with a 19-exchange network in
//     registers; K rounds of (row all-reduce max by DPP rotations on the high words, 4 readlanes, rarely a second pass
//     on the low words) pop the winners in rank order (a pop shifts the winner lane's register list).
//   frames are staged 32 at a time through LDS, two chunks ahead in registers, so no load is ever waited for.
// =====================================================================================================================
#ifdef PGASR_BEAM_DIAG
__device__ unsigned long long beam_diag_counters[4];      // frames, frames redone by the exact rounds, hash-table probes, longest probe chain
#endif
#ifndef PGASR_BEAM_UNROLL
#define PGASR_BEAM_UNROLL 1
#endif
namespace sb {
constexpr int K_MAX = 16, V_MAX = 64, H = 32768, CH = 32;     // template parameter SPL = symbols per lane: 8 (V <= 32) or 16 (V <= 64)
constexpr long long MAX_NODES = 24576;               // T * beam: load factor of the table <= 0.75
constexpr int MAX_TOKENS = 4096;                     // a hypothesis has at most T tokens and is staged in the 8 KB `frames` region (beam < 6 would admit longer T)
constexpr unsigned ROOT = 0x8000u, NONE = 0xFFFFu, BAD_ID = 0x0FFFFFFFu;
constexpr unsigned KEYMASK = 0x01FFFFFFu;
constexpr size_t LDS_TABLE = (size_t)H * 4;          // 128 KB
constexpr size_t lds_frames(int spl) { return (size_t)2 * CH * (4 * spl) * 4; }      // two chunks of CH frames, 4 * SPL symbols each
constexpr size_t LDS_MM = 128;
constexpr size_t lds_bytes(int spl) { return LDS_TABLE + lds_frames(spl) + LDS_MM; }

__device__ __forceinline__ double lse2f(double a, double b) {
    // 1 + e^x with x <= 0 is in [1, 2]: the bare v_exp_f32 / v_log_f32 (base 2) need none of the library forms' range fix-ups
    const double m = fmax(a, b), n = fmin(a, b);
    const float e = __builtin_amdgcn_exp2f(1.4426950408889634f * (float)(n - m));
    const double r = m + (double)(0.6931471805599453f * __builtin_amdgcn_logf(1.0f + e));
    return (m == -INFINITY) ? -INFINITY : r;
}

template <int CTRL> __device__ __forceinline__ unsigned dpp_u32(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
// max over the 16 lanes of every row, left in all of them (row_ror:8,4,2,1)
__device__ __forceinline__ unsigned row_allmax(unsigned v) {
    unsigned x = dpp_u32<0x128>(v); v = v > x ? v : x;
    x = dpp_u32<0x124>(v); v = v > x ? v : x;
    x = dpp_u32<0x122>(v); v = v > x ? v : x;
    x = dpp_u32<0x121>(v); v = v > x ? v : x;
    return v;
}
// the same over all 64 lanes with VALU operations only (gfx950's row swaps): nothing goes through the scalar unit, so the
// result can feed the next vector instruction of a round's chain directly
__device__ __forceinline__ unsigned wave_allmax_valu(unsigned v) {
    v = row_allmax(v);
    auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false);      // rows (0,1) and (2,3) meet
    v = a[0] > a[1] ? a[0] : a[1];
    auto c = __builtin_amdgcn_permlane32_swap(v, v, false, false);      // the two halves meet
    return c[0] > c[1] ? c[0] : c[1];
}
// the same as ONE scalar: row maxima by DPP rotations, rows 1 / 3 take row 0's / 2's lane 15 (row_bcast:15), rows 2, 3 take lane 31 (row_bcast:31),
// lane 63 holds the maximum and v_readlane hands it to the scalar unit -- seven dependent instructions instead of ten, the compare that follows
// takes a scalar operand.  Measured in the pop rounds and NOT used there (round 5): flat 3.19 -> 3.37 ms, peaked 3.68 -> 3.83 at beam 16 -- the trip
// through the scalar unit costs the chain more than three vector instructions save.  Kept for the diagnostic record only.
template <int CTRL, int RM> __device__ __forceinline__ unsigned dpp_rows(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, RM, 0xF, false);
}
__device__ __forceinline__ unsigned wave_allmax_scalar(unsigned v) {
    v = row_allmax(v);
    // the two cross-row steps as fused v_max_u32_dpp (the builtin gives v_mov_b32_dpp + v_max_u32: a row mask other than 0xf is not folded);
    // rows outside the mask keep their value; the wait states a DPP read behind a vector write needs are written out
    asm volatile("s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1" : "+v"(v));
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// row 0's value of v in all four rows
__device__ __forceinline__ unsigned row0_to_all(unsigned v) {
    auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    auto c = __builtin_amdgcn_permlane32_swap(a[0], a[0], false, false);
    return c[0];
}
__device__ __forceinline__ unsigned wave_allmax(unsigned v) {
    v = row_allmax(v);
    const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)v, 0), b = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
    const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)v, 32), d = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
    const unsigned ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}

// one 64-bit compare and four 32-bit selects per exchange (written as selects of 64-bit values the compiler emits a second compare, v_cmp_gt_u64
// beside v_cmp_lt_u64, for the other output: 19 more half-rate instructions per frame)
#define SB_CE(a, b) { const unsigned long long x_ = k[a], y_ = k[b]; const bool sw_ = x_ < y_;                                  \
                      const unsigned xl_ = (unsigned)x_, xh_ = (unsigned)(x_ >> 32), yl_ = (unsigned)y_, yh_ = (unsigned)(y_ >> 32);   \
                      k[a] = ((unsigned long long)(sw_ ? yh_ : xh_) << 32) | (sw_ ? yl_ : xl_);                                    \
                      k[b] = ((unsigned long long)(sw_ ? xh_ : yh_) << 32) | (sw_ ? xl_ : yl_); }

// N-best tail (NBEST = true, the "fast" bit of pgasr_ctc_beam_search_nbest): the search is the same; the list's arguments take the
// place of the last argument, so the NBEST = false instantiations -- what the train step runs -- keep their argument list and code.
struct SmallNbest {
    double* out_score;       // (nbest, B)
    int32_t* out_count;      // (B) min(nbest, entries of the final beam)
    int nbest;               // rows to write, 1 <= nbest <= K
    int tok_stride;          // out_tokens is (nbest, B, tok_stride), tok_stride >= T
};

// Language-model fusion (LM = true, flags bit 4 of pgasr_ctc_beam_search_lm / _nbest): the algebra of beam_search_kernel<.., LM = true> above
// (tests/beam_lm_ref.py states it in plain Python) on this kernel's lane layout.
//   * an entry carries, replicated per row like pb / pnb / tot: ctx = the index of its last n-1 symbols (the root: ctx0) and lmp = the table
//     word of its own last emission, table[ctx(parent prefix) V + last].  (The index of that word, the workgroup kernel's lmi, is only a
//     temporary here: that kernel reloads the word every frame, this one keeps it.)
//   * lane (q, j) gathers table[ctx_j V + SPL q + i], i < SPL -- consecutive words -- at the top of the frame, where j < nb, the symbol is
//     < V and not blank; every other lane and slot loads nothing and uses 0.  ctx is checked against ctx_mod first, so every index is
//     < ctx_mod V = V^n.  The loads are in flight beside the parent lookup and the stay candidate and are waited for once, at the keys.
//   * w = __dadd_rn(__dmul_rn(alpha, (double)word), beta) as in the workgroup kernel: an extension scores (p + lp) + w, the merged term of the
//     stay candidate (parent i extended by last(j)) gets w(lmp_j); the blank update and the repeat branch are unchanged.
//   * the frame's words are parked in LDS (K_MAX x 4 SPL fp32 behind the trie's control words): winner r reads its word there as it reads
//     its log-prob in `frames` -- no second gather on the dependent chain -- and sets lmp = that word, ctx = (ctx_parent V + s) % ctx_mod;
//     a stay inherits both.
// Keys, pop rounds, tied_last, the trie and both result tails are the LM = false code.  The arguments ride in the last parameter: with LM it
// is a struct of the tail's own argument and BeamLm<true>; without, it is the type it always was (an empty struct behind it would still add
// four bytes to the kernel-argument segment), so those instantiations keep their argument list, their LDS, their code and their descriptor.
struct SmallLmScore { double* out_score; BeamLm<true> lm; };      // the 1-best tail's last argument with a language model
struct SmallLmNbest : SmallNbest { BeamLm<true> lm; };           // the N-best tail's
template <bool NBEST, bool LM> struct small_tail { using type = typename std::conditional<NBEST, const SmallNbest, double* __restrict__>::type; };
template <> struct small_tail<false, true> { using type = const SmallLmScore; };
template <> struct small_tail<true, true> { using type = const SmallLmNbest; };
__device__ __forceinline__ double* small_score(double* p) { return p; }
__device__ __forceinline__ double* small_score(const SmallLmScore& a) { return a.out_score; }
constexpr size_t lds_lm(int spl) { return (size_t)K_MAX * (4 * spl) * 4; }
constexpr size_t lds_bytes_lm(int spl) { return lds_bytes(spl) + lds_lm(spl); }      // 148.1 KB at SPL = 16

template <int SPL, bool NBEST = false, bool LM = false>
__global__ __launch_bounds__(64) void beam_small_kernel(
    const float* __restrict__ lp, long long stride_t, long long stride_b, const int32_t* __restrict__ lengths,
    int T, int V, int K, int blank, int collapse, int32_t* __restrict__ out_tokens, int32_t* __restrict__ out_len,
    typename small_tail<NBEST, LM>::type out_score) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* table = reinterpret_cast<unsigned*>(smem);
    static_assert(SPL == 8 || SPL == 16, "8 or 16 symbols per lane");
    constexpr int VM = 4 * SPL, SB = (SPL == 8) ? 3 : 4;                  // symbols the four rows cover; bits of a slot number
    constexpr unsigned TKM = (unsigned)(VM << 5) - 1u;                     // largest first-touch rank (symbol << 5 | entry << 1 | bit)
    constexpr int LOWBITS = 4 + SB + (SPL == 8 ? 10 : 11);                 // [rank | slot | entry] at the bottom of a key: 17 / 19 bits
    using mask_t = typename std::conditional<SPL == 8, unsigned, unsigned long long>::type;      // one bit per symbol
    float* frames = reinterpret_cast<float*>(smem + LDS_TABLE);
    mask_t* mm = reinterpret_cast<mask_t*>(smem + LDS_TABLE + lds_frames(SPL));
    [[maybe_unused]] float* lmw = reinterpret_cast<float*>(smem + LDS_TABLE + lds_frames(SPL) + LDS_MM);      // LM only: [K_MAX][VM] table words of the frame
    const int b = blockIdx.x, lane = threadIdx.x, q = lane >> 4, j = lane & 15;
    int Tb = lengths ? lengths[b] : T; Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);

    for (int i = lane; i < H / 4; i += 64) reinterpret_cast<uint4*>(table)[i] = make_uint4(0u, 0u, 0u, 0u);
#ifdef PGASR_BEAM_DIAG
    const long long dg_c0_ = clock64();
    const bool getenv_cycles_ = (collapse & 2) != 0;      // diagnostic: flags bit 2 of the entry point -> out_score = cycles per frame
#endif

    // entry state, replicated per row
    double pb = (j == 0) ? 0.0 : -INFINITY, pnb = -INFINITY, tot = (j == 0) ? 0.0 : -INFINITY;
    unsigned id = (j == 0) ? ROOT : BAD_ID, par = NONE;
    int last = -1;
    int nb = 1, root_pos = 0;
    [[maybe_unused]] int ctx = 0;             // LM only: context index of the entry's prefix
    [[maybe_unused]] float lmp = 0.0f;        // LM only: table word of the entry's own last emission (unused while last < 0)
    if constexpr (LM) ctx = out_score.lm.ctx0;

    const float* base = lp + (long long)b * stride_b;
    constexpr int FPI = 64 / VM, NPRE = CH / FPI;          // frames one wave instruction covers (2 / 1), instructions per chunk
    const int lsym = lane & (VM - 1), lhalf = lane / VM;
    float pre[NPRE];
    auto issue = [&](int t0) {
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int t = t0 + FPI * i + lhalf;
            pre[i] = (lsym < V && t < Tb) ? base[(long long)t * stride_t + lsym] : -INFINITY;
        }
    };
    auto commit = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NPRE; ++i) frames[buf * (CH * VM) + (FPI * i + lhalf) * VM + lsym] = pre[i];
    };
    issue(0); commit(0); issue(CH);
    __syncthreads();
    bool tied_last = false;      // the previous frame needed the exact rounds: two beam entries with bit-identical totals stay tied for as long as both
                                 // live (every extension of one meets the same extension of the other), so the speculative rounds are skipped

    for (int t = 0; t < Tb; ++t) {
        if ((t & (CH - 1)) == 0 && t > 0) {          // chunk boundary: the next chunk's rows have long arrived
            commit((t >> 5) & 1);
            issue(t + CH);
            __syncthreads();
        }
        [[maybe_unused]] float tv[SPL];
        if constexpr (LM) {      // issue the gathers first: nothing depends on them until the keys
            const BeamLm<true>& lm = out_score.lm;
            const bool ok = (j < nb) && ((unsigned)ctx < (unsigned)lm.ctx_mod);      // ctx V + s < ctx_mod V = V^n <= 2^25
            const float* row = lm.table + ((long long)(ok ? ctx : 0) * V + SPL * q);
#pragma unroll
            for (int i = 0; i < SPL; ++i) {
                const int s = SPL * q + i;
                tv[i] = (ok && s < V && s != blank) ? row[i] : 0.0f;
            }
        }
        const float* fr = frames + ((t >> 5) & 1) * (CH * VM) + (t & (CH - 1)) * VM;
        float lpv[SPL];
#pragma unroll
        for (int c = 0; c < SPL / 4; ++c) {
            const float4 f4 = *reinterpret_cast<const float4*>(fr + SPL * q + 4 * c);
            lpv[4 * c] = f4.x; lpv[4 * c + 1] = f4.y; lpv[4 * c + 2] = f4.z; lpv[4 * c + 3] = f4.w;
        }
        const float lp_bl = fr[blank];
        const float lp_la = fr[last >= 0 ? last : 0];

        // ---- where is my parent, which of my children are in the beam ----
        int pidx = -1;
        if (j < nb) {
            if (par == ROOT) pidx = root_pos;
            else if (par != NONE) pidx = (int)((table[par] >> 25) & 31u) - 1;
        }
        // DS operations of one wave execute in issue order: zero, atomic-or and read need no wait between them
        if (lane < 16) mm[lane] = (mask_t)0;
        if (lane < nb && pidx >= 0) atomicOr(&mm[pidx], (mask_t)1 << last);
        const mask_t mmask = __hip_atomic_load(&mm[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);

        const int src = pidx >= 0 ? pidx : 0;
        const double pb_i = __shfl(pb, src, 16), tot_i = __shfl(tot, src, 16);
        const int last_i = __shfl(last, src, 16);

        // ---- stay candidate of entry j (:78-82, :90-96 merged, :103-106) ----
        const double npb = tot + (double)lp_bl;
        const bool has_last = last >= 0, has_par = pidx >= 0;
        const double dla = (double)lp_la;
        const double own = has_last ? pnb + dla : -INFINITY;                                    // repeat of the last symbol
        double ext = (has_last && has_par) ? ((last_i == last) ? pb_i : tot_i) + dla : -INFINITY;   // parent i extended by it
        if constexpr (LM) ext += __dadd_rn(__dmul_rn(out_score.lm.alpha, (double)lmp), out_score.lm.beta);             // that extension's own table word (-inf stays -inf)
        const double npnb = lse2f(ext, own);
        const unsigned lbits = (unsigned)(has_last ? last : 0) << 5;
        const unsigned t_bl = ((unsigned)blank << 5) | ((unsigned)j << 1);
        const unsigned t_own = has_last ? (lbits | ((unsigned)j << 1) | 1u) : 0xFFFFu;
        const unsigned t_e = (has_last && has_par) ? (lbits | ((unsigned)pidx << 1)) : 0xFFFFu;
        unsigned tie = t_bl < t_own ? t_bl : t_own;
        tie = tie < t_e ? tie : t_e;
        const double sstay = lse2f(npb, npnb);

        // ---- the SPL candidates of this lane as keys ----
        const long long tb0 = __double_as_longlong(tot);
        const double tot0 = __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)(tb0 >> 32), 0) << 32) |
                                                 (unsigned)__builtin_amdgcn_readlane((int)(unsigned)tb0, 0));
        const double ref = (tot0 == -INFINITY) ? 0.0 : tot0;
        unsigned long long k[SPL];
        if constexpr (LM) {      // park the frame's words for the winners: lane (q, j) owns row j's words SPL q .. SPL q + SPL - 1
#pragma unroll
            for (int c = 0; c < SPL / 4; ++c)
                *reinterpret_cast<float4*>(lmw + j * VM + SPL * q + 4 * c) = make_float4(tv[4 * c], tv[4 * c + 1], tv[4 * c + 2], tv[4 * c + 3]);
        }
#pragma unroll
        for (int i = 0; i < SPL; ++i) {
            const int s = SPL * q + i;
            const bool is_bl = (s == blank);
            const bool alive = (j < nb) && (s < V) && (is_bl || !((mmask >> s) & (mask_t)1));
            double sx = ((s == last) ? pb : tot) + (double)lpv[i];
            if constexpr (LM) sx += __dadd_rn(__dmul_rn(out_score.lm.alpha, (double)tv[i]), out_score.lm.beta);
            const double sc = is_bl ? sstay : sx;
            const unsigned tk = is_bl ? tie : (((unsigned)s << 5) | ((unsigned)j << 1));
            const long long bits = __double_as_longlong(sc - ref);
            unsigned long long key = (unsigned long long)bits ^ ((unsigned long long)(bits >> 63) | 0x8000000000000000ull);
            key = (key & ~((1ull << LOWBITS) - 1ull)) | ((unsigned long long)(TKM - tk) << (4 + SB)) | ((unsigned long long)i << 4) | (unsigned long long)j;
            k[i] = alive ? key : 0ull;
        }
        if constexpr (SPL == 8) {
        // descending 8-input sorting network (19 exchanges)
        SB_CE(0, 1) SB_CE(2, 3) SB_CE(4, 5) SB_CE(6, 7)
        SB_CE(0, 2) SB_CE(1, 3) SB_CE(4, 6) SB_CE(5, 7)
        SB_CE(1, 2) SB_CE(5, 6) SB_CE(0, 4) SB_CE(3, 7)
        SB_CE(1, 5) SB_CE(2, 6)
        SB_CE(1, 4) SB_CE(3, 6)
        SB_CE(2, 4) SB_CE(3, 5)
        SB_CE(3, 4)
        } else {
        // descending 16-input network: Batcher's odd-even merge sort, 63 exchanges in 10 layers (checked on all 2^16 0/1 inputs)
        SB_CE(0, 1) SB_CE(2, 3) SB_CE(0, 2) SB_CE(1, 3) SB_CE(1, 2) SB_CE(4, 5) SB_CE(6, 7) SB_CE(4, 6) SB_CE(5, 7) SB_CE(5, 6)
        SB_CE(0, 4) SB_CE(2, 6) SB_CE(2, 4) SB_CE(1, 5) SB_CE(3, 7) SB_CE(3, 5) SB_CE(1, 2) SB_CE(3, 4) SB_CE(5, 6)
        SB_CE(8, 9) SB_CE(10, 11) SB_CE(8, 10) SB_CE(9, 11) SB_CE(9, 10) SB_CE(12, 13) SB_CE(14, 15) SB_CE(12, 14) SB_CE(13, 15) SB_CE(13, 14)
        SB_CE(8, 12) SB_CE(10, 14) SB_CE(10, 12) SB_CE(9, 13) SB_CE(11, 15) SB_CE(11, 13) SB_CE(9, 10) SB_CE(11, 12) SB_CE(13, 14)
        SB_CE(0, 8) SB_CE(4, 12) SB_CE(4, 8) SB_CE(2, 10) SB_CE(6, 14) SB_CE(6, 10) SB_CE(2, 4) SB_CE(6, 8) SB_CE(10, 12)
        SB_CE(1, 9) SB_CE(5, 13) SB_CE(5, 9) SB_CE(3, 11) SB_CE(7, 15) SB_CE(7, 11) SB_CE(3, 5) SB_CE(7, 9) SB_CE(11, 13)
        SB_CE(1, 2) SB_CE(3, 4) SB_CE(5, 6) SB_CE(7, 8) SB_CE(9, 10) SB_CE(11, 12) SB_CE(13, 14)
        }
        // the lane's sorted list stays in registers; a pop shifts it (14 v_mov under a one-lane exec mask: no LDS round trip,
        // no wait on the K-round chain)

        // ---- K rounds: pop the winners in rank order ----
        // Round 5: a round used to be all-reduce (4 DPP) -> 4 readlanes -> 3 scalar max -> compare -> ballot -> ffs -> readlane of the
        // winner's low word -> 16 moves under a one-lane exec mask, ~420 cycles of mostly scalar-unit round trips, sixteen times per
        // frame (60 % of it).  Now the chain of a round is vector-only: all-reduce of the lists' HIGH words (4 DPP + 2 row swaps),
        // compare, and a shift of the eight high words of the lanes that won (v_cndmask on the compare's mask).  What a round
        // leaves behind -- which lane won (s_ff1 of the mask -> v_writelane into lane r) and a won-bit per lane -- is scalar work off
        // the chain; the winners' identities are put together AFTER the rounds: lane r fetches its winner lane's won-bits and sort
        // permutation with two ds_bpermute and finds the slot as the (number of earlier wins of that lane)-th of its sorted list.
        // A round in which two lanes share the maximal high word (equal to 2^-20 relative) makes both pop: the scalar tallies disagree and
        // the frame is redone by the exact loop below -- 0.1-0.8 % of the frames on random and model-like log-probs (make beamdiag,
        // tools/dev/r5_beam_ties.py).  Except: two beam entries with BIT-IDENTICAL totals stay tied for as long as both live (every extension of
        // one meets the same extension of the other); one such utterance of 32 fell back in 871 of its 1000 frames and set the kernel's time
        // (5.47 ms against 4.07 for the same distribution with another seed).  So a frame that follows a tied frame goes straight to the exact
        // rounds (tied_last), and those use the vector-only all-reduce as well: 4.71 ms on that data (tools/dev/r5_beam_var.py).
        // (Measured and not kept in round 4: TWO winners per round from one all-reduce over (first, second) pairs of high words.)
        unsigned packed = 0u;
        int nnew = 0;
        {
            unsigned hq[SPL];
            unsigned perm[2] = {0u, 0u};           // slot of the d-th key of the sorted list, SB bits each, eight per word
#pragma unroll
            for (int d = 0; d < SPL; ++d) { hq[d] = (unsigned)(k[d] >> 32); perm[d >> 3] |= (((unsigned)k[d] >> 4) & (unsigned)(SPL - 1)) << (SB * (d & 7)); }
            unsigned won = 0u, wl_of = 0u;
            int pops = 0, rounds = 0;
            bool need_exact = tied_last;                        // straight to the exact rounds
            if (!need_exact) {
            // sixteen rounds written out (default) or a rolled loop (-DPGASR_BEAM_UNROLL=0): written out, the compiler keeps a 64-bit "K > r" mask
            // per round alive across the frame loop (106 SGPRs) -- but the rolled loop is no faster: same box, A/B/A/B by library
            // (tools/dev/r5_beam_unroll.sh), beam 16 flat 3.37 written out / 3.55 rolled, peaked 3.91 / 4.09, beam 5 2.34 / 2.29
#if PGASR_BEAM_UNROLL
#define SB_ROUND_BODY(r, RC)                                                                                             \
            {                                                                                                            \
                const unsigned hh = hq[0];                                                                               \
                const unsigned smax = wave_allmax_valu(hh);                                                              \
                const bool win = (hh == smax) && (smax != 0u);                                                           \
                const unsigned long long m = __ballot(hh == smax) & __ballot(smax != 0u);   /* two compare masks: no 0/1 round trip */ \
                pops += __popcll(m); rounds += (m != 0ull) ? 1 : 0;                                                      \
                {   /* lane r of wl_of := the winner lane (a scalar); v_writelane has no builtin in this compiler */     \
                    const int wls = __ffsll((long long)m) - 1;                                                           \
                    asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(wl_of) : "s"(wls), RC(r));                          \
                }                                                                                                        \
                won |= win ? (1u << (r)) : 0u;                                                                           \
                _Pragma("unroll") for (int d = 0; d < SPL - 1; ++d) hq[d] = win ? hq[d + 1] : hq[d];                     \
                hq[SPL - 1] = win ? 0u : hq[SPL - 1];                                                                    \
            }
#define SB_ROUND(r) if (K > (r)) SB_ROUND_BODY(r, "n")
            SB_ROUND(0) SB_ROUND(1) SB_ROUND(2) SB_ROUND(3) SB_ROUND(4) SB_ROUND(5) SB_ROUND(6) SB_ROUND(7)
            SB_ROUND(8) SB_ROUND(9) SB_ROUND(10) SB_ROUND(11) SB_ROUND(12) SB_ROUND(13) SB_ROUND(14) SB_ROUND(15)
#undef SB_ROUND
            static_assert(K_MAX == 16, "sixteen rounds are written out");
#else
#pragma unroll 1
            for (int r = 0; r < K; ++r) {
                const unsigned hh = hq[0];
                const unsigned smax = wave_allmax_valu(hh);
                const bool win = (hh == smax) && (smax != 0u);
                const unsigned long long m = __ballot(win);
                pops += __popcll(m); rounds += (m != 0ull) ? 1 : 0;
                {   // lane r of wl_of := the winner lane (a scalar); v_writelane has no builtin in this compiler
                    const int wls = __ffsll((long long)m) - 1;
                    asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(wl_of) : "s"(wls), "s"(r) : "m0");      // two scalar operands: the lane select goes through M0
                }
                won |= win ? (1u << r) : 0u;
#pragma unroll
                for (int d = 0; d < SPL - 1; ++d) hq[d] = win ? hq[d + 1] : hq[d];
                hq[SPL - 1] = win ? 0u : hq[SPL - 1];
            }
#endif
                need_exact = pops != rounds;
            }
            tied_last = false;
            if (!need_exact) {
                nnew = rounds;
                const unsigned wl = row0_to_all(wl_of);                       // lane (q, j): the winner lane of round j
                const unsigned wwon = (unsigned)__shfl((int)won, (int)(wl & 63u), 64);
                unsigned wperm = (unsigned)__shfl((int)perm[0], (int)(wl & 63u), 64);
                const int idx = __popc(wwon & ((1u << j) - 1u));               // how many rounds before round j that lane had won
                if constexpr (SPL == 16) {
                    const unsigned wperm1 = (unsigned)__shfl((int)perm[1], (int)(wl & 63u), 64);
                    wperm = (idx & 8) ? wperm1 : wperm;
                }
                const unsigned slot = (wperm >> (SB * (idx & 7))) & (unsigned)(SPL - 1);
                packed = ((wl >> 4) << (4 + SB)) | (slot << 4) | (wl & 15u);
            } else {
#ifdef PGASR_BEAM_DIAG
                if (lane == 0) atomicAdd(&beam_diag_counters[1], 1ull);
#endif
                // exact rounds on the full keys (ties between high words; rare)
                for (int r = 0; r < K; ++r) {
                    const unsigned long long head = k[0];
                    const unsigned hh = (unsigned)(head >> 32);
                    const unsigned smax = wave_allmax_valu(hh);
                    if (smax == 0u) break;
                    unsigned long long m = __ballot(hh == smax);
                    if (__popcll(m) != 1) {
                        tied_last = true;
                        const unsigned ll = (hh == smax) ? (unsigned)head : 0u;
                        const unsigned smaxlo = wave_allmax_valu(ll);
                        m = __ballot(hh == smax && (unsigned)head == smaxlo);
                    }
                    const int wl = __ffsll((long long)m) - 1;
                    const unsigned wlo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)head, wl);
                    const unsigned pk = ((unsigned)(wl >> 4) << (4 + SB)) | (wlo & ((1u << (4 + SB)) - 1u));
                    if (j == r) packed = pk;
                    if (lane == wl) {
#pragma unroll
                        for (int d = 0; d < SPL - 1; ++d) k[d] = k[d + 1];
                        k[SPL - 1] = 0ull;
                    }
                    ++nnew;
                }
            }
        }

#ifdef PGASR_BEAM_DIAG
        if (lane == 0) atomicAdd(&beam_diag_counters[0], 1ull);
#endif
        // ---- the new beam: entry r <- winner r ----
        const int pj = (int)(packed & 15u), slot = (int)((packed >> 4) & (unsigned)(SPL - 1)), pq = (int)(packed >> (4 + SB));
        const int s = SPL * pq + slot;
        const bool valid = j < nnew;
        const bool stay = (s == blank);
        const double g_tot = __shfl(tot, pj, 16), g_pb = __shfl(pb, pj, 16);
        const double g_npb = __shfl(npb, pj, 16), g_npnb = __shfl(npnb, pj, 16), g_sstay = __shfl(sstay, pj, 16);
        const unsigned g_id = (unsigned)__shfl((int)id, pj, 16), g_par = (unsigned)__shfl((int)par, pj, 16);
        const int g_last = __shfl(last, pj, 16);
        const float lps = fr[valid ? s : 0];
        [[maybe_unused]] float g_word = 0.0f, g_lmp = 0.0f;
        [[maybe_unused]] int g_ctx = 0;
        if constexpr (LM) {
            g_word = lmw[valid ? pj * VM + s : 0];      // pj < 16, s < VM: inside the K_MAX x VM words; parked before the rounds (DS operations of one wave execute in issue order)
            g_lmp = __shfl(lmp, pj, 16);
            g_ctx = __shfl(ctx, pj, 16);
        }

        // beam-position bits of the outgoing entries are cleared before the incoming ones are set
        if (lane < nb && id != ROOT) atomicAnd(&table[id], KEYMASK);
        unsigned n_id = BAD_ID;
        if (lane < 16 && valid) {
            if (stay) n_id = g_id;
            else {
                // canonical node of (parent id, symbol): find, else insert
                const unsigned key = ((g_id << 8) | (unsigned)s) + 1u;
                // Triangular probing (h + 1, + 2, + 3, ..: visits every slot of a power-of-two table) behind a two-round mix.  Round 5: the table
                // holds every prefix an utterance ever had in its beam (up to T * beam of 32768 slots), and with linear probing behind one
                // multiplicative round the chains clustered -- up to 24-30 probes, each a dependent LDS round trip the whole wave waits for,
                // and the kernel's time followed the unluckiest utterance (same distribution, other seed: 4.07 against 5.47 ms at beam 16).
                unsigned h = key * 2654435761u;
                h ^= h >> 15; h *= 0x2C1B3C6Du;
                h >>= 17;
                for (int guard = 0; guard < H; ++guard) {
#ifdef PGASR_BEAM_DIAG
                    atomicAdd(&beam_diag_counters[2], 1ull);
                    atomicMax(&beam_diag_counters[3], (unsigned long long)(guard + 1));
#endif
                    const unsigned v = table[h];
                    if ((v & KEYMASK) == key) { n_id = h; break; }
                    if (v == 0u) {
                        const unsigned old = atomicCAS(&table[h], 0u, key);
                        if (old == 0u || (old & KEYMASK) == key) { n_id = h; break; }
                    }
                    h = (h + (unsigned)guard + 1u) & (unsigned)(H - 1);
                }
            }
        }
        n_id = (unsigned)__shfl((int)n_id, j, 64);
        if (lane < 16 && valid && n_id != ROOT && n_id != BAD_ID) atomicOr(&table[n_id], (unsigned)(lane + 1) << 25);
        const unsigned long long rootm = __ballot(lane < 16 && valid && n_id == ROOT);
        root_pos = rootm ? (__ffsll((long long)rootm) - 1) : -1;

        if (valid) {
            if (stay) {
                pb = g_npb; pnb = g_npnb; tot = g_sstay; last = g_last; par = g_par;
                if constexpr (LM) { ctx = g_ctx; lmp = g_lmp; }
            } else {
                pb = -INFINITY;
                pnb = ((s == g_last) ? g_pb : g_tot) + (double)lps;
                if constexpr (LM) {      // the candidate's score as its key had it; its word becomes the entry's own
                    pnb += __dadd_rn(__dmul_rn(out_score.lm.alpha, (double)g_word), out_score.lm.beta);
                    lmp = g_word;
                    ctx = (int)((unsigned)(g_ctx * V + s) % (unsigned)out_score.lm.ctx_mod);
                }
                tot = pnb; last = s; par = g_id;
            }
            id = n_id;
        } else {
            pb = pnb = tot = -INFINITY; last = -1; par = NONE; id = BAD_ID;
            if constexpr (LM) { ctx = 0; lmp = 0.0f; }
        }
        nb = nnew;
    }

    if constexpr (NBEST) {
        // ---- result: the first nbest entries of the final beam.  Lane r < count of row 0 holds entry r (rank order) and walks its
        // own ancestors through the table twice: once to count (with collapse, kept tokens only: a token is dropped when the one before
        // it is the same), once to write back to front.  Every walk ends at the root, at an id outside the table or after T_b steps.
        __syncthreads();
        const int B = (int)gridDim.x, N = out_score.nbest, S = out_score.tok_stride;
        const int count = N < nb ? N : nb;
        const bool coll = (collapse & 1) != 0;
        int mylen = 0;
        if (lane < count) {
            int32_t* o = out_tokens + ((size_t)lane * B + b) * S;
            int kept = 0;
            for (int pass = 0; pass < 2; ++pass) {
                unsigned cur = id;
                int pos = kept, pending = -1;          // pending: the token behind the one about to be read, not yet decided
                for (int n = 0; cur != ROOT && cur < (unsigned)H && n < Tb; ++n) {
                    const unsigned v = (table[cur] & KEYMASK) - 1u;
                    const int tok = (int)(v & 255u);
                    if (pending >= 0 && !(coll && pending == tok)) {
                        if (pass == 0) ++kept; else o[--pos] = pending;
                    }
                    pending = tok;
                    cur = v >> 8;
                }
                if (pending >= 0) {                    // the first token is always kept
                    if (pass == 0) ++kept; else o[--pos] = pending;
                }
            }
            mylen = kept;
        }
        if (lane < N) {                                // N <= K <= 16: row 0
            out_len[(size_t)lane * B + b] = mylen;
            out_score.out_score[(size_t)lane * B + b] = lane < count ? ((Tb > 0) ? -tot : -0.0) : (double)INFINITY;
        }
        if (lane == 0) out_score.out_count[b] = count;
        for (int r = 0; r < N; ++r) {                  // zero tails (and whole rows beyond count), coalesced; disjoint from the tokens written above
            int32_t* o = out_tokens + ((size_t)r * B + b) * S;
            const int lr = __builtin_amdgcn_readlane(mylen, r);
            for (int i = lr + lane; i < S; i += 64) o[i] = 0;
        }
        return;
    } else {
    // ---- result: ancestors of the best entry, in order, optionally through collapse_fn ----
    __syncthreads();
    unsigned short* tmp = reinterpret_cast<unsigned short*>(frames);      // 8 KB = 4096 tokens: the dispatch admits T <= MAX_TOKENS only
    unsigned cur = (unsigned)__builtin_amdgcn_readlane((int)id, 0);
    int n = 0;
    if (nb > 0) {
        while (cur != ROOT && cur < (unsigned)H && n < T) {
            const unsigned v = (table[cur] & KEYMASK) - 1u;
            if (lane == 0) tmp[n] = (unsigned short)(v & 255u);
            ++n;
            cur = v >> 8;
        }
    }
    __syncthreads();
    int32_t* o = out_tokens + (size_t)b * T;
    int outn = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        int tok = 0; bool keep = false;
        if (i < n) {
            tok = tmp[n - 1 - i];
            keep = !(collapse & 1) || i == 0 || tok != (int)tmp[n - i];
        }
        const unsigned long long m = __ballot(keep);
        if (keep) o[outn + __popcll(m & ((1ull << lane) - 1ull))] = tok;
        outn += __popcll(m);
    }
    if (lane == 0) {
        out_len[b] = outn;
        const double t0 = __shfl(tot, 0, 64);
        small_score(out_score)[b] = (Tb > 0) ? -t0 : -0.0;
#ifdef PGASR_BEAM_DIAG
        if (getenv_cycles_) small_score(out_score)[b] = (double)(clock64() - dg_c0_) / (double)(Tb > 0 ? Tb : 1);      // cycles per frame of this utterance
#endif
    }
    }
}
#undef SB_CE
}  // namespace sb

}  // namespace

#ifdef PGASR_BEAM_DIAG
extern "C" int pgasr_diag_beam_counters(unsigned long long* out, int reset) {      // host copy of (frames, frames redone by the exact rounds)
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(beam_diag_counters), sizeof(unsigned long long) * 4) != hipSuccess) return 1;
    if (reset) { unsigned long long z[4] = {0, 0, 0, 0}; if (hipMemcpyToSymbol(HIP_SYMBOL(beam_diag_counters), z, sizeof(z)) != hipSuccess) return 1; }
    return 0;
}
#endif

extern "C" size_t pgasr_beam_workspace_bytes(int T, int B, int V, int beam) {
    if (T <= 0 || B <= 0 || V <= 0 || beam <= 0) return 0;
    return trie_ws_layout<BEAM_SYM_BITS>(T, B, beam, nullptr, nullptr);
}

namespace {
// the single-wave kernel's limits (namespace sb)
inline bool beam_single_wave_fits(int T, int V, int beam) {
    return beam <= sb::K_MAX && V <= sb::V_MAX && (long long)T * beam <= sb::MAX_NODES && T <= sb::MAX_TOKENS;
}
}  // namespace

// Which kernel flags bit 4 picks (include/pgasr_hip.h, A7-LM): 1 = the single-wave kernel's LM instantiations.  Host only, no HIP call.
extern "C" int pgasr_beam_lm_single_wave_ok(int T, int V, int beam, int is_f64, int lm_order) {
    if (T <= 0 || V <= 0 || beam <= 0 || lm_order <= 0 || is_f64) return 0;
    if (!beam_single_wave_fits(T, V, beam)) return 0;
    long long entries = 1;
    for (int k = 0; k < lm_order; ++k) { entries *= V; if (entries > BEAM_LM_MAX_ENTRIES) return 0; }      // such a table is refused by the search itself
    return 1;
}

namespace {
// One call of the narrow search, as the five entries below fill it in: the common arguments, the list's (list = false: the 1-best
// result), the language model's (lm_order = 0: none) and the bias automaton's (a NULL table with no states: none).
struct BeamCall {
    const void* log_probs; int is_f64; long long stride_t, stride_b; const int32_t* lengths; int T, B, V, beam, blank, flags;
    int32_t* out_tokens; int32_t* out_len; double* out_score; void* workspace; size_t workspace_bytes; void* stream;
    bool list = false; int nbest = 0, tok_stride = 0; int32_t* out_count = nullptr;
    const float* lm_table = nullptr; int lm_order = 0; double lm_alpha = 0.0, lm_beta = 0.0;
    const void* bias_table = nullptr; int bias_states = 0; double bias_weight = 0.0;
    bool words = false; const void* trie = nullptr; int trie_states = 0; const int32_t* node_word = nullptr;
    const pgasr_word_lm_tables* word_tables = nullptr; int delimiter = 0; double word_alpha = 0.0, word_beta = 0.0; int flags2 = 0;

    BeamCall& with_list(int n, int stride, int32_t* count) { list = true; nbest = n; tok_stride = stride; out_count = count; return *this; }
    BeamCall& with_lm(const float* table, int order, double alpha, double beta) {
        lm_table = table; lm_order = order; lm_alpha = alpha; lm_beta = beta; return *this;
    }
    BeamCall& with_bias(const void* table, int states, double weight) { bias_table = table; bias_states = states; bias_weight = weight; return *this; }
    BeamCall& with_words(const void* t, int states, const int32_t* nw, const pgasr_word_lm_tables* tb, int d, double alpha, double beta, int f2) {
        words = true; trie = t; trie_states = states; node_word = nw; word_tables = tb; delimiter = d; word_alpha = alpha; word_beta = beta; flags2 = f2;
        return *this;
    }
};

// the language model's arguments (no HIP call): PGASR_OK with *lm filled where lm_order > 0
int beam_lm_args(const BeamCall& c, BeamLm<true>* lm) {
    if (c.lm_order < 0 || (c.lm_order > 0) != (c.lm_table != nullptr)) return PGASR_ERR_INVALID_ARG;
    if (c.lm_order > 0) {
        if (!std::isfinite(c.lm_alpha) || !std::isfinite(c.lm_beta)) return PGASR_ERR_INVALID_ARG;
        long long entries = 1, ctx_mod = 1, ctx0 = 0;
        for (int k = 0; k < c.lm_order; ++k) {
            if (k == c.lm_order - 1) ctx_mod = entries;
            entries *= c.V;
            if (entries > BEAM_LM_MAX_ENTRIES) return PGASR_ERR_UNSUPPORTED;      // refused, never truncated
        }
        for (int k = 0; k < c.lm_order - 1; ++k) ctx0 = ctx0 * c.V + c.blank;
        *lm = {c.lm_table, (int)ctx_mod, (int)ctx0, c.lm_alpha, c.lm_beta};
    }
    return PGASR_OK;
}

// the bias table's arguments (no HIP call; include/pgasr_hip.h, A7-BIAS): a NULL table with no states is "no bias"
int beam_bias_args(const BeamCall& c) {
    if (!c.bias_table && c.bias_states == 0) return PGASR_OK;
    if (!bias_table::usable(c.bias_table, c.bias_states, c.V) || !std::isfinite(c.bias_weight)) return PGASR_ERR_INVALID_ARG;
    if (c.flags & (8 | 16)) return PGASR_ERR_UNSUPPORTED;      // the single-wave kernel has no bias: refused, never run differently
    return PGASR_OK;
}

// the word fusion's arguments (no HIP call; include/pgasr_hip.h, A7-WORDFUSE)
int beam_words_args(const BeamCall& c) {
    if (!c.words) return PGASR_OK;
    if (!c.trie || !c.node_word || !c.word_tables) return PGASR_ERR_INVALID_ARG;
    const pgasr_word_lm_tables& tb = *c.word_tables;          // host memory
    if (!bias_table::usable(c.trie, c.trie_states, c.V) || !std::isfinite(c.word_alpha) || !std::isfinite(c.word_beta)) return PGASR_ERR_INVALID_ARG;
    if (tb.order < 1 || tb.order > word_ngram::WL_MAX_ORDER || tb.n_words > (1 << 22) || tb.ngram_cap > (1 << 25)) return PGASR_ERR_UNSUPPORTED;
    if (!tb.uni_logp || !tb.uni_bow || !tb.ngram_slots || tb.n_words < word_ngram::WL_RESERVED) return PGASR_ERR_INVALID_ARG;
    if (tb.ngram_cap < 1 || (tb.ngram_cap & (tb.ngram_cap - 1)) != 0) return PGASR_ERR_INVALID_ARG;
    if (c.delimiter < 0 || c.delimiter >= c.V || c.delimiter == c.blank || (c.flags2 & ~3)) return PGASR_ERR_INVALID_ARG;
    if (c.lm_table || c.lm_order != 0 || c.bias_table) return PGASR_ERR_UNSUPPORTED;      // no dense table and no bias beside the word model
    if (c.flags & (8 | 16)) return PGASR_ERR_UNSUPPORTED;      // the single-wave kernel has no word model: refused, never run differently
    return PGASR_OK;
}

// the kernels' collapse argument: flags bit 0 and, in the diagnostic build, flags bit 2 as bit 1 (1-best without bias only)
inline int beam_collapse(const BeamCall& c) {
#ifdef PGASR_BEAM_DIAG
    if (!c.list && !c.bias_table && (c.flags & 4)) return (c.flags & 1) | 2;
#endif
    return c.flags & 1;
}

// f(std::bool_constant<b>...) for runtime b...: the launchers' template arguments
template <bool... Bs, typename F> int beam_with_bools(F&& f) { return f(std::bool_constant<Bs>{}...); }
template <bool... Bs, typename F, typename... R> int beam_with_bools(F&& f, bool b, R... r) {
    return b ? beam_with_bools<Bs..., true>(f, r...) : beam_with_bools<Bs..., false>(f, r...);
}

// The workgroup-per-utterance kernel.  Its last argument is exactly the type the instantiation declares (the tails ride behind one another).
// is_f64: exact path, fp64 transcendentals (drop-in CTCDecoder.decode); fp32 device log-probs: fast transcendentals
template <bool LM, bool NBEST, bool BIAS>
int launch_workgroup(const BeamCall& c, const BeamLm<true>& lm, const BeamWs& ws, size_t lds) {
    typename std::conditional<BIAS, BeamBiased<LM, NBEST>, BeamTail<LM, NBEST>>::type tail{};
    if constexpr (LM) static_cast<BeamLm<true>&>(tail) = lm;
    if constexpr (NBEST) { tail.nbest = c.nbest; tail.tok_stride = c.tok_stride; tail.out_count = c.out_count; }
    if constexpr (BIAS) { tail.btable = (const BiasWord*)c.bias_table; tail.bstates = c.bias_states; tail.bweight = c.bias_weight; }
    const auto launch = [&](auto kern, auto* lp) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        PGASR_LAUNCH_KERNEL(kern, dim3(c.B), dim3(BEAM_THREADS), lds, (hipStream_t)c.stream, lp, c.stride_t, c.stride_b, c.lengths, c.T, c.V,
                            c.beam, c.blank, beam_collapse(c), ws, c.out_tokens, c.out_len, c.out_score, tail);
    };
    if (c.is_f64) launch(&beam_search_kernel<double, false, LM, NBEST, BIAS>, (const double*)c.log_probs);
    else launch(&beam_search_kernel<float, true, LM, NBEST, BIAS>, (const float*)c.log_probs);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

// The same kernel with the word fusion (WORDS = true): the N-best form, no dense table, no bias
int launch_words(const BeamCall& c, const BeamWs& ws, size_t lds) {
    const pgasr_word_lm_tables& tb = *c.word_tables;
    BeamWords tail{};
    tail.nbest = c.nbest; tail.tok_stride = c.tok_stride; tail.out_count = c.out_count;
    tail.trie = (const BiasWord*)c.trie; tail.node_word = c.node_word;
    tail.slots = (const NgramSlot*)tb.ngram_slots; tail.uni_logp = tb.uni_logp; tail.uni_bow = tb.uni_bow;
    tail.tstates = c.trie_states; tail.order = tb.order; tail.n_words = tb.n_words; tail.ngram_cap = tb.ngram_cap; tail.delim = c.delimiter;
    tail.finalize = c.flags2 & 1; tail.eos = (c.flags2 >> 1) & 1;
    tail.alpha = c.word_alpha; tail.beta = c.word_beta;
    const auto launch = [&](auto kern, auto* lp) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        PGASR_LAUNCH_KERNEL(kern, dim3(c.B), dim3(BEAM_THREADS), lds, (hipStream_t)c.stream, lp, c.stride_t, c.stride_b, c.lengths, c.T, c.V,
                            c.beam, c.blank, c.flags & 1, ws, c.out_tokens, c.out_len, c.out_score, tail);
    };
    if (c.is_f64) launch(&beam_search_kernel<double, false, false, true, false, true>, (const double*)c.log_probs);
    else launch(&beam_search_kernel<float, true, false, true, false, true>, (const float*)c.log_probs);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

// The single-wave kernel: one wave per utterance, trie and candidate lists in LDS, no workspace traffic; 8 symbols per lane up to V = 32
// (the English alphabet of the headline), 16 up to V = 64 (round 5: CommonVoice's larger alphabets stay on this kernel)
template <bool LM, bool NBEST>
int launch_single_wave(const BeamCall& c, const BeamLm<true>& lm) {
    const auto tail = [&] {
        if constexpr (NBEST && LM) return sb::SmallLmNbest{{c.out_score, c.out_count, c.nbest, c.tok_stride}, lm};
        else if constexpr (NBEST) return sb::SmallNbest{c.out_score, c.out_count, c.nbest, c.tok_stride};
        else if constexpr (LM) return sb::SmallLmScore{c.out_score, lm};
        else return c.out_score;
    }();
    const int spl = c.V <= 32 ? 8 : 16;
    const auto kern = spl == 8 ? &sb::beam_small_kernel<8, NBEST, LM> : &sb::beam_small_kernel<16, NBEST, LM>;
    const size_t lds = LM ? sb::lds_bytes_lm(spl) : sb::lds_bytes(spl);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    PGASR_LAUNCH_KERNEL(kern, dim3(c.B), dim3(64), lds, (hipStream_t)c.stream, (const float*)c.log_probs, c.stride_t, c.stride_b, c.lengths,
                        c.T, c.V, c.beam, c.blank, beam_collapse(c), c.out_tokens, c.out_len, tail);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

// The host side of all five entries.  The shared checks with the language model's, the bias table's and the list's in their place;
// nothing touches HIP until every check has passed.  Then one kernel family:
//   * a bias table: the workgroup kernel, BIAS = true (the single-wave kernel has none);
//   * a language model, flags bit 4 and pgasr_beam_lm_single_wave_ok: the single-wave kernel's LM instantiations (the bit is the caller's
//     explicit choice, so bits 1 and 3 are not consulted);
//   * no model, fp32 log-probs inside the single-wave limits: the single-wave kernel -- the training path -- unless flags bit 1 opts a
//     1-best call out; a list has to opt in with flags bit 3 ("fast");
//   * everything else: the workgroup kernel, whose hash table is cleared first.
int beam_search_run(const BeamCall& c) {
    BeamLm<true> lm{};
    BeamWs ws;
    if (const int st = beam_check_args(c.log_probs, c.out_tokens, c.out_len, c.out_score, c.T, c.B, c.V, c.beam, c.blank, BEAM_VMAX, BEAM_KMAX,
                                       [&] {
                                           if (const int s = beam_lm_args(c, &lm)) return s;
                                           if (const int s = beam_bias_args(c)) return s;
                                           if (const int s = beam_words_args(c)) return s;
                                           const bool bad = c.list && (c.nbest < 1 || c.nbest > c.beam || c.tok_stride < c.T || !c.out_count);
                                           return bad ? (int)PGASR_ERR_INVALID_ARG : (int)PGASR_OK;
                                       },
                                       c.workspace, c.workspace_bytes, &ws)) return st;
    const bool with_lm = c.lm_order > 0, bias = c.bias_table != nullptr;
    const bool single_wave = with_lm ? (c.flags & 16) && pgasr_beam_lm_single_wave_ok(c.T, c.V, c.beam, c.is_f64, c.lm_order)
                                     : !c.is_f64 && (c.list ? (c.flags & 8) != 0 : !(c.flags & 2)) && beam_single_wave_fits(c.T, c.V, c.beam);
    if (!bias && !c.words && single_wave)
        return beam_with_bools([&](auto l, auto nb) { return launch_single_wave<decltype(l)::value, decltype(nb)::value>(c, lm); }, with_lm, c.list);
    const size_t lds = beam_lds_bytes(c.beam, c.V, with_lm, bias, c.words);
    if (lds > 160 * 1024) return PGASR_ERR_UNSUPPORTED;
    if (hipMemsetAsync(ws.table, 0, (size_t)c.B * ws.H * sizeof(unsigned long long), (hipStream_t)c.stream) != hipSuccess) return PGASR_ERR_LAUNCH;
    if (c.words) return launch_words(c, ws, lds);
    return beam_with_bools([&](auto l, auto nb, auto bi) { return launch_workgroup<decltype(l)::value, decltype(nb)::value, decltype(bi)::value>(c, lm, ws, lds); },
                           with_lm, c.list, bias);
}
}  // namespace

extern "C" int pgasr_ctc_beam_search(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                                     const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                                     int32_t* out_tokens, int32_t* out_len, double* out_score,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    return beam_search_run(BeamCall{log_probs, is_f64, stride_t, stride_b, lengths, T, B, V, beam, blank, flags, out_tokens, out_len, out_score,
                                     workspace, workspace_bytes, stream});
}

extern "C" int pgasr_ctc_beam_search_lm(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                                        const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                                        int32_t* out_tokens, int32_t* out_len, double* out_score,
                                        void* workspace, size_t workspace_bytes, void* stream,
                                        const float* lm_table, int lm_order, double lm_alpha, double lm_beta) {
    return beam_search_run(BeamCall{log_probs, is_f64, stride_t, stride_b, lengths, T, B, V, beam, blank, flags, out_tokens, out_len, out_score,
                                     workspace, workspace_bytes, stream}
                               .with_lm(lm_table, lm_order, lm_alpha, lm_beta));
}

// The N-best list of the final beam (include/pgasr_hip.h, A7-NBEST): the same search, NBEST = true
extern "C" int pgasr_ctc_beam_search_nbest(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                                           const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                                           int nbest, int32_t* out_tokens, int tok_stride, int32_t* out_len, double* out_score,
                                           int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream,
                                           const float* lm_table, int lm_order, double lm_alpha, double lm_beta) {
    return beam_search_run(BeamCall{log_probs, is_f64, stride_t, stride_b, lengths, T, B, V, beam, blank, flags, out_tokens, out_len, out_score,
                                     workspace, workspace_bytes, stream}
                               .with_list(nbest, tok_stride, out_count).with_lm(lm_table, lm_order, lm_alpha, lm_beta));
}

// Hotword biasing (include/pgasr_hip.h, A7-BIAS): the two searches with a bias automaton; a NULL table with no states is the call without.
extern "C" int pgasr_ctc_beam_search_bias(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                                          const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                                          int32_t* out_tokens, int32_t* out_len, double* out_score,
                                          void* workspace, size_t workspace_bytes, void* stream,
                                          const float* lm_table, int lm_order, double lm_alpha, double lm_beta,
                                          const void* bias_table, int bias_states, double bias_weight) {
    return beam_search_run(BeamCall{log_probs, is_f64, stride_t, stride_b, lengths, T, B, V, beam, blank, flags, out_tokens, out_len, out_score,
                                     workspace, workspace_bytes, stream}
                               .with_lm(lm_table, lm_order, lm_alpha, lm_beta).with_bias(bias_table, bias_states, bias_weight));
}

extern "C" int pgasr_ctc_beam_search_nbest_bias(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                                                const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                                                int nbest, int32_t* out_tokens, int tok_stride, int32_t* out_len, double* out_score,
                                                int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream,
                                                const float* lm_table, int lm_order, double lm_alpha, double lm_beta,
                                                const void* bias_table, int bias_states, double bias_weight) {
    return beam_search_run(BeamCall{log_probs, is_f64, stride_t, stride_b, lengths, T, B, V, beam, blank, flags, out_tokens, out_len, out_score,
                                     workspace, workspace_bytes, stream}
                               .with_list(nbest, tok_stride, out_count).with_lm(lm_table, lm_order, lm_alpha, lm_beta)
                               .with_bias(bias_table, bias_states, bias_weight));
}

// The word n-gram model and its lexicon inside the search (include/pgasr_hip.h, A7-WORDFUSE): the N-best search, WORDS = true
extern "C" int pgasr_ctc_beam_search_words(const void* log_probs, int is_f64, long long stride_t, long long stride_b,
                                           const int32_t* lengths, int T, int B, int V, int beam, int blank, int flags,
                                           int nbest, int32_t* out_tokens, int tok_stride, int32_t* out_len, double* out_score,
                                           int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream,
                                           const float* lm_table, int lm_order, double lm_alpha, double lm_beta,
                                           const void* trie, int trie_states, const int32_t* node_word, const pgasr_word_lm_tables* tables,
                                           int delimiter, double alpha, double beta, int flags2) {
    BeamCall c{log_probs, is_f64, stride_t, stride_b, lengths, T, B, V, beam, blank, flags, out_tokens, out_len, out_score,
               workspace, workspace_bytes, stream};
    c.with_list(nbest, tok_stride, out_count).with_words(trie, trie_states, node_word, tables, delimiter, alpha, beta, flags2);
    c.lm_table = lm_table; c.lm_order = lm_order; c.lm_alpha = lm_alpha; c.lm_beta = lm_beta;      // refused by beam_words_args, never by beam_lm_args' own rules
    return beam_search_run(c);
}
