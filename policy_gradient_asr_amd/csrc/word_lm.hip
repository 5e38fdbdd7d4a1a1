// Word n-gram language model over N-best lists on gfx950 (pgasr_nbest_word_lm_score, pgasr_nbest_combine_rank; semantics in
// include/pgasr_hip.h, section A7-WORDLM; the host's statement of the query is lm.WordNgramLM.logp_sentence).
//
// pgasr_nbest_word_lm_score: one launch, one workgroup of 256 threads per hypothesis, everything in dynamic LDS:
//   1. the hypothesis is staged as 16-bit words (a delimiter and a token outside the byte range get marks of their own);
//   2. wave 0 walks the row 64 tokens at a time: a ballot of the word starts, a popcount below the lane gives the word's index;
//   3. one thread per word hashes its spelling (FNV-1a + murmur3's finaliser, lm.hash_word), probes the word table and confirms
//      the candidate byte by byte on the packed pool -- a hash match alone never decides; the id (or <unk>) goes to LDS behind
//      order-1 ids of <s>, with </s> after the last word;
//   4. one thread per start position walks the chain of contexts that start there: entry(w_p), entry(w_p w_p+1), .. up to
//      order-1 words, each a probe keyed by (entry index of the context, word id) and confirmed on that pair (lm.hash_ngram:
//      splitmix64's finaliser, multipliers 0xBF58476D1CE4E5B9ull and 0x94D049BB133111EBull; the probe itself, ngram_find, is in
//      word_ngram.h, shared with the beam search's word fusion);
//   5. one thread per scored position (every word and </s>) walks the back-off rule from the longest context to the unigram
//      on those entry indices: its probes do not depend on each other, its fp64 sum is in the contractual order;
//   6. thread 0 adds the per-word scores in word order.
// Steps 3 - 5 are chains of dependent gathers (a 16-byte slot per probe: key, logp and bow in one load); 256 words in flight per
// workgroup and several workgroups per CU hide their latency.
//
// pgasr_nbest_combine_rank: one launch, one workgroup of 128 threads per utterance; the rank is that of csrc/nbest.hip.
#include "common.h"
#include "word_ngram.h"
#include <cmath>

namespace {

using namespace word_ngram;      // NgramSlot, ngram_find and the reserved ids: shared with the beam search's word fusion

constexpr int WL_THREADS = 256;
constexpr int WL_NMAX = 128;
constexpr int WL_MAX_WORD_LEN = 32;
constexpr int WL_MAX_STRIDE = PGASR_WORD_LM_MAX_STRIDE;   // 4096: 61 KB of LDS
constexpr unsigned short WL_DELIM = 0xFFFFu, WL_BAD = 0xFFFEu;      // LDS marks: a delimiter; a token outside [0, 255]

__device__ __forceinline__ uint32_t word_hash_step(uint32_t h, uint32_t c) { return (h ^ c) * 16777619u; }
__device__ __forceinline__ uint32_t word_hash_final(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// The carve of the dynamic LDS, for the kernel and for the launch alike (every offset a multiple of 16 bytes).
struct WordLmCarve { size_t score, id, ctx, tok, start, misc, bytes; };
__host__ __device__ inline size_t al(size_t x) { return (x + 15) & ~(size_t)15; }
__host__ __device__ inline WordLmCarve word_lm_carve(int tok_stride, int order) {
    const size_t maxw = ((size_t)tok_stride + 1) / 2;     // words of a row: every second token a delimiter
    const size_t pad = order - 1, clen = order > 2 ? order - 2 : 1;
    WordLmCarve c;
    c.score = 0;                                           // fp64 [maxw + 1]: the words' scores and </s>'s
    c.id = c.score + al((maxw + 1) * sizeof(double));      // int [pad + maxw + 1]: <s> pads, the words' ids, </s>
    c.ctx = c.id + al((maxw + pad + 1) * sizeof(int));     // int [pad + maxw][order - 2]: the contexts that start at a position
    c.tok = c.ctx + al((maxw + pad) * clen * sizeof(int)); // 16-bit [tok_stride]: the staged tokens
    c.start = c.tok + al((size_t)tok_stride * sizeof(unsigned short));      // 16-bit [maxw]: where each word starts
    c.misc = c.start + al(maxw * sizeof(unsigned short));  // int [2]: words, OOV words
    c.bytes = c.misc + 16;
    return c;
}

// grid (N, B), 256 threads; dynamic LDS: word_lm_lds_bytes(tok_stride, order).
__global__ __launch_bounds__(WL_THREADS) void nbest_word_lm_kernel(
    const int32_t* __restrict__ tokens, int tok_stride, const int32_t* __restrict__ len, const int32_t* __restrict__ count,
    int N, int B, int delimiter, pgasr_word_lm_tables tb, double* __restrict__ out_logp, int32_t* __restrict__ out_words,
    int32_t* __restrict__ out_oov) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wl_lds[];
    const int n = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const size_t row = (size_t)n * B + b;
    int cnt = count[b]; cnt = cnt < 0 ? 0 : (cnt > N ? N : cnt);
    if (n >= cnt) {                                        // workgroup-uniform
        if (tid == 0) { out_logp[row] = 0.0; out_words[row] = 0; out_oov[row] = 0; }
        return;
    }
    int L = len[row]; L = L < 0 ? 0 : (L > tok_stride ? tok_stride : L);
    const int order = tb.order, pad = order - 1, clen = order > 2 ? order - 2 : 0;

    const WordLmCarve cv = word_lm_carve(tok_stride, order);
    double* s_score = (double*)(wl_lds + cv.score);
    int* s_id = (int*)(wl_lds + cv.id);
    int* s_ctx = (int*)(wl_lds + cv.ctx);
    unsigned short* s_tok = (unsigned short*)(wl_lds + cv.tok);
    unsigned short* s_start = (unsigned short*)(wl_lds + cv.start);
    int* s_misc = (int*)(wl_lds + cv.misc);             // [0] words, [1] OOV words

    // 1. stage the tokens
    const int32_t* tk = tokens + row * (size_t)tok_stride;
    for (int i = tid; i < L; i += WL_THREADS) {
        const int t = tk[i];
        s_tok[i] = t == delimiter ? WL_DELIM : ((unsigned)t > 255u ? WL_BAD : (unsigned short)t);
    }
    if (tid == 0) { s_misc[0] = 0; s_misc[1] = 0; }
    __syncthreads();

    // 2. word starts: a token that is no delimiter and follows one (or the row's start)
    if (tid < 64) {
        int nw = 0;
        const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
        for (int c = 0; c < L; c += 64) {                  // wave-uniform
            const int i = c + lane;
            const bool st = i < L && s_tok[i] != WL_DELIM && (i == 0 || s_tok[i - 1] == WL_DELIM);
            const uint64_t m = __ballot(st);
            if (st) s_start[nw + __popcll(m & below)] = (unsigned short)i;
            nw += __popcll(m);
        }
        if (lane == 0) s_misc[0] = nw;
    }
    __syncthreads();
    const int nw = s_misc[0];                              // <= maxw: two starts are at least two tokens apart

    // 3. word ids
    for (int w = tid; w < nw + pad + 1; w += WL_THREADS) {
        int id;
        if (w < pad) id = WL_BOS;
        else if (w == nw + pad) id = WL_EOS;
        else {
            const int st = s_start[w - pad];
            uint32_t h = 2166136261u;
            int wl = 0;
            bool bad = false;
            for (; wl <= WL_MAX_WORD_LEN && st + wl < L; ++wl) {       // one token past the limit: a longer word is OOV
                const unsigned short t = s_tok[st + wl];
                if (t == WL_DELIM) break;
                bad = bad || t == WL_BAD;
                h = word_hash_step(h, (uint32_t)t);
            }
            id = WL_UNK;
            if (!bad && wl <= WL_MAX_WORD_LEN) {
                const uint32_t mask = (uint32_t)tb.word_cap - 1u;
                uint32_t s = word_hash_final(h) & mask;
                for (int step = 0; step < tb.word_cap; ++step) {
                    const int e = tb.word_slots[s];
                    if (e < WL_RESERVED || e >= tb.n_words) break;      // an empty slot (-1) ends the probe; anything else out of range too
                    const int off = tb.word_off[e], el = tb.word_off[e + 1] - off;
                    bool eq = el == wl && off >= 0 && off + el <= tb.pool_bytes;
                    for (int j = 0; eq && j < wl; ++j) eq = (unsigned short)tb.word_pool[off + j] == s_tok[st + j];
                    if (eq) { id = e; break; }
                    s = (s + 1u) & mask;
                }
            }
            if (id == WL_UNK) atomicAdd(&s_misc[1], 1);
        }
        s_id[w] = id;
    }
    __syncthreads();

    const NgramSlot* slots = (const NgramSlot*)tb.ngram_slots;
    // 4. the contexts that start at position p (positions: pad ids of <s>, the words, </s>; a context never holds </s>):
    //    s_ctx[p][m - 2] = the entry index of the m words from p on, m = 2 .. order-1, or -1 where it is not stored
    if (clen > 0) {
        for (int p = tid; p < nw + pad; p += WL_THREADS) {
            int e = s_id[p];                               // a unigram's entry index is its word id
            for (int m = 2; m <= order - 1; ++m) {
                if (e >= 0 && p + m - 1 < nw + pad) {
                    NgramSlot hit;
                    const int s = ngram_find(slots, tb.ngram_cap, e, s_id[p + m - 1], hit);
                    e = s < 0 ? -1 : tb.n_words + s;
                } else {
                    e = -1;
                }
                s_ctx[(size_t)p * clen + (m - 2)] = e;
            }
        }
    }
    __syncthreads();

    // 5. the score of the word at position q under the order-1 words before it
    for (int q = pad + tid; q < nw + pad + 1; q += WL_THREADS) {
        const int w = s_id[q];
        double acc = 0.0;
        bool found = false;
        for (int m = pad; m >= 1 && !found; --m) {
            const int p = q - m;
            const int h = m == 1 ? s_id[p] : s_ctx[(size_t)p * clen + (m - 2)];
            if (h < 0) continue;                           // the context is not stored: weight 0
            NgramSlot hit;
            if (ngram_find(slots, tb.ngram_cap, h, w, hit) >= 0) {
                acc += (double)hit.logp;
                found = true;
            } else if (h < tb.n_words) {
                acc += (double)tb.uni_bow[h];
            } else {
                acc += (double)slots[h - tb.n_words].bow;
            }
        }
        if (!found) acc += (double)tb.uni_logp[w];
        s_score[q - pad] = acc;
    }
    __syncthreads();

    // 6. the sentence: one addition per word in word order, then </s>
    if (tid == 0) {
        double total = 0.0;
        for (int i = 0; i <= nw; ++i) total += s_score[i];
        out_logp[row] = total;
        out_words[row] = nw;
        out_oov[row] = s_misc[1];
    }
}

__global__ __launch_bounds__(WL_NMAX) void nbest_combine_rank_kernel(
    const double* __restrict__ base, const double* __restrict__ word_logp, const int32_t* __restrict__ n_words,
    const int32_t* __restrict__ count, int N, int B, double word_alpha, double word_beta, double* __restrict__ out_total,
    int32_t* __restrict__ out_order) {
    __shared__ double s_total[WL_NMAX];
    const int b = blockIdx.x, tid = threadIdx.x;
    int cnt = count[b]; cnt = cnt < 0 ? 0 : (cnt > N ? N : cnt);
    if (tid < N) {
        double total = INFINITY;
        const double a = base[(size_t)tid * B + b];
        if (tid < cnt && std::isfinite(a)) {
            // plain operators under contract(off): see csrc/nbest.hip
#pragma clang fp contract(off)
            const double t2 = word_alpha * word_logp[(size_t)tid * B + b], t3 = word_beta * (double)n_words[(size_t)tid * B + b];
            total = (a + -t2) + -t3;
            if (total != total) total = INFINITY;
        }
        s_total[tid] = total;
        out_total[(size_t)tid * B + b] = total;
    }
    __syncthreads();
    if (tid < N) {
        int rank = tid;                                    // rows beyond count follow in index order
        if (tid < cnt) {
            const double mine = s_total[tid];
            rank = 0;
            for (int m = 0; m < cnt; ++m) {
                const double x = s_total[m];
                rank += (x < mine || (x == mine && m < tid)) ? 1 : 0;
            }
        }
        out_order[(size_t)b * N + rank] = tid;
    }
}

bool is_pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }

}  // namespace

extern "C" int pgasr_nbest_word_lm_score(const int32_t* tokens, int tok_stride, const int32_t* len, const int32_t* count,
                                         int N, int B, int delimiter, const pgasr_word_lm_tables* tables,
                                         double* out_word_logp, int32_t* out_n_words, int32_t* out_n_oov, void* stream) {
    if (!tables) return PGASR_ERR_INVALID_ARG;
    const pgasr_word_lm_tables tb = *tables;               // host memory: read here, passed to the kernel by value
    if (tb.order < 1 || tb.order > WL_MAX_ORDER || N < 1 || N > WL_NMAX || tok_stride > WL_MAX_STRIDE) return PGASR_ERR_UNSUPPORTED;
    if (tb.n_words > (1 << 22) || tb.ngram_cap > (1 << 25)) return PGASR_ERR_UNSUPPORTED;        // 2^24 n-grams at load 0.5
    if (!tokens || !len || !count || !out_word_logp || !out_n_words || !out_n_oov || B < 1 || tok_stride < 1)
        return PGASR_ERR_INVALID_ARG;
    if (!tb.word_pool || !tb.word_off || !tb.word_slots || !tb.uni_logp || !tb.uni_bow || !tb.ngram_slots) return PGASR_ERR_INVALID_ARG;
    if (tb.n_words < WL_RESERVED || tb.pool_bytes < 0 || !is_pow2(tb.word_cap) || !is_pow2(tb.ngram_cap)) return PGASR_ERR_INVALID_ARG;
    if ((long long)(tb.n_words - WL_RESERVED) * 2 > (long long)tb.word_cap) return PGASR_ERR_INVALID_ARG;     // load factor <= 0.5
    if ((long long)(tb.n_words - WL_RESERVED) * WL_MAX_WORD_LEN < (long long)tb.pool_bytes) return PGASR_ERR_INVALID_ARG;
    PGASR_LAUNCH_KERNEL(nbest_word_lm_kernel, dim3(N, B), dim3(WL_THREADS), word_lm_carve(tok_stride, tb.order).bytes,
                       (hipStream_t)stream, tokens, tok_stride, len, count, N, B, delimiter, tb, out_word_logp, out_n_words,
                       out_n_oov);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

extern "C" int pgasr_nbest_combine_rank(const double* base, const double* word_logp, const int32_t* n_words, const int32_t* count,
                                        int N, int B, double word_alpha, double word_beta, double* out_total, int32_t* out_order,
                                        void* stream) {
    if (N < 1 || N > WL_NMAX) return PGASR_ERR_UNSUPPORTED;
    if (!base || !word_logp || !n_words || !count || !out_total || !out_order || B < 1) return PGASR_ERR_INVALID_ARG;
    if (!std::isfinite(word_alpha) || !std::isfinite(word_beta)) return PGASR_ERR_INVALID_ARG;
    PGASR_LAUNCH_KERNEL(nbest_combine_rank_kernel, dim3(B), dim3(WL_NMAX), 0, (hipStream_t)stream, base, word_logp, n_words, count,
                       N, B, word_alpha, word_beta, out_total, out_order);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
