// The n-gram table of lm.WordNgramLM (include/pgasr_hip.h, A7-WORDLM): 16-byte slots {ctx, word, logp, bow}, open addressing, at most
// half full.  Probed by the second pass over N-best lists (word_lm.hip) and by the word fusion of the beam search (beam.hip, WORDS = true).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace word_ngram {

constexpr int WL_MAX_ORDER = 5;
constexpr int WL_BOS = 0, WL_EOS = 1, WL_UNK = 2, WL_RESERVED = 3;

struct NgramSlot { int32_t ctx, word; float logp, bow; };             // 16 bytes, one load per probe

__device__ __forceinline__ uint64_t ngram_hash(uint32_t ctx, uint32_t word) {
    uint64_t x = ((uint64_t)ctx << 32) | (uint64_t)word;
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}

// The slot of the n-gram (ctx, word), or -1.  At most half the slots are taken, so an empty one ends every probe; the bound on the
// steps only keeps a damaged table from holding the thread.
__device__ __forceinline__ int ngram_find(const NgramSlot* __restrict__ slots, int cap, int ctx, int word, NgramSlot& out) {
    const uint32_t mask = (uint32_t)cap - 1u;
    uint32_t s = (uint32_t)ngram_hash((uint32_t)ctx, (uint32_t)word) & mask;
    for (int step = 0; step < cap; ++step) {
        const NgramSlot e = slots[s];
        if (e.ctx < 0) return -1;
        if (e.ctx == ctx && e.word == word) { out = e; return (int)s; }
        s = (s + 1u) & mask;
    }
    return -1;
}

}  // namespace word_ngram
