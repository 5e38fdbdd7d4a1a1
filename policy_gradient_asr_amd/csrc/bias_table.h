// The dense hotword automaton of lm.HotwordBias (include/pgasr_hip.h, A7-BIAS): S * V 8-byte words, word (q, s) at q V + s.
// Read by both beam searches (beam.hip, beam_wide.hip) and by the second pass over N-best lists (hotword.hip).
#pragma once
#include <cstdint>

namespace bias_table {

struct BiasWord { int32_t next; float bonus; };
static_assert(sizeof(BiasWord) == 8, "a table word is 8 bytes");
constexpr long long BIAS_MAX_WORDS = 1ll << 24;      // S * V words (128 MiB)

// a usable table (no HIP call); a finite weight is the searches' own check
inline bool usable(const void* table, int states, int V) {
    return table && states >= 1 && (long long)states * V <= BIAS_MAX_WORDS;
}

}  // namespace bias_table
