// The packed tables of lm.UnitNgramLM (include/pgasr_hip.h, A7-WIDE-LM) as the kernels see them: the host's check of the struct and
// the contractual query from a state.  Shared by beam_wide.hip (fusion in the wide search) and unit_lm.hip (the second pass).
#pragma once
#include "common.h"
#include <cmath>

namespace unit_lm {

constexpr int ORDER_MAX = 5;
constexpr int VMAX = 1024;
constexpr int NGRAMS_MAX = 1 << 24;

// no HIP call.  The weights are the search's; the second pass gives zeros.
inline int check_tables(const pgasr_unit_lm_tables* t, int V, int blank, double alpha, double beta) {
    if (!t || !t->states || !t->succ) return PGASR_ERR_INVALID_ARG;
    if (t->order < 1 || t->order > ORDER_MAX || t->vocab > VMAX || t->n_succ > NGRAMS_MAX || t->n_states > NGRAMS_MAX + 1) return PGASR_ERR_UNSUPPORTED;
    if (t->vocab != V || t->blank != blank || t->n_states < 1 || t->n_succ < V - 1 || t->start < 0 || t->start >= t->n_states)
        return PGASR_ERR_INVALID_ARG;
    if (!std::isfinite(alpha) || !std::isfinite(beta)) return PGASR_ERR_INVALID_ARG;
    return PGASR_OK;
}

struct Tables {
    const int4* states;      // {bow bits, back-off state, first successor, one past the last}; state 0 = the empty context
    const int4* succ;        // {symbol, logp bits, next state, 0}
    int n_states, n_succ, start, order, V, blank;
};

// lp32(state, s) for a symbol 0 <= s < V other than the blank, and the state after it: acc = 0.0; from the state down its back-off chain,
// the first state that lists s returns float32(acc + (double)logp), every state passed adds (double)bow.  At most ORDER_MAX states, a
// binary search of at most 10 steps in each (the empty context lists every symbol but the blank: indexed).  -inf / state 0 if no state
// lists s, which a model the host has checked cannot do.
__device__ __forceinline__ float query(const Tables& t, int state, int s, int* next) {
    double acc = 0.0;
    int h = (state < 0 || state >= t.n_states) ? 0 : state;
    for (int d = 0; d < ORDER_MAX; ++d) {
        const int4 rec = t.states[h];
        int lo = rec.z < 0 ? 0 : rec.z, hi = rec.w > t.n_succ ? t.n_succ : rec.w;
        int at = -1;
        if (h == 0) {
            const int i = lo + s - (s > t.blank ? 1 : 0);
            if (i < hi) at = i;
        } else {
            for (int it = 0; it < 11 && lo < hi; ++it) {
                const int mid = (lo + hi) >> 1;
                const int sym = t.succ[mid].x;
                if (sym == s) { at = mid; break; }
                if (sym < s) lo = mid + 1; else hi = mid;
            }
        }
        if (at >= 0) {
            const int4 e = t.succ[at];
            if (e.x == s) { *next = e.z; return (float)(acc + (double)__int_as_float(e.y)); }
        }
        if (h == 0) break;
        acc = acc + (double)__int_as_float(rec.x);
        h = (rec.y < 0 || rec.y >= t.n_states) ? 0 : rec.y;
    }
    *next = 0;
    return -INFINITY;
}

}  // namespace unit_lm
