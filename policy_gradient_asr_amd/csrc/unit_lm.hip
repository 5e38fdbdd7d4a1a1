// Second pass of a back-off unit n-gram model over N-best lists (include/pgasr_hip.h, A7-WIDE-LM; the model: lm.UnitNgramLM):
// lm_logp[n, b] = the fp64 sum, in index order, of (double)lp32(ctx(y_<i), y_i) over the hypothesis' tokens.  One thread per hypothesis
// walks its tokens as a state machine over the packed tables: the query from the current state (unit_lm.h), then the successor's next
// state -- no context is ever rebuilt.  Every loop is bounded: tokens by the clamped length, the chain by the order, a search by the
// list length (at most 10 halvings of 1023 successors).
#include "common.h"
#include "unit_lm.h"

namespace {

constexpr int UNIT_LM_THREADS = 64;
constexpr int UNIT_LM_NMAX = 128;

__global__ __launch_bounds__(UNIT_LM_THREADS) void nbest_unit_lm_kernel(
    const int32_t* __restrict__ tokens, int tok_stride, const int32_t* __restrict__ len, const int32_t* __restrict__ count,
    int N, int B, unit_lm::Tables t, double* __restrict__ out) {
    const int idx = blockIdx.x * UNIT_LM_THREADS + threadIdx.x;      // = n * B + b
    if (idx >= N * B) return;
    const int n = idx / B, b = idx - n * B;
    int cnt = count[b]; cnt = cnt < 0 ? 0 : (cnt > N ? N : cnt);
    double total = 0.0;
    if (n < cnt) {
        int L = len[idx]; L = L < 0 ? 0 : (L > tok_stride ? tok_stride : L);
        const int32_t* y = tokens + (size_t)idx * tok_stride;
        int state = t.start;
        for (int i = 0; i < L; ++i) {
            const int s = y[i];
            if (s < 0 || s >= t.V || s == t.blank) { total = -INFINITY; break; }      // no table word is read for it
            int next = 0;
            total = total + (double)unit_lm::query(t, state, s, &next);
            state = next;
        }
    }
    out[idx] = total;
}

}  // namespace

extern "C" int pgasr_nbest_unit_lm_score(const int32_t* tokens, int tok_stride, const int32_t* len, const int32_t* count,
                                         int N, int B, int V, int blank, const pgasr_unit_lm_tables* tables, double* out_lm_logp,
                                         void* stream) {
    // nothing below touches HIP until every check has passed
    if (N < 1 || N > UNIT_LM_NMAX || V > unit_lm::VMAX) return PGASR_ERR_UNSUPPORTED;
    if (!tokens || !len || !count || !out_lm_logp || B < 1 || tok_stride < 1 || V < 1 || blank < 0 || blank >= V) return PGASR_ERR_INVALID_ARG;
    if (const int st = unit_lm::check_tables(tables, V, blank, 0.0, 0.0)) return st;
    if ((long long)N * B > 0x7FFFFFFFll) return PGASR_ERR_UNSUPPORTED;
    unit_lm::Tables t;
    t.states = (const int4*)tables->states; t.succ = (const int4*)tables->succ;
    t.n_states = tables->n_states; t.n_succ = tables->n_succ; t.start = tables->start; t.order = tables->order;
    t.V = V; t.blank = blank;
    const int blocks = (N * B + UNIT_LM_THREADS - 1) / UNIT_LM_THREADS;
    PGASR_LAUNCH_KERNEL(nbest_unit_lm_kernel, dim3(blocks), dim3(UNIT_LM_THREADS), 0, (hipStream_t)stream, tokens, tok_stride, len, count,
                        N, B, t, out_lm_logp);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
