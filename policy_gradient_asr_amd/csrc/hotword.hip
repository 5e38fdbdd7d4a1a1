// Second pass of a hotword bias automaton over N-best lists (include/pgasr_hip.h, A7-BIAS; the builder and the host statement of
// the query: lm.HotwordBias): out[n, b] = the fp64 sum, in token order, of (double)bonus[q, y_i] along the state chain q_0 = 0,
// q_{i+1} = next[q_i, y_i] over the table's S * V words {int32 next; float bonus}.  A token outside [0, V) leaves the state and the sum
// as they are (the blank's column of the table is the identity with bonus 0, so the blank does too).
// The chain is serial by nature -- each step's address depends on the previous load -- so one lane walks one hypothesis.  Its tokens are
// staged HW_CHUNK at a time, one chunk ahead of the chain, so that the table gather is the only dependent load.  Every loop is bounded
// by the clamped length; a next outside [0, S) is taken as state 0, so every index stays below S V whatever the table holds.
#include "common.h"
#include "bias_table.h"
#include <cmath>

namespace {

constexpr int HW_THREADS = 64;
constexpr int HW_NMAX = 128;
constexpr int HW_VMAX = 1024;
constexpr int HW_CHUNK = 8;
using bias_table::BiasWord;

__global__ __launch_bounds__(HW_THREADS) void nbest_bias_kernel(
    const int32_t* __restrict__ tokens, int tok_stride, const int32_t* __restrict__ len, const int32_t* __restrict__ count,
    int N, int B, int V, const BiasWord* __restrict__ table, int S, double* __restrict__ out) {
    const int idx = blockIdx.x * HW_THREADS + threadIdx.x;      // = n * B + b
    if (idx >= N * B) return;
    const int n = idx / B, b = idx - n * B;
    int cnt = count[b]; cnt = cnt < 0 ? 0 : (cnt > N ? N : cnt);
    double total = 0.0;
    if (n < cnt) {
        int L = len[idx]; L = L < 0 ? 0 : (L > tok_stride ? tok_stride : L);
        const int32_t* y = tokens + (size_t)idx * tok_stride;
        int cur[HW_CHUNK], nxt[HW_CHUNK];
#pragma unroll
        for (int u = 0; u < HW_CHUNK; ++u) cur[u] = (u < L) ? y[u] : -1;
        int q = 0;
        for (int i = 0; i < L; i += HW_CHUNK) {
#pragma unroll
            for (int u = 0; u < HW_CHUNK; ++u) nxt[u] = (i + HW_CHUNK + u < L) ? y[i + HW_CHUNK + u] : -1;      // the next chunk, ahead of the chain
#pragma unroll
            for (int u = 0; u < HW_CHUNK; ++u) {
                const int s = cur[u];
                if ((unsigned)s < (unsigned)V) {                 // q < S and s < V: below S V words
                    const BiasWord w = table[(size_t)q * V + s];
                    total = total + (double)w.bonus;
                    q = ((unsigned)w.next < (unsigned)S) ? w.next : 0;
                }
            }
#pragma unroll
            for (int u = 0; u < HW_CHUNK; ++u) cur[u] = nxt[u];
        }
    }
    out[idx] = total;
}

}  // namespace

extern "C" int pgasr_nbest_bias_score(const int32_t* tokens, const int32_t* len, const int32_t* count, int N, int B, int tok_stride, int V,
                                      const void* bias_table, int bias_states, double* out, void* stream) {
    // nothing below touches HIP until every check has passed
    if (N < 1 || N > HW_NMAX || V > HW_VMAX) return PGASR_ERR_UNSUPPORTED;
    if (!tokens || !len || !count || !out || B < 1 || tok_stride < 1 || V < 1 || !bias_table::usable(bias_table, bias_states, V)) return PGASR_ERR_INVALID_ARG;
    if ((long long)N * B > 0x7FFFFFFFll) return PGASR_ERR_UNSUPPORTED;
    const int blocks = (N * B + HW_THREADS - 1) / HW_THREADS;
    PGASR_LAUNCH_KERNEL(nbest_bias_kernel, dim3(blocks), dim3(HW_THREADS), 0, (hipStream_t)stream, tokens, tok_stride, len, count, N, B, V,
                        (const BiasWord*)bias_table, bias_states, out);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
