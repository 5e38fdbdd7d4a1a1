// Slot masses of edit-operation strings for gfx950 (pgasr_edit_ops_slot_mass; semantics in include/pgasr_hip.h, section
// A10-CONF): per group of pairs that share one side (the pivot), the weight of the pairs whose alignment has a hit, a
// substitution or the side's own gap operation on each position of that side, and the weighted number of the other side's
// unpartnered symbols in each gap between positions.  With the N-best list against its chosen row and the list's posterior as the
// weights this is the N-best confidence of Wessel et al. (IEEE Trans. SAP 9(3), 2001).
//
// One workgroup of 512 threads per group; the group's four accumulator rows of slots + 1 doubles live in LDS (sized from `slots`:
// 36 bytes per cell with the gap-count row, 144 KB at the limit of 4095).
//   (A) slot counts: wave v counts the slot-consuming operations of pairs v, v + 8, ..; the first participating pair's count is
//       n_slots, a participating pair with another count (or one above `slots`) is left out.
//   (B) the pairs in ascending order, which IS the order of the additions in every cell.  The operation string goes through in
//       chunks of one operation per thread; two ballots per wave and the waves' totals through LDS (double buffered: one barrier a
//       chunk) give every operation the number of slot-consuming and of "other" operations in front of it.  A slot-consuming
//       operation is the only one of its pair on its slot, so its thread adds the weight into the slot's cell without a conflict
//       and records E[slot], the "other" operations in front of it.  Behind a barrier the thread of gap j forms k = E[j] - E[j-1]
//       (the last gap: total - E[n_slots-1]) and adds w * k once: several insertions in one gap never meet in one cell.
//   (C) the rows are copied out whole, zeros included: the caller initialises nothing.
// fp64 under contract(off), no floating-point atomics; the result is a pure function of the inputs.
#include "common.h"
#include <cmath>

namespace {

constexpr int SM_THREADS = 512;
constexpr int SM_WAVES = SM_THREADS / 64;
constexpr int SM_MAX_OPS = 8190;
constexpr int SM_MAX_SLOTS = 4095;
constexpr int SM_MAX_PER_GROUP = 128;

inline size_t sm_lds_bytes(int slots) { return (size_t)(slots + 1) * (4 * sizeof(double) + sizeof(int32_t)); }

__global__ __launch_bounds__(SM_THREADS) void edit_ops_slot_mass_kernel(
    const int8_t* __restrict__ ops, const int32_t* __restrict__ n_ops, int ops_stride, const double* __restrict__ weight,
    int per_group, int side, int slots, double* __restrict__ mass, int32_t* __restrict__ n_slots, int32_t* __restrict__ left_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_lds[];
    const int S1 = slots + 1;
    double* acc = reinterpret_cast<double*>(sm_lds);                    // [4][S1]
    int32_t* E = reinterpret_cast<int32_t*>(acc + (size_t)4 * S1);      // [S1]
    __shared__ int s_count[SM_MAX_PER_GROUP];                            // slot count of a pair, -1: takes no part
    __shared__ uint32_t s_tot[2][SM_WAVES];                              // per wave: slot-consuming | other << 16 of a chunk

    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int own = side == 0 ? 2 : 3, other = side == 0 ? 3 : 2;
    const size_t p0 = (size_t)g * per_group;

    for (int i = tid; i < 4 * S1; i += SM_THREADS) acc[i] = 0.0;

    // ---- (A) ----
    for (int n = wave; n < per_group; n += SM_WAVES) {
        const double w = weight[p0 + n];
        const int K = n_ops[p0 + n];
        int c = -1;
        if (std::isfinite(w) && w > 0.0 && K >= 0 && K <= ops_stride) {
            const int8_t* o = ops + (p0 + n) * (size_t)ops_stride;
            c = 0;
            for (int k = lane; k < K; k += 64) {
                const int op = o[k];
                c += (op >= 0 && op <= 3 && op != other) ? 1 : 0;
            }
#pragma unroll
            for (int x = 32; x > 0; x >>= 1) c += __shfl_xor(c, x, 64);
        }
        if (lane == 0) s_count[n] = c;
    }
    __syncthreads();
    int ns = -1, left = 0;
    for (int n = 0; n < per_group; ++n) {
        const int c = s_count[n];
        if (c < 0) continue;
        if (ns < 0) ns = c;
        left += (c != ns || c > slots) ? 1 : 0;
    }

    // ---- (B) ----
    int parity = 0;
    for (int n = 0; n < per_group; ++n) {
        const int c = s_count[n];
        if (c < 0 || c != ns || c > slots) continue;                    // workgroup-uniform
        const double w = weight[p0 + n];
        const int K = n_ops[p0 + n];
        const int8_t* o = ops + (p0 + n) * (size_t)ops_stride;
        int base_c = 0, base_o = 0;
        for (int k0 = 0; k0 < K; k0 += SM_THREADS) {
            const int k = k0 + tid;
            const int op = k < K ? (int)o[k] : -1;
            const bool is_o = op == other;
            const bool is_c = op >= 0 && op <= 3 && !is_o;
            const unsigned long long bc = __ballot(is_c), bo = __ballot(is_o);
            if (lane == 0) s_tot[parity][wave] = (uint32_t)__popcll(bc) | ((uint32_t)__popcll(bo) << 16);
            __syncthreads();
            uint32_t before = 0, all = 0;
#pragma unroll
            for (int v = 0; v < SM_WAVES; ++v) {
                const uint32_t t = s_tot[parity][v];
                before += v < wave ? t : 0u;
                all += t;
            }
            parity ^= 1;
            const unsigned long long below = (1ull << lane) - 1ull;
            if (is_c) {
                const int slot = base_c + (int)(before & 0xffffu) + __popcll(bc & below);
                const int ch = op == own ? 2 : op;
                double* cell = acc + (size_t)ch * S1 + slot;
                {
#pragma clang fp contract(off)
                    *cell = *cell + w;
                }
                E[slot] = base_o + (int)(before >> 16) + __popcll(bo & below);
            }
            base_c += (int)(all & 0xffffu);
            base_o += (int)(all >> 16);
        }
        __syncthreads();
        for (int j = tid; j <= ns; j += SM_THREADS) {
            const int hi = j < ns ? E[j] : base_o;
            const int kk = hi - (j > 0 ? E[j - 1] : 0);
            if (kk > 0) {
#pragma clang fp contract(off)
                const double term = w * (double)kk;
                double* cell = acc + (size_t)3 * S1 + j;
                *cell = *cell + term;
            }
        }
        __syncthreads();
    }

    // ---- (C) ----
    __syncthreads();
    double* out = mass + (size_t)g * 4 * S1;
    for (int i = tid; i < 4 * S1; i += SM_THREADS) out[i] = acc[i];
    if (tid == 0) { n_slots[g] = ns; left_out[g] = left; }
}

}  // namespace

extern "C" int pgasr_edit_ops_slot_mass(const int8_t* ops, const int32_t* n_ops, int ops_stride, const double* weight, int groups,
                                        int per_group, int side, int slots, double* mass, int32_t* n_slots, int32_t* left_out,
                                        void* stream) {
    if (!n_ops || !weight || !mass || !n_slots || !left_out) return PGASR_ERR_INVALID_ARG;
    if (groups < 1 || per_group < 1 || ops_stride < 0 || slots < 0 || (ops_stride > 0 && !ops)) return PGASR_ERR_INVALID_ARG;
    if (side != 0 && side != 1) return PGASR_ERR_INVALID_ARG;
    if (ops_stride > SM_MAX_OPS || slots > SM_MAX_SLOTS || per_group > SM_MAX_PER_GROUP) return PGASR_ERR_UNSUPPORTED;
    if ((long long)groups * per_group > 0x7fffffffLL) return PGASR_ERR_UNSUPPORTED;
    const size_t lds = sm_lds_bytes(slots);
    if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)edit_ops_slot_mass_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)lds) != hipSuccess)
        return PGASR_ERR_UNSUPPORTED;
    PGASR_LAUNCH_KERNEL(edit_ops_slot_mass_kernel, dim3(groups), dim3(SM_THREADS), lds, (hipStream_t)stream, ops, n_ops, ops_stride,
                        weight, per_group, side, slots, mass, n_slots, left_out);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
