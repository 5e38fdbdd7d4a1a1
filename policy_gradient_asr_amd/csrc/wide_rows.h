// One (t,b) row of up to 1024 fp32 scores held by ONE wave: lane l owns the NV consecutive labels l*NV .. l*NV + NV - 1 in
// registers, NV = ceil(V / 64) rounded up to a power of two in {1, 2, 4, 8, 16}.  Used by the wide kernels only
// (wide_vocab.hip and the wide gradient pass of ctc.hip); the kernels for V <= 64 hold one label per lane and do not use it.
#pragma once
#include "common.h"

constexpr int PGASR_WIDE_VMAX = 1024;

// the compile-time NV for a row of V labels
#define PGASR_WIDE_DISPATCH(V, CALL)                        \
    do {                                                    \
        const int nv__ = ((V) + 63) / 64;                   \
        if (nv__ <= 1) { CALL(1); }                         \
        else if (nv__ <= 2) { CALL(2); }                    \
        else if (nv__ <= 4) { CALL(4); }                    \
        else if (nv__ <= 8) { CALL(8); }                    \
        else { CALL(16); }                                  \
    } while (0)

// Rows are V floats apart, so a row is aligned for W-float vector accesses only when V % W == 0 and the tensor is: decided once per
// launch on the host (`vec`), uniform over the grid.  W = min(NV, 4).
template <int NV> constexpr int wide_vec_width() { return NV >= 4 ? 4 : NV; }
template <int NV> inline bool wide_vec_ok(const void* a, const void* b, int V) {
    constexpr int W = wide_vec_width<NV>();
    return W > 1 && V % W == 0 && ((uintptr_t)a % (W * sizeof(float))) == 0 && ((uintptr_t)b % (W * sizeof(float))) == 0;
}

// v[i] = row[lane*NV + i], `fill` past V.  With vec every W-float chunk lies wholly inside or wholly outside the row (V % W == 0).
template <int NV>
__device__ __forceinline__ void wide_row_load(const float* __restrict__ row, int V, int lane, bool vec, float fill, float (&v)[NV]) {
    constexpr int W = wide_vec_width<NV>();
    const int v0 = lane * NV;
    if constexpr (W == 4) {
        if (vec) {
#pragma unroll
            for (int c = 0; c < NV; c += 4) {
                float4 q = make_float4(fill, fill, fill, fill);
                if (v0 + c + 4 <= V) q = *reinterpret_cast<const float4*>(row + v0 + c);
                v[c] = q.x; v[c + 1] = q.y; v[c + 2] = q.z; v[c + 3] = q.w;
            }
            return;
        }
    } else if constexpr (W == 2) {
        if (vec) {
            float2 q = make_float2(fill, fill);
            if (v0 + 2 <= V) q = *reinterpret_cast<const float2*>(row + v0);
            v[0] = q.x; v[1] = q.y;
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = (v0 + i < V) ? row[v0 + i] : fill;
}

// The wide samplers' rule for a draw n that fell on a label whose e = exp(score - max) is 0 (frame_ops.hip: sample_skip_zero): n
// stays where e_n > 0; otherwise the nearest label above it with e > 0, or the last such label if there is none above.  pm: bit i
// set where the lane's label lane*NV + i has e > 0; n is uniform over the wave.  The usual case costs one ballot; the rest (about
// one draw in 2^24) two butterflies behind a wave-uniform branch.
template <int NV>
__device__ __forceinline__ int wide_sample_skip_zero(int n, unsigned pm, int lane) {
    const int own = n / NV, sub = n % NV;
    if (__ballot(lane == own && ((pm >> sub) & 1u))) return n;
    const unsigned above = lane > own ? pm : (lane == own ? pm & (~0u << sub) : 0u);
    int lo = above ? lane * NV + __ffs((int)above) - 1 : 0x7fffffff;
    int hi = pm ? lane * NV + 31 - __clz((int)pm) : -1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, 64));
        hi = max(hi, __shfl_xor(hi, o, 64));
    }
    return lo != 0x7fffffff ? lo : (hi >= 0 ? hi : n);
}

// row[lane*NV + i] = v[i] for the labels inside the row
template <int NV>
__device__ __forceinline__ void wide_row_store(float* __restrict__ row, int V, int lane, bool vec, const float (&v)[NV]) {
    constexpr int W = wide_vec_width<NV>();
    const int v0 = lane * NV;
    if constexpr (W == 4) {
        if (vec) {
#pragma unroll
            for (int c = 0; c < NV; c += 4)
                if (v0 + c + 4 <= V) *reinterpret_cast<float4*>(row + v0 + c) = make_float4(v[c], v[c + 1], v[c + 2], v[c + 3]);
            return;
        }
    } else if constexpr (W == 2) {
        if (vec) {
            if (v0 + 2 <= V) *reinterpret_cast<float2*>(row + v0) = make_float2(v[0], v[1]);
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i)
        if (v0 + i < V) row[v0 + i] = v[i];
}
