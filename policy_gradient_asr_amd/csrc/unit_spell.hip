// Spelling subword-unit rows into character rows (gfx950): pgasr_unit_spell (include/pgasr_hip.h, A11-SPELL).
//
// A subword unit may hold a space, so a row of units has no word boundaries and its edit distance is not the character or word
// distance of the text.  The spelled row -- the units' character ids, concatenated -- is a row over at most 64 symbols, which every
// narrow kernel (word ids, edit distance, pair distances, edit operations) takes as it is.
//
// One wave per row, PGASR_SPELL_ROWS rows per workgroup.  The wave walks its row in chunks of 64 units: lane l loads unit c + l and
// the two offsets of its spelling, an inclusive wave scan of the spelling lengths gives every unit's start inside the chunk's span,
// and the row position reached so far is carried in a wave-uniform register.  The span is then written by OUTPUT position: lane l of
// pass o owns character o + l of the span, finds its unit by a six-step binary search over the 64 scan values (cross-lane reads, no
// LDS) and loads its character from the pool.  Passes start at a multiple of 64 characters of the row, so consecutive lanes store
// consecutive words of one 256-byte line whatever the units' lengths are; no lane writes its unit's characters as a burst of its own.
// The tail out[out_len .. out_stride) is zeroed with 16-byte stores where the address allows.  The pool (16 KB for 1024 units) is
// read through the read-only path and stays in L2.  No workspace, no atomics, no LDS, deterministic.
#include "common.h"

namespace {

constexpr int SPELL_ROWS = 4;      // rows (waves) per workgroup

__global__ __launch_bounds__(64 * SPELL_ROWS) void unit_spell_kernel(
    const int32_t* __restrict__ tokens, const int32_t* __restrict__ lengths, int stride, int N,
    const int32_t* __restrict__ spell_off, const int32_t* __restrict__ spell_chars, int V,
    int32_t* __restrict__ out, int out_stride, int32_t* __restrict__ out_len, int32_t* __restrict__ full_len, int vec_ok) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * SPELL_ROWS + (threadIdx.x >> 6);
    if (n >= N) return;                                   // whole waves leave: no barrier below
    int len = lengths[n];
    len = len < 0 ? 0 : (len > stride ? stride : len);
    const int32_t* row = tokens + (size_t)n * stride;
    int32_t* orow = out + (size_t)n * out_stride;
    int base = 0;                                         // characters before this chunk (wave-uniform)
    for (int c = 0; c < len; c += 64) {
        const int i = c + lane;
        const int id = i < len ? row[i] : -1;
        int a = 0, l = 0;
        if (id >= 0 && id < V) {
            a = __ldg(spell_off + id);
            l = __ldg(spell_off + id + 1) - a;
            l = l < 0 ? 0 : (l > PGASR_SPELL_MAX_UNIT_CHARS ? PGASR_SPELL_MAX_UNIT_CHARS : l);
        }
        int incl = l;                                     // inclusive scan of the spelling lengths
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        const int excl = incl - l;
        const int total = __shfl(incl, 63, 64);
        // the part of the span [base, base + total) that lies inside the row
        const int room = out_stride - base;
        const int wtotal = room <= 0 ? 0 : (total < room ? total : room);
        for (int o = wtotal > 0 ? -(base & 63) : 0; o < wtotal; o += 64) {   // every lane runs every pass (the cross-lane reads need them all)
            const int p = o + lane;
            const bool mine = p >= 0 && p < wtotal;
            const int q = mine ? p : 0;
            int u = 0;                                    // units whose span ends at or before q: the first u with incl[u] > q
#pragma unroll
            for (int s = 32; s > 0; s >>= 1)
                if (__shfl(incl, u + s - 1, 64) <= q) u += s;
            u = u > 63 ? 63 : u;
            const int ua = __shfl(a, u, 64), ue = __shfl(excl, u, 64);
            if (mine) orow[base + p] = __ldg(spell_chars + ua + (q - ue));
        }
        base += total;
    }
    const int olen = base < out_stride ? base : out_stride;
    if (lane == 0) {
        out_len[n] = olen;
        if (full_len) full_len[n] = base;
    }
    // the zero tail: single words up to a 16-byte boundary, whole 16-byte stores, single words again
    size_t e = (size_t)n * out_stride + olen;
    const size_t e1 = (size_t)n * out_stride + out_stride;
    if (vec_ok) {
        size_t ea = (e + 3) & ~(size_t)3;
        if (ea > e1) ea = e1;
        if (e + lane < ea) out[e + lane] = 0;
        const size_t eb = e1 & ~(size_t)3;
        int4* o4 = reinterpret_cast<int4*>(out);
        for (size_t v = ea / 4 + lane; v < eb / 4; v += 64) o4[v] = make_int4(0, 0, 0, 0);
        e = eb > ea ? eb : ea;
    }
    for (size_t p = e + lane; p < e1; p += 64) out[p] = 0;
}

}  // namespace

extern "C" int pgasr_unit_spell(const int32_t* tokens, const int32_t* lengths, int stride, int N,
                                const int32_t* spell_off, const int32_t* spell_chars, int V,
                                int32_t* out, int out_stride, int32_t* out_len, int32_t* full_len, void* stream) {
    if (N <= 0 || stride < 0 || out_stride < 0 || V < 1) return PGASR_ERR_INVALID_ARG;
    if (!lengths || !spell_off || !out_len) return PGASR_ERR_INVALID_ARG;
    if ((stride > 0 && !tokens) || (out_stride > 0 && !out)) return PGASR_ERR_INVALID_ARG;
    if (!spell_chars && stride > 0) return PGASR_ERR_INVALID_ARG;
    if (stride > (1 << 24)) return PGASR_ERR_UNSUPPORTED;           // full_len <= stride * PGASR_SPELL_MAX_UNIT_CHARS stays an int32
    const int vec_ok = ((uintptr_t)out & 15u) == 0 ? 1 : 0;
    PGASR_LAUNCH_KERNEL(unit_spell_kernel, dim3((N + SPELL_ROWS - 1) / SPELL_ROWS), dim3(64 * SPELL_ROWS), 0, (hipStream_t)stream,
                        tokens, lengths, stride, N, spell_off, spell_chars, V, out, out_stride, out_len, full_len, vec_ok);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
