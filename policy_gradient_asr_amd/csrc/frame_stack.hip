// Low-frame-rate input (Sak et al. 2015; Pundak & Sainath 2016) for gfx950: stack `stack` neighbouring frames of a feature batch and
// keep every `skip`-th one (pgasr_frame_stack; the function is stated in include/pgasr_hip.h, section A0-LFR, and in numpy in
// tests/frame_stack_ref.py).  Pure data movement: no arithmetic on a value, so the result equals the numpy statement bit for bit.
//
// Time is the contiguous axis of x (B,F,T) and of out (B,stack*F,Tout), and an output row reads its input row at stride `skip`.  That
// read never goes to memory as such.  One 256-thread workgroup takes FS_TILE = 64 output frames of FS_ROWS = 8 feature rows of one
// utterance:
//   1. it stages the input span of the tile, (live - 1) * skip + stack frames of each row from frame t0 * skip - left on, in LDS with
//      loads coalesced along t -- one wave per row, 16-byte loads where T % 4 == 0 and x is 16-byte aligned (every row start then
//      is, and the span is begun at the multiple of 4 below its first frame), one float per lane otherwise.  The clamp of the
//      contract is applied HERE: LDS word i holds x[b, f, clamp(first + i, 0, n - 1)], so the edges replicate the first / last real
//      frame and a frame at or beyond n is never read (a 16-byte load is taken only where all four frames lie in [0, n)).
//   2. after one barrier every (row, offset j) pair is one wave's store of 64 consecutive t' (256 bytes) to out[b, j*F + f, t0 ..]:
//      lane l reads LDS word l * skip + j.  Each input word comes from HBM once per tile, plus the halo of stack - skip frames where
//      stack > skip, not `stack` times.  (The LDS read is at stride skip: free of bank conflicts for odd skip, 2- to 16-way for even
//      skip; NOTES.md 0.41 has what the kernel reaches at skip 3.)
//   Frames t' >= n' = ceil(n / skip) are written as 0.0f; a tile that lies wholly there stages nothing and has no barrier.
//   The workgroups of the first row block also write fmask_out and n_out.  Dynamic LDS: FS_ROWS * pitch floats, pitch = the span of
//   a full tile rounded up to 4 (at most 8 * 1028 * 4 = 32896 bytes at skip = stack = 16; 6272 bytes at (3,3)).  No scratch.
#include "common.h"

namespace {

constexpr int FS_THREADS = 256;
constexpr int FS_TILE = 64;       // output frames per workgroup: one wave-wide store per (row, offset)
constexpr int FS_ROWS = 8;        // feature rows per workgroup
constexpr int FS_MAX = 16;        // stack, skip

__host__ __device__ constexpr int fs_pitch(int stack, int skip) { return ((FS_TILE - 1) * skip + stack + 3 + 3) & ~3; }

template <bool VEC>
__global__ __launch_bounds__(FS_THREADS) void frame_stack_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ n_frames, int F, int T, int stack, int skip, int left, int Tout,
    float* __restrict__ out, float* __restrict__ fmask_out, int32_t* __restrict__ n_out) {
    extern __shared__ float4 fs_lds4[];                  // 16-byte aligned base
    float* lds = (float*)fs_lds4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, f0 = blockIdx.y * FS_ROWS, t0 = blockIdx.x * FS_TILE;
    int n = n_frames[b];
    n = n < 0 ? 0 : (n > T ? T : n);
    const int np = (n + skip - 1) / skip;                // n' = ceil(n / skip) <= Tout
    const int rows = F - f0 < FS_ROWS ? F - f0 : FS_ROWS;
    const int cols = Tout - t0 < FS_TILE ? Tout - t0 : FS_TILE;          // output frames of this tile, >= 1
    const int live = np - t0 < cols ? np - t0 : cols;                    // .. of which the first `live` are real (may be <= 0)
    const int pitch = fs_pitch(stack, skip);

    if (blockIdx.y == 0) {
        if (fmask_out && tid < cols) fmask_out[(size_t)b * Tout + t0 + tid] = tid < live ? 1.f : 0.f;
        if (n_out && blockIdx.x == 0 && tid == 0) n_out[b] = np;
    }

    const int first = t0 * skip - left;                  // the input frame of tap 0 of output frame t0; may be negative
    const int base = VEC ? (first & ~3) : first;         // the frame LDS word 0 stands for (floor to a multiple of 4)
    const int shift = first - base;
    if (live > 0) {                                      // the same in every thread of the workgroup; here n >= 1
        const int need = (live - 1) * skip + stack + shift;              // words of the span, <= pitch
        for (int r = wave; r < rows; r += FS_THREADS / 64) {
            const float* xr = x + ((size_t)b * F + f0 + r) * (size_t)T;
            float* lr = lds + r * pitch;
            if (VEC) {
                for (int q = lane; 4 * q < need; q += 64) {
                    const int g = base + 4 * q;
                    float4 v;
                    if (g >= 0 && g + 3 < n) {
                        v = *(const float4*)(xr + g);
                    } else {
                        const int g0 = g < 0 ? 0 : (g < n ? g : n - 1), g1 = g + 1 < 0 ? 0 : (g + 1 < n ? g + 1 : n - 1);
                        const int g2 = g + 2 < 0 ? 0 : (g + 2 < n ? g + 2 : n - 1), g3 = g + 3 < 0 ? 0 : (g + 3 < n ? g + 3 : n - 1);
                        v.x = xr[g0]; v.y = xr[g1]; v.z = xr[g2]; v.w = xr[g3];
                    }
                    *(float4*)(lr + 4 * q) = v;
                }
            } else {
                for (int q = lane; q < need; q += 64) {
                    const int g = base + q;
                    lr[q] = xr[g < 0 ? 0 : (g < n ? g : n - 1)];
                }
            }
        }
        __syncthreads();
    }

    if (lane < cols) {
        const int pairs = rows * stack;
        for (int p = wave; p < pairs; p += FS_THREADS / 64) {
            const int r = p / stack, j = p - r * stack;
            const float v = lane < live ? lds[r * pitch + shift + lane * skip + j] : 0.f;
            out[(((size_t)b * stack + j) * F + f0 + r) * (size_t)Tout + t0 + lane] = v;
        }
    }
}

}  // namespace

extern "C" int pgasr_frame_stack(const float* x, const int32_t* n_frames, int B, int F, int T, int stack, int skip, int left,
                                 int Tout, float* out, float* fmask_out, int32_t* n_out, void* stream) {
    if (!x || !n_frames || !out || (const float*)out == x) return PGASR_ERR_INVALID_ARG;
    if (B < 1 || F < 1 || T < 1) return PGASR_ERR_INVALID_ARG;
    if (stack < 1 || stack > FS_MAX || skip < 1 || skip > FS_MAX || left < 0 || left >= stack) return PGASR_ERR_INVALID_ARG;
    if ((long long)stack * F > 65535 || B > 65535) return PGASR_ERR_INVALID_ARG;
    if (Tout != (T + skip - 1) / skip) return PGASR_ERR_INVALID_ARG;
    const dim3 grid((unsigned)((Tout + FS_TILE - 1) / FS_TILE), (unsigned)((F + FS_ROWS - 1) / FS_ROWS), (unsigned)B);
    const size_t lds = (size_t)FS_ROWS * fs_pitch(stack, skip) * sizeof(float);
    const bool vec = T % 4 == 0 && ((uintptr_t)x & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        PGASR_LAUNCH_KERNEL(frame_stack_kernel<true>, grid, dim3(FS_THREADS), lds, st, x, n_frames, F, T, stack, skip, left, Tout,
                            out, fmask_out, n_out);
    else
        PGASR_LAUNCH_KERNEL(frame_stack_kernel<false>, grid, dim3(FS_THREADS), lds, st, x, n_frames, F, T, stack, skip, left, Tout,
                            out, fmask_out, n_out);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
