// Word ids for the word-level (WER) reward, and the multi-sample rewards with a separate normaliser (gfx950).
//
// pgasr_word_ids: one wave per (reference, hypothesis) pair.  A word is a maximal run of tokens between delimiters, exactly
// str.split(d) on the token row: n delimiters give n + 1 words, empty ones included.  The kernel gives every word of the pair
// the id 1 + (index of its first occurrence in ref words ++ hyp words), so that pgasr_edit_distance on the id rows is the word
// edit distance.  Everything lives in the workgroup's LDS:
//   1. the pair's tokens are copied to LDS (ref at 0, hyp after it);
//   2. per 64-token chunk a ballot over "token == d" and its popcounts give each token's word and its offset in that word; a
//      delimiter records where the next word starts, every other token adds mix(token, offset) to its word's fingerprint
//      (an LDS integer atomic: the sum does not depend on the order);
//   3. lanes run over the words in index order, 64 at a time, against an open-addressing table of the words seen so far (one
//      entry per distinct word: its index + 1), keyed by (length, fingerprint).  A key match is only a candidate: equality is
//      confirmed on the tokens in LDS (per lane for short words, by the whole wave 64 tokens at a time for long ones), and a
//      failed confirmation probes on.  Lanes with no earlier match compare with the earlier lanes of their chunk (lane order,
//      so the first occurrence wins); what is still new is inserted.  The table holds the first occurrence of each distinct
//      word, so the ids do not depend on the table's layout (which the insertion race may change).
// Deterministic, no workspace, no host sync.
#include "common.h"

namespace {

constexpr int WORD_SHORT = 16;     // words up to this length are confirmed by their own lane

__device__ __forceinline__ uint32_t word_mix(uint32_t tok, uint32_t off) {
    uint32_t h = tok * 0x9E3779B1u ^ (off + 0x7F4A7C15u) * 0x85EBCA77u;   // murmur3's finaliser on (token, offset)
    h ^= h >> 16; h *= 0x85EBCA6Bu;
    h ^= h >> 13; h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

__device__ __forceinline__ int popc64(uint64_t m) { return __popcll(m); }

// Every lane with `want` set compares tok[a .. a+len) with tok[b .. b+len); returns the result on those lanes.  Call with the whole
// wave (the long words are compared cooperatively).
__device__ bool words_equal(bool want, int a, int b, int len, const int32_t* tok, int lane) {
    bool eq = true;
    if (want && len <= WORD_SHORT) {
        for (int i = 0; i < len; ++i)
            if (tok[a + i] != tok[b + i]) { eq = false; break; }
    }
    uint64_t longm = __ballot(want && len > WORD_SHORT);
    while (longm) {
        const int l = __ffsll((unsigned long long)longm) - 1;
        longm &= longm - 1;
        const int la = __shfl(a, l, 64), lb = __shfl(b, l, 64), n = __shfl(len, l, 64);
        bool diff = false;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            if (i < n && tok[la + i] != tok[lb + i]) diff = true;
            if (__any(diff)) break;
        }
        const bool same = !__any(diff);
        if (lane == l) eq = same;
    }
    return eq;
}

// LDS layout for strides (Rs, Hs): tokens int32[Rs + Hs] | word (start | len << 16) u32[Rs + Hs + 2] | fingerprint u32[same] |
// table u32[S], S = the power of two >= 2 (Rs + Hs + 2).
__host__ __device__ inline int word_table_size(int max_words) {
    int s = 64;
    while (s < 2 * max_words) s <<= 1;
    return s;
}
inline size_t word_lds_bytes(int Rs, int Hs) {
    const int W = Rs + Hs + 2;
    return 4 * ((size_t)(Rs + Hs) + 2 * (size_t)W + (size_t)word_table_size(W));
}

// Splits n tokens (already in tok[tb ..]) into words wb, wb+1, ..: start/len packed into winfo, fingerprints into wfp (zeroed by
// the caller).  Returns the word count (delimiters + 1).
__device__ int split_words(const int32_t* tok, int tb, int n, int d, int wb, uint32_t* winfo, uint32_t* wfp, int lane) {
    int nd = 0, wstart = tb;           // delimiters so far, start of the current word (absolute LDS token index)
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int c = 0; c < n; c += 64) {
        const int p = c + lane;
        const int t = p < n ? tok[tb + p] : 0;
        const bool isd = p < n && t == d;
        const uint64_t m = __ballot(isd);
        const uint64_t mb = m & below;
        const int r = nd + popc64(mb);                       // this token's word (delimiters before it)
        const int ws = mb ? tb + c + 63 - __clzll((long long)mb) + 1 : wstart;
        if (isd) {
            // the word r ends here; word r + 1 starts after the delimiter
            const int s0 = ws;
            winfo[wb + r] = (uint32_t)s0 | ((uint32_t)(tb + p - s0) << 16);
        } else if (p < n) {
            atomicAdd(&wfp[wb + r], word_mix((uint32_t)t, (uint32_t)(tb + p - ws)));
        }
        nd += popc64(m);
        if (m) wstart = tb + c + 63 - __clzll((long long)m) + 1;
    }
    if (lane == 0) winfo[wb + nd] = (uint32_t)wstart | ((uint32_t)(tb + n - wstart) << 16);   // the last word
    return nd + 1;
}

__global__ __launch_bounds__(64) void word_ids_kernel(
    const int32_t* __restrict__ ref, const int32_t* __restrict__ ref_len, int ref_stride,
    const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_len, int hyp_stride, int delim,
    int32_t* __restrict__ ref_ids, int32_t* __restrict__ ref_words, int32_t* __restrict__ hyp_ids, int32_t* __restrict__ hyp_words) {
    extern __shared__ uint32_t word_lds[];
    const int pair = blockIdx.x;
    const int lane = threadIdx.x;
    int n = ref_len[pair]; n = n < 0 ? 0 : (n > ref_stride ? ref_stride : n);
    int m = hyp_len[pair]; m = m < 0 ? 0 : (m > hyp_stride ? hyp_stride : m);
    const int Wmax = ref_stride + hyp_stride + 2;
    int32_t* tok = (int32_t*)word_lds;
    uint32_t* winfo = word_lds + (ref_stride + hyp_stride);
    uint32_t* wfp = winfo + Wmax;
    uint32_t* table = wfp + Wmax;

    const int32_t* r = ref + (size_t)pair * ref_stride;
    const int32_t* h = hyp + (size_t)pair * hyp_stride;
#pragma unroll 4
    for (int p = lane; p < n; p += 64) tok[p] = r[p];
#pragma unroll 4
    for (int p = lane; p < m; p += 64) tok[n + p] = h[p];
    for (int w = lane; w < n + m + 2; w += 64) wfp[w] = 0u;
    __syncthreads();
    const int nr = split_words(tok, 0, n, delim, 0, winfo, wfp, lane);
    const int nh = split_words(tok, n, m, delim, nr, winfo, wfp, lane);
    const int W = nr + nh;
    const int S = word_table_size(W);
    const uint32_t smask = (uint32_t)S - 1u;
    for (int s = lane; s < S; s += 64) table[s] = 0u;
    if (lane == 0) { ref_words[pair] = nr; hyp_words[pair] = nh; }
    __syncthreads();

    int32_t* rid = ref_ids + (size_t)pair * (ref_stride + 1);
    int32_t* hid = hyp_ids + (size_t)pair * (hyp_stride + 1);
    for (int c = 0; c < W; c += 64) {
        const int w = c + lane;
        const bool valid = w < W;
        const uint32_t info = valid ? winfo[w] : 0u;
        const int st = (int)(info & 0xffffu), len = (int)(info >> 16);
        const uint32_t fp = valid ? wfp[w] : 0u;
        int found = -1;
        // (a) the distinct words of the earlier chunks
        uint32_t s = fp & smask;
        bool probing = valid;
        while (__any(probing)) {
            int cand = -1;
            while (probing) {
                const uint32_t e = table[s];
                if (e == 0u) { probing = false; break; }
                const int j = (int)e - 1;
                if ((int)(winfo[j] >> 16) == len && wfp[j] == fp) { cand = j; break; }
                s = (s + 1u) & smask;
            }
            const bool eq = words_equal(cand >= 0, cand >= 0 ? (int)(winfo[cand] & 0xffffu) : 0, st, len, tok, lane);
            if (cand >= 0) {
                if (eq) { found = cand; probing = false; }
                else s = (s + 1u) & smask;
            }
        }
        // (b) the earlier lanes of this chunk that are new words themselves, in lane order (the first occurrence wins)
        const bool unmatched = valid && found < 0;
        const uint64_t um = __ballot(unmatched);
        for (uint64_t q = um; q; q &= q - 1) {
            const int jl = __ffsll((unsigned long long)q) - 1;
            const int jst = __shfl(st, jl, 64), jlen = __shfl(len, jl, 64);
            const uint32_t jfp = (uint32_t)__shfl((int)fp, jl, 64);
            const bool want = unmatched && found < 0 && lane > jl && len == jlen && fp == jfp;
            if (!__any(want)) continue;
            const bool eq = words_equal(want, jst, st, len, tok, lane);
            if (want && eq) found = c + jl;
        }
        // (c) what is still unmatched is the first occurrence of a new word
        if (valid && found < 0) {
            uint32_t t = fp & smask;
            while (atomicCAS(&table[t], 0u, (uint32_t)(w + 1)) != 0u) t = (t + 1u) & smask;
            found = w;
        }
        if (valid) {
            if (w < nr) rid[w] = found + 1;
            else hid[w - nr] = found + 1;
        }
        __syncthreads();
    }
}

// pgasr_pg_rewards_multi with the reward normalised by reward_lengths and utt_scale by target_lengths: the same arithmetic in the
// same order, so reward_lengths == target_lengths gives pg_rewards_multi_kernel's bits.
__global__ __launch_bounds__(256) void pg_rewards_multi_ex_kernel(const int32_t* __restrict__ dist, const int32_t* __restrict__ rw_len,
                                                                  const int32_t* __restrict__ tg_len, int B, int K, int loo, float lam,
                                                                  float inv_bg, float* __restrict__ R_b, float* __restrict__ R_s,
                                                                  float* __restrict__ coef, float* __restrict__ utt_scale) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int Lr = rw_len[b], L = tg_len[b];
    const float Rf = (float)(Lr > 1 ? Lr : 1);
    const float Lf = (float)(L > 1 ? L : 1);
    const float scale = (lam * inv_bg) / (float)K;
    const int32_t* ds = dist + (loo ? 0 : B);
    if (!loo) {
        const float rg = -(float)dist[b] / Rf;
        for (int k = 0; k < K; ++k) {
            const float rs = -(float)ds[(size_t)k * B + b] / Rf;
            R_s[(size_t)k * B + b] = rs;
            coef[(size_t)k * B + b] = scale * (rs - rg);
        }
        R_b[b] = rg;
    } else {
        float S = 0.f;
        for (int k = 0; k < K; ++k) S += -(float)ds[(size_t)k * B + b] / Rf;
        float bsum = 0.f;
        for (int k = 0; k < K; ++k) {
            const float rs = -(float)ds[(size_t)k * B + b] / Rf;
            const float bk = (S - rs) / (float)(K - 1);
            R_s[(size_t)k * B + b] = rs;
            coef[(size_t)k * B + b] = scale * (rs - bk);
            bsum += bk;
        }
        R_b[b] = bsum / (float)K;
    }
    utt_scale[b] = inv_bg / Lf;
}

}  // namespace

extern "C" int pgasr_word_ids(const int32_t* ref, const int32_t* ref_len, int ref_stride,
                              const int32_t* hyp, const int32_t* hyp_len, int hyp_stride, int N, int delimiter,
                              int32_t* ref_ids, int32_t* ref_words, int32_t* hyp_ids, int32_t* hyp_words, void* stream) {
    if (N <= 0 || delimiter < 0 || ref_stride < 0 || hyp_stride < 0) return PGASR_ERR_INVALID_ARG;
    if (!ref_len || !hyp_len || !ref_ids || !ref_words || !hyp_ids || !hyp_words) return PGASR_ERR_INVALID_ARG;
    if ((ref_stride > 0 && !ref) || (hyp_stride > 0 && !hyp)) return PGASR_ERR_INVALID_ARG;
    if (ref_stride > PGASR_WORD_MAX_STRIDE || hyp_stride > PGASR_WORD_MAX_STRIDE) return PGASR_ERR_UNSUPPORTED;
    const size_t need = word_lds_bytes(ref_stride, hyp_stride);
    // Inside the train step the pairs run on the loss section's side stream BESIDE the CTC lattice, as pgasr_edit_distance's do
    // (see there): up to 128 pairs each reserve the LDS of a CU that no lattice workgroup (4 KB) leaves, so no pair shares a SIMD
    // with a lattice chain.  PGASR_WORD_LDS=0 switches the reservation off; bulk calls keep many waves per CU.
    static const int word_env = [] {
        const char* e = getenv("PGASR_WORD_LDS");
        int want = e ? atoi(e) : 156 * 1024, dev = 0, cap = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cap, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && cap > 0 && want > cap)
            want = cap;
        return want > 0 ? want : 0;
    }();
    size_t lds = need;
    if (N <= 128 && (size_t)word_env > lds) lds = (size_t)word_env;
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)word_ids_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        if (need > 64 * 1024) return PGASR_ERR_UNSUPPORTED;
        lds = need;                     // no reservation rather than a failed launch (slower beside a lattice, never wrong)
    }
    PGASR_LAUNCH_KERNEL(word_ids_kernel, dim3(N), dim3(64), lds, (hipStream_t)stream, ref, ref_len, ref_stride, hyp, hyp_len,
                        hyp_stride, delimiter, ref_ids, ref_words, hyp_ids, hyp_words);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}

extern "C" int pgasr_pg_rewards_multi_ex(const int32_t* dist, const int32_t* reward_lengths, const int32_t* target_lengths, int B, int K,
                                         int baseline, float lam, float inv_global_batch, float* R_baseline, float* R_sample,
                                         float* pg_coef, float* utt_scale, void* stream) {
    if (!dist || !reward_lengths || !target_lengths || !R_baseline || !R_sample || !pg_coef || !utt_scale || B <= 0)
        return PGASR_ERR_INVALID_ARG;
    if (K < 1 || K > PGASR_MAX_SAMPLES) return PGASR_ERR_INVALID_ARG;
    if (baseline != PGASR_BASELINE_HYPOTHESIS && baseline != PGASR_BASELINE_LEAVE_ONE_OUT) return PGASR_ERR_INVALID_ARG;
    if (baseline == PGASR_BASELINE_LEAVE_ONE_OUT && K < 2) return PGASR_ERR_INVALID_ARG;
    PGASR_LAUNCH_KERNEL(pg_rewards_multi_ex_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                        dist, reward_lengths, target_lengths, B, K, baseline == PGASR_BASELINE_LEAVE_ONE_OUT ? 1 : 0, lam,
                        inv_global_batch, R_baseline, R_sample, pg_coef, utt_scale);
    PGASR_CHECK_LAUNCH();
    return PGASR_OK;
}
