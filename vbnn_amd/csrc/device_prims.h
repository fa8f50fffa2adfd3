// device_prims.h -- the small primitives that several kernels must agree on bit for bit, each defined once: the order word of a
// float, the three-digit plan of the many-workgroup radix selects (prune.hip, acquire.hip), and the sums and scans over a wave
// or a 256-thread workgroup that run in one fixed order. Nothing here takes a flag for one caller's sake: what a caller does to
// its bits BEFORE the map (a canonical NaN, -0 folded into +0, a complement for "largest first") stays at the call site.
#pragma once
#include "common.h"

// ---- the order word: the floats' bits as unsigned integers in ascending order (-0 right below +0, the NaNs with a clear sign
// above +inf), adjacent floats adjacent words; and the inverse
__host__ __device__ __forceinline__ uint32_t vbnn_order_word(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits ^ 0x80000000u); }
__host__ __device__ __forceinline__ uint32_t vbnn_unorder_word(uint32_t w) { return (w & 0x80000000u) ? (w ^ 0x80000000u) : ~w; }
__host__ __device__ __forceinline__ bool vbnn_bits_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }
__host__ __device__ __forceinline__ bool vbnn_bits_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }

// ---- the digit plan: the k-th smallest of many 32-bit words, digit by digit, 11 + 11 + 10 bits. Pass p counts, over the words
// that match the prefix chosen so far, the values of digit p (an LDS histogram per workgroup, radix_flush to the global one); a
// one-workgroup kernel then calls radix_pick and hands the longer prefix and the rank inside the bin on in device words of its
// own. Counts are integers: nothing depends on the order of the atomics.
struct RadixPass { int shift, bits; uint32_t prefix_mask; };
static inline RadixPass radix_pass(int p) {
    switch (p) {
        case 0: return {21, 11, 0u};
        case 1: return {10, 11, 0xffe00000u};
        default: return {0, 10, 0xfffffc00u};
    }
}
// the workgroup's LDS histogram onto the global one: one integer atomic per non-empty bin (after a barrier of the caller's)
template <int THREADS>
__device__ __forceinline__ void radix_flush(const uint32_t* lds_hist, uint32_t* ghist, int bits) {
    for (int i = threadIdx.x; i < (1 << bits); i += THREADS) {
        const uint32_t c = lds_hist[i];
        if (c) atomicAdd(&ghist[i], c);
    }
}
// One workgroup of 256 threads: the bin of digit `ps` that holds the word of 0-based rank `rank0` among those counted in ghist
// (which hold more than rank0 words). True in exactly one thread, the one whose 8 or 4 consecutive bins hold it; there `bin` is
// the digit's value, `rank_in_bin` the rank among the bin's words and `bin_count` their number.
__device__ __forceinline__ bool radix_pick(const uint32_t* ghist, RadixPass ps, uint32_t rank0, uint32_t* part /* 256 words of LDS */,
                                           uint32_t& bin, uint32_t& rank_in_bin, uint32_t& bin_count) {
    const int per = (1 << ps.bits) / 256;
    uint32_t c[8];
    uint32_t own = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) { c[j] = (j < per) ? ghist[threadIdx.x * per + j] : 0u; own += c[j]; }
    part[threadIdx.x] = own;
    __syncthreads();
    uint32_t before = 0u;
    for (int i = 0; i < (int)threadIdx.x; ++i) before += part[i];
    if (rank0 < before || rank0 - before >= own) return false;
    uint32_t r = rank0 - before;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (j < per) {
            if (r < c[j]) { bin = (uint32_t)(threadIdx.x * per + j); rank_in_bin = r; bin_count = c[j]; return true; }
            r -= c[j];
        }
    }
    return false;                                                  // (not reached: r < own = the sum of c)
}

// ---- sums and scans in one fixed order
// over the 64 lanes of a wave, the shuffle-down tree (double, uint32_t, uint64_t); valid in lane 0
template <typename T>
__device__ __forceinline__ T vbnn_wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
// over the 256 threads of a workgroup: the wave sums, then the four waves in index order. `sh`: 4 doubles of LDS, which calls in
// a row may share (the first barrier waits for the readers of the call before)
__device__ __forceinline__ double vbnn_block_sum256(double v, double* sh) {
    v = vbnn_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}
// inclusive prefix over the lanes of a wave, in lane order
__device__ __forceinline__ uint32_t vbnn_wave_scan_incl(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}
