// digest.hip -- vbnn_digest: a position-dependent, order-independent 64-bit digest of a device buffer's 32-bit words, for
// checkpoints (a tensor's digest is taken on the device before the download and again after the upload) and for comparing the
// replicas of a data-parallel run in 8 bytes per tensor. A read-only streaming kernel like prune.hip's key pass: 16-byte loads
// on the aligned body, 4-byte loads for a head and a tail of up to three words each (a row slice of a parameter is only 4-byte
// aligned), a uint64 accumulator per thread, a wave reduction, one LDS reduction per workgroup and ONE 64-bit integer atomic
// add per workgroup. Integer arithmetic only: the sum is taken mod 2^64, so neither the grid nor the order of the atomics can
// change a bit of it.
//
// Traffic: 4 B read per word, nothing written but the one atomic per workgroup. Arithmetic: two 64-bit multiplies per word.
#include "device_prims.h"

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int DIGEST_THREADS = 256;
constexpr int DIGEST_UNROLL = 2;               // 16-byte loads a thread has in flight per trip of the body loop
constexpr int DIGEST_MAX_BLOCKS = 2048;        // 8 workgroups of 4 waves per CU on 256 CUs; the rest is the grid-stride loop

// the splitmix64 finaliser (include/vbnn_hip.h states it; tests/_digest_np.py restates it)
__device__ __forceinline__ uint64_t digest_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// word `w` at 1-based global position `pos1` = index0 + i + 1 (< 2^32: checked on the host)
__device__ __forceinline__ uint64_t digest_term(uint64_t pos1, uint32_t w) { return digest_mix((pos1 << 32) | (uint64_t)w); }

__device__ __forceinline__ uint64_t digest_quad(uint64_t pos1, u32x4 v) {
    return digest_term(pos1, v[0]) + digest_term(pos1 + 1, v[1]) + digest_term(pos1 + 2, v[2]) + digest_term(pos1 + 3, v[3]);
}

__global__ __launch_bounds__(DIGEST_THREADS) void k_digest(const uint32_t* __restrict__ buf, uint64_t n, uint64_t index0,
                                                           unsigned long long* __restrict__ out) {
    __shared__ uint64_t sh[DIGEST_THREADS / 64];
    // words before the first 16-byte boundary (buf is 4-byte aligned), whole 16-byte vectors, words after the last one
    uint64_t head = ((16u - (unsigned)((uintptr_t)buf & 15u)) & 15u) >> 2;
    if (head > n) head = n;
    const uint64_t quads = (n - head) >> 2;
    const uint64_t tail0 = head + (quads << 2);                    // first word of the tail; n - tail0 <= 3
    const u32x4* __restrict__ body = reinterpret_cast<const u32x4*>(buf + head);
    const uint64_t gid = (uint64_t)blockIdx.x * DIGEST_THREADS + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * DIGEST_THREADS;
    const uint64_t first = index0 + head + 1;                      // 1-based position of the body's first word
    uint64_t acc = 0;
    uint64_t t = gid;
    for (; t + stride < quads; t += 2 * stride) {                  // DIGEST_UNROLL = 2: both loads leave before either is used
        const u32x4 a = body[t];
        const u32x4 b = body[t + stride];
        acc += digest_quad(first + (t << 2), a);
        acc += digest_quad(first + ((t + stride) << 2), b);
    }
    if (t < quads) acc += digest_quad(first + (t << 2), body[t]);
    if (gid < head) acc += digest_term(index0 + gid + 1, buf[gid]);
    if (gid < n - tail0) acc += digest_term(index0 + tail0 + gid + 1, buf[tail0 + gid]);
    // wave, then workgroup: integer sums, any order gives the same bits
    acc = vbnn_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t s = 0;
#pragma unroll
        for (int w = 0; w < DIGEST_THREADS / 64; ++w) s += sh[w];
        atomicAdd(out, (unsigned long long)s);
    }
}

static inline int digest_grid(uint64_t n) {
    const uint64_t per_block = (uint64_t)DIGEST_THREADS * 4 * DIGEST_UNROLL;       // words of one trip of one workgroup
    uint64_t b = (n + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > (uint64_t)DIGEST_MAX_BLOCKS) b = DIGEST_MAX_BLOCKS;
    return (int)b;
}

extern "C" int vbnn_digest(vbnn_ctx* ctx, const void* buf, uint64_t n_words, uint64_t index0, uint64_t* out) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && out, "null argument");
    VBNN_REQUIRE(((uintptr_t)out & 7u) == 0, "out: 8-byte aligned");
    const uint64_t last = 0xffffffffull;                                            // positions are 1 .. 2^32 - 1
    VBNN_REQUIRE(n_words <= last && index0 <= last - n_words, "index0 + n_words > 2^32 - 1");
    VBNN_REQUIRE(((uintptr_t)buf & 3u) == 0, "buf: 4-byte aligned");
    if (n_words == 0) return VBNN_OK;                                               // legal: adds nothing
    VBNN_REQUIRE(buf, "null argument");
    hipLaunchKernelGGL(k_digest, dim3(digest_grid(n_words)), dim3(DIGEST_THREADS), 0, ctx->stream, (const uint32_t*)buf, n_words,
                       index0, (unsigned long long*)out);
    return vbnn_check_launch("k_digest");
    VBNN_API_END
}
