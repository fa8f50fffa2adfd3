// prune.hip -- signal-to-noise pruning of the VB layers (mainviz.lua:20-27): the key |mu| / sigma per weight, the exact
// k-th smallest key over one or several layers (device_prims.h's radix select on the key's bits), and the pruned operand shadows the
// predictive path multiplies by. Streaming kernels like the sweeps of elementwise.hip: 16-byte loads, grid-stride loops,
// integer histograms (order-independent) and double partials summed in a fixed order -- no float atomics anywhere, so
// every output is bitwise reproducible. Compiled without fp contraction (Makefile), as the other sweeps.
//
// Traffic of the chosen design: every pass re-forms the key from means / lvars (8 B per weight) -- three histogram passes
// and the pack, 32 B read + 2 x sizeof(T) written per weight. Nothing per weight is kept between the passes: the
// workspace is three histograms and two words of state.
#include "device_prims.h"

// THE key: vbnn_snr_key (common.h), one definition -- the kernels below and sparse.hip's must give one weight the same bits.

static inline int prune_grid(int64_t W) {
    int64_t b = (W + 4095) / 4096;             // >= 16 weights per thread before a second block is worth its histogram flush
    if (b < 1) b = 1;
    if (b > 1024) b = 1024;                    // 4 blocks of 4 waves per CU: 4 waves per SIMD on 256 CUs
    return (int)b;
}

// ---------------------------------------------------------------------------------- vbnn_snr
__global__ __launch_bounds__(256) void k_snr(const float* __restrict__ means, const float* __restrict__ lvars, int64_t W,
                                             float* __restrict__ out) {
    const bool vec = ((((uintptr_t)means | (uintptr_t)lvars | (uintptr_t)out) & 15u) == 0);
    const int64_t W4 = vec ? (W >> 2) : 0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < W4; t += (int64_t)gridDim.x * 256) {
        const f32x4 m = reinterpret_cast<const f32x4*>(means)[t];
        const f32x4 l = reinterpret_cast<const f32x4*>(lvars)[t];
        f32x4 s;
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = vbnn_snr_key(m[j], l[j]);
        reinterpret_cast<f32x4*>(out)[t] = s;
    }
    for (int64_t t = (W4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x; t < W; t += (int64_t)gridDim.x * 256)
        out[t] = vbnn_snr_key(means[t], lvars[t]);
}

extern "C" int vbnn_snr(vbnn_ctx* ctx, const float* means, const float* lvars, int64_t W, float* snr_out) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && means && lvars && snr_out, "null argument");
    VBNN_REQUIRE(W > 0, "W");
    hipLaunchKernelGGL(k_snr, dim3(prune_grid(W)), dim3(256), 0, ctx->stream, means, lvars, W, snr_out);
    return vbnn_check_launch("k_snr");
    VBNN_API_END
}

// ---------------------------------------------------------------------------------- vbnn_prune_select
// Non-negative floats (and the NaNs above them, sign cleared by fabsf) order as their bit patterns: the k-th smallest key
// is found digit by digit by the plan of device_prims.h (RadixPass, radix_flush, radix_pick): a histogram pass over the keys
// that match the prefix chosen so far, then a one-workgroup pick that writes the longer prefix and the rank within the bin
// to the state words the next pass reads.
constexpr int PRUNE_BINS = 2048;
constexpr int PRUNE_PASSES = 3;
constexpr size_t PRUNE_WS_WORDS = (size_t)PRUNE_PASSES * PRUNE_BINS + 16;       // histograms, then state { prefix, rank }

__device__ __forceinline__ void prune_count(uint32_t* hist, float mean, float lvar, uint32_t prefix, RadixPass ps) {
    const uint32_t b = __float_as_uint(vbnn_snr_key(mean, lvar));
    if ((b & ps.prefix_mask) == prefix) atomicAdd(&hist[(b >> ps.shift) & ((1u << ps.bits) - 1u)], 1u);
}

__global__ __launch_bounds__(256) void k_prune_hist(const float* __restrict__ means, const float* __restrict__ lvars, int64_t W,
                                                    RadixPass ps, const uint32_t* __restrict__ state, uint32_t* __restrict__ ghist) {
    __shared__ uint32_t hist[PRUNE_BINS];
    for (int i = threadIdx.x; i < PRUNE_BINS; i += 256) hist[i] = 0u;
    const uint32_t prefix = ps.prefix_mask ? state[0] : 0u;
    __syncthreads();
    const bool vec = ((((uintptr_t)means | (uintptr_t)lvars) & 15u) == 0);
    const int64_t W4 = vec ? (W >> 2) : 0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < W4; t += (int64_t)gridDim.x * 256) {
        const f32x4 m = reinterpret_cast<const f32x4*>(means)[t];
        const f32x4 l = reinterpret_cast<const f32x4*>(lvars)[t];
#pragma unroll
        for (int j = 0; j < 4; ++j) prune_count(hist, m[j], l[j], prefix, ps);
    }
    for (int64_t t = (W4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x; t < W; t += (int64_t)gridDim.x * 256)
        prune_count(hist, means[t], lvars[t], prefix, ps);
    __syncthreads();
    radix_flush<256>(hist, ghist, ps.bits);
}

// one workgroup: the bin of digit `ps` that holds rank state[1] (pass 0: k), the new prefix and the rank inside the bin
__global__ __launch_bounds__(256) void k_prune_pick(const uint32_t* __restrict__ ghist, RadixPass ps, int first, uint32_t k,
                                                    uint32_t* state, float* tau_dev) {
    __shared__ uint32_t part[256];
    const uint32_t rank = first ? k : state[1];
    const uint32_t prefix = first ? 0u : state[0];
    uint32_t bin, r, n;
    if (radix_pick(ghist, ps, rank, part, bin, r, n)) {            // exactly one thread: the counts sum to more than rank
        const uint32_t np = prefix | (bin << ps.shift);
        state[0] = np; state[1] = r;
        if (ps.shift == 0) tau_dev[0] = __uint_as_float(np);
    }
}

static int prune_total(int n_layers, const vbnn_prune_desc* layers, int64_t* total) {
    VBNN_REQUIRE(layers && n_layers >= 1 && n_layers <= 8, "n_layers (1..8)");
    int64_t W = 0;
    for (int l = 0; l < n_layers; ++l) {
        VBNN_REQUIRE(layers[l].means && layers[l].lvars, "null layer argument");
        VBNN_REQUIRE(layers[l].O > 0 && layers[l].I > 0, "layer shape");
        W += layers[l].O * layers[l].I;
    }
    VBNN_REQUIRE(W < ((int64_t)1 << 32), "more than 2^32 - 1 weights");
    *total = W;
    return VBNN_OK;
}

extern "C" int vbnn_prune_workspace_bytes(int n_layers, const vbnn_prune_desc* layers, size_t* bytes) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(bytes, "null argument");
    int64_t W;
    if (int st = prune_total(n_layers, layers, &W)) return st;
    *bytes = PRUNE_WS_WORDS * sizeof(uint32_t);
    return VBNN_OK;
    VBNN_API_END
}

extern "C" int vbnn_prune_select(vbnn_ctx* ctx, int n_layers, const vbnn_prune_desc* layers, int64_t k, float* tau_dev,
                                 void* workspace, size_t workspace_bytes) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && tau_dev && workspace, "null argument");
    int64_t W;
    if (int st = prune_total(n_layers, layers, &W)) return st;
    VBNN_REQUIRE(k >= 0 && k < W, "k (0 .. W - 1: prune everything with tau = +inf, not with k = W)");
    VBNN_REQUIRE(workspace_bytes >= PRUNE_WS_WORDS * sizeof(uint32_t) && ((uintptr_t)workspace & 3u) == 0, "workspace");
    uint32_t* ws = (uint32_t*)workspace;
    uint32_t* state = ws + (size_t)PRUNE_PASSES * PRUNE_BINS;
    VBNN_CHECK_HIP(hipMemsetAsync(ws, 0, PRUNE_WS_WORDS * sizeof(uint32_t), ctx->stream));
    for (int p = 0; p < PRUNE_PASSES; ++p) {
        const RadixPass ps = radix_pass(p);
        uint32_t* gh = ws + (size_t)p * PRUNE_BINS;
        for (int l = 0; l < n_layers; ++l) {
            const int64_t Wl = layers[l].O * layers[l].I;
            hipLaunchKernelGGL(k_prune_hist, dim3(prune_grid(Wl)), dim3(256), 0, ctx->stream, layers[l].means, layers[l].lvars, Wl,
                               ps, state, gh);
        }
        hipLaunchKernelGGL(k_prune_pick, dim3(1), dim3(256), 0, ctx->stream, gh, ps, p == 0 ? 1 : 0, (uint32_t)k, state, tau_dev);
    }
    return vbnn_check_launch("vbnn_prune_select");
    VBNN_API_END
}

// ---------------------------------------------------------------------------------- vbnn_prune_pack
// One sweep per layer: a kept weight's shadows are what k_prep_layer stores (T(mean), T(expf(lvar))), a pruned weight's
// are +0; per-workgroup partials of { pruned, sum of pruned vars, sum of vars }, added in a fixed order by the finish.
template <typename T>
__global__ __launch_bounds__(256) void k_prune_pack(const float* __restrict__ means, const float* __restrict__ lvars, int64_t O,
                                                    int64_t I, T* __restrict__ mu_p, T* __restrict__ var_p, int64_t ld_w,
                                                    uint8_t* __restrict__ mask, const float* __restrict__ tau_dev, float tau_host,
                                                    double* partial /* [gridDim.x][3] */) {
    __shared__ double sh[4];
    const float tau = tau_dev ? tau_dev[0] : tau_host;
    const int64_t quads = (I + 3) >> 2, total = O * quads;
    const bool vec_in = ((I & 3) == 0) && ((((uintptr_t)means | (uintptr_t)lvars) & 15u) == 0);
    const bool vec_out = ((ld_w & 3) == 0) && ((((uintptr_t)mu_p | (uintptr_t)var_p) & 15u) == 0);
    const bool vec_mask = ((I & 3) == 0) && (((uintptr_t)mask & 3u) == 0);
    double n_pruned = 0.0, s_pruned = 0.0, s_all = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t r = t / quads, c = (t - r * quads) * 4;
        const int valid = (int)min((int64_t)4, I - c);
        float m[4], l[4], v[4];
        load4<float>(means + r * I + c, m, valid, vec_in);
        load4<float>(lvars + r * I + c, l, valid, vec_in);
        uint32_t bits = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e < valid) {
                v[e] = expf(l[e]);
                s_all += (double)v[e];
                if (vbnn_snr_key(m[e], l[e]) < tau) {              // strict, torch.lt (mainviz.lua:21); false for a NaN key
                    n_pruned += 1.0; s_pruned += (double)v[e];
                    m[e] = 0.f; v[e] = 0.f;
                    bits |= 1u << (8 * e);
                }
            } else { m[e] = 0.f; v[e] = 0.f; }
        }
        store4<T>(mu_p + r * ld_w + c, m[0], m[1], m[2], m[3], valid, vec_out);
        store4<T>(var_p + r * ld_w + c, v[0], v[1], v[2], v[3], valid, vec_out);
        if (mask) {
            uint8_t* mp = mask + r * I + c;
            if (vec_mask) *reinterpret_cast<uint32_t*>(mp) = bits;
            else
                for (int e = 0; e < valid; ++e) mp[e] = (uint8_t)((bits >> (8 * e)) & 1u);
        }
    }
    const double r0 = vbnn_block_sum256(n_pruned, sh);
    const double r1 = vbnn_block_sum256(s_pruned, sh);
    const double r2 = vbnn_block_sum256(s_all, sh);
    if (threadIdx.x == 0) { partial[blockIdx.x * 3] = r0; partial[blockIdx.x * 3 + 1] = r1; partial[blockIdx.x * 3 + 2] = r2; }
}

struct PruneFinishArgs { const double* partial[8]; int nb[8]; int64_t W[8]; double* stats[8]; };
// block l: stats of layer l = { pruned, sum of pruned vars, sum of vars, W }, the workgroups' partials added in a fixed
// order (thread t takes workgroups t, t + 256, ...; then the block sum), as prior_finish of elementwise.hip
__global__ __launch_bounds__(256) void k_prune_finish(PruneFinishArgs a) {
    __shared__ double sh[4];
    const int l = blockIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < a.nb[l]; b += 256)
#pragma unroll
        for (int q = 0; q < 3; ++q) s[q] += a.partial[l][b * 3 + q];
    const double r0 = vbnn_block_sum256(s[0], sh);
    const double r1 = vbnn_block_sum256(s[1], sh);
    const double r2 = vbnn_block_sum256(s[2], sh);
    if (threadIdx.x == 0) { a.stats[l][0] = r0; a.stats[l][1] = r1; a.stats[l][2] = r2; a.stats[l][3] = (double)a.W[l]; }
}

extern "C" int vbnn_prune_pack(vbnn_ctx* ctx, int dtype, int n_layers, const vbnn_prune_desc* layers, const float* tau_dev,
                               float tau_host) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx, "null argument");
    int64_t Wt;
    if (int st = prune_total(n_layers, layers, &Wt)) return st;
    VBNN_REQUIRE(dtype == VBNN_F32 || dtype == VBNN_BF16, "dtype");
    VBNN_REQUIRE((size_t)n_layers * 4096 <= ctx->scratch_doubles, "scratch");
    PruneFinishArgs fa{};
    for (int l = 0; l < n_layers; ++l) {
        const vbnn_prune_desc& d = layers[l];
        VBNN_REQUIRE(d.mu_p && d.var_p && d.stats, "null layer argument");
        VBNN_REQUIRE(d.ld_w >= d.I, "layer shape");
        const int nb = prune_grid(d.O * d.I);                    // <= 1024 workgroups x 3 doubles of this layer's 4096
        double* partial = ctx->scratch + (size_t)l * 4096;
        if (dtype == VBNN_F32)
            hipLaunchKernelGGL(k_prune_pack<float>, dim3(nb), dim3(256), 0, ctx->stream, d.means, d.lvars, d.O, d.I, (float*)d.mu_p,
                               (float*)d.var_p, d.ld_w, d.mask, tau_dev, tau_host, partial);
        else
            hipLaunchKernelGGL(k_prune_pack<bf16_t>, dim3(nb), dim3(256), 0, ctx->stream, d.means, d.lvars, d.O, d.I, (bf16_t*)d.mu_p,
                               (bf16_t*)d.var_p, d.ld_w, d.mask, tau_dev, tau_host, partial);
        fa.partial[l] = partial; fa.nb[l] = nb; fa.W[l] = d.O * d.I; fa.stats[l] = d.stats;
    }
    hipLaunchKernelGGL(k_prune_finish, dim3(n_layers), dim3(256), 0, ctx->stream, fa);
    return vbnn_check_launch("vbnn_prune_pack");
    VBNN_API_END
}
