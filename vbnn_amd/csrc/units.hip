// units.hip -- structured signal-to-noise pruning: the group form of mainviz.lua:20-27. A hidden unit's key is
// ||mu_o||_2 / ||sigma_o||_2 over its incoming weights (mainviz.lua:20's |mu| / sigma when the unit has one input); the exact
// k-th smallest key over the units of one or several layers is the threshold (mainviz.lua:21 turned round, as vbnn_prune_select
// for weights); the kept units of a layer become an ascending index list; and a gather writes the parameters of the smaller
// dense network those lists describe. Streaming kernels: 16-byte accesses, integer counts and double sums in one fixed order,
// ordered lists from wave ballots (as k_sparse_fill) -- no float atomics, every output bitwise reproducible. Compiled without fp
// contraction (Makefile), as the other sweeps: expf here gives the bits it gives in k_snr.
#include "device_prims.h"

// ---------------------------------------------------------------------------------- vbnn_unit_snr
// Quad q of a row (elements 4q .. 4q + 3) belongs to thread q % T of the row's T threads (T = 64: a wave per row; 256: a
// workgroup per row); a thread adds its quads in rising q and a quad's elements in order, whether the quad came as one 16-byte
// load or as four scalar ones -- the sum does not depend on the alignment of the arrays.
template <int T>
__device__ __forceinline__ void unit_row_sums(const float* __restrict__ m, const float* __restrict__ l, int64_t I, int t, bool vec,
                                              double& sm, double& sv) {
    const int64_t quads = (I + 3) >> 2;
#pragma unroll 4
    for (int64_t q = t; q < quads; q += T) {
        const int valid = (int)min((int64_t)4, I - 4 * q);
        float a[4], b[4];
        load4<float>(m + 4 * q, a, valid, vec);
        load4<float>(l + 4 * q, b, valid, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < valid) {
                sm += (double)a[e] * (double)a[e];
                sv += (double)expf(b[e]);
            }
    }
}
// sqrt and the quotient in double, ONE rounding to fp32. NaN (a NaN parameter, 0 / 0) in its canonical positive form: the keys
// then order as their bit patterns, NaN above +inf.
__device__ __forceinline__ float unit_key(double sm, double sv) {
    const double k = sqrt(sm) / sqrt(sv);
    return (k != k) ? __uint_as_float(0x7fc00000u) : (float)k;
}

template <bool PER_WG>
__global__ __launch_bounds__(256) void k_unit_snr(const float* __restrict__ means, const float* __restrict__ lvars, int64_t O, int64_t I,
                                                  float* __restrict__ key) {
    __shared__ double sh[8];
    const bool vec = ((I & 3) == 0) && ((((uintptr_t)means | (uintptr_t)lvars) & 15u) == 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if constexpr (PER_WG) {
        for (int64_t o = blockIdx.x; o < O; o += gridDim.x) {
            double sm = 0.0, sv = 0.0;
            unit_row_sums<256>(means + o * I, lvars + o * I, I, (int)threadIdx.x, vec, sm, sv);
            sm = vbnn_block_sum256(sm, sh);                        // (its first barrier: the previous row's reads of sh are over)
            sv = vbnn_block_sum256(sv, sh + 4);
            if (threadIdx.x == 0) key[o] = unit_key(sm, sv);
        }
    } else {
        for (int64_t o = (int64_t)blockIdx.x * 4 + wave; o < O; o += (int64_t)gridDim.x * 4) {
            double sm = 0.0, sv = 0.0;
            unit_row_sums<64>(means + o * I, lvars + o * I, I, lane, vec, sm, sv);
            sm = vbnn_wave_sum(sm); sv = vbnn_wave_sum(sv);
            if (lane == 0) key[o] = unit_key(sm, sv);
        }
    }
}

static int unit_check(int n_layers, const vbnn_unit_desc* layers, int64_t* total) {
    VBNN_REQUIRE(layers && n_layers >= 1 && n_layers <= 8, "n_layers (1..8)");
    int64_t n = 0;
    for (int l = 0; l < n_layers; ++l) {
        VBNN_REQUIRE(layers[l].key, "null layer argument");
        VBNN_REQUIRE(layers[l].O > 0 && layers[l].I > 0 && layers[l].O < ((int64_t)1 << 31), "layer shape");
        n += layers[l].O;
    }
    VBNN_REQUIRE(n < ((int64_t)1 << 31), "more than 2^31 - 1 units");
    *total = n;
    return VBNN_OK;
}

extern "C" int vbnn_unit_snr(vbnn_ctx* ctx, int n_layers, const vbnn_unit_desc* layers) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx, "null argument");
    int64_t n;
    if (int st = unit_check(n_layers, layers, &n)) return st;
    for (int l = 0; l < n_layers; ++l) {
        const vbnn_unit_desc& d = layers[l];
        VBNN_REQUIRE(d.means && d.lvars, "null layer argument");
        // few long rows: a workgroup per row, or most of the chip idles; otherwise a wave per row, four rows per workgroup
        if (d.O < 1024 && d.I > 1024)
            hipLaunchKernelGGL(k_unit_snr<true>, dim3((unsigned)min(d.O, (int64_t)4096)), dim3(256), 0, ctx->stream, d.means, d.lvars,
                               d.O, d.I, d.key);
        else
            hipLaunchKernelGGL(k_unit_snr<false>, dim3((unsigned)min((d.O + 3) / 4, (int64_t)4096)), dim3(256), 0, ctx->stream, d.means,
                               d.lvars, d.O, d.I, d.key);
    }
    return vbnn_check_launch("k_unit_snr");
    VBNN_API_END
}

// ---------------------------------------------------------------------------------- vbnn_unit_select, vbnn_unit_index
struct UnitKeys { const float* key[8]; int64_t O[8]; uint32_t* keep[8]; uint32_t* n_keep[8]; int n; };
constexpr int UNIT_THREADS = 1024;

__device__ __forceinline__ uint32_t unit_bits(float k) { return (k != k) ? 0x7fc00000u : __float_as_uint(k); }

// The rank-th smallest (0-based) of the keys of layers [l0, l1), as bits, in every thread of the ONE workgroup that calls it:
// a radix select, four digits of 8 bits, integer counts in LDS. hist: 256 words, st: 2 words.
__device__ __forceinline__ uint32_t unit_kth(const UnitKeys& a, int l0, int l1, uint32_t rank, uint32_t* hist, uint32_t* st) {
    uint32_t prefix = 0u, mask = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0u;
        __syncthreads();
        for (int l = l0; l < l1; ++l)
            for (int64_t i = threadIdx.x; i < a.O[l]; i += UNIT_THREADS) {
                const uint32_t b = unit_bits(a.key[l][i]);
                if ((b & mask) == prefix) atomicAdd(&hist[(b >> shift) & 255u], 1u);
            }
        __syncthreads();
        if (threadIdx.x < 256) {
            const uint32_t own = hist[threadIdx.x];
            uint32_t before = 0u;
            for (int i = 0; i < (int)threadIdx.x; ++i) before += hist[i];
            if (rank >= before && rank - before < own) {           // exactly one thread: the counts sum to more than rank
                st[0] = prefix | ((uint32_t)threadIdx.x << shift);
                st[1] = rank - before;
            }
        }
        __syncthreads();
        prefix = st[0]; rank = st[1];
        mask |= 0xffu << shift;
    }
    return prefix;
}

__global__ __launch_bounds__(UNIT_THREADS) void k_unit_select(UnitKeys a, uint32_t k, float* __restrict__ tau_dev) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t st[2];
    const uint32_t t = unit_kth(a, 0, a.n, k, hist, st);
    if ((int)threadIdx.x < a.n) tau_dev[threadIdx.x] = __uint_as_float(t);      // one copy per listed layer: what k_unit_index reads
}

extern "C" int vbnn_unit_select(vbnn_ctx* ctx, int n_layers, const vbnn_unit_desc* layers, int64_t k, float* tau_dev) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && tau_dev, "null argument");
    int64_t n;
    if (int st = unit_check(n_layers, layers, &n)) return st;
    VBNN_REQUIRE(k >= 0 && k < n, "k (0 .. n_units - 1: prune everything with tau = +inf, not with k = n_units)");
    UnitKeys a{};
    a.n = n_layers;
    for (int l = 0; l < n_layers; ++l) { a.key[l] = layers[l].key; a.O[l] = layers[l].O; }
    hipLaunchKernelGGL(k_unit_select, dim3(1), dim3(UNIT_THREADS), 0, ctx->stream, a, (uint32_t)k, tau_dev);
    return vbnn_check_launch("k_unit_select");
    VBNN_API_END
}

// Workgroup l = layer l. n0 = units with !(key < tau); n = min(O, m ceil(max(n0, 1) / m)); the kept set is the first n units in
// the order (larger key first, NaN above all, lower index first on equal keys): everything above the n-th largest key T, and of
// the units AT T the first n - #{key > T} by index. The list is written in index order: wave w owns a contiguous run of units,
// the runs' counts meet in LDS, a unit's place is the kept units before it (closed form across runs, ballots within one).
__global__ __launch_bounds__(UNIT_THREADS) void k_unit_index(UnitKeys a, const float* __restrict__ tau_dev, float tau_host, uint32_t m) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t st[2];
    __shared__ uint32_t cnt[2][UNIT_THREADS / 64];
    const int l = blockIdx.x;
    const float tau = tau_dev ? tau_dev[l] : tau_host;
    const float* key = a.key[l];
    const uint32_t O = (uint32_t)a.O[l];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int NW = UNIT_THREADS / 64;
    if (threadIdx.x == 0) st[0] = 0u;
    __syncthreads();
    uint32_t c = 0u;
    for (uint32_t i = threadIdx.x; i < O; i += UNIT_THREADS) c += !(key[i] < tau) ? 1u : 0u;
    c = vbnn_wave_sum(c);
    if (lane == 0 && c) atomicAdd(&st[0], c);
    __syncthreads();
    const uint32_t n0 = max(st[0], 1u);
    const uint64_t up = (uint64_t)((n0 + m - 1u) / m) * m;
    const uint32_t n = (uint32_t)min((uint64_t)O, up);
    __syncthreads();                                               // (st is unit_kth's from here)
    const uint32_t T = unit_kth(a, l, l + 1, O - n, hist, st);
    // counts of the wave's run: keys above T, keys at T
    const uint32_t per = ((O + NW - 1) / NW + 63u) / 64u * 64u;     // run length, whole 64s
    const uint32_t b0 = min((uint32_t)wave * per, O), b1 = min(b0 + per, O);
    uint32_t g = 0u, e = 0u;
    for (uint32_t i = b0 + lane; i < b1; i += 64u) {
        const uint32_t u = unit_bits(key[i]);
        g += u > T ? 1u : 0u; e += u == T ? 1u : 0u;
    }
    g = vbnn_wave_sum(g); e = vbnn_wave_sum(e);
    if (lane == 0) { cnt[0][wave] = g; cnt[1][wave] = e; }
    __syncthreads();
    uint32_t g_all = 0u, g_run = 0u, e_run = 0u;
    for (int w = 0; w < NW; ++w) {
        g_all += cnt[0][w];
        if (w < wave) { g_run += cnt[0][w]; e_run += cnt[1][w]; }
    }
    const uint32_t ties = n - g_all;                               // units at T that are kept: the first `ties` by index (>= 1)
    uint32_t* keep = a.keep[l];
    for (uint32_t i0 = b0; i0 < b1; i0 += 64u) {
        const uint32_t i = i0 + lane;
        const bool in = i < b1;
        const uint32_t u = in ? unit_bits(key[i]) : 0u;
        const bool tie = in && u == T;
        const unsigned long long tb = __ballot(tie);
        const unsigned long long lt = (1ull << lane) - 1ull;
        const unsigned long long gb = __ballot(in && u > T);
        const bool kp = in && (u > T || (tie && e_run + (uint32_t)__popcll(tb & lt) < ties));
        const unsigned long long kb = __ballot(kp);
        const uint32_t pos = g_run + min(e_run, ties) + (uint32_t)__popcll(kb & lt);
        if (kp && pos < O) keep[pos] = i;
        g_run += (uint32_t)__popcll(gb);
        e_run += (uint32_t)__popcll(tb);
    }
    if (threadIdx.x == 0) a.n_keep[l][0] = n;
}

extern "C" int vbnn_unit_index(vbnn_ctx* ctx, int n_layers, const vbnn_unit_desc* layers, const float* tau_dev, float tau_host,
                               int64_t multiple) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx, "null argument");
    int64_t n;
    if (int st = unit_check(n_layers, layers, &n)) return st;
    VBNN_REQUIRE(multiple >= 1 && multiple < ((int64_t)1 << 31), "multiple (>= 1)");
    UnitKeys a{};
    a.n = n_layers;
    for (int l = 0; l < n_layers; ++l) {
        VBNN_REQUIRE(layers[l].keep && layers[l].n_keep, "null layer argument");
        a.key[l] = layers[l].key; a.O[l] = layers[l].O; a.keep[l] = layers[l].keep; a.n_keep[l] = layers[l].n_keep;
    }
    hipLaunchKernelGGL(k_unit_index, dim3(n_layers), dim3(UNIT_THREADS), 0, ctx->stream, a, tau_dev, tau_host, (uint32_t)multiple);
    return vbnn_check_launch("k_unit_index");
    VBNN_API_END
}

// ---------------------------------------------------------------------------------- vbnn_unit_gather
// A thread owns four consecutive destination columns of one destination row: one 16-byte store per array (scalar stores where
// the destination row pitch or base does not allow it), its reads four columns of ONE source row -- near each other, and the
// row is shared with the threads beside it. Index words are read from global memory (the lists are a few KiB: L2) and clamped
// to the source shape, so a list that was never filled cannot send a read outside the arrays.
template <bool DUAL>
__global__ __launch_bounds__(256) void k_unit_gather(const float* __restrict__ means, const float* __restrict__ lvars,
                                                     const float* __restrict__ bias, int64_t O, int64_t I,
                                                     const uint32_t* __restrict__ rows, int64_t n_rows,
                                                     const uint32_t* __restrict__ cols, int64_t n_cols, float* __restrict__ dst_means,
                                                     float* __restrict__ dst_lvars, float* __restrict__ dst_bias) {
    const int64_t quads = (n_cols + 3) >> 2, total = n_rows * quads;
    const bool vec = ((n_cols & 3) == 0) && ((((uintptr_t)dst_means | (DUAL ? (uintptr_t)dst_lvars : 0)) & 15u) == 0);
    const bool vec_in = !cols && ((I & 3) == 0) && ((((uintptr_t)means | (DUAL ? (uintptr_t)lvars : 0)) & 15u) == 0);
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t r = t / quads, c = (t - r * quads) * 4;
        const int valid = (int)min((int64_t)4, n_cols - c);
        const int64_t sr = rows ? (int64_t)min((uint32_t)rows[r], (uint32_t)(O - 1)) : r;
        const float* ms = means + sr * I;
        const float* ls = DUAL ? lvars + sr * I : nullptr;
        float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
        if (cols) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < valid) {
                    const uint32_t sc = min((uint32_t)cols[c + e], (uint32_t)(I - 1));
                    a[e] = ms[sc];
                    if constexpr (DUAL) b[e] = ls[sc];
                }
        } else {
            load4<float>(ms + c, a, valid, vec_in);
            if constexpr (DUAL) load4<float>(ls + c, b, valid, vec_in);
        }
        store4<float>(dst_means + r * n_cols + c, a[0], a[1], a[2], a[3], valid, vec);
        if constexpr (DUAL) store4<float>(dst_lvars + r * n_cols + c, b[0], b[1], b[2], b[3], valid, vec);
        if (bias && c == 0) dst_bias[r] = bias[sr];
    }
}

extern "C" int vbnn_unit_gather(vbnn_ctx* ctx, const vbnn_unit_gather_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a, "null ctx/args");
    VBNN_REQUIRE(a->means && a->dst_means, "means and dst_means are required");
    VBNN_REQUIRE(!a->lvars == !a->dst_lvars, "lvars and dst_lvars go together");
    VBNN_REQUIRE(!a->bias == !a->dst_bias, "bias and dst_bias go together");
    VBNN_REQUIRE(a->O > 0 && a->I > 0 && a->O < ((int64_t)1 << 31) && a->I < ((int64_t)1 << 31), "source shape");
    VBNN_REQUIRE(a->n_rows >= 1 && a->n_cols >= 1, "n_rows, n_cols (>= 1)");
    VBNN_REQUIRE(a->rows ? a->n_rows <= a->O : a->n_rows == a->O, "n_rows (<= O with a list, O without)");
    VBNN_REQUIRE(a->cols ? a->n_cols <= a->I : a->n_cols == a->I, "n_cols (<= I with a list, I without)");
    const int64_t total = a->n_rows * ((a->n_cols + 3) >> 2);
    const int64_t blocks = min((total + 255) / 256, (int64_t)4096);
#define VBNN_UNIT_GATHER(DUAL)                                                                                                    \
    hipLaunchKernelGGL(k_unit_gather<DUAL>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, a->means, a->lvars, a->bias, a->O, \
                       a->I, a->rows, a->n_rows, a->cols, a->n_cols, a->dst_means, a->dst_lvars, a->dst_bias)
    if (a->lvars) VBNN_UNIT_GATHER(true); else VBNN_UNIT_GATHER(false);
#undef VBNN_UNIT_GATHER
    return vbnn_check_launch("k_unit_gather");
    VBNN_API_END
}
