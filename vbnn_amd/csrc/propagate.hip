// propagate.hip -- the pieces of the sampling-free predictive (moment propagation, include/vbnn_hip.h) that are not a GEMM:
// vbnn_relu_moments (the moments of a rectified Gaussian, fp32 in, packed operands out), vbnn_square_shadow (mu^2 from the mu
// shadow) and vbnn_logit_draws (S Gaussian draws of R x C logits from the contract's normals). Streaming kernels: no LDS, no
// reduction, a thread works one 16-byte group of every output (G = 4 fp32 or 8 bf16 columns), grid-stride over the groups of
// the N x O block. Compiled WITHOUT floating-point contraction (Makefile): every line below is the op sequence the header states
// (sqrtf and the fp32 division: hipcc's correctly rounded ones).
#include "common.h"
#include <math.h>
#include <algorithm>

static inline int prop_grid(int64_t items) {                   // ~8 workgroups of 256 per CU, grid-stride above
    const int64_t b = std::max<int64_t>(1, (items + 255) / 256);
    return (int)std::min<int64_t>(b, (int64_t)vbnn_cu_count() * 8);
}

// G consecutive floats of a row: 16-byte loads (vec) or element by element (`valid` of them; the rest read as 0)
template <int G>
__device__ __forceinline__ void prop_load(const float* p, float (&x)[G], int valid, bool vec) {
    if (vec && valid == G) {
#pragma unroll
        for (int k = 0; k < G / 4; ++k) {
            const f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + k);
            x[4 * k] = t[0]; x[4 * k + 1] = t[1]; x[4 * k + 2] = t[2]; x[4 * k + 3] = t[3];
        }
    } else {
#pragma unroll
        for (int j = 0; j < G; ++j) x[j] = j < valid ? p[j] : 0.f;
    }
}
// G consecutive elements of a packed row: ONE 16-byte store (vec) or element by element. Plain stores: the next launch (a GEMM)
// reads them as its operand.
__device__ __forceinline__ void prop_store(float* p, const float (&x)[4], int valid, bool vec) {
    if (vec && valid == 4) {
        *reinterpret_cast<f32x4*>(p) = f32x4{x[0], x[1], x[2], x[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j < valid) p[j] = x[j];
    }
}
__device__ __forceinline__ void prop_store(bf16_t* p, const float (&x)[8], int valid, bool vec) {
    if (vec && valid == 8) {
        *reinterpret_cast<bf16x8*>(p) = bf16x8{(bf16_t)x[0], (bf16_t)x[1], (bf16_t)x[2], (bf16_t)x[3],
                                               (bf16_t)x[4], (bf16_t)x[5], (bf16_t)x[6], (bf16_t)x[7]};
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) if (j < valid) p[j] = (bf16_t)x[j];
    }
}

// ------------------------------------------------------------------------------------------------ vbnn_relu_moments
// the header's op sequence for one element
__device__ __forceinline__ void relu_moments_1(float m, float v, float& a, float& q, float& c) {
    if (v > 0.f) {
        const float s = sqrtf(v);
        const float al = m / s;
        const float phi = 0.3989423f * expf(-0.5f * (al * al));
        const float Phi = 0.5f * erfcf(-(al * 0.70710677f));
        a = fmaxf(m * Phi + s * phi, 0.f);
        q = fmaxf((m * m + v) * Phi + (m * s) * phi, 0.f);
        c = fmaxf(q - a * a, 0.f);
    } else {
        a = fmaxf(m, 0.f);
        q = a * a;
        c = 0.f;
    }
}

struct RmArgs {
    const float* m; int64_t ld_m; const float* v1; const float* v2; int64_t ld_v; int64_t N, O;
    void* a; void* q; void* c; int64_t ld_out;
    int in_vec, out_vec;
};

template <typename T, bool V2>
__global__ __launch_bounds__(256) void k_relu_moments(const RmArgs p) {
    constexpr int G = 16 / sizeof(T);
    const int64_t groups = (p.O + G - 1) / G, total = p.N * groups;
    T* const pa = (T*)p.a; T* const pq = (T*)p.q; T* const pc = (T*)p.c;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t r = t / groups, g = t - r * groups, col = g * G;
        const int valid = (int)min((int64_t)G, p.O - col);
        float m[G], v[G], w[G], a[G], q[G], c[G];
        prop_load<G>(p.m + r * p.ld_m + col, m, valid, p.in_vec);
        prop_load<G>(p.v1 + r * p.ld_v + col, v, valid, p.in_vec);
        if (V2) {
            prop_load<G>(p.v2 + r * p.ld_v + col, w, valid, p.in_vec);
#pragma unroll
            for (int j = 0; j < G; ++j) v[j] = v[j] + w[j];
        }
#pragma unroll
        for (int j = 0; j < G; ++j) relu_moments_1(m[j], v[j], a[j], q[j], c[j]);
        const int64_t o = r * p.ld_out + col;
        if (pa) prop_store(pa + o, a, valid, p.out_vec);
        if (pq) prop_store(pq + o, q, valid, p.out_vec);
        if (pc) prop_store(pc + o, c, valid, p.out_vec);
    }
}

template <typename T>
static int relu_moments_t(vbnn_ctx* ctx, const vbnn_relu_moments_args* a) {
    constexpr int G = 16 / sizeof(T);
    RmArgs p;
    p.m = a->m; p.ld_m = a->ld_m; p.v1 = a->v1; p.v2 = a->v2; p.ld_v = a->ld_v; p.N = a->N; p.O = a->O;
    p.a = a->a; p.q = a->q; p.c = a->c; p.ld_out = a->ld_out;
    p.in_vec = vbnn_al16(a->m) && vbnn_al16(a->v1) && vbnn_al16(a->v2) && (a->ld_m & 3) == 0 && (a->ld_v & 3) == 0;
    p.out_vec = vbnn_al16(a->a) && vbnn_al16(a->q) && vbnn_al16(a->c) && (a->ld_out % G) == 0;
    vbnn_cu_scope scope(ctx);
    const int nb = prop_grid(a->N * ((a->O + G - 1) / G));
    if (a->v2) hipLaunchKernelGGL((k_relu_moments<T, true>), dim3(nb), dim3(256), 0, ctx->stream, p);
    else hipLaunchKernelGGL((k_relu_moments<T, false>), dim3(nb), dim3(256), 0, ctx->stream, p);
    return vbnn_check_launch("k_relu_moments");
}

extern "C" int vbnn_relu_moments(vbnn_ctx* ctx, int dtype, const vbnn_relu_moments_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a && a->m && a->v1, "null argument (a, m, v1)");
    VBNN_REQUIRE(a->N >= 1 && a->O >= 1 && a->N < (1ll << 31) && a->O < (1ll << 31), "shape: N and O in [1, 2^31)");
    VBNN_REQUIRE(a->ld_m >= a->O && a->ld_v >= a->O && a->ld_m < (1ll << 31) && a->ld_v < (1ll << 31), "ld_m, ld_v");
    VBNN_REQUIRE(!(a->a || a->q || a->c) || (a->ld_out >= a->O && a->ld_out < (1ll << 31)), "ld_out");
    VBNN_REQUIRE(((uintptr_t)a->m & 3u) == 0 && ((uintptr_t)a->v1 & 3u) == 0 && ((uintptr_t)a->v2 & 3u) == 0, "m, v1, v2: 4-byte aligned");
    if (dtype != VBNN_F32 && dtype != VBNN_BF16) {
        vbnn_set_error("unsupported dtype %d", dtype);
        return VBNN_ERR_UNSUPPORTED;
    }
    const uintptr_t es = dtype == VBNN_F32 ? 4 : 2;
    VBNN_REQUIRE((uintptr_t)a->a % es == 0 && (uintptr_t)a->q % es == 0 && (uintptr_t)a->c % es == 0, "a, q, c: aligned to the element");
    // no output block may overlap an input block or another output (a thread stores before its neighbours have loaded)
    const uintptr_t in_bytes = (uintptr_t)((a->N - 1) * std::max(a->ld_m, a->ld_v) + a->O) * 4, out_bytes = (uintptr_t)((a->N - 1) * a->ld_out + a->O) * es;
    auto overlap = [](const void* x, uintptr_t nx, const void* y, uintptr_t ny) {
        return x && y && (uintptr_t)x < (uintptr_t)y + ny && (uintptr_t)y < (uintptr_t)x + nx;
    };
    const void* ins[3] = {a->m, a->v1, a->v2};
    const void* outs[3] = {a->a, a->q, a->c};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) VBNN_REQUIRE(!overlap(outs[i], out_bytes, ins[j], in_bytes), "an output overlaps an input");
        for (int j = i + 1; j < 3; ++j) VBNN_REQUIRE(!overlap(outs[i], out_bytes, outs[j], out_bytes), "two outputs overlap");
    }
    if (dtype == VBNN_F32) return relu_moments_t<float>(ctx, a);
    return relu_moments_t<bf16_t>(ctx, a);
    VBNN_API_END
}

// ------------------------------------------------------------------------------------------------ vbnn_square_shadow
template <typename T>
__global__ __launch_bounds__(256) void k_square_shadow(const T* __restrict__ src, int64_t ld_src, int64_t rows, int64_t cols,
                                                       T* __restrict__ dst, int64_t ld_dst, int vec) {
    constexpr int G = 16 / sizeof(T);
    typedef T TG __attribute__((ext_vector_type(G)));
    const int64_t groups = (cols + G - 1) / G, total = rows * groups;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t r = t / groups, g = t - r * groups, col = g * G;
        const int valid = (int)min((int64_t)G, cols - col);
        const T* s = src + r * ld_src + col;
        T* d = dst + r * ld_dst + col;
        if (vec && valid == G) {
            const TG x = *reinterpret_cast<const TG*>(s);
            TG y;
#pragma unroll
            for (int j = 0; j < G; ++j) { const float f = Elt<T>::from(x[j]); y[j] = Elt<T>::to(f * f); }
            *reinterpret_cast<TG*>(d) = y;
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j)
                if (j < valid) { const float f = Elt<T>::from(s[j]); d[j] = Elt<T>::to(f * f); }
        }
    }
}

extern "C" int vbnn_square_shadow(vbnn_ctx* ctx, int dtype, const void* src, int64_t ld_src, int64_t rows, int64_t cols,
                                  void* dst, int64_t ld_dst) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && src && dst, "null argument (src, dst)");
    VBNN_REQUIRE(rows >= 1 && cols >= 1 && rows < (1ll << 31) && cols < (1ll << 31), "shape: rows and cols in [1, 2^31)");
    VBNN_REQUIRE(ld_src >= cols && ld_dst >= cols && ld_src < (1ll << 31) && ld_dst < (1ll << 31), "ld_src, ld_dst");
    VBNN_REQUIRE(dtype == VBNN_F32 || dtype == VBNN_BF16, "dtype");
    const int es = dtype == VBNN_F32 ? 4 : 2, G = 16 / es;
    VBNN_REQUIRE(((uintptr_t)src % es) == 0 && ((uintptr_t)dst % es) == 0, "src, dst: aligned to the element");
    const int vec = vbnn_al16(src) && vbnn_al16(dst) && (ld_src % G) == 0 && (ld_dst % G) == 0;
    vbnn_cu_scope scope(ctx);
    const int nb = prop_grid(rows * ((cols + G - 1) / G));
    if (dtype == VBNN_F32)
        hipLaunchKernelGGL(k_square_shadow<float>, dim3(nb), dim3(256), 0, ctx->stream, (const float*)src, ld_src, rows, cols,
                           (float*)dst, ld_dst, vec);
    else
        hipLaunchKernelGGL(k_square_shadow<bf16_t>, dim3(nb), dim3(256), 0, ctx->stream, (const bf16_t*)src, ld_src, rows, cols,
                           (bf16_t*)dst, ld_dst, vec);
    return vbnn_check_launch("k_square_shadow");
    VBNN_API_END
}

// ------------------------------------------------------------------------------------------------ vbnn_logit_draws
// one thread per (draw, row, quad of columns): the quad's four normals are one Philox call
__global__ __launch_bounds__(256) void k_logit_draws(const vbnn_logit_draws_args p, int vec) {
    const int64_t quads = (p.C + 3) >> 2, per_draw = p.R * quads, total = p.S * per_draw;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t s = t / per_draw, e = t - s * per_draw, r = e / quads, qd = e - r * quads, col = 4 * qd;
        const int valid = (int)min((int64_t)4, p.C - col);
        const vbnn_f32x4 z = vbnn_normal4(p.seed, VBNN_STREAM_ZETA, p.layer, p.draw + (uint32_t)s, (uint32_t)(p.row0 + r), (uint32_t)qd);
        const float* pm = p.m + r * p.ld_m + col;
        const float* pv = p.v + r * p.ld_v + col;
        float y[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < valid) {
                const float sd = sqrtf(pv[j]);
                const float n = sd * z.v[j];
                y[j] = pm[j] + n;
            }
        prop_store(p.y + s * p.draw_stride + r * p.ld_y + col, y, valid, vec != 0);
    }
}

extern "C" int vbnn_logit_draws(vbnn_ctx* ctx, const vbnn_logit_draws_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a && a->m && a->v && a->y, "null argument (a, m, v, y)");
    VBNN_REQUIRE(a->R >= 1 && a->C >= 1 && a->S >= 1, "shape: R, C and S are at least 1");
    VBNN_REQUIRE(a->R < (1ll << 31) && a->C < (1ll << 31) && a->S < (1ll << 31), "shape: too large");
    VBNN_REQUIRE(a->layer < (1u << 24), "layer id range");
    VBNN_REQUIRE(a->ld_m >= a->C && a->ld_v >= a->C && a->ld_y >= a->C, "ld_m, ld_v, ld_y: a row holds C floats");
    VBNN_REQUIRE(a->ld_m < (1ll << 31) && a->ld_v < (1ll << 31), "ld_m, ld_v: too large");
    VBNN_REQUIRE(a->ld_y <= (1ll << 60) / a->R && a->draw_stride <= (1ll << 60) / a->S, "ld_y, draw_stride: too large");
    VBNN_REQUIRE(a->draw_stride >= a->R * a->ld_y, "draw_stride is at least R ld_y");
    const int vec = vbnn_al16(a->y) && (a->ld_y & 3) == 0 && (a->draw_stride & 3) == 0;
    vbnn_cu_scope scope(ctx);
    const int nb = prop_grid(a->S * a->R * ((a->C + 3) / 4));
    hipLaunchKernelGGL(k_logit_draws, dim3(nb), dim3(256), 0, ctx->stream, *a, vec);
    return vbnn_check_launch("k_logit_draws");
    VBNN_API_END
}
