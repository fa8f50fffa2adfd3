// quantiles.hip -- vbnn_predict_quantiles: the quantiles, the probability integral transform and the calibration counts of the
// regression predictive (include/vbnn_hip.h), the fourth member of the moments family (moments.hip). No MFMA, compiled WITHOUT
// floating-point contraction (Makefile).
//
// One thread works one element (r, d); a workgroup of T threads works a tile of T consecutive elements of the flattened
// R x D index, so consecutive threads read consecutive columns whatever D is. The S draws of the tile sit in LDS, draw-major
// (element i of draw s at [s T + i]: a thread walks its own column without a bank conflict), so every draw is read from HBM
// once whatever Q and the iteration count are. Where D, ld_y and draw_stride are multiples of 4 and the base is 16-byte
// aligned the tile is filled with 16-byte loads (a thread fills one quad of every fourth draw); otherwise every thread fills
// its own column with 4-byte loads. T follows S so that the tile fits 64 KiB of LDS: 256 threads while S (GAUSS: 2 S) <= 63, then 128, 64,
// and 32 for GAUSS at S = 128 alone.
//   EMPIRICAL: the column goes into NP = 2^k >= S registers (padded with +inf), a bitonic network sorts it (min / max only, no
//     data-dependent branch), the sorted column goes back to LDS where the interpolation picks a_k, a_{k+1} by a run-time k.
//   FIXED_NOISE, GAUSS: the column holds mu_s (and c_s = 1 / (sigma_s sqrt 2), formed in place from s); F is a running fp32
//     sum of erfcf over the column; the root search is per lane (q_mixture).
#include "device_prims.h"
#include <math.h>
#include <algorithm>

constexpr int Q_MAXQ = VBNN_QUANTILES_MAX_Q;
constexpr int Q_NEWTON_ITERS = 24;             // safeguarded Newton steps before the search turns to bisection on the bit patterns
constexpr int Q_MAX_ITERS = Q_NEWTON_ITERS + 33;
constexpr size_t Q_TILE_BYTES = 65536 - 256;   // the tile's share of a workgroup's 64 KiB of LDS
constexpr float Q_BRACKET_Z = 3.5f;            // Phi(-3.5) = 2.3e-4 < 0.001: [min mu - z sigma, max mu + z sigma] brackets every p allowed

struct QArgs {
    const float* y; int64_t ld_y, stride; const float* t; int64_t ld_t; int64_t R, D, total; int S, Q;
    float p[Q_MAXQ], zp[Q_MAXQ];               // the probabilities and their standard normal quantiles (the first guess)
    float c_fixed, sigma_fixed, s_min, s_max;
    float* q; int64_t ld_q, plane; float* pit; int64_t ld_pit; int* row_le; unsigned long long* count_le;
    int m_vec, s_vec;                          // 16-byte loads of the m (or y) half and of the s half
};

// fills one plane of the tile: lds[s T + i] = draw s of element e0 + i. Elements at or past a.total are not read.
__device__ __forceinline__ void q_fill(const QArgs& a, const float* base, bool vec, float* lds, int T, int64_t e0, bool act,
                                       int64_t r, int64_t d) {
    const int tid = threadIdx.x;
    if (vec) {                                             // D % 4 == 0: a quad never leaves its row, and total % 4 == 0
        const int qpt = T >> 2, qd = tid % qpt, s0 = tid / qpt;       // s0 = 0 .. 3
        const int64_t e = e0 + 4 * qd;
        if (e < a.total) {
            const int64_t rq = e / a.D, dq = e - rq * a.D;
            const float* p = base + rq * a.ld_y + dq;
            for (int s = s0; s < a.S; s += 4)
                *reinterpret_cast<f32x4*>(lds + s * T + 4 * qd) =
                    __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + (int64_t)s * a.stride));
        }
    } else if (act) {
        const float* p = base + r * a.ld_y + d;
        for (int s = 0; s < a.S; ++s) lds[s * T + tid] = __builtin_nontemporal_load(p + (int64_t)s * a.stride);
    }
}

// ---- what every kind does with quantile j of its element once it has it: the store, and with targets the counts. Called by
// every lane of the wave, active or not (it holds wave-wide operations). A wave whose elements share one row adds its row
// count once; a wave that spans rows adds per element. The grid-wide counts gather in LDS first.
struct QLane {
    bool act, has_t, one_row; int lane; int64_t r, d, rf; float tv;
};
__device__ __forceinline__ void q_emit(const QArgs& a, const QLane& w, int j, float qj, unsigned* cnt) {
    if (w.act && a.q) a.q[(int64_t)j * a.plane + w.r * a.ld_q + w.d] = qj;
    if (!w.has_t) return;                                  // launch-uniform
    const bool le = w.act && w.tv <= qj;                   // (a NaN on either side: false)
    const int c = __popcll(__ballot(le));
    if (a.count_le && w.lane == 0 && c > 0) atomicAdd(cnt + j, (unsigned)c);
    if (!a.row_le) return;
    if (w.one_row) {
        if (w.lane == 0 && c > 0) atomicAdd(a.row_le + w.rf * a.Q + j, c);
    } else if (le) {
        atomicAdd(a.row_le + w.r * a.Q + j, 1);
    }
}

// ---- EMPIRICAL: col = the thread's column of the tile (stride T). The bitonic network, one pass per instantiation so that
// every index is a constant and the column stays in registers.
template <int NP, int K, int J>
__device__ __forceinline__ void q_bitonic(float (&v)[NP]) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int l = i ^ J;
        if (l > i) {
            const float mn = fminf(v[i], v[l]), mx = fmaxf(v[i], v[l]);
            const bool up = (i & K) == 0;
            v[i] = up ? mn : mx;
            v[l] = up ? mx : mn;
        }
    }
    if constexpr (J > 1) q_bitonic<NP, K, J / 2>(v);
    else if constexpr (K < NP) q_bitonic<NP, 2 * K, K>(v);
}

template <int NP>
__device__ __forceinline__ void q_empirical(const QArgs& a, const QLane& w, float* col, int T, unsigned* cnt, const float* sp) {
    const int S = a.S;
    float v[NP];
    bool bad = false;
    int le = 0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        v[i] = i < S ? col[i * T] : INFINITY;
        bad = bad || v[i] != v[i];
        le += (w.has_t && i < S && v[i] <= w.tv) ? 1 : 0;
    }
    q_bitonic<NP, 2, 1>(v);
#pragma unroll
    for (int i = 0; i < NP; ++i)
        if (i < S) col[i * T] = v[i];                      // the thread's own column: it alone reads it back
    const float nan = __builtin_nanf("");
    for (int j = 0; j < a.Q; ++j) {
        float q;
        if (S == 1) {
            q = col[0];
        } else {
            const float pos = sp[j] * (float)(S - 1);
            const int k = min((int)pos, S - 2);
            const float frac = pos - (float)k;
            const float lo = col[k * T], hi = col[(k + 1) * T];
            q = fminf(lo + frac * (hi - lo), hi);          // (the minimum: rounding never lifts q above a_{k+1}, so q_j ascend)
        }
        q_emit(a, w, j, bad ? nan : q, cnt);
    }
    if (w.act && a.pit) a.pit[w.r * a.ld_pit + w.d] = (bad || w.tv != w.tv) ? nan : __fdiv_rn((float)le, (float)S);
}

// ---- the mixture kinds. sum_s erfcf((mu_s - x) c_s) = 2 S F(x), in draw order; with DERIV its derivative, for the Newton step
template <bool GAUSS, bool DERIV>
__device__ __forceinline__ float q_cdf_sum(const float* mu, const float* cs, float c_fixed, int S, int T, float x, float& dacc) {
    float acc = 0.f, dd = 0.f;
    for (int s = 0; s < S; ++s) {
        const float c = GAUSS ? cs[s * T] : c_fixed;
        const float z = (mu[s * T] - x) * c;
        acc = acc + erfcf(z);
        if (DERIV) dd = dd + c * __expf(-(z * z));
    }
    dacc = dd * 1.1283792f;                                // 2 / sqrt(pi)
    return acc;
}

template <bool GAUSS>
__device__ __forceinline__ void q_mixture(const QArgs& a, const QLane& w, const float* mu, float* cs, int T, unsigned* cnt, const float* sp) {
    const int S = a.S;
    const float nan = __builtin_nanf("");
    bool bad = !w.act;                                     // (a lane past the end: nothing to search)
    float lo = INFINITY, hi = -INFINITY, m1 = 0.f;
    for (int s = 0; s < S; ++s) {
        const float m = mu[s * T];
        float sg = a.sigma_fixed;
        if (GAUSS) {
            const float sv = cs[s * T];
            bad = bad || sv != sv;
            const float sc = fminf(fmaxf(sv, a.s_min), a.s_max);
            sg = expf(0.5f * sc);
            cs[s * T] = expf(-0.5f * sc) * 0.70710678f;    // 1 / (sigma sqrt 2)
        }
        bad = bad || m != m;
        lo = fminf(lo, m - Q_BRACKET_Z * sg);
        hi = fmaxf(hi, m + Q_BRACKET_Z * sg);
        m1 += m;
    }
    // the first guess: the Gaussian of the mixture's mean and variance
    const float mean = m1 / (float)S;
    float m2 = 0.f;
    for (int s = 0; s < S; ++s) {
        const float dm = mu[s * T] - mean;
        float var = a.sigma_fixed * a.sigma_fixed;
        if (GAUSS) { const float c = cs[s * T]; var = 0.5f / (c * c); }
        m2 += var + dm * dm;
    }
    const float sd = sqrtf(m2 / (float)S), twoS = 2.f * (float)S;
    float dacc;
    float L = lo;                                          // F32(L) < p_j: by the bracket for j = 0, by evaluation after
    for (int j = 0; j < a.Q; ++j) {
        const float p = sp[j];
        float H = hi;
        float x = mean + sp[Q_MAXQ + j] * sd;
        if (!bad) {
            for (int it = 0; it < Q_MAX_ITERS; ++it) {
                // the order words of the bracket's ends: adjacent floats are adjacent words
                const unsigned kl = vbnn_order_word(__float_as_uint(L)), kh = vbnn_order_word(__float_as_uint(H));
                if (kh - kl <= 1u) break;                  // adjacent floats: done (this lane; nobody else's result moves)
                const bool newton = it < Q_NEWTON_ITERS && kh - kl > 16u;
                if (!newton || !(x > L && x < H)) x = __uint_as_float(vbnn_unorder_word(kl + ((kh - kl) >> 1)));
                const float acc = newton ? q_cdf_sum<GAUSS, true>(mu, cs, a.c_fixed, S, T, x, dacc)
                                         : q_cdf_sum<GAUSS, false>(mu, cs, a.c_fixed, S, T, x, dacc);
                const bool below = __fdiv_rn(acc, twoS) < p;
                if (below) L = x; else H = x;
                if (newton) {
                    // the Newton step, pushed past its landing point by what the sum's own rounding is worth in x (two ulps
                    // of the sum at the root, 2 S p 2^-22, over the slope) and by two floats: near the root the next
                    // evaluation falls on the other side and the bracket closes from both ends
                    const float pad = (twoS * p * 2.4e-7f) / dacc;
                    float xn = (x + (twoS * p - acc) / dacc) + (below ? pad : -pad);
                    xn = __uint_as_float(vbnn_unorder_word(vbnn_order_word(__float_as_uint(xn)) + (below ? 2u : -2u)));
                    if (!(xn > L && xn < H)) xn = L + 0.5f * (H - L);
                    x = xn;                                // (still outside: the next turn takes the middle bit pattern)
                }
            }
        }
        // F32(L) < p_j < p_{j+1}: the next root starts above L, so q_{j+1} >= q_j
        q_emit(a, w, j, bad ? nan : H, cnt);
    }
    if (w.act && a.pit) {
        const float acc = q_cdf_sum<GAUSS, false>(mu, cs, a.c_fixed, S, T, w.tv, dacc);
        a.pit[w.r * a.ld_pit + w.d] = bad ? nan : __fdiv_rn(acc, twoS);        // (a NaN target: NaN)
    }
}

template <int KIND, int NP>
__global__ __launch_bounds__(256) void k_quantiles(const QArgs a) {
    extern __shared__ __attribute__((aligned(16))) float q_lds[];
    __shared__ unsigned cnt[Q_MAXQ];
    __shared__ float sp[2 * Q_MAXQ];                       // p and zp, read by a run-time j (from the by-value argument such an
                                                           // index would go through scratch memory)
    const int T = blockDim.x, tid = threadIdx.x;
    float* const pl0 = q_lds;
    float* const pl1 = q_lds + (size_t)a.S * T;            // GAUSS only
    const bool barrier = a.m_vec || (KIND == VBNN_QUANT_GAUSS && a.s_vec);   // launch-uniform: some thread fills another's column
    if (tid < Q_MAXQ) cnt[tid] = 0u;
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < Q_MAXQ; ++j) { sp[j] = a.p[j]; sp[Q_MAXQ + j] = a.zp[j]; }
    }
    __syncthreads();
    QLane w;
    w.lane = tid & 63; w.has_t = a.t != nullptr;
    const int64_t tiles = (a.total + T - 1) / T;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t e0 = tile * T, e = e0 + tid;
        w.act = e < a.total;
        w.r = w.act ? e / a.D : -1;
        w.d = w.act ? e - w.r * a.D : 0;
        q_fill(a, a.y, a.m_vec, pl0, T, e0, w.act, w.r, w.d);
        if (KIND == VBNN_QUANT_GAUSS) q_fill(a, a.y + a.D, a.s_vec, pl1, T, e0, w.act, w.r, w.d);
        if (barrier) __syncthreads();
        w.tv = (w.act && w.has_t) ? a.t[w.r * a.ld_t + w.d] : 0.f;
        w.rf = __shfl(w.r, 0, 64);                         // (lane 0 past the end: so is the whole wave)
        w.one_row = __all(!w.act || w.r == w.rf);
        if (KIND == VBNN_QUANT_EMPIRICAL) q_empirical<NP>(a, w, pl0 + tid, T, cnt, sp);
        else q_mixture<KIND == VBNN_QUANT_GAUSS>(a, w, pl0 + tid, pl1 + tid, T, cnt, sp);
        if (barrier) __syncthreads();                      // the next tile's fill writes other threads' columns
    }
    __syncthreads();
    if (a.count_le && tid < a.Q && cnt[tid] > 0u) atomicAdd(a.count_le + tid, (unsigned long long)cnt[tid]);
}

template <int KIND, int NP>
static void q_launch(int nb, int T, size_t lds, hipStream_t stream, const QArgs& m) {
    hipLaunchKernelGGL((k_quantiles<KIND, NP>), dim3(nb), dim3(T), lds, stream, m);
}

// the standard normal quantile, for the first guess of the root search (host, double: bisection on erfc)
static double q_norm_ppf(double p) {
    double lo = -6.0, hi = 6.0;
    for (int i = 0; i < 80; ++i) {
        const double mid = 0.5 * (lo + hi);
        if (0.5 * erfc(-mid * 0.70710678118654752440) < p) lo = mid; else hi = mid;
    }
    return 0.5 * (lo + hi);
}

extern "C" int vbnn_predict_quantiles(vbnn_ctx* ctx, const vbnn_quantiles_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a && a->y, "null argument (a, y)");
    VBNN_REQUIRE(a->R >= 1 && a->D >= 1, "shape: R and D are at least 1");
    VBNN_REQUIRE(a->R < (1ll << 31) && a->D < (1ll << 28), "shape: too large");
    VBNN_REQUIRE(a->S >= 1 && a->S <= VBNN_QUANTILES_MAX_S, "S outside [1, VBNN_QUANTILES_MAX_S]");
    VBNN_REQUIRE(a->Q >= 1 && a->Q <= VBNN_QUANTILES_MAX_Q, "Q outside [1, VBNN_QUANTILES_MAX_Q]");
    VBNN_REQUIRE(a->kind == VBNN_QUANT_EMPIRICAL || a->kind == VBNN_QUANT_FIXED_NOISE || a->kind == VBNN_QUANT_GAUSS, "kind");
    for (int j = 0; j < a->Q; ++j) {
        VBNN_REQUIRE(a->p[j] >= 0.001f && a->p[j] <= 0.999f, "p outside [0.001, 0.999]");
        VBNN_REQUIRE(j == 0 || a->p[j] > a->p[j - 1], "p is not strictly ascending");
    }
    const bool gauss = a->kind == VBNN_QUANT_GAUSS;
    const int64_t W = gauss ? 2 * a->D : a->D;
    VBNN_REQUIRE(a->ld_y >= W, "ld_y: a row holds D floats (GAUSS: 2 D)");
    // (no product below leaves int64: R ld_y < 2^60, S draw_stride < 2^60 floats, R D < 2^60, R ld_q and Q plane_stride likewise)
    VBNN_REQUIRE(a->ld_y <= (1ll << 60) / a->R && a->draw_stride <= (1ll << 60) / a->S, "ld_y, draw_stride: too large");
    VBNN_REQUIRE(a->draw_stride >= a->R * a->ld_y, "draw_stride is at least R ld_y");
    if (a->kind == VBNN_QUANT_FIXED_NOISE) VBNN_REQUIRE(a->noise_var > 0.f && std::isfinite(a->noise_var), "noise_var is above 0");
    if (gauss) VBNN_REQUIRE(a->s_min <= a->s_max, "s_min <= s_max");
    VBNN_REQUIRE(a->target || (!a->pit && !a->row_le && !a->count_le), "pit, row_le and count_le need a target");
    VBNN_REQUIRE(!a->target || (a->ld_t >= a->D && a->ld_t <= (1ll << 60) / a->R), "ld_t");
    VBNN_REQUIRE(!a->q || (a->ld_q >= a->D && a->ld_q <= (1ll << 60) / a->R && a->plane_stride <= (1ll << 60) / a->Q), "ld_q, plane_stride");
    VBNN_REQUIRE(!a->q || a->plane_stride >= (a->R - 1) * a->ld_q + a->D, "plane_stride holds a plane");
    VBNN_REQUIRE(!a->pit || (a->ld_pit >= a->D && a->ld_pit <= (1ll << 60) / a->R), "ld_pit");
    QArgs m;
    m.y = a->y; m.ld_y = a->ld_y; m.stride = a->draw_stride; m.t = a->target; m.ld_t = a->ld_t; m.R = a->R; m.D = a->D;
    m.total = a->R * a->D; m.S = (int)a->S; m.Q = a->Q;
    for (int j = 0; j < Q_MAXQ; ++j) {
        m.p[j] = j < a->Q ? a->p[j] : 0.f;
        m.zp[j] = j < a->Q ? (float)q_norm_ppf((double)a->p[j]) : 0.f;
    }
    const double nv = a->kind == VBNN_QUANT_FIXED_NOISE ? (double)a->noise_var : 1.0;
    m.c_fixed = (float)(1.0 / sqrt(2.0 * nv)); m.sigma_fixed = (float)sqrt(nv);
    m.s_min = a->s_min; m.s_max = a->s_max;
    m.q = a->q; m.ld_q = a->ld_q; m.plane = a->plane_stride; m.pit = a->pit; m.ld_pit = a->ld_pit; m.row_le = a->row_le;
    m.count_le = reinterpret_cast<unsigned long long*>(a->count_le);
    const bool quads = (a->D & 3) == 0 && (a->ld_y & 3) == 0 && (a->draw_stride & 3) == 0;
    m.m_vec = quads && vbnn_al16(a->y);
    m.s_vec = gauss && quads && vbnn_al16(a->y + a->D);
    // the tile: S draws (GAUSS: two planes) of T elements beside the kernel's few static words, in 64 KiB of LDS in all
    const int planes = gauss ? 2 : 1;
    int T = 256;                                           // (32: GAUSS at S = 128 alone -- half a wave idles)
    while ((size_t)m.S * planes * T * sizeof(float) > Q_TILE_BYTES) T >>= 1;
    const size_t lds = (size_t)m.S * planes * T * sizeof(float);
    vbnn_cu_scope scope(ctx);
    const int64_t tiles = (m.total + T - 1) / T;
    const int nb = (int)std::min<int64_t>(tiles, (int64_t)vbnn_cu_count() * 8);
    if (a->row_le) VBNN_CHECK_HIP(hipMemsetAsync(a->row_le, 0, (size_t)a->R * a->Q * sizeof(int32_t), ctx->stream));
    if (a->kind == VBNN_QUANT_FIXED_NOISE) q_launch<VBNN_QUANT_FIXED_NOISE, 1>(nb, T, lds, ctx->stream, m);
    else if (gauss) q_launch<VBNN_QUANT_GAUSS, 1>(nb, T, lds, ctx->stream, m);
    else if (m.S <= 4) q_launch<VBNN_QUANT_EMPIRICAL, 4>(nb, T, lds, ctx->stream, m);
    else if (m.S <= 8) q_launch<VBNN_QUANT_EMPIRICAL, 8>(nb, T, lds, ctx->stream, m);
    else if (m.S <= 16) q_launch<VBNN_QUANT_EMPIRICAL, 16>(nb, T, lds, ctx->stream, m);
    else if (m.S <= 32) q_launch<VBNN_QUANT_EMPIRICAL, 32>(nb, T, lds, ctx->stream, m);
    else if (m.S <= 64) q_launch<VBNN_QUANT_EMPIRICAL, 64>(nb, T, lds, ctx->stream, m);
    else q_launch<VBNN_QUANT_EMPIRICAL, 128>(nb, T, lds, ctx->stream, m);
    return vbnn_check_launch("k_quantiles");
    VBNN_API_END
}
