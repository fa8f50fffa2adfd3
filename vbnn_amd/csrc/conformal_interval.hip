// conformal_interval.hip -- vbnn_conformal_interval and vbnn_select_columns (include/vbnn_hip.h): split conformal prediction for
// a regression predictive. One expression serves three scores -- s = max(a - t, t - b) / w on a lower plane a, an upper plane b
// and an optional width w -- and one launch turns Q thresholds held ON THE DEVICE into the intervals [a - q w, b + q w] with the
// integer sums a test set's coverage is computed from. A member of the moments family: streaming, no MFMA, compiled WITHOUT
// floating-point contraction (Makefile): every line below is the fp32 operation it spells. Everything that accumulates across
// rows is an integer, so nothing depends on the grid, the arrival order, the chunking or the number of calls.
//
// k_interval / k_interval_score: k_calibration's mapping (calibration.hip). A group of G = 2^k <= 64 lanes owns a row (G covers
// the row's quads while D <= 256; a wave walks a wider row 64 quads a step), so a wave works 64 / G rows at once and nothing
// inside a row meets a barrier. The width and the target are loaded once a quad and ALL Q thresholds are compared against them
// in that one pass. What is summed over ELEMENTS stays in the lane's registers for the whole grid-stride loop; what is a ROW's
// (its covered outputs, whether it holds a NaN, its largest score) goes through a butterfly over the G lanes. After its last
// row a wave adds its sums to the workgroup's LDS copy of the accumulator, and the workgroup adds every nonzero word of that
// copy to global memory once: one workgroup of 16 waves per CU, grid-stride above (the closing adds serialise per word).
//
// k_select_columns: k_selective's radix walk (four 8-bit digits, the most significant first) for 16 neighbouring columns at
// once. A workgroup owns the tile: thread t reads column t & 15 of rows t >> 4, t >> 4 + 64, .. -- a row gives one 64-byte
// segment and a wave reads four rows an instruction. Per column the ranks' distinct prefixes are histogrammed SC_U at a time
// (uint32 LDS words [16][SC_U][256]); wave c then scans column c's histograms, one rank after the other, exactly as
// k_selective's waves do. Counts are integers: no order of the atomics matters.
#include "device_prims.h"
#include <math.h>
#include <algorithm>

typedef unsigned long long u64;

constexpr int CIV_T = 1024;                    // threads of a workgroup: 16 waves, each with rows of its own
// (more than one level a lane: 8 waves -- the budget of 256 registers keeps every level's sums and the loads the compiler
// puts in flight for them out of private memory; at the 133 and 196 registers they take ONE such workgroup is resident on a
// CU, so one per CU is what the host launches)
constexpr int civ_threads(int QB) { return QB == 1 ? 1024 : 512; }
constexpr int CIV_MAXQ = VBNN_CONFORMAL_MAX_Q;
constexpr int CIV_WORDS = 8 * CIV_MAXQ + 2;
constexpr unsigned CIV_QNAN = 0x7fc00000u;

struct CivArgs {
    const float* lower; const float* upper; int64_t ld, plane_stride; int P, Q;
    const float* scale; const float* scale2; int64_t ld_s; float scale_add; int is_var; float w_min; int per_column;
    const float* target; int64_t ld_t; int64_t R; int D;
    const float* qhat; int64_t ld_qhat;
    float* score; float* row_score; float* lo; float* hi; uint8_t* covered; int32_t* row_covered; u64* acc;
    int vec_in, vec_out;                       // 16-byte loads / stores on a row's whole quads (a partial quad goes element by element)
    int vec_cov;                               // a quad of covered bytes as one word
    int same;                                  // upper is lower: one load serves both
    int G;                                     // lanes per row
};

// columns c .. c + 3 of a row (c a multiple of 4, c < D); a column past D reads as +0 and is dropped by the caller
__device__ __forceinline__ void civ_load4(const float* rowp, int c, int D, bool vec, float (&v)[4]) {
    if (vec && c + 4 <= D) {
        const f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(rowp + c));
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = t[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (c + j < D) ? rowp[c + j] : 0.f;
    }
}
__device__ __forceinline__ void civ_store4(float* rowp, int c, int D, bool vec, const float (&v)[4]) {
    if (vec && c + 4 <= D) {
        __builtin_nontemporal_store(f32x4{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4*>(rowp + c));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c + j < D) rowp[c + j] = v[j];
    }
}

// the width of the header: the scale sum, its root for a variance, not below w_min; a NaN stays one
__device__ __forceinline__ float civ_width(const CivArgs& a, float s1, float s2) {
    float v = s1;
    if (a.scale2) v = v + s2;                  // launch-uniform
    v = v + a.scale_add;
    const float u = a.is_var ? sqrtf(v) : v;
    return u < a.w_min ? a.w_min : u;
}
// s = max(a - t, t - b) / w, NaN when either difference is
__device__ __forceinline__ float civ_score(bool scaled, float av, float bv, float tv, float w) {
    const float d1 = av - tv, d2 = tv - bv;
    float m = d1 > d2 ? d1 : d2;
    if (d1 != d1 || d2 != d2) m = __uint_as_float(CIV_QNAN);
    return scaled ? m / w : m;
}

// a wave's element sum into the workgroup's copy of word `i`
__device__ __forceinline__ void civ_flush(u64* sh, int i, unsigned v, int lane) {
    v = vbnn_wave_sum(v);
    if (lane == 0 && v) atomicAdd(&sh[i], (u64)v);
}

__global__ __launch_bounds__(CIV_T) void k_interval_score(const CivArgs a) {
    __shared__ u64 sh[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int D = a.D, G = a.G, li = lane & (G - 1), RW = 64 / G;
    const bool scaled = a.scale != nullptr;
    const float qn = __uint_as_float(CIV_QNAN);
    if (tid < 2) sh[tid] = 0ull;
    __syncthreads();
    unsigned n_nan_el = 0u, n_nan_row = 0u;
    const int64_t VR = (int64_t)a.P * a.R;     // a row of every plane pair
    const int64_t wave0 = (int64_t)blockIdx.x * (CIV_T / 64) + (tid >> 6), waves = (int64_t)gridDim.x * (CIV_T / 64);
    for (int64_t base = wave0 * RW; base < VR; base += waves * RW) {       // (wave-uniform; no barrier inside)
        const int64_t vr = base + lane / G;
        const bool act = vr < VR;
        const int64_t vrc = act ? vr : 0, p = vrc / a.R, r = vrc - p * a.R;
        const float* ap = a.lower + p * a.plane_stride + r * a.ld;
        const float* bp = a.upper + p * a.plane_stride + r * a.ld;
        const float* sp = scaled ? a.scale + r * a.ld_s : nullptr;
        const float* s2p = a.scale2 ? a.scale2 + r * a.ld_s : nullptr;
        const float* tp = a.target + r * a.ld_t;
        unsigned rmax = 0u;                    // the order word of the row's largest score (no score is below word 0)
        bool rnan = false;
        for (int c = act ? 4 * li : D; c < D; c += 4 * G) {
            float av[4], bv[4], s1[4], s2[4], tv[4], out[4];
            civ_load4(ap, c, D, a.vec_in, av);
            if (a.same) {
#pragma unroll
                for (int j = 0; j < 4; ++j) bv[j] = av[j];
            } else {
                civ_load4(bp, c, D, a.vec_in, bv);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) s1[j] = s2[j] = 1.f;
            if (scaled) civ_load4(sp, c, D, a.vec_in, s1);
            if (a.scale2) civ_load4(s2p, c, D, a.vec_in, s2);
            civ_load4(tp, c, D, a.vec_in, tv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float w = scaled ? civ_width(a, s1[j], s2[j]) : 1.f;
                const float s = civ_score(scaled, av[j], bv[j], tv[j], w);
                const bool isn = s != s, valid = c + j < D;
                out[j] = isn ? qn : s;
                if (valid) {
                    n_nan_el += isn ? 1u : 0u;
                    rnan |= isn;
                    if (!isn) rmax = max(rmax, vbnn_order_word(__float_as_uint(s)));
                }
            }
            if (a.score) civ_store4(a.score + vr * D, c, D, a.vec_out, out);
        }
        int rn = rnan ? 1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            if (off < G) {
                rmax = max(rmax, (unsigned)__shfl_xor((int)rmax, off, 64));
                rn |= __shfl_xor(rn, off, 64);
            }
        if (act && li == 0) {
            if (a.row_score) a.row_score[vr] = rn ? qn : __uint_as_float(vbnn_unorder_word(rmax));
            n_nan_row += (unsigned)rn;
        }
    }
    civ_flush(sh, 0, n_nan_el, lane);
    civ_flush(sh, 1, n_nan_row, lane);
    __syncthreads();
    if (a.acc && tid < 2 && sh[tid]) atomicAdd(a.acc + tid, sh[tid]);
}

// QB: the levels a lane keeps sums for (Q <= QB; the levels past Q are skipped by launch-uniform branches)
template <int QB>
__global__ __launch_bounds__(civ_threads(QB)) void k_interval(const CivArgs a) {
    constexpr int CIV_T = civ_threads(QB);
    __shared__ u64 sh[CIV_WORDS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int D = a.D, Q = a.Q, G = a.G, li = lane & (G - 1), RW = 64 / G;
    const bool scaled = a.scale != nullptr, has_t = a.target != nullptr, multi = a.P > 1;
    const float qn = __uint_as_float(CIV_QNAN), inf = __builtin_inff();
    static_assert(CIV_WORDS <= CIV_T, "a thread per accumulator word");
    for (int i = tid; i < CIV_WORDS; i += CIV_T) sh[i] = 0ull;
    __syncthreads();
    unsigned e_cnt[QB], e_cov[QB], e_emp[QB], r_cnt[QB], r_all[QB];
#pragma unroll
    for (int b = 0; b < QB; ++b) e_cnt[b] = e_cov[b] = e_emp[b] = r_cnt[b] = r_all[b] = 0u;
    unsigned n_nan_el = 0u, n_nan_row = 0u;
    const int64_t wave0 = (int64_t)blockIdx.x * (CIV_T / 64) + (tid >> 6), waves = (int64_t)gridDim.x * (CIV_T / 64);
    for (int64_t base = wave0 * RW; base < a.R; base += waves * RW) {      // (wave-uniform; no barrier inside)
        const int64_t r = base + lane / G;
        const bool act = r < a.R;
        const int64_t rc = act ? r : 0;
        const float* ap = a.lower + rc * a.ld;
        const float* bp = a.upper + rc * a.ld;
        const float* sp = scaled ? a.scale + rc * a.ld_s : nullptr;
        const float* s2p = a.scale2 ? a.scale2 + rc * a.ld_s : nullptr;
        const float* tp = has_t ? a.target + rc * a.ld_t : nullptr;
        int rcov[QB];
        unsigned rnan = 0u;                    // bit b: the row holds a NaN element at level b
#pragma unroll
        for (int b = 0; b < QB; ++b) rcov[b] = 0;
        for (int c = act ? 4 * li : D; c < D; c += 4 * G) {
            float s1[4], s2[4], tv[4], w[4], av[4] = {0.f, 0.f, 0.f, 0.f}, bv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) s1[j] = s2[j] = 1.f, tv[j] = 0.f;
            if (scaled) civ_load4(sp, c, D, a.vec_in, s1);
            if (a.scale2) civ_load4(s2p, c, D, a.vec_in, s2);
            if (has_t) civ_load4(tp, c, D, a.vec_in, tv);
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = scaled ? civ_width(a, s1[j], s2[j]) : 1.f;
#pragma unroll
            for (int b = 0; b < QB; ++b) {
                if (b >= Q) break;             // launch-uniform
                if (b == 0 || multi) {         // one plane pair for every level, or one per level
                    const int64_t po = multi ? (int64_t)b * a.plane_stride : 0;
                    civ_load4(ap + po, c, D, a.vec_in, av);
                    if (a.same) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) bv[j] = av[j];
                    } else {
                        civ_load4(bp + po, c, D, a.vec_in, bv);
                    }
                }
                const float* qp = a.qhat + (int64_t)b * a.ld_qhat;
                float lo[4], hi[4];
                unsigned cov4 = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool valid = c + j < D;
                    float q = a.per_column ? (valid ? qp[c + j] : 0.f) : qp[0];
                    q = (q != q) ? inf : q;    // a NaN threshold admits everything
                    const float s = has_t ? civ_score(scaled, av[j], bv[j], tv[j], w[j]) : 0.f;
                    const bool isn = av[j] != av[j] || bv[j] != bv[j] || w[j] != w[j] || s != s;
                    const float qw = scaled ? q * w[j] : q;
                    const float l = av[j] - qw, h = bv[j] + qw;
                    const bool cov = s <= q, emp = l > h;
                    lo[j] = isn ? qn : l;
                    hi[j] = isn ? qn : h;
                    cov4 |= (isn ? 255u : (cov ? 1u : 0u)) << (8 * j);
                    if (valid) {
                        if (isn) {
                            rnan |= 1u << b;
                            if (b == 0 || multi) n_nan_el += 1u;
                        } else {
                            e_cnt[b] += 1u;
                            e_emp[b] += emp ? 1u : 0u;
                            if (has_t && cov) { e_cov[b] += 1u; rcov[b] += 1; }
                        }
                    }
                }
                const int64_t o = ((int64_t)b * a.R + rc) * D;
                if (a.lo) civ_store4(a.lo + o, c, D, a.vec_out, lo);
                if (a.hi) civ_store4(a.hi + o, c, D, a.vec_out, hi);
                if (a.covered) {
                    if (a.vec_cov && c + 4 <= D) {
                        *reinterpret_cast<uint32_t*>(a.covered + o + c) = cov4;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (c + j < D) a.covered[o + c + j] = (uint8_t)(cov4 >> (8 * j));
                    }
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            if (off < G) {
                rnan |= (unsigned)__shfl_xor((int)rnan, off, 64);
                if (has_t) {
#pragma unroll
                    for (int b = 0; b < QB; ++b)
                        if (b < Q) rcov[b] += __shfl_xor(rcov[b], off, 64);
                }
            }
        if (act && li == 0) {
#pragma unroll
            for (int b = 0; b < QB; ++b) {
                if (b >= Q) break;
                const bool bad = (rnan >> b) & 1u;
                if (a.row_covered) a.row_covered[(int64_t)b * a.R + r] = bad ? -1 : rcov[b];
                r_cnt[b] += bad ? 0u : 1u;
                if (has_t) r_all[b] += (!bad && rcov[b] == D) ? 1u : 0u;
                if (b == 0 || multi) n_nan_row += bad ? 1u : 0u;
            }
        }
    }
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        if (b >= Q) break;
        civ_flush(sh, 8 * b + 0, e_cnt[b], lane);
        civ_flush(sh, 8 * b + 1, e_cov[b], lane);
        civ_flush(sh, 8 * b + 2, r_cnt[b], lane);
        civ_flush(sh, 8 * b + 3, r_all[b], lane);
        civ_flush(sh, 8 * b + 4, e_emp[b], lane);
    }
    civ_flush(sh, 8 * Q, n_nan_el, lane);
    civ_flush(sh, 8 * Q + 1, n_nan_row, lane);
    __syncthreads();
    // at most one global add per accumulator word and workgroup (words 1 and 3 stay zero without a target, 5 .. 7 always)
    if (a.acc && tid < 8 * Q + 2 && sh[tid]) atomicAdd(a.acc + tid, sh[tid]);
}

extern "C" int vbnn_conformal_interval(vbnn_ctx* ctx, const vbnn_conformal_interval_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a && a->lower && a->upper, "null argument (a, lower, upper)");
    VBNN_REQUIRE(a->P >= 1 && a->P <= VBNN_CONFORMAL_MAX_Q, "P outside [1, VBNN_CONFORMAL_MAX_Q]");
    VBNN_REQUIRE(a->Q >= 0 && a->Q <= VBNN_CONFORMAL_MAX_Q, "Q outside [0, VBNN_CONFORMAL_MAX_Q]");
    VBNN_REQUIRE(a->Q == 0 || a->P == 1 || a->P == a->Q, "P is 1 or Q in interval mode");
    VBNN_REQUIRE(a->Q == 0 || a->qhat, "qhat: the thresholds on the device (NULL only with Q = 0)");
    VBNN_REQUIRE(a->Q > 0 || a->target, "score mode (Q = 0) needs target");
    VBNN_REQUIRE(a->target || (!a->covered && !a->row_covered), "covered and row_covered need target");
    VBNN_REQUIRE(a->Q == 0 || (!a->score && !a->row_score), "score and row_score belong to score mode (Q = 0)");
    VBNN_REQUIRE(a->Q > 0 || (!a->lo && !a->hi && !a->covered && !a->row_covered), "lo, hi, covered and row_covered belong to interval mode (Q >= 1)");
    VBNN_REQUIRE(a->scale || !a->scale2, "scale2 needs scale");
    VBNN_REQUIRE(!a->scale || a->w_min > 0.f, "w_min is above 0");
    VBNN_REQUIRE(a->R >= 1 && a->D >= 1, "shape: R and D are at least 1");
    VBNN_REQUIRE(a->R < (1ll << 31) && a->D < (1ll << 28), "shape: too large");
    VBNN_REQUIRE(a->ld >= a->D && a->ld <= (1ll << 60) / a->R, "ld");
    VBNN_REQUIRE(a->plane_stride >= 0 && (a->P == 1 || a->plane_stride >= 1), "plane_stride");
    VBNN_REQUIRE(!a->scale || (a->ld_s >= a->D && a->ld_s <= (1ll << 60) / a->R), "ld_s");
    VBNN_REQUIRE(!a->target || (a->ld_t >= a->D && a->ld_t <= (1ll << 60) / a->R), "ld_t");
    VBNN_REQUIRE(a->Q == 0 || a->ld_qhat >= (a->per_column ? a->D : 1), "ld_qhat");
    const void* p4[] = {a->lower, a->upper, a->scale, a->scale2, a->target, a->qhat, a->score, a->row_score, a->lo, a->hi, a->row_covered};
    for (const void* p : p4) VBNN_REQUIRE(((uintptr_t)p & 3u) == 0, "pointers are 4-byte aligned");
    VBNN_REQUIRE(((uintptr_t)a->acc & 7u) == 0, "acc is 8-byte aligned");
    CivArgs m;
    m.lower = a->lower; m.upper = a->upper; m.ld = a->ld; m.plane_stride = a->P > 1 ? a->plane_stride : 0; m.P = a->P; m.Q = a->Q;
    m.scale = a->scale; m.scale2 = a->scale2; m.ld_s = a->ld_s; m.scale_add = a->scale_add; m.is_var = a->scale_is_variance != 0;
    m.w_min = a->w_min; m.per_column = a->per_column != 0; m.target = a->target; m.ld_t = a->ld_t; m.R = a->R; m.D = (int)a->D;
    m.qhat = a->qhat; m.ld_qhat = a->ld_qhat; m.score = a->score; m.row_score = a->row_score; m.lo = a->lo; m.hi = a->hi;
    m.covered = a->covered; m.row_covered = a->row_covered; m.acc = reinterpret_cast<u64*>(a->acc);
    m.vec_in = a->D >= 4 && (a->ld & 3) == 0 && (m.plane_stride & 3) == 0 && vbnn_al16(a->lower) && vbnn_al16(a->upper) &&
               (!a->scale || ((a->ld_s & 3) == 0 && vbnn_al16(a->scale) && vbnn_al16(a->scale2))) &&
               (!a->target || ((a->ld_t & 3) == 0 && vbnn_al16(a->target)));
    m.vec_out = (a->D & 3) == 0 && vbnn_al16(a->score) && vbnn_al16(a->lo) && vbnn_al16(a->hi);
    m.vec_cov = (a->D & 3) == 0 && ((uintptr_t)a->covered & 3u) == 0;
    m.same = a->lower == a->upper;
    const int64_t nq = (a->D + 3) >> 2;
    int G = 64;                                            // lanes per row: the row's quads, rounded up to a power of two
    if (a->D <= 256) { G = 1; while (G < nq) G <<= 1; }
    m.G = G;
    const int64_t rows = a->Q == 0 ? a->R * a->P : a->R;
    const int64_t wave_rows = (rows + 64 / G - 1) / (64 / G);              // a wave works 64 / G rows at once
    vbnn_cu_scope scope(ctx);
    // one workgroup per CU (what is resident: see civ_threads), grid-stride above
    const int T = a->Q <= 1 ? CIV_T : civ_threads(2);
    const int nb = (int)std::min<int64_t>((wave_rows + T / 64 - 1) / (T / 64), (int64_t)vbnn_cu_count());
    if (a->Q == 0) hipLaunchKernelGGL(k_interval_score, dim3(nb), dim3(T), 0, ctx->stream, m);
    else if (a->Q == 1) hipLaunchKernelGGL(k_interval<1>, dim3(nb), dim3(T), 0, ctx->stream, m);
    else if (a->Q <= 4) hipLaunchKernelGGL(k_interval<4>, dim3(nb), dim3(T), 0, ctx->stream, m);
    else hipLaunchKernelGGL(k_interval<8>, dim3(nb), dim3(T), 0, ctx->stream, m);
    return vbnn_check_launch("k_interval");
    VBNN_API_END
}

// ---- vbnn_select_columns
constexpr int SC_T = 1024;                     // threads of a workgroup: 16 columns by 64 rows a step
constexpr int SC_COLS = 16;
constexpr int SC_MAXQ = VBNN_SELECT_COLUMNS_MAX_Q;
constexpr int SC_U = 4;                        // distinct prefixes of a column histogrammed in one walk over the rows (64 KiB of LDS)
static_assert(SC_T / 64 == SC_COLS, "wave c scans column c's histograms");

struct ScArgs {
    const float* x; int64_t ld, R; int D, Q; unsigned k[SC_MAXQ]; float* tau; int64_t ld_tau; uint32_t* counts; uint32_t* n_nan;
};

__global__ __launch_bounds__(SC_T) void k_select_columns(const ScArgs a) {
    __shared__ unsigned hist[SC_COLS][SC_U][256];
    __shared__ unsigned pref[SC_MAXQ][SC_COLS];            // the digits of rank j's key found so far (the rest zero)
    __shared__ unsigned krem[SC_MAXQ][SC_COLS];            // rank j among the keys under its prefix, 1-based
    __shared__ unsigned below[SC_MAXQ][SC_COLS], tied[SC_MAXQ][SC_COLS];
    __shared__ unsigned upref[SC_MAXQ][SC_COLS];           // the column's distinct prefixes, and which of them rank j has
    __shared__ int lead[SC_MAXQ][SC_COLS];
    __shared__ int nu_s[SC_COLS];
    __shared__ unsigned nnan[SC_COLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = tid & (SC_COLS - 1), rl = tid >> 4;
    const int Q = a.Q;
    const int64_t c = (int64_t)blockIdx.x * SC_COLS + col;
    const bool colok = c < a.D;
    if (tid < SC_COLS) {
#pragma unroll
        for (int j = 0; j < SC_MAXQ; ++j) {    // (unrolled: a run-time index into the by-value argument would go through scratch)
            pref[j][tid] = 0u; krem[j][tid] = a.k[j]; below[j][tid] = 0u; tied[j][tid] = 0u;
        }
        nnan[tid] = 0u;
    }
    __syncthreads();
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned hi_mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
        if (tid < SC_COLS) {
            int nu = 0;
            for (int j = 0; j < Q; ++j) {
                int u = 0;
                while (u < nu && upref[u][tid] != pref[j][tid]) ++u;
                if (u == nu) upref[nu++][tid] = pref[j][tid];
                lead[j][tid] = u;
            }
            nu_s[tid] = nu;
        }
        __syncthreads();
        int numax = 0;
#pragma unroll
        for (int i = 0; i < SC_COLS; ++i) numax = max(numax, nu_s[i]);
        for (int u0 = 0; u0 < numax; u0 += SC_U) {
            for (int i = tid; i < SC_COLS * SC_U * 256; i += SC_T) (&hist[0][0][0])[i] = 0u;
            unsigned up[SC_U];
            const int nb = min(SC_U, nu_s[col] - u0);      // (zero or below: the column's prefixes are done)
#pragma unroll
            for (int u = 0; u < SC_U; ++u) up[u] = u < nb ? upref[u0 + u][col] : 0u;
            __syncthreads();
            if (colok && nb > 0) {
                unsigned nn = 0u;
                const float* xp = a.x + c;
                for (int64_t r = rl; r < a.R; r += SC_T / SC_COLS) {
                    const float f = xp[r * a.ld];          // the key: every NaN is the positive quiet NaN, above +inf
                    nn += (f != f) ? 1u : 0u;
                    const unsigned key = vbnn_order_word((f != f) ? CIV_QNAN : __float_as_uint(f));
                    const int digit = (int)((key >> shift) & 255u);
#pragma unroll
                    for (int u = 0; u < SC_U; ++u)
                        if (u < nb && ((key ^ up[u]) & hi_mask) == 0u) atomicAdd(&hist[col][u][digit], 1u);
                }
                if (pass == 0 && nn) atomicAdd(&nnan[col], nn);
            }
            __syncthreads();
            // wave w scans column w: lane l holds bins 4 l .. 4 l + 3; exactly one (lane, bin) holds the rank
            if ((int64_t)blockIdx.x * SC_COLS + wave < a.D) {
                for (int j = 0; j < Q; ++j) {
                    const int u = lead[j][wave] - u0;
                    if (u < 0 || u >= SC_U) continue;      // wave-uniform
                    const unsigned kr = krem[j][wave];
                    unsigned cnt[4];
#pragma unroll
                    for (int b = 0; b < 4; ++b) cnt[b] = hist[wave][u][4 * lane + b];
                    const unsigned cs = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
                    unsigned ce = vbnn_wave_scan_incl(cs) - cs;            // below this lane's first bin
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        if (kr > ce && kr <= ce + cnt[b]) {
                            pref[j][wave] |= (unsigned)(4 * lane + b) << shift;
                            krem[j][wave] = kr - ce;
                            below[j][wave] += ce;
                            tied[j][wave] = cnt[b];
                        }
                        ce += cnt[b];
                    }
                }
            }
            __syncthreads();
        }
    }
    if (tid < SC_COLS * Q && colok) {                      // (thread t: rank t >> 4 of column t & 15)
        const int j = tid >> 4;
        a.tau[(int64_t)j * a.ld_tau + c] = __uint_as_float(vbnn_unorder_word(pref[j][col]));
        if (a.counts) {
            a.counts[((int64_t)j * a.D + c) * 2 + 0] = below[j][col];
            a.counts[((int64_t)j * a.D + c) * 2 + 1] = tied[j][col];
        }
    }
    if (tid < SC_COLS && colok && a.n_nan) a.n_nan[c] = nnan[col];
}

extern "C" int vbnn_select_columns(vbnn_ctx* ctx, const vbnn_select_columns_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a && a->x && a->tau, "null argument (a, x, tau)");
    VBNN_REQUIRE(a->R >= 1 && a->R < (1ll << 31), "R outside [1, 2^31)");
    VBNN_REQUIRE(a->D >= 1 && a->D < (1ll << 31), "D outside [1, 2^31)");
    VBNN_REQUIRE(a->ld >= a->D && a->ld <= (1ll << 60) / a->R, "ld");
    VBNN_REQUIRE(a->ld_tau >= a->D, "ld_tau");
    VBNN_REQUIRE(a->Q >= 1 && a->Q <= VBNN_SELECT_COLUMNS_MAX_Q, "Q outside [1, VBNN_SELECT_COLUMNS_MAX_Q]");
    for (int j = 0; j < a->Q; ++j) VBNN_REQUIRE(a->k[j] >= 1 && a->k[j] <= a->R, "k outside [1, R]");
    const void* p4[] = {a->x, a->tau, a->counts, a->n_nan};
    for (const void* p : p4) VBNN_REQUIRE(((uintptr_t)p & 3u) == 0, "pointers are 4-byte aligned");
    ScArgs m;
    m.x = a->x; m.ld = a->ld; m.R = a->R; m.D = (int)a->D; m.Q = a->Q; m.tau = a->tau; m.ld_tau = a->ld_tau;
    m.counts = a->counts; m.n_nan = a->n_nan;
    for (int j = 0; j < SC_MAXQ; ++j) m.k[j] = j < a->Q ? (unsigned)a->k[j] : 1u;
    const int nb = (int)((a->D + SC_COLS - 1) / SC_COLS);
    hipLaunchKernelGGL(k_select_columns, dim3(nb), dim3(SC_T), 0, ctx->stream, m);
    return vbnn_check_launch("k_select_columns");
    VBNN_API_END
}
