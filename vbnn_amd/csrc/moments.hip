// moments.hip -- vbnn_predict_moments: the regression posterior predictive (include/vbnn_hip.h): Welford mean / M2 over the S
// draws of the final Linear's f32 outputs, per-row squared errors and the online logsumexp of the mixture's log density.
// vbnn_predict_gauss_moments (second half of the file): the same for the heteroscedastic Gaussian head, whose rows carry a
// log noise variance beside every mean; it shares the logsumexp below and the access, row-sum and partial-sum functions of moments_common.h.
// A streaming kernel: no MFMA, no LDS in the column loop; LDS only carries the four waves' row partials. Compiled WITHOUT
// floating-point contraction (Makefile): every line below is the fp32 operation it spells.
//
// A row is worked by TR threads: one wave while D <= 256 (four rows per workgroup), the whole workgroup above. Thread i owns
// the quads q = i, i + TR, ... (columns 4 q .. 4 q + 3) on the 16-byte AND on the scalar path, so a row sum's order depends on
// D alone. STACKED keeps mean / M2 / target of a thread's quads in registers across the draws (NQ quads: D <= 4 . 256 . NQ) and
// loads draw s + 1 while draw s is reduced; ACCUMULATE streams the state through NQ quads per thread at a time.
#include "moments_common.h"
#include <math.h>
#include <algorithm>

constexpr int MOM_NQ = 4;
static_assert(VBNN_MOMENTS_STACKED_MAX_D == 4 * 256 * MOM_NQ, "the STACKED form's register tile");

struct MomArgs {
    const float* y; int64_t ld_y; const float* t; int64_t ld_t; int64_t R, D; int S, draw; float noise_var;
    float* state; float* mean; float* var; int64_t ld_out; float* row_var; float* row_sq_err; float* row_log_lik; double* part;
    int y_vec, t_vec, o_vec, s_vec;            // 16-byte access allowed (s_vec: the state's rows alternate 16 / 8-byte alignment)
};

// ---- THE per-draw update, one quad: both forms call this and nothing else on a draw's elements
__device__ __forceinline__ void mom_draw_quad(const float (&y)[4], const float (&t)[4], bool has_t, int valid, float n,
                                              float (&mean)[4], float (&M2)[4], float& e) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < valid) {
            const float delta = y[j] - mean[j];
            mean[j] = mean[j] + __fdiv_rn(delta, n);
            M2[j] = M2[j] + delta * (y[j] - mean[j]);
            if (has_t) { const float df = t[j] - y[j]; e = e + df * df; }
        }
    }
}
// ... and on a draw's row values (one thread of the row)
__device__ __forceinline__ void mom_draw_row(float e, bool first, float c, float& sumE, float& L) {
    sumE = first ? e : sumE + e;
    if (c > 0.f) {
        const float a = -e * c;
        L = first ? a : fmaxf(L, a) + log1pf(expf(-fabsf(L - a)));       // a NaN passes through the |L - a| term
    }
}
__device__ __forceinline__ void mom_finish_quad(const float (&mean)[4], const float (&M2)[4], const float (&t)[4], bool has_t, int valid,
                                                float Sf, float (&var)[4], float& sq, float& vs) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        var[j] = 0.f;
        if (j < valid) {
            var[j] = __fdiv_rn(M2[j], Sf);
            vs = vs + var[j];
            if (has_t) { const float df = t[j] - mean[j]; sq = sq + df * df; }
        }
    }
}
// the row's finish (one thread of the row): the row outputs and the row's terms of the four totals
__device__ __forceinline__ void mom_finish_row(const MomArgs& a, int64_t r, float sq, float vs, float sumE, float L, double (&tot)[4]) {
    if (a.row_var) a.row_var[r] = __fdiv_rn(vs, (float)a.D);
    if (a.t && a.row_sq_err) a.row_sq_err[r] = sq;
    float ll = 0.f;
    if (a.t && a.noise_var > 0.f) {
        ll = L - logf((float)a.S) - (0.5f * (float)a.D) * logf(6.2831855f * a.noise_var);
        if (a.row_log_lik) a.row_log_lik[r] = ll;
    }
    tot[0] += (double)sq; tot[1] += (double)sumE; tot[2] += (double)ll; tot[3] += (double)vs;
}

template <int WPR>
__global__ __launch_bounds__(256) void k_moments_stacked(const MomArgs a) {
    constexpr int TR = 64 * WPR, RPB = 4 / WPR, NQ = WPR == 1 ? 1 : MOM_NQ;
    __shared__ float red[2][4];
    __shared__ double dred[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tr = WPR == 1 ? lane : (int)threadIdx.x;
    const int64_t nq = (a.D + 3) >> 2;
    const bool has_t = a.t != nullptr;
    const float c = a.noise_var > 0.f ? __fdiv_rn(0.5f, a.noise_var) : 0.f;
    const int ym = a.y_vec ? 2 : 0, tm = a.t_vec ? 2 : 0, om = a.o_vec ? 2 : 0;
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
    int valid[NQ];
    int64_t col[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const int64_t q = tr + (int64_t)k * TR;
        col[k] = 4 * q;
        valid[k] = q < nq ? (int)min((int64_t)4, a.D - 4 * q) : 0;
    }
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < a.R; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t r = r0 + (WPR == 1 ? wave : 0);
        if (r >= a.R) continue;                            // WPR == 1 only: a whole wave, and that path has no barrier in the loop
        float mean[NQ][4], M2[NQ][4], t[NQ][4], yc[NQ][4], yn[NQ][4];
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j) mean[k][j] = M2[k][j] = t[k][j] = yn[k][j] = 0.f;
            if (has_t) mom_load4<false>(a.t + r * a.ld_t + col[k], t[k], valid[k], tm);
            mom_load4<true>(a.y + r * a.ld_y + col[k], yc[k], valid[k], ym);
        }
        float sumE = 0.f, L = 0.f;
        for (int s = 0; s < a.S; ++s) {
            if (s + 1 < a.S) {
                const float* yr = a.y + ((int64_t)(s + 1) * a.R + r) * a.ld_y;
#pragma unroll
                for (int k = 0; k < NQ; ++k) mom_load4<true>(yr + col[k], yn[k], valid[k], ym);
            }
            float e[1] = {0.f};
#pragma unroll
            for (int k = 0; k < NQ; ++k) mom_draw_quad(yc[k], t[k], has_t, valid[k], (float)(s + 1), mean[k], M2[k], e[0]);
            if (has_t) {
                mom_row_sum<WPR, 1>(e, red, wave);
                if (tr == 0) mom_draw_row(e[0], s == 0, c, sumE, L);
            }
#pragma unroll
            for (int k = 0; k < NQ; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) yc[k][j] = yn[k][j];
        }
        float f[2] = {0.f, 0.f};                           // sum_d (t - mean)^2, sum_d var
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            float var[4];
            mom_finish_quad(mean[k], M2[k], t[k], has_t, valid[k], (float)a.S, var, f[0], f[1]);
            if (a.mean) mom_store4<false>(a.mean + r * a.ld_out + col[k], mean[k], valid[k], om);
            if (a.var) mom_store4<false>(a.var + r * a.ld_out + col[k], var, valid[k], om);
        }
        mom_row_sum<WPR, 2>(f, red, wave);
        if (tr == 0) mom_finish_row(a, r, f[0], f[1], sumE, L, tot);
    }
    mom_store_partials<WPR, 4>(a.part, tot, dred, wave, tr);
}

template <int WPR>
__global__ __launch_bounds__(256) void k_moments_accumulate(const MomArgs a) {
    constexpr int TR = 64 * WPR, RPB = 4 / WPR, NQ = WPR == 1 ? 1 : MOM_NQ;
    __shared__ float red[2][4];
    __shared__ double dred[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tr = WPR == 1 ? lane : (int)threadIdx.x;
    const int64_t nq = (a.D + 3) >> 2, W = 2 * a.D + 2;
    const bool has_t = a.t != nullptr, first = a.draw == 0, fin = a.draw == a.S - 1;
    const float c = a.noise_var > 0.f ? __fdiv_rn(0.5f, a.noise_var) : 0.f;
    const float n = (float)(a.draw + 1);
    const int ym = a.y_vec ? 2 : 0, tm = a.t_vec ? 2 : 0, om = a.o_vec ? 2 : 0;
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < a.R; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t r = r0 + (WPR == 1 ? wave : 0);
        if (r >= a.R) continue;                            // WPR == 1 only (see k_moments_stacked)
        float* st = a.state + r * W;                       // { mean[D], M2[D], sum e, L }: rows alternate 16 / 8-byte alignment
        const int sm = !a.s_vec ? 0 : (((uintptr_t)st & 15u) == 0 ? 2 : 1);
        float e[1] = {0.f};
        float f[2] = {0.f, 0.f};
        for (int64_t qb = 0; qb < nq; qb += (int64_t)NQ * TR) {
            float mean[NQ][4], M2[NQ][4], t[NQ][4], y[NQ][4];
            int valid[NQ];
            int64_t col[NQ];
#pragma unroll
            for (int k = 0; k < NQ; ++k) {                 // every load of the chunk in flight before the first use
                const int64_t q = qb + tr + (int64_t)k * TR;
                col[k] = 4 * q;
                valid[k] = q < nq ? (int)min((int64_t)4, a.D - 4 * q) : 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) mean[k][j] = M2[k][j] = t[k][j] = 0.f;
                if (!first) {
                    mom_load4<true>(st + col[k], mean[k], valid[k], sm);
                    mom_load4<true>(st + a.D + col[k], M2[k], valid[k], sm);
                }
                mom_load4<true>(a.y + r * a.ld_y + col[k], y[k], valid[k], ym);
                if (has_t) mom_load4<false>(a.t + r * a.ld_t + col[k], t[k], valid[k], tm);
            }
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                mom_draw_quad(y[k], t[k], has_t, valid[k], n, mean[k], M2[k], e[0]);
                mom_store4<true>(st + col[k], mean[k], valid[k], sm);
                mom_store4<true>(st + a.D + col[k], M2[k], valid[k], sm);
                if (fin) {
                    float var[4];
                    mom_finish_quad(mean[k], M2[k], t[k], has_t, valid[k], (float)a.S, var, f[0], f[1]);
                    if (a.mean) mom_store4<false>(a.mean + r * a.ld_out + col[k], mean[k], valid[k], om);
                    if (a.var) mom_store4<false>(a.var + r * a.ld_out + col[k], var, valid[k], om);
                }
            }
        }
        if (has_t) mom_row_sum<WPR, 1>(e, red, wave);
        float sumE = 0.f, L = 0.f;
        if (tr == 0) {                                     // the row's two running values: read, updated and written by one thread
            if (!first) { sumE = st[2 * a.D]; L = st[2 * a.D + 1]; }
            if (has_t) mom_draw_row(e[0], first, c, sumE, L);
            st[2 * a.D] = sumE; st[2 * a.D + 1] = L;
        }
        if (fin) {
            mom_row_sum<WPR, 2>(f, red, wave);
            if (tr == 0) mom_finish_row(a, r, f[0], f[1], sumE, L, tot);
        }
    }
    if (fin) mom_store_partials<WPR, 4>(a.part, tot, dred, wave, tr);
}

template <int NT>
__global__ __launch_bounds__(256) void k_moments_finish(const double* __restrict__ part, int nb, double* __restrict__ totals) {
    __shared__ double sh[NT][4];
    double v[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) v[k] = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256)
#pragma unroll
        for (int k = 0; k < NT; ++k) v[k] += part[(int64_t)k * nb + b];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < NT; ++k) v[k] += __shfl_xor(v[k], off, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < NT; ++k) sh[k][threadIdx.x >> 6] = v[k];
    __syncthreads();
    if (threadIdx.x < NT) totals[threadIdx.x] = ((sh[threadIdx.x][0] + sh[threadIdx.x][1]) + sh[threadIdx.x][2]) + sh[threadIdx.x][3];
}

extern "C" int vbnn_predict_moments(vbnn_ctx* ctx, const vbnn_moments_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a && a->y, "null argument (a, y)");
    VBNN_REQUIRE(a->R >= 1 && a->D >= 1 && a->S >= 1, "shape: R, D and S are at least 1");
    VBNN_REQUIRE(a->S < (1ll << 24) && a->D < (1ll << 28) && a->R < (1ll << 40), "shape: too large");
    VBNN_REQUIRE(a->form == VBNN_MOMENTS_STACKED || a->form == VBNN_MOMENTS_ACCUMULATE, "form");
    VBNN_REQUIRE(a->noise_var >= 0.f && a->noise_var <= 3.0e38f, "noise_var must be finite and not negative");
    VBNN_REQUIRE(a->ld_y >= a->D && (!a->target || a->ld_t >= a->D), "leading dimensions");
    VBNN_REQUIRE((!a->mean && !a->var) || a->ld_out >= a->D, "ld_out");
    VBNN_REQUIRE(a->target || (!a->row_sq_err && !a->row_log_lik && !a->totals), "row_sq_err, row_log_lik and totals need a target");
    VBNN_REQUIRE(!a->row_log_lik || a->noise_var > 0.f, "row_log_lik needs noise_var > 0");
    const bool stacked = a->form == VBNN_MOMENTS_STACKED;
    if (stacked) {
        VBNN_REQUIRE(a->D <= VBNN_MOMENTS_STACKED_MAX_D, "the STACKED form takes D <= VBNN_MOMENTS_STACKED_MAX_D: use ACCUMULATE");
    } else {
        VBNN_REQUIRE(a->state, "the ACCUMULATE form keeps its running values in `state`");
        VBNN_REQUIRE(a->draw >= 0 && a->draw < a->S, "draw outside [0, S)");
    }
    const bool fin = stacked || a->draw == a->S - 1;
    const bool d4 = (a->D & 3) == 0;
    auto al16 = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
    MomArgs m;
    m.y = a->y; m.ld_y = a->ld_y; m.t = a->target; m.ld_t = a->ld_t; m.R = a->R; m.D = a->D; m.S = (int)a->S;
    m.draw = stacked ? 0 : a->draw; m.noise_var = a->noise_var; m.state = stacked ? nullptr : a->state;
    m.mean = a->mean; m.var = a->var; m.ld_out = a->ld_out; m.row_var = a->row_var; m.row_sq_err = a->row_sq_err;
    m.row_log_lik = a->row_log_lik;
    m.y_vec = d4 && (a->ld_y & 3) == 0 && al16(a->y);
    m.t_vec = a->target && d4 && (a->ld_t & 3) == 0 && al16(a->target);
    m.o_vec = d4 && (a->ld_out & 3) == 0 && al16(a->mean) && al16(a->var);
    m.s_vec = !stacked && d4 && al16(a->state);
    const bool wave_rows = a->D <= 256;                    // one wave per row, four rows per workgroup; above: a workgroup per row
    vbnn_cu_scope scope(ctx);
    const int64_t groups = wave_rows ? (a->R + 3) / 4 : a->R;
    const int nb = (int)std::min<int64_t>(groups, (int64_t)vbnn_cu_count() * 8);   // ~8 workgroups per CU, grid-stride above
    const bool totals = fin && a->totals;
    VBNN_REQUIRE(!totals || (size_t)nb * 4 <= ctx->scratch_doubles, "reduction scratch");
    m.part = totals ? ctx->scratch : nullptr;
    if (stacked) {
        if (wave_rows) hipLaunchKernelGGL(k_moments_stacked<1>, dim3(nb), dim3(256), 0, ctx->stream, m);
        else hipLaunchKernelGGL(k_moments_stacked<4>, dim3(nb), dim3(256), 0, ctx->stream, m);
    } else {
        if (wave_rows) hipLaunchKernelGGL(k_moments_accumulate<1>, dim3(nb), dim3(256), 0, ctx->stream, m);
        else hipLaunchKernelGGL(k_moments_accumulate<4>, dim3(nb), dim3(256), 0, ctx->stream, m);
    }
    if (totals) hipLaunchKernelGGL(k_moments_finish<4>, dim3(1), dim3(256), 0, ctx->stream, ctx->scratch, nb, a->totals);
    return vbnn_check_launch("k_moments");
    VBNN_API_END
}

// =========================================================================== the heteroscedastic Gaussian head's moments
// A draw's row is { m[D], s[D] } (s = log noise variance). The thread that owns quad q of the m half owns quad q of the s half;
// the halves take their access path each (the s half starts at column D). STACKED carries mean / M2 / V / target of a quad
// and both halves of two draws: 32 registers per quad against the MSE form's 20. Two register tiles: GMOM_NQ quads per thread
// (179 VGPRs, two waves per SIMD) while D <= 4 . 256 . GMOM_NQ, GMOM_NQ_WIDE above (254 VGPRs + 60 AGPRs, one wave per SIMD) --
// the largest tile tried that builds without private memory and without VGPR spills (12 quads spill 4 VGPRs, 16 use private
// memory; 10 was not tried). Thread i owns quads i, i + T, ... under either tile, so the bits do not depend on the tile.
// These kernels are twins of k_moments_stacked / k_moments_accumulate above, loop for loop: a fix to the row loop of one
// belongs in the other too.
constexpr int GMOM_NQ = 4, GMOM_NQ_WIDE = 8;
static_assert(VBNN_GAUSS_MOMENTS_STACKED_MAX_D == 4 * 256 * GMOM_NQ_WIDE, "the Gaussian STACKED form's widest register tile");

struct GMomArgs {
    const float* y; int64_t ld_y; const float* t; int64_t ld_t; int64_t R, D; int S, draw; float s_min, s_max;
    float* state; float* mean; float* var; float* nvar; int64_t ld_out;
    float* row_var; float* row_nvar; float* row_sq_err; float* row_log_lik; double* part;
    int m_vec, sh_vec, t_vec, o_vec, s_vec;    // 16-byte access allowed: y's m half, y's s half, target, outputs, state
};

// ---- THE per-draw update, one quad of each half: both forms call this and nothing else on a draw's elements
__device__ __forceinline__ void gmom_draw_quad(const float (&m)[4], const float (&s)[4], const float (&t)[4], bool has_t, int valid,
                                               float n, bool first, float s_min, float s_max, float (&mean)[4], float (&M2)[4],
                                               float (&V)[4], float& q) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < valid) {
            const float delta = m[j] - mean[j];
            mean[j] = mean[j] + __fdiv_rn(delta, n);
            M2[j] = M2[j] + delta * (m[j] - mean[j]);
            const float sc = s[j] != s[j] ? s[j] : fminf(fmaxf(s[j], s_min), s_max);   // fmaxf / fminf drop a NaN: keep it
            const float v = expf(sc);
            V[j] = first ? v : V[j] + v;
            if (has_t) { const float w = expf(-sc); const float df = t[j] - m[j]; q = q + (sc + (df * df) * w); }
        }
    }
}
__device__ __forceinline__ void gmom_finish_quad(const float (&mean)[4], const float (&M2)[4], const float (&V)[4], const float (&t)[4],
                                                 bool has_t, int valid, float Sf, float (&var)[4], float (&nv)[4], float& sq, float& vs,
                                                 float& ns) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        var[j] = nv[j] = 0.f;
        if (j < valid) {
            var[j] = __fdiv_rn(M2[j], Sf);
            nv[j] = __fdiv_rn(V[j], Sf);
            vs = vs + var[j];
            ns = ns + nv[j];
            if (has_t) { const float df = t[j] - mean[j]; sq = sq + df * df; }
        }
    }
}
// the row's finish (one thread of the row): the row outputs and the row's terms of the five totals
__device__ __forceinline__ void gmom_finish_row(const GMomArgs& a, int64_t r, float sq, float vs, float ns, float sumN, float L,
                                                double (&tot)[5]) {
    if (a.row_var) a.row_var[r] = __fdiv_rn(vs, (float)a.D);
    if (a.row_nvar) a.row_nvar[r] = __fdiv_rn(ns, (float)a.D);
    if (a.t && a.row_sq_err) a.row_sq_err[r] = sq;
    float ll = 0.f;
    if (a.t) {
        ll = L - logf((float)a.S) - (0.5f * (float)a.D) * logf(6.2831855f);
        if (a.row_log_lik) a.row_log_lik[r] = ll;
    }
    tot[0] += (double)sq; tot[1] += (double)sumN; tot[2] += (double)ll; tot[3] += (double)vs; tot[4] += (double)ns;
}

template <int WPR, int TILE>
__global__ __launch_bounds__(256) void k_gauss_moments_stacked(const GMomArgs a) {
    constexpr int TR = 64 * WPR, RPB = 4 / WPR, NQ = WPR == 1 ? 1 : TILE;
    __shared__ float red[3][4];
    __shared__ double dred[5][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tr = WPR == 1 ? lane : (int)threadIdx.x;
    const int64_t nq = (a.D + 3) >> 2;
    const bool has_t = a.t != nullptr;
    const int mm = a.m_vec ? 2 : 0, hm = a.sh_vec ? 2 : 0, tm = a.t_vec ? 2 : 0, om = a.o_vec ? 2 : 0;
    double tot[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int valid[NQ];
    int64_t col[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const int64_t q = tr + (int64_t)k * TR;
        col[k] = 4 * q;
        valid[k] = q < nq ? (int)min((int64_t)4, a.D - 4 * q) : 0;
    }
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < a.R; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t r = r0 + (WPR == 1 ? wave : 0);
        if (r >= a.R) continue;                            // WPR == 1 only: a whole wave, and that path has no barrier in the loop
        float mean[NQ][4], M2[NQ][4], V[NQ][4], t[NQ][4], mc[NQ][4], sc[NQ][4], mn[NQ][4], sn[NQ][4];
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j) mean[k][j] = M2[k][j] = V[k][j] = t[k][j] = mn[k][j] = sn[k][j] = 0.f;
            if (has_t) mom_load4<false>(a.t + r * a.ld_t + col[k], t[k], valid[k], tm);
            mom_load4<true>(a.y + r * a.ld_y + col[k], mc[k], valid[k], mm);
            mom_load4<true>(a.y + r * a.ld_y + a.D + col[k], sc[k], valid[k], hm);
        }
        float sumN = 0.f, L = 0.f;
        for (int s = 0; s < a.S; ++s) {
            if (s + 1 < a.S) {
                const float* yr = a.y + ((int64_t)(s + 1) * a.R + r) * a.ld_y;
#pragma unroll
                for (int k = 0; k < NQ; ++k) {
                    mom_load4<true>(yr + col[k], mn[k], valid[k], mm);
                    mom_load4<true>(yr + a.D + col[k], sn[k], valid[k], hm);
                }
            }
            float q[1] = {0.f};
#pragma unroll
            for (int k = 0; k < NQ; ++k)
                gmom_draw_quad(mc[k], sc[k], t[k], has_t, valid[k], (float)(s + 1), s == 0, a.s_min, a.s_max, mean[k], M2[k], V[k], q[0]);
            if (has_t) {
                mom_row_sum<WPR, 1>(q, red, wave);
                if (tr == 0) mom_draw_row(0.5f * q[0], s == 0, 1.f, sumN, L);
            }
#pragma unroll
            for (int k = 0; k < NQ; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) { mc[k][j] = mn[k][j]; sc[k][j] = sn[k][j]; }
        }
        float f[3] = {0.f, 0.f, 0.f};                      // sum_d (t - mean)^2, sum_d var, sum_d noise_var
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            float var[4], nv[4];
            gmom_finish_quad(mean[k], M2[k], V[k], t[k], has_t, valid[k], (float)a.S, var, nv, f[0], f[1], f[2]);
            if (a.mean) mom_store4<false>(a.mean + r * a.ld_out + col[k], mean[k], valid[k], om);
            if (a.var) mom_store4<false>(a.var + r * a.ld_out + col[k], var, valid[k], om);
            if (a.nvar) mom_store4<false>(a.nvar + r * a.ld_out + col[k], nv, valid[k], om);
        }
        mom_row_sum<WPR, 3>(f, red, wave);
        if (tr == 0) gmom_finish_row(a, r, f[0], f[1], f[2], sumN, L, tot);
    }
    mom_store_partials<WPR, 5>(a.part, tot, dred, wave, tr);
}

template <int WPR>
__global__ __launch_bounds__(256) void k_gauss_moments_accumulate(const GMomArgs a) {
    constexpr int TR = 64 * WPR, RPB = 4 / WPR, NQ = WPR == 1 ? 1 : GMOM_NQ;
    __shared__ float red[3][4];
    __shared__ double dred[5][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tr = WPR == 1 ? lane : (int)threadIdx.x;
    const int64_t nq = (a.D + 3) >> 2, W = 3 * a.D + 2;
    const bool has_t = a.t != nullptr, first = a.draw == 0, fin = a.draw == a.S - 1;
    const float n = (float)(a.draw + 1);
    const int mm = a.m_vec ? 2 : 0, hm = a.sh_vec ? 2 : 0, tm = a.t_vec ? 2 : 0, om = a.o_vec ? 2 : 0;
    double tot[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < a.R; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t r = r0 + (WPR == 1 ? wave : 0);
        if (r >= a.R) continue;                            // WPR == 1 only (see k_moments_stacked)
        float* st = a.state + r * W;                       // { mean[D], M2[D], V[D], sum nll, L }: rows alternate 16 / 8-byte alignment
        const int sm = !a.s_vec ? 0 : (((uintptr_t)st & 15u) == 0 ? 2 : 1);
        float q[1] = {0.f};
        float f[3] = {0.f, 0.f, 0.f};
        for (int64_t qb = 0; qb < nq; qb += (int64_t)NQ * TR) {
            float mean[NQ][4], M2[NQ][4], V[NQ][4], t[NQ][4], m[NQ][4], s[NQ][4];
            int valid[NQ];
            int64_t col[NQ];
#pragma unroll
            for (int k = 0; k < NQ; ++k) {                 // every load of the chunk in flight before the first use
                const int64_t qq = qb + tr + (int64_t)k * TR;
                col[k] = 4 * qq;
                valid[k] = qq < nq ? (int)min((int64_t)4, a.D - 4 * qq) : 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) mean[k][j] = M2[k][j] = V[k][j] = t[k][j] = 0.f;
                if (!first) {
                    mom_load4<true>(st + col[k], mean[k], valid[k], sm);
                    mom_load4<true>(st + a.D + col[k], M2[k], valid[k], sm);
                    mom_load4<true>(st + 2 * a.D + col[k], V[k], valid[k], sm);
                }
                mom_load4<true>(a.y + r * a.ld_y + col[k], m[k], valid[k], mm);
                mom_load4<true>(a.y + r * a.ld_y + a.D + col[k], s[k], valid[k], hm);
                if (has_t) mom_load4<false>(a.t + r * a.ld_t + col[k], t[k], valid[k], tm);
            }
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                gmom_draw_quad(m[k], s[k], t[k], has_t, valid[k], n, first, a.s_min, a.s_max, mean[k], M2[k], V[k], q[0]);
                mom_store4<true>(st + col[k], mean[k], valid[k], sm);
                mom_store4<true>(st + a.D + col[k], M2[k], valid[k], sm);
                mom_store4<true>(st + 2 * a.D + col[k], V[k], valid[k], sm);
                if (fin) {
                    float var[4], nv[4];
                    gmom_finish_quad(mean[k], M2[k], V[k], t[k], has_t, valid[k], (float)a.S, var, nv, f[0], f[1], f[2]);
                    if (a.mean) mom_store4<false>(a.mean + r * a.ld_out + col[k], mean[k], valid[k], om);
                    if (a.var) mom_store4<false>(a.var + r * a.ld_out + col[k], var, valid[k], om);
                    if (a.nvar) mom_store4<false>(a.nvar + r * a.ld_out + col[k], nv, valid[k], om);
                }
            }
        }
        if (has_t) mom_row_sum<WPR, 1>(q, red, wave);
        float sumN = 0.f, L = 0.f;
        if (tr == 0) {                                     // the row's two running values: read, updated and written by one thread
            if (!first) { sumN = st[3 * a.D]; L = st[3 * a.D + 1]; }
            if (has_t) mom_draw_row(0.5f * q[0], first, 1.f, sumN, L);
            st[3 * a.D] = sumN; st[3 * a.D + 1] = L;
        }
        if (fin) {
            mom_row_sum<WPR, 3>(f, red, wave);
            if (tr == 0) gmom_finish_row(a, r, f[0], f[1], f[2], sumN, L, tot);
        }
    }
    if (fin) mom_store_partials<WPR, 5>(a.part, tot, dred, wave, tr);
}

extern "C" int vbnn_predict_gauss_moments(vbnn_ctx* ctx, const vbnn_gauss_moments_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a && a->y, "null argument (a, y)");
    VBNN_REQUIRE(a->R >= 1 && a->D >= 1 && a->S >= 1, "shape: R, D and S are at least 1");
    VBNN_REQUIRE(a->S < (1ll << 24) && a->D < (1ll << 27) && a->R < (1ll << 40), "shape: too large");
    VBNN_REQUIRE(a->form == VBNN_MOMENTS_STACKED || a->form == VBNN_MOMENTS_ACCUMULATE, "form");
    VBNN_REQUIRE(a->s_min <= a->s_max, "the clamp: s_min <= s_max");
    VBNN_REQUIRE(a->ld_y >= 2 * a->D && (!a->target || a->ld_t >= a->D), "leading dimensions (a row of y holds 2 D floats)");
    VBNN_REQUIRE((!a->mean && !a->var && !a->noise_var) || a->ld_out >= a->D, "ld_out");
    VBNN_REQUIRE(a->target || (!a->row_sq_err && !a->row_log_lik && !a->totals), "row_sq_err, row_log_lik and totals need a target");
    const bool stacked = a->form == VBNN_MOMENTS_STACKED;
    if (stacked) {
        VBNN_REQUIRE(a->D <= VBNN_GAUSS_MOMENTS_STACKED_MAX_D, "the STACKED form takes D <= VBNN_GAUSS_MOMENTS_STACKED_MAX_D: use ACCUMULATE");
    } else {
        VBNN_REQUIRE(a->state, "the ACCUMULATE form keeps its running values in `state`");
        VBNN_REQUIRE(a->draw >= 0 && a->draw < a->S, "draw outside [0, S)");
    }
    const bool fin = stacked || a->draw == a->S - 1;
    const bool d4 = (a->D & 3) == 0;
    auto al16 = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
    GMomArgs m;
    m.y = a->y; m.ld_y = a->ld_y; m.t = a->target; m.ld_t = a->ld_t; m.R = a->R; m.D = a->D; m.S = (int)a->S;
    m.draw = stacked ? 0 : a->draw; m.s_min = a->s_min; m.s_max = a->s_max; m.state = stacked ? nullptr : a->state;
    m.mean = a->mean; m.var = a->var; m.nvar = a->noise_var; m.ld_out = a->ld_out; m.row_var = a->row_var;
    m.row_nvar = a->row_noise_var; m.row_sq_err = a->row_sq_err; m.row_log_lik = a->row_log_lik;
    m.m_vec = d4 && (a->ld_y & 3) == 0 && al16(a->y);
    m.sh_vec = d4 && (a->ld_y & 3) == 0 && al16(a->y + a->D);          // the s half starts at column D
    m.t_vec = a->target && d4 && (a->ld_t & 3) == 0 && al16(a->target);
    m.o_vec = d4 && (a->ld_out & 3) == 0 && al16(a->mean) && al16(a->var) && al16(a->noise_var);
    m.s_vec = !stacked && d4 && al16(a->state);
    const bool wave_rows = a->D <= 256;                    // one wave per row, four rows per workgroup; above: a workgroup per row
    vbnn_cu_scope scope(ctx);
    const int64_t groups = wave_rows ? (a->R + 3) / 4 : a->R;
    const int nb = (int)std::min<int64_t>(groups, (int64_t)vbnn_cu_count() * 8);   // ~8 workgroups per CU, grid-stride above
    const bool totals = fin && a->totals;
    VBNN_REQUIRE(!totals || (size_t)nb * 5 <= ctx->scratch_doubles, "reduction scratch");
    m.part = totals ? ctx->scratch : nullptr;
    if (stacked) {
        if (wave_rows) hipLaunchKernelGGL((k_gauss_moments_stacked<1, GMOM_NQ>), dim3(nb), dim3(256), 0, ctx->stream, m);
        else if (a->D <= 4 * 256 * GMOM_NQ) hipLaunchKernelGGL((k_gauss_moments_stacked<4, GMOM_NQ>), dim3(nb), dim3(256), 0, ctx->stream, m);
        else hipLaunchKernelGGL((k_gauss_moments_stacked<4, GMOM_NQ_WIDE>), dim3(nb), dim3(256), 0, ctx->stream, m);
    } else {
        if (wave_rows) hipLaunchKernelGGL(k_gauss_moments_accumulate<1>, dim3(nb), dim3(256), 0, ctx->stream, m);
        else hipLaunchKernelGGL(k_gauss_moments_accumulate<4>, dim3(nb), dim3(256), 0, ctx->stream, m);
    }
    if (totals) hipLaunchKernelGGL(k_moments_finish<5>, dim3(1), dim3(256), 0, ctx->stream, ctx->scratch, nb, a->totals);
    return vbnn_check_launch("k_gauss_moments");
    VBNN_API_END
}
