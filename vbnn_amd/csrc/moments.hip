// moments.hip -- vbnn_predict_moments: the regression posterior predictive (include/vbnn_hip.h): Welford mean / M2 over the S
// draws of the final Linear's f32 outputs, per-row squared errors and the online logsumexp of the mixture's log density.
// vbnn_predict_gauss_moments: the same for the heteroscedastic Gaussian head, whose rows carry a log noise variance beside
// every mean. One STACKED and one ACCUMULATE kernel serve both, templated on the family (MseFamily, GaussFamily): its counts
// and its element and row functions; the access, tile, row-sum, partial-sum and launch-plan pieces are moments_common.h's.
// A streaming kernel: no MFMA, no LDS in the column loop; LDS only carries the four waves' row partials. Compiled WITHOUT
// floating-point contraction (Makefile): every line below is the fp32 operation it spells.
//
// A row is worked by TR threads: one wave while D <= 256 (four rows per workgroup), the whole workgroup above. Thread i owns
// the quads q = i, i + TR, ... (columns 4 q .. 4 q + 3) on the 16-byte AND on the scalar path, so a row sum's order depends on
// D alone. STACKED keeps the state planes and the target of a thread's quads in registers across the draws (NQ quads:
// D <= 4 . 256 . NQ) and loads draw s + 1 while draw s is reduced; ACCUMULATE streams the state through MOM_NQ quads per thread
// at a time.
#include "moments_common.h"
#include <math.h>

constexpr int MOM_NQ = 4;

struct MomArgs {
    const float* y; int64_t ld_y; const float* t; int64_t ld_t; int64_t R, D; int S, draw; float noise_var, s_min, s_max;
    float* state; float* mean; float* var; float* nvar; int64_t ld_out;
    float* row_var; float* row_nvar; float* row_sq_err; float* row_log_lik; double* part;
    // 16-byte access allowed: y's first half, y's s half (Gaussian), target, outputs, state (its rows alternate 16 / 8-byte alignment)
    int y_vec, sh_vec, t_vec, o_vec, s_vec;
};

// ---- on a draw's row value (one thread of the row; both families): the running sum and the online logsumexp of -e c
__device__ __forceinline__ void mom_draw_row(float e, bool first, float c, float& sumE, float& L) {
    sumE = first ? e : sumE + e;
    if (c > 0.f) {
        const float a = -e * c;
        L = first ? a : fmaxf(L, a) + log1pf(expf(-fabsf(L - a)));       // a NaN passes through the |L - a| term
    }
}

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

// A family: HALVES quads of y per quad of the row, PLANES state planes (plane 0 the mean; the finish derives one output plane
// from each of the others), SUMS row sums at the finish { sum_d (t - mean)^2, sum_d of each derived plane }, NT totals; a row
// of the state is { the planes, D floats each, the draws' running sum, L }.
struct MseFamily {
    static constexpr int HALVES = 1, PLANES = 2, SUMS = 2, NT = 4, NQ_WIDE = MOM_NQ;
    static __device__ __forceinline__ void draw_quad(const MomArgs&, const float (&y)[1][4], const float (&t)[4], bool has_t, int valid,
                                                     float n, bool, float (&st)[2][4], float& e) {
        mom_draw_quad(y[0], t, has_t, valid, n, st[0], st[1], e);
    }
    static __device__ __forceinline__ void finish_quad(const float (&st)[2][4], const float (&t)[4], bool has_t, int valid, float Sf,
                                                       float (&out)[1][4], float (&f)[2]) {
        mom_finish_quad(st[0], st[1], t, has_t, valid, Sf, out[0], f[0], f[1]);
    }
    // mom_draw_row's term and scale: e_s and 1 / 2 tau^2 (0: no log-likelihood)
    static __device__ __forceinline__ float row_term(float e) { return e; }
    static __device__ __forceinline__ float row_scale(const MomArgs& a) { return a.noise_var > 0.f ? __fdiv_rn(0.5f, a.noise_var) : 0.f; }
    // the row's finish (one thread of the row): the row outputs and the row's terms of the four totals
    static __device__ __forceinline__ void finish_row(const MomArgs& a, int64_t r, const float (&f)[2], float sumE, float L, double (&tot)[4]) {
        const float sq = f[0], vs = f[1];
        if (a.row_var) a.row_var[r] = __fdiv_rn(vs, (float)a.D);
        if (a.t && a.row_sq_err) a.row_sq_err[r] = sq;
        float ll = 0.f;
        if (a.t && a.noise_var > 0.f) {
            ll = L - logf((float)a.S) - (0.5f * (float)a.D) * logf(6.2831855f * a.noise_var);
            if (a.row_log_lik) a.row_log_lik[r] = ll;
        }
        tot[0] += (double)sq; tot[1] += (double)sumE; tot[2] += (double)ll; tot[3] += (double)vs;
    }
    // host side: the entry point's own requirements and fields
    using Api = vbnn_moments_args;
    static constexpr const char* WHAT = "k_moments";
    static constexpr const char* LD_MSG = "leading dimensions";
    static constexpr const char* CAP_MSG = "the STACKED form takes D <= VBNN_MOMENTS_STACKED_MAX_D: use ACCUMULATE";
    static int own(const Api& a, bool, MomArgs& m) {
        VBNN_REQUIRE(a.noise_var >= 0.f && a.noise_var <= 3.0e38f, "noise_var must be finite and not negative");
        VBNN_REQUIRE(!a.row_log_lik || a.noise_var > 0.f, "row_log_lik needs noise_var > 0");
        m.noise_var = a.noise_var;
        return VBNN_OK;
    }
};

// ---- the heteroscedastic Gaussian head: a draw's row is { m[D], s[D] } (s = log noise variance), the planes mean / M2 / V.
// The thread that owns quad q of the m half owns quad q of the s half; the halves take their access path each (the s half
// starts at column D). THE per-draw update, one quad of each half:
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

// STACKED carries 32 registers per quad (three planes, target, both halves of two draws) against the MSE form's 20, in two
// register tiles: MOM_NQ quads per thread while D <= 4 . 256 . MOM_NQ (two waves per SIMD), NQ_WIDE above (one wave per SIMD,
// AGPRs in use) -- the largest tile tried that builds without private memory and without VGPR spills (12 quads spill 4 VGPRs,
// 16 use private memory; 10 was not tried). Thread i owns quads i, i + T, ... under either tile, so the bits do not depend on it.
struct GaussFamily {
    static constexpr int HALVES = 2, PLANES = 3, SUMS = 3, NT = 5, NQ_WIDE = 8;
    static __device__ __forceinline__ void draw_quad(const MomArgs& a, const float (&y)[2][4], const float (&t)[4], bool has_t, int valid,
                                                     float n, bool first, float (&st)[3][4], float& q) {
        gmom_draw_quad(y[0], y[1], t, has_t, valid, n, first, a.s_min, a.s_max, st[0], st[1], st[2], q);
    }
    static __device__ __forceinline__ void finish_quad(const float (&st)[3][4], const float (&t)[4], bool has_t, int valid, float Sf,
                                                       float (&out)[2][4], float (&f)[3]) {
        gmom_finish_quad(st[0], st[1], st[2], t, has_t, valid, Sf, out[0], out[1], f[0], f[1], f[2]);
    }
    // mom_draw_row's term and scale: nll_s = q_s / 2 as it stands
    static __device__ __forceinline__ float row_term(float q) { return 0.5f * q; }
    static __device__ __forceinline__ float row_scale(const MomArgs&) { return 1.f; }
    // the row's finish (one thread of the row): the row outputs and the row's terms of the five totals
    static __device__ __forceinline__ void finish_row(const MomArgs& a, int64_t r, const float (&f)[3], float sumN, float L, double (&tot)[5]) {
        const float sq = f[0], vs = f[1], ns = f[2];
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
    using Api = vbnn_gauss_moments_args;
    static constexpr const char* WHAT = "k_gauss_moments";
    static constexpr const char* LD_MSG = "leading dimensions (a row of y holds 2 D floats)";
    static constexpr const char* CAP_MSG = "the STACKED form takes D <= VBNN_GAUSS_MOMENTS_STACKED_MAX_D: use ACCUMULATE";
    static int own(const Api& a, bool d4, MomArgs& m) {
        VBNN_REQUIRE(a.s_min <= a.s_max, "the clamp: s_min <= s_max");
        m.s_min = a.s_min; m.s_max = a.s_max; m.nvar = a.noise_var; m.row_nvar = a.row_noise_var;
        m.sh_vec = d4 && (a.ld_y & 3) == 0 && vbnn_al16(a.y + a.D);      // the s half starts at column D
        return VBNN_OK;
    }
};
static_assert(VBNN_MOMENTS_STACKED_MAX_D == 4 * 256 * MseFamily::NQ_WIDE, "the STACKED form's register tile");
static_assert(VBNN_GAUSS_MOMENTS_STACKED_MAX_D == 4 * 256 * GaussFamily::NQ_WIDE, "the Gaussian STACKED form's widest register tile");

template <typename F, int WPR, int TILE>
__global__ __launch_bounds__(256) void k_moments_stacked(const MomArgs a) {
    constexpr int TR = 64 * WPR, RPB = 4 / WPR, NQ = WPR == 1 ? 1 : TILE, H = F::HALVES, P = F::PLANES;
    __shared__ float red[F::SUMS][4];
    __shared__ double dred[F::NT][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tr = WPR == 1 ? lane : (int)threadIdx.x;
    const bool has_t = a.t != nullptr;
    const float c = F::row_scale(a);
    const int ym[2] = {a.y_vec ? 2 : 0, a.sh_vec ? 2 : 0}, tm = a.t_vec ? 2 : 0, om = a.o_vec ? 2 : 0;
    float* const derived[2] = {a.var, a.nvar};
    double tot[F::NT] = {};
    int valid[NQ];
    int64_t col[NQ];
    mom_tile<NQ, TR>((int64_t)tr, a.D, valid, col);
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < a.R; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t r = r0 + (WPR == 1 ? wave : 0);
        if (r >= a.R) continue;                            // WPR == 1 only: a whole wave, and that path has no barrier in the loop
        float st[NQ][P][4], t[NQ][4], yc[NQ][H][4], yn[NQ][H][4];
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                t[k][j] = 0.f;
#pragma unroll
                for (int p = 0; p < P; ++p) st[k][p][j] = 0.f;
#pragma unroll
                for (int h = 0; h < H; ++h) yn[k][h][j] = 0.f;
            }
            if (has_t) mom_load4<false>(a.t + r * a.ld_t + col[k], t[k], valid[k], tm);
#pragma unroll
            for (int h = 0; h < H; ++h) mom_load4<true>(a.y + r * a.ld_y + h * a.D + col[k], yc[k][h], valid[k], ym[h]);
        }
        float sumE = 0.f, L = 0.f;
        for (int s = 0; s < a.S; ++s) {
            if (s + 1 < a.S) {
                const float* yr = a.y + ((int64_t)(s + 1) * a.R + r) * a.ld_y;
#pragma unroll
                for (int k = 0; k < NQ; ++k)
#pragma unroll
                    for (int h = 0; h < H; ++h) mom_load4<true>(yr + h * a.D + col[k], yn[k][h], valid[k], ym[h]);
            }
            float e[1] = {0.f};
#pragma unroll
            for (int k = 0; k < NQ; ++k) F::draw_quad(a, yc[k], t[k], has_t, valid[k], (float)(s + 1), s == 0, st[k], e[0]);
            if (has_t) {
                mom_row_sum<WPR, 1>(e, red, wave);
                if (tr == 0) mom_draw_row(F::row_term(e[0]), s == 0, c, sumE, L);
            }
#pragma unroll
            for (int k = 0; k < NQ; ++k)
#pragma unroll
                for (int h = 0; h < H; ++h)
#pragma unroll
                    for (int j = 0; j < 4; ++j) yc[k][h][j] = yn[k][h][j];
        }
        float f[F::SUMS] = {};
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            float out[P - 1][4];                           // the mean leaves from its state plane
            F::finish_quad(st[k], t[k], has_t, valid[k], (float)a.S, out, f);
            if (a.mean) mom_store4<false>(a.mean + r * a.ld_out + col[k], st[k][0], valid[k], om);
#pragma unroll
            for (int p = 0; p < P - 1; ++p)
                if (derived[p]) mom_store4<false>(derived[p] + r * a.ld_out + col[k], out[p], valid[k], om);
        }
        mom_row_sum<WPR, F::SUMS>(f, red, wave);
        if (tr == 0) F::finish_row(a, r, f, sumE, L, tot);
    }
    mom_store_partials<WPR, F::NT>(a.part, tot, dred, wave, tr);
}

template <typename F, int WPR>
__global__ __launch_bounds__(256) void k_moments_accumulate(const MomArgs a) {
    constexpr int TR = 64 * WPR, RPB = 4 / WPR, NQ = WPR == 1 ? 1 : MOM_NQ, H = F::HALVES, P = F::PLANES;
    __shared__ float red[F::SUMS][4];
    __shared__ double dred[F::NT][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tr = WPR == 1 ? lane : (int)threadIdx.x;
    const int64_t nq = (a.D + 3) >> 2, W = P * a.D + 2;
    const bool has_t = a.t != nullptr, first = a.draw == 0, fin = a.draw == a.S - 1;
    const float c = F::row_scale(a);
    const float n = (float)(a.draw + 1);
    const int ym[2] = {a.y_vec ? 2 : 0, a.sh_vec ? 2 : 0}, tm = a.t_vec ? 2 : 0, om = a.o_vec ? 2 : 0;
    float* const derived[2] = {a.var, a.nvar};
    double tot[F::NT] = {};
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < a.R; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t r = r0 + (WPR == 1 ? wave : 0);
        if (r >= a.R) continue;                            // WPR == 1 only (see k_moments_stacked)
        float* sr = a.state + r * W;                       // { P planes of D, the draws' sum, L }: rows alternate 16 / 8-byte alignment
        const int sm = !a.s_vec ? 0 : (((uintptr_t)sr & 15u) == 0 ? 2 : 1);
        float e[1] = {0.f};
        float f[F::SUMS] = {};
        for (int64_t qb = 0; qb < nq; qb += (int64_t)NQ * TR) {
            float st[NQ][P][4], t[NQ][4], y[NQ][H][4];
            int valid[NQ];
            int64_t col[NQ];
            mom_tile<NQ, TR>(qb + tr, a.D, valid, col);
#pragma unroll
            for (int k = 0; k < NQ; ++k) {                 // every load of the chunk in flight before the first use
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    t[k][j] = 0.f;
#pragma unroll
                    for (int p = 0; p < P; ++p) st[k][p][j] = 0.f;
                }
                if (!first)
#pragma unroll
                    for (int p = 0; p < P; ++p) mom_load4<true>(sr + p * a.D + col[k], st[k][p], valid[k], sm);
#pragma unroll
                for (int h = 0; h < H; ++h) mom_load4<true>(a.y + r * a.ld_y + h * a.D + col[k], y[k][h], valid[k], ym[h]);
                if (has_t) mom_load4<false>(a.t + r * a.ld_t + col[k], t[k], valid[k], tm);
            }
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                F::draw_quad(a, y[k], t[k], has_t, valid[k], n, first, st[k], e[0]);
#pragma unroll
                for (int p = 0; p < P; ++p) mom_store4<true>(sr + p * a.D + col[k], st[k][p], valid[k], sm);
                if (fin) {
                    float out[P - 1][4];
                    F::finish_quad(st[k], t[k], has_t, valid[k], (float)a.S, out, f);
                    if (a.mean) mom_store4<false>(a.mean + r * a.ld_out + col[k], st[k][0], valid[k], om);
#pragma unroll
                    for (int p = 0; p < P - 1; ++p)
                        if (derived[p]) mom_store4<false>(derived[p] + r * a.ld_out + col[k], out[p], valid[k], om);
                }
            }
        }
        if (has_t) mom_row_sum<WPR, 1>(e, red, wave);
        float sumE = 0.f, L = 0.f;
        if (tr == 0) {                                     // the row's two running values: read, updated and written by one thread
            if (!first) { sumE = sr[P * a.D]; L = sr[P * a.D + 1]; }
            if (has_t) mom_draw_row(F::row_term(e[0]), first, c, sumE, L);
            sr[P * a.D] = sumE; sr[P * a.D + 1] = L;
        }
        if (fin) {
            mom_row_sum<WPR, F::SUMS>(f, red, wave);
            if (tr == 0) F::finish_row(a, r, f, sumE, L, tot);
        }
    }
    if (fin) mom_store_partials<WPR, F::NT>(a.part, tot, dred, wave, tr);
}

// ---- the entry points' shared body (F::Api names the fields the two argument structs share alike); F::own checks and sets the
// family's own
template <typename F>
static int mom_predict(vbnn_ctx* ctx, const typename F::Api* a) {
    VBNN_REQUIRE(ctx && a && a->y, "null argument (a, y)");
    VBNN_REQUIRE(a->R >= 1 && a->D >= 1 && a->S >= 1, "shape: R, D and S are at least 1");
    VBNN_REQUIRE(a->S < (1ll << 24) && a->D < (1ll << 28) / F::HALVES && a->R < (1ll << 40), "shape: too large");
    VBNN_REQUIRE(a->form == VBNN_MOMENTS_STACKED || a->form == VBNN_MOMENTS_ACCUMULATE, "form");
    const bool stacked = a->form == VBNN_MOMENTS_STACKED, d4 = (a->D & 3) == 0;
    MomArgs m = {};
    if (const int bad = F::own(*a, d4, m)) return bad;
    VBNN_REQUIRE(a->ld_y >= F::HALVES * a->D && (!a->target || a->ld_t >= a->D), F::LD_MSG);
    VBNN_REQUIRE((!a->mean && !a->var && !m.nvar) || a->ld_out >= a->D, "ld_out");
    VBNN_REQUIRE(a->target || (!a->row_sq_err && !a->row_log_lik && !a->totals), "row_sq_err, row_log_lik and totals need a target");
    if (stacked) {
        VBNN_REQUIRE(a->D <= 4 * 256 * F::NQ_WIDE, F::CAP_MSG);
    } else {
        VBNN_REQUIRE(a->state, "the ACCUMULATE form keeps its running values in `state`");
        VBNN_REQUIRE(a->draw >= 0 && a->draw < a->S, "draw outside [0, S)");
    }
    m.y = a->y; m.ld_y = a->ld_y; m.t = a->target; m.ld_t = a->ld_t; m.R = a->R; m.D = a->D; m.S = (int)a->S;
    m.draw = stacked ? 0 : a->draw; m.state = stacked ? nullptr : a->state;
    m.mean = a->mean; m.var = a->var; m.ld_out = a->ld_out; m.row_var = a->row_var; m.row_sq_err = a->row_sq_err;
    m.row_log_lik = a->row_log_lik;
    m.y_vec = d4 && (a->ld_y & 3) == 0 && vbnn_al16(a->y);
    m.t_vec = a->target && d4 && (a->ld_t & 3) == 0 && vbnn_al16(a->target);
    m.o_vec = d4 && (a->ld_out & 3) == 0 && vbnn_al16(a->mean) && vbnn_al16(a->var) && vbnn_al16(m.nvar);
    m.s_vec = !stacked && d4 && vbnn_al16(a->state);
    const MomPlan<F::NT> plan(ctx, a->D, a->R, (stacked || a->draw == a->S - 1) && a->totals);
    VBNN_REQUIRE(plan.fits, "reduction scratch");
    m.part = plan.part;
    const dim3 grid(plan.nb), block(256);
    if (stacked) {
        if (plan.wave_rows) hipLaunchKernelGGL((k_moments_stacked<F, 1, MOM_NQ>), grid, block, 0, ctx->stream, m);
        else if (a->D <= 4 * 256 * MOM_NQ) hipLaunchKernelGGL((k_moments_stacked<F, 4, MOM_NQ>), grid, block, 0, ctx->stream, m);
        else hipLaunchKernelGGL((k_moments_stacked<F, 4, F::NQ_WIDE>), grid, block, 0, ctx->stream, m);
    } else {
        if (plan.wave_rows) hipLaunchKernelGGL((k_moments_accumulate<F, 1>), grid, block, 0, ctx->stream, m);
        else hipLaunchKernelGGL((k_moments_accumulate<F, 4>), grid, block, 0, ctx->stream, m);
    }
    plan.finish(ctx->stream, a->totals);
    return vbnn_check_launch(F::WHAT);
}

extern "C" int vbnn_predict_moments(vbnn_ctx* ctx, const vbnn_moments_args* a) {
    VBNN_API_BEGIN
    return mom_predict<MseFamily>(ctx, a);
    VBNN_API_END
}

extern "C" int vbnn_predict_gauss_moments(vbnn_ctx* ctx, const vbnn_gauss_moments_args* a) {
    VBNN_API_BEGIN
    return mom_predict<GaussFamily>(ctx, a);
    VBNN_API_END
}
