// label_moments.hip -- vbnn_predict_label_moments: the posterior predictive of the Bernoulli likelihood head
// (include/vbnn_hip.h): D independent sigmoid outputs per row. Per draw and element the two probabilities p = sigmoid(z) and
// q = 1 - p (each formed on its own, never as a difference), their logs and the draw's entropy; per element the running sums
// P, Q, Hs over the draws; per row, with a target, the draw's log-likelihood a_s of the whole label vector, its running sum
// and the online logsumexp over the draws. The finish forms the averaged probabilities, the per-label entropy and mutual
// information (BALD per label), the row values and the five totals. The sixth member of the moments family (moments.hip): a
// streaming kernel, no MFMA, LDS only for the waves' row partials, compiled WITHOUT floating-point contraction (Makefile):
// every line below is the fp32 operation it spells.
//
// A row is worked by TR threads: one wave while D <= 256 (four rows per workgroup), the whole workgroup above. Thread i owns
// the quads q = i, i + TR, ... (columns 4 q .. 4 q + 3) on the 16-byte AND on the scalar path, so a row sum's order depends on
// D alone. STACKED keeps the three state planes and the target of a thread's quads in registers across the draws (NQ quads:
// D <= 4 . 256 . NQ) and loads draw s + 1 while draw s is reduced; ACCUMULATE streams the state through LAB_NQ quads per thread
// at a time. One expf, one logf and two divisions per element and draw (class_moments.hip: three expf and a log1p).
#include "moments_common.h"
#include <math.h>

constexpr int LAB_NQ = 4;
static_assert(VBNN_LABEL_MOMENTS_STACKED_MAX_D == 4 * 256 * LAB_NQ, "the STACKED form's widest register tile");
constexpr int LAB_NT = 5;                      // totals
constexpr int LAB_SUMS = 4;                    // row sums of the finish: entropy, mutual information, marginal log-likelihood, hits
constexpr float LAB_CLAMP = 80.f;              // |z| is clamped here: every probability is at least e^-80, a normal fp32

struct LabArgs {
    const float* y; int64_t ld_y; const float* t; int64_t ld_t; int64_t R, D; int S, draw;
    float* state; float* probs; float* entropy; float* mutual_info; int64_t ld_out;
    float* row_entropy; float* row_mutual_info; float* row_log_lik; float* row_marg_log_lik; int32_t* row_hits; double* part;
    int y_vec, t_vec, o_vec, s_vec;            // 16-byte access allowed (the state's rows alternate 16 / 8-byte alignment)
};

// log1p(u) for u = expf(-|z|) in [0, 1], w = 1 + u: the family's form (class_moments.hip: cls_log1p01). A NaN passes.
__device__ __forceinline__ float lab_log1p01(float u, float w) {
    const float r = __fdiv_rn(logf(w) * u, w - 1.f);
    return w == 1.f ? u : r;
}

// ---- THE per-draw update, one quad: both forms call this and nothing else on a draw's elements. Written without a branch per
// element (class_moments.hip): all four lanes of a quad are computed -- a lane past `valid` holds the loader's 0, its state is
// never stored -- and a select keeps such a lane out of every sum; adding the +0 it contributes instead changes no bit.
__device__ __forceinline__ void lab_draw_quad(const float (&z)[4], const float (&t)[4], bool has_t, int valid, bool first,
                                              float (&P)[4], float (&Q)[4], float (&Hs)[4], float& a) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float zc = z[j] != z[j] ? z[j] : fminf(fmaxf(z[j], -LAB_CLAMP), LAB_CLAMP);   // fmaxf / fminf drop a NaN: keep it
        const float u = expf(-fabsf(zc));
        const float w = 1.f + u;
        const float l1p = lab_log1p01(u, w);
        const float big = __fdiv_rn(1.f, w), small = __fdiv_rn(u, w);
        const bool pos = zc >= 0.f;
        const float p = pos ? big : small, q = pos ? small : big;
        const float lp = fminf(zc, 0.f) - l1p, ln = fminf(-zc, 0.f) - l1p;
        const float h = -(p * lp + q * ln);
        P[j] = first ? p : P[j] + p;
        Q[j] = first ? q : Q[j] + q;
        Hs[j] = first ? h : Hs[j] + h;
        const float term = t[j] * lp + (1.f - t[j]) * ln;
        a = a + ((has_t && j < valid) ? term : 0.f);
    }
}
// the finish, one quad: f = { sum entropy, sum mutual_info, sum (t log_p + (1 - t) log_q), hits }. It runs once a row and keeps
// its branch per element (written without, one instance of the ACCUMULATE kernel was left a 68-byte private segment).
__device__ __forceinline__ void lab_finish_quad(const float (&P)[4], const float (&Q)[4], const float (&Hs)[4], const float (&t)[4],
                                                bool has_t, int valid, int S, float (&pm)[4], float (&ent)[4], float (&mi)[4],
                                                float (&f)[LAB_SUMS]) {
    const float Sf = (float)S;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        pm[j] = ent[j] = mi[j] = 0.f;
        if (j < valid) {
            pm[j] = __fdiv_rn(P[j], Sf);
            const float qm = __fdiv_rn(Q[j], Sf);
            const float log_p = logf(pm[j]), log_q = logf(qm);
            ent[j] = -(pm[j] * log_p + qm * log_q);
            const float expected = __fdiv_rn(Hs[j], Sf);
            mi[j] = S == 1 ? 0.f : ent[j] - expected;      // one draw has no spread: +0 by definition
            f[0] = f[0] + ent[j];
            f[1] = f[1] + mi[j];
            if (has_t) {
                f[2] = f[2] + (t[j] * log_p + (1.f - t[j]) * log_q);
                const bool hit = P[j] == P[j] && (P[j] > Q[j]) == (t[j] > 0.5f);   // a tie predicts 0; a NaN is a miss
                f[3] = f[3] + (hit ? 1.f : 0.f);
            }
        }
    }
}
// on a draw's row value (one thread of the row): the running sum of -a_s and the online logsumexp of the a_s
__device__ __forceinline__ void lab_draw_row(float a, bool first, float& nsum, float& L) {
    nsum = first ? -a : nsum + (-a);
    L = first ? a : fmaxf(L, a) + log1pf(expf(-fabsf(L - a)));           // a NaN passes through the |L - a| term
}
// the row's finish (one thread of the row): the row outputs and the row's terms of the five totals
__device__ __forceinline__ void lab_finish_row(const LabArgs& a, int64_t r, const float (&f)[LAB_SUMS], float nsum, float L,
                                               double (&tot)[LAB_NT]) {
    if (a.row_entropy) a.row_entropy[r] = f[0];
    if (a.row_mutual_info) a.row_mutual_info[r] = f[1];
    if (!a.t) return;
    const float ll = L - logf((float)a.S);
    if (a.row_log_lik) a.row_log_lik[r] = ll;
    if (a.row_marg_log_lik) a.row_marg_log_lik[r] = f[2];
    if (a.row_hits) a.row_hits[r] = (int32_t)f[3];
    tot[0] += (double)ll; tot[1] += (double)f[2]; tot[2] += (double)nsum; tot[3] += (double)f[3];
    tot[4] += f[3] == (float)a.D ? 1.0 : 0.0;
}
__device__ __forceinline__ void lab_store_quad(const LabArgs& a, int64_t r, int64_t col, int valid, int om, const float (&pm)[4],
                                               const float (&ent)[4], const float (&mi)[4]) {
    if (a.probs) mom_store4<false>(a.probs + r * a.ld_out + col, pm, valid, om);
    if (a.entropy) mom_store4<false>(a.entropy + r * a.ld_out + col, ent, valid, om);
    if (a.mutual_info) mom_store4<false>(a.mutual_info + r * a.ld_out + col, mi, valid, om);
}

template <int WPR, int TILE>
__global__ __launch_bounds__(256) void k_label_stacked(const LabArgs a) {
    constexpr int TR = 64 * WPR, RPB = 4 / WPR, NQ = WPR == 1 ? 1 : TILE;
    __shared__ float red[LAB_SUMS][4];
    __shared__ double dred[LAB_NT][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tr = WPR == 1 ? lane : (int)threadIdx.x;
    const bool has_t = a.t != nullptr;
    const int ym = a.y_vec ? 2 : 0, tm = a.t_vec ? 2 : 0, om = a.o_vec ? 2 : 0;
    double tot[LAB_NT] = {};
    int valid[NQ];
    int64_t col[NQ];
    mom_tile<NQ, TR>((int64_t)tr, a.D, valid, col);
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < a.R; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t r = r0 + (WPR == 1 ? wave : 0);
        if (r >= a.R) continue;                            // WPR == 1 only: a whole wave, and that path has no barrier in the loop
        float P[NQ][4], Q[NQ][4], Hs[NQ][4], t[NQ][4], yc[NQ][4], yn[NQ][4];
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j) t[k][j] = P[k][j] = Q[k][j] = Hs[k][j] = yn[k][j] = 0.f;
            if (has_t) mom_load4<false>(a.t + r * a.ld_t + col[k], t[k], valid[k], tm);
            mom_load4<true>(a.y + r * a.ld_y + col[k], yc[k], valid[k], ym);
        }
        float nsum = 0.f, L = 0.f;
        for (int s = 0; s < a.S; ++s) {
            if (s + 1 < a.S) {
                const float* yr = a.y + ((int64_t)(s + 1) * a.R + r) * a.ld_y;
#pragma unroll
                for (int k = 0; k < NQ; ++k) mom_load4<true>(yr + col[k], yn[k], valid[k], ym);
            }
            float e[1] = {0.f};
#pragma unroll
            for (int k = 0; k < NQ; ++k) lab_draw_quad(yc[k], t[k], has_t, valid[k], s == 0, P[k], Q[k], Hs[k], e[0]);
            if (has_t) {
                mom_row_sum<WPR, 1>(e, red, wave);
                if (tr == 0) lab_draw_row(e[0], s == 0, nsum, L);
            }
#pragma unroll
            for (int k = 0; k < NQ; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) yc[k][j] = yn[k][j];
        }
        float f[LAB_SUMS] = {};
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            float pm[4], ent[4], mi[4];
            lab_finish_quad(P[k], Q[k], Hs[k], t[k], has_t, valid[k], a.S, pm, ent, mi, f);
            lab_store_quad(a, r, col[k], valid[k], om, pm, ent, mi);
        }
        mom_row_sum<WPR, LAB_SUMS>(f, red, wave);
        if (tr == 0) lab_finish_row(a, r, f, nsum, L, tot);
    }
    mom_store_partials<WPR, LAB_NT>(a.part, tot, dred, wave, tr);
}

template <int WPR>
__global__ __launch_bounds__(256) void k_label_accumulate(const LabArgs a) {
    constexpr int TR = 64 * WPR, RPB = 4 / WPR, NQ = WPR == 1 ? 1 : LAB_NQ;
    __shared__ float red[LAB_SUMS][4];
    __shared__ double dred[LAB_NT][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tr = WPR == 1 ? lane : (int)threadIdx.x;
    const int64_t nq = (a.D + 3) >> 2, W = 3 * a.D + 2;
    const bool has_t = a.t != nullptr, first = a.draw == 0, fin = a.draw == a.S - 1;
    const int ym = a.y_vec ? 2 : 0, tm = a.t_vec ? 2 : 0, om = a.o_vec ? 2 : 0;
    double tot[LAB_NT] = {};
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < a.R; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t r = r0 + (WPR == 1 ? wave : 0);
        if (r >= a.R) continue;                            // WPR == 1 only (see k_label_stacked)
        float* sr = a.state + r * W;                       // { P[D], Q[D], Hs[D], sum -a_s, L }: rows alternate 16 / 8-byte alignment
        const int sm = !a.s_vec ? 0 : (((uintptr_t)sr & 15u) == 0 ? 2 : 1);
        float e[1] = {0.f};
        float f[LAB_SUMS] = {};
        for (int64_t qb = 0; qb < nq; qb += (int64_t)NQ * TR) {
            float st[NQ][3][4], t[NQ][4], y[NQ][4];
            int valid[NQ];
            int64_t col[NQ];
            mom_tile<NQ, TR>(qb + tr, a.D, valid, col);
#pragma unroll
            for (int k = 0; k < NQ; ++k) {                 // every load of the chunk in flight before the first use
#pragma unroll
                for (int j = 0; j < 4; ++j) t[k][j] = st[k][0][j] = st[k][1][j] = st[k][2][j] = 0.f;
                if (!first)
#pragma unroll
                    for (int p = 0; p < 3; ++p) mom_load4<true>(sr + p * a.D + col[k], st[k][p], valid[k], sm);
                mom_load4<true>(a.y + r * a.ld_y + col[k], y[k], valid[k], ym);
                if (has_t) mom_load4<false>(a.t + r * a.ld_t + col[k], t[k], valid[k], tm);
            }
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                lab_draw_quad(y[k], t[k], has_t, valid[k], first, st[k][0], st[k][1], st[k][2], e[0]);
#pragma unroll
                for (int p = 0; p < 3; ++p) mom_store4<true>(sr + p * a.D + col[k], st[k][p], valid[k], sm);
                if (fin) {
                    float pm[4], ent[4], mi[4];
                    lab_finish_quad(st[k][0], st[k][1], st[k][2], t[k], has_t, valid[k], a.S, pm, ent, mi, f);
                    lab_store_quad(a, r, col[k], valid[k], om, pm, ent, mi);
                }
            }
        }
        if (has_t) mom_row_sum<WPR, 1>(e, red, wave);
        float nsum = 0.f, L = 0.f;
        if (tr == 0) {                                     // the row's two running values: read, updated and written by one thread
            if (!first) { nsum = sr[3 * a.D]; L = sr[3 * a.D + 1]; }
            if (has_t) lab_draw_row(e[0], first, nsum, L);
            sr[3 * a.D] = nsum; sr[3 * a.D + 1] = L;
        }
        if (fin) {
            mom_row_sum<WPR, LAB_SUMS>(f, red, wave);
            if (tr == 0) lab_finish_row(a, r, f, nsum, L, tot);
        }
    }
    if (fin) mom_store_partials<WPR, LAB_NT>(a.part, tot, dred, wave, tr);
}

extern "C" int vbnn_predict_label_moments(vbnn_ctx* ctx, const vbnn_label_moments_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a && a->y, "null argument (a, y)");
    VBNN_REQUIRE(a->R >= 1 && a->D >= 1 && a->S >= 1, "shape: R, D and S are at least 1");
    VBNN_REQUIRE(a->S < (1ll << 24) && a->D < (1ll << 24) && a->R < (1ll << 40), "shape: too large");   // (hits are counted in fp32)
    VBNN_REQUIRE(a->form == VBNN_MOMENTS_STACKED || a->form == VBNN_MOMENTS_ACCUMULATE, "form");
    VBNN_REQUIRE(a->ld_y >= a->D && (!a->target || a->ld_t >= a->D), "leading dimensions");
    VBNN_REQUIRE((!a->probs && !a->entropy && !a->mutual_info) || a->ld_out >= a->D, "ld_out");
    VBNN_REQUIRE(a->target || (!a->row_log_lik && !a->row_marg_log_lik && !a->row_hits && !a->totals),
                 "row_log_lik, row_marg_log_lik, row_hits and totals need a target");
    const bool stacked = a->form == VBNN_MOMENTS_STACKED, d4 = (a->D & 3) == 0;
    if (stacked) {
        VBNN_REQUIRE(a->D <= VBNN_LABEL_MOMENTS_STACKED_MAX_D, "the STACKED form takes D <= VBNN_LABEL_MOMENTS_STACKED_MAX_D: use ACCUMULATE");
    } else {
        VBNN_REQUIRE(a->state, "the ACCUMULATE form keeps its running values in `state`");
        VBNN_REQUIRE(a->draw >= 0 && a->draw < a->S, "draw outside [0, S)");
    }
    LabArgs m = {};
    m.y = a->y; m.ld_y = a->ld_y; m.t = a->target; m.ld_t = a->ld_t; m.R = a->R; m.D = a->D; m.S = (int)a->S;
    m.draw = stacked ? 0 : a->draw; m.state = stacked ? nullptr : a->state;
    m.probs = a->probs; m.entropy = a->entropy; m.mutual_info = a->mutual_info; m.ld_out = a->ld_out;
    m.row_entropy = a->row_entropy; m.row_mutual_info = a->row_mutual_info; m.row_log_lik = a->row_log_lik;
    m.row_marg_log_lik = a->row_marg_log_lik; m.row_hits = a->row_hits;
    m.y_vec = d4 && (a->ld_y & 3) == 0 && vbnn_al16(a->y);
    m.t_vec = a->target && d4 && (a->ld_t & 3) == 0 && vbnn_al16(a->target);
    m.o_vec = d4 && (a->ld_out & 3) == 0 && vbnn_al16(a->probs) && vbnn_al16(a->entropy) && vbnn_al16(a->mutual_info);
    m.s_vec = !stacked && d4 && vbnn_al16(a->state);
    const MomPlan<LAB_NT> plan(ctx, a->D, a->R, (stacked || a->draw == a->S - 1) && a->totals);
    VBNN_REQUIRE(plan.fits, "reduction scratch");
    m.part = plan.part;
    const dim3 grid(plan.nb), block(256);
    // the register tile follows D; thread i owns quads i, i + T, ... under every tile, so the bits do not depend on it
    if (stacked) {
        if (plan.wave_rows) hipLaunchKernelGGL((k_label_stacked<1, 1>), grid, block, 0, ctx->stream, m);
        else if (a->D <= 4 * 256 * 1) hipLaunchKernelGGL((k_label_stacked<4, 1>), grid, block, 0, ctx->stream, m);
        else if (a->D <= 4 * 256 * 2) hipLaunchKernelGGL((k_label_stacked<4, 2>), grid, block, 0, ctx->stream, m);
        else hipLaunchKernelGGL((k_label_stacked<4, LAB_NQ>), grid, block, 0, ctx->stream, m);
    } else {
        if (plan.wave_rows) hipLaunchKernelGGL((k_label_accumulate<1>), grid, block, 0, ctx->stream, m);
        else hipLaunchKernelGGL((k_label_accumulate<4>), grid, block, 0, ctx->stream, m);
    }
    plan.finish(ctx->stream, a->totals);
    return vbnn_check_launch("k_label_moments");
    VBNN_API_END
}
