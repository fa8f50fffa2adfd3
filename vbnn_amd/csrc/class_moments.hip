// class_moments.hip -- vbnn_predict_class_moments: the class-probability posterior predictive for any class count
// (include/vbnn_hip.h): per draw the log-softmax of the final Linear's f32 logits, per class the online logsumexp over the
// draws, per row the draws' entropies and the target's terms; the finish forms log p, p, the entropies, the top-K classes and
// the five totals. The third member of the moments family (moments.hip): a streaming kernel, no MFMA, LDS only for the waves'
// row partials, compiled WITHOUT floating-point contraction (Makefile): every line below is the fp32 operation it spells.
//
// A row is worked by TR threads: one wave while C <= 256 (four rows per workgroup), the whole workgroup above. Thread i owns
// the quads q = i, i + TR, ... (columns 4 q .. 4 q + 3) on the 16-byte AND on the scalar path, so a row sum's order depends on
// C alone. While C <= VBNN_CLASS_MOMENTS_STACKED_MAX_C a draw's row stays in the registers of its threads (NQ quads each)
// through the max, the sum and the subtraction, in both forms, which run cls_draw / cls_finish and nothing else on a row.
// Above (ACCUMULATE only) k_class_accumulate_wide makes the same three passes over y in memory with the same quad functions.
#include "moments_common.h"
#include <math.h>
#include <limits.h>

constexpr int CLS_NQ = 4;
static_assert(VBNN_CLASS_MOMENTS_STACKED_MAX_C == 4 * 256 * CLS_NQ, "the register tile of a row");
constexpr int CLS_NT = 5;                      // totals

struct ClsArgs {
    const float* y; int64_t ld_y; const int32_t* t; int64_t R, C; int S, draw, K;
    float* state; int64_t ld_state; float* probs; float* log_probs; int64_t ld_out;
    float* entropy; float* expected_entropy; float* mutual_info; int32_t* pred; int32_t* topk_idx; float* topk_prob; double* part;
    int y_vec, o_vec, s_vec;                   // 16-byte access allowed on the whole quads (a row's last, partial quad goes scalar)
};

struct ClsShared {
    float red[5][4];
    float pv[4];
    int pi[4];
    double dred[CLS_NT][4];
};

// ---- the order of the maximum reductions: the larger value, among equal values the lower index. Values are never NaN here
// (a NaN fails `>`), so the order is total and both lanes of an exchange keep the same pair.
__device__ __forceinline__ void cls_better(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
// over the row's threads: the xor butterfly inside a wave, the waves in wave order through LDS. Every thread of the row
// returns the same pair. WPR == 4: block-uniform call (two barriers).
template <int WPR>
__device__ __forceinline__ void cls_row_argmax(float& v, int& i, ClsShared& sh, int wave) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        cls_better(v, i, ov, oi);
    }
    if (WPR == 1) return;
    if ((threadIdx.x & 63) == 0) { sh.pv[wave] = v; sh.pi[wave] = i; }
    __syncthreads();
    v = sh.pv[0]; i = sh.pi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) cls_better(v, i, sh.pv[w], sh.pi[w]);
    __syncthreads();
}

// ---- THE element operations, one quad (columns col .. col + valid - 1): every kernel below calls these and nothing else. They
// are written without a branch per element: all four lanes of a quad are computed (a lane past `valid` holds the loader's 0) and
// a select keeps such a lane out of every sum, maximum and output -- adding the +0 it contributes instead changes no bit of a sum.
__device__ __forceinline__ void cls_max_quad(const float (&y)[4], int valid, int col, float& mx, int& am) {
    if (valid == 0) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool up = j < valid && y[j] > mx;
        mx = up ? y[j] : mx;
        am = up ? col + j : am;
    }
}
__device__ __forceinline__ void cls_exp_quad(const float (&y)[4], int valid, float mx, float& e) {
    if (valid == 0) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float v = expf(y[j] - mx);
        e = e + (j < valid ? v : 0.f);
    }
}
// log1p(u) for u = exp(-|d|) in [0, 1]: with w = 1 + u, log(w) . u / (w - 1) -- w - 1 is exact, and the quotient puts back what
// the rounding of 1 + u took from u (u itself where w = 1) -- a logf, a product and a correctly rounded division, within 3 ulp
// of log1p, where the library's log1pf (any argument, software throughout) costs several times the instructions: it was
// a third of this kernel's vector instructions (4073 against 2740 at the widest tile), and the kernel is bound by them. A NaN passes.
__device__ __forceinline__ float cls_log1p01(float u) {
    const float w = 1.f + u;
    const float r = __fdiv_rn(logf(w) * u, w - 1.f);
    return w == 1.f ? u : r;
}
// o = y - lse; the draw's entropy terms; the class's online logsumexp; the target's -o
__device__ __forceinline__ void cls_update_quad(const float (&y)[4], int valid, int col, float lse, bool first, int t,
                                                float (&L)[4], float& h, float& nll) {
    if (valid == 0) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float o = y[j] - lse;
        const float w = expf(o) * o;
        h = h + (j < valid ? w : 0.f);
        L[j] = first ? o : fmaxf(L[j], o) + cls_log1p01(expf(-fabsf(L[j] - o)));    // a NaN passes through the |L - o| term
        nll = col + j == t ? (first ? -o : nll + (-o)) : nll;                   // (t is inside the row: a valid lane)
    }
}
__device__ __forceinline__ void cls_finish_quad(const float (&L)[4], int valid, int col, float logS, int t,
                                                float (&lp)[4], float (&p)[4], float& ent, float& nlp) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        lp[j] = L[j] - logS;
        p[j] = expf(lp[j]);
        const float w = p[j] * lp[j];
        ent = ent + (j < valid ? w : 0.f);
        nlp = col + j == t ? -lp[j] : nlp;
    }
}
// a top-K round: the first maximum of log p among the classes that come after (pv, pi) in the order of cls_better
__device__ __forceinline__ void cls_topk_quad(const float (&L)[4], int valid, int col, float logS, float pv, int pi, float& bv, int& bi) {
    if (valid == 0) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float v = L[j] - logS;
        const int c = col + j;
        const bool up = j < valid && (v < pv || (v == pv && c > pi)) && v > bv;
        bv = up ? v : bv;
        bi = up ? c : bi;
    }
}

// the thread of the row that keeps the row's three running values: the owner of the target's column (thread 0 without one)
template <int TR>
__device__ __forceinline__ int cls_owner(int t) { return t < 0 ? 0 : (t >> 2) % TR; }

__device__ __forceinline__ int cls_target(const ClsArgs& a, int64_t r) {
    if (!a.t) return -1;
    const int t = a.t[r];
    return t < 0 ? 0 : (t > (int)a.C - 1 ? (int)a.C - 1 : t);
}

// ---- the row values after a draw's passes (every thread; the owner's copy is the one kept)
__device__ __forceinline__ void cls_draw_row(float h, int am, int t, bool first, float& sumH, float& hits) {
    const float Hs = -h;
    sumH = first ? Hs : sumH + Hs;
    const float hit = (t >= 0 && am == t) ? 1.f : 0.f;
    hits = first ? hit : hits + hit;
}

// ---- the row's finish after the element pass: f = { sum p log p, -log p[t], sum H, sum -o[t], hits }, the last four nonzero
// on one thread only (adding zeros is exact), so after the row sum every thread holds them. `scan` runs cls_topk_quad over the
// thread's quads.
template <int WPR, typename Scan>
__device__ __forceinline__ void cls_finish_row(const ClsArgs& a, int64_t r, int t, int tr, float (&f)[5], Scan scan, ClsShared& sh,
                                               int wave, double (&tot)[CLS_NT]) {
    mom_row_sum<WPR, 5>(f, sh.red, wave);
    const float entropy = -f[0];
    const float expected = __fdiv_rn(f[2], (float)a.S);
    if (tr == 0) {
        if (a.entropy) a.entropy[r] = entropy;
        if (a.expected_entropy) a.expected_entropy[r] = expected;
        if (a.mutual_info) a.mutual_info[r] = entropy - expected;
    }
    const int rounds = a.K > 0 ? a.K : ((a.pred || t >= 0) ? 1 : 0);       // launch-uniform but for t, which the row shares
    float pv = INFINITY;
    int pi = -1, pred = 0, in_top = 0;
    for (int k = 0; k < rounds; ++k) {
        float bv = -INFINITY;
        int bi = INT_MAX;
        scan(pv, pi, bv, bi);
        cls_row_argmax<WPR>(bv, bi, sh, wave);
        const bool none = bi == INT_MAX;                   // a NaN row: no class compares
        const int idx = none ? k : bi;
        if (k == 0) pred = idx;
        if (k < a.K) {
            if (tr == 0) {
                if (a.topk_idx) a.topk_idx[r * a.K + k] = idx;
                if (a.topk_prob) a.topk_prob[r * a.K + k] = none ? __builtin_nanf("") : expf(bv);
            }
            if (idx == t) in_top = 1;
        }
        pv = bv; pi = bi;
    }
    if (tr == 0) {
        if (a.pred) a.pred[r] = pred;
        if (t >= 0) {
            tot[0] += (double)f[1]; tot[1] += (pred == t) ? 1.0 : 0.0; tot[2] += (double)f[3]; tot[3] += (double)f[4];
            tot[4] += (double)in_top;
        }
    }
}

// ---- THE per-draw update of a row held in registers: both forms call this and nothing else on a draw
template <int WPR, int NQ>
__device__ __forceinline__ void cls_draw(const float (&y)[NQ][4], const int (&valid)[NQ], const int (&col)[NQ], bool first, int t,
                                         float (&L)[NQ][4], float& sumH, float& nll, float& hits, ClsShared& sh, int wave) {
    float mx = -INFINITY;
    int am = valid[0] > 0 ? col[0] : INT_MAX;              // a thread's first column: the index stays inside the row whatever y holds
#pragma unroll
    for (int k = 0; k < NQ; ++k) cls_max_quad(y[k], valid[k], col[k], mx, am);
    cls_row_argmax<WPR>(mx, am, sh, wave);
    float e[1] = {0.f};
#pragma unroll
    for (int k = 0; k < NQ; ++k) cls_exp_quad(y[k], valid[k], mx, e[0]);
    mom_row_sum<WPR, 1>(e, sh.red, wave);
    const float lse = mx + logf(e[0]);
    float h[1] = {0.f};
#pragma unroll
    for (int k = 0; k < NQ; ++k) cls_update_quad(y[k], valid[k], col[k], lse, first, t, L[k], h[0], nll);
    mom_row_sum<WPR, 1>(h, sh.red, wave);
    cls_draw_row(h[0], am, t, first, sumH, hits);
}

// ---- the finish of a row held in registers
template <int WPR, int NQ>
__device__ __forceinline__ void cls_finish(const ClsArgs& a, int64_t r, int t, int tr, int own, const float (&L)[NQ][4],
                                           const int (&valid)[NQ], const int (&col)[NQ], float sumH, float nll, float hits,
                                           ClsShared& sh, int wave, double (&tot)[CLS_NT]) {
    const float logS = logf((float)a.S);
    float f[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        float lp[4], p[4];
        cls_finish_quad(L[k], valid[k], col[k], logS, t, lp, p, f[0], f[1]);
        const int om = (a.o_vec && valid[k] == 4) ? 2 : 0;
        if (a.probs) mom_store4<false>(a.probs + r * a.ld_out + col[k], p, valid[k], om);
        if (a.log_probs) mom_store4<false>(a.log_probs + r * a.ld_out + col[k], lp, valid[k], om);
    }
    if (tr == own) { f[2] = sumH; f[3] = nll; f[4] = hits; }
    auto scan = [&](float pv, int pi, float& bv, int& bi) {
#pragma unroll
        for (int k = 0; k < NQ; ++k) cls_topk_quad(L[k], valid[k], col[k], logS, pv, pi, bv, bi);
    };
    cls_finish_row<WPR>(a, r, t, tr, f, scan, sh, wave, tot);
}

template <int WPR, int NQ>
__global__ __launch_bounds__(256) void k_class_stacked(const ClsArgs a) {
    constexpr int TR = 64 * WPR, RPB = 4 / WPR;
    __shared__ ClsShared sh;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tr = WPR == 1 ? lane : (int)threadIdx.x;
    double tot[CLS_NT] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int valid[NQ], col[NQ];
    mom_tile<NQ, TR>(tr, a.C, valid, col);
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < a.R; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t r = r0 + (WPR == 1 ? wave : 0);
        if (r >= a.R) continue;                            // WPR == 1 only: a whole wave, and that path has no barrier in the loop
        const int t = cls_target(a, r);
        float L[NQ][4], yc[NQ][4], yn[NQ][4];
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j) L[k][j] = yn[k][j] = 0.f;
            mom_load4<true>(a.y + r * a.ld_y + col[k], yc[k], valid[k], (a.y_vec && valid[k] == 4) ? 2 : 0);
        }
        float sumH = 0.f, nll = 0.f, hits = 0.f;
        for (int s = 0; s < a.S; ++s) {
            if (s + 1 < a.S) {
                const float* yr = a.y + ((int64_t)(s + 1) * a.R + r) * a.ld_y;
#pragma unroll
                for (int k = 0; k < NQ; ++k) mom_load4<true>(yr + col[k], yn[k], valid[k], (a.y_vec && valid[k] == 4) ? 2 : 0);
            }
            cls_draw<WPR, NQ>(yc, valid, col, s == 0, t, L, sumH, nll, hits, sh, wave);
#pragma unroll
            for (int k = 0; k < NQ; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) yc[k][j] = yn[k][j];
        }
        cls_finish<WPR, NQ>(a, r, t, tr, cls_owner<TR>(t), L, valid, col, sumH, nll, hits, sh, wave, tot);
    }
    mom_store_partials<WPR, CLS_NT>(a.part, tot, sh.dred, wave, tr);
}

// one draw of a row that fits the register tile: y and the row's L come in once, L goes out once
template <int WPR, int NQ>
__global__ __launch_bounds__(256) void k_class_accumulate(const ClsArgs a) {
    constexpr int TR = 64 * WPR, RPB = 4 / WPR;
    __shared__ ClsShared sh;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tr = WPR == 1 ? lane : (int)threadIdx.x;
    const bool first = a.draw == 0, fin = a.draw == a.S - 1;
    double tot[CLS_NT] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int valid[NQ], col[NQ];
    mom_tile<NQ, TR>(tr, a.C, valid, col);
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < a.R; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t r = r0 + (WPR == 1 ? wave : 0);
        if (r >= a.R) continue;                            // WPR == 1 only (see k_class_stacked)
        const int t = cls_target(a, r);
        const int own = cls_owner<TR>(t);
        float* st = a.state + r * a.ld_state;              // { L[C], sum H, sum -o[t], hits }
        float L[NQ][4], y[NQ][4];
#pragma unroll
        for (int k = 0; k < NQ; ++k) {                     // every load of the row in flight before the first use
#pragma unroll
            for (int j = 0; j < 4; ++j) L[k][j] = 0.f;
            if (!first) mom_load4<true>(st + col[k], L[k], valid[k], (a.s_vec && valid[k] == 4) ? 2 : 0);
            mom_load4<true>(a.y + r * a.ld_y + col[k], y[k], valid[k], (a.y_vec && valid[k] == 4) ? 2 : 0);
        }
        float sumH = 0.f, nll = 0.f, hits = 0.f;
        if (tr == own && !first) { sumH = st[a.C]; nll = st[a.C + 1]; hits = st[a.C + 2]; }
        cls_draw<WPR, NQ>(y, valid, col, first, t, L, sumH, nll, hits, sh, wave);
#pragma unroll
        for (int k = 0; k < NQ; ++k) mom_store4<true>(st + col[k], L[k], valid[k], (a.s_vec && valid[k] == 4) ? 2 : 0);
        if (tr == own) { st[a.C] = sumH; st[a.C + 1] = nll; st[a.C + 2] = hits; }
        if (fin) cls_finish<WPR, NQ>(a, r, t, tr, own, L, valid, col, sumH, nll, hits, sh, wave, tot);
    }
    if (fin) mom_store_partials<WPR, CLS_NT>(a.part, tot, sh.dred, wave, tr);
}

// one draw of a row wider than the register tile: the three passes of cls_draw over y in memory (the second and third read
// come from the cache), the finish's top-K rounds over the state this thread has just written
__global__ __launch_bounds__(256) void k_class_accumulate_wide(const ClsArgs a) {
    constexpr int TR = 256;
    __shared__ ClsShared sh;
    const int wave = threadIdx.x >> 6, tr = (int)threadIdx.x;
    const bool first = a.draw == 0, fin = a.draw == a.S - 1;
    const int nq = (int)((a.C + 3) >> 2), C = (int)a.C;
    const float logS = logf((float)a.S);
    double tot[CLS_NT] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t r = blockIdx.x; r < a.R; r += gridDim.x) {
        const int t = cls_target(a, r);
        const int own = cls_owner<TR>(t);
        const float* yr = a.y + r * a.ld_y;
        float* st = a.state + r * a.ld_state;
        float mx = -INFINITY;
        int am = tr < nq ? 4 * tr : INT_MAX;               // (as cls_draw)
        for (int q = tr; q < nq; q += TR) {
            const int valid = min(4, C - 4 * q);
            float y[4];
            mom_load4<false>(yr + 4 * q, y, valid, (a.y_vec && valid == 4) ? 2 : 0);
            cls_max_quad(y, valid, 4 * q, mx, am);
        }
        cls_row_argmax<4>(mx, am, sh, wave);
        float e[1] = {0.f};
        for (int q = tr; q < nq; q += TR) {
            const int valid = min(4, C - 4 * q);
            float y[4];
            mom_load4<false>(yr + 4 * q, y, valid, (a.y_vec && valid == 4) ? 2 : 0);
            cls_exp_quad(y, valid, mx, e[0]);
        }
        mom_row_sum<4, 1>(e, sh.red, wave);
        const float lse = mx + logf(e[0]);
        float h[1] = {0.f};
        float f[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        float sumH = 0.f, nll = 0.f, hits = 0.f;
        if (tr == own && !first) { sumH = st[C]; nll = st[C + 1]; hits = st[C + 2]; }
        for (int q = tr; q < nq; q += TR) {
            const int valid = min(4, C - 4 * q);
            const int sm = (a.s_vec && valid == 4) ? 2 : 0;
            float y[4], L[4] = {0.f, 0.f, 0.f, 0.f};
            if (!first) mom_load4<true>(st + 4 * q, L, valid, sm);
            mom_load4<true>(yr + 4 * q, y, valid, (a.y_vec && valid == 4) ? 2 : 0);
            cls_update_quad(y, valid, 4 * q, lse, first, t, L, h[0], nll);
            if (fin) mom_store4<false>(st + 4 * q, L, valid, sm); else mom_store4<true>(st + 4 * q, L, valid, sm);   // (the finish reads it again)
            if (fin) {
                float lp[4], p[4];
                cls_finish_quad(L, valid, 4 * q, logS, t, lp, p, f[0], f[1]);
                const int om = (a.o_vec && valid == 4) ? 2 : 0;
                if (a.probs) mom_store4<false>(a.probs + r * a.ld_out + 4 * q, p, valid, om);
                if (a.log_probs) mom_store4<false>(a.log_probs + r * a.ld_out + 4 * q, lp, valid, om);
            }
        }
        mom_row_sum<4, 1>(h, sh.red, wave);
        cls_draw_row(h[0], am, t, first, sumH, hits);
        if (tr == own) { st[C] = sumH; st[C + 1] = nll; st[C + 2] = hits; }
        if (fin) {
            if (tr == own) { f[2] = sumH; f[3] = nll; f[4] = hits; }
            auto scan = [&](float pv, int pi, float& bv, int& bi) {
                for (int q = tr; q < nq; q += TR) {        // the quads this thread stored above
                    const int valid = min(4, C - 4 * q);
                    float L[4];
                    mom_load4<false>(st + 4 * q, L, valid, (a.s_vec && valid == 4) ? 2 : 0);
                    cls_topk_quad(L, valid, 4 * q, logS, pv, pi, bv, bi);
                }
            };
            cls_finish_row<4>(a, r, t, tr, f, scan, sh, wave, tot);
        }
    }
    if (fin) mom_store_partials<4, CLS_NT>(a.part, tot, sh.dred, wave, tr);
}

template <int WPR, int NQ>
static void cls_launch(bool stacked, int nb, hipStream_t stream, const ClsArgs& m) {
    if (stacked) hipLaunchKernelGGL((k_class_stacked<WPR, NQ>), dim3(nb), dim3(256), 0, stream, m);
    else hipLaunchKernelGGL((k_class_accumulate<WPR, NQ>), dim3(nb), dim3(256), 0, stream, m);
}

extern "C" int vbnn_predict_class_moments(vbnn_ctx* ctx, const vbnn_class_moments_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a && a->y, "null argument (a, y)");
    VBNN_REQUIRE(a->R >= 1 && a->C >= 1 && a->S >= 1, "shape: R, C and S are at least 1");
    VBNN_REQUIRE(a->S < (1ll << 24) && a->C < (1ll << 28) && a->R < (1ll << 40), "shape: too large");
    VBNN_REQUIRE(a->form == VBNN_MOMENTS_STACKED || a->form == VBNN_MOMENTS_ACCUMULATE, "form");
    VBNN_REQUIRE(a->ld_y >= a->C, "ld_y");
    VBNN_REQUIRE(a->K >= 0 && a->K <= VBNN_CLASS_MOMENTS_MAX_K && a->K <= a->C, "K outside [0, min(VBNN_CLASS_MOMENTS_MAX_K, C)]");
    VBNN_REQUIRE((!a->probs && !a->log_probs) || a->ld_out >= a->C, "ld_out");
    VBNN_REQUIRE(a->target || !a->totals, "totals need a target");
    VBNN_REQUIRE(a->K > 0 || (!a->topk_idx && !a->topk_prob), "topk_idx and topk_prob need K >= 1");
    const bool stacked = a->form == VBNN_MOMENTS_STACKED;
    if (stacked) {
        VBNN_REQUIRE(a->C <= VBNN_CLASS_MOMENTS_STACKED_MAX_C, "the STACKED form takes C <= VBNN_CLASS_MOMENTS_STACKED_MAX_C: use ACCUMULATE");
    } else {
        VBNN_REQUIRE(a->state, "the ACCUMULATE form keeps its running values in `state`");
        VBNN_REQUIRE(a->ld_state >= a->C + 3, "ld_state: a row of the state holds C + 3 floats");
        VBNN_REQUIRE(a->draw >= 0 && a->draw < a->S, "draw outside [0, S)");
    }
    ClsArgs m;
    m.y = a->y; m.ld_y = a->ld_y; m.t = a->target; m.R = a->R; m.C = a->C; m.S = (int)a->S; m.draw = stacked ? 0 : a->draw;
    m.K = (int)a->K; m.state = stacked ? nullptr : a->state; m.ld_state = stacked ? 0 : a->ld_state;
    m.probs = a->probs; m.log_probs = a->log_probs; m.ld_out = a->ld_out; m.entropy = a->entropy;
    m.expected_entropy = a->expected_entropy; m.mutual_info = a->mutual_info; m.pred = a->pred; m.topk_idx = a->topk_idx;
    m.topk_prob = a->topk_prob;
    m.y_vec = (a->ld_y & 3) == 0 && vbnn_al16(a->y);
    m.o_vec = (a->ld_out & 3) == 0 && vbnn_al16(a->probs) && vbnn_al16(a->log_probs);
    m.s_vec = !stacked && (a->ld_state & 3) == 0 && vbnn_al16(a->state);
    const MomPlan<CLS_NT> plan(ctx, a->C, a->R, (stacked || a->draw == a->S - 1) && a->totals);
    VBNN_REQUIRE(plan.fits, "reduction scratch");
    m.part = plan.part;
    // the register tile follows C; thread i owns quads i, i + T, ... under every tile, so the bits do not depend on it
    if (plan.wave_rows) cls_launch<1, 1>(stacked, plan.nb, ctx->stream, m);
    else if (a->C <= 4 * 256 * 1) cls_launch<4, 1>(stacked, plan.nb, ctx->stream, m);
    else if (a->C <= 4 * 256 * 2) cls_launch<4, 2>(stacked, plan.nb, ctx->stream, m);
    else if (a->C <= 4 * 256 * CLS_NQ) cls_launch<4, CLS_NQ>(stacked, plan.nb, ctx->stream, m);
    else hipLaunchKernelGGL(k_class_accumulate_wide, dim3(plan.nb), dim3(256), 0, ctx->stream, m);
    plan.finish(ctx->stream, a->totals);
    return vbnn_check_launch("k_class_moments");
    VBNN_API_END
}
