// conformal.hip -- vbnn_conformal (include/vbnn_hip.h): split conformal prediction sets for a class predictive. Per row the
// conformity score of the target (LAC: 1 - p[t]; APS: the probability mass ranked at or above t) and, for up to Q thresholds held
// ON THE DEVICE, the prediction set { j : s(r, j) <= qhat[q] } with its size, its last admitted class, its member bits, whether it
// covers the target, and the integer sums a test set's coverage and set sizes are computed from. A member of the moments family:
// streaming, no MFMA, compiled WITHOUT floating-point contraction (Makefile); everything that accumulates across rows is an
// integer, so nothing depends on the grid, the arrival order, the chunking or the number of calls.
//
// THE METHOD. A class ranks by the pair (order word of its probability, descending; index, ascending). Along that ranking the
// score is non-decreasing in fp32 -- LAC: 1 - p rounds monotonically; APS: the masked row sum adds non-negative terms in a tree
// that depends on C alone, every fp32 add is monotone in either argument, so a larger mask never gives a smaller sum -- hence
// the set is a PREFIX of the ranking and one boundary names it: (hs, n) admits class c iff sw[c] > hs, or sw[c] == hs and c < n
// (sw: the order word with its top bit flipped, compared as a signed integer; for a probability >= +0 the float's own bits).
// LAC's boundary is the comparison itself. APS finds it by bisection with one masked row sum per step: 32 steps on the order
// word (the largest word h with sum{w >= h} > qhat), then floor(log2 C) + 1 steps on the index among the classes that share the
// word below the cut. No sort, no C^2 work; all the thresholds of a batch share each reduction (their sums ride the same
// butterfly, which is what a step waits for).
//
// THE MAPPING is k_calibration's (calibration.hip): a WAVE owns its rows from the loads to the adds, no barrier and no LDS
// round trip inside a row. The family's row-sum rule names T = 64 threads for C <= 256 and 256 above; the wave plays all of
// them (VW = 4: lane l is threads l, l + 64, l + 128, l + 192 with a partial each, four butterflies side by side, added in
// wave order). For C <= 128 the row's quads fit a group of G = 2^k < 64 lanes and the wave works 64 / G rows at once: the
// butterfly levels at and above G would add the +0 of a lane without a quad (a partial starts at +0 and adds terms >= +0 or
// -0, so it never is -0), leaving them out changes no bit. A row of C <= 4096 stays in registers as its NK VW quads per lane
// (the order words; the value is the word's own bits); a wider row is read again from memory on every step -- the same bits.
#include "device_prims.h"
#include <math.h>
#include <algorithm>

// threads of a workgroup, each wave with rows of its own: 16 waves where a lane holds one quad, 8 where it holds up to 16 (the
// budget of 256 registers keeps the row, QB x VW partials and the loads' addresses out of private memory)
constexpr int conf_threads(int VW) { return VW == 1 ? 1024 : 512; }
constexpr int CONF_MAXQ = VBNN_CONFORMAL_MAX_Q;
constexpr int CONF_WORDS = 8 * CONF_MAXQ + 2;

typedef unsigned long long u64;

struct ConfArgs {
    const float* probs; int64_t ld; const int32_t* target; int64_t R; int C, kind, Q; const float* qhat;
    float* score; int32_t* size; int32_t* cut_index; float* cut_prob; int32_t* covered; uint32_t* member; u64* acc;
    int vec;                                   // 16-byte loads on the row's whole quads (its last, partial quad goes element by element)
    int nw;                                    // member words of a row
    int ibits;                                 // floor(log2 C) + 1: the steps of the bisection on the index
};

// the signed order word: vbnn_order_word with its top bit flipped, so that a signed comparison orders as the contract's unsigned
// one. A float with a clear sign keeps its bits; -0 becomes -1, right below +0. Every NaN is taken as the positive quiet NaN (a
// NaN only ever makes its row a skipped one), which leaves INT_MIN -- the word of the NaN 0xffffffff alone -- free to mean
// "no class here": as a float it is -0 and adds nothing, it is never above a boundary, and 1 - (its value, a NaN) <= q is false.
constexpr int CONF_NONE = (int)0x80000000;
__device__ __forceinline__ int conf_sw(float x) {
    const int b = __float_as_int(x);           // (order word ^ 0x80000000: sign clear -> b, sign set -> b ^ 0x7fffffff)
    return vbnn_bits_nan((uint32_t)b) ? 0x7fc00000 : b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float conf_value(int sw) { return __uint_as_float(vbnn_unorder_word((uint32_t)sw ^ 0x80000000u)); }

// the quad at columns cb + li4 .. + 3 of a row as signed order words (cb: the same in every lane; lp: the row's column li4); a
// column that is not there (or a lane without a row) holds CONF_NONE. The loads sit under their conditions, not behind clamped
// addresses: every address is then the lane's one pointer and a constant, and a row of 64 classes a lane needs no registers
// for them.
__device__ __forceinline__ void conf_load_quad(const ConfArgs& a, const float* lp, int cb, int li4, bool act, int (&sw)[4]) {
    const int cbody = a.vec ? (a.C & ~3) : 0;  // the columns below it go as whole quads
#pragma unroll
    for (int j = 0; j < 4; ++j) sw[j] = CONF_NONE;
    if (!act) return;
    if (li4 < cbody - cb) {
        const f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(lp + cb));
#pragma unroll
        for (int j = 0; j < 4; ++j) sw[j] = conf_sw(t[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (li4 < a.C - (cb + j)) sw[j] = conf_sw(lp[cb + j]);
    }
}

// a lane's part of a row. NK >= 1: NK VW quads in registers, loaded once; NK == 0: every walk reads the row again.
// each(f) calls f(w, cb, sw) for the lane's quads -- w: the wave of the rule whose thread owns the quad; cb + 4 li: its first
// column, cb the same in every lane -- wave-uniformly, and for one w in ascending quad order (the order of that thread's partial).
template <int VW, int NK>
struct ConfRow {
    int sw[NK][VW][4];
    int li;
    __device__ __forceinline__ void load(const ConfArgs& a, const float* row, int li_, bool act) {
        li = li_;
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
            for (int w = 0; w < VW; ++w) {
                conf_load_quad(a, row + 4 * li, 4 * ((k * VW + w) * 64), 4 * li, act, sw[k][w]);
                // (the word is final here: nothing of how it was derived stays alive into the search -- 12 registers fewer
                // on the 64-class tile)
#pragma unroll
                for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(sw[k][w][j]));
            }
    }
    template <typename F>
    __device__ __forceinline__ void each(F&& f) const {
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
            for (int w = 0; w < VW; ++w) f(w, 4 * ((k * VW + w) * 64), sw[k][w]);
    }
};
template <int VW>
struct ConfRow<VW, 0> {
    const ConfArgs* a; const float* row; int li; bool act;
    __device__ __forceinline__ void load(const ConfArgs& a_, const float* row_, int li_, bool act_) { a = &a_; row = row_; li = li_; act = act_; }
    template <typename F>
    __device__ __forceinline__ void each(F&& f) const {
        const int nq = (a->C + 3) >> 2;
        for (int q0 = 0; q0 < nq; q0 += 64 * VW) {         // (launch-uniform bounds)
            int v[VW][4];
#pragma unroll
            for (int w = 0; w < VW; ++w) conf_load_quad(*a, row + 4 * li, 4 * (q0 + w * 64), 4 * li, act, v[w]);
#pragma unroll
            for (int w = 0; w < VW; ++w) f(w, 4 * (q0 + w * 64), v[w]);
        }
    }
};

// class c = cb + li4 + j is at or above the boundary (hs, n). Where a wave works one row the boundary is the same in every
// lane (scalar registers: conf_uni below) and so is n - cb - j, which leaves one vector comparison against the lane's 4 li.
template <int VW>
__device__ __forceinline__ bool conf_above(int x, int cb, int li4, int j, int hs, int n) {
    const bool idx = VW == 1 ? (cb + li4 + j < n) : (li4 < n - (cb + j));
    return (x > hs) | ((x == hs) & idx);
}
__device__ __forceinline__ int conf_uni(int v, bool uniform) { return uniform ? __builtin_amdgcn_readfirstlane(v) : v; }

// QB masked row sums in the family's order, one per boundary. LO false: class c counts iff sw[c] >= hs[b]; LO true: iff
// sw[c] > hs[b], or sw[c] == hs[b] and c < n[b]. A class that does not count adds +0; one that does adds its word's bits as a
// float, which is its value while hs >= 0 -- the caller's part: the classes from +0 down add a zero whether they count or not
// (the same bits of a sum that started at +0), so a boundary below +0 is raised to it.
template <bool LO, int QB, int VW, typename Row>
__device__ __forceinline__ void conf_masked_sums(const Row& row, const int (&hs)[QB], const int (&n)[QB], int G, float (&S)[QB]) {
    const int li4 = 4 * row.li;
    float acc[QB][VW];
#pragma unroll
    for (int b = 0; b < QB; ++b)
#pragma unroll
        for (int w = 0; w < VW; ++w) acc[b][w] = 0.f;
    row.each([&](int w, int cb, const int (&sw)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = sw[j];
#pragma unroll
            for (int b = 0; b < QB; ++b) {
                const bool m = LO ? conf_above<VW>(x, cb, li4, j, hs[b], n[b]) : x >= hs[b];
#pragma unroll
                for (int ww = 0; ww < VW; ++ww)            // (w is a constant once unrolled)
                    if (ww == w) acc[b][ww] = acc[b][ww] + (m ? __int_as_float(x) : 0.f);
            }
        }
    });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        if (off < G)                                       // (the levels at and above G would add +0)
#pragma unroll
            for (int b = 0; b < QB; ++b)
#pragma unroll
                for (int w = 0; w < VW; ++w) acc[b][w] += __shfl_xor(acc[b][w], off, 64);
#pragma unroll
    for (int b = 0; b < QB; ++b) {
        S[b] = acc[b][0];
        if constexpr (VW == 4) S[b] = ((acc[b][0] + acc[b][1]) + acc[b][2]) + acc[b][3];
        S[b] = __int_as_float(conf_uni(__float_as_int(S[b]), VW == 4));   // (every lane of the row holds the same bits)
    }
}

// VW: the waves of the rule's T = 64 VW threads, all played by this wave. NK: see ConfRow. QB: the thresholds worked together.
// Garg (VW == 1 only): the lanes that work one row, a power of two that covers the row's quads.
template <int VW, int NK, int QB>
__global__ __launch_bounds__(conf_threads(VW)) void k_conformal(const ConfArgs a, const int Garg) {
    constexpr int CONF_T = conf_threads(VW);
    __shared__ u64 sh[CONF_WORDS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int C = a.C, Q = a.Q;
    const int G = VW == 1 ? Garg : 64;
    const int li = lane & (G - 1), RW = 64 / G;            // the lane inside its row's group; rows a wave works at once
    const bool aps = a.kind == VBNN_CONFORMAL_APS;
    const float inf = __builtin_inff(), qn = __builtin_nanf("");
    static_assert(CONF_WORDS <= CONF_T, "a thread per accumulator word");
    if (tid < CONF_WORDS) sh[tid] = 0ull;
    __syncthreads();
    const int64_t wave0 = (int64_t)blockIdx.x * (CONF_T / 64) + conf_uni(tid >> 6, true), waves = (int64_t)gridDim.x * (CONF_T / 64);
    for (int64_t base = wave0 * RW; base < a.R; base += waves * RW) {      // (wave-uniform; no barrier inside)
        const int64_t r = base + lane / G;                 // (VW == 4: base, the same in every lane)
        const bool act = r < a.R;
        const int64_t rc = act ? r : 0;                    // (a lane without a row reads row 0 and drops it)
        const float* rowp = a.probs + rc * a.ld;
        int t = 0, st = 0;
        if (a.target) {                                    // launch-uniform
            const int tv = a.target[rc];
            t = tv < 0 ? 0 : (tv > C - 1 ? C - 1 : tv);
            st = conf_uni(conf_sw(rowp[t]), VW == 4);      // (ahead of the row's loads: it returns first)
        }
        ConfRow<VW, NK> row;
        row.load(a, rowp, li, act);
        const bool lead = act && li == 0;
        // the unmasked row sum decides whether the row counts at all
        bool nan;
        {
            const int all[1] = {0}, none[1] = {0};
            float S[1];
            conf_masked_sums<false, 1, VW>(row, all, none, G, S);
            nan = S[0] != S[0];
        }
        if (a.score) {                                     // launch-uniform: s(r, t)
            float s;
            if (aps) {
                const int hs[1] = {max(st, 0)}, n[1] = {t + 1};
                float S[1];
                conf_masked_sums<true, 1, VW>(row, hs, n, G, S);
                s = S[0];
            } else {
                s = 1.f - conf_value(st);
            }
            if (lead) a.score[r] = nan ? qn : s;
        }
        if (lead && nan && a.acc) atomicAdd(&sh[8 * Q], 1ull);
        for (int q0 = 0; q0 < Q; q0 += QB) {               // launch-uniform
            float qh[QB];
            int hs[QB], n[QB];
#pragma unroll
            for (int b = 0; b < QB; ++b) {
                const float v = a.qhat[min(q0 + b, Q - 1)];
                qh[b] = (v != v) ? inf : v;                // a NaN threshold admits everything
                hs[b] = CONF_NONE; n[b] = 0;
            }
            if (aps) {
                // ONE loop for both searches (the compiler then keeps no per-class comparison of the second alive across
                // its steps: 64 classes a lane times QB would not fit the registers). Steps 0 .. 31: the largest order word h
                // with sum{w >= h} > qhat, bit by bit from the top (none: the whole row is in). The steps after: the classes
                // above that word are in; of those AT it, the largest count n in index order that still fits.
                uint32_t hi[QB];
#pragma unroll
                for (int b = 0; b < QB; ++b) hi[b] = 0u;
                const int steps = 32 + a.ibits;
                for (int s = 0; s < steps; ++s) {
                    int H[QB], N[QB];
                    float S[QB];
                    if (s < 32) {
                        const uint32_t bit = 0x80000000u >> s;
#pragma unroll
                        for (int b = 0; b < QB; ++b) { H[b] = max((int)((hi[b] | bit) ^ 0x80000000u), 0); N[b] = 0; }
                        conf_masked_sums<false, QB, VW>(row, H, N, G, S);
#pragma unroll
                        for (int b = 0; b < QB; ++b) if (!(S[b] <= qh[b])) hi[b] |= bit;
                    } else {
                        const int bit = 1 << (steps - 1 - s);
#pragma unroll
                        for (int b = 0; b < QB; ++b) { H[b] = max((int)(hi[b] ^ 0x80000000u), 0); N[b] = n[b] | bit; }
                        conf_masked_sums<true, QB, VW>(row, H, N, G, S);
#pragma unroll
                        for (int b = 0; b < QB; ++b) if (S[b] <= qh[b]) n[b] = N[b];
                    }
                }
#pragma unroll
                for (int b = 0; b < QB; ++b) {
                    hs[b] = (int)(hi[b] ^ 0x80000000u);
                    if (hi[b] == 0u) n[b] = 0;             // the whole row: no class holds the word CONF_NONE
                }
            }
            // the sets themselves: the bits, the size, and the last admitted class -- the smallest word among the members and,
            // of the members that hold it, the largest index
#pragma unroll
            for (int b = 0; b < QB; ++b) {
                if (q0 + b >= Q) continue;                 // launch-uniform: a pad of the batch
                const int64_t qr = (int64_t)(q0 + b) * a.R + rc;
                const int hb = hs[b], nb = n[b];
                const float qb = qh[b];
                const int li4 = 4 * li;
                auto member = [&](int x, int cb, int j) {
                    const bool in = aps ? conf_above<VW>(x, cb, li4, j, hb, nb) : (1.f - conf_value(x)) <= qb;
                    return in && !nan;
                };
                int cnt = 0, xmin = 0x7fffffff;
                row.each([&](int w, int cb, const int (&sw)[4]) {
                    uint32_t nib = 0u;
                    const int c0 = cb + li4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool in = member(sw[j], cb, j);
                        cnt += in ? 1 : 0;
                        nib |= in ? (1u << j) : 0u;
                        xmin = in ? min(xmin, sw[j]) : xmin;
                    }
                    if (a.member) {                        // launch-uniform: a word is the quads of eight neighbouring lanes
                        uint32_t word = nib << (c0 & 31);
#pragma unroll
                        for (int off = 1; off < 8; off <<= 1)
                            if (off < G) word |= __shfl_xor(word, off, 64);
                        const int wi = c0 >> 5;
                        if (act && (li & 7) == 0 && wi < a.nw) a.member[qr * a.nw + wi] = word;
                    }
                });
#pragma unroll
                for (int off = 32; off > 0; off >>= 1)
                    if (off < G) {
                        cnt += __shfl_xor(cnt, off, 64);
                        xmin = min(xmin, __shfl_xor(xmin, off, 64));
                    }
                int ci = -1;
                if (a.cut_index) {                         // launch-uniform
                    row.each([&](int w, int cb, const int (&sw)[4]) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) ci = (sw[j] == xmin && member(sw[j], cb, j)) ? max(ci, cb + li4 + j) : ci;
                    });
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1)
                        if (off < G) ci = max(ci, __shfl_xor(ci, off, 64));
                }
                if (!lead) continue;
                const bool cov = a.target && (aps ? (st > hb || (st == hb && t < nb)) : (1.f - conf_value(st)) <= qb);
                if (a.size) a.size[qr] = nan ? -1 : cnt;
                if (a.cut_index) a.cut_index[qr] = ci;
                if (a.cut_prob) a.cut_prob[qr] = (nan || cnt == 0) ? qn : conf_value(xmin);
                if (a.covered) a.covered[qr] = nan ? -1 : (cov ? 1 : 0);
                if (a.acc && !nan) {
                    u64* w8 = sh + 8 * (q0 + b);
                    atomicAdd(&w8[0], 1ull);
                    if (cov) atomicAdd(&w8[1], 1ull);
                    if (cnt) atomicAdd(&w8[2], (u64)cnt);
                    if (cnt == 0) atomicAdd(&w8[3], 1ull);
                    if (cnt == 1) atomicAdd(&w8[4], 1ull);
                    if (cnt == 1 && cov) atomicAdd(&w8[5], 1ull);
                    if (cnt == C) atomicAdd(&w8[6], 1ull);
                }
            }
        }
    }
    __syncthreads();
    // at most one global add per accumulator word and workgroup (words 1 and 5 stay zero without targets, 7 always)
    if (a.acc && tid < 8 * Q + 1 && sh[tid]) atomicAdd(a.acc + tid, sh[tid]);
}

template <int VW, int NK>
static void conf_launch(int64_t wave_rows, hipStream_t stream, const ConfArgs& m, int G) {
    constexpr int CONF_T = conf_threads(VW);
    // as many waves per CU as one workgroup of 1024 would be, grid-stride above (the closing adds serialise per word: calibration.hip)
    const int nb = (int)std::min<int64_t>((wave_rows + CONF_T / 64 - 1) / (CONF_T / 64), (int64_t)vbnn_cu_count() * (1024 / CONF_T));
    // (the 64-class tile with three or four thresholds a batch spills two registers: it works them in pairs)
    if (m.Q <= 1) hipLaunchKernelGGL((k_conformal<VW, NK, 1>), dim3(nb), dim3(CONF_T), 0, stream, m, G);
    else if (m.Q == 2 || NK == 4) hipLaunchKernelGGL((k_conformal<VW, NK, 2>), dim3(nb), dim3(CONF_T), 0, stream, m, G);
    else if constexpr (NK != 4) {
        if (m.Q == 3 || m.Q == 6) hipLaunchKernelGGL((k_conformal<VW, NK, 3>), dim3(nb), dim3(CONF_T), 0, stream, m, G);
        else hipLaunchKernelGGL((k_conformal<VW, NK, 4>), dim3(nb), dim3(CONF_T), 0, stream, m, G);
    }
}

extern "C" int vbnn_conformal(vbnn_ctx* ctx, const vbnn_conformal_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a && a->probs, "null argument (a, probs)");
    VBNN_REQUIRE(a->kind == VBNN_CONFORMAL_LAC || a->kind == VBNN_CONFORMAL_APS, "kind is VBNN_CONFORMAL_LAC or VBNN_CONFORMAL_APS");
    VBNN_REQUIRE(a->Q >= 0 && a->Q <= VBNN_CONFORMAL_MAX_Q, "Q outside [0, VBNN_CONFORMAL_MAX_Q]");
    VBNN_REQUIRE(a->Q == 0 || a->qhat, "qhat: Q thresholds on the device (NULL only with Q = 0)");
    VBNN_REQUIRE(a->target || (!a->score && !a->covered), "score and covered need target");
    VBNN_REQUIRE(a->R >= 1 && a->C >= 1, "shape: R and C are at least 1");
    VBNN_REQUIRE(a->R < (1ll << 31) && a->C < (1ll << 28), "shape: too large");
    VBNN_REQUIRE(a->ld >= a->C && a->ld <= (1ll << 60) / a->R, "ld");
    const void* p4[] = {a->probs, a->target, a->qhat, a->score, a->size, a->cut_index, a->cut_prob, a->covered, a->member};
    for (const void* p : p4) VBNN_REQUIRE(((uintptr_t)p & 3u) == 0, "pointers are 4-byte aligned");
    VBNN_REQUIRE(((uintptr_t)a->acc & 7u) == 0, "acc is 8-byte aligned");
    ConfArgs m;
    m.probs = a->probs; m.ld = a->ld; m.target = a->target; m.R = a->R; m.C = (int)a->C; m.kind = a->kind; m.Q = a->Q;
    m.qhat = a->qhat; m.score = a->score; m.size = a->size; m.cut_index = a->cut_index; m.cut_prob = a->cut_prob;
    m.covered = a->covered; m.member = a->member; m.acc = reinterpret_cast<u64*>(a->acc);
    m.vec = (a->ld & 3) == 0 && vbnn_al16(a->probs) && a->C >= 4;
    m.nw = (int)((a->C + 31) >> 5);
    m.ibits = 1;
    while ((1ll << m.ibits) <= a->C) ++m.ibits;
    const int64_t nq = (a->C + 3) >> 2;
    int G = 64;                                            // lanes per row: the row's quads, rounded up to a power of two
    if (a->C <= 256) { G = 1; while (G < nq) G <<= 1; }
    const int64_t wave_rows = (a->R + 64 / G - 1) / (64 / G);              // a wave works 64 / G rows at once
    vbnn_cu_scope scope(ctx);
    // (a thread of the rule owns quads i, i + T, ... under every tile, so the bits do not depend on it)
    if (a->C <= 256) conf_launch<1, 1>(wave_rows, ctx->stream, m, G);
    else if (a->C <= 1024) conf_launch<4, 1>(wave_rows, ctx->stream, m, G);
    else if (a->C <= 4096) conf_launch<4, 4>(wave_rows, ctx->stream, m, G);
    else conf_launch<4, 0>(wave_rows, ctx->stream, m, G);
    return vbnn_check_launch("k_conformal");
    VBNN_API_END
}
