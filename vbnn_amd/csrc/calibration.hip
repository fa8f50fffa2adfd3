// calibration.hip -- vbnn_predict_calibration and vbnn_selective (include/vbnn_hip.h): whether a classifier's confidence is
// earned, and what accuracy is left when the most uncertain rows are handed to somebody else. The fifth member of the moments
// family (moments.hip): streaming, no MFMA, compiled WITHOUT floating-point contraction (Makefile): every line below is the fp32
// operation it spells. Everything that ACCUMULATES across rows is an integer, so neither call's result depends on the grid, the
// arrival order, the chunking or the number of calls.
//
// k_calibration: a WAVE owns its rows from the loads to the adds -- no barrier and no LDS round trip inside a row. The family's
// row-sum rule (moments_common.h) names T = 64 threads for C <= 256 and 256 above; the wave plays all of them: for T = 256 a lane
// keeps one partial per wave of the rule (VW = 4: lane l is threads l, l + 64, l + 128, l + 192), runs the four butterflies
// side by side and adds them in wave order. For C <= 128 the row's quads fit a group of G = 2^k < 64 lanes and the wave works
// 64 / G rows at once: the butterfly levels at and above G only ever add the +0 of a lane that holds no quad, so leaving them out
// changes no bit. Either way the order of ss = sum_c p[c]^2 depends on C alone, on the 16-byte AND on the scalar path. A row's
// first lane reads p[pred] and p[target] (issued ahead of the reduction), forms the row values and adds them to the workgroup's
// LDS copy of the accumulator (integer LDS atomics); after its last row the workgroup adds every nonzero word of that copy to
// global memory once (64-bit vector atomics, as vbnn_predict_quantiles.count_le). Those closing adds serialise per word, so the
// launch is one workgroup of 16 waves per CU, grid-stride above, and not many small ones.
//
// k_selective: ONE workgroup of 1024 threads, a most-significant-digit radix select (8 bits a pass, four passes) over the ordered
// keys of the scores for all Q ranks at once. A pass histograms, per distinct prefix among the ranks (the first pass: one for
// all), the next digit of the keys under that prefix -- one LDS word per bin, the count in its low half and the count of hits in
// its high half (both below 2^31, so neither carries) -- then one wave per rank scans its prefix's 256 bins, finds the bin that
// holds the rank, and adds what lies below it to the rank's `below` pair. After the last pass the prefix is the k-th key, the
// bin's word is the tied pair. No float atomics, no allocation, no host synchronisation.
#include "device_prims.h"
#include <math.h>
#include <algorithm>

constexpr int CAL_MAXB = VBNN_CALIBRATION_MAX_BINS;
constexpr int CAL_T = 1024;                    // threads of a workgroup of k_calibration: 16 waves, each with rows of its own
constexpr int SEL_MAXQ = VBNN_SELECTIVE_MAX_Q;
constexpr int SEL_T = 1024;                    // threads of the one workgroup
constexpr int SEL_U = 16;                      // distinct prefixes histogrammed in one walk over the scores (32 KiB of LDS)
static_assert(SEL_MAXQ <= 64 && SEL_T / 64 >= 1, "one wave scans a rank's histogram; thread j finishes rank j");

typedef unsigned long long u64;

struct CalArgs {
    const float* probs; int64_t ld; const int32_t* pred; const int32_t* target; int64_t R; int C, M;
    float* conf; int32_t* hit; float* brier; int32_t* bin; u64* acc;
    int vec;                                   // 16-byte loads on the row's whole quads (its last, partial quad goes element by element)
};

struct CalShared {
    unsigned count[CAL_MAXB], hits[CAL_MAXB];  // (a workgroup sees fewer than 2^31 rows)
    u64 conf_fix[CAL_MAXB];
    u64 tail[3];                               // brier_fix, n_rows, n_nan
};

__device__ __forceinline__ int cal_clamp(int v, int C) { return v < 0 ? 0 : (v > C - 1 ? C - 1 : v); }

// ---- the loads are straight-line code: a lane with nothing to load reads a clamped address inside the row and a select
// drops the value, so no load waits behind a branch and a wave keeps its whole row in flight. VEC: the row's whole quads
// [0, nbody = C / 4) as 16 bytes; otherwise every column element by element (nbody = the row's quads, the last one partial).
template <bool VEC>
__device__ __forceinline__ void cal_load_quad(const float* row, int q, int nbody, int C, bool act, float (&v)[4]) {
    const bool ok = act && q < nbody;
    if (VEC) {
        const f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(row) + min(q, nbody - 1));   // (nbody >= 1)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ok ? t[j] : 0.f;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * q + j;
            const float x = __builtin_nontemporal_load(row + min(c, C - 1));
            v[j] = (ok && c < C) ? x : 0.f;
        }
    }
}
// the squares of one quad onto the partial of the thread that owns it, in column order (a column that is not there holds +0,
// and adding +0 changes no bit of a sum of squares)
__device__ __forceinline__ void cal_square_quad(const float (&v)[4], float& acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = acc + v[j] * v[j];
}

// VW: the waves of the rule's T = 64 VW threads, all played by this wave. NK: the quads of a thread of the rule that are loaded
// together, 64 VW NK quads of the row a step (in flight before their first use); a row wider than that takes more steps. G
// (VW == 1 only): the lanes that work one row, a power of two that covers the row's quads.
template <int VW, int NK, bool VEC>
__global__ __launch_bounds__(CAL_T) void k_calibration(const CalArgs a, const int G) {
    __shared__ CalShared sh;
    const int tid = threadIdx.x, lane = tid & 63;
    const int C = a.C, M = a.M, nq = (C + 3) >> 2;
    const int nbody = VEC ? C >> 2 : nq;                   // VEC: the columns [4 nbody, C) follow element by element
    const int li = lane & (G - 1), RW = 64 / G;            // the lane inside its row's group; rows a wave works at once
    if (tid < CAL_MAXB) { sh.count[tid] = 0u; sh.hits[tid] = 0u; sh.conf_fix[tid] = 0ull; }
    if (tid < 3) sh.tail[tid] = 0ull;
    __syncthreads();
    const int64_t wave0 = (int64_t)blockIdx.x * (CAL_T / 64) + (tid >> 6), waves = (int64_t)gridDim.x * (CAL_T / 64);
    for (int64_t base = wave0 * RW; base < a.R; base += waves * RW) {      // (wave-uniform; no barrier inside)
        const int64_t r = base + lane / G;
        const bool act = r < a.R;
        const int64_t rc = act ? r : 0;                    // (a lane without a row reads row 0 and drops it)
        const float* row = a.probs + rc * a.ld;
        const int p = cal_clamp(a.pred[rc], C), t = cal_clamp(a.target[rc], C);
        float acc[VW];
#pragma unroll
        for (int w = 0; w < VW; ++w) acc[w] = 0.f;
        const float conf = row[p], pt = row[t];            // (ahead of the row's loads: they return first)
        for (int q0 = 0; q0 < nq; q0 += 64 * VW * NK) {    // (one step while C <= 1024 NK)
            float v[NK][VW][4];
#pragma unroll
            for (int k = 0; k < NK; ++k)
#pragma unroll
                for (int w = 0; w < VW; ++w) cal_load_quad<VEC>(row, q0 + (k * VW + w) * 64 + li, nbody, C, act, v[k][w]);
#pragma unroll
            for (int k = 0; k < NK; ++k)
#pragma unroll
                for (int w = 0; w < VW; ++w) cal_square_quad(v[k][w], acc[w]);
        }
        if (VEC && (C & 3)) {                              // launch-uniform: the partial quad, the LAST of the thread that owns it
            const int own = nbody % (64 * VW);
            float tv[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int c = 4 * nbody + j;
                const float x = __builtin_nontemporal_load(row + min(c, C - 1));
                tv[j] = (act && c < C) ? x : 0.f;
            }
#pragma unroll
            for (int w = 0; w < VW; ++w) {
                const bool mine = w == (own >> 6) && li == (own & 63);
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[w] = acc[w] + (mine ? tv[j] * tv[j] : 0.f);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            if (off < G)                                   // (the levels at and above G would add +0)
#pragma unroll
                for (int w = 0; w < VW; ++w) acc[w] += __shfl_xor(acc[w], off, 64);
        float ss = acc[0];
        if constexpr (VW == 4) ss = ((acc[0] + acc[1]) + acc[2]) + acc[3];
        if (!act || li != 0) continue;                     // the row's first lane goes on alone
        const bool nan = conf != conf || ss != ss;
        const float qn = __builtin_nanf("");
        const int hit = p == t ? 1 : 0;
        const float brier = fmaxf((ss - 2.f * pt) + 1.f, 0.f);
        // min(int(conf M), M - 1), clamped on the float so that no value of conf can index outside the M bins
        const int bin = (int)fminf(fmaxf(conf * (float)M, 0.f), (float)(M - 1));
        if (a.conf) a.conf[r] = nan ? qn : conf;
        if (a.hit) a.hit[r] = nan ? -1 : hit;
        if (a.brier) a.brier[r] = nan ? qn : brier;
        if (a.bin) a.bin[r] = nan ? -1 : bin;
        if (nan) {
            atomicAdd(&sh.tail[2], 1ull);
        } else {
            atomicAdd(&sh.count[bin], 1u);
            if (hit) atomicAdd(&sh.hits[bin], 1u);
            atomicAdd(&sh.conf_fix[bin], (u64)(fmaxf(conf, 0.f) * 4294967296.f));
            atomicAdd(&sh.tail[0], (u64)(brier * 4294967296.f));
            atomicAdd(&sh.tail[1], 1ull);
        }
    }
    __syncthreads();
    // at most one global add per accumulator word and workgroup
    if (tid < M) {
        if (sh.count[tid]) atomicAdd(a.acc + tid, (u64)sh.count[tid]);
        if (sh.hits[tid]) atomicAdd(a.acc + M + tid, (u64)sh.hits[tid]);
        if (sh.conf_fix[tid]) atomicAdd(a.acc + 2 * M + tid, sh.conf_fix[tid]);
    } else if (tid >= 64 && tid < 67) {                    // (M <= 64: these threads hold no bin)
        if (sh.tail[tid - 64]) atomicAdd(a.acc + 3 * M + (tid - 64), sh.tail[tid - 64]);
    }
}

template <int VW, int NK>
static void cal_launch(int nb, hipStream_t stream, const CalArgs& m, int G) {
    if (m.vec) hipLaunchKernelGGL((k_calibration<VW, NK, true>), dim3(nb), dim3(CAL_T), 0, stream, m, G);
    else hipLaunchKernelGGL((k_calibration<VW, NK, false>), dim3(nb), dim3(CAL_T), 0, stream, m, G);
}

extern "C" int vbnn_predict_calibration(vbnn_ctx* ctx, const vbnn_calibration_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a && a->probs && a->pred && a->target && a->acc, "null argument (a, probs, pred, target, acc)");
    VBNN_REQUIRE(a->R >= 1 && a->C >= 1, "shape: R and C are at least 1");
    VBNN_REQUIRE(a->R < (1ll << 31) && a->C < (1ll << 28), "shape: too large");
    VBNN_REQUIRE(a->bins >= 1 && a->bins <= VBNN_CALIBRATION_MAX_BINS, "bins outside [1, VBNN_CALIBRATION_MAX_BINS]");
    VBNN_REQUIRE(a->ld >= a->C && a->ld <= (1ll << 60) / a->R, "ld");
    VBNN_REQUIRE(((uintptr_t)a->acc & 7u) == 0, "acc is 8-byte aligned");
    CalArgs m;
    m.probs = a->probs; m.ld = a->ld; m.pred = a->pred; m.target = a->target; m.R = a->R; m.C = (int)a->C; m.M = a->bins;
    m.conf = a->conf; m.hit = a->hit; m.brier = a->brier; m.bin = a->bin; m.acc = reinterpret_cast<u64*>(a->acc);
    m.vec = (a->ld & 3) == 0 && vbnn_al16(a->probs) && a->C >= 4;
    const int64_t nq = (a->C + 3) >> 2;
    int G = 64;                                            // lanes per row: the row's quads, rounded up to a power of two
    if (a->C <= 256) { G = 1; while (G < nq) G <<= 1; }
    const int64_t wave_rows = (a->R + 64 / G - 1) / (64 / G);              // a wave works 64 / G rows at once
    vbnn_cu_scope scope(ctx);
    // ONE workgroup of 16 waves per CU, grid-stride above: every workgroup ends with its adds to the same few words, and those
    // serialise (2048 workgroups of four waves spent ~25 us on them at any size; measured, README)
    const int nb = (int)std::min<int64_t>((wave_rows + CAL_T / 64 - 1) / (CAL_T / 64), (int64_t)vbnn_cu_count());
    // (a thread of the rule owns quads i, i + T, ... under every tile, so the bits do not depend on it)
    if (a->C <= 256) cal_launch<1, 1>(nb, ctx->stream, m, G);
    else if (a->C <= 4 * 256 * 1) cal_launch<4, 1>(nb, ctx->stream, m, G);
    else cal_launch<4, 2>(nb, ctx->stream, m, G);
    return vbnn_check_launch("k_calibration");
    VBNN_API_END
}

// ---- vbnn_selective
struct SelArgs {
    const float* score; const int32_t* hit; int64_t R; int Q; int64_t k[SEL_MAXQ]; float* tau; u64* counts;
};

__global__ __launch_bounds__(SEL_T) void k_selective(const SelArgs a) {
    __shared__ u64 hist[SEL_U][256];           // low half: keys in the bin; high half: hits among them
    __shared__ unsigned pref[SEL_MAXQ];        // the digits of rank j's key found so far (the rest zero)
    __shared__ unsigned krem[SEL_MAXQ];        // rank j among the keys under its prefix, 1-based
    __shared__ u64 below[SEL_MAXQ], tied[SEL_MAXQ];
    __shared__ unsigned upref[SEL_MAXQ];       // the distinct prefixes, and which of them rank j has
    __shared__ int lead[SEL_MAXQ];
    __shared__ int nu_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Q = a.Q;
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < SEL_MAXQ; ++j) {   // (unrolled: a run-time index into the by-value argument would go through scratch)
            pref[j] = 0u; krem[j] = (unsigned)a.k[j]; below[j] = 0ull; tied[j] = 0ull;
        }
    }
    __syncthreads();
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned hi_mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
        if (tid == 0) {
            int nu = 0;
            for (int j = 0; j < Q; ++j) {
                int u = 0;
                while (u < nu && upref[u] != pref[j]) ++u;
                if (u == nu) upref[nu++] = pref[j];
                lead[j] = u;
            }
            nu_s = nu;
        }
        __syncthreads();
        const int nu = nu_s;
        for (int u0 = 0; u0 < nu; u0 += SEL_U) {
            const int nb = min(SEL_U, nu - u0);
            for (int i = tid; i < nb * 256; i += SEL_T) hist[i >> 8][i & 255] = 0ull;
            __syncthreads();
            for (int64_t i = tid; i < a.R; i += SEL_T) {
                const float f = a.score[i];                // the key: every NaN is the positive quiet NaN, above +inf
                const unsigned key = vbnn_order_word((f != f) ? 0x7fc00000u : __float_as_uint(f));
                const u64 inc = 1ull | (a.hit[i] != 0 ? (1ull << 32) : 0ull);
                const int digit = (int)((key >> shift) & 255u);
                for (int u = 0; u < nb; ++u)
                    if (((key ^ upref[u0 + u]) & hi_mask) == 0u) atomicAdd(&hist[u][digit], inc);
            }
            __syncthreads();
            // one wave per rank: lane l holds bins 4 l .. 4 l + 3; exactly one (lane, bin) holds the rank
            for (int j = wave; j < Q; j += SEL_T / 64) {
                const int u = lead[j] - u0;
                if (u < 0 || u >= nb) continue;            // wave-uniform
                const unsigned kr = krem[j];
                unsigned c[4], h[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const u64 w = hist[u][4 * lane + b];
                    c[b] = (unsigned)w; h[b] = (unsigned)(w >> 32);
                }
                const unsigned cs = (c[0] + c[1]) + (c[2] + c[3]), hs = (h[0] + h[1]) + (h[2] + h[3]);
                const unsigned ci = vbnn_wave_scan_incl(cs), hh = vbnn_wave_scan_incl(hs);
                unsigned ce = ci - cs, he = hh - hs;       // below this lane's first bin
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    if (kr > ce && kr <= ce + c[b]) {
                        pref[j] |= (unsigned)(4 * lane + b) << shift;
                        krem[j] = kr - ce;
                        below[j] += (u64)ce | ((u64)he << 32);
                        tied[j] = (u64)c[b] | ((u64)h[b] << 32);
                    }
                    ce += c[b]; he += h[b];
                }
            }
            __syncthreads();
        }
    }
    if (tid < Q) {
        a.tau[tid] = __uint_as_float(vbnn_unorder_word(pref[tid]));
        a.counts[4 * tid + 0] = below[tid] & 0xffffffffull;
        a.counts[4 * tid + 1] = below[tid] >> 32;
        a.counts[4 * tid + 2] = tied[tid] & 0xffffffffull;
        a.counts[4 * tid + 3] = tied[tid] >> 32;
    }
}

extern "C" int vbnn_selective(vbnn_ctx* ctx, const vbnn_selective_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a && a->score && a->hit && a->tau && a->counts, "null argument (a, score, hit, tau, counts)");
    VBNN_REQUIRE(a->R >= 1 && a->R < (1ll << 31), "R outside [1, 2^31)");
    VBNN_REQUIRE(a->Q >= 1 && a->Q <= VBNN_SELECTIVE_MAX_Q, "Q outside [1, VBNN_SELECTIVE_MAX_Q]");
    for (int j = 0; j < a->Q; ++j) VBNN_REQUIRE(a->k[j] >= 1 && a->k[j] <= a->R, "k outside [1, R]");
    VBNN_REQUIRE(((uintptr_t)a->counts & 7u) == 0, "counts is 8-byte aligned");
    SelArgs m;
    m.score = a->score; m.hit = a->hit; m.R = a->R; m.Q = a->Q; m.tau = a->tau; m.counts = reinterpret_cast<u64*>(a->counts);
    for (int j = 0; j < SEL_MAXQ; ++j) m.k[j] = j < a->Q ? a->k[j] : 1;
    hipLaunchKernelGGL(k_selective, dim3(1), dim3(SEL_T), 0, ctx->stream, m);
    return vbnn_check_launch("k_selective");
    VBNN_API_END
}
