// ranking.hip -- vbnn_rank_metrics (include/vbnn_hip.h): per column of an R x D score matrix the integers that AUROC, average
// precision and the hit counts at chosen thresholds are ratios of. Everything that is counted is an integer and the sort is
// exact, so the output does not depend on the grid, the arrival order of the atomics or the arrangement of the sort. Compiled
// WITHOUT floating-point contraction like the rest of the moments family (Makefile); the only float operations are the two
// comparisons t > 0.5f and x != x.
//
// k_rank_pack: tiles of RK_TILE = 4096 elements, TC columns (a power of two that covers D, at most 64) by 4096 / TC rows, so a
// thread's column is the same in every step and in every tile: it keeps the column's counts in registers over all the tiles of
// its workgroup. A tile is read row-major (lanes along the columns), turned in LDS and written column-major (lanes along the
// rows): both sides of the transposition are contiguous.
// k_rank_column: ONE workgroup of 1024 threads per column, start to end -- the four digit histograms, the stable radix passes
// through the two halves of the workspace, the walk. The stable rank of a record inside its wave comes from eight ballots on the
// digit's bits (the lanes that hold the same digit), the waves' counts per digit are prefixed in wave order in LDS, and the
// running base of each digit moves on tile by tile. A workgroup reads in one pass what its own waves wrote in the pass before:
// they share the CU's L1, and __syncthreads orders the accesses. The walk closes a run of equal order words at the START of the
// next run (the last one after the loop), from the counts of positives and negatives before the run, carried across tiles.
#include "device_prims.h"
#include <string.h>
#include <algorithm>

constexpr int RK_MAXQ = VBNN_RANK_MAX_Q;
constexpr int RK_WORDS = 3 + 2 * RK_MAXQ;      // the counts the pack pass takes for a column: n_pos, n_neg, n_nan, tp_q, fp_q
constexpr int RK_TILE = 4096;                  // elements of a pack tile
constexpr int RK_PT = 256;                     // threads of a pack workgroup
constexpr int RK_ST = 1024;                    // threads of a column's workgroup: 16 waves
constexpr int RK_SW = RK_ST / 64;
static_assert(RK_TILE % RK_PT == 0 && RK_PT % 64 == 0 && RK_ST >= 256, "a pack thread keeps its column; a sort thread per digit");

typedef unsigned long long u64;

struct RankArgs {
    const uint32_t* score; int64_t ld;
    const float* target; int64_t ld_t;
    const int32_t* tclass;
    int64_t R, D;
    int Q;
    uint32_t tauk[RK_MAXQ];                    // the thresholds' order words (0xffffffff for a NaN: above every counted score)
    u64* out; u64* ws;
    int ltc;                                   // log2 of the pack tile's columns
    int64_t ncol_t, nrow_t, nrg;               // column tiles, row tiles, workgroups that share a column tile's row tiles
};

__global__ __launch_bounds__(RK_PT) void k_rank_pack(const RankArgs a) {
    __shared__ u64 tile[RK_TILE + 64];         // [TC][TR + 1] records
    __shared__ unsigned cnt[64 * RK_WORDS];    // [TC][RK_WORDS] (a workgroup sees fewer than 2^31 elements of a column)
    const int tid = threadIdx.x;
    const int ltc = a.ltc, TC = 1 << ltc, TR = RK_TILE >> ltc, ltr = 12 - ltc;
    const int64_t ct = blockIdx.x / a.nrg, rg = blockIdx.x % a.nrg;
    const int64_t c0 = ct * TC;
    const int col = tid & (TC - 1);            // (RK_PT is a multiple of TC: the same column in every step)
    const int64_t c = c0 + col;
    const bool cok = c < a.D;
    const int Q = a.Q;
    for (int i = tid; i < TC * RK_WORDS; i += RK_PT) cnt[i] = 0u;
    __syncthreads();
    unsigned n_pos = 0u, n_neg = 0u, n_nan = 0u, tp[RK_MAXQ], fp[RK_MAXQ];
#pragma unroll
    for (int q = 0; q < RK_MAXQ; ++q) { tp[q] = 0u; fp[q] = 0u; }
    for (int64_t rt = rg; rt < a.nrow_t; rt += a.nrg) {
        const int64_t r0 = rt * TR;
#pragma unroll 4
        for (int k = 0; k < RK_TILE / RK_PT; ++k) {
            const int row = (tid + RK_PT * k) >> ltc;
            const int64_t r = r0 + row;
            if (cok && r < a.R) {
                uint32_t u = a.score[r * a.ld + c];
                bool counted = !vbnn_bits_nan(u), pos;
                if (a.target) {
                    const float t = a.target[r * a.ld_t + c];
                    counted = counted && t == t;
                    pos = t > 0.5f;
                } else {
                    const int64_t t = a.tclass[r];
                    pos = (t < 0 ? 0 : (t > a.D - 1 ? a.D - 1 : t)) == c;
                }
                if (u == 0x80000000u) u = 0u;          // -0 as +0: what s + 0.0f gives
                const uint32_t key = vbnn_order_word(u);
                tile[col * (TR + 1) + row] = counted ? (((u64)key << 1) | (pos ? 1ull : 0ull)) : ~0ull;
                if (!counted) ++n_nan;
                else {
                    if (pos) ++n_pos; else ++n_neg;
#pragma unroll
                    for (int q = 0; q < RK_MAXQ; ++q)
                        if (q < Q && key >= a.tauk[q]) { if (pos) ++tp[q]; else ++fp[q]; }
                }
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < RK_TILE / RK_PT; ++k) {
            const int i = tid + RK_PT * k, row = i & (TR - 1), wc = i >> ltr;
            const int64_t r = r0 + row, cc = c0 + wc;
            if (cc < a.D && r < a.R) a.ws[cc * a.R + r] = tile[wc * (TR + 1) + row];
        }
        __syncthreads();
    }
    // the thread's counts onto its column's (LDS), then at most one global add per word and workgroup
    unsigned* mine = cnt + col * RK_WORDS;
    if (n_pos) atomicAdd(mine + 0, n_pos);
    if (n_neg) atomicAdd(mine + 1, n_neg);
    if (n_nan) atomicAdd(mine + 2, n_nan);
#pragma unroll
    for (int q = 0; q < RK_MAXQ; ++q) {
        if (tp[q]) atomicAdd(mine + 3 + 2 * q, tp[q]);
        if (fp[q]) atomicAdd(mine + 4 + 2 * q, fp[q]);
    }
    __syncthreads();
    const int words = 3 + 2 * Q, stride = 6 + 2 * Q;
    for (int i = tid; i < TC * words; i += RK_PT) {
        const int wc = i / words, w = i - wc * words;
        const unsigned v = cnt[wc * RK_WORDS + w];
        if (v && c0 + wc < a.D) atomicAdd(a.out + (c0 + wc) * stride + (w < 3 ? w : w + 3), (u64)v);
    }
}

// the lanes of the wave that are `valid` and hold the digit d (eight ballots)
__device__ __forceinline__ u64 rk_match(unsigned d, bool valid) {
    u64 m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const u64 bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

__global__ __launch_bounds__(RK_ST) void k_rank_column(const RankArgs a) {
    __shared__ unsigned hist[4][256];          // the column's records per digit value, for each of the four digits
    __shared__ unsigned wcnt[RK_SW][256];      // a tile's records per wave and digit value; then where the wave's first of them goes
    __shared__ unsigned base[256];             // where the next tile's first record of a digit value goes
    __shared__ int skip[4];
    __shared__ unsigned wpos[RK_SW];           // the walk: positives in each wave of the tile
    __shared__ int wstart[RK_SW];              //   the last run start in each wave (-1: none)
    __shared__ unsigned spex[RK_ST];           //   positives before each record of the tile
    __shared__ u64 red[2][RK_SW];
    __shared__ unsigned carry[4];              //   positives so far; the open run's positives / negatives before it; its order word
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 below = (1ull << lane) - 1ull;
    const int64_t n = a.R;
    const int stride = 6 + 2 * a.Q;
    u64* outc = a.out + (int64_t)blockIdx.x * stride;
    u64* cur = a.ws + (int64_t)blockIdx.x * n;
    u64* alt = cur + a.R * a.D;

    // ---- the four histograms of the order word's digits (bits 1 .. 32 of a record), in one read
    for (int i = tid; i < 4 * 256; i += RK_ST) hist[i >> 8][i & 255] = 0u;
    __syncthreads();
    for (int64_t i0 = 0; i0 < n; i0 += RK_ST) {
        const int64_t i = i0 + tid;
        const bool valid = i < n;
        const u64 rec = valid ? cur[i] : 0ull;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const unsigned d = (unsigned)(rec >> (1 + 8 * p)) & 255u;
            const u64 m = rk_match(d, valid);
            if (valid && (m & below) == 0ull) atomicAdd(&hist[p][d], (unsigned)__popcll(m));
        }
    }
    __syncthreads();
    if (tid < 4) skip[tid] = 0;
    __syncthreads();
    {   // a digit on which every record agrees decides nothing
        const int p = tid >> 8, d = tid & 255;
        if (hist[p][d] == (unsigned)n) skip[p] = 1;
    }
    __syncthreads();

    // ---- the stable passes, least significant digit first
    for (int p = 0; p < 4; ++p) {
        if (skip[p]) continue;                 // (workgroup-uniform)
        if (tid < 256) {                       // the exclusive prefix of the digit's histogram: one wave scan per 64 values
            const unsigned v = hist[p][tid];
            const unsigned inc = vbnn_wave_scan_incl(v);
            base[tid] = inc - v;
            if (lane == 63) wpos[wave] = inc;
        }
        __syncthreads();
        if (tid < 256) {
            unsigned add = 0u;
            for (int w = 0; w < wave; ++w) add += wpos[w];
            base[tid] += add;
        }
        __syncthreads();
        const int shift = 1 + 8 * p;
        for (int64_t i0 = 0; i0 < n; i0 += RK_ST) {
            const int64_t i = i0 + tid;
            const bool valid = i < n;
            const u64 rec = valid ? cur[i] : 0ull;
            const unsigned d = (unsigned)(rec >> shift) & 255u;
            for (int j = tid; j < RK_SW * 256; j += RK_ST) wcnt[j >> 8][j & 255] = 0u;
            __syncthreads();
            const u64 m = rk_match(d, valid);
            const unsigned rank = (unsigned)__popcll(m & below);
            if (valid && rank == 0u) wcnt[wave][d] = (unsigned)__popcll(m);
            __syncthreads();
            if (tid < 256) {
                unsigned at = base[tid];
#pragma unroll
                for (int w = 0; w < RK_SW; ++w) {
                    const unsigned v = wcnt[w][tid];
                    wcnt[w][tid] = at;
                    at += v;
                }
                base[tid] = at;
            }
            __syncthreads();
            if (valid) alt[wcnt[wave][d] + rank] = rec;       // (below n: the digit's base plus its records before this one)
            __syncthreads();
        }
        u64* t = cur; cur = alt; alt = t;
    }

    // ---- the walk over the counted records (they come first: a record that is not counted is all ones)
    const unsigned n_pos = (unsigned)outc[0], n_neg = (unsigned)outc[1];
    const int64_t nc = (int64_t)n_pos + (int64_t)n_neg;
    if (tid < 4) carry[tid] = 0u;
    __syncthreads();
    u64 u2 = 0ull, ap = 0ull;
    for (int64_t i0 = 0; i0 < nc; i0 += RK_ST) {
        const int64_t i = i0 + tid;
        const bool valid = i < nc;
        const u64 rec = valid ? cur[i] : 0ull;
        const bool pos = valid && (rec & 1ull);
        const unsigned key = (unsigned)(rec >> 1);
        // the record before this one: the lane below, the wave below's last (global memory), the tile before's last (carry)
        unsigned pk = __shfl_up(key, 1, 64);
        if (lane == 0 && valid && i > 0) pk = (unsigned)(cur[i - 1] >> 1);
        const bool start = valid && (i == 0 || pk != key);
        const u64 bp = __ballot(pos), bs = __ballot(start);
        if (lane == 0) {
            wpos[wave] = (unsigned)__popcll(bp);
            wstart[wave] = bs ? wave * 64 + 63 - __clzll((long long)bs) : -1;
        }
        __syncthreads();
        unsigned pex = carry[0] + (unsigned)__popcll(bp & below);     // positives before this record in the column
        int sprev = -1;                                               // the run start of the record before this one (tile index)
        for (int w = 0; w < wave; ++w) {
            pex += wpos[w];
            if (wstart[w] >= 0) sprev = wstart[w];
        }
        if (bs & below) sprev = wave * 64 + 63 - __clzll((long long)(bs & below));
        spex[tid] = pex;
        __syncthreads();
        if (start && i > 0) {                  // closes the run that ends at i - 1
            const unsigned pb = sprev >= 0 ? spex[sprev] : carry[1];
            const unsigned nb = sprev >= 0 ? (unsigned)(i0 + sprev) - pb : carry[2];
            const u64 p = pex - pb, m = ((unsigned)i - pex) - nb;
            u2 += p * (2ull * nb + m);
            if (p) {
                const u64 tpv = n_pos - pb, fpv = n_neg - nb;
                ap += p * ((tpv << 32) / (tpv + fpv));
            }
        }
        __syncthreads();
        if (valid && (tid == RK_ST - 1 || i == nc - 1)) {      // the tile's last record: what the next tile needs
            const int s = start ? tid : sprev;
            if (s >= 0) { carry[1] = spex[s]; carry[2] = (unsigned)(i0 + s) - spex[s]; }
            carry[0] = pex + (pos ? 1u : 0u);
        }
        __syncthreads();
    }
    if (tid == 0 && nc > 0) {                  // the last run
        const unsigned pb = carry[1], nb = carry[2];
        const u64 p = n_pos - pb, m = n_neg - nb;
        u2 += p * (2ull * nb + m);
        if (p) ap += p * ((p << 32) / (p + m));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        u2 += __shfl_xor(u2, off, 64);
        ap += __shfl_xor(ap, off, 64);
    }
    if (lane == 0) { red[0][wave] = u2; red[1][wave] = ap; }
    __syncthreads();
    if (tid < 2) {
        u64 s = 0ull;
        for (int w = 0; w < RK_SW; ++w) s += red[tid][w];
        outc[3 + tid] = s;
    }
}

static int rank_shape(int64_t R, int64_t D) {
    VBNN_REQUIRE(R >= 1 && D >= 1, "shape: R and D are at least 1");
    VBNN_REQUIRE(R <= 0x7fffffffll && D <= 0x7fffffffll && R <= 0x7fffffffll / D, "shape: R D is at most 2^31 - 1");
    return VBNN_OK;
}

extern "C" int vbnn_rank_metrics_workspace_bytes(int64_t R, int64_t D, size_t* bytes) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(bytes, "null argument");
    if (int st = rank_shape(R, D)) return st;
    *bytes = (size_t)16 * (size_t)R * (size_t)D;
    return VBNN_OK;
    VBNN_API_END
}

extern "C" int vbnn_rank_metrics(vbnn_ctx* ctx, const vbnn_rank_metrics_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a, "null argument");
    if (int st = rank_shape(a->R, a->D)) return st;
    VBNN_REQUIRE(a->Q >= 0 && a->Q <= VBNN_RANK_MAX_Q, "Q outside [0, VBNN_RANK_MAX_Q]");
    VBNN_REQUIRE(a->score && a->out && a->workspace, "null score, out or workspace");
    VBNN_REQUIRE((a->target != nullptr) != (a->target_class != nullptr), "exactly one of target and target_class");
    VBNN_REQUIRE(a->ld >= a->D && a->ld <= (1ll << 60) / a->R, "ld");
    VBNN_REQUIRE(!a->target || (a->ld_t >= a->D && a->ld_t <= (1ll << 60) / a->R), "ld_t");
    VBNN_REQUIRE(((uintptr_t)a->score & 3u) == 0 && ((uintptr_t)a->target & 3u) == 0 && ((uintptr_t)a->target_class & 3u) == 0 &&
                 ((uintptr_t)a->out & 7u) == 0 && ((uintptr_t)a->workspace & 7u) == 0, "alignment (4 bytes; out and the workspace 8)");
    VBNN_REQUIRE(a->workspace_bytes >= (size_t)16 * (size_t)a->R * (size_t)a->D, "workspace_bytes");

    RankArgs m;
    m.score = reinterpret_cast<const uint32_t*>(a->score); m.ld = a->ld;
    m.target = a->target; m.ld_t = a->ld_t; m.tclass = a->target_class;
    m.R = a->R; m.D = a->D; m.Q = a->Q;
    for (int q = 0; q < RK_MAXQ; ++q) {
        uint32_t u = 0x7fc00000u;
        if (q < a->Q) memcpy(&u, &a->tau[q], 4);
        if (u == 0x80000000u) u = 0u;          // as the scores: -0 as +0
        m.tauk[q] = vbnn_bits_nan(u) ? 0xffffffffu : vbnn_order_word(u);
    }
    m.out = reinterpret_cast<u64*>(a->out); m.ws = reinterpret_cast<u64*>(a->workspace);
    m.ltc = 0;
    while (m.ltc < 6 && (1ll << m.ltc) < a->D) ++m.ltc;
    const int64_t TC = 1ll << m.ltc, TR = RK_TILE / TC;
    m.ncol_t = (a->D + TC - 1) / TC;
    m.nrow_t = (a->R + TR - 1) / TR;
    vbnn_cu_scope scope(ctx);
    // ~8 pack workgroups per CU: a workgroup's closing adds serialise per word, so a column tile's row tiles are shared by few
    m.nrg = std::min<int64_t>(m.nrow_t, std::max<int64_t>(1, (int64_t)vbnn_cu_count() * 8 / m.ncol_t));
    VBNN_CHECK_HIP(hipMemsetAsync(a->out, 0, (size_t)a->D * (size_t)(6 + 2 * a->Q) * sizeof(u64), ctx->stream));
    hipLaunchKernelGGL(k_rank_pack, dim3((unsigned)(m.ncol_t * m.nrg)), dim3(RK_PT), 0, ctx->stream, m);
    hipLaunchKernelGGL(k_rank_column, dim3((unsigned)a->D), dim3(RK_ST), 0, ctx->stream, m);
    return vbnn_check_launch("vbnn_rank_metrics");
    VBNN_API_END
}
