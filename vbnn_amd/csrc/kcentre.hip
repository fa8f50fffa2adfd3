// kcentre.hip -- vbnn_kcentre: greedy k-centre (core-set) selection over R x D fp32 features, optionally weighted by a per-row
// score. The contract is include/vbnn_hip.h's; this file is its shape. Compiled without fp contraction (Makefile): a distance
// is subtractions, multiplications and additions rounded one by one, in an order that depends on D alone.
//
// Shape: one kernel, k_kc_pass, in two instantiations per row width.
//   * the initial centres go in blocks of kc_block(D) (<= 8) centres per pass over feat, the block's rows staged in LDS;
//   * then k + 1 step launches. Launch j reads the pick of launch j - 1 from the device word best[j - 1], stages that ONE row
//     in LDS, lowers every row's running minimum by its distance to it, forms the row's key and folds (order word << 32 | ~row)
//     over the workgroup; one 64-bit integer atomic max per workgroup settles best[j]. The maximum of a set does not depend
//     on the order of arrival, so neither do the bits. Launch k only applies the last pick. No launch waits for another
//     workgroup, nothing returns to the host between launches.
//   * a one-workgroup finish writes index / key, the tail and the counts.
// The first launch of a call (whichever it is) also takes every row's squared norm -- the void rows -- and the row's standing
// (candidate or not: one byte per row of workspace, which later launches read instead of exclude and the weight's sign).
// feat is re-read by every launch and takes plain loads: up to about 200 MB it stays in the 256 MiB Infinity Cache between
// launches (the per-row streams of a launch are 9 B a row). min_dist, weight and the standing are read once per launch, but a
// 4-byte scalar per row per wave has no vector form to hint.
#include "moments_common.h"
#include "device_prims.h"

constexpr int KC_THREADS = 256;
constexpr int KC_WAVE_MAX_D = 1024;                              // a wave per row up to here (four quads a lane), the workgroup above
constexpr int KC_MAX_NQ = VBNN_KCENTRE_MAX_D / 4 / KC_THREADS;   // quads a thread holds of a workgroup-wide row: 8
constexpr int KC_MAX_BLOCK = 8;                                  // initial centres per pass, at most
constexpr int KC_BLOCK_FLOATS = 32768;                           // ... and as many as fit 128 KiB of LDS
static_assert(VBNN_KCENTRE_MAX_D % (4 * KC_THREADS) == 0, "a thread's quads cover the cap");
// workspace bytes: ignored centres (int64) | cand, void, excluded (uint32 x 4) | best[MAX_K + 1] (uint64) | standing[R] (uint8)
constexpr size_t KC_OFF_CNT = 8, KC_OFF_BEST = 64;
constexpr size_t KC_OFF_FLAG = KC_OFF_BEST + 8 * (size_t)(VBNN_KCENTRE_MAX_K + 1);
static inline size_t kc_ws_bytes(int64_t R) { return KC_OFF_FLAG + (size_t)R; }
static inline int kc_dq(int64_t D) { return (int)((D + 3) / 4 * 4); }
static inline int kc_block(int64_t D) { return std::max(1, std::min(KC_MAX_BLOCK, KC_BLOCK_FLOATS / kc_dq(D))); }

struct KcPass {
    const float* feat; int64_t ld, R; int32_t D, mode;           // mode 2: 16-byte loads, 1: 8-byte, 0: 4-byte
    const float* weight; const uint8_t* exclude;
    float* min_dist; uint8_t* flag;
    const int32_t* centres; int32_t nc;                          // this pass's slice of the initial centres, or
    const unsigned long long* prev;                              // the word the previous step left (step launches; NULL: no centre)
    unsigned long long* best;                                    // where this launch's pick is settled, or NULL
    float* dist_out;                                             // dist[j - 1] (step launches; may be NULL)
    uint32_t* cnt;                                               // first launch: candidates, void, excluded
    int32_t first, resume;
};

// columns col .. col + 3 of a row (`valid` of them inside the row; the rest read as 0 and are never loaded: a pad is not read)
__device__ __forceinline__ void kc_load4(const float* p, float (&v)[4], int valid, int mode) {
    if (valid == 4) { mom_load4<false>(p, v, 4, mode); return; }
    v[0] = v[1] = v[2] = v[3] = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) if (j < valid) v[j] = p[j];
}

// TPR threads share a row (64: a wave, four rows a workgroup, no barrier in the row loop -- at D = 512 a workgroup per row left
// half its threads idle and spent 118 us a step on 10^5 rows; 256: the workgroup), each holding NQ quads: quad i, i + TPR, ...
// NC: the centres a pass can apply (1: a step launch; KC_MAX_BLOCK: an initial block).
template <int TPR, int NQ, int NC>
__global__ __launch_bounds__(KC_THREADS) void k_kc_pass(KcPass a) {
    extern __shared__ __attribute__((aligned(16))) float cen[];   // NC rows of dq floats, zero past D
    __shared__ float red[NC + 1][4];
    __shared__ int c_row[NC];                                     // the centre's row, -1: none (out of range, void)
    __shared__ unsigned long long wg_best[KC_THREADS / 64];
    __shared__ uint32_t wg_cnt[3];
    constexpr int WPR = TPR / 64, RPB = KC_THREADS / TPR;
    const int tid = threadIdx.x, wave = tid >> 6, tr = tid % TPR;
    const int dq = (a.D + 3) / 4 * 4, nquad = dq / 4;
    int nc = a.nc;
    if (a.prev) {                                                 // a step launch after the first: the previous launch's pick
        const unsigned long long b = *a.prev;
        if (b == 0ull) return;                                    // the candidates ran out: nothing to apply, nothing to pick
        nc = 1;
        if (tid == 0) c_row[0] = (int)~(uint32_t)b;
    } else if (tid < NC) {
        int c = -1;
        if (tid < nc) { c = a.centres[tid]; if (c < 0 || (int64_t)c >= a.R) c = -1; }
        c_row[tid] = c;
    }
    if (tid < 3) wg_cnt[tid] = 0u;
    __syncthreads();
    // stage the block's rows; then every workgroup takes their norms in the row order and drops the void ones
    for (int j = 0; j < nc; ++j) {
        const int c = c_row[j];
        for (int q = tid; q < nquad; q += KC_THREADS) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (c >= 0) kc_load4(a.feat + (int64_t)c * a.ld + 4 * q, v, min(4, a.D - 4 * q), a.mode);
            *reinterpret_cast<f32x4*>(cen + (size_t)j * dq + 4 * q) = f32x4{v[0], v[1], v[2], v[3]};
        }
    }
    __syncthreads();
    {
        float n[NC + 1];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            n[j] = 0.f;
            if (j < nc) {
#pragma unroll
                for (int k = 0; k < NQ; ++k) {
                    const int q = tr + k * TPR;
                    if (q < nquad) {
                        const f32x4 cv = *reinterpret_cast<const f32x4*>(cen + (size_t)j * dq + 4 * q);
#pragma unroll
                        for (int e = 0; e < 4; ++e) n[j] = n[j] + cv[e] * cv[e];
                    }
                }
            }
        }
        n[NC] = 0.f;
        mom_row_sum<WPR, NC + 1>(n, red, wave);
        __syncthreads();                                          // (WPR == 1: every wave holds the same norms; one writes)
        if (tid < NC && tid < nc) {
            float nj = 0.f;
#pragma unroll
            for (int j = 0; j < NC; ++j) if (j == tid) nj = n[j];
            const int c = c_row[tid];
            bool ok = c >= 0 && vbnn_bits_finite(__float_as_uint(nj));
            if (ok && (!a.first || a.resume)) ok = !vbnn_bits_nan(__float_as_uint(a.min_dist[c]));     // a NaN stays one: no race with its owner
            if (!ok) c_row[tid] = -1;
        }
        __syncthreads();
    }
    const float inf = __uint_as_float(0x7f800000u), qnan = __uint_as_float(0x7fc00000u);
    unsigned long long mine = 0ull;
    uint32_t n_cand = 0u, n_void = 0u, n_excl = 0u;
    const int64_t groups = (a.R + RPB - 1) / RPB;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t r = g * RPB + (RPB > 1 ? wave : 0);
        const bool live = r < a.R;                                // wave-uniform; block-uniform when the workgroup shares a row
        float f[NQ][4];
        float m_old = inf, w = 1.f;
        uint32_t fl = 0u, ex = 0u;
        if (live) {
            const float* row = a.feat + r * a.ld;
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                const int q = tr + k * TPR;
                if (q < nquad) kc_load4(row + 4 * q, f[k], min(4, a.D - 4 * q), a.mode);
                else f[k][0] = f[k][1] = f[k][2] = f[k][3] = 0.f;
            }
            if (!a.first || a.resume) m_old = a.min_dist[r];
            if (a.weight) w = a.weight[r];
            if (!a.first) fl = a.flag[r];
            else if (a.exclude) ex = a.exclude[r];
        } else {
#pragma unroll
            for (int k = 0; k < NQ; ++k) f[k][0] = f[k][1] = f[k][2] = f[k][3] = 0.f;
        }
        float d[NC + 1];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            d[j] = 0.f;
            if (j < nc) {
#pragma unroll
                for (int k = 0; k < NQ; ++k) {
                    const int q = tr + k * TPR;
                    if (q < nquad) {
                        const f32x4 cv = *reinterpret_cast<const f32x4*>(cen + (size_t)j * dq + 4 * q);
#pragma unroll
                        for (int e = 0; e < 4; ++e) { const float t = f[k][e] - cv[e]; d[j] = d[j] + t * t; }
                    }
                }
            }
        }
        d[NC] = 0.f;
        if (a.first && !a.resume) {
#pragma unroll
            for (int k = 0; k < NQ; ++k)
#pragma unroll
                for (int e = 0; e < 4; ++e) d[NC] = d[NC] + f[k][e] * f[k][e];
        }
        mom_row_sum<WPR, NC + 1>(d, red, wave);
        if (!live) continue;
        // the row's own arithmetic, the same in every thread of the row; thread 0 of the row writes
        const bool is_void = (a.first && !a.resume) ? !vbnn_bits_finite(__float_as_uint(d[NC])) : vbnn_bits_nan(__float_as_uint(m_old));
        float m = is_void ? qnan : m_old;
        bool picked = false;
        if (!is_void) {
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                if (j < nc) {
                    const int c = c_row[j];
                    if (c >= 0) {
                        if (d[j] < m) m = d[j];
                        if (a.prev && (int64_t)c == r) picked = true;
                    }
                }
            }
        }
        if (a.first) {
            const bool w_void = a.weight && (vbnn_bits_nan(__float_as_uint(w)) || w < 0.f);
            fl = (ex || is_void || w_void) ? 1u : 0u;
            if (tr == 0) {
                if (ex) n_excl += 1u; else if (is_void || w_void) n_void += 1u; else n_cand += 1u;
            }
        }
        if (picked) fl = 1u;
        if (tr == 0) {
            if (picked && a.dist_out) *a.dist_out = m_old;
            if (a.first || __float_as_uint(m) != __float_as_uint(m_old)) a.min_dist[r] = m;
            if (a.first || picked) a.flag[r] = (uint8_t)fl;
            if (a.best && !fl) {
                float key;
                if (m == inf) key = a.weight ? w : inf;
                else key = a.weight ? m * w : m;
                if (vbnn_bits_nan(__float_as_uint(key))) key = 0.f;        // 0 * inf
                const unsigned long long p = ((unsigned long long)vbnn_order_word(__float_as_uint(key)) << 32) | (unsigned long long)~(uint32_t)r;
                if (p > mine) mine = p;
            }
        }
    }
    if ((tid & 63) == 0) wg_best[wave] = mine;
    if (a.first && tr == 0) {
        if (n_cand) atomicAdd(&wg_cnt[0], n_cand);
        if (n_void) atomicAdd(&wg_cnt[1], n_void);
        if (n_excl) atomicAdd(&wg_cnt[2], n_excl);
    }
    __syncthreads();
    if (tid == 0 && a.best) {
        unsigned long long b = wg_best[0];
#pragma unroll
        for (int i = 1; i < KC_THREADS / 64; ++i) b = wg_best[i] > b ? wg_best[i] : b;
        if (b) atomicMax(a.best, b);
    }
    if (a.first && tid < 3 && wg_cnt[tid]) atomicAdd(&a.cnt[tid], wg_cnt[tid]);
}

// one workgroup: index / key of every step, the tail past the last pick, the counts, the centres that were out of range
__global__ __launch_bounds__(KC_THREADS) void k_kc_finish(const unsigned long long* __restrict__ best, int32_t k, int64_t R,
                                                          const int32_t* __restrict__ centres, int32_t n_centres,
                                                          const uint32_t* __restrict__ cnt, int32_t* __restrict__ index,
                                                          uint32_t* __restrict__ key, uint32_t* __restrict__ dist,
                                                          int64_t* __restrict__ counts, int64_t* __restrict__ ignored) {
    __shared__ uint32_t n_sel, n_bad;
    if (threadIdx.x == 0) { n_sel = 0u; n_bad = 0u; }
    __syncthreads();
    uint32_t sel = 0u, bad = 0u;
    for (int j = threadIdx.x; j < k; j += KC_THREADS) {
        const unsigned long long b = best[j];
        if (b) {
            index[j] = (int32_t)~(uint32_t)b;
            if (key) key[j] = vbnn_unorder_word((uint32_t)(b >> 32));
            sel += 1u;
        } else {
            index[j] = -1;
            if (key) key[j] = 0x7fc00000u;
            if (dist) dist[j] = 0x7fc00000u;
        }
    }
    for (int i = threadIdx.x; i < n_centres; i += KC_THREADS) {
        const int c = centres[i];
        bad += (c < 0 || (int64_t)c >= R) ? 1u : 0u;
    }
    if (sel) atomicAdd(&n_sel, sel);
    if (bad) atomicAdd(&n_bad, bad);
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[0] = (int64_t)n_sel;
        counts[1] = (int64_t)cnt[0];
        counts[2] = (int64_t)cnt[1];
        counts[3] = (int64_t)cnt[2];
        *ignored = (int64_t)n_bad;
    }
}

// ---------------------------------------------------------------------------------- the entry points
static int kc_shape(int64_t R, int64_t D, int32_t k) {
    VBNN_REQUIRE(R >= 1 && R < ((int64_t)1 << 31), "R (1 .. 2^31 - 1)");
    VBNN_REQUIRE(D >= 1 && D <= VBNN_KCENTRE_MAX_D, "D (1 .. VBNN_KCENTRE_MAX_D)");
    VBNN_REQUIRE(k >= 1 && k <= VBNN_KCENTRE_MAX_K, "k (1 .. VBNN_KCENTRE_MAX_K)");
    return VBNN_OK;
}

extern "C" int vbnn_kcentre_workspace_bytes(int64_t R, int64_t D, int32_t k, size_t* bytes) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(bytes, "null argument");
    if (int st = kc_shape(R, D, k)) return st;
    *bytes = kc_ws_bytes(R);
    return VBNN_OK;
    VBNN_API_END
}

template <int TPR, int NQ, int NC>
static int kc_launch(const vbnn_ctx* ctx, const KcPass& p, int nb) {
    auto kern = k_kc_pass<TPR, NQ, NC>;
    const size_t lds = (size_t)std::min(NC, kc_block(p.D)) * kc_dq(p.D) * sizeof(float);
    if (NC > 1) {                                                 // up to 128 KiB, beyond what a launch may ask for unasked: opt in, once per device
        static vbnn_per_device_flag configured;
        if (!configured[ctx->device]) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               KC_BLOCK_FLOATS * (int)sizeof(float));
            if (e != hipSuccess) { vbnn_set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return VBNN_ERR_HIP; }
            configured[ctx->device] = true;
        }
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(KC_THREADS), lds, ctx->stream, p);
    return VBNN_OK;
}
// an initial block (NC = KC_MAX_BLOCK, of which kc_block(D) are used) or a step launch (NC = 1), by the row width alone
static int kc_pass(const vbnn_ctx* ctx, const KcPass& p, bool block, int nb_wave, int nb_wg) {
    if (p.D <= 256) return block ? kc_launch<64, 1, KC_MAX_BLOCK>(ctx, p, nb_wave) : kc_launch<64, 1, 1>(ctx, p, nb_wave);
    if (p.D <= KC_WAVE_MAX_D) return block ? kc_launch<64, 4, KC_MAX_BLOCK>(ctx, p, nb_wave) : kc_launch<64, 4, 1>(ctx, p, nb_wave);
    if (p.D <= 2048) return block ? kc_launch<256, 2, KC_MAX_BLOCK>(ctx, p, nb_wg) : kc_launch<256, 2, 1>(ctx, p, nb_wg);
    return block ? kc_launch<256, KC_MAX_NQ, KC_MAX_BLOCK>(ctx, p, nb_wg) : kc_launch<256, KC_MAX_NQ, 1>(ctx, p, nb_wg);
}

extern "C" int vbnn_kcentre(vbnn_ctx* ctx, const vbnn_kcentre_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a, "null argument");
    if (int st = kc_shape(a->R, a->D, a->k)) return st;
    VBNN_REQUIRE(a->ld >= a->D, "ld (>= D)");
    VBNN_REQUIRE(a->n_centres >= 0 && (a->n_centres == 0 || a->centres), "centres (n_centres >= 0; NULL only with n_centres = 0)");
    VBNN_REQUIRE(a->resume == 0 || a->resume == 1, "resume (0 or 1)");
    VBNN_REQUIRE(a->feat && a->index && a->min_dist && a->counts && a->workspace, "null feat, index, min_dist, counts or workspace");
    VBNN_REQUIRE(((uintptr_t)a->feat & 3u) == 0 && ((uintptr_t)a->weight & 3u) == 0 && ((uintptr_t)a->centres & 3u) == 0 &&
                 ((uintptr_t)a->index & 3u) == 0 && ((uintptr_t)a->key & 3u) == 0 && ((uintptr_t)a->dist & 3u) == 0 &&
                 ((uintptr_t)a->min_dist & 3u) == 0 && ((uintptr_t)a->counts & 7u) == 0, "alignment (4 bytes; counts 8)");
    VBNN_REQUIRE(a->workspace_bytes >= kc_ws_bytes(a->R) && ((uintptr_t)a->workspace & 7u) == 0, "workspace (size; 8-byte aligned)");

    vbnn_cu_scope scope(ctx);
    const int64_t cap = (int64_t)std::max(vbnn_cu_count(), 1) * 8;
    const int nb_wave = (int)std::min<int64_t>((a->R + 3) / 4, cap), nb_wg = (int)std::min<int64_t>(a->R, cap);
    char* ws = (char*)a->workspace;
    unsigned long long* best = reinterpret_cast<unsigned long long*>(ws + KC_OFF_BEST);
    VBNN_CHECK_HIP(hipMemsetAsync(ws, 0, KC_OFF_BEST + 8 * (size_t)(a->k + 1), ctx->stream));

    KcPass p;
    p.feat = a->feat; p.ld = a->ld; p.R = a->R; p.D = (int32_t)a->D;
    p.mode = (vbnn_al16(a->feat) && a->ld % 4 == 0) ? 2 : ((((uintptr_t)a->feat & 7u) == 0 && a->ld % 2 == 0) ? 1 : 0);
    p.weight = a->weight; p.exclude = a->exclude;
    p.min_dist = a->min_dist; p.flag = reinterpret_cast<uint8_t*>(ws + KC_OFF_FLAG);
    p.cnt = reinterpret_cast<uint32_t*>(ws + KC_OFF_CNT);
    p.resume = a->resume;
    p.first = 1;
    // the initial centres, a block per pass
    const int blk = kc_block(a->D);
    for (int32_t c0 = 0; c0 < a->n_centres; c0 += blk) {
        p.centres = a->centres + c0; p.nc = std::min<int32_t>(blk, a->n_centres - c0);
        p.prev = nullptr; p.best = nullptr; p.dist_out = nullptr;
        if (int st = kc_pass(ctx, p, true, nb_wave, nb_wg)) return st;
        p.first = 0;
    }
    // launch j picks step j (j < k) after applying the pick of step j - 1 (j > 0)
    p.centres = nullptr; p.nc = 0;
    for (int32_t j = 0; j <= a->k; ++j) {
        p.prev = j > 0 ? best + (j - 1) : nullptr;
        p.best = j < a->k ? best + j : nullptr;
        p.dist_out = (j > 0 && a->dist) ? a->dist + (j - 1) : nullptr;
        if (int st = kc_pass(ctx, p, false, nb_wave, nb_wg)) return st;
        p.first = 0;
    }
    hipLaunchKernelGGL(k_kc_finish, dim3(1), dim3(KC_THREADS), 0, ctx->stream, best, a->k, a->R, a->centres, a->n_centres,
                       p.cnt, a->index, reinterpret_cast<uint32_t*>(a->key), reinterpret_cast<uint32_t*>(a->dist), a->counts,
                       reinterpret_cast<int64_t*>(ws));
    return vbnn_check_launch("vbnn_kcentre");
    VBNN_API_END
}
