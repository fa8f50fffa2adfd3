// acquire.hip -- vbnn_top_rows: the exact top-k of R fp32 scores WITH their row indices (pool acquisition for active
// learning), deterministic or by Gumbel top-k in its exponential-race form. The contract is include/vbnn_hip.h's; this file
// is its shape. Many workgroups, integer atomics only, no allocation, no host synchronisation; compiled without fp
// contraction (Makefile) so that the stochastic key is vbnn_philox.h evaluated as written.
//
// Shape (device_prims.h's radix select, taken one step further to the rows themselves):
//   1. the three digit passes of that plan over the ORDER WORD of every candidate, each followed by a one-workgroup pick
//      that hands prefix and rank on in device words.
//      They end with T (the order word of the k-th candidate), the size of its tie and `need`, the tied rows wanted.
//   2. when the tie has to be split (more rows equal T than are needed) one count pass writes each workgroup's number of
//      tied rows; otherwise that launch returns at once. Workgroups own CONTIGUOUS row ranges, so a prefix over those
//      counts is a prefix in index order.
//   3. one take pass copies (order word, row) of every row before T and of the `need` tied rows with the lowest indices to
//      the candidate list. Which slot a row lands in depends on the arrival order; WHICH rows land does not, and
//   4. a one-workgroup bitonic sort of the <= 4096 (order word, row) pairs in LDS fixes the order, then writes the outputs.
// Deterministic: the order word is re-formed from score / exclude in every pass:
// nothing per row is kept and a pass reads 4 B (+ 1 B of exclude) per row -- what reading a stored key would cost, without
// the pass that stores it. Stochastic: a key is one Philox block per four rows and three vbnn_det_logf per row, about 50 us
// of arithmetic a pass at R = 10^7 against 8 us of bytes, so the FIRST pass stores the keys (4 B per row of workspace) and
// the later passes walk over them as over scores; a row whose score is a NaN keeps a NaN key there.
#include "device_prims.h"

typedef uint32_t acq_u32x4 __attribute__((ext_vector_type(4)));

constexpr int ACQ_BINS = 2048;
constexpr int ACQ_PASSES = 3;
constexpr int ACQ_THREADS = 1024;                  // the streaming kernels: 16 waves share one LDS histogram and one flush
constexpr int ACQ_MAX_WG = 1024;                   // a cap only (the tie counts' array): the grid is one workgroup per compute
                                                   // unit of the context (vbnn_cu_count: 256 on an MI355X) -- the registers of a
                                                   // 1024-thread workgroup allow no second one on a unit
constexpr int ACQ_TILE = 4 * ACQ_THREADS;          // rows per workgroup step: four rows a thread (one 16-byte load)
constexpr int ACQ_AHEAD = 4;                       // steps whose loads are issued before the first is used
constexpr int ACQ_MAX_K = VBNN_TOP_ROWS_MAX_K;
// workspace words: histograms | state | per-workgroup tie counts | candidate order words | candidate rows | R stochastic keys
constexpr size_t ACQ_OFF_STATE = (size_t)ACQ_PASSES * ACQ_BINS;
constexpr size_t ACQ_OFF_TIES = ACQ_OFF_STATE + 16;
constexpr size_t ACQ_OFF_OK = ACQ_OFF_TIES + ACQ_MAX_WG;
constexpr size_t ACQ_OFF_IDX = ACQ_OFF_OK + ACQ_MAX_K;
constexpr size_t ACQ_OFF_KEYS = ACQ_OFF_IDX + ACQ_MAX_K;      // (a multiple of 4 words: 16-byte stores when the workspace is aligned)
static_assert(ACQ_OFF_KEYS % 4 == 0, "the stored keys start on a 16-byte boundary of the workspace");
static inline size_t acq_ws_words(int64_t R) { return ACQ_OFF_KEYS + (size_t)R; }
// state words
enum { ST_PREFIX = 0, ST_REM = 1, ST_KEFF = 3, ST_NEED = 4, ST_TIED = 5, ST_SLOTS = 6, ST_CAND = 7, ST_NAN = 8,
       ST_EXCL = 9 };
// what a row is
enum { ROW_CANDIDATE = 0, ROW_NAN = 1, ROW_EXCLUDED = 2, ROW_NONE = 3 };

struct AcqSrc {
    const uint32_t* score;      // the scores' bits, or NULL
    const uint8_t* exclude;
    int64_t R;
    int64_t chunk;              // rows per workgroup (a multiple of ACQ_TILE)
    int32_t largest, stochastic, vec;
    float beta;
    uint32_t k0, k1, draw;
    uint64_t row0;
};

// the stochastic key of the header, op for op: x the row's Philox word, sb the score's bits (not a NaN)
__device__ __forceinline__ float acq_race_key(uint32_t x, uint32_t sb, bool has_score, float beta) {
    uint32_t t = (x >> 8) + 1u;
    if (t > 0x00ffffffu) t = 0x00ffffffu;
    const float u = (float)t * 5.96046448e-8f;                  // * 2^-24, exact
    const float E = -vbnn_det_logf(u);
    float L = 0.0f;
    if (has_score) {
        if (sb >= 0x00800000u && sb <= 0x7f7fffffu) L = vbnn_det_logf(__uint_as_float(sb));
        else if (sb == 0x7f800000u) L = __uint_as_float(0x7f800000u);
        else L = __uint_as_float(0xff800000u);
    }
    return fmaf(beta, L, -vbnn_det_logf(E));
}

// Rows r .. r + 3 (r a multiple of 4) of a workgroup's range, which ends at `end` (<= R): first the loads alone, so that a
// loop can issue several steps' loads before it uses the first ...
struct AcqRaw { uint32_t sb[4]; uint32_t ex; };
__device__ __forceinline__ AcqRaw acq_fetch(const AcqSrc& s, int64_t r, int64_t end) {
    AcqRaw w;
#pragma unroll
    for (int j = 0; j < 4; ++j) w.sb[j] = 0u;
    w.ex = 0u;
    if (r >= end) return w;
    if (s.vec && r + 3 < end) {
        if (s.score) {
            const acq_u32x4 v = reinterpret_cast<const acq_u32x4*>(s.score)[r >> 2];
#pragma unroll
            for (int j = 0; j < 4; ++j) w.sb[j] = v[j];
        }
        if (s.exclude) w.ex = reinterpret_cast<const uint32_t*>(s.exclude)[r >> 2];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (r + j < end) {
                if (s.score) w.sb[j] = s.score[r + j];
                if (s.exclude) w.ex |= (uint32_t)s.exclude[r + j] << (8 * j);
            }
        }
    }
    return w;
}
// ... then what each row is, and the order word of the candidates -- the k rows wanted are always the k SMALLEST order
// words (largest: the map's complement).
__device__ __forceinline__ void acq_classify(const AcqSrc& s, int64_t r, int64_t end, const AcqRaw& w, uint32_t ok[4],
                                             uint32_t what[4]) {
    vbnn_u32x4 blk;
    uint32_t q = 0xffffffffu;                                    // no global row has this quad: row0 + R <= 2^32
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (r + j >= end) { ok[j] = 0u; what[j] = ROW_NONE; continue; }
        const uint32_t sb = w.sb[j];
        const bool nan = s.score && vbnn_bits_nan(sb);
        what[j] = ((w.ex >> (8 * j)) & 0xffu) ? ROW_EXCLUDED : (nan ? ROW_NAN : ROW_CANDIDATE);
        uint32_t kb = sb;
        if (s.stochastic) {
            const uint64_t g = s.row0 + (uint64_t)(r + j);
            if ((uint32_t)(g >> 2) != q) {
                q = (uint32_t)(g >> 2);
                blk = vbnn_philox4x32_10(q, 0u, s.draw, VBNN_STREAM_ACQUIRE, s.k0, s.k1);
            }
            const uint32_t wd = (uint32_t)g & 3u;
            const uint32_t x = wd == 0u ? blk.v[0] : (wd == 1u ? blk.v[1] : (wd == 2u ? blk.v[2] : blk.v[3]));
            kb = __float_as_uint(acq_race_key(x, sb, s.score != nullptr, s.beta));
        }
        const uint32_t m = vbnn_order_word(kb);
        ok[j] = s.largest ? ~m : m;
    }
}
// The walk of a workgroup over its rows, ACQ_AHEAD steps at a time: `step(r, ok, what)` sees the steps in row order, the
// same steps in every thread (the take pass scans across the block inside it).
template <typename F>
__device__ __forceinline__ void acq_walk(const AcqSrc& s, F step) {
    const int64_t begin = (int64_t)blockIdx.x * s.chunk;
    const int64_t end = begin + s.chunk < s.R ? begin + s.chunk : s.R;
    for (int64_t base = begin; base < end; base += (int64_t)ACQ_AHEAD * ACQ_TILE) {
        AcqRaw w[ACQ_AHEAD];
#pragma unroll
        for (int u = 0; u < ACQ_AHEAD; ++u) w[u] = acq_fetch(s, base + (int64_t)u * ACQ_TILE + 4 * (int64_t)threadIdx.x, end);
#pragma unroll
        for (int u = 0; u < ACQ_AHEAD; ++u) {
            if (base + (int64_t)u * ACQ_TILE < end) {                // block-uniform
                const int64_t r = base + (int64_t)u * ACQ_TILE + 4 * (int64_t)threadIdx.x;
                uint32_t ok[4], what[4];
                acq_classify(s, r, end, w[u], ok, what);
                step(r, ok, what);
            }
        }
    }
}

// ---------------------------------------------------------------------------------- the digit passes
__global__ __launch_bounds__(ACQ_THREADS) void k_acq_hist(AcqSrc s, RadixPass ps, int first, const uint32_t* state,
                                                          uint32_t* __restrict__ ghist, uint32_t* counts_out,
                                                          uint32_t* __restrict__ keys_out) {
    __shared__ uint32_t hist[ACQ_BINS];
    __shared__ uint32_t kinds[4];
    for (int i = threadIdx.x; i < ACQ_BINS; i += ACQ_THREADS) hist[i] = 0u;
    if (threadIdx.x < 4) kinds[threadIdx.x] = 0u;
    const uint32_t prefix = ps.prefix_mask ? state[ST_PREFIX] : 0u;
    __syncthreads();
    uint32_t n_cand = 0u, n_nan = 0u, n_excl = 0u;
    const bool vec_out = vbnn_al16(keys_out);
    acq_walk(s, [&](int64_t r, const uint32_t ok[4], const uint32_t what[4]) {
        if (keys_out) {                                            // the stochastic key, formed ONCE: the later passes read it as a score
            acq_u32x4 kb;                                          // (a NaN score's row keeps a NaN there: no candidate later either)
#pragma unroll
            for (int j = 0; j < 4; ++j) kb[j] = what[j] == ROW_NAN ? 0x7fc00000u : vbnn_unorder_word(~ok[j]);
            if (vec_out && what[3] != ROW_NONE) {
                reinterpret_cast<acq_u32x4*>(keys_out)[r >> 2] = kb;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (what[j] != ROW_NONE) keys_out[r + j] = kb[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (what[j] == ROW_CANDIDATE && (ok[j] & ps.prefix_mask) == prefix)
                atomicAdd(&hist[(ok[j] >> ps.shift) & ((1u << ps.bits) - 1u)], 1u);
            n_cand += what[j] == ROW_CANDIDATE ? 1u : 0u;
            n_nan += what[j] == ROW_NAN ? 1u : 0u;
            n_excl += what[j] == ROW_EXCLUDED ? 1u : 0u;
        }
    });
    if (first) {
        if (n_cand) atomicAdd(&kinds[0], n_cand);
        if (n_nan) atomicAdd(&kinds[1], n_nan);
        if (n_excl) atomicAdd(&kinds[2], n_excl);
    }
    __syncthreads();
    radix_flush<ACQ_THREADS>(hist, ghist, ps.bits);
    if (first && threadIdx.x < 3 && kinds[threadIdx.x]) atomicAdd(&counts_out[threadIdx.x], kinds[threadIdx.x]);
}

// one workgroup: the bin of digit `ps` that holds the rem-th smallest of the rows matching the prefix (rem is 1-based;
// pass 0: min(k, candidates)). Writes the longer prefix and the rank inside the bin; the last pass
// leaves T = state[ST_PREFIX], need = state[ST_NEED] and the size of T's tie in state[ST_TIED].
__global__ __launch_bounds__(256) void k_acq_pick(const uint32_t* __restrict__ ghist, RadixPass ps, int first, uint32_t k,
                                                  uint32_t* state) {
    __shared__ uint32_t part[256];
    const uint32_t n_cand = state[ST_CAND];
    const uint32_t rem = first ? (k < n_cand ? k : n_cand) : state[ST_REM];
    const uint32_t prefix = first ? 0u : state[ST_PREFIX];
    if (first && threadIdx.x == 0) state[ST_KEFF] = rem;
    if (rem == 0u) return;                                         // no candidate at all: the take pass does nothing
    uint32_t bin, r, tied;
    if (radix_pick(ghist, ps, rem - 1u, part, bin, r, tied)) {     // exactly one thread: the bins hold at least rem rows
        state[ST_PREFIX] = prefix | (bin << ps.shift);
        state[ST_REM] = r + 1u;
        if (ps.shift == 0) { state[ST_NEED] = r + 1u; state[ST_TIED] = tied; }
    }
}

// ---------------------------------------------------------------------------------- the tie counts
__global__ __launch_bounds__(ACQ_THREADS) void k_acq_ties(AcqSrc s, const uint32_t* __restrict__ state,
                                                          uint32_t* __restrict__ wg_ties) {
    if (state[ST_KEFF] == 0u || state[ST_TIED] == state[ST_NEED]) return;     // every tied row is taken: nothing to split
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0u;
    __syncthreads();
    const uint32_t T = state[ST_PREFIX];
    uint32_t n = 0u;
    acq_walk(s, [&](int64_t, const uint32_t ok[4], const uint32_t what[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) n += (what[j] == ROW_CANDIDATE && ok[j] == T) ? 1u : 0u;
    });
    if (n) atomicAdd(&total, n);
    __syncthreads();
    if (threadIdx.x == 0) wg_ties[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------------- the take pass
// exclusive prefix of v over the threads of the block in thread order, and the block's total
__device__ __forceinline__ uint32_t acq_block_scan(uint32_t v, uint32_t* sh /* ACQ_THREADS / 64 words */, uint32_t* total) {
    const uint32_t inc = vbnn_wave_scan_incl(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                              // the previous step's readers of sh are done
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    uint32_t wave_base = 0u, all = 0u;
#pragma unroll
    for (int i = 0; i < ACQ_THREADS / 64; ++i) {
        const uint32_t c = sh[i];
        wave_base += (i < wave) ? c : 0u;
        all += c;
    }
    *total = all;
    return wave_base + inc - v;
}

// The rows a workgroup takes are listed in LDS first and get their place in the candidate list with ONE global add (k adds
// to one word from every CU took longer than the pass itself).
__global__ __launch_bounds__(ACQ_THREADS) void k_acq_take(AcqSrc s, int n_wg, uint32_t* state, const uint32_t* __restrict__ wg_ties,
                                                          uint32_t* __restrict__ cand_ok, uint32_t* __restrict__ cand_idx) {
    __shared__ uint32_t sh[ACQ_THREADS / 64];
    __shared__ uint32_t l_ok[ACQ_MAX_K], l_idx[ACQ_MAX_K];
    __shared__ uint32_t ties_before, l_n, l_base;
    if (state[ST_KEFF] == 0u) return;
    const uint32_t T = state[ST_PREFIX], need = state[ST_NEED];
    const bool all_ties = state[ST_TIED] == need;
    if (threadIdx.x == 0) { ties_before = 0u; l_n = 0u; }
    __syncthreads();
    if (!all_ties && (int)threadIdx.x < (int)blockIdx.x && (int)threadIdx.x < n_wg) {     // (n_wg <= ACQ_MAX_WG <= ACQ_THREADS)
        const uint32_t c = wg_ties[threadIdx.x];
        if (c) atomicAdd(&ties_before, c);                         // integers: any order gives this sum
    }
    __syncthreads();
    uint32_t tie_base = ties_before;                               // tied rows in the workgroups before this one
    acq_walk(s, [&](int64_t r, const uint32_t ok[4], const uint32_t what[4]) {
        bool take[4], tied[4];
        uint32_t n_tied = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            tied[j] = what[j] == ROW_CANDIDATE && ok[j] == T;
            take[j] = what[j] == ROW_CANDIDATE && (ok[j] < T || (tied[j] && all_ties));
            n_tied += tied[j] ? 1u : 0u;
        }
        if (!all_ties && tie_base < need) {                        // block-uniform: this workgroup may still own wanted ties
            uint32_t total;
            uint32_t rank = tie_base + acq_block_scan(n_tied, sh, &total);   // tied rows with a lower index
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (tied[j]) { take[j] = rank < need; rank += 1u; }
            }
            tie_base += total;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (take[j]) {
                const uint32_t slot = atomicAdd(&l_n, 1u);
                if (slot < (uint32_t)ACQ_MAX_K) { l_ok[slot] = ok[j]; l_idx[slot] = (uint32_t)(r + j); }
            }
        }
    });
    __syncthreads();
    const uint32_t n = l_n < (uint32_t)ACQ_MAX_K ? l_n : (uint32_t)ACQ_MAX_K;
    if (n == 0u) return;
    if (threadIdx.x == 0) l_base = atomicAdd(&state[ST_SLOTS], n);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += ACQ_THREADS) {
        const uint32_t slot = l_base + i;
        if (slot < (uint32_t)ACQ_MAX_K) { cand_ok[slot] = l_ok[i]; cand_idx[slot] = l_idx[i]; }
    }
}

// ---------------------------------------------------------------------------------- the sort and the outputs
constexpr int ACQ_SORT_THREADS = 1024;             // one workgroup of 16 waves: two pairs a thread and step at k = 4096
__global__ __launch_bounds__(ACQ_SORT_THREADS) void k_acq_sort(AcqSrc s, int32_t k, const uint32_t* __restrict__ state,
                                                  const uint32_t* __restrict__ cand_ok, const uint32_t* __restrict__ cand_idx,
                                                  int32_t* __restrict__ index, uint32_t* __restrict__ value,
                                                  uint32_t* __restrict__ key, int64_t* __restrict__ counts) {
    __shared__ uint64_t e[ACQ_MAX_K];
    uint32_t n = state[ST_KEFF];                                   // == the rows the take pass listed
    if (n > (uint32_t)k) n = (uint32_t)k;
    if (n > state[ST_SLOTS]) n = state[ST_SLOTS];
    uint32_t P = 2u;
    while (P < n) P <<= 1;
    for (uint32_t i = threadIdx.x; i < P; i += ACQ_SORT_THREADS)
        e[i] = i < n ? (((uint64_t)cand_ok[i] << 32) | (uint64_t)cand_idx[i]) : ~(uint64_t)0;
    __syncthreads();
    for (uint32_t size = 2u; size <= P; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0u; stride >>= 1) {
            for (uint32_t t = threadIdx.x; t < (P >> 1); t += ACQ_SORT_THREADS) {
                const uint32_t lo = 2u * t - (t & (stride - 1u));  // the pair (lo, lo + stride)
                const uint32_t hi = lo + stride;
                const bool up = (lo & size) == 0u;
                const uint64_t a = e[lo], b = e[hi];
                if ((a > b) == up) { e[lo] = b; e[hi] = a; }
            }
            __syncthreads();
        }
    }
    for (uint32_t j = threadIdx.x; j < (uint32_t)k; j += ACQ_SORT_THREADS) {
        if (j < n) {
            const uint32_t ok = (uint32_t)(e[j] >> 32), row = (uint32_t)e[j];
            index[j] = (int32_t)row;
            value[j] = s.score ? s.score[(int64_t)row < s.R ? row : 0u] : 0x3f800000u;       // no scores: the weight every candidate has, 1
            if (key) key[j] = vbnn_unorder_word(s.largest ? ~ok : ok);
        } else {
            index[j] = -1;
            value[j] = 0x7fc00000u;
            if (key) key[j] = 0x7fc00000u;
        }
    }
    if (threadIdx.x == 0) {
        counts[0] = (int64_t)n;
        counts[1] = (int64_t)state[ST_CAND];
        counts[2] = (int64_t)state[ST_NAN];
        counts[3] = (int64_t)state[ST_EXCL];
    }
}

// ---------------------------------------------------------------------------------- the entry points
static int acq_shape(int64_t R, int32_t k) {
    VBNN_REQUIRE(R >= 1 && R < ((int64_t)1 << 31), "R (1 .. 2^31 - 1)");
    VBNN_REQUIRE(k >= 1 && k <= VBNN_TOP_ROWS_MAX_K, "k (1 .. VBNN_TOP_ROWS_MAX_K)");
    return VBNN_OK;
}

extern "C" int vbnn_top_rows_workspace_bytes(int64_t R, int32_t k, size_t* bytes) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(bytes, "null argument");
    if (int st = acq_shape(R, k)) return st;
    *bytes = acq_ws_words(R) * sizeof(uint32_t);
    return VBNN_OK;
    VBNN_API_END
}

extern "C" int vbnn_top_rows(vbnn_ctx* ctx, const vbnn_top_rows_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a, "null argument");
    if (int st = acq_shape(a->R, a->k)) return st;
    VBNN_REQUIRE(a->index && a->value && a->counts && a->workspace, "null output or workspace");
    VBNN_REQUIRE(a->largest == 0 || a->largest == 1, "largest (0 or 1)");
    VBNN_REQUIRE(a->stochastic == 0 || a->stochastic == 1, "stochastic (0 or 1)");
    if (a->stochastic) {
        VBNN_REQUIRE(a->largest == 1, "a stochastic selection takes the largest keys (largest = 1)");
        VBNN_REQUIRE(a->beta > 0.0f && a->beta <= 3.402823466e38f, "beta (> 0, finite)");
        VBNN_REQUIRE(a->row0 >= 0 && a->row0 + a->R <= ((int64_t)1 << 32), "row0 (row0 + R <= 2^32)");
    } else {
        VBNN_REQUIRE(a->score, "score (NULL only with stochastic = 1)");
    }
    VBNN_REQUIRE(((uintptr_t)a->score & 3u) == 0 && ((uintptr_t)a->index & 3u) == 0 && ((uintptr_t)a->value & 3u) == 0 &&
                 ((uintptr_t)a->key & 3u) == 0 && ((uintptr_t)a->counts & 7u) == 0, "alignment (4 bytes; counts 8)");
    VBNN_REQUIRE(a->workspace_bytes >= acq_ws_words(a->R) * sizeof(uint32_t) && ((uintptr_t)a->workspace & 3u) == 0, "workspace");

    AcqSrc s;
    s.score = reinterpret_cast<const uint32_t*>(a->score);
    s.exclude = a->exclude;
    s.R = a->R;
    vbnn_cu_scope scope(ctx);
    const int64_t max_wg = std::min<int64_t>(std::max(vbnn_cu_count(), 1), ACQ_MAX_WG);
    int64_t n_wg = (a->R + 4 * ACQ_TILE - 1) / (4 * ACQ_TILE);    // >= 16 rows per thread before another histogram flush
    if (n_wg > max_wg) n_wg = max_wg;
    s.chunk = ((a->R + n_wg - 1) / n_wg + ACQ_TILE - 1) / ACQ_TILE * ACQ_TILE;
    n_wg = (a->R + s.chunk - 1) / s.chunk;
    s.largest = a->largest;
    s.stochastic = a->stochastic;
    s.vec = (vbnn_al16(a->score) && ((uintptr_t)a->exclude & 3u) == 0) ? 1 : 0;
    s.beta = a->beta;
    s.k0 = (uint32_t)a->seed;
    s.k1 = (uint32_t)(a->seed >> 32);
    s.draw = a->draw;
    s.row0 = a->stochastic ? (uint64_t)a->row0 : 0u;

    uint32_t* ws = (uint32_t*)a->workspace;
    uint32_t* state = ws + ACQ_OFF_STATE;
    // a stochastic key costs a Philox block per four rows and three logarithms: the first pass stores it, the others read it
    uint32_t* keys = a->stochastic ? ws + ACQ_OFF_KEYS : nullptr;
    AcqSrc later = s;                                              // what the passes after the first walk over
    if (keys) {
        later.score = keys;
        later.stochastic = 0;
        later.vec = (vbnn_al16(keys) && ((uintptr_t)a->exclude & 3u) == 0) ? 1 : 0;
    }
    VBNN_CHECK_HIP(hipMemsetAsync(ws, 0, ACQ_OFF_TIES * sizeof(uint32_t), ctx->stream));
    const dim3 grid((unsigned)n_wg), block(ACQ_THREADS);
    for (int p = 0; p < ACQ_PASSES; ++p) {
        const RadixPass ps = radix_pass(p);
        uint32_t* gh = ws + (size_t)p * ACQ_BINS;
        hipLaunchKernelGGL(k_acq_hist, grid, block, 0, ctx->stream, p == 0 ? s : later, ps, p == 0 ? 1 : 0, state, gh,
                           state + ST_CAND, p == 0 ? keys : nullptr);
        hipLaunchKernelGGL(k_acq_pick, dim3(1), dim3(256), 0, ctx->stream, gh, ps, p == 0 ? 1 : 0, (uint32_t)a->k, state);
    }
    hipLaunchKernelGGL(k_acq_ties, grid, block, 0, ctx->stream, later, state, ws + ACQ_OFF_TIES);
    hipLaunchKernelGGL(k_acq_take, grid, block, 0, ctx->stream, later, (int)n_wg, state, ws + ACQ_OFF_TIES, ws + ACQ_OFF_OK,
                       ws + ACQ_OFF_IDX);
    hipLaunchKernelGGL(k_acq_sort, dim3(1), dim3(ACQ_SORT_THREADS), 0, ctx->stream, s, a->k, state, ws + ACQ_OFF_OK,
                       ws + ACQ_OFF_IDX, a->index, reinterpret_cast<uint32_t*>(a->value), reinterpret_cast<uint32_t*>(a->key),
                       a->counts);
    return vbnn_check_launch("vbnn_top_rows");
    VBNN_API_END
}
