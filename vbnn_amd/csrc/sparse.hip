// sparse.hip -- the compressed form of a signal-to-noise pruning (CSR over output rows: vbnn_prune_compress) and one VB
// layer's forward on it (vbnn_forward_sparse). The dense pruned shadows of prune.hip stream every +0; at 2-10 % density no MFMA
// shape fits what is left, so the forward is a gather kernel: a wave per output unit, a lane per operand row, the row's
// entries broadcast from registers (v_readlane) and each entry one coalesced read of a K-major input line that stays in the
// XCD's L2. The epilogue is EpiFwd (epilogues.h), the dense forward's own. No atomics, no hand-off between workgroups; every
// sum has one fixed order. Compiled without fp contraction (Makefile): the key bits are prune.hip's.
#include "epilogues.h"
#include "device_prims.h"

// ---------------------------------------------------------------------------------- vbnn_prune_compress
static inline int sparse_row_grid(int64_t O) {
    int64_t b = (O + 3) / 4;                   // a wave per row, four rows per workgroup, grid-stride beyond 4096 workgroups
    if (b < 1) b = 1;
    if (b > 4096) b = 4096;
    return (int)b;
}

// kept = what k_prune_pack keeps: !(key < tau), so a NaN key (and everything under a NaN tau) is kept
__device__ __forceinline__ bool sparse_kept(float mean, float lvar, float tau) { return !(vbnn_snr_key(mean, lvar) < tau); }

// row_ptr[o + 1] = kept weights of row o (the scan turns the counts into offsets)
__global__ __launch_bounds__(256) void k_sparse_count(const float* __restrict__ means, const float* __restrict__ lvars, int64_t O, int64_t I,
                                                      const float* __restrict__ tau_dev, float tau_host, uint32_t* __restrict__ row_ptr) {
    const float tau = tau_dev ? tau_dev[0] : tau_host;
    const int lane = threadIdx.x & 63;
    for (int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); o < O; o += (int64_t)gridDim.x * 4) {
        const float* m = means + o * I;
        const float* l = lvars + o * I;
        uint32_t c = 0u;
        for (int64_t i = lane; i < I; i += 64) c += sparse_kept(m[i], l[i], tau) ? 1u : 0u;
        c = vbnn_wave_sum(c);
        if (lane == 0) row_ptr[o + 1] = c;
    }
}

struct SparseScanArgs { uint32_t* row_ptr[8]; int64_t O[8]; uint32_t* nnz_dev[8]; };
// block l: layer l's counts (row_ptr[1 .. O]) into inclusive sums in place, row_ptr[0] = 0, nnz_dev = row_ptr[O]. One workgroup:
// thread t owns a contiguous run of rows, the 256 run totals are added in thread order.
__global__ __launch_bounds__(256) void k_sparse_scan(SparseScanArgs a) {
    __shared__ uint32_t part[256];
    uint32_t* rp = a.row_ptr[blockIdx.x];
    const int64_t O = a.O[blockIdx.x];
    const int64_t per = (O + 255) / 256;
    const int64_t b = min((int64_t)threadIdx.x * per, O), e = min(b + per, O);
    uint32_t s = 0u;
    for (int64_t i = b; i < e; ++i) s += rp[i + 1];
    part[threadIdx.x] = s;
    __syncthreads();
    uint32_t run = 0u;
    for (int i = 0; i < (int)threadIdx.x; ++i) run += part[i];
    for (int64_t i = b; i < e; ++i) { run += rp[i + 1]; rp[i + 1] = run; }
    if (threadIdx.x == 0) rp[0] = 0u;
    if (threadIdx.x == 255 && a.nnz_dev[blockIdx.x]) a.nnz_dev[blockIdx.x][0] = run;      // (thread 255's run ends at row O, or is empty)
}

// a wave walks its row in column order, 64 columns a step: an entry's place is the row's offset + the kept weights before it
template <typename T, typename IDX>
__global__ __launch_bounds__(256) void k_sparse_fill(const float* __restrict__ means, const float* __restrict__ lvars, int64_t O, int64_t I,
                                                     const float* __restrict__ tau_dev, float tau_host,
                                                     const uint32_t* __restrict__ row_ptr, IDX* __restrict__ cols, T* __restrict__ mu_v,
                                                     T* __restrict__ var_v, int64_t cap) {
    const float tau = tau_dev ? tau_dev[0] : tau_host;
    const int lane = threadIdx.x & 63;
    for (int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); o < O; o += (int64_t)gridDim.x * 4) {
        const float* m = means + o * I;
        const float* l = lvars + o * I;
        int64_t base = row_ptr[o];
        for (int64_t i0 = 0; i0 < I; i0 += 64) {
            const int64_t i = i0 + lane;
            const bool in = i < I;
            const float mv = in ? m[i] : 0.f, lv = in ? l[i] : 0.f;
            const bool keep = in && sparse_kept(mv, lv, tau);
            const unsigned long long bal = __ballot(keep);
            const int64_t pos = base + __popcll(bal & ((1ull << lane) - 1ull));
            if (keep && pos < cap) {
                cols[pos] = (IDX)i;
                mu_v[pos] = Elt<T>::to(mv);
                if (var_v) var_v[pos] = Elt<T>::to(expf(lv));
            }
            base += __popcll(bal);
        }
    }
}

extern "C" int vbnn_prune_compress(vbnn_ctx* ctx, int dtype, int n_layers, const vbnn_prune_desc* layers, const vbnn_sparse_desc* sparse,
                                   const float* tau_dev, float tau_host) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && layers && sparse, "null argument");
    VBNN_REQUIRE(n_layers >= 1 && n_layers <= 8, "n_layers (1..8)");
    VBNN_REQUIRE(dtype == VBNN_F32 || dtype == VBNN_BF16, "dtype");
    int64_t Wt = 0;
    for (int l = 0; l < n_layers; ++l) {
        const vbnn_prune_desc& d = layers[l];
        const vbnn_sparse_desc& s = sparse[l];
        VBNN_REQUIRE(d.means && d.lvars && s.row_ptr && s.cols && s.mu_v, "null layer argument");
        VBNN_REQUIRE(d.O > 0 && d.I > 0 && s.O == d.O && s.I == d.I, "layer shape");
        VBNN_REQUIRE(s.nnz_cap >= 0, "nnz_cap");
        VBNN_REQUIRE(s.idx_bytes == 4 || (s.idx_bytes == 2 && d.I <= 65536), "idx_bytes (2: I <= 65536 only; 4)");
        Wt += d.O * d.I;
    }
    VBNN_REQUIRE(Wt < ((int64_t)1 << 32), "more than 2^32 - 1 weights");
    SparseScanArgs sa{};
    for (int l = 0; l < n_layers; ++l) {
        const vbnn_prune_desc& d = layers[l];
        hipLaunchKernelGGL(k_sparse_count, dim3(sparse_row_grid(d.O)), dim3(256), 0, ctx->stream, d.means, d.lvars, d.O, d.I, tau_dev, tau_host,
                           sparse[l].row_ptr);
        sa.row_ptr[l] = sparse[l].row_ptr; sa.O[l] = d.O; sa.nnz_dev[l] = sparse[l].nnz_dev;
    }
    hipLaunchKernelGGL(k_sparse_scan, dim3(n_layers), dim3(256), 0, ctx->stream, sa);
    for (int l = 0; l < n_layers; ++l) {
        const vbnn_prune_desc& d = layers[l];
        const vbnn_sparse_desc& s = sparse[l];
        const dim3 g(sparse_row_grid(d.O));
#define VBNN_SPARSE_FILL(T, IDX)                                                                                                  \
        hipLaunchKernelGGL((k_sparse_fill<T, IDX>), g, dim3(256), 0, ctx->stream, d.means, d.lvars, d.O, d.I, tau_dev, tau_host,  \
                           (const uint32_t*)s.row_ptr, (IDX*)s.cols, (T*)s.mu_v, (T*)s.var_v, s.nnz_cap)
        if (dtype == VBNN_F32) { if (s.idx_bytes == 2) VBNN_SPARSE_FILL(float, uint16_t); else VBNN_SPARSE_FILL(float, uint32_t); }
        else { if (s.idx_bytes == 2) VBNN_SPARSE_FILL(bf16_t, uint16_t); else VBNN_SPARSE_FILL(bf16_t, uint32_t); }
#undef VBNN_SPARSE_FILL
    }
    return vbnn_check_launch("vbnn_prune_compress");
    VBNN_API_END
}

// ---------------------------------------------------------------------------------- vbnn_forward_sparse
constexpr int SP_UNROLL = 8;        // gathers in flight per wave

__device__ __forceinline__ float sp_bcast(float v, int j) { return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), j)); }

// Workgroup = four waves = the four output units of one Philox block; blockIdx.y = a tile of 64 operand rows, lane = row.
// Wave w walks row 4 blockIdx.x + w: 64 entries at a time are loaded coalesced (lane e holds entry e) and broadcast one by
// one; every entry is one line of xT read by the whole wave. The four sums meet in LDS and wave 0 runs EpiFwd on the quad.
template <typename T, bool DUAL, bool X2>
__global__ __launch_bounds__(256) void k_sparse_fwd(const uint32_t* __restrict__ row_ptr, const void* __restrict__ cols, int idx16,
                                                    const T* __restrict__ mu_v, const T* __restrict__ var_v, const T* __restrict__ xT,
                                                    const T* __restrict__ x2T, int64_t ld_xT, int N, int I, int O, EpiFwd<T> epi) {
    __shared__ float red[4][2][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int o = (int)blockIdx.x * 4 + wave;
    const int n = (int)blockIdx.y * 64 + lane;
    float a1 = 0.f, a2 = 0.f;
    if (o < O) {
        const uint32_t s = row_ptr[o], e = row_ptr[o + 1];
        const unsigned nl = (unsigned)min(n, N - 1);               // lanes past N re-read the last row; the epilogue masks them
        const uint32_t last = (uint32_t)(I - 1);
        auto term = [&](float xv, float x2v, float m, float v) {
            a1 = fmaf(m, xv, a1);
            if constexpr (DUAL) a2 = fmaf(v, X2 ? x2v : Elt<T>::from(Elt<T>::to(xv * xv)), a2);
        };
        for (uint32_t c0 = s; c0 < e; c0 += 64u) {
            const int cnt = (int)min(64u, e - c0);
            uint32_t ci = 0u;
            float mv = 0.f, vv = 0.f;
            if (lane < cnt) {
                const uint32_t k = c0 + (uint32_t)lane;
                ci = idx16 ? (uint32_t)reinterpret_cast<const uint16_t*>(cols)[k] : reinterpret_cast<const uint32_t*>(cols)[k];
                mv = Elt<T>::from(mu_v[k]);
                if constexpr (DUAL) vv = Elt<T>::from(var_v[k]);
            }
            int j = 0;
            for (; j + SP_UNROLL <= cnt; j += SP_UNROLL) {
                float xv[SP_UNROLL], x2v[SP_UNROLL];
#pragma unroll
                for (int u = 0; u < SP_UNROLL; ++u) {
                    // a wave-uniform row base + the lane's 32-bit offset: the SGPR-base form of the load
                    const int64_t off = (int64_t)min((uint32_t)__builtin_amdgcn_readlane(ci, j + u), last) * ld_xT;
                    xv[u] = Elt<T>::from((xT + off)[nl]);
                    x2v[u] = (DUAL && X2) ? Elt<T>::from((x2T + off)[nl]) : 0.f;
                }
#pragma unroll
                for (int u = 0; u < SP_UNROLL; ++u) term(xv[u], x2v[u], sp_bcast(mv, j + u), sp_bcast(vv, j + u));
            }
            for (; j < cnt; ++j) {
                const int64_t off = (int64_t)min((uint32_t)__builtin_amdgcn_readlane(ci, j), last) * ld_xT;
                term(Elt<T>::from((xT + off)[nl]), (DUAL && X2) ? Elt<T>::from((x2T + off)[nl]) : 0.f, sp_bcast(mv, j), sp_bcast(vv, j));
            }
        }
    }
    red[wave][0][lane] = a1;
    red[wave][1][lane] = a2;
    __syncthreads();
    if (wave != 0) return;
    const f32x4 s1 = {red[0][0][lane], red[1][0][lane], red[2][0][lane], red[3][0][lane]};
    const f32x4 s2 = {red[0][1][lane], red[1][1][lane], red[2][1][lane], red[3][1][lane]};
    epi((int)blockIdx.x * 4, n, s1, s2);                           // guards n >= N and the units past O
}

template <typename T>
static int forward_sparse_t(vbnn_ctx* ctx, const vbnn_sparse_fwd_args* a) {
    EpiFwd<T> e;
    e.bias = a->bias;
    e.noise = a->var_v != nullptr ? 1 : 0;
    e.seed = a->seed; e.layer = a->layer; e.draw = a->draw; e.row0 = a->row0; e.draw_dev = nullptr;
    e.rpd = (int)a->rows_per_draw;
    e.y = a->y; e.ld_y = a->ld_y; e.y_vec = a->y && vbnn_al16(a->y) && (a->ld_y % 4 == 0);
    e.r = nullptr; e.r_t = nullptr; e.ld_r = 0; e.r_vec = 0;
    e.relu = (int)a->relu;
    e.h = (T*)a->h; e.h2 = (T*)a->h2; e.ld_h = a->ld_h;
    e.hT = (T*)a->hT; e.h2T = (T*)a->h2T; e.ld_hT = a->ld_hT;
    e.O = (int)a->O; e.N = (int)a->N;
    const dim3 grid((unsigned)((a->O + 3) / 4), (unsigned)((a->N + 63) / 64));
#define VBNN_SPARSE_FWD(DUAL, X2)                                                                                                  \
    hipLaunchKernelGGL((k_sparse_fwd<T, DUAL, X2>), grid, dim3(256), 0, ctx->stream, a->row_ptr, a->cols, a->idx_bytes == 2 ? 1 : 0, \
                       (const T*)a->mu_v, (const T*)a->var_v, (const T*)a->xT, (const T*)a->x2T, a->ld_xT, (int)a->N, (int)a->I,   \
                       (int)a->O, e)
    if (!a->var_v) VBNN_SPARSE_FWD(false, false);
    else if (a->x2T) VBNN_SPARSE_FWD(true, true);
    else VBNN_SPARSE_FWD(true, false);
#undef VBNN_SPARSE_FWD
    return vbnn_check_launch("k_sparse_fwd");
}

extern "C" int vbnn_forward_sparse(vbnn_ctx* ctx, int dtype, const vbnn_sparse_fwd_args* a) {
    VBNN_API_BEGIN
    VBNN_REQUIRE(ctx && a, "null ctx/args");
    VBNN_REQUIRE(a->row_ptr && a->cols && a->mu_v && a->xT, "row_ptr, cols, mu_v and xT are required");
    VBNN_REQUIRE(!a->x2T || a->var_v, "x2T needs var_v (LRT pair)");
    VBNN_REQUIRE(a->N > 0 && a->I > 0 && a->O > 0, "N, I, O must be positive");
    VBNN_REQUIRE(a->N < (1ll << 22) && a->I < (1ll << 31) && a->O < (1ll << 31), "dimension too large");
    VBNN_REQUIRE(a->idx_bytes == 4 || (a->idx_bytes == 2 && a->I <= 65536), "idx_bytes (2: I <= 65536 only; 4)");
    VBNN_REQUIRE(a->ld_xT >= a->N, "ld_xT");
    VBNN_REQUIRE(a->rows_per_draw >= 0 && a->rows_per_draw < (1ll << 31), "rows_per_draw");
    VBNN_REQUIRE(!a->h2 || a->h, "h2 needs h");
    VBNN_REQUIRE(!a->h2T || a->hT, "h2T needs hT");
    VBNN_REQUIRE(!a->h || (a->ld_h >= a->O && a->ld_h % 4 == 0), "ld_h");
    VBNN_REQUIRE(!a->hT || a->ld_hT >= a->N, "ld_hT");
    VBNN_REQUIRE(!a->y || a->ld_y >= a->O, "ld_y");
    if (dtype == VBNN_F32) return forward_sparse_t<float>(ctx, a);
    if (dtype == VBNN_BF16) return forward_sparse_t<bf16_t>(ctx, a);
    vbnn_set_error("unsupported dtype %d", dtype);
    return VBNN_ERR_UNSUPPORTED;
    VBNN_API_END
}
