// moments_common.h -- what the kernels of the moments family (moments.hip, class_moments.hip, label_moments.hip) share: the quad
// access paths, a thread's tile of a row, the row sum whose order depends on the row width alone, the workgroup partials of the
// double totals with the kernel that adds them, and the host's launch plan. kcentre.hip takes the quad loads and the row sum.
#pragma once
#include "common.h"
#include <algorithm>

typedef float f32x2 __attribute__((ext_vector_type(2)));

// four consecutive floats; mode 2: one 16-byte access, 1: two 8-byte, 0: element by element (`valid` of them). The streams a
// launch reads or writes once take the nontemporal hint (NT) on their vector accesses; 4-byte stores stay plain, which the L2
// combines (the update sweep's finding).
template <bool NT>
__device__ __forceinline__ void mom_load4(const float* p, float (&v)[4], int valid, int mode) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (valid == 0) return;
    if (mode == 2) {
        const f32x4 t = NT ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)) : *reinterpret_cast<const f32x4*>(p);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else if (mode == 1) {
        const f32x2* p2 = reinterpret_cast<const f32x2*>(p);
        const f32x2 a = NT ? __builtin_nontemporal_load(p2) : p2[0];
        const f32x2 b = NT ? __builtin_nontemporal_load(p2 + 1) : p2[1];
        v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j < valid) v[j] = NT ? __builtin_nontemporal_load(p + j) : p[j];
    }
}
template <bool NT>
__device__ __forceinline__ void mom_store4(float* p, const float (&v)[4], int valid, int mode) {
    if (valid == 0) return;
    if (mode == 2) {
        const f32x4 t = {v[0], v[1], v[2], v[3]};
        if (NT) __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(p)); else *reinterpret_cast<f32x4*>(p) = t;
    } else if (mode == 1) {
        f32x2* p2 = reinterpret_cast<f32x2*>(p);
        const f32x2 a = {v[0], v[1]}, b = {v[2], v[3]};
        if (NT) { __builtin_nontemporal_store(a, p2); __builtin_nontemporal_store(b, p2 + 1); } else { p2[0] = a; p2[1] = b; }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j < valid) p[j] = v[j];
    }
}

// a thread's NQ quads of a row of `width` columns, the first of them quad q0: quads q0, q0 + TR, ... (columns col[k] ..
// col[k] + valid[k] - 1; valid 0 past the row's end). Thread i of the row passes q0 = i, plus the chunk's first quad.
template <int NQ, int TR, typename I>
__device__ __forceinline__ void mom_tile(I q0, int64_t width, int (&valid)[NQ], I (&col)[NQ]) {
    const I nq = (I)((width + 3) >> 2);
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const I q = q0 + (I)k * TR;
        col[k] = 4 * q;
        valid[k] = q < nq ? (int)min((I)4, (I)width - 4 * q) : 0;
    }
}

// sum over the row's threads: lane-strided partials in, the xor butterfly inside a wave, the waves in wave order through LDS.
// Every thread of the row returns the same bits. WPR == 4: block-uniform call (two barriers).
template <int WPR, int N>
__device__ __forceinline__ void mom_row_sum(float (&v)[N], float (*red)[4], int wave) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] += __shfl_xor(v[k], off, 64);
    if (WPR == 1) return;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < N; ++k) red[k][wave] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
    __syncthreads();
}

// the workgroup's partial of the NT totals (four; the Gaussian head's and the classes' five): [NT][gridDim.x] doubles, which
// k_moments_finish adds in workgroup order
template <int WPR, int NT>
__device__ __forceinline__ void mom_store_partials(double* part, const double (&tot)[NT], double (*dred)[4], int wave, int tr) {
    if (!part) return;                                     // launch-uniform
    if (WPR == 1) {
        if (tr == 0)
#pragma unroll
            for (int k = 0; k < NT; ++k) dred[k][wave] = tot[k];
        __syncthreads();
        if (threadIdx.x < NT) {
            const int k = threadIdx.x;
            part[(int64_t)k * gridDim.x + blockIdx.x] = ((dred[k][0] + dred[k][1]) + dred[k][2]) + dred[k][3];
        }
    } else if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NT; ++k) part[(int64_t)k * gridDim.x + blockIdx.x] = tot[k];
    }
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

// ---- host side
// the launch plan of a family's kernels over R rows of `width` columns; `totals`: this launch finishes and the caller wants the
// NT totals. The caller requires `fits` ("reduction scratch"), launches nb workgroups of 256 with `part`, then calls finish().
template <int NT>
struct MomPlan {
    vbnn_cu_scope scope;
    bool wave_rows;                                        // one wave per row, four rows per workgroup; else a workgroup per row
    int nb;                                                // ~8 workgroups per CU, grid-stride above
    bool fits;
    double* part;                                          // the workgroups' partials, null without totals
    MomPlan(const vbnn_ctx* ctx, int64_t width, int64_t R, bool totals) : scope(ctx), wave_rows(width <= 256) {
        nb = (int)std::min<int64_t>(wave_rows ? (R + 3) / 4 : R, (int64_t)vbnn_cu_count() * 8);
        fits = !totals || (size_t)nb * NT <= ctx->scratch_doubles;
        part = totals ? ctx->scratch : nullptr;
    }
    void finish(hipStream_t stream, double* totals) const {
        if (part) hipLaunchKernelGGL(k_moments_finish<NT>, dim3(1), dim3(256), 0, stream, part, nb, totals);
    }
};
