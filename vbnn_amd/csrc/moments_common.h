// moments_common.h -- what the kernels of the moments family (moments.hip, class_moments.hip) share: the quad access paths,
// the row sum whose order depends on the row width alone, and the workgroup partials of the double totals.
#pragma once
#include "common.h"

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

// the workgroup's partial of the NT totals (four; the Gaussian head's five): [NT][gridDim.x] doubles, which k_moments_finish
// adds in workgroup order
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
