// The workgroup and wavefront reductions of the cone kernels (scaling.hip, step.hip, step_cone3.hip, step_genpow.hip, step_psd.hip).
// One definition each: the rows a kernel of one file computes must be bit-identical to what another file's kernel gives for them.
#pragma once
#include <hip/hip_runtime.h>

namespace hipkkt {

// 256 threads, red[4] in LDS; every thread gets the result.  The first barrier is there because red[] may still be read from the
// previous reduction.
__device__ __forceinline__ double block_sum(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ double block_min(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_down(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
}
// a minimum that keeps a NaN
__device__ __forceinline__ double nan_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double block_nan_min(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v = nan_min(v, __shfl_down(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return nan_min(nan_min(red[0], red[1]), nan_min(red[2], red[3]));
}

// one wavefront of 64, butterfly: every lane gets the result
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_prod(double v) {
    for (int o = 32; o > 0; o >>= 1) v *= __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_or(int v) {
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

}  // namespace hipkkt
