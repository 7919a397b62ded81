// Small helpers shared by the kernel files: the launchers' grid size, a wave-uniform lane read, the max-|v| reductions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hipkkt {

static inline unsigned nblk(int64_t n, int bs = 256) { return (unsigned)((n + bs - 1) / bs); }

__device__ __forceinline__ double readlane_f64(double x, int l) {   // l wave-uniform
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, l), hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ void atomic_max_abs(unsigned long long *slot, double v) {
    // |v| as an ordered integer; NaN (all-ones exponent, non-zero mantissa) compares largest,
    // so a NaN anywhere surfaces as a non-finite maximum
    unsigned long long bits = (unsigned long long)__double_as_longlong(fabs(v));
    atomicMax(slot, bits);
}

__device__ __forceinline__ double wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) {
        double o = __shfl_xor(v, off, 64);
        v = (o > v || o != o) ? o : v;
    }
    return v;
}

// one same-address atomic per BLOCK (same-word atomics serialise at ~88/us on this chip)
__device__ __forceinline__ void block_atomic_max_abs(unsigned long long *slot, double a) {
    __shared__ double wm_[16];
    a = wave_max(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if (lane == 0) wm_[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = wm_[0];
        for (int i = 1; i < nw; i++) m = (wm_[i] > m || wm_[i] != wm_[i]) ? wm_[i] : m;
        atomic_max_abs(slot, m);
    }
}

}  // namespace hipkkt
