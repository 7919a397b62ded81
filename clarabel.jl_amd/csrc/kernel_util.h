// Small helpers shared by the kernel files, one definition each: the launchers' grid size, wave-uniform reads, global accesses with a
// uniform base, the relaxed hand-off accesses, the pivot reciprocals, the LDS-only barrier, the matrix-core settle, the max-|v| reductions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hipkkt {

static inline unsigned nblk(int64_t n, int bs = 256) { return (unsigned)((n + bs - 1) / bs); }

typedef double v4f64 __attribute__((ext_vector_type(4)));   // one accumulator of the 16x16x4 FP64 matrix-core instruction

__device__ __forceinline__ double readlane_f64(double x, int l) {   // l wave-uniform
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, l), hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// wave-uniform values are forced into SGPRs (a record read through a plain pointer lands in VGPRs otherwise)
__device__ __forceinline__ int rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }

template <class T>
__device__ __forceinline__ T *rfl_ptr(T *p) {
    const unsigned long long u = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return (T *)(((unsigned long long)hi << 32) | lo);
}
#define HK_GLOBAL __attribute__((address_space(1)))
__device__ __forceinline__ double ld_off(const double *base, unsigned byte_off) {
    // uniform base + 32-bit lane offset, explicitly in the global address space (global_load ... saddr)
    return *(const HK_GLOBAL double *)((const HK_GLOBAL char *)base + byte_off);
}
__device__ __forceinline__ void st_off(double *base, unsigned byte_off, double v) {
    *(HK_GLOBAL double *)((HK_GLOBAL char *)base + byte_off) = v;
}

// relaxed, agent-scope accesses of the words and values workgroups hand to each other (front_block.hip, front_block2.hip)
__device__ __forceinline__ int ld_relaxed_i(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ld_relaxed(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_relaxed(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// 1/d on the pivot-to-pivot critical path: hardware reciprocal + two Newton steps (~50 clocks) instead of the IEEE
// division sequence (~112 clocks, tools/ubench.hip).  |relative error| <= 1 ulp; the D and 1/D that are stored for
// the solves are formed with the exact division after the loop.  d is never zero or subnormal here (the pivot rule
// has replaced such values by +-delta); an infinite or NaN d propagates and is caught by the non-finite check.
__device__ __forceinline__ double pivot_rcp(double d) {
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    r = fma(fma(-d, r, 1.0), r, r);
    return r;
}

// 1 / d on the pivot chain: the hardware reciprocal r (2^-27 or better), then r (1 + e + e^2) with e = 1 - d r -- three dependent
// operations instead of the four of two Newton steps (error ~ e^3 + one rounding: 1.9 units of 2^-53 measured over 6.7e7 values,
// tools/ubench_pivot.hip).  k_factor_panel and both forms of the front-batch kernel share this one: their pivots agree bit for bit.
__device__ __forceinline__ double pivot_rcp3(double d) {
    const double r = __builtin_amdgcn_rcp(d);
    const double e = fma(-d, r, 1.0);
    const double e2 = fma(e, e, e);
    return fma(r, e2, r);
}

// LDS-only workgroup barrier: __syncthreads() also waits for this wave's outstanding global stores (vmcnt), which would put the
// write-through latency of every streamed record on the pivot chain (and global memory into the barriers of k_factor_panel's pivot
// loop).  Nothing in the loops that use it communicates through global memory inside the workgroup.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// An exec-masked block (s_cbranch_execz) between a matrix-core instruction and the first read of its accumulators (v_accvgpr_read)
// is a trap: the waves that skip the block arrive at the read with fewer wait states than the compiler's hazard recogniser counted
// along the fall-through path, and read accumulators that are still being written (measured in round 4: deterministic 1e-4 errors
// of the factorisation with a store block of two of the four waves behind the rank-8 update).  The front-batch loops keep such blocks
// away from that path (they sit behind a barrier, next to wave 0's eliminations); where one cannot be avoided (or at a loop
// back-edge), this pins 24 wait states (enough for the 16-pass FP64 MFMA) between the matrix-core instructions before it and
// whatever follows.
__device__ __forceinline__ void mfma_settle() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
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
