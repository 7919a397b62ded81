// What the PSD triangle cone kernels share (step_psd.hip, scaling_psd.hip): the LDS layout of one n x n matrix, the cone record of the
// step's table (cone_layout.h kPsd*) and the svec_to_mat loader.  One definition each: both files read a cone's rows the same way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cone_layout.h"

namespace hipkkt {

constexpr int kPsdMaxN = 64;                                   // HIPKKT_PSD_STEP_MAX_DIM
constexpr int kPsdMatDoubles = kPsdMaxN * (kPsdMaxN + 1);      // one n x n matrix with its padded leading dimension
constexpr double kPsdIsqrt2 = 0.7071067811865475;              // 1 / sqrt(2) as the caller rounds it

// column-major, leading dimension n + 1 when n is a multiple of 32 (the column reads of A' would otherwise hit the same banks)
struct Cone { int64_t row0; int n, ld; int64_t foff, loff; bool ok; };

__device__ __forceinline__ Cone cone_of(const int64_t *__restrict__ tab, int c) {
    Cone K;
    K.row0 = tab[kPsdTab * c + kPsdRow0];
    const int64_t n = tab[kPsdTab * c + kPsdN];
    K.foff = tab[kPsdTab * c + kPsdFactor0];
    K.loff = tab[kPsdTab * c + kPsdLambda0];
    K.ok = n >= 1 && n <= kPsdMaxN;
    K.n = K.ok ? (int)n : 0;
    K.ld = (K.n % 32 == 0) ? K.n + 1 : K.n;
    return K;
}

// X = svec_to_mat(x)
__device__ __forceinline__ void load_svec(double *X, const double *__restrict__ x, const Cone &K) {
    const int n = K.n;
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const int i = e % n, j = e / n;
        const int r = i < j ? i : j, c = i < j ? j : i;
        const double v = x[c * (c + 1) / 2 + r];
        X[i + j * K.ld] = i == j ? v : v * kPsdIsqrt2;
    }
}

}  // namespace hipkkt
