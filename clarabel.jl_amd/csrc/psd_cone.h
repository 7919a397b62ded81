// What the PSD triangle cone kernels share (step_psd.hip, step_psd_large.hip, scaling_psd.hip, barrier_psd.hip, start.hip): the LDS
// layout of one n x n matrix, the cone record of the step's table (cone_layout.h kPsd*), the entries of svec_to_mat / mat_to_svec and
// of their round trip, the affine_ds entry, pos_finite and the two-sided Jacobi iteration.  One definition each: these files are
// compiled with -ffp-contract=off and the reference modules of tests/ emulate the rounding order of the expressions below, so a
// kernel that needs one of them calls it here and every kernel rounds alike.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cone_layout.h"
#include "cone_reduce.h"

namespace hipkkt {

constexpr int kPsdMaxN = 64;                                   // HIPKKT_PSD_STEP_MAX_DIM
constexpr int kPsdMatDoubles = kPsdMaxN * (kPsdMaxN + 1);      // one n x n matrix with its padded leading dimension
constexpr double kPsdIsqrt2 = 0.7071067811865475;              // 1 / sqrt(2) as the caller rounds it

// column-major, leading dimension n + 1 when n is a multiple of 32 (the column reads of A' would otherwise hit the same banks)
struct Cone { int64_t row0; int n, ld; int64_t foff, loff; bool ok; };

// the record of cone c; a side outside lo .. hi (step_psd_large.hip: lmin .. kPsdLargeMaxN) is not ok and gets n = 0
__device__ __forceinline__ Cone cone_of(const int64_t *__restrict__ tab, int c, int lo = 1, int hi = kPsdMaxN) {
    Cone K;
    K.row0 = tab[kPsdTab * c + kPsdRow0];
    const int64_t n = tab[kPsdTab * c + kPsdN];
    K.foff = tab[kPsdTab * c + kPsdFactor0];
    K.loff = tab[kPsdTab * c + kPsdLambda0];
    K.ok = n >= 1 && n >= lo && n <= hi;
    K.n = K.ok ? (int)n : 0;
    K.ld = (K.n % 32 == 0) ? K.n + 1 : K.n;
    return K;
}

__device__ __forceinline__ bool pos_finite(double v) { return v > 0.0 && v - v == 0.0; }

// entry (i, j) of svec_to_mat(x)
__device__ __forceinline__ double svec_entry(const double *__restrict__ x, int i, int j) {
    const int r = i < j ? i : j, c = i < j ? j : i;
    const double v = x[c * (c + 1) / 2 + r];
    return i == j ? v : v * kPsdIsqrt2;
}
// X = svec_to_mat(x)
__device__ __forceinline__ void load_svec(double *X, const double *__restrict__ x, const Cone &K) {
    const int n = K.n;
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const int i = e % n, j = e / n;
        X[i + j * K.ld] = svec_entry(x, i, j);
    }
}
// what an off-diagonal pair (up, lo) becomes on its way through mat_to_svec and back through svec_to_mat
__device__ __forceinline__ double round_trip_pair(double up, double lo) { return ((up + lo) * kPsdIsqrt2) * kPsdIsqrt2; }
// entry (i, j) of svec_to_mat(mat_to_svec(Y)): what a result of mul_W goes through before the next operation reads it as a matrix
__device__ __forceinline__ double round_trip_entry(const double *Y, int ld, int i, int j) {
    if (i == j) return Y[i + i * ld];
    const int r = i < j ? i : j, c = i < j ? j : i;
    return round_trip_pair(Y[r + c * ld], Y[c + r * ld]);
}
// entry e = i + j n of the n x n matrix Y into out = mat_to_svec(Y) (the lower triangle i > j writes nothing); diag_add goes to the
// diagonal positions; addc != NULL: out = -(out + addc)
__device__ __forceinline__ void store_svec_entry(double *out, const double *Y, int n, int ld, int e, double diag_add, const double *addc) {
    const int i = e % n, j = e / n;
    if (i > j) return;
    double v = i == j ? Y[i + i * ld] + diag_add : (Y[i + j * ld] + Y[j + i * ld]) * kPsdIsqrt2;
    const int k = j * (j + 1) / 2 + i;
    if (addc) v = -(v + addc[k]);
    out[k] = v;
}
// the same entry of affine_ds: lambda_j^2 at the diagonal positions, 0 elsewhere
__device__ __forceinline__ void affine_ds_entry(double *out, const double *lam, int n, int e) {
    const int i = e % n, j = e / n;
    if (i > j) return;
    const double l = lam[j];
    out[j * (j + 1) / 2 + i] = i == j ? l * l : 0.0;
}

constexpr int kPsdMaxSweeps = 30;
constexpr double kPsdEps = 2.220446049250313e-16;

// The cyclic two-sided Jacobi iteration of the step length (step_psd.hip k_psd_len, step_psd_large.hip k_psdl_len) and of the default
// start's margins (start.hip) on the symmetric n x n matrix M in LDS; tot2 = |M|_F^2, the same value in every thread.  red[4], rc / rs /
// rp / rq[half of the caller's largest side]: LDS scratch (rs = the rotations' s, rc = their s / (1 + c), rp < rq their index pairs).
// Returns whether M was finite; afterwards the diagonal of M holds the eigenvalues (after a barrier: the last loop ends with one).
// kPairLanes >= n / 2 and kRowLanes >= n are the lane widths of the two rotation passes: <32, 64> for a side up to 64, <64, 128> up
// to 128.  The rotations of one set touch disjoint rows / columns, so the widths change no bit.  One definition: every kernel rounds alike.
template <int kPairLanes = 32, int kRowLanes = 64>
__device__ __forceinline__ bool psd_jacobi_sweeps(double *M, const Cone &K, double tot2, double *red, double *rc, double *rs, int *rp,
                                                  int *rq) {
    static_assert(256 % kPairLanes == 0 && 256 % kRowLanes == 0, "a 256-thread workgroup is cut into whole groups of lanes");
    const int n = K.n, ld = K.ld, t = threadIdx.x;
    // cyclic Jacobi: per sweep np - 1 sets of np / 2 disjoint rotations (round robin over np = n rounded up to even; the index n of an
    // odd n is a dummy).  Stops when off(M) <= eps |M|_F; a non-finite |M|_F skips the sweeps (uniform: block_sum gives every thread
    // the same value)
    const int np = n + (n & 1), half = np / 2;
    const bool finite = tot2 - tot2 == 0.0;
    for (int sweep = 0; finite && sweep < kPsdMaxSweeps; sweep++) {
        double off2 = 0.0;
        for (int e = t; e < n * n; e += 256) {
            const int i = e % n, j = e / n;
            if (i != j) off2 += M[i + j * ld] * M[i + j * ld];
        }
        off2 = block_sum(off2, red);
        if (!(off2 > kPsdEps * kPsdEps * tot2)) break;
        for (int r = 0; r < np - 1; r++) {
            // pair k of set r: (np - 1, r) for k = 0, ((r + k) mod (np - 1), (r - k) mod (np - 1)) otherwise; a pair with the dummy index
            // or with a zero entry keeps s = 0 and is skipped below
            if (t < half) {
                const int a = t == 0 ? np - 1 : (r + t) % (np - 1), b = (r + np - 1 - t) % (np - 1);
                const int p = a < b ? a : b, q = a < b ? b : a;
                // the stable formula: t = sign(tau) / (|tau| + sqrt(1 + tau^2)), c = 1 / sqrt(1 + t^2), s = t c; the rotation is applied
                // as x_p - s (x_q + r x_p), x_q + s (x_p - r x_q) with r = s / (1 + c), whose rounding error shrinks with the angle
                double sn = 0.0, rr = 0.0;
                if (q < n) {
                    const double apq = M[p + q * ld];
                    if (apq != 0.0) {
                        const double tau = (M[q + q * ld] - M[p + p * ld]) / (2.0 * apq);
                        const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        const double cs = 1.0 / sqrt(1.0 + tt * tt);
                        sn = tt * cs;
                        rr = sn / (1.0 + cs);
                    }
                }
                rs[t] = sn; rc[t] = rr; rp[t] = p; rq[t] = q;
            }
            __syncthreads();
            // rows: M <- J' M.  Lane -> (pair k = t mod kPairLanes, column j = t / kPairLanes + (256 / kPairLanes) i): half <= kPairLanes,
            // no division in the loop
            {
                const int k = t % kPairLanes;
                if (k < half && rs[k] != 0.0) {
                    const int p = rp[k], q = rq[k];
                    const double sn = rs[k], rr = rc[k];
                    for (int j = t / kPairLanes; j < n; j += 256 / kPairLanes) {
                        const double mp = M[p + j * ld], mq = M[q + j * ld];
                        M[p + j * ld] = mp - sn * (mq + rr * mp);
                        M[q + j * ld] = mq + sn * (mp - rr * mq);
                    }
                }
            }
            __syncthreads();
            // columns: M <- M J.  Lane -> (row i = t mod kRowLanes, pair k = t / kRowLanes + (256 / kRowLanes) i); the rotated pair is
            // zero by construction
            {
                const int i = t % kRowLanes;
                if (i < n) {
                    for (int k = t / kRowLanes; k < half; k += 256 / kRowLanes) {
                        const double sn = rs[k], rr = rc[k];
                        if (sn == 0.0) continue;
                        const int p = rp[k], q = rq[k];
                        const double mp = M[i + p * ld], mq = M[i + q * ld];
                        M[i + p * ld] = i == q ? 0.0 : mp - sn * (mq + rr * mp);
                        M[i + q * ld] = i == p ? 0.0 : mq + sn * (mp - rr * mq);
                    }
                }
            }
            __syncthreads();
        }
    }
    return finite;
}

}  // namespace hipkkt
