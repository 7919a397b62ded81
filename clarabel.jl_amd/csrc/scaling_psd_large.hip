// The Nesterov-Todd scaling of PSD triangle cones of side 65 .. 128 on the device (opt-in, hipkkt_psd_scaling_enable_large on a handle
// enabled through hipkkt_step_enable_psd_large): the algorithm of scaling_psd.hip operation for operation -- right-looking lower
// Cholesky factors of S and Z with ascending k-sums, G = L2' L1, the one-sided Jacobi iteration on the columns of G (round-robin
// pairs, eight lanes per pair with lane l summing rows l, l + 8, .., the three-step butterfly, the small-angle rotation, stop after a
// sweep without a rotation, kMaxSweeps, one polishing sweep), sigma, R = (L1 V) sigma^-1/2, Rinv = sigma^-3/2 g' L2', the dot2
// refinement of lambda with four lanes per column and the rescaling, the counting sort -- in another placement, because four
// 128 x 129 matrices are 528 KB and a compute unit has 160 KiB of LDS.
//
// One workgroup of 512 threads per cone (8 ceil(n / 2) <= 512: the "eight lanes own pair k" layout of the small kernel, and with it
// every order of summation) and ONE matrix M in LDS (psd_cone.h layout: leading dimension n + 1 when n % 32 == 0); everything else
// lives in the cone's four matrices of the large workspace (kernels.h kPsdLargeMats, column-major, leading dimension n):
//   phase                         M (LDS)             ws 0        ws 1        ws 2          ws 3
//   Cholesky of S                 S -> L1             <- L1
//   Cholesky of Z                 Z -> L2             L1          <- L2
//   G = L2' L1, V = I             L2                  L1          L2          <- I          <- G
//   Jacobi, sigma                 G -> U Sigma        L1          L2          V
//   Rinv' -> Rinv_all (staging)   G                               L2
//   R -> R_all (staging)                              L1                      V
//   refinement, r' Z r and q' r   R                   <- S        <- Z        <- R          <- Rinv'
//   refinement, q' S q            Rinv'               S
//   sort, outputs                                                             R             Rinv'
// A lane rotates its own rows of G in LDS and of V in device memory; one barrier per set orders the workgroup's own global stores
// and loads, as the small kernel already relies on for its staging copies.  Every entry is computed by one thread with the small
// kernel's expression and the small kernel's order of k, so a cone of side <= 64 gets the bits of scaling_psd.hip
// (tests/test_gpu_psd_scaling_large.py holds it to that through the testing switch PSD_LARGE_MIN); svec_to_mat is symmetric bit for
// bit, so the refinement reads row i of S / Z as column i.
//
// A cone that fails (a pivot that is not pos_finite, a non-finite input -- it reaches a pivot --, the sweep bound, a sigma that is not
// finite and positive) sets the call's fail word and its own word of `bad` and gets NaN R, Rinv, lambda; the caller's k_psd_hs launch
// then writes no K entry of it.  No assert, no trap, no spin, no communication between workgroups; every loop is bounded by n,
// kMaxSweeps or a launch-time constant; every exit is taken by all threads of a workgroup on an LDS word read behind a barrier.
// Compiled with -ffp-contract=off (the fma calls of dot2 are explicit).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cone_layout.h"
#include "kernels.h"
#include "psd_cone.h"
#include "psd_nt.h"

namespace hipkkt {

namespace {

constexpr int kMaxSweeps = 40;
constexpr double kEps = kPsdNtEps;
constexpr int kMaxN = kPsdLargeMaxN;
constexpr int kThreads = 512;
constexpr int kLdsDoubles = kMaxN * (kMaxN + 1);
static_assert(kPsdLargeMats >= 4, "L1, L2, V and one staging matrix per cone");
static_assert(8 * (kMaxN / 2) <= kThreads && 4 * kMaxN <= kThreads, "eight lanes per pair, four lanes per column");

// the number of rotations of a sweep over the workgroup: whole numbers, exact in any order; every thread gets the result
__device__ __forceinline__ double block_count(double v, double *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
}

// the right-looking lower Cholesky factor of M in place: entry (i, k) receives m_ik - l_i0 l_k0 - l_i1 l_k1 - .. with the k-sums in
// ascending order, the diagonal keeps the pivot until the end.  A pivot that is not pos_finite sets *flag (the same value in every
// thread: the exit is uniform).  Ends with a barrier.
__device__ __forceinline__ void cholesky_lds(double *M, int n, int ld, int *flag) {
    const int t = threadIdx.x;
    bool ok = true;
    for (int j = 0; j < n; j++) {
        const double d = M[j + j * ld];
        if (!pos_finite(d)) { ok = false; break; }
        const double piv = sqrt(d);
        for (int i = j + 1 + t; i < n; i += kThreads) M[i + j * ld] = M[i + j * ld] / piv;
        __syncthreads();
        {
            const int i = j + 1 + (t & 127);
            if (i < n) {
                const double li = M[i + j * ld];
                for (int k = j + 1 + (t >> 7); k <= i; k += kThreads / 128) M[i + k * ld] = M[i + k * ld] - li * M[k + j * ld];
            }
        }
        __syncthreads();
    }
    if (!ok && t == 0) *flag = 1;
    if (ok && t < n) M[t + t * ld] = sqrt(M[t + t * ld]);
    __syncthreads();
}

// M = svec_to_mat(x) in the LDS layout; dst = the same, leading dimension n
__device__ __forceinline__ void load_svec_lds(double *M, const double *__restrict__ x, int n, int ld) {
    for (int e = threadIdx.x; e < n * n; e += kThreads) { const int i = e % n, j = e / n; M[i + j * ld] = svec_entry(x, i, j); }
}
__device__ __forceinline__ void lds_to_ws(double *dst, const double *M, int n, int ld) {
    for (int e = threadIdx.x; e < n * n; e += kThreads) dst[e] = M[e % n + (e / n) * ld];
}
__device__ __forceinline__ void ws_to_lds(double *M, const double *src, int n, int ld) {
    for (int e = threadIdx.x; e < n * n; e += kThreads) M[e % n + (e / n) * ld] = src[e];
}

}  // namespace

__global__ void __launch_bounds__(kThreads)
k_psdl_nt_scaling(const int64_t *__restrict__ tab, const int *__restrict__ lidx, int lmin, const double *__restrict__ s_all,
                  const double *__restrict__ z_all, double *R_all, double *Rinv_all, double *__restrict__ lam_all, double *ws,
                  int *__restrict__ bad, int *__restrict__ fail) {
    __shared__ double M[kLdsDoubles];
    __shared__ double red[kThreads / 64], sig[kMaxN], lis[kMaxN], red2[kMaxN];
    __shared__ int rank[kMaxN], flag, sigbad;      // flag: Cholesky / sweep bound; sigbad: a sigma that is not finite and positive
    const int slot = blockIdx.x, t = threadIdx.x;
    const int c = lidx[slot];
    const Cone K = cone_of(tab, c, lmin, kMaxN);
    if (!K.ok) return;
    const int n = K.n, ld = K.ld;
    double *Rg = R_all + K.foff, *Rig = Rinv_all + K.foff, *lamg = lam_all + K.loff;
    double *A = ws + (int64_t)slot * kPsdLargeMats * kPsdLargeMatDoubles, *B = A + kPsdLargeMatDoubles, *V = B + kPsdLargeMatDoubles,
           *T = V + kPsdLargeMatDoubles;
    if (t == 0) { flag = 0; sigbad = 0; }
    load_svec_lds(M, s_all + K.row0, n, ld);
    __syncthreads();

    // ---- the two Cholesky factors, one after the other in M: L1 to ws 0, L2 to ws 1 and kept in M for the product below
    cholesky_lds(M, n, ld, &flag);
    if (flag == 0) {
        lds_to_ws(A, M, n, ld);
        __syncthreads();      // (every read of M is done)
        load_svec_lds(M, z_all + K.row0, n, ld);
        __syncthreads();
        cholesky_lds(M, n, ld, &flag);
    }
    // ---- G = L2' L1 (through ws 3: M is an operand), V = I
    if (flag == 0) {
        lds_to_ws(B, M, n, ld);
        for (int e = t; e < n * n; e += kThreads) {
            const int i = e % n, j = e / n;
            double acc = 0.0;
            for (int k = i > j ? i : j; k < n; k++) acc += M[k + i * ld] * A[k + j * n];
            T[e] = acc;
            V[e] = i == j ? 1.0 : 0.0;
        }
        __syncthreads();
        ws_to_lds(M, T, n, ld);      // (each thread reads back the entries it wrote)
    }
    __syncthreads();

    // ---- one-sided Jacobi: G in M, V in ws 2
    if (flag == 0) {
        const int np = n + (n & 1), half = np / 2;
        const int k = t >> 3, l = t & 7;
        bool converged = false;
        for (int sweep = 0; sweep <= kMaxSweeps; sweep++) {
            // after the sweep without a rotation: one polishing sweep, in which every pair with c != 0 rotates (scaling_psd.hip)
            const bool polish = converged;
            if (!polish && sweep == kMaxSweeps) break;
            double nrot = 0.0;
            for (int r = 0; r < np - 1; r++) {
                // pair k of set r: (np - 1, r) for k = 0, ((r + k) mod (np - 1), (r - k) mod (np - 1)) otherwise
                if (k < half) {
                    const int a_ = k == 0 ? np - 1 : (r + k) % (np - 1), b_ = (r + np - 1 - k) % (np - 1);
                    const int p = a_ < b_ ? a_ : b_, q = a_ < b_ ? b_ : a_;
                    if (q < n) {
                        double *gp = M + p * ld, *gq = M + q * ld;
                        double a = 0.0, b = 0.0, cc = 0.0;
                        for (int i = l; i < n; i += 8) {
                            const double x = gp[i], y = gq[i];
                            a += x * x; b += y * y; cc += x * y;
                        }
                        a = sum8(a); b = sum8(b); cc = sum8(cc);
                        if (polish ? cc != 0.0 : fabs(cc) > kEps * sqrt(a * b)) {
                            const double zeta = (b - a) / (2.0 * cc);
                            const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                            const double cs = 1.0 / sqrt(1.0 + tt * tt);
                            const double sn = tt * cs, rr = sn / (1.0 + cs);
                            // (the lane's rows of V are loaded together: their device-memory latencies overlap, and with the rotation of G)
                            double *vp = V + p * n, *vq = V + q * n;
                            double u[kMaxN / 8], w[kMaxN / 8];
#pragma unroll
                            for (int ii = 0; ii < kMaxN / 8; ii++) {
                                const int i = l + 8 * ii;
                                if (i < n) { u[ii] = vp[i]; w[ii] = vq[i]; }
                            }
                            for (int i = l; i < n; i += 8) {
                                const double x = gp[i], y = gq[i];
                                gp[i] = x - sn * (y + rr * x);
                                gq[i] = y + sn * (x - rr * y);
                            }
#pragma unroll
                            for (int ii = 0; ii < kMaxN / 8; ii++) {
                                const int i = l + 8 * ii;
                                if (i < n) {
                                    vp[i] = u[ii] - sn * (w[ii] + rr * u[ii]);
                                    vq[i] = w[ii] + sn * (u[ii] - rr * w[ii]);
                                }
                            }
                            if (l == 0) nrot += 1.0;
                        }
                    }
                }
                __syncthreads();
            }
            if (polish) break;
            nrot = block_count(nrot, red);
            if (nrot == 0.0) converged = true;
        }
        if (!converged && t == 0) flag = 1;      // (the same in every thread: block_count; thread 0 records it)
    }
    __syncthreads();

    // ---- sigma_j = |g_j|, lisqrt_j = 1 / sqrt(sigma_j)
    if (flag == 0) {
        const int l = t & 7;
        for (int j = t >> 3; j < n; j += kThreads / 8) {
            const double *gj = M + j * ld;
            double a = 0.0;
            for (int i = l; i < n; i += 8) a += gj[i] * gj[i];
            a = sum8(a);
            if (l == 0) {
                const double sg = sqrt(a);
                sig[j] = sg;
                lis[j] = 1.0 / sqrt(sg);
                if (!pos_finite(sg)) sigbad = 1;      // (its own word: flag is only read in this phase)
            }
        }
    }
    __syncthreads();
    if (flag != 0 || sigbad != 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int e = t; e < n * n; e += kThreads) { Rg[e] = nan; Rig[e] = nan; }
        if (t < n) lamg[t] = nan;
        if (t == 0) { bad[c] = 1; atomicOr(fail, 1); }
        return;
    }
    if (t == 0) bad[c] = 0;

    // ---- column j of the staging copy in Rinv_all = row j of Rinv = (lisqrt_j / sigma_j) g_j' L2'; R = (L1 V) lisqrt in R_all; not
    // sorted yet
    // (neighbouring lanes take neighbouring i: the reads of L2 and the stores are contiguous, column j of G is a broadcast; each
    // entry is the small kernel's sum over k = 0 .. i in the same order)
    for (int e = t; e < n * n; e += kThreads) {
        const int i = e % n, j = e / n;
        double acc = 0.0;
        for (int k = 0; k <= i; k++) acc += M[k + j * ld] * B[i + k * n];
        Rig[e] = acc * (lis[j] / sig[j]);
    }
    for (int e = t; e < n * n; e += kThreads) {
        const int i = e % n, j = e / n;
        double acc = 0.0;
        for (int k = 0; k <= i; k++) acc += A[i + k * n] * V[k + j * n];
        Rg[e] = acc * lis[j];
    }
    __syncthreads();      // (L1, L2, V and G are consumed; the staging copies are visible to the workgroup)
    for (int e = t; e < n * n; e += kThreads) {
        const int i = e % n, j = e / n;
        A[e] = svec_entry(s_all + K.row0, i, j);      // S, Z again
        B[e] = svec_entry(z_all + K.row0, i, j);
        const double r = Rg[e];
        V[e] = r;                                     // R, Rinv' unsorted: the outputs below overwrite R_all / Rinv_all in sorted order
        T[e] = Rig[e];
        M[i + j * ld] = r;
    }
    __syncthreads();

    // ---- the refinement of lambda (scaling_psd.hip): lambda_j^2 = (r_j' Z r_j)(q_j' S q_j) / (q_j' r_j)^2 in twice the precision, four
    // lanes per column, lane l the rows l, l + 4, ..; the three sums are independent accumulators, so the two passes (M = R, then
    // M = Rinv') change no bit.  Row i of the symmetric S / Z is read as column i.
    const int jc = t >> 2, lc = t & 3;
    double h1 = 0.0, l1 = 0.0, h2 = 0.0, l2 = 0.0, h3 = 0.0, l3 = 0.0;
    if (jc < n) {
        const double *rj = M + jc * ld, *qj = T + jc * n;
        for (int i = lc; i < n; i += 4) {
            const double *zi = B + i * n;
            double yh = 0.0, yl = 0.0;      // y = (Z r_j)_i
            for (int k = 0; k < n; k++) dot2_step(zi[k], rj[k], yh, yl);
            dot2_step_pair(rj[i], yh, yl, h1, l1);
            dot2_step(qj[i], rj[i], h3, l3);
        }
    }
    __syncthreads();
    ws_to_lds(M, T, n, ld);
    __syncthreads();
    double lamj = 0.0, fa = 1.0, fb = 1.0;
    if (jc < n) {
        const double *qj = M + jc * ld;
        for (int i = lc; i < n; i += 4) {
            const double *si = A + i * n;
            double wh = 0.0, wl = 0.0;      // w = (S q_j)_i
            for (int k = 0; k < n; k++) dot2_step(si[k], qj[k], wh, wl);
            dot2_step_pair(qj[i], wh, wl, h2, l2);
        }
        sum4_pair(h1, l1); sum4_pair(h2, l2); sum4_pair(h3, l3);
        // sqrt of the product of two pairs, then the division by the third
        double p = h1 * h2, e = fma(h1, h2, -p);
        e = e + (h1 * l2 + l1 * h2);
        const double x0 = sqrt(p);
        const double x = x0 + (fma(-x0, x0, p) + e) / (2.0 * x0);
        double v = x / h3;
        v = v - v * (l3 / h3);
        lamj = sig[jc];
        if (pos_finite(v) && pos_finite(h1) && pos_finite(h2)) { lamj = v; fa = sqrt(v / h1); fb = sqrt(v / h2); }
    }
    __syncthreads();      // (every read of sig[] above is done)
    if (jc < n && lc == 0) { sig[jc] = lamj; lis[jc] = fa; red2[jc] = fb; }
    __syncthreads();
    // ---- the descending order by counting (ties by index: a bijection), the outputs to their sorted positions
    if (t < n) {
        const double sj = sig[t];
        int rk = 0;
        for (int i = 0; i < n; i++) rk += (sig[i] > sj || (sig[i] == sj && i < t)) ? 1 : 0;
        rank[t] = rk;
        lamg[rk] = sj;
    }
    __syncthreads();
    for (int e = t; e < n * n; e += kThreads) {
        const int i = e % n, j = e / n;
        Rg[i + rank[j] * n] = V[e] * lis[j];
        Rig[rank[j] + i * n] = T[e] * red2[j];
    }
}

// the cones of P.large (side lmin .. 128): (R, Rinv, lam) of the same layout as launch_psd_nt_scaling, which is given lmin - 1 as its
// largest side in the same call
void launch_psd_large_nt_scaling(hipStream_t st, const PsdView &P, const double *s, const double *z, double *R, double *Rinv,
                                 double *lam, int *bad, int *fail) {
    const PsdLargeBatch &L = P.large;
    if (L.nlarge <= 0) return;
    hipLaunchKernelGGL(k_psdl_nt_scaling, dim3(L.nlarge), dim3(kThreads), 0, st, P.tab, L.lidx, L.lmin, s, z, R, Rinv, lam, L.ws, bad, fail);
}

}  // namespace hipkkt
