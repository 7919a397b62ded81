// The barrier of PSD triangle cones on the device: compute_barrier / _logdet_barrier, coneops_psdtrianglecone.jl:256-290, which a cone set
// with a non-symmetric member searches in every Dual-strategy iteration (hipkkt_step_enable_mixed; a symmetric set never asks for it).
//   Q = svec_to_mat(x + alpha dx)         one product and one sum per entry, off-diagonal entries times 1 / sqrt(2) as load_svec forms them
//   Q = L L'                              right-looking lower Cholesky in place: entry (i, k) receives a_ik - l_i0 l_k0 - l_i1 l_k1 - .. in
//                                         ascending order; a pivot that is not > 0 or not finite ends it, as cholesky!(check = false) does
//   logdet = dd + dd, dd = sum_j log l_jj one thread, ascending j, plain log: logdet(::Cholesky).  A failed factorisation gives +Inf
//   barrier = (0 - logdet_z) - logdet_s   so a shifted point outside the cone gives -Inf, the reference's `barrier -= typemax(T)`
// One 256-thread workgroup per (cone, candidate, side z | s) with one n x n matrix in LDS (psd_cone.h: column-major, leading dimension
// n + 1 when n % 32 == 0; 33 280 B at n = 64, four workgroups per CU by LDS).  Few PSD cones times at most 8 candidates is a small grid on
// 256 CUs, so the two sides run as workgroups of their own and leave two slots [(0 - logdet_z) | logdet_s] per (cone, candidate);
// k_bar_psd_add, one workgroup behind k_bar_final, subtracts the second from the first and adds the cones' terms in PSD-cone order to
// out[2 j].  The shifted dot out[2 j + 1] is k_bar_rows's over all rows and needs nothing here.
// No assert, no trap, no spin, every loop bounded by n.  Every thread reads the same pivot from LDS, so the exit is uniform; a NaN in
// the input reaches a pivot and takes the failure arm.  Compiled with -ffp-contract=off: tests/psd_barrier_reference.py emulates the
// order of the subtractions and of the log sum.
// A cone of side 65 .. 128 (hipkkt_step_enable_mixed_large, the cones of P.large) takes the failure arm of k_bar_psd; k_bar_psd_large
// behind it on the same stream overwrites those two slots: the same expressions in the same order with one 128 x 129 matrix in LDS
// (132 096 B, one workgroup per CU, the budget of start.hip's k_start_margin_psd_large) and 512 threads as 128 row lanes x 4 column
// groups.  The rows of one column are disjoint across lanes and each entry's subtractions stay in ascending j, so applied to a side
// <= 64 it gives the bits of k_bar_psd (tests/test_gpu_mixed_step_large.py holds it to that through the testing switch PSD_LARGE_MIN).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cone_layout.h"
#include "kernels.h"
#include "psd_cone.h"

namespace hipkkt {

namespace {

constexpr int kBarPsdMax = 8;      // candidates per launch: step3_max_candidates()
constexpr int kBarPsdSlots = 2 * kBarPsdMax;      // doubles per PSD cone: [(0 - logdet_z) | logdet_s] per candidate

struct BarPsdAlphas { double a[kBarPsdMax]; };      // (pos_finite of the pivot test: psd_cone.h)

}  // namespace

// grid (npsd, nalpha, 2): blockIdx.z = 0 the z side, 1 the s side
__global__ void __launch_bounds__(256)
k_bar_psd(const int64_t *__restrict__ tab, const double *__restrict__ z_all, const double *__restrict__ s_all,
          const double *__restrict__ dz_all, const double *__restrict__ ds_all, BarPsdAlphas A, double *__restrict__ slots) {
    __shared__ double Q[kPsdMatDoubles];
    const int c = blockIdx.x, cand = blockIdx.y, side = blockIdx.z, t = threadIdx.x;
    const Cone K = cone_of(tab, c);
    double *slot = slots + (int64_t)c * kBarPsdSlots + 2 * cand + side;
    if (!K.ok) {      // (the enable admits no such cone) nothing is factored: the failure arm
        if (t == 0) *slot = side ? __builtin_huge_val() : 0.0 - __builtin_huge_val();
        return;
    }
    const int n = K.n, ld = K.ld;
    const double *x = (side ? s_all : z_all) + K.row0, *dx = (side ? ds_all : dz_all) + K.row0;
    const double a = A.a[cand];
    // the lower triangle of Q = svec_to_mat(x + a dx); the upper one is never read
    for (int e = t; e < n * n; e += 256) {
        const int i = e % n, j = e / n;
        if (i < j) continue;
        const int idx = i * (i + 1) / 2 + j;
        const double v = x[idx] + a * dx[idx];
        Q[i + j * ld] = i == j ? v : v * kPsdIsqrt2;
    }
    __syncthreads();
    // right-looking: the diagonal keeps the pivot d_j = l_jj^2 until the log sum
    bool ok = true;
    for (int j = 0; j < n; j++) {
        const double d = Q[j + j * ld];      // the same value in every thread
        if (!pos_finite(d)) { ok = false; break; }
        const double piv = sqrt(d);
        for (int i = j + 1 + t; i < n; i += 256) Q[i + j * ld] = Q[i + j * ld] / piv;
        __syncthreads();
        {
            const int i = j + 1 + (t & 63);
            if (i < n) {
                const double li = Q[i + j * ld];
                for (int k = j + 1 + (t >> 6); k <= i; k += 4) Q[i + k * ld] = Q[i + k * ld] - li * Q[k + j * ld];
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        double logdet = __builtin_huge_val();
        if (ok) {
            double dd = 0.0;
            for (int j = 0; j < n; j++) dd += log(sqrt(Q[j + j * ld]));
            logdet = dd + dd;
        }
        *slot = side ? logdet : 0.0 - logdet;
    }
}

// grid (nlarge, nalpha, 2): the cones lidx[0 .. nlarge) of the table, sides lmin .. kPsdLargeMaxN; k_bar_psd statement by statement but
// for the lane map of the update: row i = j + 1 + (t mod 128), columns k = j + 1 + t / 128 + 4 q.  Consecutive lanes read consecutive
// rows of a column (no bank conflict with the padded leading dimension) and the same Q[k + j ld] (a broadcast)
__global__ void __launch_bounds__(512)
k_bar_psd_large(const int64_t *__restrict__ tab, const int *__restrict__ lidx, int lmin, const double *__restrict__ z_all,
                const double *__restrict__ s_all, const double *__restrict__ dz_all, const double *__restrict__ ds_all, BarPsdAlphas A,
                double *__restrict__ slots) {
    __shared__ double Q[kPsdLargeMaxN * (kPsdLargeMaxN + 1)];
    const int c = lidx[blockIdx.x], cand = blockIdx.y, side = blockIdx.z, t = threadIdx.x;
    const Cone K = cone_of(tab, c, lmin, kPsdLargeMaxN);
    if (!K.ok) return;      // (the list holds no such cone) the slot keeps what k_bar_psd left
    double *slot = slots + (int64_t)c * kBarPsdSlots + 2 * cand + side;
    const int n = K.n, ld = K.ld;
    const double *x = (side ? s_all : z_all) + K.row0, *dx = (side ? ds_all : dz_all) + K.row0;
    const double a = A.a[cand];
    for (int e = t; e < n * n; e += 512) {
        const int i = e % n, j = e / n;
        if (i < j) continue;
        const int idx = i * (i + 1) / 2 + j;
        const double v = x[idx] + a * dx[idx];
        Q[i + j * ld] = i == j ? v : v * kPsdIsqrt2;
    }
    __syncthreads();
    bool ok = true;
    for (int j = 0; j < n; j++) {
        const double d = Q[j + j * ld];      // the same value in every thread
        if (!pos_finite(d)) { ok = false; break; }
        const double piv = sqrt(d);
        for (int i = j + 1 + t; i < n; i += 512) Q[i + j * ld] = Q[i + j * ld] / piv;
        __syncthreads();
        {
            const int i = j + 1 + (t & 127);
            if (i < n) {
                const double li = Q[i + j * ld];
                for (int k = j + 1 + (t >> 7); k <= i; k += 4) Q[i + k * ld] = Q[i + k * ld] - li * Q[k + j * ld];
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        double logdet = __builtin_huge_val();
        if (ok) {
            double dd = 0.0;
            for (int j = 0; j < n; j++) dd += log(sqrt(Q[j + j * ld]));
            logdet = dd + dd;
        }
        *slot = side ? logdet : 0.0 - logdet;
    }
}

// out[2 j] += sum over the PSD cones, in their order, of (0 - logdet_z) - logdet_s; thread j owns candidate j
__global__ void __launch_bounds__(64)
k_bar_psd_add(const double *__restrict__ slots, int npsd, int nalpha, double *__restrict__ out) {
    const int j = threadIdx.x;
    if (j >= nalpha) return;
    double acc = out[2 * j];
    for (int c = 0; c < npsd; c++) {
        const double *p = slots + (int64_t)c * kBarPsdSlots + 2 * j;
        acc += p[0] - p[1];
    }
    out[2 * j] = acc;
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
// the PSD cones' slots in the barrier's work buffer, behind the Generalized Power cones' partials: step3_barrier_doubles(ncones) holds
// 16 doubles per registered cone behind the row slices, of which a second-order, three-row or Generalized Power cone takes 8 and a PSD
// cone these 16
double *psd_barrier_slots(double *work, int nsoc, int n3, int ngp) {
    return step3_barrier_gppart(work, nsoc, n3) + (int64_t)kBarPsdMax * (ngp > 0 ? ngp : 0);
}
void launch_psd_barrier(hipStream_t st, const PsdView &P, const double *z, const double *s, const double *dz, const double *ds,
                        const double *alphas, int nalpha, double *slots) {
    if (P.npsd <= 0 || nalpha <= 0) return;
    if (nalpha > kBarPsdMax) nalpha = kBarPsdMax;
    BarPsdAlphas A;
    for (int j = 0; j < kBarPsdMax; j++) A.a[j] = j < nalpha ? alphas[j] : 0.0;
    hipLaunchKernelGGL(k_bar_psd, dim3(P.npsd, nalpha, 2), dim3(256), 0, st, P.tab, z, s, dz, ds, A, slots);
}
void launch_psd_barrier_large(hipStream_t st, const PsdView &P, const double *z, const double *s, const double *dz, const double *ds,
                              const double *alphas, int nalpha, double *slots) {
    if (P.large.nlarge <= 0 || nalpha <= 0) return;
    if (nalpha > kBarPsdMax) nalpha = kBarPsdMax;
    BarPsdAlphas A;
    for (int j = 0; j < kBarPsdMax; j++) A.a[j] = j < nalpha ? alphas[j] : 0.0;
    hipLaunchKernelGGL(k_bar_psd_large, dim3(P.large.nlarge, nalpha, 2), dim3(512), 0, st, P.tab, P.large.lidx, P.large.lmin, z, s, dz, ds,
                       A, slots);
}
void launch_psd_barrier_add(hipStream_t st, int npsd, const double *slots, int nalpha, double *out) {
    if (npsd <= 0 || nalpha <= 0) return;
    if (nalpha > kBarPsdMax) nalpha = kBarPsdMax;
    hipLaunchKernelGGL(k_bar_psd_add, dim3(1), dim3(64), 0, st, slots, npsd, nalpha, out);
}

}  // namespace hipkkt
