// The cone algebra of one interior-point step on the rows of PSD triangle cones (opt-in, hipkkt_step_enable_psd), from the caller's
// factors (R, Rinv, lambda) of the Nesterov-Todd scaling -- the Cholesky / SVD of update_scaling! stay with the caller
// (coneops_psdtrianglecone.jl:78-143).  X = svec_to_mat of a cone's rows (1 / sqrt 2 on the off-diagonals), results go back through
// mat_to_svec (:469-497).
//   affine_ds            lambda_k^2 at the diagonal positions, 0 elsewhere                     :190-205
//   mul_W / mul_Winv     :N  A' X A,  :T  A X A'  with A = R resp. Rinv                        :409-437
//   mul_Hs               W'(W x)                                                               :164-187
//   combined_ds_shift    A = W dz, B = W^-T ds, svec((B A + A B) / 2) - sigma mu on the diagonal  coneops_symmetric_common.jl:1-35
//   ds_from_dz_offset    X~_ij = 2 DS_ij / (lambda_i + lambda_j), out = R X~ R'                 coneops_symmetric_common.jl:39-52
//   step_length          D = R' dZ R resp. Rinv dS Rinv', M = Lambda^-1/2 D Lambda^-1/2, gamma = lambda_min(M),
//                        alpha = gamma < 0 ? min(1 / -gamma, alpha_max) : alpha_max                :230-254, :439-466
// One 256-thread workgroup per cone and operation (step length: per cone and per z / s), the factor, X and a work matrix in LDS
// (column-major, leading dimension n + 1 when n is a multiple of 32: the column reads of A' would otherwise hit the same banks).
// Products are plain FP64 FMA chains, every k-sum in ascending order: deterministic.  The smallest eigenvalue comes from a cyclic
// two-sided Jacobi iteration in LDS (psd_cone.h psd_jacobi_sweeps: round-robin sets of disjoint rotations, at most kPsdMaxSweeps
// sweeps); a non-finite M gives a NaN gamma and therefore alpha_max, as the reference's `gamma < 0` does.  No assert, no trap, every
// loop has a fixed trip bound.
// The cone table: cone_layout.h kPsd* ([row0 | n | offset of the n x n factors | offset of lambda]); n <= kMaxN is the enable's condition
// and is checked again here (a larger cone is left alone).  The entry expressions of svec_to_mat, mat_to_svec, their round trip and
// affine_ds are psd_cone.h's, which step_psd_large.hip calls as well; the launchers take the tables as one PsdView (kernels.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cone_layout.h"
#include "cone_reduce.h"
#include "kernels.h"
#include "psd_cone.h"

namespace hipkkt {

namespace {

// the matrix layout, the cone record (Cone, cone_of), load_svec and the entry expressions of the loops below: psd_cone.h
constexpr int kMaxN = kPsdMaxN;
constexpr int kMatDoubles = kPsdMatDoubles;

// F = the cone's n x n column-major factor
__device__ __forceinline__ void load_factor(double *F, const double *__restrict__ src, const Cone &K) {
    const int n = K.n;
    for (int e = threadIdx.x; e < n * n; e += 256) { const int i = e % n, j = e / n; F[i + j * K.ld] = src[e]; }
}
// out = mat_to_svec(Y); diag_add goes to the diagonal positions; addc != NULL: out = -(out + addc)
__device__ __forceinline__ void store_svec(double *__restrict__ out, const double *Y, const Cone &K, double diag_add,
                                           const double *__restrict__ addc) {
    const int n = K.n;
    for (int e = threadIdx.x; e < n * n; e += 256) store_svec_entry(out, Y, n, K.ld, e, diag_add, addc);
}
// Y <- svec_to_mat(mat_to_svec(Y)): what a result of mul_W goes through before the next operation reads it as a matrix
__device__ __forceinline__ void svec_round_trip(double *Y, const Cone &K) {
    const int n = K.n;
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const int i = e % n, j = e / n;
        if (i >= j) continue;
        const double v = round_trip_pair(Y[i + j * K.ld], Y[j + i * K.ld]);
        Y[i + j * K.ld] = v;
        Y[j + i * K.ld] = v;
    }
}
// X <- A' X A (transpose = false) resp. A X A' (transpose = true); T is the work matrix.  Every thread of the workgroup calls it.
__device__ __forceinline__ void triple(const double *A, double *X, double *T, const Cone &K, bool transpose) {
    const int n = K.n, ld = K.ld;
    __syncthreads();
    for (int e = threadIdx.x; e < n * n; e += 256) {      // T = X A resp. X A'
        const int i = e % n, j = e / n;
        double acc = 0.0;
        if (!transpose) for (int k = 0; k < n; k++) acc = fma(X[i + k * ld], A[k + j * ld], acc);
        else for (int k = 0; k < n; k++) acc = fma(X[i + k * ld], A[j + k * ld], acc);
        T[i + j * ld] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n * n; e += 256) {      // X = A' T resp. A T
        const int i = e % n, j = e / n;
        double acc = 0.0;
        if (!transpose) for (int k = 0; k < n; k++) acc = fma(A[k + i * ld], T[k + j * ld], acc);
        else for (int k = 0; k < n; k++) acc = fma(A[i + k * ld], T[k + j * ld], acc);
        X[i + j * ld] = acc;
    }
    __syncthreads();
}

}  // namespace

// ---- affine_ds --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_psd_affine_ds(const int64_t *__restrict__ tab, const double *__restrict__ lam_all, double *__restrict__ out_all) {
    const Cone K = cone_of(tab, blockIdx.x);
    if (!K.ok) return;
    const int n = K.n;
    for (int e = threadIdx.x; e < n * n; e += 256) affine_ds_entry(out_all + K.row0, lam_all + K.loff, n, e);
}

// ---- mul_Hs; with addc != NULL: y = -(Hs x + addc) -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_psd_mulhs(const int64_t *__restrict__ tab, const double *__restrict__ R_all, const double *__restrict__ x_all,
            const double *__restrict__ addc_all, double *__restrict__ y_all) {
    __shared__ double F[kMatDoubles], X[kMatDoubles], T[kMatDoubles];
    const Cone K = cone_of(tab, blockIdx.x);
    if (!K.ok) return;
    load_factor(F, R_all + K.foff, K);
    load_svec(X, x_all + K.row0, K);
    triple(F, X, T, K, false);
    svec_round_trip(X, K);
    triple(F, X, T, K, true);
    store_svec(y_all + K.row0, X, K, 0.0, addc_all ? addc_all + K.row0 : nullptr);
}

// ---- combined_ds_shift ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_psd_shift(const int64_t *__restrict__ tab, const double *__restrict__ R_all, const double *__restrict__ Rinv_all,
            const double *__restrict__ dz_all, const double *__restrict__ ds_all, double sigma_mu, double *__restrict__ out_all) {
    __shared__ double F[kMatDoubles], A[kMatDoubles], B[kMatDoubles], T[kMatDoubles];
    const Cone K = cone_of(tab, blockIdx.x);
    if (!K.ok) return;
    const int n = K.n, ld = K.ld;
    load_factor(F, R_all + K.foff, K);
    load_svec(A, dz_all + K.row0, K);
    triple(F, A, T, K, false);               // A = W dz
    svec_round_trip(A, K);
    __syncthreads();
    load_factor(F, Rinv_all + K.foff, K);
    load_svec(B, ds_all + K.row0, K);
    triple(F, B, T, K, true);                // B = W^-T ds
    svec_round_trip(B, K);
    __syncthreads();
    for (int e = threadIdx.x; e < n * n; e += 256) {      // circ_op: (B A + A B) / 2
        const int i = e % n, j = e / n;
        double ba = 0.0, ab = 0.0;
        for (int k = 0; k < n; k++) {
            ba = fma(B[i + k * ld], A[k + j * ld], ba);
            ab = fma(A[i + k * ld], B[k + j * ld], ab);
        }
        T[i + j * ld] = 0.5 * (ba + ab);
    }
    __syncthreads();
    store_svec(out_all + K.row0, T, K, -sigma_mu, nullptr);
}

// ---- ds_from_dz_offset ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_psd_offset(const int64_t *__restrict__ tab, const double *__restrict__ R_all, const double *__restrict__ lam_all,
             const double *__restrict__ ds_all, double *__restrict__ out_all) {
    __shared__ double F[kMatDoubles], X[kMatDoubles], T[kMatDoubles];
    const Cone K = cone_of(tab, blockIdx.x);
    if (!K.ok) return;
    const int n = K.n, ld = K.ld;
    const double *lam = lam_all + K.loff;
    load_factor(F, R_all + K.foff, K);
    load_svec(X, ds_all + K.row0, K);
    __syncthreads();
    for (int e = threadIdx.x; e < n * n; e += 256) {      // lambda_inv_circ_op (every thread rewrites its own entry)
        const int i = e % n, j = e / n;
        X[i + j * ld] = 2.0 * X[i + j * ld] / (lam[i] + lam[j]);
    }
    __syncthreads();
    svec_round_trip(X, K);
    triple(F, X, T, K, true);
    store_svec(out_all + K.row0, X, K, 0.0, nullptr);
}

// ---- step_length -------------------------------------------------------------------------------------------------------------------
// blockIdx.y = 0: z with R (:N), 1: s with Rinv (:T).  part[2 c + blockIdx.y] = the cone's alpha.
__global__ void __launch_bounds__(256)
k_psd_len(const int64_t *__restrict__ tab, const double *__restrict__ R_all, const double *__restrict__ Rinv_all,
          const double *__restrict__ lam_all, const double *__restrict__ dz_all, const double *__restrict__ ds_all, double alpha_max,
          double *__restrict__ part) {
    __shared__ double F[kMatDoubles], M[kMatDoubles], T[kMatDoubles];
    __shared__ double red[4], rc[kMaxN / 2], rs[kMaxN / 2];      // rs = the rotations' s, rc = their s / (1 + c)
    __shared__ int rp[kMaxN / 2], rq[kMaxN / 2];                  // and their index pairs p < q
    const int c = blockIdx.x, which = blockIdx.y, t = threadIdx.x;
    const Cone K = cone_of(tab, c);
    if (!K.ok) { if (t == 0) part[2 * c + which] = alpha_max; return; }
    const int n = K.n, ld = K.ld;
    const double *lam = lam_all + K.loff;
    load_factor(F, (which ? Rinv_all : R_all) + K.foff, K);
    load_svec(M, (which ? ds_all : dz_all) + K.row0, K);
    triple(F, M, T, K, which != 0);
    svec_round_trip(M, K);
    __syncthreads();
    double tot2 = 0.0;
    for (int e = t; e < n * n; e += 256) {                // M = Lambda^-1/2 D Lambda^-1/2
        const int i = e % n, j = e / n;
        const double v = ((1.0 / sqrt(lam[i])) * M[i + j * ld]) * (1.0 / sqrt(lam[j]));
        M[i + j * ld] = v;
        tot2 += v * v;
    }
    tot2 = block_sum(tot2, red);                          // (its barriers order the writes above before the reads below)
    // cyclic Jacobi sweeps until off(M) <= eps |M|_F (psd_cone.h, shared with the default start's margins); a non-finite |M|_F skips them
    const bool finite = psd_jacobi_sweeps(M, K, tot2, red, rc, rs, rp, rq);
    double g = finite ? 1.7976931348623157e308 : tot2 - tot2;      // (a non-finite M: gamma = NaN)
    if (finite) for (int i = t; i < n; i += 256) g = nan_min(M[i + i * ld], g);
    g = block_nan_min(g, red);
    if (t == 0) part[2 * c + which] = g < 0.0 ? fmin(1.0 / (-g), alpha_max) : alpha_max;
}
// out2 = min(the symmetric cones' pair, every PSD cone's pair)
__global__ void __launch_bounds__(256)
k_psd_len_final(const double *__restrict__ part, int npsd, const double *__restrict__ sym2, double *__restrict__ out2) {
    __shared__ double red[4];
    double az = sym2[0], as = sym2[1];
    for (int k = threadIdx.x; k < npsd; k += 256) { az = fmin(az, part[2 * k]); as = fmin(as, part[2 * k + 1]); }
    for (int o = 32; o > 0; o >>= 1) { az = fmin(az, __shfl_down(az, o)); as = fmin(as, __shfl_down(as, o)); }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = az;
    __syncthreads();
    az = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = as;
    __syncthreads();
    as = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    if (threadIdx.x == 0) { out2[0] = az; out2[1] = as; }
}

// ---- the factors' check: a lambda that is not finite or not positive fails the scaling ------------------------------------------------
__global__ void __launch_bounds__(256)
k_psd_check_lambda(const double *__restrict__ lam, int64_t len, int *__restrict__ fail) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const double l = lam[i];
    if (!(l > 0.0) || !(l - l == 0.0)) atomicOr(fail, 1);
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
int psd_step_max_dim() { return kMaxN; }

void launch_psd_step_affine_ds(hipStream_t st, const PsdView &P, double *out) {
    if (P.npsd > 0) hipLaunchKernelGGL(k_psd_affine_ds, dim3(P.npsd), dim3(256), 0, st, P.tab, P.lam, out);
}
void launch_psd_step_mulhs(hipStream_t st, const PsdView &P, const double *x, const double *addc, double *y) {
    if (P.npsd > 0) hipLaunchKernelGGL(k_psd_mulhs, dim3(P.npsd), dim3(256), 0, st, P.tab, P.R, x, addc, y);
}
void launch_psd_step_shift(hipStream_t st, const PsdView &P, const double *dz, const double *ds, double sigma_mu, double *out) {
    if (P.npsd > 0) hipLaunchKernelGGL(k_psd_shift, dim3(P.npsd), dim3(256), 0, st, P.tab, P.R, P.Rinv, dz, ds, sigma_mu, out);
}
void launch_psd_step_offset(hipStream_t st, const PsdView &P, const double *ds, double *out) {
    if (P.npsd > 0) hipLaunchKernelGGL(k_psd_offset, dim3(P.npsd), dim3(256), 0, st, P.tab, P.R, P.lam, ds, out);
}
void launch_psd_step_length_cones(hipStream_t st, const PsdView &P, const double *dz, const double *ds, double alpha_max, double *part) {
    if (P.npsd > 0) hipLaunchKernelGGL(k_psd_len, dim3(P.npsd, 2), dim3(256), 0, st, P.tab, P.R, P.Rinv, P.lam, dz, ds, alpha_max, part);
}
void launch_psd_step_length_final(hipStream_t st, int npsd, const double *sym2, const double *part, double *out2) {
    if (npsd > 0) hipLaunchKernelGGL(k_psd_len_final, dim3(1), dim3(256), 0, st, part, npsd, sym2, out2);
}
void launch_psd_step_check(hipStream_t st, const double *lam, int64_t len, int *fail) {
    if (len > 0) hipLaunchKernelGGL(k_psd_check_lambda, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, lam, len, fail);
}

}  // namespace hipkkt
