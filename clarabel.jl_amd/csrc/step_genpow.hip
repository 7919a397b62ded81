// The cone algebra of one interior-point step for the Generalized Power cones on the device (coneops_genpowcone.jl), next to step.hip
// (Zero / Nonnegative / SecondOrder) and step_cone3.hip (Exponential / Power).  Everything works on what hipkkt_update_scaling_ex[_dev]
// left resident: (s, z), the cone's slot [grad (dim) | d1 (dim1) | d2 | p (dim) | q (dim1) | r (dim2)] written by k_scaling_genpow, the
// descriptor table (cone_layout.h kGp*) and the exponents.
//   affine_ds            ds = s                                                                        :137-147
//   ds_from_dz_offset    out = ds                                                                      :170-183
//   combined_ds_shift    grad sigma mu (no third-order correction)                                     :149-168
//   mul_Hs               mu (D x + (p.x) p - (q.x1) q - (r.x2) r)                                      :111-135
//   step_length          backtrack_search on is_dual_feasible(z + alpha dz), is_primal_feasible(s + alpha ds)   :186-207, :249-292
//   compute_barrier      barrier_dual + barrier_primal (gradient_primal!, _newton_raphson_genpowcone)  :209-234, :294-333, :393-472
// One wavefront (= one workgroup of 64) per cone, as k_scaling_genpow; loops over dim1 and dim2 are strided by 64.  Sums and products
// over a cone are butterfly reductions, so every lane holds the same value and every branch on one (feasible or not, the Newton halt,
// the exit of the backtracking loop) is uniform over the wavefront.  Expressions keep the reference's association except for the
// order inside a reduction (-ffp-contract=off).  No assert, no trap: the backtracking loop is bounded by the trip count the host
// derives from (step, alpha_min), the Newton iteration by the reference's 100 steps (coneops_nonsymmetric_common.jl:170-192); a point
// outside the cone gives what logsafe gives.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cone3_math.h"
#include "cone_layout.h"
#include "cone_reduce.h"
#include "kernels.h"

namespace hipkkt {

namespace {

constexpr int kGpBarMax = 8;          // candidates per launch (step3_max_candidates())
constexpr double kEps = 2.220446049250313e-16;

struct GpCone { int64_t row0, dim1, dim2, out0; const double *a; double psi; };
__device__ __forceinline__ GpCone gp_cone(const int64_t *desc, const double *alpha_all, int c) {
    const int64_t *d = desc + kGpDesc * (int64_t)c;
    GpCone K{d[kGpRow0], d[kGpDim1], d[kGpDim2], d[kGpOut0], alpha_all + d[kGpAlpha0], 0.0};
    K.psi = __longlong_as_double(d[kGpPsiBits]);      // 1 / <alpha, alpha> (cone_types.jl GenPowerConeData), the host's bits
    return K;
}

// is_dual_feasible / is_primal_feasible at q + alpha dq, :249-292
template <bool DUAL>
__device__ __forceinline__ bool gp_feasible(const GpCone &K, const double *q, const double *dq, double alpha, int t) {
    int bad = 0;
    double res = 0.0, n2 = 0.0;
    for (int64_t i = t; i < K.dim1; i += 64) {
        const double v = q[i] + alpha * dq[i];
        if (!(v > 0.0)) bad = 1;
        res += DUAL ? 2.0 * K.a[i] * logsafe(v / K.a[i]) : 2.0 * K.a[i] * logsafe(v);
    }
    for (int64_t i = t; i < K.dim2; i += 64) {
        const double w = q[K.dim1 + i] + alpha * dq[K.dim1 + i];
        n2 += w * w;
    }
    bad = wave_or(bad);
    res = wave_sum(res);
    n2 = wave_sum(n2);
    if (bad) return false;
    return exp(res) - n2 > 0.0;
}

// backtrack_search, coneops_nonsymmetric_common.jl:5-33, with the loop bounded by `trips`; every exit is uniform over the wavefront
template <bool DUAL>
__device__ __forceinline__ double gp_backtrack(const GpCone &K, const double *q, const double *dq, double alpha0, double alpha_min,
                                               double step, int trips, int t) {
    double alpha = alpha0;
    for (int k = 0; k < trips; k++) {
        if (gp_feasible<DUAL>(K, q, dq, alpha, t)) return alpha;
        alpha *= step;
        if (alpha < alpha_min) return 0.0;
    }
    return 0.0;
}

// barrier_dual at z + al dz, :313-333
__device__ __forceinline__ double gp_barrier_dual(const GpCone &K, const double *z, const double *dz, double al, int t) {
    double res = 0.0, n2 = 0.0, lg = 0.0;
    for (int64_t i = t; i < K.dim1; i += 64) {
        const double v = z[i] + al * dz[i];
        res += 2.0 * K.a[i] * logsafe(v / K.a[i]);
        lg += (1.0 - K.a[i]) * logsafe(v);
    }
    for (int64_t i = t; i < K.dim2; i += 64) {
        const double w = z[K.dim1 + i] + al * dz[K.dim1 + i];
        n2 += w * w;
    }
    res = wave_sum(res);
    n2 = wave_sum(n2);
    lg = wave_sum(lg);
    return -logsafe(exp(res) - n2) - lg;
}

// _newton_raphson_genpowcone, :437-472, with the halting rule of _newton_raphson_onesided; p = (s + al ds)[0 .. dim1)
__device__ __forceinline__ double gp_newton(const GpCone &K, const double *s, const double *ds, double al, double norm_r, double phi,
                                            int t) {
    const double psi = K.psi;
    double x = -1.0 / norm_r + (psi * norm_r + sqrt((phi / norm_r / norm_r + psi * psi - 1.0) * phi)) / (phi - norm_r * norm_r);
    for (int it = 0; it < 100; it++) {
        double f0 = 0.0, f1 = 0.0;
        for (int64_t i = t; i < K.dim1; i += 64) {
            const double a = K.a[i], p = s[i] + al * ds[i];
            f0 += 2.0 * a * (logsafe(x * norm_r + (1.0 + a) / a) - logsafe(p));
            f1 += 2.0 * a * norm_r / (norm_r * x + (1.0 + a) / a);
        }
        f0 = -logsafe(2.0 * x / norm_r + x * x) + wave_sum(f0);
        const double dfdx = -(2.0 * x + 2.0 / norm_r) / (x * x + 2.0 * x / norm_r) + wave_sum(f1);
        const double dx = -f0 / dfdx;
        if (dx < kEps || fabs(dx / x) < kSqrtEps || fabs(dfdx) < kEps) break;      // (uniform: f0, dfdx come from butterflies)
        x += dx;
    }
    return x;
}

// barrier_primal at s + al ds, :294-310: -barrier_dual(-g(s)) - degree with g from gradient_primal!, :393-426
__device__ __forceinline__ double gp_barrier_primal(const GpCone &K, const double *s, const double *ds, double al, int t) {
    double phi = 1.0, n2 = 0.0;
    for (int64_t i = t; i < K.dim1; i += 64) phi *= pow(s[i] + al * ds[i], 2.0 * K.a[i]);
    for (int64_t i = t; i < K.dim2; i += 64) {
        const double w = s[K.dim1 + i] + al * ds[K.dim1 + i];
        n2 += w * w;
    }
    phi = wave_prod(phi);
    const double norm_r = sqrt(wave_sum(n2));
    const bool far = norm_r > kEps;                  // (uniform)
    const double g1 = far ? gp_newton(K, s, ds, al, norm_r, phi, t) : 0.0;
    // barrier_dual(-g): -g[i] = (1 + a + a g1 |r|) / p[i], -g[dim1 + i] = -(g1 r[i] / |r|)
    double res = 0.0, lg = 0.0, m2 = 0.0;
    for (int64_t i = t; i < K.dim1; i += 64) {
        const double a = K.a[i], p = s[i] + al * ds[i];
        const double mg = far ? (1.0 + a + a * g1 * norm_r) / p : (1.0 + a) / p;
        res += 2.0 * a * logsafe(mg / a);
        lg += (1.0 - a) * logsafe(mg);
    }
    if (far)
        for (int64_t i = t; i < K.dim2; i += 64) {
            const double w = s[K.dim1 + i] + al * ds[K.dim1 + i];
            const double gr = g1 * w / norm_r;
            m2 += gr * gr;
        }
    res = wave_sum(res);
    m2 = wave_sum(m2);
    lg = wave_sum(lg);
    const double bd = -logsafe(exp(res) - m2) - lg;
    return -bd - (double)(K.dim1 + 1);
}

struct GpAlphas { double a[kGpBarMax]; int n; };

}  // namespace

// ---- row copies: affine_ds (src = the resident s), ds_from_dz_offset (src = ds) ------------------------------------------------------
__global__ void __launch_bounds__(64)
k_gp_copy(const int64_t *__restrict__ desc, const double *__restrict__ src, double *__restrict__ out) {
    const int64_t *d = desc + kGpDesc * (int64_t)blockIdx.x;
    const int64_t row0 = d[kGpRow0], dim = d[kGpDim1] + d[kGpDim2];
    for (int64_t i = threadIdx.x; i < dim; i += 64) out[row0 + i] = src[row0 + i];
}

// ---- combined_ds_shift ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_gp_shift(const int64_t *__restrict__ desc, const double *__restrict__ nsout, double sigma_mu, double *__restrict__ out) {
    const int64_t *d = desc + kGpDesc * (int64_t)blockIdx.x;
    const int64_t row0 = d[kGpRow0], dim = d[kGpDim1] + d[kGpDim2];
    const double *g = nsout + d[kGpOut0];
    for (int64_t i = threadIdx.x; i < dim; i += 64) out[row0 + i] = g[i] * sigma_mu;
}

// ---- mul_Hs; with addc != NULL: y = -(Hs x + addc) --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_gp_mulhs(const int64_t *__restrict__ desc, const double *__restrict__ nsout, double mu, const double *__restrict__ x_all,
           const double *__restrict__ addc, double *__restrict__ y_all) {
    const int t = threadIdx.x;
    const int64_t *d = desc + kGpDesc * (int64_t)blockIdx.x;
    const int64_t row0 = d[kGpRow0], dim1 = d[kGpDim1], dim2 = d[kGpDim2], dim = dim1 + dim2;
    // (the slot's pointers stay chained, as in k_scaling_genpow)
    const double *g = nsout + d[kGpOut0], *od1 = g + dim, *od2 = od1 + dim1, *p = od2 + 1, *q = p + dim, *r = q + dim1;
    const double *x = x_all + row0;
    double cp = 0.0, cq = 0.0, cr = 0.0;
    for (int64_t i = t; i < dim1; i += 64) { cp += p[i] * x[i]; cq += q[i] * x[i]; }
    for (int64_t i = t; i < dim2; i += 64) { cp += p[dim1 + i] * x[dim1 + i]; cr += r[i] * x[dim1 + i]; }
    cp = wave_sum(cp); cq = wave_sum(cq); cr = wave_sum(cr);
    const double d2 = od2[0];
    for (int64_t i = t; i < dim; i += 64) {
        double v = i < dim1 ? od1[i] * x[i] - cq * q[i] : d2 * x[i] - cr * r[i - dim1];
        v += cp * p[i];
        v *= mu;
        if (addc) v = -(v + addc[row0 + i]);
        y_all[row0 + i] = v;
    }
}

// ---- step_length: part[c] = min(alpha_z, alpha_s) of cone c on the grid alpha0 step^k -------------------------------------------------
__global__ void __launch_bounds__(64)
k_gp_len(const int64_t *__restrict__ desc, const double *__restrict__ alpha_all, const double *__restrict__ z_all,
         const double *__restrict__ s_all, const double *__restrict__ dz_all, const double *__restrict__ ds_all,
         const double *__restrict__ sym2, StepTK T, double alpha_max, double step, double alpha_min, int trips,
         double *__restrict__ part) {
    const int c = blockIdx.x, t = threadIdx.x;
    const GpCone K = gp_cone(desc, alpha_all, c);
    const double a0 = alpha_start(sym2, T, alpha_max);
    const double az = gp_backtrack<true>(K, z_all + K.row0, dz_all + K.row0, a0, alpha_min, step, trips, t);
    const double as = gp_backtrack<false>(K, s_all + K.row0, ds_all + K.row0, a0, alpha_min, step, trips, t);
    if (t == 0) part[c] = fmin(az, as);
}

// ---- compute_barrier: cpart[c * 8 + j] at candidate j ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_gp_barrier(const int64_t *__restrict__ desc, const double *__restrict__ alpha_all, const double *__restrict__ z_all,
             const double *__restrict__ s_all, const double *__restrict__ dz_all, const double *__restrict__ ds_all, GpAlphas A,
             double *__restrict__ cpart) {
    const int c = blockIdx.x, t = threadIdx.x;
    const GpCone K = gp_cone(desc, alpha_all, c);
    for (int j = 0; j < kGpBarMax; j++) {
        if (j >= A.n) break;
        const double bp = gp_barrier_primal(K, s_all + K.row0, ds_all + K.row0, A.a[j], t);
        const double bd = gp_barrier_dual(K, z_all + K.row0, dz_all + K.row0, A.a[j], t);
        if (t == 0) cpart[(int64_t)c * kGpBarMax + j] = bp + bd;
    }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
void launch_genpow_copy(hipStream_t st, int ngp, const int64_t *desc, const double *src, double *out) {
    if (ngp > 0) hipLaunchKernelGGL(k_gp_copy, dim3(ngp), dim3(64), 0, st, desc, src, out);
}
void launch_genpow_shift(hipStream_t st, int ngp, const int64_t *desc, const double *nsout, double sigma_mu, double *out) {
    if (ngp > 0) hipLaunchKernelGGL(k_gp_shift, dim3(ngp), dim3(64), 0, st, desc, nsout, sigma_mu, out);
}
void launch_genpow_mulhs(hipStream_t st, int ngp, const int64_t *desc, const double *nsout, double mu, const double *x, const double *addc,
                         double *y) {
    if (ngp > 0) hipLaunchKernelGGL(k_gp_mulhs, dim3(ngp), dim3(64), 0, st, desc, nsout, mu, x, addc, y);
}
void launch_genpow_length(hipStream_t st, int ngp, const int64_t *desc, const double *alpha, const double *z, const double *s,
                          const double *dz, const double *ds, const double *sym2, const double *dtau, double tau, double kappa,
                          double rhs_kappa, double alpha_max, double step, double alpha_min, int trips, double *part) {
    const StepTK T{dtau, tau, kappa, rhs_kappa};
    if (ngp > 0)
        hipLaunchKernelGGL(k_gp_len, dim3(ngp), dim3(64), 0, st, desc, alpha, z, s, dz, ds, sym2, T, alpha_max, step, alpha_min, trips, part);
}
void launch_genpow_barrier(hipStream_t st, int ngp, const int64_t *desc, const double *alpha, const double *z, const double *s,
                           const double *dz, const double *ds, const double *alphas, int nalpha, double *cpart) {
    GpAlphas A;
    A.n = nalpha < kGpBarMax ? nalpha : kGpBarMax;
    for (int j = 0; j < kGpBarMax; j++) A.a[j] = j < nalpha ? alphas[j] : 0.0;
    if (ngp > 0) hipLaunchKernelGGL(k_gp_barrier, dim3(ngp), dim3(64), 0, st, desc, alpha, z, s, dz, ds, A, cpart);
}

}  // namespace hipkkt
