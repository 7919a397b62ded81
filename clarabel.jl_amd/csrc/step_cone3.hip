// The cone algebra of one interior-point step for the three-row non-symmetric cones (Exponential, Power) on the device, next to
// step.hip's Zero / Nonnegative / SecondOrder kernels, plus the barrier of a whole cone set.  Everything works on what
// hipkkt_update_scaling_ex[_dev] left resident: (s, z) and, per cone, its slot [pack_triu(Hs) | pack_triu(H_dual) | grad] (cone_layout.h).
//   affine_ds            ds = s                                   coneops_expcone.jl / coneops_powcone.jl affine_ds!
//   ds_from_dz_offset    out = ds
//   mul_Hs               y = Hs x with the resident 3 x 3 block (what the matrix holds)      coneops_expcone.jl:103-116
//   combined_ds_shift    grad sigma mu - higher_correction(step_s, step_z)    coneops_expcone.jl:130-148, :319-367, coneops_powcone.jl:329-405
//   step_length          backtracking from alpha0 = min(alpha_tau, alpha_kappa, 1, the symmetric cones, 1 - sqrt(eps)), separately for
//                        z + alpha dz and s + alpha ds           coneops_expcone.jl:166-187, coneops_nonsymmetric_common.jl:5-33,
//                        coneops_compositecone.jl:216-252, variables.jl:14-43.  Every cone walks the same grid alpha0 step^k by the same
//                        multiplications, so the minimum over the lanes is what the reference's sequential loop arrives at.
//   barrier              compute_barrier of every cone kind at up to 8 candidate step lengths and the shifted <z, s>
//                        coneops_expcone.jl:189-248, coneops_powcone.jl:228-251, coneops_nncone.jl, coneops_socone.jl:288-305
// One lane per three-row cone, one launch per kind over the [Exponential | Power] tables so that a wavefront runs one body.  Expressions
// keep the reference's association (-ffp-contract=off).  No assert, no trap: the backtracking loop is bounded by a trip count the host
// derives from (step, alpha_min), the Newton iteration by the reference's 100 steps; a point outside a cone gives +Inf or what logsafe gives.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cone3_math.h"
#include "cone_layout.h"
#include "cone_reduce.h"
#include "kernels.h"

namespace hipkkt {

namespace {

constexpr int kBarBlocks = 64;        // fixed slices of the row sums of the barrier
constexpr int kBarMax = 8;            // candidates per launch

// higher_correction!, coneops_expcone.jl:319-367: u = H_dual^-1 ds, v = step_z, at the scaling point z
__device__ __forceinline__ void exp_higher_correction(const double Hd[6], const double z[3], const double ds[3], const double v[3],
                                                      double eta[3]) {
    eta[0] = eta[1] = eta[2] = 0.0;
    double L[6], u[3];
    if (!chol3_factor(Hd, L)) return;
    chol3_solve(L, ds, u);
    eta[1] = 1.0;
    eta[2] = -z[0] / z[2];
    eta[0] = logsafe(eta[2]);
    const double psi = z[0] * eta[0] - z[0] + z[1];
    const double dpu = eta[0] * u[0] + eta[1] * u[1] + eta[2] * u[2];
    const double dpv = eta[0] * v[0] + eta[1] * v[1] + eta[2] * v[2];
    const double coef = ((u[0] * (v[0] / z[0] - v[2] / z[2]) + u[2] * (z[0] * v[2] / z[2] - v[0]) / z[2]) * psi - 2.0 * dpu * dpv) /
                        (psi * psi * psi);
    eta[0] *= coef; eta[1] *= coef; eta[2] *= coef;
    const double inv_psi2 = 1.0 / psi / psi;
    eta[0] += ((1.0 / psi - 2.0 / z[0]) * u[0] * v[0] / (z[0] * z[0]) - u[2] * v[2] / (z[2] * z[2]) / psi +
               dpu * inv_psi2 * (v[0] / z[0] - v[2] / z[2]) + dpv * inv_psi2 * (u[0] / z[0] - u[2] / z[2]));
    eta[2] += (2.0 * (z[0] / psi - 1.0) * u[2] * v[2] / (z[2] * z[2] * z[2]) - (u[2] * v[0] + u[0] * v[2]) / (z[2] * z[2]) / psi +
               dpu * inv_psi2 * (z[0] * v[2] / (z[2] * z[2]) - v[0] / z[2]) + dpv * inv_psi2 * (z[0] * u[2] / (z[2] * z[2]) - u[0] / z[2]));
    eta[0] /= 2.0; eta[1] /= 2.0; eta[2] /= 2.0;
}
// higher_correction!, coneops_powcone.jl:329-405
__device__ __forceinline__ void pow_higher_correction(const double Hd[6], const double z[3], double a, const double ds[3],
                                                      const double v[3], double eta[3]) {
    eta[0] = eta[1] = eta[2] = 0.0;
    double L[6], u[3];
    if (!chol3_factor(Hd, L)) return;
    chol3_solve(L, ds, u);
    const double phi = pow(z[0] / a, 2.0 * a) * pow(z[1] / (1.0 - a), 2.0 - 2.0 * a);
    const double psi = phi - z[2] * z[2];
    eta[0] = 2.0 * a * phi / z[0];
    eta[1] = 2.0 * (1.0 - a) * phi / z[1];
    eta[2] = -2.0 * z[2];
    const double h11 = 2.0 * a * (2.0 * a - 1.0) * phi / (z[0] * z[0]);
    const double h12 = 4.0 * a * (1.0 - a) * phi / (z[0] * z[1]);
    const double h22 = 2.0 * (1.0 - a) * (1.0 - 2.0 * a) * phi / (z[1] * z[1]);
    const double dpu = eta[0] * u[0] + eta[1] * u[1] + eta[2] * u[2];
    const double dpv = eta[0] * v[0] + eta[1] * v[1] + eta[2] * v[2];
    const double Hv[3] = {h11 * v[0] + h12 * v[1], h12 * v[0] + h22 * v[1], -2.0 * v[2]};
    const double coef = ((u[0] * Hv[0] + u[1] * Hv[1] + u[2] * Hv[2]) * psi - 2.0 * dpu * dpv) / (psi * psi * psi);
    const double coef2 = 4.0 * a * (2.0 * a - 1.0) * (1.0 - a) * phi * (u[0] / z[0] - u[1] / z[1]) * (v[0] / z[0] - v[1] / z[1]) / psi;
    const double inv_psi2 = 1.0 / psi / psi;
    eta[0] = coef * eta[0] - 2.0 * (1.0 - a) * u[0] * v[0] / (z[0] * z[0] * z[0]) + coef2 / z[0] + Hv[0] * dpu * inv_psi2;
    eta[1] = coef * eta[1] - 2.0 * a * u[1] * v[1] / (z[1] * z[1] * z[1]) - coef2 / z[1] + Hv[1] * dpu * inv_psi2;
    eta[2] = coef * eta[2] + Hv[2] * dpu * inv_psi2;
    const double Hu[3] = {h11 * u[0] + h12 * u[1], h12 * u[0] + h22 * u[1], -2.0 * u[2]};
    for (int i = 0; i < 3; i++) eta[i] = (eta[i] + Hu[i] * dpv * inv_psi2) / 2.0;
}

// barrier_dual + barrier_primal at one point, coneops_expcone.jl:223-248
__device__ __forceinline__ double exp_barrier(const double z[3], const double s[3]) {
    const double lg = logsafe(-z[2] / z[0]);
    const double bd = -logsafe(-z[2] * z[0]) - logsafe(z[1] - z[0] - z[0] * lg);
    const double arg = 1.0 - s[0] / s[1] - logsafe(s[1] / s[2]);
    if (!(arg >= 0.0)) return __builtin_huge_val();      // (_wright_omega throws: s is outside the cone)
    double om = wright_omega(arg);
    om = (om - 1.0) * (om - 1.0) / om;
    const double bp = -logsafe(om) - 2.0 * logsafe(s[1]) - logsafe(s[2]) - 3.0;
    return bd + bp;
}
// coneops_powcone.jl:228-251
__device__ __forceinline__ double pow_barrier(const double z[3], const double s[3], double a) {
    const double bd = -logsafe(pow(z[0] / a, 2.0 * a) * pow(z[1] / (1.0 - a), 2.0 - 2.0 * a) - z[2] * z[2]) - (1.0 - a) * logsafe(z[0]) -
                      a * logsafe(z[1]);
    double g[3];
    int trips = 0;
    if (!pow_gradient_primal(s, a, g, &trips)) return __builtin_huge_val();
    const double bp = logsafe(pow(-g[0] / a, 2.0 * a) * pow(-g[1] / (1.0 - a), 2.0 - 2.0 * a) - g[2] * g[2]) + (1.0 - a) * logsafe(-g[0]) +
                      a * logsafe(-g[1]) - 3.0;
    return bd + bp;
}

// backtrack_search, coneops_nonsymmetric_common.jl:5-33, with the loop bounded by `trips`
template <bool POW, bool DUAL>
__device__ __forceinline__ double backtrack(const double q[3], const double dq[3], double a, double alpha0, double alpha_min, double step,
                                            int trips) {
    double alpha = alpha0;
    for (int t = 0; t < trips; t++) {
        const double w[3] = {q[0] + alpha * dq[0], q[1] + alpha * dq[1], q[2] + alpha * dq[2]};
        const bool in = POW ? (DUAL ? pow_dual_feasible(w, a) : pow_primal_feasible(w, a))
                            : (DUAL ? exp_dual_feasible(w) : exp_primal_feasible(w));
        if (in) return alpha;
        alpha *= step;
        if (alpha < alpha_min) return 0.0;
    }
    return 0.0;
}

}  // namespace

// ---- row copies: affine_ds (src = the resident s), ds_from_dz_offset (src = ds) ------------------------------------------------------
__global__ void __launch_bounds__(256)
k_step3_copy(int n3, const int64_t *__restrict__ row0_t, const double *__restrict__ src, double *__restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n3) return;
    const int64_t r = row0_t[c];
    out[r] = src[r]; out[r + 1] = src[r + 1]; out[r + 2] = src[r + 2];
}

// ---- mul_Hs; with addc != NULL: y = -(Hs x + addc) --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_step3_mulhs(int n3, const int64_t *__restrict__ row0_t, const int64_t *__restrict__ out0_t, const double *__restrict__ nsout,
              const double *__restrict__ x, const double *__restrict__ addc, double *__restrict__ y) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n3) return;
    const int64_t r = row0_t[c];
    const double *H = nsout + out0_t[c] + kSlot3Hs;      // pack_triu {00, 01, 11, 02, 12, 22}
    const double Hf[3][3] = {{H[0], H[1], H[3]}, {H[1], H[2], H[4]}, {H[3], H[4], H[5]}};
    const double x0 = x[r], x1 = x[r + 1], x2 = x[r + 2];
    for (int i = 0; i < 3; i++) {
        double v = Hf[i][0] * x0 + Hf[i][1] * x1 + Hf[i][2] * x2;
        if (addc) v = -(v + addc[r + i]);
        y[r + i] = v;
    }
}

// ---- combined_ds_shift ------------------------------------------------------------------------------------------------------------------
template <bool POW>
__global__ void __launch_bounds__(256)
k_step3_shift(int first, int count, const int64_t *__restrict__ row0_t, const int64_t *__restrict__ out0_t,
              const double *__restrict__ alpha_t, const double *__restrict__ nsout, const double *__restrict__ z_all,
              const double *__restrict__ dz_all, const double *__restrict__ ds_all, double sigma_mu, double *__restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const int c = first + k;
    const int64_t r = row0_t[c];
    const double *o = nsout + out0_t[c];
    const double *hd = o + kSlot3Hdual;
    const double Hd[6] = {hd[0], hd[1], hd[2], hd[3], hd[4], hd[5]};
    const double z[3] = {z_all[r], z_all[r + 1], z_all[r + 2]};
    const double v[3] = {dz_all[r], dz_all[r + 1], dz_all[r + 2]};
    const double ds[3] = {ds_all[r], ds_all[r + 1], ds_all[r + 2]};
    double eta[3];
    if (POW) pow_higher_correction(Hd, z, alpha_t[c], ds, v, eta);
    else exp_higher_correction(Hd, z, ds, v, eta);
    for (int i = 0; i < 3; i++) out[r + i] = o[kSlot3Grad + i] * sigma_mu - eta[i];
}

// ---- step_length ------------------------------------------------------------------------------------------------------------------------
// part: one value per workgroup (min over its lanes of alpha_z and alpha_s), Exponential workgroups first
template <bool POW>
__global__ void __launch_bounds__(256)
k_step3_len(int first, int count, const int64_t *__restrict__ row0_t, const double *__restrict__ alpha_t,
            const double *__restrict__ z_all, const double *__restrict__ s_all, const double *__restrict__ dz_all,
            const double *__restrict__ ds_all, const double *__restrict__ sym2, StepTK T, double alpha_max, double step, double alpha_min,
            int trips, double *__restrict__ part) {
    __shared__ double red[4];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const double a0 = alpha_start(sym2, T, alpha_max);
    double v = a0;
    if (k < count) {
        const int c = first + k;
        const int64_t r = row0_t[c];
        const double a = POW ? alpha_t[c] : 0.0;
        const double z[3] = {z_all[r], z_all[r + 1], z_all[r + 2]}, dz[3] = {dz_all[r], dz_all[r + 1], dz_all[r + 2]};
        const double s[3] = {s_all[r], s_all[r + 1], s_all[r + 2]}, ds[3] = {ds_all[r], ds_all[r + 1], ds_all[r + 2]};
        const double az = backtrack<POW, true>(z, dz, a, a0, alpha_min, step, trips);
        const double as = backtrack<POW, false>(s, ds, a, a0, alpha_min, step, trips);
        v = fmin(az, as);
    }
    v = block_min(v, red);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}
__global__ void __launch_bounds__(256)
k_step3_len_final(const double *__restrict__ part, int nparts, const double *__restrict__ sym2, StepTK T, double alpha_max,
                  double *__restrict__ out2) {
    __shared__ double red[4];
    double v = alpha_start(sym2, T, alpha_max);
    for (int k = threadIdx.x; k < nparts; k += 256) v = fmin(v, part[k]);
    v = block_min(v, red);
    if (threadIdx.x == 0) { out2[0] = v; out2[1] = v; }
}

// ---- barrier ----------------------------------------------------------------------------------------------------------------------------
struct BarAlphas { double a[kBarMax]; int n; };

// rows: the Nonnegative cones' -log((s + a ds)(z + a dz)) and the shifted <z, s> of ALL rows, kBarBlocks fixed slices.
// part[(2 j) * kBarBlocks + b] the barrier, part[(2 j + 1) * kBarBlocks + b] the dot of candidate j in slice b
__global__ void __launch_bounds__(256)
k_bar_rows(const signed char *__restrict__ row_kind, const double *__restrict__ z, const double *__restrict__ s,
           const double *__restrict__ dz, const double *__restrict__ ds, BarAlphas A, double *__restrict__ part, int64_t m) {
    __shared__ double red[4];
    double bar[kBarMax], dot[kBarMax];
    for (int j = 0; j < kBarMax; j++) { bar[j] = 0.0; dot[j] = 0.0; }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)kBarBlocks * 256) {
        const bool nn = row_kind[i] == 1;
        const double zi = z[i], si = s[i], dzi = dz[i], dsi = ds[i];
        for (int j = 0; j < kBarMax; j++) {
            if (j >= A.n) break;
            const double zz = zi + A.a[j] * dzi, ss = si + A.a[j] * dsi;
            dot[j] += zz * ss;
            if (nn) bar[j] -= logsafe(ss * zz);
        }
    }
    for (int j = 0; j < kBarMax; j++) {
        if (j >= A.n) break;                   // (uniform over the workgroup)
        const double b = block_sum(bar[j], red), d = block_sum(dot[j], red);
        if (threadIdx.x == 0) { part[(2 * j) * kBarBlocks + blockIdx.x] = b; part[(2 * j + 1) * kBarBlocks + blockIdx.x] = d; }
    }
}
// one workgroup per second-order cone, coneops_socone.jl:288-305; cpart[c * kBarMax + j]
__global__ void __launch_bounds__(256)
k_bar_soc(const int64_t *__restrict__ desc, const double *__restrict__ z_all, const double *__restrict__ s_all,
          const double *__restrict__ dz_all, const double *__restrict__ ds_all, BarAlphas A, double *__restrict__ cpart) {
    __shared__ double red[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int64_t row0 = desc[kSocDesc * c + kSocRow0], dim = desc[kSocDesc * c + kSocDim];
    const double *z = z_all + row0, *s = s_all + row0, *dz = dz_all + row0, *ds = ds_all + row0;
    for (int j = 0; j < kBarMax; j++) {
        if (j >= A.n) break;
        const double a = A.a[j];
        double accz = 0.0, accs = 0.0;
        for (int64_t i = 1 + t; i < dim; i += 256) {
            const double zz = z[i] + a * dz[i], ss = s[i] + a * ds[i];
            accz += zz * zz; accs += ss * ss;
        }
        const double z1 = sqrt(block_sum(accz, red)), s1 = sqrt(block_sum(accs, red));
        const double z0 = z[0] + a * dz[0], s0 = s[0] + a * ds[0];
        const double res_z = (z0 - z1) * (z0 + z1), res_s = (s0 - s1) * (s0 + s1);
        const double v = (res_s > 0.0 && res_z > 0.0) ? -logsafe(res_s * res_z) / 2.0 : __builtin_huge_val();
        if (t == 0) cpart[(int64_t)c * kBarMax + j] = v;
    }
}
template <bool POW>
__global__ void __launch_bounds__(256)
k_bar_cone3(int first, int count, const int64_t *__restrict__ row0_t, const double *__restrict__ alpha_t,
            const double *__restrict__ z_all, const double *__restrict__ s_all, const double *__restrict__ dz_all,
            const double *__restrict__ ds_all, BarAlphas A, double *__restrict__ cpart) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const int c = first + k;
    const int64_t r = row0_t[c];
    const double a = POW ? alpha_t[c] : 0.0;
    for (int j = 0; j < kBarMax; j++) {
        if (j >= A.n) break;
        const double al = A.a[j];
        const double z[3] = {z_all[r] + al * dz_all[r], z_all[r + 1] + al * dz_all[r + 1], z_all[r + 2] + al * dz_all[r + 2]};
        const double s[3] = {s_all[r] + al * ds_all[r], s_all[r + 1] + al * ds_all[r + 1], s_all[r + 2] + al * ds_all[r + 2]};
        cpart[(int64_t)c * kBarMax + j] = POW ? pow_barrier(z, s, a) : exp_barrier(z, s);
    }
}
// one workgroup: out[2 j] = the cones' barrier, out[2 j + 1] = the shifted dot; every sum in a fixed order
__global__ void __launch_bounds__(256)
k_bar_final(const double *__restrict__ part, const double *__restrict__ socpart, int nsoc, const double *__restrict__ c3part, int n3,
            const double *__restrict__ gppart, int ngp, int nalpha, double *__restrict__ out) {
    __shared__ double red[4];
    for (int j = 0; j < nalpha; j++) {
        double acc = 0.0;
        for (int c = threadIdx.x; c < nsoc; c += 256) acc += socpart[(int64_t)c * kBarMax + j];
        const double bsoc = block_sum(acc, red);
        acc = 0.0;
        for (int c = threadIdx.x; c < n3; c += 256) acc += c3part[(int64_t)c * kBarMax + j];
        const double b3 = block_sum(acc, red);
        double bgp = 0.0;
        if (ngp > 0) {                         // (uniform; a set without Generalized Power cones adds nothing, not even 0.0)
            acc = 0.0;
            for (int c = threadIdx.x; c < ngp; c += 256) acc += gppart[(int64_t)c * kBarMax + j];
            bgp = block_sum(acc, red);
        }
        if (threadIdx.x == 0) {
            double b = 0.0, d = 0.0;
            for (int k = 0; k < kBarBlocks; k++) { b += part[(2 * j) * kBarBlocks + k]; d += part[(2 * j + 1) * kBarBlocks + k]; }
            out[2 * j] = ngp > 0 ? ((b + bsoc) + b3) + bgp : (b + bsoc) + b3;
            out[2 * j + 1] = d;
        }
    }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
static inline dim3 lanes_grid(int n) { return dim3((unsigned)((n + 255) / 256)); }

int step3_max_candidates() { return kBarMax; }
// where launch_step3_barrier expects the partials of the Generalized Power cones (kBarMax per cone) in its work buffer
double *step3_barrier_gppart(double *work, int nsoc, int n3) {
    return work + 2 * kBarMax * kBarBlocks + (int64_t)kBarMax * ((nsoc > 0 ? nsoc : 0) + n3);
}
// doubles of the barrier's work buffer for a handle with `ncones` cones
int64_t step3_barrier_doubles(int64_t ncones) { return 2 * (int64_t)kBarMax * kBarBlocks + 2 * kBarMax * ncones + 2 * kBarMax; }

void launch_step3_copy(hipStream_t st, int n3, const int64_t *row0, const double *src, double *out) {
    if (n3 > 0) hipLaunchKernelGGL(k_step3_copy, lanes_grid(n3), dim3(256), 0, st, n3, row0, src, out);
}
void launch_step3_mulhs(hipStream_t st, int n3, const int64_t *row0, const int64_t *out0, const double *nsout, const double *x,
                        const double *addc, double *y) {
    if (n3 > 0) hipLaunchKernelGGL(k_step3_mulhs, lanes_grid(n3), dim3(256), 0, st, n3, row0, out0, nsout, x, addc, y);
}
void launch_step3_shift(hipStream_t st, int nexp, int npow, const int64_t *row0, const int64_t *out0, const double *alpha,
                        const double *nsout, const double *z, const double *dz, const double *ds, double sigma_mu, double *out) {
    if (nexp > 0)
        hipLaunchKernelGGL(k_step3_shift<false>, lanes_grid(nexp), dim3(256), 0, st, 0, nexp, row0, out0, alpha, nsout, z, dz, ds, sigma_mu, out);
    if (npow > 0)
        hipLaunchKernelGGL(k_step3_shift<true>, lanes_grid(npow), dim3(256), 0, st, nexp, npow, row0, out0, alpha, nsout, z, dz, ds, sigma_mu, out);
}
// sym2 = (alpha_z, alpha_s) of the symmetric cones (device); dtau (device, may be NULL: then alpha_max is the start) with tau, kappa,
// rhs_kappa; part: at least (nexp + 255) / 256 + (npow + 255) / 256 + ngp doubles, the last ngp of them already written on this stream by
// launch_genpow_length (step_genpow.hip); out2 = the composite (alpha, alpha)
int step3_length_parts(int nexp, int npow) { return (nexp + 255) / 256 + (npow + 255) / 256; }
void launch_step3_length(hipStream_t st, int nexp, int npow, const int64_t *row0, const double *alpha, const double *z, const double *s,
                         const double *dz, const double *ds, const double *sym2, const double *dtau, double tau, double kappa,
                         double rhs_kappa, double alpha_max, double step, double alpha_min, int trips, double *part, double *out2, int ngp) {
    const StepTK T{dtau, tau, kappa, rhs_kappa};
    const int be = (nexp + 255) / 256, bp = (npow + 255) / 256;
    if (nexp > 0)
        hipLaunchKernelGGL(k_step3_len<false>, dim3(be), dim3(256), 0, st, 0, nexp, row0, alpha, z, s, dz, ds, sym2, T, alpha_max, step,
                           alpha_min, trips, part);
    if (npow > 0)
        hipLaunchKernelGGL(k_step3_len<true>, dim3(bp), dim3(256), 0, st, nexp, npow, row0, alpha, z, s, dz, ds, sym2, T, alpha_max, step,
                           alpha_min, trips, part + be);
    hipLaunchKernelGGL(k_step3_len_final, dim3(1), dim3(256), 0, st, part, be + bp + ngp, sym2, T, alpha_max, out2);
}
// work: step3_barrier_doubles(ncones) doubles; out: 2 * nalpha doubles (device); with ngp > 0 launch_genpow_barrier (step_genpow.hip) has
// written the Generalized Power cones' partials to step3_barrier_gppart(work, nsoc, nexp + npow) on this stream
void launch_step3_barrier(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, int nexp, int npow,
                          const int64_t *row0, const double *alpha, const double *z, const double *s, const double *dz, const double *ds,
                          const double *alphas, int nalpha, double *work, double *out, int64_t m, int ngp) {
    BarAlphas A;
    A.n = nalpha;
    for (int j = 0; j < kBarMax; j++) A.a[j] = j < nalpha ? alphas[j] : 0.0;
    double *part = work, *socpart = part + 2 * kBarMax * kBarBlocks, *c3part = socpart + (int64_t)kBarMax * (nsoc > 0 ? nsoc : 0);
    hipLaunchKernelGGL(k_bar_rows, dim3(kBarBlocks), dim3(256), 0, st, row_kind, z, s, dz, ds, A, part, m);
    if (nsoc > 0) hipLaunchKernelGGL(k_bar_soc, dim3(nsoc), dim3(256), 0, st, desc, z, s, dz, ds, A, socpart);
    if (nexp > 0) hipLaunchKernelGGL(k_bar_cone3<false>, lanes_grid(nexp), dim3(256), 0, st, 0, nexp, row0, alpha, z, s, dz, ds, A, c3part);
    if (npow > 0) hipLaunchKernelGGL(k_bar_cone3<true>, lanes_grid(npow), dim3(256), 0, st, nexp, npow, row0, alpha, z, s, dz, ds, A, c3part);
    hipLaunchKernelGGL(k_bar_final, dim3(1), dim3(256), 0, st, part, socpart, nsoc, c3part, nexp + npow,
                       c3part + (int64_t)kBarMax * (nexp + npow), ngp, nalpha, out);
}

}  // namespace hipkkt
