// update_scaling! + get_Hs! of the symmetric cones on the device, written straight into the resident KKT
// values (kktsolver_directldl.jl:197-245 then consumes them unchanged).  Given (s, z) in cone order:
//   Zero          Hs = 0                                                       (coneops_zerocone.jl:91)
//   Nonnegative   lambda = sqrt(s z), w = sqrt(s / z), Hs = w^2                (coneops_nncone.jl:77-101)          bit-exact
//   SecondOrder   eta, w, lambda, sparse (d, u, v) or the dense <= 4 block     (coneops_socone.jl:75-192)          sums are tree sums
//   PSDTriangle   W = R R^T from the caller's R (the Cholesky / SVD of :78-143 stay with the caller), then the skron block of
//                 k_psd_hs (values.hip)                                        (coneops_psdtrianglecone.jl:145-161)
// Expressions keep the reference's association; this file is compiled with -ffp-contract=off so that a*x + b*y is two rounded
// products and a sum like Julia's, not an FMA.  Everything is HBM / latency bound: 2 m doubles in, (w, lambda) out, O(m) K entries.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cone3_math.h"
#include "cone_layout.h"
#include "cone_reduce.h"
#include "kernels.h"

namespace hipkkt {

// one entry per row of a Zero / Nonnegative cone: kind 0 zero, 1 nonnegative, other rows are skipped
__global__ void __launch_bounds__(256)
k_scaling_diag(const signed char *__restrict__ row_kind, const int64_t *__restrict__ row_hs, const int64_t *__restrict__ map_hs,
               const double *__restrict__ s, const double *__restrict__ z, double *__restrict__ w, double *__restrict__ lam,
               double *__restrict__ kval, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int kind = row_kind[i];
    if (kind == 0) {
        w[i] = 0.0; lam[i] = 0.0;
        kval[map_hs[row_hs[i]]] = -0.0;
    } else if (kind == 1) {
        const double l = sqrt(s[i] * z[i]), ww = sqrt(s[i] / z[i]);
        lam[i] = l; w[i] = ww;
        kval[map_hs[row_hs[i]]] = -(ww * ww);
    }
}

__device__ __forceinline__ double sqrt_soc_residual(double z0, double z1norm) {   // coneops_socone.jl:395-407
    const double r = (z0 - z1norm) * (z0 + z1norm);
    return r > 0.0 ? sqrt(r) : 0.0;
}

// one workgroup per second-order cone, desc: its descriptors (cone_layout.h kSoc*)
__global__ void __launch_bounds__(256)
k_scaling_soc(const int64_t *__restrict__ desc, const int64_t *__restrict__ map_hs, const double *__restrict__ s_all,
              const double *__restrict__ z_all, double *__restrict__ w_all, double *__restrict__ lam_all, double *__restrict__ eta_out,
              double *__restrict__ soc_u, double *__restrict__ soc_v, double *__restrict__ soc_eta2, double *__restrict__ kval,
              int *__restrict__ fail) {
    __shared__ double red[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int64_t row0 = desc[kSocDesc * c + kSocRow0], dim = desc[kSocDesc * c + kSocDim], hs0 = desc[kSocDesc * c + kSocHs0];
    const int64_t uv0 = desc[kSocDesc * c + kSocUv0], ord = desc[kSocDesc * c + kSocOrd];
    const double *s = s_all + row0, *z = z_all + row0;
    double *w = w_all + row0, *lam = lam_all + row0;
    double a = 0.0, b = 0.0;
    for (int64_t i = 1 + t; i < dim; i += 256) { a += z[i] * z[i]; b += s[i] * s[i]; }
    const double z1 = sqrt(block_sum(a, red)), s1 = sqrt(block_sum(b, red));
    const double z0 = z[0], s0 = s[0];
    const double zscale = sqrt_soc_residual(z0, z1), sscale = sqrt_soc_residual(s0, s1);
    if (zscale == 0.0 || sscale == 0.0) { if (t == 0) atomicOr(fail, 1); return; }     // :88-90, uniform over the workgroup
    const double eta = sqrt(sscale / zscale);
    // w = s / sscale +- z / zscale, then normalised (:96-113)
    a = 0.0;
    for (int64_t i = t; i < dim; i += 256) {
        double v = s[i] / sscale;
        if (i == 0) v += z0 / zscale; else { v -= z[i] / zscale; a += v * v; }
        w[i] = v;
    }
    const double w1 = sqrt(block_sum(a, red));        // block_sum's barriers also order the w[] stores before the reads below
    const double wscale = sqrt_soc_residual(s0 / sscale + z0 / zscale, w1);
    if (wscale == 0.0) { if (t == 0) atomicOr(fail, 1); return; }
    a = 0.0;
    for (int64_t i = 1 + t; i < dim; i += 256) { const double v = w[i] / wscale; w[i] = v; a += v * v; }
    const double w1sq = block_sum(a, red);
    const double w0 = sqrt(1.0 + w1sq);
    // lambda = W z (:115-123)
    const double gamma = 0.5 * wscale;
    const double cs = (gamma + z0 / zscale) / sscale, cz = (gamma + s0 / sscale) / zscale;
    const double cinv = 1.0 / (s0 / sscale + z0 / zscale + 2.0 * gamma), root = sqrt(sscale * zscale);
    for (int64_t i = 1 + t; i < dim; i += 256) {
        double l = cs * s[i] + cz * z[i];
        l *= cinv;
        lam[i] = l * root;
    }
    const double eta2 = eta * eta;
    if (t == 0) { w[0] = w0; lam[0] = gamma * root; eta_out[c] = eta; }
    if (uv0 >= 0) {
        // sparse expansion terms (:125-153) and the diagonal block eta^2 * [d, 1, ..., 1] (:166-171)
        const double alpha = 2.0 * w0, wsq = w0 * w0 + w1sq, wsqinv = 1.0 / wsq, d = wsqinv / 2.0;
        const double u0 = sqrt(wsq - d), u1 = alpha / u0, v1 = sqrt(2.0 * (2.0 + wsqinv) / (2.0 * wsq - wsqinv));
        double *u = soc_u + uv0, *v = soc_v + uv0;
        for (int64_t i = t; i < dim; i += 256) {
            const double wi = i == 0 ? w0 : w[i];
            u[i] = i == 0 ? u0 : u1 * wi;
            v[i] = i == 0 ? 0.0 : v1 * wi;
            kval[map_hs[hs0 + i]] = -(i == 0 ? eta2 * d : eta2);
        }
        if (t == 0) soc_eta2[ord] = eta2;
    } else if (t == 0) {
        // dense packed upper triangle of eta^2 (2 w w' - J), dim <= 4 (:173-189)
        const double r2 = sqrt(2.0);
        double wl[4];
        wl[0] = w0;
        for (int i = 1; i < (int)dim; i++) wl[i] = w[i];
        int64_t h = 0;
        kval[map_hs[hs0 + h++]] = -(((r2 * wl[0] - 1.0) * (r2 * wl[0] + 1.0)) * eta2);
        for (int col = 1; col < (int)dim; col++)
            for (int row = 0; row <= col; row++) {
                double e = 2.0 * wl[row] * wl[col];
                if (row == col) e += 1.0;
                kval[map_hs[hs0 + h++]] = -(e * eta2);
            }
    }
}

// W = R R^T of one PSD cone (n x n, column-major), both triangles with the same summation order so that W is exactly symmetric
__global__ void __launch_bounds__(256)
k_psd_rrt(const double *__restrict__ R, double *__restrict__ W, int n) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)n * n) return;
    const int i = (int)(e % n), j = (int)(e / n);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    double acc = 0.0;
    for (int k = 0; k < n; k++) acc += R[lo + (int64_t)k * n] * R[hi + (int64_t)k * n];
    W[e] = acc;
}

// ---- the non-symmetric cones (hipkkt_update_scaling_ex) ------------------------------------------------------------------------
//   Exponential   coneops_expcone.jl:63-83 (update_scaling!), :284-297 (gradient_primal), :370-467 (update_dual_grad_H, Wright omega)
//   Power         coneops_powcone.jl:65-85, :288-317, :408-478 (one-sided Newton-Raphson, at most 100 steps)
//   both          coneops_nonsymmetric_common.jl:50-192 (Dual: Hs = mu H*, PrimalDual: the BFGS form or the central-path fallback)
//   GenPower      coneops_genpowcone.jl:64-108, :343-396 and _csc_update_sparsecone, directldl_datamaps.jl:146-167
// A cone whose z is not strictly inside the dual cone, whose s is not strictly inside the primal cone (PrimalDual), or whose result is
// not finite sets the fail word, fills its slot of the output vector with NaN and leaves its entries of K alone: no assert, no trap.
// Every loop is bounded (the Newton iteration by the reference's 100 steps) and every index comes from the tables of the handle.
// logsafe, the Wright omega function, the cones' gradients / Hessians and the 3 x 3 Cholesky test are in cone3_math.h (shared with
// step_cone3.hip).

// use_primal_dual_scaling, coneops_nonsymmetric_common.jl:82-164: st = K.g, zt = -f'(s); Hs in pack_triu order
__device__ bool primal_dual_hs(const Cone3 &K, const double s[3], const double z[3], const double zt[3], double Hs[6]) {
    const double eps = 2.220446049250313e-16, sqrt_eps = 1.4901161193847656e-08;
    const double *st = K.g, *H = K.H;
    const double Hf[3][3] = {{H[0], H[1], H[3]}, {H[1], H[2], H[4]}, {H[3], H[4], H[5]}};
    const double dot_sz = z[0] * s[0] + z[1] * s[1] + z[2] * s[2];
    const double mu = dot_sz / 3.0;
    const double mut = (zt[0] * st[0] + zt[1] * st[1] + zt[2] * st[2]) / 3.0;
    double ds[3], dz[3];
    for (int i = 0; i < 3; i++) { ds[i] = s[i] + mu * st[i]; dz[i] = z[i] + mu * zt[i]; }
    const double dot_dsz = ds[0] * dz[0] + ds[1] * dz[1] + ds[2] * dz[2];
    const double de1 = mu * mut - 1.0;
    double Hz[3];
    for (int i = 0; i < 3; i++) Hz[i] = Hf[i][0] * zt[0] + Hf[i][1] * zt[1] + Hf[i][2] * zt[2];
    const double de2 = (zt[0] * Hz[0] + zt[1] * Hz[1] + zt[2] * Hz[2]) - 3.0 * mut * mut;
    if (fabs(de1) > sqrt_eps && fabs(de2) > eps && dot_sz > 0.0 && dot_dsz > 0.0) {
        double tmp[3];
        for (int i = 0; i < 3; i++) tmp[i] = mut * st[i] - Hf[i][0] * zt[0] - Hf[i][1] * zt[1] - Hf[i][2] * zt[2];
        double nrm2 = 0.0;
        for (int j = 0; j < 3; j++)
            for (int i = 0; i < 3; i++) {
                const double e = Hf[i][j] - (st[i] * st[j] / 3.0 + tmp[i] * tmp[j] / de2);
                nrm2 += e * e;
            }
        const double t = mu * sqrt(nrm2);      // Frobenius norm
        if (!(t > 0.0)) return false;          // (:135 asserts)
        double ax[3] = {z[1] * zt[2] - z[2] * zt[1], z[2] * zt[0] - z[0] * zt[2], z[0] * zt[1] - z[1] * zt[0]};
        const double inv = 1.0 / sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
        for (int i = 0; i < 3; i++) ax[i] *= inv;
        int h = 0;
        for (int j = 0; j < 3; j++)
            for (int i = 0; i <= j; i++) Hs[h++] = s[i] * s[j] / dot_sz + ds[i] * ds[j] / dot_dsz + t * ax[i] * ax[j];
    } else {
        for (int i = 0; i < 6; i++) Hs[i] = mu * H[i];      // on the central path: the LOCAL mu = <s, z> / 3 (:159)
    }
    return true;
}

// On late iterates Hs, positive definite in exact arithmetic, reaches condition numbers of 1e16 .. 4e18 and the 3 x 3 Cholesky of the
// rounded block can break down (on the reference's own host values as well).  Such a block gets the smallest shift
// 2^k eps max(diag) on its diagonal, k = 1 .. 8, with which the factorisation goes through -- a change in the last one or two bits of the
// diagonal (k = 1 on every block met so far), far below what one ulp of (s, z) moves such a block by.  A block that needs more is
// left as the reference's formulas give it.  Blocks whose Cholesky goes through are never touched.
__device__ __forceinline__ void keep_positive_definite(double Hs[6]) {
    if (chol3_ok(Hs)) return;
    const double dmax = fmax(Hs[0], fmax(Hs[2], Hs[5]));
    double delta = 2.220446049250313e-16 * dmax;
    for (int k = 1; k <= 8; k++) {
        delta *= 2.0;
        double T[6] = {Hs[0] + delta, Hs[1], Hs[2] + delta, Hs[3], Hs[4], Hs[5] + delta};
        if (chol3_ok(T)) {
            for (int i = 0; i < 6; i++) Hs[i] = T[i];
            return;
        }
    }
}

// One lane per three-row cone; a launch holds cones of one kind only (POW = false Exponential, true Power): the tables are ordered
// by kind, this launch takes the `count` cones from `first` on.  strategy 0 PrimalDual, 1 Dual (types.jl:73-76).
// Per cone: Hs (6) negated through map_hs into kval; Hs (6), H_dual (6), grad (3) into its slot out[out0 ..) (cone_layout.h kSlot3*).  trips (may be NULL) receives the
// steps of the Newton iteration.
template <bool POW>
__global__ void __launch_bounds__(256)
k_scaling_cone3(int first, int count, const int64_t *__restrict__ row0_t, const int64_t *__restrict__ hs0_t,
                const int64_t *__restrict__ out0_t, const double *__restrict__ alpha_t, const int64_t *__restrict__ map_hs,
                const double *__restrict__ s_all, const double *__restrict__ z_all, double mu, int strategy,
                double *__restrict__ kval, double *__restrict__ out, int *__restrict__ trips_out, int *__restrict__ fail) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const int c = first + k;
    const int64_t row0 = row0_t[c], hs0 = hs0_t[c], out0 = out0_t[c];
    const double a = POW ? alpha_t[c] : 0.0;
    const double s[3] = {s_all[row0], s_all[row0 + 1], s_all[row0 + 2]};
    const double z[3] = {z_all[row0], z_all[row0 + 1], z_all[row0 + 2]};
    Cone3 K;
    double Hs[6];
    int trips = 0;
    bool ok = POW ? pow_dual_grad_H(z, a, K) : exp_dual_grad_H(z, K);
    if (ok) {
        if (strategy == 1) {
            for (int i = 0; i < 6; i++) Hs[i] = mu * K.H[i];      // use_dual_scaling, coneops_nonsymmetric_common.jl:71-78
        } else {
            double zt[3];
            ok = POW ? pow_gradient_primal(s, a, zt, &trips) : exp_gradient_primal(s, zt);
            ok = ok && finite3(zt[0], zt[1], zt[2]) && primal_dual_hs(K, s, z, zt, Hs);
        }
    }
    if (ok) {
        ok = finite3(K.g[0], K.g[1], K.g[2]);
        for (int i = 0; i < 6; i++) ok = ok && isfinite(Hs[i]) && isfinite(K.H[i]);
    }
    if (ok) keep_positive_definite(Hs);
    double *o = out + out0;
    if (trips_out) trips_out[c] = trips;
    if (!ok) {
        atomicOr(fail, 1);
        for (int i = 0; i < kSlot3; i++) o[i] = __builtin_nan("");
        return;
    }
    for (int i = 0; i < 6; i++) {
        kval[map_hs[hs0 + i]] = -Hs[i];
        o[kSlot3Hs + i] = Hs[i];
        o[kSlot3Hdual + i] = K.H[i];
    }
    for (int i = 0; i < 3; i++) o[kSlot3Grad + i] = K.g[i];
}

// One wavefront (= one workgroup of 64) per Generalized Power cone.  desc: its descriptors (cone_layout.h kGp*; step_genpow.hip reads
// the bits of psi); the index table is [map.q (dim1) | map.r (dim2) | map.p (dim) | map.D (3)] of the cone's GenPowExpansionMap
// (directldl_datamaps.jl:81-99), resident.
// The cone always takes the Dual scaling with the caller's mu (coneops_genpowcone.jl:21, :64-80).  Products and sums over the cone
// are butterfly reductions: every lane holds the same phi, |w|^2.
// out slot: cone_layout.h gp_slot.
__global__ void __launch_bounds__(64)
k_scaling_genpow(const int64_t *__restrict__ desc, const double *__restrict__ alpha_all, const int64_t *__restrict__ idx_all,
                 const int64_t *__restrict__ map_hs, const double *__restrict__ z_all, double mu, double sqrtmu,
                 double *__restrict__ kval, double *__restrict__ out, int *__restrict__ fail) {
    const int c = blockIdx.x, t = threadIdx.x;
    const int64_t *d = desc + kGpDesc * (int64_t)c;
    const int64_t row0 = d[kGpRow0], dim1 = d[kGpDim1], dim2 = d[kGpDim2], hs0 = d[kGpHs0], dim = dim1 + dim2;
    const double *z = z_all + row0, *a = alpha_all + d[kGpAlpha0];
    const int64_t *qi = idx_all + d[kGpIdx0], *ri = qi + dim1, *pi = ri + dim2, *Di = pi + dim;
    // (the slot's pointers stay chained and its length 3 dim + dim1 + 1 spelled out: gp_slot() gives other address arithmetic)
    double *g = out + d[kGpOut0], *od1 = g + dim, *od2 = od1 + dim1, *op = od2 + 1, *oq = op + dim, *orr = oq + dim1;
    // update_dual_grad_H, :343-396
    double phi = 1.0, n2 = 0.0;
    int bad = 0;
    for (int64_t i = t; i < dim1; i += 64) {
        if (!(z[i] > 0.0)) bad = 1;
        phi *= pow(z[i] / a[i], 2.0 * a[i]);
    }
    for (int64_t i = t; i < dim2; i += 64) n2 += z[dim1 + i] * z[dim1 + i];
    phi = wave_prod(phi);
    const double norm2w = wave_sum(n2);
    const double zeta = phi - norm2w;
    bad = wave_or(bad);
    if (!bad && !(zeta > 0.0 && isfinite(phi))) bad = 1;      // (:357 asserts); uniform over the wavefront
    const double p0 = sqrt(phi * (phi + norm2w) / 2.0), p1 = -2.0 * phi / p0, q0 = sqrt(zeta * phi / 2.0);
    const double r1 = 2.0 * sqrt(zeta / (phi + norm2w)), d2 = 2.0 / zeta;
    // two passes with the same expressions: the first only looks for a non-finite result, so that a failing cone writes nothing
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1) {
            bad = wave_or(bad);
            if (bad) {
                if (t == 0) atomicOr(fail, 1);
                for (int64_t i = t; i < 3 * dim + dim1 + 1; i += 64) g[i] = __builtin_nan("");
                return;
            }
        } else if (bad) {
            continue;
        }
        for (int64_t i = t; i < dim1; i += 64) {
            const double tau = 2.0 * a[i] / z[i];
            const double gi = -tau * phi / zeta - (1.0 - a[i]) / z[i];
            const double d1 = tau * phi / (zeta * z[i]) + (1.0 - a[i]) / (z[i] * z[i]);
            const double p = p0 * tau / zeta, q = tau * (q0 / zeta);
            if (pass == 0) {
                if (!(finite3(gi, d1, p) && isfinite(q) && isfinite(mu * d1) && d1 > 0.0)) bad = 1;
            } else {
                g[i] = gi; od1[i] = d1; op[i] = p; oq[i] = q;
                kval[map_hs[hs0 + i]] = -(mu * d1);                       // get_Hs!, :91-108
                kval[qi[i]] = q * -sqrtmu;                                // directldl_datamaps.jl:157-162
                kval[pi[i]] = p * -sqrtmu;
            }
        }
        for (int64_t i = t; i < dim2; i += 64) {
            const double w = z[dim1 + i];
            const double gi = 2.0 * w / zeta, p = p1 * w / zeta, r = r1 * w / zeta;
            if (pass == 0) {
                if (!finite3(gi, p, r)) bad = 1;
            } else {
                g[dim1 + i] = gi; op[dim1 + i] = p; orr[i] = r;
                kval[map_hs[hs0 + dim1 + i]] = -(mu * d2);
                kval[ri[i]] = r * -sqrtmu;
                kval[pi[dim1 + i]] = p * -sqrtmu;
            }
        }
        if (pass == 0) {
            if (!(finite3(d2, mu * d2, sqrtmu) && d2 > 0.0)) bad = 1;
        } else if (t == 0) {
            od2[0] = d2;
            kval[Di[0]] = -1.0; kval[Di[1]] = -1.0; kval[Di[2]] = 1.0;      // :165
        }
    }
}

void launch_scaling_cone3(hipStream_t st, int nexp, int npow, const int64_t *row0, const int64_t *hs0, const int64_t *out0,
                          const double *alpha, const int64_t *map_hs, const double *s, const double *z, double mu, int strategy,
                          double *kval, double *out, int *trips, int *fail) {
    if (nexp > 0)
        hipLaunchKernelGGL(k_scaling_cone3<false>, dim3((unsigned)((nexp + 255) / 256)), dim3(256), 0, st, 0, nexp, row0, hs0, out0,
                           alpha, map_hs, s, z, mu, strategy, kval, out, trips, fail);
    if (npow > 0)
        hipLaunchKernelGGL(k_scaling_cone3<true>, dim3((unsigned)((npow + 255) / 256)), dim3(256), 0, st, nexp, npow, row0, hs0, out0,
                           alpha, map_hs, s, z, mu, strategy, kval, out, trips, fail);
}
void launch_scaling_genpow(hipStream_t st, int ngenpow, const int64_t *desc, const double *alpha, const int64_t *idx,
                           const int64_t *map_hs, const double *z, double mu, double sqrtmu, double *kval, double *out, int *fail) {
    if (ngenpow > 0)
        hipLaunchKernelGGL(k_scaling_genpow, dim3(ngenpow), dim3(64), 0, st, desc, alpha, idx, map_hs, z, mu, sqrtmu, kval, out, fail);
}

void launch_scaling_diag(hipStream_t st, const signed char *row_kind, const int64_t *row_hs, const int64_t *map_hs, const double *s,
                         const double *z, double *w, double *lam, double *kval, int64_t m) {
    if (m > 0)
        hipLaunchKernelGGL(k_scaling_diag, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, row_kind, row_hs, map_hs, s, z, w, lam,
                           kval, m);
}
void launch_scaling_soc(hipStream_t st, int nsoc, const int64_t *desc, const int64_t *map_hs, const double *s, const double *z,
                        double *w, double *lam, double *eta_out, double *soc_u, double *soc_v, double *soc_eta2, double *kval,
                        int *fail) {
    if (nsoc > 0)
        hipLaunchKernelGGL(k_scaling_soc, dim3(nsoc), dim3(256), 0, st, desc, map_hs, s, z, w, lam, eta_out, soc_u, soc_v, soc_eta2,
                           kval, fail);
}
void launch_psd_rrt(hipStream_t st, const double *R, double *W, int n) {
    const int64_t nn = (int64_t)n * n;
    if (nn > 0) hipLaunchKernelGGL(k_psd_rrt, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, R, W, n);
}

}  // namespace hipkkt
