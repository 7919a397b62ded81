// Device helpers shared by the scaling (scaling.hip) and the step (step_cone3.hip) of the three-row non-symmetric cones: logsafe, the
// Wright omega function, the feasibility tests, the dual gradient / Hessian and the primal gradient of the Exponential and the Power
// cone, the 3 x 3 Cholesky; and the start of the non-symmetric cones' line search, which step_genpow.hip shares with step_cone3.hip.
// Expressions keep the reference's association; every user is compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hipkkt {

__device__ __forceinline__ double logsafe(double v) {      // mathutils.jl:12-18
    if (v < 0.0) return -1.7976931348623157e308;
    if (v == 0.0) return -__builtin_huge_val();
    return log(v);
}
__device__ __forceinline__ bool finite3(double a, double b, double c) { return isfinite(a) && isfinite(b) && isfinite(c); }

// coneops_expcone.jl:412-467; the caller has checked z >= 0
__device__ double wright_omega(double z) {
    double w;
    if (z < 1.0 + 3.141592653589793) {
        const double zm1 = z - 1.0;
        double p = zm1;
        w = 1.0 + 0.5 * p;
        p *= zm1;
        w += (1.0 / 16.0) * p;
        p *= zm1;
        w -= (1.0 / 192.0) * p;
        p *= zm1;
        w -= (1.0 / 3072.0) * p;
        p *= zm1;
        w += (13.0 / 61440.0) * p;
    } else {
        const double logz = logsafe(z), zinv = 1.0 / z;
        w = z - logz;
        double q = logz * zinv;
        w += q;
        q *= zinv;
        w += q * (logz / 2.0 - 1.0);
        w += q * (logz * logz / 3.0 - (3.0 / 2.0) * logz + 1.0);      // (:451 does not store q * zinv)
    }
    double r = z - w - logsafe(w);
    for (int k = 0; k < 2; k++) {
        const double wp1 = w + 1.0;
        const double t = wp1 * (wp1 + (2.0 * r) / 3.0);
        w *= 1.0 + (r / wp1) * (t - 0.5 * r) / (t - r);
        r = (2.0 * w * w - 8.0 * w - 1.0) / (72.0 * (wp1 * wp1 * wp1 * wp1 * wp1 * wp1)) * r * r * r * r;
    }
    return w;
}

// H = the dual Hessian in pack_triu order {00, 01, 11, 02, 12, 22}
struct Cone3 { double g[3], H[6]; };

// is_dual_feasible / is_primal_feasible, coneops_expcone.jl:253-281
__device__ __forceinline__ bool exp_dual_feasible(const double z[3]) {
    if (!(z[2] > 0.0 && z[0] < 0.0)) return false;
    return z[1] - z[0] - z[0] * logsafe(-z[2] / z[0]) > 0.0;
}
__device__ __forceinline__ bool exp_primal_feasible(const double s[3]) {
    if (!(s[2] > 0.0 && s[1] > 0.0)) return false;
    return s[1] * logsafe(s[2] / s[1]) - s[0] > 0.0;
}

__device__ __forceinline__ bool exp_dual_grad_H(const double z[3], Cone3 &K) {      // coneops_expcone.jl:269-281, :370-400
    if (!exp_dual_feasible(z)) return false;
    const double l = logsafe(-z[2] / z[0]);
    const double r = -z[0] * l - z[0] + z[1];
    const double c2 = 1.0 / r;
    K.g[0] = c2 * l - 1.0 / z[0];
    K.g[1] = -c2;
    K.g[2] = (c2 * z[0] - 1.0) / z[2];
    K.H[0] = (r * r - z[0] * r + l * l * z[0] * z[0]) / (r * z[0] * z[0] * r);
    K.H[1] = -l / (r * r);
    K.H[2] = 1.0 / (r * r);
    K.H[3] = (z[1] - z[0]) / (r * r * z[2]);
    K.H[4] = -z[0] / (r * r * z[2]);
    K.H[5] = (r * r - z[0] * r + z[0] * z[0]) / (r * r * z[2] * z[2]);
    return true;
}
__device__ __forceinline__ bool exp_gradient_primal(const double s[3], double g[3]) {      // coneops_expcone.jl:253-266, :284-297
    if (!exp_primal_feasible(s)) return false;
    const double arg = 1.0 - s[0] / s[1] - logsafe(s[1] / s[2]);
    if (!(arg >= 0.0)) return false;                       // (:415 throws)
    const double om = wright_omega(arg);
    g[0] = 1.0 / ((om - 1.0) * s[1]);
    g[1] = g[0] + g[0] * logsafe(om * s[1] / s[2]) - 1.0 / s[1];
    g[2] = om / ((1.0 - om) * s[2]);
    return true;
}

// is_dual_feasible / is_primal_feasible, coneops_powcone.jl:256-285
__device__ __forceinline__ bool pow_dual_feasible(const double z[3], double a) {
    if (!(z[0] > 0.0 && z[1] > 0.0)) return false;
    return exp(2.0 * a * logsafe(z[0] / a) + 2.0 * (1.0 - a) * logsafe(z[1] / (1.0 - a))) - z[2] * z[2] > 0.0;
}
__device__ __forceinline__ bool pow_primal_feasible(const double s[3], double a) {
    if (!(s[0] > 0.0 && s[1] > 0.0)) return false;
    return exp(2.0 * a * logsafe(s[0]) + 2.0 * (1.0 - a) * logsafe(s[1])) - s[2] * s[2] > 0.0;
}

__device__ __forceinline__ bool pow_dual_grad_H(const double z[3], double a, Cone3 &K) {      // coneops_powcone.jl:272-285, :408-442
    if (!pow_dual_feasible(z, a)) return false;
    const double phi = pow(z[0] / a, 2.0 * a) * pow(z[1] / (1.0 - a), 2.0 - 2.0 * a);
    const double psi = phi - z[2] * z[2];
    const double gp0 = 2.0 * a * phi / (z[0] * psi), gp1 = 2.0 * (1.0 - a) * phi / (z[1] * psi), gp2 = -2.0 * z[2] / psi;
    K.H[0] = gp0 * gp0 - 2.0 * a * (2.0 * a - 1.0) * phi / (z[0] * z[0] * psi) + (1.0 - a) / (z[0] * z[0]);
    K.H[1] = gp0 * gp1 - 4.0 * a * (1.0 - a) * phi / (z[0] * z[1] * psi);
    K.H[2] = gp1 * gp1 - 2.0 * (1.0 - a) * (1.0 - 2.0 * a) * phi / (z[1] * z[1] * psi) + a / (z[1] * z[1]);
    K.H[3] = gp0 * gp2;
    K.H[4] = gp1 * gp2;
    K.H[5] = gp2 * gp2 + 2.0 / psi;
    K.g[0] = -2.0 * a * phi / (z[0] * psi) - (1.0 - a) / z[0];
    K.g[1] = -2.0 * (1.0 - a) * phi / (z[1] * psi) - a / z[1];
    K.g[2] = 2.0 * z[2] / psi;
    return true;
}
// coneops_powcone.jl:449-478 with _newton_raphson_onesided, coneops_nonsymmetric_common.jl:170-192 (at most 100 steps)
__device__ double pow_newton_raphson(double s3, double phi, double a, int *trips) {
    const double eps = 2.220446049250313e-16, sqrt_eps = 1.4901161193847656e-08;
    double x = -1.0 / s3 + (2.0 * s3 + sqrt(phi * phi / s3 / s3 + 3.0 * phi)) / (phi - s3 * s3);
    const double t0 = -2.0 * a * logsafe(a) - 2.0 * (1.0 - a) * logsafe(1.0 - a);
    int it = 0;
    while (it < 100) {
        it++;
        const double t1 = x * x;
        const double t2 = 2.0 * x / s3, t2d = x * 2.0 / s3;
        const double dfdx = 2.0 * a * a / (a * x + (1.0 + a) / s3) + 2.0 * (1.0 - a) * (1.0 - a) / ((1.0 - a) * x + (2.0 - a) / s3) -
                            2.0 * (x + 1.0 / s3) / (t1 + t2d);
        const double f = 2.0 * a * logsafe(2.0 * a * t1 + (1.0 + a) * t2) + 2.0 * (1.0 - a) * logsafe(2.0 * (1.0 - a) * t1 + (2.0 - a) * t2) -
                         logsafe(phi) - logsafe(t1 + t2) - 2.0 * logsafe(t2) + t0;
        const double dx = -f / dfdx;
        if (dx < eps || fabs(dx / x) < sqrt_eps || fabs(dfdx) < eps) break;
        x += dx;
    }
    *trips = it;
    return x;
}
__device__ __forceinline__ bool pow_gradient_primal(const double s[3], double a, double g[3], int *trips) {   // :256-269, :288-317
    if (!pow_primal_feasible(s, a)) return false;
    const double phi = pow(s[0], 2.0 * a) * pow(s[1], 2.0 - 2.0 * a);
    const double abs_s = fabs(s[2]);
    if (abs_s > 2.220446049250313e-16) {
        g[2] = pow_newton_raphson(abs_s, phi, a, trips);
        if (s[2] < 0.0) g[2] = -g[2];
        g[0] = -(a * g[2] * s[2] + 1.0 + a) / s[0];
        g[1] = -((1.0 - a) * g[2] * s[2] + 2.0 - a) / s[1];
    } else {
        g[2] = 0.0;
        g[0] = -(1.0 + a) / s[0];
        g[1] = -(2.0 - a) / s[1];
    }
    return true;
}

// cholesky_3x3_explicit_factor!, mathutils.jl:427-451, on a pack_triu matrix: does the factorisation go through?
__device__ __forceinline__ bool chol3_ok(const double A[6]) {
    double t = A[0];
    if (!(t > 0.0)) return false;
    const double l11 = sqrt(t), l21 = A[1] / l11;
    t = A[2] - l21 * l21;
    if (!(t > 0.0)) return false;
    const double l22 = sqrt(t), l31 = A[3] / l11, l32 = (A[4] - l21 * l31) / l22;
    t = A[5] - l31 * l31 - l32 * l32;
    return t > 0.0;
}
// cholesky_3x3_explicit_factor! / cholesky_3x3_explicit_solve!, mathutils.jl:427-466: L = {l11, l21, l22, l31, l32, l33} of a pack_triu matrix
__device__ __forceinline__ bool chol3_factor(const double A[6], double L[6]) {
    double t = A[0];
    if (!(t > 0.0)) return false;
    L[0] = sqrt(t);
    L[1] = A[1] / L[0];
    t = A[2] - L[1] * L[1];
    if (!(t > 0.0)) return false;
    L[2] = sqrt(t);
    L[3] = A[3] / L[0];
    L[4] = (A[4] - L[1] * L[3]) / L[2];
    t = A[5] - L[3] * L[3] - L[4] * L[4];
    if (!(t > 0.0)) return false;
    L[5] = sqrt(t);
    return true;
}
__device__ __forceinline__ void chol3_solve(const double L[6], const double b[3], double x[3]) {
    const double l11 = L[0], l21 = L[1], l22 = L[2], l31 = L[3], l32 = L[4], l33 = L[5];
    const double c1 = b[0] / l11;
    const double c2 = (b[1] * l11 - b[0] * l21) / (l11 * l22);
    const double c3 = (b[2] * l11 * l22 - b[1] * l11 * l32 + b[0] * l21 * l32 - b[0] * l22 * l31) / (l11 * l22 * l33);
    x[0] = (c1 * l22 * l33 - c2 * l21 * l33 + c3 * l21 * l32 - c3 * l22 * l31) / (l11 * l22 * l33);
    x[1] = (c2 * l33 - c3 * l32) / (l22 * l33);
    x[2] = c3 / l33;
}

// ---- the start of the non-symmetric cones' line search (step_cone3.hip, step_genpow.hip) ---------------------------------------------
constexpr double kFloatMax3 = 1.7976931348623157e308;
constexpr double kSqrtEps = 1.4901161193847656e-08;

// the scalars of variables.jl:14-43 a fused call hands to the step length: dtau comes from the reduction's device scalars
struct StepTK { const double *dtau; double tau, kappa, rhs_kappa; };

// alpha0 of the non-symmetric cones: min(alpha_tau, alpha_kappa, 1) when T.dtau is given, else alpha_max; then the symmetric cones'
// (alpha_z, alpha_s); then 1 - sqrt(eps) (coneops_compositecone.jl:238-240)
__device__ __forceinline__ double alpha_start(const double *sym2, const StepTK T, double alpha_max) {
    double a = alpha_max;
    if (T.dtau) {
        const double dtau = T.dtau[0];
        const double dkappa = -(T.rhs_kappa + T.kappa * dtau) / T.tau;
        const double a_tau = dtau < 0.0 ? -T.tau / dtau : kFloatMax3;
        const double a_kap = dkappa < 0.0 ? -T.kappa / dkappa : kFloatMax3;
        a = fmin(fmin(a_tau, a_kap), 1.0);
    }
    a = fmin(fmin(a, sym2[0]), sym2[1]);
    return fmin(a, 1.0 - kSqrtEps);
}

}  // namespace hipkkt
