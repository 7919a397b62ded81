"""A 50-digit reference (mpmath) for the interior-point step algebra of the three-row non-symmetric cones (Exponential, Power), and the
inputs that tests/test_cone3_reference.py (CPU) and tests/test_gpu_cone3_step_edges.py (GPU) share.  No tests here.

Two layers:
  * `ref_*`: the reference's OWN expressions (coneops_expcone.jl:319-367 and coneops_powcone.jl:329-405 higher_correction!, :223-248 /
    :228-251 the barriers, :253-281 / :256-285 the feasibility expressions, :284-297 / :288-317 gradient_primal, :412-467 the Wright
    omega algorithm, coneops_nonsymmetric_common.jl:170-192 the one-sided Newton iteration WITH its halting rule), association kept,
    evaluated at 50 digits on the exact float64 inputs: what the stand-in's and the kernels' numbers would be without rounding.
    u = H_dual^-1 ds is solved exactly from the float64 H_dual that is resident (and multiplied back).  Under 1 ms per cone.
  * `def_*`: the DEFINITIONS, which share no worked-out formula with the stand-in: the dual barriers f*(z) written out as functions,
    eta = 1/2 grad^3 f*(z)[u, v] by mpmath.diff with the partial orders (1, 1, 1) on (t_u, t_v, t_i) -> f*(z + t_u u + t_v v + t_i e_i),
    the Wright omega function as lambertw(e^arg), the Exponential primal gradient as the exact conjugate (grad f*(-g) = -s is
    verified), the Power primal gradient from the ROOT of the Newton iteration's function.  0.03 .. 0.08 s per correction.
    The two layers agree to 1e-30 wherever the reference's expression is exact: everywhere except the Power cone's primal gradient
    (and barrier) at alpha != 1/2, where the reference halts at its closed-form start (tests/test_nonsymmetric_cones.py), and the
    Wright omega ALGORITHM, whose two corrector steps leave a truncation error that test_cone3_reference.py measures.

Also here: the relative margin of a point (the feasibility expression over the sum of its absolute terms, at 50 digits), generators
of (s, z) at prescribed margins, the cone sets of the regime tests, the constructed line-search directions, and HOST_ERR, the measured
error of the float64 stand-in against the `ref_*` layer per bucket (see test_cone3_reference.py)."""
import math

import mpmath
import numpy as np

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from julia_standin import cones_nonsym as cn

mp = mpmath.mp.clone()
mp.dps = 50
mpf = mp.mpf
EPS = mpf(float(np.finfo(np.float64).eps))
FLOATMAX = mpf(float(np.finfo(np.float64).max))
SQRT_EPS64 = math.sqrt(float(np.finfo(np.float64).eps))


def V(a):
    """float64 vector -> list of 50-digit numbers (exact)"""
    return [mpf(float(v)) for v in a]


def max_err(got, ref):
    return max(float(abs(mpf(float(g)) - r)) for g, r in zip(got, ref))


def max_abs(ref):
    return max(float(abs(r)) for r in ref)


def logsafe(v):      # mathutils.jl:12-18
    if v < 0:
        return -FLOATMAX
    if v == 0:
        return -mp.inf
    return mp.log(v)


# ---- u = H_dual^-1 ds from the resident float64 matrix ----------------------------------------------------------------------------------

def unpack_triu(t):
    """pack_triu {00, 01, 11, 02, 12, 22} -> 3 x 3 rows of 50-digit numbers"""
    t = V(t)
    return [[t[0], t[1], t[3]], [t[1], t[2], t[4]], [t[3], t[4], t[5]]]


def solve_u(Hd6, ds):
    """the u with H_dual u = ds, by Cramer's rule on the exact float64 entries, multiplied back"""
    H, b = unpack_triu(Hd6), V(ds)

    def det(M):
        return (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])
                + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]))

    d = det(H)
    assert d > 0, "the resident H_dual is not positive definite"
    u = []
    for k in range(3):
        M = [[b[i] if j == k else H[i][j] for j in range(3)] for i in range(3)]
        u.append(det(M) / d)
    back = [mp.fdot(H[i], u) for i in range(3)]
    scale = max(abs(mp.fdot([abs(h) for h in H[i]], [abs(t) for t in u])) for i in range(3))
    assert max(abs(p - q) for p, q in zip(back, b)) <= mpf(10) ** -40 * scale, "H_dual u = ds does not hold"
    return u


# ---- the reference's own expressions at 50 digits -----------------------------------------------------------------------------------------

def ref_exp_correction(Hd6, z, ds, v):      # coneops_expcone.jl:319-367
    u, z, v = solve_u(Hd6, ds), V(z), V(v)
    eta = [mpf(0)] * 3
    eta[1] = mpf(1)
    eta[2] = -z[0] / z[2]
    eta[0] = logsafe(eta[2])
    psi = z[0] * eta[0] - z[0] + z[1]
    dpu, dpv = mp.fdot(eta, u), mp.fdot(eta, v)
    coef = ((u[0] * (v[0] / z[0] - v[2] / z[2]) + u[2] * (z[0] * v[2] / z[2] - v[0]) / z[2]) * psi - 2 * dpu * dpv) / (psi * psi * psi)
    eta = [e * coef for e in eta]
    inv_psi2 = 1 / psi / psi
    eta[0] += ((1 / psi - 2 / z[0]) * u[0] * v[0] / (z[0] * z[0]) - u[2] * v[2] / (z[2] * z[2]) / psi
               + dpu * inv_psi2 * (v[0] / z[0] - v[2] / z[2]) + dpv * inv_psi2 * (u[0] / z[0] - u[2] / z[2]))
    eta[2] += (2 * (z[0] / psi - 1) * u[2] * v[2] / (z[2] * z[2] * z[2]) - (u[2] * v[0] + u[0] * v[2]) / (z[2] * z[2]) / psi
               + dpu * inv_psi2 * (z[0] * v[2] / (z[2] * z[2]) - v[0] / z[2]) + dpv * inv_psi2 * (z[0] * u[2] / (z[2] * z[2]) - u[0] / z[2]))
    return [e / 2 for e in eta], u


def ref_pow_correction(Hd6, z, a, ds, v):      # coneops_powcone.jl:329-405
    u, z, v, a = solve_u(Hd6, ds), V(z), V(v), mpf(float(a))
    phi = (z[0] / a) ** (2 * a) * (z[1] / (1 - a)) ** (2 - 2 * a)
    psi = phi - z[2] * z[2]
    eta = [2 * a * phi / z[0], 2 * (1 - a) * phi / z[1], -2 * z[2]]
    H11 = 2 * a * (2 * a - 1) * phi / (z[0] * z[0])
    H12 = 4 * a * (1 - a) * phi / (z[0] * z[1])
    H22 = 2 * (1 - a) * (1 - 2 * a) * phi / (z[1] * z[1])
    dpu, dpv = mp.fdot(eta, u), mp.fdot(eta, v)
    Hv = [H11 * v[0] + H12 * v[1], H12 * v[0] + H22 * v[1], -2 * v[2]]
    coef = (mp.fdot(u, Hv) * psi - 2 * dpu * dpv) / (psi * psi * psi)
    coef2 = 4 * a * (2 * a - 1) * (1 - a) * phi * (u[0] / z[0] - u[1] / z[1]) * (v[0] / z[0] - v[1] / z[1]) / psi
    inv_psi2 = 1 / psi / psi
    eta[0] = coef * eta[0] - 2 * (1 - a) * u[0] * v[0] / (z[0] * z[0] * z[0]) + coef2 / z[0] + Hv[0] * dpu * inv_psi2
    eta[1] = coef * eta[1] - 2 * a * u[1] * v[1] / (z[1] * z[1] * z[1]) - coef2 / z[1] + Hv[1] * dpu * inv_psi2
    eta[2] = coef * eta[2] + Hv[2] * dpu * inv_psi2
    Hu = [H11 * u[0] + H12 * u[1], H12 * u[0] + H22 * u[1], -2 * u[2]]
    return [(e + h * dpv * inv_psi2) / 2 for e, h in zip(eta, Hu)], u


def ref_correction(kind, Hd6, z, a, ds, v):
    """-> (eta, u) of one cone; combined_ds_shift is grad sigma_mu - eta (coneops_expcone.jl:130-148)"""
    return ref_exp_correction(Hd6, z, ds, v) if kind == "exp" else ref_pow_correction(Hd6, z, a, ds, v)


def ref_shift(kind, slot, z, a, dz, ds, sigma_mu):
    """combined_ds_shift of one cone from its resident 15 doubles [pack_triu(Hs) | pack_triu(H_dual) | grad]"""
    eta, _ = ref_correction(kind, slot[6:12], z, a, ds, dz)
    return [g * mpf(float(sigma_mu)) - e for g, e in zip(V(slot[12:15]), eta)]


def ref_mul_hs(slot, x):
    H, x = unpack_triu(slot[0:6]), V(x)
    return [mp.fdot(H[i], x) for i in range(3)]


def ref_wright_omega(z):      # coneops_expcone.jl:412-467: the ALGORITHM at 50 digits (series or asymptotic start, two corrector steps)
    assert z >= 0
    if z < 1 + mp.pi:
        zm1 = z - 1
        p = zm1
        w = 1 + p / 2
        p *= zm1
        w += p / 16
        p *= zm1
        w -= p / 192
        p *= zm1
        w -= p / 3072
        p *= zm1
        w += mpf(13) / 61440 * p
    else:
        logz = logsafe(z)
        zinv = 1 / z
        w = z - logz
        q = logz * zinv
        w += q
        q *= zinv
        w += q * (logz / 2 - 1)
        w += q * (logz * logz / 3 - mpf(3) / 2 * logz + 1)      # (:451 does not store q * zinv)
    r = z - w - logsafe(w)
    for _ in range(2):
        wp1 = w + 1
        t = wp1 * (wp1 + (2 * r) / 3)
        w *= 1 + (r / wp1) * (t - r / 2) / (t - r)
        r = (2 * w * w - 8 * w - 1) / (72 * wp1 ** 6) * r ** 4
    return w


def exp_omega_argument(s):
    s = V(s)
    return 1 - s[0] / s[1] - logsafe(s[1] / s[2])


def ref_exp_barrier_dual(z):      # :223-232
    z = V(z)
    lg = logsafe(-z[2] / z[0])
    return -logsafe(-z[2] * z[0]) - logsafe(z[1] - z[0] - z[0] * lg)


def _exp_barrier_primal(s, omega):      # :234-248
    s = V(s)
    om = omega(exp_omega_argument(s))
    om = (om - 1) * (om - 1) / om
    return -logsafe(om) - 2 * logsafe(s[1]) - logsafe(s[2]) - 3


def _exp_gradient_primal(s, omega):      # :284-297
    s = V(s)
    om = omega(exp_omega_argument(s))
    g1 = 1 / ((om - 1) * s[1])
    return [g1, g1 + g1 * logsafe(om * s[1] / s[2]) - 1 / s[1], om / ((1 - om) * s[2])]


def ref_exp_barrier_primal(s):
    return _exp_barrier_primal(s, ref_wright_omega)


def ref_exp_gradient_primal(s):
    return _exp_gradient_primal(s, ref_wright_omega)


def _pow_phi_dual(z, a):
    return (z[0] / a) ** (2 * a) * (z[1] / (1 - a)) ** (2 - 2 * a)


def ref_pow_barrier_dual(z, a):      # coneops_powcone.jl:228-237
    z, a = V(z), mpf(float(a))
    return -logsafe(_pow_phi_dual(z, a) - z[2] * z[2]) - (1 - a) * logsafe(z[0]) - a * logsafe(z[1])


def _pow_newton_functions(s3, phi, a):      # :449-478
    t0 = -2 * a * logsafe(a) - 2 * (1 - a) * logsafe(1 - a)

    def f0(x):
        t1, t2 = x * x, 2 * x / s3
        return (2 * a * logsafe(2 * a * t1 + (1 + a) * t2) + 2 * (1 - a) * logsafe(2 * (1 - a) * t1 + (2 - a) * t2)
                - logsafe(phi) - logsafe(t1 + t2) - 2 * logsafe(t2) + t0)

    def f1(x):
        t1, t2 = x * x, x * 2 / s3
        return 2 * a * a / (a * x + (1 + a) / s3) + 2 * (1 - a) * (1 - a) / ((1 - a) * x + (2 - a) / s3) - 2 * (x + 1 / s3) / (t1 + t2)

    x0 = -1 / s3 + (2 * s3 + mp.sqrt(phi * phi / s3 / s3 + 3 * phi)) / (phi - s3 * s3)
    return x0, f0, f1


def _pow_gradient_primal(s, a, root):      # :288-317; `root`: (x0, f0, f1) -> g3 for |s3|
    s, a = V(s), mpf(float(a))
    phi = s[0] ** (2 * a) * s[1] ** (2 - 2 * a)
    abs_s = abs(s[2])
    if abs_s > EPS:
        g3 = root(*_pow_newton_functions(abs_s, phi, a))
        if s[2] < 0:
            g3 = -g3
        return [-(a * g3 * s[2] + 1 + a) / s[0], -((1 - a) * g3 * s[2] + 2 - a) / s[1], g3], a
    return [-(1 + a) / s[0], -(2 - a) / s[1], mpf(0)], a


def _newton_onesided(x0, f0, f1):      # coneops_nonsymmetric_common.jl:170-192, the halting rule with the float64 constants
    x, it = x0, 0
    while it < 100:
        it += 1
        dfdx = f1(x)
        dx = -f0(x) / dfdx
        if dx < EPS or abs(dx / x) < mp.sqrt(EPS) or abs(dfdx) < EPS:
            break
        x += dx
    return x


def _newton_root(x0, f0, f1):
    """the root itself: Newton from x0 on the 50-digit function until the correction vanishes, then f0(root) = 0 is checked"""
    x = x0
    for _ in range(200):
        dx = -f0(x) / f1(x)
        x += dx
        if abs(dx) <= mpf(10) ** -45 * abs(x):
            break
    assert abs(f0(x)) <= mpf(10) ** -40, "the Newton iteration of the definition did not reach the root"
    return x


def ref_pow_gradient_primal(s, a):
    return _pow_gradient_primal(s, a, _newton_onesided)[0]


def _pow_barrier_primal(s, a, root):      # :239-251
    g, a = _pow_gradient_primal(s, a, root)
    return logsafe((-g[0] / a) ** (2 * a) * (-g[1] / (1 - a)) ** (2 - 2 * a) - g[2] * g[2]) + (1 - a) * logsafe(-g[0]) + a * logsafe(-g[1]) - 3


def ref_pow_barrier_primal(s, a):
    return _pow_barrier_primal(s, a, _newton_onesided)


def ref_barrier(kind, z, s, a):
    """compute_barrier of one cone at the point (z, s): barrier_dual + barrier_primal"""
    if kind == "exp":
        return ref_exp_barrier_dual(z) + ref_exp_barrier_primal(s)
    return ref_pow_barrier_dual(z, a) + ref_pow_barrier_primal(s, a)


# feasibility expressions -> the list of terms whose sum is the expression, or None when a sign condition decides

def feasibility_terms(kind, q, a, dual):
    q = V(q)
    if kind == "exp":
        if dual:      # :269-281
            if not (q[2] > 0 and q[0] < 0):
                return None
            return [q[1], -q[0], -q[0] * logsafe(-q[2] / q[0])]
        if not (q[2] > 0 and q[1] > 0):      # :253-266
            return None
        return [q[1] * logsafe(q[2] / q[1]), -q[0]]
    a = mpf(float(a))
    if not (q[0] > 0 and q[1] > 0):
        return None
    if dual:      # coneops_powcone.jl:272-285
        return [mp.exp(2 * a * logsafe(q[0] / a) + 2 * (1 - a) * logsafe(q[1] / (1 - a))), -q[2] * q[2]]
    return [mp.exp(2 * a * logsafe(q[0]) + 2 * (1 - a) * logsafe(q[1])), -q[2] * q[2]]      # :256-269


def margin(kind, q, a, dual):
    """the feasibility expression divided by the sum of its absolute terms, at 50 digits; None when a sign condition decides"""
    t = feasibility_terms(kind, q, a, dual)
    return None if t is None else float(mp.fsum(t) / mp.fsum(abs(x) for x in t))


def inside(kind, q, a, dual):
    t = feasibility_terms(kind, q, a, dual)
    return t is not None and mp.fsum(t) > 0


# ---- the definitions ----------------------------------------------------------------------------------------------------------------------

def def_exp_barrier_dual(z):
    """f*(z) = -log(z2 - z1 - z1 log(z3 / -z1)) - log(-z1) - log(z3)"""
    return -mp.log(z[1] - z[0] - z[0] * mp.log(z[2] / -z[0])) - mp.log(-z[0]) - mp.log(z[2])


def def_pow_barrier_dual(z, a):
    """f*(z) = -log((z1 / a)^(2a) (z2 / (1 - a))^(2 - 2a) - z3^2) - (1 - a) log z1 - a log z2"""
    return -mp.log((z[0] / a) ** (2 * a) * (z[1] / (1 - a)) ** (2 - 2 * a) - z[2] ** 2) - (1 - a) * mp.log(z[0]) - a * mp.log(z[1])


def def_barrier_dual(kind, z, a):
    return def_exp_barrier_dual(V(z)) if kind == "exp" else def_pow_barrier_dual(V(z), mpf(float(a)))


def def_correction(kind, z, a, u, v):
    """eta = 1/2 grad^3 f*(z)[u, v]: the mixed third derivative of (t_u, t_v, t_i) -> f*(z + t_u u + t_v v + t_i e_i) at 0, for i = 1, 2, 3;
    u at 50 digits (solve_u), v float64"""
    z, v = V(z), V(v)
    a = None if kind == "exp" else mpf(float(a))
    f = def_exp_barrier_dual if kind == "exp" else (lambda p: def_pow_barrier_dual(p, a))
    eta = []
    for i in range(3):
        e = [mpf(int(j == i)) for j in range(3)]
        eta.append(mp.diff(lambda tu, tv, ti: f([z[j] + tu * u[j] + tv * v[j] + ti * e[j] for j in range(3)]), (0, 0, 0), (1, 1, 1)) / 2)
    return eta


def def_wright_omega(z):
    """omega(z) with omega + log(omega) = z: W(e^z), verified in the defining equation"""
    w = mp.lambertw(mp.exp(z))
    assert abs(w + mp.log(w) - z) <= mpf(10) ** -45 * (1 + abs(z))
    return w


def def_exp_barrier_primal(s):
    return _exp_barrier_primal(s, def_wright_omega)


def def_exp_gradient_primal(s):
    """g(s) of the conjugate barrier: the g with -g in the dual cone and grad f*(-g) = -s (verified by differentiating f*)"""
    g = _exp_gradient_primal(s, def_wright_omega)
    z = [-t for t in g]
    assert z[2] > 0 and z[0] < 0 and z[1] - z[0] - z[0] * mp.log(-z[2] / z[0]) > 0
    for i in range(3):
        d = mp.diff(lambda t: def_exp_barrier_dual([z[j] + (t if j == i else 0) for j in range(3)]), 0)
        assert abs(d + mpf(float(s[i]))) <= mpf(10) ** -30 * max(abs(mpf(float(t))) for t in s), "grad f*(-g) = -s does not hold"
    return g


def def_pow_gradient_primal(s, a):
    return _pow_gradient_primal(s, a, _newton_root)[0]


def def_pow_barrier_primal(s, a):
    return _pow_barrier_primal(s, a, _newton_root)


def def_barrier(kind, z, s, a):
    if kind == "exp":
        return def_exp_barrier_dual(V(z)) + def_exp_barrier_primal(s)
    return def_pow_barrier_dual(V(z), mpf(float(a))) + def_pow_barrier_primal(s, a)


# ---- points at prescribed margins ---------------------------------------------------------------------------------------------------------

KINDS = ("exp", "pow")
DECADES = ("central", 1e-2, 1e-4, 1e-6)      # relative margin in [d, 10 d)
SCALES = (1e-6, 1.0, 1e6)
ALPHAS = (0.001, 0.1, 0.101, 0.5, 0.899, 0.9, 0.999)
PER_KIND = 64


def _host_cone(kind, a):
    return cn.ExponentialCone() if kind == "exp" else cn.PowerCone(a)


def central_point(kind, a, dual, rng, variant=0):
    """a positive multiple of the cone's central ray plus a perturbation that stays inside (fixtures.scale_cones_nonsymmetric).
    Exponential primal points: the central ray has the Wright-omega argument 1 + 2.7, just below the branch at 1 + pi; variant 1 moves
    s1 down so that the argument lies in (1 + pi, 12), variant 2 far down (argument 20 .. 500: deep interior)."""
    c = _host_cone(kind, a)
    q0 = np.zeros(3)
    c.unit_initialization(np.zeros(3), q0)      # (z = s on the central ray)
    feasible = c.is_dual_feasible if dual else c.is_primal_feasible
    for _ in range(200):
        t = q0 * rng.uniform(0.5, 2.0) + 0.2 * rng.standard_normal(3)
        if kind == "exp" and not dual and variant == 1:
            t[0] -= rng.uniform(1.0, 8.0) * abs(t[1])
        if kind == "exp" and not dual and variant == 2:
            t[0] -= rng.uniform(20.0, 500.0) * abs(t[1])
        if kind == "pow" and variant == 3:
            t[2] = 0.0      # the branch |s3| <= eps of gradient_primal
        if feasible(t) and feasible(q0 + 0.5 * (t - q0)):
            return t
    raise AssertionError("no interior point")


def point_at_margin(kind, a, dual, target, rng):
    """a float64 point whose relative margin (see `margin`) is `target` up to the rounding of its entries"""
    t = float(target)
    if kind == "exp":
        if dual:
            z1, z3 = -rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0)
            lg = math.log(-z3 / z1)
            A, B = -z1 - z1 * lg, abs(z1) + abs(z1 * lg)
            z2 = (t * B - A) / (1.0 - t)
            if z2 < 0:
                z2 = (t * B - A) / (1.0 + t)
            return np.array([z1, z2, z3])
        s2, s3 = rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0)
        L = s2 * math.log(s3 / s2)
        s1 = (L - t * abs(L)) / (1.0 + t)
        if s1 < 0:
            s1 = (L - t * abs(L)) / (1.0 - t)
        return np.array([s1, s2, s3])
    q1, q2 = rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0)
    phi = (q1 / a) ** (2 * a) * (q2 / (1 - a)) ** (2 - 2 * a) if dual else q1 ** (2 * a) * q2 ** (2 - 2 * a)
    q3 = math.sqrt(phi * (1.0 - t) / (1.0 + t)) * (1.0 if rng.random() < 0.5 else -1.0)
    return np.array([q1, q2, q3])


def regime_set(decade, side, scale, seed=0):
    """PER_KIND Exponential then PER_KIND Power cones (the alphas of ALPHAS in turn) with the `side` ("dual": z, "primal": s) of every
    cone at a relative margin in [1.5, 6] x decade and the other side central, everything times `scale`
    -> (kinds, alphas, s, z): lists of length 2 PER_KIND and arrays of 6 PER_KIND rows in that order"""
    rng = np.random.default_rng([17, seed, DECADES.index(decade), ("dual", "primal").index(side), SCALES.index(scale)])
    kinds, alphas, s, z = [], [], [], []
    for kind in KINDS:
        for i in range(PER_KIND):
            a = 0.0 if kind == "exp" else ALPHAS[i % len(ALPHAS)]
            variant = i % 4 if kind == "exp" else (3 if i == len(ALPHAS) else 0)      # (s3 = 0: the first cone after one of every alpha)
            pts = {}
            for dual in (True, False):
                if decade != "central" and dual == (side == "dual"):
                    pts[dual] = point_at_margin(kind, a, dual, decade * rng.uniform(1.5, 6.0), rng)
                else:
                    pts[dual] = central_point(kind, a, dual, rng, variant)
            kinds.append(kind)
            alphas.append(a)
            z.append(pts[True] * scale)
            s.append(pts[False] * scale)
    return kinds, alphas, np.concatenate(s), np.concatenate(z)


def regime_specs(kinds, alphas):
    return [cl.ExponentialConeT() if k == "exp" else cl.PowerConeT(a) for k, a in zip(kinds, alphas)]


def regime_directions(decade, side, scale, m):
    """(dz, ds) of a regime set: N(0, 1) times the scale of the points"""
    rng = np.random.default_rng([23, DECADES.index(decade), ("dual", "primal").index(side), SCALES.index(scale)])
    return scale * rng.standard_normal(m), scale * rng.standard_normal(m)


def bucket(op, kind, side, decade):
    return (op, kind, side, "central" if decade == "central" else f"{decade:.0e}")


def correction_error(got_eta, ref_eta):
    """max |eta - ref| / max |ref| of one cone"""
    return max_err(got_eta, ref_eta) / max(max_abs(ref_eta), 1e-300)


def barrier_error(got, ref):
    """|barrier - ref| / max(1, |ref|) of one cone"""
    return float(abs(mpf(float(got)) - ref) / max(mpf(1), abs(ref)))


# The float64 stand-in (julia_standin/cones_nonsym.py) against the `ref_*` layer on the regime sets: the largest error per bucket over
# the three scales, MEASURED by tests/test_cone3_reference.py (which prints them and holds the stand-in to 10 x these); the device is
# held to 10 x these as well (tests/test_gpu_cone3_step_edges.py).  correction: correction_error; barrier: barrier_error of
# barrier_dual + barrier_primal at the point.  The correction's `side` is always "dual" (it is evaluated at z); "central" has both
# sides central.
HOST_ERR = {
    ('barrier', 'exp', 'dual', 'central'): 3.05e-16,
    ('barrier', 'exp', 'dual', '1e-02'): 3.35e-15,
    ('barrier', 'exp', 'dual', '1e-04'): 9.45e-14,
    ('barrier', 'exp', 'dual', '1e-06'): 6.72e-12,
    ('barrier', 'exp', 'primal', '1e-02'): 1.01e-13,
    ('barrier', 'exp', 'primal', '1e-04'): 3.66e-12,
    ('barrier', 'exp', 'primal', '1e-06'): 1.13e-10,
    ('barrier', 'pow', 'dual', 'central'): 1.38e-15,
    ('barrier', 'pow', 'dual', '1e-02'): 7.55e-15,
    ('barrier', 'pow', 'dual', '1e-04'): 1.97e-13,
    ('barrier', 'pow', 'dual', '1e-06'): 7.56e-12,
    ('barrier', 'pow', 'primal', '1e-02'): 2.72e-14,
    ('barrier', 'pow', 'primal', '1e-04'): 4.25e-13,
    ('barrier', 'pow', 'primal', '1e-06'): 2.91e-11,
    ('correction', 'exp', 'dual', 'central'): 2.68e-15,
    ('correction', 'exp', 'dual', '1e-02'): 4.44e-13,
    ('correction', 'exp', 'dual', '1e-04'): 5.22e-09,
    ('correction', 'exp', 'dual', '1e-06'): 8.06e-05,
    ('correction', 'pow', 'dual', 'central'): 1.42e-14,
    ('correction', 'pow', 'dual', '1e-02'): 1.12e-11,
    ('correction', 'pow', 'dual', '1e-04'): 2.96e-08,
    ('correction', 'pow', 'dual', '1e-06'): 4.92e-04,
    ('gradient_primal', 'exp', 'dual', 'central'): 3.91e-16,
    ('gradient_primal', 'exp', 'dual', '1e-02'): 4.21e-16,
    ('gradient_primal', 'exp', 'dual', '1e-04'): 4.08e-16,
    ('gradient_primal', 'exp', 'dual', '1e-06'): 5.80e-16,
    ('gradient_primal', 'exp', 'primal', '1e-02'): 7.93e-13,
    ('gradient_primal', 'exp', 'primal', '1e-04'): 1.73e-10,
    ('gradient_primal', 'exp', 'primal', '1e-06'): 3.04e-09,
}


# ---- constructed line-search directions -----------------------------------------------------------------------------------------------------

def grid_alpha(alpha0, step, k):
    """alpha0 step^k by k multiplications, as backtrack_search forms it"""
    a = alpha0
    for _ in range(k):
        a *= step
    return a


def boundary_direction(kind, q, a, dual, alpha_cross, sign=None):
    """A direction d of one cone's rows along which q + alpha d is inside the cone exactly for alpha < alpha_cross (up to rounding far
    below the margins that the tests assert): d moves only the row in which the feasibility expression is monotone -- z2 resp. s1 of
    the Exponential cone (the expression is linear in it), z3 resp. s3 of the Power cone (away from zero, towards +-sqrt(phi))."""
    q = np.asarray(q, dtype=float)
    d = np.zeros(3)
    if kind == "exp":
        t = feasibility_terms(kind, q, a, dual)
        assert t is not None
        feas = float(mp.fsum(t))
        assert feas > 0
        if dual:
            d[1] = -feas / alpha_cross      # z2 - feas: the expression reaches zero at alpha_cross
        else:
            d[0] = feas / alpha_cross       # s1 + feas
        return d
    t = feasibility_terms(kind, q, a, dual)
    assert t is not None
    root = float(mp.sqrt(t[0]))
    sgn = (1.0 if q[2] >= 0 else -1.0) if sign is None else sign
    d[2] = (sgn * root - q[2]) / alpha_cross
    return d


def crossing_between(alpha0, step, k):
    """the geometric mean of the grid points k - 1 and k: grid point k is the first inside"""
    return math.sqrt(grid_alpha(alpha0, step, k - 1) * grid_alpha(alpha0, step, k))
