"""A 50-digit reference (mpmath) for the interior-point step algebra of the Generalized Power cone (coneops_genpowcone.jl), and the inputs
that tests/test_genpow_reference.py (CPU) and tests/test_gpu_genpow_step.py / tests/test_gpu_genpow_ipm.py (GPU) share.  No tests here.

Two layers, as tests/cone3_reference.py:
  * `ref_*`: the reference's OWN expressions (:249-292 the feasibility expressions, :313-333 barrier_dual, :393-472 gradient_primal! with
    _newton_raphson_genpowcone and the halting rule of coneops_nonsymmetric_common.jl:170-192, :294-310 barrier_primal, :111-135
    mul_Hs! from a given slot), association kept, evaluated at 50 digits on the exact float64 inputs: what the stand-in's and the
    kernels' numbers would be without rounding.
  * `def_*`: the DEFINITIONS, which share no worked-out formula with the stand-in: f*(z) written out with the product (not the
    exponential of a sum of logarithms), the primal gradient from the ROOT of the Newton function (mpmath.findroot, verified in the
    function) with the check grad f*(-g(s)) = -s by differentiating f*, the primal barrier as -f*(-g) - (dim1 + 1).
    The two layers agree to 1e-30 wherever the reference's expression is exact: barrier_dual everywhere, gradient_primal / barrier_primal
    on the branch norm_r <= eps.  On the Newton branch the reference halts once |dx / x| < sqrt(eps) or on the first step that is
    not positive; test_genpow_reference.py measures what that leaves.

Also here: the relative margin of a point (the feasibility expression over the sum of its absolute terms), generators of (s, z) at
prescribed margins for every shape of the GPU tests, constructed line-search directions, and HOST_ERR, the measured error of the float64
stand-in (julia_standin/cones_nonsym.py GenPowerCone) against the `ref_*` layer per bucket (operation, side, margin decade)."""
import math

import mpmath
import numpy as np

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from julia_standin import cones_nonsym as cn

mp = mpmath.mp.clone()
mp.dps = 50
mpf = mp.mpf
EPS64 = float(np.finfo(np.float64).eps)
EPS = mpf(EPS64)
SQRT_EPS = mpf(math.sqrt(EPS64))
FLOATMAX = mpf(float(np.finfo(np.float64).max))
SQRT_EPS64 = math.sqrt(EPS64)


def V(a):
    """float64 vector -> list of 50-digit numbers (exact)"""
    return [mpf(float(v)) for v in a]


def logsafe(v):      # mathutils.jl:12-18
    if v < 0:
        return -FLOATMAX
    if v == 0:
        return -mp.inf
    return mp.log(v)


# ---- the reference's own expressions at 50 digits -----------------------------------------------------------------------------------------

def feasibility_terms(alpha, q, dual):
    """the terms whose sum is the feasibility expression of :249-292: [exp(sum 2 a_i log(q_i [/ a_i])), -w_1^2, ...]; None when a sign
    condition decides.  q: 50-digit numbers or float64"""
    a, q = V(alpha), [mpf(v) for v in q]
    d1 = len(a)
    if not all(v > 0 for v in q[:d1]):
        return None
    res = mpf(0)
    for i in range(d1):
        res += 2 * a[i] * logsafe(q[i] / a[i] if dual else q[i])
    return [mp.exp(res)] + [-w * w for w in q[d1:]]


def margin(alpha, q, dual):
    """the feasibility expression divided by the sum of its absolute terms, at 50 digits; None when a sign condition decides"""
    t = feasibility_terms(alpha, q, dual)
    return None if t is None else float(mp.fsum(t) / mp.fsum(abs(x) for x in t))


def inside(alpha, q, dual):
    t = feasibility_terms(alpha, q, dual)
    return t is not None and mp.fsum(t) > 0


def moved(q, dq, alpha):
    """q + alpha dq at 50 digits from float64 inputs (the device and the stand-in round this; the margins asserted dwarf that)"""
    return [mpf(float(a)) + mpf(float(alpha)) * mpf(float(b)) for a, b in zip(q, dq)]


def ref_barrier_dual(alpha, z):      # :313-333; z: 50-digit numbers
    a = V(alpha)
    d1 = len(a)
    res = mpf(0)
    for i in range(d1):
        res += 2 * a[i] * logsafe(z[i] / a[i])
    res = mp.exp(res) - mp.fsum(w * w for w in z[d1:])
    barrier = -logsafe(res)
    for i in range(d1):
        barrier -= (1 - a[i]) * logsafe(z[i])
    return barrier


def _newton_functions(a, p, norm_r):      # f0, f1 of :452-469
    def f0(x):
        f = -logsafe(2 * x / norm_r + x * x)
        for i in range(len(a)):
            f += 2 * a[i] * (logsafe(x * norm_r + (1 + a[i]) / a[i]) - logsafe(p[i]))
        return f

    def f1(x):
        f = -(2 * x + 2 / norm_r) / (x * x + 2 * x / norm_r)
        for i in range(len(a)):
            f += 2 * a[i] * norm_r / (norm_r * x + (1 + a[i]) / a[i])
        return f
    return f0, f1


def _newton_start(a, phi, norm_r):      # :446, psi = 1 / <alpha, alpha> (cone_types.jl:301)
    psi = 1 / mp.fsum(v * v for v in a)
    return -1 / norm_r + (psi * norm_r + mp.sqrt((phi / norm_r / norm_r + psi * psi - 1) * phi)) / (phi - norm_r * norm_r)


def _newton_halting(x0, f0, f1):      # coneops_nonsymmetric_common.jl:170-192
    x, it = x0, 0
    while it < 100:
        it += 1
        dfdx = f1(x)
        dx = -f0(x) / dfdx
        if dx < EPS or abs(dx / x) < SQRT_EPS or abs(dfdx) < EPS:
            break
        x += dx
    return x, it


def _newton_root(x0, f0, f1):
    x = mp.findroot(f0, x0, df=f1, solver="newton", tol=mpf(10) ** -45, maxsteps=200, verify=False)
    assert abs(f0(x)) <= mpf(10) ** -40, "the Newton function has no root where the iteration ends"
    return x, 0


def _gradient_primal(alpha, s, solve):      # :393-426; s: 50-digit numbers
    a = V(alpha)
    d1 = len(a)
    phi = mpf(1)
    for i in range(d1):
        phi *= s[i] ** (2 * a[i])
    p, r = s[:d1], s[d1:]
    norm_r = mp.sqrt(mp.fsum(w * w for w in r))
    if norm_r > EPS:
        f0, f1 = _newton_functions(a, p, norm_r)
        g1, trips = solve(_newton_start(a, phi, norm_r), f0, f1)
        gr = [g1 * w / norm_r for w in r]
        gp = [-(1 + a[i] + a[i] * g1 * norm_r) / p[i] for i in range(d1)]
    else:
        trips = -1
        gr = [mpf(0)] * len(r)
        gp = [-(1 + a[i]) / p[i] for i in range(d1)]
    return gp + gr, trips


def ref_gradient_primal(alpha, s):
    """-> (g, Newton trips; -1 on the branch norm_r <= eps)"""
    return _gradient_primal(alpha, s, _newton_halting)


def ref_barrier_primal(alpha, s):      # :294-310
    g, _ = ref_gradient_primal(alpha, s)
    return -ref_barrier_dual(alpha, [-v for v in g]) - (len(alpha) + 1)


def ref_barrier(alpha, z, s):
    """compute_barrier at a point, :209-234; z, s float64"""
    return ref_barrier_primal(alpha, V(s)) + ref_barrier_dual(alpha, V(z))


def split_slot(slot, dim1, dim2):
    """[grad | d1 | d2 | p | q | r] (scaling.hip k_scaling_genpow) -> dict of float64 views"""
    d = dim1 + dim2
    o, out = 0, {}
    for name, k in (("grad", d), ("d1", dim1), ("d2", 1), ("p", d), ("q", dim1), ("r", dim2)):
        out[name] = np.asarray(slot[o:o + k], dtype=float)
        o += k
    assert o == len(slot)
    return out


def ref_mul_hs(slot, dim1, dim2, mu, x):
    """mul_Hs! from the resident slot, :111-135 -> (y at 50 digits, first-order propagated sum of absolute terms per row)"""
    S = split_slot(slot, dim1, dim2)
    d1, d2, p, q, r, x, mu = V(S["d1"]), mpf(float(S["d2"][0])), V(S["p"]), V(S["q"]), V(S["r"]), V(x), mpf(float(mu))
    cp, cq, cr = mp.fdot(p, x), mp.fdot(q, x[:dim1]), mp.fdot(r, x[dim1:])
    ap = mp.fsum(abs(u * v) for u, v in zip(p, x))
    aq = mp.fsum(abs(u * v) for u, v in zip(q, x[:dim1]))
    ar = mp.fsum(abs(u * v) for u, v in zip(r, x[dim1:]))
    y, terms = [], []
    for i in range(dim1 + dim2):
        if i < dim1:
            v, t = d1[i] * x[i] - cq * q[i], abs(d1[i] * x[i]) + aq * abs(q[i])
        else:
            v, t = d2 * x[i] - cr * r[i - dim1], abs(d2 * x[i]) + ar * abs(r[i - dim1])
        y.append(mu * (v + cp * p[i]))
        terms.append(float(mu * (t + ap * abs(p[i]))))
    return y, terms


# ---- the definitions ----------------------------------------------------------------------------------------------------------------------

def def_barrier_dual(alpha, z):
    """f*(z) = -log(prod (z_i / a_i)^(2 a_i) - |w|^2) - sum (1 - a_i) log z_i"""
    a = V(alpha)
    d1 = len(a)
    phi = mpf(1)
    for i in range(d1):
        phi *= (z[i] / a[i]) ** (2 * a[i])
    return -mp.log(phi - mp.fsum(w ** 2 for w in z[d1:])) - mp.fsum((1 - a[i]) * mp.log(z[i]) for i in range(d1))


def def_gradient_primal(alpha, s, check=True):
    """g(s) of the conjugate barrier: the root of the Newton function, then -g in the dual cone and grad f*(-g) = -s (verified by
    differentiating f* when `check`)"""
    g, _ = _gradient_primal(alpha, s, _newton_root)
    if check:
        z = [-t for t in g]
        assert inside(alpha, z, True)
        scale = max(abs(t) for t in s)
        for i in range(len(s)):
            d = mp.diff(lambda t: def_barrier_dual(alpha, [z[j] + (t if j == i else 0) for j in range(len(z))]), 0)
            assert abs(d + s[i]) <= mpf(10) ** -30 * scale, "grad f*(-g) = -s does not hold"
    return g


def def_barrier_primal(alpha, s, check=True):
    g = def_gradient_primal(alpha, s, check)
    return -def_barrier_dual(alpha, [-v for v in g]) - (len(alpha) + 1)


# ---- points at prescribed margins ---------------------------------------------------------------------------------------------------------

SHAPES = ((2, 1), (3, 2), (63, 1), (64, 64), (65, 65), (130, 3), (2, 130))      # (dim1, dim2): every loop form of one wavefront per cone
DECADES = (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8)                     # relative margin in [1.5, 6] x decade
SIDES = ("dual", "primal")
PER_SHAPE = 3


def shape_alpha(dim1, seed=0):
    """exponents of a cone of the given dim1: positive, sum 1 (the form problems.nonsymmetric_mix uses)"""
    rng = np.random.default_rng([31, dim1, seed])
    a = rng.uniform(0.2, 1.0, dim1)
    a = a / a.sum()
    a[-1] = 1.0 - a[:-1].sum()
    assert np.all(a > 0) and np.all(a < 1)
    return a


def host_cone(alpha, dim2):
    return cn.GenPowerCone(alpha, dim2)


def central_point(alpha, dim2, dual, rng):
    """a positive multiple of the central ray sqrt(1 + alpha) with w of moderate norm: relative margin 0.3 .. 0.9"""
    a = np.asarray(alpha)
    u = np.sqrt(1.0 + a) * rng.uniform(0.7, 1.4) * (1.0 + 0.1 * rng.uniform(-1, 1, a.size))
    phi = float(np.exp(np.sum(2 * a * np.log(u / a if dual else u))))
    w = rng.standard_normal(dim2)
    w *= math.sqrt(phi * rng.uniform(0.05, 0.5)) / np.linalg.norm(w)
    return np.concatenate([u, w])


def point_at_margin(alpha, dim2, dual, target, rng):
    """a float64 point whose relative margin (see `margin`) is `target` up to the rounding of its entries: (phi - |w|^2) / (phi + |w|^2)"""
    a = np.asarray(alpha)
    t = float(target)
    u = np.sqrt(1.0 + a) * rng.uniform(0.7, 1.4) * (1.0 + 0.1 * rng.uniform(-1, 1, a.size))
    phi = float(mp.exp(mp.fsum(2 * mpf(float(ai)) * mp.log(mpf(float(ui)) / mpf(float(ai)) if dual else mpf(float(ui))) for ai, ui in zip(a, u))))
    w = rng.standard_normal(dim2)
    w *= math.sqrt(phi * (1.0 - t) / (1.0 + t)) / np.linalg.norm(w)
    return np.concatenate([u, w])


def regime_points(shape, side, decade, k):
    """-> (alpha, s, z) of one cone: the `side` at a relative margin in [1.5, 6] x decade, the other side central"""
    dim1, dim2 = shape
    rng = np.random.default_rng([41, dim1, dim2, SIDES.index(side), DECADES.index(decade), k])
    alpha = shape_alpha(dim1, k)
    pts = {}
    for dual in (True, False):
        if dual == (side == "dual"):
            pts[dual] = point_at_margin(alpha, dim2, dual, decade * rng.uniform(1.5, 6.0), rng)
        else:
            pts[dual] = central_point(alpha, dim2, dual, rng)
    return alpha, pts[False], pts[True]


def unit_points(shape, k, norm_r):
    """the unit initialisation (s = z = sqrt(1 + alpha), w = 0: the branch norm_r <= eps), or the same with |w| = norm_r in s"""
    dim1, dim2 = shape
    alpha = shape_alpha(dim1, k)
    c = host_cone(alpha, dim2)
    z, s = np.zeros(c.dim), np.zeros(c.dim)
    c.unit_initialization(z, s)
    if norm_r:
        s[dim1] = norm_r
    return alpha, s, z


def bucket(op, side, decade):
    return (op, side, decade if isinstance(decade, str) else f"{decade:.0e}")


def barrier_error(got, ref):
    """|barrier - ref| / max(1, |ref|) of one cone; inf for a non-finite value"""
    if not np.isfinite(got):
        return float("inf")
    return float(abs(mpf(float(got)) - ref) / max(mpf(1), abs(ref)))


def regime_cases():
    """every (bucket, shape, alpha, s, z) of the barrier regimes, in a fixed order"""
    for side in SIDES:
        for decade in DECADES:
            for shape in SHAPES:
                for k in range(PER_SHAPE):
                    yield (bucket("barrier", side, decade), shape) + regime_points(shape, side, decade, k)
    for name, above in (("w0", 0.0), ("eps", 4.0 * EPS64), ("1e-07", 1e-7)):
        for shape in SHAPES:
            for k in range(PER_SHAPE):
                yield (bucket("barrier", "unit", name), shape) + unit_points(shape, k, above)


# The float64 stand-in (julia_standin/cones_nonsym.py GenPowerCone.compute_barrier at alpha = 0) against ref_barrier on regime_cases():
# the largest barrier_error per bucket, MEASURED by tests/test_genpow_reference.py, which prints each value and asserts that the
# stand-in is still under it (recorded values are the measured ones rounded up to two digits).  The device is held to 10 x these
# (tests/test_gpu_genpow_step.py): it evaluates the same expressions, only log / exp / pow and the order inside a reduction differ.
# ('barrier', 'unit', 'eps'): with 0 < norm_r = 4 eps the Newton start of :446 is the difference of two numbers of size 1 / norm_r whose
# true value is of size norm_r; in float64 it cancels to 0, f1(0) divides by zero and the reference's own expression returns NaN
# (it does for norm_r up to about 1e-9; the 50-digit value is -(dim1 + 1) to 1e-15).  The stand-in's error is therefore infinite,
# and so is the allowance: the device is only required to return, without a trap.  ('barrier', 'unit', '1e-07') is the smallest
# decade of norm_r at which the float64 expression works on every shape.
HOST_ERR = {
    ('barrier', 'dual', '1e-01'): 2.2e-14,
    ('barrier', 'dual', '1e-02'): 3.6e-14,
    ('barrier', 'dual', '1e-03'): 4.0e-14,
    ('barrier', 'dual', '1e-04'): 2.4e-13,
    ('barrier', 'dual', '1e-05'): 1.8e-11,
    ('barrier', 'dual', '1e-06'): 7.5e-11,
    ('barrier', 'dual', '1e-07'): 4.7e-10,
    ('barrier', 'dual', '1e-08'): 4.1e-09,
    ('barrier', 'primal', '1e-01'): 1.2e-14,
    ('barrier', 'primal', '1e-02'): 2.6e-14,
    ('barrier', 'primal', '1e-03'): 3.8e-13,
    ('barrier', 'primal', '1e-04'): 3.7e-12,
    ('barrier', 'primal', '1e-05'): 2.7e-11,
    ('barrier', 'primal', '1e-06'): 3.0e-10,
    ('barrier', 'primal', '1e-07'): 2.0e-09,
    ('barrier', 'primal', '1e-08'): 8.8e-09,
    ('barrier', 'unit', 'w0'): 7.3e-17,
    ('barrier', 'unit', 'eps'): float("inf"),
    ('barrier', 'unit', '1e-07'): 2.4e-16,
}


# ---- constructed line-search directions -----------------------------------------------------------------------------------------------------

def grid_alpha(alpha0, step, k):
    """alpha0 step^k by k multiplications, as backtrack_search forms it"""
    a = alpha0
    for _ in range(k):
        a *= step
    return a


def crossing_between(alpha0, step, k):
    """the geometric mean of the grid points k - 1 and k: grid point k is the first inside"""
    return math.sqrt(grid_alpha(alpha0, step, k - 1) * grid_alpha(alpha0, step, k))


def boundary_direction(alpha, q, dual, alpha_cross):
    """A direction d of one cone's rows along which q + a d is inside the cone exactly for a < alpha_cross: d moves w along itself
    until |w| reaches sqrt(phi) at alpha_cross (|w + a d| is linear in a, phi does not move)"""
    q = np.asarray(q, dtype=float)
    d1 = len(alpha)
    t = feasibility_terms(alpha, q, dual)
    assert t is not None and mp.fsum(t) > 0
    root = float(mp.sqrt(t[0]))
    w = q[d1:]
    nw = float(np.linalg.norm(w))
    assert nw > 0
    d = np.zeros(q.size)
    d[d1:] = w * ((root / nw - 1.0) / alpha_cross)
    return d


def leaving_direction(alpha, q, alpha_min, through_norm):
    """a direction along which q + a d is outside the cone for every a >= alpha_min / 2: the first entry driven negative, or |w| driven
    to ten times the product"""
    q = np.asarray(q, dtype=float)
    d1 = len(alpha)
    d = np.zeros(q.size)
    if through_norm:
        t = feasibility_terms(alpha, q, True)      # (either side: a bound on the product within a factor that 10 x covers)
        root = 10.0 * max(float(mp.sqrt(t[0])), float(np.prod(q[:d1] ** np.asarray(alpha))))
        w = q[d1:]
        d[d1:] = w / np.linalg.norm(w) * (2.0 * root / alpha_min)
    else:
        d[0] = -2.0 * q[0] / alpha_min
    return d


def genpow_spec(alpha, dim2):
    return cl.GenPowerConeT(tuple(float(v) for v in alpha), int(dim2))
