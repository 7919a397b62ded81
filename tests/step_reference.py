"""A 50-digit reference (mpmath) for the cone algebra of the interior-point step on Zero / Nonnegative / SecondOrder cones, and the
inputs that tests/test_step_reference.py (CPU) and tests/test_gpu_step_edges.py (GPU) share.  No tests here.

Three kinds of reference:
  * `ref_*`: the reference's OWN expressions (coneops_socone.jl:201-216 mul_Hs!, :219-228 / :376-391 affine_ds! / circ_op!, :241-268
    ds_from_dz_offset!, :313-357 mul_W! / mul_Winv!, :443-512 _step_length_soc_component, coneops_symmetric_common.jl:1-36
    combined_ds_shift!, info.jl norm_scaled), association kept, evaluated at 50 digits on float64 inputs: what the stand-in's numbers
    would be without rounding;
  * `def_*`: the DEFINITIONS, which share no factored formula with the stand-in: the dense W = eta [[w0, w1'], [w1, I + w1 w1'/(1 + w0)]],
    shift = (W^-1 ds) o (W dz) - sigma mu e with W^-1 ds obtained as the solution v of W v = ds (verified by multiplying back),
    Hs x = W (W x), offset = W u with Arw(lambda) u = ds (verified by multiplying back), step length = the smallest positive root of
    res(x + alpha y) = 0 capped by alpha_max, with a, b, c from the unfactored y0^2 - |y1|^2 etc. and the root verified in res itself.
    W is materialised up to DENSE_MAX rows; longer cones apply the same rows without forming w1 w1' (soc_W_apply), and
    test_step_reference.py holds that form against the dense matrix at every dimension up to DENSE_MAX;
  * `soc_step_exit`: which exit of _step_length_soc_component a float64 evaluation takes."""
import math

import mpmath
import numpy as np

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from julia_standin.cones import FLOATMAX, SecondOrderCone, _soc_residual
from tests import fixtures as fx

mp = mpmath.mp.clone()
mp.dps = 50
mpf = mp.mpf
DENSE_MAX = 258


def V(a):
    """float64 vector -> list of 50-digit numbers (exact)"""
    return [mpf(float(v)) for v in a]


def dot(a, b):
    return mp.fdot(a, b)


def max_err(got, ref):
    """max_i |got_i - ref_i| with got float64 and ref at 50 digits, as a float"""
    return max(float(abs(mpf(float(g)) - r)) for g, r in zip(got, ref))


def max_abs(ref):
    return max(float(abs(r)) for r in ref)


# ---- the reference's own expressions at 50 digits ---------------------------------------------------------------------------------------

def _residual(z):      # coneops_socone.jl:415-419
    z1 = mp.sqrt(dot(z[1:], z[1:]))
    return (z[0] - z1) * (z[0] + z1)


def _circ(y, z):      # :376-391
    y0, z0 = y[0], z[0]
    return [dot(y, z)] + [y0 * zi + z0 * yi for yi, zi in zip(y[1:], z[1:])]


def ref_affine_ds(lam):
    lam = V(lam)
    return _circ(lam, lam)


def _mul_W(w, eta, x):      # :313-333
    zeta = dot(w[1:], x[1:])
    c = x[0] + zeta / (1 + w[0])
    return [eta * (w[0] * x[0] + zeta)] + [eta * (xi + c * wi) for xi, wi in zip(x[1:], w[1:])]


def _mul_Winv(w, eta, x):      # :336-357
    zeta = dot(w[1:], x[1:])
    c = -x[0] + zeta / (1 + w[0])
    etainv = 1 / eta
    return [etainv * (w[0] * x[0] - zeta)] + [etainv * (xi + c * wi) for xi, wi in zip(x[1:], w[1:])]


def ref_combined_ds_shift(w, eta, dz, ds, sigma_mu):      # coneops_symmetric_common.jl:1-36
    w, eta = V(w), mpf(float(eta))
    zW, sW = _mul_W(w, eta, V(dz)), _mul_Winv(w, eta, V(ds))
    out = _circ(sW, zW)
    out[0] += -mpf(float(sigma_mu))
    return out


def ref_ds_from_dz_offset(w, lam, eta, z, ds):      # :241-268
    w, lam, eta, z, ds = V(w), V(lam), mpf(float(eta)), V(z), V(ds)
    resz = _residual(z)
    l1ds1, w1ds1 = dot(lam[1:], ds[1:]), dot(w[1:], ds[1:])
    out = [z[0]] + [-zi for zi in z[1:]]
    c = lam[0] * ds[0] - l1ds1
    out = [o * (c / resz) for o in out]
    out[0] += eta * w1ds1
    g = w1ds1 / (1 + w[0])
    out[1:] = [o + eta * (dsi + g * wi) for o, dsi, wi in zip(out[1:], ds[1:], w[1:])]
    return [o * (1 / lam[0]) for o in out]


def ref_mul_Hs(w, eta, x):      # :201-216
    w, eta, x = V(w), mpf(float(eta)), V(x)
    c = 2 * dot(w, x)
    y = [-x[0]] + x[1:]
    return [(yi + c * wi) * eta ** 2 for yi, wi in zip(y, w)]


def ref_step_length_soc_component(x, y, alpha_max):      # :443-512
    x, y, alpha_max = V(x), V(y), mpf(float(alpha_max))
    if x[0] >= 0 and y[0] < 0:
        alpha_max = min(alpha_max, -x[0] / y[0])
    a = _residual(y)
    b = 2 * (x[0] * y[0] - dot(x[1:], y[1:]))
    c = max(mpf(0), _residual(x))
    d = b ** 2 - 4 * a * c
    if (a > 0 and b > 0) or d < 0:
        return alpha_max
    if a == 0:
        return alpha_max
    if c == 0:
        return alpha_max if a >= 0 else mpf(0)
    t = (-b - mp.sqrt(d)) if b >= 0 else (-b + mp.sqrt(d))
    r1, r2 = (2 * c) / t, t / (2 * a)
    r1 = mpf(FLOATMAX) if r1 < 0 else r1
    r2 = mpf(FLOATMAX) if r2 < 0 else r2
    return min(alpha_max, r1, r2)


def ref_norm_scaled(m, v):      # info.jl: norm_scaled(m, v) = sqrt(sum_i (m_i v_i)^2)
    return mp.sqrt(mp.fsum((mpf(float(a)) * mpf(float(b)) for a, b in zip(m, v)), squared=True))


def ref_info_norms(d, e, xzs, res):
    """the eight scaled norms of info_update! on [x | z | s] and [rx | rz | rx_inf | rz_inf | Px]; dinv = 1 ./ d and einv = 1 ./ e are
    the float64 quotients that problemdata.jl stores"""
    n, m = len(d), len(e)
    dinv, einv = 1.0 / np.asarray(d), 1.0 / np.asarray(e)
    x, z, s = xzs[:n], xzs[n:n + m], xzs[n + m:]
    o = np.cumsum([0, n, m, n, m, n])
    rx, rz, rx_inf, rz_inf, Px = (res[o[k]:o[k + 1]] for k in range(5))
    return [ref_norm_scaled(*p) for p in ((d, x), (e, z), (einv, s), (dinv, rx), (einv, rz), (dinv, rx_inf), (einv, rz_inf), (dinv, Px))]


# ---- the definitions ------------------------------------------------------------------------------------------------------------------

def soc_W_dense(w, eta):
    """rows of W = eta [[w0, w1'], [w1, I + w1 w1' / (1 + w0)]] at 50 digits"""
    w, eta = V(w), mpf(float(eta))
    dim, f = len(w), 1 / (1 + w[0])
    rows = [[eta * wi for wi in w]]
    for i in range(1, dim):
        wi = w[i] * f
        row = [eta * w[i]] + [eta * (wi * wj) for wj in w[1:]]
        row[i] += eta
        rows.append(row)
    return rows


def soc_W_apply(w, eta, x, dense=None):
    """W x for 50-digit x: by the materialised rows, or (cones longer than DENSE_MAX) row by row without forming w1 w1'"""
    if dense is not None:
        return [dot(row, x) for row in dense]
    w, eta = V(w), mpf(float(eta))
    t = dot(w[1:], x[1:])
    return [eta * (w[0] * x[0] + t)] + [eta * (wi * x[0] + xi + wi * t / (1 + w[0])) for wi, xi in zip(w[1:], x[1:])]


def soc_W_solve(w, eta, b, dense=None):
    """the v with W v = b.  J W J / eta^2 (J = diag(1, -1, ..., -1)) inverts W only as far as w0^2 - |w1|^2 = 1 holds, which a float64 w
    does to 1e-16: it serves as the approximate inverse of an iterative refinement on W itself, and v is accepted only if W v = b"""
    eta_m = mpf(float(eta))

    def approx_inverse(r):
        t = soc_W_apply(w, eta, [r[0]] + [-ri for ri in r[1:]], dense)
        return [t[0] / eta_m ** 2] + [-ti / eta_m ** 2 for ti in t[1:]]

    scale = max(abs(t) for t in b)
    tol = mpf(10) ** -40 * scale * (1 + 2 * mpf(float(w[0])) ** 2)
    v = approx_inverse(b)
    for _ in range(6):
        r = [p - q for p, q in zip(b, soc_W_apply(w, eta, v, dense))]
        if max(abs(t) for t in r) <= tol:
            return v
        v = [p + q for p, q in zip(v, approx_inverse(r))]
    raise AssertionError("W v = b does not hold")


def _arw_solve(lam, b):
    """the u with Arw(lambda) u = lambda o u = b, Arw = [[l0, l1'], [l1, l0 I]]: Schur complement on the first row, then multiplied back"""
    l0, l1 = lam[0], lam[1:]
    u0 = (b[0] - dot(l1, b[1:]) / l0) / (l0 - dot(l1, l1) / l0)
    u = [u0] + [(bi - li * u0) / l0 for bi, li in zip(b[1:], l1)]
    back = [dot(lam, u)] + [li * u[0] + l0 * ui for li, ui in zip(l1, u[1:])]
    scale = max(abs(t) for t in b)
    assert max(abs(p - q) for p, q in zip(back, b)) <= mpf(10) ** -35 * scale * (l0 / (l0 - mp.sqrt(dot(l1, l1)))), "Arw(lambda) u = b does not hold"
    return u


def def_combined_ds_shift(w, eta, dz, ds, sigma_mu, dense=None):
    """`dense`: soc_W_dense(w, eta), or None for the row-by-row form (likewise below)"""
    zW = soc_W_apply(w, eta, V(dz), dense)
    sW = soc_W_solve(w, eta, V(ds), dense)
    out = [dot(sW, zW)] + [sW[0] * zi + zW[0] * si for si, zi in zip(sW[1:], zW[1:])]
    out[0] -= mpf(float(sigma_mu))
    return out


def def_mul_Hs(w, eta, x, dense=None):
    return soc_W_apply(w, eta, soc_W_apply(w, eta, V(x), dense), dense)


def def_ds_from_dz_offset(w, lam, eta, ds, dense=None):
    return soc_W_apply(w, eta, _arw_solve(V(lam), V(ds)), dense)


def def_step_length(x, y, alpha_max):
    """min(alpha_max, the smallest positive root of res(x + alpha y) = (x0 + alpha y0)^2 - |x1 + alpha y1|^2); the linear bound of the
    reference (x0 + alpha y0 >= 0) never binds before that root for an x inside the cone: at x0 + alpha y0 = 0 the residual is <= 0"""
    x, y, cap = V(x), V(y), mpf(float(alpha_max))
    a = y[0] ** 2 - dot(y[1:], y[1:])
    b = 2 * (x[0] * y[0] - dot(x[1:], y[1:]))
    c = x[0] ** 2 - dot(x[1:], x[1:])
    assert c > 0, "x is not inside the cone"
    if a == 0:
        roots = [-c / b] if b != 0 else []
    else:
        disc = b ** 2 - 4 * a * c
        if disc < 0:
            roots = []
        else:
            roots = [(-b - mp.sqrt(disc)) / (2 * a), (-b + mp.sqrt(disc)) / (2 * a)]
    pos = [r for r in roots if r > 0]
    if not pos:
        return cap
    r = min(pos)
    p = [xi + r * yi for xi, yi in zip(x, y)]
    scale = p[0] ** 2 + dot(p[1:], p[1:])
    assert abs(p[0] ** 2 - dot(p[1:], p[1:])) <= mpf(10) ** -30 * scale * (1 + abs(b) / mp.sqrt(abs(b * b - 4 * a * c) + mpf(10) ** -60)), \
        "the root does not zero the residual"
    return min(cap, r)


# ---- which exit of _step_length_soc_component a float64 evaluation takes ------------------------------------------------------------------

def soc_step_exit(x, y, alpha_max):
    """-> dict(exit, r1_replaced, r2_replaced, returned, linear_bound, value): `exit` is one of "interior_dir" (a > 0 and b > 0),
    "d_neg", "a_zero", "c_zero", "two_root_bpos", "two_root_bneg"; `returned` is "cap" (alpha_max, after the linear bound -x0/y0 if
    `linear_bound` says it was lowered), "root" or "zero".  The same float64 operations as julia_standin.cones
    ._step_length_soc_component (coneops_socone.jl:443-512): `value` is its result."""
    info = dict(exit=None, r1_replaced=False, r2_replaced=False, returned="cap", linear_bound=False, value=None)
    if x[0] >= 0 and y[0] < 0:
        lowered = min(alpha_max, -x[0] / y[0])
        info["linear_bound"] = bool(lowered < alpha_max)
        alpha_max = lowered
    a = _soc_residual(y)
    b = 2.0 * (x[0] * y[0] - float(np.dot(x[1:], y[1:])))
    c = max(0.0, _soc_residual(x))
    d = b * b - 4.0 * a * c
    info["value"] = alpha_max
    if a > 0 and b > 0:
        info["exit"] = "interior_dir"
    elif d < 0:
        info["exit"] = "d_neg"
    elif a == 0:
        info["exit"] = "a_zero"
    elif c == 0:
        info["exit"] = "c_zero"
        if not a >= 0:
            info["returned"], info["value"] = "zero", 0.0
    else:
        info["exit"] = "two_root_bpos" if b >= 0 else "two_root_bneg"
        t = (-b - math.sqrt(d)) if b >= 0 else (-b + math.sqrt(d))
        r1, r2 = (2.0 * c) / t, t / (2.0 * a)
        info["r1_replaced"], info["r2_replaced"] = bool(r1 < 0), bool(r2 < 0)
        r1 = FLOATMAX if r1 < 0 else r1
        r2 = FLOATMAX if r2 < 0 else r2
        info["value"] = min(alpha_max, r1, r2)
        info["returned"] = "root" if min(r1, r2) < alpha_max else "cap"
    return info


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------------

LONG_DIMS = (2, 255, 256, 257, 258, 511, 512, 513, 1025)      # 257: second pass of the `i = t` loops; 258: of tail_dot's `i = 1 + t`
POINT_SEEDS = (11, 12)


def long_cone_specs():
    return [cl.ZeroConeT(1), cl.NonnegativeConeT(1)] + [cl.SecondOrderConeT(d) for d in LONG_DIMS]


def exit_cone_specs():
    return [cl.ZeroConeT(1), cl.NonnegativeConeT(1), cl.SecondOrderConeT(2), cl.SecondOrderConeT(3), cl.SecondOrderConeT(258)]


def scaled_point(cones, seed, late):
    """(s, z, rng) of a cone set: fixtures.scale_cones / scale_cones_late from one generator per (seed, late); the host cones are scaled"""
    rng = np.random.default_rng(4000 + 2 * seed + int(late))
    s, z = (fx.scale_cones_late if late else fx.scale_cones)(cones, rng)
    return s, z, rng


def soc_cones(cones):
    return [(c, r) for c, r in zip(cones.cones, cones.rng_cones) if isinstance(c, SecondOrderCone)]


def isolated_directions(x, rng):
    """the three directions of one cone's own rows for the step-length tests: name -> (y, alpha_max)"""
    k = len(x)
    return {
        "hits the boundary": (-(0.5 + rng.random(k)) * x + 0.3 * np.abs(x) * rng.standard_normal(k), 1.0),
        "stays under the cap": (rng.standard_normal(k) * 1e-3 * np.abs(x), 0.7),
        "never hits": (0.5 * x, 1.0),
    }


def binding_direction(x, rng):
    """a direction along which x leaves its cone before alpha = 1: x0 + alpha y0 reaches zero at 1 / (1.5 + u - 0.1 g) < 1"""
    k = len(x)
    return -(1.5 + rng.random(k)) * x + 0.1 * np.abs(x) * rng.standard_normal(k)


def per_cone_directions(cones, s, z, rng):
    """for every cone of the set, in order: (cone, rows, {name: (y_z, y_s, alpha_max)}) from one generator, so that the CPU and the GPU
    test see the same directions"""
    out = []
    for c, r in zip(cones.cones, cones.rng_cones):
        dz, ds = isolated_directions(z[r], rng), isolated_directions(s[r], rng)
        out.append((c, r, {name: (dz[name][0], ds[name][0], dz[name][1]) for name in dz}))
    return out


D_NEG_SCALES = [1.0 + 0.03125 * j for j in range(1, 400)]


def soc_exit_cases(x):
    """Directions y for a point x strictly inside a second-order cone, one per reachable exit of _step_length_soc_component:
    name -> (y, alpha_max, expected) with expected = the fields of soc_step_exit that must hold.

    `d_neg`: for an x inside the cone b^2 >= 4ac holds for EVERY y (the reversed Cauchy-Schwarz inequality of the Lorentz form), so d < 0
    is a rounding event of a double root, y = -k x.  k is the first of D_NEG_SCALES at which the float64 evaluation gives d < 0.  The
    cap is 0.8 / k, below the double root 1 / k: an evaluation whose sums round the other way takes the two-root exit with both roots
    at 1 / k (1 +- 1e-8), and returns the same cap.  In a cone of dimension 2 every sum has one term, so every evaluation rounds alike;
    there the cap is 1 and the returned value is the linear bound -x0 / y0 itself.
    `minus x scaled`: y = (-2 x0, -x1), not a multiple of -x, so that the two positive roots are distinct (d = 4 x0^2 |x1|^2)."""
    dim = len(x)
    x1n = float(np.linalg.norm(x[1:]))
    assert x[0] > x1n > 0.0
    u = x[1:] / x1n
    cases = {}
    y = np.abs(x) + 1.0
    y[0] = float(np.linalg.norm(y[1:])) + 1.0
    y[1:] *= np.sign(x[1:])
    cases["interior"] = (y, 1.0, dict(exit="interior_dir", returned="cap", linear_bound=False))
    y = -x.copy()
    y[0] = -2.0 * x[0]
    cases["minus x scaled"] = (y, 1.0, dict(exit="two_root_bneg", r1_replaced=False, r2_replaced=False, returned="root"))
    y = np.zeros(dim)
    y[0] = 5.0
    if dim == 2:
        y[1] = -5.0
    else:
        y[1:3] = (3.0, 4.0)
    cases["a zero"] = (y, 0.9, dict(exit="a_zero", returned="cap", linear_bound=False))
    y = np.concatenate([[0.25], -3.0 * u])
    cases["outside, b >= 0"] = (y, 1e3, dict(exit="two_root_bpos", r1_replaced=True, r2_replaced=False, returned="root"))
    y = np.concatenate([[-0.25], 3.0 * u])
    cases["outside, b < 0"] = (y, 10.0, dict(exit="two_root_bneg", r1_replaced=False, r2_replaced=True, returned="root"))
    for k in D_NEG_SCALES:
        y = -k * x
        if soc_step_exit(x, y, 1.0)["exit"] == "d_neg":
            cap = 1.0 if dim == 2 else 0.8 / k
            cases["d negative"] = (y, cap, dict(exit="d_neg", returned="cap", linear_bound=(dim == 2)))
            break
    y = np.concatenate([[0.25], -3.0 * u]) * 0.01
    cases["root above the cap"] = (y, 1.0, dict(exit="two_root_bpos", r1_replaced=True, returned="cap"))
    y = np.concatenate([[-0.25], 3.0 * u]) * 0.5
    cases["root below the cap"] = (y, 100.0, dict(exit="two_root_bneg", r2_replaced=True, returned="root"))
    return cases


EXIT_CASE_NAMES = ("interior", "minus x scaled", "a zero", "outside, b >= 0", "outside, b < 0", "d negative", "root above the cap",
                   "root below the cap")
REACHABLE_EXITS = {"interior_dir", "d_neg", "a_zero", "two_root_bpos", "two_root_bneg"}
