"""A 50-digit reference (mpmath) for the Nesterov-Todd scaling of second-order cones (update_scaling!, coneops_socone.jl:75-157, and the
sparse terms d, u, v of :125-153), the gates that tests/test_soc_scaling_reference.py (CPU) and tests/test_gpu_soc_scaling.py (GPU)
share, and their inputs.  No tests here.

  * `exact_scaling`: the scaling from its DEFINITION (it shares no factored expression with the stand-in or the kernel):
    sbar = s / sqrt(res s), zbar = z / sqrt(res z), gamma = sqrt((1 + <sbar, zbar>) / 2), w = (sbar + J zbar) / (2 gamma),
    eta = (res s / res z)^(1/4), lambda = W z; res x = x0^2 - |x1|^2, J = diag(1, -1, ..., -1);
  * R1 .. R4: residuals of identities that a float64 (w, lambda, eta[, u, v, d]) must satisfy, evaluated at 50 digits.  They are well
    conditioned at every point, whereas the forward error of the scaling grows like eps / (the relative gap (x0 - |x1|) / x0);
  * `emulate_kernel`: k_scaling_soc's order of operations in numpy (strided partial sums of 256 threads, the shuffle tree of a
    wavefront, (r0 + r1) + (r2 + r3) across the four), with switches that plant the defects the tests must be able to see;
  * `allowance`: the first-order bound on the forward error of a float64 evaluation whose sums have the kernel's depth (below);
  * the gates (`Figures`, `residual_gate`, `check_*`) and the two shared cone sets with their early / late points."""
import functools
import math

import numpy as np

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from julia_standin.cones import NonnegativeCone, SecondOrderCone, ZeroCone
from tests import step_reference as sr
from tests.step_reference import V, _mul_W, _mul_Winv, dot, mp, mpf, scaled_point

EPS = 2.0 ** -52
U = 2.0 ** -53            # unit roundoff: one correctly rounded operation moves its result by at most U relative
FACTOR = 8.0              # device residual / error over the host's: the factor of the PSD scaling tests, for the other summation order


def M(a):
    """float64 or 50-digit values -> list of 50-digit numbers"""
    return [x if isinstance(x, mp.mpf) else mpf(float(x)) for x in a]


def m1(x):
    return x if isinstance(x, mp.mpf) else mpf(float(x))


# ---- the exact scaling, from the definition ----------------------------------------------------------------------------------------------

def res(x):
    return x[0] ** 2 - dot(x[1:], x[1:])


def exact_scaling(s, z):
    """(w, lambda, eta) at 50 digits for float64 (s, z) strictly inside the cone"""
    s, z = V(s), V(z)
    rs, rz = res(s), res(z)
    assert rs > 0 and rz > 0 and s[0] > 0 and z[0] > 0
    sbar, zbar = [x / mp.sqrt(rs) for x in s], [x / mp.sqrt(rz) for x in z]
    gamma = mp.sqrt((1 + dot(sbar, zbar)) / 2)
    w = [(sbar[0] + zbar[0]) / (2 * gamma)] + [(a - b) / (2 * gamma) for a, b in zip(sbar[1:], zbar[1:])]
    eta = mp.sqrt(mp.sqrt(rs / rz))
    return w, _mul_W(w, eta, z), eta


def exact_sparse_terms(w):
    """(u, v, d) of D + u u' - v v' = 2 w w' - J, D = diag(d, 1, ..., 1) (coneops_socone.jl:125-153), at 50 digits"""
    w = M(w)
    wsq = dot(w, w)
    d = 1 / (2 * wsq)
    u0 = mp.sqrt(wsq - d)
    u1, v1 = 2 * w[0] / u0, mp.sqrt(2 * (2 + 1 / wsq) / (2 * wsq - 1 / wsq))
    return [u0] + [u1 * x for x in w[1:]], [mpf(0)] + [v1 * x for x in w[1:]], d


# ---- residuals of a float64 (or 50-digit) scaling, as floats -------------------------------------------------------------------------------

def R1(w):
    """the hyperboloid: |w0^2 - |w1|^2 - 1| / w0^2"""
    w = M(w)
    return float(abs(res(w) - 1) / w[0] ** 2)


def R2(w, lam, eta, s, z):
    """max(|W z - lambda|, |W^-1 s - lambda|) / max |lambda|; its unit is eps w0^2"""
    w, lam, eta = M(w), M(lam), m1(eta)
    a, b = _mul_W(w, eta, M(z)), _mul_Winv(w, eta, M(s))
    big = max(abs(x) for x in lam)
    return float(max(max(abs(p - l), abs(q - l)) for p, q, l in zip(a, b, lam)) / big)


def R3(eta, s, z):
    """|eta^4 res(z) - res(s)| / res(s)"""
    rs, rz = res(M(s)), res(M(z))
    return float(abs(m1(eta) ** 4 * rz - rs) / rs)


def r4_vectors(dim):
    """the three fixed random x of R4 for a cone of this dimension"""
    return np.random.default_rng(7700 + dim).standard_normal((3, dim))


def R4(w, u, v, d):
    """|(D + u u' - v v') x - (2 w w' - J) x| / |(2 w w' - J) x|, the largest over r4_vectors; no matrix is formed"""
    w, u, v, d = M(w), M(u), M(v), m1(d)
    worst = mpf(0)
    for x in r4_vectors(len(w)):
        x = V(x)
        ux, vx, wx = dot(u, x), dot(v, x), dot(w, x)
        lhs = [(d if i == 0 else 1) * xi + ui * ux - vi * vx for i, (xi, ui, vi) in enumerate(zip(x, u, v))]
        rhs = [2 * wi * wx - (xi if i == 0 else -xi) for i, (xi, wi) in enumerate(zip(x, w))]
        diff = [p - q for p, q in zip(lhs, rhs)]
        worst = max(worst, mp.sqrt(dot(diff, diff) / dot(rhs, rhs)))
    return float(worst)


RESIDUALS = ("R1", "R2", "R3", "R4")


def residuals(w, lam, eta, s, z, u=None, v=None, d=None):
    """name -> value; R4 only with (u, v, d)"""
    out = dict(R1=R1(w), R2=R2(w, lam, eta, s, z), R3=R3(eta, s, z))
    if u is not None:
        out["R4"] = R4(w, u, v, d)
    return out


def residual_unit(name, w0):
    """eps w0^2 for R2 (the entries of W z cancel from products of size w0^2 |lambda|), eps for the others; w0 from the exact scaling"""
    return EPS * float(w0) ** 2 if name == "R2" else EPS


# ---- the kernel's order of operations in numpy ---------------------------------------------------------------------------------------------

def block_sum_order(terms, first):
    """the sum of terms[first:] as k_scaling_soc forms it: thread t adds the elements first + t, first + t + 256, ... in that order to
    0.0, a wavefront of 64 folds by __shfl_down 32, 16, ..., 1 (lane 0 holds the tree sum), then (r0 + r1) + (r2 + r3)"""
    part = np.zeros(256)
    for base in range(first, len(terms), 256):
        chunk = terms[base:base + 256]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    v = part.reshape(4, 64).copy()
    o = 32
    while o > 0:
        v[:, :o] = v[:, :o] + v[:, o:2 * o]
        o >>= 1
    r = v[:, 0]
    return float((r[0] + r[1]) + (r[2] + r[3]))


def _sqrt_res(x0, x1):
    r = (x0 - x1) * (x0 + x1)
    return math.sqrt(r) if r > 0.0 else 0.0


def emulate_kernel(s, z, drop=None):
    """k_scaling_soc on one cone -> dict(ok, w, lam, eta, eta2, u, v, d) in float64 with the kernel's association and summation order.
    drop = (k, i): the planted defect, element i is left out of the k-th of the four sums (0 |z1|^2, 1 |s1|^2, 2 |w1|^2 before and 3
    after the normalisation)."""
    s, z = np.asarray(s, dtype=np.float64), np.asarray(z, dtype=np.float64)
    dim = len(s)

    def total(k, terms):
        """sums 0, 1, 3 run over i = 1 + t, 1 + t + 256, ...; sum 2 shares the `i = t` loop that stores w and skips element 0 there"""
        terms = terms.copy()
        if drop is not None and drop[0] == k:
            terms[drop[1]] = 0.0
        if k == 2:
            terms[0] = 0.0
        return block_sum_order(terms, 0 if k == 2 else 1)

    z1, s1 = math.sqrt(total(0, z * z)), math.sqrt(total(1, s * s))
    z0, s0 = float(z[0]), float(s[0])
    zscale, sscale = _sqrt_res(z0, z1), _sqrt_res(s0, s1)
    if zscale == 0.0 or sscale == 0.0:
        return dict(ok=False)
    eta = math.sqrt(sscale / zscale)
    w = s / sscale
    w[1:] = w[1:] - z[1:] / zscale
    w[0] = w[0] + z0 / zscale
    w1 = math.sqrt(total(2, w * w))
    wscale = _sqrt_res(s0 / sscale + z0 / zscale, w1)
    if wscale == 0.0:
        return dict(ok=False)
    w[1:] = w[1:] / wscale
    w1sq = total(3, w * w)
    w0 = math.sqrt(1.0 + w1sq)
    gamma = 0.5 * wscale
    cs, cz = (gamma + z0 / zscale) / sscale, (gamma + s0 / sscale) / zscale
    cinv, root = 1.0 / (s0 / sscale + z0 / zscale + 2.0 * gamma), math.sqrt(sscale * zscale)
    lam = np.empty(dim)
    lam[1:] = ((cs * s[1:] + cz * z[1:]) * cinv) * root
    lam[0] = gamma * root
    w[0] = w0
    eta2 = eta * eta
    out = dict(ok=True, w=w, lam=lam, eta=eta, eta2=eta2)
    if dim > 4:
        alpha, wsq = 2.0 * w0, w0 * w0 + w1sq
        wsqinv = 1.0 / wsq
        d = wsqinv / 2.0
        u0 = math.sqrt(wsq - d)
        u1, v1 = alpha / u0, math.sqrt(2.0 * (2.0 + wsqinv) / (2.0 * wsq - wsqinv))
        u, v = u1 * w, v1 * w
        u[0], v[0] = u0, 0.0
        out.update(u=u, v=v, d=d)
    return out


def dense_block(w, eta):
    """the packed upper triangle of eta^2 (2 w w' - J) of a cone of dimension <= 4 with the kernel's association, negated as K holds it"""
    eta2 = eta * eta
    r2 = math.sqrt(2.0)
    wl = [float(x) for x in w]
    out = [-(((r2 * wl[0] - 1.0) * (r2 * wl[0] + 1.0)) * eta2)]
    for col in range(1, len(wl)):
        for row in range(col + 1):
            e = 2.0 * wl[row] * wl[col]
            if row == col:
                e += 1.0
            out.append(-(e * eta2))
    return np.array(out)


# ---- the forward-error allowance of a float64 evaluation with the kernel's summation depth --------------------------------------------------
# One of the kernel's four sums of squares over a cone of dimension dim, relative to the sum of its (non-negative) terms, to first order:
#   * a thread adds ceil(dim / 256) terms one after the other to 0.0: the first addition is exact, so ceil(dim / 256) - 1 rounded ones;
#   * 6 shuffle levels inside a wavefront and 2 additions across the four wavefronts: 8 more on the path of any one term;
#   * the product that forms the term: 1;
#   * the square root taken of the sum: its own rounding U on the root is what 2 U on the radicand gives.
# Every term passes ceil(dim / 256) - 1 + 8 additions at the most, each of which moves a partial sum of non-negative terms by U relative,
# so the sum is within (ceil(dim / 256) + 10) U of the exact one.  SOC(1025): 15 U = 1.7e-15, against step_support.SUM_TOL = 1e-13.

def sum_roundings(dim):
    return -(-dim // 256) + 10


# What else rounds, counted per result in units of U times the MAGNITUDE of the result's terms (|s_i| / sscale + |z_i| / zscale and the
# like, so that a cancellation inside one element is covered): sscale, zscale apart from their sums 3 each (difference, sum, product; the
# root halves them, its own rounding makes 3 again at the most); unnormalised w_i 3 + 1 (division) + 1 (difference) = 5; wscale 4;
# w_i 5 + 4 + 1 = 10; lambda_i: cs 10, cinv 12, root 5, two products, a sum, two more products <= 32; eta 5.  These enter twice more:
# as perturbations of the terms of the third and fourth sum (2 x 5 and 2 x 10 on top of sum_roundings, on sum |w_i| mag_i), and of
# w0' = s0 / sscale + z0 / zscale (5), whose difference with |w1| in wscale amplifies it: that scalar is a bumped slot like a sum.
E_W, E_LAM, E_ETA = 10, 32, 5
N_SLOTS = 5


class _Bumps:
    """sums and amplified scalars in evaluation order; `bump` moves the k-th one by its bound"""

    def __init__(self, bump=None):
        self.k, self.bump = 0, bump

    def _hit(self):
        hit = self.k == self.bump
        self.k += 1
        return hit

    def sumsq(self, a, mag, roundings):
        v = float(np.dot(a, a))
        if self._hit():
            v += roundings * U * float(np.dot(np.abs(a), mag))
        return v

    def scalar(self, x, roundings):
        return x + roundings * U * abs(x) if self._hit() else x


def _twin(S, s, z):
    """update_scaling! with pluggable sums -> ([w | lambda | eta], the magnitudes of their terms)"""
    dim, n = len(s), sum_roundings(len(s))
    z1, s1 = math.sqrt(S.sumsq(z[1:], np.abs(z[1:]), n)), math.sqrt(S.sumsq(s[1:], np.abs(s[1:]), n))
    zscale, sscale = math.sqrt((z[0] - z1) * (z[0] + z1)), math.sqrt((s[0] - s1) * (s[0] + s1))
    eta = math.sqrt(sscale / zscale)
    sb, zb = s / sscale, z / zscale
    w = sb - zb
    w[0] = sb[0] + zb[0]
    mag = np.abs(sb) + np.abs(zb)
    w0p = S.scalar(float(w[0]), 5)
    w1 = math.sqrt(S.sumsq(w[1:], mag[1:], n + 10))
    wscale = math.sqrt((w0p - w1) * (w0p + w1))
    w, mag = w / wscale, mag / wscale
    w[0] = math.sqrt(1.0 + S.sumsq(w[1:], mag[1:], n + 20))
    mag[0] = w[0]
    gamma = 0.5 * wscale
    cs, cz = (gamma + zb[0]) / sscale, (gamma + sb[0]) / zscale
    cinv, root = 1.0 / (w0p + 2.0 * gamma), math.sqrt(sscale * zscale)
    lam = (cs * s + cz * z) * cinv * root
    lmag = (np.abs(cs * s) + np.abs(cz * z)) * cinv * root
    lam[0] = lmag[0] = gamma * root
    return np.concatenate([w, lam, [eta]]), np.concatenate([E_W * mag, E_LAM * lmag, [E_ETA * eta]])


def allowance(s, z):
    """(the twin's [w | lambda | eta], the bound on |float64 evaluation - exact| per entry)"""
    s, z = np.asarray(s, dtype=np.float64), np.asarray(z, dtype=np.float64)
    ref, mags = _twin(_Bumps(), s, z)
    tol = U * mags + 1e-300
    for k in range(N_SLOTS):
        tol = tol + np.abs(_twin(_Bumps(k), s, z)[0] - ref)
    return ref, tol


# ---- shared inputs --------------------------------------------------------------------------------------------------------------------------

def long_specs():
    """step_reference.long_cone_specs plus SOC(3, 4, 5): every pass boundary of both loop shapes, the dense forms, the smallest sparse one"""
    return sr.long_cone_specs() + [cl.SecondOrderConeT(3), cl.SecondOrderConeT(4), cl.SecondOrderConeT(5)]


def many_specs():
    """300 cones: SOC(5 .. 8) interleaved with SOC(2), SOC(3), SOC(4) and Nonnegative cones, so that a sparse cone's index among the
    sparse ones differs from its index among the second-order cones, the offsets into (u, v) are irregular, and a Nonnegative cone
    straddles row 256 and another row 512 (the workgroup edges of k_scaling_diag)"""
    specs, row = [], 0
    for k in range(100):
        group = [cl.SecondOrderConeT(5 + k % 4), cl.SecondOrderConeT(2 + k % 3)]
        row += sum(c.dim for c in group)
        nn = 1 + k % 3
        for edge in (256, 512):
            if row < edge <= row + 8:
                nn = edge - row + 2
        group.append(cl.NonnegativeConeT(nn))
        row += nn
        specs += group
    return specs


CONE_SETS = {"long": long_specs, "many": many_specs}
POINTS = [(seed, late) for late in (False, True) for seed in sr.POINT_SEEDS]


def problem(name):
    from tests.test_gpu_step_edges import _problem
    return _problem(CONE_SETS[name](), 31 if name == "long" else 32)


def host_cones(name, seed, late):
    """(cones, s, z): the stand-in's cones of a set scaled at one of POINTS"""
    cones = cl.CompositeCone(cl.cones_new_collapsed(CONE_SETS[name]()))
    s, z, _ = scaled_point(cones, seed, late)
    return cones, s, z


def soc_list(cones):
    """[(ordinal among the second-order cones, cone, rows, Hs block range, offset into (u, v) or None)]"""
    out, k, uv = [], 0, 0
    for c, r, rb in zip(cones.cones, cones.rng_cones, cones.rng_blocks):
        if isinstance(c, SecondOrderCone):
            out.append((k, c, r, rb, uv if c.is_sparse_expandable else None))
            k += 1
            if c.is_sparse_expandable:
                uv += c.dim
    return out


# ---- figures of one scaling of a cone set against the exact one, and the gates ---------------------------------------------------------------

def _fwd(got, ref):
    """max |got - ref| / max |ref|"""
    return sr.max_err(got, ref) / sr.max_abs(ref)


class Figures:
    """per second-order cone of one (set, point): the exact scaling, the residuals R1 .. R4 and the forward errors of a float64 scaling"""

    def __init__(self, exact, rows):
        self.exact, self.rows = exact, rows      # exact[k] = (w, lam, eta) at 50 digits; rows[k] = dict of floats


def exact_for(cones, s, z):
    return [exact_scaling(s[r], z[r]) for _, _, r, _, _ in soc_list(cones)]


def figures_of(cones, s, z, exact, w, lam, eta, u_all=None, v_all=None, d_of=None):
    """rows of Figures for the float64 scaling (w, lam: m-vectors, eta: per second-order cone, u_all / v_all: concatenated over the
    sparse cones, d_of(k, cone) -> d)"""
    rows = []
    for (k, c, r, _, uv), (ew, el, ee) in zip(soc_list(cones), exact):
        sparse = uv is not None and u_all is not None
        row = residuals(w[r], lam[r], eta[k], s[r], z[r], *((u_all[uv:uv + c.dim], v_all[uv:uv + c.dim], d_of(k, c)) if sparse else ()))
        row.update(dim=c.dim, w0=float(ew[0]), err_w=_fwd(w[r], ew), err_lam=_fwd(lam[r], el), err_eta=float(abs(m1(eta[k]) - ee) / ee),
                   abs_err=np.array([float(abs(m1(g) - t)) for g, t in zip(list(w[r]) + list(lam[r]) + [eta[k]], ew + el + [ee])]))
        rows.append(row)
    return rows


def host_scaling(cones):
    """the scaling that the stand-in's cones hold, in the layout of figures_of: (w, lam, eta, u_all, v_all, d_of)"""
    socs = soc_list(cones)
    w, lam, eta = np.zeros(cones.numel), np.zeros(cones.numel), np.zeros(len(socs))
    for k, c, r, _, _ in socs:
        w[r], lam[r], eta[k] = c.w, c.lam, c.eta
    sparse = [c for _, c, _, _, uv in socs if uv is not None]
    return w, lam, eta, np.concatenate([c.u for c in sparse]), np.concatenate([c.v for c in sparse]), lambda k, c: c.d


@functools.lru_cache(maxsize=None)
def standin_figures(name, seed, late):
    """Figures of the stand-in's own scaling; computed once per (set, point) and shared"""
    cones, s, z = host_cones(name, seed, late)
    exact = exact_for(cones, s, z)
    return Figures(exact, figures_of(cones, s, z, exact, *host_scaling(cones)))


@functools.lru_cache(maxsize=None)
def standin_constants():
    """C per residual: the stand-in's largest normalised residual over all cones, both sets and all points; and its worst forward error
    of w, lambda, eta over the EARLY points"""
    C = {name: 0.0 for name in RESIDUALS}
    early = dict(err_w=0.0, err_lam=0.0, err_eta=0.0)
    for name in CONE_SETS:
        for seed, late in POINTS:
            for row in standin_figures(name, seed, late).rows:
                for rn in RESIDUALS:
                    if rn in row:
                        C[rn] = max(C[rn], row[rn] / residual_unit(rn, row["w0"]))
                if not late:
                    for q in early:
                        early[q] = max(early[q], row[q])
    return C, early


def residual_gate(rn, host_row, C):
    return FACTOR * max(host_row[rn], C[rn] * residual_unit(rn, host_row["w0"]))


def check_rows(tag, rows, host_rows, late, tols, C, early, out=print):
    """the gates of one (set, point): `rows` (the scaling under test) against the stand-in's `host_rows`; tols[k] = allowance of cone k
    (late points).  Prints value / gate per cone and returns the largest ratio per quantity."""
    worst = {}
    failures = []
    for k, (row, host) in enumerate(zip(rows, host_rows)):
        ratios = {}
        for rn in RESIDUALS:
            if rn in row:
                ratios[rn] = row[rn] / residual_gate(rn, host, C)
        if late:
            ratios["fwd"] = float(np.max(row["abs_err"] / tols[k]))
        else:
            for q in early:
                ratios[q] = row[q] / (FACTOR * max(host[q], early[q]))
        out(f"[soc scaling {tag}] cone {k} SOC({row['dim']}) value / gate: " + ", ".join(f"{q} {v:.3f}" for q, v in ratios.items()))
        for q, v in ratios.items():
            worst[q] = max(worst.get(q, 0.0), v)
            if not v <= 1.0:
                failures.append((k, row["dim"], q, v))
    assert not failures, (tag, failures)
    return worst


def late_tolerances(cones, s, z, exact):
    """allowance per second-order cone, after checking that the twin itself stays within it of the exact scaling"""
    tols = []
    for (k, c, r, _, _), (ew, el, ee) in zip(soc_list(cones), exact):
        twin, tol = allowance(s[r], z[r])
        drift = np.array([float(abs(mpf(float(g)) - t)) for g, t in zip(twin, ew + el + [ee])])
        assert np.all(drift <= tol), ("the twin of update_scaling! left its own allowance", c.dim, float(np.max(drift / tol)))
        tols.append(tol)
    return tols


def row0_tolerance(dim):
    """relative bound on K's row-0 entry -eta^2 d of a sparse cone against eta^2 / (2 (w0^2 + |w1|^2)) from the RETURNED (w, eta): the
    kernel's w1sq is one of its tree sums (sum_roundings, which counts a root it does not take here: generous by 2), w0^2 is the square
    of the rounded sqrt(1 + w1sq) (3), then the reciprocal, eta * eta and the product (3; the halving is exact)"""
    return (sum_roundings(dim) + 6) * U


def check_soc_entries(tag, cones, K, map_hs, umaps, w, lam, eta, u_all, v_all):
    """what K holds for the second-order cones, from the returned (w, eta) and the resident (u, v): bit for bit except row 0 of a sparse
    cone (row0_tolerance).  umaps[i] = (u indices, v indices, D pair) of the i-th sparse cone.  -> d per sparse cone, by ordinal"""
    d_of, i = {}, 0
    for k, c, r, rb, uv in soc_list(cones):
        idx = map_hs[rb.start:rb.stop]
        eta2 = float(eta[k]) * float(eta[k])
        if uv is None:
            assert np.array_equal(K[idx], dense_block(w[r], float(eta[k]))), (tag, "dense block", k, c.dim)
            continue
        assert np.all(K[idx[1:]] == -eta2), (tag, "diagonal of a sparse cone", k, c.dim)
        ww = M(w[r])
        d_ref = 1 / (2 * dot(ww, ww))
        want = -mpf(eta2) * d_ref
        rel = float(abs(mpf(float(K[idx[0]])) - want) / abs(want))
        assert rel <= row0_tolerance(c.dim), (tag, "row 0 of a sparse cone", k, c.dim, rel)
        d_of[k] = -float(K[idx[0]]) / eta2
        ui, vi, di = umaps[i]
        i += 1
        u, v = u_all[uv:uv + c.dim], v_all[uv:uv + c.dim]
        assert np.array_equal(K[ui], u * (-eta2)) and np.array_equal(K[vi], v * (-eta2)), (tag, "u / v columns", k, c.dim)
        assert K[di[0]] == -eta2 and K[di[1]] == eta2, (tag, "D pair", k, c.dim)
    return d_of


def check_diag_rows(tag, cones, K, map_hs, s, z, w, lam):
    """Zero and Nonnegative rows: bit for bit"""
    for c, r, rb in zip(cones.cones, cones.rng_cones, cones.rng_blocks):
        idx = map_hs[rb.start:rb.stop]
        if isinstance(c, ZeroCone):
            assert not np.any(w[r]) and not np.any(lam[r]) and not np.any(K[idx]), (tag, "Zero rows")
        elif isinstance(c, NonnegativeCone):
            assert np.array_equal(lam[r], np.sqrt(s[r] * z[r])) and np.array_equal(w[r], np.sqrt(s[r] / z[r])), (tag, "Nonnegative rows")
            assert np.array_equal(K[idx], -(w[r] * w[r])), (tag, "Nonnegative entries of K")
