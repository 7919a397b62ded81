"""The default start of a symmetric cone set restated for the tests of the device-resident start (include/hipkkt.h
hipkkt_cone_margins / hipkkt_cone_shift_to_interior / hipkkt_step_default_start_dev): margins(::CompositeCone)
(coneops_compositecone.jl:49-63 with the per-cone rules of coneops_zerocone.jl:27-39, coneops_nncone.jl:19-38, coneops_socone.jl:13-22,
coneops_psdtrianglecone.jl:8-27) and _shift_to_cone_interior! (variables.jl:180-208), with JULIA's NaN semantics: `min` and `max`
propagate a NaN (Python's keep their first argument), `x > 0 ? x : 0` drops it, and a NaN min_margin fails both comparisons of the
shift, so the last arm (shift by 0) is taken.

Three layers:
  margins64 / shift64        float64, in the reference's order of operations (cone order); what the stand-in computes on finite inputs
  margins_mp                 the same margins at 50 digits (mpmath; eigenvalues by mp.eigsy as tests/psd_scaling_reference.py uses it),
                             with what the tests' gates need: the binding cone, the scale of every sum, |Z|_2 of every PSD cone
  decision / apply_shift     the three arms for a GIVEN (min_margin, pos_margin) resp. (min_margin, target), bit for bit
A plain module: it holds no test and changes no pytest setting."""
import math

import mpmath
import numpy as np

import clarabel_jl_amd  # noqa: F401
from julia_standin.cones import NonnegativeCone, PSDTriangleCone, SecondOrderCone, ZeroCone

mp = mpmath.mp.clone()
mp.dps = 50
mpf = mp.mpf
EPS = float(np.finfo(np.float64).eps)
FLOATMAX = float(np.finfo(np.float64).max)
PD = {"primal": 0, "dual": 1, 0: 0, 1: 1}


def jl_min(a, b):
    return a if (a < b or a != a) else b


def jl_max(a, b):
    return a if (a > b or a != a) else b


# ---- float64, the reference's order -------------------------------------------------------------------------------------------------

def cone_margins64(c, z):
    if isinstance(c, ZeroCone):
        return FLOATMAX, 0.0
    if isinstance(c, NonnegativeCone):
        alpha = FLOATMAX
        for v in z:                       # minimum(z): a NaN anywhere gives NaN
            alpha = jl_min(alpha, float(v))
        beta = 0.0
        for v in z:
            beta += float(v) if v > 0 else 0.0
        return alpha, beta
    if isinstance(c, SecondOrderCone):
        alpha = float(z[0] - np.linalg.norm(z[1:]))
        return alpha, jl_max(0.0, alpha)
    if isinstance(c, PSDTriangleCone):
        if z.size == 0:
            return FLOATMAX, 0.0
        if not np.all(np.isfinite(z)):     # (LAPACK would throw; the device gives NaN margins)
            return float("nan"), float("nan")
        ev = np.linalg.eigvalsh(c.svec_to_mat(z))
        beta = 0.0
        for e in ev:
            beta = beta + float(e) if e > 0 else beta
        return float(ev.min()), beta
    raise TypeError(type(c).__name__)


def margins64(cones, z):
    alpha, beta = FLOATMAX, 0.0
    for c, r in zip(cones.cones, cones.rng_cones):
        a, b = cone_margins64(c, z[r])
        alpha = jl_min(alpha, a)
        beta += b
    return alpha, beta


def target_of(pos_margin, degree):
    """max(1, 0.1 pos_margin / degree); degree 0 gives 1 as the stand-in does"""
    return jl_max(1.0, 0.1 * pos_margin / degree) if degree > 0 else 1.0


def branch_of(min_margin, target):
    """0 / 1 / 2 = the three arms of variables.jl:189-204 in source order"""
    if min_margin <= 0:
        return 0
    if min_margin < target:
        return 1
    return 2


def unit_shift(cones, v, a, pd):
    """scaled_unit_shift!(cones, v, a, pd) in place"""
    pd = PD[pd]
    for c, r in zip(cones.cones, cones.rng_cones):
        if isinstance(c, ZeroCone):
            if pd == 0:
                v[r] = 0.0
        elif isinstance(c, NonnegativeCone):
            v[r] += a
        elif isinstance(c, SecondOrderCone):
            v[r.start] += a
        elif isinstance(c, PSDTriangleCone):
            v[r.start + c._diagidx] += a
        else:
            raise TypeError(type(c).__name__)


def apply_shift(cones, v, pd, min_margin, target):
    """-> (shifted copy, branch) for the given (min_margin, target): arm 0 adds -min_margin and then target (two additions), arm 1
    target - min_margin, arm 2 adds 0.0 (which turns -0.0 into +0.0)"""
    w = np.array(v, dtype=np.float64, copy=True)
    br = branch_of(min_margin, target)
    if br == 0:
        unit_shift(cones, w, -min_margin, pd)
        unit_shift(cones, w, target, pd)
    elif br == 1:
        unit_shift(cones, w, target - min_margin, pd)
    else:
        unit_shift(cones, w, 0.0, pd)
    return w, br


def shift64(cones, v, pd):
    """_shift_to_cone_interior! of a copy -> (shifted, min_margin, pos_margin, target, branch)"""
    mn, pos = margins64(cones, v)
    tg = target_of(pos, cones.degree)
    w, br = apply_shift(cones, v, pd, mn, tg)
    return w, mn, pos, tg, br


# ---- 50 digits -------------------------------------------------------------------------------------------------------------------------

def _norm2(Z):
    return float(np.linalg.norm(Z, 2)) if Z.size else 0.0


def margins_mp(cones, z):
    """-> dict: alpha, beta (mpf), binder = index of the cone that attains alpha, kind = its class, and the scales of the gates:
    nn_sum = sum of the positive Nonnegative entries, soc = [(cone, |z0| + |z1|, alpha_k)], psd = [(cone, n, |Z|_2, alpha_k, beta_k,
    host_alpha, host_beta)] where host_* is what eigvalsh gives for the same matrix.  z must be finite."""
    alpha, beta, binder = mpf(FLOATMAX), mpf(0), None
    nn_sum, soc, psd = mpf(0), [], []
    for k, (c, r) in enumerate(zip(cones.cones, cones.rng_cones)):
        zz = z[r]
        if isinstance(c, ZeroCone):
            continue
        if isinstance(c, NonnegativeCone):
            if zz.size == 0:
                continue
            a = mpf(float(zz.min()))
            b = mp.fsum(mpf(float(v)) for v in zz if v > 0)
            nn_sum += b
        elif isinstance(c, SecondOrderCone):
            t = mp.sqrt(mp.fsum(mpf(float(v)) ** 2 for v in zz[1:]))
            a = mpf(float(zz[0])) - t
            b = a if a > 0 else mpf(0)
            soc.append((k, abs(float(zz[0])) + float(t), a))
        elif isinstance(c, PSDTriangleCone):
            Z = c.svec_to_mat(zz)            # the float64 matrix both the host and the device decompose
            if not np.any(Z - np.diag(np.diag(Z))):      # a diagonal matrix: its eigenvalues are its entries, exactly
                ev = [mpf(float(e)) for e in np.diag(Z)]
            else:
                ev = mp.eigsy(mp.matrix(Z.tolist()), eigvals_only=True)
                ev = [ev[i] for i in range(c.n)]
            a = min(ev)
            b = mp.fsum(e for e in ev if e > 0)
            ha, hb = cone_margins64(c, zz)
            psd.append((k, c.n, _norm2(Z), a, b, ha, hb))
        else:
            raise TypeError(type(c).__name__)
        if a < alpha:
            alpha, binder = a, k
        beta += b
    kind = type(cones.cones[binder]) if binder is not None else None
    return dict(alpha=alpha, beta=beta, binder=binder, kind=kind, nn_sum=nn_sum, soc=soc, psd=psd, degree=cones.degree)


def decision_mp(ref):
    """-> (target, branch, decision margin) at 50 digits: the distance of min_margin from 0 resp. from target, relative to target
    (the smaller of the two)"""
    deg = ref["degree"]
    target = max(mpf(1), mpf("0.1") * ref["beta"] / deg) if deg > 0 else mpf(1)
    a = ref["alpha"]
    br = 0 if a <= 0 else (1 if a < target else 2)
    return target, br, float(min(abs(a), abs(a - target)) / target)


def margin_allowances(ref, sum_tol):
    """-> (allowance of alpha, allowance of beta, worst host error of a PSD alpha / beta in eps |Z|_2) under the project's gates.
    alpha: a Nonnegative alpha is exact; a second-order alpha lies within sum_tol (|z0| + |z1|); a PSD alpha within psd_allowance of
    what eigvalsh gives for the same matrix.  beta is a sum of non-negative terms, each charged once: sum_tol x beta for the additions
    (a Nonnegative-only beta is held to sum_tol x beta), plus the error of each second-order term max(0, alpha_k) (its alpha's
    allowance, where alpha_k can be positive at all) and of each PSD term (psd_allowance of that cone's beta)."""
    tol_a, tol_b = 0.0, sum_tol * float(ref["beta"])
    rh_a = rh_b = 0.0
    for k, scale, a in ref["soc"]:
        if float(a) > -sum_tol * scale:           # (a cone whose alpha is safely negative adds exactly 0)
            tol_b += sum_tol * scale
        if k == ref["binder"]:
            tol_a = sum_tol * scale
    for k, n, norm2, a, b, ha, hb in ref["psd"]:
        ta, ra = psd_allowance(n, norm2, abs(mpf(ha) - a))
        tb, rb = psd_allowance(n, norm2, abs(mpf(hb) - b))
        rh_a, rh_b = max(rh_a, ra), max(rh_b, rb)
        if b > 0 or hb > 0:                       # (a cone without a positive eigenvalue adds exactly 0)
            tol_b += tb
        if k == ref["binder"]:
            tol_a = ta
    return tol_a, tol_b, rh_a, rh_b


def psd_allowance(n, norm2, host_err):
    """the rule of tests/test_gpu_psd_step.py: max(8 x the host's error in the same case, 2 n) in units of eps |Z|_2"""
    unit = EPS * norm2
    rh = float(host_err) / unit if unit > 0 else 0.0
    return max(8.0 * rh, 2.0 * n) * unit, rh


def same_bits(a, b):
    """bit-identical float64 arrays (a NaN equals a NaN of any payload: an addition may quieten it)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | nan))


def is_finite(x):
    return not (math.isnan(x) or math.isinf(x))
