"""The device-resident interior-point step for PSD triangle cones next to Exponential / Power / Generalized Power cones on the GPU
(hipkkt_step_enable_mixed, Settings.device_step_mixed; the log-det barrier of barrier_psd.hip).

Gates.
  * The PSD cones' barrier against the 50-digit value of tests/psd_barrier_reference.py: per (side, point, candidate) the PSD term is the
    barrier of the set [PSD(n), Exponential] minus the same call on a handle that holds the Exponential rows only; its error is at most
    max(8 x the host's error in the same case, 2 n) in units of eps x scale (the rule of tests/test_gpu_psd_step.py), plus the last
    rounding of the two float64 sums the difference is taken from, 1 eps x the larger of their sum |terms|.
  * A candidate outside a PSD cone: -Inf, `==` (the reference's `barrier -= typemax`).
  * The four row operations on the mixed set: rows of kinds 0..2 and 4..6 bit for bit those of a handle without the PSD cones, PSD rows
    bit for bit those of a PSD-mode handle without the non-symmetric cones (np.array_equal); the same for the blocks of K.
  * The barrier of a set against the stand-in's composite: 1e-10 max(1, sum |terms|); the shifted dot: 1e-13 sum |terms|.
  * Step length: the symmetric + PSD start `==` the PSD-mode twin's; from there the device's alpha `==` alpha0 step^k of the binding cone,
    every decision constructed with a 50-digit margin >= 1e-3 (asserted), none excluded.
  * Fused calls: 1e-10 against the stand-in's kkt_solve on the same plugin; alpha `==` the granular call's.
  * End to end: SOLVED on every path, |dobj| <= 2 max(tol_gap_abs, tol_gap_rel max(1, |obj|)).
No case is skipped or filtered.  Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt, problems
from clarabel_jl_amd.cone_api import nvars
from clarabel_jl_amd.kktsolver import HipKKTSolver
from julia_standin import ipm
from julia_standin.cones import NonnegativeCone, PSDTriangleCone, SecondOrderCone, ZeroCone
from tests import psd_barrier_reference as br
from tests import psd_scaling_reference as sr
from tests import psd_step_reference as pr
from tests.step_support import PARITY, STEP_FLAGS, _check_barrier, _Timeout
from tests.test_gpu_genpow_step import ALPHA0, MARGIN, _boundary, _margin_of, _moved
from tests import genpow_reference as gp

pytestmark = pytest.mark.gpu

T = cl
MIXED = dict(device_step=True, device_step_nonsymmetric=True, device_step_genpower=True, device_step_psd=True, device_step_mixed=True,
             **STEP_FLAGS)
MIXEDN = dict(MIXED, device_scaling_psd=True)
NONSYM = dict(device_step=True, device_step_nonsymmetric=True, device_step_genpower=True, **STEP_FLAGS)
PSD = dict(device_step=True, device_step_psd=True, **STEP_FLAGS)
STEP, AMIN = 0.8, 1e-4
EPS = br.EPS


def _mixed_specs(genpow=True):
    specs = [T.NonnegativeConeT(3), T.PSDTriangleConeT(3), T.ExponentialConeT(), T.SecondOrderConeT(4), T.PowerConeT(0.3),
             T.PSDTriangleConeT(8), T.ZeroConeT(2), T.GenPowerConeT((0.6, 0.4), 1), T.PSDTriangleConeT(2)]
    return specs if genpow else [c for c in specs if not isinstance(c, T.GenPowerConeT)]


def _is_psd(c):
    return isinstance(c, PSDTriangleCone)


def _is_sym(c):
    return bool(getattr(c, "is_symmetric", True))


def _problem(specs, seed):
    rng = np.random.default_rng(seed)
    m = sum(nvars(c) for c in specs)
    n = min(6, m)
    A = sp.random(m, n, density=min(1.0, 12.0 / m + 0.2), random_state=np.random.RandomState(seed), format="csc") + \
        sp.vstack([sp.identity(n), sp.csc_matrix((m - n, n))]).tocsc()
    return sp.identity(n, format="csc") * 1.5, rng.standard_normal(n), A.tocsc(), rng.standard_normal(m), specs


def _handle(specs, seed, flags=MIXED):
    """(plugin, cones, settings) for the cone set as given (not collapsed)"""
    P, q, A, b, specs = _problem(specs, seed)
    cones = cl.CompositeCone(specs)
    Pt = sp.triu(sp.csc_matrix(P), format="csc")
    Pt.sort_indices()
    A = sp.csc_matrix(A)
    A.sort_indices()
    m, n = A.shape
    st = cl.Settings(linesearch_backtrack_step=STEP, min_terminate_step_length=AMIN, **flags)
    cones.use_settings(st)
    return HipKKTSolver(Pt, A, cones, m, n, st), cones, st


def _nonsym_point(c, rng):
    """(s, z) of one Exponential / Power / Generalized Power cone: the fixture's draw around the central ray, repeated until both have a
    50-digit margin of twice the step-length tests' MARGIN"""
    z0, s0 = np.zeros(c.numel), np.zeros(c.numel)
    c.unit_initialization(z0, s0)
    out = []
    for dual, inside in ((False, c.is_primal_feasible), (True, c.is_dual_feasible)):
        for _ in range(400):
            t = s0 * rng.uniform(0.5, 2.0) + 0.2 * rng.standard_normal(c.numel)
            if inside(t) and inside(s0 + 0.5 * (t - s0)):
                mg = _margin_of(c, t, dual)
                if mg is not None and mg >= 2.0 * MARGIN:
                    break
        else:
            raise AssertionError("no interior point with a margin")
        out.append(t)
    return out[0], out[1]


def _point(cones, rng, late):
    """(s, z, mu): PSD members from psd_step_reference.random_sz (late: S Z ~ 1e-9 I), Nonnegative rows random (late: s o z = 1e-9),
    second-order and non-symmetric members at interior points with margins"""
    m = cones.numel
    s, z = np.zeros(m), np.zeros(m)
    for c, r in zip(cones.cones, cones.rng_cones):
        if _is_psd(c):
            s[r], z[r], _ = pr.random_sz(c, rng, late)
        elif isinstance(c, ZeroCone):
            continue
        elif isinstance(c, NonnegativeCone):
            if late:
                s[r] = 10.0 ** rng.uniform(-6.0, 0.0, c.numel)
                z[r] = 1e-9 / s[r]
            else:
                s[r], z[r] = rng.random(c.numel) + 0.2, rng.random(c.numel) + 0.2
        elif isinstance(c, SecondOrderCone):
            for v in (s, z):
                t = rng.standard_normal(c.dim)
                t[0] = np.linalg.norm(t[1:]) + 0.5 + rng.random()
                v[r] = t
        else:
            s[r], z[r] = _nonsym_point(c, rng)
    mu = float(s @ z) / (cones.degree + 1)
    assert mu > 0
    return s, z, mu


def _psd_R(cones):
    return np.concatenate([c.R.ravel(order="F") for c in cones.cones if _is_psd(c)])


def _scale(hk, cones, s, z, mu, strategy):
    """the scaling on the device from the host's PSD factors; the host cones adopt the device's values -> (w, lambda, eta, nonsym)"""
    for c, r in zip(cones.cones, cones.rng_cones):
        if _is_psd(c):
            assert c.update_scaling(s[r], z[r], mu)
    R = _psd_R(cones) if hk._psd_cones else None
    if hk.steps_psd:
        hk.h.psd_set_factors(*hk._psd_factors())
    if hk.scales_nonsymmetric:
        ok, w, lam, eta, nonsym = hk.h.update_scaling_ex(s, z, mu, strategy, R)
    else:
        ok, w, lam, eta = hk.h.update_scaling(s, z, R)
        nonsym = np.zeros(0)
    assert ok
    off, k = 0, 0
    for c, r in zip(cones.cones, cones.rng_cones):
        if hasattr(c, "adopt_scaling"):
            n = c.scaling_slot_len
            c.adopt_scaling(nonsym[off:off + n], z[r], mu)
            off += n
        elif isinstance(c, SecondOrderCone):
            c.adopt_symmetric_scaling(w[r], lam[r], eta[k])
            k += 1
        elif isinstance(c, NonnegativeCone):
            assert c.update_scaling(s[r], z[r], mu)
    assert off == len(nonsym)
    return w, lam, eta, nonsym


def _rows(cones, keep):
    return np.concatenate([np.arange(r.start, r.stop) for c, r in zip(cones.cones, cones.rng_cones) if keep(c)])


def _sub_handle(specs, cones, keep, seed, flags):
    """a handle for the members of the set that `keep` selects, and their rows in the full set"""
    sub = [sp_ for sp_, c in zip(specs, cones.cones) if keep(c)]
    hk, sc, _ = _handle(sub, seed, flags)
    return hk, sc, _rows(cones, keep)


_sets = {}


def _mixed_set(genpow, late, strategy, seed=3):
    """the mixed set scaled at one point, with its two twins scaled at the same rows: `ns` without the PSD cones (GenPow / Cone3 mode),
    `ps` without the non-symmetric cones (PSD mode).  Built once per (genpow, late, strategy)."""
    key = (genpow, late, strategy, seed)
    if key not in _sets:
        specs = _mixed_specs(genpow)
        hk, cones, st = _handle(specs, seed)
        assert hk.steps_on_device and hk.steps_mixed and hk.steps_psd and hk.steps_nonsymmetric
        rng = np.random.default_rng(300 + seed + 10 * int(late))
        s, z, mu = _point(cones, rng, late)
        code = {"primal_dual": 0, "dual": 1}[strategy]
        out = _scale(hk, cones, s, z, mu, code)
        ns, nsc, nsrows = _sub_handle(specs, cones, lambda c: not _is_psd(c), seed + 50, NONSYM)
        assert ns.steps_on_device and ns.steps_nonsymmetric and not ns.steps_psd
        ps, psc, psrows = _sub_handle(specs, cones, _is_sym, seed + 60, PSD)
        assert ps.steps_on_device and ps.steps_psd and not ps.steps_nonsymmetric
        assert ns.h.update_scaling_ex(s[nsrows], z[nsrows], mu, code)[0]
        for c, cf in zip(psc.cones, [c for c in cones.cones if _is_sym(c)]):
            if _is_psd(c):
                c.R[:], c.Rinv[:], c.lam[:] = cf.R, cf.Rinv, cf.lam
        ps.h.psd_set_factors(*ps._psd_factors())
        assert ps.h.update_scaling(s[psrows], z[psrows], _psd_R(psc))[0]
        _sets[key] = dict(hk=hk, cones=cones, st=st, s=s, z=z, mu=mu, out=out, ns=ns, nsc=nsc, nsrows=nsrows, ps=ps, psc=psc,
                          psrows=psrows, rng=rng, specs=specs)
    return _sets[key]


POINTS = [(True, False, "dual"), (True, True, "dual"), (False, False, "primal_dual"), (False, True, "primal_dual"),
          (False, False, "dual"), (False, True, "dual")]
POINT_IDS = [f"{'genpow' if g else 'no_genpow'}-{'late' if l else 'early'}-{s}" for g, l, s in POINTS]


# ---- the barrier of one PSD cone next to one Exponential cone --------------------------------------------------------------------------

_pairs = {}
_worst = {}


def _barrier_pair(n):
    """([PSD(n), Exponential] in mixed mode, [Exponential] in Cone3 mode), built once per side"""
    if n not in _pairs:
        hm, cm, _ = _handle([T.PSDTriangleConeT(n), T.ExponentialConeT()], 11)
        he, ce, _ = _handle([T.ExponentialConeT()], 12, NONSYM)
        assert hm.steps_mixed and he.steps_nonsymmetric and not he.steps_psd
        _pairs[n] = (hm, cm, he, ce)
    return _pairs[n]


@pytest.mark.parametrize("late", [False, True], ids=["early", "late"])
@pytest.mark.parametrize("n", br.SIDES)
def test_barrier_of_one_psd_cone_next_to_an_exponential_cone(n, late):
    with _Timeout(120):
        cs = br.case(n, late)
        hm, cm, he, ce = _barrier_pair(n)
        rng = np.random.default_rng(500 + n)
        pc, ec = cm.cones
        rp, rexp = cm.rng_cones
        s, z = np.zeros(cm.numel), np.zeros(cm.numel)
        s[rp], z[rp] = cs["s"], cs["z"]
        s[rexp], z[rexp] = _nonsym_point(ec, rng)
        mu = float(s @ z) / (cm.degree + 1)
        _scale(hm, cm, s, z, mu, 1)
        assert he.h.update_scaling_ex(s[rexp], z[rexp], mu, 1)[0]
        dz, ds = np.zeros(cm.numel), np.zeros(cm.numel)
        dz[rp], ds[rp] = cs["dz"], cs["ds"]
        dz[rexp], ds[rexp] = 0.01 * rng.standard_normal(3) * np.abs(z[rexp]), 0.01 * rng.standard_normal(3) * np.abs(s[rexp])
        assert math.isfinite(ec.compute_barrier(z[rexp], s[rexp], dz[rexp], ds[rexp], cs["alphas"][0]))
        worst_d = worst_h = 0.0
        for nalpha in (1, 3, 8):
            alphas = cs["alphas"][:nalpha]
            bars, dots = hm.cone_barrier(dz, ds, alphas)
            bars_e, _ = he.cone_barrier(dz[rexp], ds[rexp], alphas)
            for j, a in enumerate(alphas):
                assert math.isfinite(bars[j]) and math.isfinite(bars_e[j]), (n, late, a, bars[j], bars_e[j])
                term = bars[j] - bars_e[j]
                ref, scale, rh = cs["ref"][j], cs["scale"][j], cs["host_ratio"][j]
                sums = EPS * (abs(float(ref)) + abs(bars_e[j]))      # sum |terms| of the larger sum: the PSD term and the Exponential one
                allowed = br.allowed(rh, n)
                err = float(abs(br.mpf(term) - ref))
                rd = err / (EPS * scale)
                print(f"[mixed barrier] n={n} late={late} {nalpha} candidates, alpha={a:.4f}: PSD term {term:.6e}, device {rd:.3f}, "
                      f"host {rh:.3f}, allowed {allowed:.1f} (eps x scale {scale:.3e}) + {sums:.2e} for the two sums")
                assert err <= allowed * EPS * scale + sums, (n, late, nalpha, a, rd, rh)
                worst_d, worst_h = max(worst_d, rd), max(worst_h, rh)
                zz, ss = z + a * dz, s + a * ds
                assert abs(dots[j] - float(zz @ ss)) <= 1e-13 * float(np.abs(zz) @ np.abs(ss))
        w = _worst.setdefault(n, [0.0, 0.0])
        w[0], w[1] = max(w[0], worst_d), max(w[1], worst_h)
        print(f"[mixed barrier] n={n}: worst device {w[0]:.3f}, worst host {w[1]:.3f} (eps x scale) so far; device / host "
              f"{w[0] / max(w[1], 1e-300):.2f}")


def test_barrier_edges_outside_nan_zero_direction_zero_step():
    with _Timeout(60):
        cs = br.case(3, False)
        hm, cm, he, ce = _barrier_pair(3)
        rng = np.random.default_rng(17)
        pc, ec = cm.cones
        rp, rexp = cm.rng_cones
        s, z = np.zeros(cm.numel), np.zeros(cm.numel)
        s[rp], z[rp] = cs["s"], cs["z"]
        s[rexp], z[rexp] = _nonsym_point(ec, rng)
        mu = float(s @ z) / (cm.degree + 1)
        _scale(hm, cm, s, z, mu, 1)
        zero = np.zeros(cm.numel)
        out_z, out_s = zero.copy(), zero.copy()
        out_z[rp] = pc.mat_to_svec(-2.0 * pc.svec_to_mat(z[rp]))      # Z + 1 (-2 Z) = -Z
        out_s[rp] = pc.mat_to_svec(-2.0 * pc.svec_to_mat(s[rp]))
        for what, (dz, ds) in {"z side": (out_z, zero), "s side": (zero, out_s), "both": (out_z, out_s)}.items():
            bars, dots = hm.cone_barrier(dz, ds, [1.0, 0.25, 0.0])
            print(f"[mixed barrier edges] outside on the {what}: {bars}")
            assert bars[0] == -math.inf, (what, bars)
            assert cm.compute_barrier(z, s, dz, ds, 1.0) == -math.inf
            assert math.isfinite(bars[1]) and math.isfinite(bars[2])
            assert abs(bars[1] - cm.compute_barrier(z, s, dz, ds, 0.25)) <= PARITY * max(1.0, abs(bars[1]))
        nan = zero.copy()
        nan[rp.start + 1] = math.nan
        bars, _ = hm.cone_barrier(nan, zero, [0.5, 0.25])
        assert bars[0] == -math.inf and bars[1] == -math.inf, bars      # a NaN reaches a pivot: the failure arm
        dz, ds = zero.copy(), zero.copy()
        dz[rp], ds[rp] = cs["dz"], cs["ds"]
        at_point, _ = hm.cone_barrier(zero, zero, [0.7, 0.3])
        at_zero, _ = hm.cone_barrier(dz, ds, [0.0])
        assert at_point[0] == at_point[1] == at_zero[0] and math.isfinite(at_zero[0])
        only_ds, _ = hm.cone_barrier(zero, ds, [0.5])                # dZ = 0 alone
        assert abs(only_ds[0] - cm.compute_barrier(z, s, zero, ds, 0.5)) <= PARITY * max(1.0, abs(only_ds[0]))
        assert np.array_equal(hm.cone_affine_ds()[rexp], s[rexp])     # the handle still serves


# ---- the mixed set: rows, K, barrier ---------------------------------------------------------------------------------------------------

def _directions(M, rng):
    """(dz, ds, x): random rows, the PSD rows symmetric directions of the size of the point"""
    cones, s, z = M["cones"], M["s"], M["z"]
    m = cones.numel
    dz, ds, x = rng.standard_normal(m), rng.standard_normal(m), rng.standard_normal(m)
    for c, r in zip(cones.cones, cones.rng_cones):
        if _is_psd(c):
            dz[r], ds[r] = pr.direction(c, rng, z[r]), pr.direction(c, rng, s[r])
    return dz, ds, x


def _row_ops(hk, dz, ds, x, sm):
    return {"affine_ds": hk.cone_affine_ds(), "combined_ds_shift": hk.cone_combined_ds_shift(dz, ds, sm),
            "ds_from_dz_offset": hk.cone_ds_from_dz_offset(x), "mul_Hs": hk.cone_mul_hs(x)}


@pytest.mark.parametrize("genpow,late,strategy", POINTS, ids=POINT_IDS)
def test_row_operations_and_K_are_each_family_s_own_bits(genpow, late, strategy):
    with _Timeout(120):
        M = _mixed_set(genpow, late, strategy)
        hk, cones, ns, ps, nsrows, psrows = M["hk"], M["cones"], M["ns"], M["ps"], M["nsrows"], M["psrows"]
        dz, ds, x = _directions(M, np.random.default_rng(41))
        sm = 0.3 * M["mu"]
        got = _row_ops(hk, dz, ds, x, sm)
        tw_ns = _row_ops(ns, dz[nsrows], ds[nsrows], x[nsrows], sm)
        tw_ps = _row_ops(ps, dz[psrows], ds[psrows], x[psrows], sm)
        psd_in_ps = _rows(M["psc"], _is_psd)                          # the PSD rows inside the PSD-mode twin
        psd_rows = _rows(cones, _is_psd)
        for op in got:
            assert np.all(np.isfinite(got[op])), op
            assert np.array_equal(got[op][nsrows], tw_ns[op]), (op, "kinds 0..2 and 4..6")
            assert np.array_equal(got[op][psd_rows], tw_ps[op][psd_in_ps]), (op, "PSD rows")
        # K after the scaling: per cone its Hs block
        Kd, Kn, Kp = hk.h.debug_dump(4), ns.h.debug_dump(4), ps.h.debug_dump(4)
        mp_d, mp_n, mp_p = hk.h.map(2), ns.h.map(2), ps.h.map(2)
        bn, bp = iter(M["nsc"].rng_blocks), iter(M["psc"].rng_blocks)
        for c, rb in zip(cones.cones, cones.rng_blocks):
            if _is_psd(c):
                rb_n, rb_p = None, next(bp)
            elif _is_sym(c):
                rb_n, rb_p = next(bn), next(bp)
            else:
                rb_n, rb_p = next(bn), None
            if rb_n is not None:
                assert np.array_equal(Kd[mp_d[rb]], Kn[mp_n[rb_n]]), type(c).__name__
            if rb_p is not None:
                assert np.array_equal(Kd[mp_d[rb]], Kp[mp_p[rb_p]]), type(c).__name__
        print(f"[mixed rows] genpow={genpow} late={late} {strategy}: 4 operations and {len(cones.cones)} K blocks bit for bit")


@pytest.mark.parametrize("genpow,late,strategy", POINTS, ids=POINT_IDS)
def test_barrier_of_the_mixed_set_matches_the_stand_in(genpow, late, strategy):
    with _Timeout(120):
        M = _mixed_set(genpow, late, strategy)
        hk, cones, st, s, z = M["hk"], M["cones"], M["st"], M["s"], M["z"]
        rng = np.random.default_rng(43)
        m = cones.numel
        dz, ds = 0.2 * rng.standard_normal(m) * np.abs(z), 0.2 * rng.standard_normal(m) * np.abs(s)
        for c, r in zip(cones.cones, cones.rng_cones):
            if _is_psd(c):
                dz[r], ds[r] = br.interior_direction(c, z[r], rng), br.interior_direction(c, s[r], rng)
            elif isinstance(c, SecondOrderCone):
                dz[r], ds[r] = 0.2 * z[r], -0.2 * s[r]
        a0 = st.max_step_fraction * min(cones.step_length(dz, ds, z, s, 1.0))
        assert a0 > 0
        alphas = [a0 * st.linesearch_backtrack_step ** k for k in range(8)]
        bars, dots = hk.cone_barrier(dz, ds, alphas)
        assert all(math.isfinite(b) for b in bars)
        _check_barrier(bars, dots, cones, z, s, dz, ds, alphas, f"mixed genpow={genpow} late={late} {strategy} 8")
        for n in (1, 3):
            b, d = hk.cone_barrier(dz, ds, alphas[2:2 + n])
            assert np.array_equal(b, bars[2:2 + n]) and np.array_equal(d, dots[2:2 + n]), n


# ---- the mixed set: step length ---------------------------------------------------------------------------------------------------------

def _host_composite(M, dz, ds, start):
    """the stand-in's non-symmetric cones walking the grid from `start` (coneops_compositecone.jl:216-252, second half)"""
    cones, st, s, z = M["cones"], M["st"], M["s"], M["z"]
    alpha = min(start, ALPHA0)
    for c, r in zip(cones.cones, cones.rng_cones):
        if not _is_sym(c):
            alpha = min(c.step_length(dz[r], ds[r], z[r], s[r], alpha, st))
    return alpha


def _assert_margins(M, dz, ds, alpha):
    """every non-symmetric cone is inside at `alpha` with a 50-digit margin >= MARGIN on both sides: it accepts the first grid point"""
    for c, r in zip(M["cones"].cones, M["cones"].rng_cones):
        if _is_sym(c):
            continue
        for dual, q, d in ((True, M["z"][r], dz[r]), (False, M["s"][r], ds[r])):
            mg = _margin_of(c, _moved(q, d, alpha), dual)
            assert mg is not None and mg >= MARGIN, (type(c).__name__, dual, mg)


@pytest.mark.parametrize("genpow,late,strategy", POINTS, ids=POINT_IDS)
def test_step_length_every_member_binding_alone_and_a_random_direction(genpow, late, strategy):
    with _Timeout(120):
        M = _mixed_set(genpow, late, strategy)
        hk, cones, ps, psrows, s, z = M["hk"], M["cones"], M["ps"], M["psrows"], M["s"], M["z"]
        m = cones.numel
        zero = np.zeros(m)
        rng = np.random.default_rng(47)
        assert hk.cone_step_length(zero, zero, 1.0) == (ALPHA0, ALPHA0)
        assert hk.cone_step_length(zero, zero, 0.4) == (0.4, 0.4)
        decisions = 0
        for k, (c, r) in enumerate(zip(cones.cones, cones.rng_cones)):
            if isinstance(c, ZeroCone):
                continue
            if _is_sym(c):
                # a symmetric or PSD member binds: the start is the PSD-mode twin's pair, the non-symmetric members stay where they are
                for side in (0, 1):
                    dz, ds = zero.copy(), zero.copy()
                    q = (z, s)[side]
                    (dz, ds)[side][r] = -2.5 * q[r] + (0.05 * pr.direction(c, rng, q[r]) if _is_psd(c) else 0.0)
                    pair = ps.cone_step_length(dz[psrows], ds[psrows], 1.0)
                    start = min(pair)
                    assert pair[side] < 0.5 and pair[1 - side] == 1.0, (k, side, pair)
                    got = hk.cone_step_length(dz, ds, 1.0)
                    assert got == (start, start), (k, type(c).__name__, side, got, pair)
                    assert got[0] == _host_composite(M, dz, ds, start)
                    decisions += 1
            else:
                # a non-symmetric member binds at a chosen grid point; the symmetric + PSD start is alpha_max
                for dual in (True, False):
                    for grid_k in (1, 2, 7):
                        q = (z if dual else s)[r]
                        d = _boundary(c, q, dual, gp.crossing_between(ALPHA0, STEP, grid_k))
                        acc, rej = gp.grid_alpha(ALPHA0, STEP, grid_k), gp.grid_alpha(ALPHA0, STEP, grid_k - 1)
                        m_acc, m_rej = _margin_of(c, _moved(q, d, acc), dual), _margin_of(c, _moved(q, d, rej), dual)
                        assert m_acc is not None and m_acc >= MARGIN and m_rej is not None and m_rej <= -MARGIN, (k, dual, grid_k)
                        full = zero.copy()
                        full[r] = d
                        dz, ds = (full, zero) if dual else (zero, full)
                        assert ps.cone_step_length(dz[psrows], ds[psrows], 1.0) == (1.0, 1.0)
                        got = hk.cone_step_length(dz, ds, 1.0)
                        assert got == (acc, acc), (k, type(c).__name__, dual, grid_k, got, acc)
                        decisions += 1
        # a random direction: PSD and symmetric rows move far (they set the start), the non-symmetric rows a little
        dz, ds = 0.05 * rng.standard_normal(m) * np.abs(z), 0.05 * rng.standard_normal(m) * np.abs(s)
        for c, r in zip(cones.cones, cones.rng_cones):
            if _is_psd(c):
                dz[r], ds[r] = -1.5 * z[r] + br.interior_direction(c, z[r], rng), -1.2 * s[r] + br.interior_direction(c, s[r], rng)
            elif isinstance(c, (NonnegativeCone, SecondOrderCone)):
                dz[r], ds[r] = -1.3 * z[r] + 0.1 * rng.standard_normal(c.numel) * np.abs(z[r]), 0.3 * s[r]
        pair = ps.cone_step_length(dz[psrows], ds[psrows], 1.0)
        start = min(pair)
        assert start < ALPHA0
        _assert_margins(M, dz, ds, start)
        got = hk.cone_step_length(dz, ds, 1.0)
        print(f"[mixed step length] genpow={genpow} late={late} {strategy}: {decisions} constructed decisions; random direction: "
              f"PSD-mode twin {pair!r}, device {got!r}")
        assert got == (start, start) and start == _host_composite(M, dz, ds, start)
        # ... and one where a non-symmetric member backtracks from that start
        k = max(i for i, c in enumerate(cones.cones) if not _is_sym(c))
        c, r = cones.cones[k], cones.rng_cones[k]
        a2 = start * STEP * STEP
        dz2 = dz.copy()
        dz2[r] = _boundary(c, z[r], True, math.sqrt((start * STEP) * a2))
        m_acc, m_rej = _margin_of(c, _moved(z[r], dz2[r], a2), True), _margin_of(c, _moved(z[r], dz2[r], start * STEP), True)
        assert m_acc is not None and m_acc >= MARGIN and m_rej is not None and m_rej <= -MARGIN, (m_acc, m_rej)
        ds2 = ds.copy()
        ds2[r] = 0.0
        assert ps.cone_step_length(dz2[psrows], ds2[psrows], 1.0) == pair
        _assert_margins(dict(M, cones=_Only(cones, lambda i: i != k)), dz2, ds2, start)
        got = hk.cone_step_length(dz2, ds2, 1.0)
        assert got == (a2, a2), (got, a2, start)
        assert a2 == _host_composite(M, dz2, ds2, start)


class _Only:
    """a view of a cone set that lists the members an index predicate selects"""

    def __init__(self, cones, keep):
        idx = [i for i in range(len(cones.cones)) if keep(i)]
        self.cones = [cones.cones[i] for i in idx]
        self.rng_cones = [cones.rng_cones[i] for i in idx]


# ---- determinism --------------------------------------------------------------------------------------------------------------------------

def test_two_runs_of_every_operation_give_the_same_bits():
    with _Timeout(120):
        M = _mixed_set(True, False, "dual")
        hk, cones, s, z, mu = M["hk"], M["cones"], M["s"], M["z"], M["mu"]
        dz, ds, x = _directions(M, np.random.default_rng(53))
        dzb, dsb = 0.1 * dz, 0.1 * ds
        for c, r in zip(cones.cones, cones.rng_cones):
            if _is_psd(c):
                dzb[r], dsb[r] = br.interior_direction(c, z[r], np.random.default_rng(54)), br.interior_direction(c, s[r], np.random.default_rng(55))

        def run():
            _scale(hk, cones, s, z, mu, 1)
            ops = _row_ops(hk, dz, ds, x, 0.3 * mu)
            return [hk.h.debug_dump(4)] + [ops[k] for k in sorted(ops)] + [np.array(hk.cone_step_length(dz, ds, 1.0))] + \
                [np.array(v) for v in hk.cone_barrier(dzb, dsb, [0.9, 0.5, 0.25])]

        first, second = run(), run()
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, second))
        # the device-side PSD scaling as well
        hn, cn_, _ = _handle(_mixed_specs(True), 3, MIXEDN)
        assert hn.steps_mixed and hn.scales_psd
        outs = []
        for _ in range(2):
            assert hn.h.update_scaling_ex(s, z, mu, 1, None)[0]
            outs.append([hn.h.debug_dump(4), *hn.h.psd_get_factors(), hn.cone_mul_hs(x), np.array(hn.cone_barrier(dzb, dsb, [0.9, 0.5])[0])])
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(*outs))


# ---- the protocol -------------------------------------------------------------------------------------------------------------------------

def test_the_enable_refuses_what_it_cannot_serve():
    bad_sets = ([T.PSDTriangleConeT(65), T.ExponentialConeT()],                          # a side above 64
                [T.NonnegativeConeT(3), T.SecondOrderConeT(4)],                          # symmetric
                [T.PSDTriangleConeT(3), T.NonnegativeConeT(2)],                          # PSD without a non-symmetric member
                [T.ExponentialConeT(), T.NonnegativeConeT(2)])                           # no PSD member
    for specs in bad_sets:
        hk, cones, _ = _handle(specs, 1)
        assert not hk.steps_mixed, specs
        with pytest.raises(ValueError, match="step_enable_mixed"):
            hk.h.step_enable_mixed(True, STEP, AMIN)
        hk.h.step_enable_mixed(False, STEP, AMIN)                    # switching off is always possible
    hk, cones, _ = _handle([T.PSDTriangleConeT(65), T.ExponentialConeT()], 1)
    assert not hk.steps_on_device
    # a mixed registration: bad line-search parameters, and every other enable keeps refusing it
    hk, cones, _ = _handle([T.PSDTriangleConeT(3), T.ExponentialConeT()], 2, flags={})
    assert not hk.steps_on_device
    for step, amin in ((0.0, 1e-4), (1.0, 1e-4), (1.5, 1e-4), (-0.1, 1e-4), (float("nan"), 1e-4), (0.8, 0.0), (0.8, -1.0),
                       (0.8, float("inf")), (0.999999, 1e-4)):
        with pytest.raises(ValueError):
            hk.h.step_enable_mixed(True, step, amin)
    for fn in (hk.h.step_enable_cone3, hk.h.step_enable_genpow):
        with pytest.raises(ValueError):
            fn(True, STEP, AMIN)
    for fn in (hk.h.step_enable_psd, hk.h.step_enable_psd_large):
        with pytest.raises(ValueError):
            fn(True)
    with pytest.raises(ValueError):
        hk.h.psd_set_factors(np.zeros(9), np.ones(3))               # not before the enable
    hk.h.step_enable_mixed(True, STEP, AMIN)


def test_scaling_protocol_failed_cone_and_default_start():
    with _Timeout(120):
        specs = _mixed_specs(True)
        hk, cones, st = _handle(specs, 5, flags={})
        m = cones.numel
        rng = np.random.default_rng(9)
        s, z, mu = _point(cones, rng, False)
        for c, r in zip(cones.cones, cones.rng_cones):
            if _is_psd(c):
                assert c.update_scaling(s[r], z[r], mu)
        R = _psd_R(cones)
        # without the enable the registration scales as it always did and the step calls refuse it
        assert hk.h.update_scaling_ex(s, z, mu, 1, R)[0]
        with pytest.raises(ValueError):
            hk.cone_affine_ds()
        hk.h.step_enable_mixed(True, STEP, AMIN)
        with pytest.raises(ValueError):
            hk.cone_affine_ds()                                     # a scaling from before the enable does not count
        with pytest.raises(hipkkt.HipKKTError, match="psd_set_factors"):
            hk.h.update_scaling_ex(s, z, mu, 1, R)                  # no factors staged
        with pytest.raises(hipkkt.HipKKTError):
            hk.h.update_scaling_ex(s, z, mu, 1, None)
        with pytest.raises(ValueError):
            hk.cone_affine_ds()
        rinv = np.concatenate([c.Rinv.ravel(order="F") for c in cones.cones if _is_psd(c)])
        lam = np.concatenate([c.lam for c in cones.cones if _is_psd(c)])
        hk.h.psd_set_factors(rinv, lam)
        assert hk.h.update_scaling_ex(s, z, mu, 1, R)[0]
        first = hk.cone_affine_ds()
        assert np.all(np.isfinite(first))
        # the barrier calls serve this mode; the default-start calls keep refusing
        bars, _ = hk.cone_barrier(np.zeros(m), np.zeros(m), [0.0])
        assert math.isfinite(bars[0])
        for call in (hk.h.cone_set_identity_scaling, lambda: hk.h.cone_margins(s, 0), lambda: hk.h.cone_shift_to_interior(s.copy(), 0)):
            with pytest.raises(ValueError):
                call()
        assert not hk.default_start_on_device
        # accepted without staged factors after hipkkt_psd_scaling_enable
        hk.h.psd_scaling_enable(True)
        with pytest.raises(ValueError):
            hk.cone_affine_ds()                                     # the enable invalidates the resident scaling
        assert hk.h.update_scaling_ex(s, z, mu, 1, None)[0]
        good_fac, K_good = hk.h.psd_get_factors(), hk.h.debug_dump(4)
        assert np.array_equal(hk.cone_affine_ds()[_rows(cones, lambda c: not _is_psd(c))], first[_rows(cones, lambda c: not _is_psd(c))])
        # a failed PSD cone (S = 0) among good ones: scaling_ok = 0, its K entries untouched, the others served
        psd = [k for k, c in enumerate(cones.cones) if _is_psd(c)]
        kb = psd[1]
        rb = cones.rng_cones[kb]
        s_bad = s.copy()
        s_bad[rb] = 0.0
        z2 = z.copy()
        z2[cones.rng_cones[0]] *= 1.5                                # (the Nonnegative rows move, so their K entries must change)
        ok, *_ = hk.h.update_scaling_ex(s_bad, z2, mu, 1, None)
        assert not ok
        fac, Kb = hk.h.psd_get_factors(), hk.h.debug_dump(4)
        hs = [hk.h.map(2)[r] for r in cones.rng_blocks]
        assert np.array_equal(Kb[hs[kb]], K_good[hs[kb]])
        assert not np.array_equal(Kb[hs[0]], K_good[hs[0]])
        for k in psd:
            if k != kb:
                assert np.array_equal(Kb[hs[k]], K_good[hs[k]])
        n0 = sum(cones.cones[k].n ** 2 for k in psd[:1])
        nb = cones.cones[kb].n ** 2
        assert np.all(np.isnan(fac[0][n0:n0 + nb])) and np.array_equal(fac[0][:n0], good_fac[0][:n0])
        with pytest.raises(ValueError):
            hk.cone_affine_ds()                                     # a failed scaling leaves no step
        assert hk.h.update_scaling_ex(s, z, mu, 1, None)[0]
        assert np.array_equal(hk.h.debug_dump(4), K_good)
        # enable = 0 and a new registration switch it off
        hk.h.step_enable_mixed(False, STEP, AMIN)
        with pytest.raises(ValueError):
            hk.cone_affine_ds()
        with pytest.raises(ValueError):
            hk.h.psd_scaling_enable(True)
        hk.h.step_enable_mixed(True, STEP, AMIN)
        kinds, alpha = cones.kkt_cone_kinds_ex()
        hk.h.set_cone_types_ex(kinds, alpha)
        assert hk.h.update_scaling_ex(s, z, mu, 1, R)[0]
        with pytest.raises(ValueError):
            hk.cone_affine_ds()


# ---- the PSD scaling on the device in mixed mode -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("late", [False, True], ids=["early", "late"])
def test_device_psd_scaling_in_mixed_mode_meets_the_invariants(late):
    with _Timeout(120):
        hn, cones, _ = _handle(_mixed_specs(True), 3, MIXEDN)
        assert hn.steps_mixed and hn.scales_psd
        s, z, mu = _point(cones, np.random.default_rng(61 + int(late)), late)
        assert hn.h.update_scaling_ex(s, z, mu, 1, None)[0]
        R, Ri, lam = hn.h.psd_get_factors()
        fo = lo = 0
        for k, (c, r) in enumerate(zip(cones.cones, cones.rng_cones)):
            if not _is_psd(c):
                continue
            n = c.n
            Rc, Ric, lc = R[fo:fo + n * n].reshape(n, n, order="F"), Ri[fo:fo + n * n].reshape(n, n, order="F"), lam[lo:lo + n]
            fo, lo = fo + n * n, lo + n
            if n != 8:
                continue
            assert np.all(lc > 0) and np.all(np.diff(lc) <= 0)
            assert c.update_scaling(s[r], z[r], mu)
            ref = sr.Reference(n, s[r], z[r])
            sr.gate(f"mixed mode late={late} PSD(8)", n, ref.residuals(Rc, Ric, lc), ref.residuals(c.R, c.Rinv, c.lam))


# ---- the fused calls ------------------------------------------------------------------------------------------------------------------------

def _mix20gp():
    return problems.mixed_psd_nonsym(n=20, psd_sides=[3, 8, 2], nexp=3, npow=3, ngenpow=3, nn=4, nzero=2, socdim=4, seed=6)


@pytest.mark.parametrize("seed,tau", [(5, 0.9), (4, 1e-3)])
def test_fused_steps_and_the_resident_barrier_match_the_granular_calls_and_the_stand_in(seed, tau):
    with _Timeout(120):
        S = cl.Solver(*_mix20gp(), cl.Settings(**MIXED))
        ks, data, cones, v, st = S.kktsystem.kktsolver, S.data, S.cones, S.variables, S.settings
        assert S._device_step and S._device_step_psd and ks.steps_mixed
        n, m = data.n, data.m
        rng = np.random.default_rng(70 + seed)
        s, z, _ = _point(cones, rng, False)
        for c, r in zip(cones.cones, cones.rng_cones):
            if _is_psd(c):
                assert c.update_scaling(s[r], z[r], 1.0)
        v.x[:], v.z[:], v.s[:], v.tau, v.kappa = rng.standard_normal(n), z, s, tau, 0.4
        xzs, res = ks.device_buffer(n + 2 * m), ks.device_buffer(3 * n + 2 * m)
        xzs.upload(np.concatenate([v.x, v.z, v.s]))
        r = S.residuals
        ks.residuals_update_dev(xzs, res, v.tau, v.kappa)
        S._residuals_update()
        mu = (r.dot_sz + v.tau * v.kappa) / (cones.degree + 1)
        # the loop's own scaling call (factors in one upload), then the host-pointer form: the same K, and the host cones adopt
        assert ks.kktsolver_update_scaling_dev_ex(xzs, mu, "dual") and ks.kktsolver_refactor()
        K0 = ks.h.debug_dump(4)
        assert cones.update_scaling(v.s, v.z, mu, "dual")            # every host cone at the point; the non-symmetric ones adopt below
        assert ks.kktsolver_update_scaled(cones, v.s, v.z, mu=mu, strategy="dual")
        assert np.array_equal(ks.h.debug_dump(4), K0)
        exact = _rows(cones, lambda c: isinstance(c, (ZeroCone, NonnegativeCone)) or (not _is_sym(c) and c.numel == 3))

        def check_step(step, scal, ds_const, rhs_kappa, alpha, dtau, dkappa, fraction, lhs_ref, what):
            dx, dz, ds = step[:n], step[n:n + m], step[n + m:]
            scale = max(1.0, np.max(np.abs(lhs_ref.x)), np.max(np.abs(lhs_ref.z)))
            print(f"[mixed fused {what}] max |dx - ref| / scale {np.max(np.abs(dx - lhs_ref.x)) / scale:.2e}, "
                  f"|dz - ref| / scale {np.max(np.abs(dz - lhs_ref.z)) / scale:.2e}")
            assert np.max(np.abs(dx - lhs_ref.x)) <= PARITY * scale and np.max(np.abs(dz - lhs_ref.z)) <= PARITY * scale, what
            assert abs(dtau - lhs_ref.tau) <= PARITY * max(1.0, abs(lhs_ref.tau)), what
            ref = np.zeros(m)
            cones.mul_Hs(ref, dz, np.zeros(m))
            ref = -(ref + ds_const)
            assert np.array_equal(ds[exact], ref[exact]), what
            assert np.max(np.abs(ds - ref)) <= PARITY * max(1.0, np.max(np.abs(ref))), what
            assert dkappa == -(rhs_kappa + v.kappa * dtau) / v.tau, what
            a_tau = -v.tau / dtau if dtau < 0 else ipm.FLOATMAX
            a_kap = -v.kappa / dkappa if dkappa < 0 else ipm.FLOATMAX
            start = min(a_tau, a_kap, 1.0)
            comp = ks.cone_step_length(dz, ds, start)
            print(f"[mixed fused {what}] min(alpha_tau, alpha_kappa, 1) = {start!r}, composite {scal[3]!r}, alpha {alpha!r}")
            assert (scal[3], scal[4]) == comp and comp[0] == comp[1], (what, scal[3:5], comp)
            assert alpha == comp[0] * fraction and scal[0] == alpha, (what, alpha, comp)
            return dz, ds, start

        ok, alpha_aff, dtau_aff, dkappa_aff = ks.kktsolver_step_affine(xzs, res, v.tau, v.kappa, r.rtau, True)
        assert ok
        scal_aff, step_aff = ks.last_step_scalars.copy(), ks.h.step_get()
        lhs, rhs = S.step_lhs, S.step_rhs
        rhs.x[:], rhs.z[:] = r.rx, r.rz
        cones.affine_ds(rhs.s, v.s)
        rhs.tau, rhs.kappa = r.rtau, v.tau * v.kappa
        S.kktsystem._const_pending, S.kktsystem._have_const_dev = False, True
        assert S.kktsystem.kkt_solve(lhs, rhs, data, v, cones, "affine")
        _, _, start_aff = check_step(step_aff, scal_aff, v.s, rhs.kappa, alpha_aff, dtau_aff, dkappa_aff, 1.0, lhs, "affine")
        print(f"[mixed fused affine] tau = {tau}: the line search started from min(alpha_tau, alpha_kappa, 1) = {start_aff!r}")
        sigma, mcorr = (1.0 - alpha_aff) ** 3, 0.5 + 0.4 * alpha_aff
        ok, alpha, dtau, dkappa = ks.kktsolver_step_combined(xzs, res, v.tau, v.kappa, r.rtau, dtau_aff, dkappa_aff, sigma, mu, mcorr)
        assert ok
        scal, step = ks.last_step_scalars.copy(), ks.h.step_get()
        lhs.x[:], lhs.z[:], lhs.s[:] = step_aff[:n], step_aff[n:n + m], step_aff[n + m:]
        lhs.tau, lhs.kappa = dtau_aff, dkappa_aff
        sm = sigma * mu
        rhs.x[:] = (1.0 - sigma) * r.rx
        rhs.tau = (1.0 - sigma) * r.rtau
        rhs.kappa = -sm + mcorr * lhs.tau * lhs.kappa + v.tau * v.kappa
        lhs.z *= mcorr
        cones.affine_ds(rhs.s, v.s)
        cones.combined_ds_shift(rhs.z, lhs.z, lhs.s, sm)
        rhs.s += rhs.z
        rhs.z[:] = (1.0 - sigma) * r.rz
        assert S.kktsystem.kkt_solve(lhs, rhs, data, v, cones, "combined")
        rhs_s_dev = ks.cone_affine_ds() + ks.cone_combined_ds_shift(step_aff[n:n + m] * mcorr, step_aff[n + m:], sm)
        ds_const_dev = ks.cone_ds_from_dz_offset(rhs_s_dev)
        dz, ds, _ = check_step(step, scal, ds_const_dev, rhs.kappa, alpha, dtau, dkappa, st.max_step_fraction, lhs, "combined")
        alphas = [alpha * st.linesearch_backtrack_step ** k for k in range(8)]
        bars, dots = ks.kktsolver_step_barrier(xzs, alphas)
        bars_g, dots_g = ks.cone_barrier(dz, ds, alphas)
        assert np.array_equal(bars, bars_g) and np.array_equal(dots, dots_g)
        if alpha > 0.0:
            _check_barrier(bars, dots, cones, v.z, v.s, dz, ds, alphas, f"mixed resident step {seed}")
        before = xzs.download()
        ks.kktsolver_step_apply(alpha, xzs)
        assert np.array_equal(ks.h.step_get(), step)
        assert np.array_equal(xzs.download(), before + alpha * step)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------

END_TO_END = {
    "exp_psd": dict(n=12, psd_sides=[3, 2], nexp=3, npow=0, ngenpow=0, nn=3, nzero=2, socdim=4, seed=5),
    "mix20": dict(n=20, psd_sides=[3, 8, 1], nexp=3, npow=3, ngenpow=0, nn=4, nzero=2, socdim=4, seed=6),
    "mix20gp": dict(n=20, psd_sides=[3, 8, 2], nexp=3, npow=3, ngenpow=3, nn=4, nzero=2, socdim=4, seed=6),
    "mix40_33": dict(n=40, psd_sides=[33, 5], nexp=5, npow=5, ngenpow=0, nn=6, nzero=3, socdim=5, seed=8),
}
SCALAR_BYTES = 2048      # per iteration: five dots, eight norms, flags, two times fifteen step scalars, up to seven barrier calls of 16


class _Trace(list):
    """the solver's per-iteration records, each with the bytes that had crossed PCIe when the iteration began"""

    def append(self, rec):
        super().append(dict(rec, h2d=hipkkt.TRAFFIC["h2d_bytes"], d2h=hipkkt.TRAFFIC["d2h_bytes"]))


def _solve(prob, forced, **flags):
    st = cl.Settings(**flags)
    if forced:
        st.min_switch_step_length = 1.0      # every PrimalDual step is too short: the Dual strategy from the first iteration on
    S = cl.Solver(*prob, st)
    S.trace = _Trace()
    return S, S.solve()


@pytest.mark.parametrize("forced", [False, True], ids=["default", "forced_dual"])
@pytest.mark.parametrize("name", list(END_TO_END))
def test_ipm_with_the_mixed_device_step_matches_the_host_cone_algebra(name, forced):
    prob = problems.mixed_psd_nonsym(**END_TO_END[name])
    with _Timeout(180):
        H, ref = _solve(prob, forced, **STEP_FLAGS)
        D, got = _solve(prob, forced, **MIXED)
        N, gotn = _solve(prob, forced, **MIXEDN)
    assert not H._device_step
    for S in (D, N):
        ks = S.kktsystem.kktsolver
        assert S._device_step and S._device_step_psd and ks.steps_mixed and S._device_scaling_psd == (S is N)
    st = D.settings
    tol = 2.0 * max(st.tol_gap_abs, st.tol_gap_rel * max(1.0, abs(ref.obj_val)))

    def per_iter(S, sol):
        t = S.trace
        return [(t[k + 1]["h2d"] - t[k]["h2d"], t[k + 1]["d2h"] - t[k]["d2h"]) for k in range(min(sol.iterations, len(t) - 1))]

    bh, bd, bn = per_iter(H, ref), per_iter(D, got), per_iter(N, gotn)
    for what, S, sol, b in (("host cone algebra", H, ref, bh), ("device_step_mixed", D, got, bd), ("+ device_scaling_psd", N, gotn, bn)):
        print(f"[mixed end to end {name} forced={forced}] {what}: {sol.status} in {sol.iterations} iterations, obj {sol.obj_val!r}, "
              f"|dobj| {abs(sol.obj_val - ref.obj_val):.2e} (allowed {tol:.2e}), bytes / iteration up {max(u for u, _ in b)} down "
              f"{max(d for _, d in b)}, barrier searches {S.barrier_searches} (backtracks {S.barrier_backtracks})")
    assert ref.status == got.status == gotn.status == ipm.SOLVED, (ref.status, got.status, gotn.status)
    assert abs(got.obj_val - ref.obj_val) <= tol and abs(gotn.obj_val - ref.obj_val) <= tol
    assert all(u + d <= SCALAR_BYTES for u, d in bn), bn      # scalars only: no row of (s, z) comes down, no factor goes up
    if forced or name == "mix20gp":
        assert D.barrier_searches > 0 and N.barrier_searches > 0      # the Dual strategy searched the barrier on the device
    if forced:
        assert H.barrier_searches > 0
