"""The device-resident interior-point step for PSD triangle cones on the GPU (step_psd.hip, hipkkt_step_enable_psd /
hipkkt_psd_set_factors, Settings.device_step_psd) against the 50-digit reference of tests/psd_step_reference.py, which takes the
resident float64 (R, Rinv, lambda) as exact inputs: the caller's Cholesky / SVD are not charged to the step.

Gates.  Per operation and case the error of the stand-in's host implementation (numpy / LAPACK) against the 50-digit value is measured
in units of eps x the operation's scale (the entrywise bound |A|' |X| |A| pushed through the operation for products, |M|_2 for gamma,
|M|_2 / gamma^2 for alpha = 1 / -gamma).  The device passes when its error is at most
    max(8 x the worst host ratio of that operation at that side, 2 n)        in the same units:
2 n eps is the first-order bound of an n-term dot product applied twice, the factor 8 covers the other summation order and the Jacobi
sweeps.  Where the reference gives alpha_max (gamma >= 0) the device must give alpha_max exactly.  affine_ds is one rounding: `==`.
Rows of kinds 0..2 are compared bit for bit with a handle that has no PSD cone.  Fused calls and end-to-end solves: the gates of
tests/test_gpu_device_step.py (1e-10).  No case is skipped or filtered.  Every figure is printed before it is asserted."""
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
from tests import fixtures as fx
from tests import psd_step_reference as pr
from tests.step_support import PARITY, STEP_FLAGS, _allowance, _soc_mul_hs, _Timeout

pytestmark = pytest.mark.gpu

PSD = dict(device_step=True, device_step_psd=True, **STEP_FLAGS)
SIDES = (1, 2, 3, 5, 8, 17, 32, 33, 64)
T = cl


def _mixed_specs():
    return [T.NonnegativeConeT(3), T.PSDTriangleConeT(3), T.SecondOrderConeT(4), T.PSDTriangleConeT(1), T.ZeroConeT(2),
            T.PSDTriangleConeT(8), T.PSDTriangleConeT(2)]


SETS = {f"side_{n}": (lambda n=n: [T.PSDTriangleConeT(n)]) for n in SIDES}
SETS["mixed"] = _mixed_specs
SETS["twenty_of_5"] = lambda: [T.PSDTriangleConeT(5)] * 20


def _is_psd(c):
    return isinstance(c, PSDTriangleCone)


def _problem(specs, seed):
    rng = np.random.default_rng(seed)
    m = sum(nvars(c) for c in specs)
    n = min(6, m)
    A = sp.random(m, n, density=min(1.0, 12.0 / m + 0.2), random_state=np.random.RandomState(seed), format="csc") + \
        sp.vstack([sp.identity(n), sp.csc_matrix((m - n, n))]).tocsc()
    return sp.identity(n, format="csc") * 1.5, rng.standard_normal(n), A.tocsc(), rng.standard_normal(m), specs


def _handle(specs, seed, flags=PSD):
    """(plugin, cones) for the cone set as given: NOT collapsed, so that a PSD cone of side 1 stays one"""
    P, q, A, b, specs = _problem(specs, seed)
    cones = cl.CompositeCone(specs)
    Pt = sp.triu(sp.csc_matrix(P), format="csc")
    Pt.sort_indices()
    A = sp.csc_matrix(A)
    A.sort_indices()
    m, n = A.shape
    return HipKKTSolver(Pt, A, cones, m, n, cl.Settings(**flags)), cones


def _point(cones, rng, late):
    """(s, z): the PSD members from psd_step_reference.random_sz, the others from the fixtures; every cone's scaling updated"""
    s, z = (fx.scale_cones_late if late else fx.scale_cones)(cones, rng)
    for c, r in zip(cones.cones, cones.rng_cones):
        if _is_psd(c):
            s[r], z[r], mu = pr.random_sz(c, rng, late)
            assert c.update_scaling(s[r], z[r], mu)
    return s, z


def _scale(hk, cones, s, z):
    """factors + scaling on the device (no factorisation); the host's second-order cones adopt the device's (w, lambda, eta)"""
    R = np.concatenate([c.R.ravel(order="F") for c in cones.cones if _is_psd(c)])
    if hk.steps_psd:
        hk.h.psd_set_factors(*hk._psd_factors())
    ok, w, lam, eta = hk.h.update_scaling(s, z, R)
    assert ok
    k = 0
    for c, r in zip(cones.cones, cones.rng_cones):
        if isinstance(c, SecondOrderCone):
            c.adopt_symmetric_scaling(w[r], lam[r], eta[k])
            k += 1


def _scaled(name, seed, late):
    hk, cones = _handle(SETS[name](), seed)
    assert hk.steps_on_device and hk.steps_psd
    rng = np.random.default_rng(900 + seed)
    s, z = _point(cones, rng, late)
    _scale(hk, cones, s, z)
    return hk, cones, s, z, rng


def _ratio(e, scale):
    """max error in units of eps x scale; an entry of scale 0 must be exact"""
    e, scale = np.asarray(e, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(scale > 0, e / (pr.EPS * scale), np.where(e > 0, np.inf, 0.0))
    return float(np.max(q))


def _gate(what, n, got, host, ref, scale):
    rd, rh = _ratio(pr.err(got, ref), scale), _ratio(pr.err(host, ref), scale)
    allowed = max(8.0 * rh, 2.0 * n)
    print(f"[psd step] {what} n={n}: device {rd:.3f}, host {rh:.3f}, allowed {allowed:.1f} (eps x scale)")
    assert rd <= allowed, (what, n, rd, rh)
    return rd, rh


def _alpha_gate(what, n, got, host, a_ref, gamma, norm2):
    """alpha of one cone and side against the reference: `==` where the reference gives its alpha_max"""
    if gamma >= 0:
        print(f"[psd step] {what} n={n}: gamma {float(gamma):.3e} >= 0, device {got!r}, reference {float(a_ref)!r}")
        assert got == float(a_ref), (what, n, got)
        return 0.0, 0.0
    unit = pr.EPS * norm2 / float(gamma) ** 2
    rh, rd = float(abs(pr.mpf(host) - a_ref)) / unit, float(abs(pr.mpf(got) - a_ref)) / unit
    tol = pr.alpha_allowance(gamma, norm2, max(8.0 * rh, 2.0 * n))
    print(f"[psd step] {what} n={n}: gamma / |M|_2 {float(gamma) / norm2:.3e}, device {rd:.3f}, host {rh:.3f}, "
          f"allowed {max(8.0 * rh, 2.0 * n):.1f} (eps |M|_2 / gamma^2)")
    assert abs(pr.mpf(got) - a_ref) <= tol, (what, n, got, float(a_ref), rd, rh)
    return rd, rh


# ---- the granular operations on every set, early and late -------------------------------------------------------------------------------

@pytest.mark.parametrize("late", [False, True])
@pytest.mark.parametrize("name", list(SETS))
def test_granular_operations_match_the_reference(name, late):
    with _Timeout(120):
        hk, cones, s, z, rng = _scaled(name, 3, late)
        m = cones.numel
        K0 = hk.h.debug_dump(4)
        dz = np.concatenate([pr.direction(c, rng, z[r]) if _is_psd(c) else rng.standard_normal(c.numel) * np.abs(z[r]).max()
                             for c, r in zip(cones.cones, cones.rng_cones)])
        ds = np.concatenate([pr.direction(c, rng, s[r]) if _is_psd(c) else rng.standard_normal(c.numel) * np.abs(s[r]).max()
                             for c, r in zip(cones.cones, cones.rng_cones)])
        mu = 1e-9 if late else 1.0
        sm = 0.37 * mu
        dz0, ds0 = dz.copy(), ds.copy()
        got = {"affine_ds": hk.cone_affine_ds(), "mul_Hs": hk.cone_mul_hs(dz), "combined_ds_shift": hk.cone_combined_ds_shift(dz, ds, sm),
               "ds_from_dz_offset": hk.cone_ds_from_dz_offset(ds)}
        assert np.array_equal(dz, dz0) and np.array_equal(ds, ds0)
        assert np.array_equal(hk.h.debug_dump(4), K0)          # no step call writes K
        host = {k: np.zeros(m) for k in got}
        cones.affine_ds(host["affine_ds"], s)
        cones.mul_Hs(host["mul_Hs"], dz, np.zeros(m))
        cones.combined_ds_shift(host["combined_ds_shift"], dz.copy(), ds.copy(), sm)
        cones.ds_from_dz_offset(host["ds_from_dz_offset"], ds, np.zeros(m), z)
        for k, (c, r) in enumerate(zip(cones.cones, cones.rng_cones)):
            if not _is_psd(c):
                continue
            assert np.array_equal(got["affine_ds"][r], host["affine_ds"][r])
            assert pr.err(got["affine_ds"][r], pr.ref_affine_ds(c.lam)).max() <= pr.EPS * float(c.lam.max()) ** 2
            refs = {"mul_Hs": pr.ref_mul_hs(c.R, dz[r]), "combined_ds_shift": pr.ref_shift(c.R, c.Rinv, dz[r], ds[r], sm),
                    "ds_from_dz_offset": pr.ref_offset(c.R, c.lam, ds[r])}
            for op, (ref, scale) in refs.items():
                _gate(f"{name} late={late} cone {k} {op}", c.n, got[op][r], host[op][r], ref, scale)
        # step length: the minimum over the cones of the set, with the allowance of every cone that can be the binding one
        for amax in (1.0, 1e300):
            az, as_ = hk.cone_step_length(dz, ds, amax)
            cand = [[], []]      # per side: (alpha_ref, allowance) of every cone
            for c, r in zip(cones.cones, cones.rng_cones):
                if _is_psd(c):
                    (a_z, a_s), gam, nrm = pr.ref_step_length(c.R, c.Rinv, c.lam, dz[r], ds[r], amax)
                    hz, hs = c.step_length(dz[r], ds[r], z[r], s[r], amax)
                    for side, (a, g, nm, h) in enumerate(((a_z, gam[0], nrm[0], hz), (a_s, gam[1], nrm[1], hs))):
                        rh = 0.0 if g >= 0 else float(abs(pr.mpf(h) - a)) / (pr.EPS * nm / float(g) ** 2)
                        unit = 0.0 if g >= 0 else pr.EPS * nm / float(g) ** 2
                        cand[side].append((float(a), pr.alpha_allowance(g, nm, max(8.0 * rh, 2.0 * c.n)), unit, rh, c.n))
                else:
                    hz, hs = c.step_length(dz[r], ds[r], z[r], s[r], amax)
                    cand[0].append((hz, PARITY * hz if isinstance(c, SecondOrderCone) else 0.0, 0.0, 0.0, 0))
                    cand[1].append((hs, PARITY * hs if isinstance(c, SecondOrderCone) else 0.0, 0.0, 0.0, 0))
            for side, a_dev in enumerate((az, as_)):
                a_ref, _, unit, rh, nb = min(cand[side])
                tol = max(t for a, t, *_ in cand[side] if a - t <= a_ref + max(tt for aa, tt, *_ in cand[side] if aa == a_ref))
                ratio = f"{abs(a_dev - a_ref) / unit:.3f}" if unit > 0 else "-"
                print(f"[psd step] {name} late={late} alpha_max={amax:g} side {'zs'[side]}: device {a_dev!r}, reference {a_ref!r}, "
                      f"allowance {tol:.3e}; binding n={nb}: device {ratio}, host {rh:.3f} (eps |M|_2 / gamma^2)")
                assert abs(a_dev - a_ref) <= tol, (name, late, amax, side, a_dev, a_ref, tol)


# ---- step length: the binding cone ---------------------------------------------------------------------------------------------------------

def test_every_member_of_the_mixed_set_can_bind_alone():
    """directions that stay inside every cone but one, which is left at alpha ~ 1 / c: each PSD cone in turn, then the Nonnegative and
    the second-order member"""
    with _Timeout(120):
        hk, cones, s, z, rng = _scaled("mixed", 4, False)
        members = list(zip(cones.cones, cones.rng_cones))
        for k, (cb, rb) in enumerate(members):
            if isinstance(cb, ZeroCone):
                continue
            dz, ds = 0.5 * z, 0.25 * s                         # inside every cone: alpha_max
            cfac = 2.0 + 0.5 * k
            dz[rb] = -cfac * z[rb]
            ds[rb] = -(cfac + 1.0) * s[rb]
            if _is_psd(cb):
                dz[rb] += 0.05 * pr.direction(cb, rng, z[rb])
                ds[rb] += 0.05 * pr.direction(cb, rng, s[rb])
            az, as_ = hk.cone_step_length(dz, ds, 1.0)
            hz, hs = cb.step_length(dz[rb], ds[rb], z[rb], s[rb], 1.0)
            if _is_psd(cb):
                (a_z, a_s), gam, nrm = pr.ref_step_length(cb.R, cb.Rinv, cb.lam, dz[rb], ds[rb], 1.0)
                assert a_z < 1 and a_s < 1
                _alpha_gate(f"binding PSD cone {k} z", cb.n, az, hz, a_z, gam[0], nrm[0])
                _alpha_gate(f"binding PSD cone {k} s", cb.n, as_, hs, a_s, gam[1], nrm[1])
            elif isinstance(cb, NonnegativeCone):
                print(f"[psd step] binding Nonnegative cone {k}: device {(az, as_)!r}, host {(hz, hs)!r}")
                assert (az, as_) == (hz, hs) and hz < 1.0
            else:
                print(f"[psd step] binding second-order cone {k}: device {(az, as_)!r}, host {(hz, hs)!r}")
                assert abs(az - hz) <= PARITY * hz and abs(as_ - hs) <= PARITY * hs and hz < 1.0
            # nobody else binds
            for j, (c, r) in enumerate(members):
                if j != k:
                    assert c.step_length(dz[r], ds[r], z[r], s[r], 1.0) == (1.0, 1.0)


# ---- step length: edge matrices ------------------------------------------------------------------------------------------------------------

def _dz_with_M(c, Mwant):
    """the svec of dZ = Rinv' Lambda^1/2 M Lambda^1/2 Rinv, for which Lambda^-1/2 R' dZ R Lambda^-1/2 ~ M"""
    L = np.sqrt(c.lam)
    D = c.Rinv.T @ ((L[:, None] * Mwant) * L[None, :]) @ c.Rinv
    return c.mat_to_svec(0.5 * (D + D.T))


@pytest.mark.parametrize("n", [2, 5, 32, 33])
def test_step_length_on_edge_matrices(n):
    with _Timeout(120):
        hk, cones, s, z, rng = _scaled(f"side_{n}", 5, False)
        c = cones.cones[0]
        pos = 0.5 + rng.random(n)
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        B = rng.standard_normal((n, n))
        deg = pos.copy()
        deg[:2] = -1.5
        tiny = pos.copy()
        tiny[0] = -1e-12 * pos.max()
        edges = {
            "dZ = -2 Z (M a multiple of I)": (-2.0 * z, 1.0),
            "M diagonal": (_dz_with_M(c, np.diag(np.linspace(-3.0, 2.0, n))), 1.0),
            "dZ positive definite": (c.mat_to_svec(B @ B.T + np.eye(n)), 1.0),
            "one eigenvalue at -1e-12 |M|": (_dz_with_M(c, (Q * tiny) @ Q.T), 1e300),
            "two-fold smallest eigenvalue": (_dz_with_M(c, (Q * deg) @ Q.T), 1.0),
        }
        for what, (dz, amax) in edges.items():
            ds = 0.5 * s
            az, as_ = hk.cone_step_length(dz, ds, amax)
            hz, _ = c.step_length(dz, ds, z, s, amax)
            (a_z, a_s), gam, nrm = pr.ref_step_length(c.R, c.Rinv, c.lam, dz, ds, amax)
            assert as_ == amax == float(a_s)
            if what == "dZ positive definite":
                assert gam[0] > 0 and az == amax
            else:
                assert gam[0] < 0
            if what == "one eigenvalue at -1e-12 |M|":
                assert -2e-12 < float(gam[0]) / nrm[0] < -0.5e-12
            _alpha_gate(what, n, az, hz, a_z, gam[0], nrm[0])


def test_a_nan_in_dz_gives_alpha_max_for_that_side():
    """an M with a non-finite entry: gamma is NaN and `gamma < 0` is false, on the host and on the device; the call returns at once"""
    with _Timeout(30):
        hk, cones, s, z, rng = _scaled("side_8", 6, False)
        c = cones.cones[0]
        dz, ds = -2.0 * z, -3.0 * s
        dz[4] = np.nan
        az, as_ = hk.cone_step_length(dz, ds, 0.9)
        (_, a_s), gam, nrm = pr.ref_step_length(c.R, c.Rinv, c.lam, -2.0 * z, ds, 0.9)
        _, hs = c.step_length(-2.0 * z, ds, z, s, 0.9)
        print(f"[psd step] NaN direction: alpha_z {az!r}, alpha_s {as_!r}")
        assert az == 0.9
        _alpha_gate("alpha_s next to a NaN dz", c.n, as_, hs, a_s, gam[1], nrm[1])


# ---- the fused calls -----------------------------------------------------------------------------------------------------------------------

def _feasible_problem(specs, seed, n=12):
    """the recipe of problems.sdp_blocks for any symmetric cone set: sparse rows, b = A x0 + an interior point of every cone, P = 0.01 I"""
    rng = np.random.default_rng(seed)
    cones = cl.CompositeCone(specs)
    m = cones.numel
    A = problems._sparse_rows(rng, m, n, 3)
    b = A @ rng.standard_normal(n)
    s0, _ = fx.scale_cones(cones, rng)
    for c, r in zip(cones.cones, cones.rng_cones):
        if isinstance(c, ZeroCone):
            s0[r] = 0.0
    return sp.identity(n, format="csc") * 0.01, rng.standard_normal(n), A, b + s0, specs


@pytest.mark.parametrize("seed,late", [(3, False), (5, True)])
def test_fused_steps_match_the_stand_in_on_the_same_plugin(seed, late):
    """hipkkt_step_affine_dev, _combined_dev and _apply_dev on the mixed set against ipm.KKTSystem.kkt_solve and the host cones driven
    through the same plugin (the pattern of tests/test_gpu_device_step.py)"""
    with _Timeout(120):
        S = cl.Solver(*_feasible_problem(_mixed_specs(), seed), cl.Settings(**PSD))
        assert S._device_step and S._device_step_psd
        ks, data, cones, v = S.kktsystem.kktsolver, S.data, S.cones, S.variables
        n, m = data.n, data.m
        rng = np.random.default_rng(77 + seed)
        s, z = _point(cones, rng, late)
        v.x[:], v.z[:], v.s[:], v.tau, v.kappa = rng.standard_normal(n), z, s, 0.9, 0.4
        xzs, res = ks.device_buffer(n + 2 * m), ks.device_buffer(3 * n + 2 * m)
        xzs.upload(np.concatenate([v.x, v.z, v.s]))
        r = S.residuals
        scal = ks.residuals_update_dev(xzs, res, v.tau, v.kappa)
        S._residuals_update()
        assert scal == (r.dot_qx, r.dot_bz, r.dot_sz, r.dot_xPx, r.rtau)
        # the scaling from the resident iterate, as the loop does it: PSD rows to the host, factors along with the call
        s_h, z_h = ks.psd_rows_download(xzs)
        for c, rr in zip(cones.cones, cones.rng_cones):
            if _is_psd(c):
                assert np.array_equal(s_h[rr], s[rr]) and np.array_equal(z_h[rr], z[rr])
        assert ks.kktsolver_update_scaling_dev(xzs) and ks.kktsolver_refactor()
        K0 = ks.h.debug_dump(4)
        assert ks.kktsolver_update_scaled(cones, v.s, v.z)      # host-pointer form: the same factors, outputs (w, lambda, eta), refactor
        assert np.array_equal(ks.h.debug_dump(4), K0)
        k = 0
        for c, rr in zip(cones.cones, cones.rng_cones):
            if isinstance(c, SecondOrderCone):
                c.adopt_symmetric_scaling(ks.scaling_w[rr], ks.scaling_lambda[rr], ks.scaling_soc_eta[k])
                k += 1
        mu = (r.dot_sz + v.tau * v.kappa) / (cones.degree + 1)

        def check_step(step, ds_const, rhs_kappa, alpha, dtau, dkappa, fraction, lhs_ref, what):
            dx, dz, ds = step[:n], step[n:n + m], step[n + m:]
            scale = max(1.0, np.max(np.abs(lhs_ref.x)), np.max(np.abs(lhs_ref.z)))
            print(f"[psd step fused {what}] max |dx - ref| / scale {np.max(np.abs(dx - lhs_ref.x)) / scale:.2e}, "
                  f"|dz - ref| / scale {np.max(np.abs(dz - lhs_ref.z)) / scale:.2e}")
            assert np.max(np.abs(dx - lhs_ref.x)) <= PARITY * scale and np.max(np.abs(dz - lhs_ref.z)) <= PARITY * scale, what
            assert abs(dtau - lhs_ref.tau) <= PARITY * max(1.0, abs(lhs_ref.tau)), what
            # ds = -(Hs dz + ds_const) from the DEVICE's own dz
            ref = np.zeros(m)
            cones.mul_Hs(ref, dz, np.zeros(m))
            href = -(ref + ds_const)
            cand = [[], []]
            a_tau = -v.tau / dtau if dtau < 0 else ipm.FLOATMAX
            a_kap = -v.kappa / dkappa if dkappa < 0 else ipm.FLOATMAX
            for c, rr in zip(cones.cones, cones.rng_cones):
                if isinstance(c, (ZeroCone, NonnegativeCone)):
                    assert np.array_equal(ds[rr], href[rr]), (what, type(c).__name__)
                elif isinstance(c, SecondOrderCone):
                    t, tol = _allowance(_soc_mul_hs, 1, c, dz[rr])
                    assert np.all(np.abs(ds[rr] - href[rr]) <= tol + 1e-13 * np.abs(ds_const[rr])), what
                else:
                    hs_ref, hs_scale = pr.ref_mul_hs(c.R, dz[rr])
                    ref_c = -(hs_ref + pr.M(ds_const[rr]))
                    _gate(f"fused {what} ds of PSD({c.n})", c.n, ds[rr], href[rr], ref_c, hs_scale + np.abs(ds_const[rr]))
                # (the fused calls run the cones' step length with alpha_max = 1 and take the minimum with alpha_tau, alpha_kappa on the host)
                hz, hs = c.step_length(dz[rr], ds[rr], v.z[rr], v.s[rr], 1.0)
                if _is_psd(c):
                    (a_z, a_s), gam, nrm = pr.ref_step_length(c.R, c.Rinv, c.lam, dz[rr], ds[rr], 1.0)
                    for side, (a, g, nm, h) in enumerate(((a_z, gam[0], nrm[0], hz), (a_s, gam[1], nrm[1], hs))):
                        rh = 0.0 if g >= 0 else float(abs(pr.mpf(h) - a)) / (pr.EPS * nm / float(g) ** 2)
                        cand[side].append((float(a), pr.alpha_allowance(g, nm, max(8.0 * rh, 2.0 * c.n))))
                else:
                    cand[0].append((hz, PARITY * hz))
                    cand[1].append((hs, PARITY * hs))
            assert dkappa == -(rhs_kappa + v.kappa * dtau) / v.tau, what
            got2 = ks.last_step_scalars[3:5]
            for side in (0, 1):
                a_ref = min(a for a, _ in cand[side])
                tol = max(t for a, t in cand[side] if a - t <= a_ref + max(tt for aa, tt in cand[side] if aa == a_ref))
                print(f"[psd step fused {what}] side {'zs'[side]}: device {got2[side]!r}, reference {a_ref!r}, allowance {tol:.3e}")
                assert abs(got2[side] - a_ref) <= tol, (what, side)
            assert alpha == min(a_tau, a_kap, 1.0, got2[0], got2[1]) * fraction, what

        ok, alpha_aff, dtau_aff, dkappa_aff = ks.kktsolver_step_affine(xzs, res, v.tau, v.kappa, r.rtau, True)
        assert ok and np.array_equal(ks.h.debug_dump(4), K0)
        step_aff = ks.h.step_get()
        lhs, rhs = S.step_lhs, S.step_rhs
        rhs.x[:], rhs.z[:] = r.rx, r.rz
        cones.affine_ds(rhs.s, v.s)
        rhs.tau, rhs.kappa = r.rtau, v.tau * v.kappa
        S.kktsystem._const_pending, S.kktsystem._have_const_dev = False, True
        assert S.kktsystem.kkt_solve(lhs, rhs, data, v, cones, "affine")
        check_step(step_aff, v.s, rhs.kappa, alpha_aff, dtau_aff, dkappa_aff, 1.0, lhs, "affine")
        sigma, mcorr = (1.0 - alpha_aff) ** 3, 0.5 + 0.4 * alpha_aff
        ok, alpha, dtau, dkappa = ks.kktsolver_step_combined(xzs, res, v.tau, v.kappa, r.rtau, dtau_aff, dkappa_aff, sigma, mu, mcorr)
        assert ok and np.array_equal(ks.h.debug_dump(4), K0)
        step = ks.h.step_get()
        lhs.x[:], lhs.z[:], lhs.s[:] = step_aff[:n], step_aff[n:n + m], step_aff[n + m:]
        lhs.tau, lhs.kappa = dtau_aff, dkappa_aff
        sm = sigma * mu
        rhs.x[:] = (1.0 - sigma) * r.rx
        rhs.tau = (1.0 - sigma) * r.rtau
        rhs.kappa = -sm + mcorr * lhs.tau * lhs.kappa + v.tau * v.kappa
        lhs.z *= mcorr
        cones.combined_ds_shift(rhs.z, lhs.z, lhs.s, sm)
        rhs.s += rhs.z
        rhs.z[:] = (1.0 - sigma) * r.rz
        assert S.kktsystem.kkt_solve(lhs, rhs, data, v, cones, "combined")
        # ds_const from the granular operations (each held against the reference above): the fused call composes exactly those
        dz_m = step_aff[n:n + m] * mcorr
        rhs_s_dev = ks.cone_affine_ds() + ks.cone_combined_ds_shift(dz_m, step_aff[n + m:], sm)
        ds_const_dev = ks.cone_ds_from_dz_offset(rhs_s_dev)
        check_step(step, ds_const_dev, rhs.kappa, alpha, dtau, dkappa, S.settings.max_step_fraction, lhs, "combined")
        before = xzs.download()
        ks.kktsolver_step_apply(alpha, xzs)
        assert np.array_equal(ks.h.step_get(), step)
        assert np.array_equal(xzs.download(), before + alpha * step)
        assert np.array_equal(ks.h.debug_dump(4), K0)


# ---- the protocol --------------------------------------------------------------------------------------------------------------------------

def test_enable_is_refused_for_what_it_cannot_serve():
    for specs in ([T.PSDTriangleConeT(65)], [T.PSDTriangleConeT(3), T.ExponentialConeT()], [T.NonnegativeConeT(3), T.SecondOrderConeT(4)]):
        hk, cones = _handle(specs, 1, flags={})
        assert not hk.steps_psd
        with pytest.raises(ValueError, match="step_enable_psd"):
            hk.h.step_enable_psd(True)
        hk.h.step_enable_psd(False)                             # switching off is always possible
    # the other enables keep refusing kind 3
    hk, cones = _handle([T.PSDTriangleConeT(3), T.NonnegativeConeT(2)], 1, flags={})
    for fn in (hk.h.step_enable_cone3, hk.h.step_enable_genpow):
        with pytest.raises(ValueError):
            fn(True, 0.8, 1e-4)
    # and a plugin asked for the step on a set that does not qualify keeps the host loop
    hk, cones = _handle([T.PSDTriangleConeT(65)], 1)
    assert not hk.steps_on_device and not hk.steps_psd


def test_scaling_protocol_of_an_enabled_handle():
    hk, cones = _handle(_mixed_specs(), 2)
    m = cones.numel
    rng = np.random.default_rng(5)
    s, z = _point(cones, rng, False)
    R = np.concatenate([c.R.ravel(order="F") for c in cones.cones if _is_psd(c)])
    rinv, lam = hk._psd_factors()
    with pytest.raises(ValueError):
        hk.cone_affine_ds()                                     # no scaling yet
    with pytest.raises(hipkkt.HipKKTError, match="psd_set_factors"):
        hk.h.update_scaling(s, z, R)                            # no factors staged
    hk.h.psd_set_factors(rinv, lam)
    with pytest.raises(hipkkt.HipKKTError):
        hk.h.update_scaling(s, z, None)                         # factors but no psd_R
    ok, *_ = hk.h.update_scaling(s, z, R)
    assert ok
    first = hk.cone_affine_ds()
    with pytest.raises(hipkkt.HipKKTError):
        hk.h.update_scaling(s, z, R)                            # the factors were consumed
    with pytest.raises(ValueError):
        hk.cone_affine_ds()                                     # and the failed call left no scaling
    # a lambda that is not positive: scaling_ok = 0
    bad = lam.copy()
    bad[3] = 0.0
    hk.h.psd_set_factors(rinv, bad)
    ok, *_ = hk.h.update_scaling(s, z, R)
    assert not ok
    with pytest.raises(ValueError):
        hk.cone_mul_hs(np.ones(m))
    bad[3] = np.inf
    hk.h.psd_set_factors(rinv, bad)
    assert not hk.h.update_scaling(s, z, R)[0]
    hk.h.psd_set_factors(rinv, lam)
    assert hk.h.update_scaling(s, z, R)[0]
    assert np.array_equal(hk.cone_affine_ds(), first)
    # the barrier calls stay refused: the set is symmetric
    with pytest.raises(ValueError):
        hk.h.cone_barrier(np.ones(m), np.ones(m), [1.0])
    # a new registration clears the enable: the scaling needs no factors again and the step calls refuse the PSD handle
    hk.h.set_cone_types(cones.kkt_cone_kinds())
    assert hk.h.update_scaling(s, z, R)[0]
    with pytest.raises(ValueError):
        hk.cone_affine_ds()
    with pytest.raises(ValueError):
        hk.h.psd_set_factors(rinv, lam)
    hk.h.step_enable_psd(True)
    with pytest.raises(ValueError):
        hk.cone_affine_ds()                                     # enabling invalidates the resident scaling
    hk.h.psd_set_factors(rinv, lam)
    assert hk.h.update_scaling(s, z, R)[0]
    assert np.array_equal(hk.cone_affine_ds(), first)


def test_rows_of_the_other_kinds_are_bit_identical_to_a_handle_without_psd_cones():
    hk, cones, s, z, rng = _scaled("mixed", 7, False)
    free_specs = [T.NonnegativeConeT(3), T.SecondOrderConeT(4), T.ZeroConeT(2)]
    hf, fcones = _handle(free_specs, 7, flags={})
    assert hf.steps_on_device and not hf.steps_psd
    m = cones.numel
    rows = np.concatenate([np.arange(r.start, r.stop) for c, r in zip(cones.cones, cones.rng_cones) if not _is_psd(c)])
    assert len(rows) == fcones.numel
    ok, *_ = hf.h.update_scaling(s[rows], z[rows])
    assert ok
    dz, ds, x = rng.standard_normal(m), rng.standard_normal(m), rng.standard_normal(m)
    for c, r in zip(cones.cones, cones.rng_cones):
        if _is_psd(c):
            dz[r], ds[r] = 0.5 * z[r], 0.5 * s[r]              # no PSD cone binds
    dz[rows[0]] = -2.0 * z[rows[0]]                            # the first Nonnegative row does
    pairs = [(hk.cone_affine_ds()[rows], hf.cone_affine_ds()), (hk.cone_mul_hs(x)[rows], hf.cone_mul_hs(x[rows])),
             (hk.cone_combined_ds_shift(dz, ds, 0.3)[rows], hf.cone_combined_ds_shift(dz[rows], ds[rows], 0.3)),
             (hk.cone_ds_from_dz_offset(x)[rows], hf.cone_ds_from_dz_offset(x[rows]))]
    for a, b in pairs:
        assert np.array_equal(a, b)
    assert hk.cone_step_length(dz, ds, 1.0) == hf.cone_step_length(dz[rows], ds[rows], 1.0)
    assert hk.cone_step_length(dz, ds, 1.0)[0] < 1.0


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------

def _sdp_relaxation():
    """min <W, X> with diag(X) = 1, X_ij >= -0.2, X in the 3 x 3 PSD cone (x = svec X): a Zero, a Nonnegative and a PSD block"""
    r2 = np.sqrt(2.0)
    W = np.array([[0.0, 1.0, 2.0], [1.0, 0.0, 0.5], [2.0, 0.5, 0.0]])
    q = np.array([W[0, 0], r2 * W[0, 1], W[1, 1], r2 * W[0, 2], r2 * W[1, 2], W[2, 2]])
    diag, off = [0, 2, 5], [1, 3, 4]
    A = np.zeros((12, 6))
    b = np.zeros(12)
    for k, j in enumerate(diag):
        A[k, j], b[k] = 1.0, 1.0
    for k, j in enumerate(off):
        A[3 + k, j], b[3 + k] = -1.0 / r2, 0.2
    A[6:, :] = -np.eye(6)
    return sp.csc_matrix((6, 6)), q, sp.csc_matrix(A), b, [T.ZeroConeT(3), T.NonnegativeConeT(3), T.PSDTriangleConeT(3)]


END_TO_END = {
    "sdp_relaxation_3x3": _sdp_relaxation,
    "three_psd_6": lambda: problems.sdp_blocks(n=30, ncones=3, dim=6, seed=5),
    "mixed_set": lambda: _feasible_problem(_mixed_specs(), 11),
}
_iteration_mismatches = []


@pytest.mark.parametrize("name", list(END_TO_END))
def test_ipm_with_the_psd_device_step_matches_the_host_cone_algebra(name, capsys):
    """Settings(device_step=True, device_step_psd=True) against the host cone algebra on the same plugin: the gate of
    tests/test_gpu_device_step.py test_ipm_with_device_step_matches_the_host_cone_algebra"""
    prob = END_TO_END[name]()
    with _Timeout(120):
        ref_solver = cl.Solver(*prob, cl.Settings(**STEP_FLAGS))
        ref_solver.trace = []
        ref = ref_solver.solve()
        dev_solver = cl.Solver(*prob, cl.Settings(**PSD))
        assert dev_solver._device_step and dev_solver._device_step_psd and not ref_solver._device_step
        dev_solver.trace = []
        got = dev_solver.solve()
    assert got.status == ref.status, (got.status, ref.status)
    assert ref.status == "SOLVED"
    assert abs(got.iterations - ref.iterations) <= 1
    if got.iterations != ref.iterations:      # cause: a step-length / termination test decided by digits below 1e-10
        k = min(got.iterations, ref.iterations)
        with capsys.disabled():
            print(f"\n[psd device-step {name}] iterations {got.iterations} vs {ref.iterations}; at iteration {k}: "
                  f"device {dev_solver.trace[k]} host {ref_solver.trace[k]}")
        _iteration_mismatches.append(name)
        assert len(_iteration_mismatches) <= 1, _iteration_mismatches
        return
    print(f"[psd device-step {name}] {got.status} in {got.iterations} iterations; |dobj| / max(1, |obj|) "
          f"{abs(got.obj_val - ref.obj_val) / max(1.0, abs(ref.obj_val)):.2e}, |d r_prim| {abs(got.r_prim - ref.r_prim):.2e}, "
          f"|d r_dual| {abs(got.r_dual - ref.r_dual):.2e}")
    assert abs(got.obj_val - ref.obj_val) <= PARITY * max(1.0, abs(ref.obj_val)), (got.obj_val, ref.obj_val)
    assert abs(got.r_prim - ref.r_prim) <= PARITY and abs(got.r_dual - ref.r_dual) <= PARITY
