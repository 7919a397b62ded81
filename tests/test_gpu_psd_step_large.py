"""The device-resident interior-point step for PSD triangle cones of side 65 .. 128 on the GPU (step_psd_large.hip,
hipkkt_step_enable_psd_large, Settings.device_step_psd_large).

Two yardsticks.  (1) The kernels of step_psd_large.hip repeat the arithmetic of step_psd.hip with another operand placement, so on a cone
of side <= 64 (testing switch PSD_LARGE_MIN = 1) they must give the bits of step_psd.hip: `np.array_equal` and `==`, no tolerance.
(2) On sides 65 .. 128 the gates of tests/test_gpu_psd_step.py against the 50-digit reference of tests/psd_step_reference.py: device
error <= max(8 x the host stand-in's error ratio at that side, 2 n) in units of eps x the operation's scale, `==` where the reference
gives alpha_max.  mul_W / mul_Winv are held through their compositions mul_Hs = W'(W x) and combined_ds_shift (W dz, W^-T ds), as there.
Fused calls and end-to-end solves: 1e-10 against the stand-in on the same plugin.  No case is skipped or filtered; figures are printed
before they are asserted.  The 50-digit references of one (set, point) are computed once and shared."""
import functools

import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt, problems
from julia_standin import ipm
from julia_standin.cones import SecondOrderCone
from tests import psd_step_reference as pr
from tests import test_gpu_psd_step as tp
from tests.step_support import PARITY, STEP_FLAGS, _Timeout

pytestmark = pytest.mark.gpu

LARGE = dict(device_step=True, device_step_psd=True, device_step_psd_large=True, **STEP_FLAGS)
T = cl


def _mixed_large():
    return [T.NonnegativeConeT(3), T.PSDTriangleConeT(65), T.SecondOrderConeT(4), T.PSDTriangleConeT(8), T.ZeroConeT(2),
            T.PSDTriangleConeT(66)]


SETS = {"side_65": lambda: [T.PSDTriangleConeT(65)], "side_96": lambda: [T.PSDTriangleConeT(96)], "mixed_large": _mixed_large,
        "side_128": lambda: [T.PSDTriangleConeT(128)]}


def _scaled(specs, seed, late, flags=LARGE):
    hk, cones = tp._handle(specs, seed, flags)
    rng = np.random.default_rng(900 + seed)
    s, z = tp._point(cones, rng, late)
    tp._scale(hk, cones, s, z)
    return hk, cones, s, z, rng


def _directions(cones, s, z, rng, bind):
    """(dz, ds): bind -- every PSD cone is left at alpha_z ~ 1 / 2, alpha_s ~ 1 / 3; otherwise no cone binds"""
    dz, ds = 0.5 * z, 0.25 * s
    if bind:
        for c, r in zip(cones.cones, cones.rng_cones):
            if tp._is_psd(c):
                dz[r] = -2.0 * z[r] + 0.05 * pr.direction(c, rng, z[r])
                ds[r] = -3.0 * s[r] + 0.05 * pr.direction(c, rng, s[r])
    return dz, ds


# ---- 1. the bits of the small path ------------------------------------------------------------------------------------------------------

BIT_SETS = {f"side_{n}": (lambda n=n: [T.PSDTriangleConeT(n)]) for n in (1, 2, 5, 32, 33, 63, 64)}
BIT_SETS["mixed"] = tp._mixed_specs


def _pair_of_handles(specs, monkeypatch):
    """the same problem twice, both enabled through hipkkt_step_enable_psd_large: the first routes every PSD cone to step_psd_large.hip
    (PSD_LARGE_MIN = 1, read at the enable), the second routes them to step_psd.hip"""
    monkeypatch.setenv("HIPKKT_PSD_LARGE_MIN", "1")
    hl, cones = tp._handle(specs, 3, flags={})
    hl.h.step_enable_psd_large(True)
    monkeypatch.delenv("HIPKKT_PSD_LARGE_MIN")
    hs, _ = tp._handle(specs, 3, flags={})
    hs.h.step_enable_psd_large(True)
    npsd = sum(tp._is_psd(c) for c in cones.cones)
    assert list(hl.h.debug_dump(24)) == list(range(npsd)) and hs.h.debug_dump(24).size == 0      # who computes which cone
    return hl, hs, cones


def _large_kernels_wrote(hl, hs, cones, y):
    """step_psd.hip computes a cone of side <= 64 on both handles and step_psd_large.hip writes the same rows after it, so equal results
    alone do not show that the large kernels ran.  Their workspace does (debug_dump 25, kernels.h kPsdLargeMats matrices of 128 x 128
    doubles per served cone): after mul_Hs matrix 1 of every served cone holds Y = W'(W x), and mat_to_svec(Y) is the result, bit for
    bit.  The second handle serves no cone through them and has no workspace."""
    assert hs.h.debug_dump(25).size == 0
    ws = hl.h.debug_dump(25)
    psd = [(c, r) for c, r in zip(cones.cones, cones.rng_cones) if tp._is_psd(c)]
    assert ws.size == len(psd) * 4 * 128 * 128
    for slot, (c, r) in enumerate(psd):
        n = c.n
        Y = ws[(4 * slot + 1) * 128 * 128:][:n * n].reshape((n, n), order="F")
        got = np.array([Y[i, j] if i == j else (Y[i, j] + Y[j, i]) * 0.7071067811865475 for j in range(n) for i in range(j + 1)])
        assert np.array_equal(got, y[r]), (slot, n)
        assert np.any(y[r] != 0.0)


@pytest.mark.parametrize("late", [False, True])
@pytest.mark.parametrize("name", list(BIT_SETS))
def test_the_large_kernels_give_the_bits_of_the_small_ones(name, late, monkeypatch):
    with _Timeout(120):
        hl, hs, cones = _pair_of_handles(BIT_SETS[name](), monkeypatch)
        m = cones.numel
        rng = np.random.default_rng(31)
        s, z = tp._point(cones, rng, late)
        R = np.concatenate([c.R.ravel(order="F") for c in cones.cones if tp._is_psd(c)])
        rinv, lam = hl._psd_factors()                           # (`cones` are the first handle's: both get these factors)
        for hk in (hl, hs):
            hk.h.psd_set_factors(rinv, lam)
            assert hk.h.update_scaling(s, z, R)[0]
        sm = 0.37 * (1e-9 if late else 1.0)
        x = rng.standard_normal(m)
        bind, free = _directions(cones, s, z, rng, True), _directions(cones, s, z, rng, False)
        nan = (bind[0].copy(), bind[1])
        nan[0][cones.rng_cones[[tp._is_psd(c) for c in cones.cones].index(True)].start] = np.nan
        assert np.array_equal(hl.cone_affine_ds(), hs.cone_affine_ds())
        y = hl.cone_mul_hs(x)
        assert np.array_equal(y, hs.cone_mul_hs(x))
        _large_kernels_wrote(hl, hs, cones, y)
        assert np.array_equal(hl.cone_ds_from_dz_offset(x), hs.cone_ds_from_dz_offset(x))
        for what, (dz, ds) in (("binding", bind), ("free", free), ("nan", nan)):
            a, b = hl.cone_step_length(dz, ds, 1.0), hs.cone_step_length(dz, ds, 1.0)
            print(f"[psd large bits] {name} late={late} {what}: step lengths {a!r} / {b!r}")
            assert a == b, (what, a, b)
            assert a == hl.cone_step_length(dz, ds, 1.0)
            if what == "binding":
                assert a[0] < 1.0 and a[1] < 1.0
            if what == "free":
                assert a == (1.0, 1.0)
            for amax in (0.9, 1e300):
                assert hl.cone_step_length(dz, ds, amax) == hs.cone_step_length(dz, ds, amax), (what, amax)
            nanok = what == "nan"
            assert np.array_equal(hl.cone_combined_ds_shift(dz, ds, sm), hs.cone_combined_ds_shift(dz, ds, sm), equal_nan=nanok), what
            assert np.array_equal(hl.cone_mul_hs(dz), hs.cone_mul_hs(dz), equal_nan=nanok), what
            assert np.array_equal(hl.cone_ds_from_dz_offset(ds), hs.cone_ds_from_dz_offset(ds)), what


def test_the_fused_calls_give_the_bits_of_the_small_path(monkeypatch):
    """one hipkkt_step_affine_dev + hipkkt_step_combined_dev pair on the mixed set through both routings: hipkkt_step_get bit for bit"""
    with _Timeout(120):
        steps = []
        for lmin in ("1", None):
            if lmin:
                monkeypatch.setenv("HIPKKT_PSD_LARGE_MIN", lmin)
            else:
                monkeypatch.delenv("HIPKKT_PSD_LARGE_MIN")
            S = cl.Solver(*tp._feasible_problem(tp._mixed_specs(), 3), cl.Settings(**STEP_FLAGS))
            ks, data, cones, v, r = S.kktsystem.kktsolver, S.data, S.cones, S.variables, S.residuals
            ks.h.step_enable_psd_large(True)
            assert ks.h.debug_dump(24).size == (sum(tp._is_psd(c) for c in cones.cones) if lmin else 0) and any(map(tp._is_psd, cones.cones))
            n, m = data.n, data.m
            rng = np.random.default_rng(80)
            s, z = tp._point(cones, rng, False)
            v.x[:], v.z[:], v.s[:], v.tau, v.kappa = rng.standard_normal(n), z, s, 0.9, 0.4
            xzs, res = ks.device_buffer(n + 2 * m), ks.device_buffer(3 * n + 2 * m)
            xzs.upload(np.concatenate([v.x, v.z, v.s]))
            ks.residuals_update_dev(xzs, res, v.tau, v.kappa)
            S._residuals_update()
            R = np.concatenate([c.R.ravel(order="F") for c in cones.cones if tp._is_psd(c)])
            ks.h.psd_set_factors(*ks._psd_factors())
            assert ks.h.update_scaling(v.s, v.z, R)[0] and ks.kktsolver_refactor()
            mu = (r.dot_sz + v.tau * v.kappa) / (cones.degree + 1)
            ok, alpha_aff, dtau_aff, dkappa_aff = ks.kktsolver_step_affine(xzs, res, v.tau, v.kappa, r.rtau, True)
            assert ok
            aff = ks.h.step_get()
            ok, alpha, dtau, dkappa = ks.kktsolver_step_combined(xzs, res, v.tau, v.kappa, r.rtau, dtau_aff, dkappa_aff,
                                                                 (1.0 - alpha_aff) ** 3, mu, 0.5 + 0.4 * alpha_aff)
            assert ok
            steps.append((aff, ks.h.step_get(), alpha_aff, alpha, tuple(ks.last_step_scalars[3:5])))
        (a0, c0, *s0), (a1, c1, *s1) = steps
        print(f"[psd large bits] fused: alphas {s0!r} / {s1!r}")
        assert np.array_equal(a0, a1) and np.array_equal(c0, c1) and s0 == s1


# ---- 2. against the 50-digit reference -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(name, late):
    """the scaled handle, the inputs and the device's results of one (set, point): shared by the tests below, never modified"""
    hk, cones, s, z, rng = _scaled(SETS[name](), 3, late)
    assert hk.steps_on_device and hk.steps_psd and hk.steps_psd_large
    psd_sides = [c.n for c in cones.cones if tp._is_psd(c)]
    assert list(hk.h.debug_dump(24)) == [k for k, n in enumerate(psd_sides) if n >= 65]      # the others stay with step_psd.hip
    dz, ds = _directions(cones, s, z, rng, True)
    x = np.concatenate([pr.direction(c, rng, z[r]) if tp._is_psd(c) else rng.standard_normal(c.numel) * np.abs(z[r]).max()
                        for c, r in zip(cones.cones, cones.rng_cones)])
    sm = 0.37 * (1e-9 if late else 1.0)
    return dict(hk=hk, cones=cones, s=s, z=z, dz=dz, ds=ds, x=x, sm=sm)


def _ops(C):
    hk = C["hk"]
    return {"affine_ds": hk.cone_affine_ds(), "mul_Hs": hk.cone_mul_hs(C["x"]),
            "combined_ds_shift": hk.cone_combined_ds_shift(C["dz"], C["ds"], C["sm"]),
            "ds_from_dz_offset": hk.cone_ds_from_dz_offset(C["ds"]), "step_length": hk.cone_step_length(C["dz"], C["ds"], 1.0),
            "step_length_free": hk.cone_step_length(C["dz"], C["ds"], 1e300)}


def _check_step_length(name, cones, s, z, dz, ds, got1, gotfree):
    """both alpha_max with one reference gamma per cone and side: the minimum over the set, with the allowance of every cone that can bind"""
    cand = {1.0: [[], []], 1e300: [[], []]}
    for c, r in zip(cones.cones, cones.rng_cones):
        if tp._is_psd(c):
            gam = (pr.ref_gamma(c.R, c.lam, dz[r], False), pr.ref_gamma(c.Rinv, c.lam, ds[r], True))
        for amax in cand:
            hz, hs = c.step_length(dz[r], ds[r], z[r], s[r], amax)
            for side, h in enumerate((hz, hs)):
                if tp._is_psd(c):
                    g, nm = gam[side]
                    a = pr.alpha_of(g, amax)
                    rh = 0.0 if g >= 0 else float(abs(pr.mpf(h) - a)) / (pr.EPS * nm / float(g) ** 2)
                    unit = 0.0 if g >= 0 else pr.EPS * nm / float(g) ** 2
                    cand[amax][side].append((float(a), pr.alpha_allowance(g, nm, max(8.0 * rh, 2.0 * c.n)), unit, rh, c.n))
                else:
                    cand[amax][side].append((h, PARITY * h if isinstance(c, SecondOrderCone) else 0.0, 0.0, 0.0, 0))
    for amax, got in ((1.0, got1), (1e300, gotfree)):
        for side, a_dev in enumerate(got):
            a_ref, _, unit, rh, nb = min(cand[amax][side])
            tol = max(t for a, t, *_ in cand[amax][side]
                      if a - t <= a_ref + max(tt for aa, tt, *_ in cand[amax][side] if aa == a_ref))
            ratio = f"{abs(a_dev - a_ref) / unit:.3f}" if unit > 0 else "-"
            print(f"[psd large] {name} alpha_max={amax:g} side {'zs'[side]}: device {a_dev!r}, reference {a_ref!r}, allowance {tol:.3e}; "
                  f"binding n={nb}: device {ratio}, host {rh:.3f} (eps |M|_2 / gamma^2)")
            assert abs(a_dev - a_ref) <= tol, (name, amax, side, a_dev, a_ref, tol)
    assert got1[0] < 1.0 and got1[1] < 1.0                # the direction binds


@pytest.mark.parametrize("late", [False, True])
@pytest.mark.parametrize("name", ["side_65", "side_96", "mixed_large"])
def test_granular_operations_match_the_reference(name, late):
    with _Timeout(300):
        C = _case(name, late)
        hk, cones, s, z, dz, ds, x, sm = (C[k] for k in ("hk", "cones", "s", "z", "dz", "ds", "x", "sm"))
        m = cones.numel
        K0 = hk.h.debug_dump(4)
        got = _ops(C)
        assert np.array_equal(hk.h.debug_dump(4), K0)          # no step call writes K
        host = {k: np.zeros(m) for k in ("affine_ds", "mul_Hs", "combined_ds_shift", "ds_from_dz_offset")}
        cones.affine_ds(host["affine_ds"], s)
        cones.mul_Hs(host["mul_Hs"], x, np.zeros(m))
        cones.combined_ds_shift(host["combined_ds_shift"], dz.copy(), ds.copy(), sm)
        cones.ds_from_dz_offset(host["ds_from_dz_offset"], ds, np.zeros(m), z)
        for k, (c, r) in enumerate(zip(cones.cones, cones.rng_cones)):
            if not tp._is_psd(c):
                continue
            assert np.array_equal(got["affine_ds"][r], host["affine_ds"][r])
            assert pr.err(got["affine_ds"][r], pr.ref_affine_ds(c.lam)).max() <= pr.EPS * float(c.lam.max()) ** 2
            refs = {"mul_Hs": pr.ref_mul_hs(c.R, x[r]), "combined_ds_shift": pr.ref_shift(c.R, c.Rinv, dz[r], ds[r], sm),
                    "ds_from_dz_offset": pr.ref_offset(c.R, c.lam, ds[r])}
            for op, (ref, scale) in refs.items():
                tp._gate(f"{name} late={late} cone {k} {op}", c.n, got[op][r], host[op][r], ref, scale)
        _check_step_length(f"{name} late={late}", cones, s, z, dz, ds, got["step_length"], got["step_length_free"])


def test_side_128_at_the_lds_limit():
    """one early point; mul_Hs and the step length of z and s: three references"""
    with _Timeout(300):
        C = _case("side_128", False)
        hk, cones, s, z, dz, ds, x = (C[k] for k in ("hk", "cones", "s", "z", "dz", "ds", "x"))
        c = cones.cones[0]
        host = np.zeros(cones.numel)
        cones.mul_Hs(host, x, np.zeros(cones.numel))
        ref, scale = pr.ref_mul_hs(c.R, x)
        tp._gate("side_128 mul_Hs", c.n, hk.cone_mul_hs(x), host, ref, scale)
        az, as_ = hk.cone_step_length(dz, ds, 1.0)
        hz, hs = c.step_length(dz, ds, z, s, 1.0)
        (gz, nz), (gs, ns) = pr.ref_gamma(c.R, c.lam, dz, False), pr.ref_gamma(c.Rinv, c.lam, ds, True)
        assert gz < 0 and gs < 0 and az < 1.0 and as_ < 1.0
        tp._alpha_gate("side_128 z", c.n, az, hz, pr.alpha_of(gz, 1.0), gz, nz)
        tp._alpha_gate("side_128 s", c.n, as_, hs, pr.alpha_of(gs, 1.0), gs, ns)


def test_every_psd_member_of_the_mixed_set_can_bind_alone():
    """directions that stay inside every cone but one PSD cone, which is left at alpha ~ 1 / c: PSD(65) (slot 0 of the batch), PSD(8)
    (step_psd.hip) and PSD(66) (slot 1, the batch's largest side) in turn -- a pair written to the wrong place would leave alpha_max"""
    with _Timeout(300):
        C = _case("mixed_large", False)
        hk, cones, s, z = C["hk"], C["cones"], C["s"], C["z"]
        rng = np.random.default_rng(41)
        members = list(zip(cones.cones, cones.rng_cones))
        for k, (cb, rb) in enumerate(members):
            if not tp._is_psd(cb):
                continue
            dz, ds = 0.5 * z, 0.25 * s
            cfac = 2.0 + 0.5 * k
            dz[rb] = -cfac * z[rb] + 0.05 * pr.direction(cb, rng, z[rb])
            ds[rb] = -(cfac + 1.0) * s[rb] + 0.05 * pr.direction(cb, rng, s[rb])
            az, as_ = hk.cone_step_length(dz, ds, 1.0)
            hz, hs = cb.step_length(dz[rb], ds[rb], z[rb], s[rb], 1.0)
            (a_z, a_s), gam, nrm = pr.ref_step_length(cb.R, cb.Rinv, cb.lam, dz[rb], ds[rb], 1.0)
            assert a_z < 1 and a_s < 1
            tp._alpha_gate(f"binding PSD cone {k} z", cb.n, az, hz, a_z, gam[0], nrm[0])
            tp._alpha_gate(f"binding PSD cone {k} s", cb.n, as_, hs, a_s, gam[1], nrm[1])
            for j, (c, r) in enumerate(members):
                if j != k:
                    assert c.step_length(dz[r], ds[r], z[r], s[r], 1.0) == (1.0, 1.0)


# ---- 3. step length: edge matrices ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [65, 96])
def test_step_length_on_edge_matrices(n):
    with _Timeout(300):
        C = _case(f"side_{n}", False)
        hk, cones, s, z = C["hk"], C["cones"], C["s"], C["z"]
        rng = np.random.default_rng(5)
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
            "M diagonal": (tp._dz_with_M(c, np.diag(np.linspace(-3.0, 2.0, n))), 1.0),
            "dZ positive definite": (c.mat_to_svec(B @ B.T + np.eye(n)), 1.0),
            "one eigenvalue at -1e-12 |M|": (tp._dz_with_M(c, (Q * tiny) @ Q.T), 1e300),
            "two-fold smallest eigenvalue": (tp._dz_with_M(c, (Q * deg) @ Q.T), 1.0),
        }
        ds = 0.5 * s
        for what, (dz, amax) in edges.items():
            az, as_ = hk.cone_step_length(dz, ds, amax)
            hz, _ = c.step_length(dz, ds, z, s, amax)
            gz, nz = pr.ref_gamma(c.R, c.lam, dz, False)
            assert as_ == amax                                  # dS = S / 2: M_s = I / 2, gamma_s > 0 without a reference
            if what == "dZ positive definite":
                assert gz > 0 and az == amax
            else:
                assert gz < 0
            if what == "one eigenvalue at -1e-12 |M|":
                assert -2e-12 < float(gz) / nz < -0.5e-12
            tp._alpha_gate(what, n, az, hz, pr.alpha_of(gz, amax), gz, nz)


# ---- 4. rows the feature must not touch ---------------------------------------------------------------------------------------------------

def test_rows_of_the_other_kinds_and_of_the_small_psd_cone_are_bit_identical():
    with _Timeout(120):
        C = _case("mixed_large", False)
        hk, cones, s, z = C["hk"], C["cones"], C["s"], C["z"]
        m = cones.numel
        rng = np.random.default_rng(17)
        members = list(zip(cones.cones, cones.rng_cones))
        free_rows = np.concatenate([np.arange(r.start, r.stop) for c, r in members if not tp._is_psd(c)])
        small_rows = np.concatenate([np.arange(r.start, r.stop) for c, r in members if not tp._is_psd(c) or c.n == 8])
        hf, fcones = tp._handle([T.NonnegativeConeT(3), T.SecondOrderConeT(4), T.ZeroConeT(2)], 7, flags={})
        assert hf.steps_on_device and not hf.steps_psd and len(free_rows) == fcones.numel
        assert hf.h.update_scaling(s[free_rows], z[free_rows])[0]
        h8, cones8 = tp._handle([T.NonnegativeConeT(3), T.SecondOrderConeT(4), T.PSDTriangleConeT(8), T.ZeroConeT(2)], 7, flags=tp.PSD)
        assert h8.steps_psd and not h8.steps_psd_large and len(small_rows) == cones8.numel
        c8 = [c for c in cones.cones if tp._is_psd(c) and c.n == 8][0]
        h8.h.psd_set_factors(c8.Rinv.ravel(order="F"), c8.lam)
        assert h8.h.update_scaling(s[small_rows], z[small_rows], c8.R.ravel(order="F"))[0]
        dz, ds, x = rng.standard_normal(m), rng.standard_normal(m), rng.standard_normal(m)
        for c, r in members:
            if tp._is_psd(c):
                dz[r], ds[r] = 0.5 * z[r], 0.5 * s[r]          # no PSD cone binds ...
        dz[free_rows[0]] = -2.0 * z[free_rows[0]]              # ... the first Nonnegative row does
        for rows, other in ((free_rows, hf), (small_rows, h8)):
            pairs = [(hk.cone_affine_ds()[rows], other.cone_affine_ds()), (hk.cone_mul_hs(x)[rows], other.cone_mul_hs(x[rows])),
                     (hk.cone_combined_ds_shift(dz, ds, 0.3)[rows], other.cone_combined_ds_shift(dz[rows], ds[rows], 0.3)),
                     (hk.cone_ds_from_dz_offset(x)[rows], other.cone_ds_from_dz_offset(x[rows]))]
            for a, b in pairs:
                assert np.array_equal(a, b)
            assert hk.cone_step_length(dz, ds, 1.0) == other.cone_step_length(dz[rows], ds[rows], 1.0)
        assert hk.cone_step_length(dz, ds, 1.0)[0] < 1.0
        # the PSD(8) cone binding alone: its pair comes from step_psd.hip on both handles
        r8 = [r for c, r in members if c is c8][0]
        dz[free_rows[0]] = 0.5 * z[free_rows[0]]
        dz[r8], ds[r8] = -2.5 * z[r8] + 0.05 * pr.direction(c8, rng, z[r8]), -3.5 * s[r8]
        a = hk.cone_step_length(dz, ds, 1.0)
        assert a == h8.cone_step_length(dz[small_rows], ds[small_rows], 1.0) and a[0] < 1.0 and a[1] < 1.0


# ---- 5. the fused calls --------------------------------------------------------------------------------------------------------------------

def test_fused_steps_match_the_stand_in_on_the_same_plugin():
    """hipkkt_step_affine_dev, _combined_dev and _apply_dev on mixed_large against ipm.KKTSystem.kkt_solve and the host cones driven
    through the same plugin at PARITY; ds and the step lengths are the granular operations' (held to the reference above) bit for bit"""
    with _Timeout(300):
        S = cl.Solver(*tp._feasible_problem(_mixed_large(), 3), cl.Settings(**LARGE))
        assert S._device_step and S._device_step_psd and not S._device_scaling_psd and not S._device_default_start
        ks, data, cones, v, r = S.kktsystem.kktsolver, S.data, S.cones, S.variables, S.residuals
        assert ks.steps_psd_large
        n, m = data.n, data.m
        rng = np.random.default_rng(80)
        s, z = tp._point(cones, rng, False)
        v.x[:], v.z[:], v.s[:], v.tau, v.kappa = rng.standard_normal(n), z, s, 0.9, 0.4
        xzs, res = ks.device_buffer(n + 2 * m), ks.device_buffer(3 * n + 2 * m)
        xzs.upload(np.concatenate([v.x, v.z, v.s]))
        scal = ks.residuals_update_dev(xzs, res, v.tau, v.kappa)
        S._residuals_update()
        assert scal == (r.dot_qx, r.dot_bz, r.dot_sz, r.dot_xPx, r.rtau)
        assert ks.kktsolver_update_scaling_dev(xzs) and ks.kktsolver_refactor()
        K0 = ks.h.debug_dump(4)
        assert ks.kktsolver_update_scaled(cones, v.s, v.z)
        assert np.array_equal(ks.h.debug_dump(4), K0)
        k = 0
        for c, rr in zip(cones.cones, cones.rng_cones):
            if isinstance(c, SecondOrderCone):
                c.adopt_symmetric_scaling(ks.scaling_w[rr], ks.scaling_lambda[rr], ks.scaling_soc_eta[k])
                k += 1
        mu = (r.dot_sz + v.tau * v.kappa) / (cones.degree + 1)
        psd_rows = np.concatenate([np.arange(rr.start, rr.stop) for c, rr in zip(cones.cones, cones.rng_cones) if tp._is_psd(c)])

        def check_step(step, ds_const, rhs_kappa, alpha, dtau, dkappa, fraction, lhs_ref, what):
            dx, dz, ds = step[:n], step[n:n + m], step[n + m:]
            scale = max(1.0, np.max(np.abs(lhs_ref.x)), np.max(np.abs(lhs_ref.z)))
            print(f"[psd large fused {what}] max |dx - ref| / scale {np.max(np.abs(dx - lhs_ref.x)) / scale:.2e}, "
                  f"|dz - ref| / scale {np.max(np.abs(dz - lhs_ref.z)) / scale:.2e}, |dtau - ref| {abs(dtau - lhs_ref.tau):.2e}")
            assert np.max(np.abs(dx - lhs_ref.x)) <= PARITY * scale and np.max(np.abs(dz - lhs_ref.z)) <= PARITY * scale, what
            assert abs(dtau - lhs_ref.tau) <= PARITY * max(1.0, abs(lhs_ref.tau)), what
            assert dkappa == -(rhs_kappa + v.kappa * dtau) / v.tau, what
            # ds = -(Hs dz + ds_const) from the DEVICE's own dz: the granular mul_Hs on the PSD rows bit for bit, the stand-in at PARITY
            assert np.array_equal(ds[psd_rows], -(ks.cone_mul_hs(dz) + ds_const)[psd_rows]), what
            ref = np.zeros(m)
            cones.mul_Hs(ref, dz, np.zeros(m))
            href = -(ref + ds_const)
            sc = max(1.0, np.max(np.abs(href)))
            print(f"[psd large fused {what}] max |ds - stand-in| / scale {np.max(np.abs(ds - href)) / sc:.2e}")
            assert np.max(np.abs(ds - href)) <= PARITY * sc, what
            got2 = tuple(ks.last_step_scalars[3:5])
            assert got2 == ks.cone_step_length(dz, ds, 1.0), what
            a_tau = -v.tau / dtau if dtau < 0 else ipm.FLOATMAX
            a_kap = -v.kappa / dkappa if dkappa < 0 else ipm.FLOATMAX
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
        dz_m = step_aff[n:n + m] * mcorr
        rhs_s_dev = ks.cone_affine_ds() + ks.cone_combined_ds_shift(dz_m, step_aff[n + m:], sm)
        ds_const_dev = ks.cone_ds_from_dz_offset(rhs_s_dev)
        check_step(step, ds_const_dev, rhs.kappa, alpha, dtau, dkappa, S.settings.max_step_fraction, lhs, "combined")
        before = xzs.download()
        ks.kktsolver_step_apply(alpha, xzs)
        assert np.array_equal(ks.h.step_get(), step)
        assert np.array_equal(xzs.download(), before + alpha * step)
        assert np.array_equal(ks.h.debug_dump(4), K0)          # hipkkt_step_apply_dev leaves K untouched


# ---- 6. the protocol -----------------------------------------------------------------------------------------------------------------------

def test_enables_refuse_what_they_cannot_serve():
    for specs in ([T.PSDTriangleConeT(129)], [T.PSDTriangleConeT(65), T.ExponentialConeT()], [T.NonnegativeConeT(3), T.SecondOrderConeT(4)]):
        hk, cones = tp._handle(specs, 1, flags={})
        with pytest.raises(ValueError, match="step_enable_psd_large"):
            hk.h.step_enable_psd_large(True)
        hk.h.step_enable_psd_large(False)                       # switching off is always possible
    hk, cones = tp._handle([T.PSDTriangleConeT(65)], 1, flags={})
    with pytest.raises(ValueError, match="step_enable_psd"):
        hk.h.step_enable_psd(True)                              # the small enable keeps its limit
    hk.h.step_enable_psd_large(True)
    # a plugin asked for everything on [PSD(65)]: the step on the device, the Cholesky / SVD and the default start with the caller
    hk, cones = tp._handle([T.PSDTriangleConeT(65)], 1, flags=dict(LARGE, device_scaling_psd=True, device_default_start=True))
    assert hk.steps_on_device and hk.steps_psd and hk.steps_psd_large and not hk.scales_psd and not hk.default_start_on_device
    # without the setting the set keeps the host loop; sides above 128 keep it with the setting
    assert not tp._handle([T.PSDTriangleConeT(65)], 1, flags=tp.PSD)[0].steps_on_device
    assert not tp._handle([T.PSDTriangleConeT(129)], 1, flags=LARGE)[0].steps_on_device


def test_scaling_and_start_calls_refuse_a_side_above_64_and_serve_the_others():
    hk, cones = tp._handle([T.PSDTriangleConeT(65), T.NonnegativeConeT(2)], 2, flags=LARGE)
    assert hk.steps_psd_large
    m = cones.numel
    v = np.ones(m)
    xzs = hk.device_buffer(hk.n + 2 * m)
    hk.h.set_qb(np.ones(hk.n), np.ones(m))
    for call in (lambda: hk.h.psd_scaling_enable(True), hk.h.cone_set_identity_scaling, lambda: hk.h.cone_margins(v, 0),
                 lambda: hk.h.cone_shift_to_interior(v, 1), lambda: hk.h.step_default_start_dev(xzs.ptr)):
        with pytest.raises(ValueError):
            call()
    specs = [T.PSDTriangleConeT(8), T.NonnegativeConeT(2)]
    hl, cones = tp._handle(specs, 2, flags={})
    hl.h.step_enable_psd_large(True)
    hs, _ = tp._handle(specs, 2, flags=tp.PSD)
    rng = np.random.default_rng(4)
    v = rng.standard_normal(cones.numel)
    assert hl.h.cone_margins(v, 0) == hs.h.cone_margins(v, 0)
    a, b = hl.h.cone_shift_to_interior(v, 1), hs.h.cone_shift_to_interior(v, 1)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    hl.h.cone_set_identity_scaling()
    hl.h.psd_scaling_enable(True)
    hl.h.set_qb(np.ones(hl.n), np.ones(cones.numel))
    xzs = hl.device_buffer(hl.n + 2 * cones.numel)
    assert hl.h.step_default_start_dev(xzs.ptr)[0]


def test_scaling_protocol_of_an_enabled_handle():
    hk, cones = tp._handle([T.PSDTriangleConeT(65), T.NonnegativeConeT(3)], 2, flags=LARGE)
    m = cones.numel
    rng = np.random.default_rng(5)
    s, z = tp._point(cones, rng, False)
    R = np.concatenate([c.R.ravel(order="F") for c in cones.cones if tp._is_psd(c)])
    rinv, lam = hk._psd_factors()
    with pytest.raises(ValueError):
        hk.cone_affine_ds()                                     # no scaling yet
    with pytest.raises(hipkkt.HipKKTError, match="psd_set_factors"):
        hk.h.update_scaling(s, z, R)                            # no factors staged
    hk.h.psd_set_factors(rinv, lam)
    with pytest.raises(hipkkt.HipKKTError):
        hk.h.update_scaling(s, z, None)                         # factors but no psd_R
    assert hk.h.update_scaling(s, z, R)[0]
    first = hk.cone_affine_ds()
    Rg, Rinvg, lamg = hk.h.psd_get_factors()
    assert np.array_equal(Rg, R) and np.array_equal(Rinvg, rinv) and np.array_equal(lamg, lam)
    with pytest.raises(hipkkt.HipKKTError):
        hk.h.update_scaling(s, z, R)                            # the factors were consumed
    with pytest.raises(ValueError):
        hk.cone_affine_ds()                                     # and the failed call left no scaling
    bad = lam.copy()
    bad[3] = 0.0
    hk.h.psd_set_factors(rinv, bad)
    assert not hk.h.update_scaling(s, z, R)[0]                  # a lambda that is not positive: scaling_ok = 0
    with pytest.raises(ValueError):
        hk.cone_mul_hs(np.ones(m))
    bad[3] = np.inf
    hk.h.psd_set_factors(rinv, bad)
    assert not hk.h.update_scaling(s, z, R)[0]
    hk.h.psd_set_factors(rinv, lam)
    assert hk.h.update_scaling(s, z, R)[0]
    assert np.array_equal(hk.cone_affine_ds(), first)
    with pytest.raises(ValueError):
        hk.h.cone_barrier(np.ones(m), np.ones(m), [1.0])        # the set is symmetric
    # a new registration clears the enable; enabling again invalidates the resident scaling
    hk.h.set_cone_types(cones.kkt_cone_kinds())
    assert hk.h.update_scaling(s, z, R)[0]
    with pytest.raises(ValueError):
        hk.cone_affine_ds()
    with pytest.raises(ValueError):
        hk.h.psd_set_factors(rinv, lam)
    hk.h.step_enable_psd_large(True)
    with pytest.raises(ValueError):
        hk.cone_affine_ds()
    hk.h.psd_set_factors(rinv, lam)
    assert hk.h.update_scaling(s, z, R)[0]
    assert np.array_equal(hk.cone_affine_ds(), first)
    hk.h.step_enable_psd_large(False)                           # what hipkkt_step_enable_psd(h, 0) does
    with pytest.raises(ValueError):
        hk.cone_affine_ds()


# ---- 7. determinism ------------------------------------------------------------------------------------------------------------------------

def test_every_operation_gives_the_same_bits_twice():
    with _Timeout(120):
        C = _case("side_96", False)
        a, b = _ops(C), _ops(C)
        for k in a:
            assert np.array_equal(a[k], b[k]), k


# ---- 8. end to end -------------------------------------------------------------------------------------------------------------------------

END_TO_END = {
    "one_psd_65": lambda: problems.sdp_blocks(n=40, ncones=1, dim=65, seed=7),
    "mixed_with_psd_65": lambda: tp._feasible_problem([T.NonnegativeConeT(3), T.PSDTriangleConeT(65), T.SecondOrderConeT(4),
                                                       T.PSDTriangleConeT(8), T.ZeroConeT(2)], 11),
}
_iteration_mismatches = []


@pytest.mark.parametrize("name", list(END_TO_END))
def test_ipm_with_the_large_psd_device_step_matches_the_host_cone_algebra(name, capsys):
    prob = END_TO_END[name]()
    with _Timeout(300):
        ref_solver = cl.Solver(*prob, cl.Settings(**STEP_FLAGS))
        ref_solver.trace = []
        ref = ref_solver.solve()
        dev_solver = cl.Solver(*prob, cl.Settings(**LARGE))
        assert dev_solver._device_step and dev_solver._device_step_psd and not ref_solver._device_step
        assert dev_solver.kktsystem.kktsolver.steps_psd_large
        dev_solver.trace = []
        got = dev_solver.solve()
    assert got.status == ref.status, (got.status, ref.status)
    assert ref.status == "SOLVED"
    assert abs(got.iterations - ref.iterations) <= 1
    if got.iterations != ref.iterations:      # cause: a step-length / termination test decided by digits below 1e-10
        k = min(got.iterations, ref.iterations)
        with capsys.disabled():
            print(f"\n[psd large device-step {name}] iterations {got.iterations} vs {ref.iterations}; at iteration {k}: "
                  f"device {dev_solver.trace[k]} host {ref_solver.trace[k]}")
        _iteration_mismatches.append(name)
        assert len(_iteration_mismatches) <= 1, _iteration_mismatches
        return
    print(f"[psd large device-step {name}] {got.status} in {got.iterations} iterations; |dobj| / max(1, |obj|) "
          f"{abs(got.obj_val - ref.obj_val) / max(1.0, abs(ref.obj_val)):.2e}, |d r_prim| {abs(got.r_prim - ref.r_prim):.2e}, "
          f"|d r_dual| {abs(got.r_dual - ref.r_dual):.2e}")
    assert abs(got.obj_val - ref.obj_val) <= PARITY * max(1.0, abs(ref.obj_val)), (got.obj_val, ref.obj_val)
    assert abs(got.r_prim - ref.r_prim) <= PARITY and abs(got.r_dual - ref.r_dual) <= PARITY
