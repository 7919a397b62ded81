"""The Nesterov-Todd scaling of PSD triangle cones on the GPU (scaling_psd.hip, hipkkt_psd_scaling_enable / hipkkt_psd_get_factors,
Settings.device_scaling_psd) against the 50-digit residuals of tests/psd_scaling_reference.py.

R is unique only up to column signs and, among equal singular values, rotations: nothing compares R with the host's R entry by entry.
Per case the five residuals of the device's (R, Rinv, lambda) -- R' Z R - Lambda, Rinv S Rinv' - Lambda, Rinv R - I, W Z W - S and
lambda against sqrt(eigsy(L1' Z L1)) at n <= 17 -- are measured in units of eps x scale and must be at most
    max(8 x the host's error in the same case, 2 n),
the host being the stand-in's PSDTriangleCone.update_scaling (LAPACK potrf / gesdd) on the same float64 (s, z).  The PSD block of the
resident K is held, with the same rule, to triu(skron(W)) of the exact W = R R' of the device's own R (W itself is pinned by residual
4), the host's figure being its float64 skron(R R') against the exact one of its R; that comparison runs on every point at n <= 33
and, at n = 63 and 64 (2.1 million exact entries, two seconds per evaluation), on the first early and the first late point.  On every
point of every side the block must also be, bit for bit, what a handle without the enable writes when it is handed the device's
factors: the kernels that form K from R are the existing ones.  Step operations after a device scaling pass the gate of
tests/test_gpu_psd_step.py against the 50-digit step reference fed the device's own factors.  End to end: the solver's own tolerances.
No case is skipped or filtered.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt
from julia_standin.cones import PSDTriangleCone, SecondOrderCone
from tests import psd_scaling_reference as sr
from tests import psd_step_reference as pr
from tests.step_support import _Timeout
from tests.test_gpu_psd_step import END_TO_END, PSD, SETS, _alpha_gate, _gate, _handle, _is_psd, _point

pytestmark = pytest.mark.gpu

PSDN = dict(PSD, device_scaling_psd=True)
T = cl
SETS = dict(SETS, **{f"side_{n}": (lambda n=n: [T.PSDTriangleConeT(n)]) for n in sr.SIDES})
K_GATE_MAX_N = 33                       # the exact K block on every point up to this side ...
K_GATE_LARGE = ("early_0", "late_0")    # ... and on these points above it
_handles = {}


def _pair(name, seed=3):
    """(enabled plugin, plugin with the PSD step only, cones) for one cone set, built once"""
    if name not in _handles:
        he, cones = _handle(SETS[name](), seed, PSDN)
        hn, _ = _handle(SETS[name](), seed, PSD)
        assert he.steps_psd and he.scales_psd and hn.steps_psd and not hn.scales_psd
        _handles[name] = (he, hn, cones)
    return _handles[name]


def _split(hk, cones):
    """[(R, Rinv, lambda)] per PSD cone from hipkkt_psd_get_factors"""
    R, Ri, lam = hk.h.psd_get_factors()
    out, fo, lo = [], 0, 0
    for c in cones.cones:
        if _is_psd(c):
            n = c.n
            out.append((R[fo:fo + n * n].reshape(n, n, order="F").copy(), Ri[fo:fo + n * n].reshape(n, n, order="F").copy(), lam[lo:lo + n].copy()))
            fo, lo = fo + n * n, lo + n
    return out


def _hs_entries(hk, cones):
    """per cone the indices of its Hs block in the value array of K (debug_dump 4)"""
    mp = hk.h.map(2)
    return [mp[r] for r in cones.rng_blocks]


def _host_cone(n, s, z):
    K = PSDTriangleCone(n)
    assert K.update_scaling(s, z, 1.0)
    return K


def _k_gate(what, n, R_dev, block_dev, s, z):
    K = _host_cone(n, s, z)
    hb = np.zeros(K.numel * (K.numel + 1) // 2)
    K.get_Hs(hb)
    rd, rh = sr.skron_error(R_dev, block_dev), sr.skron_error(K.R, hb)
    allowed = max(8.0 * rh, 2.0 * n)
    print(f"[psd scaling] {what} n={n} K block: device {rd:.3f}, host {rh:.3f}, allowed {allowed:.1f} (eps x skron(|R| |R|'))")
    assert rd <= allowed, (what, n, rd, rh)


# ---- single cones: every side, early / late / edge points -------------------------------------------------------------------------------

_worst = {}


@pytest.mark.parametrize("group", sr.GROUPS)
@pytest.mark.parametrize("n", sr.SIDES)
def test_single_cone_factors_meet_the_gate(n, group):
    with _Timeout(120):
        he, hn, cones = _pair(f"side_{n}")
        hs = _hs_entries(he, cones)[0]
        for case, s, z, ref, host in sr.cases(n, group):
            ok, *_ = he.h.update_scaling(s, z, None)
            assert ok, (n, case)
            (R, Ri, lam), = _split(he, cones)
            assert np.all(lam > 0) and np.all(np.diff(lam) <= 0), (n, case, lam)
            w = sr.gate(f"device {case}", n, ref.residuals(R, Ri, lam), host)
            _worst[n] = max(_worst.get(n, 0.0), w)
            Kd = he.h.debug_dump(4)
            if n <= K_GATE_MAX_N or case in K_GATE_LARGE:
                _k_gate(f"device {case}", n, R, -Kd[hs], s, z)
            # the same factors through the caller's path on a handle without the enable: the same K, bit for bit
            hn.h.psd_set_factors(Ri.ravel(order="F"), lam)
            assert hn.h.update_scaling(s, z, R.ravel(order="F"))[0]
            assert np.array_equal(hn.h.debug_dump(4), Kd), (n, case)
            assert np.array_equal(hn.cone_affine_ds(), he.cone_affine_ds())
    print(f"[psd scaling] n={n} {group}: worst device / host ratio so far {_worst[n]:.2f}")


# ---- several cones: table offsets, the other kinds' rows ----------------------------------------------------------------------------------

@pytest.mark.parametrize("late", [False, True])
@pytest.mark.parametrize("name", ["mixed", "twenty_of_5"])
def test_cone_sets_meet_the_gate_and_leave_the_other_kinds_alone(name, late):
    with _Timeout(120):
        he, hn, cones = _pair(name)
        hs = _hs_entries(he, cones)
        misses = []
        for seed in sr.SEEDS:
            s, z = _point(cones, np.random.default_rng(40 + seed), late)
            ok, w, lam_v, eta = he.h.update_scaling(s, z, None)
            assert ok
            fac = _split(he, cones)
            Kd = he.h.debug_dump(4)
            j = 0
            for k, (c, r) in enumerate(zip(cones.cones, cones.rng_cones)):
                if not _is_psd(c):
                    continue
                R, Ri, lam = fac[j]
                j += 1
                assert np.all(lam > 0) and np.all(np.diff(lam) <= 0)
                ref = sr.Reference(c.n, s[r], z[r])
                sr.gate(f"{name} late={late} seed {seed} cone {k}", c.n, ref.residuals(R, Ri, lam), ref.residuals(c.R, c.Rinv, c.lam),
                        misses)
                _k_gate(f"{name} late={late} seed {seed} cone {k}", c.n, R, -Kd[hs[k]], s[r], z[r])
            # the caller's path with the host's factors on the other handle: rows and K entries of kinds 0..2 bit for bit
            hn.h.psd_set_factors(*he._psd_factors())             # (the host cones that _point has just scaled are the enabled plugin's)
            ok, w0, lam0, eta0 = hn.h.update_scaling(s, z, np.concatenate([c.R.ravel(order="F") for c in cones.cones if _is_psd(c)]))
            assert ok
            K0 = hn.h.debug_dump(4)
            assert np.array_equal(w, w0) and np.array_equal(lam_v, lam0) and np.array_equal(eta, eta0)
            other = np.ones(len(K0), dtype=bool)
            for k, c in enumerate(cones.cones):
                if _is_psd(c):
                    other[hs[k]] = False
            assert np.array_equal(Kd[other], K0[other])
        assert not misses, misses


# ---- failures: ordinary inputs the reference rejects too ---------------------------------------------------------------------------------

def _bad_inputs(c, s, z):
    Zi = c.svec_to_mat(z).copy()
    Zi[0, 0] = -abs(Zi[0, 0])
    nan_s = s.copy()
    nan_s[len(s) // 2] = np.nan
    return {"S = 0": (np.zeros_like(s), z), "Z indefinite": (s, c.mat_to_svec(Zi)), "a NaN in s": (nan_s, z)}


@pytest.mark.parametrize("name", ["side_5", "side_33", "mixed"])
def test_a_cone_that_cannot_be_scaled_fails_alone(name):
    with _Timeout(60):
        he, hn, cones = _pair(name)
        hs = _hs_entries(he, cones)
        s, z = _point(cones, np.random.default_rng(61), False)
        assert he.h.update_scaling(s, z, None)[0]
        good, K_good = _split(he, cones), he.h.debug_dump(4)
        psd = [k for k, c in enumerate(cones.cones) if _is_psd(c)]
        kb = psd[len(psd) // 2]                                # the bad cone: the only one, or one among good ones
        cb, rb = cones.cones[kb], cones.rng_cones[kb]
        for what, (sb, zb) in _bad_inputs(cb, s[rb], z[rb]).items():
            s2, z2 = s.copy(), z.copy()
            s2[rb], z2[rb] = sb, zb
            if what != "a NaN in s":
                assert not cb.update_scaling(sb, zb, 1.0)       # the reference rejects it too
            ok, *_ = he.h.update_scaling(s2, z2, None)          # HIPKKT_OK: no exception
            print(f"[psd scaling] {name}, {what} in cone {kb}: scaling_ok = {ok}")
            assert not ok
            fac, Kb = _split(he, cones), he.h.debug_dump(4)
            for j, k in enumerate(psd):
                if k == kb:
                    assert all(np.all(np.isnan(a)) for a in fac[j])
                else:
                    assert all(np.array_equal(a, b) for a, b in zip(fac[j], good[j]))
            assert np.array_equal(Kb[hs[kb]], K_good[hs[kb]])  # no K entry of the failed cone was written
            keep = np.ones(len(Kb), dtype=bool)
            keep[hs[kb]] = False
            assert np.array_equal(Kb[keep], K_good[keep])       # and the good cones got what they get without it
            with pytest.raises(ValueError):
                he.cone_affine_ds()                             # a failed scaling leaves no step
            assert he.h.update_scaling(s, z, None)[0]
            assert np.array_equal(he.h.debug_dump(4), K_good)


# ---- the protocol -------------------------------------------------------------------------------------------------------------------------

def test_protocol_of_the_enable_and_the_caller_supplied_path():
    with _Timeout(60):
        he, hn, cones = _pair("mixed")
        s, z = _point(cones, np.random.default_rng(71), False)
        R = np.concatenate([c.R.ravel(order="F") for c in cones.cones if _is_psd(c)])
        rinv, lam = he._psd_factors()
        # the caller-supplied path on an enabled handle equals a handle without the enable, bit for bit
        outs = []
        for hk in (he, hn):
            hk.h.psd_set_factors(rinv, lam)
            ok, *wle = hk.h.update_scaling(s, z, R)
            assert ok
            x = np.linspace(-1.0, 1.0, cones.numel)
            outs.append((hk.h.debug_dump(4), wle, hk.cone_affine_ds(), hk.cone_mul_hs(x), hk.h.psd_get_factors()))
        for a, b in zip(outs[0][1:], outs[1][1:]):
            assert all(np.array_equal(p, q) for p, q in zip(a, b)) if isinstance(a, (list, tuple)) else np.array_equal(a, b)
        assert np.array_equal(outs[0][0], outs[1][0])
        assert np.array_equal(outs[0][4][0], R) and np.array_equal(outs[0][4][1], rinv) and np.array_equal(outs[0][4][2], lam)
        # mixed forms keep today's refusal; a handle without the enable refuses a scaling without psd_R
        with pytest.raises(hipkkt.HipKKTError, match="psd_set_factors"):
            he.h.update_scaling(s, z, R)                        # psd_R without staged factors
        he.h.psd_set_factors(rinv, lam)
        with pytest.raises(hipkkt.HipKKTError):
            he.h.update_scaling(s, z, None)                     # staged factors without psd_R
        with pytest.raises(ValueError):
            he.h.psd_get_factors()                              # the refused call left no scaling
        assert he.h.update_scaling(s, z, R)[0]
        with pytest.raises(hipkkt.HipKKTError, match="psd_set_factors"):
            hn.h.update_scaling(s, z, None)
        # enabling / disabling invalidates the resident scaling; the enable needs the PSD step mode
        assert he.h.update_scaling(s, z, None)[0]
        first = he.cone_affine_ds()
        he.h.psd_scaling_enable(False)
        with pytest.raises(ValueError):
            he.cone_affine_ds()
        with pytest.raises(ValueError):
            he.h.psd_get_factors()
        with pytest.raises(hipkkt.HipKKTError):
            he.h.update_scaling(s, z, None)
        he.h.psd_scaling_enable(True)
        assert he.h.update_scaling(s, z, None)[0]
        assert np.array_equal(he.cone_affine_ds(), first)       # the same bits on every run
        free, _ = _handle([T.NonnegativeConeT(3), T.SecondOrderConeT(4)], 1, flags={})
        with pytest.raises(ValueError, match="psd_scaling_enable"):
            free.h.psd_scaling_enable(True)
        he.h.step_enable_psd(False)
        with pytest.raises(ValueError, match="psd_scaling_enable"):
            he.h.psd_scaling_enable(True)
        he.h.step_enable_psd(True)                              # (back to what _pair hands out)
        he.h.psd_scaling_enable(True)
        assert he.h.update_scaling(s, z, None)[0]
        assert np.array_equal(he.cone_affine_ds(), first)


# ---- the step operations compose ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed", "side_33"])
def test_step_operations_after_a_device_scaling_match_the_reference(name):
    with _Timeout(120):
        he, hn, cones = _pair(name)
        rng = np.random.default_rng(83)
        s, z = _point(cones, rng, False)
        ok, w, lam_v, eta = he.h.update_scaling(s, z, None)
        assert ok
        fac = _split(he, cones)
        # host cones on the device's factors: what the stand-in computes from the same (R, Rinv, lambda)
        j, q = 0, 0
        for c, r in zip(cones.cones, cones.rng_cones):
            if _is_psd(c):
                c.R[:], c.Rinv[:], c.lam[:] = fac[j]
                c.lisqrt[:] = 1.0 / np.sqrt(c.lam)
                j += 1
            elif isinstance(c, SecondOrderCone):
                c.adopt_symmetric_scaling(w[r], lam_v[r], eta[q])
                q += 1
        m = cones.numel
        dz = np.concatenate([pr.direction(c, rng, z[r]) if _is_psd(c) else 0.5 * z[r] for c, r in zip(cones.cones, cones.rng_cones)])
        ds = np.concatenate([pr.direction(c, rng, s[r]) if _is_psd(c) else 0.5 * s[r] for c, r in zip(cones.cones, cones.rng_cones)])
        sm = 0.37
        got = {"mul_Hs": he.cone_mul_hs(dz), "combined_ds_shift": he.cone_combined_ds_shift(dz, ds, sm),
               "ds_from_dz_offset": he.cone_ds_from_dz_offset(ds)}
        host = {k: np.zeros(m) for k in got}
        cones.mul_Hs(host["mul_Hs"], dz, np.zeros(m))
        cones.combined_ds_shift(host["combined_ds_shift"], dz.copy(), ds.copy(), sm)
        cones.ds_from_dz_offset(host["ds_from_dz_offset"], ds, np.zeros(m), z)
        psd = [(k, c, r) for k, (c, r) in enumerate(zip(cones.cones, cones.rng_cones)) if _is_psd(c)]
        for k, c, r in psd:
            refs = {"mul_Hs": pr.ref_mul_hs(c.R, dz[r]), "combined_ds_shift": pr.ref_shift(c.R, c.Rinv, dz[r], ds[r], sm),
                    "ds_from_dz_offset": pr.ref_offset(c.R, c.lam, ds[r])}
            for op, (ref, scale) in refs.items():
                _gate(f"{name} after the device scaling, cone {k} {op}", c.n, got[op][r], host[op][r], ref, scale)
        # step length: one PSD cone binds at a time (the others and the kinds 0..2 move inward), each held to the reference's alpha
        for k, c, r in psd:
            dz1, ds1 = 0.5 * z, 0.25 * s
            dz1[r] = -2.5 * z[r] + 0.05 * pr.direction(c, rng, z[r])
            ds1[r] = -3.5 * s[r] + 0.05 * pr.direction(c, rng, s[r])
            az, as_ = he.cone_step_length(dz1, ds1, 1.0)
            hz, hs_ = c.step_length(dz1[r], ds1[r], z[r], s[r], 1.0)
            (a_z, a_s), gam, nrm = pr.ref_step_length(c.R, c.Rinv, c.lam, dz1[r], ds1[r], 1.0)
            assert a_z < 1 and a_s < 1
            _alpha_gate(f"{name} after the device scaling, binding cone {k} z", c.n, az, hz, a_z, gam[0], nrm[0])
            _alpha_gate(f"{name} after the device scaling, binding cone {k} s", c.n, as_, hs_, a_s, gam[1], nrm[1])


# ---- end to end, with the traffic of every iteration ---------------------------------------------------------------------------------------

class _Trace(list):
    """the solver's per-iteration records, each with the bytes that had crossed PCIe when the iteration began"""

    def append(self, rec):
        super().append(dict(rec, h2d=hipkkt.TRAFFIC["h2d_bytes"], d2h=hipkkt.TRAFFIC["d2h_bytes"]))


@pytest.mark.parametrize("name", list(END_TO_END))
def test_ipm_with_the_device_scaling_matches_the_caller_side_scaling(name):
    prob = END_TO_END[name]()
    with _Timeout(120):
        runs = []
        for flags in (PSD, PSDN):
            S = cl.Solver(*prob, cl.Settings(**flags))
            assert S._device_step and S._device_step_psd and S._device_scaling_psd == (flags is PSDN)
            S.trace = _Trace()
            runs.append((S, S.solve()))
    (S0, off), (S1, on) = runs
    st = S1.settings
    tol = 2.0 * max(st.tol_gap_abs, st.tol_gap_rel * max(1.0, abs(off.obj_val)))
    print(f"[psd scaling {name}] {on.status} in {on.iterations} iterations (caller-side scaling: {off.status} in {off.iterations}); "
          f"|dobj| {abs(on.obj_val - off.obj_val):.2e}, allowed {tol:.2e}")
    assert on.status == off.status == "SOLVED"
    assert abs(on.iterations - off.iterations) <= 1
    assert abs(on.obj_val - off.obj_val) <= tol
    # per iteration: no factors go up, no PSD rows come down
    sides = [c.n for c in S1.cones.cones if _is_psd(c)]
    lo, hi = S1.kktsystem.kktsolver._psd_span
    up, down = 8 * sum(2 * n * n + n for n in sides), 8 * 2 * (hi - lo)
    for k in range(min(on.iterations, off.iterations)):
        d_up = (S0.trace[k + 1]["h2d"] - S0.trace[k]["h2d"]) - (S1.trace[k + 1]["h2d"] - S1.trace[k]["h2d"])
        d_down = (S0.trace[k + 1]["d2h"] - S0.trace[k]["d2h"]) - (S1.trace[k + 1]["d2h"] - S1.trace[k]["d2h"])
        if k == 0:
            print(f"[psd scaling {name}] iteration 0: host -> device {S1.trace[1]['h2d'] - S1.trace[0]['h2d']} B "
                  f"({d_up} B fewer, the factors are {up} B), device -> host {S1.trace[1]['d2h'] - S1.trace[0]['d2h']} B "
                  f"({d_down} B fewer, the PSD rows of (s, z) are {down} B)")
        assert d_up >= up and d_down >= down, (name, k, d_up, up, d_down, down)
