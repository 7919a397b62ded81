"""The Nesterov-Todd scaling of PSD triangle cones of side 65 .. 128 on the GPU (scaling_psd_large.hip, hipkkt_psd_scaling_enable_large,
Settings.device_scaling_psd_large).

Two yardsticks, as in tests/test_gpu_psd_step_large.py.  (1) The kernel of scaling_psd_large.hip repeats the arithmetic of scaling_psd.hip
in another placement, every sum in the same order, so on a cone of side <= 64 (testing switch PSD_LARGE_MIN = 1 at the step enable) it
must give the bits of scaling_psd.hip: `np.array_equal` on R, Rinv, lambda, the resident K and affine_ds, no tolerance.  (2) On sides
65 .. 128 the gate of tests/test_gpu_psd_scaling.py: residuals 1 - 4 of tests/psd_scaling_reference.py `Reference` (50 digits) at most
max(8 x the host's error in the same case, 2 n) eps x scale, lambda > 0 and descending, and K bit for bit what a handle without the new
enable writes when it is handed the device's factors (the kernels that form K from R are the existing ones).  On early_0 and late_0 of
every side -- 65, 66, 96 and 128 -- the K block is also held, with the same rule, to the exact triu(skron(R R')) of the device's own R
(tests/psd_skron_sliced.py: the exact integer arithmetic of psd_scaling_reference.skron_error over slices of the 2.3 to 34 million
packed entries, so that memory stays bounded; the two evaluations of a case, device and host, take well under a minute at side 128).
Failures, the protocol, the step operations after a device scaling (the gate of tests/test_gpu_psd_step.py) and end-to-end solves with
their traffic follow.  No case is skipped or filtered; every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt, problems
from julia_standin.cones import SecondOrderCone
from tests import psd_scaling_reference as sr
from tests import psd_skron_sliced as sk
from tests import psd_step_reference as pr
from tests import test_gpu_psd_scaling as ts
from tests import test_gpu_psd_step as tp
from tests.step_support import STEP_FLAGS, _Timeout
from tests.test_gpu_psd_scaling import _hs_entries, _host_cone, _split

pytestmark = pytest.mark.gpu

LARGE = dict(device_step=True, device_step_psd=True, device_step_psd_large=True, **STEP_FLAGS)
LARGEN = dict(LARGE, device_scaling_psd=True, device_scaling_psd_large=True)
T = cl
K_GATE_POINTS = ("early_0", "late_0")      # the exact K block, at every side


def _mixed_large():
    return [T.NonnegativeConeT(3), T.PSDTriangleConeT(65), T.SecondOrderConeT(4), T.PSDTriangleConeT(8), T.ZeroConeT(2),
            T.PSDTriangleConeT(66)]


SETS = {"side_65": lambda: [T.PSDTriangleConeT(65)], "side_66": lambda: [T.PSDTriangleConeT(66)],
        "side_96": lambda: [T.PSDTriangleConeT(96)], "side_128": lambda: [T.PSDTriangleConeT(128)],
        "two_of_128": lambda: [T.PSDTriangleConeT(128), T.PSDTriangleConeT(128)], "mixed_large": _mixed_large}


@functools.lru_cache(maxsize=None)
def _pair(name):
    """(plugin with the new enable, plugin with the large PSD step only, cones) for one cone set, built once"""
    he, cones = tp._handle(SETS[name](), 3, LARGEN)
    hn, _ = tp._handle(SETS[name](), 3, LARGE)
    assert he.steps_psd and he.steps_psd_large and he.scales_psd and hn.steps_psd_large and not hn.scales_psd
    sides = [c.n for c in cones.cones if tp._is_psd(c)]
    assert list(he.h.debug_dump(24)) == [k for k, n in enumerate(sides) if n >= 65]      # the others stay with scaling_psd.hip
    return he, hn, cones


@functools.lru_cache(maxsize=None)
def _one(n, name):
    """(s, z, Reference, the host's residuals) of one point of the family of tests/psd_scaling_reference.py, computed once"""
    (s, z), = [(s, z) for nm, s, z in sr.points(n) if nm == name]
    ref = sr.Reference(n, s, z)
    return s, z, ref, ref.residuals(*sr.host_factors(n, s, z))


def _k_gate(what, n, R_dev, block_dev, s, z):
    """the K gate of tests/test_gpu_psd_scaling.py with the exact skron evaluated in slices: the device's block against the exact skron of
    its own R, the host's float64 skron(R R') against the exact one of its R, max(8 x host, 2 n) eps x skron(|R| |R|')"""
    K = _host_cone(n, s, z)
    hb = np.zeros(K.numel * (K.numel + 1) // 2)
    K.get_Hs(hb)
    rd, rh = sk.skron_error(R_dev, block_dev), sk.skron_error(K.R, hb)
    allowed = max(8.0 * rh, 2.0 * n)
    print(f"[psd scaling large] {what} n={n} K block: device {rd:.3f}, host {rh:.3f}, allowed {allowed:.1f} (eps x skron(|R| |R|'))")
    assert rd <= allowed, (what, n, rd, rh)


def _same_k_from_the_devices_factors(he, hn, cones, s, z, what):
    """the device's factors through the caller's path on the handle without the enable: the same K and affine_ds, bit for bit"""
    R, Ri, lam = he.h.psd_get_factors()
    hn.h.psd_set_factors(Ri, lam)
    assert hn.h.update_scaling(s, z, R)[0]
    assert np.array_equal(hn.h.debug_dump(4), he.h.debug_dump(4)), what
    assert np.array_equal(hn.cone_affine_ds(), he.cone_affine_ds()), what


def _check_single(name, n, case, s, z, ref, host, misses=None):
    he, hn, cones = _pair(name)
    ok, *_ = he.h.update_scaling(s, z, None)
    assert ok, (n, case)
    (R, Ri, lam), = _split(he, cones)
    assert np.all(lam > 0) and np.all(np.diff(lam) <= 0), (n, case, lam)
    res = ref.residuals(R, Ri, lam)
    res.pop(5, None)
    w = sr.gate(f"device {case}", n, res, host, misses)
    if case in K_GATE_POINTS:
        _k_gate(f"device {case}", n, R, -he.h.debug_dump(4)[_hs_entries(he, cones)[0]], s, z)
    _same_k_from_the_devices_factors(he, hn, cones, s, z, (n, case))
    return w


# ---- 1. the bits of the small path ------------------------------------------------------------------------------------------------------

BIT_SETS = {f"side_{n}": (lambda n=n: [T.PSDTriangleConeT(n)]) for n in (1, 2, 5, 32, 33, 63, 64)}
BIT_SETS["mixed"] = tp._mixed_specs
BIT_POINTS = ("early_0", "late_0", "identity", "n_fold", "two_fold")


def _pair_of_handles(specs, monkeypatch):
    """the same problem twice, both through hipkkt_step_enable_psd_large + hipkkt_psd_scaling_enable_large: on the first
    scaling_psd_large.hip computes every PSD cone (PSD_LARGE_MIN = 1, read at the step enable), on the second scaling_psd.hip"""
    monkeypatch.setenv("HIPKKT_PSD_LARGE_MIN", "1")
    hl, cones = tp._handle(specs, 3, flags={})
    hl.h.step_enable_psd_large(True)
    monkeypatch.delenv("HIPKKT_PSD_LARGE_MIN")
    hs, _ = tp._handle(specs, 3, flags={})
    hs.h.step_enable_psd_large(True)
    for hk in (hl, hs):
        hk.h.psd_scaling_enable_large(True)
    npsd = sum(tp._is_psd(c) for c in cones.cones)
    assert list(hl.h.debug_dump(24)) == list(range(npsd)) and hs.h.debug_dump(24).size == 0      # who computes which cone
    return hl, hs, cones


def _bit_points(cones):
    """name -> (s, z) of the whole set: one early and one late point, and the three edge cases in every PSD member"""
    out = {}
    for late in (False, True):
        out["late" if late else "early"] = tp._point(cones, np.random.default_rng(31 + late), late)
    s0, z0 = out["early"]
    for case in BIT_POINTS[2:]:
        s, z = s0.copy(), z0.copy()
        for c, r in zip(cones.cones, cones.rng_cones):
            if tp._is_psd(c):
                S, Z = sr.edge_cases(c.n, np.random.default_rng(7000 + c.n))[case]
                s[r], z[r] = c.mat_to_svec(S), c.mat_to_svec(Z)
        out[case] = (s, z)
    return out


@pytest.mark.parametrize("name", list(BIT_SETS))
def test_the_large_kernel_gives_the_bits_of_the_small_one(name, monkeypatch):
    with _Timeout(120):
        hl, hs, cones = _pair_of_handles(BIT_SETS[name](), monkeypatch)
        psd = [(c, r) for c, r in zip(cones.cones, cones.rng_cones) if tp._is_psd(c)]
        for case, (s, z) in _bit_points(cones).items():
            got = []
            for hk in (hl, hs):
                ok, *wle = hk.h.update_scaling(s, z, None)
                assert ok, (name, case)
                got.append((hk.h.psd_get_factors(), hk.h.debug_dump(4), hk.cone_affine_ds(), wle))
            (fl, Kl, al, wl), (fs, Ks, as_, ws_) = got
            print(f"[psd scaling large bits] {name} {case}: lambda_max {fl[2].max()!r} / {fs[2].max()!r}")
            for a, b, what in zip(fl, fs, ("R", "Rinv", "lambda")):
                assert np.array_equal(a, b), (name, case, what)
            assert np.array_equal(Kl, Ks) and np.array_equal(al, as_), (name, case)
            assert all(np.array_equal(a, b) for a, b in zip(wl, ws_)), (name, case)
            # equal results alone do not show which kernel ran: the large kernel leaves S = svec_to_mat(s) in matrix 0 of the cone's
            # workspace slot (debug_dump 25), and the second handle has no workspace
            assert hs.h.debug_dump(25).size == 0
            wsp = hl.h.debug_dump(25)
            assert wsp.size == len(psd) * 4 * 128 * 128
            for slot, (c, r) in enumerate(psd):
                S = wsp[4 * slot * 128 * 128:][:c.n * c.n].reshape((c.n, c.n), order="F")
                assert np.array_equal(S, c.svec_to_mat(s[r])), (name, case, slot)


# ---- 2. sides 65 .. 128 against 50 digits -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", sr.GROUPS)
def test_side_65_meets_the_gate_on_the_whole_family(group):
    """the smallest large side; odd, so the pairing has a dummy index"""
    with _Timeout(300):
        worst = max(_check_single("side_65", 65, case, s, z, ref, host) for case, s, z, ref, host in sr.cases(65, group))
    print(f"[psd scaling large] n=65 {group}: worst device / host ratio {worst:.2f}")


@pytest.mark.parametrize("n,case", [(66, "early_0"), (66, "late_0"), (96, "early_0"), (128, "early_0"), (128, "late_0"),
                                    (128, "S_equals_Z")])
def test_single_cones_meet_the_gate(n, case):
    """66: an even side; 96: side % 32 == 0, the padded leading dimension; 128: every lane and the LDS budget at the limit"""
    with _Timeout(300):
        w = _check_single(f"side_{n}", n, case, *_one(n, case))
    print(f"[psd scaling large] n={n} {case}: device / host ratio {w:.2f}")


def test_two_cones_of_side_128_use_their_own_workspace_slots():
    with _Timeout(300):
        he, hn, cones = _pair("two_of_128")
        s1, z1, ref1, host1 = _one(128, "early_0")
        s2, z2, ref2, host2 = _one(128, "late_0")
        s, z = np.concatenate([s1, s2]), np.concatenate([z1, z2])
        assert he.h.update_scaling(s, z, None)[0]
        fac = _split(he, cones)
        for k, (ref, host) in enumerate(((ref1, host1), (ref2, host2))):
            R, Ri, lam = fac[k]
            assert np.all(lam > 0) and np.all(np.diff(lam) <= 0)
            res = ref.residuals(R, Ri, lam)
            sr.gate(f"two_of_128 cone {k}", 128, res, host)
        _same_k_from_the_devices_factors(he, hn, cones, s, z, "two_of_128")
        # each cone alone on its own handle: the same bits (nothing of one slot reaches the other)
        h1, _, c1 = _pair("side_128")
        for k, (sk, zk) in enumerate(((s1, z1), (s2, z2))):
            assert h1.h.update_scaling(sk, zk, None)[0]
            assert all(np.array_equal(a, b) for a, b in zip(_split(h1, c1)[0], fac[k])), k


@pytest.mark.parametrize("late", [False, True])
def test_the_mixed_large_set_runs_both_kernels_in_one_call(late):
    with _Timeout(300):
        he, hn, cones = _pair("mixed_large")
        hs = _hs_entries(he, cones)
        s, z = tp._point(cones, np.random.default_rng(40 + late), late)
        ok, w, lam_v, eta = he.h.update_scaling(s, z, None)
        assert ok
        fac, Kd = _split(he, cones), he.h.debug_dump(4)
        misses, j = [], 0
        for k, (c, r) in enumerate(zip(cones.cones, cones.rng_cones)):
            if not tp._is_psd(c):
                continue
            R, Ri, lam = fac[j]
            j += 1
            assert np.all(lam > 0) and np.all(np.diff(lam) <= 0)
            ref = sr.Reference(c.n, s[r], z[r])
            dev, host = ref.residuals(R, Ri, lam), ref.residuals(c.R, c.Rinv, c.lam)
            dev.pop(5, None)
            sr.gate(f"mixed_large late={late} cone {k}", c.n, dev, host, misses)
        assert not misses, misses
        _same_k_from_the_devices_factors(he, hn, cones, s, z, "mixed_large")
        # a handle without the large cones: the rows of kinds 0 .. 2 and the PSD(8) cone bit for bit
        specs = [T.NonnegativeConeT(3), T.SecondOrderConeT(4), T.PSDTriangleConeT(8), T.ZeroConeT(2)]
        hsm, csm = tp._handle(specs, 3, dict(tp.PSD, device_scaling_psd=True))
        keep = [0, 2, 3, 4]
        s2, z2 = (np.concatenate([v[cones.rng_cones[k]] for k in keep]) for v in (s, z))
        ok, w2, lam2, eta2 = hsm.h.update_scaling(s2, z2, None)
        assert ok
        for k2, k in enumerate(keep):
            r, r2 = cones.rng_cones[k], csm.rng_cones[k2]
            assert np.array_equal(w[r], w2[r2]) and np.array_equal(lam_v[r], lam2[r2]), k
            assert np.array_equal(Kd[hs[k]], hsm.h.debug_dump(4)[_hs_entries(hsm, csm)[k2]]), k
        assert np.array_equal(eta, eta2)
        assert all(np.array_equal(a, b) for a, b in zip(fac[1], _split(hsm, csm)[0]))      # PSD(8): scaling_psd.hip on both


# ---- failures: ordinary inputs the reference rejects too --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["side_65", "mixed_large"])
def test_a_large_cone_that_cannot_be_scaled_fails_alone(name):
    with _Timeout(300):
        he, hn, cones = _pair(name)
        hs = _hs_entries(he, cones)
        s, z = tp._point(cones, np.random.default_rng(61), False)
        assert he.h.update_scaling(s, z, None)[0]
        good, K_good = _split(he, cones), he.h.debug_dump(4)
        psd = [k for k, c in enumerate(cones.cones) if tp._is_psd(c)]
        kb = psd[0]                                            # the PSD(65) cone: the only one, or one among good ones
        cb, rb = cones.cones[kb], cones.rng_cones[kb]
        assert cb.n == 65
        for what, (sb, zb) in ts._bad_inputs(cb, s[rb], z[rb]).items():
            s2, z2 = s.copy(), z.copy()
            s2[rb], z2[rb] = sb, zb
            if what != "a NaN in s":
                assert not cb.update_scaling(sb, zb, 1.0)       # the reference rejects it too
            runs = []
            for _ in range(2):                                  # the same (s, z) twice: the same bits
                ok, *_ = he.h.update_scaling(s2, z2, None)      # HIPKKT_OK: no exception
                assert not ok
                runs.append((_split(he, cones), he.h.debug_dump(4)))
            print(f"[psd scaling large] {name}, {what} in cone {kb}: scaling_ok = {ok}")
            (fac, Kb), (fac2, Kb2) = runs
            assert np.array_equal(Kb, Kb2)
            for j, k in enumerate(psd):
                if k == kb:
                    assert all(np.all(np.isnan(a)) for a in fac[j]) and all(np.all(np.isnan(a)) for a in fac2[j])
                else:
                    assert all(np.array_equal(a, b) for a, b in zip(fac[j], good[j]))
                    assert all(np.array_equal(a, b) for a, b in zip(fac2[j], good[j]))
            assert np.array_equal(Kb[hs[kb]], K_good[hs[kb]])  # no K entry of the failed cone was written
            keep = np.ones(len(Kb), dtype=bool)
            keep[hs[kb]] = False
            assert np.array_equal(Kb[keep], K_good[keep])       # and the good cones got what they get without it
            with pytest.raises(ValueError):
                he.cone_affine_ds()                             # a failed scaling leaves no step
            assert he.h.update_scaling(s, z, None)[0]
            assert np.array_equal(he.h.debug_dump(4), K_good)
            assert all(np.array_equal(a, b) for f, g in zip(_split(he, cones), good) for a, b in zip(f, g))


# ---- the protocol ------------------------------------------------------------------------------------------------------------------------

def test_protocol_of_the_new_enable():
    with _Timeout(120):
        # refused without hipkkt_step_enable_psd_large: no enable at all, the small enable, a Mixed handle, a side of 129
        free, _ = tp._handle([T.PSDTriangleConeT(8), T.NonnegativeConeT(2)], 1, flags={})
        with pytest.raises(ValueError, match="psd_scaling_enable_large"):
            free.h.psd_scaling_enable_large(True)
        free.h.step_enable_psd(True)
        with pytest.raises(ValueError, match="psd_scaling_enable_large"):
            free.h.psd_scaling_enable_large(True)
        mixed, _ = tp._handle([T.PSDTriangleConeT(3), T.ExponentialConeT()], 1, flags={})
        mixed.h.step_enable_mixed(True, 0.8, 1e-4)
        with pytest.raises(ValueError, match="psd_scaling_enable_large"):
            mixed.h.psd_scaling_enable_large(True)
        big, _ = tp._handle([T.PSDTriangleConeT(129)], 1, flags={})
        with pytest.raises(ValueError, match="step_enable_psd_large"):
            big.h.step_enable_psd_large(True)
        with pytest.raises(ValueError, match="psd_scaling_enable_large"):
            big.h.psd_scaling_enable_large(True)
        # a plugin asked for everything but the new flags keeps the factors with the caller, as before
        hk, cones = tp._handle([T.PSDTriangleConeT(65), T.NonnegativeConeT(3)], 2, flags=dict(LARGE, device_scaling_psd=True))
        assert hk.steps_psd_large and not hk.scales_psd
        with pytest.raises(ValueError, match="psd_scaling_enable"):
            hk.h.psd_scaling_enable(True)                       # the old enable still refuses the large handle
        s, z = tp._point(cones, np.random.default_rng(5), False)
        with pytest.raises(hipkkt.HipKKTError, match="psd_set_factors"):
            hk.h.update_scaling(s, z, None)
        hk.h.psd_scaling_enable_large(True)
        assert hk.h.update_scaling(s, z, None)[0]
        first, fac = hk.cone_affine_ds(), hk.h.psd_get_factors()
        # the caller-supplied path on the enabled handle is today's: the factors come back as they went in
        R = np.concatenate([c.R.ravel(order="F") for c in cones.cones if tp._is_psd(c)])
        rinv, lam = hk._psd_factors()
        hk.h.psd_set_factors(rinv, lam)
        assert hk.h.update_scaling(s, z, R)[0]
        Rg, Rinvg, lamg = hk.h.psd_get_factors()
        assert np.array_equal(Rg, R) and np.array_equal(Rinvg, rinv) and np.array_equal(lamg, lam)
        with pytest.raises(hipkkt.HipKKTError, match="psd_set_factors"):
            hk.h.update_scaling(s, z, R)                        # psd_R without staged factors
        # switching off invalidates the resident scaling and restores the refusal of a scaling without psd_R
        assert hk.h.update_scaling(s, z, None)[0]
        hk.h.psd_scaling_enable_large(False)
        with pytest.raises(ValueError):
            hk.cone_affine_ds()
        with pytest.raises(ValueError):
            hk.h.psd_get_factors()
        with pytest.raises(hipkkt.HipKKTError, match="psd_set_factors"):
            hk.h.update_scaling(s, z, None)
        hk.h.psd_scaling_enable_large(True)
        with pytest.raises(ValueError):
            hk.cone_affine_ds()                                 # enabling invalidates as well
        assert hk.h.update_scaling(s, z, None)[0]
        assert np.array_equal(hk.cone_affine_ds(), first)       # the same bits on every run
        assert all(np.array_equal(a, b) for a, b in zip(hk.h.psd_get_factors(), fac))
        # the step enable and a new registration clear it
        hk.h.step_enable_psd_large(True)
        with pytest.raises(hipkkt.HipKKTError, match="psd_set_factors"):
            hk.h.update_scaling(s, z, None)
        hk.h.psd_scaling_enable_large(True)
        hk.h.set_cone_types(cones.kkt_cone_kinds())
        with pytest.raises(ValueError, match="psd_scaling_enable_large"):
            hk.h.psd_scaling_enable_large(True)


# ---- the step operations compose -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["side_65", "mixed_large"])
def test_step_operations_after_a_device_scaling_match_the_reference(name):
    """the five operations against the 50-digit step reference fed the device's own factors, with the gates of
    tests/test_gpu_psd_step.py (the body of the test of that name in tests/test_gpu_psd_scaling.py, on the handles of this file)"""
    with _Timeout(300):
        he, hn, cones = _pair(name)
        rng = np.random.default_rng(83)
        s, z = tp._point(cones, rng, False)
        ok, w, lam_v, eta = he.h.update_scaling(s, z, None)
        assert ok
        fac = _split(he, cones)
        # host cones on the device's factors: what the stand-in computes from the same (R, Rinv, lambda)
        j, q = 0, 0
        for c, r in zip(cones.cones, cones.rng_cones):
            if tp._is_psd(c):
                c.R[:], c.Rinv[:], c.lam[:] = fac[j]
                c.lisqrt[:] = 1.0 / np.sqrt(c.lam)
                j += 1
            elif isinstance(c, SecondOrderCone):
                c.adopt_symmetric_scaling(w[r], lam_v[r], eta[q])
                q += 1
        m = cones.numel
        dz = np.concatenate([pr.direction(c, rng, z[r]) if tp._is_psd(c) else 0.5 * z[r] for c, r in zip(cones.cones, cones.rng_cones)])
        ds = np.concatenate([pr.direction(c, rng, s[r]) if tp._is_psd(c) else 0.5 * s[r] for c, r in zip(cones.cones, cones.rng_cones)])
        sm = 0.37
        got = {"mul_Hs": he.cone_mul_hs(dz), "combined_ds_shift": he.cone_combined_ds_shift(dz, ds, sm),
               "ds_from_dz_offset": he.cone_ds_from_dz_offset(ds)}
        host = {k: np.zeros(m) for k in got}
        cones.mul_Hs(host["mul_Hs"], dz, np.zeros(m))
        cones.combined_ds_shift(host["combined_ds_shift"], dz.copy(), ds.copy(), sm)
        cones.ds_from_dz_offset(host["ds_from_dz_offset"], ds, np.zeros(m), z)
        psd = [(k, c, r) for k, (c, r) in enumerate(zip(cones.cones, cones.rng_cones)) if tp._is_psd(c)]
        for k, c, r in psd:
            refs = {"mul_Hs": pr.ref_mul_hs(c.R, dz[r]), "combined_ds_shift": pr.ref_shift(c.R, c.Rinv, dz[r], ds[r], sm),
                    "ds_from_dz_offset": pr.ref_offset(c.R, c.lam, ds[r])}
            for op, (ref, scale) in refs.items():
                tp._gate(f"{name} after the device scaling, cone {k} {op}", c.n, got[op][r], host[op][r], ref, scale)
        # step length: one PSD cone binds at a time (the others and the kinds 0..2 move inward), each held to the reference's alpha
        for k, c, r in psd:
            dz1, ds1 = 0.5 * z, 0.25 * s
            dz1[r] = -2.5 * z[r] + 0.05 * pr.direction(c, rng, z[r])
            ds1[r] = -3.5 * s[r] + 0.05 * pr.direction(c, rng, s[r])
            az, as_ = he.cone_step_length(dz1, ds1, 1.0)
            hz, hs_ = c.step_length(dz1[r], ds1[r], z[r], s[r], 1.0)
            (a_z, a_s), gam, nrm = pr.ref_step_length(c.R, c.Rinv, c.lam, dz1[r], ds1[r], 1.0)
            assert a_z < 1 and a_s < 1
            tp._alpha_gate(f"{name} after the device scaling, binding cone {k} z", c.n, az, hz, a_z, gam[0], nrm[0])
            tp._alpha_gate(f"{name} after the device scaling, binding cone {k} s", c.n, as_, hs_, a_s, gam[1], nrm[1])


# ---- end to end, with the traffic of every iteration ---------------------------------------------------------------------------------------

END_TO_END = {
    "one_psd_65": lambda: problems.sdp_blocks(n=40, ncones=1, dim=65, seed=7),
    "mixed_with_psd_65": lambda: tp._feasible_problem([T.NonnegativeConeT(3), T.PSDTriangleConeT(65), T.SecondOrderConeT(4),
                                                       T.PSDTriangleConeT(8), T.ZeroConeT(2)], 11),
}
PATHS = {"scaling": dict(device_scaling_psd=True, device_scaling_psd_large=True),
         "start": dict(device_default_start=True, device_default_start_psd_large=True),
         "both": dict(device_scaling_psd=True, device_scaling_psd_large=True, device_default_start=True,
                      device_default_start_psd_large=True)}


@functools.lru_cache(maxsize=None)
def _baseline(name):
    """the solve with the large PSD step alone (the flags of the parent): shared by the three paths"""
    S = cl.Solver(*END_TO_END[name](), cl.Settings(**LARGE))
    assert S._device_step and S._device_step_psd and not S._device_scaling_psd and not S._device_default_start
    S.trace = ts._Trace()
    t0 = dict(hipkkt.TRAFFIC)
    return S, S.solve(), t0, {k: hipkkt.TRAFFIC[k] - t0[k] for k in t0}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(END_TO_END))
def test_ipm_with_the_new_flags_matches_the_solve_without_them(name, path):
    with _Timeout(300):
        S0, off, start0, total0 = _baseline(name)
        S1 = cl.Solver(*END_TO_END[name](), cl.Settings(**dict(LARGE, **PATHS[path])))
        scaling, start = path != "start", path != "scaling"
        assert S1._device_step and S1._device_step_psd and S1._device_scaling_psd == scaling and S1._device_default_start == start
        S1.trace = ts._Trace()
        t0 = dict(hipkkt.TRAFFIC)
        on = S1.solve()
        total1 = {k: hipkkt.TRAFFIC[k] - t0[k] for k in t0}
    st = S1.settings
    tol = 2.0 * max(st.tol_gap_abs, st.tol_gap_rel * max(1.0, abs(off.obj_val)))
    print(f"[psd scaling large {name} {path}] {on.status} in {on.iterations} iterations (without the flags: {off.status} in "
          f"{off.iterations}); |dobj| {abs(on.obj_val - off.obj_val):.2e}, allowed {tol:.2e}; whole solve host -> device "
          f"{total1['h2d_bytes']} B (without: {total0['h2d_bytes']} B), device -> host {total1['d2h_bytes']} B (without: "
          f"{total0['d2h_bytes']} B)")
    assert on.status == off.status == "SOLVED"
    assert abs(on.iterations - off.iterations) <= 1             # (what the existing PSD end-to-end tests allow)
    assert abs(on.obj_val - off.obj_val) <= tol
    sides = [c.n for c in S1.cones.cones if tp._is_psd(c)]
    lo, hi = S1.kktsystem.kktsolver._psd_span
    up, down = 8 * sum(2 * n * n + n for n in sides), 8 * 2 * (hi - lo)
    for k in range(min(on.iterations, off.iterations)):
        d_up = (S0.trace[k + 1]["h2d"] - S0.trace[k]["h2d"]) - (S1.trace[k + 1]["h2d"] - S1.trace[k]["h2d"])
        d_down = (S0.trace[k + 1]["d2h"] - S0.trace[k]["d2h"]) - (S1.trace[k + 1]["d2h"] - S1.trace[k]["d2h"])
        if k == 0:
            print(f"[psd scaling large {name} {path}] iteration 0: host -> device {S1.trace[1]['h2d'] - S1.trace[0]['h2d']} B ({d_up} B "
                  f"fewer, the factors are {up} B), device -> host {S1.trace[1]['d2h'] - S1.trace[0]['d2h']} B ({d_down} B fewer, the "
                  f"PSD rows of (s, z) are {down} B)")
        # derived, not tuned: exactly the factors no longer go up and exactly the PSD rows no longer come down -- or nothing changes
        assert (d_up, d_down) == ((up, down) if scaling else (0, 0)), (name, path, k, d_up, up, d_down, down)
    if start:
        # the start's uploads are gone from the solve's total: the Hs vector of the identity scaling (nHs doubles) and the iterate
        ks = S1.kktsystem.kktsolver
        before0, before1 = S0.trace[0]["h2d"] - start0["h2d_bytes"], S1.trace[0]["h2d"] - t0["h2d_bytes"]
        print(f"[psd scaling large {name} {path}] before the first iteration: host -> device {before1} B (without: {before0} B; "
              f"Hs is {8 * ks.h.nHs} B, the iterate {8 * (S1.data.n + 2 * S1.data.m)} B)")
        assert before0 - before1 >= 8 * ks.h.nHs + 8 * (S1.data.n + 2 * S1.data.m)
        assert total0["h2d_bytes"] - total1["h2d_bytes"] >= 8 * ks.h.nHs
