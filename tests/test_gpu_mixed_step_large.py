"""The device-resident interior-point step for PSD triangle cones of side 65 .. 128 next to Exponential / Power / Generalized Power cones
on the GPU (hipkkt_step_enable_mixed_large, Settings.device_step_mixed_large; k_bar_psd_large of barrier_psd.hip).

Gates.
  * k_bar_psd_large repeats the arithmetic of k_bar_psd with another lane map, and the rows / step length of a large cone go through
    step_psd_large.hip: on a cone of side <= 64 (testing switch PSD_LARGE_MIN = 1, read at the enable) a handle of the new enable gives
    the bits of a handle of hipkkt_step_enable_mixed -- `==` and np.array_equal, the -Inf and the NaN arm included.
  * The barrier at sides 65, 96, 97 and 128 against the 50-digit value of tests/psd_barrier_reference.py with the construction and the
    gate of tests/test_gpu_mixed_step.py: PSD term = the set [PSD(n), Exponential] minus an Exponential-only handle, error at most
    max(8 x the host's error in the same case, 2 n) eps x scale plus the last rounding of the two float64 sums.  The reference is taken
    at all 8 candidates of side 65 and at candidates 0, 2 and 7 of the others (one 50-digit barrier costs 0.5 s at side 65 and 3 s at
    128); every candidate of every side is `==` across the launches of 8, 3 and 1 candidates.  Shifted dot: 1e-13 sum |terms|.
  * Rows and K blocks of a mixed set: kinds 0..2 and 4..6 bit for bit those of a handle without the PSD cones, PSD rows bit for bit
    those of a hipkkt_step_enable_psd_large handle without the non-symmetric cones; the symmetric + PSD start of the step length `==`.
  * End to end: SOLVED on every path, |dobj| <= 2 max(tol_gap_abs, tol_gap_rel max(1, |obj|)), scalars only with the device scaling.
No case is skipped or filtered.  Every figure is printed before it is asserted."""
import functools
import math

import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt, problems
from julia_standin import ipm
from julia_standin.cones import NonnegativeCone, PSDTriangleCone, SecondOrderCone, ZeroCone
from tests import psd_barrier_reference as br
from tests import psd_scaling_reference as sr
from tests import psd_step_reference as pr
from tests import test_gpu_mixed_step as tm
from tests.step_support import PARITY, STEP_FLAGS, _Timeout

pytestmark = pytest.mark.gpu

T = cl
MIXEDL = dict(tm.MIXED, device_step_psd_large=True, device_step_mixed_large=True)
MIXEDLN = dict(MIXEDL, device_scaling_psd=True, device_scaling_psd_large=True)
PSDL = dict(tm.PSD, device_step_psd_large=True)
STEP, AMIN, EPS = tm.STEP, tm.AMIN, br.EPS
_is_psd, _is_sym = tm._is_psd, tm._is_sym


def _stage_and_scale(hk, cones_of_factors, s, z, mu, strategy):
    """the scaling of a handle enabled by hand (a plugin built without flags): the host's PSD factors of `cones_of_factors` staged, then
    hipkkt_update_scaling_ex with their R"""
    psd = [c for c in cones_of_factors.cones if _is_psd(c)]
    hk.h.psd_set_factors(np.concatenate([c.Rinv.ravel(order="F") for c in psd]), np.concatenate([c.lam for c in psd]))
    ok, *_ = hk.h.update_scaling_ex(s, z, mu, strategy, tm._psd_R(cones_of_factors))
    assert ok


# ---- 1. the bits of the small path ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("late", [False, True], ids=["early", "late"])
@pytest.mark.parametrize("n", br.SIDES)
def test_the_large_routing_gives_the_bits_of_hipkkt_step_enable_mixed(n, late, monkeypatch):
    """What this test can and cannot see: with PSD_LARGE_MIN = 1 the side is <= 64, so k_bar_psd has already written the cone's two
    slots with the right values before k_bar_psd_large overwrites them.  A k_bar_psd_large that wrote other bits fails here; one that
    wrote nothing would pass (debug_dump(24) shows the routing list, not the write).  A missing write is caught at sides 65 .. 128
    (section 2 below), where k_bar_psd leaves the failure arm and an untouched slot makes the barrier non-finite."""
    with _Timeout(120):
        specs = [T.PSDTriangleConeT(n), T.ExponentialConeT()]
        monkeypatch.setenv("HIPKKT_PSD_LARGE_MIN", "1")
        hl, cones, _ = tm._handle(specs, 11, flags={})
        hl.h.step_enable_mixed_large(True, STEP, AMIN)
        monkeypatch.delenv("HIPKKT_PSD_LARGE_MIN")
        hs, _, _ = tm._handle(specs, 11, flags={})
        hs.h.step_enable_mixed(True, STEP, AMIN)
        assert list(hl.h.debug_dump(24)) == [0] and hs.h.debug_dump(24).size == 0      # who computes the PSD cone
        cs = br.case(n, late)
        rng = np.random.default_rng(500 + n)
        pc, ec = cones.cones
        rp, rexp = cones.rng_cones
        m = cones.numel
        s, z = np.zeros(m), np.zeros(m)
        s[rp], z[rp] = cs["s"], cs["z"]
        s[rexp], z[rexp] = tm._nonsym_point(ec, rng)
        mu = float(s @ z) / (cones.degree + 1)
        assert pc.update_scaling(s[rp], z[rp], mu)
        for hk in (hl, hs):
            _stage_and_scale(hk, cones, s, z, mu, 1)
        assert np.array_equal(hl.h.debug_dump(4), hs.h.debug_dump(4))                   # the blocks of K
        dz, ds = np.zeros(m), np.zeros(m)
        dz[rp], ds[rp] = cs["dz"], cs["ds"]
        dz[rexp], ds[rexp] = 0.01 * rng.standard_normal(3) * np.abs(z[rexp]), 0.01 * rng.standard_normal(3) * np.abs(s[rexp])
        for nalpha in (1, 3, 8):
            (bl, dl), (bs, dsm) = hl.cone_barrier(dz, ds, cs["alphas"][:nalpha]), hs.cone_barrier(dz, ds, cs["alphas"][:nalpha])
            print(f"[mixed large bits] n={n} late={late} {nalpha} candidates: {list(bl)}")
            assert all(math.isfinite(b) for b in bl)
            assert all(a == b for a, b in zip(bl, bs)) and np.array_equal(dl, dsm), (n, late, nalpha, bl, bs)
        # the outside-the-cone arm and the NaN arm
        zero = np.zeros(m)
        out_z, out_s, nan = zero.copy(), zero.copy(), zero.copy()
        out_z[rp] = pc.mat_to_svec(-2.0 * pc.svec_to_mat(z[rp]))
        out_s[rp] = pc.mat_to_svec(-2.0 * pc.svec_to_mat(s[rp]))
        nan[rp.start + (1 if n > 1 else 0)] = math.nan
        for what, (a, b), inf_at in (("z side", (out_z, zero), 1), ("s side", (zero, out_s), 1), ("both", (out_z, out_s), 1),
                                     ("nan", (nan, zero), 3)):
            (bl, _), (bs, _) = hl.cone_barrier(a, b, [1.0, 0.25, 0.0]), hs.cone_barrier(a, b, [1.0, 0.25, 0.0])
            print(f"[mixed large bits] n={n} late={late} {what}: {list(bl)}")
            assert all(v == -math.inf for v in bl[:inf_at]) and all(math.isfinite(v) for v in bl[inf_at:]), (what, bl)
            assert np.array_equal(bl, bs), (what, bl, bs)
        # the four row operations and the step length
        x = rng.standard_normal(m)
        dzr, dsr = rng.standard_normal(m), rng.standard_normal(m)
        dzr[rp], dsr[rp] = pr.direction(pc, rng, z[rp]), pr.direction(pc, rng, s[rp])
        ol, os_ = tm._row_ops(hl, dzr, dsr, x, 0.3 * mu), tm._row_ops(hs, dzr, dsr, x, 0.3 * mu)
        for op in ol:
            assert np.all(np.isfinite(ol[op])) and np.array_equal(ol[op], os_[op]), (op, n, late)
        bind_z, bind_s = zero.copy(), zero.copy()
        bind_z[rp] = -2.5 * z[rp] + 0.05 * pr.direction(pc, rng, z[rp])
        bind_s[rp] = -2.5 * s[rp] + 0.05 * pr.direction(pc, rng, s[rp])
        small = 0.01 * dzr * np.abs(z) / np.maximum(np.abs(dzr), 1e-300)
        for a, b in ((bind_z, zero), (zero, bind_s), (bind_z, bind_s), (small, zero), (zero, zero)):
            gl, gs = hl.cone_step_length(a, b, 1.0), hs.cone_step_length(a, b, 1.0)
            assert gl == gs and 0.0 < gl[0] <= 1.0, (n, late, gl, gs)


# ---- 2. the barrier at sides 65 .. 128 against 50 digits ----------------------------------------------------------------------------------

LARGE_SIDES = (65, 96, 97, 128)


def _ref_candidates(n):
    return tuple(range(br.NALPHA)) if n == 65 else (0, 2, 7)


@functools.lru_cache(maxsize=None)
def _large_case(n, late):
    """psd_barrier_reference.case for a side above 64, the 50-digit barrier at _ref_candidates(n) only -> dict(..., ref / scale /
    host_ratio: {candidate: value}).  Computed once per process; callers must not modify the arrays."""
    rng = np.random.default_rng(7000 + 10 * n + int(late))
    K = PSDTriangleCone(n)
    s, z, _ = pr.random_sz(K, rng, late)
    dz, ds = br.interior_direction(K, z, rng), br.interior_direction(K, s, rng)
    alphas = br.candidates()
    ref, scale, ratio = {}, {}, {}
    for j in _ref_candidates(n):
        b, sc = br.ref_barrier(n, z, s, dz, ds, alphas[j])
        ref[j], scale[j] = b, sc
        ratio[j] = float(abs(br.mpf(K.compute_barrier(z, s, dz, ds, alphas[j])) - b)) / (EPS * sc)
    for v in (s, z, dz, ds):
        v.setflags(write=False)
    return dict(K=K, n=n, late=late, s=s, z=z, dz=dz, ds=ds, alphas=alphas, ref=ref, scale=scale, host_ratio=ratio)


_pairs = {}


def _barrier_pair(n):
    """([PSD(n), Exponential] through hipkkt_step_enable_mixed_large, [Exponential] in Cone3 mode), built once per side"""
    if n not in _pairs:
        hm, cm, _ = tm._handle([T.PSDTriangleConeT(n), T.ExponentialConeT()], 11, MIXEDL)
        he, ce, _ = tm._handle([T.ExponentialConeT()], 12, tm.NONSYM)
        assert hm.steps_mixed and hm.steps_psd_large and hm.steps_psd and hm.steps_nonsymmetric and not hm.default_start_on_device
        assert not hm.scales_psd and not hm.starts_psd_large and he.steps_nonsymmetric and not he.steps_psd
        assert list(hm.h.debug_dump(24)) == [0]
        _pairs[n] = (hm, cm, he, ce)
    return _pairs[n]


def _pair_at(n, cs, seed):
    """the pair scaled at the case's point -> (hm, cm, he, s, z, mu, rng)"""
    hm, cm, he, ce = _barrier_pair(n)
    rng = np.random.default_rng(seed)
    rp, rexp = cm.rng_cones
    s, z = np.zeros(cm.numel), np.zeros(cm.numel)
    s[rp], z[rp] = cs["s"], cs["z"]
    s[rexp], z[rexp] = tm._nonsym_point(cm.cones[1], rng)
    mu = float(s @ z) / (cm.degree + 1)
    tm._scale(hm, cm, s, z, mu, 1)
    assert he.h.update_scaling_ex(s[rexp], z[rexp], mu, 1)[0]
    return hm, cm, he, s, z, mu, rng


@pytest.mark.parametrize("late", [False, True], ids=["early", "late"])
@pytest.mark.parametrize("n", LARGE_SIDES)
def test_barrier_of_one_large_psd_cone_next_to_an_exponential_cone(n, late):
    with _Timeout(180):
        cs = _large_case(n, late)
        hm, cm, he, s, z, mu, rng = _pair_at(n, cs, 500 + n)
        pc, ec = cm.cones
        rp, rexp = cm.rng_cones
        dz, ds = np.zeros(cm.numel), np.zeros(cm.numel)
        dz[rp], ds[rp] = cs["dz"], cs["ds"]
        dz[rexp], ds[rexp] = 0.01 * rng.standard_normal(3) * np.abs(z[rexp]), 0.01 * rng.standard_normal(3) * np.abs(s[rexp])
        assert math.isfinite(ec.compute_barrier(z[rexp], s[rexp], dz[rexp], ds[rexp], cs["alphas"][0]))
        runs = {}
        for nalpha in (1, 3, 8):
            alphas = cs["alphas"][:nalpha]
            bars, dots = hm.cone_barrier(dz, ds, alphas)
            bars_e, _ = he.cone_barrier(dz[rexp], ds[rexp], alphas)
            runs[nalpha] = (bars, dots, bars_e)
        bars, dots, bars_e = runs[8]
        worst_d = worst_h = 0.0
        for j, a in enumerate(cs["alphas"]):
            assert math.isfinite(bars[j]) and math.isfinite(bars_e[j]), (n, late, a, bars[j], bars_e[j])
            for nalpha in (1, 3):      # the same candidate in a shorter launch: the same slot arithmetic, the same bits
                if j < nalpha:
                    assert runs[nalpha][0][j] == bars[j] and runs[nalpha][1][j] == dots[j] and runs[nalpha][2][j] == bars_e[j], (n, j, nalpha)
            zz, ss = z + a * dz, s + a * ds
            assert abs(dots[j] - float(zz @ ss)) <= 1e-13 * float(np.abs(zz) @ np.abs(ss))
            if j not in cs["ref"]:
                continue
            term = bars[j] - bars_e[j]
            ref, scale, rh = cs["ref"][j], cs["scale"][j], cs["host_ratio"][j]
            sums = EPS * (abs(float(ref)) + abs(bars_e[j]))      # sum |terms| of the larger sum: the PSD term and the Exponential one
            allowed = br.allowed(rh, n)
            err = float(abs(br.mpf(term) - ref))
            rd = err / (EPS * scale)
            print(f"[mixed large barrier] n={n} late={late} candidate {j}, alpha={a:.4f}: PSD term {term:.6e}, device {rd:.3f}, "
                  f"host {rh:.3f}, allowed {allowed:.1f} (eps x scale {scale:.3e}) + {sums:.2e} for the two sums")
            assert err <= allowed * EPS * scale + sums, (n, late, j, a, rd, rh)
            worst_d, worst_h = max(worst_d, rd), max(worst_h, rh)
        print(f"[mixed large barrier] n={n} late={late}: worst device {worst_d:.3f}, worst host {worst_h:.3f} (eps x scale)")


# ---- 3. edges at side 65 --------------------------------------------------------------------------------------------------------------------

def test_barrier_edges_outside_nan_zero_direction_zero_step_at_side_65():
    with _Timeout(120):
        cs = _large_case(65, False)
        hm, cm, he, s, z, mu, rng = _pair_at(65, cs, 17)
        pc, ec = cm.cones
        rp, rexp = cm.rng_cones
        zero = np.zeros(cm.numel)
        out_z, out_s = zero.copy(), zero.copy()
        out_z[rp] = pc.mat_to_svec(-2.0 * pc.svec_to_mat(z[rp]))      # Z + 1 (-2 Z) = -Z
        out_s[rp] = pc.mat_to_svec(-2.0 * pc.svec_to_mat(s[rp]))
        for what, (dz, ds) in {"z side": (out_z, zero), "s side": (zero, out_s), "both": (out_z, out_s)}.items():
            bars, dots = hm.cone_barrier(dz, ds, [1.0, 0.25, 0.0])
            print(f"[mixed large barrier edges] outside on the {what}: {bars}")
            assert bars[0] == -math.inf, (what, bars)
            assert cm.compute_barrier(z, s, dz, ds, 1.0) == -math.inf
            assert math.isfinite(bars[1]) and math.isfinite(bars[2])
            assert abs(bars[1] - cm.compute_barrier(z, s, dz, ds, 0.25)) <= PARITY * max(1.0, abs(bars[1]))
            assert np.array_equal(hm.cone_affine_ds()[rexp], s[rexp])     # the handle still serves
        nan = zero.copy()
        nan[rp.start + 1] = math.nan
        bars, _ = hm.cone_barrier(nan, zero, [0.5, 0.25])
        assert bars[0] == -math.inf and bars[1] == -math.inf, bars      # a NaN reaches a pivot: the failure arm
        nan_last = zero.copy()
        nan_last[rp.stop - 1] = math.nan                                # the last pivot, row 64: the second group of 64 rows
        bars, _ = hm.cone_barrier(zero, nan_last, [0.5])
        assert bars[0] == -math.inf, bars
        assert np.array_equal(hm.cone_affine_ds()[rexp], s[rexp])
        dz, ds = zero.copy(), zero.copy()
        dz[rp], ds[rp] = cs["dz"], cs["ds"]
        at_point, _ = hm.cone_barrier(zero, zero, [0.7, 0.3])
        at_zero, _ = hm.cone_barrier(dz, ds, [0.0])
        assert at_point[0] == at_point[1] == at_zero[0] and math.isfinite(at_zero[0])
        only_ds, _ = hm.cone_barrier(zero, ds, [0.5])                # dZ = 0 alone
        assert abs(only_ds[0] - cm.compute_barrier(z, s, zero, ds, 0.5)) <= PARITY * max(1.0, abs(only_ds[0]))
        assert np.array_equal(hm.cone_affine_ds()[rexp], s[rexp])     # the handle still serves


# ---- 4. a mixed set: rows, K, the start of the step length -----------------------------------------------------------------------------------

def _set_specs():
    return [T.NonnegativeConeT(3), T.PSDTriangleConeT(65), T.ExponentialConeT(), T.SecondOrderConeT(4), T.PowerConeT(0.3),
            T.PSDTriangleConeT(8), T.GenPowerConeT((0.6, 0.4), 1), T.PSDTriangleConeT(2)]


_sets = {}


def _large_set(late, strategy, seed=3):
    """the set scaled at one point with its two twins scaled at the same rows: `ns` without the PSD cones (GenPow mode), `ps` without the
    non-symmetric cones (PSD mode through hipkkt_step_enable_psd_large).  Built once per (late, strategy)."""
    key = (late, strategy)
    if key not in _sets:
        specs = _set_specs()
        hk, cones, st = tm._handle(specs, seed, MIXEDL)
        assert hk.steps_on_device and hk.steps_mixed and hk.steps_psd and hk.steps_psd_large and hk.steps_nonsymmetric
        assert list(hk.h.debug_dump(24)) == [0]                       # PSD(65) alone goes to the large kernels
        rng = np.random.default_rng(300 + seed + 10 * int(late))
        s, z, mu = tm._point(cones, rng, late)
        code = {"primal_dual": 0, "dual": 1}[strategy]
        tm._scale(hk, cones, s, z, mu, code)
        ns, nsc, nsrows = tm._sub_handle(specs, cones, lambda c: not _is_psd(c), seed + 50, tm.NONSYM)
        assert ns.steps_on_device and ns.steps_nonsymmetric and not ns.steps_psd
        ps, psc, psrows = tm._sub_handle(specs, cones, _is_sym, seed + 60, PSDL)
        assert ps.steps_on_device and ps.steps_psd and ps.steps_psd_large and not ps.steps_nonsymmetric
        assert ns.h.update_scaling_ex(s[nsrows], z[nsrows], mu, code)[0]
        for c, cf in zip(psc.cones, [c for c in cones.cones if _is_sym(c)]):
            if _is_psd(c):
                c.R[:], c.Rinv[:], c.lam[:] = cf.R, cf.Rinv, cf.lam
        ps.h.psd_set_factors(*ps._psd_factors())
        assert ps.h.update_scaling(s[psrows], z[psrows], tm._psd_R(psc))[0]
        _sets[key] = dict(hk=hk, cones=cones, st=st, s=s, z=z, mu=mu, ns=ns, nsc=nsc, nsrows=nsrows, ps=ps, psc=psc, psrows=psrows)
    return _sets[key]


SET_POINTS = [(False, "dual"), (True, "dual"), (False, "primal_dual")]
SET_IDS = [f"{'late' if l else 'early'}-{s}" for l, s in SET_POINTS]


@pytest.mark.parametrize("late,strategy", SET_POINTS, ids=SET_IDS)
def test_row_operations_K_and_the_start_of_the_step_length_are_each_family_s_own_bits(late, strategy):
    with _Timeout(180):
        M = _large_set(late, strategy)
        hk, cones, ns, ps, nsrows, psrows = M["hk"], M["cones"], M["ns"], M["ps"], M["nsrows"], M["psrows"]
        s, z = M["s"], M["z"]
        rng = np.random.default_rng(41)
        dz, ds, x = tm._directions(M, rng)
        sm = 0.3 * M["mu"]
        got = tm._row_ops(hk, dz, ds, x, sm)
        tw_ns = tm._row_ops(ns, dz[nsrows], ds[nsrows], x[nsrows], sm)
        tw_ps = tm._row_ops(ps, dz[psrows], ds[psrows], x[psrows], sm)
        psd_in_ps, psd_rows = tm._rows(M["psc"], _is_psd), tm._rows(cones, _is_psd)
        for op in got:
            assert np.all(np.isfinite(got[op])), op
            assert np.array_equal(got[op][nsrows], tw_ns[op]), (op, "kinds 0..2 and 4..6")
            assert np.array_equal(got[op][psd_rows], tw_ps[op][psd_in_ps]), (op, "PSD rows")
        Kd, Kn, Kp = hk.h.debug_dump(4), ns.h.debug_dump(4), ps.h.debug_dump(4)
        mp_d, mp_n, mp_p = hk.h.map(2), ns.h.map(2), ps.h.map(2)
        bn, bp = iter(M["nsc"].rng_blocks), iter(M["psc"].rng_blocks)
        for c, rb in zip(cones.cones, cones.rng_blocks):
            rb_n = None if _is_psd(c) else next(bn)
            rb_p = next(bp) if _is_sym(c) else None
            if rb_n is not None:
                assert np.array_equal(Kd[mp_d[rb]], Kn[mp_n[rb_n]]), type(c).__name__
            if rb_p is not None:
                assert np.array_equal(Kd[mp_d[rb]], Kp[mp_p[rb_p]]), type(c).__name__
        # the step length: a symmetric or PSD member binds alone, the non-symmetric members stay where they are; then a direction on all
        zero = np.zeros(cones.numel)
        assert hk.cone_step_length(zero, zero, 0.4) == (0.4, 0.4)
        decisions = 0
        for k, (c, r) in enumerate(zip(cones.cones, cones.rng_cones)):
            if isinstance(c, ZeroCone) or not _is_sym(c):
                continue
            for side in (0, 1):
                dzb, dsb = zero.copy(), zero.copy()
                q = (z, s)[side]
                (dzb, dsb)[side][r] = -2.5 * q[r] + (0.05 * pr.direction(c, rng, q[r]) if _is_psd(c) else 0.0)
                pair = ps.cone_step_length(dzb[psrows], dsb[psrows], 1.0)
                start = min(pair)
                assert pair[side] < 0.5 and pair[1 - side] == 1.0, (k, side, pair)
                got_l = hk.cone_step_length(dzb, dsb, 1.0)
                print(f"[mixed large step length] late={late} {strategy} cone {k} ({type(c).__name__}) side {side}: twin {pair!r}, "
                      f"device {got_l!r}")
                assert got_l == (start, start), (k, type(c).__name__, side, got_l, pair)
                decisions += 1
        dzr, dsr = 0.05 * rng.standard_normal(cones.numel) * np.abs(z), 0.05 * rng.standard_normal(cones.numel) * np.abs(s)
        for c, r in zip(cones.cones, cones.rng_cones):
            if _is_psd(c):
                dzr[r], dsr[r] = -1.5 * z[r] + br.interior_direction(c, z[r], rng), -1.2 * s[r] + br.interior_direction(c, s[r], rng)
            elif isinstance(c, (NonnegativeCone, SecondOrderCone)):
                dzr[r], dsr[r] = -1.3 * z[r] + 0.1 * rng.standard_normal(c.numel) * np.abs(z[r]), 0.3 * s[r]
        pair = ps.cone_step_length(dzr[psrows], dsr[psrows], 1.0)
        start = min(pair)
        assert start < tm.ALPHA0
        tm._assert_margins(M, dzr, dsr, start)
        got_l = hk.cone_step_length(dzr, dsr, 1.0)
        print(f"[mixed large step length] late={late} {strategy}: {decisions} binding members; random direction: twin {pair!r}, "
              f"device {got_l!r}")
        assert got_l == (start, start) and start == tm._host_composite(M, dzr, dsr, start)
        # the barrier of the whole set against the stand-in's composite, and its slots across launch widths
        dzb, dsb = 0.2 * rng.standard_normal(cones.numel) * np.abs(z), 0.2 * rng.standard_normal(cones.numel) * np.abs(s)
        for c, r in zip(cones.cones, cones.rng_cones):
            if _is_psd(c):
                dzb[r], dsb[r] = br.interior_direction(c, z[r], rng), br.interior_direction(c, s[r], rng)
            elif isinstance(c, SecondOrderCone):
                dzb[r], dsb[r] = 0.2 * z[r], -0.2 * s[r]
        st = M["st"]
        a0 = st.max_step_fraction * min(cones.step_length(dzb, dsb, z, s, 1.0))
        assert a0 > 0
        alphas = [a0 * st.linesearch_backtrack_step ** k for k in range(8)]
        bars, dots = hk.cone_barrier(dzb, dsb, alphas)
        assert all(math.isfinite(b) for b in bars)
        tm._check_barrier(bars, dots, cones, z, s, dzb, dsb, alphas, f"mixed large late={late} {strategy} 8")
        for n in (1, 3):
            b, d = hk.cone_barrier(dzb, dsb, alphas[2:2 + n])
            assert np.array_equal(b, bars[2:2 + n]) and np.array_equal(d, dots[2:2 + n]), n


# ---- 5. the protocol -------------------------------------------------------------------------------------------------------------------------

def test_the_enables_refuse_what_they_cannot_serve():
    with _Timeout(120):
        hk, cones, _ = tm._handle([T.PSDTriangleConeT(65), T.ExponentialConeT()], 1, flags={})
        with pytest.raises(ValueError, match="step_enable_mixed"):
            hk.h.step_enable_mixed(True, STEP, AMIN)                    # the first enable keeps its side limit
        bad_sets = ([T.PSDTriangleConeT(129), T.ExponentialConeT()],                         # a side above 128
                    [T.NonnegativeConeT(3), T.SecondOrderConeT(4)],                          # symmetric
                    [T.PSDTriangleConeT(65), T.NonnegativeConeT(2)],                         # PSD without a non-symmetric member
                    [T.ExponentialConeT(), T.NonnegativeConeT(2)])                           # no PSD member
        for specs in bad_sets:
            hb, _, _ = tm._handle(specs, 1, MIXEDL)
            assert not hb.steps_mixed, specs
            with pytest.raises(ValueError, match="step_enable_mixed_large"):
                hb.h.step_enable_mixed_large(True, STEP, AMIN)
            hb.h.step_enable_mixed_large(False, STEP, AMIN)              # switching off is always possible
        # the plugin: every flag but the new one keeps the host loop for a side of 65
        hh, _, _ = tm._handle([T.PSDTriangleConeT(65), T.ExponentialConeT()], 1, dict(tm.MIXED, device_step_psd_large=True))
        assert not hh.steps_on_device and not hh.steps_mixed
        # bad line-search parameters leave the handle as it was: not enabled ...
        s, z, mu = tm._point(cones, np.random.default_rng(9), False)
        assert cones.cones[0].update_scaling(s[cones.rng_cones[0]], z[cones.rng_cones[0]], mu)
        bad = ((0.0, 1e-4), (1.0, 1e-4), (1.5, 1e-4), (-0.1, 1e-4), (float("nan"), 1e-4), (0.8, 0.0), (0.8, -1.0), (0.8, float("inf")),
               (0.999999, 1e-4))
        for step, amin in bad:
            with pytest.raises(ValueError):
                hk.h.step_enable_mixed_large(True, step, amin)
        with pytest.raises(ValueError):
            hk.h.psd_set_factors(np.zeros(65 * 65), np.ones(65))        # not before the enable
        assert hk.h.debug_dump(24).size == 0
        for fn in (hk.h.step_enable_cone3, hk.h.step_enable_genpow):
            with pytest.raises(ValueError):
                fn(True, STEP, AMIN)
        for fn in (hk.h.step_enable_psd, hk.h.step_enable_psd_large):
            with pytest.raises(ValueError):
                fn(True)
        hk.h.step_enable_mixed_large(True, STEP, AMIN)
        assert list(hk.h.debug_dump(24)) == [0]
        _stage_and_scale(hk, cones, s, z, mu, 1)
        first = hk.cone_affine_ds()
        # ... and, once enabled and scaled, still enabled and scaled
        for step, amin in bad:
            with pytest.raises(ValueError):
                hk.h.step_enable_mixed_large(True, step, amin)
        assert np.array_equal(hk.cone_affine_ds(), first) and list(hk.h.debug_dump(24)) == [0]
        m = cones.numel
        bars, _ = hk.cone_barrier(np.zeros(m), np.zeros(m), [0.0])
        assert math.isfinite(bars[0])
        # the default start stays with the caller
        for call in (hk.h.cone_set_identity_scaling, lambda: hk.h.cone_margins(s, 0), lambda: hk.h.cone_shift_to_interior(s.copy(), 0)):
            with pytest.raises(ValueError):
                call()
        with pytest.raises(ValueError, match="step_default_start_enable_psd_large"):
            hk.h.step_default_start_enable_psd_large(True)
        assert np.array_equal(hk.cone_affine_ds(), first)
        # the scaling: the small enable refuses, the large one accepts and needs no factors
        with pytest.raises(ValueError, match="psd_scaling_enable"):
            hk.h.psd_scaling_enable(True)
        assert np.array_equal(hk.cone_affine_ds(), first)
        with pytest.raises(hipkkt.HipKKTError):
            hk.h.update_scaling_ex(s, z, mu, 1, None)
        hk.h.psd_scaling_enable_large(True)
        with pytest.raises(ValueError):
            hk.cone_affine_ds()                                         # the enable invalidates the resident scaling
        assert hk.h.update_scaling_ex(s, z, mu, 1, None)[0]
        nonpsd = tm._rows(cones, lambda c: not _is_psd(c))
        assert np.array_equal(hk.cone_affine_ds()[nonpsd], first[nonpsd])
        # a handle whose sides are all <= 64: both scaling enables serve it after the new enable (no side above the small limit)
        hs, cs_, _ = tm._handle([T.PSDTriangleConeT(3), T.ExponentialConeT()], 2, flags={})
        hs.h.step_enable_mixed_large(True, STEP, AMIN)
        assert hs.h.debug_dump(24).size == 0
        hs.h.psd_scaling_enable(True)
        hs.h.psd_scaling_enable_large(True)
        # enable = 0 and a new registration switch it off
        hk.h.step_enable_mixed_large(False, STEP, AMIN)
        with pytest.raises(ValueError):
            hk.cone_affine_ds()
        with pytest.raises(ValueError):
            hk.h.psd_scaling_enable_large(True)
        assert hk.h.debug_dump(24).size == 0
        hk.h.step_enable_mixed_large(True, STEP, AMIN)
        hk.h.step_enable_mixed(False, STEP, AMIN)                       # the first enable's off switch is the same switch
        with pytest.raises(ValueError):
            hk.h.psd_scaling_enable_large(True)
        hk.h.step_enable_mixed_large(True, STEP, AMIN)
        hk.h.psd_scaling_enable_large(True)
        kinds, alpha = cones.kkt_cone_kinds_ex()
        hk.h.set_cone_types_ex(kinds, alpha)
        with pytest.raises(ValueError):
            hk.h.psd_scaling_enable_large(True)
        assert hk.h.update_scaling_ex(s, z, mu, 1, tm._psd_R(cones))[0]
        with pytest.raises(ValueError):
            hk.cone_affine_ds()


@pytest.mark.parametrize("late", [False, True], ids=["early", "late"])
def test_device_psd_scaling_of_a_side_of_65_in_mixed_mode_meets_the_invariants(late):
    with _Timeout(300):
        hn, cones, _ = tm._handle([T.PSDTriangleConeT(65), T.ExponentialConeT(), T.PSDTriangleConeT(8)], 3, MIXEDLN)
        assert hn.steps_mixed and hn.steps_psd_large and hn.scales_psd and not hn.starts_psd_large
        assert list(hn.h.debug_dump(24)) == [0]
        s, z, mu = tm._point(cones, np.random.default_rng(61 + int(late)), late)
        assert hn.h.update_scaling_ex(s, z, mu, 1, None)[0]
        R, Ri, lam = hn.h.psd_get_factors()
        assert np.all(np.isfinite(hn.cone_mul_hs(np.ones(cones.numel))))
        c, r = cones.cones[0], cones.rng_cones[0]
        n = c.n
        Rc, Ric, lc = R[:n * n].reshape(n, n, order="F"), Ri[:n * n].reshape(n, n, order="F"), lam[:n]
        assert np.all(lc > 0) and np.all(np.diff(lc) <= 0)
        assert c.update_scaling(s[r], z[r], mu)
        ref = sr.Reference(n, s[r], z[r])
        sr.gate(f"mixed large mode late={late} PSD(65)", n, ref.residuals(Rc, Ric, lc), ref.residuals(c.R, c.Rinv, c.lam))
        # the same factors from a symmetric handle of hipkkt_psd_scaling_enable_large: one kernel, one set of bits
        hp, pc, _ = tm._handle([T.PSDTriangleConeT(65), T.PSDTriangleConeT(8)], 4, dict(PSDL, device_scaling_psd=True,
                                                                                     device_scaling_psd_large=True))
        assert hp.scales_psd and hp.steps_psd_large
        keep = tm._rows(cones, _is_psd)
        assert hp.h.update_scaling(s[keep], z[keep], None)[0]
        assert all(np.array_equal(a, b) for a, b in zip(hp.h.psd_get_factors(), (R, Ri, lam)))


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------------

END_TO_END = {
    "mix30_72": (dict(n=30, psd_sides=[5, 72], nexp=2, npow=2, ngenpow=2, nn=3, nzero=2, socdim=4, seed=6), (False, True)),
    "exp30_65": (dict(n=30, psd_sides=[65, 3], nexp=3, npow=0, ngenpow=0, nn=3, nzero=2, socdim=4, seed=5), (False,)),
}
E2E_CASES = [(name, forced) for name, (_, modes) in END_TO_END.items() for forced in modes]


@pytest.mark.parametrize("name,forced", E2E_CASES, ids=[f"{n}-{'forced_dual' if f else 'default'}" for n, f in E2E_CASES])
def test_ipm_with_the_mixed_large_device_step_matches_the_host_cone_algebra(name, forced):
    prob = problems.mixed_psd_nonsym(**END_TO_END[name][0])
    with _Timeout(300):
        H, ref = tm._solve(prob, forced, **STEP_FLAGS)
        D, got = tm._solve(prob, forced, **MIXEDL)
        N, gotn = tm._solve(prob, forced, **MIXEDLN)
    assert not H._device_step
    for S in (D, N):
        ks = S.kktsystem.kktsolver
        assert S._device_step and S._device_step_psd and ks.steps_mixed and ks.steps_psd_large and S._device_scaling_psd == (S is N)
        assert not S._device_default_start and ks.h.debug_dump(24).size == 1
    st = D.settings
    tol = 2.0 * max(st.tol_gap_abs, st.tol_gap_rel * max(1.0, abs(ref.obj_val)))

    def per_iter(S, sol):
        t = S.trace
        return [(t[k + 1]["h2d"] - t[k]["h2d"], t[k + 1]["d2h"] - t[k]["d2h"]) for k in range(min(sol.iterations, len(t) - 1))]

    bh, bd, bn = per_iter(H, ref), per_iter(D, got), per_iter(N, gotn)
    for what, S, sol, b in (("host cone algebra", H, ref, bh), ("device_step_mixed_large", D, got, bd),
                            ("+ device_scaling_psd_large", N, gotn, bn)):
        print(f"[mixed large end to end {name} forced={forced}] {what}: {sol.status} in {sol.iterations} iterations, obj {sol.obj_val!r}, "
              f"|dobj| {abs(sol.obj_val - ref.obj_val):.2e} (allowed {tol:.2e}), bytes / iteration up {max(u for u, _ in b)} down "
              f"{max(d for _, d in b)}, barrier searches {S.barrier_searches} (backtracks {S.barrier_backtracks})")
    assert ref.status == got.status == gotn.status == ipm.SOLVED, (ref.status, got.status, gotn.status)
    assert abs(got.obj_val - ref.obj_val) <= tol and abs(gotn.obj_val - ref.obj_val) <= tol
    assert all(u + d <= tm.SCALAR_BYTES for u, d in bn), bn      # scalars only: no row of (s, z) comes down, no factor goes up
    if name == "mix30_72":
        assert D.barrier_searches > 0 and N.barrier_searches > 0      # the Dual strategy searched the barrier on the device
    if forced:
        assert H.barrier_searches > 0
