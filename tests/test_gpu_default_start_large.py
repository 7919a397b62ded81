"""The default start of a symmetric cone set with PSD sides of 65 .. 128 on the device (hipkkt_step_default_start_enable_psd_large,
Settings.device_default_start_psd_large; csrc/start.hip k_start_margin_psd_large and the side bound of k_start_shift).

Two yardsticks.  (1) The margins of a large cone come from the Jacobi sweeps of the smaller cones' kernel with wider lane mappings, so
on a cone of side <= 64 (testing switch PSD_LARGE_MIN = 1 at the step enable) every stage gives the bits of the existing path: `==`
and `np.array_equal`.  (2) On sides 65 .. 128 the stages and the gates of tests/test_gpu_default_start.py (its checking functions and
its vector constructions are imported; handles, cone sets and flags are this file's own): the identity scaling bit for bit the host
path's K, margins within max(8 x host, 2 n) eps |Z|_2 of 50 digits, the three arms of the shift `==` the reference shift with the
device's (min_margin, target), the fused call's [x | z | s] bit for bit the host _default_start's with the device's margins.
mp.eigsy takes 1 s at side 65 and 6 s at side 128, so side 128 gets one random vector; the diagonal matrix and Z = -2 I need no eigsy
and run at 65, 96 and 128.  Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt
from clarabel_jl_amd.kktsolver import HipKKTSolver
from julia_standin.cones import ZeroCone
from tests import default_start_reference as dr
from tests import test_gpu_psd_step as tp
from tests.step_support import STEP_FLAGS, _problem, _Timeout
from tests.test_gpu_default_start import CASES_LARGE, _check_margins, _host_default_start, _placed, _print_worst

pytestmark = pytest.mark.gpu

T = cl
LARGE = dict(device_step=True, device_step_psd=True, device_step_psd_large=True, **STEP_FLAGS)
LARGE_ALL = dict(LARGE, device_scaling_psd=True, device_scaling_psd_large=True, device_default_start=True,
                 device_default_start_psd_large=True)


def _mixed_large():
    return [T.NonnegativeConeT(3), T.PSDTriangleConeT(65), T.SecondOrderConeT(4), T.PSDTriangleConeT(8), T.ZeroConeT(2),
            T.PSDTriangleConeT(66)]


SETS = {"side_65": lambda: [T.PSDTriangleConeT(65)], "side_96": lambda: [T.PSDTriangleConeT(96)],
        "side_128": lambda: [T.PSDTriangleConeT(128)], "mixed_large": _mixed_large}
BOTH_P = pytest.mark.parametrize("pzero", [False, True], ids=["P", "P0"])


def _build(specs, pzero, flags, seed=3):
    """(plugin, cones, problem) for the cone set as given (not collapsed), with P or with structural P = 0"""
    P, q, A, b, specs = _problem(specs, seed)
    if pzero:
        P = sp.csc_matrix(P.shape)
    cones = cl.CompositeCone(specs)
    Pt = sp.triu(sp.csc_matrix(P), format="csc")
    Pt.sort_indices()
    A = sp.csc_matrix(A)
    A.sort_indices()
    m, n = A.shape
    return HipKKTSolver(Pt, A, cones, m, n, cl.Settings(**flags)), cones, (Pt, q, A, b)


def _handle(name, pzero=False):
    hk, cones, prob = _build(SETS[name](), pzero, LARGE_ALL)
    assert hk.steps_psd_large and hk.scales_psd and hk.starts_psd_large and hk.default_start_on_device
    return hk, cones, prob


# ---- 1. the bits of the existing path -------------------------------------------------------------------------------------------------------

BIT_SETS = {f"side_{n}": (lambda n=n: [T.PSDTriangleConeT(n)]) for n in (1, 8, 33, 64)}
BIT_SETS["mixed"] = tp._mixed_specs


def _fused(hk, xzs):
    st = hk.settings
    return hk.h.step_default_start_dev(xzs.ptr, st.static_regularization_enable, st.static_regularization_constant,
                                       st.static_regularization_proportional, **hk._ir())


@pytest.mark.parametrize("name", list(BIT_SETS))
def test_the_large_margins_give_the_bits_of_the_small_ones(name, monkeypatch):
    """both handles through hipkkt_step_enable_psd_large + hipkkt_step_default_start_enable_psd_large: on the first
    k_start_margin_psd_large overwrites every PSD cone's margins (PSD_LARGE_MIN = 1, read at the step enable), on the second none"""
    with _Timeout(120):
        pair = []
        for lmin in ("1", None):
            if lmin:
                monkeypatch.setenv("HIPKKT_PSD_LARGE_MIN", lmin)
            else:
                monkeypatch.delenv("HIPKKT_PSD_LARGE_MIN")
            hk, cones, prob = _build(BIT_SETS[name](), False, {})
            hk.h.step_enable_psd_large(True)
            hk.h.step_default_start_enable_psd_large(True)
            npsd = sum(tp._is_psd(c) for c in cones.cones)
            assert list(hk.h.debug_dump(24)) == (list(range(npsd)) if lmin else [])
            pair.append((hk, prob))
        (hl, prob), (hs, _) = pair
        rng = np.random.default_rng(17)
        vectors = [rng.standard_normal(cones.numel), 100.0 * rng.standard_normal(cones.numel)]
        vectors += [_placed(cones, rng, k, d, gap) for k, c in enumerate(cones.cones) if tp._is_psd(c)
                    for d, gap, _ in CASES_LARGE][:6]
        for v in vectors:
            for pd in ("primal", "dual"):
                a, b = hl.h.cone_margins(v, pd), hs.h.cone_margins(v, pd)
                print(f"[default start large bits] {name} {pd}: margins {a!r} / {b!r}")
                assert a == b
                wl, ws = hl.h.cone_shift_to_interior(v, pd), hs.h.cone_shift_to_interior(v, pd)
                assert np.array_equal(wl[0], ws[0]) and wl[1:] == ws[1:]
        outs = []
        for hk in (hl, hs):
            hk.h.cone_set_identity_scaling()
            K = hk.h.kkt()[2].copy()
            hk.set_problem_vectors(prob[1], prob[3])
            xzs = hk.device_buffer(hk.n + 2 * hk.m)
            ok, scal, steps = _fused(hk, xzs)
            assert ok
            outs.append((K, np.array(scal), list(steps), xzs.download()))
            xzs.close()
        (K0, sc0, st0, x0), (K1, sc1, st1, x1) = outs
        assert dr.same_bits(K0, K1) and dr.same_bits(sc0, sc1) and st0 == st1 and dr.same_bits(x0, x1)


# ---- 2. identity scaling ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["side_65", "side_128", "mixed_large"])
@BOTH_P
def test_identity_scaling_writes_the_bits_of_the_host_path(name, pzero):
    with _Timeout(120):
        hk, cones, _ = _handle(name, pzero)
        twin, tcones, _ = _handle(name, pzero)
        # a resident scaling first: the identity must drop it
        s, z = tp._point(cones, np.random.default_rng(5), False)
        assert hk.h.update_scaling(s, z)[0]
        hk.cone_affine_ds()
        before = hipkkt.TRAFFIC["h2d_bytes"]
        hk.h.cone_set_identity_scaling()
        assert hipkkt.TRAFFIC["h2d_bytes"] == before             # nothing is uploaded
        with pytest.raises(ValueError):
            hk.cone_affine_ds()                                  # refused until the next successful scaling
        tcones.set_identity_scaling()
        assert twin.kktsolver_update(tcones)                     # the host path: Hs assembled and uploaded
        kd, kh = hk.h.kkt()[2], twin.h.kkt()[2]
        same = kd.view(np.uint64) == kh.view(np.uint64)
        assert np.all(same), (name, int(np.sum(~same)), kd[~same][:5], kh[~same][:5])
        if any(isinstance(c, ZeroCone) for c in cones.cones):
            assert np.any(np.signbit(kd) & (kd == 0.0))          # the negated zero of hipkkt_set_hs
        assert hk.kktsolver_refactor()
        assert (hk.diagonal_regularizer, hk.last_nreg) == (twin.diagonal_regularizer, twin.last_nreg)
        assert hk.h.update_scaling(s, z)[0]                      # and a scaling brings the step calls back
        hk.cone_affine_ds()


# ---- 3. margins -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,random", [(65, True), (96, False), (128, True)])
def test_margins_of_a_large_cone(n, random):
    """a diagonal matrix and Z = -2 I (their eigenvalues are their entries), and one random symmetric matrix at 65 and 128"""
    with _Timeout(120):
        name = f"side_{n}"
        hk, cones, _ = _handle(name)
        c = cones.cones[0]
        rng = np.random.default_rng(500 + n)
        vectors = [("diagonal", c.mat_to_svec(np.diag(rng.standard_normal(n)))), ("Z = -2 I", c.mat_to_svec(-2.0 * np.eye(n)))]
        if random:
            vectors.append(("random", rng.standard_normal(cones.numel)))
        for label, v in vectors:
            ref = dr.margins_mp(cones, v)
            for pd in ("primal", "dual"):
                a, b = hk.h.cone_margins(v, pd)
                _check_margins(f"{name} {pd} {label}", a, b, ref)
        _print_worst(name)


# ---- 4. shift ---------------------------------------------------------------------------------------------------------------------------------

def test_shift_takes_the_reference_arm_at_side_65():
    """the three arms, one constructed vector each: margins within the gate, the reference's arm, rows `==` the reference shift with the
    device's (min_margin, target)"""
    with _Timeout(120):
        hk, cones, _ = _handle("side_65")
        rng = np.random.default_rng(65)
        arms = set()
        for d, gap, arm in CASES_LARGE:
            v = _placed(cones, rng, 0, d, gap)
            ref = dr.margins_mp(cones, v)
            tgt, br, margin = dr.decision_mp(ref)
            assert margin >= 1e-6 and br == arm, (d, gap, br, arm, margin)
            for pd in ("primal", "dual"):
                a, b = hk.h.cone_margins(v, pd)
                _check_margins(f"side_65 {pd} d={d}", a, b, ref)
                w, mn, pos, tg, got_br = hk.h.cone_shift_to_interior(v, pd)
                assert (mn, pos) == (a, b)
                assert got_br == br, (pd, d, got_br, br, mn, tg)
                assert tg == dr.target_of(pos, cones.degree)
                want, want_br = dr.apply_shift(cones, v, pd, mn, tg)
                assert want_br == br and dr.same_bits(w, want), (pd, d, np.flatnonzero(w != want)[:8])
            arms.add(br)
        assert arms == {0, 1, 2}


def test_a_nan_row_inside_the_large_cone_gives_nan_margins_and_the_last_arm():
    hk, cones, _ = _handle("mixed_large")
    r = cones.rng_cones[1]                       # the PSD(65) cone
    v = _placed(cones, np.random.default_rng(9), 1, -0.7, 1.0)      # without the NaN: arm 0
    row = r.start + 4
    v[row] = float("nan")
    v[cones.rng_cones[0].start] = -0.0           # a Nonnegative row: the zero shift makes it +0.0
    with _Timeout(30):
        for pd in ("primal", "dual"):
            a, b = hk.h.cone_margins(v, pd)
            assert math.isnan(a) and math.isnan(b)
            w, mn, pos, tg, br = hk.h.cone_shift_to_interior(v, pd)
            assert math.isnan(mn) and br == 2
            ref_mn, ref_pos = dr.margins64(cones, v)
            assert math.isnan(ref_mn) and math.isnan(ref_pos) == math.isnan(pos)
            assert math.isnan(tg) == math.isnan(dr.target_of(ref_pos, cones.degree))
            want, want_br = dr.apply_shift(cones, v, pd, mn, tg)
            assert want_br == 2 and dr.same_bits(w, want)
            assert math.isnan(w[row]) and int(np.sum(np.isnan(w))) == 1
            assert w[cones.rng_cones[0].start] == 0.0 and not np.signbit(w[cones.rng_cones[0].start])


# ---- 5. the fused call ------------------------------------------------------------------------------------------------------------------------

@BOTH_P
def test_fused_call_matches_the_host_default_start_on_the_mixed_large_set(pzero):
    with _Timeout(120):
        hk, cones, prob = _handle("mixed_large", pzero)
        twin, tcones, _ = _handle("mixed_large", pzero)
        Pt, q, A, b = prob
        m, n = A.shape
        xzs = hk.device_buffer(n + 2 * m)
        hk.set_problem_vectors(q, b)
        before = dict(hipkkt.TRAFFIC)
        ok, scal, steps = _fused(hk, xzs)
        assert hipkkt.TRAFFIC["h2d_bytes"] == before["h2d_bytes"] and hipkkt.TRAFFIC["d2h_bytes"] - before["d2h_bytes"] == 64
        assert ok
        got = xzs.download()
        x, z, s, hsteps, hok = _host_default_start(twin, tcones, prob)
        assert hok
        assert (scal[0], int(scal[1])) == (twin.diagonal_regularizer, twin.last_nreg)        # eps, regularised pivots
        assert list(steps) == hsteps, (list(steps), hsteps)                                    # refinement steps
        # the device's margins against 50 digits of the host's unshifted (s, z)
        for what, v, o in (("s", s, 2), ("z", z, 5)):
            _check_margins(f"mixed_large fused {what}", scal[o], scal[o + 1], dr.margins_mp(tcones, v))
            assert scal[o + 2] == dr.target_of(scal[o + 1], tcones.degree)
        # the host's two shifts with the device's margins: the same bits, all rows
        s_sh, _ = dr.apply_shift(tcones, s, "primal", scal[2], scal[4])
        z_sh, _ = dr.apply_shift(tcones, z, "dual", scal[5], scal[7])
        want = np.concatenate([x, z_sh, s_sh])
        assert dr.same_bits(got, want), (pzero, np.flatnonzero(got != want)[:8], float(np.max(np.abs(got - want))))
        ok2, scal2, steps2 = _fused(hk, xzs)                     # twice in a row: the same bits
        assert ok2 and dr.same_bits(scal2, scal) and list(steps2) == list(steps) and dr.same_bits(xzs.download(), got)
        with pytest.raises(ValueError):
            hk.cone_affine_ds()                                  # the step calls wait for a scaling
        xzs.close()


# ---- 6. the protocol --------------------------------------------------------------------------------------------------------------------------

def test_protocol_of_the_start_enable():
    specs = [T.PSDTriangleConeT(65), T.NonnegativeConeT(2)]
    # refused without hipkkt_step_enable_psd_large: no enable at all, the small enable, a side of 129
    free, _ = tp._handle([T.PSDTriangleConeT(8), T.NonnegativeConeT(2)], 1, flags={})
    with pytest.raises(ValueError, match="step_default_start_enable_psd_large"):
        free.h.step_default_start_enable_psd_large(True)
    free.h.step_enable_psd(True)
    with pytest.raises(ValueError, match="step_default_start_enable_psd_large"):
        free.h.step_default_start_enable_psd_large(True)
    big, _ = tp._handle([T.PSDTriangleConeT(129)], 1, flags={})
    with pytest.raises(ValueError, match="step_default_start_enable_psd_large"):
        big.h.step_default_start_enable_psd_large(True)
    # a plugin with the base flags alone keeps the start with the caller
    hk, cones = tp._handle(specs, 2, flags=dict(LARGE, device_default_start=True))
    assert hk.steps_psd_large and not hk.starts_psd_large and not hk.default_start_on_device
    m = cones.numel
    v = np.random.default_rng(3).standard_normal(m)
    xzs = hk.device_buffer(hk.n + 2 * m)
    hk.h.set_qb(np.ones(hk.n), np.ones(m))
    calls = (hk.h.cone_set_identity_scaling, lambda: hk.h.cone_margins(v, 0), lambda: hk.h.cone_shift_to_interior(v, 1),
             lambda: hk.h.step_default_start_dev(xzs.ptr))
    for call in calls:
        with pytest.raises(ValueError, match="step_default_start_enable_psd_large"):
            call()
    hk.h.step_default_start_enable_psd_large(True)
    for call in calls:
        call()
    first = hk.h.cone_margins(v, 0)
    hk.h.step_default_start_enable_psd_large(False)             # switching off restores the refusal
    for call in calls:
        with pytest.raises(ValueError):
            call()
    hk.h.step_default_start_enable_psd_large(True)
    assert hk.h.cone_margins(v, 0) == first
    hk.h.step_enable_psd_large(True)                            # the step enable clears it
    with pytest.raises(ValueError):
        hk.h.cone_margins(v, 0)
    xzs.close()
