"""The device-resident interior-point step for Generalized Power cones on the GPU (step_genpow.hip, hipkkt_step_enable_genpow): the
granular calls after a Dual scaling, against the 50-digit reference of tests/genpow_reference.py.  The reference takes the resident
slot [grad | d1 | d2 | p | q | r] (the scaling's output vector) and the resident (s, z) as exact inputs, so the scaling's error is not
charged to the step.

Gates:
  * affine_ds, ds_from_dz_offset, combined_ds_shift on Generalized Power rows: `==` (row copies; grad sigma_mu is one rounding);
    rows of every other kind: bit for bit what a handle without the Generalized Power cones gives for the same rows;
  * mul_Hs: per row 1e-13 (SUM_TOL, the project's dot gate) of the first-order propagated sum of absolute terms of the three dots
    and the row expression, against 50 digits;
  * step length: constructed directions; the accepted and the last rejected grid point of the binding cone and every other cone at
    alpha0 have a relative margin >= 1e-3 at 50 digits (asserted), so the device's alpha is `==` alpha0 step^k by repeated
    multiplication, or 0; nothing is excluded;
  * barrier of single-cone handles by regime: <= 10 x genpow_reference.HOST_ERR[bucket] against 50 digits;
  * barrier of cone sets: 1e-10 max(1, sum |terms|) for the barrier, 1e-13 sum |terms| for the shifted dot, against the stand-in."""
import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd.kktsolver import HipKKTSolver
from julia_standin import cones_nonsym as cn
from tests import cone3_reference as c3
from tests import fixtures as fx
from tests import genpow_reference as gp
from tests.step_support import STEP_FLAGS, SUM_TOL, _check_barrier, _prep, _problem, _Timeout

pytestmark = pytest.mark.gpu

GENPOW = dict(device_step=True, device_step_nonsymmetric=True, device_step_genpower=True, **STEP_FLAGS)
ALPHA0 = 1.0 - gp.SQRT_EPS64
MARGIN = 1e-3


def _is_gp(c):
    return isinstance(c, cn.GenPowerCone)


def _handle(specs, seed, step=0.8, amin=1e-4, flags=GENPOW):
    Pt, A, cones = _prep(_problem(specs, seed))
    m, n = A.shape
    st = cl.Settings(linesearch_backtrack_step=step, min_terminate_step_length=amin, **flags)
    cones.use_settings(st)
    hk = HipKKTSolver(Pt, A, cones, m, n, st)
    return hk, cones, st


def _scale(hk, cones, s, z, mu=None):
    """the Dual scaling on the device; the host cones adopt the device's slots -> (mu, the output vector)"""
    mu = float(s @ z) / (cones.degree + 1) if mu is None else mu
    assert mu > 0
    ok, _, _, _, nonsym = hk.h.update_scaling_ex(s, z, mu, 1)
    assert ok
    off = 0
    for c, r in zip(cones.cones, cones.rng_cones):
        if hasattr(c, "adopt_scaling"):
            k = c.scaling_slot_len
            c.adopt_scaling(nonsym[off:off + k], z[r], mu)
            off += k
    assert off == len(nonsym)
    return mu, nonsym


def _slots(cones, nonsym):
    """{cone index: its slot} of the Generalized Power cones"""
    off, out = 0, {}
    for k, c in enumerate(cones.cones):
        if hasattr(c, "adopt_scaling"):
            n = c.scaling_slot_len
            if _is_gp(c):
                out[k] = nonsym[off:off + n]
            off += n
    return out


def _mixed_specs():
    A = gp.shape_alpha
    return [gp.genpow_spec(A(3), 2), cl.ExponentialConeT(), cl.PowerConeT(0.3), gp.genpow_spec(A(2), 1), cl.SecondOrderConeT(4),
            cl.NonnegativeConeT(3), gp.genpow_spec(A(65), 2), cl.ZeroConeT(2), cl.PowerConeT(0.7), gp.genpow_spec(A(2, 1), 3)]


def _many_specs():
    return [gp.genpow_spec(gp.shape_alpha(2, k % 7), 1) for k in range(300)]


def _only_specs():
    return [gp.genpow_spec(gp.shape_alpha(d1, 2), d2) for d1, d2 in ((2, 1), (3, 2), (64, 64), (2, 130))]


SETS = {"mixed": _mixed_specs, "many": _many_specs, "genpow_only": _only_specs}
SETS.update({f"single_{d1}_{d2}": (lambda d1=d1, d2=d2: [gp.genpow_spec(gp.shape_alpha(d1), d2)]) for d1, d2 in gp.SHAPES})


def _points(cones, rng):
    """central (s, z): the Generalized Power members from genpow_reference.central_point (|w| > 0, margins 0.3 .. 0.9), the others from
    the fixture"""
    s, z, _ = fx.scale_cones_nonsymmetric(cones, rng, "dual")
    for c, r in zip(cones.cones, cones.rng_cones):
        if _is_gp(c):
            s[r] = gp.central_point(c.alpha, c.dim2, False, rng)
            z[r] = gp.central_point(c.alpha, c.dim2, True, rng)
    return s, z


def _scaled_set(name, seed, step=0.8, amin=1e-4):
    hk, cones, st = _handle(SETS[name](), seed, step, amin)
    assert hk.steps_on_device and hk.steps_nonsymmetric
    rng = np.random.default_rng(700 + seed)
    s, z = _points(cones, rng)
    mu, nonsym = _scale(hk, cones, s, z)
    return hk, cones, st, s, z, mu, nonsym, rng


# ---- row operations and mul_Hs -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SETS))
def test_row_operations_and_mul_hs(name):
    with _Timeout(60):
        hk, cones, st, s, z, mu, nonsym, rng = _scaled_set(name, 3)
        m = cones.numel
        dz, ds, v = rng.standard_normal(m), rng.standard_normal(m), rng.standard_normal(m)
        sm = 0.3 * mu
        got = {"affine_ds": hk.cone_affine_ds(), "ds_from_dz_offset": hk.cone_ds_from_dz_offset(v), "mul_Hs": hk.cone_mul_hs(v),
               "combined_ds_shift": hk.cone_combined_ds_shift(dz, ds, sm)}
        slots = _slots(cones, nonsym)
        worst = 0.0
        for k, (c, r) in enumerate(zip(cones.cones, cones.rng_cones)):
            if not _is_gp(c):
                continue
            assert np.array_equal(got["affine_ds"][r], s[r]) and np.array_equal(got["ds_from_dz_offset"][r], v[r])
            grad = gp.split_slot(slots[k], c.dim1, c.dim2)["grad"]
            assert np.array_equal(got["combined_ds_shift"][r], grad * sm), k
            if name == "many" and k % 37:      # (the 50-digit product for a sample of the 300 equal-shaped cones)
                continue
            ref, terms = gp.ref_mul_hs(slots[k], c.dim1, c.dim2, mu, v[r])
            for i in range(c.dim):
                e = float(abs(gp.mpf(float(got["mul_Hs"][r][i])) - ref[i]))
                worst = max(worst, e / terms[i])
                assert e <= SUM_TOL * terms[i], (name, k, i, e, terms[i])
        print(f"[genpow rows {name}] mul_Hs: max |y - ref| / sum |terms| = {worst:.2e} (gate {SUM_TOL:.0e})")
        # the rows of every other kind: a handle without the Generalized Power cones, scaled at the same rows with the same mu
        rest = [(c, r) for c, r in zip(cones.cones, cones.rng_cones) if not _is_gp(c)]
        if rest:
            specs = [sp_ for sp_, c in zip(SETS[name](), cones.cones) if not _is_gp(c)]
            rows = np.concatenate([np.arange(r.start, r.stop) for _, r in rest])
            tw, tcones, _ = _handle(specs, 93, flags=dict(device_step=True, device_step_nonsymmetric=True, **STEP_FLAGS))
            assert tw.steps_on_device and tw.steps_nonsymmetric
            assert tw.h.update_scaling_ex(s[rows], z[rows], mu, 1)[0]
            twin = {"affine_ds": tw.cone_affine_ds(), "ds_from_dz_offset": tw.cone_ds_from_dz_offset(v[rows]), "mul_Hs": tw.cone_mul_hs(v[rows]),
                    "combined_ds_shift": tw.cone_combined_ds_shift(dz[rows], ds[rows], sm)}
            for k in twin:
                assert np.array_equal(got[k][rows], twin[k]), k


# ---- step length -------------------------------------------------------------------------------------------------------------------------

def _margin_of(c, q, dual):
    if _is_gp(c):
        return gp.margin(c.alpha, q, dual)
    kind = "exp" if isinstance(c, cn.ExponentialCone) else "pow"
    return c3.margin(kind, [float(v) for v in q], getattr(c, "alpha", 0.0), dual)


def _boundary(c, q, dual, cross):
    if _is_gp(c):
        return gp.boundary_direction(c.alpha, q, dual, cross)
    kind = "exp" if isinstance(c, cn.ExponentialCone) else "pow"
    return c3.boundary_direction(kind, q, getattr(c, "alpha", 0.0), dual, cross)


def _moved(q, d, a):
    return [float(v) for v in gp.moved(q, d, a)]      # (rounded once more: far below the margins asserted)


def _assert_rest_at_alpha0(cones, s, z):
    """with a zero direction a cone stays at its point: every non-symmetric cone has a margin >= 1e-3 there"""
    for c, r in zip(cones.cones, cones.rng_cones):
        if getattr(c, "is_symmetric", True):
            continue
        for dual, q in ((True, z[r]), (False, s[r])):
            mg = _margin_of(c, q, dual)
            assert mg is not None and mg >= MARGIN, (type(c).__name__, dual, mg)


def _bind_and_check(hk, cones, s, z, k, dual, grid_k, step, amin):
    """the cone k binds on the given side so that grid point grid_k is the first inside -> the device's step length"""
    c, r = cones.cones[k], cones.rng_cones[k]
    q = (z if dual else s)[r]
    d = _boundary(c, q, dual, gp.crossing_between(ALPHA0, step, grid_k))
    acc, rej = gp.grid_alpha(ALPHA0, step, grid_k), gp.grid_alpha(ALPHA0, step, grid_k - 1)
    m_acc, m_rej = _margin_of(c, _moved(q, d, acc), dual), _margin_of(c, _moved(q, d, rej), dual)
    assert m_acc is not None and m_acc >= MARGIN and m_rej is not None and m_rej <= -MARGIN, (k, dual, grid_k, m_acc, m_rej)
    full = np.zeros(cones.numel)
    full[r] = d
    zero = np.zeros(cones.numel)
    got = hk.cone_step_length(full, zero, 1.0) if dual else hk.cone_step_length(zero, full, 1.0)
    want = acc if acc >= amin else 0.0
    assert got == (want, want), (k, type(c).__name__, dual, grid_k, got, want)
    return got


@pytest.mark.parametrize("name", ["mixed", "genpow_only", "single_2_1", "single_64_64", "single_65_65", "single_130_3", "single_2_130"])
def test_step_length_is_the_grid_point_of_the_binding_cone(name):
    with _Timeout(60):
        hk, cones, st, s, z, mu, nonsym, rng = _scaled_set(name, 4)
        _assert_rest_at_alpha0(cones, s, z)
        zero = np.zeros(cones.numel)
        assert hk.cone_step_length(zero, zero, 1.0) == (ALPHA0, ALPHA0)
        assert hk.cone_step_length(zero, zero, 0.4) == (0.4, 0.4)
        n = 0
        for k, c in enumerate(cones.cones):
            if getattr(c, "is_symmetric", True):
                continue
            for dual in (True, False):
                for grid_k in (1, 2, 7):
                    _bind_and_check(hk, cones, s, z, k, dual, grid_k, 0.8, 1e-4)
                    n += 1
        print(f"[genpow step length {name}] {n} constructed decisions, all == alpha0 step^k; none excluded")


def test_step_length_is_the_minimum_over_more_than_256_cones():
    with _Timeout(60):
        hk, cones, st, s, z, mu, nonsym, rng = _scaled_set("many", 5)
        _assert_rest_at_alpha0(cones, s, z)
        for k, dual, grid_k in ((0, True, 3), (255, False, 2), (256, True, 5), (299, False, 4)):
            _bind_and_check(hk, cones, s, z, k, dual, grid_k, 0.8, 1e-4)
        # two cones bind at different grid points: the deeper one decides
        full = np.zeros(cones.numel)
        for k, grid_k in ((10, 2), (290, 6)):
            r = cones.rng_cones[k]
            full[r] = _boundary(cones.cones[k], z[r], True, gp.crossing_between(ALPHA0, 0.8, grid_k))
        want = gp.grid_alpha(ALPHA0, 0.8, 6)
        assert hk.cone_step_length(full, np.zeros(cones.numel), 1.0) == (want, want)


def _deepest(step, amin):
    a, k = ALPHA0, 0
    while True:
        nxt = a * step
        if nxt < amin:
            return k
        a, k = nxt, k + 1


@pytest.mark.parametrize("step,amin", [(0.8, 1e-4), (0.5, 1e-3)])
def test_trip_count_reaches_the_deepest_grid_point(step, amin):
    with _Timeout(60):
        hk, cones, st, s, z, mu, nonsym, rng = _scaled_set("mixed", 6, step, amin)
        K = _deepest(step, amin)
        assert K == {(0.8, 1e-4): 41, (0.5, 1e-3): 9}[(step, amin)]
        deepest = gp.grid_alpha(ALPHA0, step, K)
        assert deepest >= amin > deepest * step
        for k in (0, 6):      # a short and a long Generalized Power cone
            for dual in (True, False):
                got = _bind_and_check(hk, cones, s, z, k, dual, K, step, amin)
                assert got == (deepest, deepest)
                got = _bind_and_check(hk, cones, s, z, k, dual, K + 1, step, amin)      # first inside below alpha_min
                assert got == (0.0, 0.0)


@pytest.mark.parametrize("name", ["single_3_2", "single_65_65", "mixed"])
def test_directions_that_leave_the_cone_never_trap(name):
    with _Timeout(60):
        hk, cones, st, s, z, mu, nonsym, rng = _scaled_set(name, 7)
        k = next(i for i, c in enumerate(cones.cones) if _is_gp(c))
        c, r = cones.cones[k], cones.rng_cones[k]
        zero = np.zeros(cones.numel)
        for dual, q in ((True, z), (False, s)):
            for through_norm in (False, True):
                d = zero.copy()
                d[r] = gp.leaving_direction(c.alpha, q[r], 1e-4, through_norm)
                got = hk.cone_step_length(d, zero, 1.0) if dual else hk.cone_step_length(zero, d, 1.0)
                assert got == (0.0, 0.0), (dual, through_norm, got)
                ref = c.step_length(d[r] if dual else zero[r], zero[r] if dual else d[r], z[r], s[r], ALPHA0, st)
                assert min(ref) == 0.0
                bars, _ = hk.cone_barrier(d, zero, [1.0, 0.5]) if dual else hk.cone_barrier(zero, d, [1.0, 0.5])
                if dual or not through_norm:      # (the stand-in's primal barrier outside through |w| is whatever its Newton start gives)
                    assert all((not np.isfinite(b)) or abs(b) > 1e300 for b in bars), (dual, through_norm, bars)
        nan = zero.copy()
        nan[r] = np.nan
        assert hk.cone_step_length(nan, zero, 1.0) == (0.0, 0.0) and hk.cone_step_length(zero, nan, 1.0) == (0.0, 0.0)
        bars, _ = hk.cone_barrier(nan, zero, [0.5])
        assert not np.isfinite(bars[0]) or abs(bars[0]) > 1e300
        assert np.array_equal(hk.cone_affine_ds()[r], s[r])      # the handle still serves


# ---- barrier, single-cone handles, by regime -----------------------------------------------------------------------------------------------

_REFERENCE = {}


def _reference_barriers():
    """ref_barrier of every regime case, computed once"""
    if not _REFERENCE:
        for i, (b, shape, alpha, s, z) in enumerate(gp.regime_cases()):
            _REFERENCE[i] = gp.ref_barrier(alpha, z, s)
    return _REFERENCE


@pytest.mark.parametrize("side", ["dual", "primal", "unit"])
def test_barrier_of_single_cones_by_regime(side):
    with _Timeout(120):
        refs = _reference_barriers()
        handles, worst = {}, {}
        for i, (b, shape, alpha, s, z) in enumerate(gp.regime_cases()):
            if b[1] != side:
                continue
            key = (shape, tuple(alpha))
            if key not in handles:
                handles[key] = _handle([gp.genpow_spec(alpha, shape[1])], 11)
            hk, cones, st = handles[key]
            _scale(hk, cones, s, z)
            zero = np.zeros(cones.numel)
            bars, dots = hk.cone_barrier(zero, zero, [0.0])
            e = gp.barrier_error(bars[0], refs[i])
            worst[b] = max(worst.get(b, 0.0), e)
            assert dots[0] == pytest.approx(float(s @ z), rel=1e-13)
        for b in sorted(worst, key=str):
            allow = 10.0 * gp.HOST_ERR[b]
            print(f"[genpow barrier regime] {b}: worst error {worst[b]:.2e}, allowance {allow:.2e}")
        for b, e in worst.items():
            assert e <= 10.0 * gp.HOST_ERR[b], (b, e, gp.HOST_ERR[b])
        assert len(worst) == (3 if side == "unit" else len(gp.DECADES))


# ---- barrier, cone sets ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed", "many", "genpow_only"])
def test_barrier_of_cone_sets(name):
    with _Timeout(60):
        hk, cones, st, s, z, mu, nonsym, rng = _scaled_set(name, 8)
        m = cones.numel
        dz, ds = 0.2 * rng.standard_normal(m) * np.abs(z), 0.2 * rng.standard_normal(m) * np.abs(s)
        a0 = st.max_step_fraction * cones.step_length(dz, ds, z, s, 1.0)[0]
        assert a0 > 0
        alphas = [a0 * st.linesearch_backtrack_step ** k for k in range(8)]
        bars, dots = hk.cone_barrier(dz, ds, alphas)
        _check_barrier(bars, dots, cones, z, s, dz, ds, alphas, f"genpow {name} 8")
        for n in (1, 3):
            b, d = hk.cone_barrier(dz, ds, alphas[2:2 + n])
            assert np.array_equal(b, bars[2:2 + n]) and np.array_equal(d, dots[2:2 + n]), n
        # a candidate outside one Generalized Power cone
        k = max(i for i, c in enumerate(cones.cones) if _is_gp(c))
        c, r = cones.cones[k], cones.rng_cones[k]
        out = np.zeros(m)
        out[r] = gp.leaving_direction(c.alpha, z[r], 1e-4, True)
        bars, _ = hk.cone_barrier(out, np.zeros(m), [1.0, 0.0, 0.5])
        ref = [cones.compute_barrier(z, s, out, np.zeros(m), a) for a in (1.0, 0.0, 0.5)]
        for j in (0, 2):
            assert (not np.isfinite(bars[j])) or abs(bars[j]) > 1e300, bars
            assert (not np.isfinite(ref[j])) or abs(ref[j]) > 1e300, ref
        assert np.isfinite(bars[1]) and abs(bars[1]) < 1e300


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals():
    plain = dict(device_step=True, device_step_nonsymmetric=True, **STEP_FLAGS)
    for make in (fx.basic_qp, fx.basic_exp, fx.basic_sdp):      # symmetric only, Exponential only, PSD
        Pt, A, cones = _prep(make())
        m, n = A.shape
        hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings(**GENPOW))
        with pytest.raises(ValueError):
            hk.h.step_enable_genpow(True, 0.8, 1e-4)
    # a Generalized Power handle without the setting: not enabled, the cone calls refuse; hipkkt_step_enable_cone3 keeps refusing it
    Pt, A, cones = _prep(fx.basic_genpow())
    m, n = A.shape
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings(**plain))
    assert not hk.steps_on_device
    s, z, mu = fx.scale_cones_nonsymmetric(cones, np.random.default_rng(2), "dual")
    assert hk.h.update_scaling_ex(s, z, mu, 1)[0]
    with pytest.raises(ValueError):
        hk.cone_affine_ds()
    with pytest.raises(ValueError):
        hk.h.step_enable_cone3(True, 0.8, 1e-4)
    for step, amin in ((0.0, 1e-4), (1.0, 1e-4), (1.5, 1e-4), (-0.1, 1e-4), (float("nan"), 1e-4), (0.8, 0.0), (0.8, -1.0),
                       (0.8, float("inf")), (0.999999, 1e-4)):
        with pytest.raises(ValueError):
            hk.h.step_enable_genpow(True, step, amin)
    # enabled: a scaling from before the enable does not count; then served; enable = 0 restores the refusal
    hk.h.step_enable_genpow(True, 0.8, 1e-4)
    with pytest.raises(ValueError):
        hk.cone_affine_ds()
    assert hk.h.update_scaling_ex(s, z, mu, 1)[0]
    assert np.array_equal(hk.cone_affine_ds(), s)
    with pytest.raises(ValueError):
        hk.h.step_enable_cone3(True, 0.8, 1e-4)      # still refused, and the enable stays in place
    assert np.array_equal(hk.cone_affine_ds(), s)
    hk.h.step_enable_genpow(False, 0.8, 1e-4)
    assert hk.h.update_scaling_ex(s, z, mu, 1)[0]
    for call in (hk.cone_affine_ds, lambda: hk.cone_mul_hs(np.ones(m)), lambda: hk.cone_step_length(np.ones(m), np.ones(m), 1.0),
                 lambda: hk.cone_barrier(np.ones(m), np.ones(m), [0.5])):
        with pytest.raises(ValueError):
            call()
    # a new registration clears the enable
    hk.h.step_enable_genpow(True, 0.8, 1e-4)
    kinds, alpha = cones.kkt_cone_kinds_ex()
    hk.h.set_cone_types_ex(kinds, alpha)
    assert hk.h.update_scaling_ex(s, z, mu, 1)[0]
    with pytest.raises(ValueError):
        hk.cone_affine_ds()


def test_switching_one_mode_off():
    """The three enables move one step state: what switching one of them off does to a handle another one serves."""
    plain = dict(device_step=True, device_step_nonsymmetric=True, **STEP_FLAGS)
    # Generalized Power: hipkkt_step_enable_cone3(0) takes the enable away as well
    Pt, A, cones = _prep(fx.basic_genpow())
    m, n = A.shape
    assert m <= 8
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings(**plain))
    s, z, mu = fx.scale_cones_nonsymmetric(cones, np.random.default_rng(2), "dual")
    hk.h.step_enable_genpow(True, 0.8, 1e-4)
    assert hk.h.update_scaling_ex(s, z, mu, 1)[0]
    assert np.array_equal(hk.cone_affine_ds(), s)
    hk.h.step_enable_cone3(False, 0.8, 1e-4)
    with pytest.raises(ValueError):
        hk.cone_affine_ds()
    # Exponential: hipkkt_step_enable_psd(0) leaves it alone, hipkkt_step_enable_genpow(0) switches it off
    Pt, A, cones = _prep(fx.basic_exp())
    m, n = A.shape
    assert m <= 8
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings(**plain))
    s, z, mu = fx.scale_cones_nonsymmetric(cones, np.random.default_rng(3), "dual")
    hk.h.step_enable_cone3(True, 0.8, 1e-4)
    assert hk.h.update_scaling_ex(s, z, mu, 1)[0]
    before = hk.cone_affine_ds()
    hk.h.step_enable_psd(False)
    assert np.array_equal(hk.cone_affine_ds(), before)
    hk.h.step_enable_genpow(False, 0.8, 1e-4)
    with pytest.raises(ValueError):
        hk.cone_affine_ds()
    # PSD: the other two leave it alone, hipkkt_step_enable_psd(0) switches it off
    Pt, A, _ = _prep(_problem([cl.PSDTriangleConeT(3), cl.NonnegativeConeT(2)], 4))
    cones = cl.CompositeCone([cl.PSDTriangleConeT(3), cl.NonnegativeConeT(2)])
    m, n = A.shape
    assert m <= 8
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    s, z = fx.scale_cones(cones, np.random.default_rng(4))
    hk.h.step_enable_psd(True)
    hk.h.psd_set_factors(*hk._psd_factors())
    assert hk.h.update_scaling(s, z, cones.cones[0].R.ravel(order="F"))[0]
    before = hk.cone_affine_ds()
    hk.h.step_enable_cone3(False, 0.8, 1e-4)
    assert np.array_equal(hk.cone_affine_ds(), before)
    hk.h.step_enable_genpow(False, 0.8, 1e-4)
    assert np.array_equal(hk.cone_affine_ds(), before)
    hk.h.step_enable_psd(False)
    with pytest.raises(ValueError):
        hk.cone_affine_ds()
