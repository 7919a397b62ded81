"""tests/genpow_reference.py checked on the CPU: the two layers of the 50-digit reference agree where the reference's expression is
exact, the generated points have the margins they claim, and the float64 stand-in (julia_standin/cones_nonsym.py GenPowerCone) is
still under the recorded HOST_ERR per bucket -- the numbers that tests/test_gpu_genpow_step.py holds the device to ten times of.

Bounds chosen here, with their reasons:
  * LAYERS = 1e-30: both layers run at 50 digits; what they share is the input, so they differ by rounding at 1e-50 times condition
    numbers of at most 1e8 (the smallest margin) -- twelve orders below the bound.
  * The Newton branch of gradient_primal! is NOT exact and is only measured: the reference halts once |dx / x| < sqrt(eps) without
    taking that step, and it also halts on the first step that is not positive ("one-sided").  Away from the boundary that leaves a
    relative error of the gradient of up to 1e-9 and of the barrier below 1e-18 (second order: the barrier is stationary in g at the
    true gradient); at primal margins of 1e-7 and below the closed-form start of :446 can lie to the right of the root, the iteration
    halts after one trip and the gradient is off by up to 13 % (barrier: 7e-3).  Both layers are the reference's: HOST_ERR and the
    device gates are measured against the `ref_*` layer, which halts where the reference halts.  Printed per run."""
import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
from tests import genpow_reference as gp

LAYERS = 1e-30


def test_generated_points_have_the_margins_they_claim():
    seen = {}
    for b, shape, alpha, s, z in gp.regime_cases():
        assert len(alpha) == shape[0] and s.size == z.size == shape[0] + shape[1]
        assert abs(float(np.sum(alpha)) - 1.0) < 1e-12
        mz, ms = gp.margin(alpha, z, True), gp.margin(alpha, s, False)
        assert mz is not None and ms is not None and mz > 0 and ms > 0, (b, shape)
        c = gp.host_cone(alpha, shape[1])
        assert c.is_dual_feasible(z) and c.is_primal_feasible(s), (b, shape)
        if b[1] in gp.SIDES:
            decade = float(b[2])
            near, far = (mz, ms) if b[1] == "dual" else (ms, mz)
            assert 1.5 * decade * (1 - 1e-6) <= near <= 6.0 * decade * (1 + 1e-6), (b, shape, near)
            assert far > 0.2, (b, shape, far)
        elif b[2] == "w0":
            assert np.all(s[shape[0]:] == 0.0) and gp.ref_gradient_primal(alpha, gp.V(s))[1] == -1
        else:
            assert 0.0 < np.linalg.norm(s[shape[0]:]) <= 1e-7 and gp.ref_gradient_primal(alpha, gp.V(s))[1] >= 1
        seen[b] = seen.get(b, 0) + 1
    assert len(seen) == 2 * len(gp.DECADES) + 3 and all(v == len(gp.SHAPES) * gp.PER_SHAPE for v in seen.values())


def test_the_two_layers_agree_where_the_reference_is_exact():
    worst_dual = worst_w0 = worst_newton = worst_newton_b = 0.0
    one_trip = 0
    for b, shape, alpha, s, z in gp.regime_cases():
        if shape[0] + shape[1] > 64:      # (the definitions add nothing on the long shapes)
            continue
        zz, ss = gp.V(z), gp.V(s)
        bd, dd = gp.ref_barrier_dual(alpha, zz), gp.def_barrier_dual(alpha, zz)
        e = float(abs(bd - dd) / max(1, abs(dd)))
        worst_dual = max(worst_dual, e)
        assert e <= LAYERS, (b, shape, e)
        check = shape[0] + shape[1] <= 8      # grad f*(-g) = -s by differentiation on the short shapes
        g_ref, trips = gp.ref_gradient_primal(alpha, ss)
        g_def = gp.def_gradient_primal(alpha, ss, check)
        bp_ref, bp_def = gp.ref_barrier_primal(alpha, ss), gp.def_barrier_primal(alpha, ss, False)
        eg = max(float(abs(p - q)) for p, q in zip(g_ref, g_def)) / max(float(abs(q)) for q in g_def)
        eb = float(abs(bp_ref - bp_def) / max(1, abs(bp_def)))
        if trips == -1:
            worst_w0 = max(worst_w0, eg, eb)
            assert eg <= LAYERS and eb <= LAYERS, (b, shape, eg, eb)
        else:
            assert 1 <= trips < 100, (b, shape, trips)
            worst_newton, worst_newton_b = max(worst_newton, eg), max(worst_newton_b, eb)
            one_trip += trips == 1
    print(f"[genpow reference] layers: barrier_dual {worst_dual:.2e}, branch norm_r <= eps {worst_w0:.2e}; what the halting rule leaves on "
          f"the Newton branch: gradient {worst_newton:.2e}, barrier {worst_newton_b:.2e}; "
          f"{one_trip} points on which the iteration halts after one trip")


def test_feasibility_of_the_stand_in_matches_50_digits_on_the_generated_points():
    for b, shape, alpha, s, z in gp.regime_cases():
        c = gp.host_cone(alpha, shape[1])
        assert c.is_dual_feasible(z) == gp.inside(alpha, z, True) and c.is_primal_feasible(s) == gp.inside(alpha, s, False)
        assert not c.is_dual_feasible(-z) and not gp.inside(alpha, -z, True)


def measure_host_err():
    worst, counts = {}, {}
    for b, shape, alpha, s, z in gp.regime_cases():
        c = gp.host_cone(alpha, shape[1])
        zero = np.zeros(c.dim)
        with np.errstate(all="ignore"):      # (the 'eps' bucket: the reference's expression divides by zero, see HOST_ERR)
            got = c.compute_barrier(z, s, zero, zero, 0.0)
        e = gp.barrier_error(got, gp.ref_barrier(alpha, z, s))
        worst[b] = max(worst.get(b, 0.0), e)
        counts[b] = counts.get(b, 0) + 1
    return worst, counts


def test_stand_in_barrier_is_under_the_recorded_error():
    worst, counts = measure_host_err()
    for b in sorted(worst, key=str):
        rec = gp.HOST_ERR.get(b)
        print(f"[genpow reference] {b}: {counts[b]} cases, max error of the stand-in {worst[b]:.2e} (recorded {rec if rec is None else format(rec, '.2e')})")
    for b, w in worst.items():
        assert b in gp.HOST_ERR, f"no recorded value for {b}: measured {w:.2e}"
        assert w <= gp.HOST_ERR[b], (b, w, gp.HOST_ERR[b])
    assert set(gp.HOST_ERR) == set(worst)


def test_mul_hs_of_the_stand_in_is_within_the_dot_gate():
    """the stand-in's mul_Hs against 50 digits from its own slot: 1e-13 of the propagated sum of absolute terms per row"""
    for shape in gp.SHAPES:
        alpha, s, z = gp.regime_points(shape, "dual", 1e-2, 0)
        c = gp.host_cone(alpha, shape[1])
        assert c.update_scaling(s, z, 0.37)
        slot = np.concatenate([c.grad, c.d1, [c.d2], c.p, c.q, c.r])
        x = np.random.default_rng(shape[0]).standard_normal(c.dim)
        y = np.zeros(c.dim)
        c.mul_Hs(y, x, None)
        ref, terms = gp.ref_mul_hs(slot, shape[0], shape[1], c.mu, x)
        for i in range(c.dim):
            assert abs(gp.mpf(float(y[i])) - ref[i]) <= 1e-13 * terms[i], (shape, i)


@pytest.mark.parametrize("dual", [True, False], ids=["dual", "primal"])
def test_constructed_directions_cross_where_they_say(dual):
    rng = np.random.default_rng(5)
    a0 = 1.0 - gp.SQRT_EPS64
    for shape in gp.SHAPES[:4]:
        alpha = gp.shape_alpha(shape[0])
        q = gp.central_point(alpha, shape[1], dual, rng)
        for k in (1, 3):
            d = gp.boundary_direction(alpha, q, dual, gp.crossing_between(a0, 0.8, k))
            acc, rej = gp.grid_alpha(a0, 0.8, k), gp.grid_alpha(a0, 0.8, k - 1)
            m_acc, m_rej = gp.margin(alpha, gp.moved(q, d, acc), dual), gp.margin(alpha, gp.moved(q, d, rej), dual)
            assert m_acc >= 1e-3 and m_rej <= -1e-3, (shape, k, m_acc, m_rej)
        for through_norm in (False, True):
            d = gp.leaving_direction(alpha, q, 1e-4, through_norm)
            for a in (1.0, 1e-2, 1e-4, 5e-5):
                assert not gp.inside(alpha, gp.moved(q, d, a), dual), (shape, through_norm, a)
