"""The float64 stand-in's Exponential / Power step algebra (julia_standin/cones_nonsym.py) against tests/cone3_reference.py, without a
GPU: the stand-in is what tests/test_gpu_device_step_nonsym.py holds the device against, and its third-order correction was so far
checked only against a central difference at 2e-5.  No code of the HIP library runs.

Points: cone3_reference.regime_set -- 64 Exponential and 64 Power cones (alpha = 0.001, 0.1, 0.101, 0.5, 0.899, 0.9, 0.999 in turn)
per (margin decade, side, scale): central points (Exponential primal points with Wright-omega arguments below the branch at 1 + pi,
above it, and at 20 .. 500; one Power point with s3 = 0), relative margins in [1.5, 6] x {1e-2, 1e-4, 1e-6} on the dual side (correction
and barrier) and on the primal side (barrier), overall scales 1e-6, 1, 1e6.  A bucket = (operation, cone kind, side, decade) holds the
three scales: 192 cases.  Every point must scale under both strategies (asserted, nothing is dropped).

1. Stand-in against the reference's own expressions at 50 digits (`ref_*`).  MEASURED largest error per bucket (printed by the tests;
   the gate is 10 x the recorded value, HOST_ERR in cone3_reference.py; correction: max |eta - ref| / max |ref| per cone, barrier:
   |barrier_dual + barrier_primal - ref| / max(1, |ref|)):

       decade     correction exp  correction pow  barrier exp dual  barrier exp primal  barrier pow dual  barrier pow primal
       central    2.68e-15        1.42e-14        3.05e-16          (same set)          1.38e-15          (same set)
       1e-2       4.44e-13        1.12e-11        3.35e-15          1.01e-13            7.55e-15          2.72e-14
       1e-4       5.22e-09        2.96e-08        9.45e-14          3.66e-12            1.97e-13          4.25e-13
       1e-6       8.06e-05        4.92e-04        6.72e-12          1.13e-10            7.56e-12          2.91e-11

   and the Exponential cone's gradient_primal (max |g - ref| / max |ref|): 5.8e-16 with a central s, 7.93e-13 / 1.73e-10 / 3.04e-09 at
   primal margins 1e-2 / 1e-4 / 1e-6.  The correction loses about eps / margin^2 (u = H_dual^-1 ds through a float64 Cholesky factor of a matrix whose condition grows
   like margin^-2, then cancellation in psi); the barriers lose about eps / margin.  That is conditioning, not a wrong term: the
   definitional layer below agrees with the reference's expressions to 1e-30 at every one of these points.

2. The two layers against each other, on the first cones of every kind per (decade, side, scale): 1e-30 relative wherever the
   reference's expression is exact.  Not exact, and measured instead:
     * the Wright omega ALGORITHM (series or asymptotic start and two corrector steps) against lambertw(e^arg): its truncation error
       reaches 5.9e-14 relative for arguments between 3 and 12 (test_wright_omega_algorithm_against_lambertw); the Exponential primal
       barrier and gradient of the two layers agree up to that truncation, measured at each point's own argument, and to 1e-30 beyond;
     * the Power cone's primal gradient at alpha != 1/2, where the one-sided Newton iteration halts at its closed-form start: the
       distance of that start from the root is printed (1e-6 .. 0.8 relative); at alpha = 1/2 (where the start IS the root) and on
       the branch |s3| <= eps, 1e-30 is asserted (measured: 1.5e-44 at worst)."""
import functools

import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from julia_standin import cones_nonsym as cn
from tests import cone3_reference as c3

LAYERS = 1e-30
DEF_PER_KIND = 4        # cones of every kind per (decade, side, scale) that get the definitional layer


def _pack(H):
    return np.array([H[0, 0], H[0, 1], H[1, 1], H[0, 2], H[1, 2], H[2, 2]])


@functools.lru_cache(maxsize=None)
def _scaled_set(decade, side, scale):
    """the regime set with its host cones scaled (dual strategy; the correction and the barrier do not depend on Hs)"""
    kinds, alphas, s, z = c3.regime_set(decade, side, scale)
    cones = cl.CompositeCone(cl.cones_new_collapsed(c3.regime_specs(kinds, alphas)))
    mu = float(s @ z) / (cones.degree + 1)
    assert mu > 0 and cones.update_scaling(s, z, mu, "dual")
    return kinds, alphas, s, z, cones, mu


SETS = [(d, "dual") for d in c3.DECADES] + [(d, "primal") for d in c3.DECADES if d != "central"]


@pytest.mark.parametrize("decade,side", SETS)
def test_every_point_scales_under_both_strategies(decade, side):
    for scale in c3.SCALES:
        kinds, alphas, s, z, cones, mu = _scaled_set(decade, side, scale)
        assert len(kinds) == 2 * c3.PER_KIND
        for strategy in ("primal_dual", "dual"):
            fresh = cl.CompositeCone(cl.cones_new_collapsed(c3.regime_specs(kinds, alphas)))
            assert fresh.update_scaling(s, z, mu, strategy), (decade, side, scale, strategy)
            for k, (c, r) in enumerate(zip(fresh.cones, fresh.rng_cones)):
                assert c.is_dual_feasible(z[r]) and c.is_primal_feasible(s[r]), (decade, side, scale, k)
                assert cn._chol3_factor(c.H_dual) is not None and cn._chol3_factor(c.Hs) is not None, (decade, side, scale, strategy, k)
                assert np.all(np.isfinite(c.Hs)) and np.all(np.isfinite(c.grad))
        # the margins are what the set is named for
        for k, (kind, a) in enumerate(zip(kinds, alphas)):
            r = slice(3 * k, 3 * k + 3)
            for dual, q in ((True, z[r]), (False, s[r])):
                mg = c3.margin(kind, q, a, dual)
                assert mg is not None and mg > 0
                if decade != "central" and dual == (side == "dual"):
                    assert decade <= mg < 10 * decade, (decade, side, scale, k, mg)
    # one Power point with s3 = 0, outside the first cones of every alpha (which get the definitional layer on the Newton branch)
    assert [k for k in range(c3.PER_KIND, 2 * c3.PER_KIND) if s[3 * k + 2] == 0.0] == ([c3.PER_KIND + len(c3.ALPHAS)] if decade == "central" or side == "dual" else [])
    if decade == "central":
        # Wright-omega arguments on both sides of the branch at 1 + pi, and deep in the interior
        args = [float(c3.exp_omega_argument(s[3 * k:3 * k + 3])) for k in range(c3.PER_KIND)]
        branch = 1.0 + np.pi
        assert sum(a < branch for a in args) >= 8 and sum(branch < a < 12.0 for a in args) >= 8 and sum(a > 20.0 for a in args) >= 8, args


def _report(worst, counts):
    for b in sorted(worst, key=str):
        rec = c3.HOST_ERR.get(b)
        print(f"[cone3 reference] {b}: {counts[b]} cases, max error of the stand-in {worst[b]:.2e} (recorded {rec if rec is None else format(rec, '.2e')})")
    for b, w in worst.items():
        assert counts[b] >= 32, (b, counts[b])
        assert b in c3.HOST_ERR, f"no recorded value for {b}: measured {w:.2e}"
        assert w <= 10.0 * c3.HOST_ERR[b], (b, w, c3.HOST_ERR[b])


@pytest.mark.parametrize("decade", c3.DECADES)
def test_stand_in_correction_against_50_digits_and_the_third_derivative(decade):
    worst, counts, layers = {}, {}, 0.0
    for scale in c3.SCALES:
        kinds, alphas, s, z, cones, mu = _scaled_set(decade, "dual", scale)
        dz, ds = c3.regime_directions(decade, "dual", scale, cones.numel)
        seen = {"exp": 0, "pow": 0}
        for kind, a, c, r in zip(kinds, alphas, cones.cones, cones.rng_cones):
            got = c.higher_correction(ds[r], dz[r])
            ref, u = c3.ref_correction(kind, _pack(c.H_dual), c.z, a, ds[r], dz[r])
            b = c3.bucket("correction", kind, "dual", decade)
            worst[b] = max(worst.get(b, 0.0), c3.correction_error(got, ref))
            counts[b] = counts.get(b, 0) + 1
            if seen[kind] < DEF_PER_KIND or (kind == "pow" and seen[kind] < len(c3.ALPHAS)):      # (every alpha once)
                seen[kind] += 1
                true = c3.def_correction(kind, c.z, a, u, dz[r])
                e = max(float(abs(p - q)) for p, q in zip(ref, true)) / c3.max_abs(true)
                layers = max(layers, e)
                assert e <= LAYERS, (kind, a, decade, scale, e)
    print(f"[cone3 reference] correction, decade {decade}: reference expressions against 1/2 grad^3 f*[u, v]: max relative difference {layers:.2e}")
    _report(worst, counts)


@pytest.mark.parametrize("decade,side", SETS)
def test_stand_in_barrier_against_50_digits_and_the_definitions(decade, side):
    worst, counts, layers, start, omega_trunc, exact = {}, {}, 0.0, {}, 0.0, 0.0
    for scale in c3.SCALES:
        kinds, alphas, s, z, cones, mu = _scaled_set(decade, side, scale)
        seen = {"exp": 0, "pow": 0}
        for kind, a, c, r in zip(kinds, alphas, cones.cones, cones.rng_cones):
            got = c.barrier_dual(z[r]) + c.barrier_primal(s[r])
            assert got == c.compute_barrier(z[r], s[r], np.zeros(3), np.zeros(3), 0.0)
            ref = c3.ref_barrier(kind, z[r], s[r], a)
            b = c3.bucket("barrier", kind, side, decade)
            worst[b] = max(worst.get(b, 0.0), c3.barrier_error(got, ref))
            counts[b] = counts.get(b, 0) + 1
            if kind == "exp":
                gref = c3.ref_exp_gradient_primal(s[r])
                b = c3.bucket("gradient_primal", kind, side, decade)
                worst[b] = max(worst.get(b, 0.0), c3.correction_error(c.gradient_primal(s[r]), gref))
                counts[b] = counts.get(b, 0) + 1
            s3_zero = kind == "pow" and s[r][2] == 0.0
            if seen[kind] < (DEF_PER_KIND if kind == "exp" else len(c3.ALPHAS)) or s3_zero:      # (every alpha once on the Newton branch)
                seen[kind] += 0 if s3_zero else 1
                # the dual barrier as a function, everywhere
                dref = c3.ref_exp_barrier_dual(z[r]) if kind == "exp" else c3.ref_pow_barrier_dual(z[r], a)
                ddef = c3.def_barrier_dual(kind, z[r], a)
                e = float(abs(dref - ddef) / max(1, abs(ddef)))
                layers = max(layers, e)
                assert e <= LAYERS, (kind, a, decade, side, scale, e)
                if kind == "exp":
                    # exact up to the truncation of the omega algorithm AT THIS ARGUMENT (measured here against lambertw), which the
                    # barrier sees through d barrier / d log(omega) = (omega + 1) / (omega - 1) and the gradient through at most
                    # omega / (omega - 1) + 1 per entry; the factor 2 covers the second-order term
                    arg = c3.exp_omega_argument(s[r])
                    om = c3.def_wright_omega(arg)
                    trunc = float(abs(c3.ref_wright_omega(arg) - om) / om)
                    omega_trunc = max(omega_trunc, trunc)
                    amp = float((om + 1) / (om - 1))
                    e = float(abs(c3.ref_exp_barrier_primal(s[r]) - c3.def_exp_barrier_primal(s[r])))
                    assert e <= 2.0 * amp * trunc + LAYERS, (decade, side, scale, e, amp, trunc)
                    gdef = c3.def_exp_gradient_primal(s[r])
                    e = max(float(abs(p - q)) for p, q in zip(gref, gdef)) / c3.max_abs(gdef)
                    assert e <= 2.0 * (amp + 1.0) * trunc + LAYERS, (decade, side, scale, e, amp, trunc)
                else:
                    b_def = c3.def_pow_barrier_primal(s[r], a)
                    e = float(abs(c3.ref_pow_barrier_primal(s[r], a) - b_def) / max(1, abs(b_def)))
                    g_ref, g_def = c3.ref_pow_gradient_primal(s[r], a), c3.def_pow_gradient_primal(s[r], a)
                    eg = max(float(abs(p - q)) for p, q in zip(g_ref, g_def)) / c3.max_abs(g_def)
                    if a == 0.5 or s3_zero:
                        # exact: at alpha = 1/2 the closed-form start of the Newton iteration IS the root, and |s3| <= eps takes the branch
                        # without an iteration
                        exact = max(exact, eg, e)
                        assert eg <= LAYERS and e <= LAYERS, (a, decade, side, scale, eg, e)
                    else:
                        start[a] = max(start.get(a, (0.0, 0.0)), (eg, e))
    print(f"[cone3 reference] barrier, decade {decade}, {side} side: dual barriers, expressions against the functions: {layers:.2e}; truncation of the omega "
          f"algorithm at these points up to {omega_trunc:.1e}; Power "
          f"primal gradient / barrier at alpha = 1/2 and at s3 = 0: {exact:.1e}; Power "
          f"primal gradient / barrier, reference's halted Newton against the root, per alpha (gradient relative / barrier over max(1, |barrier|)): "
          + ", ".join(f"{a}: {eg:.1e} / {e:.1e}" for a, (eg, e) in sorted(start.items())))
    _report(worst, counts)


def test_wright_omega_algorithm_against_lambertw():
    """The truncation error of the reference's algorithm, evaluated at 50 digits.  MEASURED: below 1e-17 for arguments up to 3 and from
    12 on, but up to 5.9e-14 between (5.2e-16 at 3.5, 1.5e-14 at 4, 5.5e-14 just above the branch at 1 + pi, 5.7e-14 at 5, 2.2e-14 at 6,
    1.4e-15 at 8): two corrector steps do not reach double precision from either start there, and the asymptotic start lacks the factor
    1 / z of its last term (coneops_expcone.jl:451 does not store the product).  That is the reference's algorithm, which the stand-in
    and the kernels restate as it is; an evaluation at 50 digits is deterministic, so the gates are the measured ceilings themselves."""
    branch = float(1 + c3.mp.pi)
    grid = [0.0, 1e-12, 1e-6, 0.5, 1.0 - 1e-9, 1.0, 1.0 + 1e-9, 2.0, 3.0, 4.0, np.nextafter(branch, 0.0), np.nextafter(branch, 9.0), 4.2,
            5.0, 8.0, 20.0, 100.0, 600.0] + list(np.linspace(0.0, 12.0, 97))
    worst = 0.0
    for a in grid:
        a = c3.mpf(float(a))
        got, true = c3.ref_wright_omega(a), c3.def_wright_omega(a)
        worst = max(worst, float(abs(got - true) / true))
        assert float(abs(got - true) / true) <= (1e-13 if 3.0 <= a <= 12.0 else 1e-17), float(a)
    print(f"[cone3 reference] Wright omega algorithm against lambertw(e^arg): max relative truncation error {worst:.2e}")
    # the stand-in's float64 evaluation of the same algorithm
    w64 = max(float(abs(c3.mpf(cn._wright_omega(float(a))) - c3.def_wright_omega(c3.mpf(float(a)))) / c3.def_wright_omega(c3.mpf(float(a)))) for a in grid)
    print(f"[cone3 reference] the stand-in's _wright_omega against lambertw(e^arg): max relative error {w64:.2e}")
    assert w64 <= 1e-13 + 8 * float(c3.EPS)


def test_constructed_directions_cross_where_they_say():
    """boundary_direction: q + alpha d is inside exactly below alpha_cross, on both sides of both cones"""
    rng = np.random.default_rng(3)
    for kind, a in (("exp", 0.0), ("pow", 0.5), ("pow", 0.101), ("pow", 0.999)):
        for dual in (True, False):
            q = c3.central_point(kind, a, dual, rng)
            for cross in (0.93, 1e-4):
                d = c3.boundary_direction(kind, q, a, dual, cross)
                for f, want in ((0.5, True), (0.999, True), (1.001, False), (1.2, False)):
                    assert c3.inside(kind, q + f * cross * d, a, dual) == want, (kind, a, dual, cross, f)
    a0 = 1.0 - c3.SQRT_EPS64
    assert c3.grid_alpha(a0, 0.8, 2) == a0 * 0.8 * 0.8
    assert c3.grid_alpha(a0, 0.8, 7) < c3.crossing_between(a0, 0.8, 7) < c3.grid_alpha(a0, 0.8, 6)
