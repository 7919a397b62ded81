"""The device-resident interior-point step for cone sets with Generalized Power members on the GPU, fused and end to end
(hipkkt_step_enable_genpow, Settings.device_step_genpower): the fused calls against the stand-in's kkt_solve on the same plugin and
against the granular calls; the two paths of the IPM end to end; and a shadow run in which the host path drives and the granular device
calls get the same inputs at every iteration.

Gates:
  * fused dx, dz: 1e-10 of the scale (the project's parity gate); alpha exactly what the granular call gives for the same start;
    hipkkt_step_barrier_dev == hipkkt_cone_barrier for the same step;
  * end to end: SOLVED on both paths, objective within 2 max(tol_gap_abs, tol_gap_rel max(1, |obj|)); iterations and bytes per
    iteration are printed, not gated;
  * shadow: Generalized Power combined_ds_shift `==`, mul_Hs within 1e-13 of the propagated sum of absolute terms against 50 digits, at
    every iteration; every step-length call `==` the stand-in's walk of the same grid, except (cone, call) pairs whose decision margin at
    50 digits (accepted or last rejected grid point) is below 1e-8, at most 5 % of the pairs.  The symmetric cones' part of the start
    comes from the device's own kernels on a symmetric-only twin handle (tree sums where a second-order cone binds), as in
    tests/test_gpu_device_step_nonsym.py."""
import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt, problems
from julia_standin import cones_nonsym as cn
from julia_standin import ipm
from julia_standin.cones import SecondOrderCone
from tests import cone3_reference as c3
from tests import fixtures as fx
from tests import genpow_reference as gp
from tests.step_support import PARITY, STEP_FLAGS, SUM_TOL, _check_barrier, _symmetric_twin_handle, _Timeout, _twin_step_length

pytestmark = pytest.mark.gpu

GENPOW = dict(device_step=True, device_step_nonsymmetric=True, device_step_genpower=True, **STEP_FLAGS)
DECISION_MARGIN = 1e-8


def _is_gp(c):
    return isinstance(c, cn.GenPowerCone)


def _mix20():
    return problems.nonsymmetric_mix(n=20, nexp=3, npow=3, ngenpow=3, nn=6, nzero=2, socdim=4, seed=9)


def _mix60():
    return problems.nonsymmetric_mix(n=60, nexp=8, npow=8, ngenpow=8, nn=20, nzero=3, socdim=5, seed=5)


# ---- the fused calls ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,tau", [(5, 0.9), (4, 1e-3)])
def test_fused_steps_and_the_resident_barrier_match_the_granular_calls_and_the_stand_in(seed, tau):
    with _Timeout(60):
        S = cl.Solver(*_mix20(), cl.Settings(**GENPOW))
        assert S._device_step and S.kktsystem.kktsolver.steps_nonsymmetric
        ks, data, cones, v, st = S.kktsystem.kktsolver, S.data, S.cones, S.variables, S.settings
        n, m = data.n, data.m
        rng = np.random.default_rng(70 + seed)
        s, z, _ = fx.scale_cones_nonsymmetric(cones, rng, "dual")
        v.x[:], v.z[:], v.s[:], v.tau, v.kappa = rng.standard_normal(n), z, s, tau, 0.4
        xzs, res = ks.device_buffer(n + 2 * m), ks.device_buffer(3 * n + 2 * m)
        xzs.upload(np.concatenate([v.x, v.z, v.s]))
        r = S.residuals
        ks.residuals_update_dev(xzs, res, v.tau, v.kappa)
        S._residuals_update()
        mu = (r.dot_sz + v.tau * v.kappa) / (cones.degree + 1)
        assert ks.kktsolver_update_scaled(cones, v.s, v.z, mu=mu, strategy="dual")      # the host cones adopt the device's scaling
        exact = np.concatenate([np.arange(q.start, q.stop) for c, q in zip(cones.cones, cones.rng_cones)
                                if not isinstance(c, SecondOrderCone) and not _is_gp(c)])

        def check_step(step, scal, ds_const, rhs_kappa, alpha, dtau, dkappa, fraction, lhs_ref, what):
            dx, dz, ds = step[:n], step[n:n + m], step[n + m:]
            scale = max(1.0, np.max(np.abs(lhs_ref.x)), np.max(np.abs(lhs_ref.z)))
            print(f"[genpow fused {what}] max |dx - ref| / scale {np.max(np.abs(dx - lhs_ref.x)) / scale:.2e}, "
                  f"|dz - ref| / scale {np.max(np.abs(dz - lhs_ref.z)) / scale:.2e}")
            assert np.max(np.abs(dx - lhs_ref.x)) <= PARITY * scale and np.max(np.abs(dz - lhs_ref.z)) <= PARITY * scale, what
            assert abs(dtau - lhs_ref.tau) <= PARITY * max(1.0, abs(lhs_ref.tau)), what
            ref = np.zeros(m)
            cones.mul_Hs(ref, dz, np.zeros(m))
            ref = -(ref + ds_const)
            assert np.array_equal(ds[exact], ref[exact]), what
            assert np.max(np.abs(ds - ref)) <= PARITY * max(1.0, np.max(np.abs(ref))), what      # (tree sums on the other rows)
            assert dkappa == -(rhs_kappa + v.kappa * dtau) / v.tau, what
            a_tau = -v.tau / dtau if dtau < 0 else ipm.FLOATMAX
            a_kap = -v.kappa / dkappa if dkappa < 0 else ipm.FLOATMAX
            start = min(a_tau, a_kap, 1.0)
            comp = ks.cone_step_length(dz, ds, start)
            print(f"[genpow fused {what}] min(alpha_tau, alpha_kappa, 1) = {start!r}, composite {scal[3]!r}, alpha {alpha!r}")
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
        if tau < 0.1:
            assert start_aff < 1.0, "min(alpha_tau, alpha_kappa, 1) was meant to bind in the affine step"
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
            _check_barrier(bars, dots, cones, v.z, v.s, dz, ds, alphas, f"genpow resident step {seed}")
        before = xzs.download()
        ks.kktsolver_step_apply(alpha, xzs)
        assert np.array_equal(ks.h.step_get(), step)
        assert np.array_equal(xzs.download(), before + alpha * step)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------

END_TO_END = {"basic_genpow": fx.basic_genpow, "mix20": _mix20, "mix60": _mix60}


def _solve_counting(prob, **flags):
    solver = cl.Solver(*prob, cl.Settings(**flags))
    for k in hipkkt.TRAFFIC:
        hipkkt.TRAFFIC[k] = 0
    sol = solver.solve()
    it = max(sol.iterations, 1)
    return solver, sol, (hipkkt.TRAFFIC["h2d_bytes"] + hipkkt.TRAFFIC["d2h_bytes"]) / it, 1e3 * solver.info.timers["IP iteration"] / it


@pytest.mark.parametrize("name", list(END_TO_END))
def test_ipm_with_the_genpower_device_step_matches_the_host_path(name):
    prob = END_TO_END[name]()
    with _Timeout(120):
        ref_solver, ref, ref_bytes, ref_ms = _solve_counting(prob, **STEP_FLAGS)
        dev_solver, got, dev_bytes, dev_ms = _solve_counting(prob, **GENPOW)
    assert dev_solver._device_step and dev_solver.kktsystem.kktsolver.steps_nonsymmetric and not ref_solver._device_step
    st = dev_solver.settings
    print(f"[genpow end to end {name}] host path: {ref.status}, {ref.iterations} iterations, {ref_bytes:.0f} bytes / iteration, "
          f"{ref_ms:.3f} ms / iteration; device step: {got.status}, {got.iterations} iterations, {dev_bytes:.0f} bytes / iteration, "
          f"{dev_ms:.3f} ms / iteration; |dobj| {abs(got.obj_val - ref.obj_val):.2e}; barrier searches {dev_solver.barrier_searches} "
          f"(backtracks {dev_solver.barrier_backtracks})")
    assert got.status == ref.status == ipm.SOLVED, (got.status, ref.status)
    assert abs(got.obj_val - ref.obj_val) <= 2.0 * max(st.tol_gap_abs, st.tol_gap_rel * max(1.0, abs(ref.obj_val)))
    assert dev_solver.barrier_searches > 0      # the Dual strategy throughout


# ---- shadow run: the host path drives, the device gets the same inputs ----------------------------------------------------------------

def _margin50(c, q, dq, a, dual):
    p = gp.moved(q, dq, a)
    if _is_gp(c):
        return gp.margin(c.alpha, p, dual)
    kind = "exp" if isinstance(c, cn.ExponentialCone) else "pow"
    return c3.margin(kind, [float(t) for t in p], getattr(c, "alpha", 0.0), dual)


def walk_step_length(cones, dz, ds, z, s, alpha_max, st, sym_alpha):
    """the composite rule of coneops_compositecone.jl:216-252 with the stand-in's non-symmetric cones, started from sym_alpha (the
    symmetric cones' part) -> (alpha, (cone, call) pairs whose decision margin at 50 digits is below 1e-8, pairs)"""
    alpha = min(min(alpha_max, sym_alpha), 1.0 - gp.SQRT_EPS64)
    step, amin = st.linesearch_backtrack_step, st.min_terminate_step_length
    near = pairs = 0
    for c, r in zip(cones.cones, cones.rng_cones):
        if getattr(c, "is_symmetric", True):
            continue
        pairs += 1
        is_near, res = False, []
        for q, dq, dual, inside in ((z[r], dz[r], True, c.is_dual_feasible), (s[r], ds[r], False, c.is_primal_feasible)):
            a, rejected = alpha, None
            while True:
                if inside(q + a * dq):
                    break
                rejected = a
                a *= step
                if a < amin:
                    a = 0.0
                    break
            for aa in (a, rejected):
                if aa is not None:
                    mg = _margin50(c, q, dq, aa, dual)
                    is_near = is_near or (mg is not None and abs(mg) < DECISION_MARGIN)
            res.append(a)
        assert tuple(res) == c.step_length(dz[r], ds[r], z[r], s[r], alpha, st), "the test's walk of the stand-in's line search drifted"
        near += is_near
        alpha = min(alpha, res[0], res[1])
    return alpha, near, pairs


def test_shadow_run_on_the_host_driven_ipm():
    with _Timeout(120):
        S = cl.Solver(*_mix20(), cl.Settings(device_scaling=True))
        assert not S._device_step
        ks, cones, st = S.kktsystem.kktsolver, S.cones, S.settings
        ks.h.step_enable_genpow(True, st.linesearch_backtrack_step, st.min_terminate_step_length)
        twin, rows_sym = _symmetric_twin_handle(cones, 11)
        rec = dict(shift=0, mulhs=0, worst_mulhs=0.0, sl_calls=0, sl_pairs=0, sl_excluded=0, sl_differ=0)
        host_shift, host_mul, host_step_length = cones.combined_ds_shift, cones.mul_Hs, cones.step_length

        def shift(out, step_z, step_s, sigma_mu):
            sz0, ss0 = step_z.copy(), step_s.copy()
            host_shift(out, step_z, step_s, sigma_mu)
            dev = ks.cone_combined_ds_shift(sz0, ss0, sigma_mu)
            for c, r in zip(cones.cones, cones.rng_cones):
                if _is_gp(c):
                    assert np.array_equal(dev[r], c.grad * sigma_mu) and np.array_equal(dev[r], out[r])
                    rec["shift"] += 1

        def mul_hs(y, x, work):
            x0 = x.copy()
            host_mul(y, x, work)
            dev = ks.cone_mul_hs(x0)
            for c, r in zip(cones.cones, cones.rng_cones):
                if _is_gp(c):
                    slot = np.concatenate([c.grad, c.d1, [c.d2], c.p, c.q, c.r])
                    ref, terms = gp.ref_mul_hs(slot, c.dim1, c.dim2, c.mu, x0[r])
                    for i in range(c.dim):
                        e = float(abs(gp.mpf(float(dev[r][i])) - ref[i]))
                        rec["worst_mulhs"] = max(rec["worst_mulhs"], e / max(terms[i], 1e-300))
                        assert e <= SUM_TOL * terms[i], (i, e, terms[i])
                    rec["mulhs"] += 1

        def step_length(dz, ds, z, s, alpha_max):
            got = ks.cone_step_length(dz, ds, alpha_max)
            assert twin.h.update_scaling(s[rows_sym], z[rows_sym])[0]
            ref, near, pairs = walk_step_length(cones, dz, ds, z, s, alpha_max, st, _twin_step_length(twin, rows_sym, dz, ds, alpha_max))
            assert got[0] == got[1]
            rec["sl_calls"] += 1
            rec["sl_pairs"] += pairs
            rec["sl_excluded"] += near
            if got[0] != ref:
                rec["sl_differ"] += 1
                print(f"[genpow shadow] step-length call {rec['sl_calls']}: device {got[0]!r}, stand-in {ref!r}, near-boundary pairs {near}")
                assert near > 0, (got, ref)
            return host_step_length(dz, ds, z, s, alpha_max)

        cones.combined_ds_shift, cones.mul_Hs, cones.step_length = shift, mul_hs, step_length
        sol = S.solve()
    assert sol.status == ipm.SOLVED, sol.status
    share = rec["sl_excluded"] / max(rec["sl_pairs"], 1)
    print(f"[genpow shadow mix20] {sol.iterations} iterations; Generalized Power shifts {rec['shift']} (all ==), mul_Hs {rec['mulhs']} "
          f"(max |y - ref| / sum |terms| {rec['worst_mulhs']:.2e}); step-length calls {rec['sl_calls']}, excluded {rec['sl_excluded']} of "
          f"{rec['sl_pairs']} (cone, call) pairs ({100 * share:.2f} %), calls that differ {rec['sl_differ']}")
    assert rec["shift"] >= 3 * sol.iterations and rec["mulhs"] >= 6 * sol.iterations
    assert rec["sl_calls"] >= 2 * sol.iterations and share <= 0.05
