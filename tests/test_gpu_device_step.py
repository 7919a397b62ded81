"""The device-resident interior-point step on the GPU (step.hip, hipkkt_cone_* / hipkkt_step_*, Settings.device_step) against the
stand-in's numpy cones and its own kkt_solve.

Gates (the project's own):
  * row-wise results (Zero / Nonnegative rows of every operation, add_step): BIT-IDENTICAL -- same expressions, no contraction;
  * results that contain a sum (second-order cones, norms, fused scalars): every `dot` of the reference may differ by
    1e-13 * sum|terms| (the gate of test_gpu_kkt.py for the sums of N2 / N4: a tree sum against numpy's order).  An element that is a
    FUNCTION of such sums gets the first-order propagation of exactly those allowances through the reference's own expressions
    (evaluated by re-running them with one sum moved by its allowance) plus 1e-13 of its own magnitude for its row-wise roundings;
  * step lengths and end-to-end quantities: 1e-10 relative.
The second-order cones of the host object ADOPT the device's (w, lambda, eta) before anything is compared, so both sides work on the
same scaling (the scaling itself is test_gpu_kkt.py's subject)."""
import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import problems
from clarabel_jl_amd.kktsolver import HipKKTSolver
from julia_standin import ipm
from tests import fixtures as fx
from tests.step_support import (PARITY, STEP_FLAGS, SUM_TOL, _adopt, _allowance, _check_cone_vector, _mixed_problem, _prep,
                                _soc_affine_ds, _soc_mul_hs, _soc_offset, _soc_shift, _Timeout)

pytestmark = pytest.mark.gpu


def _scaled_solver(seed, late):
    Pt, A, cones = _prep(_mixed_problem(seed))
    m, n = A.shape
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    assert hk.steps_on_device
    rng = np.random.default_rng(1000 + seed)
    s, z = (fx.scale_cones_late if late else fx.scale_cones)(cones, rng)
    ok, w, lam, eta = hk.h.update_scaling(s, z)
    assert ok
    _adopt(cones, w, lam, eta)
    return hk, cones, s, z, rng



CASES = [(seed, late) for late in (False, True) for seed in (3, 4, 5)]


@pytest.mark.parametrize("seed,late", CASES)
def test_granular_cone_operations_match_the_host_cones(seed, late):
    hk, cones, s, z, rng = _scaled_solver(seed, late)
    m = cones.numel
    K0 = hk.h.debug_dump(4)
    # affine_ds
    ref = np.zeros(m)
    cones.affine_ds(ref, s)
    _check_cone_vector(cones, hk.cone_affine_ds(), ref, lambda c, r: _allowance(_soc_affine_ds, 1, c), "affine_ds")
    # combined_ds_shift: inputs stay intact (the reference overwrites step_z / step_s)
    dz, ds, sm = rng.standard_normal(m), rng.standard_normal(m), 0.37 * (1e-9 if late else 1.0)
    dz0, ds0 = dz.copy(), ds.copy()
    got = hk.cone_combined_ds_shift(dz, ds, sm)
    assert np.array_equal(dz, dz0) and np.array_equal(ds, ds0)
    ref = np.zeros(m)
    cones.combined_ds_shift(ref, dz.copy(), ds.copy(), sm)
    _check_cone_vector(cones, got, ref, lambda c, r: _allowance(_soc_shift, 3, c, dz[r], ds[r], sm), "combined_ds_shift")
    # ds_from_dz_offset
    v = rng.standard_normal(m)
    ref = np.zeros(m)
    cones.ds_from_dz_offset(ref, v, np.zeros(m), z)
    _check_cone_vector(cones, hk.cone_ds_from_dz_offset(v), ref, lambda c, r: _allowance(_soc_offset, 3, c, z[r], v[r]), "ds_from_dz_offset")
    # mul_Hs
    ref = np.zeros(m)
    cones.mul_Hs(ref, v, np.zeros(m))
    _check_cone_vector(cones, hk.cone_mul_hs(v), ref, lambda c, r: _allowance(_soc_mul_hs, 1, c, v[r]), "mul_Hs")
    assert np.array_equal(hk.h.debug_dump(4), K0)          # no step call writes K


@pytest.mark.parametrize("seed,late", CASES)
def test_step_length_matches_the_host_cones(seed, late):
    hk, cones, s, z, rng = _scaled_solver(seed, late)
    m = cones.numel
    directions = {
        "hits the boundary": (-(0.5 + rng.random(m)) * z + 0.3 * np.abs(z) * rng.standard_normal(m),
                              -(0.5 + rng.random(m)) * s + 0.3 * np.abs(s) * rng.standard_normal(m), 1.0),
        "stays below the cap": (rng.standard_normal(m) * 1e-3 * np.abs(z), rng.standard_normal(m) * 1e-3 * np.abs(s), 0.7),
        "never hits": (0.5 * z, 2.0 * s, 1.0),
        "zero direction": (np.zeros(m), np.zeros(m), 0.9),
    }
    for name, (dz, ds, amax) in directions.items():
        az, as_ = hk.cone_step_length(dz, ds, amax)
        # the host's composite minimum, per component (coneops_compositecone.jl:216-252 returns min of the two)
        rz, rs = amax, amax
        for c, r in zip(cones.cones, cones.rng_cones):
            a, b = c.step_length(dz[r], ds[r], z[r], s[r], amax)
            rz, rs = min(rz, a), min(rs, b)
        print(f"[device-step step_length, {name}] alpha_z {az!r} (host {rz!r}), alpha_s {as_!r} (host {rs!r})")
        assert abs(az - rz) <= PARITY * rz and abs(as_ - rs) <= PARITY * rs, (name, az, rz, as_, rs)
        if name in ("never hits", "zero direction"):
            assert az == amax and as_ == amax, name
        if name == "hits the boundary":
            assert 0.0 < min(az, as_) < 1.0


@pytest.mark.parametrize("seed,late", [(3, False), (4, False), (5, True)])
def test_fused_steps_match_the_stand_in_on_the_same_plugin(seed, late):
    """hipkkt_step_affine_dev (constant-rhs solve pending) and hipkkt_step_combined_dev (resident constant solution, m_corr != 1)
    against ipm.KKTSystem.kkt_solve driven through the same plugin; apply, step_get and the info norms on the way"""
    _fused_steps_case(seed, late)


def _fused_steps_case(seed, late, settings=None, expect_steps=None):
    """settings: further Settings fields for both sides (tests/test_gpu_refinement_branches.py: forced refinement steps);
    expect_steps: the refinement steps every solve of the fused calls and of the host loop must report"""
    prob = _mixed_problem(seed)
    S = cl.Solver(*prob, cl.Settings(device_step=True, **STEP_FLAGS, **(settings or {})))
    assert S._device_step
    ks, data, cones, v = S.kktsystem.kktsolver, S.data, S.cones, S.variables
    n, m = data.n, data.m
    rng = np.random.default_rng(77 + seed)
    s, z = (fx.scale_cones_late if late else fx.scale_cones)(cones, rng)
    v.x[:], v.z[:], v.s[:], v.tau, v.kappa = rng.standard_normal(n), z, s, 0.9, 0.4
    xzs, res = ks.device_buffer(n + 2 * m), ks.device_buffer(3 * n + 2 * m)
    xzs.upload(np.concatenate([v.x, v.z, v.s]))
    r = S.residuals
    scal = ks.residuals_update_dev(xzs, res, v.tau, v.kappa)
    S._residuals_update()                                   # the host copy of the same residuals (device_residuals: hipkkt_residuals)
    assert scal == (r.dot_qx, r.dot_bz, r.dot_sz, r.dot_xPx, r.rtau)
    # info norms
    got8 = ks.kktsolver_info_norms(xzs, res)
    ns = ipm._norm_scaled
    ref8 = [ns(data.d, v.x), ns(data.e, v.z), ns(data.einv, v.s), ns(data.dinv, r.rx), ns(data.einv, r.rz), ns(data.dinv, r.rx_inf),
            ns(data.einv, r.rz_inf), ns(data.dinv, r.Px)]
    for g, t in zip(got8, ref8):
        print(f"[device-step info norm] relative difference {abs(g - t) / max(t, 1e-300):.2e}")
        assert abs(g - t) <= SUM_TOL * t + 1e-300, (g, t)      # |sqrt(a) - sqrt(b)| <= |a - b| / (2 sqrt(b)), a, b = the sums of squares
    # scaling on the device from the resident iterate, the host cones adopt it
    assert ks.kktsolver_update_scaled(cones, v.s, v.z)      # host-pointer form: outputs (w, lambda, eta) + refactor
    _adopt(cones, ks.scaling_w, ks.scaling_lambda, ks.scaling_soc_eta)
    K0 = ks.h.debug_dump(4)
    mu = (r.dot_sz + v.tau * v.kappa) / (cones.degree + 1)

    def check_step(step, ds_const, rhs_kappa, alpha, dtau, dkappa, fraction, lhs_ref, what):
        dx, dz, ds = step[:n], step[n:n + m], step[n + m:]
        scale = max(1.0, np.max(np.abs(lhs_ref.x)), np.max(np.abs(lhs_ref.z)))
        print(f"[device-step fused {what}] max |dx - ref| / scale {np.max(np.abs(dx - lhs_ref.x)) / scale:.2e}, "
              f"|dz - ref| / scale {np.max(np.abs(dz - lhs_ref.z)) / scale:.2e}")
        assert np.max(np.abs(dx - lhs_ref.x)) <= PARITY * scale and np.max(np.abs(dz - lhs_ref.z)) <= PARITY * scale, what
        assert abs(dtau - lhs_ref.tau) <= PARITY * max(1.0, abs(lhs_ref.tau)), what
        # ds, dkappa and alpha from the DEVICE's own dz, dtau through the host expressions
        ref = np.zeros(m)
        cones.mul_Hs(ref, dz, np.zeros(m))
        ref = -(ref + ds_const)

        def allowance(c, rr):      # ds = -(Hs dz + ds_const): the one sum of mul_Hs
            t, tol = _allowance(_soc_mul_hs, 1, c, dz[rr])
            return -(t + ds_const[rr]), tol + SUM_TOL * np.abs(ds_const[rr])
        _check_cone_vector(cones, ds, ref, allowance, what + " ds")
        assert dkappa == -(rhs_kappa + v.kappa * dtau) / v.tau, what
        a_tau = -v.tau / dtau if dtau < 0 else ipm.FLOATMAX
        a_kap = -v.kappa / dkappa if dkappa < 0 else ipm.FLOATMAX
        az, as_ = cones.step_length(dz, ds, v.z, v.s, min(a_tau, a_kap, 1.0))
        a_ref = min(az, as_) * fraction
        print(f"[device-step fused {what}] alpha {alpha!r}, from the device's step through the host cones {a_ref!r}")
        assert abs(alpha - a_ref) <= PARITY * a_ref, (what, alpha, a_ref)

    # ---- affine step, the constant-rhs solve pending
    total = ks.total_ir_steps
    ok, alpha_aff, dtau_aff, dkappa_aff = ks.kktsolver_step_affine(xzs, res, v.tau, v.kappa, r.rtau, True)
    assert ok and np.array_equal(ks.h.debug_dump(4), K0)
    if expect_steps is not None:       # both solves (this step's and the constant right-hand side's; neither can exceed max_iter)
        assert ks.last_ir_steps == expect_steps and ks.total_ir_steps - total == 2 * expect_steps
    step_aff = ks.h.step_get()
    lhs, rhs = S.step_lhs, S.step_rhs
    rhs.x[:], rhs.z[:] = r.rx, r.rz
    cones.affine_ds(rhs.s, v.s)
    rhs.tau, rhs.kappa = r.rtau, v.tau * v.kappa
    S.kktsystem._const_pending, S.kktsystem._have_const_dev = False, True      # (x2, z2) of this factorisation is resident now
    assert S.kktsystem.kkt_solve(lhs, rhs, data, v, cones, "affine")
    assert expect_steps is None or ks.last_ir_steps == expect_steps
    check_step(step_aff, v.s, rhs.kappa, alpha_aff, dtau_aff, dkappa_aff, 1.0, lhs, "affine")
    # ---- combined step on the resident constant solution, m_corr != 1
    sigma, mcorr = (1.0 - alpha_aff) ** 3, 0.5 + 0.4 * alpha_aff
    ok, alpha, dtau, dkappa = ks.kktsolver_step_combined(xzs, res, v.tau, v.kappa, r.rtau, dtau_aff, dkappa_aff, sigma, mu, mcorr)
    assert ok and np.array_equal(ks.h.debug_dump(4), K0)
    assert expect_steps is None or ks.last_ir_steps == expect_steps
    step = ks.h.step_get()
    # the host's right-hand side from the DEVICE's affine step (variables.jl:124-162)
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
    assert expect_steps is None or ks.last_ir_steps == expect_steps
    # ds = -(Hs dz + ds_const) is checked with the ds_const that the granular operations (each held against the host cones above)
    # give for the device's own affine step: the fused call must compose exactly those
    dz_m = step_aff[n:n + m] * mcorr
    rhs_s_dev = ks.cone_affine_ds() + ks.cone_combined_ds_shift(dz_m, step_aff[n + m:], sm)
    ds_const_dev = ks.cone_ds_from_dz_offset(rhs_s_dev)
    check_step(step, ds_const_dev, rhs.kappa, alpha, dtau, dkappa, S.settings.max_step_fraction, lhs, "combined")
    # ---- apply: bit-identical to numpy's v += alpha * dv
    before = xzs.download()
    ks.kktsolver_step_apply(alpha, xzs)
    assert np.array_equal(ks.h.step_get(), step)            # (a synchronising call on the handle: apply itself does not wait)
    after = xzs.download()
    assert np.array_equal(after, before + alpha * step)
    assert np.array_equal(ks.h.debug_dump(4), K0)


def test_step_entry_points_refuse_what_they_cannot_serve():
    """HIPKKT_ERR_ARGUMENT (ValueError in the binding): a PSD handle, an Exponential handle, no scaling yet, no hipkkt_set_qb"""
    # PSD
    Pt, A, cones = _prep(fx.basic_sdp())
    m, n = A.shape
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    assert not hk.steps_on_device
    s, z = fx.scale_cones(cones, np.random.default_rng(1))
    assert hk.kktsolver_update_scaled(cones, s, z)
    for call in (hk.cone_affine_ds, lambda: hk.cone_mul_hs(np.ones(m)), lambda: hk.cone_step_length(np.ones(m), np.ones(m), 1.0)):
        with pytest.raises(ValueError):
            call()
    # Exponential
    Pt, A, cones = _prep(fx.basic_exp())
    m, n = A.shape
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    assert not hk.steps_on_device
    s, z, mu = fx.scale_cones_nonsymmetric(cones, np.random.default_rng(2))
    assert hk.kktsolver_update_scaled(cones, s, z, mu=mu)
    with pytest.raises(ValueError):
        hk.cone_affine_ds()
    with pytest.raises(ValueError):
        hk.cone_ds_from_dz_offset(np.ones(m))
    # no scaling yet, then no set_qb
    Pt, A, cones = _prep(fx.basic_qp())
    m, n = A.shape
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    assert hk.steps_on_device
    with pytest.raises(ValueError):
        hk.cone_mul_hs(np.ones(m))
    xzs, res = hk.device_buffer(n + 2 * m), hk.device_buffer(3 * n + 2 * m)
    with pytest.raises(ValueError):
        hk.kktsolver_step_apply(0.5, xzs)
    s, z = fx.scale_cones(cones, np.random.default_rng(3))
    assert hk.kktsolver_update_scaled(cones, s, z)
    ref = np.zeros(m)
    cones.mul_Hs(ref, np.ones(m), np.zeros(m))
    assert np.array_equal(hk.cone_mul_hs(np.ones(m)), ref)
    with pytest.raises(ValueError):
        hk.kktsolver_step_affine(xzs, res, 1.0, 1.0, 0.0, True)      # hipkkt_set_qb has not been called
    hk.set_problem_vectors(np.ones(n), np.ones(m))
    with pytest.raises(ValueError):
        hk.kktsolver_step_combined(xzs, res, 1.0, 1.0, 0.0, 0.0, 0.0, 0.5, 1.0, 1.0)      # no affine step resident


END_TO_END = {
    "basic_qp": fx.basic_qp, "basic_lp": fx.basic_lp, "basic_socp": fx.basic_socp, "lasso_socp": fx.lasso_socp,
    "basic_qp_dualinf": fx.basic_qp_dualinf,
    "random_sparse_qp": lambda: problems.random_sparse_qp(n=1000, m=2000),
    "portfolio_socp": lambda: problems.portfolio_socp(n=500, nsoc=10, socdim=21),
}
_iteration_mismatches = []


@pytest.mark.parametrize("name", list(END_TO_END))
def test_ipm_with_device_step_matches_the_host_cone_algebra(name, capsys):
    """Settings(device_step=True) against the same problem with device_step=False (the other three device flags on in both): status
    equal, iterations equal or +-1 on at most one problem with the deciding quantity logged (the allowance of
    test_gpu_kkt.py test_ipm_matches_oracle_on_its_own_ordering), objective and residuals within 1e-10"""
    prob = END_TO_END[name]()
    with _Timeout(120):
        ref_solver = cl.Solver(*prob, cl.Settings(**STEP_FLAGS))
        ref_solver.trace = []
        ref = ref_solver.solve()
        dev_solver = cl.Solver(*prob, cl.Settings(device_step=True, **STEP_FLAGS))
        assert dev_solver._device_step and not ref_solver._device_step
        dev_solver.trace = []
        got = dev_solver.solve()
    assert got.status == ref.status, (got.status, ref.status)
    assert abs(got.iterations - ref.iterations) <= 1
    if got.iterations != ref.iterations:      # cause: a step-length / termination test decided by digits below 1e-10
        k = min(got.iterations, ref.iterations)
        with capsys.disabled():
            print(f"\n[device-step {name}] iterations {got.iterations} vs {ref.iterations}; at iteration {k}: "
                  f"device {dev_solver.trace[k]} host {ref_solver.trace[k]}")
        _iteration_mismatches.append(name)
        assert len(_iteration_mismatches) <= 1, _iteration_mismatches
        return
    print(f"[device-step {name}] {got.status} in {got.iterations} iterations; |dobj| / max(1, |obj|) "
          f"{abs(got.obj_val - ref.obj_val) / max(1.0, abs(ref.obj_val)):.2e}, |d r_prim| {abs(got.r_prim - ref.r_prim):.2e}, "
          f"|d r_dual| {abs(got.r_dual - ref.r_dual):.2e}")
    if ref.status == "SOLVED":
        assert abs(got.obj_val - ref.obj_val) <= PARITY * max(1.0, abs(ref.obj_val)), (got.obj_val, ref.obj_val)
    assert abs(got.r_prim - ref.r_prim) <= PARITY and abs(got.r_dual - ref.r_dual) <= PARITY
