"""The device-resident interior-point step for Exponential / Power cones on the GPU (step_cone3.hip, hipkkt_step_enable_cone3,
hipkkt_cone_barrier / hipkkt_step_barrier_dev, Settings.device_step_nonsymmetric) against the stand-in's numpy cones
(julia_standin/cones_nonsym.py) AFTER they adopted the device's scaling, so both sides use the same Hs / H_dual / grad.

Gates:
  * affine_ds, ds_from_dz_offset, mul_Hs on the three-row cones: BIT-IDENTICAL (row copies; two rounded products and sums, no contraction);
  * Zero / Nonnegative / SecondOrder rows of every row-wise operation: bit-identical to a symmetric-only handle fed the same rows;
  * combined_ds_shift: 1e-10 of max |ref| per cone (the project's parity gate);
  * barrier: 1e-10 * max(1, sum |cone terms|) per candidate; shifted dot: 1e-13 * sum |terms| (the gate of the sums / norms);
  * step length: EQUAL to what the stand-in's cones give, decision by decision, except a decision of an Exponential / Power cone whose
    host feasibility margin is within 1e-10 relative of zero: the feasibility expression divided by the sum of its absolute terms, at
    the accepted alpha or at the last rejected one.  Such a decision is excluded and counted per (cone, call), at most 5 %.
    The symmetric cones' part of the composite rule (coneops_compositecone.jl:216-252) contains tree sums on the device where a
    second-order cone binds (the unchanged kernels of step.hip, held to 1e-10 by test_gpu_device_step.py), so that part is taken from
    the device: a symmetric-only twin handle fed the same rows runs the same kernels on the same numbers.  From
    min(that, 1 - sqrt(eps)) the stand-in's Exponential / Power cones walk their grid alpha0 step^k multiplication by multiplication
    and the device's result must be `==`.  Where no second-order cone binds the twin's value is the host's bit for bit and the
    reference is the stand-in's composite step_length itself (asserted).
The shadow runs let the host path drive the IPM and give the granular device calls the same inputs at every iteration; the
end-to-end runs compare the two paths."""
import math

import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt, problems
from clarabel_jl_amd.kktsolver import HipKKTSolver
from julia_standin import cones_nonsym as cn
from julia_standin import ipm
from julia_standin.cones import SecondOrderCone
from tests import fixtures as fx
from tests.step_support import (NONSYM, PARITY, SQRT_EPS, STEP_FLAGS, _check_barrier, _is3, _prep, _problem, _symmetric_twin_handle, _Timeout,
                                _twin_step_length)

pytestmark = pytest.mark.gpu

MARGIN = 1e-10


def _interleaved_many():
    specs = []
    for k in range(300):
        specs.append(cl.ExponentialConeT())
        if k < 260:
            specs.append(cl.PowerConeT(0.1 + 0.8 * ((k * 37) % 101) / 100.0))
    return specs


CONE_SETS = {
    "exp_alone": lambda: [cl.ExponentialConeT()],
    "pow_alone": lambda: [cl.PowerConeT(0.37)],
    "interleaved": lambda: [cl.PowerConeT(0.3), cl.ExponentialConeT(), cl.NonnegativeConeT(3), cl.ExponentialConeT(), cl.PowerConeT(0.7),
                            cl.SecondOrderConeT(4), cl.ZeroConeT(2), cl.ExponentialConeT()],
    "many": _interleaved_many,          # 300 + 260 cones: more than one 256-lane workgroup in both launches
    "alphas": lambda: [cl.PowerConeT(0.5), cl.NonnegativeConeT(2), cl.PowerConeT(0.1), cl.PowerConeT(0.9), cl.PowerConeT(0.101),
                       cl.PowerConeT(0.899)],
}


def _scaled(setname, strategy, seed):
    """an enabled handle at a central fixture point, the host cones holding the DEVICE's scaling"""
    Pt, A, cones = _prep(_problem(CONE_SETS[setname](), seed))
    m, n = A.shape
    st = cl.Settings(**NONSYM)
    cones.use_settings(st)
    hk = HipKKTSolver(Pt, A, cones, m, n, st)
    assert hk.steps_on_device and hk.steps_nonsymmetric
    rng = np.random.default_rng(500 + seed)
    s, z, mu = fx.scale_cones_nonsymmetric(cones, rng, strategy)
    assert hk.kktsolver_update_scaled(cones, s, z, mu=mu, strategy=strategy)
    return hk, cones, s, z, mu, rng, st


def _symmetric_twin(cones, s, z, seed):
    """a handle with the symmetric members only, scaled at the same rows -> (twin, rows of the full set)"""
    twin, rows = _symmetric_twin_handle(cones, seed)
    if twin is not None:
        assert twin.h.update_scaling(s[rows], z[rows])[0]
    return twin, rows


# ---- the host's backtracking, walked again for its margins --------------------------------------------------------------------------

def _margin(c, q, dual):
    """feasibility expression / sum of its absolute terms; None when a sign condition decides"""
    if isinstance(c, cn.ExponentialCone):
        if dual:
            if not (q[2] > 0 and q[0] < 0):
                return None
            t = [q[1], -q[0], -q[0] * cn.logsafe(-q[2] / q[0])]
        else:
            if not (q[2] > 0 and q[1] > 0):
                return None
            t = [q[1] * cn.logsafe(q[2] / q[1]), -q[0]]
    else:
        a = c.alpha
        if not (q[0] > 0 and q[1] > 0):
            return None
        if dual:
            t = [math.exp(2 * a * cn.logsafe(q[0] / a) + 2 * (1 - a) * cn.logsafe(q[1] / (1 - a))), -q[2] * q[2]]
        else:
            t = [math.exp(2 * a * cn.logsafe(q[0]) + 2 * (1 - a) * cn.logsafe(q[1])), -q[2] * q[2]]
    return sum(t) / sum(abs(v) for v in t)


def _host_step_length(cones, dz, ds, z, s, alpha_max, st, sym_alpha):
    """The composite rule with the stand-in's Exponential / Power cones, started from the DEVICE's symmetric part sym_alpha
    -> (alpha, three-row cones with a near-boundary decision, number of three-row cones, does a second-order cone bind?)"""
    alpha = no_soc = alpha_max
    for c, r in zip(cones.cones, cones.rng_cones):
        if getattr(c, "is_symmetric", True):
            az, as_ = c.step_length(dz[r], ds[r], z[r], s[r], alpha)
            alpha = min(alpha, az, as_)
            if not isinstance(c, SecondOrderCone):
                az, as_ = c.step_length(dz[r], ds[r], z[r], s[r], no_soc)
                no_soc = min(no_soc, az, as_)
    soc_bound = alpha != no_soc
    start = min(alpha_max, sym_alpha)
    if not soc_bound:      # Zero / Nonnegative rows are bit-exact on the device: the start is the host's
        assert start == alpha, (start, alpha)
    alpha = min(start, 1.0 - SQRT_EPS)
    near = n3 = 0
    step, amin = st.linesearch_backtrack_step, st.min_terminate_step_length
    for c, r in zip(cones.cones, cones.rng_cones):
        if not _is3(c):
            continue
        n3 += 1
        is_near = False
        res = []
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
                    mg = _margin(c, q + aa * dq, dual)
                    is_near = is_near or (mg is not None and abs(mg) < MARGIN)
            res.append(a)
        assert tuple(res) == c.step_length(dz[r], ds[r], z[r], s[r], alpha, st), "the test's walk of the stand-in's line search drifted"
        near += is_near
        alpha = min(alpha, res[0], res[1])
    if not soc_bound:
        assert alpha == type(cones).step_length(cones, dz, ds, z, s, alpha_max)[0]      # (the class's: the shadow run wraps the instance's)
    return alpha, near, n3, soc_bound


def _check_step_length(got, cones, dz, ds, z, s, alpha_max, st, what, sym_alpha):
    """-> (excluded (cone, call) pairs, (cone, call) pairs of this call, does a second-order cone bind?)"""
    ref, near, n3, soc_bound = _host_step_length(cones, dz, ds, z, s, alpha_max, st, sym_alpha)
    assert got[0] == got[1], what
    if got[0] != ref:
        print(f"[nonsym step length {what}] device {got[0]!r} host {ref!r} (relative {abs(got[0] - ref) / ref:.2e}): near-boundary cones "
              f"{near}, a second-order cone binds {soc_bound}")
        assert near > 0, (what, got, ref)
    return near, n3, soc_bound


# ---- granular ----------------------------------------------------------------------------------------------------------------------------

GRANULAR = [(name, strategy, seed) for name in CONE_SETS for strategy in ("primal_dual", "dual") for seed in (3, 4, 5)]
_granular_excluded = [0, 0]


@pytest.mark.parametrize("setname,strategy,seed", GRANULAR)
def test_granular_operations_match_the_adopting_host_cones(setname, strategy, seed):
    with _Timeout(60):
        hk, cones, s, z, mu, rng, st = _scaled(setname, strategy, seed)
        m = cones.numel
        K0 = hk.h.debug_dump(4)
        rows3 = np.concatenate([np.arange(r.start, r.stop) for c, r in zip(cones.cones, cones.rng_cones) if _is3(c)])
        twin, rows_sym = _symmetric_twin(cones, s, z, seed)
        dz, ds, v = rng.standard_normal(m), rng.standard_normal(m), rng.standard_normal(m)
        sm = 0.3 * mu
        # affine_ds, ds_from_dz_offset, mul_Hs: bit for bit on the three-row cones
        got = {"affine_ds": hk.cone_affine_ds(), "ds_from_dz_offset": hk.cone_ds_from_dz_offset(v), "mul_Hs": hk.cone_mul_hs(v),
               "combined_ds_shift": hk.cone_combined_ds_shift(dz, ds, sm)}
        ref = {k: np.zeros(m) for k in got}
        cones.affine_ds(ref["affine_ds"], s)
        cones.ds_from_dz_offset(ref["ds_from_dz_offset"], v, np.zeros(m), z)
        cones.mul_Hs(ref["mul_Hs"], v, np.zeros(m))
        cones.combined_ds_shift(ref["combined_ds_shift"], dz.copy(), ds.copy(), sm)
        for k in ("affine_ds", "ds_from_dz_offset", "mul_Hs"):
            assert np.array_equal(got[k][rows3], ref[k][rows3]), k
        # combined_ds_shift: 1e-10 of max |ref| per cone
        worst = 0.0
        for c, r in zip(cones.cones, cones.rng_cones):
            if _is3(c):
                e = float(np.max(np.abs(got["combined_ds_shift"][r] - ref["combined_ds_shift"][r])) / np.max(np.abs(ref["combined_ds_shift"][r])))
                worst = max(worst, e)
                assert e <= PARITY, (type(c).__name__, e)
        print(f"[nonsym granular {setname} {strategy} {seed}] combined_ds_shift: max |got - ref| / max |ref| per cone = {worst:.2e}")
        # the symmetric rows: the kernels of the symmetric-only path, bit for bit
        if twin is not None:
            tw = {"affine_ds": twin.cone_affine_ds(), "ds_from_dz_offset": twin.cone_ds_from_dz_offset(v[rows_sym]),
                  "mul_Hs": twin.cone_mul_hs(v[rows_sym]), "combined_ds_shift": twin.cone_combined_ds_shift(dz[rows_sym], ds[rows_sym], sm)}
            for k in tw:
                assert np.array_equal(got[k][rows_sym], tw[k]), k
        # step length: random directions (several backtracks), short ones (alpha0 itself), alpha_max below 1
        for what, f, amax in (("N(0,1)", 1.0, 1.0), ("short", 1e-3, 1.0), ("alpha_max 0.4", 0.3, 0.4)):
            ex, n3, _ = _check_step_length(hk.cone_step_length(f * dz, f * ds, amax), cones, f * dz, f * ds, z, s, amax, st,
                                           f"{setname} {strategy} {seed} {what}", _twin_step_length(twin, rows_sym, f * dz, f * ds, amax))
            _granular_excluded[0] += ex
            _granular_excluded[1] += n3
        # barrier at max_step_fraction times the accepted step length and seven further grid points (inside the cones: they are convex)
        a0 = st.max_step_fraction * cones.step_length(dz, ds, z, s, 1.0)[0]
        alphas = [a0 * st.linesearch_backtrack_step ** k for k in range(8)]
        bars, dots = hk.cone_barrier(dz, ds, alphas)
        _check_barrier(bars, dots, cones, z, s, dz, ds, alphas, f"{setname} {strategy} {seed}")
        bars1, dots1 = hk.cone_barrier(dz, ds, alphas[2:3])        # a single candidate: the same numbers
        assert bars1[0] == bars[2] and dots1[0] == dots[2]
        assert np.array_equal(hk.h.debug_dump(4), K0)              # no step call writes K
    print(f"[nonsym granular] excluded step-length decisions so far: {_granular_excluded[0]} of {_granular_excluded[1]} (cone, call) pairs")
    assert _granular_excluded[0] <= 0.05 * max(_granular_excluded[1], 1)


def test_refusals():
    st = cl.Settings(**NONSYM)
    # a handle that was not enabled
    Pt, A, cones = _prep(fx.basic_exp())
    m, n = A.shape
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    assert not hk.steps_on_device
    s, z, mu = fx.scale_cones_nonsymmetric(cones, np.random.default_rng(2))
    assert hk.kktsolver_update_scaled(cones, s, z, mu=mu)
    for call in (hk.cone_affine_ds, lambda: hk.cone_step_length(np.ones(m), np.ones(m), 1.0),
                 lambda: hk.cone_barrier(np.ones(m), np.ones(m), [0.5])):
        with pytest.raises(ValueError):
            call()
    # bad line-search constants, a trip count above 4096
    for step, amin in ((0.0, 1e-4), (1.0, 1e-4), (1.5, 1e-4), (-0.1, 1e-4), (float("nan"), 1e-4), (0.8, 0.0), (0.8, -1.0),
                       (0.8, float("inf")), (0.999999, 1e-4)):
        with pytest.raises(ValueError):
            hk.h.step_enable_cone3(True, step, amin)
    # enabled: use before a successful _ex scaling, then served; a new registration clears the enable
    hk.h.step_enable_cone3(True, 0.8, 1e-4)
    with pytest.raises(ValueError):
        hk.cone_affine_ds()
    assert hk.kktsolver_update_scaled(cones, s, z, mu=mu)
    assert np.array_equal(hk.cone_affine_ds()[-3:], s[-3:])      # (the Exponential cone is the last one)
    assert hk.cone_barrier(np.zeros(m), np.zeros(m), np.zeros(8))[0].shape == (8,)
    with pytest.raises(ValueError):
        hk.cone_barrier(np.zeros(m), np.zeros(m), np.zeros(9))
    kinds, alpha = cones.kkt_cone_kinds_ex()
    hk.h.set_cone_types_ex(kinds, alpha)
    assert hk.kktsolver_update_scaled(cones, s, z, mu=mu)
    with pytest.raises(ValueError):
        hk.cone_affine_ds()
    hk.h.step_enable_cone3(True, 0.8, 1e-4)
    hk.h.step_enable_cone3(False, 0.8, 1e-4)                     # switched off again
    assert hk.kktsolver_update_scaled(cones, s, z, mu=mu)
    with pytest.raises(ValueError):
        hk.cone_mul_hs(np.ones(m))
    # Generalized Power and PSD handles are refused at the enable, with the setting on as well
    for make in (fx.basic_genpow, fx.basic_sdp):
        Pt, A, cones = _prep(make())
        m, n = A.shape
        hk = HipKKTSolver(Pt, A, cones, m, n, st)
        assert not hk.steps_on_device
        with pytest.raises(ValueError):
            hk.h.step_enable_cone3(True, 0.8, 1e-4)
    # a symmetric set has nothing to enable
    Pt, A, cones = _prep(fx.basic_qp())
    m, n = A.shape
    hk = HipKKTSolver(Pt, A, cones, m, n, st)
    assert hk.steps_on_device and not hk.steps_nonsymmetric
    with pytest.raises(ValueError):
        hk.h.step_enable_cone3(True, 0.8, 1e-4)


@pytest.mark.parametrize("setname", ["exp_alone", "pow_alone"])
def test_directions_that_leave_the_cone_never_trap(setname):
    hk, cones, s, z, mu, rng, st = _scaled(setname, "primal_dual", 3)
    out = np.array([1e8, 0.0, 0.0]) if setname == "exp_alone" else np.array([-1e8, 0.0, 0.0])      # z1 < 0 resp. z1 > 0 is lost for every alpha >= alpha_min
    for dz, ds in ((out, np.zeros(3)), (np.zeros(3), -1e8 * np.array([0.0, 1.0, 0.0])), (out, out)):
        got = hk.cone_step_length(dz, ds, 1.0)
        assert got == (0.0, 0.0), got
        assert cones.step_length(dz, ds, z, s, 1.0) == (0.0, 0.0)
        bars, dots = hk.cone_barrier(dz, ds, [1.0, 0.5])
        assert all((not np.isfinite(b)) or abs(b) > 1e300 for b in bars), bars
    bars, _ = hk.cone_barrier(np.full(3, np.nan), np.zeros(3), [0.5])
    assert not np.isfinite(bars[0]) or abs(bars[0]) > 1e300
    assert hk.cone_step_length(np.full(3, np.nan), np.zeros(3), 1.0) == (0.0, 0.0)
    # the handle still serves
    assert np.array_equal(hk.cone_affine_ds(), s)


# ---- the fused calls ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strategy,seed,tau", [("primal_dual", 3, 0.9), ("dual", 4, 0.9), ("primal_dual", 5, 1e-3)])
def test_fused_steps_and_the_resident_barrier_match_the_granular_calls_and_the_stand_in(strategy, seed, tau):
    """hipkkt_step_affine_dev / _combined_dev on an enabled handle: dx, dz against the stand-in's kkt_solve on the same plugin (1e-10);
    ds = -(Hs dz + ds_const) bit for bit on the Exponential / Power / Nonnegative / Zero rows; dkappa exactly the host expression; the
    composite step length, whose start min(alpha_tau, alpha_kappa, 1) is formed on the device, exactly what the granular call (held
    to the stand-in above) gives for that start; hipkkt_step_barrier_dev exactly what hipkkt_cone_barrier gives for the same step.
    tau = 1e-3 makes that start bind in the affine step: dkappa_aff = -kappa (1 + dtau / tau), so dtau > 0 gives
    alpha_kappa = 1 / (1 + dtau / tau) < 1 and dtau < -tau gives alpha_tau = tau / |dtau| < 1."""
    with _Timeout(60):
        S = cl.Solver(*_mix20(), cl.Settings(**NONSYM))
        assert S._device_step
        ks, data, cones, v, st = S.kktsystem.kktsolver, S.data, S.cones, S.variables, S.settings
        n, m = data.n, data.m
        rng = np.random.default_rng(70 + seed)
        s, z, _ = fx.scale_cones_nonsymmetric(cones, rng, strategy)
        v.x[:], v.z[:], v.s[:], v.tau, v.kappa = rng.standard_normal(n), z, s, tau, 0.4
        xzs, res = ks.device_buffer(n + 2 * m), ks.device_buffer(3 * n + 2 * m)
        xzs.upload(np.concatenate([v.x, v.z, v.s]))
        r = S.residuals
        ks.residuals_update_dev(xzs, res, v.tau, v.kappa)
        S._residuals_update()
        mu = (r.dot_sz + v.tau * v.kappa) / (cones.degree + 1)
        assert ks.kktsolver_update_scaled(cones, v.s, v.z, mu=mu, strategy=strategy)      # the host cones adopt the device's scaling
        exact = np.concatenate([np.arange(q.start, q.stop) for c, q in zip(cones.cones, cones.rng_cones)
                                if not isinstance(c, SecondOrderCone)])
        binding = []

        def check_step(step, scal, ds_const, rhs_kappa, alpha, dtau, dkappa, fraction, lhs_ref, what):
            dx, dz, ds = step[:n], step[n:n + m], step[n + m:]
            scale = max(1.0, np.max(np.abs(lhs_ref.x)), np.max(np.abs(lhs_ref.z)))
            print(f"[nonsym fused {what}] max |dx - ref| / scale {np.max(np.abs(dx - lhs_ref.x)) / scale:.2e}, "
                  f"|dz - ref| / scale {np.max(np.abs(dz - lhs_ref.z)) / scale:.2e}")
            assert np.max(np.abs(dx - lhs_ref.x)) <= PARITY * scale and np.max(np.abs(dz - lhs_ref.z)) <= PARITY * scale, what
            assert abs(dtau - lhs_ref.tau) <= PARITY * max(1.0, abs(lhs_ref.tau)), what
            ref = np.zeros(m)
            cones.mul_Hs(ref, dz, np.zeros(m))
            ref = -(ref + ds_const)
            assert np.array_equal(ds[exact], ref[exact]), what
            assert dkappa == -(rhs_kappa + v.kappa * dtau) / v.tau, what
            a_tau = -v.tau / dtau if dtau < 0 else ipm.FLOATMAX
            a_kap = -v.kappa / dkappa if dkappa < 0 else ipm.FLOATMAX
            start = min(a_tau, a_kap, 1.0)
            binding.append(start < 1.0)
            comp = ks.cone_step_length(dz, ds, start)
            print(f"[nonsym fused {what}] min(alpha_tau, alpha_kappa, 1) = {start!r}, composite {scal[3]!r}, alpha {alpha!r}")
            assert (scal[3], scal[4]) == comp and comp[0] == comp[1], (what, scal[3:5], comp)
            assert alpha == comp[0] * fraction and scal[0] == alpha, (what, alpha, comp)
            return dz, ds

        ok, alpha_aff, dtau_aff, dkappa_aff = ks.kktsolver_step_affine(xzs, res, v.tau, v.kappa, r.rtau, True)
        assert ok
        scal_aff, step_aff = ks.last_step_scalars.copy(), ks.h.step_get()
        lhs, rhs = S.step_lhs, S.step_rhs
        rhs.x[:], rhs.z[:] = r.rx, r.rz
        cones.affine_ds(rhs.s, v.s)
        rhs.tau, rhs.kappa = r.rtau, v.tau * v.kappa
        S.kktsystem._const_pending, S.kktsystem._have_const_dev = False, True
        assert S.kktsystem.kkt_solve(lhs, rhs, data, v, cones, "affine")
        check_step(step_aff, scal_aff, v.s, rhs.kappa, alpha_aff, dtau_aff, dkappa_aff, 1.0, lhs, "affine")
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
        dz, ds = check_step(step, scal, ds_const_dev, rhs.kappa, alpha, dtau, dkappa, st.max_step_fraction, lhs, "combined")
        print(f"[nonsym fused {strategy} {seed} tau={tau}] start below 1 in (affine, combined): {binding}")
        if tau < 0.1:
            assert binding[0], "min(alpha_tau, alpha_kappa, 1) was meant to bind in the affine step"
        # the barrier on the resident iterate and step: the numbers of the granular call, and the stand-in's within the gates
        alphas = [alpha * st.linesearch_backtrack_step ** k for k in range(8)]
        bars, dots = ks.kktsolver_step_barrier(xzs, alphas)
        bars_g, dots_g = ks.cone_barrier(dz, ds, alphas)
        assert np.array_equal(bars, bars_g) and np.array_equal(dots, dots_g)
        if alpha > 0.0:
            _check_barrier(bars, dots, cones, v.z, v.s, dz, ds, alphas, f"resident step {strategy} {seed}")
        before = xzs.download()
        ks.kktsolver_step_apply(alpha, xzs)
        assert np.array_equal(ks.h.step_get(), step)
        assert np.array_equal(xzs.download(), before + alpha * step)


# ---- shadow run: the host path drives, the device gets the same inputs ----------------------------------------------------------------

def _mix20():
    return problems.nonsymmetric_mix(n=20, nexp=5, npow=4, ngenpow=0, nn=6, nzero=2, socdim=4, seed=9)


def _mix80():
    return problems.nonsymmetric_mix(n=80, nexp=30, npow=20, ngenpow=0, nn=20, nzero=3, socdim=5, seed=5)


def _ulp(rng, v):
    v = np.array(v, dtype=float)
    return np.where(rng.integers(0, 2, v.shape) == 1, np.nextafter(v, np.inf), np.nextafter(v, -np.inf))


@pytest.mark.parametrize("forced_dual", [False, True], ids=["default", "forced_dual"])
@pytest.mark.parametrize("name", ["mix20", "mix80"])
def test_shadow_run_on_the_host_driven_ipm(name, forced_dual):
    """Correction rows: a three-row cone whose host spread over eight fixed-seed +-1-ulp perturbations of (z, step_z, step_s) is <= 1e-12
    (of max |ref|) is HELD to 1e-10; at least 0.6 of all are held (0.80 .. 0.86 on these problems with the CPU oracle); for the others
    error and error / spread must be finite.  Step-length calls: equal to the host's or excluded (module docstring), at most 5 %
    excluded.  Barrier decisions: the index of the first candidate < 1 equals the host's unless |barrier - 1| < 1e-8, at most 5 %."""
    extra = dict(min_switch_step_length=1.0) if forced_dual else {}
    prob = {"mix20": _mix20, "mix80": _mix80}[name]()
    with _Timeout(120):
        S = cl.Solver(*prob, cl.Settings(device_scaling=True, **extra))
        assert not S._device_step
        ks, cones, st = S.kktsystem.kktsolver, S.cones, S.settings
        ks.h.step_enable_cone3(True, st.linesearch_backtrack_step, st.min_terminate_step_length)
        rng = np.random.default_rng(0)
        twin, rows_sym = _symmetric_twin_handle(cones, 11)      # the device's symmetric kernels alone, for the start of the line search
        rec = dict(soc_bound=0, rows=0, held=0, worst_held=0.0, unheld=[], sl_pairs=0, sl_excluded=0, sl_calls=0, bar_calls=0, bar_excluded=0,
                   bar_err=0.0)
        host_shift, host_step_length, host_backtrack = cones.combined_ds_shift, cones.step_length, S._backtrack_step_to_barrier

        def shift(out, step_z, step_s, sigma_mu):
            sz0, ss0 = step_z.copy(), step_s.copy()
            host_shift(out, step_z, step_s, sigma_mu)
            dev = ks.cone_combined_ds_shift(sz0, ss0, sigma_mu)
            for c, r in zip(cones.cones, cones.rng_cones):
                if not _is3(c):
                    continue
                ref, z0, spread = out[r].copy(), c.z.copy(), 0.0
                for _ in range(8):
                    t = np.zeros(3)
                    c.z[:] = _ulp(rng, z0)
                    c.combined_ds_shift(t, _ulp(rng, sz0[r]), _ulp(rng, ss0[r]), sigma_mu)
                    spread = max(spread, float(np.max(np.abs(t - ref))))
                c.z[:] = z0
                scale = max(float(np.max(np.abs(ref))), 1e-300)
                err, spread = float(np.max(np.abs(dev[r] - ref))) / scale, spread / scale
                rec["rows"] += 1
                if spread <= 1e-12:
                    rec["held"] += 1
                    rec["worst_held"] = max(rec["worst_held"], err)
                    assert err <= PARITY, (type(c).__name__, err, spread)
                else:
                    assert np.isfinite(err) and np.isfinite(err / spread), (err, spread)
                    rec["unheld"].append((err, err / spread))

        def step_length(dz, ds, z, s, alpha_max):
            got = ks.cone_step_length(dz, ds, alpha_max)
            assert twin.h.update_scaling(s[rows_sym], z[rows_sym])[0]
            ex, n3, soc_bound = _check_step_length(got, cones, dz, ds, z, s, alpha_max, st, f"{name} call {rec['sl_calls']}",
                                                   _twin_step_length(twin, rows_sym, dz, ds, alpha_max))
            rec["soc_bound"] += soc_bound
            rec["sl_calls"] += 1
            rec["sl_pairs"] += n3
            rec["sl_excluded"] += ex
            return host_step_length(dz, ds, z, s, alpha_max)

        def backtrack(alpha_init):
            alpha = host_backtrack(alpha_init)
            v, lhs, step = S.variables, S.step_lhs, st.linesearch_backtrack_step
            cand, a = [], alpha_init
            for _ in range(8):
                cand.append(a)
                a = step * a
            bars, dots = ks.cone_barrier(lhs.z, lhs.s, cand)
            central = cones.degree + 1
            dev_b, host_b = [], []
            for a, bar, sz in zip(cand, bars, dots):
                tau, kap = v.tau + a * lhs.tau, v.kappa + a * lhs.kappa
                dev_b.append(central * ipm._logsafe((float(sz) + tau * kap) / central) - ipm._logsafe(tau) - ipm._logsafe(kap) + float(bar))
                host_b.append(S._variables_barrier(a))
                if np.isfinite(host_b[-1]):
                    rec["bar_err"] = max(rec["bar_err"], abs(dev_b[-1] - host_b[-1]) / max(1.0, abs(host_b[-1])))
            dev_k = next((k for k, b in enumerate(dev_b) if b < 1.0), None)
            host_k = next((k for k, b in enumerate(host_b) if b < 1.0), None)
            assert host_k is None or cand[host_k] == alpha
            # the accepted candidate and the last rejected one decide (all eight when none of them is accepted)
            deciding = host_b if host_k is None else host_b[max(host_k - 1, 0):host_k + 1]
            near = any(abs(b - 1.0) < 1e-8 for b in deciding)
            rec["bar_calls"] += 1
            if near:
                rec["bar_excluded"] += 1
            else:
                assert dev_k == host_k, (dev_k, host_k)
            return alpha

        cones.combined_ds_shift, cones.step_length, S._backtrack_step_to_barrier = shift, step_length, backtrack
        sol = S.solve()
    assert sol.status == ipm.SOLVED, sol.status
    held = rec["held"] / max(rec["rows"], 1)
    un = np.array(rec["unheld"]) if rec["unheld"] else np.zeros((0, 2))
    print(f"[nonsym shadow {name} forced_dual={forced_dual}] {sol.iterations} iterations; correction rows {rec['rows']}, held {held:.3f} "
          f"(worst held error {rec['worst_held']:.2e}); not held: max error {un[:, 0].max() if len(un) else 0.0:.2e}, "
          f"max error / spread {un[:, 1].max() if len(un) else 0.0:.2e}; step-length calls {rec['sl_calls']} ({rec['soc_bound']} with a second-order cone binding), excluded "
          f"{rec['sl_excluded']} of {rec['sl_pairs']} (cone, call) pairs; barrier searches {rec['bar_calls']}, excluded {rec['bar_excluded']}, "
          f"max |variables_barrier - host| / max(1, |host|) {rec['bar_err']:.2e}")
    assert rec["rows"] > 0 and held >= 0.6
    assert rec["sl_calls"] >= 2 * sol.iterations and rec["sl_excluded"] <= 0.05 * rec["sl_pairs"]
    assert rec["bar_excluded"] <= 0.05 * max(rec["bar_calls"], 1)
    if forced_dual:
        assert rec["bar_calls"] >= 14
    else:
        assert rec["bar_calls"] == 0


# ---- end to end --------------------------------------------------------------------------------------------------------------------------

END_TO_END = {"basic_exp": fx.basic_exp, "basic_pow": fx.basic_pow, "mix20": _mix20, "mix80": _mix80}


def _solve_counting(prob, **flags):
    solver = cl.Solver(*prob, cl.Settings(**flags))
    for k in hipkkt.TRAFFIC:
        hipkkt.TRAFFIC[k] = 0
    sol = solver.solve()
    it = max(sol.iterations, 1)
    return solver, sol, (hipkkt.TRAFFIC["h2d_bytes"] + hipkkt.TRAFFIC["d2h_bytes"]) / it, 1e3 * solver.info.timers["IP iteration"] / it


@pytest.mark.parametrize("forced_dual", [False, True], ids=["default", "forced_dual"])
@pytest.mark.parametrize("name", list(END_TO_END))
def test_ipm_with_the_nonsymmetric_device_step_matches_the_host_path(name, forced_dual):
    extra = dict(min_switch_step_length=1.0) if forced_dual else {}
    prob = END_TO_END[name]()
    with _Timeout(120):
        ref_solver, ref, ref_bytes, ref_ms = _solve_counting(prob, **STEP_FLAGS, **extra)
        dev_solver, got, dev_bytes, dev_ms = _solve_counting(prob, **NONSYM, **extra)
    assert dev_solver._device_step and dev_solver.kktsystem.kktsolver.steps_nonsymmetric and not ref_solver._device_step
    st = dev_solver.settings
    print(f"[nonsym end to end {name} forced_dual={forced_dual}] host path: {ref.status}, {ref.iterations} iterations, {ref_bytes:.0f} bytes / "
          f"iteration, {ref_ms:.3f} ms / iteration; device step: {got.status}, {got.iterations} iterations, {dev_bytes:.0f} bytes / iteration, "
          f"{dev_ms:.3f} ms / iteration; |dobj| {abs(got.obj_val - ref.obj_val):.2e}; barrier searches {dev_solver.barrier_searches} "
          f"(backtracks {dev_solver.barrier_backtracks})")
    assert got.status == ref.status == ipm.SOLVED, (got.status, ref.status)
    assert abs(got.obj_val - ref.obj_val) <= 2.0 * max(st.tol_gap_abs, st.tol_gap_rel * max(1.0, abs(ref.obj_val)))
    assert got.iterations <= st.max_iter and ref.iterations <= st.max_iter
    assert dev_bytes < ref_bytes, (dev_bytes, ref_bytes)
    if forced_dual:
        assert dev_solver.barrier_searches > 0
