"""The device-resident interior-point step (Settings.device_step, include/hipkkt.h hipkkt_cone_* / hipkkt_step_*), checked without a
GPU: the header, the ctypes mirror and the Julia glue agree on the new entry points within ABI version 5; the setting is off by
default and demands the three flags it builds on; only Zero / Nonnegative / SecondOrder cone sets qualify; and the stand-in's
device_step loop, driven by a plugin that implements the step methods with the stand-in's own numpy cones and the CPU oracle, follows
the host loop bit for bit."""
import os
import re

import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt
from clarabel_jl_amd.kktsolver import cone_set_steps_on_device
from julia_standin import ipm
from julia_standin.cones import CompositeCone
from tests import fixtures as fx
from tests.test_julia_glue import JL_FILES, c_prototypes, jl_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEP_SYMBOLS = ["hipkkt_cone_affine_ds", "hipkkt_cone_combined_ds_shift", "hipkkt_cone_ds_from_dz_offset", "hipkkt_cone_mul_hs",
                "hipkkt_cone_step_length", "hipkkt_set_equilibration", "hipkkt_step_affine_dev", "hipkkt_step_combined_dev",
                "hipkkt_step_apply_dev", "hipkkt_step_info_norms_dev", "hipkkt_step_get"]


def test_header_binding_and_julia_glue_agree_on_the_step_entry_points():
    protos = c_prototypes()
    glue = {c[0] for c in jl_ccalls(JL_FILES[1])}          # julia/ext/hipkkt_lib.jl
    L = hipkkt.lib()
    for s in STEP_SYMBOLS:
        assert s in protos, f"{s} is not declared in include/hipkkt.h"
        assert s in hipkkt.SYMBOLS and hasattr(L, s), s
        assert s in glue, f"{s} has no wrapper in julia/ext/hipkkt_lib.jl"
    # every pointer of the fused calls except the scalar arrays is a device pointer by name
    for s in ("hipkkt_step_affine_dev", "hipkkt_step_combined_dev"):
        params = protos[s][1]
        assert "xzs_dev" in params[1] and "res_dev" in params[2]
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hipkkt_step_apply_dev" in text and "device_step" in text


def test_the_abi_version_is_still_5():
    hdr = open(os.path.join(ROOT, "include", "hipkkt.h")).read()
    assert re.search(r"#define\s+HIPKKT_ABI_VERSION\s+5\b", hdr)
    assert hipkkt.ABI_VERSION == 5 and hipkkt.lib().hipkkt_abi_version() == 5
    assert "Added within 5" in hdr


def test_device_step_is_off_by_default_and_needs_the_three_flags():
    assert cl.Settings().device_step is False
    prob = fx.basic_qp()
    for missing in ("device_scaling", "device_reduced", "device_residuals"):
        kw = dict(device_step=True, device_scaling=True, device_reduced=True, device_residuals=True)
        kw[missing] = False
        with pytest.raises(ValueError):
            cl.Solver(*prob, cl.Settings(**kw), kktsolver_factory=lambda *a: _FakeStepPlugin(*a))


def test_steps_on_device_only_for_zero_nonnegative_and_second_order_cones():
    T = cl
    yes = [[T.ZeroConeT(2)], [T.NonnegativeConeT(3)], [T.SecondOrderConeT(3), T.SecondOrderConeT(9)],
           [T.ZeroConeT(1), T.NonnegativeConeT(4), T.SecondOrderConeT(6)]]
    no = [[T.PSDTriangleConeT(3)], [T.NonnegativeConeT(2), T.PSDTriangleConeT(2)], [T.ExponentialConeT()],
          [T.ZeroConeT(1), T.PowerConeT(0.3)], [T.GenPowerConeT([0.6, 0.4], 1), T.NonnegativeConeT(2)], []]
    for specs in yes:
        assert cone_set_steps_on_device(CompositeCone(specs)), specs
    for specs in no:
        assert not cone_set_steps_on_device(CompositeCone(specs)), specs


# ---- orchestration -------------------------------------------------------------------------------------------------------------------

class _HostBuffer:
    """what the plugin hands out as device memory, here a numpy array"""

    def __init__(self, n):
        self.a = np.zeros(n)

    def upload(self, host):
        self.a[:] = host

    def download(self):
        return self.a.copy()

    def copy_from(self, other):
        self.a[:] = other.a

    def close(self):
        pass


class _Data:
    pass


class _FakeStepPlugin:
    """The plugin interface of the device_step loop (clarabel.jl_amd/kktsolver.py) served on the host: the KKT solves by the CPU
    oracle, the cone algebra by the stand-in's numpy cones and its own kkt_solve -- exactly what the host loop computes, so the two
    trajectories must coincide bit for bit if the loop hands the right quantities over in the right order."""
    steps_on_device = True

    def __init__(self, P, A, cones, m, n, settings):
        from oracle.kkt_oracle import OracleKKTSolver

        self.settings = settings
        self.inner = OracleKKTSolver(P, A, cones, m, n, settings)
        self.cones, self.m, self.n = cones, m, n
        self.data = _Data()
        self.data.P, self.data.A = P, A
        self.sys = ipm.KKTSystem(self.inner, m, n)
        self.lhs, self.rhs = ipm.Variables.zeros(n, m), ipm.Variables.zeros(n, m)
        self.calls = []

    # the contract methods the default start needs
    def kktsolver_update(self, cones):
        return self.inner.kktsolver_update(cones)

    def kktsolver_setrhs(self, rx, rz):
        self.inner.kktsolver_setrhs(rx, rz)

    def kktsolver_solve(self, lx, lz):
        return self.inner.kktsolver_solve(lx, lz)

    def set_problem_vectors(self, q, b):
        self.data.q, self.data.b = q, b

    def set_equilibration(self, d, e):
        self.d, self.e, self.dinv, self.einv = d, e, 1.0 / d, 1.0 / e

    def device_buffer(self, n):
        return _HostBuffer(n)

    def _split(self, xzs):
        n, m = self.n, self.m
        return xzs.a[:n], xzs.a[n:n + m], xzs.a[n + m:]

    def _res(self, res):
        n, m = self.n, self.m
        o = np.cumsum([0, n, m, n, m, n])
        return [res.a[o[k]:o[k + 1]] for k in range(5)]

    def residuals_update_dev(self, xzs, res, tau, kappa):      # residuals.jl:1-37 as ipm.Solver._residuals_update
        self.calls.append("residuals")
        x, z, s = self._split(xzs)
        rx, rz, rx_inf, rz_inf, Px = self._res(res)
        d = self.data
        qx, bz, sz = float(np.dot(d.q, x)), float(np.dot(d.b, z)), float(np.dot(s, z))
        Px[:] = ipm._symv(d.P, x)
        xPx = float(np.dot(x, Px))
        rx_inf[:] = -(d.A.T @ z)
        rz_inf[:] = s + d.A @ x
        rx[:] = rx_inf - Px - d.q * tau
        rz[:] = rz_inf - d.b * tau
        return qx, bz, sz, xPx, qx + bz + kappa + xPx / tau

    def kktsolver_info_norms(self, xzs, res):
        self.calls.append("norms")
        x, z, s = self._split(xzs)
        rx, rz, rx_inf, rz_inf, Px = self._res(res)
        ns = ipm._norm_scaled
        return [ns(self.d, x), ns(self.e, z), ns(self.einv, s), ns(self.dinv, rx), ns(self.einv, rz), ns(self.dinv, rx_inf),
                ns(self.einv, rz_inf), ns(self.dinv, Px)]

    def kktsolver_update_scaling_dev(self, xzs):
        self.calls.append("scaling")
        _, z, s = self._split(xzs)
        return self.cones.update_scaling(s, z, 0.0)

    def kktsolver_refactor(self):
        self.calls.append("refactor")
        return self.sys.kkt_update(self.data, self.cones)

    def _vars(self, xzs, tau, kappa):
        x, z, s = self._split(xzs)
        return ipm.Variables(x, s, z, tau, kappa)

    def _alpha(self, v, fraction):      # variables.jl:14-43
        step = self.lhs
        a_tau = -v.tau / step.tau if step.tau < 0 else ipm.FLOATMAX
        a_kap = -v.kappa / step.kappa if step.kappa < 0 else ipm.FLOATMAX
        alpha = min(a_tau, a_kap, 1.0)
        az, as_ = self.cones.step_length(step.z, step.s, v.z, v.s, alpha)
        return min(az, as_) * fraction

    def kktsolver_step_affine(self, xzs, res, tau, kappa, r_tau, const_pending):
        self.calls.append("affine")
        assert const_pending
        v, rhs, lhs = self._vars(xzs, tau, kappa), self.rhs, self.lhs
        rx, rz = self._res(res)[:2]
        rhs.x[:] = rx
        rhs.z[:] = rz
        self.cones.affine_ds(rhs.s, v.s)
        rhs.tau, rhs.kappa = r_tau, tau * kappa
        if not self.sys.kkt_solve(lhs, rhs, self.data, v, self.cones, "affine"):
            return False, 0.0, 0.0, 0.0
        return True, self._alpha(v, 1.0), lhs.tau, lhs.kappa

    def kktsolver_step_combined(self, xzs, res, tau, kappa, r_tau, dtau_aff, dkappa_aff, sigma, mu, m_corr):
        self.calls.append("combined")
        v, rhs, lhs = self._vars(xzs, tau, kappa), self.rhs, self.lhs
        assert (dtau_aff, dkappa_aff) == (lhs.tau, lhs.kappa)
        rx, rz = self._res(res)[:2]
        sm = sigma * mu
        rhs.x[:] = (1.0 - sigma) * rx
        rhs.tau = (1.0 - sigma) * r_tau
        rhs.kappa = -sm + m_corr * lhs.tau * lhs.kappa + tau * kappa
        if m_corr != 1.0:
            lhs.z *= m_corr
        self.cones.affine_ds(rhs.s, v.s)
        self.cones.combined_ds_shift(rhs.z, lhs.z, lhs.s, sm)
        rhs.s += rhs.z
        rhs.z[:] = (1.0 - sigma) * rz
        if not self.sys.kkt_solve(lhs, rhs, self.data, v, self.cones, "combined"):
            return False, 0.0, 0.0, 0.0
        return True, self._alpha(v, self.settings.max_step_fraction), lhs.tau, lhs.kappa

    def kktsolver_step_apply(self, alpha, xzs):
        self.calls.append("apply")
        x, z, s = self._split(xzs)
        x += alpha * self.lhs.x
        z += alpha * self.lhs.z
        s += alpha * self.lhs.s


ORCHESTRATION_CASES = {
    "basic_qp": (fx.basic_qp, ipm.SOLVED), "basic_lp": (fx.basic_lp, ipm.SOLVED), "basic_socp": (fx.basic_socp, ipm.SOLVED),
    "lasso_socp": (fx.lasso_socp, ipm.SOLVED), "basic_qp_dualinf": (fx.basic_qp_dualinf, ipm.DUAL_INFEASIBLE),
    "eq_constrained": (fx.eq_constrained, ipm.SOLVED),
}
STEP_SETTINGS = dict(device_step=True, device_scaling=True, device_reduced=True, device_residuals=True)


@pytest.mark.parametrize("name", list(ORCHESTRATION_CASES))
def test_device_step_loop_reproduces_the_host_loop_bit_for_bit(name, oracle_factory):
    make, status = ORCHESTRATION_CASES[name]
    prob = make()
    host = cl.Solver(*prob, cl.Settings(), kktsolver_factory=oracle_factory)
    host.trace = []
    sol_h = host.solve()
    assert sol_h.status == status, sol_h.status          # the host loop ends where the reference's own test says
    dev = cl.Solver(*prob, cl.Settings(**STEP_SETTINGS), kktsolver_factory=lambda *a: _FakeStepPlugin(*a))
    assert dev._device_step
    dev.trace = []
    sol_d = dev.solve()
    assert sol_d.status == sol_h.status and sol_d.iterations == sol_h.iterations
    assert len(dev.trace) == len(host.trace)
    for th, td in zip(host.trace, dev.trace):
        assert th == td, (th, td)                         # alpha, sigma, mu, costs, residuals, kappa / tau per iteration
    for a in ("x", "z", "s"):
        assert np.array_equal(getattr(sol_d, a), getattr(sol_h, a)), a
    assert (sol_d.obj_val == sol_h.obj_val or (np.isnan(sol_d.obj_val) and np.isnan(sol_h.obj_val)))
    assert (dev.variables.tau, dev.variables.kappa) == (host.variables.tau, host.variables.kappa)
    # the order the issue prescribes: residuals, norms, (termination,) scaling, refactor, affine, combined, apply
    calls = dev.kktsystem.kktsolver.calls
    per_iter = ["residuals", "norms", "scaling", "refactor", "affine", "combined", "apply"]
    assert calls[:len(per_iter) * sol_d.iterations] == per_iter * sol_d.iterations
    assert calls[len(per_iter) * sol_d.iterations:] == ["residuals", "norms"]


def test_other_cone_sets_silently_take_the_host_loop(oracle_factory):
    class NoSteps(_FakeStepPlugin):
        steps_on_device = False

    prob = fx.basic_sdp()
    ref = cl.Solver(*prob, cl.Settings(), kktsolver_factory=oracle_factory).solve()
    S = cl.Solver(*prob, cl.Settings(**STEP_SETTINGS), kktsolver_factory=lambda *a: NoSteps(*a))
    assert not S._device_step
    got = S.solve()
    assert got.status == ref.status == ipm.SOLVED and got.iterations == ref.iterations and np.array_equal(got.x, ref.x)
    assert S.kktsystem.kktsolver.calls == []
