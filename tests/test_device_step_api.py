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
from tests.step_support import STEP_SETTINGS, _FakeStepPlugin
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


ORCHESTRATION_CASES = {
    "basic_qp": (fx.basic_qp, ipm.SOLVED), "basic_lp": (fx.basic_lp, ipm.SOLVED), "basic_socp": (fx.basic_socp, ipm.SOLVED),
    "lasso_socp": (fx.lasso_socp, ipm.SOLVED), "basic_qp_dualinf": (fx.basic_qp_dualinf, ipm.DUAL_INFEASIBLE),
    "eq_constrained": (fx.eq_constrained, ipm.SOLVED),
}


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
