"""The device-resident interior-point step for cone sets with Generalized Power members (Settings.device_step_genpower,
include/hipkkt.h hipkkt_step_enable_genpow), checked without a GPU: the setting, the qualification rule, the new symbol in the header,
the ctypes mirror, the library and the Julia glue; and the stand-in's non-symmetric device-step loop on such sets, driven by a plugin
that serves the step methods with the stand-in's numpy cones and the CPU oracle, reproduces the host loop exactly."""
import os
import re

import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt, problems
from clarabel_jl_amd.kktsolver import cone_set_steps_on_device
from julia_standin import ipm
from julia_standin.cones import CompositeCone
from tests import fixtures as fx
from tests.step_support import NONSYM_SETTINGS, _FakeNonsymPlugin
from tests.test_julia_glue import JL_FILES, c_prototypes, jl_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENPOW_SETTINGS = dict(NONSYM_SETTINGS, device_step_genpower=True)


def test_the_setting_is_off_by_default_and_needs_device_step_nonsymmetric():
    assert cl.Settings().device_step_genpower is False
    kw = dict(GENPOW_SETTINGS, device_step_nonsymmetric=False)
    with pytest.raises(ValueError, match="device_step_genpower"):
        cl.Solver(*fx.basic_genpow(), cl.Settings(**kw), kktsolver_factory=lambda *a: _FakeNonsymPlugin(*a))
    # the existing check still comes first
    with pytest.raises(ValueError):
        cl.Solver(*fx.basic_genpow(), cl.Settings(**dict(GENPOW_SETTINGS, device_step=False)),
                  kktsolver_factory=lambda *a: _FakeNonsymPlugin(*a))


def test_generalized_power_sets_qualify_only_when_asked():
    T = cl
    yes = [[T.ExponentialConeT()], [T.PowerConeT(0.3)], [T.ZeroConeT(1), T.PowerConeT(0.3)],
           [T.ZeroConeT(2), T.NonnegativeConeT(3), T.SecondOrderConeT(5), T.ExponentialConeT(), T.PowerConeT(0.5)],
           [T.NonnegativeConeT(3)], [T.SecondOrderConeT(3), T.ZeroConeT(1)]]
    genpow = [[T.GenPowerConeT([0.6, 0.4], 1), T.NonnegativeConeT(2)], [T.ExponentialConeT(), T.GenPowerConeT([0.6, 0.4], 1)],
              [T.GenPowerConeT([0.2, 0.3, 0.5], 3)]]
    no = [[T.PSDTriangleConeT(3)], [T.PowerConeT(0.2), T.PSDTriangleConeT(2)], [], [T.GenPowerConeT([0.6, 0.4], 1), T.PSDTriangleConeT(2)]]
    for specs in yes + genpow:
        assert cone_set_steps_on_device(CompositeCone(specs), nonsymmetric=True, genpower=True), specs
    for specs in genpow + no:
        # the one- and two-argument forms answer what they answered before
        assert not cone_set_steps_on_device(CompositeCone(specs)), specs
        assert not cone_set_steps_on_device(CompositeCone(specs), nonsymmetric=True), specs
        assert not cone_set_steps_on_device(CompositeCone(specs), nonsymmetric=True, genpower=False), specs
    for specs in no:
        assert not cone_set_steps_on_device(CompositeCone(specs), nonsymmetric=True, genpower=True), specs
    for specs in yes:
        assert cone_set_steps_on_device(CompositeCone(specs), nonsymmetric=True), specs
    for specs in yes[:4]:
        assert not cone_set_steps_on_device(CompositeCone(specs)), specs
        assert not cone_set_steps_on_device(CompositeCone(specs), genpower=True), specs      # (genpower alone widens nothing)
    for specs in yes[4:]:
        assert cone_set_steps_on_device(CompositeCone(specs)), specs


def test_header_binding_library_and_julia_glue_agree_on_the_new_entry_point():
    s = "hipkkt_step_enable_genpow"
    protos = c_prototypes()
    glue = {c[0] for c in jl_ccalls(JL_FILES[1])}          # julia/ext/hipkkt_lib.jl
    L = hipkkt.lib()
    assert s in protos, f"{s} is not declared in include/hipkkt.h"
    assert protos[s] == protos["hipkkt_step_enable_cone3"]      # the same signature
    assert s in hipkkt.SYMBOLS and hasattr(L, s) and hasattr(hipkkt.Handle, "step_enable_genpow")
    assert s in glue, f"{s} has no wrapper in julia/ext/hipkkt_lib.jl"
    hdr = open(os.path.join(ROOT, "include", "hipkkt.h")).read()
    assert re.search(r"#define\s+HIPKKT_ABI_VERSION\s+5\b", hdr)
    added = hdr[hdr.index("Added within 5"):hdr.index("#define HIPKKT_ABI_VERSION")]
    assert s in added
    assert hipkkt.ABI_VERSION == 5 and L.hipkkt_abi_version() == 5
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert s in text and "device_step_genpower" in text and "hip_step_enable_genpow!" in text


# ---- orchestration -------------------------------------------------------------------------------------------------------------------

def _mix_genpow():
    return problems.nonsymmetric_mix(n=20, nexp=3, npow=3, ngenpow=3, nn=6, nzero=2, socdim=4, seed=9)


LOOP_CASES = {"basic_genpow": fx.basic_genpow, "mix_genpow": _mix_genpow}


@pytest.mark.parametrize("name", list(LOOP_CASES))
def test_genpower_device_step_loop_reproduces_the_host_loop(name, oracle_factory):
    prob = LOOP_CASES[name]()
    host = cl.Solver(*prob, cl.Settings(), kktsolver_factory=oracle_factory)
    host.trace = []
    sol_h = host.solve()
    assert sol_h.status == ipm.SOLVED, sol_h.status
    dev = cl.Solver(*prob, cl.Settings(**GENPOW_SETTINGS), kktsolver_factory=lambda *a: _FakeNonsymPlugin(*a))
    assert dev._device_step and not dev.cones.is_symmetric() and not dev.cones.allows_primal_dual_scaling()
    dev.trace = []
    sol_d = dev.solve()
    assert sol_d.status == sol_h.status and sol_d.iterations == sol_h.iterations
    assert np.array_equal(sol_d.x, sol_h.x)
    assert len(dev.trace) == len(host.trace)
    for th, td in zip(host.trace, dev.trace):
        assert th == td, (th, td)
    calls = dev.kktsystem.kktsolver.calls
    # a set with a Generalized Power member runs the Dual strategy throughout: every iteration searches the barrier
    assert "scaling_ex:dual" in calls and "scaling_ex:primal_dual" not in calls and "barrier" in calls
    assert dev.barrier_searches == host.barrier_searches >= sol_d.iterations - 1
    print(f"[genpow loop] {name}: {sol_d.iterations} iterations, {dev.barrier_searches} barrier searches, {dev.barrier_backtracks} backtracks")


def test_a_genpower_set_keeps_the_host_loop_without_the_setting(oracle_factory):
    S = cl.Solver(*_mix_genpow(), cl.Settings(**NONSYM_SETTINGS), kktsolver_factory=lambda *a: _FakeNonsymPlugin(*a))
    assert not S._device_step
    sol = S.solve()
    assert sol.status == ipm.SOLVED and S.kktsystem.kktsolver.calls == []
