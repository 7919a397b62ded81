"""The device-resident interior-point step for cone sets with Exponential / Power members (Settings.device_step_nonsymmetric,
include/hipkkt.h hipkkt_step_enable_cone3 / hipkkt_cone_barrier / hipkkt_step_barrier_dev), checked without a GPU: the setting, the
qualification rule, the three new symbols in the header, the ctypes mirror and the Julia glue; and the stand-in's non-symmetric
device-step loop, driven by a plugin that serves the step methods with the stand-in's numpy cones and the CPU oracle, follows the host
loop bit for bit -- under default settings (PrimalDual throughout on these problems) and with min_switch_step_length = 1, which
forces the Dual strategy and its barrier search from the first iteration on."""
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
from tests.step_support import NONSYM_SETTINGS, STEP_SETTINGS, _FakeNonsymPlugin
from tests.test_julia_glue import JL_FILES, c_prototypes, jl_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["hipkkt_step_enable_cone3", "hipkkt_cone_barrier", "hipkkt_step_barrier_dev"]


def test_the_setting_is_off_by_default_and_needs_device_step():
    assert cl.Settings().device_step_nonsymmetric is False
    kw = dict(NONSYM_SETTINGS, device_step=False)
    with pytest.raises(ValueError):
        cl.Solver(*fx.basic_exp(), cl.Settings(**kw), kktsolver_factory=lambda *a: _FakeNonsymPlugin(*a))


def test_exponential_and_power_sets_qualify_only_when_asked():
    T = cl
    yes = [[T.ExponentialConeT()], [T.PowerConeT(0.3)], [T.ZeroConeT(1), T.PowerConeT(0.3)],
           [T.ZeroConeT(2), T.NonnegativeConeT(3), T.SecondOrderConeT(5), T.ExponentialConeT(), T.PowerConeT(0.5)],
           [T.NonnegativeConeT(3)], [T.SecondOrderConeT(3), T.ZeroConeT(1)]]
    no = [[T.GenPowerConeT([0.6, 0.4], 1), T.NonnegativeConeT(2)], [T.ExponentialConeT(), T.GenPowerConeT([0.6, 0.4], 1)],
          [T.PSDTriangleConeT(3)], [T.PowerConeT(0.2), T.PSDTriangleConeT(2)], []]
    for specs in yes:
        assert cone_set_steps_on_device(CompositeCone(specs), nonsymmetric=True), specs
    for specs in no:
        assert not cone_set_steps_on_device(CompositeCone(specs), nonsymmetric=True), specs
        assert not cone_set_steps_on_device(CompositeCone(specs)), specs
    # the one-argument form is what it was
    for specs in yes[:4]:
        assert not cone_set_steps_on_device(CompositeCone(specs)), specs
        assert not cone_set_steps_on_device(CompositeCone(specs), nonsymmetric=False), specs
    for specs in yes[4:]:
        assert cone_set_steps_on_device(CompositeCone(specs)), specs


def test_header_binding_and_julia_glue_agree_on_the_new_entry_points():
    protos = c_prototypes()
    glue = {c[0] for c in jl_ccalls(JL_FILES[1])}          # julia/ext/hipkkt_lib.jl
    L = hipkkt.lib()
    for s in NEW_SYMBOLS:
        assert s in protos, f"{s} is not declared in include/hipkkt.h"
        assert s in hipkkt.SYMBOLS and hasattr(L, s), s
        assert s in glue, f"{s} has no wrapper in julia/ext/hipkkt_lib.jl"
    assert "xzs_dev" in protos["hipkkt_step_barrier_dev"][1][1]
    hdr = open(os.path.join(ROOT, "include", "hipkkt.h")).read()
    assert re.search(r"#define\s+HIPKKT_ABI_VERSION\s+5\b", hdr) and "Added within 5" in hdr
    assert hipkkt.ABI_VERSION == 5 and L.hipkkt_abi_version() == 5
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hipkkt_step_enable_cone3" in text and "device_step_nonsymmetric" in text


# ---- orchestration -------------------------------------------------------------------------------------------------------------------


def _mix20():
    return problems.nonsymmetric_mix(n=20, nexp=5, npow=4, ngenpow=0, nn=6, nzero=2, socdim=4, seed=9)


def _mix80():
    return problems.nonsymmetric_mix(n=80, nexp=30, npow=20, ngenpow=0, nn=20, nzero=3, socdim=5, seed=5)


LOOP_CASES = {"basic_exp": fx.basic_exp, "basic_pow": fx.basic_pow, "mix20": _mix20}
# iterations under min_switch_step_length = 1 (Dual from the first iteration on), from the host loop on the CPU oracle
FORCED_DUAL_ITERATIONS = {"basic_exp": 18, "basic_pow": 15, "mix20": 20, "mix80": 23}


@pytest.mark.parametrize("forced_dual", [False, True], ids=["default", "forced_dual"])
@pytest.mark.parametrize("name", list(LOOP_CASES))
def test_nonsymmetric_device_step_loop_reproduces_the_host_loop_bit_for_bit(name, forced_dual, oracle_factory):
    prob = LOOP_CASES[name]()
    extra = dict(min_switch_step_length=1.0) if forced_dual else {}
    host = cl.Solver(*prob, cl.Settings(**extra), kktsolver_factory=oracle_factory)
    host.trace = []
    sol_h = host.solve()
    assert sol_h.status == ipm.SOLVED, sol_h.status
    dev = cl.Solver(*prob, cl.Settings(**NONSYM_SETTINGS, **extra), kktsolver_factory=lambda *a: _FakeNonsymPlugin(*a))
    assert dev._device_step and not dev.cones.is_symmetric()
    dev.trace = []
    sol_d = dev.solve()
    assert sol_d.status == sol_h.status and sol_d.iterations == sol_h.iterations
    assert len(dev.trace) == len(host.trace)
    for th, td in zip(host.trace, dev.trace):
        assert th == td, (th, td)
    for a in ("x", "z", "s"):
        assert np.array_equal(getattr(sol_d, a), getattr(sol_h, a)), a
    assert sol_d.obj_val == sol_h.obj_val
    assert (dev.variables.tau, dev.variables.kappa) == (host.variables.tau, host.variables.kappa)
    assert (dev.barrier_searches, dev.barrier_backtracks) == (host.barrier_searches, host.barrier_backtracks)
    calls = dev.kktsystem.kktsolver.calls
    print(f"[nonsym loop] {name} forced_dual={forced_dual}: {sol_d.iterations} iterations, {dev.barrier_searches} barrier searches, "
          f"{dev.barrier_backtracks} barrier backtracks, {calls.count('scaling_ex:dual')} Dual scalings")
    if forced_dual:
        assert sol_h.iterations == FORCED_DUAL_ITERATIONS[name]
        assert 14 <= dev.barrier_searches <= 22 and "scaling_ex:dual" in calls and "barrier" in calls
        if name == "basic_exp":
            assert dev.barrier_backtracks == 2
    else:      # Dual is never reached on these problems under default settings: the forced case is the coverage of that branch
        assert dev.barrier_searches == 0 and "scaling_ex:dual" not in calls


def test_forced_dual_still_solves_the_larger_mix_on_the_host_loop(oracle_factory):
    sol = cl.Solver(*_mix80(), cl.Settings(min_switch_step_length=1.0), kktsolver_factory=oracle_factory).solve()
    assert sol.status == ipm.SOLVED and sol.iterations == FORCED_DUAL_ITERATIONS["mix80"]


def test_a_genpower_set_silently_takes_the_host_loop(oracle_factory):
    prob = fx.basic_genpow()
    ref = cl.Solver(*prob, cl.Settings(), kktsolver_factory=oracle_factory).solve()
    S = cl.Solver(*prob, cl.Settings(**NONSYM_SETTINGS), kktsolver_factory=lambda *a: _FakeNonsymPlugin(*a))
    assert not S._device_step
    got = S.solve()
    assert got.status == ref.status == ipm.SOLVED and got.iterations == ref.iterations and np.array_equal(got.x, ref.x)
    assert S.kktsystem.kktsolver.calls == []


def test_an_exponential_set_keeps_the_host_loop_without_the_setting(oracle_factory):
    S = cl.Solver(*fx.basic_exp(), cl.Settings(**STEP_SETTINGS), kktsolver_factory=lambda *a: _FakeNonsymPlugin(*a))
    assert not S._device_step


# ---- the strategy checkpoints of the new loop, forced -------------------------------------------------------------------------------

def _force_insufficient_progress(solver, at_call):
    """the at_call-th termination test reports INSUFFICIENT_PROGRESS (solver.jl:453-473 then restores the previous iterate)"""
    orig, count = solver._check_termination, [0]

    def check(it):
        count[0] += 1
        if count[0] == at_call:
            solver.info.status = ipm.INSUFFICIENT_PROGRESS
            return True
        return orig(it)
    solver._check_termination = check


def _fail_once(obj, name, at_call, result):
    orig, count = getattr(obj, name), [0]

    def call(*a, **k):
        count[0] += 1
        if count[0] == at_call:
            return result
        return orig(*a, **k)
    setattr(obj, name, call)


def _same_run(host, dev):
    sol_h, sol_d = host.solve(), dev.solve()
    assert sol_d.status == sol_h.status and sol_d.iterations == sol_h.iterations, (sol_d.status, sol_h.status, sol_d.iterations, sol_h.iterations)
    assert len(dev.trace) == len(host.trace)
    for th, td in zip(host.trace, dev.trace):
        assert th == td, (th, td)
    for a in ("x", "z", "s"):
        assert np.array_equal(getattr(sol_d, a), getattr(sol_h, a)), a
    return sol_h, sol_d


def _pair(prob, oracle_factory):
    host = cl.Solver(*prob, cl.Settings(), kktsolver_factory=oracle_factory)
    dev = cl.Solver(*prob, cl.Settings(**NONSYM_SETTINGS), kktsolver_factory=lambda *a: _FakeNonsymPlugin(*a))
    assert dev._device_step
    host.trace, dev.trace = [], []
    return host, dev


def test_insufficient_progress_restores_the_iterate_and_switches_to_dual(oracle_factory):
    host, dev = _pair(_mix20(), oracle_factory)
    for S in (host, dev):
        _force_insufficient_progress(S, 5)
    sol_h, sol_d = _same_run(host, dev)
    calls = dev.kktsystem.kktsolver.calls
    assert sol_d.status == ipm.SOLVED and "scaling_ex:dual" in calls and dev.barrier_searches > 0
    assert calls.index("scaling_ex:dual") > calls.index("scaling_ex:primal_dual")


def test_a_failed_solve_switches_to_dual_and_fails_under_dual(oracle_factory):
    # the combined solve of the third iteration fails: PrimalDual -> Dual, the iteration is repeated on the same iterate
    host, dev = _pair(_mix20(), oracle_factory)
    _fail_once(host.kktsystem, "kkt_solve", 6, False)
    _fail_once(dev.kktsystem.kktsolver, "kktsolver_step_combined", 3, (False, 0.0, 0.0, 0.0))
    sol_h, sol_d = _same_run(host, dev)
    assert sol_d.status == ipm.SOLVED and "scaling_ex:dual" in dev.kktsystem.kktsolver.calls
    # ... and a second failure, now under Dual, ends both loops with NUMERICAL_ERROR
    host, dev = _pair(_mix20(), oracle_factory)
    for k in (6, 8):
        _fail_once(host.kktsystem, "kkt_solve", k, False)
    for k in (3, 4):
        _fail_once(dev.kktsystem.kktsolver, "kktsolver_step_combined", k, (False, 0.0, 0.0, 0.0))
    sol_h, sol_d = _same_run(host, dev)
    assert sol_d.status == ipm.NUMERICAL_ERROR


def test_a_failed_scaling_is_told_apart_by_the_cone_that_failed(oracle_factory):
    # an Exponential / Power member: the numerical-error checkpoint (kkt_update! fails on the host path with device_scaling)
    _, dev = _pair(_mix20(), oracle_factory)
    _fail_once(dev.kktsystem.kktsolver, "kktsolver_update_scaling_dev_ex", 3, False)
    sol = dev.solve()
    calls = dev.kktsystem.kktsolver.calls
    assert sol.status == ipm.SOLVED and "scaling_ex:dual" in calls
    # a symmetric member that is not interior: NUMERICAL_ERROR before the iteration counts, as update_scaling! of the host loop
    _, dev = _pair(_mix20(), oracle_factory)
    ks = dev.kktsystem.kktsolver
    orig, count = ks.kktsolver_update_scaling_dev_ex, [0]

    def scaling(xzs, mu, strategy):
        count[0] += 1
        if count[0] == 3:
            soc = next(r for c, r in zip(ks.cones.cones, ks.cones.rng_cones) if type(c).__name__ == "SecondOrderCone")
            xzs.a[ks.n + ks.m + soc.start] = -1.0         # s of the second-order cone leaves it
            return False
        return orig(xzs, mu, strategy)
    ks.kktsolver_update_scaling_dev_ex = scaling
    sol = dev.solve()
    assert sol.status == ipm.NUMERICAL_ERROR and sol.iterations == 2
