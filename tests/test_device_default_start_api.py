"""The default start on the device (Settings.device_default_start; include/hipkkt.h hipkkt_cone_set_identity_scaling /
hipkkt_cone_margins / hipkkt_cone_shift_to_interior / hipkkt_step_default_start_dev), checked without a GPU: the setting, the loop of
_solve_device_step on a host-served plugin, and the new symbols in the header, in both libraries, in the ctypes mirror and in the
Julia glue."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt
from julia_standin import ipm
from tests import default_start_reference as dr
from tests import fixtures as fx
from tests.step_support import STEP_SETTINGS, _FakeStepPlugin, _HostBuffer
from tests.test_julia_glue import JL_FILES, c_prototypes, jl_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hipkkt_cone_set_identity_scaling", "hipkkt_cone_margins", "hipkkt_cone_shift_to_interior", "hipkkt_step_default_start_dev")
FLAGS = dict(device_scaling=True, device_reduced=True, device_residuals=True)


class _FakeStartPlugin(_FakeStepPlugin):
    """_FakeStepPlugin plus the default start on the `resident` iterate: solver.jl:383-405 with the plugin's own cones and solves"""
    default_start_on_device = True

    def kktsolver_default_start(self, xzs):
        self.calls.append("default_start")
        v = ipm.Variables.zeros(self.n, self.m)
        self.cones.set_identity_scaling()
        ok = self.sys.kkt_update(self.data, self.cones)
        ok = ok and self.sys.kkt_solve_initial_point(v, self.data)
        s, mn_s, pos_s, tg_s, _ = dr.shift64(self.cones, v.s, "primal")
        z, mn_z, pos_z, tg_z, _ = dr.shift64(self.cones, v.z, "dual")
        xzs.a[:] = np.concatenate([v.x, z, s])
        return ok, np.array([0.0, 0.0, mn_s, pos_s, tg_s, mn_z, pos_z, tg_z])


class _FailingStartPlugin(_FakeStartPlugin):
    def kktsolver_default_start(self, xzs):
        self.calls.append("default_start")
        return False, np.zeros(8)


def test_the_setting_is_off_by_default_and_needs_device_step(oracle_factory):
    assert cl.Settings().device_default_start is False
    with pytest.raises(ValueError, match="device_default_start"):
        cl.Solver(*fx.basic_qp(), cl.Settings(device_default_start=True, **FLAGS), kktsolver_factory=oracle_factory)
    # a plugin without the step calls keeps the host loop and its host start, as with the other device_* flags
    S = cl.Solver(*fx.basic_qp(), cl.Settings(device_default_start=True, **STEP_SETTINGS), kktsolver_factory=oracle_factory)
    assert not S._device_step and not S._device_default_start
    # a plugin with the step calls but without the start keeps the host start
    S = cl.Solver(*fx.basic_qp(), cl.Settings(device_default_start=True, **STEP_SETTINGS), kktsolver_factory=lambda *a: _FakeStepPlugin(*a))
    assert S._device_step and not S._device_default_start
    # the flag off: a plugin that offers the start is not asked
    S = cl.Solver(*fx.basic_qp(), cl.Settings(**STEP_SETTINGS), kktsolver_factory=lambda *a: _FakeStartPlugin(*a))
    assert S._device_step and not S._device_default_start


@pytest.mark.parametrize("prob", [fx.basic_qp, fx.basic_lp, fx.basic_socp])
def test_the_loop_asks_the_plugin_for_the_start_and_neither_starts_nor_uploads_itself(prob, monkeypatch):
    ref_solver = cl.Solver(*prob(), cl.Settings(**STEP_SETTINGS), kktsolver_factory=lambda *a: _FakeStepPlugin(*a))
    ref_solver.trace = []
    ref = ref_solver.solve()
    dev = cl.Solver(*prob(), cl.Settings(device_default_start=True, **STEP_SETTINGS), kktsolver_factory=lambda *a: _FakeStartPlugin(*a))
    assert dev._device_step and dev._device_default_start

    def forbidden(*a, **k):
        raise AssertionError("the host default start / the upload of the iterate must not happen")
    monkeypatch.setattr(ipm.Solver, "_default_start", forbidden)
    monkeypatch.setattr(_HostBuffer, "upload", forbidden)
    dev.trace = []
    got = dev.solve()
    calls = dev.kktsystem.kktsolver.calls
    assert calls[0] == "default_start" and calls.count("default_start") == 1 and calls[1] == "residuals"
    assert (dev.variables.tau, dev.variables.kappa) != (0.0, 0.0)
    # the plugin computed what the host start computes: the trajectories coincide bit for bit
    assert got.status == ref.status and got.iterations == ref.iterations
    assert len(dev.trace) == len(ref_solver.trace)
    for a, b in zip(dev.trace, ref_solver.trace):
        assert a == b
    assert np.array_equal(got.x, ref.x) and np.array_equal(got.z, ref.z) and np.array_equal(got.s, ref.s)
    assert "default start" in dev.info.timers


def test_a_failed_start_ends_with_numerical_error():
    S = cl.Solver(*fx.basic_qp(), cl.Settings(device_default_start=True, **STEP_SETTINGS), kktsolver_factory=lambda *a: _FailingStartPlugin(*a))
    sol = S.solve()
    assert sol.status == ipm.NUMERICAL_ERROR and sol.iterations == 0
    assert S.kktsystem.kktsolver.calls == ["default_start"]


def test_header_binding_libraries_and_julia_glue_agree_on_the_new_entry_points():
    protos = c_prototypes()
    glue = {c[0] for c in jl_ccalls(JL_FILES[1])}          # julia/ext/hipkkt_lib.jl
    hdr = open(os.path.join(ROOT, "include", "hipkkt.h")).read()
    assert re.search(r"#define\s+HIPKKT_ABI_VERSION\s+5\b", hdr)
    added = hdr[hdr.index("Added within 5"):hdr.index("#define HIPKKT_ABI_VERSION")]
    pkg = os.path.dirname(hipkkt.__file__)
    libs = [C.CDLL(os.path.join(pkg, name)) for name in ("libclarabel_hipkkt.so", "libclarabel_hipkkt_testing.so")]
    for s in NEW:
        assert s in protos, f"{s} is not declared in include/hipkkt.h"
        assert s in added and s in hipkkt.SYMBOLS and s in glue
        for L in libs:
            assert hasattr(L, s), s
    L = hipkkt.lib()
    vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    assert list(L.hipkkt_cone_set_identity_scaling.argtypes) == [vp]
    assert len(L.hipkkt_cone_margins.argtypes) == 4 and L.hipkkt_cone_margins.argtypes[2] is i32
    assert len(L.hipkkt_cone_shift_to_interior.argtypes) == 4 and L.hipkkt_cone_shift_to_interior.argtypes[2] is i32
    a = list(L.hipkkt_step_default_start_dev.argtypes)
    assert a[:10] == [vp, vp, i32, f64, f64, i32, f64, f64, i64, f64] and len(a) == 12 and a[11] is vp
    for name in ("cone_set_identity_scaling", "cone_margins", "cone_shift_to_interior", "step_default_start_dev"):
        assert hasattr(hipkkt.Handle, name), name
    from clarabel_jl_amd.kktsolver import HipKKTSolver
    assert hasattr(HipKKTSolver, "kktsolver_default_start") and isinstance(HipKKTSolver.default_start_on_device, property)
    assert hipkkt.ABI_VERSION == 5 and L.hipkkt_abi_version() == 5
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW + ("device_default_start", "hip_step_default_start_dev!"):
        assert s in text, s
