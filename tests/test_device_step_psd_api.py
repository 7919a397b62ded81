"""The device-resident interior-point step for PSD triangle cones (Settings.device_step_psd, include/hipkkt.h hipkkt_step_enable_psd /
hipkkt_psd_set_factors[_dev]), checked without a GPU: the setting, the qualification rule, the new symbols in the header, in both
libraries, in the ctypes mirror and in the Julia glue."""
import ctypes as C
import os
import re

import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt
from clarabel_jl_amd.kktsolver import cone_set_steps_on_device
from julia_standin.cones import CompositeCone
from tests import fixtures as fx
from tests.test_julia_glue import JL_FILES, c_prototypes, jl_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hipkkt_step_enable_psd", "hipkkt_psd_set_factors", "hipkkt_psd_set_factors_dev")
FLAGS = dict(device_scaling=True, device_reduced=True, device_residuals=True)


def test_the_setting_is_off_by_default_and_needs_device_step(oracle_factory):
    assert cl.Settings().device_step_psd is False
    with pytest.raises(ValueError, match="device_step_psd"):
        cl.Solver(*fx.basic_sdp(), cl.Settings(device_step_psd=True, **FLAGS), kktsolver_factory=oracle_factory)
    # a plugin without the step calls keeps the host loop, as with the other device_* flags
    S = cl.Solver(*fx.basic_sdp(), cl.Settings(device_step=True, device_step_psd=True, **FLAGS), kktsolver_factory=oracle_factory)
    assert not S._device_step and not S._device_step_psd


def test_psd_sets_qualify_only_when_asked_and_only_up_to_the_lds_maximum():
    T = cl
    yes = [[T.PSDTriangleConeT(64)], [T.PSDTriangleConeT(1)], [T.NonnegativeConeT(3), T.PSDTriangleConeT(3), T.SecondOrderConeT(4),
                                                                T.PSDTriangleConeT(1), T.ZeroConeT(2), T.PSDTriangleConeT(8)]]
    no = [[T.PSDTriangleConeT(65)], [T.PSDTriangleConeT(3), T.PSDTriangleConeT(65)], [T.PSDTriangleConeT(3), T.PowerConeT(0.3)],
          [T.PSDTriangleConeT(3), T.ExponentialConeT()], [T.GenPowerConeT([0.6, 0.4], 1), T.PSDTriangleConeT(2)], []]
    for specs in yes:
        assert cone_set_steps_on_device(CompositeCone(specs), psd=True), specs
        assert not cone_set_steps_on_device(CompositeCone(specs)), specs
        assert not cone_set_steps_on_device(CompositeCone(specs), nonsymmetric=True, genpower=True), specs
    for specs in no:
        assert not cone_set_steps_on_device(CompositeCone(specs), psd=True), specs
        assert not cone_set_steps_on_device(CompositeCone(specs), nonsymmetric=True, genpower=True, psd=True), specs
    # psd=True widens nothing else
    assert cone_set_steps_on_device(CompositeCone([T.NonnegativeConeT(3)]), psd=True)
    assert not cone_set_steps_on_device(CompositeCone([T.PowerConeT(0.3)]), psd=True)
    assert cone_set_steps_on_device(CompositeCone([T.PowerConeT(0.3)]), nonsymmetric=True, psd=True)
    assert hipkkt.PSD_STEP_MAX_DIM == 64


def test_header_binding_libraries_and_julia_glue_agree_on_the_new_entry_points():
    protos = c_prototypes()
    glue = {c[0] for c in jl_ccalls(JL_FILES[1])}          # julia/ext/hipkkt_lib.jl
    hdr = open(os.path.join(ROOT, "include", "hipkkt.h")).read()
    assert re.search(r"#define\s+HIPKKT_PSD_STEP_MAX_DIM\s+64\b", hdr)
    assert re.search(r"#define\s+HIPKKT_ABI_VERSION\s+5\b", hdr)
    added = hdr[hdr.index("Added within 5"):hdr.index("#define HIPKKT_ABI_VERSION")]
    pkg = os.path.dirname(hipkkt.__file__)
    libs = [C.CDLL(os.path.join(pkg, name)) for name in ("libclarabel_hipkkt.so", "libclarabel_hipkkt_testing.so")]
    for s in NEW:
        assert s in protos, f"{s} is not declared in include/hipkkt.h"
        assert s in added and s in hipkkt.SYMBOLS and s in glue
        for L in libs:
            assert hasattr(L, s), s
    assert "HIPKKT_PSD_STEP_MAX_DIM" in added
    assert protos["hipkkt_psd_set_factors"] == protos["hipkkt_psd_set_factors_dev"]
    L = hipkkt.lib()
    vp, i32 = C.c_void_p, C.c_int32
    assert list(L.hipkkt_step_enable_psd.argtypes) == [vp, i32]
    assert list(L.hipkkt_psd_set_factors_dev.argtypes) == [vp, vp, vp]
    assert len(L.hipkkt_psd_set_factors.argtypes) == 3 and L.hipkkt_psd_set_factors.argtypes[0] is vp
    assert hasattr(hipkkt.Handle, "step_enable_psd") and hasattr(hipkkt.Handle, "psd_set_factors")
    assert hipkkt.ABI_VERSION == 5 and L.hipkkt_abi_version() == 5
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW + ("device_step_psd", "hip_step_enable_psd!", "hip_psd_set_factors!", "hip_psd_set_factors_dev!"):
        assert s in text, s
