"""The device-resident interior-point step for PSD triangle cones of side 65 .. 128 (Settings.device_step_psd_large, include/hipkkt.h
hipkkt_step_enable_psd_large), checked without a GPU: the setting, the qualification rule, the new symbol in the header, in both
libraries, in the ctypes mirror and in the Julia glue, and the testing switch."""
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
NEW = "hipkkt_step_enable_psd_large"
FLAGS = dict(device_scaling=True, device_reduced=True, device_residuals=True)


def test_the_setting_is_off_by_default_and_needs_device_step_psd(oracle_factory):
    assert cl.Settings().device_step_psd_large is False
    with pytest.raises(ValueError, match="device_step_psd_large needs device_step_psd"):
        cl.Solver(*fx.basic_sdp(), cl.Settings(device_step=True, device_step_psd_large=True, **FLAGS), kktsolver_factory=oracle_factory)
    # a plugin without the step calls keeps the host loop, as with the other device_* flags
    S = cl.Solver(*fx.basic_sdp(), cl.Settings(device_step=True, device_step_psd=True, device_step_psd_large=True, **FLAGS),
                  kktsolver_factory=oracle_factory)
    assert not S._device_step and not S._device_step_psd


def test_psd_sets_up_to_side_128_qualify_only_with_both_flags():
    T = cl
    yes = [[T.PSDTriangleConeT(65)], [T.PSDTriangleConeT(128)], [T.PSDTriangleConeT(3), T.PSDTriangleConeT(65)],
           [T.NonnegativeConeT(3), T.PSDTriangleConeT(96), T.SecondOrderConeT(4), T.ZeroConeT(2)]]
    no = [[T.PSDTriangleConeT(129)], [T.PSDTriangleConeT(65), T.PowerConeT(0.3)], [T.PSDTriangleConeT(65), T.ExponentialConeT()], []]
    for specs in yes:
        cones = CompositeCone(specs)
        assert cone_set_steps_on_device(cones, psd=True, psd_large=True), specs
        assert not cone_set_steps_on_device(cones, psd=True), specs                  # psd alone keeps refusing 65
        assert not cone_set_steps_on_device(cones, psd_large=True), specs            # psd_large alone widens nothing
        assert not cone_set_steps_on_device(cones), specs
    for specs in no:
        cones = CompositeCone(specs)
        assert not cone_set_steps_on_device(cones, psd=True, psd_large=True), specs
        assert not cone_set_steps_on_device(cones, nonsymmetric=True, genpower=True, psd=True, psd_large=True), specs
    # what qualified before still does, and psd_large alone admits no PSD cone at all
    assert cone_set_steps_on_device(CompositeCone([T.PSDTriangleConeT(64)]), psd=True, psd_large=True)
    assert not cone_set_steps_on_device(CompositeCone([T.PSDTriangleConeT(3)]), psd_large=True)
    assert cone_set_steps_on_device(CompositeCone([T.NonnegativeConeT(3)]), psd_large=True)
    assert hipkkt.PSD_STEP_LARGE_MAX_DIM == 128 and hipkkt.PSD_STEP_MAX_DIM == 64


def test_header_binding_libraries_and_julia_glue_agree_on_the_new_entry_point():
    protos = c_prototypes()
    glue = {c[0] for c in jl_ccalls(JL_FILES[1])}          # julia/ext/hipkkt_lib.jl
    hdr = open(os.path.join(ROOT, "include", "hipkkt.h")).read()
    assert re.search(r"#define\s+HIPKKT_PSD_STEP_LARGE_MAX_DIM\s+128\b", hdr)
    assert re.search(r"#define\s+HIPKKT_PSD_STEP_MAX_DIM\s+64\b", hdr)
    assert re.search(r"#define\s+HIPKKT_ABI_VERSION\s+5\b", hdr)
    added = hdr[hdr.index("Added within 5"):hdr.index("#define HIPKKT_ABI_VERSION")]
    assert NEW in protos, f"{NEW} is not declared in include/hipkkt.h"
    assert NEW in added and "HIPKKT_PSD_STEP_LARGE_MAX_DIM" in added
    assert NEW in hipkkt.SYMBOLS and NEW in glue
    pkg = os.path.dirname(hipkkt.__file__)
    for name in ("libclarabel_hipkkt.so", "libclarabel_hipkkt_testing.so"):
        assert hasattr(C.CDLL(os.path.join(pkg, name)), NEW), name
    assert protos[NEW] == protos["hipkkt_step_enable_psd"]
    L = hipkkt.lib()
    assert list(L.hipkkt_step_enable_psd_large.argtypes) == [C.c_void_p, C.c_int32]
    assert hasattr(hipkkt.Handle, "step_enable_psd_large")
    assert "PSD_LARGE_MIN" in hipkkt.DEBUG_KEYS
    assert hipkkt.ABI_VERSION == 5 and L.hipkkt_abi_version() == 5
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in (NEW, "device_step_psd_large", "hip_step_enable_psd_large!"):
        assert s in text, s
    assert "PSD_LARGE_MIN" in open(os.path.join(ROOT, "README.md")).read()


def test_the_testing_switch_takes_sides_up_to_128_and_the_product_refuses_it():
    pkg = os.path.dirname(hipkkt.__file__)
    prod, testing = (C.CDLL(os.path.join(pkg, name)) for name in ("libclarabel_hipkkt.so", "libclarabel_hipkkt_testing.so"))
    for L in (prod, testing):
        L.hipkkt_debug_set.argtypes = [C.c_char_p, C.c_char_p]
        L.hipkkt_debug_set.restype = C.c_int32
    assert prod.hipkkt_debug_set(b"PSD_LARGE_MIN", b"1") != 0
    for value in (b"0", b"1", b"64", b"65", b"128", None):
        assert testing.hipkkt_debug_set(b"PSD_LARGE_MIN", value) == 0, value
    for value in (b"129", b"-1", b"1.5", b"x"):
        assert testing.hipkkt_debug_set(b"PSD_LARGE_MIN", value) != 0, value
    assert testing.hipkkt_debug_set(b"PSD_LARGE_MIN", None) == 0
