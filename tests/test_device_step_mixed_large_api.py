"""The device-resident interior-point step for PSD triangle cones of side 65 .. 128 next to Exponential / Power / Generalized Power cones
(Settings.device_step_mixed_large, include/hipkkt.h hipkkt_step_enable_mixed_large), checked without a GPU: the setting and its
prerequisites, the qualification rule, and the new symbol in the header, in both libraries, in the ctypes mirror, in the Julia glue and
in the documents."""
import ctypes as C
import os
import re

import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt
from clarabel_jl_amd.kktsolver import cone_set_steps_on_device
from clarabel_jl_amd.problems import mixed_psd_nonsym
from julia_standin.cones import CompositeCone
from tests import fixtures as fx
from tests.test_julia_glue import JL_FILES, c_prototypes, jl_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "hipkkt_step_enable_mixed_large"
FLAGS = dict(device_scaling=True, device_reduced=True, device_residuals=True)
MIXED = dict(device_step=True, device_step_nonsymmetric=True, device_step_psd=True, device_step_mixed=True, **FLAGS)
GENPOW = ((0.6, 0.4), 1)


def test_the_setting_is_off_by_default_and_names_what_it_needs(oracle_factory):
    assert cl.Settings().device_step_mixed_large is False
    with pytest.raises(ValueError, match="device_step_mixed_large needs device_step_mixed"):
        cl.Solver(*fx.basic_sdp(), cl.Settings(device_step=True, device_step_nonsymmetric=True, device_step_psd=True,
                                               device_step_psd_large=True, device_step_mixed_large=True, **FLAGS),
                  kktsolver_factory=oracle_factory)
    with pytest.raises(ValueError, match="device_step_mixed_large needs device_step_psd_large"):
        cl.Solver(*fx.basic_sdp(), cl.Settings(device_step_mixed_large=True, **MIXED), kktsolver_factory=oracle_factory)
    # an earlier prerequisite is named first, as before
    with pytest.raises(ValueError, match="device_step_mixed needs device_step_psd"):
        cl.Solver(*fx.basic_sdp(), cl.Settings(device_step=True, device_step_nonsymmetric=True, device_step_mixed=True,
                                               device_step_mixed_large=True, **FLAGS), kktsolver_factory=oracle_factory)
    with pytest.raises(ValueError, match="device_step_psd_large needs device_step_psd"):
        cl.Solver(*fx.basic_sdp(), cl.Settings(device_step=True, device_step_psd_large=True, device_step_mixed_large=True, **FLAGS),
                  kktsolver_factory=oracle_factory)


def test_a_plugin_without_the_step_calls_keeps_the_host_loop(oracle_factory):
    S = cl.Solver(*mixed_psd_nonsym(n=12, psd_sides=[65, 2], nexp=3, npow=0, ngenpow=0, nn=3, nzero=2, socdim=4, seed=5),
                  cl.Settings(device_step_psd_large=True, device_step_mixed_large=True, **MIXED), kktsolver_factory=oracle_factory)
    assert not S._device_step and not S._device_step_psd


def test_a_side_above_64_qualifies_next_to_nonsymmetric_members_only_with_mixed_large():
    T = cl
    on = dict(nonsymmetric=True, psd=True, mixed=True)
    big = CompositeCone([T.PSDTriangleConeT(65), T.ExponentialConeT()])
    assert not cone_set_steps_on_device(big, **on)
    assert not cone_set_steps_on_device(big, psd_large=True, **on)                      # psd_large alone keeps widening nothing here
    assert cone_set_steps_on_device(big, mixed_large=True, **on)
    assert cone_set_steps_on_device(big, mixed_large=True, psd_large=True, **on)
    sets = [[T.NonnegativeConeT(3), T.PSDTriangleConeT(128), T.PowerConeT(0.3), T.SecondOrderConeT(4), T.PSDTriangleConeT(2), T.ZeroConeT(2)],
            [T.PSDTriangleConeT(96), T.ExponentialConeT(), T.PSDTriangleConeT(64)]]
    for specs in sets:
        cones = CompositeCone(specs)
        assert cone_set_steps_on_device(cones, mixed_large=True, **on), specs
        assert not cone_set_steps_on_device(cones, **on), specs
        # each of the three flags below it is needed; mixed_large alone widens nothing
        assert not cone_set_steps_on_device(cones, mixed_large=True), specs
        assert not cone_set_steps_on_device(cones, mixed_large=True, nonsymmetric=True, psd=True), specs
        assert not cone_set_steps_on_device(cones, mixed_large=True, nonsymmetric=True, mixed=True), specs
        assert not cone_set_steps_on_device(cones, mixed_large=True, psd=True, psd_large=True, mixed=True), specs
    gp = CompositeCone([T.GenPowerConeT(*GENPOW), T.PSDTriangleConeT(65)])
    assert cone_set_steps_on_device(gp, genpower=True, mixed_large=True, **on)
    assert not cone_set_steps_on_device(gp, mixed_large=True, **on)                     # a GenPow member without genpower
    too_big = CompositeCone([T.PSDTriangleConeT(129), T.ExponentialConeT()])
    assert not cone_set_steps_on_device(too_big, mixed_large=True, psd_large=True, **on)
    # a set without a non-symmetric member does not look at it
    sym65 = CompositeCone([T.PSDTriangleConeT(65), T.NonnegativeConeT(2)])
    assert not cone_set_steps_on_device(sym65, psd=True, mixed_large=True)
    assert not cone_set_steps_on_device(sym65, mixed_large=True, **on)
    assert cone_set_steps_on_device(sym65, psd=True, psd_large=True, mixed_large=True)
    small = CompositeCone([T.PSDTriangleConeT(3), T.ExponentialConeT()])
    for f in (dict(), dict(nonsymmetric=True), dict(psd=True), on, dict(psd_large=True, **on)):
        assert cone_set_steps_on_device(small, mixed_large=True, **f) == cone_set_steps_on_device(small, **f), f


def test_header_binding_libraries_julia_glue_and_documents_agree_on_the_new_entry_point():
    protos = c_prototypes()
    glue = {c[0] for c in jl_ccalls(JL_FILES[1])}          # julia/ext/hipkkt_lib.jl
    hdr = open(os.path.join(ROOT, "include", "hipkkt.h")).read()
    assert re.search(r"#define\s+HIPKKT_ABI_VERSION\s+5\b", hdr)
    added = hdr[hdr.index("Added within 5"):hdr.index("#define HIPKKT_ABI_VERSION")]
    assert NEW in protos, f"{NEW} is not declared in include/hipkkt.h"
    assert NEW in added
    assert protos[NEW] == protos["hipkkt_step_enable_mixed"] == protos["hipkkt_step_enable_cone3"]
    assert "coneops_psdtrianglecone.jl:256-290" in hdr[hdr.index("hipkkt_step_enable_mixed_large accepts"):]
    assert NEW in hipkkt.SYMBOLS and NEW in glue
    assert "hip_step_enable_mixed_large!" in open(JL_FILES[1]).read()
    pkg = os.path.dirname(hipkkt.__file__)
    for name in ("libclarabel_hipkkt.so", "libclarabel_hipkkt_testing.so"):
        assert hasattr(C.CDLL(os.path.join(pkg, name)), NEW), name
    L = hipkkt.lib()
    assert list(L.hipkkt_step_enable_mixed_large.argtypes) == list(L.hipkkt_step_enable_mixed.argtypes) == \
        [C.c_void_p, C.c_int32, C.c_double, C.c_double]
    assert hasattr(hipkkt.Handle, "step_enable_mixed_large")
    assert hipkkt.ABI_VERSION == 5 and L.hipkkt_abi_version() == 5
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for s in (NEW, "device_step_mixed_large"):
            assert s in text, (doc, s)
    assert "hip_step_enable_mixed_large!" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "k_bar_psd_large" in open(os.path.join(ROOT, "DESIGN.md")).read()
