"""The device-resident interior-point step for PSD triangle cones next to Exponential / Power / Generalized Power cones
(Settings.device_step_mixed, include/hipkkt.h hipkkt_step_enable_mixed), checked without a GPU: the setting and its prerequisites, the
qualification rule, the new symbol in the header, in both libraries, in the ctypes mirror, in the Julia glue and in INTEGRATION.md, and the
problem generator the end-to-end tests use."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt
from clarabel_jl_amd.kktsolver import cone_set_steps_on_device
from clarabel_jl_amd.problems import mixed_psd_nonsym, nonsymmetric_mix
from julia_standin.cones import CompositeCone
from tests import fixtures as fx
from tests.test_julia_glue import JL_FILES, c_prototypes, jl_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "hipkkt_step_enable_mixed"
FLAGS = dict(device_scaling=True, device_reduced=True, device_residuals=True)
GENPOW = ((0.6, 0.4), 1)


def test_the_setting_is_off_by_default_and_names_what_it_needs(oracle_factory):
    assert cl.Settings().device_step_mixed is False
    with pytest.raises(ValueError, match="device_step_mixed needs device_step_nonsymmetric"):
        cl.Solver(*fx.basic_sdp(), cl.Settings(device_step=True, device_step_psd=True, device_step_mixed=True, **FLAGS),
                  kktsolver_factory=oracle_factory)
    with pytest.raises(ValueError, match="device_step_mixed needs device_step_psd"):
        cl.Solver(*fx.basic_sdp(), cl.Settings(device_step=True, device_step_nonsymmetric=True, device_step_mixed=True, **FLAGS),
                  kktsolver_factory=oracle_factory)
    # the prerequisites' own prerequisite is named first, as before
    with pytest.raises(ValueError, match="device_step_nonsymmetric needs device_step"):
        cl.Solver(*fx.basic_sdp(), cl.Settings(device_step_nonsymmetric=True, device_step_psd=True, device_step_mixed=True, **FLAGS),
                  kktsolver_factory=oracle_factory)
    # a plugin without the step calls keeps the host loop, as with the other device_* flags
    S = cl.Solver(*mixed_psd_nonsym(n=12, psd_sides=[3, 2], nexp=3, npow=0, ngenpow=0, nn=3, nzero=2, socdim=4, seed=5),
                  cl.Settings(device_step=True, device_step_nonsymmetric=True, device_step_psd=True, device_step_mixed=True, **FLAGS),
                  kktsolver_factory=oracle_factory)
    assert not S._device_step and not S._device_step_psd


def test_psd_members_qualify_next_to_nonsymmetric_ones_only_with_all_three_flags():
    T = cl
    on = dict(nonsymmetric=True, psd=True, mixed=True)
    yes = [[T.PSDTriangleConeT(3), T.ExponentialConeT()], [T.PowerConeT(0.2), T.PSDTriangleConeT(2)],
           [T.NonnegativeConeT(3), T.PSDTriangleConeT(64), T.ExponentialConeT(), T.SecondOrderConeT(4), T.ZeroConeT(2)]]
    for specs in yes:
        cones = CompositeCone(specs)
        assert cone_set_steps_on_device(cones, **on), specs
        assert cone_set_steps_on_device(cones, genpower=True, **on), specs
        assert cone_set_steps_on_device(cones, psd_large=True, **on), specs
        # each flag is needed; mixed alone widens nothing
        assert not cone_set_steps_on_device(cones, mixed=True), specs
        assert not cone_set_steps_on_device(cones, nonsymmetric=True, mixed=True), specs
        assert not cone_set_steps_on_device(cones, psd=True, mixed=True), specs
        assert not cone_set_steps_on_device(cones, nonsymmetric=True, psd=True), specs
        assert not cone_set_steps_on_device(cones, nonsymmetric=True, genpower=True, psd=True, psd_large=True), specs
    gp = CompositeCone([T.GenPowerConeT(*GENPOW), T.PSDTriangleConeT(2)])
    assert cone_set_steps_on_device(gp, genpower=True, **on)
    assert not cone_set_steps_on_device(gp, **on)                                       # a GenPow member without genpower
    assert not cone_set_steps_on_device(gp, genpower=True, psd=True, mixed=True)        # genpower counts with nonsymmetric only
    big = CompositeCone([T.PSDTriangleConeT(65), T.ExponentialConeT()])
    assert not cone_set_steps_on_device(big, **on)
    assert not cone_set_steps_on_device(big, psd_large=True, **on)                      # the barrier keeps its matrix in LDS: 64 is the limit
    assert not cone_set_steps_on_device(CompositeCone([]), **on)


def test_every_answer_without_mixed_is_what_it_was():
    T = cl
    sets = {
        "sym": [T.NonnegativeConeT(3), T.SecondOrderConeT(4), T.ZeroConeT(2)],
        "exp": [T.NonnegativeConeT(3), T.ExponentialConeT(), T.PowerConeT(0.3)],
        "gp": [T.GenPowerConeT(*GENPOW), T.ExponentialConeT()],
        "psd": [T.PSDTriangleConeT(3), T.NonnegativeConeT(2)],
        "psd65": [T.PSDTriangleConeT(65)],
        "psd129": [T.PSDTriangleConeT(129)],
        "mixed": [T.PSDTriangleConeT(3), T.ExponentialConeT()],
    }
    flags = [dict(), dict(nonsymmetric=True), dict(nonsymmetric=True, genpower=True), dict(genpower=True), dict(psd=True),
             dict(psd=True, psd_large=True), dict(psd_large=True), dict(nonsymmetric=True, genpower=True, psd=True, psd_large=True)]
    # the rule as it stood: kinds 0..2 always; 4, 5 with nonsymmetric; 6 with nonsymmetric and genpower; 3 with psd in a set without
    # kinds 4..6, up to side 64, or 128 with psd_large
    def before(name, nonsymmetric=False, genpower=False, psd=False, psd_large=False):
        if name == "sym":
            return True
        if name == "exp":
            return nonsymmetric
        if name == "gp":
            return nonsymmetric and genpower
        if name == "psd":
            return psd
        if name == "psd65":
            return psd and psd_large
        return False
    for name, specs in sets.items():
        cones = CompositeCone(specs)
        for f in flags:
            assert cone_set_steps_on_device(cones, **f) == before(name, **f), (name, f)
            assert cone_set_steps_on_device(cones, mixed=False, **f) == before(name, **f), (name, f)
            if name != "mixed":      # mixed=True changes the answer for no set without both families
                assert cone_set_steps_on_device(cones, mixed=True, **f) == before(name, **f), (name, f)


def test_header_binding_libraries_julia_glue_and_documents_agree_on_the_new_entry_point():
    protos = c_prototypes()
    glue = {c[0] for c in jl_ccalls(JL_FILES[1])}          # julia/ext/hipkkt_lib.jl
    hdr = open(os.path.join(ROOT, "include", "hipkkt.h")).read()
    assert re.search(r"#define\s+HIPKKT_ABI_VERSION\s+5\b", hdr)
    added = hdr[hdr.index("Added within 5"):hdr.index("#define HIPKKT_ABI_VERSION")]
    assert NEW in protos, f"{NEW} is not declared in include/hipkkt.h"
    assert NEW in added
    assert protos[NEW] == protos["hipkkt_step_enable_cone3"]
    assert NEW in hipkkt.SYMBOLS and NEW in glue
    pkg = os.path.dirname(hipkkt.__file__)
    for name in ("libclarabel_hipkkt.so", "libclarabel_hipkkt_testing.so"):
        assert hasattr(C.CDLL(os.path.join(pkg, name)), NEW), name
    L = hipkkt.lib()
    assert list(L.hipkkt_step_enable_mixed.argtypes) == list(L.hipkkt_step_enable_cone3.argtypes) == \
        [C.c_void_p, C.c_int32, C.c_double, C.c_double]
    assert hasattr(hipkkt.Handle, "step_enable_mixed")
    assert hipkkt.ABI_VERSION == 5 and L.hipkkt_abi_version() == 5
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in (NEW, "device_step_mixed", "hip_step_enable_mixed!"):
        assert s in text, s
    assert "device_step_mixed" in open(os.path.join(ROOT, "README.md")).read()


def test_the_generator_orders_the_cones_and_leaves_nonsymmetric_mix_alone():
    kw = dict(n=20, psd_sides=[3, 8, 2], nexp=3, npow=3, ngenpow=3, nn=4, nzero=2, socdim=4, seed=6)
    P, q, A, b, cones = mixed_psd_nonsym(**kw)
    names = [type(c).__name__ for c in cones]
    assert names == ["ZeroConeT", "NonnegativeConeT", "PSDTriangleConeT", "PSDTriangleConeT"] + ["ExponentialConeT"] * 3 + \
        ["PowerConeT"] * 3 + ["GenPowerConeT"] * 3 + ["SecondOrderConeT", "PSDTriangleConeT"]
    assert [c.dim for c in cones if type(c).__name__ == "PSDTriangleConeT"] == [3, 8, 2]
    K = CompositeCone(cones)
    assert A.shape == (K.numel, 20) and b.shape == (K.numel,) and q.shape == (20,) and P.shape == (20, 20)
    P2, q2, A2, b2, _ = mixed_psd_nonsym(**kw)
    assert np.array_equal(b, b2) and np.array_equal(q, q2) and (A != A2).nnz == 0 and (P != P2).nnz == 0
    # without PSD draws between them the other families' slacks are those of nonsymmetric_mix: the same recipe
    ref = nonsymmetric_mix(n=20, nexp=3, npow=3, ngenpow=3, nn=4, nzero=2, socdim=4, seed=6)
    assert [type(c).__name__ for c in ref[4]] == [n for n in names if n != "PSDTriangleConeT"]
