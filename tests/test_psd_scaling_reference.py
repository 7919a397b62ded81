"""The device-side Nesterov-Todd scaling of PSD triangle cones (csrc/scaling_psd.hip, Settings.device_scaling_psd,
include/hipkkt.h hipkkt_psd_scaling_enable / hipkkt_psd_get_factors), checked without a GPU:

  * the numpy emulation of the kernel's exact algorithm (tests/psd_scaling_reference.py `emulate`) on the whole test family of
    tests/test_gpu_psd_scaling.py, its five 50-digit residuals held to the project's PSD gate against the stand-in's LAPACK factors;
  * the sweep count it needs against kMaxSweeps of the source (at least twice as many are allowed);
  * the setting, and the new symbols in the header, both libraries, the ctypes mirror and the Julia glue."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt
from julia_standin.cones import PSDTriangleCone
from tests import fixtures as fx
from tests import psd_scaling_reference as sr
from tests.test_julia_glue import JL_FILES, c_prototypes, jl_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hipkkt_psd_scaling_enable", "hipkkt_psd_get_factors")
FLAGS = dict(device_scaling=True, device_reduced=True, device_residuals=True)
_sweeps = {}


@pytest.mark.parametrize("group", sr.GROUPS)
@pytest.mark.parametrize("n", sr.SIDES)
def test_the_emulated_kernel_meets_the_gate_on_the_whole_family(n, group):
    worst, most = 0.0, 0
    for name, s, z, ref, host in sr.cases(n, group):
        out = sr.emulate(n, s, z)
        assert out is not None, (n, name)
        R, Rinv, lam, sweeps = out
        most = max(most, sweeps)
        assert np.all(lam > 0) and np.all(np.diff(lam) <= 0), (n, name)
        worst = max(worst, sr.gate(f"emulation {name}", n, ref.residuals(R, Rinv, lam), host))
    _sweeps[n] = max(most, _sweeps.get(n, 0))
    print(f"[psd scaling] emulation n={n} {group}: at most {most} sweeps, worst device / host ratio {worst:.2f}")
    assert 2 * most <= sr.max_sweeps_in_source(), (n, most)


def test_the_sweep_bound_is_at_least_twice_what_the_family_needs():
    """(the per-side assertion above, over the sides that ran in this process; alone, this test runs the largest side itself)"""
    if not _sweeps:
        n = sr.SIDES[-1]
        _sweeps[n] = max(sr.emulate(n, s, z)[3] for _, s, z in sr.points(n))
    most = max(_sweeps.values())
    print(f"[psd scaling] the emulation needs at most {most} sweeps (sides {sorted(_sweeps)}); kMaxSweeps = {sr.max_sweeps_in_source()}")
    assert sr.max_sweeps_in_source() >= 2 * most


def test_the_emulation_fails_the_cones_the_reference_fails():
    n = 5
    K = PSDTriangleCone(n)
    rng = np.random.default_rng(3)
    s, z, _ = sr.pr.random_sz(K, rng)
    assert sr.emulate(n, s, z) is not None
    assert sr.emulate(n, np.zeros_like(s), z) is None                          # S = 0
    Zi = np.diag([1.0, 2.0, -0.5, 1.0, 3.0])
    assert sr.emulate(n, s, K.mat_to_svec(Zi)) is None                         # Z indefinite
    bad = s.copy()
    bad[7] = np.nan
    assert sr.emulate(n, bad, z) is None                                       # a NaN reaches a pivot
    assert not K.update_scaling(np.zeros_like(s), z, 1.0) and not K.update_scaling(s, K.mat_to_svec(Zi), 1.0)
    assert sr.emulate(n, s, z, max_sweeps=1) is None                           # the sweep bound


def test_the_sort_is_descending_with_ties_broken_by_index():
    n = 6
    K = PSDTriangleCone(n)
    R, Rinv, lam, _ = sr.emulate(n, K.mat_to_svec(np.eye(n)), K.mat_to_svec(4.0 * np.eye(n)))
    assert np.array_equal(lam, np.full(n, 2.0))
    assert np.array_equal(R, np.eye(n) * (1.0 / math.sqrt(2.0)))               # no rotation: V = I, ties keep their index order
    assert np.allclose(Rinv @ R, np.eye(n), rtol=0, atol=4 * sr.EPS)
    D = np.diag([1.0, 9.0, 4.0, 9.0, 16.0, 1.0])
    R, Rinv, lam, _ = sr.emulate(n, K.mat_to_svec(D), K.mat_to_svec(np.eye(n)))
    assert np.allclose(lam, np.array([4.0, 3.0, 3.0, 2.0, 1.0, 1.0]), rtol=2 * sr.EPS, atol=0) and lam[1] == lam[2] and lam[4] == lam[5]
    # column k of R belongs to lambda_k: R' Z R = diag(lambda) pins the order, the index rule the columns of equal lambda
    cols = [int(np.argmax(np.abs(R[:, k]))) for k in range(n)]
    assert cols == [4, 1, 3, 2, 0, 5]


def test_the_setting_is_off_by_default_and_needs_device_step_psd(oracle_factory):
    assert cl.Settings().device_scaling_psd is False
    with pytest.raises(ValueError, match="device_scaling_psd"):
        cl.Solver(*fx.basic_sdp(), cl.Settings(device_step=True, device_scaling_psd=True, **FLAGS), kktsolver_factory=oracle_factory)
    # a plugin without the step calls keeps the host loop, as with the other device_* flags
    S = cl.Solver(*fx.basic_sdp(), cl.Settings(device_step=True, device_step_psd=True, device_scaling_psd=True, **FLAGS),
                  kktsolver_factory=oracle_factory)
    assert not S._device_step and not S._device_step_psd and not S._device_scaling_psd


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
    vp, i32 = C.c_void_p, C.c_int32
    assert list(L.hipkkt_psd_scaling_enable.argtypes) == [vp, i32]
    assert list(L.hipkkt_psd_get_factors.argtypes) == [vp, vp, vp, vp]
    assert hasattr(hipkkt.Handle, "psd_scaling_enable") and hasattr(hipkkt.Handle, "psd_get_factors")
    assert hipkkt.ABI_VERSION == 5 and L.hipkkt_abi_version() == 5
    # the header's sweep bound is the source's
    assert f"at most {sr.max_sweeps_in_source()} sweeps" in hdr
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW + ("device_scaling_psd", "hip_psd_scaling_enable!", "hip_psd_get_factors!"):
        assert s in text, s
