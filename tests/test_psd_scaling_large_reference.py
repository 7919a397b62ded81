"""The device-side Nesterov-Todd scaling and default start of PSD triangle cones of side 65 .. 128 (csrc/scaling_psd_large.hip,
csrc/start.hip; include/hipkkt.h hipkkt_psd_scaling_enable_large / hipkkt_step_default_start_enable_psd_large;
Settings.device_scaling_psd_large / device_default_start_psd_large), checked without a GPU:

  * scaling_psd_large.hip executes the arithmetic of scaling_psd.hip, which tests/psd_scaling_reference.py `emulate` repeats in numpy:
    the emulation must meet the project's PSD gate (50-digit residuals, max(8 x the host's error, 2 n) eps x scale) at the sides the
    new kernels serve -- 65 and 66 on the whole family, 128 on five points;
  * kMaxSweeps of the NEW source against the sweeps the emulation takes on those points (at least twice as many are allowed);
  * the two settings, and the two symbols in the header, both libraries, the ctypes mirror and the Julia glue."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt
from tests import fixtures as fx
from tests import psd_scaling_reference as sr
from tests.test_julia_glue import JL_FILES, c_prototypes, jl_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hipkkt_psd_scaling_enable_large", "hipkkt_step_default_start_enable_psd_large")
FLAGS = dict(device_scaling=True, device_reduced=True, device_residuals=True)
POINTS_128 = ("early_0", "late_0", "S_equals_Z", "two_fold", "n_fold")
_sweeps = {}


def max_sweeps_in_new_source():
    src = open(os.path.join(ROOT, "clarabel.jl_amd", "csrc", "scaling_psd_large.hip")).read()
    return int(re.search(r"constexpr\s+int\s+kMaxSweeps\s*=\s*(\d+)\s*;", src).group(1))


def _emulation_meets_the_gate(n, name, s, z, ref, host):
    out = sr.emulate(n, s, z, max_sweeps=max_sweeps_in_new_source())
    assert out is not None, (n, name)
    R, Rinv, lam, sweeps = out
    assert np.all(lam > 0) and np.all(np.diff(lam) <= 0), (n, name)
    _sweeps[n] = max(sweeps, _sweeps.get(n, 0))
    return sr.gate(f"emulation {name}", n, ref.residuals(R, Rinv, lam), host), sweeps


@pytest.mark.parametrize("group", sr.GROUPS)
@pytest.mark.parametrize("n", [65, 66])
def test_the_emulated_kernel_meets_the_gate_at_the_smallest_large_sides(n, group):
    worst, most = 0.0, 0
    for name, s, z, ref, host in sr.cases(n, group):
        w, sweeps = _emulation_meets_the_gate(n, name, s, z, ref, host)
        worst, most = max(worst, w), max(most, sweeps)
    print(f"[psd scaling large] emulation n={n} {group}: at most {most} sweeps, worst device / host ratio {worst:.2f}")
    assert 2 * most <= max_sweeps_in_new_source(), (n, most)


@pytest.mark.parametrize("name", POINTS_128)
def test_the_emulated_kernel_meets_the_gate_at_side_128(name):
    n = 128
    (s, z), = [(s, z) for nm, s, z in sr.points(n) if nm == name]
    ref = sr.Reference(n, s, z)
    w, sweeps = _emulation_meets_the_gate(n, name, s, z, ref, ref.residuals(*sr.host_factors(n, s, z)))
    print(f"[psd scaling large] emulation n={n} {name}: {sweeps} sweeps, device / host ratio {w:.2f}")
    assert 2 * sweeps <= max_sweeps_in_new_source(), (name, sweeps)


def test_the_sweep_bound_of_the_new_source_is_the_small_kernels_and_twice_what_the_points_need():
    """(over the sides that ran in this process; alone, this test runs one point of side 65 itself)"""
    assert max_sweeps_in_new_source() == sr.max_sweeps_in_source()
    if not _sweeps:
        name, s, z = sr.points(65)[0]
        _sweeps[65] = sr.emulate(65, s, z)[3]
    most = max(_sweeps.values())
    print(f"[psd scaling large] the emulation needs at most {most} sweeps (sides {sorted(_sweeps)}); kMaxSweeps = {max_sweeps_in_new_source()}")
    assert max_sweeps_in_new_source() >= 2 * most


def test_the_settings_are_off_by_default_and_need_their_base_flags(oracle_factory):
    st = cl.Settings()
    assert st.device_scaling_psd_large is False and st.device_default_start_psd_large is False
    base = dict(device_step=True, device_step_psd=True, **FLAGS)
    for flags, what in ((dict(base, device_scaling_psd_large=True), "device_scaling_psd_large"),
                        (dict(base, device_scaling_psd=True, device_scaling_psd_large=True), "device_scaling_psd_large"),
                        (dict(base, device_step_psd_large=True, device_scaling_psd_large=True), "device_scaling_psd_large"),
                        (dict(base, device_default_start_psd_large=True), "device_default_start_psd_large"),
                        (dict(base, device_default_start=True, device_default_start_psd_large=True), "device_default_start_psd_large"),
                        (dict(base, device_step_psd_large=True, device_default_start_psd_large=True), "device_default_start_psd_large")):
        with pytest.raises(ValueError, match=what + " needs"):
            cl.Solver(*fx.basic_sdp(), cl.Settings(**flags), kktsolver_factory=oracle_factory)
    # with their base flags a plugin without the step calls keeps the host loop, as with the other device_* flags
    S = cl.Solver(*fx.basic_sdp(), cl.Settings(**dict(base, device_step_psd_large=True, device_scaling_psd=True, device_default_start=True,
                                                      device_scaling_psd_large=True, device_default_start_psd_large=True)),
                  kktsolver_factory=oracle_factory)
    assert not S._device_step and not S._device_scaling_psd and not S._device_default_start


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
        assert protos[s] == protos["hipkkt_psd_scaling_enable"]
        assert s in added and s in hipkkt.SYMBOLS and s in glue
        for L in libs:                                      # the production library exports them too
            assert hasattr(L, s), s
    L = hipkkt.lib()
    vp, i32 = C.c_void_p, C.c_int32
    assert list(L.hipkkt_psd_scaling_enable_large.argtypes) == [vp, i32]
    assert list(L.hipkkt_step_default_start_enable_psd_large.argtypes) == [vp, i32]
    assert hasattr(hipkkt.Handle, "psd_scaling_enable_large") and hasattr(hipkkt.Handle, "step_default_start_enable_psd_large")
    assert hipkkt.ABI_VERSION == 5 and L.hipkkt_abi_version() == 5
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW + ("device_scaling_psd_large", "device_default_start_psd_large", "hip_psd_scaling_enable_large!",
                    "hip_step_default_start_enable_psd_large!"):
        assert s in text, s
    assert "scaling_psd_large.hip" in open(os.path.join(ROOT, "README.md")).read()


@pytest.mark.parametrize("n", [3, 8, 17])
def test_the_sliced_exact_k_gate_is_the_unsliced_one(n):
    """tests/psd_skron_sliced.py against psd_scaling_reference.skron_error on the host's float64 block and on a perturbed one, with
    slices of a few columns and with one slice"""
    from julia_standin.cones import PSDTriangleCone
    from tests import psd_skron_sliced as sk

    name, s, z = sr.points(n)[0]
    K = PSDTriangleCone(n)
    assert K.update_scaling(s, z, 1.0)
    hb = np.zeros(K.numel * (K.numel + 1) // 2)
    K.get_Hs(hb)
    bad = hb.copy()
    bad[len(bad) // 2] *= 1.0 + 64 * sr.EPS
    for block in (hb, bad):
        want = sr.skron_error(K.R, block)
        assert sk.skron_error(K.R, block, limit=40) == want and sk.skron_error(K.R, block) == want, n
    assert sr.skron_error(K.R, bad) > sr.skron_error(K.R, hb)
    assert sk._column_slices(5, 4) == [(0, 2), (2, 3), (3, 4), (4, 5)] and sk._column_slices(3, 100) == [(0, 3)]
