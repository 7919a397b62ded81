"""The device scaling of Zero / Nonnegative / second-order cones (k_scaling_diag, k_scaling_soc, k_soc_batch behind
hipkkt_update_scaling[_dev|_ex]) against the 50-digit reference of tests/soc_scaling_reference.py, at the shapes where the kernel takes
another path: cones longer than one and two passes of its 256-thread loops (257 for the `i = t` loops, 258 for the `i = 1 + t` ones), the
single-thread dense form (dim <= 4), 200 cones whose three tables (kSocUv0, kSocOrd, kSocHs0) all differ, Nonnegative cones across the
workgroup edges of k_scaling_diag.

Gates (soc_scaling_reference.check_rows; tests/test_soc_scaling_reference.py holds the stand-in and a numpy emulation of the kernel's
order of operations to the same ones, and shows that planted defects miss them):
  * R1 .. R4 per cone and point: <= 8 x max(the stand-in's residual there, C unit), C = the stand-in's largest normalised residual;
  * forward error of w, lambda, eta against the exact scaling: early points <= 8 x max(the stand-in's, its worst over the early points),
    late points <= soc_scaling_reference.allowance (first-order propagation of the kernel's own summation depth);
  * what K, u, v hold: bit for bit from the returned (w, eta), row 0 of a sparse cone to row0_tolerance.
Handles are built as tests/test_gpu_step_edges._handle builds them."""
import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd.kktsolver import HipKKTSolver
from tests import soc_scaling_reference as ssr
from tests.step_support import _prep
from tests.test_gpu_kkt import _DevBuf

pytestmark = pytest.mark.gpu


def _new_handle(name):
    Pt, A, cones = _prep(ssr.problem(name))
    m, n = A.shape
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    assert hk.steps_on_device
    h = hk.h
    umaps = [(h.sparse_map(i, 0), h.sparse_map(i, 1), h.sparse_map(i, 3)) for i in range(h.nsparse)]
    return hk, h.map(2), umaps


@pytest.fixture(scope="module", params=list(ssr.CONE_SETS))
def handle(request):
    return (request.param,) + _new_handle(request.param)


def _state(h, ok, w, lam, eta):
    """everything a scaling call leaves behind, as bytes"""
    assert ok
    return tuple(a.tobytes() for a in (h.debug_dump(4), w, lam, eta, h.debug_dump(7), h.debug_dump(8)))


@pytest.mark.parametrize("seed,late", ssr.POINTS)
def test_device_scaling_against_the_exact_scaling(handle, seed, late):
    name, hk, map_hs, umaps = handle
    tag = f"device {name} seed {seed} {'late' if late else 'early'}"
    cones, s, z = ssr.host_cones(name, seed, late)
    host = ssr.standin_figures(name, seed, late)
    C, early = ssr.standin_constants()
    print(f"[soc scaling] C (the stand-in's largest normalised residual) {C}, its worst early forward errors {early}")
    ok, w, lam, eta = hk.h.update_scaling(s, z)
    first = _state(hk.h, ok, w, lam, eta)
    K, u_all, v_all = hk.h.debug_dump(4), hk.h.debug_dump(7), hk.h.debug_dump(8)
    ssr.check_diag_rows(tag, cones, K, map_hs, s, z, w, lam)
    d = ssr.check_soc_entries(tag, cones, K, map_hs, umaps, w, lam, eta, u_all, v_all)
    rows = ssr.figures_of(cones, s, z, host.exact, w, lam, eta, u_all, v_all, lambda k, c: d[k])
    tols = ssr.late_tolerances(cones, s, z, host.exact) if late else None
    worst = ssr.check_rows(tag, rows, host.rows, late, tols, C, early)
    print(f"[soc scaling {tag}] worst value / gate {worst}")
    # the same input again: the same bytes
    assert _state(hk.h, *hk.h.update_scaling(s, z)) == first


def test_device_pointer_and_ex_forms_leave_the_same_bits(handle):
    name, hk, map_hs, umaps = handle
    seed, late = ssr.POINTS[-1]
    cones, s, z = ssr.host_cones(name, seed, late)
    ok, w, lam, eta = hk.h.update_scaling(s, z)
    want = _state(hk.h, ok, w, lam, eta)
    wipe = ssr.host_cones(name, *ssr.POINTS[0])
    assert _state(hk.h, *hk.h.update_scaling(wipe[1], wipe[2])) != want      # so that the next call must rewrite everything
    sd, zd = _DevBuf(s), _DevBuf(z)
    wd, ld, ed = _DevBuf(len(w)), _DevBuf(len(lam)), _DevBuf(len(eta))
    assert hk.h.update_scaling_dev(sd.ptr, zd.ptr, None, wd.ptr, ld.ptr, ed.ptr)
    assert _state(hk.h, True, wd.get(), ld.get(), ed.get()) == want
    hk.h.update_scaling(wipe[1], wipe[2])
    ok, w2, lam2, eta2, _ = hk.h.update_scaling_ex(s, z, 0.25, 0)
    assert _state(hk.h, ok, w2, lam2, eta2) == want


def _failing_inputs(cones, s, z):
    """(label, s, z) with ONE second-order cone made to fail: the first, a middle and the last one, of the sparse and of the dense form.
    `wscale == 0` is not among them: <sbar, zbar> >= 1 for any two points inside the cone, so res(sbar + J zbar) = 2 + 2 <sbar, zbar> >= 4
    and no finite interior (s, z) reaches it; it is not constructed."""
    socs = ssr.soc_list(cones)
    for form, members in (("sparse", [t for t in socs if t[4] is not None]), ("dense", [t for t in socs if t[4] is None])):
        for where, (k, c, r, _, _) in (("first", members[0]), ("middle", members[len(members) // 2]), ("last", members[-1])):
            label = f"{where} {form} cone, ordinal {k}, SOC({c.dim})"
            zb = z.copy()
            zb[r] = 0.0
            zb[r.start], zb[r.start + 1] = 5.0, 5.0
            if c.dim > 2:
                zb[r.start + 1], zb[r.stop - 1] = 3.0, 4.0      # |z1|^2 = 25 in any summation order: exactly on the boundary
            yield label + ": z on the boundary", s, zb
            so = s.copy()
            so[r.start] = 0.5 * float(np.linalg.norm(s[r][1:]))
            yield label + ": s outside", so, z
            zn = z.copy()
            zn[r.stop - 1] = np.nan
            yield label + ": NaN in z", s, zn
            si = s.copy()
            si[r.start + (c.dim > 256) * 256] = np.inf
            yield label + ": Inf in s", si, z


def test_a_failing_cone_is_reported_and_a_later_call_repairs_everything(handle):
    """include/hipkkt.h: scaling_ok = 0 with HIPKKT_OK (no exception), the state is then unspecified; the next good call leaves what a
    fresh handle that saw only the good call holds"""
    name, hk, map_hs, umaps = handle
    seed, late = ssr.POINTS[1]
    cones, s, z = ssr.host_cones(name, seed, late)
    fresh = _new_handle(name)[0]
    want = _state(fresh.h, *fresh.h.update_scaling(s, z))
    count = 0
    for label, sb, zb in _failing_inputs(cones, s, z):
        ok, *_ = hk.h.update_scaling(sb, zb)
        assert not ok, label
        assert _state(hk.h, *hk.h.update_scaling(s, z)) == want, label
        count += 1
    assert count == 24
