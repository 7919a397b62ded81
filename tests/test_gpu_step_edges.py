"""The device-resident interior-point step (step.hip, hipkkt_cone_* / hipkkt_step_*) cone by cone, at the shapes where its kernels take
another path: second-order cones longer than one pass of a 256-thread workgroup, every reachable exit of soc_step_component,
Nonnegative rows at the edges of a row block, a final step-length reduction and norms that wrap, cone sets without rows or without
cones.  Handles are built as test_gpu_device_step._scaled_solver builds them and the host cones adopt the device's (w, lambda, eta).

Gates (the project's own, from test_gpu_device_step.py; no new number):
  * Zero / Nonnegative rows: BIT-IDENTICAL to the stand-in;
  * second-order rows: within _allowance of the stand-in, through _check_cone_vector (which prints error / allowance per cone);
  * step lengths: PARITY (1e-10 relative) against the stand-in's value for the one cone whose rows the direction touches, and on
    scale_cones points also against the 50-digit smallest positive root (tests/step_reference.py; test_step_reference.py shows that
    the stand-in alone meets that on these directions); exact where the result is the cap or a quotient of a single row;
  * norms: SUM_TOL * t against the 50-digit norms.
Every test re-checks debug_dump(4): no step call writes K."""
import numpy as np
import pytest
import scipy.sparse as sp

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd.cone_api import nvars
from clarabel_jl_amd.kktsolver import HipKKTSolver
from julia_standin import ipm
from julia_standin.cones import NonnegativeCone, SecondOrderCone, ZeroCone
from tests import step_reference as sr
from tests.step_support import (PARITY, STEP_FLAGS, SUM_TOL, _adopt, _allowance, _check_cone_vector, _mixed_problem, _prep, _soc_affine_ds,
                                _soc_mul_hs, _soc_offset, _soc_shift)

pytestmark = pytest.mark.gpu


def _problem(specs, seed, n=24, density=0.05):
    """a sparse random A plus an identity block, P = M M' + I, for the cone set `specs`"""
    rng = np.random.default_rng(seed)
    m = sum(nvars(c) for c in specs)
    n = min(n, m)
    A = sp.random(m, n, density=density, random_state=np.random.RandomState(seed), format="csc") + \
        sp.vstack([sp.identity(n), sp.csc_matrix((m - n, n))]).tocsc()
    Pm = sp.random(n, n, density=0.1, random_state=np.random.RandomState(seed + 1))
    P = (Pm @ Pm.T + sp.identity(n)).tocsc()
    return P, rng.standard_normal(n), A.tocsc(), rng.standard_normal(m), specs


def _handle(prob, seed, late):
    """(hk, cones, s, z, rng): the handle scaled at step_reference.scaled_point(seed, late), the host cones on the device's scaling"""
    Pt, A, cones = _prep(prob)
    m, n = A.shape
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    assert hk.steps_on_device
    s, z, rng = sr.scaled_point(cones, seed, late)
    ok, w, lam, eta = hk.h.update_scaling(s, z)
    assert ok
    _adopt(cones, w, lam, eta)
    return hk, cones, s, z, rng


def _check_four_operations(hk, cones, s, z, rng, late, tag):
    """affine_ds, combined_ds_shift, ds_from_dz_offset, mul_Hs against the stand-in under the project's gates; inputs stay intact"""
    m = cones.numel
    ref = np.zeros(m)
    cones.affine_ds(ref, s)
    first = hk.cone_affine_ds()
    _check_cone_vector(cones, first, ref, lambda c, r: _allowance(_soc_affine_ds, 1, c), tag + " affine_ds")
    dz, ds, sm = rng.standard_normal(m), rng.standard_normal(m), 0.37 * (1e-9 if late else 1.0)
    dz0, ds0 = dz.copy(), ds.copy()
    got = hk.cone_combined_ds_shift(dz, ds, sm)
    assert np.array_equal(dz, dz0) and np.array_equal(ds, ds0)
    ref = np.zeros(m)
    cones.combined_ds_shift(ref, dz.copy(), ds.copy(), sm)
    _check_cone_vector(cones, got, ref, lambda c, r: _allowance(_soc_shift, 3, c, dz[r], ds[r], sm), tag + " combined_ds_shift")
    v = rng.standard_normal(m)
    v0 = v.copy()
    ref = np.zeros(m)
    cones.ds_from_dz_offset(ref, v, np.zeros(m), z)
    _check_cone_vector(cones, hk.cone_ds_from_dz_offset(v), ref, lambda c, r: _allowance(_soc_offset, 3, c, z[r], v[r]),
                       tag + " ds_from_dz_offset")
    ref = np.zeros(m)
    cones.mul_Hs(ref, v, np.zeros(m))
    _check_cone_vector(cones, hk.cone_mul_hs(v), ref, lambda c, r: _allowance(_soc_mul_hs, 1, c, v[r]), tag + " mul_Hs")
    assert np.array_equal(v, v0)
    # no step call wrote the resident scaling: the first operation again, bit for bit
    assert np.array_equal(hk.cone_affine_ds(), first)


def _isolated(cones, r, yz, ys):
    dz, ds = np.zeros(cones.numel), np.zeros(cones.numel)
    dz[r], ds[r] = yz, ys
    return dz, ds


def _close(got, want):
    return abs(got - want) <= PARITY * abs(want)


def _check_isolated_step_lengths(hk, cones, s, z, rng, late, tag):
    """every cone alone: a direction that is zero outside its rows, so that every other cone returns alpha_max exactly"""
    for k, (c, r, dirs) in enumerate(sr.per_cone_directions(cones, s, z, rng)):
        for name, (yz, ys, amax) in dirs.items():
            az, as_ = hk.cone_step_length(*_isolated(cones, r, yz, ys), amax)
            rz, rs = c.step_length(yz, ys, z[r], s[r], amax)
            assert _close(az, rz) and _close(as_, rs), (tag, k, type(c).__name__, c.dim, name, az, rz, as_, rs)
            if isinstance(c, (ZeroCone, NonnegativeCone)):
                assert (az, as_) == (rz, rs), (tag, k, name)      # no sums in these rows
            if name == "never hits":
                assert (az, as_) == (amax, amax), (tag, k, name)
            if isinstance(c, SecondOrderCone) and not late:
                tz, ts = float(sr.def_step_length(z[r], yz, amax)), float(sr.def_step_length(s[r], ys, amax))
                assert _close(az, tz) and _close(as_, ts), (tag, k, c.dim, name, az, tz, as_, ts)


POINTS = [(seed, late) for late in (False, True) for seed in sr.POINT_SEEDS]


# ---- A. long cones and pass boundaries, B. the step length of one cone at a time ---------------------------------------------------------

@pytest.mark.parametrize("seed,late", POINTS)
def test_long_second_order_cones_match_the_host_cones(seed, late):
    """SOC(d), d = 2, 255, 256, 257, 258, 511, 512, 513, 1025: 257 is the first dimension at which the `i = t` loops of the
    second-order kernels take a second pass, 258 the first at which tail_dot does"""
    hk, cones, s, z, rng = _handle(_problem(sr.long_cone_specs(), 21), seed, late)
    K0 = hk.h.debug_dump(4)
    _check_four_operations(hk, cones, s, z, rng, late, "long cones")
    assert np.array_equal(hk.h.debug_dump(4), K0)


@pytest.mark.parametrize("seed,late", POINTS)
def test_step_length_of_every_cone_alone(seed, late):
    for tag, prob in (("long cones", _problem(sr.long_cone_specs(), 21)), ("mixed cones", _mixed_problem(3))):
        hk, cones, s, z, rng = _handle(prob, seed, late)
        K0 = hk.h.debug_dump(4)
        _check_isolated_step_lengths(hk, cones, s, z, rng, late, tag)
        assert np.array_equal(hk.h.debug_dump(4), K0)


# ---- C. every reachable exit of soc_step_component ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", sr.POINT_SEEDS)
def test_every_reachable_exit_of_the_second_order_step_length(seed):
    """step_reference.soc_exit_cases on SOC(2), SOC(3), SOC(258); test_step_reference.py holds that each input takes the exit it is
    named for in a float64 evaluation.  `c == 0` needs a resident point on the boundary, which update_scaling rejects: not tested."""
    hk, cones, s, z, rng = _handle(_problem(sr.exit_cone_specs(), 22), seed, False)
    K0 = hk.h.debug_dump(4)
    seen = set()
    for c, r in sr.soc_cones(cones):
        cz, cs = sr.soc_exit_cases(z[r]), sr.soc_exit_cases(s[r])
        assert tuple(cz) == tuple(cs) == sr.EXIT_CASE_NAMES
        for name in sr.EXIT_CASE_NAMES:
            (yz, amax_z, _), (ys, amax_s, _) = cz[name], cs[name]
            # (the cap of a case may depend on the point: z and s are asked one after the other, the other side's direction zero)
            az, _ = hk.cone_step_length(*_isolated(cones, r, yz, np.zeros(c.dim)), amax_z)
            _, as_ = hk.cone_step_length(*_isolated(cones, r, np.zeros(c.dim), ys), amax_s)
            for got, x, y, amax in ((az, z[r], yz, amax_z), (as_, s[r], ys, amax_s)):
                info = sr.soc_step_exit(x, y, amax)
                want = c.step_length(y, y, x, x, amax)[0]
                assert want == info["value"]
                print(f"[step edges exit] SOC({c.dim}) {name}: exit {info['exit']}, returned {info['returned']}, device {got!r}, host {want!r}")
                if info["returned"] == "root":
                    assert _close(got, want), (c.dim, name, got, want)
                    assert _close(got, float(sr.def_step_length(x, y, amax))), (c.dim, name, got)
                elif name == "d negative" and info["linear_bound"]:
                    assert _close(got, want), (c.dim, name, got, want)      # the linear bound -x0 / y0, one division
                else:
                    assert got == want, (c.dim, name, got, want)           # the cap itself
                seen.add(info["exit"])
    assert seen == sr.REACHABLE_EXITS
    assert np.array_equal(hk.h.debug_dump(4), K0)


# ---- D. Nonnegative rows at the edges of a row block --------------------------------------------------------------------------------------

def test_nonnegative_step_length_at_block_edges():
    hk, cones, s, z, rng = _handle(_problem([cl.NonnegativeConeT(600)], 23), sr.POINT_SEEDS[0], False)
    K0 = hk.h.debug_dump(4)
    nn = cones.cones[0]
    amax = 10.0
    special = {1: -0.0, 257: 0.0, 598: -5e-324}      # not below zero, zero, and a quotient far above the cap

    def host(dz, ds):
        with np.errstate(over="ignore", divide="ignore"):
            return nn.step_length(dz, ds, z, s, amax)

    for i in (0, 255, 256, 511, 512, 599):
        dz, ds = rng.random(600), rng.random(600)
        dz[rng.random(600) < 0.3] = 0.0
        for j, v in special.items():
            dz[j], ds[599 - j] = v, v
        dz[i] = -(1.0 + rng.random())
        ds[599 - i] = -(1.0 + rng.random())
        dz0, ds0 = dz.copy(), ds.copy()
        az, as_ = hk.cone_step_length(dz, ds, amax)
        assert np.array_equal(dz, dz0) and np.array_equal(ds, ds0)
        assert (az, as_) == (-z[i] / dz[i], -s[599 - i] / ds[599 - i]), (i, az, as_)
        assert (az, as_) == host(dz, ds), i
        assert az < amax and as_ < amax
    # nothing but the three special rows is negative: the cap
    dz, ds = rng.random(600), rng.random(600)
    for j, v in special.items():
        dz[j], ds[599 - j] = v, v
    assert hk.cone_step_length(dz, ds, amax) == host(dz, ds) == (amax, amax)
    assert np.array_equal(hk.h.debug_dump(4), K0)


# ---- E. the final reduction of the step length wraps ----------------------------------------------------------------------------------------

def test_step_length_reduction_over_more_than_256_pairs():
    """Nonnegative(300) and 300 second-order cones of dimension 2, 3, 4: m = 1200 rows in 5 row blocks, so 305 (alpha_z, alpha_s)
    pairs: k_step_len_final takes a second pass from second-order cone 251 on, and the pairs of the cones start at part + 2 * 5.
    Every cone in turn is the only one that binds.  Then one fused affine step on the same handle."""
    specs = [cl.NonnegativeConeT(300)] + [cl.SecondOrderConeT(2 + k % 3) for k in range(300)]
    prob = _problem(specs, 24)
    S = cl.Solver(*prob, cl.Settings(device_step=True, **STEP_FLAGS))
    assert S._device_step
    ks, data, cones, v = S.kktsystem.kktsolver, S.data, S.cones, S.variables
    n, m = data.n, data.m
    assert len(cones.cones) == 301 and (m + 255) // 256 + 300 > 256
    s, z, rng = sr.scaled_point(cones, sr.POINT_SEEDS[0], False)
    v.x[:], v.z[:], v.s[:], v.tau, v.kappa = rng.standard_normal(n), z, s, 0.9, 0.4
    xzs, res = ks.device_buffer(n + 2 * m), ks.device_buffer(3 * n + 2 * m)
    xzs.upload(np.concatenate([v.x, v.z, v.s]))
    ks.residuals_update_dev(xzs, res, v.tau, v.kappa)
    S._residuals_update()
    r = S.residuals
    assert ks.kktsolver_update_scaled(cones, v.s, v.z)
    _adopt(cones, ks.scaling_w, ks.scaling_lambda, ks.scaling_soc_eta)
    K0 = ks.h.debug_dump(4)
    amax = 1.0
    for k, (c, rr) in enumerate(zip(cones.cones, cones.rng_cones)):
        yz, ys = sr.binding_direction(z[rr], rng), sr.binding_direction(s[rr], rng)
        az, as_ = ks.cone_step_length(*_isolated(cones, rr, yz, ys), amax)
        rz, rs = c.step_length(yz, ys, z[rr], s[rr], amax)
        assert 0.0 < rz < amax and 0.0 < rs < amax
        assert _close(az, rz) and _close(as_, rs), (k, c.dim, az, rz, as_, rs)
    assert np.array_equal(ks.h.debug_dump(4), K0)
    # the fused affine step: alpha from the DEVICE's own dz, ds through the host cones
    ok, alpha, dtau, dkappa = ks.kktsolver_step_affine(xzs, res, v.tau, v.kappa, r.rtau, True)
    assert ok and np.array_equal(ks.h.debug_dump(4), K0)
    step = ks.h.step_get()
    dz, ds = step[n:n + m], step[n + m:]
    assert dkappa == -(v.tau * v.kappa + v.kappa * dtau) / v.tau
    a_tau = -v.tau / dtau if dtau < 0 else ipm.FLOATMAX
    a_kap = -v.kappa / dkappa if dkappa < 0 else ipm.FLOATMAX
    az, as_ = cones.step_length(dz, ds, v.z, v.s, min(a_tau, a_kap, 1.0))
    a_ref = min(az, as_)
    per_cone = [min(c.step_length(dz[rr], ds[rr], v.z[rr], v.s[rr], 1.0)) for c, rr in zip(cones.cones, cones.rng_cones)]
    print(f"[step edges fused affine] alpha {alpha!r}, from the device's step through the host cones {a_ref!r}; the binding cone is "
          f"number {int(np.argmin(per_cone))} of 301 (tau / kappa bound {min(a_tau, a_kap)!r})")
    assert abs(alpha - a_ref) <= PARITY * a_ref, (alpha, a_ref)


# ---- F. norms that wrap --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def norm_handle():
    """n = 16384 + 5, m = 2 * 16384 + 3 Nonnegative rows: k_step_norm_part covers 64 * 256 = 16384 elements per pass, so the n-long
    vectors take a second pass and the m-long ones a third.  P diagonal, A = identity over one entry per row."""
    n, m = 16384 + 5, 2 * 16384 + 3
    rng = np.random.default_rng(25)
    P = sp.diags(1.0 + rng.random(n)).tocsc()
    low = sp.csc_matrix((rng.standard_normal(m - n), (np.arange(m - n), rng.integers(0, n, m - n))), shape=(m - n, n))
    A = sp.vstack([sp.identity(n), low]).tocsc()
    Pt, A, cones = _prep((P, None, A, None, [cl.NonnegativeConeT(m)]))
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    d, e = 10.0 ** rng.uniform(-2.0, 2.0, n), 10.0 ** rng.uniform(-2.0, 2.0, m)
    hk.set_equilibration(d, e)
    assert hk.h.update_scaling(np.ones(m), np.ones(m))[0]      # (so that every value of K that debug_dump(4) returns is defined)
    return hk, n, m, d, e, rng


@pytest.mark.parametrize("variant", ["six decades either way", "one huge entry on the second and on the last pass"])
def test_info_norms_over_more_than_one_pass(norm_handle, variant):
    hk, n, m, d, e, rng = norm_handle
    K0 = hk.h.debug_dump(4)

    def spread(k):
        return rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(-6.0, 6.0, k)

    if variant == "six decades either way":
        host_xzs, host_res = spread(n + 2 * m), spread(3 * n + 2 * m)
    else:
        host_xzs, host_res = rng.standard_normal(n + 2 * m), rng.standard_normal(3 * n + 2 * m)
        # index 16384 (second pass) and the last index (second pass of an n-long vector, third of an m-long one) of each of the eight
        for buf, starts_lens in ((host_xzs, ((0, n), (n, m), (n + m, m))),
                                 (host_res, ((0, n), (n, m), (n + m, n), (2 * n + m, m), (2 * n + 2 * m, n)))):
            for start, ln in starts_lens:
                buf[start + 16384] = 3e9
                buf[start + ln - 1] = -7e10
    xzs, res = hk.device_buffer(n + 2 * m), hk.device_buffer(3 * n + 2 * m)
    xzs.upload(host_xzs)
    res.upload(host_res)
    got = hk.kktsolver_info_norms(xzs, res)
    again = hk.kktsolver_info_norms(xzs, res)
    assert np.array_equal(got, again)                        # fixed slices, fixed order: deterministic
    ref = sr.ref_info_norms(d, e, host_xzs, host_res)
    for k, (g, t) in enumerate(zip(got, ref)):
        rel = float(abs(sr.mpf(float(g)) - t) / t)
        print(f"[step edges info norm {k}, {variant}] relative difference to 50 digits {rel:.2e}")
        assert rel <= SUM_TOL, (k, g, float(t))
    assert np.array_equal(xzs.download(), host_xzs) and np.array_equal(res.download(), host_res)
    assert np.array_equal(hk.h.debug_dump(4), K0)
    xzs.close()
    res.close()


# ---- G. degenerate cone sets ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,specs", [
    ("zero only", [cl.ZeroConeT(5)]),
    ("second-order only", [cl.SecondOrderConeT(5), cl.SecondOrderConeT(3), cl.SecondOrderConeT(300), cl.SecondOrderConeT(2)]),
])
def test_cone_sets_without_rows_or_without_cones(name, specs):
    """no second-order cone (the cone kernels are not launched), and no Zero / Nonnegative row (the row kernels run over second-order
    rows only and must leave them alone)"""
    for late in (False, True):
        hk, cones, s, z, rng = _handle(_problem(specs, 26, n=4), sr.POINT_SEEDS[0], late)
        K0 = hk.h.debug_dump(4)
        _check_four_operations(hk, cones, s, z, rng, late, name)
        _check_isolated_step_lengths(hk, cones, s, z, rng, late, name)
        # all cones at once
        m = cones.numel
        dz = -(0.5 + rng.random(m)) * z + 0.3 * np.abs(z) * rng.standard_normal(m)
        ds = -(0.5 + rng.random(m)) * s + 0.3 * np.abs(s) * rng.standard_normal(m)
        az, as_ = hk.cone_step_length(dz, ds, 1.0)
        rz, rs = 1.0, 1.0
        for c, r in zip(cones.cones, cones.rng_cones):
            a, b = c.step_length(dz[r], ds[r], z[r], s[r], 1.0)
            rz, rs = min(rz, a), min(rs, b)
        assert _close(az, rz) and _close(as_, rs), (name, az, rz, as_, rs)
        if name == "zero only":
            assert (az, as_) == (1.0, 1.0)
        assert np.array_equal(hk.h.debug_dump(4), K0)
