"""Every branch of the device-decided iterative refinement (refine.hip k_refine_decide) and everything that has to be redone when a
solve needs more refinement steps than the one inside its captured graph (hipkkt_solve.cpp solve_finish: the device copy-out;
kkt_solve_reduced_impl: the speculative reduction; hipkkt_step.cpp: the work chained behind it), by construction.

A. Forced step counts.  reltol = abstol = 0 and stop_ratio = 0 make the loop take exactly max_iter steps and accept every candidate (the
   ABI does not refuse zeros: a refused value would raise HipKKTError in every case here); static_regularization_constant = 1e-2 makes
   every step move the solution by far more than any gate (asserted on the oracle: consecutive iterates up to three steps differ by
   >= 1e-6 max(1, |x|)).  So a result that is a step short -- a stale copy-out, a stale reduction -- is 1e4 gates away.
B. The decision branches through a STALE FACTOR: factorise, scale every stored value of K by c, do not refactor.  Refinement then
   iterates with M ~ K / c against K, the error is multiplied by 1 - c per step: c = 4 makes the candidate worse (ratio 1/3), c = 0.5
   improves by 2 (below stop_ratio: take it, stop), c = 0.875 improves by 8 per step.  The same sequence runs on the CPU oracle on the
   handle's own elimination order; before anything is asserted about the device, the oracle's residual norms are asserted to be
   decisive (refinement_support.assert_decisive: ratios 1.5 away from 1 and stop_ratio, norms a factor 2 away from the tolerance).

Gates: refined solves 1e-10 max(1, |x|) (the header of test_gpu_kkt.py); the stale-factor iterates 1e-9 max(1, |x|) (that file's gate
for unrefined solves: the accuracy of these iterates is that of the first solve; neighbouring iterates differ by >= 1e-5 there);
residual rows 1e-13 (|K| |x| + |b|) against the correctly rounded residual (the bound of test_dense_triangle_spmv_matches_host_product);
step counts, bit-identities and norms `==`."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt
from tests import default_start_reference as dr
from tests.accuracy import exact_residual
from tests.refinement_support import (DEFAULT_REG, PROBLEMS, assert_decisive, deviation, forced, gpu_solve, ir_kw, system, with_ir)

pytestmark = pytest.mark.gpu

REFINED_GATE = 1e-10
UNREFINED_GATE = 1e-9
NAMES = list(PROBLEMS)


@pytest.fixture(autouse=True)
def _front_batches_on_small_fronts(monkeypatch):
    """as in test_gpu_kkt.py: small fronts take the front-batch factorisation too"""
    if os.environ.get("HIPKKT_TEST_PRODUCTION", "0") != "1":
        monkeypatch.setenv("HIPKKT_FRONT_BLOCK_MIN_ROWS", "0")


def _unrefined(hk, rx, rz):
    return gpu_solve(hk, with_ir(hk.settings.static_regularization_constant, enable=False), rx, rz)


# ---- A. the extra-step loop on every entry point -----------------------------------------------------------------------------------------

def _forced_solve_case(name, k):
    S = system(name)
    st = forced(k, S.reg)
    hk = S.handle(st)
    gaps = S.assert_forced_iterates_differ()
    x, z, steps = gpu_solve(hk, st, S.rx[0], S.rz[0])
    xo, zo, so, _ = S.oracle_solve(st, S.rx[0], S.rz[0], key=0)
    dev = deviation(x, z, xo, zo)
    print(f"[refinement forced {name} k={k}] steps {steps} (oracle {so}); |x - oracle| / max(1, |x|) {dev:.2e}; the oracle's iterates "
          f"after 0..3 steps differ by {', '.join(f'{g:.1e}' for g in gaps)}")
    assert so == k and steps == k
    assert dev <= REFINED_GATE
    return S, hk, st, x, z


@pytest.mark.parametrize("k", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("name", NAMES)
def test_forced_step_count_on_solve(name, k):
    S, hk, st, x, z = _forced_solve_case(name, k)
    if k == 0:       # a refined solve that may take no step returns the bits of the unrefined solve
        x0, z0, s0 = _unrefined(hk, S.rx[0], S.rz[0])
        assert s0 == 0 and np.array_equal(x0, x) and np.array_equal(z0, z)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_residual_kernels_read_the_candidate(name, k):
    """k_spmv_residual / k_spmv_long / k_spmv_dense_tri with a refinement state: the residual left by the last step (debug_dump 18) is
    that of the last candidate = the returned iterate (debug_dump 26: with its expansion variables), row by row against the correctly
    rounded b - K x; the state's norms are exactly the norms of that residual and of b.  From the second step on the candidate buffer
    alternates."""
    S, hk, st, x, z = _forced_solve_case(name, k)
    n, m, N = S.n, S.m, hk.h.N
    K = S.K(hk)
    if name == "sdp_blocks":
        assert int(hk.h.debug_dump(19)[0]) == 8
    if name == "portfolio_small":
        assert int(np.max(np.diff(K.indptr))) > 192          # a row for k_spmv_long (refine.hip kLongRow): the case is not vacuous
    e = hk.h.debug_dump(18)
    xfull = hk.h.debug_dump(26)
    assert len(e) == N and len(xfull) == N
    assert np.array_equal(xfull[:n], x) and np.array_equal(xfull[n:n + m], z)
    bfull = np.concatenate([S.rx[0], S.rz[0], np.zeros(N - n - m)])
    r, d = exact_residual(K, xfull, bfull)
    worst = float(np.max(np.abs(e - r) / np.maximum(d, 1e-300)))
    lastnorme, normb, norme, steps = hk.h.debug_dump(17)
    print(f"[refinement residual {name} k={k}] worst row |e - (b - K x)| / (|K| |x| + |b|) {worst:.2e}; norme {norme:.3e}")
    assert np.all(np.abs(e - r) <= 1e-13 * d)
    assert steps == k
    assert norme == float(np.max(np.abs(e)))
    assert normb == float(np.max(np.abs(bfull)))
    assert lastnorme == norme                                # (every candidate was accepted)


@pytest.mark.parametrize("name", NAMES)
def test_entry_points_return_the_same_bits_after_three_steps(name):
    """solve, solve_dev, solve_multi (three right-hand sides: two rounds, both contexts) and solve_multi_dev at k = 3: the second
    copy-out of solve_finish.  A stale device copy holds the one-step iterate."""
    S = system(name)
    st = forced(3, S.reg)
    hk = S.handle(st)
    S.assert_forced_iterates_differ()
    n, m = S.n, S.m
    kw = ir_kw(st)
    ref = []
    for r in range(3):
        x, z, steps = gpu_solve(hk, st, S.rx[r], S.rz[r])
        assert steps == 3
        xo, zo, so, _ = S.oracle_solve(st, S.rx[r], S.rz[r], key=r)
        assert so == 3 and deviation(x, z, xo, zo) <= REFINED_GATE
        ref.append(np.concatenate([x, z]))
    out = hipkkt.DeviceBuffer(n + m)
    for r in range(3):
        hk.kktsolver_setrhs(S.rx[r], S.rz[r])
        ok, steps = hk.h.solve_dev(out.ptr, **kw)
        assert ok and steps == 3
        assert np.array_equal(out.download(), ref[r]), ("solve_dev", r)
    lx, lz = np.zeros((3, n)), np.zeros((3, m))
    ok, steps = hk.h.solve_multi(S.rx, S.rz, lx, lz, **kw)
    assert ok and list(steps) == [3, 3, 3]
    for r in range(3):
        assert np.array_equal(np.concatenate([lx[r], lz[r]]), ref[r]), ("solve_multi", r)
    rhs, outs = hipkkt.DeviceBuffer(3 * (n + m)), hipkkt.DeviceBuffer(3 * (n + m))
    rhs.upload(np.concatenate([np.concatenate([S.rx[r], S.rz[r]]) for r in range(3)]))
    ok, steps = hk.h.solve_multi_dev(3, rhs.ptr, outs.ptr, **kw)
    assert ok and list(steps) == [3, 3, 3]
    got = outs.download().reshape(3, n + m)
    for r in range(3):
        assert np.array_equal(got[r], ref[r]), ("solve_multi_dev", r)
    for b in (out, rhs, outs):
        b.close()


def _check_reduced(S, hk, st, q, b, rhs_x, workz, var_x, scal_in, sc, lhs, what):
    """the ten scalars and lhs of a reduced solve against the reference's formulas in numpy on the solve_multi results of the same
    options (gates of test_gpu_kkt.py test_kkt_solve_reduced_on_device) -> the step counts of those two solves (constant, this)"""
    n, m = S.n, S.m
    tau, kappa, rtau, rkappa = scal_in
    X, Z = np.zeros((2, n)), np.zeros((2, m))
    ok, steps = hk.h.solve_multi(np.vstack([-q, rhs_x]), np.vstack([b, workz]), X, Z, **ir_kw(st))
    assert ok
    x2, z2, x1, z1 = X[0], Z[0], X[1], Z[1]
    Pfull = (S.Pt + sp.triu(S.Pt, 1).T).tocsr()
    xi = var_x / tau
    terms = [(q, x1), (b, z1), (xi, Pfull @ x1), (q, x2), (b, z2), (xi - x2, Pfull @ (xi - x2)), (x2, Pfull @ x2)]
    for i, (got, (a, c)) in enumerate(zip(sc[3:10], terms)):
        assert abs(got - float(a @ c)) <= 1e-13 * max(1.0, float(np.abs(a) @ np.abs(c))), (what, i, got, float(a @ c))
    num = rtau - rkappa / tau + sc[3] + sc[4] + 2.0 * sc[5]
    den = kappa / tau - sc[6] - sc[7] + sc[8] - sc[9]
    assert abs(sc[1] - num) <= 1e-15 * max(1.0, abs(num)) * 8 and abs(sc[2] - den) <= 1e-15 * max(1.0, abs(den)) * 8, what
    dtau = sc[0]
    assert abs(dtau - sc[1] / sc[2]) <= 1e-15 * abs(dtau) and abs(dtau - num / den) <= 1e-13 * max(1.0, abs(num / den)), what
    lx, lz = lhs[:n], lhs[n:]
    assert np.max(np.abs(lx - (x1 + dtau * x2))) <= 1e-13 * max(1.0, np.max(np.abs(x1)) + abs(dtau) * np.max(np.abs(x2))), what
    assert np.max(np.abs(lz - (z1 + dtau * z2))) <= 1e-13 * max(1.0, np.max(np.abs(z1)) + abs(dtau) * np.max(np.abs(z2))), what
    return list(steps)


def _reduced_call(hk, st, on_device, rhs_x, workz, var_x, scal_in, pending):
    n, m = hk.n, hk.m
    if on_device:
        inp, out = hipkkt.DeviceBuffer(2 * n + m), hipkkt.DeviceBuffer(n + m)
        inp.upload(np.concatenate([rhs_x, workz, var_x]))
        ok, dtau, sc, steps = hk.h.kkt_solve_reduced_dev(inp.ptr, *scal_in, pending, out.ptr, **ir_kw(st))
        lhs = out.download()
        inp.close()
        out.close()
    else:
        lx, lz = np.zeros(n), np.zeros(m)
        ok, dtau, sc, steps = hk.h.kkt_solve_reduced(rhs_x, workz, var_x, *scal_in, pending, lx, lz, **ir_kw(st))
        lhs = np.concatenate([lx, lz])
    assert ok and dtau == sc[0]
    return sc, list(steps), lhs


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("name", ["plain", "portfolio_small"])
def test_reduced_solve_repeats_its_reduction_after_three_steps(name, on_device):
    """kkt_solve_reduced / kkt_solve_reduced_dev at k = 3, the constant-rhs solve pending and then resident: redo, join_const and
    reduce() of kkt_solve_reduced_impl.  A reduction left from the speculative pass saw the one-step iterates."""
    S = system(name)
    st = forced(3, S.reg)
    hk = S.handle(st)
    S.assert_forced_iterates_differ()
    rng = np.random.default_rng(41)
    hk.set_problem_vectors(S.q, S.b)
    for pending in (True, False):
        rhs_x, workz, var_x = rng.standard_normal(S.n), rng.standard_normal(S.m), rng.standard_normal(S.n)
        scal_in = (0.8, 0.4, float(rng.standard_normal()), float(rng.standard_normal()))
        sc, steps, lhs = _reduced_call(hk, st, on_device, rhs_x, workz, var_x, scal_in, pending)
        assert steps == ([3, 3] if pending else [3, 0]), (pending, steps)
        msteps = _check_reduced(S, hk, st, S.q, S.b, rhs_x, workz, var_x, scal_in, sc, lhs, (name, on_device, pending))
        assert msteps == [3, 3]


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("which", ["only_B", "only_A"])
def test_reduced_solve_when_only_one_context_takes_extra_steps(which, on_device):
    """one right-hand side so small that its first residual is below abstol, the other's above: only context B (the constant
    right-hand side [-q; b]) takes extra steps, then only context A.  abstol = the geometric mean of the two first-residual norms on
    the oracle, which must be a factor 16 apart"""
    S = system("plain")
    hk = S.handle(forced(3, S.reg))
    rng = np.random.default_rng(43)
    rhs_x, workz, var_x = rng.standard_normal(S.n), rng.standard_normal(S.m), rng.standard_normal(S.n)
    q, b = S.q.copy(), S.b.copy()
    tiny = 2.0 ** -40
    if which == "only_B":
        rhs_x, workz = rhs_x * tiny, workz * tiny
    else:
        q, b = q * tiny, b * tiny
    probe = forced(3, S.reg)
    nA = S.oracle_solve(probe, rhs_x, workz)[3][0]
    nB = S.oracle_solve(probe, -q, b)[3][0]
    assert max(nA, nB) >= 16.0 * min(nA, nB), (nA, nB)
    st = forced(3, S.reg)
    st.iterative_refinement_abstol = float(np.sqrt(nA * nB))
    want = [0, 3] if which == "only_B" else [3, 0]
    # the oracle takes these step counts, decided by norms a factor 2 away from abstol (the last step ends at max_iter)
    for (rx_, rz_), w in zip(((rhs_x, workz), (-q, b)), want):
        _, _, so, norms = S.oracle_solve(st, rx_, rz_)
        assert so == w and assert_decisive(norms, float(max(np.max(np.abs(rx_)), np.max(np.abs(rz_)))), st) == w
    hk.set_problem_vectors(q, b)
    scal_in = (0.8, 0.4, 0.3, -0.2)
    sc, steps, lhs = _reduced_call(hk, st, on_device, rhs_x, workz, var_x, scal_in, True)
    assert steps == want, (which, steps)
    msteps = _check_reduced(S, hk, st, q, b, rhs_x, workz, var_x, scal_in, sc, lhs, (which, on_device))
    assert msteps == want[::-1]                              # (solve_multi was given the constant right-hand side first)


FORCED_IR = dict(static_regularization_constant=1e-2, iterative_refinement_reltol=0.0, iterative_refinement_abstol=0.0,
                 iterative_refinement_stop_ratio=0.0, iterative_refinement_max_iter=3)


def test_device_step_after_three_refinement_steps():
    """hipkkt_step_affine_dev (constant-rhs solve pending) and hipkkt_step_combined_dev at the forced settings, k = 3, against the host
    loop of the stand-in under the same Settings, through the comparison and the gates of test_gpu_device_step.py: after_reduce of
    fused_solve runs twice, and alpha, dtau, dkappa and the resident [dx | dz | ds] must be those of the three-step solution"""
    from tests.test_gpu_device_step import _fused_steps_case
    _fused_steps_case(3, False, settings=FORCED_IR, expect_steps=3)


@pytest.mark.parametrize("pzero", [True, False], ids=["P0", "P"])
def test_device_default_start_after_three_refinement_steps(pzero):
    """hipkkt_step_default_start_dev at k = 3 with nnz(P) == 0 (two solves: `after` of solve_many waits for both contexts and runs
    again) and with P != 0, against the host default start of a twin under the same Settings (the harness and the comparison of
    test_gpu_default_start.py test_fused_call_matches_the_host_default_start)"""
    from tests.test_gpu_default_start import SYM_FLAGS, _handle, _host_default_start
    flags = dict(SYM_FLAGS, **FORCED_IR)
    hk, cones, prob = _handle("soc_mix", pzero, flags=flags)
    twin, tcones, _ = _handle("soc_mix", pzero, flags=flags)
    Pt, q, A, b = prob
    m, n = A.shape
    assert (Pt.nnz == 0) == pzero
    xzs = hk.device_buffer(n + 2 * m)
    hk.set_problem_vectors(q, b)
    st = hk.settings
    ok, scal, steps = hk.h.step_default_start_dev(xzs.ptr, st.static_regularization_enable, st.static_regularization_constant,
                                                  st.static_regularization_proportional, **hk._ir())
    assert ok
    got = xzs.download()
    x, z, s, hsteps, hok = _host_default_start(twin, tcones, prob)
    assert hok
    assert hsteps == ([3, 3] if pzero else [3, 0]) and list(steps) == hsteps, (list(steps), hsteps)
    assert (scal[0], int(scal[1])) == (twin.diagonal_regularizer, twin.last_nreg)
    # the unrefined start is far from this one: a start shifted from a stale copy of the solves cannot pass the comparison below
    twin.settings = cl.Settings(**dict(flags, iterative_refinement_max_iter=1))
    x1, z1, s1, _, _ = _host_default_start(twin, tcones, prob)
    assert max(np.max(np.abs(x1 - x)), np.max(np.abs(z1 - z))) >= 1e-6 * max(1.0, np.max(np.abs(x)), np.max(np.abs(z)))
    s_sh, _ = dr.apply_shift(tcones, s, "primal", scal[2], scal[4])
    z_sh, _ = dr.apply_shift(tcones, z, "dual", scal[5], scal[7])
    want = np.concatenate([x, z_sh, s_sh])
    assert dr.same_bits(got, want), (pzero, np.flatnonzero(got != want)[:8], float(np.max(np.abs(got - want))))
    xzs.close()


def test_refinement_graphs_follow_the_options():
    """one handle through k = 3 -> defaults -> k = 0 -> k = 3 -> no refinement -> k = 3: RefineOpts::same_graph, the invalidation of the
    step graph, and a first graph captured with a step inside is not replayed for max_iter = 0.  Every result carries the bits of the
    same call on a fresh handle."""
    S = system("plain")
    opts = {"k3": forced(3, S.reg), "defaults": with_ir(S.reg), "k0": forced(0, S.reg), "off": with_ir(S.reg, enable=False)}
    fresh = {}
    for key, st in opts.items():
        fresh[key] = gpu_solve(S.handle(), st, S.rx[1], S.rz[1])
    assert fresh["k3"][2] == 3 and fresh["k0"][2] == 0 and fresh["off"][2] == 0 and fresh["defaults"][2] > 1
    assert not np.array_equal(fresh["k3"][0], fresh["defaults"][0]) and not np.array_equal(fresh["k3"][0], fresh["k0"][0])
    assert np.array_equal(fresh["k0"][0], fresh["off"][0]) and np.array_equal(fresh["k0"][1], fresh["off"][1])
    hk = S.handle()
    for i, key in enumerate(["k3", "defaults", "k0", "k3", "off", "k3"]):
        x, z, steps = gpu_solve(hk, opts[key], S.rx[1], S.rz[1])
        fx_, fz_, fsteps = fresh[key]
        assert steps == fsteps and np.array_equal(x, fx_) and np.array_equal(z, fz_), (i, key, steps, fsteps)


@pytest.mark.parametrize("switch", ["HIPKKT_NO_PERSIST", "HIPKKT_NO_GRAPH"])
def test_forced_steps_under_the_sweep_switches(switch, monkeypatch):
    """k = 3 on cfg1 with the per-level solve kernels, and without captured graphs: the same step count, the same oracle gate"""
    monkeypatch.setenv(switch, "1")
    S, hk, st, x, z = _forced_solve_case("cfg1", 3)
    if switch == "HIPKKT_NO_PERSIST":
        assert not hk.h.counters()["persistent"]


# ---- B. every decision branch, by construction ------------------------------------------------------------------------------------------

def _stale_pair(c, reg=DEFAULT_REG):
    """(system, handle, oracle) factorised and then, c != 1, every stored value of K scaled by c without a new factorisation"""
    S = system("plain", reg)
    hk = S.handle()
    o = S.new_oracle()
    if c != 1.0:
        idx = np.arange(hk.h.nnzK, dtype=np.int64)
        hk.h.scale_values(idx, c)
        o.k.L.oracle_kkt_scale_values(o.k.h, idx, len(idx), c)
        assert np.array_equal(hk.h.kkt()[2], o.k.nzval)
    return S, hk, o


def _oracle_solve(o, st, rx, rz):
    o.settings = st
    x, z = np.zeros(o.n), np.zeros(o.m)
    o.kktsolver_setrhs(rx, rz)
    assert o.kktsolver_solve(x, z)
    return x, z, o.last_ir_steps, o.last_norms.copy()


def _branch_case(c, st, what, reg=DEFAULT_REG, rhs_scale=1.0):
    """the same solve on the stale handle and the stale oracle; the oracle's norms decisive; counts equal; iterates within the gate"""
    S, hk, o = _stale_pair(c, reg)
    rx, rz = S.rx[0] * rhs_scale, S.rz[0] * rhs_scale
    xo, zo, so, norms = _oracle_solve(o, st, rx, rz)
    normb = float(max(np.max(np.abs(rx)), np.max(np.abs(rz))))
    assert assert_decisive(norms, normb, st) == so
    x, z, steps = gpu_solve(hk, st, rx, rz)
    lastnorme, nb, norme, dsteps = hk.h.debug_dump(17)
    dev = deviation(x, z, xo, zo)
    print(f"[refinement branch {what}] steps {steps} (oracle {so}); |x - oracle| / max(1, |x|) {dev:.2e}; residual norms oracle "
          f"{', '.join(f'{v:.4e}' for v in norms)}; device state: before the last step {lastnorme:.4e}, after it {norme:.4e}")
    assert steps == so and dsteps == steps and nb == normb
    assert dev <= UNREFINED_GATE
    x0, z0, _ = _unrefined(hk, rx, rz)
    return dict(S=S, hk=hk, o=o, x=x, z=z, steps=steps, norms=norms, x0=x0, z0=z0, state=(lastnorme, nb, norme, dsteps), rx=rx, rz=rz)


def test_a_worse_candidate_is_rejected():
    """c = 4: the residual grows by 3.  One step, and the result is the unrefined solve bit for bit"""
    r = _branch_case(4.0, with_ir(), "c=4 defaults")
    assert r["steps"] == 1
    assert r["norms"][1] > 1.5 * r["norms"][0]
    assert np.array_equal(r["x"], r["x0"]) and np.array_equal(r["z"], r["z0"])
    lastnorme, _, norme, _ = r["state"]
    assert norme > lastnorme


def test_a_better_candidate_below_the_ratio_is_taken_and_the_loop_stops():
    """c = 0.5: the residual halves, below stop_ratio = 5.  One step, and the candidate is the result"""
    r = _branch_case(0.5, with_ir(), "c=0.5 defaults")
    assert r["steps"] == 1
    assert not np.array_equal(r["x"], r["x0"])
    assert deviation(r["x"], r["z"], r["x0"], r["z0"]) >= 1e-5       # (neighbouring iterates are far apart next to the gate)


def test_a_ratio_above_stop_ratio_continues():
    """c = 0.5 with stop_ratio = 1.25: the ratio 2 now continues, to the oracle's count.  (Not 1.5: the ratio 2 is only a factor 1.33 above
    it, and every deciding ratio is required to be a factor 1.5 away from stop_ratio; 1.25 is a factor 1.6 below the ratio.)"""
    r = _branch_case(0.5, with_ir(stop_ratio=1.25), "c=0.5 stop_ratio=1.25")
    assert r["steps"] > 1


@pytest.mark.parametrize("j", [2, 4])
def test_the_absolute_tolerance_stops_after_exactly_j_steps(j):
    """c = 0.875, reltol = 0, abstol = the geometric mean of the oracle's norms after steps j - 1 and j (a factor 8 apart)"""
    S, hk, o = _stale_pair(0.875)
    norms = _oracle_solve(o, with_ir(reltol=0.0), S.rx[0], S.rz[0])[3]
    assert len(norms) > j and norms[j - 1] >= 4.0 * norms[j]
    r = _branch_case(0.875, with_ir(reltol=0.0, abstol=float(np.sqrt(norms[j - 1] * norms[j]))), f"c=0.875 abstol after step {j}")
    assert r["steps"] == j


def test_a_tolerance_met_at_entry_takes_no_step():
    """c = 0.875, abstol above the first residual's norm: no step, the unrefined solve bit for bit -- the step inside the first graph is a
    no-op for an inactive state"""
    S, hk, o = _stale_pair(0.875)
    first = _oracle_solve(o, with_ir(reltol=0.0), S.rx[0], S.rz[0])[3][0]
    r = _branch_case(0.875, with_ir(reltol=0.0, abstol=4.0 * first), "c=0.875 abstol above the first norm")
    assert r["steps"] == 0
    assert np.array_equal(r["x"], r["x0"]) and np.array_equal(r["z"], r["z0"])


def test_max_iter_caps_the_loop():
    r = _branch_case(0.875, with_ir(max_iter=3), "c=0.875 max_iter=3")
    assert r["steps"] == 3


def test_a_zero_right_hand_side():
    """norme = normb = 0: no step, the result exactly zero, success"""
    S = system("plain", DEFAULT_REG)
    hk = S.handle()
    x, z, steps = gpu_solve(hk, with_ir(), np.zeros(S.n), np.zeros(S.m))
    assert steps == 0 and not np.any(x) and not np.any(z)
    lastnorme, normb, norme, dsteps = hk.h.debug_dump(17)
    assert (lastnorme, normb, norme, dsteps) == (0.0, 0.0, 0.0, 0.0)


@pytest.mark.parametrize("stop_ratio", [50.0, 5.0])
def test_natural_slow_convergence(stop_ratio):
    """no stale factor: static_regularization_constant = 1e-2 converges by about 20 per step.  stop_ratio = 50: improved, below the
    ratio -- one step, the candidate taken.  stop_ratio = 5: the oracle's count (8).  The right-hand side is scaled by 1/8 so that the
    norm that ends the second case (3.4e-13) is a factor 2 below abstol + reltol |b| = 1.05e-12 and the one before it a factor 2 above."""
    r = _branch_case(1.0, with_ir(1e-2, stop_ratio=stop_ratio), f"reg=1e-2 stop_ratio={stop_ratio:g}", reg=1e-2, rhs_scale=0.125)
    if stop_ratio == 50.0:
        assert r["steps"] == 1 and not np.array_equal(r["x"], r["x0"])
        assert deviation(r["x"], r["z"], r["x0"], r["z0"]) >= 1e-5
    else:
        assert r["steps"] == 8


def test_two_contexts_of_one_call_decide_independently():
    """solve_multi with a zero right-hand side on context 0 and one that needs four steps on context 1: counts [0, 4], each result
    the bits of its separate solve"""
    S, hk, o = _stale_pair(0.875)
    norms = _oracle_solve(o, with_ir(reltol=0.0), S.rx[0], S.rz[0])[3]
    st = with_ir(reltol=0.0, abstol=float(np.sqrt(norms[3] * norms[4])))
    _, _, so, norms = _oracle_solve(o, st, S.rx[0], S.rz[0])
    assert so == 4 and assert_decisive(norms, float(max(np.max(np.abs(S.rx[0])), np.max(np.abs(S.rz[0])))), st) == 4
    rx, rz = np.vstack([np.zeros(S.n), S.rx[0]]), np.vstack([np.zeros(S.m), S.rz[0]])
    lx, lz = np.zeros((2, S.n)), np.zeros((2, S.m))
    ok, steps = hk.h.solve_multi(rx, rz, lx, lz, **ir_kw(st))
    assert ok and list(steps) == [0, 4]
    assert not np.any(lx[0]) and not np.any(lz[0])
    x, z, s1 = gpu_solve(hk, st, rx[1], rz[1])
    assert s1 == 4 and np.array_equal(x, lx[1]) and np.array_equal(z, lz[1])
