"""The device step of the Exponential / Power cones (step_cone3.hip: combined_ds_shift, mul_Hs, step length, barrier of a cone set)
against the 50-digit reference of tests/cone3_reference.py, at the margins, lane counts, positions and loop lengths where its kernels
can go wrong.  Granular calls (cone_combined_ds_shift, cone_step_length, cone_barrier, cone_mul_hs) plus one fused
hipkkt_step_barrier_dev.  The scaling comes from kktsolver_update_scaled; the reference takes the RESIDENT 15 doubles per cone
[pack_triu(Hs) | pack_triu(H_dual) | grad] and the resident (s, z) as exact inputs, so the scaling's error is not charged to the step.

Gates:
  * correction and barrier by regime: the device's error against the 50-digit evaluation of the reference's expressions, per bucket
    (operation, cone kind, side, margin decade), <= 10 x cone3_reference.HOST_ERR[bucket], the measured error of the float64 stand-in
    on the SAME points: the device evaluates the same expressions in the same association (-ffp-contract=off), only log / pow / exp
    differ from the host's.  Every cone is held; the largest error / allowance per bucket is printed.  A sample of at most 16 cones
    per case is also held against the definition 1/2 grad^3 f*(z)[u, v].
    The barrier of a cone SET is all the library returns, so the barrier of one cone is taken from a handle that holds that cone
    alone (one handle for the Exponential cone, one per alpha), scaled at the very point; the 128-cone sets check the sum.
  * lane counts: per cone, shift within 10 x HOST_ERR[correction, central] of max |eta| plus the two roundings of grad sigma_mu - eta;
    mul_Hs bit-identical to the row sums in the reference's association; the barrier term of cone c from the difference of two
    candidates along a direction that moves cone c only, within 2 x 1e-10 max(1, sum |terms|) (the project's barrier gate, twice).
  * step lengths of the constructed directions: `==` alpha0 step^k formed by repeated multiplication (or 0); nothing is excluded --
    the accepted and the last rejected point of the binding cone, and every other cone at alpha0, have a relative margin of at least
    1e-3 at 50 digits (asserted).
  * barrier loops: 1e-10 max(1, sum |terms|) and 1e-13 sum |terms| for the shifted dot (the gates of test_gpu_device_step_nonsym.py)
    against 50-digit sums.

The trip count: the kernels bound the backtracking loop by ceil(log alpha_min / log step) + 2 trips.  Grid point k is tested in trip k,
and the deepest admissible k is at most floor(log(alpha_min / alpha0) / log step) <= ceil(log alpha_min / log step) - 1 + 1, so the
bound has a slack of two trips: lowering it by one or two changes no result, lowering it by three loses the deepest grid point, which
test_trip_count_reaches_the_deepest_grid_point expects exactly."""
import math

import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import problems
from clarabel_jl_amd.kktsolver import HipKKTSolver
from julia_standin.cones import NonnegativeCone, SecondOrderCone, ZeroCone
from tests import cone3_reference as c3
from tests.step_support import NONSYM, PARITY, SQRT_EPS, SUM_TOL, _is3, _prep, _problem, _Timeout

pytestmark = pytest.mark.gpu

mp, mpf = c3.mp, c3.mpf
EPS64 = float(np.finfo(np.float64).eps)
ALPHA0 = 1.0 - SQRT_EPS
MARGIN = 1e-3


# ---- handles ----------------------------------------------------------------------------------------------------------------------------

def _handle(specs, seed=31, step=None, amin=None):
    Pt, A, cones = _prep(_problem(specs, seed))
    m, n = A.shape
    st = cl.Settings(**NONSYM)
    cones.use_settings(st)
    hk = HipKKTSolver(Pt, A, cones, m, n, st)
    assert hk.steps_on_device and hk.steps_nonsymmetric
    if step is not None:
        hk.h.step_enable_cone3(True, step, amin)
    return hk, cones, st


def _scale(hk, cones, s, z, strategy="primal_dual"):
    """kktsolver_update_scaled at (s, z); -> the resident 15 doubles of every three-row cone, in cone order"""
    mu = float(s @ z) / (cones.degree + 1)
    assert mu > 0 and hk.kktsolver_update_scaled(cones, s, z, mu=mu, strategy=strategy), "the device's update_scaling failed"
    slots = np.asarray(hk.scaling_nonsym).reshape(-1, 15)
    assert len(slots) == sum(_is3(c) for c in cones.cones)
    return slots, mu


def _kind(c):
    return "exp" if isinstance(c, cl.cones_nonsym.ExponentialCone) else "pow"


def _cones3(cones):
    """(kind, alpha, rows) of every three-row cone, in cone order"""
    return [(_kind(c), getattr(c, "alpha", 0.0), r) for c, r in zip(cones.cones, cones.rng_cones) if _is3(c)]


def _central_points(cones, rng):
    """(s, z): three-row cones at cone3_reference.central_point, Nonnegative rows in (0.2, 1.2), second-order cones 0.5 .. 1.5 inside"""
    m = cones.numel
    s, z = np.zeros(m), np.zeros(m)
    for c, r in zip(cones.cones, cones.rng_cones):
        if _is3(c):
            kind, a = _kind(c), getattr(c, "alpha", 0.0)
            z[r], s[r] = c3.central_point(kind, a, True, rng), c3.central_point(kind, a, False, rng)
        elif isinstance(c, SecondOrderCone):
            for v in (s, z):
                t = rng.standard_normal(c.dim)
                t[0] = np.linalg.norm(t[1:]) + 0.5 + rng.random()
                v[r] = t
        elif isinstance(c, NonnegativeCone):
            s[r], z[r] = rng.random(c.numel) + 0.2, rng.random(c.numel) + 0.2
        else:
            assert isinstance(c, ZeroCone)
    return s, z


# ---- 50-digit barrier terms of a whole cone set ---------------------------------------------------------------------------------------------

def _set_terms(cones, z, s):
    """the barrier term of every cone at the float64 point (z, s), at 50 digits (Zero cones contribute nothing)"""
    terms = []
    for c, r in zip(cones.cones, cones.rng_cones):
        if _is3(c):
            terms.append(c3.ref_barrier(_kind(c), z[r], s[r], getattr(c, "alpha", 0.0)))
        elif isinstance(c, NonnegativeCone):      # coneops_nncone.jl: -sum log(s_i z_i)
            terms.append(-mp.fsum(mp.log(mpf(float(a)) * mpf(float(b))) for a, b in zip(s[r], z[r])))
        elif isinstance(c, SecondOrderCone):      # coneops_socone.jl:288-305: -log(res_s res_z) / 2
            res = []
            for q in (s[r], z[r]):
                q = c3.V(q)
                res.append(q[0] ** 2 - mp.fdot(q[1:], q[1:]))
            assert res[0] > 0 and res[1] > 0
            terms.append(-mp.log(res[0] * res[1]) / 2)
    return terms


def _check_set_barrier(bars, dots, cones, z, s, dz, ds, alphas, what):
    worst_b = worst_d = 0.0
    for a, b, d in zip(alphas, bars, dots):
        zz, ss = z + a * dz, s + a * ds      # (two roundings per entry, as the kernels form the point)
        terms = _set_terms(cones, zz, ss)
        rb, tb = mp.fsum(terms), mp.fsum(abs(t) for t in terms)
        am = mpf(float(a))
        prods = [(p + am * dp) * (q + am * dq) for p, dp, q, dq in zip(c3.V(z), c3.V(dz), c3.V(s), c3.V(ds))]
        rd, td = mp.fsum(prods), mp.fsum(abs(t) for t in prods)
        eb, ed = float(abs(mpf(float(b)) - rb) / max(mpf(1), tb)), float(abs(mpf(float(d)) - rd) / td)
        worst_b, worst_d = max(worst_b, eb), max(worst_d, ed)
        assert eb <= PARITY, (what, a, b, float(rb))
        assert ed <= SUM_TOL, (what, a, d, float(rd))
    print(f"[cone3 edges barrier {what}] max |barrier - 50 digits| / max(1, sum |terms|) = {worst_b:.2e}, max |dot - 50 digits| / sum |terms| = {worst_d:.2e}")


def _raw_barrier(hk, dz, ds, alphas):
    """hipkkt_cone_barrier into a 16-long output filled with a sentinel -> (barrier, dot); the slots past 2 nalpha must stay untouched"""
    a = np.ascontiguousarray(alphas, dtype=np.float64)
    out = np.full(16, -777.25)
    rc = hk.h.L.hipkkt_cone_barrier(hk.h.h, np.ascontiguousarray(dz), np.ascontiguousarray(ds), a, a.size, out)
    assert rc == 0
    assert np.all(out[2 * a.size:] == -777.25), out
    return out[0:2 * a.size:2].copy(), out[1:2 * a.size:2].copy()


# ---- 1. correction and barrier by regime ----------------------------------------------------------------------------------------------------

SETS = [(d, "dual") for d in c3.DECADES] + [(d, "primal") for d in c3.DECADES if d != "central"]
DEF_SAMPLE = {"exp": 2, "pow": 3}      # cones per scale that are also held against the third derivative: 15 per case


@pytest.fixture(scope="module")
def single_cone_handles():
    """one handle per cone kind and alpha, each holding that one cone"""
    out = {("exp", 0.0): _handle([cl.ExponentialConeT()], 41)}
    for a in c3.ALPHAS:
        out[("pow", a)] = _handle([cl.PowerConeT(a)], 42)
    return out


def _gate(worst, what):
    for b in sorted(worst, key=str):
        err, allow = worst[b], 10.0 * c3.HOST_ERR[b]
        print(f"[cone3 edges regime {what}] {b}: max device error {err:.2e}, allowance {allow:.2e}, error / allowance {err / allow:.3f}")
    for b, err in worst.items():
        assert err <= 10.0 * c3.HOST_ERR[b], (b, err, c3.HOST_ERR[b])


@pytest.mark.parametrize("decade,side", SETS)
def test_correction_and_barrier_by_regime(decade, side, single_cone_handles):
    with _Timeout(120):
        worst, layers = {}, 0.0
        kinds, alphas, _, _ = c3.regime_set(decade, side, 1.0)
        hk, cones, st = _handle(c3.regime_specs(kinds, alphas), 32)
        for j, scale in enumerate(c3.SCALES):
            kinds, alphas, s, z = c3.regime_set(decade, side, scale)
            slots, mu = _scale(hk, cones, s, z, ("primal_dual", "dual")[j % 2])
            m = cones.numel
            if side == "dual":
                dz, ds = c3.regime_directions(decade, side, scale, m)
                shift = hk.cone_combined_ds_shift(dz, ds, 0.0)      # sigma mu = 0: the shift is -eta (the grad term: the lane-count test)
                seen = {"exp": 0, "pow": 0}
                for k, (kind, a) in enumerate(zip(kinds, alphas)):
                    r = slice(3 * k, 3 * k + 3)
                    ref, u = c3.ref_correction(kind, slots[k, 6:12], z[r], a, ds[r], dz[r])
                    b = c3.bucket("correction", kind, "dual", decade)
                    worst[b] = max(worst.get(b, 0.0), c3.correction_error(-shift[r], ref))
                    if seen[kind] < DEF_SAMPLE[kind]:
                        seen[kind] += 1
                        true = c3.def_correction(kind, z[r], a, u, dz[r])
                        layers = max(layers, max(float(abs(p - q)) for p, q in zip(ref, true)) / c3.max_abs(true))
                        e = c3.correction_error(-shift[r], true)
                        assert e <= 10.0 * c3.HOST_ERR[b] + 1e-30, (kind, a, decade, scale, e)
            # the set's barrier and shifted dot at the point itself and at seven short steps from it
            dzb, dsb = c3.regime_directions(decade, side, scale, m)
            # (the Power point with s3 = 0 keeps it: the branch |s3| <= eps of gradient_primal is absolute, and a step to |s3| ~ 1e-15 next
            # to s1, s2 ~ 1e-6 leaves it for a Newton start -1 / s3 + ... that cancels to NaN in float64, in the reference as here)
            dsb[s == 0.0] = 0.0
            f = 1e-3 * (1.0 if decade == "central" else decade)
            alphas8 = [0.0] + [0.9 * 0.8 ** k for k in range(7)]
            bars, dots = hk.cone_barrier(f * dzb, f * dsb, alphas8)
            _check_set_barrier(bars[:2], dots[:2], cones, z, s, f * dzb, f * dsb, alphas8[:2], f"{decade} {side} {scale:g}")
            assert np.all(np.isfinite(bars)) and np.all(np.isfinite(dots))
            # the barrier of every cone alone
            for k, (kind, a) in enumerate(zip(kinds, alphas)):
                r = slice(3 * k, 3 * k + 3)
                h1, c1, _ = single_cone_handles[(kind, a)]
                _scale(h1, c1, s[r], z[r], ("primal_dual", "dual")[j % 2])
                got, dot = h1.cone_barrier(np.zeros(3), np.zeros(3), [0.0])
                b = c3.bucket("barrier", kind, side, decade)
                worst[b] = max(worst.get(b, 0.0), c3.barrier_error(got[0], c3.ref_barrier(kind, z[r], s[r], a)))
                assert abs(dot[0] - float(z[r] @ s[r])) <= SUM_TOL * float(np.abs(z[r]) @ np.abs(s[r]))
        if side == "dual":
            print(f"[cone3 edges regime {decade} {side}] reference expressions against 1/2 grad^3 f*[u, v] on the sample: {layers:.2e}")
            assert layers <= 1e-30
        _gate(worst, f"{decade} {side}")


# ---- 2. lane counts ---------------------------------------------------------------------------------------------------------------------------

LANE_COUNTS = [(1, 0), (0, 1), (255, 0), (256, 0), (257, 0), (0, 256), (0, 257), (513, 1), (1, 513), (256, 256)]


def _lane_specs(nexp, npow):
    """Exponential and Power cones interleaved as far as both last, so that a table position is not the cone's index"""
    specs, e, p = [], 0, 0
    while e < nexp or p < npow:
        if e < nexp:
            specs.append(cl.ExponentialConeT())
            e += 1
        if p < npow:
            specs.append(cl.PowerConeT(c3.ALPHAS[p % len(c3.ALPHAS)]))
            p += 1
    return specs


@pytest.mark.parametrize("nexp,npow", LANE_COUNTS)
def test_every_lane_is_covered(nexp, npow):
    with _Timeout(120):
        hk, cones, st = _handle(_lane_specs(nexp, npow), 33)
        rng = np.random.default_rng(100 * nexp + npow)
        s, z = _central_points(cones, rng)
        slots, mu = _scale(hk, cones, s, z)
        K0 = hk.h.debug_dump(4)
        m = cones.numel
        c3s = _cones3(cones)
        assert len(c3s) == nexp + npow and m == 3 * (nexp + npow)
        dz, ds, x, sm = rng.standard_normal(m), rng.standard_normal(m), rng.standard_normal(m), 0.3 * mu
        shift, hs = hk.cone_combined_ds_shift(dz, ds, sm), hk.cone_mul_hs(x)
        base_b, base_d = hk.cone_barrier(np.zeros(m), np.zeros(m), [0.0])
        worst = {"exp": 0.0, "pow": 0.0}
        worst_bar = 0.0
        total = mp.fsum(abs(t) for t in _set_terms(cones, z, s))
        for k, (kind, a, r) in enumerate(c3s):
            # combined_ds_shift = grad sigma_mu - eta
            eta, _ = c3.ref_correction(kind, slots[k, 6:12], z[r], a, ds[r], dz[r])
            ref = [g * mpf(sm) - e for g, e in zip(c3.V(slots[k, 12:15]), eta)]
            allow = 10.0 * c3.HOST_ERR[c3.bucket("correction", kind, "dual", "central")] * c3.max_abs(eta) + \
                2.0 * EPS64 * (float(np.max(np.abs(slots[k, 12:15]))) * sm + c3.max_abs(eta))
            e = c3.max_err(shift[r], ref)
            worst[kind] = max(worst[kind], e / allow)
            assert e <= allow, (kind, k, e, allow)
            # mul_Hs: the row sums in the reference's association, bit for bit
            H = slots[k, 0:6]
            Hf = [[H[0], H[1], H[3]], [H[1], H[2], H[4]], [H[3], H[4], H[5]]]
            want = [Hf[i][0] * x[r][0] + Hf[i][1] * x[r][1] + Hf[i][2] * x[r][2] for i in range(3)]
            assert list(hs[r]) == want, (kind, k)
            assert c3.max_err(hs[r], c3.ref_mul_hs(slots[k], x[r])) <= 3.0 * EPS64 * float(np.max(np.abs(np.array(Hf)) @ np.abs(x[r]))), (kind, k)
            # the barrier term of this cone: two candidates along a direction that moves this cone only
            d_z, d_s = np.zeros(m), np.zeros(m)
            # (0.1 of the point itself, along which either barrier falls by 3 log 1.1, plus a perturbation: the difference is never small)
            d_z[r] = 0.1 * z[r] + 0.03 * c3.margin(kind, z[r], a, True) * np.abs(z[r]) * rng.standard_normal(3)
            d_s[r] = 0.1 * s[r] + 0.03 * c3.margin(kind, s[r], a, False) * np.abs(s[r]) * rng.standard_normal(3)
            assert c3.inside(kind, z[r] + 1.0 * d_z[r], a, True) and c3.inside(kind, s[r] + 1.0 * d_s[r], a, False), (kind, k)
            bars, dots = hk.cone_barrier(d_z, d_s, [0.0, 1.0])
            assert bars[0] == base_b[0] and dots[0] == base_d[0]
            want = c3.ref_barrier(kind, z[r] + 1.0 * d_z[r], s[r] + 1.0 * d_s[r], a) - c3.ref_barrier(kind, z[r], s[r], a)
            e = float(abs(mpf(float(bars[1])) - mpf(float(bars[0])) - want))
            worst_bar = max(worst_bar, e / float(max(mpf(1), total)))
            assert abs(want) >= 0.1, (kind, k, float(want))      # (the difference is far above the gate: a lane left out would show)
            assert e <= 2.0 * PARITY * float(max(mpf(1), total)), (kind, k, e, float(want))
        print(f"[cone3 edges lanes {nexp} + {npow}] shift: max error / allowance Exponential {worst['exp']:.3f}, Power {worst['pow']:.3f}; barrier "
              f"term of one cone from two candidates: max error / max(1, sum |terms|) {worst_bar:.2e}")
        assert np.array_equal(hk.h.debug_dump(4), K0)


# ---- 3. the binding cone by position, 4. the trip count -----------------------------------------------------------------------------------------

def _short_directions(cones, s, z, rng):
    m = cones.numel
    return 1e-3 * np.abs(z) * rng.standard_normal(m), 1e-3 * np.abs(s) * rng.standard_normal(m)


def _assert_margins(c3s, q, dq, alpha, dual, at_least=MARGIN):
    for kind, a, r in c3s:
        mg = c3.margin(kind, q[r] + alpha * dq[r], a, dual)
        assert mg is not None and mg >= at_least, (kind, a, dual, mg)


def _bind(c3s, k, q, dq, dual, cross):
    """dq with cone k's rows replaced by the direction that crosses the boundary at `cross`"""
    kind, a, r = c3s[k]
    out = dq.copy()
    out[r] = c3.boundary_direction(kind, q[r], a, dual, cross)
    return out


def _decision_margins(c3s, k, q, dq, dual, accepted, rejected):
    """the accepted point is inside and the last rejected one outside, both by a relative margin of at least 1e-3 at 50 digits"""
    kind, a, r = c3s[k]
    if accepted is not None:
        mg = c3.margin(kind, q[r] + accepted * dq[r], a, dual)
        assert mg is not None and mg >= MARGIN, (kind, a, dual, accepted, mg)
    if rejected is not None:
        mg = c3.margin(kind, q[r] + rejected * dq[r], a, dual)
        assert mg is not None and mg <= -MARGIN, (kind, a, dual, rejected, mg)      # (no sign condition decides: the expression itself)


@pytest.mark.parametrize("dual", [True, False], ids=["dual side", "primal side"])
def test_binding_cone_at_every_position(dual):
    """300 Exponential and 300 Power cones, interleaved; every direction is short, so alpha0 = 1 - sqrt(eps) is accepted, except for one
    cone whose direction crosses the boundary midway (geometrically) between the grid points k - 1 and k, for k = 1 and 7, at the table
    positions 0, 63, 64, 255, 256 and 299 of either table: first and last lane of a wavefront, of a workgroup, the partial workgroup."""
    with _Timeout(120):
        n3 = 300
        hk, cones, st = _handle(_lane_specs(n3, n3), 34)
        rng = np.random.default_rng(7 + int(dual))
        s, z = _central_points(cones, rng)
        _scale(hk, cones, s, z)
        K0 = hk.h.debug_dump(4)
        c3s = _cones3(cones)
        dz, ds = _short_directions(cones, s, z, rng)
        _assert_margins(c3s, z, dz, ALPHA0, True)
        _assert_margins(c3s, s, ds, ALPHA0, False)
        assert hk.cone_step_length(dz, ds, 1.0) == (ALPHA0, ALPHA0)
        step = st.linesearch_backtrack_step
        q, dq = (z, dz) if dual else (s, ds)
        for kind in c3.KINDS:
            table = [i for i, t in enumerate(c3s) if t[0] == kind]
            assert len(table) == n3
            for pos in (0, 63, 64, 255, 256, n3 - 1):
                for k in (1, 7):
                    bound = _bind(c3s, table[pos], q, dq, dual, c3.crossing_between(ALPHA0, step, k))
                    want = c3.grid_alpha(ALPHA0, step, k)
                    _decision_margins(c3s, table[pos], q, bound, dual, want, c3.grid_alpha(ALPHA0, step, k - 1))
                    got = hk.cone_step_length(bound, ds, 1.0) if dual else hk.cone_step_length(dz, bound, 1.0)
                    assert got == (want, want), (kind, pos, k, got, want)
        assert np.array_equal(hk.h.debug_dump(4), K0)


def _deepest(step, amin):
    """the largest k with alpha0 step^k >= alpha_min, as backtrack_search walks the grid"""
    a, k = ALPHA0, 0
    while True:
        nxt = a * step
        if nxt < amin:
            return k
        a, k = nxt, k + 1


@pytest.mark.parametrize("step,amin", [(0.8, 1e-4), (0.5, 1e-3)])
def test_trip_count_reaches_the_deepest_grid_point(step, amin):
    """a direction that is accepted at the deepest grid point that is still >= alpha_min gives exactly that point; one that first becomes
    feasible one grid point later gives 0 -- for either cone, on either side, in the last lane of a wavefront"""
    with _Timeout(120):
        hk, cones, st = _handle(_lane_specs(64, 64), 35, step, amin)
        rng = np.random.default_rng(9)
        s, z = _central_points(cones, rng)
        _scale(hk, cones, s, z)
        c3s = _cones3(cones)
        dz, ds = _short_directions(cones, s, z, rng)
        _assert_margins(c3s, z, dz, ALPHA0, True)
        _assert_margins(c3s, s, ds, ALPHA0, False)
        K = _deepest(step, amin)
        assert K == {(0.8, 1e-4): 41, (0.5, 1e-3): 9}[(step, amin)]
        deepest = c3.grid_alpha(ALPHA0, step, K)
        assert deepest >= amin > deepest * step
        print(f"[cone3 edges trips ({step}, {amin})] deepest grid point k = {K}: {deepest!r}; the library's bound is "
              f"{math.ceil(math.log(amin) / math.log(step)) + 2} trips")
        for kind in c3.KINDS:
            k3 = [i for i, t in enumerate(c3s) if t[0] == kind][63]
            for dual, q, dq in ((True, z, dz), (False, s, ds)):
                # accepted at grid point K
                bound = _bind(c3s, k3, q, dq, dual, c3.crossing_between(ALPHA0, step, K))
                _decision_margins(c3s, k3, q, bound, dual, deepest, c3.grid_alpha(ALPHA0, step, K - 1))
                got = hk.cone_step_length(bound, ds, 1.0) if dual else hk.cone_step_length(dz, bound, 1.0)
                assert got == (deepest, deepest), (kind, dual, got, deepest)
                # feasible only from grid point K + 1 on, which is below alpha_min: 0
                bound = _bind(c3s, k3, q, dq, dual, c3.crossing_between(ALPHA0, step, K + 1))
                _decision_margins(c3s, k3, q, bound, dual, None, deepest)
                got = hk.cone_step_length(bound, ds, 1.0) if dual else hk.cone_step_length(dz, bound, 1.0)
                assert got == (0.0, 0.0), (kind, dual, got)


# ---- 5. barrier loops -----------------------------------------------------------------------------------------------------------------------------

LOOP_SETS = {
    # k_bar_rows covers 64 x 256 = 16384 rows per pass: the Nonnegative rows take a second one
    "rows wrap": lambda: [cl.NonnegativeConeT(16385 + 300), cl.ExponentialConeT(), cl.PowerConeT(0.3)],
    # k_bar_soc strides one cone by 256
    "long second-order cones": lambda: [cl.ExponentialConeT(), cl.SecondOrderConeT(2), cl.SecondOrderConeT(255), cl.PowerConeT(0.7),
                                        cl.SecondOrderConeT(256), cl.SecondOrderConeT(257), cl.ExponentialConeT(), cl.SecondOrderConeT(513),
                                        cl.SecondOrderConeT(1025), cl.PowerConeT(0.101)],
    # k_bar_final strides the second-order cones and the three-row cones by 256
    "257 + 257 cones": lambda: [t for k in range(257) for t in (cl.SecondOrderConeT(3), cl.ExponentialConeT() if k % 2 == 0 else
                                                                   cl.PowerConeT(c3.ALPHAS[k % len(c3.ALPHAS)]))],
}


@pytest.mark.parametrize("name", list(LOOP_SETS))
def test_barrier_loops_that_wrap(name):
    with _Timeout(120):
        hk, cones, st = _handle(LOOP_SETS[name](), 36)
        rng = np.random.default_rng(11)
        s, z = _central_points(cones, rng)
        _scale(hk, cones, s, z)
        K0 = hk.h.debug_dump(4)
        m = cones.numel
        dz, ds = 0.05 * np.abs(z) * rng.standard_normal(m), 0.05 * np.abs(s) * rng.standard_normal(m)
        for c, r in zip(cones.cones, cones.rng_cones):
            if isinstance(c, SecondOrderCone):      # (a short step of the whole cone: scale by its distance to the boundary)
                for q, dq in ((z, dz), (s, ds)):
                    dq[r] = 0.05 * (q[r][0] - np.linalg.norm(q[r][1:])) * rng.standard_normal(c.dim) / math.sqrt(c.dim)
        alphas = [0.9 * 0.8 ** k for k in range(8)]
        bars, dots = _raw_barrier(hk, dz, ds, alphas)
        # candidates 0, 3 and 7 against 50 digits (the last row block, the last pass of every loop serve every candidate alike)
        pick = [0, 3, 7]
        _check_set_barrier(bars[pick], dots[pick], cones, z, s, dz, ds, [alphas[j] for j in pick], name)
        # 7 and 1 candidates: the same numbers, the other output slots untouched
        bars7, dots7 = _raw_barrier(hk, dz, ds, alphas[:7])
        assert np.array_equal(bars7, bars[:7]) and np.array_equal(dots7, dots[:7])
        bars1, dots1 = _raw_barrier(hk, dz, ds, alphas[7:8])
        assert bars1[0] == bars[7] and dots1[0] == dots[7]
        assert np.array_equal(hk.h.debug_dump(4), K0)


# ---- 6. a candidate outside the cone ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dual", [True, False], ids=["dual side", "primal side"])
def test_candidate_outside_one_cone(dual):
    """70 + 70 cones; one lane's direction crosses its cone's boundary at alpha = 0.5 (finite inputs, an ordinary step that is too long):
    the candidates 0.6 and 1.0 must come back non-finite or above 1e300, the candidates 0.2 and 0.4 as if the others had not been asked.
    The Exponential cone's primal barrier flags a point only where its Wright-omega argument is negative (between 0 and 1 the omega
    algorithm returns a value for a point outside the cone, in the reference as here), so on that side the far candidate is 3.0 and the
    candidate 0.6 is held to the 50-digit value of the reference's expression instead."""
    with _Timeout(120):
        hk, cones, st = _handle(_lane_specs(70, 70), 37)
        rng = np.random.default_rng(13 + int(dual))
        s, z = _central_points(cones, rng)
        _scale(hk, cones, s, z)
        c3s = _cones3(cones)
        m = cones.numel
        dz, ds = _short_directions(cones, s, z, rng)
        q, dq = (z, dz) if dual else (s, ds)
        for kind in c3.KINDS:
            table = [i for i, t in enumerate(c3s) if t[0] == kind]
            for pos in (0, 69):
                far = 3.0 if (kind == "exp" and not dual) else 1.0
                k3 = table[pos]
                bound = _bind(c3s, k3, q, dq, dual, 0.5)
                _decision_margins(c3s, k3, q, bound, dual, 0.4, 0.6)
                kd, a, r = c3s[k3]
                if kind == "exp" and not dual:
                    assert c3.exp_omega_argument(q[r] + far * bound[r]) < 0
                args = (bound, ds) if dual else (dz, bound)
                # every other cone stays inside up to `far`
                others = [t for i, t in enumerate(c3s) if i != k3]
                _assert_margins(others, z, dz, far, True)
                _assert_margins(others, s, ds, far, False)
                bars, dots = hk.cone_barrier(*args, [0.2, 0.6, 0.4, far])
                inside_b, inside_d = hk.cone_barrier(*args, [0.2, 0.4])
                assert bars[0] == inside_b[0] and bars[2] == inside_b[1] and dots[0] == inside_d[0] and dots[2] == inside_d[1]
                assert np.all(np.isfinite(inside_b)) and np.all(np.abs(inside_b) < 1e300)
                _check_set_barrier(inside_b, inside_d, cones, z, s, *args, [0.2, 0.4], f"outside {kind} {pos}")
                outside = [bars[3]] if (kind == "exp" and not dual) else [bars[1], bars[3]]
                if kind == "exp" and not dual:
                    # 0.6 is outside the cone with an omega argument in (0, 1): the reference's expression has a value there, and the
                    # device must return that value
                    assert 0 < c3.exp_omega_argument(q[r] + 0.6 * bound[r]) < 1
                    _check_set_barrier(bars[1:2], dots[1:2], cones, z, s, *args, [0.6], f"outside {kind} {pos}, omega argument in (0, 1)")
                assert all((not np.isfinite(b)) or b > 1e300 for b in outside), (kind, pos, bars)
                assert np.all(np.isfinite(dots))
        assert np.array_equal(hk.cone_affine_ds(), s)      # the handle still serves


# ---- 7. the fused barrier returns the granular numbers ------------------------------------------------------------------------------------------------

def test_fused_barrier_returns_the_granular_numbers():
    """hipkkt_step_barrier_dev on the resident iterate and the resident step of a fused affine step, on a set whose three-row cones take a
    second pass of k_bar_final: the numbers of hipkkt_cone_barrier for the same step (which the tests above hold to 50 digits)"""
    with _Timeout(120):
        prob = problems.nonsymmetric_mix(n=20, nexp=130, npow=130, ngenpow=0, nn=6, nzero=2, socdim=4, seed=9)
        S = cl.Solver(*prob, cl.Settings(**NONSYM))
        assert S._device_step
        ks, data, cones, v = S.kktsystem.kktsolver, S.data, S.cones, S.variables
        n, m = data.n, data.m
        rng = np.random.default_rng(15)
        s, z = _central_points(cones, rng)
        v.x[:], v.z[:], v.s[:], v.tau, v.kappa = rng.standard_normal(n), z, s, 0.9, 0.4
        xzs, res = ks.device_buffer(n + 2 * m), ks.device_buffer(3 * n + 2 * m)
        xzs.upload(np.concatenate([v.x, v.z, v.s]))
        ks.residuals_update_dev(xzs, res, v.tau, v.kappa)
        S._residuals_update()
        mu = (S.residuals.dot_sz + v.tau * v.kappa) / (cones.degree + 1)
        assert ks.kktsolver_update_scaled(cones, v.s, v.z, mu=mu, strategy="primal_dual")
        ok, alpha, dtau, dkappa = ks.kktsolver_step_affine(xzs, res, v.tau, v.kappa, S.residuals.rtau, True)
        assert ok
        step = ks.h.step_get()
        dz, ds = step[n:n + m], step[n + m:]
        for alphas in ([alpha * 0.99 * 0.8 ** k for k in range(8)], [alpha * 0.5], [alpha * 0.99 * 0.8 ** k for k in range(7)]):
            fused_b, fused_d = ks.kktsolver_step_barrier(xzs, alphas)
            gran_b, gran_d = ks.cone_barrier(dz, ds, alphas)
            assert np.array_equal(fused_b, gran_b) and np.array_equal(fused_d, gran_d), (alphas, fused_b, gran_b)
            assert np.all(np.isfinite(fused_b))
        _check_set_barrier(gran_b[:1], gran_d[:1], cones, v.z, v.s, dz, ds, alphas[:1], "fused affine step")
        xzs.close()
        res.close()
