"""SURVEY section 8(f) row N1 for the NON-SYMMETRIC cones: update_scaling! + get_Hs! + _csc_update_sparsecone of Exponential, Power and
Generalized Power cones formed on the device from (s, z, mu, strategy) (include/hipkkt.h hipkkt_set_cone_types_ex /
hipkkt_update_scaling_ex[_dev], csrc/scaling.hip k_scaling_cone3 / k_scaling_genpow).

The comparison side is always the stand-in's host cone algebra (julia_standin/cones_nonsym.py, held to finite differences, conjugacy
and the secant equations by tests/test_nonsymmetric_cones.py), never a second run of the device code.  The bound on a block is the
project's parity gate, 1e-10 in the relative Frobenius norm.  On late IPM iterates the reference's own formulas are ill-conditioned (a
1-ulp change of (s, z) moves a block by up to percents): there a block is held to the gate only where the stand-in itself is stable
(its spread over 8 random +-1-ulp perturbations of (s, z) is <= 1e-12), see test_shadow_run_on_ipm_iterates."""
import json
import math
import os
import zlib

import numpy as np
import pytest
import scipy.sparse as sp

import clarabel_jl_amd  # noqa: F401  (registers the dotted package directory)
import julia_standin as cl
from clarabel_jl_amd import hipkkt, problems
from clarabel_jl_amd.kktsolver import HipKKTSolver
from julia_standin.cones_nonsym import ExponentialCone, GenPowerCone, PowerCone, _chol3_factor
from tests import fixtures as fx

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SQRT_EPS = math.sqrt(float(np.finfo(np.float64).eps))
GATE = 1e-10


@pytest.fixture(autouse=True)
def _front_batches_on_small_fronts(monkeypatch):
    if os.environ.get("HIPKKT_TEST_PRODUCTION", "0") != "1":   # (the production library has no switches: its own threshold applies)
        monkeypatch.setenv("HIPKKT_FRONT_BLOCK_MIN_ROWS", "0")      # as in tests/test_gpu_nonsymmetric.py


def _exp_pow_only():
    return problems.nonsymmetric_mix(n=80, nexp=30, npow=20, ngenpow=0, nn=20, nzero=3, socdim=5, seed=5)


PROBLEMS = {
    "exp_fixture": fx.basic_exp,
    "pow_fixture": fx.basic_pow,
    "genpow_fixture": fx.basic_genpow,
    "mix_60": lambda: problems.nonsymmetric_mix(n=60, nexp=8, npow=6, ngenpow=3, nn=20, nzero=3, socdim=5, seed=3),
    "mix_300": lambda: problems.nonsymmetric_mix(),
    "mix_1000": lambda: problems.nonsymmetric_mix(n=1000, nexp=300, npow=200, ngenpow=40, nn=400, nzero=30, socdim=12, seed=11),
    "exp_pow_only": _exp_pow_only,
}
STRATEGY = {"primal_dual": 0, "dual": 1}


def _cones_of(specs):
    cones = cl.CompositeCone(cl.cones_new_collapsed(specs))
    cones.use_settings(cl.Settings())
    return cones


def _prep(prob):
    P, q, A, b, specs = prob
    Pt = sp.triu(sp.csc_matrix(P), format="csc")
    Pt.sort_indices()
    A = sp.csc_matrix(A)
    A.sort_indices()
    return Pt, A, specs


def _triu(M):      # pack_triu, mathutils.jl:402-412
    return np.array([M[0, 0], M[0, 1], M[1, 1], M[0, 2], M[1, 2], M[2, 2]])


def _full(t):
    return np.array([[t[0], t[1], t[3]], [t[1], t[2], t[4]], [t[3], t[4], t[5]]])


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _is3(c):
    return isinstance(c, (ExponentialCone, PowerCone))


def _nonsym(c):
    return _is3(c) or isinstance(c, GenPowerCone)


def _de1(c, s, z):
    """de1 of use_primal_dual_scaling (coneops_nonsymmetric_common.jl:108) at (s, z), with the cone's own host functions"""
    k = PowerCone(c.alpha) if isinstance(c, PowerCone) else ExponentialCone()
    k.update_dual_grad_H(z)
    zt = k.gradient_primal(s)
    mu = float(z[0] * s[0] + z[1] * s[1] + z[2] * s[2]) / 3
    mut = float(zt[0] * k.grad[0] + zt[1] * k.grad[1] + zt[2] * k.grad[2]) / 3
    return mu * mut - 1


def _near_branch(de1):
    return SQRT_EPS / 4.0 <= abs(de1) <= 4.0 * SQRT_EPS


def _host_slot(c):
    """what the cone's slot of the output vector holds, from the host cone: a list of (name, values)"""
    if _is3(c):
        return [("Hs", _triu(c.Hs)), ("H_dual", _triu(c.H_dual)), ("grad", c.grad.copy())]
    return [("grad", c.grad.copy()), ("d1", c.d1.copy()), ("d2", np.array([c.d2])), ("p", c.p.copy()), ("q", c.q.copy()), ("r", c.r.copy())]


def _split_slot(c, slot):
    out, o = [], 0
    for name, v in _host_slot(c):
        out.append((name, slot[o:o + len(v)]))
        o += len(v)
    assert o == len(slot) == c.scaling_slot_len
    return out


def _k_index_sets(h, cones):
    """per non-symmetric cone: the indices of its entries of K (Hs block; GenPower: + q, r, p columns and the three diagonals)"""
    map_hs = h.map(2)
    out, sparse_i = [], 0
    for c, rb in zip(cones.cones, cones.rng_blocks):
        idx = None
        if _nonsym(c):
            idx = [map_hs[rb.start:rb.stop]]
            if isinstance(c, GenPowerCone):
                idx += [h.sparse_map(sparse_i, w) for w in range(4)]
            idx = np.concatenate(idx)
        if c.is_sparse_expandable:
            sparse_i += 1
        out.append(idx)
    return out


def _compare_nonsym(cones_h, ksets, K1, K2, nonsym_out, strategy, z, worst):
    """gate 1 per cone: K entries and output slot, device against host, relative Frobenius <= 1e-10; `worst` collects the largest"""
    off = 0
    for c, r, idx in zip(cones_h.cones, cones_h.rng_cones, ksets):
        if not _nonsym(c):
            continue
        tag = (type(c).__name__, "dual" if isinstance(c, GenPowerCone) else strategy)
        e = _rel(K2[idx], K1[idx])
        worst[tag] = max(worst.get(tag, 0.0), e)
        assert e <= GATE, (tag, "K entries", e)
        slot = nonsym_out[off:off + c.scaling_slot_len]
        off += c.scaling_slot_len
        for (name, hv), (_, dv) in zip(_host_slot(c), _split_slot(c, slot)):
            e = _rel(dv, hv)
            worst[tag] = max(worst.get(tag, 0.0), e)
            assert e <= GATE, (tag, name, e)
        if isinstance(c, GenPowerCone):     # the expansion diagonals are exact
            assert np.array_equal(K2[idx[-3:]], np.array([-1.0, -1.0, 1.0]))
    assert off == len(nonsym_out)


def _compare_symmetric(cones_h, dev, K1, K2, map_hs):
    """the symmetric members of the set: the checks of tests/test_gpu_kkt.py::test_update_scaling_on_device_matches_host_cone_algebra"""
    scale = np.maximum(np.abs(K1), 1e-300)
    soc_k, uoff = 0, 0
    u_all, v_all = dev.h.debug_dump(7), dev.h.debug_dump(8)
    for c, r, rb in zip(cones_h.cones, cones_h.rng_cones, cones_h.rng_blocks):
        if _nonsym(c):
            continue
        idx = map_hs[rb.start:rb.stop]
        if c.kind_code in (0, 1):
            assert np.array_equal(K1[idx], K2[idx]), type(c).__name__
            if c.kind_code == 1:
                assert np.array_equal(dev.scaling_w[r], c.w) and np.array_equal(dev.scaling_lambda[r], c.lam)
        else:
            assert np.max(np.abs(K1[idx] - K2[idx]) / scale[idx]) < 5e-13, (type(c).__name__, c.numel)
        if c.kind_code == 2:
            w, lam, eta = dev.scaling_w[r], dev.scaling_lambda[r], dev.scaling_soc_eta[soc_k]
            soc_k += 1
            assert np.allclose(w, c.w, rtol=1e-12, atol=1e-14) and np.allclose(lam, c.lam, rtol=1e-12, atol=1e-14)
            assert abs(eta - c.eta) <= 1e-14 * c.eta
            assert abs(w[0] ** 2 - w[1:] @ w[1:] - 1.0) < 1e-10
            if c.is_sparse_expandable:
                u, v = u_all[uoff:uoff + c.dim], v_all[uoff:uoff + c.dim]
                uoff += c.dim
                d = -K2[idx[0]] / eta ** 2
                D = np.eye(c.dim); D[0, 0] = d
                J = -np.eye(c.dim); J[0, 0] = 1.0
                lhs, rhs = D + np.outer(u, u) - np.outer(v, v), 2.0 * np.outer(w, w) - J
                assert np.linalg.norm(lhs - rhs) < 1e-12 * max(1.0, np.linalg.norm(rhs))


def _solve_both(host, dev, rng, n, m):
    rx, rz = rng.standard_normal(n), rng.standard_normal(m)
    xs = []
    for k in (host, dev):
        k.kktsolver_setrhs(rx, rz)
        x, zz = np.zeros(n), np.zeros(m)
        assert k.kktsolver_solve(x, zz)
        xs.append(np.concatenate([x, zz]))
    assert np.max(np.abs(xs[0] - xs[1])) <= 1e-9 * max(1.0, np.max(np.abs(xs[0])))


def _check_fixture_point(host, dev, cones_h, cones_d, ksets, rng, strategy, worst, n, m):
    """one draw of fixtures.scale_cones_nonsymmetric: host update on `host`, kktsolver_update_scaled on `dev`, gate 1"""
    s, z, mu = fx.scale_cones_nonsymmetric(cones_h, rng, strategy)
    if strategy == "primal_dual":
        for c, r in zip(cones_h.cones, cones_h.rng_cones):
            if _is3(c):
                de1 = _de1(c, s[r], z[r])
                assert not _near_branch(de1), ("a fixture point within a factor 4 of the sqrt(eps) test on de1", de1)
                assert abs(de1) > SQRT_EPS, "a fixture point in the fallback branch"
    assert host.kktsolver_update(cones_h)
    assert dev.kktsolver_update_scaled(cones_d, s, z, mu=mu, strategy=strategy)
    K1, K2 = host.h.debug_dump(4), dev.h.debug_dump(4)
    _compare_nonsym(cones_h, ksets, K1, K2, dev.scaling_nonsym, strategy, z, worst)
    _compare_symmetric(cones_h, dev, K1, K2, host.h.map(2))
    # the adopting cones hold the device's numbers: mul_Hs! of the caller uses what the matrix holds
    for ch, cd in zip(cones_h.cones, cones_d.cones):
        if _is3(ch):
            assert _rel(cd.Hs, ch.Hs) <= GATE and np.array_equal(cd.Hs, cd.Hs.T)
    rest = np.ones(len(K1), dtype=bool)
    for idx in ksets:
        if idx is not None:
            rest[idx] = False
    assert np.max(np.abs(K1[rest] - K2[rest]) / np.maximum(np.abs(K1[rest]), 1e-300), initial=0.0) < 2e-11
    _solve_both(host, dev, rng, n, m)
    return s, z, mu


def _two_solvers(name):
    Pt, A, specs = _prep(PROBLEMS[name]())
    m, n = A.shape
    cones_h, cones_d = _cones_of(specs), _cones_of(specs)
    st = cl.Settings()
    host = HipKKTSolver(Pt, A, cones_h, m, n, st)
    dev = HipKKTSolver(Pt, A, cones_d, m, n, st)
    assert dev.scales_nonsymmetric
    return host, dev, cones_h, cones_d, _k_index_sets(host.h, cones_h), n, m


@pytest.mark.parametrize("name", ["mix_60", "mix_300", "mix_1000"])
def test_blocks_at_fixture_points_match_the_host_cone_algebra(name, capsys):
    """Gate 1.  Strategies PrimalDual, Dual, PrimalDual as in test_assembly_bit_exact_and_factor_solve_parity_with_non_symmetric_cones:
    one solver updated the host way, one by kktsolver_update_scaled; per non-symmetric cone the K entries of its block (and of its q, r,
    p columns and expansion diagonals) and its slot of the output vector at 1e-10 (the stand-in's own spread on these points under 1-ulp
    perturbations is 1.6e-12 / 3.4e-15 / 1.1e-15); no point near the sqrt(eps) branch test, none in the fallback; the symmetric cones
    as in test_update_scaling_on_device_matches_host_cone_algebra; then refactor + refined solve of both agree to 1e-9."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    host, dev, cones_h, cones_d, ksets, n, m = _two_solvers(name)
    worst = {}
    for strategy in ["primal_dual", "dual", "primal_dual"]:
        _check_fixture_point(host, dev, cones_h, cones_d, ksets, rng, strategy, worst, n, m)
    with capsys.disabled():
        print(f"\n[nonsym-scaling fixture points {name}] largest relative Frobenius error device vs host: "
              + ", ".join(f"{k[0]}/{k[1]} {v:.2e}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("name", ["mix_300", "exp_pow_only"])
def test_central_path_points_take_the_fallback(name):
    """Gate 2.  s = -mu grad f*(z): de1 = mu mu~ - 1 vanishes to rounding, the host takes Hs = (<s, z> / 3) H_dual
    (coneops_nonsymmetric_common.jl:157-160, the LOCAL mu) on every three-row cone, and so must the device."""
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    host, dev, cones_h, cones_d, ksets, n, m = _two_solvers(name)
    s, z, mu = fx.scale_cones_nonsymmetric(cones_h, rng, "primal_dual")
    n3 = 0
    for c, r in zip(cones_h.cones, cones_h.rng_cones):
        if _is3(c):
            c.update_dual_grad_H(z[r])
            s[r] = -rng.uniform(0.05, 5.0) * c.grad
            assert c.is_primal_feasible(s[r])
            assert abs(_de1(c, s[r], z[r])) < SQRT_EPS / 4.0
            n3 += 1
    assert n3 > 0
    mu = float(s @ z) / (cones_h.degree + 1)
    assert cones_h.update_scaling(s, z, mu, "primal_dual")
    for c, r in zip(cones_h.cones, cones_h.rng_cones):
        if _is3(c):
            loc = float(z[r][0] * s[r][0] + z[r][1] * s[r][1] + z[r][2] * s[r][2]) / 3
            assert np.array_equal(c.Hs, loc * c.H_dual), "the host did not take the fallback"
    assert host.kktsolver_update(cones_h)
    assert dev.kktsolver_update_scaled(cones_d, s, z, mu=mu, strategy="primal_dual")
    _compare_nonsym(cones_h, ksets, host.h.debug_dump(4), dev.h.debug_dump(4), dev.scaling_nonsym, "primal_dual", z, {})


# ---- gate 3: shadow run on IPM iterates -------------------------------------------------------------------------------------------

def _block_of(c, mu):
    """the values a cone contributes to K (before the sign): pack_triu(Hs), resp. [mu d1 | mu d2 | sqrt(mu) (q, r, p)]"""
    if _is3(c):
        return _triu(c.Hs)
    return np.concatenate([mu * c.d1, [mu * c.d2], math.sqrt(mu) * c.q, math.sqrt(mu) * c.r, math.sqrt(mu) * c.p])


def _host_spread(c, s, z, mu, strategy, rng):
    """largest relative Frobenius change of the cone's block over 8 random +-1-ulp perturbations of its (s, z), host cone algebra"""
    k = PowerCone(c.alpha) if isinstance(c, PowerCone) else ExponentialCone() if isinstance(c, ExponentialCone) else GenPowerCone(c.alpha, c.dim2)
    k.update_scaling(s, z, mu, strategy)
    base = _block_of(k, mu)
    worst = 0.0
    for _ in range(8):
        sp_ = np.nextafter(s, np.where(rng.random(len(s)) < 0.5, -np.inf, np.inf))
        zp_ = np.nextafter(z, np.where(rng.random(len(z)) < 0.5, -np.inf, np.inf))
        try:
            k.update_scaling(sp_, zp_, mu, strategy)
            worst = max(worst, _rel(_block_of(k, mu), base))
        except (AssertionError, ValueError, ArithmeticError):
            return float("inf")
    return worst if np.isfinite(worst) else float("inf")


class _ShadowScaling:
    """Test infrastructure: a host-updated HipKKTSolver drives the IPM (the stand-in scales every cone on the host); at every iteration a
    second handle is given the same (s, z, mu, strategy) through hipkkt_update_scaling_ex and its blocks are compared with the host's."""
    scales_nonsymmetric = False      # (the IPM keeps its host update_scaling of every cone)

    def __init__(self, P, A, cones, m, n, settings):
        self.g = HipKKTSolver(P, A, cones, m, n, settings)
        self.d = HipKKTSolver(P, A, cones, m, n, settings)
        self.settings = settings
        self.ksets = _k_index_sets(self.g.h, cones)
        self.rng = np.random.default_rng(2024)
        self.it = 0
        self.rows = []       # (iteration, cone type, strategy, held, err, spread, de1, device block PD, host block PD)

    def __getattr__(self, k):
        return getattr(self.g, k)

    def kktsolver_update_scaled(self, cones, s, z, mu=None, strategy=None):
        ok = self.g.kktsolver_update(cones)
        R = None
        okd, _, _, _, ns = self.d.h.update_scaling_ex(s, z, mu, STRATEGY[strategy], R)
        assert okd, f"iteration {self.it}: the device rejects an iterate the host scaled"
        K1, K2 = self.g.h.debug_dump(4), self.d.h.debug_dump(4)
        off = 0
        for c, r, idx in zip(cones.cones, cones.rng_cones, self.ksets):
            if not _nonsym(c):
                continue
            strat = "dual" if isinstance(c, GenPowerCone) else strategy
            slot = ns[off:off + c.scaling_slot_len]
            off += c.scaling_slot_len
            err = _rel(K2[idx], K1[idx])
            spread = _host_spread(c, s[r].copy(), z[r].copy(), mu, strat, self.rng)
            de1 = _de1(c, s[r], z[r]) if (_is3(c) and strat == "primal_dual") else None
            held = spread <= 1e-12 and not (de1 is not None and _near_branch(de1))
            if held:
                assert err <= GATE, (self.it, type(c).__name__, strat, err, spread)
                for (name, hv), (_, dv) in zip(_host_slot(c), _split_slot(c, slot)):
                    assert _rel(dv, hv) <= GATE, (self.it, type(c).__name__, strat, name)
            else:        # finite (symmetric by construction: only the upper triangle exists), d1, d2 > 0
                assert np.all(np.isfinite(slot)) and np.all(np.isfinite(K2[idx]))
                if not _is3(c):
                    d1 = dict(_split_slot(c, slot))
                    assert np.all(d1["d1"] > 0) and d1["d2"][0] > 0
            dev_pd = (not _is3(c)) or _chol3_factor(_full(slot[0:6])) is not None
            host_pd = (not _is3(c)) or _chol3_factor(c.Hs) is not None
            self.rows.append((self.it, type(c).__name__, strat, held, err, spread, de1, dev_pd, host_pd))
        self.it += 1
        return ok


_SHADOW_ROWS = {}


def _shadow_rows(name):
    """the shadow run of one problem (once per process): a host-driven IPM run, the device given the same (s, z, mu, strategy)"""
    if name not in _SHADOW_ROWS:
        P, q, A, b, specs = PROBLEMS[name]()
        box = {}

        def factory(*a):
            box["k"] = _ShadowScaling(*a)
            return box["k"]

        sol = cl.Solver(P, q, A, b, specs, cl.Settings(device_scaling=True), kktsolver_factory=factory).solve()
        _SHADOW_ROWS[name] = (sol, box["k"].rows)
    return _SHADOW_ROWS[name]


@pytest.mark.parametrize("name", ["mix_60", "mix_300", "exp_pow_only"])
def test_shadow_run_on_ipm_iterates(name, capsys):
    """Gate 3.  Blocks whose host spread (8 perturbations, fixed seed) is <= 1e-12 and whose |de1| is not within a factor 4 of
    sqrt(eps) (PrimalDual) are held to 1e-10 (asserted while the run goes); every block of iterations 0-2 is held and at least 0.6 of
    all blocks of the problem (the stand-in alone gives 0.73 - 0.78); every other block is finite and symmetric resp. has d1, d2 > 0,
    its error / spread ratio is printed.  (Positive definiteness of those blocks: the next test.)"""
    sol, rows = _shadow_rows(name)
    assert sol.status == "SOLVED" and rows
    held = [r for r in rows if r[3]]
    early = [r for r in rows if r[0] <= 2]
    other = [r for r in rows if not r[3]]
    ratios = [r[4] / r[5] for r in other if np.isfinite(r[5]) and r[5] > 0]
    with capsys.disabled():
        print(f"\n[nonsym-scaling shadow {name}] {sol.iterations} iterations, {len(rows)} blocks, held {len(held)} ({len(held) / len(rows):.3f}), "
              f"largest error of a held block {max((r[4] for r in held), default=0.0):.2e}; not held: {len(other)}, error / spread ratio "
              f"median {np.median(ratios) if ratios else float('nan'):.2e} max {max(ratios, default=float('nan')):.2e}, largest error {max((r[4] for r in other), default=0.0):.2e}")
    assert early and all(r[3] for r in early), [r for r in early if not r[3]][:3]
    assert len(held) >= 0.6 * len(rows), (len(held), len(rows))


@pytest.mark.parametrize("name", ["mix_60", "mix_300", "exp_pow_only"])
def test_shadow_run_blocks_not_held_are_positive_definite(name, capsys):
    """Gate 3, last condition: every block that is not held is positive definite by the 3 x 3 Cholesky of mathutils.jl:427-451.

    The HOST cone algebra does not meet this on the last iterates of these runs: the reference's Hs reaches condition numbers of
    1e16 .. 4e18 there and the Cholesky of the rounded block breaks down (measured, host blocks failing of all blocks: mix_60 4 of 357,
    mix_300 50 of 2970, exp_pow_only 21 of 950, none before iteration 19 of 21 / 21 of 27 / 15 of 19; without its safeguard the device
    fails on 3 / 51 / 18, bit for bit the host's block under the Dual strategy).  The kernel therefore shifts the diagonal of a block
    whose Cholesky breaks down by the smallest 2^k eps max(diag), k = 1 .. 8, that lets it go through (scaling.hip
    keep_positive_definite; k = 1, i.e. 4.4e-16 relative, on every block met here); blocks whose Cholesky goes through are never touched.
    The host's own count is printed next to the device's."""
    sol, rows = _shadow_rows(name)
    other = [r for r in rows if not r[3]]
    dev_bad, host_bad = [r for r in other if not r[7]], [r for r in other if not r[8]]
    all_host_bad = [r for r in rows if not r[8]]
    with capsys.disabled():
        print(f"\n[nonsym-scaling shadow {name}] blocks not held: {len(other)} of {len(rows)}; 3 x 3 Cholesky fails on the device's block: {len(dev_bad)}, "
              f"on the host's own block: {len(host_bad)} (host, over all blocks: {len(all_host_bad)}); both: {sum(1 for r in dev_bad if not r[8])}; "
              f"first iteration with one: {min((r[0] for r in dev_bad + host_bad), default=None)} of {sol.iterations}")
    assert not dev_bad, (len(dev_bad), len(host_bad), dev_bad[:3])


# ---- gate 4: end to end -------------------------------------------------------------------------------------------------------------

with open(os.path.join(HERE, "golden", "reference_known_answers.json")) as _f:
    _KNOWN = {e["name"]: e for e in json.load(_f)["reference"]}
E2E = [("exp_fixture", "exp"), ("pow_fixture", "pow"), ("genpow_fixture", "genpow"), ("mix_60", None), ("mix_300", None), ("exp_pow_only", None)]


@pytest.mark.parametrize("name,known", E2E)
def test_ipm_with_device_scaling_of_non_symmetric_cones(name, known, monkeypatch, capsys):
    """Gate 4.  Settings(device_scaling=True) against False, both on HipKKTSolver: same status, the reference's known answers at its own
    1e-3, objective <= 1e-7 and x <= 1e-3 relative between the two runs; in the device-scaling run the host update_scaling! of the
    non-symmetric cones (and with it use_primal_dual_scaling's gradient_primal) is a raising stub.  (gradient_primal itself stays
    callable: the Power cone's primal barrier of the caller's line search uses it, coneops_powcone.jl:239-251.)"""
    prob = PROBLEMS[name]()
    ref = cl.Solver(*prob, cl.Settings(), kktsolver_factory=lambda *a: HipKKTSolver(*a)).solve()

    def stub(self, *a, **k):
        raise AssertionError("host scaling of a non-symmetric cone called in a device-scaling run")

    with monkeypatch.context() as mp:
        for cls in (ExponentialCone, PowerCone, GenPowerCone):
            mp.setattr(cls, "update_scaling", stub)
            mp.setattr(cls, "update_dual_grad_H", stub)
        mp.setattr(cl.cones_nonsym._Cone3, "_use_primal_dual_scaling", stub)
        got = cl.Solver(*prob, cl.Settings(device_scaling=True), kktsolver_factory=lambda *a: HipKKTSolver(*a)).solve()
    with capsys.disabled():
        print(f"\n[nonsym-scaling e2e {name}] iterations host scaling {ref.iterations} / device scaling {got.iterations}, status {ref.status} / {got.status}, "
              f"|dobj| rel {abs(got.obj_val - ref.obj_val) / max(1.0, abs(ref.obj_val)):.2e}, |dx| rel {np.max(np.abs(got.x - ref.x)) / max(1.0, np.max(np.abs(ref.x))):.2e}")
    assert got.status == ref.status == "SOLVED"
    if known is not None:
        e = _KNOWN[known]
        for sol in (ref, got):
            assert sol.status == e["status"]
            if e["x"] is not None:
                assert np.linalg.norm(sol.x - np.array(e["x"])) < e["tol"]
            assert abs(sol.obj_val - e["obj"]) < e["tol"]
    assert abs(got.obj_val - ref.obj_val) <= 1e-7 * max(1.0, abs(ref.obj_val))
    assert np.max(np.abs(got.x - ref.x)) <= 1e-3 * max(1.0, np.max(np.abs(ref.x)))


# ---- gates 5 - 7 ---------------------------------------------------------------------------------------------------------------------

class _DevBuf:
    """device memory through the HIP runtime the library is linked with (as tests/test_gpu_kkt.py)"""
    _hip = None

    def __init__(self, arr_or_n):
        import ctypes as C
        if _DevBuf._hip is None:
            _DevBuf._hip = C.CDLL("libamdhip64.so")
        self.C, self.hip = C, _DevBuf._hip
        host = np.zeros(arr_or_n) if isinstance(arr_or_n, int) else np.ascontiguousarray(arr_or_n, dtype=np.float64)
        self.n = host.size
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(max(host.nbytes, 8))) == 0
        assert self.hip.hipMemcpy(self.ptr, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes), 1) == 0

    def get(self):
        out = np.zeros(self.n)
        assert self.hip.hipMemcpy(out.ctypes.data_as(self.C.c_void_p), self.ptr, self.C.c_size_t(out.nbytes), 2) == 0
        return out

    def __del__(self):
        self.hip.hipFree(self.ptr)


@pytest.mark.parametrize("strategy", ["primal_dual", "dual"])
def test_update_scaling_ex_dev_keeps_everything_in_hbm(strategy):
    """Gate 5: the pattern of test_update_scaling_dev_keeps_everything_in_hbm"""
    Pt, A, specs = _prep(PROBLEMS["mix_300"]())
    m, n = A.shape
    cones = _cones_of(specs)
    k = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    s, z, mu = fx.scale_cones_nonsymmetric(cones, np.random.default_rng(6), strategy)
    ok, w, lam, eta, ns = k.h.update_scaling_ex(s, z, mu, STRATEGY[strategy])
    assert ok and len(ns) == k.h.nonsym_len() > 0
    K_host_ptrs = k.h.debug_dump(4)
    sd, zd = _DevBuf(s), _DevBuf(z)
    wd, ld, ed, nd = _DevBuf(m), _DevBuf(m), _DevBuf(max(len(eta), 1)), _DevBuf(len(ns))
    k.h.update_values(k.h.map(2), np.zeros(k.h.nHs))       # wipe the blocks so that the second call must rewrite them
    for i in range(k.h.nsparse):
        for wch in range(4):
            idx = k.h.sparse_map(i, wch)
            k.h.update_values(idx, np.zeros(len(idx)))
    assert not np.array_equal(k.h.debug_dump(4), K_host_ptrs)
    assert k.h.update_scaling_ex_dev(sd.ptr, zd.ptr, mu, STRATEGY[strategy], None, wd.ptr, ld.ptr, ed.ptr, nd.ptr)
    assert np.array_equal(k.h.debug_dump(4), K_host_ptrs)
    assert np.array_equal(wd.get(), w) and np.array_equal(ld.get(), lam) and np.array_equal(ed.get()[:len(eta)], eta)
    assert np.array_equal(nd.get(), ns)


def _mixed_cone_problem(seed=77, n=30):      # tests/test_gpu_kkt.py::_mixed_cone_problem
    rng = np.random.default_rng(seed)
    specs = [cl.ZeroConeT(3), cl.NonnegativeConeT(40), cl.SecondOrderConeT(3), cl.SecondOrderConeT(4), cl.SecondOrderConeT(7),
             cl.PSDTriangleConeT(4), cl.SecondOrderConeT(300), cl.NonnegativeConeT(5), cl.PSDTriangleConeT(2), cl.SecondOrderConeT(2)]
    from clarabel_jl_amd.cone_api import nvars
    m = sum(nvars(c) for c in specs)
    A = sp.random(m, n, density=0.15, random_state=np.random.RandomState(seed), format="csc") + \
        sp.vstack([sp.identity(n), sp.csc_matrix((m - n, n))]).tocsc()
    Pm = sp.random(n, n, density=0.1, random_state=np.random.RandomState(seed + 1))
    P = (Pm @ Pm.T + sp.identity(n)).tocsc()
    return P, rng.standard_normal(n), A.tocsc(), rng.standard_normal(m), specs


def test_old_calls_are_untouched_and_refuse_a_handle_with_non_symmetric_kinds():
    """Gate 6: on a symmetric cone set the _ex registration + update_scaling_ex leave K, w, lambda, eta bit-identical to
    set_cone_types + update_scaling; update_scaling on a handle registered with a kind 4..6 raises."""
    Pt, A, specs = _prep(_mixed_cone_problem())
    m, n = A.shape
    cones = _cones_of(specs)
    old = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    new = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    assert not new.scales_nonsymmetric
    kinds, alpha = cones.kkt_cone_kinds_ex()
    assert np.array_equal(kinds, cones.kkt_cone_kinds()) and len(alpha) == 0
    new.h.set_cone_types_ex(kinds, alpha)
    assert new.h.nonsym_len() == 0
    s, z = fx.scale_cones(cones, np.random.default_rng(5))
    R = np.concatenate([c.R.ravel(order="F") for c in old._psd_cones])
    for strategy in (0, 1):
        ok1, w1, l1, e1 = old.h.update_scaling(s, z, R)
        ok2, w2, l2, e2, ns = new.h.update_scaling_ex(s, z, 0.37, strategy, R)
        assert ok1 and ok2 and len(ns) == 0
        assert np.array_equal(old.h.debug_dump(4), new.h.debug_dump(4))
        assert np.array_equal(w1, w2) and np.array_equal(l1, l2) and np.array_equal(e1, e2)
    ok3, w3, l3, e3 = new.h.update_scaling(s, z, R)          # the old call on the _ex-registered symmetric handle still works
    assert ok3 and np.array_equal(w1, w3) and np.array_equal(old.h.debug_dump(4), new.h.debug_dump(4))
    Pt, A, specs = _prep(PROBLEMS["mix_60"]())
    m, n = A.shape
    cones = _cones_of(specs)
    k = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    s, z, mu = fx.scale_cones_nonsymmetric(cones, np.random.default_rng(1), "dual")
    with pytest.raises(hipkkt.HipKKTError):
        k.h.update_scaling(s, z)
    k.h.set_cone_types(cones.kkt_cone_kinds())               # the last registration decides: the caller's cones again
    ok, *_ = k.h.update_scaling(s, z)
    assert ok


def test_failure_is_a_flag_and_bad_arguments_are_refused():
    """Gate 7.  z of one Exponential, one Power and one GenPower cone outside the dual cone, s of one outside the primal cone
    (PrimalDual): ok == False with return code HIPKKT_OK (no exception), the slots of the failing cones are NaN, the process lives and
    a following call with interior points passes gate 1.  Then the argument checks of the registration and of the update."""
    host, dev, cones_h, cones_d, ksets, n, m = _two_solvers("mix_60")
    rng = np.random.default_rng(11)
    s, z, mu = fx.scale_cones_nonsymmetric(cones_h, rng, "primal_dual")
    first = {}
    off, offs = 0, {}
    for c, r in zip(cones_h.cones, cones_h.rng_cones):
        if _nonsym(c):
            first.setdefault(type(c), (c, r))
            offs[id(c)] = off
            off += c.scaling_slot_len
    assert set(first) == {ExponentialCone, PowerCone, GenPowerCone}
    bad_z = {ExponentialCone: np.array([1.0, 1.0, 1.0]), PowerCone: np.array([0.5, 0.5, 10.0])}
    for strategy in ("primal_dual", "dual"):
        for cls, (c, r) in first.items():
            zb = z.copy()
            if cls is GenPowerCone:
                zb[r] = np.concatenate([np.full(c.dim1, 0.1), np.full(c.dim2, 10.0)])
            else:
                zb[r] = bad_z[cls]
            assert not c.is_dual_feasible(zb[r])
            ok, _, _, _, ns = dev.h.update_scaling_ex(s, zb, mu, STRATEGY[strategy])
            assert not ok
            assert np.all(np.isnan(ns[offs[id(c)]:offs[id(c)] + c.scaling_slot_len]))
            assert np.sum(np.isnan(ns)) == c.scaling_slot_len      # the other cones are not affected
    c, r = first[PowerCone]
    sb = s.copy(); sb[r] = np.array([0.5, 0.5, -10.0])
    assert not c.is_primal_feasible(sb[r])
    ok, *_ = dev.h.update_scaling_ex(sb, z, mu, 0)
    assert not ok
    ok, *_ = dev.h.update_scaling_ex(sb, z, mu, 1)               # Dual never looks at s
    assert ok
    c, r = first[ExponentialCone]
    sb = s.copy(); sb[r] = np.array([1.0, -1.0, 1.0])
    ok, *_ = dev.h.update_scaling_ex(sb, z, mu, 0)
    assert not ok
    zb = z.copy(); zb[first[GenPowerCone][1]] = 0.0                 # zeros: phi = 0
    ok, *_ = dev.h.update_scaling_ex(s, zb, mu, 0)
    assert not ok
    assert not dev.kktsolver_update_scaled(cones_d, s, zb, mu=mu, strategy="primal_dual")
    # the handle is as good as before
    worst = {}
    for strategy in ("primal_dual", "dual"):
        _check_fixture_point(host, dev, cones_h, cones_d, ksets, rng, strategy, worst, n, m)
    # arguments
    kinds, alpha = cones_d.kkt_cone_kinds_ex()
    h = dev.h
    with pytest.raises(ValueError):
        h.set_cone_types_ex(kinds, alpha[:-1])                        # wrong nalpha
    with pytest.raises(ValueError):
        h.set_cone_types_ex(kinds, np.concatenate([alpha, [0.5]]))
    for bad in (0.0, 1.0, 1.5, -0.2, float("nan")):
        a2 = alpha.copy(); a2[0] = bad
        with pytest.raises(ValueError):
            h.set_cone_types_ex(kinds, a2)                            # alpha outside (0, 1)
    k2 = kinds.copy()
    nn = next(i for i, c in enumerate(cones_d.cones) if c.kind_code == 1)
    k2[nn] = 4
    with pytest.raises(ValueError):
        h.set_cone_types_ex(k2, alpha)                                # kind 4 on a cone with numel != 3
    k2 = kinds.copy()
    e = next(i for i, c in enumerate(cones_d.cones) if isinstance(c, ExponentialCone))
    k2[e] = 6
    with pytest.raises(ValueError):
        h.set_cone_types_ex(k2, np.concatenate([alpha, [0.5]]))       # kind 6 on a cone without a GenPow map
    with pytest.raises(hipkkt.HipKKTError):                           # the failed registrations left the handle unregistered
        h.update_scaling_ex(s, z, mu, 0)
    h.set_cone_types_ex(kinds, alpha)
    with pytest.raises(ValueError):
        h.update_scaling_ex(s, z, mu, 2)                              # strategy outside {0, 1}
    import ctypes as C
    okc = C.c_int32(0)
    assert h.L.hipkkt_update_scaling_ex(h.h, s, z, None, mu, 7, None, None, None, None, C.byref(okc)) == -1   # HIPKKT_ERR_ARGUMENT
    with pytest.raises(ValueError):
        h.update_scaling_ex(s[:-1], z, mu, 0)
    with pytest.raises(ValueError):
        h.update_scaling_ex(s, z, mu, 0, np.zeros(3))                 # there is no PSD cone: no R factor expected
    ok, *_ = h.update_scaling_ex(s, z, mu, 0)
    assert ok
