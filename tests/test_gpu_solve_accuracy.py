"""Backward error of the UNREFINED LDL solve, solve path by solve path (hipkkt_ldl_solve; hipkkt_solve_multi without refinement).

The solve kernels multiply by explicit inverses of diagonal blocks -- supernodes and 64-column front panels (k_invert_diag*), the
512 x 512 super-blocks of a long front (k_invert_super) -- where the reference substitutes.  A normwise forward error against the
oracle (what tests/test_gpu_kkt.py checks) hides errors in small components, and on ill-conditioned systems it mostly measures the
conditioning.  What tells a backward-stable solve from one that is not is the componentwise backward error of x against the matrix
that was really factored,
    omega(x) = max_i |b - K~ x|_i / (|K~| |x| + |b|)_i,         K~ = K + eps diag(Dsigns),
with the residual computed exactly (tests/accuracy.py).  Every case compares the HIP handle's unrefined solve with the oracle's
(scalar QDLDL, substitution everywhere) on the same permutation, the same K~ and the same b, against a bound fixed in advance:
    omega_hip <= 4 max(omega_oracle, 2^-50)
A case that fails is a finding about the kernels, never a reason to widen the bound.  Each case also asserts that it reached its
solve path (counters, plan tables 10 - 14 and the front table 22 of hipkkt_debug_dump) and that no pivot was dynamically
regularised (otherwise the factored matrix is not known exactly)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import clarabel_jl_amd  # noqa: F401  (registers the dotted package directory)
import julia_standin as cl
from clarabel_jl_amd import problems
from clarabel_jl_amd.kktsolver import HipKKTSolver
from oracle.kkt_oracle import OracleKKT, OracleKKTSolver
from tests import accuracy as acc
from tests import plan_support as ps
from tests.fixtures import scale_cones, scale_cones_late

pytestmark = pytest.mark.gpu

BOUND, FLOOR = 4.0, 2.0 ** -50

# Three iterates per case, from one seed fixed before any GPU run: at every one of them neither the oracle nor the plan interpreter
# regularises a pivot dynamically (asserted below), and of seeds 0 - 3 it is the one at which the interpreter predicts the largest loss
# for the super-block inverses (tests/test_front_inverse_accuracy.py) -- the test must contain the iterate most likely to expose it.
SEED = 2
ITERATES = {
    "central": lambda cones, rng: scale_cones(cones, rng),
    "late_mu1e-9": lambda cones, rng: scale_cones_late(cones, rng, mu=1e-9, span=6),
    "late_mu1e-10": lambda cones, rng: scale_cones_late(cones, rng, mu=1e-10, span=8),
}


def _prep(prob):
    P, q, A, b, specs = prob
    cones = cl.CompositeCone(cl.cones_new_collapsed(specs))
    Pt = sp.triu(sp.csc_matrix(P), format="csc")
    Pt.sort_indices()
    A = sp.csc_matrix(A)
    A.sort_indices()
    return Pt, A, cones


def _factored(h, eps):
    colptr, rowval, nz = h.kkt()
    return acc.factored_kkt(colptr, rowval, nz, h.dsigns(), eps, h.map(4))


def _report(capsys, path, iterate, wg, wc, marked):
    with capsys.disabled():
        print(f"\n[solve-accuracy {path} / {iterate}] omega hip {wg:.3e} oracle {wc:.3e} ratio {wg / max(wc, FLOOR):.2f} "
              f"marked blocks {marked}")


def _fronts(h):
    """hipkkt_debug_dump 22, checked against the plan tables 10 / 12 / 14: one row (first panel, panels, rows, panels per super-block)
    per front; a front's panels are consecutive supernodes of at most 64 columns that the segment sweeps do not solve"""
    F = h.debug_dump(22).reshape(-1, 4).astype(np.int64)
    first, rows, member = h.debug_dump(10), h.debug_dump(12), h.debug_dump(14)
    for s0, npan, rF, g in F:
        assert npan >= 1 and rows[s0] == rF and g in (0, 8)
        assert not np.any(member[s0:s0 + npan])
        assert np.all(np.diff(first[s0:s0 + npan + 1]) <= 64)
    return F


def _omega(hk, o, cones, iterate, path, capsys):
    """the case's iterate on both solvers, then one unrefined solve each: -> (omega_hip, omega_oracle)"""
    rng = np.random.default_rng(SEED)
    ITERATES[iterate](cones, rng)
    assert hk.kktsolver_update(cones) and o.kktsolver_update(cones)
    assert hk.last_nreg == 0 and o.k.L.oracle_kkt_nreg(o.k.h) == 0       # no substituted pivot: K~ is exactly what was factored
    assert abs(hk.diagonal_regularizer - o.diagonal_regularizer) <= 1e-16 * max(1.0, o.diagonal_regularizer)
    assert np.array_equal(hk.h.kkt()[2], o.k.nzval)
    b = rng.standard_normal(hk.h.N)
    wg = acc.backward_error(_factored(hk.h, hk.diagonal_regularizer), hk.h.ldl_solve(b), b)
    wc = acc.backward_error(_factored(hk.h, o.diagonal_regularizer), o.k.ldl_solve(b), b)
    _report(capsys, path, iterate, wg, wc, hk.h.profile()["refined_blocks"])
    return wg, wc


# ---- cfg 1 (1000 x 2000 NN QP): a 12-panel root front, thousands of narrow leaves, segment sweeps.  Switches and options that move its
# root front between the solve forms and the factorisation forms; HIPKKT_PLAN_CACHE=0 because they change the plan
CFG1 = {
    "panel_hop": ({"HIPKKT_SUPERHOP": "0"}, {}),
    "super_block": ({"HIPKKT_SUPERHOP": "1"}, {}),
    "super_block_w16": ({"HIPKKT_SUPERHOP": "1"}, {"supernode_max_width": 16}),
    "front_block2": ({"HIPKKT_FRONT_BLOCK_MIN_ROWS": "0"}, {}),
    "front_block1": ({"HIPKKT_FRONT_BLOCK_MIN_ROWS": "0", "HIPKKT_FB_V2": "0"}, {}),
}


@pytest.mark.parametrize("iterate", list(ITERATES))
@pytest.mark.parametrize("path", list(CFG1))
def test_cfg1_front_paths(path, iterate, monkeypatch, capsys):
    env, kw = CFG1[path]
    monkeypatch.setenv("HIPKKT_PLAN_CACHE", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    Pt, A, cones = _prep(problems.random_sparse_qp(1000, 2000, 1, 4, 2))
    m, n = A.shape
    st = cl.Settings()
    hk = HipKKTSolver(Pt, A, cones, m, n, st, **kw)
    o = OracleKKTSolver(Pt, A, cones, m, n, st, ordering=hk.h.perm())
    c = hk.h.counters()
    assert c["fronts"] >= 1 and c["persistent"]
    F = _fronts(hk.h)
    sb = F[F[:, 3] > 0]
    if path == "super_block":
        assert len(sb) >= 1 and np.any((sb[:, 1] >= 10) & (sb[:, 1] % sb[:, 3] != 0))   # the 12-panel root: a partial second super-block
    elif path == "super_block_w16":
        assert len(sb) >= 1 and sb[:, 1].max() >= 16             # the root in 16-column panels: k_invert_super's narrow-panel path
    else:
        assert len(sb) == 0 and F[:, 1].max() >= 10              # the root, one hop per panel
    wg, wc = _omega(hk, o, cones, iterate, f"cfg1 {path}", capsys)
    c = hk.h.counters()
    assert c["sweep_timeouts"] == 0
    if path.startswith("front_block"):
        assert c["front_batches"] >= 1 and c["front_block"]      # the fronts were factored by one launch per update batch
    assert wg <= BOUND * max(wc, FLOOR), (wg, wc)


@pytest.mark.parametrize("iterate", list(ITERATES))
@pytest.mark.parametrize("name", ["sdp_small", "portfolio_small"])
def test_dense_cone_blocks(name, iterate, capsys):
    prob = problems.sdp_blocks(n=60, ncones=3, dim=8, seed=5) if name == "sdp_small" else \
        problems.portfolio_socp(n=300, nsoc=4, socdim=21, seed=3)
    Pt, A, cones = _prep(prob)
    m, n = A.shape
    st = cl.Settings()
    hk = HipKKTSolver(Pt, A, cones, m, n, st)
    o = OracleKKTSolver(Pt, A, cones, m, n, st, ordering=hk.h.perm())
    _fronts(hk.h)
    wg, wc = _omega(hk, o, cones, iterate, name, capsys)
    assert hk.h.counters()["sweep_timeouts"] == 0
    assert wg <= BOUND * max(wc, FLOOR), (wg, wc)


# ---- batch seed 324 at IPM iteration 19 (tests/test_block_refinement.py): the oracle-driven IPM's K, eps and first right-hand side of
# that iteration, loaded into a HIP handle with hipkkt_update_values + refactor.  No dynamically regularised pivot there (asserted).
class _Capture(OracleKKTSolver):
    it, want, caps = 0, 19, []

    def kktsolver_update(self, cones):
        _Capture.it += 1
        return super().kktsolver_update(cones)

    def kktsolver_setrhs(self, rx, rz):
        self._b = np.concatenate([rx, rz, np.zeros(self.k.N - len(rx) - len(rz))])
        super().kktsolver_setrhs(rx, rz)

    def kktsolver_solve(self, lx, lz):
        ok = super().kktsolver_solve(lx, lz)
        if _Capture.it == _Capture.want and not _Capture.caps:
            _Capture.caps.append(dict(b=self._b.copy(), nz=self.k.nzval, eps=self.diagonal_regularizer,
                                      nreg=int(self.k.L.oracle_kkt_nreg(self.k.h))))
        return ok


@functools.lru_cache(maxsize=1)
def _seed324():
    P, q, A, b, specs = problems.batch_problem(324)
    Pt, Ac, cones = _prep((P, q, A, b, specs))
    k0 = OracleKKT(Pt, Ac, *cones.kkt_descriptors())
    rc, _, perm, _ = ps.run(k0.N, k0.colptr, k0.rowval, k0.nzval.copy(), k0.map("dsigns"), symbolic_only=True)
    assert rc == 0
    _Capture.it, _Capture.caps = 0, []
    sol = cl.Solver(P, q, A, b, specs, cl.Settings(), kktsolver_factory=lambda *a: _Capture(*a, ordering=perm)).solve()
    assert sol.status == "SOLVED" and sol.iterations == 23 and len(_Capture.caps) == 1
    return Pt, Ac, cones, _Capture.caps[0]


def _seed324_handle():
    """a HIP handle and the oracle (same permutation) holding iteration 19's K~: -> (handle, oracle, K~)"""
    Pt, Ac, cones, c = _seed324()
    assert c["nreg"] == 0
    m, n = Ac.shape
    st = cl.Settings()
    h = HipKKTSolver(Pt, Ac, cones, m, n, st).h
    idx = np.arange(h.nnzK, dtype=np.int64)
    h.update_values(idx, c["nz"])
    ok, eps, nreg = h.refactor(True, st.static_regularization_constant, st.static_regularization_proportional)
    assert ok and nreg == 0 and eps == c["eps"]
    assert np.array_equal(h.kkt()[2], c["nz"])
    o = OracleKKT(Pt, Ac, *cones.kkt_descriptors())
    o.symbolic(h.perm())
    o.L.oracle_kkt_update_values(o.h, idx, np.ascontiguousarray(c["nz"]), len(idx))
    oeps = C.c_double(0)
    assert o.L.oracle_kkt_regularize_and_refactor(o.h, 1, st.static_regularization_constant, st.static_regularization_proportional,
                                                  C.byref(oeps))
    assert oeps.value == eps and o.L.oracle_kkt_nreg(o.h) == 0
    return h, o, _factored(h, eps)


def _seed324_case(capsys, path):
    b = _seed324()[3]["b"]
    h, o, K = _seed324_handle()
    wg, wc = acc.backward_error(K, h.ldl_solve(b), b), acc.backward_error(K, o.ldl_solve(b), b)
    marked = h.profile()["refined_blocks"]
    _report(capsys, f"seed 324 {path}", "IPM iteration 19", wg, wc, marked)
    return wg, wc, marked, h


def test_seed324_segment_sweeps(capsys):
    """the persistent segment sweeps (k_fwd_seg / k_bwd_seg) with the refinement step on the marked wide blocks"""
    wg, wc, marked, h = _seed324_case(capsys, "segment sweeps")
    c = h.counters()
    assert c["persistent"] and c["sweep_timeouts"] == 0 and h.debug_dump(14).sum() > 0
    assert marked > 0
    assert wg <= BOUND * max(wc, FLOOR), (wg, wc)


def test_seed324_per_level_kernels(monkeypatch, capsys):
    """HIPKKT_NO_PERSIST=1: every supernode through the per-level kernels (k_fwd_level / k_bwd_final / the narrow kernels)"""
    monkeypatch.setenv("HIPKKT_NO_PERSIST", "1")
    wg, wc, marked, h = _seed324_case(capsys, "per-level kernels")
    c = h.counters()
    assert not c["persistent"] and c["sweep_timeouts"] == 0
    assert marked > 0
    assert wg <= BOUND * max(wc, FLOOR), (wg, wc)


def test_seed324_unrefined_blocks_are_detected(monkeypatch, capsys):
    """negative control: HIPKKT_ACCURATE=0 (never refine a block: the defect fixed in round 5) must show in omega, as e_inv >= 2 e_sub
    does in tests/test_block_refinement.py"""
    wg, _, marked, _ = _seed324_case(capsys, "segment sweeps")
    monkeypatch.setenv("HIPKKT_ACCURATE", "0")
    w0, _, marked0, _ = _seed324_case(capsys, "segment sweeps, ACCURATE=0")
    assert marked > 0 and marked0 == 0
    assert w0 >= 2.0 * wg, (w0, wg)


def test_seed324_solve_multi_without_refinement(capsys):
    """hipkkt_solve_multi with ir_enable = 0: three right-hand sides on the concurrent solve contexts, each column against the bound"""
    _, Ac, _, c = _seed324()
    m, n = Ac.shape
    rng = np.random.default_rng(SEED)
    B = np.stack([c["b"], rng.standard_normal(n + m), rng.standard_normal(n + m)])
    h, o, K = _seed324_handle()
    assert h.p == 0
    lx, lz = np.zeros((3, n)), np.zeros((3, m))
    ok, _ = h.solve_multi(B[:, :n], B[:, n:], lx, lz, ir_enable=False)
    assert ok
    for j in range(3):
        wg, wc = acc.backward_error(K, np.concatenate([lx[j], lz[j]]), B[j]), acc.backward_error(K, o.ldl_solve(B[j]), B[j])
        _report(capsys, f"seed 324 solve_multi rhs {j}", "IPM iteration 19", wg, wc, h.profile()["refined_blocks"])
        assert wg <= BOUND * max(wc, FLOOR), (j, wg, wc)


@pytest.mark.slow
@pytest.mark.parametrize("iterate", list(ITERATES))
def test_cfg2a_root_front(iterate, capsys):
    """cfg 2a at full size, default path: the 88-panel root swept super-block by super-block (the oracle needs ~25 s per factorisation)"""
    Pt, A, cones = _prep(problems.random_sparse_qp(10000, 20000, 2, 3, 1))
    m, n = A.shape
    st = cl.Settings()
    hk = HipKKTSolver(Pt, A, cones, m, n, st)
    o = OracleKKTSolver(Pt, A, cones, m, n, st, ordering=hk.h.perm())
    F = _fronts(hk.h)
    assert np.any((F[:, 1] >= 16) & (F[:, 3] > 0))
    wg, wc = _omega(hk, o, cones, iterate, "cfg2a default", capsys)
    assert hk.h.counters()["sweep_timeouts"] == 0
    assert wg <= BOUND * max(wc, FLOOR), (wg, wc)
