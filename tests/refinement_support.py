"""Test support for tests/test_gpu_refinement_branches.py: the four problems, their scaled cones and right-hand sides, handles of the
product on them and ONE CPU oracle per problem and static regulariser on the handles' own elimination order, whose solves are computed
once per (refinement options, right-hand side) and shared by the tests."""
import zlib

import numpy as np
import scipy.sparse as sp

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import problems
from clarabel_jl_amd.kktsolver import HipKKTSolver
from oracle.kkt_oracle import OracleKKTSolver
from tests.fixtures import scale_cones

PROBLEMS = {
    "plain": lambda: problems.random_sparse_qp(400, 700, 21, 3, 1),
    "portfolio_small": lambda: problems.portfolio_socp(n=300, nsoc=4, socdim=21, seed=3),    # a row beyond kLongRow: k_spmv_long
    "sdp_blocks": lambda: problems.sdp_blocks(n=300, ncones=8, dim=24, seed=7),              # dense triangles: k_spmv_dense_tri
    "cfg1": lambda: problems.random_sparse_qp(1000, 2000, 1, 4, 2),                          # front sweeps and segment sweeps
}
# static regulariser of the forced-step cases per problem: large enough that consecutive forced iterates up to three steps differ by
# 1e-6 max(1, |x|) on the oracle (System.assert_forced_iterates_differ)
FORCED_REG = {"plain": 1e-2, "portfolio_small": 1e-2, "sdp_blocks": 1e-2, "cfg1": 1e-2}
DEFAULT_REG = cl.Settings().static_regularization_constant


def forced(k, reg=1e-2, **kw):
    """exactly k refinement steps: no tolerance stops the loop, no ratio rejects a candidate"""
    return cl.Settings(static_regularization_constant=reg, iterative_refinement_reltol=0.0, iterative_refinement_abstol=0.0,
                       iterative_refinement_stop_ratio=0.0, iterative_refinement_max_iter=k, **kw)


def with_ir(reg=DEFAULT_REG, **kw):
    """Settings with the given refinement options under their short names (reltol, abstol, max_iter, stop_ratio, enable)"""
    return cl.Settings(static_regularization_constant=reg, **{"iterative_refinement_" + k: v for k, v in kw.items()})


def ir_key(st):
    return (st.iterative_refinement_enable, st.iterative_refinement_reltol, st.iterative_refinement_abstol,
            st.iterative_refinement_max_iter, st.iterative_refinement_stop_ratio)


def ir_kw(st):
    return dict(ir_enable=st.iterative_refinement_enable, reltol=st.iterative_refinement_reltol, abstol=st.iterative_refinement_abstol,
                max_iter=st.iterative_refinement_max_iter, stop_ratio=st.iterative_refinement_stop_ratio)


class System:
    def __init__(self, name, reg):
        self.name, self.reg = name, reg
        P, q, A, b, specs = PROBLEMS[name]()
        self.cones = cl.CompositeCone(cl.cones_new_collapsed(specs))
        self.Pt = sp.triu(sp.csc_matrix(P), format="csc")
        self.Pt.sort_indices()
        self.A = sp.csc_matrix(A)
        self.A.sort_indices()
        self.q, self.b = np.asarray(q, dtype=np.float64), np.asarray(b, dtype=np.float64)
        self.m, self.n = self.A.shape
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        scale_cones(self.cones, rng)
        self.rx, self.rz = rng.standard_normal((3, self.n)), rng.standard_normal((3, self.m))
        self.rng = rng
        self.perm = None
        self._oracle = None
        self._solves = {}
        self._K = None

    def handle(self, st=None):
        """a fresh handle, factorised with the system's static regulariser (st: its Settings; refinement options are per solve)"""
        st = st if st is not None else cl.Settings(static_regularization_constant=self.reg)
        assert st.static_regularization_constant == self.reg
        hk = HipKKTSolver(self.Pt, self.A, self.cones, self.m, self.n, st)
        assert hk.kktsolver_update(self.cones)
        if self.perm is None:
            self.perm = hk.h.perm()
        assert np.array_equal(hk.h.perm(), self.perm)          # (every handle on this pattern orders alike: one oracle serves them all)
        return hk

    def new_oracle(self, st=None):
        assert self.perm is not None, "build a handle first: the oracle runs on the handle's own elimination order"
        st = st if st is not None else cl.Settings(static_regularization_constant=self.reg)
        o = OracleKKTSolver(self.Pt, self.A, self.cones, self.m, self.n, st, ordering=self.perm)
        assert o.kktsolver_update(self.cones)
        return o

    def oracle_solve(self, st, rx, rz, key=None):
        """-> (x, z, steps, last_norms) of the oracle under st's refinement options; cached under key (with the options) if given"""
        assert st.static_regularization_constant == self.reg
        k = None if key is None else (ir_key(st), key)
        if k is not None and k in self._solves:
            return self._solves[k]
        if self._oracle is None:
            self._oracle = self.new_oracle()
        o = self._oracle
        o.settings = st                                          # (read by every solve; the factorisation used st's regulariser already)
        x, z = np.zeros(self.n), np.zeros(self.m)
        o.kktsolver_setrhs(np.ascontiguousarray(rx), np.ascontiguousarray(rz))
        assert o.kktsolver_solve(x, z)
        out = (x, z, o.last_ir_steps, o.last_norms.copy())
        if k is not None:
            self._solves[k] = out
        return out

    def assert_forced_iterates_differ(self):
        """the precondition of the forced-step cases, on the oracle alone: its iterates after 0, 1, 2, 3 steps differ pairwise by at least
        1e-6 max(1, |x|), i.e. 1e4 times the gate the device is held to -- a result with a step too few or too many cannot pass"""
        it = []
        for k in range(4):
            x, z, steps, _ = self.oracle_solve(forced(k, self.reg), self.rx[0], self.rz[0], key=0)
            assert steps == k
            it.append(np.concatenate([x, z]))
        scale = max(1.0, np.max(np.abs(it[3])))
        gaps = [float(np.max(np.abs(it[k + 1] - it[k]))) / scale for k in range(3)]
        assert min(gaps) >= 1e-6, (self.name, self.reg, gaps)
        return gaps

    def K(self, hk):
        """the unregularised K the handle holds as a full symmetric CSR matrix"""
        if self._K is None:
            colptr, rowval, nz = hk.h.kkt()
            N = hk.h.N
            U = sp.csc_matrix((nz, rowval, colptr), shape=(N, N))
            self._K = (U + sp.triu(U, 1).T).tocsr()
            self._K.sort_indices()
        return self._K


_SYSTEMS = {}


def system(name, reg=None):
    reg = FORCED_REG[name] if reg is None else reg
    if (name, reg) not in _SYSTEMS:
        _SYSTEMS[(name, reg)] = System(name, reg)
    return _SYSTEMS[(name, reg)]


def gpu_solve(hk, st, rx, rz):
    """setrhs + solve under st's refinement options -> (x, z, steps)"""
    hk.settings = st
    x, z = np.zeros(hk.n), np.zeros(hk.m)
    hk.kktsolver_setrhs(rx, rz)
    assert hk.kktsolver_solve(x, z)
    return x, z, hk.last_ir_steps


def deviation(x, z, xo, zo):
    """max |device - oracle| over max(1, |oracle|_inf)"""
    scale = max(1.0, np.max(np.abs(xo)), np.max(np.abs(zo)))
    return max(float(np.max(np.abs(x - xo))), float(np.max(np.abs(z - zo)))) / scale


def assert_decisive(norms, normb, st):
    """the precondition of the branch cases, on the oracle's residual norms alone (last_norms: the first residual's, then one per step):
    replaying kktsolver_directldl.jl:418-446, every ratio that decides a branch is a factor 1.5 away from 1 and from stop_ratio, and
    every norm that decides a tolerance test is a factor 2 away from the tolerance -- the device, whose sums associate differently,
    cannot take another branch.  -> the step count the replay arrives at"""
    _, reltol, abstol, max_iter, stop_ratio = ir_key(st)
    tol = abstol + reltol * normb

    def tolerance_met(v):
        assert tol == 0.0 or v >= 2.0 * tol or v <= 0.5 * tol, ("norm within a factor 2 of the tolerance", v, tol)
        return v <= tol

    last, steps = norms[0], 0
    while steps < max_iter and not tolerance_met(last):
        steps += 1
        v = norms[steps]
        ratio = last / v
        for ref in (1.0, stop_ratio):
            assert ref == 0.0 or ratio >= 1.5 * ref or ratio <= ref / 1.5, ("ratio within a factor 1.5 of a threshold", ratio, ref)
        if ratio < stop_ratio:
            break
        last = v
    assert steps == len(norms) - 1, (steps, norms)
    return steps
