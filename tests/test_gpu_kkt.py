"""GPU parity tests proper (-m gpu): every call goes through the C ABI of libclarabel_hipkkt.so and
is compared with the CPU oracle on identical inputs.

Tolerances (Float64, stated by north_star: residuals/objective to 1e-10):
  * integer structures (KKT pattern, LDLDataMap indices, Dsigns): bit-exact
  * LDL solve without refinement: ||x_gpu - x_cpu||_inf <= 1e-9 * max(1,||x||_inf)  (different
    elimination order => different rounding; conditioning of the regularised K enters)
  * solve WITH refinement (per kktsolver_solve! call), IPM residuals and objective: 1e-10
    (objective of the tiny reference fixtures: 1e-9, see test_ipm_known_answers_and_oracle_parity)
  * final IPM iterate x: 1e-6 * max(1,||x||_inf).  The IPM stops at tol 1e-8, so x itself is only
    determined to roughly that level: 1e-13-level rounding differences of the KKT solves (different
    elimination order on the GPU) are amplified by the barrier's conditioning near a cone boundary
    (observed 4e-9 on the reference's SOCP fixture while objective and residuals agree to 1e-12).
"""
X_TOL = 1e-6
import zlib

import os

import numpy as np
import pytest
import scipy.sparse as sp

import clarabel_jl_amd  # noqa: F401  (registers the dotted package directory)
import julia_standin as cl
from clarabel_jl_amd import hipkkt, problems
from clarabel_jl_amd.kktsolver import HipKKTSolver
from tests import fixtures as fx
from tests import soc_scaling_reference as ssr
from tests.fixtures import scale_cones as _scale_cones

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _front_batches_on_small_fronts(monkeypatch):
    """the problems of this file are small: let their fronts take the one-launch-per-update-batch factorisation (front_block.hip)
    that the product reserves for fronts of >= 1024 rows, so that it is covered here against the oracle as well"""
    if os.environ.get("HIPKKT_TEST_PRODUCTION", "0") != "1":   # (the production library has no switches: its own threshold applies)
        monkeypatch.setenv("HIPKKT_FRONT_BLOCK_MIN_ROWS", "0")

EPS2 = float(np.finfo(np.float64).eps) ** 2


def _prep(prob):
    P, q, A, b, specs = prob
    specs = cl.cones_new_collapsed(specs)
    cones = cl.CompositeCone(specs)
    Pt = sp.triu(sp.csc_matrix(P), format="csc")
    Pt.sort_indices()
    A = sp.csc_matrix(A)
    A.sort_indices()
    return Pt, A, cones




def test_mfma_layout_selftest():
    import ctypes as C

    err = C.c_double(-1)
    rc = hipkkt.lib().hipkkt_selftest_mfma(0, C.byref(err))
    assert rc == 0, f"f64 MFMA lane map mismatch, max err {err.value}"


PROBLEMS = {
    "qp_fixture": lambda: fx.basic_qp(),
    "socp_fixture": lambda: fx.basic_socp(),
    "sdp_fixture": lambda: fx.basic_sdp(),
    "lasso_sparse_soc": lambda: fx.lasso_socp(),
    "rand_uniform_300": lambda: problems.random_sparse_qp(300, 600, 11, 3, 1),
    "rand_window_2000": lambda: problems.random_sparse_qp(2000, 4000, 12, 4, 2, window=20),
    "cfg1": lambda: problems.random_sparse_qp(1000, 2000, 1, 4, 2),
    "portfolio_small": lambda: problems.portfolio_socp(n=300, nsoc=4, socdim=21, seed=3),
    "sdp_small": lambda: problems.sdp_blocks(n=60, ncones=3, dim=8, seed=5),
}


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_assembly_bit_exact_and_factor_solve_parity(name, oracle_factory):
    rng = np.random.default_rng(zlib.crc32(name.encode()))   # a fixed seed per case (str hashes vary per process)
    Pt, A, cones = _prep(PROBLEMS[name]())
    m, n = A.shape
    st = cl.Settings()
    hk = HipKKTSolver(Pt, A, cones, m, n, st)
    ok_ = oracle_factory(Pt, A, cones, m, n, st, ordering=hk.h.perm())   # same order => same flops
    o = ok_.k
    # ---- integer structures: bit exact
    colptr, rowval, nzval = hk.h.kkt()
    assert (hk.h.N, hk.h.p, hk.h.nnzK) == (o.N, o.p, o.nnzK)
    assert np.array_equal(colptr, o.colptr) and np.array_equal(rowval, o.rowval)
    assert np.array_equal(nzval, o.nzval)
    for w, nm in enumerate(["map_P", "map_A", "map_Hs", "map_diagP", "map_diag_full"]):
        assert np.array_equal(hk.h.map(w), o.map(nm)), nm
    assert np.array_equal(hk.h.dsigns(), o.map("dsigns"))
    for i in range(o.nsparse):
        for w in (0, 1, 3):
            assert np.array_equal(hk.h.sparse_map(i, w), o.sparse_map(i, w))
    assert hk.h.nnzL == o.nnzL
    # ---- update + factor + solve, three different scalings
    for rep in range(3):
        if rep == 0:
            cones.set_identity_scaling()
        else:
            _scale_cones(cones, rng)
        assert hk.kktsolver_update(cones)
        assert ok_.kktsolver_update(cones)
        assert abs(hk.diagonal_regularizer - ok_.diagonal_regularizer) <= 1e-16 * max(1.0, ok_.diagonal_regularizer)
        assert hk.last_nreg == o.L.oracle_kkt_nreg(o.h)
        _, _, kv = hk.h.kkt()
        assert np.array_equal(kv, o.nzval)               # resident K == oracle's K, bit for bit
        b = rng.standard_normal(o.N)
        xg = hk.h.ldl_solve(b)
        xc = o.ldl_solve(b)
        assert np.max(np.abs(xg - xc)) <= 1e-9 * max(1.0, np.max(np.abs(xc)))
        # refined solve through the L1 calls
        rx, rz = rng.standard_normal(n), rng.standard_normal(m)
        lx_g, lz_g, lx_c, lz_c = np.zeros(n), np.zeros(m), np.zeros(n), np.zeros(m)
        hk.kktsolver_setrhs(rx, rz)
        ok_.kktsolver_setrhs(rx, rz)
        assert hk.kktsolver_solve(lx_g, lz_g) and ok_.kktsolver_solve(lx_c, lz_c)
        scale = max(1.0, np.max(np.abs(lx_c)), np.max(np.abs(lz_c)))
        assert np.max(np.abs(lx_g - lx_c)) <= 1e-10 * scale
        assert np.max(np.abs(lz_g - lz_c)) <= 1e-10 * scale
        # the refined solution satisfies the reference's own stopping rule against the TRUE K
        res = np.concatenate([rx, rz, np.zeros(o.p)]) - o.symv(np.concatenate([lx_g, lz_g, np.zeros(o.p)]))
        if o.p == 0:
            assert np.max(np.abs(res)) <= 1e-9 * max(1.0, np.max(np.abs(np.concatenate([rx, rz]))))


@pytest.mark.parametrize("policy,maxw", [(1, 64), (0, 16), (0, 1), (2, 64), (2, 5)])
def test_plan_variants_agree(policy, maxw, oracle_factory):
    rng = np.random.default_rng(77)
    Pt, A, cones = _prep(problems.random_sparse_qp(400, 700, 21, 3, 1))
    m, n = A.shape
    st = cl.Settings()
    hk = HipKKTSolver(Pt, A, cones, m, n, st, update_policy=policy, supernode_max_width=maxw)
    ok_ = oracle_factory(Pt, A, cones, m, n, st, ordering=hk.h.perm())
    _scale_cones(cones, rng)
    assert hk.kktsolver_update(cones) and ok_.kktsolver_update(cones)
    b = rng.standard_normal(hk.h.N)
    xg, xc = hk.h.ldl_solve(b), ok_.k.ldl_solve(b)
    assert np.max(np.abs(xg - xc)) <= 1e-9 * max(1.0, np.max(np.abs(xc)))


# Alternative code paths selected by developer switches (read when a handle is created): every one must give the same
# answers as the default path.  cfg1-sized problem: a root front (persistent front sweeps, just-in-time updates),
# thousands of narrow leaves, segment sweeps.
@pytest.mark.parametrize("env", [
    {"HIPKKT_NO_GRAPH": "1"},
    {"HIPKKT_NO_PERSIST": "1"},
    {"HIPKKT_NO_FRONT": "1"},
    {"HIPKKT_FB_STREAM": "0", "HIPKKT_FRONT_BLOCK_MIN_ROWS": "0"},
    {"HIPKKT_FB_V2": "0", "HIPKKT_FRONT_BLOCK_MIN_ROWS": "0"},
    {"HIPKKT_ACCURATE": "-1"},       # every factorisation's solves in the accurate mode (per-level kernels + refined block solves)
    {"HIPKKT_FRONT_BLOCK_MIN_ROWS": "0"},
    {"HIPKKT_ORDERING": "amd"},
    {"HIPKKT_FRONT_BLOCK": "0"},
])
def test_developer_switches_keep_parity(env, oracle_factory, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(5)
    Pt, A, cones = _prep(problems.random_sparse_qp(1000, 2000, 1, 4, 2))
    m, n = A.shape
    st = cl.Settings()
    hk = HipKKTSolver(Pt, A, cones, m, n, st)
    ok_ = oracle_factory(Pt, A, cones, m, n, st, ordering=hk.h.perm())
    for rep in range(2):
        _scale_cones(cones, rng)
        assert hk.kktsolver_update(cones) and ok_.kktsolver_update(cones)
        b = rng.standard_normal(hk.h.N)
        xg, xc = hk.h.ldl_solve(b), ok_.k.ldl_solve(b)
        assert np.max(np.abs(xg - xc)) <= 1e-9 * max(1.0, np.max(np.abs(xc)))
        rx, rz = rng.standard_normal(n), rng.standard_normal(m)
        lx_g, lz_g, lx_c, lz_c = np.zeros(n), np.zeros(m), np.zeros(n), np.zeros(m)
        hk.kktsolver_setrhs(rx, rz)
        ok_.kktsolver_setrhs(rx, rz)
        assert hk.kktsolver_solve(lx_g, lz_g) and ok_.kktsolver_solve(lx_c, lz_c)
        scale = max(1.0, np.max(np.abs(lx_c)), np.max(np.abs(lz_c)))
        assert np.max(np.abs(lx_g - lx_c)) <= 1e-10 * scale and np.max(np.abs(lz_g - lz_c)) <= 1e-10 * scale


# SURVEY section 8(f) row N4 (building block): Px, A'z, Ax of residuals_update! from the resident values, also after
# kktsolver_update_P! / update_A!
@pytest.mark.parametrize("name", ["qp_fixture", "rand_uniform_300", "portfolio_small", "sdp_small"])
def test_block_products_match_scipy(name):
    rng = np.random.default_rng(3)
    Pt, A, cones = _prep(PROBLEMS[name]())
    m, n = A.shape
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    for rep in range(2):
        if rep == 1:   # new values on the same pattern
            Pt = Pt.copy(); Pt.data = Pt.data * (1.0 + 0.1 * rng.random(Pt.nnz))
            A = A.copy(); A.data = A.data * (1.0 + 0.1 * rng.random(A.nnz))
            hk.kktsolver_update_P(Pt)
            hk.kktsolver_update_A(A)
        x, z = rng.standard_normal(n), rng.standard_normal(m)
        Px, ATz, Ax = hk.h.block_products(x, z)
        Pfull = Pt + sp.triu(Pt, 1).T
        for got, ref in ((Px, Pfull @ x), (ATz, A.T @ z), (Ax, A @ x)):
            assert np.max(np.abs(got - ref)) <= 1e-13 * max(1.0, np.max(np.abs(ref)))


def test_plan_statistics_tables_are_consistent():
    """hipkkt_debug_dump 20 / 21 (development tables behind tools/dense_stage_stats.py): six values per dense update tile, five per
    supernode of the persistent segment sweeps; checked against the plan tables 10 - 14 of the same handle."""
    Pt, A, cones = _prep(problems.random_sparse_qp(1000, 2000, 1, 4, 2))
    m, n = A.shape
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    tiles = hk.h.debug_dump(20)
    assert tiles.size % 6 == 0 and tiles.size > 0
    tiles = tiles.reshape(-1, 6)
    levels = hk.h.debug_dump(11)
    assert np.all(tiles[:, 0] >= 0) and np.all(tiles[:, 0] <= levels.max())          # stage = a level of the tree
    assert np.all(tiles[:, 1] >= 1) and np.all(tiles[:, 2] >= tiles[:, 1])           # >= 1 contribution, each >= 1 column wide
    assert np.all(tiles[:, 3] <= tiles[:, 1]) and np.all((tiles[:, 4] == 0) | (tiles[:, 4] == 1))
    assert np.all(tiles[:, 5] <= 4096 * tiles[:, 2])                                 # rows x columns x width <= a full tile per column
    seg = hk.h.debug_dump(21)
    assert seg.size % 5 == 0
    seg = seg.reshape(-1, 5)
    member = hk.h.debug_dump(14)
    assert len(seg) == int(member.sum())
    first, rows = hk.h.debug_dump(10), hk.h.debug_dump(12)
    idx = np.nonzero(member)[0]
    assert np.array_equal(seg[:, 0], levels[idx]) and np.array_equal(seg[:, 1], np.diff(first)[idx]) and np.array_equal(seg[:, 2], rows[idx])
    assert np.all(seg[:, 3] >= seg[:, 4] - 1e-12)                                    # longest list >= mean list


def test_l0_seam_matches_oracle(oracle_factory):
    """AbstractDirectLDLSolver seam: create from an assembled KKT, update_values / scale_values /
    refactor / solve (directldl_qdldl.jl call pattern)."""
    rng = np.random.default_rng(3)
    Pt, A, cones = _prep(problems.random_sparse_qp(150, 260, 5, 3, 1))
    m, n = A.shape
    st = cl.Settings()
    o = oracle_factory(Pt, A, cones, m, n, st).k
    h = hipkkt.Handle.from_kkt(o.colptr, o.rowval, o.nzval, o.map("dsigns"))
    o.symbolic(h.perm())
    hsmap = o.map("map_Hs")
    vals = -(rng.random(len(hsmap)) + 0.3)
    h.update_values(hsmap, vals)
    o.L.oracle_kkt_update_values(o.h, hsmap, vals, len(hsmap))
    h.scale_values(hsmap[:50], 1.7)
    o.L.oracle_kkt_scale_values(o.h, hsmap[:50], 50, 1.7)
    okg, epsg, _ = h.refactor(True, 1e-8, EPS2)
    import ctypes as C
    eps = C.c_double(0)
    assert o.L.oracle_kkt_regularize_and_refactor(o.h, 1, 1e-8, EPS2, C.byref(eps)) and okg
    assert abs(eps.value - epsg) < 1e-20
    b = rng.standard_normal(o.N)
    xg, xc = h.ldl_solve(b), o.ldl_solve(b)
    assert np.max(np.abs(xg - xc)) <= 1e-9 * max(1.0, np.max(np.abs(xc)))
    h.close()


def test_failure_semantics():
    """non-finite pivot -> refactor reports numerical failure (Julia `false`), never throws"""
    Pt, A, cones = _prep(fx.basic_qp())
    m, n = A.shape
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    cones.set_identity_scaling()
    hk.Hsblocks[:] = np.nan
    hk.h.set_hs(hk.Hsblocks)
    ok, _, _ = hk.h.refactor(True, 1e-8, EPS2)
    assert not ok
    with pytest.raises(hipkkt.HipKKTError):
        hk.h.set_hs(np.zeros(3))     # wrong length -> usage error (<0)


GOLDEN = [
    ("qp", fx.basic_qp, "SOLVED", [0.3, 0.7], 1.88),
    ("lp", fx.basic_lp, "SOLVED", [-0.5, 0.5, -0.5], -3.0),
    ("eq", lambda: fx.eq_constrained(2), "SOLVED", [10 / 6, 1 / 6, 1 / 6], None),
    ("unc", fx.unconstrained, "SOLVED", [-1.0, -2.0, 3.0], None),
    ("socp", fx.basic_socp, "SOLVED", [-0.5, 0.435603, -0.245459], -0.84590),
    ("sdp", fx.basic_sdp, "SOLVED", [-3.0729833267361095, 0.3696004167288786, -0.022226685581313674,
                                     0.31441213129613066, -0.026739700851545107, -0.016084530571308823], 4.840076866013861),
    ("lasso", fx.lasso_socp, "SOLVED", None, None),
]


@pytest.mark.parametrize("name,mk,status,xref,obj", GOLDEN)
def test_ipm_known_answers_and_oracle_parity(name, mk, status, xref, obj, oracle_factory):
    """test/OptTests/linear_solvers.jl:11-71 with `:hip` added to the solver list, plus 1e-10
    parity with the oracle-driven run on the same data."""
    P, q, A, b, cones = mk()
    sg = cl.Solver(P, q, A, b, cones, cl.Settings())
    solg = sg.solve()
    assert solg.status == status
    if xref is not None:
        assert np.linalg.norm(solg.x - xref) < 1e-3     # the reference's own tolerance
    if obj is not None:
        assert abs(solg.obj_val - obj) < 1e-3
    perm = sg.kktsystem.kktsolver.h.perm()
    sc = cl.Solver(P, q, A, b, cones, cl.Settings(),
                   kktsolver_factory=lambda *a: oracle_factory(*a, ordering=perm))
    solc = sc.solve()
    assert solc.status == solg.status
    assert solc.iterations == solg.iterations
    assert np.max(np.abs(solg.x - solc.x)) <= X_TOL * max(1.0, np.max(np.abs(solc.x)))
    # residuals: 1e-10 (north_star).  Objective: the two runs stop at the same iteration with iterates that
    # differ in the digits the IPM has not converged yet (|dx| up to 2e-8 on the SOCP fixture, whose optimum
    # sits on the cone boundary), so the objective agrees to ~|q|.|dx|: held to 1e-9 here (measured 1.0e-10
    # on that fixture, <= 1e-12 on the others); the well-conditioned medium problems below keep 1e-10.
    assert abs(solg.obj_val - solc.obj_val) <= 1e-9 * max(1.0, abs(solc.obj_val))
    assert abs(solg.r_prim - solc.r_prim) <= 1e-10 and abs(solg.r_dual - solc.r_dual) <= 1e-10


def test_ipm_infeasible_statuses():
    P, c, A, b, cones = fx.basic_qp()
    b[0] = b[3] = -1.0
    assert cl.Solver(P, c, A, b, cones).solve().status == "PRIMAL_INFEASIBLE"
    assert cl.Solver(*fx.basic_qp_dualinf()).solve().status == "DUAL_INFEASIBLE"


def test_data_updating(oracle_factory):
    """data_updating.jl (tol 1e-7): re-solve after update_P!/update_A! == fresh solve"""
    P, q, A, b, cones = fx.updating_data()
    s1 = cl.Solver(P, q, A, b, cones)
    s1.solve()
    P2 = P.tolil()
    P2[0, 0] = 100.0
    P2 = sp.csc_matrix(P2)
    s1.update_P(sp.triu(P2, format="csc").data)
    A2 = A.copy()
    A2.data[1] = -1000.0
    s1.update_A(A2.data)
    x1 = s1.solve().x
    x2 = cl.Solver(P2, q, A2, b, cones).solve().x
    assert np.linalg.norm(x1 - x2) < 1e-7


@pytest.mark.parametrize("name", ["cfg1", "rand_window_2000", "portfolio_small", "sdp_small"])
def test_ipm_parity_medium(name, oracle_factory):
    P, q, A, b, cones = PROBLEMS[name]()
    sg = cl.Solver(P, q, A, b, cones, cl.Settings())
    solg = sg.solve()
    assert solg.status == "SOLVED"
    perm = sg.kktsystem.kktsolver.h.perm()
    sc = cl.Solver(P, q, A, b, cones, cl.Settings(), kktsolver_factory=lambda *a: oracle_factory(*a, ordering=perm))
    solc = sc.solve()
    assert solc.status == "SOLVED" and solc.iterations == solg.iterations
    assert np.max(np.abs(solg.x - solc.x)) <= X_TOL * max(1.0, np.max(np.abs(solc.x)))
    # 1e-10, plus what the reference path ITSELF moves by when only the elimination order changes (oracle on its own
    # MMD order vs oracle in the product's order): 0 to 1e-14 for cfg1 / rand_window / portfolio; ~1e-9 for sdp_small, whose
    # last iterations are decided by digits no LDL^T implementation reproduces (measured CPU vs CPU)
    soln = cl.Solver(P, q, A, b, cones, cl.Settings(), kktsolver_factory=lambda *a: oracle_factory(*a, ordering="mmd")).solve()
    spread_obj = abs(solc.obj_val - soln.obj_val) / max(1.0, abs(solc.obj_val)) if soln.iterations == solc.iterations else 0.0
    spread_res = max(abs(solc.r_prim - soln.r_prim), abs(solc.r_dual - soln.r_dual)) if soln.iterations == solc.iterations else 0.0
    if name != "sdp_small":
        assert spread_obj <= 1e-12 and spread_res <= 1e-12      # the allowance is only ever used by the degenerate SDP
    assert abs(solg.obj_val - solc.obj_val) <= (1e-10 + 4.0 * spread_obj) * max(1.0, abs(solc.obj_val))
    assert abs(solg.r_prim - solc.r_prim) <= 1e-10 + 4.0 * spread_res and abs(solg.r_dual - solc.r_dual) <= 1e-10 + 4.0 * spread_res


def test_genpow_and_soc_expansion_maps_through_the_abi():
    """GenPowExpansionMap (directldl_datamaps.jl:81-167) next to an SOC expansion, driven through the C ABI:
    hipkkt_create_from_parts(sparse_kind = 2) must produce the oracle's image and maps bit for bit (the oracle's
    GenPow layout is pinned by hand in tests/test_oracle_layers.py), hipkkt_set_genpow must write what
    _csc_update_sparsecone(::GenPowerCone) writes, and the factorisation of the resulting quasi-definite K
    (Dsigns (-1,-1,+1) on the three extra columns) must solve like the oracle's."""
    from oracle.kkt_oracle import OracleKKT
    import ctypes as C

    rng = np.random.default_rng(2024)
    n = 30
    numel = np.array([5, 5, 6, 6])
    hs_dense = np.zeros(4, dtype=np.int32)
    sparse_kind = np.array([0, 2, 1, 2], dtype=np.int32)     # NN, GenPow(3+2), SOC(6), GenPow(2+4)
    dim1 = np.array([0, 3, 0, 2])
    m = int(numel.sum())
    S = sp.random(n, n, density=0.08, random_state=np.random.RandomState(5), format="csc")
    Pt = sp.triu(S + S.T + sp.diags(np.asarray(abs(S + S.T).sum(axis=1)).ravel() + 0.5), format="csc")
    Pt.sort_indices()
    A = sp.random(m, n, density=0.15, random_state=np.random.RandomState(6), format="csc")
    A.sort_indices()
    h = hipkkt.Handle.from_parts(Pt, A, numel, hs_dense, sparse_kind, dim1)
    o = OracleKKT(Pt, A, numel, hs_dense, sparse_kind, dim1)
    assert (h.N, h.p, h.nnzK, h.nsparse) == (o.N, o.p, o.nnzK, o.nsparse) == (n + m + 8, 8, o.nnzK, 3)
    colptr, rowval, nzval = h.kkt()
    assert np.array_equal(colptr, o.colptr) and np.array_equal(rowval, o.rowval) and np.array_equal(nzval, o.nzval)
    for w, nm in enumerate(["map_P", "map_A", "map_Hs", "map_diagP", "map_diag_full"]):
        assert np.array_equal(h.map(w), o.map(nm)), nm
    assert np.array_equal(h.dsigns(), o.map("dsigns"))
    assert list(h.dsigns()[n + m:]) == [-1, -1, 1, -1, 1, -1, -1, 1]       # GenPow, SOC, GenPow
    for i in range(3):
        for w in range(4):
            assert np.array_equal(h.sparse_map(i, w), o.sparse_map(i, w)), (i, w)
    o.symbolic(h.perm())
    for rep in range(2):
        hs = rng.random(h.nHs) + 0.5
        h.set_hs(hs)
        o.L.oracle_kkt_update_Hs(o.h, hs)
        for i, (k, d1, ne) in enumerate([(2, 3, 5), (1, 0, 6), (2, 2, 6)]):
            if k == 2:
                # like the cone's own data (coneops_genpowcone.jl:91-108): Hs + mu (p p' - q q' - r r') stays positive definite,
                # i.e. the expanded K is quasi-definite with the signs (-1,-1,+1)
                pv, qv, rv = rng.standard_normal(ne), 0.15 * rng.standard_normal(d1), 0.15 * rng.standard_normal(ne - d1)
                sq = float(np.sqrt(rng.random() + 0.1))
                h.set_genpow(i, sq, pv, qv, rv)
                o.L.oracle_kkt_update_genpow(o.h, i, sq, pv, qv, rv)
            else:
                u, v, eta2 = 0.3 * rng.standard_normal(ne), 0.3 * rng.standard_normal(ne), float(rng.random() + 0.5)
                h.set_soc(i, eta2, u, v)
                o.L.oracle_kkt_update_soc(o.h, i, eta2, u, v)
        assert np.array_equal(h.kkt()[2], o.nzval)
        okg, epsg, nregg = h.refactor(True, 1e-8, EPS2)
        eps = C.c_double(0)
        assert o.L.oracle_kkt_regularize_and_refactor(o.h, 1, 1e-8, EPS2, C.byref(eps)) and okg
        assert abs(eps.value - epsg) <= 1e-16 * max(1.0, eps.value) and nregg == o.L.oracle_kkt_nreg(o.h)
        b = rng.standard_normal(o.N)
        xg, xc = h.ldl_solve(b), o.ldl_solve(b)
        assert np.max(np.abs(xg - xc)) <= 1e-9 * max(1.0, np.max(np.abs(xc)))
    with pytest.raises(hipkkt.HipKKTError):
        h.set_genpow(1, 1.0, np.zeros(6), np.zeros(2), np.zeros(4))          # map 1 is the SOC
    h.close()


# ---- parity with the oracle on ITS OWN fill-reducing order (north_star: results match the reference's QDLDL path, which
# orders with SuiteSparse AMD; here: SuperLU's MMD on K, independent of the product's ordering code).  Different
# elimination orders change the rounding of every solve and which pivots the dynamic regulariser touches, so what is
# compared is what the caller sees: refined solves, and the IPM's iterations / objective / residuals.
ORDER_CASES = {
    "nn_cfg1": lambda: problems.random_sparse_qp(1000, 2000, 1, 4, 2),
    "nn_window_2000": lambda: problems.random_sparse_qp(2000, 4000, 12, 4, 2, window=20),
    "soc_portfolio_small": lambda: problems.portfolio_socp(n=300, nsoc=4, socdim=21, seed=3),
    "soc_lasso": lambda: fx.lasso_socp(),
    "psd_sdp_small": lambda: problems.sdp_blocks(n=60, ncones=3, dim=8, seed=5),
    "psd_sdp_fixture": lambda: fx.basic_sdp(),
}


@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_refined_solve_matches_oracle_on_its_own_ordering(name, oracle_factory):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    Pt, A, cones = _prep(ORDER_CASES[name]())
    m, n = A.shape
    st = cl.Settings()
    hk = HipKKTSolver(Pt, A, cones, m, n, st)
    ok_ = oracle_factory(Pt, A, cones, m, n, st, ordering="mmd")
    assert not np.array_equal(hk.h.perm(), ok_.k._perm)            # really two different elimination orders
    for rep in range(2):
        _scale_cones(cones, rng)
        assert hk.kktsolver_update(cones) and ok_.kktsolver_update(cones)
        assert abs(hk.diagonal_regularizer - ok_.diagonal_regularizer) <= 1e-16 * max(1.0, ok_.diagonal_regularizer)
        rx, rz = rng.standard_normal(n), rng.standard_normal(m)
        lx_g, lz_g, lx_c, lz_c = np.zeros(n), np.zeros(m), np.zeros(n), np.zeros(m)
        hk.kktsolver_setrhs(rx, rz)
        ok_.kktsolver_setrhs(rx, rz)
        assert hk.kktsolver_solve(lx_g, lz_g) and ok_.kktsolver_solve(lx_c, lz_c)
        scale = max(1.0, np.max(np.abs(lx_c)), np.max(np.abs(lz_c)))
        assert np.max(np.abs(lx_g - lx_c)) <= 1e-10 * scale and np.max(np.abs(lz_g - lz_c)) <= 1e-10 * scale


@pytest.mark.parametrize("name", list(ORDER_CASES))
def test_ipm_matches_oracle_on_its_own_ordering(name, oracle_factory, capsys):
    """BASELINE.md parity gate: iterations equal (or +-1 with the cause logged), objective and residuals to 1e-10.
    The gate is applied relative to what the reference path ITSELF shows between two elimination orders: the oracle is
    also run on a second order (the product's) and its own ordering spread is added to the 1e-10 (measured here on the CPU: <= 1e-14
    for the NN / SOC families, 1e-9 on the objective of sdp_small, whose optimum is degenerate -- no LDL^T
    implementation, the reference's included, reproduces those digits across orderings)."""
    P, q, A, b, cones = ORDER_CASES[name]()
    sg = cl.Solver(P, q, A, b, cones, cl.Settings())
    solg = sg.solve()
    perm = sg.kktsystem.kktsolver.h.perm()
    solc = cl.Solver(P, q, A, b, cones, cl.Settings(), kktsolver_factory=lambda *a: oracle_factory(*a, ordering="mmd")).solve()
    soln = cl.Solver(P, q, A, b, cones, cl.Settings(), kktsolver_factory=lambda *a: oracle_factory(*a, ordering=perm)).solve()
    assert solg.status == solc.status == "SOLVED"
    spread_obj = abs(solc.obj_val - soln.obj_val) / max(1.0, abs(solc.obj_val))
    spread_res = max(abs(solc.r_prim - soln.r_prim), abs(solc.r_dual - soln.r_dual))
    dobj = abs(solg.obj_val - solc.obj_val) / max(1.0, abs(solc.obj_val))
    dres = max(abs(solg.r_prim - solc.r_prim), abs(solg.r_dual - solc.r_dual))
    with capsys.disabled():
        print(f"\n[order-parity {name}] iterations hip/oracle(mmd)/oracle(product's order) = {solg.iterations}/{solc.iterations}/"
              f"{soln.iterations}; |dobj| hip-oracle {dobj:.2e} (oracle's own ordering spread {spread_obj:.2e}); "
              f"|dres| {dres:.2e} (spread {spread_res:.2e})")
    assert abs(solg.iterations - solc.iterations) <= 1
    if solg.iterations != solc.iterations:   # cause: a step-length / termination test decided by digits below 1e-10
        assert abs(solc.iterations - soln.iterations) <= 1
        return
    assert dobj <= 1e-10 + 4.0 * spread_obj
    assert dres <= 1e-10 + 4.0 * spread_res


def test_sweep_timeout_recovers_with_oracle_equal_results(oracle_factory, monkeypatch, capfd):
    """A persistent sweep that times out (forced here with a spin bound of zero polls: every hand-off that is not
    satisfied at once gives up) must fail the solve internally, re-arm, repeat it on the per-level kernels and return
    oracle-equal results; the downgrade is temporary (persistent kernels are retried after HIPKKT_PERSIST_RETRY solves)."""
    monkeypatch.setenv("HIPKKT_SPIN_LIMIT", "0")
    monkeypatch.setenv("HIPKKT_PERSIST_RETRY", "3")
    rng = np.random.default_rng(9)
    Pt, A, cones = _prep(problems.random_sparse_qp(1000, 2000, 1, 4, 2))
    m, n = A.shape
    st = cl.Settings()
    hk = HipKKTSolver(Pt, A, cones, m, n, st)
    ok_ = oracle_factory(Pt, A, cones, m, n, st, ordering=hk.h.perm())
    assert hk.h.counters()["persistent"] and hk.h.counters()["fronts"] >= 1
    assert hk.h.counters()["front_batches"] >= 1 and hk.h.counters()["front_block"]
    _scale_cones(cones, rng)
    assert hk.kktsolver_update(cones) and ok_.kktsolver_update(cones)
    # the front-batch factorisation kernel (front_block.hip) shares the spin bound: its first hand-off gave up, the factorisation
    # was repeated with one launch per panel and the handle keeps that path
    assert not hk.h.counters()["front_block"] and hk.h.counters()["sweep_timeouts"] >= 1
    for rep in range(8):
        b = rng.standard_normal(hk.h.N)
        xg, xc = hk.h.ldl_solve(b), ok_.k.ldl_solve(b)
        assert np.max(np.abs(xg - xc)) <= 1e-9 * max(1.0, np.max(np.abs(xc)))
    c = hk.h.counters()
    assert c["sweep_timeouts"] >= 2, c        # timed out, fell back, retried the persistent kernels, timed out again
    rx, rz = rng.standard_normal(n), rng.standard_normal(m)
    lx_g, lz_g, lx_c, lz_c = np.zeros(n), np.zeros(m), np.zeros(n), np.zeros(m)
    hk.kktsolver_setrhs(rx, rz)
    ok_.kktsolver_setrhs(rx, rz)
    assert hk.kktsolver_solve(lx_g, lz_g) and ok_.kktsolver_solve(lx_c, lz_c)
    scale = max(1.0, np.max(np.abs(lx_c)), np.max(np.abs(lz_c)))
    assert np.max(np.abs(lx_g - lx_c)) <= 1e-10 * scale and np.max(np.abs(lz_g - lz_c)) <= 1e-10 * scale
    err_text = capfd.readouterr().err
    assert "timed out" in err_text and "front-batch factorisation timed out" in err_text


def test_output_arrays_are_validated():
    Pt, A, cones = _prep(fx.basic_qp())
    m, n = A.shape
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    cones.set_identity_scaling()
    assert hk.kktsolver_update(cones)
    hk.kktsolver_setrhs(np.ones(n), np.ones(m))
    for bad in (np.zeros(n, dtype=np.float32), np.zeros(2 * n)[::2], np.zeros(max(n - 1, 0))):
        with pytest.raises(hipkkt.HipKKTError):
            hk.h.solve(bad, np.zeros(m))


@pytest.mark.parametrize("name", ["cfg1", "portfolio_small", "sdp_small", "rand_window_2000"])
def test_solve_multi_matches_separate_solves(name, oracle_factory):
    """hipkkt_solve_multi solves its right-hand sides on concurrent device contexts; every one must
    be BIT-IDENTICAL to what a separate kktsolver_setrhs! / kktsolver_solve! pair returns (same kernels, same order of
    operations, private work areas) and match the oracle's separate solves to 1e-10.  Three right-hand sides = two rounds
    (2 concurrent + 1)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    Pt, A, cones = _prep(PROBLEMS[name]())
    m, n = A.shape
    st = cl.Settings()
    hk = HipKKTSolver(Pt, A, cones, m, n, st)
    ok_ = oracle_factory(Pt, A, cones, m, n, st, ordering=hk.h.perm())
    for rep in range(2):
        _scale_cones(cones, rng)
        assert hk.kktsolver_update(cones) and ok_.kktsolver_update(cones)
        rx, rz = rng.standard_normal((3, n)), rng.standard_normal((3, m))
        lx, lz = np.zeros((3, n)), np.zeros((3, m))
        assert hk.kktsolver_solve_multi(rx, rz, lx, lz)
        for k in range(3):
            sx, sz, cx, cz = np.zeros(n), np.zeros(m), np.zeros(n), np.zeros(m)
            hk.kktsolver_setrhs(rx[k], rz[k])
            assert hk.kktsolver_solve(sx, sz)
            assert np.array_equal(sx, lx[k]) and np.array_equal(sz, lz[k])
            ok_.kktsolver_setrhs(rx[k], rz[k])
            assert ok_.kktsolver_solve(cx, cz)
            scale = max(1.0, np.max(np.abs(cx)), np.max(np.abs(cz)))
            assert np.max(np.abs(lx[k] - cx)) <= 1e-10 * scale and np.max(np.abs(lz[k] - cz)) <= 1e-10 * scale


def test_refinement_steps_match_oracle_on_a_hard_system(oracle_factory):
    """the device-side replay of _iterative_refinement's branches (kktsolver_directldl.jl:418-446): on a badly scaled
    system the number of refinement steps and the accepted iterate must be the oracle's"""
    rng = np.random.default_rng(31)
    Pt, A, cones = _prep(problems.random_sparse_qp(400, 700, 21, 3, 1))
    m, n = A.shape
    st = cl.Settings()
    hk = HipKKTSolver(Pt, A, cones, m, n, st)
    ok_ = oracle_factory(Pt, A, cones, m, n, st, ordering=hk.h.perm())
    s, z = rng.random(m) * 1e-7 + 1e-9, rng.random(m) + 0.1        # late-IPM scaling: Hs = s/z spans many decades
    s[::3] = rng.random(len(s[::3])) * 1e3
    assert cones.update_scaling(s, z, 1.0)
    assert hk.kktsolver_update(cones) and ok_.kktsolver_update(cones)
    seen = set()
    for rep in range(6):
        rx, rz = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4), rng.standard_normal(m) * 10.0 ** rng.integers(-3, 4)
        lx_g, lz_g, lx_c, lz_c = np.zeros(n), np.zeros(m), np.zeros(n), np.zeros(m)
        hk.kktsolver_setrhs(rx, rz)
        ok_.kktsolver_setrhs(rx, rz)
        assert hk.kktsolver_solve(lx_g, lz_g) and ok_.kktsolver_solve(lx_c, lz_c)
        seen.add(ok_.last_ir_steps)
        assert abs(hk.last_ir_steps - ok_.last_ir_steps) <= 1      # a stopping test decided by the last digits of a norm may differ
        scale = max(1.0, np.max(np.abs(lx_c)), np.max(np.abs(lz_c)))
        assert np.max(np.abs(lx_g - lx_c)) <= 1e-9 * scale and np.max(np.abs(lz_g - lz_c)) <= 1e-9 * scale
    print("refinement steps seen on the oracle:", sorted(seen))
    assert max(seen) >= 2          # (the oracle takes 1, 1, 2, 1, 2, 1 steps on these six: the loop beyond the first step runs)


@pytest.mark.parametrize("name", ["qp_fixture", "cfg1", "portfolio_small", "sdp_small"])
def test_residuals_update_on_device(name):
    """residuals_update! (residuals.jl:1-37) from the resident P, A against the numpy caller's own
    (1e-13 relative; the dot products are summed in a different but fixed order), also after update_P!/update_A!, and the
    whole IPM driven with device residuals reaches the same answer as with host residuals."""
    rng = np.random.default_rng(17)
    P, q, A, b, cones = PROBLEMS[name]()
    ref = cl.Solver(P, q, A, b, cones, cl.Settings())
    dev = cl.Solver(P, q, A, b, cones, cl.Settings(device_residuals=True))
    assert dev._device_residuals
    for rep in range(2):
        for S in (ref, dev):
            v = S.variables
            v.x[:], v.z[:], v.s[:] = rng.standard_normal(v.x.size), rng.random(v.z.size), rng.random(v.s.size)
            v.tau, v.kappa = 0.7 + rep, 0.3
        dev.variables.x[:], dev.variables.z[:], dev.variables.s[:] = ref.variables.x, ref.variables.z, ref.variables.s
        ref._residuals_update()
        dev._residuals_update()
        for nm in ("rx", "rz", "rx_inf", "rz_inf", "Px"):
            a, c = getattr(dev.residuals, nm), getattr(ref.residuals, nm)
            assert np.max(np.abs(a - c)) <= 1e-13 * max(1.0, np.max(np.abs(c))), nm
        for nm in ("dot_qx", "dot_bz", "dot_sz", "dot_xPx", "rtau"):
            a, c = getattr(dev.residuals, nm), getattr(ref.residuals, nm)
            assert abs(a - c) <= 1e-12 * max(1.0, abs(c)), nm
        if rep == 0:      # new values on the same pattern: the device products follow kktsolver_update_P!/A!
            Pt = sp.triu(sp.csc_matrix(P), format="csc")
            for S in (ref, dev):
                S.update_P(Pt.data * 1.25)
                S.update_A(sp.csc_matrix(A).data * 0.75)
    solr = cl.Solver(P, q, A, b, cones, cl.Settings()).solve()
    sold = cl.Solver(P, q, A, b, cones, cl.Settings(device_residuals=True)).solve()
    assert solr.status == sold.status == "SOLVED" and abs(solr.iterations - sold.iterations) <= 1
    assert abs(solr.obj_val - sold.obj_val) <= 1e-7 * max(1.0, abs(solr.obj_val))


@pytest.mark.parametrize("name", ["qp_fixture", "lp_like", "cfg1", "portfolio_small", "sdp_small"])
def test_kkt_solve_reduced_on_device(name):
    """SURVEY section 8(f) row N2, second half: kkt_solve! (kktsystem.jl:135-215) between the caller's cone algebra and mul_Hs! done
    by the plugin (hipkkt_kkt_solve_reduced): the seven dot products / quadratic forms against numpy on the very same (x1, z1),
    (x2, z2) to 1e-13 of their term sums (fixed but different summation order), d tau, dx, dz from them, first with the pending
    constant-rhs solve in the same call, then (combined step) with the resident one; and the whole IPM driven that way reaches the
    same answer as with the host algebra."""
    rng = np.random.default_rng(23)
    if name == "lp_like":      # nnz(P) == 0: every quadratic form vanishes
        P, q, A, b, cones = PROBLEMS["rand_uniform_300"]()
        P = sp.csc_matrix(P.shape)
    else:
        P, q, A, b, cones = PROBLEMS[name]()
    S = cl.Solver(P, q, A, b, cones, cl.Settings(device_reduced=True))
    assert S.kktsystem._device_reduced and S._needs_qb
    ks, data, v = S.kktsystem.kktsolver, S.data, S.variables
    n, m = data.n, data.m
    _scale_cones(S.cones, rng)
    assert ks.kktsolver_update(S.cones)
    Pfull = (data.P + sp.triu(data.P, 1).T).tocsr()
    for step, pending in enumerate((True, False, False)):
        rhs_x, workz = rng.standard_normal(n), rng.standard_normal(m)
        v.x[:] = rng.standard_normal(n)
        tau, kappa, rtau, rkappa = 0.8 + 0.1 * step, 0.4, rng.standard_normal(), rng.standard_normal()
        lx, lz = np.zeros(n), np.zeros(m)
        ok, dtau = ks.kktsolver_kkt_solve_reduced(rhs_x, workz, v.x, tau, kappa, rtau, rkappa, pending, lx, lz)
        assert ok
        sc = ks.last_reduced_scalars
        # the same two solutions through the plain solve entry points (bit-identical contexts), then the reference's formulas in numpy
        X, Z = np.zeros((2, n)), np.zeros((2, m))
        assert ks.kktsolver_solve_multi(np.vstack([-data.q, rhs_x]), np.vstack([data.b, workz]), X, Z)
        x2, z2, x1, z1 = X[0], Z[0], X[1], Z[1]
        xi = v.x / tau
        terms = [(data.q, x1), (data.b, z1), (xi, Pfull @ x1), (data.q, x2), (data.b, z2), (xi - x2, Pfull @ (xi - x2)), (x2, Pfull @ x2)]
        for got, (a, c) in zip(sc[3:10], terms):
            assert abs(got - float(a @ c)) <= 1e-13 * max(1.0, float(np.abs(a) @ np.abs(c))), (name, step)
        num = rtau - rkappa / tau + sc[3] + sc[4] + 2.0 * sc[5]
        den = kappa / tau - sc[6] - sc[7] + sc[8] - sc[9]
        assert abs(sc[1] - num) <= 1e-15 * max(1.0, abs(num)) * 8 and abs(sc[2] - den) <= 1e-15 * max(1.0, abs(den)) * 8
        assert dtau == sc[0] and abs(dtau - sc[1] / sc[2]) <= 1e-15 * abs(dtau) and abs(dtau - num / den) <= 1e-13 * max(1.0, abs(num / den))
        assert np.max(np.abs(lx - (x1 + dtau * x2))) <= 1e-13 * max(1.0, np.max(np.abs(x1)) + abs(dtau) * np.max(np.abs(x2)))
        assert np.max(np.abs(lz - (z1 + dtau * z2))) <= 1e-13 * max(1.0, np.max(np.abs(z1)) + abs(dtau) * np.max(np.abs(z2)))
    assert ks._refactor()        # a new factorisation invalidates the resident (x2, z2): asking for it is a usage error
    with pytest.raises(hipkkt.HipKKTError):
        ks.kktsolver_kkt_solve_reduced(rhs_x, workz, v.x, 1.0, 1.0, 0.0, 0.0, False, None, None)
    if name != "lp_like":
        solr = cl.Solver(P, q, A, b, cones, cl.Settings()).solve()
        sold = cl.Solver(P, q, A, b, cones, cl.Settings(device_reduced=True, device_residuals=True)).solve()
        assert solr.status == sold.status == "SOLVED" and abs(solr.iterations - sold.iterations) <= 1
        assert abs(solr.obj_val - sold.obj_val) <= 1e-7 * max(1.0, abs(solr.obj_val))
        if solr.iterations == sold.iterations:
            assert abs(solr.obj_val - sold.obj_val) <= 1e-9 * max(1.0, abs(solr.obj_val))


def test_plan_cache_reuses_the_analysis_of_an_identical_pattern(oracle_factory):
    """A second handle on the SAME KKT pattern and options takes its symbolic plan from the process-wide cache (DESIGN.md section 8:
    batches of structurally identical problems) and behaves exactly like the first: same permutation, bit-identical solves."""
    rng = np.random.default_rng(31)
    Pt, A, cones = _prep(problems.random_sparse_qp(400, 700, 41, 3, 1))
    m, n = A.shape
    h1 = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    c1 = h1.h.counters()
    Pt2 = Pt.copy()
    Pt2.data *= 1.5                                   # new values, same pattern
    h2 = HipKKTSolver(Pt2, A, cones, m, n, cl.Settings())
    c2 = h2.h.counters()
    assert c2["plan_cache_hits"] == c1["plan_cache_hits"] + 1 and c2["plan_cache_misses"] == c1["plan_cache_misses"]
    assert np.array_equal(h1.h.perm(), h2.h.perm()) and h1.h.nnzL == h2.h.nnzL
    h3 = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    _scale_cones(cones, rng)
    assert h1.kktsolver_update(cones) and h3.kktsolver_update(cones)
    b = rng.standard_normal(h1.h.N)
    assert np.array_equal(h1.h.ldl_solve(b), h3.h.ldl_solve(b))
    ok_ = oracle_factory(Pt, A, cones, m, n, cl.Settings(), ordering=h3.h.perm())
    assert ok_.kktsolver_update(cones)
    xc = ok_.k.ldl_solve(b)
    assert np.max(np.abs(h3.h.ldl_solve(b) - xc)) <= 1e-9 * max(1.0, np.max(np.abs(xc)))


def _image(h):
    colptr, rowval, nzval = h.kkt()
    maps = [h.map(w) for w in range(5)]
    smaps = [[h.sparse_map(i, w) for w in range(4)] for i in range(h.nsparse)]
    return colptr, rowval, nzval, maps, smaps, h.dsigns()


@pytest.mark.parametrize("name", ["qp_fixture", "socp_fixture", "sdp_fixture", "lasso_sparse_soc", "cfg1", "portfolio_small",
                                  "sdp_small", "genpow_mix", "p_without_diagonal", "long_rows"])
def test_device_assembly_equals_host_assembly(name, monkeypatch):
    """J1: the count -> scan -> fill kernels of assemble_dev.hip (the default of hipkkt_create_from_parts) against the host
    twin assemble.cpp (HIPKKT_HOST_ASSEMBLY=1), which tests/test_gpu_kkt.py::test_assembly_bit_exact_... and the hand-derived
    layouts pin on the oracle: colptr / rowval / nzval, every LDLDataMap vector, the expansion maps and Dsigns, bit for bit."""
    if name == "genpow_mix":
        n = 30
        numel, hs_dense = np.array([5, 5, 0, 6, 6, 4]), np.array([0, 0, 0, 0, 0, 1], dtype=np.int32)
        sparse_kind, dim1 = np.array([0, 2, 0, 1, 2, 0], dtype=np.int32), np.array([0, 3, 0, 0, 2, 0])
        S = sp.random(n, n, density=0.08, random_state=np.random.RandomState(5), format="csc")
        Pt = sp.triu(S + S.T + sp.diags(np.asarray(abs(S + S.T).sum(axis=1)).ravel() + 0.5), format="csc")
        A = sp.random(int(numel.sum()), n, density=0.15, random_state=np.random.RandomState(6), format="csc")
        desc = (numel, hs_dense, sparse_kind, dim1)
    elif name == "p_without_diagonal":
        n = 40
        S = sp.random(n, n, density=0.1, random_state=np.random.RandomState(8), format="csc")
        Pt = sp.triu(S + S.T, k=0, format="csc").tolil()
        for j in range(0, n, 3):
            Pt[j, j] = 0.0                                   # columns without a stored diagonal -> structural zero inserted
        Pt = sp.csc_matrix(Pt)
        Pt.eliminate_zeros()
        A = sp.random(70, n, density=0.1, random_state=np.random.RandomState(9), format="csc")
        desc = (np.array([70]), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64))
    elif name == "long_rows":                                # rows of A beyond the wavefront-per-row ranking (k_asm_place_A_long)
        n = 3000
        rng = np.random.default_rng(4)
        Pt = sp.identity(n, format="csc")
        A = sp.random(40, n, density=0.01, random_state=np.random.RandomState(3), format="lil")
        A[3, :] = rng.standard_normal(n)                     # a budget row: n entries
        A[17, ::2] = rng.standard_normal(n // 2)             # 1500 entries
        A[25, :600] = 1.0                                    # 600 entries
        A = sp.csc_matrix(A)
        desc = (np.array([40]), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64))
    else:
        Pt, A, cones = _prep(PROBLEMS[name]())
        desc = cones.kkt_descriptors()
    Pt.sort_indices()
    A.sort_indices()
    hd = hipkkt.Handle.from_parts(Pt, A, *desc)                 # device assembly
    monkeypatch.setenv("HIPKKT_HOST_ASSEMBLY", "1")
    hh = hipkkt.Handle.from_parts(Pt, A, *desc)
    a, b = _image(hd), _image(hh)
    assert (hd.N, hd.p, hd.nnzK, hd.nHs) == (hh.N, hh.p, hh.nnzK, hh.nHs)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    for x, y in zip(a[3], b[3]):
        assert np.array_equal(x, y)
    assert len(a[4]) == len(b[4])
    for sx, sy in zip(a[4], b[4]):
        for x, y in zip(sx, sy):
            assert np.array_equal(x, y)
    assert np.array_equal(a[5], b[5])
    hd.close()
    hh.close()


# ---- update_scaling! + get_Hs! on the device ------------------------------------------------
def _mixed_cone_problem(seed=77, n=30):
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


def test_update_scaling_on_device_matches_host_cone_algebra():
    """coneops_nncone.jl:77-101 (bit-exact), coneops_socone.jl:75-192 (the identities of test_coneops_secondordercone.jl:31-66 and
    the host values to rounding), coneops_psdtrianglecone.jl:145-161 (R R^T + skron), scattered as kktsolver_directldl.jl:223-241"""
    Pt, A, cones = _prep(_mixed_cone_problem())
    m, n = A.shape
    st = cl.Settings()
    host = HipKKTSolver(Pt, A, cones, m, n, st)
    dev = HipKKTSolver(Pt, A, cones, m, n, st)
    rng = np.random.default_rng(5)
    for trial in range(2):
        s, z = _scale_cones(cones, rng)                    # host: update_scaling!(cones, s, z, mu)
        if trial == 1:                                     # a badly scaled iterate, as late IPM iterations produce
            s *= 1e-6; z *= 1e4
            assert cones.update_scaling(s, z, 1.0)
        assert host.kktsolver_update(cones)                # host get_Hs! + uploads (the reference's call pattern)
        assert dev.kktsolver_update_scaled(cones, s, z)    # only (s, z) and the PSD R factors cross PCIe
        K1, K2 = host.h.debug_dump(4), dev.h.debug_dump(4)
        map_hs = host.h.map(2)
        scale = np.maximum(np.abs(K1), 1e-300)
        # per cone: NN / Zero blocks bit-exact, PSD to rounding of the sums
        u_all, v_all = dev.h.debug_dump(7), dev.h.debug_dump(8)
        umaps = [(dev.h.sparse_map(i, 0), dev.h.sparse_map(i, 1), dev.h.sparse_map(i, 3)) for i in range(dev.h.nsparse)]
        elsewhere = np.ones(len(K1), dtype=bool)
        for c, r, rb in zip(cones.cones, cones.rng_cones, cones.rng_blocks):
            idx = map_hs[rb.start:rb.stop]
            if c.kind_code in (0, 1):
                assert np.array_equal(K1[idx], K2[idx]), type(c).__name__
                if c.kind_code == 1:
                    assert np.array_equal(dev.scaling_w[r], c.w) and np.array_equal(dev.scaling_lambda[r], c.lam)
            else:
                elsewhere[idx] = False
                if c.kind_code == 3:
                    assert np.max(np.abs(K1[idx] - K2[idx]) / scale[idx]) < 5e-13, (type(c).__name__, c.numel)
        for maps in umaps:
            for ix in maps:
                elsewhere[ix] = False
        # the second-order cones under the gates of tests/soc_scaling_reference.py (the stand-in's own residuals and forward errors
        # against the 50-digit scaling set them: a few eps here, where the figures written by hand were 1e-14 .. 1e-10): what K holds
        # follows bit for bit from the returned (w, eta) and the resident (u, v) (row 0 of a sparse cone to row0_tolerance), w is on the
        # hyperboloid (R1), lambda = W z = W^-1 s (R2), eta (R3), D + u u' - v v' = 2 w w' - J as test_coneops_secondordercone.jl:31-66
        # (R4), and w, lambda, eta are within 8 x the stand-in's own error of the exact scaling
        tag = f"mixed cones, trial {trial}"
        w, lam, eta = dev.scaling_w, dev.scaling_lambda, dev.scaling_soc_eta
        ssr.check_diag_rows(tag, cones, K2, map_hs, s, z, w, lam)
        d = ssr.check_soc_entries(tag, cones, K2, map_hs, umaps, w, lam, eta, u_all, v_all)
        exact = ssr.exact_for(cones, s, z)
        host_rows = ssr.figures_of(cones, s, z, exact, *ssr.host_scaling(cones))
        rows = ssr.figures_of(cones, s, z, exact, w, lam, eta, u_all, v_all, lambda k, c: d[k])
        C, early = ssr.standin_constants()
        worst = ssr.check_rows(tag, rows, host_rows, False, None, C, early)
        print(f"[soc scaling {tag}] worst value / gate {worst}")
        # (kept next to the gates above, which measure against max |w| of a cone and, for eta, allow 8 x 14 eps: element by element
        # against the stand-in, as before)
        for k, c, r, _, _ in ssr.soc_list(cones):
            assert np.allclose(w[r], c.w, rtol=1e-12, atol=1e-14) and np.allclose(lam[r], c.lam, rtol=1e-12, atol=1e-14)
            assert abs(eta[k] - c.eta) <= 1e-14 * c.eta
        # everything that is neither a second-order nor a PSD entry is the same bits in both handles
        assert np.array_equal(K1[elsewhere], K2[elsewhere])
        # and the factorisations / refined solves agree
        rx, rz = rng.standard_normal(n), rng.standard_normal(m)
        xs = []
        for k in (host, dev):
            k.kktsolver_setrhs(rx, rz)
            x, zz = np.zeros(n), np.zeros(m)
            assert k.kktsolver_solve(x, zz)
            xs.append(np.concatenate([x, zz]))
        assert np.max(np.abs(xs[0] - xs[1])) <= 1e-9 * max(1.0, np.max(np.abs(xs[0])))
    # a second-order cone with z on the boundary: update_scaling! reports failure (coneops_socone.jl:88-90)
    r7 = [r for c, r in zip(cones.cones, cones.rng_cones) if c.kind_code == 2 and c.dim == 7][0]
    zb = z.copy(); zb[r7] = 0.0
    ok, *_ = dev.h.update_scaling(s, zb, None)
    assert not ok
    with pytest.raises(ValueError):
        dev.h.update_scaling(s[:-1], z)
    with pytest.raises(ValueError):
        dev.h.update_scaling(s, z, np.zeros(3))          # wrong length of the concatenated R factors


class _DevBuf:
    """device memory through the HIP runtime the library is linked with (PyTorch would bring a second runtime into the process)"""
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


def test_update_scaling_dev_keeps_everything_in_hbm():
    Pt, A, cones = _prep(_mixed_cone_problem(seed=78))
    m, n = A.shape
    k = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    s, z = _scale_cones(cones, np.random.default_rng(6))
    R = np.concatenate([c.R.ravel(order="F") for c in k._psd_cones])
    ok, w, lam, eta = k.h.update_scaling(s, z, R)
    assert ok
    K_host_ptrs = k.h.debug_dump(4)
    sd, zd, Rd = _DevBuf(s), _DevBuf(z), _DevBuf(R)
    wd, ld, ed = _DevBuf(m), _DevBuf(m), _DevBuf(len(eta))
    k.h.update_values(k.h.map(2), np.zeros(k.h.nHs))       # wipe the blocks so that the second call must rewrite them
    assert not np.array_equal(k.h.debug_dump(4), K_host_ptrs)
    assert k.h.update_scaling_dev(sd.ptr, zd.ptr, Rd.ptr, wd.ptr, ld.ptr, ed.ptr)
    assert np.array_equal(k.h.debug_dump(4), K_host_ptrs)
    assert np.array_equal(wd.get(), w) and np.array_equal(ld.get(), lam) and np.array_equal(ed.get(), eta)


@pytest.mark.parametrize("name", ["socp_fixture", "lasso_sparse_soc", "portfolio_small", "sdp_small"])
def test_ipm_with_device_scaling_reaches_the_same_answer(name):
    prob = PROBLEMS[name]()
    ref = cl.Solver(*prob, cl.Settings(), kktsolver_factory=lambda *a: HipKKTSolver(*a)).solve()
    got = cl.Solver(*prob, cl.Settings(device_scaling=True), kktsolver_factory=lambda *a: HipKKTSolver(*a)).solve()
    assert got.status == ref.status and abs(got.iterations - ref.iterations) <= 1
    assert abs(got.obj_val - ref.obj_val) <= 1e-8 * max(1.0, abs(ref.obj_val))
    assert np.max(np.abs(got.x - ref.x)) <= 1e-6 * max(1.0, np.max(np.abs(ref.x)))
