"""CPU prediction for tests/test_gpu_solve_accuracy.py, before any GPU run: the host interpreter of the plan (tests/support/plan_check.cpp)
solves cfg 1's root front the ways the kernels do, and the componentwise backward error omega (tests/accuracy.py) of each form is set
against substitution on the same plan, at the late iterates of the GPU test.

* substitution: every block by substitution, the super-block fronts panel by panel too (PLANCHECK_SB_SUBST=1) -- the oracle's
  algorithm in the plan's order;
* the kernels' forms: products with the explicit inverses -- of the 64-column panels (one hop per panel, k_front_fwd / _bwd) or of the
  512 x 512 super-blocks (k_invert_super, k_front_fwd_sb / _bwd_sb) -- with the refinement step on the marked wide blocks outside the
  fronts and none inside them (PLANCHECK_EXPLICIT_INV=2, PLANCHECK_FRONT_REFINE=0).

Bound as on the GPU: omega_kernels <= 4 max(omega_substitution, 2^-50).  The panel inverses keep it on every iterate (ratios 0.7 -
1.0).  The host twin of the super-block inverses (SbEmu: plain sums in tile order) does not at the mu = 1e-10 iterate: 4.6x with 64-
and with 16-column panels, a predicted break, marked xfail(strict).  The kernels themselves (k_invert_super: fused multiply-adds in
four interleaved partial sums) measured 2.3x and 1.0x on the same factored matrix and right-hand side in
tests/test_gpu_solve_accuracy.py: inside the bound, so the front sweeps keep their unrefined products; this file keeps the twin's
margin on record for the rewrite of the sweeps."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import problems
from oracle.kkt_oracle import OracleKKT, OracleKKTSolver
from tests import accuracy as acc
from tests import plan_support as ps
from tests.test_gpu_solve_accuracy import BOUND, FLOOR, ITERATES, SEED

_SB_TWIN_BREAKS = pytest.mark.xfail(strict=True, reason="the host twin of the super-block inverses loses 4.6x against substitution at this "
                                "iterate (the GPU kernels: 2.3x / 1.0x, tests/test_gpu_solve_accuracy.py)")

CASES = [  # path, PLANCHECK_SUPERHOP, supernode width, iterate
    pytest.param("panel_hop", "0", 64, "late_mu1e-9"),
    pytest.param("panel_hop", "0", 64, "late_mu1e-10"),
    pytest.param("super_block", "1", 64, "late_mu1e-9"),
    pytest.param("super_block", "1", 64, "late_mu1e-10", marks=_SB_TWIN_BREAKS),
    pytest.param("super_block_w16", "1", 16, "late_mu1e-9"),
    pytest.param("super_block_w16", "1", 16, "late_mu1e-10", marks=_SB_TWIN_BREAKS),
]


@pytest.mark.parametrize("path,superhop,width,iterate", CASES)
def test_front_inverses_against_substitution(path, superhop, width, iterate, monkeypatch, capsys):
    for k in [k for k in os.environ if k.startswith("PLANCHECK_")]:
        monkeypatch.delenv(k)
    monkeypatch.setenv("PLANCHECK_SUPERHOP", superhop)
    P, q, A, b, specs = problems.random_sparse_qp(1000, 2000, 1, 4, 2)
    cones = cl.CompositeCone(cl.cones_new_collapsed(specs))
    Pt = sp.triu(sp.csc_matrix(P), format="csc"); Pt.sort_indices()
    A = sp.csc_matrix(A); A.sort_indices()
    m, n = A.shape
    k0 = OracleKKT(Pt, A, *cones.kkt_descriptors())
    rc, _, perm, st = ps.run(k0.N, k0.colptr, k0.rowval, k0.nzval.copy(), k0.map("dsigns"), max_width=width, symbolic_only=True)
    assert rc == 0 and st["nfronts"] >= 1
    if superhop == "1":
        assert st["nsb_fronts"] >= 1 and st["max_front_panels"] >= (16 if width == 16 else 10)
    else:
        assert st["nsb_fronts"] == 0 and st["max_front_panels"] >= 10
    o = OracleKKTSolver(Pt, A, cones, m, n, cl.Settings(), ordering=perm)
    rng = np.random.default_rng(SEED)
    ITERATES[iterate](cones, rng)
    assert o.kktsolver_update(cones) and o.k.L.oracle_kkt_nreg(o.k.h) == 0
    k = o.k
    ds, diag, nz, eps = k.map("dsigns"), k.map("map_diag_full"), k.nzval, o.diagonal_regularizer
    nz_reg = nz.copy()
    nz_reg[diag] += eps * ds
    K = acc.factored_kkt(k.colptr, k.rowval, nz, ds, eps, diag)
    rhs = rng.standard_normal(k.N)

    def omega(**env):
        for key, v in env.items():
            monkeypatch.setenv("PLANCHECK_" + key, v)
        rc_, x, _, st_ = ps.run(k.N, k.colptr, k.rowval, nz_reg, ds, b=rhs, perm=perm, max_width=width)
        for key in env:
            monkeypatch.delenv("PLANCHECK_" + key)
        assert rc_ == 0 and st_["nreg"] == 0
        return acc.backward_error(K, x, rhs)

    w_oracle = acc.backward_error(K, k.ldl_solve(rhs), rhs)
    w_sub = omega(EXPLICIT_INV="0", SB_SUBST="1")
    w_kern = omega(EXPLICIT_INV="2", INV_WMIN="17", INV_TAU="64", FRONT_REFINE="0")
    with capsys.disabled():
        print(f"\n[front-inverse prediction cfg1 {path} / {iterate}] omega substitution {w_sub:.3e} kernels' form {w_kern:.3e} "
              f"ratio {w_kern / max(w_sub, FLOOR):.2f} (oracle {w_oracle:.3e})")
    assert w_sub <= BOUND * max(w_oracle, FLOOR)            # the plan with substitution is the oracle's algorithm in another order
    assert w_kern <= BOUND * max(w_sub, FLOOR), (w_kern, w_sub)
