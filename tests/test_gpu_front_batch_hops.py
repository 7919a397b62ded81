"""The front-batch kernel (front_block2.hip) on every path of a diagonal workgroup's step head: the head records of the next panel are
requested at the end of a step, awaited in front of the next one, and the batch's last diagonal workgroup stores a finished panel
behind them.  The paths that differ:
  * early panel stores on (the batch has workgroups below the diagonal) and off (the front's last batch);
  * a full batch of five panels and shorter ones;
  * a front whose last row block is short (fewer than 64 rows).
The smallest problem that reaches all of them is cfg 1's 12-panel root front with 3, 4 and 5 levels per update batch (the batches are
aligned to levels: 2 to 5 panels, with and without workgroups below the diagonal).  Per setting: the factorisation is deterministic
(bit-identical when repeated), agrees with the first form of the kernel (front_block.hip, HIPKKT_FB_V2=0) as
test_front_block_second_form_equals_first_form demands of the full-size configs, and its refined solve holds against the true K."""
import numpy as np
import pytest
import scipy.sparse as sp

import clarabel_jl_amd  # noqa: F401  (registers the dotted package directory)
import julia_standin as cl
from clarabel_jl_amd import problems
from clarabel_jl_amd.kktsolver import HipKKTSolver
from oracle.kkt_oracle import OracleKKTSolver
from tests import accuracy as acc
from tests.fixtures import scale_cones

pytestmark = pytest.mark.gpu

BOUND, FLOOR = 4.0, 2.0 ** -50        # tests/test_gpu_solve_accuracy.py: omega_hip <= BOUND * max(omega_oracle, FLOOR)


def _prep(prob):
    P, q, A, b, specs = prob
    cones = cl.CompositeCone(cl.cones_new_collapsed(specs))
    Pt = sp.triu(sp.csc_matrix(P), format="csc")
    Pt.sort_indices()
    A = sp.csc_matrix(A)
    A.sort_indices()
    return Pt, A, cones


def _handle(monkeypatch, Pt, A, cones, update_batch, v2):
    monkeypatch.setenv("HIPKKT_PLAN_CACHE", "0")
    monkeypatch.setenv("HIPKKT_FRONT_BLOCK_MIN_ROWS", "0")       # cfg 1's root is below the product's threshold for the front batches
    monkeypatch.setenv("HIPKKT_FB_V2", v2)
    m, n = A.shape
    return HipKKTSolver(Pt, A, cones, m, n, cl.Settings(), update_batch=update_batch)


def _refined(hk, rx, rz):
    lx, lz = np.zeros(len(rx)), np.zeros(len(rz))
    hk.kktsolver_setrhs(rx, rz)
    assert hk.kktsolver_solve(lx, lz)
    return np.concatenate([lx, lz])


@pytest.mark.parametrize("update_batch", [3, 4, 5])
def test_front_batch_step_heads(update_batch, monkeypatch, capsys):
    rng = np.random.default_rng(31)
    Pt, A, cones = _prep(problems.random_sparse_qp(1000, 2000, 1, 4, 2))
    m, n = A.shape
    scale_cones(cones, rng)
    hk1 = _handle(monkeypatch, Pt, A, cones, update_batch, "1")
    assert hk1.kktsolver_update(cones)
    c = hk1.h.counters()
    assert c["front_batches"] > 0 and c["front_block"] and c["sweep_timeouts"] == 0
    N = hk1.h.N
    b = rng.standard_normal(N)
    rx, rz = rng.standard_normal(n), rng.standard_normal(m)

    # 1. factor twice: bit-identical pivots and unrefined solve
    d1, x1 = hk1.h.debug_dump(5), hk1.h.ldl_solve(b)
    assert hk1.kktsolver_update(cones)
    assert np.array_equal(hk1.h.debug_dump(5), d1)
    assert np.array_equal(hk1.h.ldl_solve(b), x1)
    assert hk1.h.counters()["sweep_timeouts"] == 0

    # 2. against the first form of the kernel
    hk0 = _handle(monkeypatch, Pt, A, cones, update_batch, "0")
    assert hk0.kktsolver_update(cones)
    c0 = hk0.h.counters()
    assert c0["front_batches"] > 0 and c0["front_block"] and c0["sweep_timeouts"] == 0
    assert hk0.last_nreg == hk1.last_nreg
    d0 = hk0.h.debug_dump(5)
    assert np.all(np.sign(d0) == np.sign(d1))
    assert np.max(np.abs(d1 - d0) / np.maximum(np.abs(d0), 1e-300)) <= 1e-6
    x0 = hk0.h.ldl_solve(b)
    assert np.max(np.abs(x1 - x0)) <= 1e-9 * max(1.0, np.max(np.abs(x0)))
    s0, s1 = _refined(hk0, rx, rz), _refined(hk1, rx, rz)
    assert np.max(np.abs(s1 - s0)) <= 1e-9 * max(1.0, np.max(np.abs(s0)))

    # 3. the refined solve against the true (unregularised) K: the reference's stopping rule as asserted at every size
    #    (tests/test_gpu_fullsize.py), and the componentwise backward error against the oracle's refined solve on the same permutation
    #    under the bound of tests/test_gpu_solve_accuracy.py
    assert hk1.h.p == 0
    colptr, rowval, nz = hk1.h.kkt()
    K = acc.factored_kkt(colptr, rowval, nz, hk1.h.dsigns(), 0.0, hk1.h.map(4))
    rhs = np.concatenate([rx, rz])
    res = rhs - K @ s1
    o = OracleKKTSolver(Pt, A, cones, m, n, cl.Settings(), ordering=hk1.h.perm())
    assert o.kktsolver_update(cones)
    so = _refined(o, rx, rz)
    wg, wc = acc.backward_error(K, s1, rhs), acc.backward_error(K, so, rhs)
    with capsys.disabled():
        print(f"\n[front-batch heads, update_batch {update_batch}] batches {c['front_batches']} nreg {hk1.last_nreg} "
              f"|res| {np.max(np.abs(res)):.3e} omega hip {wg:.3e} oracle {wc:.3e}")
    assert np.max(np.abs(res)) <= 1e-9 * max(1.0, np.max(np.abs(rhs)))
    assert wg <= BOUND * max(wc, FLOOR), (wg, wc)
