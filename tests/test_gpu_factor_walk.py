"""The launch walk of the factorisation (hipkkt_factor.cpp enqueue_factor) on each of its callers: captured into the graph, replayed,
run eagerly with the profiling probe (hipkkt_set_profiling 1 and 2), replayed again behind the eager runs, and run eagerly without a
graph (HIPKKT_NO_GRAPH=1).  It is one walk, so all of them leave the same pivots, the same unrefined solve and the same count of
regularised pivots, bit for bit, and the probe counts what the walk launched.  Problem: the smallest one with front batches (the one
of test_gpu_front_batch_hops.py), with batches that have workgroups below the diagonal and without (update_batch 3, 5), and with the
batches off (the level kernels only).  Riders cannot occur at this size; test_gpu_fullsize.py owns them."""
import numpy as np
import pytest
import scipy.sparse as sp

import clarabel_jl_amd  # noqa: F401  (registers the dotted package directory)
import julia_standin as cl
from clarabel_jl_amd import problems
from clarabel_jl_amd.kktsolver import HipKKTSolver
from tests.fixtures import scale_cones

pytestmark = pytest.mark.gpu


def _handle(monkeypatch, Pt, A, cones, update_batch, front_block, no_graph):
    monkeypatch.setenv("HIPKKT_PLAN_CACHE", "0")
    monkeypatch.setenv("HIPKKT_FRONT_BLOCK_MIN_ROWS", "0")       # the root front is below the product's threshold for the front batches
    monkeypatch.setenv("HIPKKT_FRONT_BLOCK", front_block)
    monkeypatch.setenv("HIPKKT_NO_GRAPH", no_graph)
    m, n = A.shape
    return HipKKTSolver(Pt, A, cones, m, n, cl.Settings(), update_batch=update_batch)


def _batch_panels(h, update_batch):
    """(batches, panels in them) restated from the plan: a front's 64-wide panels, one per level, in windows of update_batch levels;
    a window of at least two panels is one batch (symbolic.cpp front_batches; dump 22 = the fronts, 10 / 11 = columns / level per supernode)"""
    first, level = h.debug_dump(10), h.debug_dump(11)
    batches = panels = 0
    for s0, npan, _, _ in h.debug_dump(22).reshape(-1, 4).astype(int):
        sn = np.arange(s0, s0 + npan)
        wide = first[sn + 1] - first[sn] == 64
        for win in np.unique(level[sn] // update_batch):
            k = level[sn] // update_batch == win
            if k.sum() >= 2 and wide[k].all():
                batches, panels = batches + 1, panels + int(k.sum())
    return batches, panels


@pytest.mark.parametrize("update_batch,front_block", [(3, "1"), (5, "1"), (3, "0")])
def test_one_walk_for_graph_profile_and_eager(update_batch, front_block, monkeypatch):
    rng = np.random.default_rng(47)
    P, q, A, b_, specs = problems.random_sparse_qp(1000, 2000, 1, 4, 2)
    cones = cl.CompositeCone(cl.cones_new_collapsed(specs))
    Pt = sp.triu(sp.csc_matrix(P), format="csc")
    Pt.sort_indices()
    A = sp.csc_matrix(A)
    A.sort_indices()
    scale_cones(cones, rng)
    hk = _handle(monkeypatch, Pt, A, cones, update_batch, front_block, "0")
    b = rng.standard_normal(hk.h.N)

    def factor(s=hk):
        assert s.kktsolver_update(cones)
        assert s.h.counters()["sweep_timeouts"] == 0
        return s.h.debug_dump(5), s.h.ldl_solve(b), s.last_nreg

    def same(got, want):
        return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]

    # 1. the graph path: capture, then replay
    ref = factor()
    assert same(factor(), ref)
    c = hk.h.counters()
    on = front_block == "1"
    assert c["front_block"] == on and (c["front_batches"] > 0) == on
    nbatch, npanels = _batch_panels(hk.h, update_batch) if on else (0, 0)
    assert c["front_batches"] == nbatch

    # 2. the same walk, eager, with the probe
    hk.h.set_profiling(True)
    assert same(factor(), ref)
    p = hk.h.profile()
    assert p["front_block_launches"] == nbatch and p["front_block_panels"] == npanels
    assert p["front_block_extra_tiles"] == 0            # (no stage of this problem is big enough for riders)

    # 3. ... keeping every tile in its own stage's launch
    hk.h.set_profiling(2)
    assert same(factor(), ref)
    p = hk.h.profile()
    assert p["front_block_launches"] == nbatch and p["front_block_panels"] == npanels and p["front_block_extra_tiles"] == 0

    # 4. the graph is still good behind the eager runs
    hk.h.set_profiling(False)
    assert same(factor(), ref)

    # 5. eager without the probe, on a handle of its own
    hk2 = _handle(monkeypatch, Pt, A, cones, update_batch, front_block, "1")
    assert same(factor(hk2), ref)
    assert hk2.h.counters()["front_batches"] == nbatch
