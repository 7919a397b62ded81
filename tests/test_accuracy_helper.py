"""tests/accuracy.py (the exact residual and the componentwise backward error behind tests/test_gpu_solve_accuracy.py) against mpmath at
60 digits: every row's residual must be the correctly rounded value of the exact b_i - sum_j K_ij x_j, on rows where plain double
gets it wrong."""
import math

import mpmath
import numpy as np
import scipy.sparse as sp

from tests import accuracy as acc


def _rows():
    """(K, x, b): one row per situation; magnitudes within about 2^+-20 (rows 0 - 4, 6) or 2^+-45 (row 5), so that 60 digits (199 bits)
    hold each row's exact sum or miss it far below the last bit of the result"""
    rng = np.random.default_rng(2024)
    n = 6000
    x = rng.uniform(-1.0, 1.0, n) * 2.0 ** rng.integers(-20, 20, n)
    rows, b = [], []
    # 0: b_i = fl(K_i x) in plain double, i.e. exact cancellation up to the rounding errors of 3000 products and sums
    c = rng.choice(n, 3000, replace=False)
    v = rng.standard_normal(3000)
    rows.append((c, v)); b.append(float(np.dot(v, x[c])))
    # 1: one product against its own rounded value: r = the product's lost low bits, which plain double reports as 0
    j = 7
    rows.append((np.array([j]), np.array([1.0 + 2.0 ** -30]))); b.append(float((1.0 + 2.0 ** -30) * x[j]))
    # 2: products that lose bits, of alternating sign, summed against their rounded sum
    c = np.arange(100, 140)
    v = (1.0 + 2.0 ** -27 * rng.integers(1, 1 << 26, 40)) * np.where(np.arange(40) % 2 == 0, 1.0, -1.0)
    rows.append((c, v)); b.append(math.fsum((v * x[c]).tolist()))
    # 3: an empty row with b_i = 0 (skipped by omega) and 4: an empty row with b_i != 0 (r = b_i)
    rows.append((np.zeros(0, dtype=np.int64), np.zeros(0))); b.append(0.0)
    rows.append((np.zeros(0, dtype=np.int64), np.zeros(0))); b.append(0.75)
    # 5: dense row of a root front: 5000 entries of widely spread magnitude, b near the sum
    c = rng.choice(n, 5000, replace=False)
    v = rng.standard_normal(5000) * 2.0 ** rng.integers(-20, 20, 5000)
    rows.append((c, v)); b.append(float(np.sum(v * x[c])) * (1.0 + 2.0 ** -40))
    # 6: plain random row, no cancellation
    c = rng.choice(n, 50, replace=False)
    v = rng.standard_normal(50)
    rows.append((c, v)); b.append(float(rng.standard_normal()))
    indptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])])
    K = sp.csr_matrix((np.concatenate([r[1] for r in rows]), np.concatenate([r[0] for r in rows]).astype(np.int64), indptr),
                      shape=(len(rows), n))
    return K, x, np.array(b)


def test_exact_residual_is_correctly_rounded_against_mpmath():
    K, x, b = _rows()
    r, d = acc.exact_residual(K, x, b)
    plain = b - K @ x
    wrong_in_double = 0
    for i in range(K.shape[0]):
        a, e = K.indptr[i], K.indptr[i + 1]
        with mpmath.workdps(60):
            s = mpmath.mpf(b[i])
            for kij, j in zip(K.data[a:e].tolist(), K.indices[a:e].tolist()):
                s -= mpmath.mpf(kij) * mpmath.mpf(x[j])
            want = float(s)                                  # round to nearest
        assert r[i] == want, (i, r[i], want)
        wrong_in_double += plain[i] != want
        dd = math.fsum(abs(kij) * abs(x[j]) for kij, j in zip(K.data[a:e].tolist(), K.indices[a:e].tolist())) + abs(b[i])
        assert abs(d[i] - dd) <= 1e-12 * dd
    assert r[3] == 0.0 and r[4] == 0.75 and d[3] == 0.0
    assert r[1] != 0.0 and plain[1] == 0.0                 # the lost low bits of one product
    assert wrong_in_double >= 3                             # rows 0, 1, 2 at least: the cases the helper exists for
    # omega: the row maximum of |r| / d, the zero row skipped
    keep = d > 0
    w = acc.backward_error(K, x, b)
    assert w == float(np.max(np.abs(r[keep]) / d[keep])) and math.isfinite(w)
    assert acc.backward_error(sp.csr_matrix((2, 2)), np.ones(2), np.zeros(2)) == 0.0


def test_two_product_is_exact():
    rng = np.random.default_rng(7)
    a = rng.standard_normal(2000) * 2.0 ** rng.integers(-300, 300, 2000)
    c = rng.standard_normal(2000) * 2.0 ** rng.integers(-300, 300, 2000)
    p, e = acc.two_product(a, c)
    with mpmath.workdps(60):
        for ai, ci, pi, ei in zip(a.tolist(), c.tolist(), p.tolist(), e.tolist()):
            assert mpmath.mpf(pi) + mpmath.mpf(ei) == mpmath.mpf(ai) * mpmath.mpf(ci)


def test_factored_kkt_adds_the_regulariser_on_the_diagonal():
    # upper triangle of [[2, 1, 0], [1, -3, 4], [0, 4, 5]] in CSC, diagonal entries at 0, 2, 4
    colptr = np.array([0, 1, 3, 5])
    rowval = np.array([0, 0, 1, 1, 2])
    nz = np.array([2.0, 1.0, -3.0, 4.0, 5.0])
    K = acc.factored_kkt(colptr, rowval, nz, np.array([1, -1, 1]), 1e-8, np.array([0, 2, 4]))
    want = np.array([[2.0 + 1e-8, 1.0, 0.0], [1.0, -3.0 - 1e-8, 4.0], [0.0, 4.0, 5.0 + 1e-8]])
    assert np.array_equal(K.toarray(), want)
    x = np.array([1.0, 2.0, -1.0])
    assert acc.backward_error(K, np.linalg.solve(want, x), x) <= 4 * np.finfo(float).eps
