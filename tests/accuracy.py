"""Exact residuals and componentwise backward errors of a linear solve (test support, CPU only).

    r = b - K x     correctly rounded per row: every product K_ij x_j becomes an exact pair (p, e), p + e == K_ij x_j, through
                    Dekker's TwoProduct with Veltkamp's splitting (no fused multiply-add needed); each row's pairs and b_i are
                    then summed by math.fsum, which returns the exact sum rounded once
    omega           the componentwise (Oettli-Prager) backward error  max_i |r_i| / (|K| |x| + |b|)_i  over the rows whose
                    denominator is not 0: the smallest w with (K + dK) x = b + db for some |dK| <= w |K|, |db| <= w |b|

np.longdouble is not used on purpose: its 2^-64 is not far enough below 1e-16 for rows of thousands of entries (the dense rows of
a root front).  The pairs are exact as long as no |K_ij| or |x_j| exceeds 2^996 and no product falls below 2^-969: true for the
KKT systems of the suite."""
import math

import numpy as np
import scipy.sparse as sp

_VELTKAMP = float(2 ** 27 + 1)


def _split(a):
    c = _VELTKAMP * a
    hi = c - (c - a)
    return hi, a - hi


def two_product(a, b):
    """(p, e) with p = fl(a * b) and p + e == a * b exactly (elementwise, float64)"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def factored_kkt(colptr, rowval, nzval, dsigns, eps, diag):
    """what an LDL^T factorisation of the KKT system factors, K + eps * diag(Dsigns), as a full symmetric CSR matrix: colptr / rowval /
    nzval = the upper triangle (CSC, unregularised: hipkkt_get_kkt or the oracle's image), diag = the position of every diagonal entry
    in nzval (map_diag_full), eps = the static regulariser of that factorisation"""
    nz = np.array(nzval, dtype=np.float64)
    nz[np.asarray(diag, dtype=np.int64)] += eps * np.asarray(dsigns, dtype=np.float64)
    N = len(colptr) - 1
    U = sp.csc_matrix((nz, np.asarray(rowval, dtype=np.int64), np.asarray(colptr, dtype=np.int64)), shape=(N, N))
    K = (U + sp.triu(U, 1).T).tocsr()
    K.sort_indices()
    return K


def exact_residual(K, x, b):
    """-> (r, d): r = b - K x correctly rounded per row; d = |K| |x| + |b| in plain double (a scale, not a result)"""
    K = sp.csr_matrix(K)
    x = np.asarray(x, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    N = K.shape[0]
    ptr = np.asarray(K.indptr, dtype=np.int64)
    cnt = np.diff(ptr)
    p, e = two_product(K.data, x[K.indices])
    # one flat list of terms; row i owns [start[i], start[i + 1]): b_i, then -p and -e of each of its entries
    start = np.concatenate([[0], np.cumsum(2 * cnt + 1)])
    row = np.repeat(np.arange(N), cnt)
    k = np.arange(len(K.data)) - ptr[row]
    terms = np.empty(int(start[-1]))
    terms[start[:-1]] = b
    terms[start[row] + 1 + k] = -p
    terms[start[row] + 1 + cnt[row] + k] = -e
    tl = terms.tolist()
    r = np.array([math.fsum(tl[start[i]:start[i + 1]]) for i in range(N)], dtype=np.float64)
    d = abs(K) @ np.abs(x) + np.abs(b)
    return r, d


def backward_error(K, x, b):
    """the componentwise backward error omega of x as a solution of K x = b (rows with |K| |x| + |b| == 0 are skipped)"""
    r, d = exact_residual(K, x, b)
    keep = d > 0
    if not np.any(keep):
        return 0.0
    return float(np.max(np.abs(r[keep]) / d[keep]))
