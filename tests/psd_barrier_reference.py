"""A 50-digit reference (mpmath) for the barrier of a PSD triangle cone, compute_barrier / _logdet_barrier of
coneops_psdtrianglecone.jl:256-290, and the cases that tests/test_psd_barrier_reference.py (CPU) and tests/test_gpu_mixed_step.py (GPU)
share.  No tests here.

What is exact.  The reference forms q = x + alpha dx in float64 (`@. q = x + alpha*dx`: one product, one sum), and so do the stand-in
and the kernel, with the same two roundings.  That vector is taken as given, like every input of tests/psd_step_reference.py; from it
    Q = svec_to_mat(q)   (off-diagonal entries times the float64 constant 1 / sqrt 2, the product unrounded here)
    barrier = -logdet(Q_z) - logdet(Q_s)
is evaluated at 50 digits by a Cholesky factorisation.  A Q that is not positive definite at 50 digits has no logdet: ref_logdet gives
None and the cone's barrier is the reference's `barrier -= typemax(T)`, i.e. -Inf.

The error scale of one logdet,
    scale = sum_ij (|Q^-1| o |L| |L'|)_ij + sum_j |log l_jj^2|,
has two parts.  A float64 Cholesky factorises Q + E with |E| <= c n eps |L| |L'| componentwise (Higham, Accuracy and Stability,
Theorem 10.3), and logdet(Q + E) - logdet(Q) = tr(Q^-1 E) to first order, so |tr(Q^-1 E)| <= c n eps sum(|Q^-1| o |L| |L'|); the
rounding of the off-diagonal products q_k / sqrt 2 is an E <= eps |Q| <= eps |L| |L'| of the same kind.  The second part is the rounding of
the n logarithms and of their running sum.  The scale of a barrier is the sum of the scales of its two logdets.  It is computed at 50
digits for n <= 33 and in float64 at n = 64 (a scale needs two digits).

emulate_kernel repeats barrier_psd.hip in float64: the lower triangle of Q, the right-looking Cholesky whose entry (i, k) receives
a_ik - l_i0 l_k0 - l_i1 l_k1 - .. in ascending order, product and difference rounded separately, a pivot that is not > 0 or not finite
ends it with +Inf, logdet = dd + dd with dd the running sum of log(sqrt(pivot_j)) in ascending j, barrier = (0 - logdet_z) - logdet_s.
(numpy's log stands in for the device's: the emulation is held to the 50-digit value, not to the device's bits.)"""
import functools
import math
import os
import re

import numpy as np

import clarabel_jl_amd  # noqa: F401
from julia_standin.cones import _ISQRT2, PSDTriangleCone
from tests import psd_step_reference as pr

mp, mpf, EPS = pr.mp, pr.mpf, pr.EPS
SIDES = (1, 2, 3, 17, 32, 33, 64)
SCALE_MP_MAX_N = 33
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def max_candidates_in_source():
    """the candidates one launch of k_bar_psd serves: the cases carry that many"""
    src = open(os.path.join(ROOT, "clarabel.jl_amd", "csrc", "barrier_psd.hip")).read()
    return int(re.search(r"constexpr\s+int\s+kBarPsdMax\s*=\s*(\d+)\s*;", src).group(1))


NALPHA = max_candidates_in_source()


# ---- 50 digits -------------------------------------------------------------------------------------------------------------------------

def shifted(x, dx, alpha):
    """q = x + alpha dx as the reference, the stand-in and the kernel form it: float64, product and sum rounded separately"""
    return np.asarray(x, dtype=np.float64) + float(alpha) * np.asarray(dx, dtype=np.float64)


def _chol_mp(Q):
    """lower Cholesky factor of the object matrix Q at 50 digits, or None when a pivot is not positive"""
    n = Q.shape[0]
    L = Q.copy()
    for j in range(n):
        d = L[j, j]
        if not d > 0:
            return None
        piv = mp.sqrt(d)
        L[j, j] = piv
        if j + 1 < n:
            col = L[j + 1:, j] / piv
            L[j + 1:, j] = col
            for k in range(j + 1, n):      # the lower triangle only
                L[k:, k] = L[k:, k] - col[k - j - 1:] * col[k - j - 1]
    for j in range(n):
        L[j, j + 1:] = mpf(0)
    return L


def ref_logdet(q, n):
    """-> (logdet(svec_to_mat(q)) at 50 digits or None when it is not positive definite, its Cholesky factor or None)"""
    if not np.all(np.isfinite(q)):
        return None, None
    L = _chol_mp(pr.svec_to_mat(q, n))
    if L is None:
        return None, None
    return 2 * sum((mp.log(L[j, j]) for j in range(n)), mpf(0)), L


def logdet_scale(q, n, L=None):
    """sum(|Q^-1| o |L| |L'|) + sum_j |log l_jj^2| as a float: at 50 digits up to SCALE_MP_MAX_N (needs the factor L), float64 above"""
    if n <= SCALE_MP_MAX_N:
        Linv = np.empty((n, n), dtype=object)
        for c in range(n):      # forward substitution on the columns of the identity
            for i in range(n):
                if i < c:
                    Linv[i, c] = mpf(0)
                    continue
                acc = mpf(1) if i == c else mpf(0)
                for k in range(c, i):
                    acc -= L[i, k] * Linv[k, c]
                Linv[i, c] = acc / L[i, i]
        Qinv = pr.mm(Linv.T.copy(), Linv)
        LL = pr.mm(np.vectorize(abs, otypes=[object])(L), np.vectorize(abs, otypes=[object])(L.T.copy()))
        first = sum(abs(a) * b for a, b in zip(Qinv.ravel(), LL.ravel()))
        second = sum(abs(2 * mp.log(L[j, j])) for j in range(n))
        return float(first + second)
    Q = PSDTriangleCone(n).svec_to_mat(np.asarray(q, dtype=np.float64))
    L64 = np.linalg.cholesky(Q)
    return float(np.sum(np.abs(np.linalg.inv(Q)) * (np.abs(L64) @ np.abs(L64.T))) + np.sum(np.abs(2.0 * np.log(np.diag(L64)))))


def ref_barrier(n, z, s, dz, ds, alpha, want_scale=True):
    """-> (barrier at 50 digits, or -inf when a shifted point is outside the cone; its error scale, or None then)"""
    total, scale = mpf(0), 0.0
    for x, dx in ((z, dz), (s, ds)):
        q = shifted(x, dx, alpha)
        ld, L = ref_logdet(q, n)
        if ld is None:
            return -math.inf, None
        total -= ld
        if want_scale:
            scale += logdet_scale(q, n, L)
    return total, (scale if want_scale else None)


# ---- the kernel's arithmetic in float64 ------------------------------------------------------------------------------------------------

def emulate_logdet(q, n):
    Q = np.zeros((n, n))
    r, c = pr._idx(n)      # packed entry k = (r, c) of the upper triangle, r <= c: the lower triangle's (c, r)
    Q[c, r] = np.where(r == c, q, q * _ISQRT2)
    pivots = np.zeros(n)
    for j in range(n):
        d = Q[j, j]
        if not (d > 0.0 and math.isfinite(d)):
            return math.inf
        pivots[j] = d
        piv = math.sqrt(d)
        col = Q[j + 1:, j] / piv
        Q[j + 1:, j] = col
        Q[j + 1:, j + 1:] = Q[j + 1:, j + 1:] - np.outer(col, col)      # (the upper triangle goes along unread)
    dd = 0.0
    for j in range(n):
        dd += math.log(math.sqrt(pivots[j]))
    return dd + dd


def emulate_kernel(n, z, s, dz, ds, alpha):
    with np.errstate(all="ignore"):
        return (0.0 - emulate_logdet(shifted(z, dz, alpha), n)) - emulate_logdet(shifted(s, ds, alpha), n)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------

def interior_direction(K, x, rng, size=0.5):
    """dx = svec(L E L') with X = L L' and E symmetric of 2-norm `size` < 1: X + alpha dX = L (I + alpha E) L' stays positive definite
    for 0 <= alpha <= 1, at an early iterate and at a late one whose X is ill conditioned"""
    L = np.linalg.cholesky(K.svec_to_mat(x))
    E = rng.standard_normal((K.n, K.n))
    E = 0.5 * (E + E.T)
    E *= size / max(np.linalg.norm(E, 2), 1e-300)
    D = L @ E @ L.T
    return K.mat_to_svec(0.5 * (D + D.T))


def candidates(nalpha=NALPHA):
    """the backtracking grid alpha0 step^k by repeated multiplication, as the caller forms it"""
    out, a = [], 0.99
    for _ in range(nalpha):
        out.append(a)
        a = 0.8 * a
    return out


@functools.lru_cache(maxsize=None)
def case(n, late):
    """-> dict(K, s, z, dz, ds, alphas[8], ref[8], scale[8], host[8], host_ratio[8]): one PSD cone of side n at an early point (cond 1e3)
    or a late one (S Z ~ mu I, mu = 1e-9), a direction that keeps every candidate inside, the 50-digit barrier, its scale, the stand-in's
    value and the stand-in's error in units of eps x scale.  Computed once per process; callers must not modify the arrays."""
    rng = np.random.default_rng(7000 + 10 * n + int(late))
    K = PSDTriangleCone(n)
    s, z, _ = pr.random_sz(K, rng, late)
    dz, ds = interior_direction(K, z, rng), interior_direction(K, s, rng)
    alphas = candidates()
    ref, scale, host, ratio = [], [], [], []
    for a in alphas:
        b, sc = ref_barrier(n, z, s, dz, ds, a)
        h = K.compute_barrier(z, s, dz, ds, a)
        ref.append(b)
        scale.append(sc)
        host.append(h)
        ratio.append(float(abs(mpf(h) - b)) / (EPS * sc))
    for v in (s, z, dz, ds):
        v.setflags(write=False)
    return dict(K=K, n=n, late=late, s=s, z=z, dz=dz, ds=ds, alphas=alphas, ref=ref, scale=scale, host=host, host_ratio=ratio)


def ratio(got, ref, scale):
    """|got - ref| in units of eps x scale"""
    return float(abs(mpf(float(got)) - ref)) / (EPS * scale)


def allowed(host_ratio, n):
    """the project's rule (tests/test_gpu_psd_step.py): 8 x the host's error in the same case, at least 2 n, in units of eps x scale"""
    return max(8.0 * host_ratio, 2.0 * n)
