"""A 50-digit reference (mpmath) for the interior-point step algebra of PSD triangle cones, and the inputs that
tests/test_psd_step_reference.py (CPU) and tests/test_gpu_psd_step.py (GPU) share.  No tests here.

The functions evaluate the reference's OWN formulas (coneops_psdtrianglecone.jl:164-254, :409-497, coneops_symmetric_common.jl:1-52, as
restated in julia_standin/cones.py PSDTriangleCone) at 50 digits on the float64 (R, Rinv, lambda) and vectors AS GIVEN: what the
stand-in's and the kernels' numbers would be without rounding.  Whether R, Rinv, lambda are a good Nesterov-Todd scaling of some (s, z) is
not the step's business (the identities R' Z R = Lambda = Rinv S Rinv' are checked in test_psd_step_reference.py).  The 1 / sqrt 2 of
svec_to_mat / mat_to_svec is the float64 constant the stand-in multiplies with, taken as given like every other input.

Matrices are numpy object arrays of 50-digit numbers.  A product converts both factors to integers times a power of two (every
50-digit binary number is one, exactly), multiplies exactly and rounds once: far faster than mpmath's own matrix product at n = 64.
gamma = lambda_min(M) comes from mp.eigsy(..., eigvals_only=True).

Every function also returns the float64 SCALE the tolerance of its result is stated in (tests/test_gpu_psd_step.py): for products the
entrywise bound |A|' |X| |A| pushed through the same operations, for gamma the 2-norm of M."""
import math

import mpmath
import numpy as np

import clarabel_jl_amd  # noqa: F401
from julia_standin.cones import _ISQRT2, PSDTriangleCone

mp = mpmath.mp.clone()
mp.dps = 50
mpf = mp.mpf
EPS = float(np.finfo(np.float64).eps)
ISQRT2 = mpf(_ISQRT2)


# ---- matrices ------------------------------------------------------------------------------------------------------------------------

def M(a):
    """float64 array -> object array of 50-digit numbers (exact)"""
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    for idx, v in np.ndenumerate(a):
        out[idx] = mpf(float(v))
    return out


def _ints(A):
    """object array of mpf -> (object array of ints, e) with A = ints * 2^e, exactly"""
    parts = [x._mpf_ for x in A.ravel()]
    exps = [p[2] for p in parts if p[1] != 0]
    e = min(exps) if exps else 0
    ints = np.empty(A.size, dtype=object)
    for k, (sign, man, ex, _) in enumerate(parts):
        ints[k] = (-(int(man) << (ex - e)) if sign else (int(man) << (ex - e))) if man != 0 else 0
    return ints.reshape(A.shape), e


def mm(A, B):
    """A B, exact up to one rounding per entry"""
    Ai, ea = _ints(A)
    Bi, eb = _ints(B)
    Ci = Ai.dot(Bi)
    out = np.empty(Ci.shape, dtype=object)
    for idx, v in np.ndenumerate(Ci):
        out[idx] = mp.ldexp(mpf(int(v)), ea + eb)
    return out


def _idx(n):
    """(row, col) of the packed entries: column-major upper triangle"""
    r = np.array([i for j in range(n) for i in range(j + 1)])
    c = np.array([j for j in range(n) for i in range(j + 1)])
    return r, c


def svec_to_mat(x, n):
    x = M(x) if not (isinstance(x, np.ndarray) and x.dtype == object) else x
    X = np.empty((n, n), dtype=object)
    r, c = _idx(n)
    for k in range(len(r)):
        v = x[k] if r[k] == c[k] else x[k] * ISQRT2
        X[r[k], c[k]] = v
        X[c[k], r[k]] = v
    return X


def mat_to_svec(Y):
    n = Y.shape[0]
    r, c = _idx(n)
    return np.array([Y[r[k], c[k]] if r[k] == c[k] else (Y[r[k], c[k]] + Y[c[k], r[k]]) * ISQRT2 for k in range(len(r))], dtype=object)


def _svec_to_mat64(x, n):
    K = PSDTriangleCone(n)
    return K.svec_to_mat(np.asarray(x, dtype=np.float64))


def _mat_to_svec64(Y):
    K = PSDTriangleCone(Y.shape[0])
    return K.mat_to_svec(Y)


def err(got, ref):
    """|got - ref| per entry, float64"""
    return np.array([float(abs(mpf(float(g)) - r)) for g, r in zip(np.ravel(got), np.ravel(ref))])


# ---- the six operations ----------------------------------------------------------------------------------------------------------------

def ref_affine_ds(lam):
    n = len(lam)
    out = np.array([mpf(0)] * (n * (n + 1) // 2), dtype=object)
    for k in range(n):
        out[(k + 1) * (k + 2) // 2 - 1] = mpf(float(lam[k])) ** 2
    return out


def ref_mul_W(F, x, transpose):
    """mul_W (F = R) resp. mul_Winv (F = Rinv): :N  F' X F, :T  F X F'  -> (svec, scale)"""
    n = F.shape[0]
    Fm, X = M(F), svec_to_mat(x, n)
    Y = mm(mm(Fm, X), Fm.T) if transpose else mm(mm(Fm.T, X), Fm)
    Fa, Xa = np.abs(F), np.abs(_svec_to_mat64(x, n))
    Ya = Fa @ Xa @ Fa.T if transpose else Fa.T @ Xa @ Fa
    return mat_to_svec(Y), _mat_to_svec64(Ya)


def ref_mul_hs(R, x):
    n = R.shape[0]
    w, wa = ref_mul_W(R, x, False)
    Rm = M(R)
    Y = mm(mm(Rm, svec_to_mat(w, n)), Rm.T)
    Ra = np.abs(R)
    return mat_to_svec(Y), _mat_to_svec64(Ra @ _svec_to_mat64(wa, n) @ Ra.T)


def ref_shift(R, Rinv, dz, ds, sigma_mu):
    """combined_ds_shift: svec((B A + A B) / 2) - sigma mu on the diagonal, A = W dz, B = W^-T ds"""
    n = R.shape[0]
    a, aa = ref_mul_W(R, dz, False)
    b, ba = ref_mul_W(Rinv, ds, True)
    A, B = svec_to_mat(a, n), svec_to_mat(b, n)
    C = (mm(B, A) + mm(A, B)) * mpf(0.5)
    out = mat_to_svec(C)
    for k in range(n):
        out[(k + 1) * (k + 2) // 2 - 1] -= mpf(float(sigma_mu))
    Aa, Ba = _svec_to_mat64(aa, n), _svec_to_mat64(ba, n)
    scale = _mat_to_svec64(0.5 * (Ba @ Aa + Aa @ Ba))
    scale[[(k + 1) * (k + 2) // 2 - 1 for k in range(n)]] += abs(float(sigma_mu))
    return out, scale


def ref_offset(R, lam, ds):
    """ds_from_dz_offset: X~_ij = 2 DS_ij / (lambda_i + lambda_j), out = R X~ R'"""
    n = R.shape[0]
    D, l = svec_to_mat(ds, n), M(lam)
    Xt = np.empty((n, n), dtype=object)
    for i in range(n):
        for j in range(n):
            Xt[i, j] = 2 * D[i, j] / (l[i] + l[j])
    Xt = svec_to_mat(mat_to_svec(Xt), n)
    Rm = M(R)
    Y = mm(mm(Rm, Xt), Rm.T)
    lam = np.asarray(lam, dtype=np.float64)
    Xa = 2.0 * np.abs(_svec_to_mat64(ds, n)) / (lam[:, None] + lam[None, :])
    Ra = np.abs(R)
    return mat_to_svec(Y), _mat_to_svec64(Ra @ Xa @ Ra.T)


def ref_gamma(F, lam, d, transpose):
    """-> (gamma = lambda_min(M), |M|_2) for M = Lambda^-1/2 svec_to_mat(mul_W(d)) Lambda^-1/2"""
    n = F.shape[0]
    w, _ = ref_mul_W(F, d, transpose)
    D = svec_to_mat(w, n)
    li = [1 / mp.sqrt(mpf(float(v))) for v in lam]
    Mm = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            Mm[i, j] = (li[i] * D[i, j]) * li[j]
    ev = mp.eigsy(Mm, eigvals_only=True)
    ev = [ev[k] for k in range(n)]
    return min(ev), float(max(abs(e) for e in ev))


def alpha_of(gamma, alpha_max):
    return min(1 / (-gamma), mpf(float(alpha_max))) if gamma < 0 else mpf(float(alpha_max))


def ref_step_length(R, Rinv, lam, dz, ds, alpha_max):
    """-> ((alpha_z, alpha_s), (gamma_z, gamma_s), (|M_z|_2, |M_s|_2))"""
    gz, nz = ref_gamma(R, lam, dz, False)
    gs, ns = ref_gamma(Rinv, lam, ds, True)
    return (alpha_of(gz, alpha_max), alpha_of(gs, alpha_max)), (gz, gs), (nz, ns)


def alpha_allowance(gamma, norm2, ratio):
    """the allowance of alpha = 1 / -gamma when gamma may be off by ratio eps |M|_2 (first order), plus one rounding of the division;
    0 where the reference gives alpha_max (gamma >= 0)"""
    g = float(gamma)
    if g >= 0:
        return 0.0
    return ratio * EPS * norm2 / (g * g) + EPS / (-g)


# ---- scaled points ---------------------------------------------------------------------------------------------------------------------

def _orth(n, rng):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return Q


def spd(n, cond, rng):
    """a random symmetric positive definite matrix with the given condition number (eigenvalues log-spaced in [1 / cond, 1])"""
    Q = _orth(n, rng)
    ev = np.logspace(0.0, -math.log10(cond), n) if n > 1 else np.ones(1)
    S = (Q * ev) @ Q.T
    return 0.5 * (S + S.T)


def random_sz(K, rng, late=False, cond=1e3):
    """-> (s, z, mu) for the cone K: random symmetric positive definite S, Z with condition number `cond`;
    late: S Z ~ mu I at mu = 1e-9 with cond(S) ~ 1e8 (a late interior-point iterate)"""
    n = K.n
    if late:
        mu = 1e-9
        Q = _orth(n, rng)
        ls = 10.0 ** rng.uniform(-8.0, 0.0, n)
        ls[0] = 1.0
        if n > 1:
            ls[-1] = 1e-8
        S = (Q * ls) @ Q.T
        Z = (Q * (mu / ls * (1.0 + 0.1 * rng.random(n)))) @ Q.T
        S, Z = 0.5 * (S + S.T), 0.5 * (Z + Z.T)
    else:
        mu = 1.0
        S, Z = spd(n, cond, rng), spd(n, cond, rng)
    return K.mat_to_svec(S), K.mat_to_svec(Z), mu


def scaled_point(n, rng, late=False, cond=1e3):
    """-> (cone, s, z): a PSDTriangleCone of side n scaled at random_sz by the stand-in's update_scaling"""
    K = PSDTriangleCone(n)
    s, z, mu = random_sz(K, rng, late, cond)
    assert K.update_scaling(s, z, mu)
    return K, s, z


def direction(K, rng, scale_like):
    """a random symmetric direction in svec form, of the size of `scale_like` (an svec)"""
    D = rng.standard_normal((K.n, K.n))
    return K.mat_to_svec(0.5 * (D + D.T)) * float(np.max(np.abs(scale_like)))
