"""The Nesterov-Todd scaling of PSD triangle cones on the device (csrc/scaling_psd.hip, hipkkt_psd_scaling_enable): what
tests/test_psd_scaling_reference.py (CPU) and tests/test_gpu_psd_scaling.py (GPU) share.  No tests here.

1.  50-digit residuals of a float64 (R, Rinv, lambda) against the float64 (S, Z) it was computed from.  R is unique only up to column
    signs and, among equal singular values, rotations, so nothing compares R entry by entry; the residuals are products only (the exact
    product `mm` of tests/psd_step_reference.py), each with the float64 scale its error is stated in:
      1  R' Z R - diag(lambda)            scale |R|' |Z| |R|
      2  Rinv S Rinv' - diag(lambda)      scale |Rinv| |S| |Rinv|'
      3  Rinv R - I                       scale |Rinv| |R|
      4  W Z W - S, W = R R'              scale |W| |Z| |W|, |W| = |R| |R|'      (W is the unique NT point: this pins W and, through skron, K)
      5  lambda against sqrt(eigsy(L1' Z L1)), L1 the 50-digit Cholesky factor of S, relative; n <= 17 only (the decomposition is slow)
    and the packed triu(skron(W)) of W = R R' evaluated exactly, with the scale skron(|R| |R|'), for the PSD block of K.
2.  `emulate`: the kernel's algorithm in numpy, operation by operation -- the right-looking Cholesky with its k-sums in ascending
    order, G = L2' L1 summed from k = max(i, j), the round-robin pairs, the eight-lane partial sums with their butterfly, the rotation
    formulas in the small-angle form, the stopping rule with its polishing sweep, the two output products, the refinement of lambda in twice the precision with
    the rescaling of R and Rinv, the sort by counting.  numpy rounds a * b + c as a
    product and a sum, which is what -ffp-contract=off makes of the kernel's expressions.
3.  The test family: sides, early / late points (psd_step_reference.random_sz) and the edge cases.

The gate (the project's PSD rule, tests/test_gpu_psd_step.py): an error in units of eps x scale must be at most
max(8 x the host's error in the same case, 2 n), the host being the stand-in's PSDTriangleCone.update_scaling (LAPACK potrf / gesdd) on
the same float64 (s, z)."""
import math
import os
import re

import numpy as np

import clarabel_jl_amd  # noqa: F401
from julia_standin.cones import PSDTriangleCone
from tests import psd_step_reference as pr

mp, mpf, EPS = pr.mp, pr.mpf, pr.EPS
SIDES = (1, 2, 3, 5, 8, 17, 32, 33, 63, 64)
SEEDS = (0, 1, 2)
LAMBDA_REF_MAX_N = 17
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def max_sweeps_in_source():
    src = open(os.path.join(ROOT, "clarabel.jl_amd", "csrc", "scaling_psd.hip")).read()
    return int(re.search(r"constexpr\s+int\s+kMaxSweeps\s*=\s*(\d+)\s*;", src).group(1))


# ---- the family -------------------------------------------------------------------------------------------------------------------------

def _sym(A):
    return 0.5 * (A + A.T)


def edge_cases(n, rng):
    """name -> (S, Z), float64 symmetric positive definite"""
    Q = pr._orth(n, rng)
    a = 0.5 + rng.random(n)
    b = 0.5 + rng.random(n)
    if n > 1:
        b[1] = a[0] * b[0] / a[1]                      # lambda_0 = lambda_1 = sqrt(a_0 b_0)
    S3 = pr.spd(n, 1e3, rng)
    Sinv = _sym(np.linalg.inv(S3))
    return {
        "identity": (np.eye(n), np.eye(n)),
        "S_equals_Z": (S3.copy(), S3.copy()),                                  # lambda = eig(S)
        "diagonal": (np.diag(0.1 + rng.random(n)), np.diag(0.1 + 10.0 * rng.random(n))),
        "two_fold": (_sym((Q * a) @ Q.T), _sym((Q * b) @ Q.T)),                # S, Z commute: lambda_i = sqrt(a_i b_i)
        "n_fold": (S3.copy(), 4.0 * Sinv),                                     # every lambda = 2
        "Z_is_S_inverse": (S3.copy(), Sinv),                                   # every lambda = 1
    }


def points(n):
    """[(name, s, z)]: early (cond 1e3) and late (S Z ~ mu I, mu = 1e-9, cond 1e8) at three seeds, then the edge cases"""
    K = PSDTriangleCone(n)
    out = []
    for late in (False, True):
        for seed in SEEDS:
            s, z, _ = pr.random_sz(K, np.random.default_rng(1000 * n + 10 * seed + late), late)
            out.append((f"{'late' if late else 'early'}_{seed}", s, z))
    for name, (S, Z) in edge_cases(n, np.random.default_rng(7000 + n)).items():
        out.append((name, K.mat_to_svec(S), K.mat_to_svec(Z)))
    return out


def host_factors(n, s, z):
    """(R, Rinv, lambda) of the stand-in's update_scaling"""
    K = PSDTriangleCone(n)
    assert K.update_scaling(np.asarray(s, dtype=np.float64), np.asarray(z, dtype=np.float64), 1.0)
    return K.R.copy(), K.Rinv.copy(), K.lam.copy()


# ---- 50-digit residuals -----------------------------------------------------------------------------------------------------------------

def _ratio(E, scale):
    """max |E| / (eps scale); an entry of scale 0 must be exact"""
    worst = 0.0
    for e, sc in zip(np.ravel(E), np.ravel(scale)):
        e = float(abs(e))
        if sc > 0:
            worst = max(worst, e / (EPS * float(sc)))
        elif e > 0:
            return math.inf
    return worst


class Reference:
    """the 50-digit side of one (s, z): built once, shared by the device's and the host's residuals"""

    def __init__(self, n, s, z):
        K = PSDTriangleCone(n)
        self.n = n
        self.S64, self.Z64 = K.svec_to_mat(np.asarray(s, dtype=np.float64)), K.svec_to_mat(np.asarray(z, dtype=np.float64))
        self.S, self.Z = pr.M(self.S64), pr.M(self.Z64)
        self.lam_ref = None
        if n <= LAMBDA_REF_MAX_N:
            L1 = mp.cholesky(mp.matrix(self.S.tolist()))
            L1 = np.array([[L1[i, j] for j in range(n)] for i in range(n)], dtype=object)
            T = pr.mm(pr.mm(L1.T, self.Z), L1)
            ev = mp.eigsy(mp.matrix(_sym_obj(T).tolist()), eigvals_only=True)
            self.lam_ref = sorted((mp.sqrt(ev[k]) for k in range(n)), reverse=True)

    def residuals(self, R, Rinv, lam):
        """-> {1..5: error in units of eps x scale}"""
        n = self.n
        Rm, Rim = pr.M(R), pr.M(Rinv)
        Ra, Ria, Sa, Za = np.abs(R), np.abs(Rinv), np.abs(self.S64), np.abs(self.Z64)
        D = np.zeros((n, n), dtype=object)
        for k in range(n):
            D[k, k] = mpf(float(lam[k]))
        Id = np.zeros((n, n), dtype=object)
        for k in range(n):
            Id[k, k] = mpf(1)
        out = {}
        out[1] = _ratio(pr.mm(pr.mm(Rm.T, self.Z), Rm) - D, Ra.T @ Za @ Ra)
        out[2] = _ratio(pr.mm(pr.mm(Rim, self.S), Rim.T) - D, Ria @ Sa @ Ria.T)
        out[3] = _ratio(pr.mm(Rim, Rm) - Id, Ria @ Ra)
        W, Wa = pr.mm(Rm, Rm.T), Ra @ Ra.T
        out[4] = _ratio(pr.mm(pr.mm(W, self.Z), W) - self.S, Wa @ Za @ Wa)
        if self.lam_ref is not None:
            out[5] = max(float(abs(mpf(float(l)) - r) / r) for l, r in zip(lam, self.lam_ref)) / EPS
        return out


GROUPS = ("early", "late", "edges")
_cases = {}


def cases(n, group):
    """[(name, s, z, Reference, the host's residuals)] of one side and group ("early" / "late": three seeds, "edges"), computed once
    per process and shared by the CPU and the GPU tests"""
    if (n, group) not in _cases:
        pts = [p for p in points(n) if (p[0].split("_")[0] == group if group != "edges" else p[0].split("_")[0] not in ("early", "late"))]
        out = []
        for name, s, z in pts:
            ref = Reference(n, s, z)
            out.append((name, s, z, ref, ref.residuals(*host_factors(n, s, z))))
        _cases[(n, group)] = out
    return _cases[(n, group)]


def _sym_obj(T):
    return (T + T.T) * mpf(0.5)


def gate(what, n, dev, host, misses=None):
    """asserts the project's PSD rule for every residual of one case; -> the worst device / host ratio (host errors floored at 1 eps).
    misses: a list that collects the cases over the gate instead, for a caller that asserts it empty after its other checks"""
    worst = 0.0
    for k in sorted(dev):
        allowed = max(8.0 * host[k], 2.0 * n)
        print(f"[psd scaling] {what} n={n} residual {k}: device {dev[k]:.3f}, host {host[k]:.3f}, allowed {allowed:.1f} (eps x scale)")
        if misses is not None and not dev[k] <= allowed:
            misses.append((what, n, k, dev[k], host[k]))
            continue
        assert dev[k] <= allowed, (what, n, k, dev[k], host[k])
        worst = max(worst, dev[k] / max(host[k], 1.0))
    return worst


# ---- triu(skron(W)) of W = R R', exactly ------------------------------------------------------------------------------------------------

_pairs = {}


def _packed_pairs(n):
    """(i, j, k, l) of the packed entries of the block: entry (a, b), a <= b, a = (i, j), b = (k, l); per side, computed once"""
    if n not in _pairs:
        r, c = pr._idx(n)
        numel = len(r)
        cols = np.repeat(np.arange(numel), np.arange(1, numel + 1))
        rows = np.arange(len(cols)) - (cols * (cols + 1)) // 2
        _pairs[n] = (r[rows], c[rows], r[cols], c[cols])
    return _pairs[n]


def _exact_error(v, ref, ex):
    """|v - ref 2^ex| per entry as float64, exactly up to the last conversion: v float64, ref an object array of integers"""
    m_, e_ = np.frexp(v)
    vi = (m_ * float(1 << 53)).astype(np.int64).astype(object)              # v = vi 2^(e_ - 53), exactly
    sh = e_.astype(np.int64) - 53
    lo = min(int(sh.min()), ex)
    for u in np.unique(sh):                                                 # (a few hundred distinct exponents at most)
        if u != lo:
            m = sh == u
            vi[m] = vi[m] * (1 << int(u - lo))
    if ex != lo:
        ref = ref * (1 << (ex - lo))
    d = np.abs(vi - ref)
    if lo > -900:
        return np.ldexp(d.astype(np.float64), lo)
    # entries of R far below 1e-100 (products of many small rotations) put the common exponent out of float64's range: per entry
    return np.array([math.ldexp(float(x >> max(x.bit_length() - 64, 0)), lo + max(x.bit_length() - 64, 0)) for x in d])


def skron_error(R, block):
    """block = the packed upper triangle (column-major, numel (numel + 1) / 2 doubles) of a float64 W (x)_s W computed from W = R R';
    -> its error against skron of the exact R R' (coneops_psdtrianglecone.jl:502-540; sqrt 2 is the float64 constant, taken as given like
    every input), in units of eps x skron(|R| |R|').  W at 50 digits as integers x 2^e; the products of skron are then exact integer arithmetic."""
    n = R.shape[0]
    Wi, e = pr._ints(pr.mm(pr.M(R), pr.M(R).T))                             # W = Wi 2^e: R R' rounded once per entry at 50 digits
    Wa = np.abs(R) @ np.abs(R).T
    i, j, k, l = _packed_pairs(n)
    block = np.asarray(block, dtype=np.float64)
    s2 = mpf(math.sqrt(2.0))
    s2i, s2e = int(s2.man), int(s2.exp)
    sc2 = math.sqrt(2.0)
    ij, kl = i == j, k == l
    err, scale = np.zeros(len(block)), np.zeros(len(block))
    # the four cases of skron!, each on its own exponent: i != j, k != l: W_ik W_jl + W_il W_jk;  i == j, k != l: (sqrt2 W_jl) W_jk;
    # i != j, k == l: (sqrt2 W_il) W_jk;  i == j, k == l: W_jl W_jl
    for m, a, b, c2, d2, root in ((~ij & ~kl, (i, k), (j, l), (i, l), (j, k), False), (ij & ~kl, (j, l), (j, k), None, None, True),
                                  (~ij & kl, (i, l), (j, k), None, None, True), (ij & kl, (j, l), (j, l), None, None, False)):
        if not m.any():
            continue
        ref = Wi[a[0][m], a[1][m]] * Wi[b[0][m], b[1][m]]
        sc = Wa[a[0][m], a[1][m]] * Wa[b[0][m], b[1][m]]
        if c2 is not None:
            ref = ref + Wi[c2[0][m], c2[1][m]] * Wi[d2[0][m], d2[1][m]]
            sc = sc + Wa[c2[0][m], c2[1][m]] * Wa[d2[0][m], d2[1][m]]
        if root:
            ref, sc = ref * s2i, sc2 * sc
        err[m] = _exact_error(block[m], ref, 2 * e + (s2e if root else 0))
        scale[m] = sc
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(scale > 0, err / (EPS * scale), np.where(err > 0, np.inf, 0.0))
    return float(np.max(q))


# ---- the kernel's algorithm in numpy ----------------------------------------------------------------------------------------------------

def _pos_finite(v):
    return v > 0.0 and math.isfinite(v)


def _sum8(P):
    """P[l] = the partial sum of lane l (8 x ...): the butterfly xor 4, 2, 1 as lane 0 adds it (every lane gets the same bits)"""
    a = P[[0, 1, 2, 3]] + P[[4, 5, 6, 7]]
    b = a[[0, 1]] + a[[2, 3]]
    return b[0] + b[1]


def _lane_sums(X, Y):
    """sum_i X[i] Y[i] over the rows, per column: lane l adds rows l, l + 8, .. in ascending order, then the butterfly"""
    n = X.shape[0]
    rows = -(-n // 8)
    pad = np.zeros((8 * rows - n,) + X.shape[1:])
    P = (np.concatenate([X, pad]) * np.concatenate([Y, pad])).reshape((rows, 8) + X.shape[1:])
    acc = np.zeros((8,) + X.shape[1:])
    for r in range(rows):
        acc = acc + P[r]
    return _sum8(acc)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """(p, e) with p + e = a b exactly: what fma(a, b, -p) gives the kernel, here by Dekker's splitting"""
    p = a * b
    f = 134217729.0
    ah = (a * f) - ((a * f) - a)
    bh = (b * f) - ((b * f) - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_add(x, y):
    s, t = _two_sum(x[0], y[0])
    return s, (x[1] + y[1]) + t


def _lanes4(H, L):
    """the four lanes' pairs (rows l, l + 4, .. already summed: arrays 4 x n) -> one pair per column: xor 2, then xor 1"""
    a = _dd_add((H[[0, 1]], L[[0, 1]]), (H[[2, 3]], L[[2, 3]]))
    h, l = _dd_add((a[0][0], a[1][0]), (a[0][1], a[1][1]))
    hn = h + l                                       # normalised: the high part is the rounded sum
    return hn, l - (hn - h)


def _dot2_lanes(X, Y, Ylo):
    """per column j: sum_i X[i, j] (Y[i, j] + Ylo[i, j]) in twice the precision; lane l of four adds rows l, l + 4, .. in ascending order"""
    n = X.shape[0]
    H, L = np.zeros((4, X.shape[1])), np.zeros((4, X.shape[1]))
    for i in range(n):
        l = i % 4
        p, e = _two_prod(X[i], Y[i])
        sm, t = _two_sum(H[l], p)
        L[l] = L[l] + ((t + e) + (X[i] * Ylo[i] if Ylo is not None else 0.0))
        H[l] = sm
    return _lanes4(H, L)


def _quad2(M, X):
    """per column j: x_j' M x_j in twice the precision: y = M x_j with the k-sums in ascending order, then the lanes' sums over the rows"""
    n = M.shape[0]
    H, L = np.zeros_like(X), np.zeros_like(X)
    for k in range(n):
        p, e = _two_prod(M[:, k][:, None] * np.ones_like(X), X[k][None, :] * np.ones_like(X))
        sm, t = _two_sum(H, p)
        L = L + (t + e)
        H = sm
    return _dot2_lanes(X, H, L)


def _cholesky_lower(A):
    """right-looking, in place on a copy; None when a pivot is not > 0 or not finite"""
    A = A.copy()
    n = A.shape[0]
    for j in range(n):
        d = A[j, j]
        if not _pos_finite(d):
            return None
        piv = math.sqrt(d)
        col = A[j + 1:, j] / piv
        A[j + 1:, j] = col
        A[j + 1:, j + 1:] = A[j + 1:, j + 1:] - np.outer(col, col)
    A[np.diag_indices(n)] = np.sqrt(np.diag(A))
    return np.tril(A)


def emulate(n, s, z, max_sweeps=None):
    """-> (R, Rinv, lambda, sweeps) as k_psd_nt_scaling computes them, or None where it fails the cone.  `sweeps` counts the sweeps that
    ran against kMaxSweeps: the last one (without a rotation) included, the polishing sweep not."""
    max_sweeps = max_sweeps_in_source() if max_sweeps is None else max_sweeps
    K = PSDTriangleCone(n)
    with np.errstate(all="ignore"):
        L1 = _cholesky_lower(K.svec_to_mat(np.asarray(s, dtype=np.float64)))
        L2 = _cholesky_lower(K.svec_to_mat(np.asarray(z, dtype=np.float64)))
        if L1 is None or L2 is None:
            return None
        G = np.zeros((n, n))
        for k in range(n):                               # the terms k < max(i, j) are zeros of the triangles: the sum starts at max(i, j)
            G = G + np.outer(L2[k, :], L1[k, :])
        V = np.eye(n)
        npad = n + (n & 1)
        half = npad // 2
        ks = np.arange(half)
        sweeps, converged = 0, False
        for sweep in range(max_sweeps + 1):
            # after the sweep without a rotation: one polishing sweep that rotates every pair with c != 0
            polish = converged
            if not polish and sweep == max_sweeps:
                break
            sweeps += 0 if polish else 1
            nrot = 0
            for r in range(npad - 1):
                a_ = np.where(ks == 0, npad - 1, (r + ks) % (npad - 1))
                b_ = (r + npad - 1 - ks) % (npad - 1)
                p, q = np.minimum(a_, b_), np.maximum(a_, b_)
                live = q < n
                p, q = p[live], q[live]
                if p.size == 0:
                    continue
                Gp, Gq = G[:, p], G[:, q]
                a, b, c = _lane_sums(Gp, Gp), _lane_sums(Gq, Gq), _lane_sums(Gp, Gq)
                rot = (c != 0.0) if polish else np.abs(c) > EPS * np.sqrt(a * b)
                if not rot.any():
                    continue
                p, q, a, b, c = p[rot], q[rot], a[rot], b[rot], c[rot]
                zeta = (b - a) / (2.0 * c)
                tt = np.where(zeta >= 0.0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                cs = 1.0 / np.sqrt(1.0 + tt * tt)
                sn = tt * cs
                rr = sn / (1.0 + cs)
                for Mx in (G, V):
                    x, y = Mx[:, p], Mx[:, q]
                    Mx[:, p] = x - sn * (y + rr * x)
                    Mx[:, q] = y + sn * (x - rr * y)
                nrot += int(rot.sum())
            if polish:
                break
            if nrot == 0:
                converged = True
        if not converged:
            return None
        sig = np.sqrt(_lane_sums(G, G))
        if not all(_pos_finite(float(v)) for v in sig):
            return None
        lis = 1.0 / np.sqrt(sig)
        acc = np.zeros((n, n))
        for k in range(n):
            acc = acc + np.outer(L1[:, k], V[k, :])
        Ru = acc * lis[None, :]                          # column j of R, not sorted yet
        acc = np.zeros((n, n))
        for k in range(n):
            acc = acc + np.outer(G[k, :], L2[:, k])
        Qu = (acc * (lis / sig)[:, None]).T              # column j = row j of Rinv
        # the refinement: lambda_j^2 = (r_j' Z r_j)(q_j' S q_j) / (q_j' r_j)^2, stationary in r_j and q_j, sums in twice the precision
        S, Z = K.svec_to_mat(np.asarray(s, dtype=np.float64)), K.svec_to_mat(np.asarray(z, dtype=np.float64))
        t1, t2, t3 = _quad2(Z, Ru), _quad2(S, Qu), _dot2_lanes(Qu, Ru, None)
        lam_u, fa, fb = sig.copy(), np.ones(n), np.ones(n)
        for j in range(n):
            (h1, l1), (h2, l2), (h3, l3) = (t1[0][j], t1[1][j]), (t2[0][j], t2[1][j]), (t3[0][j], t3[1][j])
            p, e = _two_prod(h1, h2)
            e = e + (h1 * l2 + l1 * h2)
            x0 = np.sqrt(p)
            q, qe = _two_prod(x0, x0)
            x = x0 + (((p - q) - qe) + e) / (2.0 * x0)      # the square root of p + e: fma(-x0, x0, p) + e in the kernel
            v = x / h3
            v = v - v * (l3 / h3)
            if _pos_finite(float(v)) and _pos_finite(float(h1)) and _pos_finite(float(h2)):
                lam_u[j], fa[j], fb[j] = v, np.sqrt(v / h1), np.sqrt(v / h2)
        idx = np.arange(n)
        rank = np.array([int(np.sum((lam_u > lam_u[t]) | ((lam_u == lam_u[t]) & (idx < t)))) for t in range(n)])
        lam = np.empty(n)
        lam[rank] = lam_u
        R = np.empty((n, n))
        R[:, rank] = Ru * fa[None, :]
        Rinv = np.empty((n, n))
        Rinv[rank, :] = (Qu * fb[None, :]).T
    return R, Rinv, lam, sweeps
