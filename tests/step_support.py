"""Helpers that the tests of the device-resident interior-point step share: constants and gates, problem builders, the second-order
cones' reference expressions with their allowances, the symmetric twin handle, the barrier check, and the host-side plugins that stand
in for the device in the tests that need no GPU.  A plain module: it holds no test and changes no pytest setting."""
import math
import signal

import numpy as np
import scipy.sparse as sp

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd.cone_api import nvars
from clarabel_jl_amd.kktsolver import HipKKTSolver
from julia_standin import cones_nonsym as cn
from julia_standin import ipm
from julia_standin.cones import NonnegativeCone, SecondOrderCone, ZeroCone

SUM_TOL = 1e-13
PARITY = 1e-10
SQRT_EPS = math.sqrt(float(np.finfo(np.float64).eps))
STEP_FLAGS = dict(device_scaling=True, device_reduced=True, device_residuals=True)
NONSYM = dict(device_step=True, device_step_nonsymmetric=True, **STEP_FLAGS)
STEP_SETTINGS = dict(device_step=True, device_scaling=True, device_reduced=True, device_residuals=True)
NONSYM_SETTINGS = dict(STEP_SETTINGS, device_step_nonsymmetric=True)


class _Timeout:
    """a time limit of its own for one case (SIGALRM: raises in the interpreter)"""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        def fire(*_):
            raise TimeoutError(f"case exceeded {self.seconds} s")
        self.old = signal.signal(signal.SIGALRM, fire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        signal.signal(signal.SIGALRM, self.old)


# ---- problems and handles ----------------------------------------------------------------------------------------------------------------

def _mixed_problem(seed, n=24):
    """Zero, Nonnegative, sparse second-order cones (dim 6, 101) and dense ones (dim 2, 3, 4)"""
    rng = np.random.default_rng(seed)
    specs = [cl.ZeroConeT(3), cl.NonnegativeConeT(37), cl.SecondOrderConeT(6), cl.SecondOrderConeT(2), cl.SecondOrderConeT(101),
             cl.NonnegativeConeT(300), cl.SecondOrderConeT(3), cl.SecondOrderConeT(4), cl.ZeroConeT(1)]
    m = sum(nvars(c) for c in specs)
    A = sp.random(m, n, density=0.15, random_state=np.random.RandomState(seed), format="csc") + \
        sp.vstack([sp.identity(n), sp.csc_matrix((m - n, n))]).tocsc()
    Pm = sp.random(n, n, density=0.1, random_state=np.random.RandomState(seed + 1))
    P = (Pm @ Pm.T + sp.identity(n)).tocsc()
    return P, rng.standard_normal(n), A.tocsc(), rng.standard_normal(m), specs


def _problem(specs, seed):
    rng = np.random.default_rng(seed)
    m = sum(nvars(c) for c in specs)
    n = min(6, m)
    A = sp.random(m, n, density=min(1.0, 12.0 / m + 0.2), random_state=np.random.RandomState(seed), format="csc") + \
        sp.vstack([sp.identity(n), sp.csc_matrix((m - n, n))]).tocsc()
    P = sp.identity(n, format="csc") * 1.5
    return P, rng.standard_normal(n), A.tocsc(), rng.standard_normal(m), specs


def _prep(prob):
    P, q, A, b, specs = prob
    cones = cl.CompositeCone(cl.cones_new_collapsed(specs))
    Pt = sp.triu(sp.csc_matrix(P), format="csc")
    Pt.sort_indices()
    A = sp.csc_matrix(A)
    A.sort_indices()
    return Pt, A, cones


def _adopt(cones, w, lam, eta):
    k = 0
    for c, r in zip(cones.cones, cones.rng_cones):
        if isinstance(c, SecondOrderCone):
            c.adopt_symmetric_scaling(w[r], lam[r], eta[k])
            k += 1
        elif isinstance(c, NonnegativeCone):
            assert np.array_equal(c.w, w[r]) and np.array_equal(c.lam, lam[r])      # bit-exact already (test_gpu_kkt.py)


def _is3(c):
    return isinstance(c, cn._Cone3)


def _symmetric_twin_handle(cones, seed):
    specs, rows = [], []
    for c, r in zip(cones.cones, cones.rng_cones):
        if getattr(c, "is_symmetric", True):
            specs.append({0: cl.ZeroConeT, 1: cl.NonnegativeConeT, 2: cl.SecondOrderConeT}[c.kind_code](c.numel))
            rows.extend(range(r.start, r.stop))
    if not specs:
        return None, None
    Pt, A, tc = _prep(_problem(specs, seed + 90))
    m, n = A.shape
    twin = HipKKTSolver(Pt, A, tc, m, n, cl.Settings())
    assert twin.steps_on_device and not twin.steps_nonsymmetric
    return twin, np.array(rows)


def _twin_step_length(twin, rows, dz, ds, alpha_max):
    """min(alpha_z, alpha_s) of the symmetric cones from the device's own kernels (alpha_max without such cones)"""
    return alpha_max if twin is None else min(twin.cone_step_length(dz[rows], ds[rows], alpha_max))


# ---- the reference's second-order-cone expressions with a pluggable `dot`, for the allowance of a result that is a function of sums ------

class _Sums:
    """dot products in evaluation order; `bump` moves the k-th one by its allowance SUM_TOL * sum|terms|"""

    def __init__(self, bump=None):
        self.k, self.bump = 0, bump

    def dot(self, a, b):
        v = float(np.dot(a, b))
        if self.k == self.bump:
            v += SUM_TOL * float(np.dot(np.abs(a), np.abs(b)))
        self.k += 1
        return v


def _resid(S, z):
    z1 = math.sqrt(S.dot(z[1:], z[1:]))
    return (z[0] - z1) * (z[0] + z1)


def _soc_affine_ds(S, K):
    out = np.empty(K.dim)
    out[0] = S.dot(K.lam, K.lam)
    out[1:] = K.lam[0] * K.lam[1:] + K.lam[0] * K.lam[1:]
    return out


def _soc_shift(S, K, dz, ds, sm):
    w, eta = K.w, K.eta
    zz, zs = S.dot(w[1:], dz[1:]), S.dot(w[1:], ds[1:])
    zW, sW = np.empty(K.dim), np.empty(K.dim)
    zW[0] = eta * (w[0] * dz[0] + zz)
    zW[1:] = eta * (dz[1:] + (dz[0] + zz / (1.0 + w[0])) * w[1:])
    sW[0] = (1.0 / eta) * (w[0] * ds[0] - zs)
    sW[1:] = (1.0 / eta) * (ds[1:] + (-ds[0] + zs / (1.0 + w[0])) * w[1:])
    out = np.empty(K.dim)
    out[0] = S.dot(sW, zW) - sm
    out[1:] = sW[0] * zW[1:] + zW[0] * sW[1:]
    return out


def _soc_offset(S, K, z, ds):
    resz = _resid(S, z)
    l1, w1 = S.dot(K.lam[1:], ds[1:]), S.dot(K.w[1:], ds[1:])
    out = -z.copy()
    out[0] = z[0]
    out *= (K.lam[0] * ds[0] - l1) / resz
    out[0] += K.eta * w1
    out[1:] += K.eta * (ds[1:] + w1 / (1.0 + K.w[0]) * K.w[1:])
    return out * (1.0 / K.lam[0])


def _soc_mul_hs(S, K, x):
    c = 2.0 * S.dot(K.w, x)
    y = x.copy()
    y[0] = -x[0]
    return (y + c * K.w) * (K.eta * K.eta)


def _allowance(fn, nsums, *args):
    """first-order propagation of every sum's allowance through fn, plus SUM_TOL of the element itself"""
    ref = fn(_Sums(), *args)
    tol = SUM_TOL * np.abs(ref) + 1e-300
    for k in range(nsums):
        tol = tol + np.abs(fn(_Sums(k), *args) - ref)
    return ref, tol


def _check_cone_vector(cones, got, ref, soc_allowance, what):
    """Zero / Nonnegative rows bit-identical to the stand-in's `ref`; second-order rows within soc_allowance(cone, range)"""
    for c, r in zip(cones.cones, cones.rng_cones):
        if isinstance(c, (ZeroCone, NonnegativeCone)):
            assert np.array_equal(got[r], ref[r]), (what, type(c).__name__)
        else:
            twin, tol = soc_allowance(c, r)
            assert np.all(np.abs(twin - ref[r]) <= tol), (what, "the test's twin of the reference expressions drifted")
            err = np.abs(got[r] - ref[r])
            print(f"[device-step {what}] SOC({c.dim}): max |got - ref| / allowance = {float(np.max(err / tol)):.3f}, "
                  f"relative to max |ref| = {float(np.max(err) / max(np.max(np.abs(ref[r])), 1e-300)):.2e}")
            assert np.all(err <= tol), (what, c.dim, float(np.max(err / tol)))


# ---- the barrier of a cone set against the stand-in --------------------------------------------------------------------------------------

def _barrier_reference(cones, z, s, dz, ds, a):
    terms = [c.compute_barrier(z[r], s[r], dz[r], ds[r], a) for c, r in zip(cones.cones, cones.rng_cones)]
    zz, ss = z + a * dz, s + a * ds
    return float(sum(terms)), float(sum(abs(t) for t in terms)), float(np.dot(zz, ss)), float(np.dot(np.abs(zz), np.abs(ss)))


def _check_barrier(bars, dots, cones, z, s, dz, ds, alphas, what):
    worst_b = worst_d = 0.0
    for a, b, d in zip(alphas, bars, dots):
        rb, tb, rd, td = _barrier_reference(cones, z, s, dz, ds, a)
        eb, ed = abs(b - rb) / max(1.0, tb), abs(d - rd) / max(td, 1e-300)
        worst_b, worst_d = max(worst_b, eb), max(worst_d, ed)
        assert eb <= PARITY, (what, a, b, rb)
        assert ed <= SUM_TOL, (what, a, d, rd)
    print(f"[nonsym barrier {what}] max |barrier - ref| / max(1, sum |terms|) = {worst_b:.2e}, max |dot - ref| / sum |terms| = {worst_d:.2e}")


# ---- the step plugins served on the host (the tests without a GPU) -----------------------------------------------------------------------

class _HostBuffer:
    """what the plugin hands out as device memory, here a numpy array"""

    def __init__(self, n):
        self.a = np.zeros(n)

    def upload(self, host):
        self.a[:] = host

    def download(self):
        return self.a.copy()

    def copy_from(self, other):
        self.a[:] = other.a

    def close(self):
        pass


class _Data:
    pass


class _FakeStepPlugin:
    """The plugin interface of the device_step loop (clarabel.jl_amd/kktsolver.py) served on the host: the KKT solves by the CPU
    oracle, the cone algebra by the stand-in's numpy cones and its own kkt_solve -- exactly what the host loop computes, so the two
    trajectories must coincide bit for bit if the loop hands the right quantities over in the right order."""
    steps_on_device = True

    def __init__(self, P, A, cones, m, n, settings):
        from oracle.kkt_oracle import OracleKKTSolver

        self.settings = settings
        self.inner = OracleKKTSolver(P, A, cones, m, n, settings)
        self.cones, self.m, self.n = cones, m, n
        self.data = _Data()
        self.data.P, self.data.A = P, A
        self.sys = ipm.KKTSystem(self.inner, m, n)
        self.lhs, self.rhs = ipm.Variables.zeros(n, m), ipm.Variables.zeros(n, m)
        self.calls = []

    # the contract methods the default start needs
    def kktsolver_update(self, cones):
        return self.inner.kktsolver_update(cones)

    def kktsolver_setrhs(self, rx, rz):
        self.inner.kktsolver_setrhs(rx, rz)

    def kktsolver_solve(self, lx, lz):
        return self.inner.kktsolver_solve(lx, lz)

    def set_problem_vectors(self, q, b):
        self.data.q, self.data.b = q, b

    def set_equilibration(self, d, e):
        self.d, self.e, self.dinv, self.einv = d, e, 1.0 / d, 1.0 / e

    def device_buffer(self, n):
        return _HostBuffer(n)

    def _split(self, xzs):
        n, m = self.n, self.m
        return xzs.a[:n], xzs.a[n:n + m], xzs.a[n + m:]

    def _res(self, res):
        n, m = self.n, self.m
        o = np.cumsum([0, n, m, n, m, n])
        return [res.a[o[k]:o[k + 1]] for k in range(5)]

    def residuals_update_dev(self, xzs, res, tau, kappa):      # residuals.jl:1-37 as ipm.Solver._residuals_update
        self.calls.append("residuals")
        x, z, s = self._split(xzs)
        rx, rz, rx_inf, rz_inf, Px = self._res(res)
        d = self.data
        qx, bz, sz = float(np.dot(d.q, x)), float(np.dot(d.b, z)), float(np.dot(s, z))
        Px[:] = ipm._symv(d.P, x)
        xPx = float(np.dot(x, Px))
        rx_inf[:] = -(d.A.T @ z)
        rz_inf[:] = s + d.A @ x
        rx[:] = rx_inf - Px - d.q * tau
        rz[:] = rz_inf - d.b * tau
        return qx, bz, sz, xPx, qx + bz + kappa + xPx / tau

    def kktsolver_info_norms(self, xzs, res):
        self.calls.append("norms")
        x, z, s = self._split(xzs)
        rx, rz, rx_inf, rz_inf, Px = self._res(res)
        ns = ipm._norm_scaled
        return [ns(self.d, x), ns(self.e, z), ns(self.einv, s), ns(self.dinv, rx), ns(self.einv, rz), ns(self.dinv, rx_inf),
                ns(self.einv, rz_inf), ns(self.dinv, Px)]

    def kktsolver_update_scaling_dev(self, xzs):
        self.calls.append("scaling")
        _, z, s = self._split(xzs)
        return self.cones.update_scaling(s, z, 0.0)

    def kktsolver_refactor(self):
        self.calls.append("refactor")
        return self.sys.kkt_update(self.data, self.cones)

    def _vars(self, xzs, tau, kappa):
        x, z, s = self._split(xzs)
        return ipm.Variables(x, s, z, tau, kappa)

    def _alpha(self, v, fraction):      # variables.jl:14-43
        step = self.lhs
        a_tau = -v.tau / step.tau if step.tau < 0 else ipm.FLOATMAX
        a_kap = -v.kappa / step.kappa if step.kappa < 0 else ipm.FLOATMAX
        alpha = min(a_tau, a_kap, 1.0)
        az, as_ = self.cones.step_length(step.z, step.s, v.z, v.s, alpha)
        return min(az, as_) * fraction

    def kktsolver_step_affine(self, xzs, res, tau, kappa, r_tau, const_pending):
        self.calls.append("affine")
        assert const_pending
        v, rhs, lhs = self._vars(xzs, tau, kappa), self.rhs, self.lhs
        rx, rz = self._res(res)[:2]
        rhs.x[:] = rx
        rhs.z[:] = rz
        self.cones.affine_ds(rhs.s, v.s)
        rhs.tau, rhs.kappa = r_tau, tau * kappa
        if not self.sys.kkt_solve(lhs, rhs, self.data, v, self.cones, "affine"):
            return False, 0.0, 0.0, 0.0
        return True, self._alpha(v, 1.0), lhs.tau, lhs.kappa

    def kktsolver_step_combined(self, xzs, res, tau, kappa, r_tau, dtau_aff, dkappa_aff, sigma, mu, m_corr):
        self.calls.append("combined")
        v, rhs, lhs = self._vars(xzs, tau, kappa), self.rhs, self.lhs
        assert (dtau_aff, dkappa_aff) == (lhs.tau, lhs.kappa)
        rx, rz = self._res(res)[:2]
        sm = sigma * mu
        rhs.x[:] = (1.0 - sigma) * rx
        rhs.tau = (1.0 - sigma) * r_tau
        rhs.kappa = -sm + m_corr * lhs.tau * lhs.kappa + tau * kappa
        if m_corr != 1.0:
            lhs.z *= m_corr
        self.cones.affine_ds(rhs.s, v.s)
        self.cones.combined_ds_shift(rhs.z, lhs.z, lhs.s, sm)
        rhs.s += rhs.z
        rhs.z[:] = (1.0 - sigma) * rz
        if not self.sys.kkt_solve(lhs, rhs, self.data, v, self.cones, "combined"):
            return False, 0.0, 0.0, 0.0
        return True, self._alpha(v, self.settings.max_step_fraction), lhs.tau, lhs.kappa

    def kktsolver_step_apply(self, alpha, xzs):
        self.calls.append("apply")
        x, z, s = self._split(xzs)
        x += alpha * self.lhs.x
        z += alpha * self.lhs.z
        s += alpha * self.lhs.s


class _FakeNonsymPlugin(_FakeStepPlugin):
    """_FakeStepPlugin plus what the non-symmetric loop calls: the scaling with (mu, strategy) and the barrier of the resident step"""

    def kktsolver_update_scaling_dev_ex(self, xzs, mu, strategy):
        self.calls.append("scaling_ex:" + strategy)
        _, z, s = self._split(xzs)
        return self.cones.update_scaling(s, z, mu, strategy)

    def kktsolver_step_barrier(self, xzs, alphas):
        self.calls.append("barrier")
        assert 1 <= len(alphas) <= 8
        _, z, s = self._split(xzs)
        dz, ds = self.lhs.z, self.lhs.s
        bars = [self.cones.compute_barrier(z, s, dz, ds, a) for a in alphas]
        dots = [float(np.dot(z + a * dz, s + a * ds)) for a in alphas]
        return bars, dots
