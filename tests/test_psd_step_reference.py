"""tests/psd_step_reference.py (the 50-digit reference of the PSD triangle cone's step algebra) against the stand-in's
PSDTriangleCone and against hand-checked cases.  No GPU.

Gate of the comparison with the stand-in (numpy / LAPACK in float64): per family the first-order bound of its dot products in the
reference's own scale -- 2 n eps |A|' |X| |A| per triple product (an n-term dot product applied twice; twice that for mul_Hs and the
shift, which chain two), 8 n eps |M|_2 for gamma (eigvalsh's own error of a few eps |M|_2 plus the products that form M).  The measured
ratios are printed: tests/test_gpu_psd_step.py holds the device to 8 x the host's ratio."""
import numpy as np
import pytest

from julia_standin.cones import PSDTriangleCone
from tests import psd_step_reference as pr

SIDES = (1, 2, 3, 5, 8, 17, 32)
CASES = [(n, late) for n in SIDES for late in (False, True)]


@pytest.mark.parametrize("n,late", CASES)
def test_reference_agrees_with_the_stand_in(n, late):
    rng = np.random.default_rng(100 * n + late)
    K, s, z = pr.scaled_point(n, rng, late)
    dz, ds, x = pr.direction(K, rng, z), pr.direction(K, rng, s), pr.direction(K, rng, z)
    eps, w = pr.EPS, np.zeros(K.numel)
    # mul_W / mul_Winv, both transposes
    for name, F, fn in (("mul_W", K.R, K.mul_W), ("mul_Winv", K.Rinv, K.mul_Winv)):
        for tr in (False, True):
            got = np.zeros(K.numel)
            fn(got, x, transpose=tr)
            ref, scale = pr.ref_mul_W(F, x, tr)
            ratio = np.max(pr.err(got, ref) / scale) / eps
            print(f"[psd reference] n={n} late={late} {name} transpose={tr}: host error {ratio:.3f} eps scale")
            assert ratio <= 2 * n
    got = np.zeros(K.numel)
    K.mul_Hs(got, x, w)
    ref, scale = pr.ref_mul_hs(K.R, x)
    assert np.max(pr.err(got, ref) / scale) / eps <= 4 * n
    sm = 0.3 * float(np.mean(K.lam) ** 2)
    got = np.zeros(K.numel)
    K.combined_ds_shift(got, dz.copy(), ds.copy(), sm)
    ref, scale = pr.ref_shift(K.R, K.Rinv, dz, ds, sm)
    assert np.max(pr.err(got, ref) / scale) / eps <= 4 * n + 2
    got = np.zeros(K.numel)
    K.ds_from_dz_offset(got, ds, w, z)
    ref, scale = pr.ref_offset(K.R, K.lam, ds)
    assert np.max(pr.err(got, ref) / scale) / eps <= 2 * n + 2
    got = np.zeros(K.numel)
    K.affine_ds(got, s)
    assert np.max(pr.err(got, pr.ref_affine_ds(K.lam)) / np.maximum(np.abs(got), 1e-300)) <= eps
    # step length: alpha_max far away, so that alpha = 1 / -gamma shows gamma
    big = 1e300
    (az, as_), gam, norms = pr.ref_step_length(K.R, K.Rinv, K.lam, dz, ds, big)
    haz, has = K.step_length(dz, ds, z, s, big)
    for h, a, g, nm, what in ((haz, az, gam[0], norms[0], "z"), (has, as_, gam[1], norms[1], "s")):
        tol = pr.alpha_allowance(g, nm, 8 * n)
        print(f"[psd reference] n={n} late={late} step length {what}: host {h!r}, reference {float(a)!r}, allowance {tol:.3e}")
        assert abs(pr.mpf(h) - a) <= tol


@pytest.mark.parametrize("n,late", CASES)
def test_the_factors_scale_both_points_to_lambda(n, late):
    """R' Z R = Lambda = Rinv S Rinv' at 50 digits, to the accuracy a float64 Cholesky / SVD of matrices with the generator's condition
    number can give: 8 n eps cond"""
    rng = np.random.default_rng(200 * n + late)
    K, s, z = pr.scaled_point(n, rng, late)
    cond = 1e8 if late else 1e3
    R, Rinv = pr.M(K.R), pr.M(K.Rinv)
    for what, Y in (("R' Z R", pr.mm(pr.mm(R.T, pr.svec_to_mat(z, n)), R)), ("Rinv S Rinv'", pr.mm(pr.mm(Rinv, pr.svec_to_mat(s, n)), Rinv.T))):
        off = max(abs(float(Y[i, j] - (K.lam[i] if i == j else 0.0))) for i in range(n) for j in range(n)) / float(K.lam.max())
        print(f"[psd reference] n={n} late={late} {what} - Lambda: {off:.2e} of lambda_max")
        assert off <= 8 * n * pr.EPS * cond


def test_side_one_is_the_scalar_formulas():
    K = PSDTriangleCone(1)
    s, z = np.array([3.0]), np.array([0.75])
    assert K.update_scaling(s, z, 1.0)
    r, ri, lam = pr.mpf(float(K.R[0, 0])), pr.mpf(float(K.Rinv[0, 0])), pr.mpf(float(K.lam[0]))
    x, dz, ds = np.array([-1.25]), np.array([-2.0]), np.array([0.5])
    assert pr.ref_mul_W(K.R, x, False)[0][0] == r * pr.mpf(-1.25) * r
    assert pr.ref_mul_hs(K.R, x)[0][0] == r * (r * pr.mpf(-1.25) * r) * r
    assert pr.ref_affine_ds(K.lam)[0] == lam * lam
    a, b = r * pr.mpf(-2.0) * r, ri * pr.mpf(0.5) * ri
    assert abs(pr.ref_shift(K.R, K.Rinv, dz, ds, 0.125)[0][0] - (a * b - pr.mpf(0.125))) <= pr.mpf(10) ** -45
    assert abs(pr.ref_offset(K.R, K.lam, ds)[0][0] - r * (pr.mpf(0.5) / lam) * r) <= pr.mpf(10) ** -45
    (az, as_), (gz, gs), _ = pr.ref_step_length(K.R, K.Rinv, K.lam, dz, ds, 10.0)
    assert abs(gz - a / lam) <= pr.mpf(10) ** -45 and gz < 0 and abs(az - 1 / (-gz)) <= pr.mpf(10) ** -45
    assert gs > 0 and as_ == 10
    # alpha_z is where z + alpha dz leaves the cone: z / -dz, up to the float64 rounding of the factors
    assert abs(float(az) - 0.75 / 2.0) <= 8 * pr.EPS


def test_side_two_with_dz_equal_to_minus_z_gives_one():
    """dZ = -Z: M = -Lambda^-1/2 (R' Z R) Lambda^-1/2 = -I when R' Z R = Lambda holds exactly, so gamma = -1 and alpha_z = 1 at the
    reference's full precision.  Z = diag(4, 16), S = diag(4, 1) have the scaling lambda = (4, 4), R = diag(1, 1/2), Rinv = diag(1, 2):
    every factor is a binary fraction, so the identity is exact.  dS = -S / 2 gives alpha_s = 2 the same way."""
    n = 2
    K = PSDTriangleCone(n)
    z, s = K.mat_to_svec(np.diag([4.0, 16.0])), K.mat_to_svec(np.diag([4.0, 1.0]))
    R, Rinv, lam = np.diag([1.0, 0.5]), np.diag([1.0, 2.0]), np.array([4.0, 4.0])
    Y = pr.mm(pr.mm(pr.M(R).T, pr.svec_to_mat(z, n)), pr.M(R))
    assert all(Y[i, j] == (4 if i == j else 0) for i in range(n) for j in range(n))
    (az, as_), (gz, gs), (nz, _) = pr.ref_step_length(R, Rinv, lam, -z, -0.5 * s, 7.0)
    assert abs(gz + 1) <= pr.mpf(10) ** -45 and abs(az - 1) <= pr.mpf(10) ** -45 and abs(nz - 1.0) <= 1e-15
    assert abs(gs + pr.mpf(0.5)) <= pr.mpf(10) ** -45 and abs(as_ - 2) <= pr.mpf(10) ** -45
    # and the stand-in on its own factors of the same point
    assert K.update_scaling(s, z, 1.0)
    haz, has = K.step_length(-z, -0.5 * s, z, s, 7.0)
    assert abs(haz - 1.0) <= 16 * pr.EPS and abs(has - 2.0) <= 32 * pr.EPS
