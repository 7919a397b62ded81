"""The barrier of a PSD triangle cone against 50 digits, without a GPU: the stand-in's PSDTriangleCone.compute_barrier (numpy / LAPACK)
and the float64 emulation of barrier_psd.hip's arithmetic (tests/psd_barrier_reference.py emulate_kernel) are held to the reference at
the cases the GPU file uses, and the host's error per case is what that file's gate is built from.

Gates, in units of eps x scale (scale = sum(|Q^-1| o |L| |L'|) + sum |log l_jj^2| per logdet, see the reference module):
  the stand-in   at most 2 n + 4: the componentwise backward error of an n x n Cholesky is below (n + 1) eps |L| |L'| (Higham, Theorem
                 10.3), which the first part of the scale turns into (n + 1) units per logdet at most, hence for both together; the
                 n logarithms, their sum and the doubling add at most (n + 2) eps sum |log l_jj| <= (n + 2) / 2 units of the second part;
                 the rounding of q_k / sqrt 2 one more unit.  LAPACK's blocked order changes constants, not the bound.
  the emulation  max(8 x the stand-in's error in the same case, 2 n): the rule the device is held to.
Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest

from tests import psd_barrier_reference as br


@pytest.mark.parametrize("late", [False, True], ids=["early", "late"])
@pytest.mark.parametrize("n", br.SIDES)
def test_stand_in_and_kernel_emulation_against_50_digits(n, late):
    cs = br.case(n, late)
    worst_h = worst_e = 0.0
    for j, a in enumerate(cs["alphas"]):
        assert cs["scale"][j] > 0 and math.isfinite(float(cs["ref"][j]))
        rh = cs["host_ratio"][j]
        re = br.ratio(br.emulate_kernel(n, cs["z"], cs["s"], cs["dz"], cs["ds"], a), cs["ref"][j], cs["scale"][j])
        print(f"[psd barrier] n={n} late={late} alpha={a:.4f}: barrier {float(cs['ref'][j]):.6e}, scale {cs['scale'][j]:.3e}, "
              f"stand-in {rh:.3f}, emulation {re:.3f}, allowed {br.allowed(rh, n):.1f} (eps x scale)")
        assert rh <= 2 * n + 4, (n, late, a, rh)
        assert re <= br.allowed(rh, n), (n, late, a, re, rh)
        worst_h, worst_e = max(worst_h, rh), max(worst_e, re)
    print(f"[psd barrier] n={n} late={late}: worst stand-in {worst_h:.3f}, worst emulation {worst_e:.3f}")


def test_the_cases_carry_as_many_candidates_as_one_launch_serves():
    assert br.NALPHA == 8 and len(br.candidates()) == br.NALPHA and len(br.case(1, False)["alphas"]) == br.NALPHA
    from clarabel_jl_amd import hipkkt
    assert "hipkkt_step_enable_mixed" in hipkkt.SYMBOLS      # the entry point whose barrier calls launch the kernel


def test_the_late_cases_are_late_and_every_candidate_is_interior():
    for n in (3, 17):
        cs = br.case(n, True)
        K = cs["K"]
        ev = np.linalg.eigvalsh(K.svec_to_mat(cs["s"]))
        assert ev.min() > 0 and ev.max() / ev.min() > 1e7
        for a in cs["alphas"]:
            for x, dx in ((cs["z"], cs["dz"]), (cs["s"], cs["ds"])):
                assert np.linalg.eigvalsh(K.svec_to_mat(br.shifted(x, dx, a))).min() > 0


def test_a_point_outside_the_cone_gives_minus_infinity_as_the_reference_does():
    """`barrier -= typemax(T)`: +Inf from _logdet_barrier, so -Inf for the cone, whichever side leaves it"""
    cs = br.case(3, False)
    K, z, s = cs["K"], cs["z"], cs["s"]
    out = K.mat_to_svec(-2.0 * K.svec_to_mat(z))       # Z + 1 (-2 Z) = -Z
    out_s = K.mat_to_svec(-2.0 * K.svec_to_mat(s))
    zero = np.zeros_like(z)
    for dz, ds in ((out, zero), (zero, out_s), (out, out_s)):
        assert br.ref_barrier(3, z, s, dz, ds, 1.0)[0] == -math.inf
        assert K.compute_barrier(z, s, dz, ds, 1.0) == -math.inf
        assert br.emulate_kernel(3, z, s, dz, ds, 1.0) == -math.inf
        # the same direction at a step that stays inside is finite everywhere
        assert math.isfinite(K.compute_barrier(z, s, dz, ds, 0.25)) and math.isfinite(br.emulate_kernel(3, z, s, dz, ds, 0.25))
    nan = zero.copy()
    nan[1] = math.nan
    assert br.ref_barrier(3, z, s, nan, zero, 0.5)[0] == -math.inf      # a NaN reaches a pivot: the failure arm
    assert br.emulate_kernel(3, z, s, nan, zero, 0.5) == -math.inf


def test_zero_direction_and_zero_step_give_the_barrier_of_the_point():
    cs = br.case(17, False)
    K, z, s, dz, ds = cs["K"], cs["z"], cs["s"], cs["dz"], cs["ds"]
    at_point = br.emulate_kernel(17, z, s, np.zeros_like(z), np.zeros_like(s), 0.7)
    assert at_point == br.emulate_kernel(17, z, s, dz, ds, 0.0)
    ref, scale = br.ref_barrier(17, z, s, dz, ds, 0.0)
    assert br.ratio(at_point, ref, scale) <= 2 * 17
