"""tests/default_start_reference.py held to the stand-in (julia_standin: CompositeCone.margins, Solver._shift_to_cone_interior) on
finite inputs, to its own 50-digit margins, and to hand-worked cases of each arm of the shift.  Needs no GPU."""
import math
import types

import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from julia_standin import ipm
from julia_standin.cones import CompositeCone
from tests import default_start_reference as dr

T = cl


def _sets():
    return {
        "soc_mix": [T.ZeroConeT(2), T.NonnegativeConeT(5), T.SecondOrderConeT(3), T.SecondOrderConeT(6)],
        "mixed": [T.NonnegativeConeT(3), T.PSDTriangleConeT(3), T.SecondOrderConeT(4), T.PSDTriangleConeT(1), T.ZeroConeT(2),
                  T.PSDTriangleConeT(8), T.PSDTriangleConeT(2)],
        "zero_only": [T.ZeroConeT(3)],
        "psd_5": [T.PSDTriangleConeT(5)],
    }


def _standin_shift(cones, v, pd):
    w = v.copy()
    ipm.Solver._shift_to_cone_interior(types.SimpleNamespace(cones=cones), w, pd)
    return w


@pytest.mark.parametrize("name", list(_sets()))
@pytest.mark.parametrize("pd", ["primal", "dual"])
def test_reference_equals_the_stand_in_on_finite_inputs(name, pd):
    cones = CompositeCone(_sets()[name])
    rng = np.random.default_rng(11)
    seen = set()
    for scale, offset in [(1.0, 0.0), (1.0, 0.4), (0.05, 0.5), (1.0, 8.0), (3.0, 60.0), (0.1, -2.0)]:
        v = scale * rng.standard_normal(cones.numel)
        dr.unit_shift(cones, v, offset, "dual")      # (moves every cone's margin by `offset`, leaves Zero rows alone)
        assert dr.margins64(cones, v) == cones.margins(v, pd)
        w, mn, pos, tg, br = dr.shift64(cones, v, pd)
        assert dr.same_bits(w, _standin_shift(cones, v, pd)), (name, pd, scale, offset)
        seen.add(br)
        # and the 50-digit margins agree with the float64 ones far below any decision of these cases
        ref = dr.margins_mp(cones, v)
        scale2 = max(1.0, float(np.max(np.abs(v)))) * cones.numel
        if name != "zero_only":
            assert abs(float(ref["alpha"]) - mn) <= 1e-12 * scale2 and abs(float(ref["beta"]) - pos) <= 1e-12 * scale2
        tgt, brm, margin = dr.decision_mp(ref)
        assert margin < 1e-6 or brm == br
    assert seen == ({2} if name == "zero_only" else {0, 1, 2}), seen


def test_hand_worked_arms():
    cones = CompositeCone([T.ZeroConeT(1), T.NonnegativeConeT(2), T.SecondOrderConeT(3), T.PSDTriangleConeT(2)])
    assert cones.degree == 2 + 1 + 2
    r2 = math.sqrt(2.0)
    # arm 0: the second-order cone binds with alpha = 1 - 5 = -4; two separate additions
    v = np.array([7.0, 2.0, 3.0, 1.0, 3.0, 4.0, 2.0, 0.0, 2.0])
    assert dr.margins64(cones, v) == (-4.0, 2.0 + 3.0 + 0.0 + 2.0 + 2.0)
    w, mn, pos, tg, br = dr.shift64(cones, v, "primal")
    assert (mn, pos, tg, br) == (-4.0, 9.0, 1.0, 0)
    assert np.array_equal(w, [0.0, 7.0, 8.0, 6.0, 3.0, 4.0, 7.0, 0.0, 7.0])
    assert np.array_equal(dr.shift64(cones, v, "dual")[0], [7.0, 7.0, 8.0, 6.0, 3.0, 4.0, 7.0, 0.0, 7.0])
    # ... and they are two roundings: 1e-17 + 1e30 - ... would vanish in one
    big = np.array([0.0, -1e30, 1.0, 5.0, 0.0, 0.0, 1.0, 0.0, 1.0])
    w = dr.shift64(cones, big, "dual")[0]
    assert w[1] == (-1e30 + 1e30) + 1.0 == 1.0 and w[2] == (1.0 + 1e30) + 1.0
    # arm 1: min_margin 0.25 (PSD eigenvalue), target 1: everything moves by 0.75
    v = np.array([1.0, 2.0, 3.0, 5.0, 3.0, 0.0, 1.25, r2 * 0.5, 0.75 + 0.5])       # eigenvalues of [[1.25, .5], [.5, 1.25]]: 0.75, 1.75
    v[6:] = [0.75, r2 * 0.5, 0.75]                                                 # [[.75, .5], [.5, .75]]: 0.25, 1.25
    mn, pos = dr.margins64(cones, v)
    assert abs(mn - 0.25) < 1e-15 and abs(pos - (5.0 + 2.0 + 1.5)) < 1e-14
    w, mn, pos, tg, br = dr.shift64(cones, v, "dual")
    assert (tg, br) == (1.0, 1)
    d = 1.0 - mn
    assert np.array_equal(w, [1.0, 2.0 + d, 3.0 + d, 5.0 + d, 3.0, 0.0, 0.75 + d, r2 * 0.5, 0.75 + d])
    # arm 1 with target = 0.1 beta / degree > 1
    v = np.array([0.0, 100.0, 200.0, 50.0, 0.0, 0.0, 2.0, 0.0, 2.0])
    w, mn, pos, tg, br = dr.shift64(cones, v, "dual")
    assert (mn, pos, br) == (2.0, 354.0, 1) and tg == 0.1 * 354.0 / 5 and tg > 1.0
    assert w[6] == 2.0 + (tg - 2.0) and w[7] == 0.0 and w[3] == 50.0 + (tg - 2.0)
    # arm 2: a good margin still zeroes the Zero rows of a primal vector and really adds 0.0
    v = np.array([-3.0, 4.0, 5.0, 9.0, 0.0, -0.0, 6.0, -0.0, 7.0])
    w, mn, pos, tg, br = dr.shift64(cones, v, "primal")
    assert (mn, br) == (4.0, 2) and tg == max(1.0, 0.1 * (9.0 + 9.0 + 13.0) / 5)
    assert dr.same_bits(w, [0.0, 4.0, 5.0, 9.0, 0.0, -0.0, 6.0, -0.0, 7.0])           # unshifted rows keep their -0.0
    assert dr.same_bits(dr.shift64(cones, v, "dual")[0], [-3.0, 4.0, 5.0, 9.0, 0.0, -0.0, 6.0, -0.0, 7.0])
    # -0.0 on a shifted row under the zero shift becomes +0.0 (reachable with a NaN margin: both comparisons fail)
    v = np.array([1.0, -0.0, 5.0, float("nan"), 0.0, 0.0, 6.0, 0.0, 7.0])
    w, mn, pos, tg, br = dr.shift64(cones, v, "dual")
    assert math.isnan(mn) and math.isnan(pos) and math.isnan(tg) and br == 2
    assert dr.same_bits(w[:3], [1.0, 0.0, 5.0]) and not np.signbit(w[1]) and math.isnan(w[3])
    # a NaN in a Nonnegative row: NaN min_margin, but `z > 0 ? z : 0` drops it from pos_margin
    v = np.array([1.0, float("nan"), 5.0, 9.0, 0.0, 0.0, 6.0, 0.0, 7.0])
    w, mn, pos, tg, br = dr.shift64(cones, v, "dual")
    assert math.isnan(mn) and pos == 5.0 + 9.0 + 13.0 and br == 2
    # Python's min / max would have hidden both
    assert min(1.0, float("nan")) == 1.0 and math.isnan(dr.jl_min(1.0, float("nan"))) and math.isnan(dr.jl_max(1.0, float("nan")))
    # degree 0: target 1
    zc = CompositeCone([T.ZeroConeT(2)])
    w, mn, pos, tg, br = dr.shift64(zc, np.array([3.0, -4.0]), "primal")
    assert (mn, pos, tg, br) == (dr.FLOATMAX, 0.0, 1.0, 2) and np.array_equal(w, [0.0, 0.0])


def test_apply_shift_takes_the_arm_of_the_given_margins():
    cones = CompositeCone([T.NonnegativeConeT(2)])
    v = np.array([1.0, 2.0])
    assert dr.apply_shift(cones, v, "dual", -0.5, 3.0)[1] == 0 and np.array_equal(dr.apply_shift(cones, v, "dual", -0.5, 3.0)[0], [4.5, 5.5])
    assert dr.apply_shift(cones, v, "dual", 0.0, 1.0)[1] == 0
    assert dr.apply_shift(cones, v, "dual", 1.0, 3.0)[1] == 1 and np.array_equal(dr.apply_shift(cones, v, "dual", 1.0, 3.0)[0], [3.0, 4.0])
    assert dr.apply_shift(cones, v, "dual", 3.0, 3.0)[1] == 2
    assert dr.apply_shift(cones, v, "dual", float("nan"), 3.0)[1] == 2
