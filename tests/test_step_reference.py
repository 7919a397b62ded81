"""The float64 stand-in's second-order-cone step algebra (julia_standin/cones.py) against tests/step_reference.py, without a GPU: the
stand-in is what tests/test_gpu_device_step.py and tests/test_gpu_step_edges.py hold the device against, so it is held here against
something of higher precision.  No code of the HIP library runs.

Cone set: Zero(1), Nonnegative(1), SOC(d) for d in 2, 255, 256, 257, 258, 511, 512, 513, 1025; points: fixtures.scale_cones and
scale_cones_late, two seeds each (step_reference.scaled_point).

1. Stand-in against its own expressions at 50 digits.  MEASURED: the largest |stand-in - 50 digits| / max |50 digits| over the cones
   and seeds, per operation and fixture (printed by the test; gate = 10 x the recorded value):

       operation            scale_cones   scale_cones_late
       affine_ds            5.55e-16      3.03e-16
       combined_ds_shift    1.20e-15      4.53e-11
       ds_from_dz_offset    5.81e-15      1.88e-10
       mul_Hs               7.22e-16      8.32e-15
       step_length          6.10e-15      1.88e-10

   (step_length: _step_length_soc_component on the "hits the boundary" direction of step_reference.isolated_directions, relative to
   the 50-digit value.)  The late figures are the conditioning of those points (a margin of 1e-6 |z1| turns one rounding of |z1| into
   1e-10 of the residual), not a defect of the expressions.

2. Stand-in against the definitions (dense W, W^-1 as a solve, Arw(lambda) as a solve, smallest positive root), scale_cones points
   only, 1e-9 of max |result| per cone; the step lengths of every isolated direction of test_gpu_step_edges.py on those points at
   1e-10 relative (PARITY), which is what lets that test compare the device with the 50-digit root at PARITY.

3. The constructed step-length inputs of step_reference.soc_exit_cases take the exit they are named for, and every exit of
   _step_length_soc_component is reached except `c == 0`: that one needs a resident s or z exactly on the cone's boundary, which
   update_scaling rejects (a zero residual fails the scaling), so no handle can hold such a point.  It is left untested."""
import numpy as np
import pytest

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from julia_standin.cones import SecondOrderCone, _step_length_soc_component
from tests import step_reference as sr
from tests.step_support import _mixed_problem

FIXTURES = [(False, "scale_cones"), (True, "scale_cones_late")]

# the measured values of item 1 (see the docstring): RECORDED[operation][late]
RECORDED = {
    "affine_ds": {False: 5.55e-16, True: 3.03e-16},
    "combined_ds_shift": {False: 1.20e-15, True: 4.53e-11},
    "ds_from_dz_offset": {False: 5.81e-15, True: 1.88e-10},
    "mul_Hs": {False: 7.22e-16, True: 8.32e-15},
    "step_length": {False: 6.10e-15, True: 1.88e-10},
}
DEFINITION_TOL = 1e-9
PARITY = 1e-10


def _points(late):
    for seed in sr.POINT_SEEDS:
        cones = cl.CompositeCone(cl.cones_new_collapsed(sr.long_cone_specs()))
        s, z, rng = sr.scaled_point(cones, seed, late)
        m = cones.numel
        dz, ds, v = rng.standard_normal(m), rng.standard_normal(m), rng.standard_normal(m)
        yield seed, cones, s, z, dz, ds, v, 0.37 * (1e-9 if late else 1.0), rng


def _standin_ops(K, r, s, z, dz, ds, v, sm):
    """the four vector operations of one cone by the stand-in -> name -> float64 result"""
    out = {}
    o = np.zeros(K.dim)
    K.affine_ds(o, s[r])
    out["affine_ds"] = o
    o = np.zeros(K.dim)
    K.combined_ds_shift(o, dz[r].copy(), ds[r].copy(), sm)
    out["combined_ds_shift"] = o
    o = np.zeros(K.dim)
    K.ds_from_dz_offset(o, v[r], np.zeros(K.dim), z[r])
    out["ds_from_dz_offset"] = o
    o = np.zeros(K.dim)
    K.mul_Hs(o, v[r], np.zeros(K.dim))
    out["mul_Hs"] = o
    return out


@pytest.mark.parametrize("late,fixture", FIXTURES)
def test_stand_in_matches_its_own_expressions_at_50_digits(late, fixture):
    worst = {k: 0.0 for k in RECORDED}
    for seed, cones, s, z, dz, ds, v, sm, rng in _points(late):
        for K, r in sr.soc_cones(cones):
            got = _standin_ops(K, r, s, z, dz, ds, v, sm)
            ref = {"affine_ds": sr.ref_affine_ds(K.lam),
                   "combined_ds_shift": sr.ref_combined_ds_shift(K.w, K.eta, dz[r], ds[r], sm),
                   "ds_from_dz_offset": sr.ref_ds_from_dz_offset(K.w, K.lam, K.eta, z[r], v[r]),
                   "mul_Hs": sr.ref_mul_Hs(K.w, K.eta, v[r])}
            for name in ref:
                worst[name] = max(worst[name], sr.max_err(got[name], ref[name]) / sr.max_abs(ref[name]))
            for x in (z[r], s[r]):
                y, amax = sr.isolated_directions(x, rng)["hits the boundary"]
                t = sr.ref_step_length_soc_component(x, y, amax)
                worst["step_length"] = max(worst["step_length"], float(abs(sr.mpf(_step_length_soc_component(x, y, amax)) - t) / t))
    for name, w in worst.items():
        print(f"[step reference, {fixture}] {name}: max |stand-in - 50 digits| / max |50 digits| = {w:.2e} (recorded {RECORDED[name][late]:.2e})")
    for name, w in worst.items():
        assert w <= 10.0 * RECORDED[name][late], (name, fixture, w)


def test_block_form_of_W_is_the_dense_matrix():
    """soc_W_apply without the materialised rows (used above DENSE_MAX) against the dense W at every dimension up to DENSE_MAX"""
    cones = cl.CompositeCone(cl.cones_new_collapsed(sr.long_cone_specs()))
    s, z, rng = sr.scaled_point(cones, sr.POINT_SEEDS[0], False)
    seen = []
    for K, r in sr.soc_cones(cones):
        if K.dim > sr.DENSE_MAX:
            continue
        x = sr.V(rng.standard_normal(K.dim))
        dense = sr.soc_W_apply(K.w, K.eta, x, sr.soc_W_dense(K.w, K.eta))
        block = sr.soc_W_apply(K.w, K.eta, x)
        assert max(abs(p - q) for p, q in zip(dense, block)) <= sr.mpf(10) ** -45 * max(abs(p) for p in dense), K.dim
        seen.append(K.dim)
    assert seen == [d for d in sr.LONG_DIMS if d <= sr.DENSE_MAX]


def test_stand_in_matches_the_definitions():
    for seed, cones, s, z, dz, ds, v, sm, rng in _points(False):
        for K, r in sr.soc_cones(cones):
            # lambda = W z = W^-1 s is what makes the definitions and the reference's expressions the same thing
            dense = sr.soc_W_dense(K.w, K.eta) if K.dim <= sr.DENSE_MAX else None
            got = _standin_ops(K, r, s, z, dz, ds, v, sm)
            ref = {"combined_ds_shift": sr.def_combined_ds_shift(K.w, K.eta, dz[r], ds[r], sm, dense),
                   "ds_from_dz_offset": sr.def_ds_from_dz_offset(K.w, K.lam, K.eta, v[r], dense),
                   "mul_Hs": sr.def_mul_Hs(K.w, K.eta, v[r], dense)}
            for name in ref:
                e = sr.max_err(got[name], ref[name]) / sr.max_abs(ref[name])
                print(f"[step definitions, seed {seed}] SOC({K.dim}) {name}: max |stand-in - definition| / max |definition| = {e:.2e}")
                assert e <= DEFINITION_TOL, (name, K.dim, seed, e)


def test_stand_in_step_lengths_match_the_smallest_positive_root():
    """every isolated direction that test_gpu_step_edges.py uses on scale_cones points (the long cones, the mixed cone set and the exit cases)"""
    worst = 0.0
    for seed in sr.POINT_SEEDS:
        for specs in (sr.long_cone_specs(), sr.exit_cone_specs(), _mixed_problem(3)[4]):
            cones = cl.CompositeCone(cl.cones_new_collapsed(specs))
            s, z, rng = sr.scaled_point(cones, seed, False)
            for K, r, dirs in sr.per_cone_directions(cones, s, z, rng):
                if not isinstance(K, SecondOrderCone):
                    continue
                todo = [(n, x, y, amax) for n, (yz, ys, amax) in dirs.items() for x, y in ((z[r], yz), (s[r], ys))]
                if len(specs) == len(sr.exit_cone_specs()):
                    todo += [(n, x, y, amax) for x in (z[r], s[r]) for n, (y, amax, _) in sr.soc_exit_cases(x).items()]
                for name, x, y, amax in todo:
                    got, ref = _step_length_soc_component(x, y, amax), sr.def_step_length(x, y, amax)
                    e = float(abs(sr.mpf(got) - ref) / ref)
                    worst = max(worst, e)
                    assert e <= PARITY, (name, K.dim, seed, got, float(ref))
    print(f"[step definitions] step length: max |stand-in - smallest positive root| / root = {worst:.2e}")


def test_constructed_inputs_take_the_exit_they_are_named_for():
    reached = set()
    for seed in sr.POINT_SEEDS:
        cones = cl.CompositeCone(cl.cones_new_collapsed(sr.exit_cone_specs()))
        s, z, _ = sr.scaled_point(cones, seed, False)
        for K, r in sr.soc_cones(cones):
            for x in (z[r], s[r]):
                cases = sr.soc_exit_cases(x)
                assert tuple(cases) == sr.EXIT_CASE_NAMES, (K.dim, tuple(cases))
                for name, (y, amax, expected) in cases.items():
                    info = sr.soc_step_exit(x, y, amax)
                    assert info["value"] == _step_length_soc_component(x, y, amax), (name, K.dim)      # the same float64 operations
                    for key, want in expected.items():
                        assert info[key] == want, (name, K.dim, key, info)
                    if info["returned"] == "cap" and not info["linear_bound"]:
                        assert info["value"] == amax
                    if info["returned"] == "root":
                        assert 0.0 < info["value"] < amax
                    reached.add(info["exit"])
    assert reached == sr.REACHABLE_EXITS, reached
    # c == 0 is not reachable from a point that update_scaling accepts (see the module docstring); soc_step_exit still names it
    x = np.array([5.0, 3.0, 4.0])
    assert sr.soc_step_exit(x, np.array([-1.0, 0.0, 0.0]), 1.0)["exit"] == "c_zero"
    assert not cl.CompositeCone([cl.SecondOrderConeT(3)]).update_scaling(x, np.array([2.0, 0.0, 1.0]), 1.0)
