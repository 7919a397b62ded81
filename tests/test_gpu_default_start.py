"""The default start of a symmetric cone set on the device (include/hipkkt.h hipkkt_cone_set_identity_scaling / hipkkt_cone_margins /
hipkkt_cone_shift_to_interior / hipkkt_step_default_start_dev; csrc/start.hip), stage by stage against the host path on a twin handle
of the same problem and against tests/default_start_reference.py:
  identity scaling   the resident K bit for bit what HipKKTSolver.kktsolver_update leaves after the host cones' set_identity_scaling
  margins            against 50 digits: a Nonnegative alpha `==`; sums within SUM_TOL x sum |terms|; a PSD cone's alpha / beta within
                     max(8 x the host's error in the same case, 2 n) eps |Z|_2 (the rule of tests/test_gpu_psd_step.py)
  shift              the reference's arm (decision margin >= 1e-6 at 50 digits, asserted), every row `==` the reference shift applied
                     with the DEVICE's (min_margin, target)
  NaN                the reference's rules, not Python's min
  fused call         eps, regularised pivots, refinement steps equal and [x | z | s] bit for bit the host _default_start's with the
                     device's margins
  end to end         Settings(device_default_start=True) against the same settings without it
Each cone set runs with P != 0 and with structural P = 0 (both branches of kkt_solve_initial_point!).  The 50-digit references are
computed once per cone set and shared.  One mp.eigsy of a 64 x 64 matrix at 50 digits takes about two seconds, so the large PSD sides
get fewer vectors in the margins and shift tests: sides >= 32 three of the six constructed arm / target cases (one per arm, both
targets among them), the two-fold smallest eigenvalue only up to side 33, and side 64 no random vector there -- its random data are the
solved (s, z) of the fused test, which are held to 50 digits too.  The diagonal matrix and Z = -2 I run at every side: their
eigenvalues are their entries and need no eigsy.  The margins tests print the worst device / host error per PSD side at their end."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

import clarabel_jl_amd  # noqa: F401
import julia_standin as cl
from clarabel_jl_amd import hipkkt
from clarabel_jl_amd.kktsolver import HipKKTSolver
from julia_standin.cones import NonnegativeCone, PSDTriangleCone, SecondOrderCone, ZeroCone
from tests import default_start_reference as dr
from tests import fixtures as fx
from tests.step_support import STEP_FLAGS, SUM_TOL, _problem, _Timeout
from tests.test_gpu_device_step import END_TO_END as SYM_END_TO_END
from tests.test_gpu_psd_step import END_TO_END as PSD_END_TO_END
from tests.test_gpu_psd_step import _mixed_specs, _point

pytestmark = pytest.mark.gpu

T = cl
SIDES = (1, 2, 3, 8, 17, 32, 33, 64)
SETS = {
    "soc_mix": lambda: [T.ZeroConeT(2), T.NonnegativeConeT(5), T.SecondOrderConeT(3), T.SecondOrderConeT(6)],
    "mixed": _mixed_specs,
    "nn_700": lambda: [T.NonnegativeConeT(700)],
    "soc_300": lambda: [T.SecondOrderConeT(300)],
    "twenty_of_5": lambda: [T.PSDTriangleConeT(5)] * 20,
}
SETS.update({f"side_{n}": (lambda n=n: [T.PSDTriangleConeT(n)]) for n in SIDES})
PSD_FLAGS = dict(device_step=True, device_step_psd=True, device_scaling_psd=True, **STEP_FLAGS)
SYM_FLAGS = dict(device_step=True, **STEP_FLAGS)
BOTH_P = pytest.mark.parametrize("pzero", [False, True], ids=["P", "P0"])
ALL_SETS = pytest.mark.parametrize("name", list(SETS))


def _has_psd(specs):
    return any(isinstance(s, T.PSDTriangleConeT) for s in specs)


def _handle(name, pzero, seed=3, flags=None):
    """(plugin, cones, problem) for the cone set as given: NOT collapsed, so that a PSD cone of side 1 stays one"""
    specs = SETS[name]()
    P, q, A, b, specs = _problem(specs, seed)
    if pzero:
        P = sp.csc_matrix(P.shape)
    cones = cl.CompositeCone(specs)
    Pt = sp.triu(sp.csc_matrix(P), format="csc")
    Pt.sort_indices()
    A = sp.csc_matrix(A)
    A.sort_indices()
    m, n = A.shape
    if flags is None:
        flags = PSD_FLAGS if _has_psd(specs) else SYM_FLAGS
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings(**flags))
    return hk, cones, (Pt, q, A, b)


# ---- constructed vectors: one per arm and target, every cone kind of the set binding alone in turn --------------------------------------

def _base(cones, rng):
    """per cone a vector whose margin lies in about [-1, 0] and whose spread is about 2, so that a cone's unit shift places its margin"""
    v = np.empty(cones.numel)
    for c, r in zip(cones.cones, cones.rng_cones):
        if isinstance(c, ZeroCone):
            v[r] = rng.standard_normal(c.numel)
        elif isinstance(c, NonnegativeCone):
            v[r] = rng.uniform(0.0, 2.0, c.numel)
        elif isinstance(c, SecondOrderCone):
            t = rng.standard_normal(c.numel - 1)
            v[r] = np.concatenate([[rng.uniform(0.0, 1.0)], t / np.linalg.norm(t)])
        else:
            A = rng.standard_normal((c.n, c.n))
            v[r] = c.mat_to_svec((A + A.T) / (2.0 * math.sqrt(2.0 * c.n) + 1.0))
    return v


def _shift_cone(c, r, v, a):
    if isinstance(c, NonnegativeCone):
        v[r] += a
    elif isinstance(c, SecondOrderCone):
        v[r.start] += a
    elif isinstance(c, PSDTriangleCone):
        v[r.start + c._diagidx] += a


def _placed(cones, rng, binder, d, gap):
    """the binder's margin at about d, every other cone's at about d + gap and more"""
    v = _base(cones, rng)
    for k, (c, r) in enumerate(zip(cones.cones, cones.rng_cones)):
        if isinstance(c, ZeroCone):
            continue
        want = d if k == binder else d + gap + 0.25 * (1 + k % 3)
        _shift_cone(c, r, v, want - dr.cone_margins64(c, v[r])[0])
    return v


# (margin of the binder, distance of the others, intended arm): both targets (1 and 0.1 beta / degree > 1) where the set allows them
CASES = [(-0.7, 1.0, 0), (-0.7, 60.0, 0), (0.4, 1.0, 1), (0.4, 60.0, 1), (3.0, 1.0, 2), (30.0, 1.0, 2)]
CASES_LARGE = [(-0.7, 1.0, 0), (0.4, 1.0, 1), (30.0, 1.0, 2)]      # PSD sides >= 32: the 50-digit eigenvalues take seconds each


@functools.lru_cache(maxsize=None)
def _vectors(name):
    """[(label, vector, 50-digit reference, intended arm or None)]: the constructed vectors, random ones, and for a single PSD cone a
    two-fold smallest eigenvalue, a diagonal matrix and Z = -2 I"""
    cones = cl.CompositeCone(SETS[name]())
    rng = np.random.default_rng(sum(map(ord, name)))
    large = any(isinstance(c, PSDTriangleCone) and c.n >= 32 for c in cones.cones)
    out = []
    first = {}
    for k, c in enumerate(cones.cones):
        if not isinstance(c, ZeroCone):
            first.setdefault(type(c), k)
    for kind, binder in first.items():
        for d, gap, arm in (CASES_LARGE if large else CASES):
            out.append((f"{kind.__name__} binds d={d} gap={gap}", _placed(cones, rng, binder, d, gap), arm))
    res = []
    for label, v, arm in out:
        res.append((label, v, dr.margins_mp(cones, v), arm))

    def drawn(label, draw):
        """a random vector whose decision margin at 50 digits is at least 1e-6: drawn again otherwise (bounded), never skipped"""
        for _ in range(8):
            v = draw()
            ref = dr.margins_mp(cones, v)
            if dr.decision_mp(ref)[2] >= 1e-6:
                res.append((label, v, ref, None))
                return
        raise AssertionError(f"{name} {label}: eight draws in a row within 1e-6 of a threshold")

    if not any(isinstance(c, PSDTriangleCone) and c.n >= 64 for c in cones.cones):      # (side 64: see the module's docstring)
        drawn("random", lambda: rng.standard_normal(cones.numel))
    if not large:
        drawn("random x 100", lambda: 100.0 * rng.standard_normal(cones.numel))
    if len(cones.cones) == 1 and isinstance(cones.cones[0], PSDTriangleCone):
        c = cones.cones[0]
        n = c.n
        if 2 <= n <= 33:
            Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
            lam = np.concatenate([[-1.5, -1.5], rng.uniform(0.5, 3.0, n - 2)])
            Z = (Q * lam) @ Q.T
            v = c.mat_to_svec(0.5 * (Z + Z.T))
            res.append(("two-fold smallest eigenvalue", v, dr.margins_mp(cones, v), None))
        drawn("diagonal", lambda: c.mat_to_svec(np.diag(rng.standard_normal(n))))
        v = c.mat_to_svec(-2.0 * np.eye(n))
        res.append(("Z = -2 I", v, dr.margins_mp(cones, v), None))
    return tuple(res)


# worst error of a single PSD cone's margins in eps |Z|_2 per side: [alpha device, alpha host, beta device, beta host]
WORST = {}


def _print_worst(name):
    for n in sorted(WORST):
        w = WORST[n]
        print(f"[default start margins] worst so far, n={n} in eps |Z|_2 ({name}): alpha device {w[0]:.2f} / host {w[1]:.2f}, "
              f"beta device {w[2]:.2f} / host {w[3]:.2f}")


def _check_margins(what, got_a, got_b, ref):
    tol_a, tol_b, rh_a, rh_b = dr.margin_allowances(ref, SUM_TOL)
    ea, eb = float(abs(dr.mpf(got_a) - ref["alpha"])), float(abs(dr.mpf(got_b) - ref["beta"]))
    line = f"[default start margins] {what}: |alpha - ref| {ea:.3e} (allowed {tol_a:.3e}), |beta - ref| {eb:.3e} (allowed {tol_b:.3e})"
    if len(ref["psd"]) == 1 and ref["kind"] is PSDTriangleCone:
        k, n, norm2, a, b, ha, hb = ref["psd"][0]
        unit = dr.EPS * norm2
        line += f"; n={n} in eps |Z|_2: alpha device {ea / unit:.2f} host {rh_a:.2f}, beta device {eb / unit:.2f} host {rh_b:.2f}"
        w = WORST.setdefault(n, [0.0, 0.0, 0.0, 0.0])
        for i, x in enumerate((ea / unit, rh_a, eb / unit, rh_b)):
            w[i] = max(w[i], x)
    print(line)
    if ref["kind"] is NonnegativeCone:
        assert got_a == float(ref["alpha"]), (what, got_a, float(ref["alpha"]))
    assert ea <= tol_a, (what, got_a, float(ref["alpha"]), ea, tol_a)
    assert eb <= tol_b, (what, got_b, float(ref["beta"]), eb, tol_b)
    return ea, eb


# ---- 1. identity scaling ---------------------------------------------------------------------------------------------------------------

@ALL_SETS
@BOTH_P
def test_identity_scaling_writes_the_bits_of_the_host_path(name, pzero):
    hk, cones, _ = _handle(name, pzero)
    twin, tcones, _ = _handle(name, pzero)
    # a resident scaling first: the identity must drop it
    rng = np.random.default_rng(5)
    s, z = _point(cones, rng, False)
    ok = hk.h.update_scaling(s, z)[0]
    assert ok
    hk.cone_affine_ds()
    before = hipkkt.TRAFFIC["h2d_bytes"]
    hk.h.cone_set_identity_scaling()
    assert hipkkt.TRAFFIC["h2d_bytes"] == before
    with pytest.raises(ValueError):
        hk.cone_affine_ds()                      # refused until the next successful scaling
    with pytest.raises(ValueError):
        hk.cone_step_length(np.zeros(hk.m), np.zeros(hk.m), 1.0)
    tcones.set_identity_scaling()
    assert twin.kktsolver_update(tcones)
    kd, kh = hk.h.kkt()[2], twin.h.kkt()[2]
    same = kd.view(np.uint64) == kh.view(np.uint64)
    assert np.all(same), (name, int(np.sum(~same)), kd[~same][:5], kh[~same][:5])
    if any(isinstance(c, ZeroCone) for c in cones.cones):
        assert np.any(np.signbit(kd) & (kd == 0.0))      # the negated zero of hipkkt_set_hs
    assert hk.kktsolver_refactor()
    assert (hk.diagonal_regularizer, hk.last_nreg) == (twin.diagonal_regularizer, twin.last_nreg)
    # and a scaling brings the step calls back
    assert hk.h.update_scaling(s, z)[0]
    hk.cone_affine_ds()


# ---- 2. margins ----------------------------------------------------------------------------------------------------------------------------

@ALL_SETS
def test_margins_against_fifty_digits(name):
    hk, cones, _ = _handle(name, False)
    for pd in ("primal", "dual"):
        for label, v, ref, arm in _vectors(name):
            a, b = hk.h.cone_margins(v, pd)
            _check_margins(f"{name} {pd} {label}", a, b, ref)
    # the second-order rule on its own: alpha within SUM_TOL (|z0| + |z1|), beta = max(0, alpha)
    if name in ("soc_300", "soc_mix"):
        for label, v, ref, arm in _vectors(name):
            a, b = hk.h.cone_margins(v, "dual")
            if ref["kind"] is SecondOrderCone and len(cones.cones) == 1:
                assert b == max(0.0, a)
    _print_worst(name)


def test_margins_are_the_same_with_and_without_P():
    for name in ("mixed", "soc_mix"):
        h0, _, _ = _handle(name, False)
        h1, _, _ = _handle(name, True)
        for label, v, ref, arm in _vectors(name)[:4]:
            assert h0.h.cone_margins(v, "dual") == h1.h.cone_margins(v, "primal")


# ---- 3. shift ----------------------------------------------------------------------------------------------------------------------------------

@ALL_SETS
@BOTH_P
def test_shift_takes_the_reference_arm_and_adds_what_the_reference_adds(name, pzero):
    hk, cones, _ = _handle(name, pzero)
    zero_rows = np.concatenate([np.arange(r.start, r.stop) for c, r in zip(cones.cones, cones.rng_cones) if isinstance(c, ZeroCone)] +
                               [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    arms, targets = set(), set()
    for pd in ("primal", "dual"):
        for label, v, ref, arm in _vectors(name):
            tgt, br, margin = dr.decision_mp(ref)
            assert margin >= 1e-6, (name, label, margin)
            if arm is not None:
                assert br == arm, (name, label, br, arm, float(ref["alpha"]), float(tgt))
            w, mn, pos, tg, got_br = hk.h.cone_shift_to_interior(v, pd)
            _check_margins(f"{name} {pd} {label} (shift)", mn, pos, ref)
            assert got_br == br, (name, pd, label, got_br, br, mn, tg)
            assert tg == dr.target_of(pos, cones.degree), (name, label, tg, pos)
            want, want_br = dr.apply_shift(cones, v, pd, mn, tg)
            assert want_br == br
            assert dr.same_bits(w, want), (name, pd, label, np.flatnonzero(w != want)[:8])
            if zero_rows.size:
                if pd == "primal":
                    assert np.all(w[zero_rows] == 0.0) and not np.any(np.signbit(w[zero_rows]))
                else:
                    assert dr.same_bits(w[zero_rows], v[zero_rows])
            arms.add(br)
            targets.add(tg > 1.0)
    assert arms == {0, 1, 2}, (name, arms)
    if name in ("mixed", "soc_mix", "nn_700", "soc_300"):
        assert targets == {False, True}, (name, targets)


def test_zero_rows_and_minus_zero_under_the_zero_shift():
    hk, cones, _ = _handle("soc_mix", False)
    v = _placed(cones, np.random.default_rng(2), 1, 5.0, 1.0)
    v[0], v[1] = -0.0, -3.5                      # the Zero rows
    w, mn, pos, tg, br = hk.h.cone_shift_to_interior(v, "primal")
    assert br == 2 and dr.same_bits(w, dr.apply_shift(cones, v, "primal", mn, tg)[0])
    assert dr.same_bits(w[:2], [0.0, 0.0])
    w, mn, pos, tg, br = hk.h.cone_shift_to_interior(v, "dual")
    assert br == 2 and dr.same_bits(w[:2], [-0.0, -3.5]) and dr.same_bits(w[2:], v[2:])


# ---- 4. NaN -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["nonnegative", "second_order", "psd_8"])
def test_a_nan_row_gives_nan_margins_and_the_last_arm(where):
    hk, cones, _ = _handle("mixed", False)
    kinds = {"nonnegative": 0, "second_order": 2, "psd_8": 5}
    k = kinds[where]
    r = cones.rng_cones[k]
    v = _placed(cones, np.random.default_rng(9), 1, -0.7, 1.0)      # without the NaN: arm 0
    row = r.start + (1 if where != "psd_8" else 4)
    v[row] = float("nan")
    if where != "nonnegative":
        v[cones.rng_cones[0].start] = -0.0       # a Nonnegative row: the zero shift makes it +0.0
    with _Timeout(30):
        for pd in ("primal", "dual"):
            a, b = hk.h.cone_margins(v, pd)
            assert math.isnan(a)
            assert math.isnan(b) == (where != "nonnegative")      # `z > 0 ? z : 0` drops a Nonnegative NaN from beta
            w, mn, pos, tg, br = hk.h.cone_shift_to_interior(v, pd)
            assert math.isnan(mn) and br == 2
            ref_mn, ref_pos = dr.margins64(cones, v)
            assert math.isnan(ref_mn) and math.isnan(ref_pos) == math.isnan(pos)
            assert math.isnan(tg) == math.isnan(dr.target_of(ref_pos, cones.degree))
            want, want_br = dr.apply_shift(cones, v, pd, mn, tg)
            assert want_br == 2 and dr.same_bits(w, want)
            assert math.isnan(w[row]) and int(np.sum(np.isnan(w))) == 1
            if where != "nonnegative":
                assert w[cones.rng_cones[0].start] == 0.0 and not np.signbit(w[cones.rng_cones[0].start])


# ---- 5. the fused call -----------------------------------------------------------------------------------------------------------------------

def _host_default_start(twin, tcones, prob):
    """_default_start (solver.jl:383-405) up to the shifts on the host path of a twin plugin -> (x, z, s, steps, ok)"""
    Pt, q, A, b = prob
    m, n = A.shape
    tcones.set_identity_scaling()
    assert twin.kktsolver_update(tcones)
    x, z, s = np.zeros(n), np.zeros(m), np.zeros(m)
    steps = [0, 0]
    if Pt.nnz == 0:                              # kktsystem.jl:105-120
        twin.kktsolver_setrhs(np.zeros(n), b)
        ok = twin.kktsolver_solve(x, s)
        steps[0] = twin.last_ir_steps
        s *= -1.0
        twin.kktsolver_setrhs(-q, np.zeros(m))
        ok = twin.kktsolver_solve(None, z) and ok
        steps[1] = twin.last_ir_steps
    else:                                        # :121-128
        twin.kktsolver_setrhs(-q, b)
        ok = twin.kktsolver_solve(x, z)
        steps[0] = twin.last_ir_steps
        s[:] = -z
    return x, z, s, steps, ok


@ALL_SETS
@BOTH_P
def test_fused_call_matches_the_host_default_start(name, pzero):
    hk, cones, prob = _handle(name, pzero)
    twin, tcones, _ = _handle(name, pzero)
    Pt, q, A, b = prob
    m, n = A.shape
    xzs = hk.device_buffer(n + 2 * m)
    with pytest.raises(ValueError):
        hk.kktsolver_default_start(xzs)          # before hipkkt_set_qb
    hk.set_problem_vectors(q, b)
    before = dict(hipkkt.TRAFFIC)
    ir = hk._ir()
    st = hk.settings
    ok, scal, steps = hk.h.step_default_start_dev(xzs.ptr, st.static_regularization_enable, st.static_regularization_constant,
                                                  st.static_regularization_proportional, **ir)
    assert hipkkt.TRAFFIC["h2d_bytes"] == before["h2d_bytes"] and hipkkt.TRAFFIC["d2h_bytes"] - before["d2h_bytes"] == 64
    assert ok
    got = xzs.download()
    x, z, s, hsteps, hok = _host_default_start(twin, tcones, prob)
    assert hok
    assert (scal[0], int(scal[1])) == (twin.diagonal_regularizer, twin.last_nreg)
    assert list(steps) == hsteps, (list(steps), hsteps)
    # the device's margins against 50 digits of the host's unshifted (s, z), the gates of the margins test
    for what, v, o in (("s", s, 2), ("z", z, 5)):
        _check_margins(f"{name} fused {what}", scal[o], scal[o + 1], dr.margins_mp(tcones, v))
        assert scal[o + 2] == dr.target_of(scal[o + 1], tcones.degree)
    # the host's two shifts with the device's margins: the same bits, all rows
    s_sh, _ = dr.apply_shift(tcones, s, "primal", scal[2], scal[4])
    z_sh, _ = dr.apply_shift(tcones, z, "dual", scal[5], scal[7])
    want = np.concatenate([x, z_sh, s_sh])
    assert dr.same_bits(got, want), (name, pzero, np.flatnonzero(got != want)[:8], float(np.max(np.abs(got - want))))
    # twice in a row: the same bits
    ok2, scal2, steps2 = hk.h.step_default_start_dev(xzs.ptr, st.static_regularization_enable, st.static_regularization_constant,
                                                     st.static_regularization_proportional, **ir)
    _print_worst(name)
    assert ok2 and dr.same_bits(scal2, scal) and list(steps2) == list(steps) and dr.same_bits(xzs.download(), got)
    # the step calls wait for a scaling
    with pytest.raises(ValueError):
        hk.cone_affine_ds()
    xzs.close()


def test_fused_call_refuses_what_it_cannot_serve():
    from tests.step_support import _prep
    # a kind-4 registration
    Pt, A, cones = _prep(fx.basic_exp())
    m, n = A.shape
    hk = HipKKTSolver(Pt, A, cones, m, n, cl.Settings())
    hk.set_problem_vectors(np.ones(n), np.ones(m))
    xzs = hk.device_buffer(n + 2 * m)
    with pytest.raises(ValueError):
        hk.h.step_default_start_dev(xzs.ptr)
    with pytest.raises(ValueError):
        hk.h.cone_set_identity_scaling()
    with pytest.raises(ValueError):
        hk.h.cone_margins(np.ones(m), "dual")
    with pytest.raises(ValueError):
        hk.h.cone_shift_to_interior(np.ones(m), "primal")
    xzs.close()
    # PSD without the enable
    hk, cones, prob = _handle("mixed", False, flags={})
    assert not hk.steps_on_device
    hk.set_problem_vectors(prob[1], prob[3])
    xzs = hk.device_buffer(hk.n + 2 * hk.m)
    with pytest.raises(ValueError):
        hk.h.step_default_start_dev(xzs.ptr)
    with pytest.raises(ValueError):
        hk.h.cone_margins(np.ones(hk.m), "dual")
    xzs.close()
    # a pd that is neither primal nor dual
    hk, cones, prob = _handle("soc_mix", False)
    with pytest.raises(ValueError):
        hk.h.cone_margins(np.ones(hk.m), 2)


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------------------

E2E = [(f"sym:{k}", f, SYM_FLAGS) for k, f in SYM_END_TO_END.items()]
E2E += [(f"psd:{k}", f, dict(device_step=True, device_step_psd=True, **STEP_FLAGS)) for k, f in PSD_END_TO_END.items()]
E2E += [(f"psd_scaling:{k}", f, PSD_FLAGS) for k, f in PSD_END_TO_END.items()]


@pytest.mark.parametrize("case", E2E, ids=[c[0] for c in E2E])
def test_ipm_with_the_device_default_start_matches_the_host_start(case, monkeypatch):
    name, make, flags = case
    prob = make()
    with _Timeout(120):
        ref_solver = cl.Solver(*prob, cl.Settings(**flags))
        assert ref_solver._device_step and not ref_solver._device_default_start
        t0 = dict(hipkkt.TRAFFIC)
        ref = ref_solver.solve()
        t1 = dict(hipkkt.TRAFFIC)
        dev_solver = cl.Solver(*prob, cl.Settings(device_default_start=True, **flags))
        assert dev_solver._device_step and dev_solver._device_default_start
        host_start_calls = []
        monkeypatch.setattr(type(dev_solver), "_default_start", lambda self: host_start_calls.append(1))
        t2 = dict(hipkkt.TRAFFIC)
        got = dev_solver.solve()
        t3 = dict(hipkkt.TRAFFIC)
    assert not host_start_calls
    st = dev_solver.settings
    print(f"[default start {name}] {got.status} in {got.iterations} iterations (host start: {ref.iterations}); objective {got.obj_val!r} "
          f"vs {ref.obj_val!r}; default start {1e3 * dev_solver.info.timers['default start']:.2f} ms vs "
          f"{1e3 * ref_solver.info.timers['default start']:.2f} ms; h2d bytes {t3['h2d_bytes'] - t2['h2d_bytes']} vs "
          f"{t1['h2d_bytes'] - t0['h2d_bytes']}")
    assert got.status == ref.status, (got.status, ref.status)
    assert abs(got.iterations - ref.iterations) <= 1, (got.iterations, ref.iterations)
    if dr.is_finite(ref.obj_val) or dr.is_finite(got.obj_val):
        bound = 2.0 * max(st.tol_gap_abs, st.tol_gap_rel * max(1.0, abs(ref.obj_val)))
        assert abs(got.obj_val - ref.obj_val) <= bound, (got.obj_val, ref.obj_val, bound)
    ks = dev_solver.kktsystem.kktsolver
    saved = (t1["h2d_bytes"] - t0["h2d_bytes"]) - (t3["h2d_bytes"] - t2["h2d_bytes"])
    assert saved >= 8 * (ks.h.nHs + ks.n + 2 * ks.m), (saved, ks.h.nHs, ks.n, ks.m)
