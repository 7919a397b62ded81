"""CPU side of the on-device scaling of the non-symmetric cones (include/hipkkt.h hipkkt_set_cone_types_ex / hipkkt_update_scaling_ex):
what the stand-in hands to the plugin (kinds 0..6 + exponents), the length rule of the output vector, the adopt-from-slot round trip
of the three cone classes, and the agreement of header, ctypes binding and Julia glue on ABI 5 and the new prototypes.  No GPU."""
import os
import re

import numpy as np

import clarabel_jl_amd  # noqa: F401  (registers the dotted package directory)
import julia_standin as cl
from clarabel_jl_amd import hipkkt
from julia_standin.cones_nonsym import ExponentialCone, GenPowerCone, PowerCone
from tests import fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hipkkt_set_cone_types_ex", "hipkkt_get_nonsym_len", "hipkkt_update_scaling_ex", "hipkkt_update_scaling_ex_dev"]


def _cone_set():      # the cone set of tests/test_nonsymmetric_cones.py (kkt_cone_kinds() pinned there)
    return cl.CompositeCone([cl.ZeroConeT(2), cl.NonnegativeConeT(3), cl.ExponentialConeT(), cl.PowerConeT(0.3),
                             cl.GenPowerConeT([0.2, 0.8], 2), cl.SecondOrderConeT(6)])


def test_kinds_ex_names_the_non_symmetric_cones_and_leaves_the_old_kinds_alone():
    cones = _cone_set()
    kinds, alpha = cones.kkt_cone_kinds_ex()
    assert list(kinds) == [0, 1, 4, 5, 6, 2] and kinds.dtype == np.int32
    assert np.array_equal(alpha, [0.3, 0.2, 0.8]) and alpha.dtype == np.float64
    assert list(cones.kkt_cone_kinds()) == [0, 1, -1, -1, -1, 2]
    sym = cl.CompositeCone([cl.ZeroConeT(2), cl.NonnegativeConeT(3), cl.SecondOrderConeT(6), cl.PSDTriangleConeT(3)])
    kinds, alpha = sym.kkt_cone_kinds_ex()
    assert np.array_equal(kinds, sym.kkt_cone_kinds()) and len(alpha) == 0


def test_output_vector_length_rule():
    """15 doubles per three-row cone (Hs 6, H_dual 6, grad 3), 3 dim + dim1 + 1 per GenPower cone (grad dim, d1 dim1, d2 1, p dim,
    q dim1, r dim2)"""
    assert ExponentialCone().scaling_slot_len == 15 and PowerCone(0.4).scaling_slot_len == 15
    for d1, d2 in ((2, 1), (2, 2), (4, 3), (3, 1)):
        c = GenPowerCone(np.full(d1, 1.0 / d1), d2)
        assert c.scaling_slot_len == 3 * (d1 + d2) + d1 + 1
        assert c.scaling_slot_len == len(c.grad) + len(c.d1) + 1 + len(c.p) + len(c.q) + len(c.r)
    cones = _cone_set()
    assert sum(c.scaling_slot_len for c in cones if hasattr(c, "adopt_scaling")) == 15 + 15 + (3 * 4 + 2 + 1)


def _triu(M):
    return np.array([M[0, 0], M[0, 1], M[1, 1], M[0, 2], M[1, 2], M[2, 2]])


def test_adopt_from_slot_round_trip():
    """a cone that adopts the slot another cone's host scaling would produce ends in the same state: same Hs block, same mul_Hs!,
    same combined_ds_shift!"""
    rng = np.random.default_rng(3)
    for strategy in ("primal_dual", "dual"):
        src = _cone_set()
        s, z, mu = fx.scale_cones_nonsymmetric(src, rng, strategy)
        dst = _cone_set()
        for a, b, r in zip(src.cones, dst.cones, src.rng_cones):
            if isinstance(a, (ExponentialCone, PowerCone)):
                slot = np.concatenate([_triu(a.Hs), _triu(a.H_dual), a.grad])
            elif isinstance(a, GenPowerCone):
                slot = np.concatenate([a.grad, a.d1, [a.d2], a.p, a.q, a.r])
            else:
                assert not hasattr(b, "adopt_scaling")
                continue
            assert len(slot) == b.scaling_slot_len
            b.adopt_scaling(slot, z[r], mu)
            h1, h2 = np.zeros(6 if a.numel == 3 else a.numel), np.zeros(6 if a.numel == 3 else a.numel)
            a.get_Hs(h1)
            b.get_Hs(h2)
            assert np.array_equal(h1, h2) and np.array_equal(a.z, b.z) and np.array_equal(a.grad, b.grad)
            x = rng.standard_normal(a.numel)
            y1, y2 = np.zeros(a.numel), np.zeros(a.numel)
            a.mul_Hs(y1, x, np.zeros(a.numel))
            b.mul_Hs(y2, x, np.zeros(a.numel))
            assert np.array_equal(y1, y2)
            ds, dz = 0.01 * rng.standard_normal(a.numel), 0.01 * rng.standard_normal(a.numel)
            t1, t2 = np.zeros(a.numel), np.zeros(a.numel)
            a.combined_ds_shift(t1, dz.copy(), ds.copy(), 0.1 * mu)
            b.combined_ds_shift(t2, dz.copy(), ds.copy(), 0.1 * mu)
            assert np.array_equal(t1, t2)
            if isinstance(a, GenPowerCone):
                assert b.mu == mu and b.d2 == a.d2
            else:
                assert np.array_equal(b.Hs, b.Hs.T) and np.array_equal(b.H_dual, a.H_dual)


def test_host_scaling_can_leave_the_non_symmetric_cones_to_the_plugin():
    cones = _cone_set()
    s, z, mu = fx.scale_cones_nonsymmetric(cones, np.random.default_rng(4), "dual")
    fresh = _cone_set()
    assert fresh.update_scaling(s, z, mu, "dual", host_nonsymmetric=False)
    for a, b in zip(cones.cones, fresh.cones):
        if hasattr(b, "adopt_scaling"):
            assert not np.any(b.grad) and np.any(a.grad)           # untouched
        elif hasattr(a, "w"):
            assert np.array_equal(a.w, b.w)                         # the symmetric cones are scaled as before


def test_second_order_cone_adopts_the_device_scaling():
    """in a cone set with non-symmetric members the second-order cones take the plugin's (w, lambda, eta) too: same state as the host's
    own update_scaling! when handed the host's values"""
    rng = np.random.default_rng(8)
    for dim in (3, 7):
        a, b = cl.cones.SecondOrderCone(dim), cl.cones.SecondOrderCone(dim)
        s, z = rng.standard_normal(dim), rng.standard_normal(dim)
        s[0], z[0] = np.linalg.norm(s[1:]) + 0.7, np.linalg.norm(z[1:]) + 0.4
        assert a.update_scaling(s, z, 1.0)
        b.adopt_symmetric_scaling(a.w.copy(), a.lam.copy(), a.eta)
        nb = dim if a.is_sparse_expandable else dim * (dim + 1) // 2
        h1, h2 = np.zeros(nb), np.zeros(nb)
        a.get_Hs(h1)
        b.get_Hs(h2)
        assert np.array_equal(h1, h2) and np.array_equal(a.lam, b.lam)
        if a.is_sparse_expandable:
            assert np.array_equal(a.u, b.u) and np.array_equal(a.v, b.v)
        x = rng.standard_normal(dim)
        y1, y2 = np.zeros(dim), np.zeros(dim)
        a.mul_Hs(y1, x, np.zeros(dim))
        b.mul_Hs(y2, x, np.zeros(dim))
        assert np.array_equal(y1, y2)


def _strip(txt):
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


def test_header_binding_and_julia_glue_agree_on_abi_5_and_the_new_prototypes():
    hdr = open(os.path.join(ROOT, "include", "hipkkt.h")).read()
    v = int(re.search(r"#define\s+HIPKKT_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert v == 5 and hipkkt.ABI_VERSION == 5
    assert "const HIPKKT_ABI_VERSION = Int32(5)" in open(os.path.join(ROOT, "julia", "ext", "hipkkt_lib.jl")).read()
    for name, val in (("HIPKKT_CONE_EXP", 4), ("HIPKKT_CONE_POW", 5), ("HIPKKT_CONE_GENPOW", 6)):
        assert re.search(rf"#define\s+{name}\s+{val}\b", hdr), name
    src = re.sub(r"\s+", " ", _strip(hdr))
    want = {
        "hipkkt_set_cone_types_ex": "hipkkt_handle h, int64_t ncones, const int32_t *kinds, int64_t nalpha, const double *alpha",
        "hipkkt_get_nonsym_len": "hipkkt_handle h, int64_t *len",
        "hipkkt_update_scaling_ex": "hipkkt_handle h, const double *s, const double *z, const double *psd_R, double mu, int32_t strategy, "
                                    "double *w_out, double *lambda_out, double *soc_eta_out, double *nonsym_out, int32_t *scaling_ok",
        "hipkkt_update_scaling_ex_dev": "hipkkt_handle h, const double *s_dev, const double *z_dev, const double *psd_R_dev, double mu, "
                                        "int32_t strategy, double *w_out_dev, double *lambda_out_dev, double *soc_eta_out_dev, "
                                        "double *nonsym_out_dev, int32_t *scaling_ok",
    }
    for name, params in want.items():
        m = re.search(r"int32_t " + name + r"\s*\(([^()]*)\)\s*;", src)
        assert m, name
        assert re.sub(r"\s+", " ", m.group(1)).strip() == params, name
        assert name in hipkkt.SYMBOLS
    # the old prototypes are what they were
    assert "int32_t hipkkt_set_cone_types(hipkkt_handle h, int64_t ncones, const int32_t *kinds);" in src
    assert ("int32_t hipkkt_update_scaling(hipkkt_handle h, const double *s, const double *z, const double *psd_R, double *w_out, "
            "double *lambda_out, double *soc_eta_out, int32_t *scaling_ok);") in src
    # the ctypes binding binds them with the header's parameter counts; the Handle offers the four methods
    L = hipkkt.lib()
    counts = {"hipkkt_set_cone_types_ex": 5, "hipkkt_get_nonsym_len": 2, "hipkkt_update_scaling_ex": 11, "hipkkt_update_scaling_ex_dev": 11}
    for name in NEW:
        assert len(getattr(L, name).argtypes) == counts[name], name
    for meth in ("set_cone_types_ex", "nonsym_len", "update_scaling_ex", "update_scaling_ex_dev"):
        assert callable(getattr(hipkkt.Handle, meth))
    # the Julia glue registers kinds 4..6 with their exponents and reads the slots back
    jl = open(os.path.join(ROOT, "julia", "ext", "kktsolver_hip.jl")).read()
    for name in ("hipkkt_set_cone_types_ex", "hipkkt_get_nonsym_len", "hipkkt_update_scaling_ex"):
        assert f"(:{name}, libhipkkt)" in jl, name
    assert "c isa ExponentialCone ? 4 : c isa PowerCone ? 5 : c isa GenPowerCone ? 6" in jl
    for field in ("K.Hs", "K.H_dual", "K.grad", "K.z", "dat.grad", "dat.d1", "dat.d2", "dat.p", "dat.q", "dat.r", "dat.μ", "dat.z"):
        assert field in jl, field


def test_the_solver_mirror_reaches_the_cones_by_duck_typing():
    """nothing under clarabel.jl_amd/ names the stand-in (tests/test_abi.py); kktsolver.py asks the cones object for kkt_cone_kinds_ex()
    and each cone for adopt_scaling / scaling_slot_len"""
    src = open(os.path.join(ROOT, "clarabel.jl_amd", "kktsolver.py")).read()
    for tok in ("kkt_cone_kinds_ex", "adopt_scaling", "scaling_slot_len", "update_scaling_ex", "set_cone_types_ex"):
        assert tok in src, tok
    assert "julia_standin" not in src and "cones_nonsym" not in src
