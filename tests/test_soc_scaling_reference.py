"""The CPU half of the second-order cones' scaling tests (tests/soc_scaling_reference.py): the exact scaling satisfies the identities
R1 .. R4, the stand-in alone meets every gate that tests/test_gpu_soc_scaling.py puts on the device, k_scaling_soc's order of operations
emulated in numpy meets them too, and the same emulation with a planted defect -- one element left out of one sum at a pass boundary, a
slipped offset into (u, v), the eta^2 of the wrong cone -- does not."""
import numpy as np
import pytest

from tests import soc_scaling_reference as ssr


def _emulated_set(cones, s, z, drop=None):
    """emulate_kernel over a cone set -> (w, lam, eta, u_all, v_all, d by ordinal); drop = {ordinal: (sum, element)}"""
    socs = ssr.soc_list(cones)
    w, lam, eta = np.zeros(cones.numel), np.zeros(cones.numel), np.zeros(len(socs))
    u_all, v_all, d = [], [], {}
    for k, c, r, _, uv in socs:
        o = ssr.emulate_kernel(s[r], z[r], (drop or {}).get(k))
        assert o["ok"]
        w[r], lam[r], eta[k] = o["w"], o["lam"], o["eta"]
        if uv is not None:
            u_all.append(o["u"])
            v_all.append(o["v"])
            d[k] = o["d"]
    return w, lam, eta, np.concatenate(u_all), np.concatenate(v_all), d


def _gates(name, seed, late, scaling, tag):
    cones, s, z = ssr.host_cones(name, seed, late)
    host = ssr.standin_figures(name, seed, late)
    C, early = ssr.standin_constants()
    w, lam, eta, u_all, v_all, d = scaling(cones, s, z)
    rows = ssr.figures_of(cones, s, z, host.exact, w, lam, eta, u_all, v_all, lambda k, c: d[k])
    tols = ssr.late_tolerances(cones, s, z, host.exact) if late else None
    return ssr.check_rows(f"{tag} {name} seed {seed} {'late' if late else 'early'}", rows, host.rows, late, tols, C, early)


def test_sum_bound_and_cone_sets():
    assert [ssr.sum_roundings(d) for d in (2, 256, 257, 512, 513, 1025)] == [11, 11, 12, 12, 13, 15]
    cones, _, _ = ssr.host_cones("many", *ssr.POINTS[0])
    assert len(cones.cones) == 300
    socs = ssr.soc_list(cones)
    sparse = [k for k, c, _, _, uv in socs if uv is not None]
    assert len(socs) == 200 and sparse != list(range(len(sparse)))      # kSocOrd != the cone's index among the second-order cones
    assert len({c.dim for _, c, _, _, _ in socs}) == 7                   # SOC(2 .. 8): uv0 is irregular
    for edge in (256, 512):
        assert any(c.kind_code == 1 and r.start < edge < r.stop - 1 for c, r in zip(cones.cones, cones.rng_cones)), edge
    dims = [c.dim for _, c, _, _, _ in ssr.soc_list(ssr.host_cones("long", *ssr.POINTS[0])[0])]
    assert dims == [2, 255, 256, 257, 258, 511, 512, 513, 1025, 3, 4, 5]


@pytest.mark.parametrize("name", list(ssr.CONE_SETS))
@pytest.mark.parametrize("seed,late", [ssr.POINTS[0], ssr.POINTS[-1]])
def test_exact_scaling_satisfies_the_identities(name, seed, late):
    """50 digits: unit 1e-50.  The sums have up to 1025 terms, res(s) and res(z) of a late point lose up to 6 digits to their relative
    gap and R2 another log10(w0^2): 1e-45 times those two factors"""
    cones, s, z = ssr.host_cones(name, seed, late)
    worst = {}
    for (k, c, r, _, uv), (w, lam, eta) in zip(ssr.soc_list(cones), ssr.standin_figures(name, seed, late).exact):
        gap = min(float((x[0] - np.linalg.norm(x[1:])) / x[0]) for x in (s[r], z[r]))
        terms = ssr.exact_sparse_terms(w) if uv is not None else ()
        for rn, v in ssr.residuals(w, lam, eta, s[r], z[r], *terms).items():
            bound = 1e-45 / gap * (float(w[0]) ** 2 if rn == "R2" else 1.0)
            worst[rn] = max(worst.get(rn, 0.0), v / bound)
            assert v <= bound, (c.dim, rn, v, bound)
    print(f"[soc scaling exact {name} {'late' if late else 'early'}] largest residual / bound: {worst}")


@pytest.mark.parametrize("name", list(ssr.CONE_SETS))
@pytest.mark.parametrize("seed,late", ssr.POINTS)
def test_standin_meets_every_gate(name, seed, late):
    C, early = ssr.standin_constants()
    print(f"[soc scaling] C (largest normalised residual of the stand-in) {C}; its worst early forward errors / eps "
          f"{ {q: v / ssr.EPS for q, v in early.items()} }")

    def standin(cones, s, z):
        return ssr.host_scaling(cones)[:5] + ({k: c.d for k, c, _, _, uv in ssr.soc_list(cones) if uv is not None},)

    worst = _gates(name, seed, late, standin, "stand-in")
    print(f"[soc scaling stand-in {name} seed {seed} {'late' if late else 'early'}] worst value / gate {worst}")


@pytest.mark.parametrize("name", list(ssr.CONE_SETS))
@pytest.mark.parametrize("seed,late", ssr.POINTS)
def test_kernel_order_in_numpy_meets_every_gate(name, seed, late):
    worst = _gates(name, seed, late, _emulated_set, "kernel order")
    print(f"[soc scaling kernel order {name} seed {seed} {'late' if late else 'early'}] worst value / gate {worst}")


def _ordinal(cones, dim):
    return [k for k, c, _, _, _ in ssr.soc_list(cones) if c.dim == dim][0]


@pytest.mark.parametrize("seed,late", ssr.POINTS)
@pytest.mark.parametrize("dim,which,element", [(257, 2, 256), (258, 0, 257), (258, 1, 257), (258, 3, 257), (1025, 2, 1024), (1025, 3, 1024),
                                               (255, 2, 1)])
def test_negative_control_an_element_left_out_of_a_sum(seed, late, dim, which, element):
    """one element missing from one of the four sums: the first of the second pass (element 256 of the `i = t` loop that forms sum 2,
    element 257 of the `i = 1 + t` loops of the others), thread 0's fifth pass and the last element of SOC(1025), the first element of a
    cone of one pass.  R2 catches each, on that cone and no other"""
    cones, s, z = ssr.host_cones("long", seed, late)
    k = _ordinal(cones, dim)
    with pytest.raises(AssertionError) as e:
        _gates("long", seed, late, lambda *a: _emulated_set(*a, drop={k: (which, element)}), "planted")
    failed = {(kk, q) for kk, _, q, _ in e.value.args[0][1]}
    assert (k, "R2") in failed and all(kk == k for kk, _ in failed), failed


@pytest.mark.parametrize("seed,late", ssr.POINTS)
def test_negative_control_slipped_tables(seed, late):
    """(u, v) of a sparse cone read one element off its offset, and a row 0 written with the eta^2 of the next sparse cone (a slipped
    kSocUv0 / kSocOrd): R4 catches both, on the cone that was hit only"""
    cones, _, _ = ssr.host_cones("many", seed, late)
    sparse = [(k, c, uv) for k, c, _, _, uv in ssr.soc_list(cones) if uv is not None]
    for slip in ("uv0", "ord"):
        k, c, uv = sparse[len(sparse) // 2]

        def planted(cones, s, z):
            w, lam, eta, u_all, v_all, d = _emulated_set(cones, s, z)
            if slip == "uv0":
                u_all[uv:uv + c.dim], v_all[uv:uv + c.dim] = u_all[uv + 1:uv + 1 + c.dim].copy(), v_all[uv + 1:uv + 1 + c.dim].copy()
            else:
                k2 = sparse[len(sparse) // 2 + 1][0]
                d[k] = d[k] * (eta[k2] * eta[k2]) / (eta[k] * eta[k])
            return w, lam, eta, u_all, v_all, d

        with pytest.raises(AssertionError) as e:
            _gates("many", seed, late, planted, "planted " + slip)
        failed = {(kk, q) for kk, _, q, _ in e.value.args[0][1]}
        assert failed == {(k, "R4")}, (slip, failed)


def test_dense_block_is_the_stand_ins():
    """dense_block (the kernel's association) against get_Hs of the stand-in, which multiplies by eta^2 last as well: bit for bit"""
    cones, s, z = ssr.host_cones("many", *ssr.POINTS[0])
    for k, c, r, rb, uv in ssr.soc_list(cones):
        if uv is None:
            block = np.zeros(rb.stop - rb.start)
            c.get_Hs(block)
            assert np.array_equal(-block, ssr.dense_block(c.w, c.eta)), c.dim
