"""``HipKKTSolver`` — host-side mirror of the reference's KKT-solver plugin for seam L1.

It implements the ``AbstractKKTSolver`` contract (src/kktsolvers/kktsolver_defaults.jl:2-47) with
the same names, argument meaning and success semantics as the reference's ``DirectLDLKKTSolver``
(src/kktsolvers/kktsolver_directldl.jl); everything below the method boundary runs in the HIP
library through the C ABI (include/hipkkt.h).  The Julia file a maintainer would add is shown in
INTEGRATION.md; this class is its Python twin so that parity tests read like the reference's."""
from __future__ import annotations

import os

import numpy as np

from . import hipkkt
from .settings import Settings


_DEBUG = os.environ.get("HIPKKT_DEBUG", "0") == "1"


def cone_set_steps_on_device(cones, nonsymmetric=False, genpower=False, psd=False, psd_large=False, mixed=False, mixed_large=False) -> bool:
    """the step entry points (hipkkt_cone_* / hipkkt_step_*) serve cone sets of ZeroCone, NonnegativeCone and SecondOrderCone only: a PSD
    cone's step length needs eigenvalue decompositions, the non-symmetric cones need backtracking and barriers.
    nonsymmetric=True: ExponentialCone and PowerCone members qualify as well (hipkkt_step_enable_cone3); Generalized Power and PSD
    members still do not.
    genpower=True (with nonsymmetric=True): Generalized Power members qualify too (hipkkt_step_enable_genpow); PSD members do not.
    psd=True: PSD triangle members qualify when every side is at most hipkkt.PSD_STEP_MAX_DIM and the set has no Exponential / Power /
    Generalized Power member (hipkkt_step_enable_psd).
    psd_large=True (with psd=True): the side limit is hipkkt.PSD_STEP_LARGE_MAX_DIM (hipkkt_step_enable_psd_large); alone it widens
    nothing.
    mixed=True (with nonsymmetric=True and psd=True): PSD triangle members of side at most hipkkt.PSD_STEP_MAX_DIM qualify next to
    Exponential / Power members, and next to Generalized Power members with genpower=True (hipkkt_step_enable_mixed); psd_large does not
    widen that limit; alone it widens nothing.
    mixed_large=True (with mixed=True, nonsymmetric=True and psd=True): the side limit of such a set is hipkkt.PSD_STEP_LARGE_MAX_DIM
    (hipkkt_step_enable_mixed_large); alone it widens nothing"""
    if not hasattr(cones, "kkt_cone_kinds"):
        return False
    kinds = cones.kkt_cone_kinds_ex()[0] if hasattr(cones, "kkt_cone_kinds_ex") else cones.kkt_cone_kinds()
    kinds = np.asarray(kinds)
    ok = (kinds >= 0) & (kinds <= 2)
    if nonsymmetric:
        ok = ok | (kinds == 4) | (kinds == 5)
        if genpower:
            ok = ok | (kinds == 6)
    has_nonsym = bool(np.any(kinds >= 4))
    if psd and bool(np.any(kinds == 3)) and (not has_nonsym or (mixed and nonsymmetric)):
        numel = np.asarray(cones.kkt_descriptors()[0])[kinds == 3]
        sides = ((np.sqrt(8.0 * numel + 1.0) - 1.0) / 2.0 + 0.5).astype(np.int64)
        large = mixed_large if has_nonsym else psd_large
        limit = hipkkt.PSD_STEP_LARGE_MAX_DIM if large else hipkkt.PSD_STEP_MAX_DIM
        if bool(np.all(sides <= limit)):
            ok = ok | (kinds == 3)
    return kinds.size > 0 and bool(np.all(ok))


class HipKKTSolver:
    def __init__(self, P, A, cones, m, n, settings: Settings, **optkw):
        """ref: DirectLDLKKTSolver{T}(P,A,cones,m,n,settings), kktsolver_directldl.jl:46-92.
        P: n x n triu CSC (scipy), A: m x n CSC, cones: CompositeCone."""
        self.settings = settings
        self.m, self.n = m, n
        numel, hs_dense, sparse_kind, dim1 = cones.kkt_descriptors()
        self.p_nnz = int(P.nnz)
        self.h = hipkkt.Handle.from_parts(
            P, A, numel, hs_dense, sparse_kind, dim1, device=settings.device_id,
            dynamic_reg_eps=settings.dynamic_regularization_eps,
            dynamic_reg_delta=settings.dynamic_regularization_delta, **optkw)
        self.p = self.h.p
        self.Hsblocks = np.zeros(self.h.nHs)          # ref: _allocate_kkt_Hsblocks
        # sparse-expandable cones in sparse-map order: SOC (rank-2 expansion, batched upload) and GenPow (rank-3 expansion)
        sparse = [c for c in cones if c.is_sparse_expandable]
        self._soc = [c for c in sparse if getattr(c, "sparse_kind", 1) == 1]
        self._genpow = [(i, c) for i, c in enumerate(sparse) if getattr(c, "sparse_kind", 1) == 2]
        self._soc_total = sum(c.dim for c in self._soc)
        self._u = np.zeros(self._soc_total)
        self._v = np.zeros(self._soc_total)
        self._eta2 = np.zeros(len(self._soc))
        # PSD cones: the Hs block (packed triu of W (x)_s W, numel^2/2 values) is formed on the device from the
        # n x n matrix W = R R^T (hipkkt_set_hs_psd): no host skron!, no upload of the block
        self._psd = [(c, r.start) for c, r in zip(cones.cones, cones.rng_blocks) if hasattr(c, "RRt")]
        self._psd_off = np.array([off for _, off in self._psd], dtype=np.int64)
        self._psd_dim = np.array([c.n for c, _ in self._psd], dtype=np.int64)
        self._psd_cones = tuple(c for c, _ in self._psd)
        # N1: cone types for the on-device update_scaling! / get_Hs! (hipkkt_set_cone_types); optional in the cones object
        # (hipkkt_set_cone_types knows the symmetric cones; a cones object that also offers kkt_cone_kinds_ex() -> (kinds 0..6, alpha)
        # and has an Exponential / Power / GenPower member is registered through hipkkt_set_cone_types_ex)
        kinds = cones.kkt_cone_kinds() if hasattr(cones, "kkt_cone_kinds") else None
        self._has_cone_kinds = kinds is not None and bool(np.all(np.asarray(kinds) >= 0))
        self.scales_nonsymmetric = False
        kinds_ex, alpha = cones.kkt_cone_kinds_ex() if hasattr(cones, "kkt_cone_kinds_ex") else (None, None)
        if kinds_ex is not None and bool(np.any(np.asarray(kinds_ex) >= 4)) and bool(np.all(np.asarray(kinds_ex) >= 0)):
            self.h.set_cone_types_ex(kinds_ex, alpha)
            self._kinds_ex = [int(k) for k in kinds_ex]
            self._has_cone_kinds = self.scales_nonsymmetric = True
        elif self._has_cone_kinds:
            self.h.set_cone_types(kinds)
        # the interior-point step on the device (hipkkt_cone_* / hipkkt_step_*) serves Zero / Nonnegative / SecondOrder cone sets only
        self._steps_on_device = cone_set_steps_on_device(cones)
        # ... and, opted in by Settings.device_step_nonsymmetric, sets with Exponential / Power members
        self.steps_nonsymmetric = False
        if not self._steps_on_device and getattr(settings, "device_step_nonsymmetric", False) and self.scales_nonsymmetric \
                and cone_set_steps_on_device(cones, nonsymmetric=True):
            self.h.step_enable_cone3(True, settings.linesearch_backtrack_step, settings.min_terminate_step_length)
            self._steps_on_device = self.steps_nonsymmetric = True
        # ... and, opted in by Settings.device_step_genpower on top of it, sets with Generalized Power members
        elif not self._steps_on_device and getattr(settings, "device_step_nonsymmetric", False) \
                and getattr(settings, "device_step_genpower", False) and self.scales_nonsymmetric \
                and cone_set_steps_on_device(cones, nonsymmetric=True, genpower=True):
            self.h.step_enable_genpow(True, settings.linesearch_backtrack_step, settings.min_terminate_step_length)
            self._steps_on_device = self.steps_nonsymmetric = True
        # ... and, opted in by Settings.device_step_psd, symmetric sets with PSD triangle members: the Cholesky / SVD of their scaling stay
        # with the caller, whose (R, Rinv, lambda) go to the device with every scaling (hipkkt_step_enable_psd)
        # With Settings.device_step_psd_large on top, a set with a side of 65 .. 128 qualifies too (hipkkt_step_enable_psd_large); its
        # Cholesky / SVD and its default start stay with the caller whatever device_scaling_psd / device_default_start say, unless
        # Settings.device_scaling_psd_large / device_default_start_psd_large are set on top of those (below)
        self.steps_psd = self.steps_psd_large = False
        psd_ok = not self._steps_on_device and getattr(settings, "device_step_psd", False) and self._has_cone_kinds \
            and not self.scales_nonsymmetric
        if psd_ok and cone_set_steps_on_device(cones, psd=True):
            self.h.step_enable_psd(True)
            self._steps_on_device = self.steps_psd = True
        elif psd_ok and getattr(settings, "device_step_psd_large", False) and cone_set_steps_on_device(cones, psd=True, psd_large=True):
            self.h.step_enable_psd_large(True)
            self._steps_on_device = self.steps_psd = self.steps_psd_large = True
        # ... and, opted in by Settings.device_step_mixed on top of device_step_nonsymmetric and device_step_psd, sets that hold PSD
        # triangle members (sides <= 64) next to Exponential / Power members, and next to Generalized Power members with
        # device_step_genpower (hipkkt_step_enable_mixed).  The PSD factors follow the protocol of steps_psd / scales_psd
        # With Settings.device_step_mixed_large (and device_step_psd_large) on top, sides of 65 .. 128 qualify in such a set too
        # (hipkkt_step_enable_mixed_large); its Cholesky / SVD follow device_scaling_psd_large as for steps_psd_large, its start stays
        # the caller's unit initialisation
        self.steps_mixed = False
        mixed_ok = not self._steps_on_device and getattr(settings, "device_step_mixed", False) \
            and getattr(settings, "device_step_nonsymmetric", False) and getattr(settings, "device_step_psd", False) \
            and self.scales_nonsymmetric and self._psd_cones
        mixed_kw = dict(nonsymmetric=True, genpower=bool(getattr(settings, "device_step_genpower", False)), psd=True, mixed=True)
        if mixed_ok and cone_set_steps_on_device(cones, **mixed_kw):
            self.h.step_enable_mixed(True, settings.linesearch_backtrack_step, settings.min_terminate_step_length)
            self._steps_on_device = self.steps_nonsymmetric = self.steps_psd = self.steps_mixed = True
        elif mixed_ok and getattr(settings, "device_step_mixed_large", False) and getattr(settings, "device_step_psd_large", False) \
                and cone_set_steps_on_device(cones, mixed_large=True, **mixed_kw):
            self.h.step_enable_mixed_large(True, settings.linesearch_backtrack_step, settings.min_terminate_step_length)
            self._steps_on_device = self.steps_nonsymmetric = self.steps_psd = self.steps_psd_large = self.steps_mixed = True
        if self.steps_psd:
            rows = [r for c, r in zip(cones.cones, cones.rng_cones) if hasattr(c, "RRt")]
            self._psd_rows = rows
            self._psd_span = (rows[0].start, rows[-1].stop)
            self._psd_nr = int(np.sum(self._psd_dim * self._psd_dim))
            self._psd_dev = None      # [R | Rinv | lambda] in device memory (kktsolver_update_scaling_dev)
        # ... whose Cholesky / SVD the device does as well when Settings.device_scaling_psd is set (hipkkt_psd_scaling_enable): the
        # scaling call then takes nothing but the resident (s, z)
        self.scales_psd = False
        if self.steps_psd and not self.steps_psd_large and getattr(settings, "device_scaling_psd", False):
            self.h.psd_scaling_enable(True)
            self.scales_psd = True
        # ... for a set with a side of 65 .. 128 when Settings.device_scaling_psd_large is set on top (hipkkt_psd_scaling_enable_large)
        elif self.steps_psd_large and getattr(settings, "device_scaling_psd", False) \
                and getattr(settings, "device_scaling_psd_large", False):
            self.h.psd_scaling_enable_large(True)
            self.scales_psd = True
        # ... and whose default start the device serves when Settings.device_default_start_psd_large is set on top of
        # device_default_start (hipkkt_step_default_start_enable_psd_large)
        self.starts_psd_large = False
        if self.steps_psd_large and not self.steps_mixed and getattr(settings, "device_default_start", False) \
                and getattr(settings, "device_default_start_psd_large", False):
            self.h.step_default_start_enable_psd_large(True)
            self.starts_psd_large = True
        self.scaling_nonsym = None
        self.scaling_w = self.scaling_lambda = self.scaling_soc_eta = None
        self.diagonal_regularizer = 0.0
        self.last_ir_steps = 0
        self.total_ir_steps = 0
        self.nsolves = 0
        self.last_nreg = 0

    # ref: kktsolver_update!, kktsolver_directldl.jl:197-245
    def kktsolver_update(self, cones) -> bool:
        # PSD cones whose block is not formed yet (i.e. after update_scaling!; the identity scaling sets Hs = I exactly,
        # :66-75, and goes the host way) get it from the device-side skron
        dev = [k for k, c in enumerate(self._psd_cones) if not c._hs_valid]
        cones.get_Hs(self.Hsblocks, skip=tuple(self._psd_cones[k] for k in dev))   # :223 (host cone algebra)
        self.h.set_hs(self.Hsblocks)                   # :225-228 negate + scatter, on the device
        if dev:
            self.h.set_hs_psd(self._psd_off[dev], self._psd_dim[dev],
                              np.concatenate([self._psd_cones[k].RRt.ravel() for k in dev]))
        if self._soc:                                  # :235-241 sparse-cone expansion columns
            off = 0
            for i, c in enumerate(self._soc):
                self._u[off:off + c.dim] = c.u
                self._v[off:off + c.dim] = c.v
                self._eta2[i] = c.eta * c.eta
                off += c.dim
            self.h.set_soc_batch(self._eta2, self._u, self._v)
        for i, c in self._genpow:                      # _csc_update_sparsecone(::GenPowerCone), directldl_datamaps.jl:146-167
            self.h.set_genpow(i, float(np.sqrt(c.mu)), c.p, c.q, c.r)
        return self._refactor()

    def _refactor(self) -> bool:
        st = self.settings                             # :243, :247-294
        ok, eps, nreg = self.h.refactor(st.static_regularization_enable, st.static_regularization_constant,
                                        st.static_regularization_proportional)
        self.diagonal_regularizer = eps
        self.last_nreg = nreg
        if _DEBUG:
            print(f"[hipkkt] refactor ok={ok} eps={eps:.3e} dynamic_regularisations={nreg}")
        return ok

    # kktsolver_update! fed with the iterate instead of the cones' scaling -- update_scaling! + get_Hs! of
    # the Zero / Nonnegative / SecondOrder cones and skron(R R^T) of the PSD cones run on the device (hipkkt_update_scaling); nothing
    # but (s, z) and the PSD cones' R factors crosses PCIe.  The device's (w, lambda, eta) are kept for the caller.
    # With Exponential / Power / GenPower members (hipkkt_update_scaling_ex) the call needs mu and the scaling strategy
    # ("primal_dual" / "dual" or 0 / 1; None = what the cone set allows, solver.jl:222); every such cone then ADOPTS the device's values
    # from its slot of the output vector (cone.adopt_scaling(slot, z, mu)), so that the matrix and the caller's mul_Hs! /
    # combined_ds_shift! use the same numbers.
    def kktsolver_update_scaled(self, cones, s, z, mu=None, strategy=None) -> bool:
        if not self._has_cone_kinds:
            raise hipkkt.HipKKTError("kktsolver_update_scaled: the cones object does not provide kkt_cone_kinds()")
        R = np.concatenate([c.R.ravel(order="F") for c in self._psd_cones]) if self._psd_cones else None
        if self.scales_nonsymmetric:
            if mu is None:
                raise ValueError("kktsolver_update_scaled: a cone set with Exponential / Power / GenPower cones needs mu")
            if strategy is None:
                strategy = 0 if cones.allows_primal_dual_scaling() else 1
            strategy = {"primal_dual": 0, "dual": 1}.get(strategy, strategy)
            if self.steps_psd:      # (steps_mixed: the step reads the PSD factors, as below)
                self.h.psd_set_factors(*self._psd_factors())
            ok, self.scaling_w, self.scaling_lambda, self.scaling_soc_eta, self.scaling_nonsym = \
                self.h.update_scaling_ex(s, z, mu, strategy, R)
            if not ok:
                return False
            # (a second-order cone that offers adopt_symmetric_scaling takes the device's w, lambda, eta as well: on the late iterates
            # of these problems a host copy that differs from the matrix in the last bits makes the primal residual grow again)
            off, soc = 0, 0
            for c, r, kind in zip(cones.cones, cones.rng_cones, self._kinds_ex):
                if hasattr(c, "adopt_scaling"):
                    k = c.scaling_slot_len
                    c.adopt_scaling(self.scaling_nonsym[off:off + k], np.asarray(z)[r], float(mu))
                    off += k
                elif kind == 2:
                    if hasattr(c, "adopt_symmetric_scaling"):
                        c.adopt_symmetric_scaling(self.scaling_w[r], self.scaling_lambda[r], self.scaling_soc_eta[soc])
                    soc += 1
            assert off == len(self.scaling_nonsym)
            return self._refactor()
        if self.steps_psd:
            self.h.psd_set_factors(*self._psd_factors())
        ok, self.scaling_w, self.scaling_lambda, self.scaling_soc_eta = self.h.update_scaling(s, z, R)
        if not ok:
            return False
        return self._refactor()

    # ref: kktsolver_setrhs!, :313-327
    def kktsolver_setrhs(self, rhsx, rhsz):
        self.h.setrhs(rhsx, rhsz)

    # ref: kktsolver_solve!, :346-371 (lhsx / lhsz may be None = Julia `nothing`)
    def kktsolver_solve(self, lhsx, lhsz) -> bool:
        st = self.settings
        ok, steps = self.h.solve(lhsx, lhsz, st.iterative_refinement_enable, st.iterative_refinement_reltol,
                                 st.iterative_refinement_abstol, st.iterative_refinement_max_iter,
                                 st.iterative_refinement_stop_ratio)
        self.last_ir_steps = steps
        self.total_ir_steps += steps
        self.nsolves += 1
        if _DEBUG:
            print(f"[hipkkt] solve ok={ok} ir_steps={steps}")
        return ok

    # several right-hand sides on the current factorisation (rhsx [k, n], rhsz [k, m]), refined
    # like kktsolver_solve! refines one, two at a time on concurrent device contexts
    def kktsolver_solve_multi(self, rhsx, rhsz, lhsx, lhsz) -> bool:
        st = self.settings
        ok, steps = self.h.solve_multi(rhsx, rhsz, lhsx, lhsz, st.iterative_refinement_enable, st.iterative_refinement_reltol,
                                       st.iterative_refinement_abstol, st.iterative_refinement_max_iter,
                                       st.iterative_refinement_stop_ratio)
        self.last_ir_steps = int(steps[-1]) if len(steps) else 0
        self.total_ir_steps += int(np.sum(steps))
        self.nsolves += len(steps)
        if _DEBUG:
            print(f"[hipkkt] solve_multi ok={ok} ir_steps={list(steps)}")
        return ok

    # SURVEY section 8(f) row N2, second half: kkt_solve! (kktsystem.jl:135-215) between the caller's cone algebra and mul_Hs! --
    # the solve for (x1, z1), the d tau numerator / denominator (dots with q, b, quad_form with P) and dx, dz on the device.
    # const_pending: the constant-rhs solve that kkt_update! left pending runs in the same call (its solution stays resident).
    # Needs set_problem_vectors(q, b).  Returns (ok, dtau).
    def kktsolver_kkt_solve_reduced(self, rhs_x, workz, var_x, tau, kappa, rhs_tau, rhs_kappa, const_pending, lhs_x, lhs_z):
        st = self.settings
        ok, dtau, scal, steps = self.h.kkt_solve_reduced(rhs_x, workz, var_x, tau, kappa, rhs_tau, rhs_kappa, const_pending, lhs_x, lhs_z,
                                                         st.iterative_refinement_enable, st.iterative_refinement_reltol,
                                                         st.iterative_refinement_abstol, st.iterative_refinement_max_iter,
                                                         st.iterative_refinement_stop_ratio)
        self.last_ir_steps = int(steps[0])
        self.total_ir_steps += int(steps[0]) + (int(steps[1]) if const_pending else 0)
        self.nsolves += 2 if const_pending else 1
        self.last_reduced_scalars = scal
        if _DEBUG:
            print(f"[hipkkt] kkt_solve_reduced ok={ok} dtau={dtau:.6e} ir_steps={list(steps)}")
        return ok, dtau

    # residuals_update!(residuals, variables, data) (residuals.jl:1-37) from the resident P, A
    def set_problem_vectors(self, q, b):
        self.h.set_qb(q, b)
        self._has_qb = True

    def residuals_update(self, r, v):
        """fills the residual object `r` (rx, rz, rx_inf, rz_inf, Px, rtau, dot_*) from the variables `v` (x, z, s, tau, kappa)"""
        r.dot_qx, r.dot_bz, r.dot_sz, r.dot_xPx, r.rtau = self.h.residuals(v.x, v.z, v.s, v.tau, v.kappa, r.rx, r.rz, r.rx_inf,
                                                                          r.rz_inf, r.Px)

    # ---- the interior-point step on the device (include/hipkkt.h hipkkt_cone_* / hipkkt_step_*) -------------------------------------
    # What the caller's loop does between the calls above, on an iterate [x | z | s] and a residual buffer [rx | rz | rx_inf | rz_inf | Px]
    # that stay in device memory (device_buffer); only scalars cross PCIe.  Zero / Nonnegative / SecondOrder cone sets.
    @property
    def steps_on_device(self) -> bool:
        return self._steps_on_device

    def device_buffer(self, n):
        return hipkkt.DeviceBuffer(n)

    def set_equilibration(self, d, e):
        self.h.set_equilibration(d, e)

    # the granular operations on the scaling the last kktsolver_update_scaled[_dev] left resident (vectors of length m, cone order)
    def cone_affine_ds(self):
        return self.h.cone_affine_ds()

    def cone_combined_ds_shift(self, step_z, step_s, sigma_mu):
        return self.h.cone_combined_ds_shift(step_z, step_s, sigma_mu)

    def cone_ds_from_dz_offset(self, ds):
        return self.h.cone_ds_from_dz_offset(ds)

    def cone_mul_hs(self, x):
        return self.h.cone_mul_hs(x)

    def cone_step_length(self, dz, ds, alpha_max):
        return self.h.cone_step_length(dz, ds, alpha_max)

    def residuals_update_dev(self, xzs, res, tau, kappa):
        """residuals_update! from the resident iterate into the resident buffer -> (dot_qx, dot_bz, dot_sz, dot_xPx, r_tau)"""
        return self.h.residuals_dev(xzs.ptr, tau, kappa, res.ptr)

    def kktsolver_info_norms(self, xzs, res):
        """the eight scaled 2-norms of info_update! (info.jl:1-60): |d x|, |e z|, |einv s|, |dinv rx|, |einv rz|, |dinv rx_inf|,
        |einv rz_inf|, |dinv Px|"""
        return self.h.step_info_norms_dev(xzs.ptr, res.ptr)

    def _psd_factors(self):
        """(Rinv, lambda) of the PSD cones' current scaling, concatenated like psd_R"""
        return (np.concatenate([c.Rinv.ravel(order="F") for c in self._psd_cones]), np.concatenate([c.lam for c in self._psd_cones]))

    def _psd_factors_upload(self):
        """[R | Rinv | lambda] of the PSD cones' current scaling in one upload, (Rinv, lambda) staged for the next scaling call -> the
        device pointer of R"""
        if self._psd_dev is None:
            self._psd_dev = hipkkt.DeviceBuffer(2 * self._psd_nr + int(np.sum(self._psd_dim)))
        rinv, lam = self._psd_factors()
        self._psd_dev.upload(np.concatenate([np.concatenate([c.R.ravel(order="F") for c in self._psd_cones]), rinv, lam]))
        p = self._psd_dev.ptr
        self.h.psd_set_factors(p + 8 * self._psd_nr, p + 16 * self._psd_nr, dev=True)
        return p

    def psd_rows_download(self, xzs):
        """-> (s, z) of length m with the rows first PSD row .. last PSD row filled from the resident iterate (steps_psd: what the
        caller's update_scaling! of the PSD cones needs), the rest zero"""
        lo, hi = self._psd_span
        s, z = np.zeros(self.m), np.zeros(self.m)
        z[lo:hi] = xzs.download_range(self.n + lo, hi - lo)
        s[lo:hi] = xzs.download_range(self.n + self.m + lo, hi - lo)
        return s, z

    def kktsolver_update_scaling_dev(self, xzs) -> bool:
        """update_scaling! + get_Hs! from the resident (s, z); False = a cone's s or z is not interior.
        steps_psd: the PSD cones' (R, Rinv, lambda) of the caller's update_scaling! go along in one upload -- unless scales_psd, where
        the device computes them from the resident (s, z) and nothing is uploaded"""
        if self.steps_psd and not self.scales_psd:
            p = self._psd_factors_upload()
            return self.h.update_scaling_dev(xzs.ptr + 8 * (self.n + self.m), xzs.ptr + 8 * self.n, R_ptr=p)
        return self.h.update_scaling_dev(xzs.ptr + 8 * (self.n + self.m), xzs.ptr + 8 * self.n)

    def kktsolver_update_scaling_dev_ex(self, xzs, mu, strategy) -> bool:
        """the same with Exponential / Power members: mu and the strategy ("primal_dual" / "dual" or 0 / 1) as kktsolver_update_scaled.
        steps_psd (a mixed set): the PSD cones' (R, Rinv, lambda) go along as in kktsolver_update_scaling_dev, unless scales_psd"""
        strategy = {"primal_dual": 0, "dual": 1}.get(strategy, strategy)
        if self.steps_psd and not self.scales_psd:
            p = self._psd_factors_upload()
            return self.h.update_scaling_ex_dev(xzs.ptr + 8 * (self.n + self.m), xzs.ptr + 8 * self.n, mu, strategy, R_ptr=p)
        return self.h.update_scaling_ex_dev(xzs.ptr + 8 * (self.n + self.m), xzs.ptr + 8 * self.n, mu, strategy)

    def cone_barrier(self, dz, ds, alphas):
        """(barrier, dot) per candidate step length: the cones' compute_barrier and <z + a dz, s + a ds> on the resident (s, z)"""
        return self.h.cone_barrier(dz, ds, alphas)

    def kktsolver_step_barrier(self, xzs, alphas):
        """the same on the resident iterate and the resident step of the last fused call (at most 8 candidates per call)"""
        return self.h.step_barrier_dev(xzs.ptr, alphas)

    def kktsolver_refactor(self) -> bool:
        return self._refactor()

    def _ir(self):
        st = self.settings
        return dict(ir_enable=st.iterative_refinement_enable, reltol=st.iterative_refinement_reltol, abstol=st.iterative_refinement_abstol,
                    max_iter=st.iterative_refinement_max_iter, stop_ratio=st.iterative_refinement_stop_ratio)

    def _step_done(self, ok, scal, steps, const_pending):
        self.last_ir_steps = int(steps[0])
        self.total_ir_steps += int(steps[0]) + (int(steps[1]) if const_pending else 0)
        self.nsolves += 2 if const_pending else 1
        self.last_step_scalars = scal
        return ok, float(scal[0]), float(scal[1]), float(scal[2])

    def kktsolver_step_affine(self, xzs, res, tau, kappa, r_tau, const_pending):
        """variables_affine_step_rhs! + kkt_solve!(:affine) + the affine step length -> (ok, alpha, dtau, dkappa); the step stays resident"""
        ok, scal, steps = self.h.step_affine_dev(xzs.ptr, res.ptr, tau, kappa, r_tau, const_pending, **self._ir())
        return self._step_done(ok, scal, steps, const_pending)

    def kktsolver_step_combined(self, xzs, res, tau, kappa, r_tau, dtau_aff, dkappa_aff, sigma, mu, m_corr):
        """variables_combined_step_rhs! + kkt_solve!(:combined) + the step length times max_step_fraction -> (ok, alpha, dtau, dkappa)"""
        ok, scal, steps = self.h.step_combined_dev(xzs.ptr, res.ptr, tau, kappa, r_tau, dtau_aff, dkappa_aff, sigma, mu, m_corr,
                                                   self.settings.max_step_fraction, False, **self._ir())
        return self._step_done(ok, scal, steps, False)

    @property
    def default_start_on_device(self) -> bool:
        """the default start of the cone set (solver.jl:383-405) can run on the resident iterate: kktsolver_default_start"""
        return self._steps_on_device and not self.steps_nonsymmetric and (not self.steps_psd_large or self.starts_psd_large)

    def kktsolver_default_start(self, xzs):
        """set_identity_scaling! + kkt_update! + kkt_solve_initial_point! + variables_symmetric_initialization! into the resident
        [x | z | s] -> (ok, scal[8] = eps_used, regularised pivots, (min_margin, pos_margin, target) of s and of z); tau = kappa = 1
        are the caller's.  Needs set_problem_vectors(q, b)."""
        st = self.settings
        ok, scal, steps = self.h.step_default_start_dev(xzs.ptr, st.static_regularization_enable, st.static_regularization_constant,
                                                        st.static_regularization_proportional, **self._ir())
        self.diagonal_regularizer = float(scal[0])
        self.last_nreg = int(scal[1])
        self.last_ir_steps = int(steps[0])
        self.total_ir_steps += int(np.sum(steps))
        self.nsolves += 1 if self.p_nnz else 2
        self.last_start_scalars = scal
        if _DEBUG:
            print(f"[hipkkt] default_start ok={ok} eps={scal[0]:.3e} dynamic_regularisations={int(scal[1])} ir_steps={list(steps)}")
        return ok, scal

    def kktsolver_step_apply(self, alpha, xzs):
        """[x | z | s] += alpha [dx | dz | ds] in place (not synchronised: the next call on the handle reads the result)"""
        self.h.step_apply_dev(alpha, xzs.ptr)

    # ref: kktsolver_update_P!/A!, :374-386
    def kktsolver_update_P(self, P):
        self.h.update_P(P.data)

    def kktsolver_update_A(self, A):
        self.h.update_A(A.data)

    # ref: kktsolver_linear_solver_info -> LinearSolverInfo(name,threads,direct,nnzA,nnzL), types.jl:198-206
    def kktsolver_linear_solver_info(self):
        return dict(name="hip", threads=1, direct=True, nnzA=self.h.nnzK, nnzL=self.h.nnzL)
