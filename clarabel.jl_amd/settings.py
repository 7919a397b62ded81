"""Settings mirror of the reference's ``Settings{T}`` (src/settings.jl:70-148).

Only the fields the KKT path and the stand-in IPM caller read are kept; defaults are the
struct defaults of the reference (the docstring table at settings.jl:44-57 is stale)."""
from dataclasses import dataclass, field

import numpy as np

_EPS = float(np.finfo(np.float64).eps)


@dataclass
class Settings:
    max_iter: int = 200                         # settings.jl:72
    time_limit: float = float("inf")
    verbose: bool = False
    max_step_fraction: float = 0.99             # :75
    tol_gap_abs: float = 1e-8                   # :78-83
    tol_gap_rel: float = 1e-8
    tol_feas: float = 1e-8
    tol_infeas_abs: float = 1e-8
    tol_infeas_rel: float = 1e-8
    tol_ktratio: float = 1e-6
    reduced_tol_gap_abs: float = 5e-5           # :90-95
    reduced_tol_gap_rel: float = 5e-5
    reduced_tol_feas: float = 1e-4
    reduced_tol_infeas_abs: float = 5e-12
    reduced_tol_infeas_rel: float = 5e-5
    reduced_tol_ktratio: float = 1e-4
    equilibrate_enable: bool = True             # :98-101
    equilibrate_max_iter: int = 10
    equilibrate_min_scaling: float = 1e-4
    equilibrate_max_scaling: float = 1e4
    linesearch_backtrack_step: float = 0.8      # :104-106 (line search of the non-symmetric cones)
    min_switch_step_length: float = 1e-1
    min_terminate_step_length: float = 1e-4
    max_threads: int = 0                        # :110
    direct_solve_method: str = "hip"            # :114 (reference default :auto)
    static_regularization_enable: bool = True   # :117-119
    static_regularization_constant: float = 1e-8
    static_regularization_proportional: float = _EPS * _EPS
    dynamic_regularization_enable: bool = True  # :122-124 (never read by the reference either)
    dynamic_regularization_eps: float = 1e-13
    dynamic_regularization_delta: float = 2e-7
    iterative_refinement_enable: bool = True    # :127-132
    iterative_refinement_reltol: float = 1e-13
    iterative_refinement_abstol: float = 1e-12
    iterative_refinement_max_iter: int = 10
    iterative_refinement_stop_ratio: float = 5.0
    presolve_enable: bool = True                # :135
    chordal_decomposition_enable: bool = False  # :139 (out of scope here; configs run with it off)
    # device selection for the :hip KKT solver (not in the reference)
    device_id: int = 0
    # SURVEY section 8(f) rows widened beyond the reference's plugin seam (all off by default = the reference's call pattern)
    device_residuals: bool = False            # N4: residuals_update! computed by the plugin from the resident P, A
    device_scaling: bool = False              # N1: update_scaling! / get_Hs! of the symmetric cones formed by the plugin from (s, z)
    device_reduced: bool = False              # N2: the reduced-system algebra of kkt_solve! (d tau dots, quad_form, dx, dz) done by the plugin
    # the cone algebra between those calls (affine_ds!, combined_ds_shift!, mul_Hs!, step length, add_step!, the norms of info_update!) done
    # by the plugin on a device-resident iterate, for Zero / Nonnegative / SecondOrder cone sets (any other cone set takes the host path).
    # Needs device_scaling, device_reduced and device_residuals: the caller raises ValueError when one of them is off.
    device_step: bool = False
    # device_step for cone sets that also hold Exponential / Power cones (backtracking line search, third-order correction and the
    # barrier of the Dual strategy on the device); Generalized Power (without device_step_genpower) and PSD cone sets keep the host path.  Needs device_step: the
    # caller raises ValueError otherwise.
    device_step_nonsymmetric: bool = False
    # device_step_nonsymmetric for cone sets that also hold Generalized Power cones (hipkkt_step_enable_genpow: feasibility backtracking
    # and the barrier with its Newton iteration for the primal gradient, one wavefront per cone); PSD cone sets keep the host path.
    # Needs device_step_nonsymmetric: the caller raises ValueError otherwise.
    device_step_genpower: bool = False
    # device_step for symmetric cone sets that also hold PSD triangle cones of side <= 64 (hipkkt_step_enable_psd: the triple products
    # and the step length's smallest eigenvalue on the device, one workgroup per cone).  The Cholesky / SVD of the cones' scaling stay
    # on the host: every iteration downloads the PSD rows of (s, z) and uploads (R, Rinv, lambda).  Needs device_step: the caller
    # raises ValueError otherwise.
    device_step_psd: bool = False
    # device_step_psd with the Cholesky / SVD of the PSD cones' scaling on the device as well (hipkkt_psd_scaling_enable: one workgroup
    # per cone, one-sided Jacobi sweeps in LDS): no download of (s, z) rows and no upload of factors, an iteration moves scalars only.
    # Needs device_step_psd: the caller raises ValueError otherwise.
    device_scaling_psd: bool = False
    # device_step with the default start (solver.jl:383-405) on the device as well (hipkkt_step_default_start_dev: the identity scaling
    # written into the resident K, the first factorisation, the initial-point solves and the shifts into the cones), for symmetric cone
    # sets the device step serves: no Hs upload, no host eigenvalues, no upload of the start.  Non-symmetric sets keep their host unit
    # initialisation.  Needs device_step: the caller raises ValueError otherwise.
    device_default_start: bool = False
    # device_step_psd for PSD triangle cones of side 65 .. 128 as well (hipkkt_step_enable_psd_large: the same arithmetic with the
    # matrices in device memory, products as batched tile launches).  For a set with such a side the Cholesky / SVD of the scaling and
    # the default start stay on the host, whatever device_scaling_psd / device_default_start say, unless the two flags below are set;
    # sides above 128 keep the host loop.  Needs device_step_psd: the caller raises ValueError otherwise.
    device_step_psd_large: bool = False
    # device_scaling_psd for a set with a PSD side of 65 .. 128 (hipkkt_psd_scaling_enable_large: the same Cholesky / one-sided Jacobi
    # iteration with one matrix in LDS and the others in device memory): no download of (s, z) rows and no upload of factors for
    # such a set either.  Needs device_scaling_psd and device_step_psd_large: the caller raises ValueError otherwise.
    device_scaling_psd_large: bool = False
    # device_default_start for a set with a PSD side of 65 .. 128 (hipkkt_step_default_start_enable_psd_large): no Hs upload and no
    # host eigenvalues for such a set either.  Needs device_default_start and device_step_psd_large: the caller raises ValueError
    # otherwise.
    device_default_start_psd_large: bool = False
    # device_step for cone sets that hold PSD triangle cones of side <= 64 next to Exponential / Power cones -- and next to Generalized
    # Power cones when device_step_genpower is set -- (hipkkt_step_enable_mixed: each family's kernels composed, plus the log-det
    # barrier of the PSD cones for the Dual strategy's search).  The PSD factors follow device_scaling_psd as in a symmetric set; the
    # unit initialisation stays on the host.  A PSD side above 64 in such a set keeps the host loop.  Needs device_step_nonsymmetric
    # and device_step_psd: the caller raises ValueError otherwise.
    device_step_mixed: bool = False
    # device_step_mixed for a set with a PSD side of 65 .. 128 as well (hipkkt_step_enable_mixed_large: the larger cones' rows and step
    # length through the kernels of device_step_psd_large, their log-det barrier with one 128 x 129 matrix in LDS).  The PSD factors
    # follow device_scaling_psd + device_scaling_psd_large; the unit initialisation stays on the host; sides above 128 keep the host
    # loop.  Needs device_step_mixed and device_step_psd_large: the caller raises ValueError otherwise.
    device_step_mixed_large: bool = False
    extra: dict = field(default_factory=dict)
