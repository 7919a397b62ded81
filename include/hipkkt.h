/*
 * libclarabel_hipkkt.so — C ABI of the MI355X-native KKT linear-system path for Clarabel.jl.
 *
 * This is the drop-in boundary.  Every entry point replaces one
 * method of the reference's KKT-solver plugin contracts; the `ref:` tag on each declaration cites
 * the reference interface it stands in for (paths relative to /root/reference):
 *
 *   seam L1  AbstractKKTSolver        src/kktsolvers/kktsolver_defaults.jl:2-47
 *            (concrete reference impl src/kktsolvers/kktsolver_directldl.jl)
 *   seam L0  AbstractDirectLDLSolver  src/kktsolvers/direct-ldl/directldl_defaults.jl:1-72
 *            (concrete reference impls directldl_qdldl.jl, ext/directldl_pardiso.jl)
 *
 * Conventions
 *   - plain C types only; all pointers are HOST memory unless the name ends in `_dev`
 *     (device pointers on the handle's GPU, e.g. a torch tensor's data_ptr()).
 *   - integer arrays are int64_t holding indices of base `opts.index_base` (1 = exactly what Julia
 *     holds in SparseMatrixCSC.colptr/rowval and LDLDataMap; 0 = numpy/scipy).
 *   - the caller owns every array it passes; the library copies during the call and keeps no host
 *     pointers (Julia's GC may move or free them after ccall returns).
 *   - return value int32_t: 0 = ok; >0 = numerical failure (maps to Julia `false`);
 *     <0 = usage / device error (maps to `error()` in a constructor, `false` elsewhere).
 *     Nothing is thrown across the boundary.
 *   - every call is synchronous (returns after the handle's stream has drained), sets the device
 *     of the handle, and touches no global mutable state: distinct handles may be driven from
 *     distinct threads / processes.  Only Float64 is accelerated.
 */
#ifndef HIPKKT_H
#define HIPKKT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hipkkt_solver *hipkkt_handle;

/* status codes */
#define HIPKKT_OK 0
#define HIPKKT_NUMERICAL_FAILURE 1   /* non-finite pivot / non-finite refinement residual */
#define HIPKKT_ERR_ARGUMENT (-1)
#define HIPKKT_ERR_DEVICE (-2)
#define HIPKKT_ERR_ALLOC (-3)
#define HIPKKT_ERR_INTERNAL (-4)

/* cone structure codes for hipkkt_create_from_parts (what the KKT pattern needs to know) */
#define HIPKKT_SPARSE_NONE 0
#define HIPKKT_SPARSE_SOC 1      /* SOCExpansionMap,    directldl_datamaps.jl:8-22  (pdim 2) */
#define HIPKKT_SPARSE_GENPOW 2   /* GenPowExpansionMap, directldl_datamaps.jl:81-99 (pdim 3) */

typedef struct hipkkt_opts {
    int32_t index_base;            /* 0 or 1 */
    int32_t supernode_max_width;   /* 0 = default (64) */
    int32_t relax_supernodes;      /* 1 = relaxed amalgamation (default), 0 = fundamental only */
    int32_t update_policy;         /* 0 = right-looking, 1 = left-looking, 2 = batched right-looking (default) */
    int32_t update_batch;          /* policy 2: #levels whose updates are applied together (0 = automatic: 4, or 5
                                      when a front of >= 64 panels dominates the factorisation) */
    int32_t front_min_panels;      /* chains of >= this many panels of one wide supernode are solved by the
                                      persistent front kernels; 0 = default (4), < 0 = never */
    double dynamic_reg_eps;        /* ref: settings.jl:123, passed at directldl_qdldl.jl:21 */
    double dynamic_reg_delta;      /* ref: settings.jl:124, passed at directldl_qdldl.jl:22 */
    double amd_dense_scale;        /* ref: directldl_qdldl.jl:24 (1.5); <=0 = default */
    const int64_t *user_perm;      /* optional fill-reducing order (index_base based); NULL = own AMD */
} hipkkt_opts;

/* defaults = the reference's Settings defaults (src/settings.jl:117-132) */
void hipkkt_default_opts(hipkkt_opts *opts);

/* ref: ldlsolver_is_available(::Val{:hip}) (pattern: ext/directldl_pardiso.jl:144,148).
 * Number of usable HIP devices (0 = not available).  Never fails. */
int32_t hipkkt_is_available(void);
/* Version of THIS interface.  A binding compares it with the HIPKKT_ABI_VERSION it was written against when it loads the library
 * and refuses a mismatch (the Julia glue and the ctypes mirror do): signatures may change between versions, never within one.
 * 4: hipkkt_get_profile / hipkkt_get_counters take the capacity of the caller's buffer (they wrote a fixed, growing number of values).
 * 5: hipkkt_set_cone_types_ex / hipkkt_get_nonsym_len / hipkkt_update_scaling_ex[_dev] (the bindings bind them when they load).
 *    Added within 5, no signature changed: the step entry points hipkkt_cone_* / hipkkt_set_equilibration / hipkkt_step_*;
 *    hipkkt_step_enable_cone3 / hipkkt_cone_barrier / hipkkt_step_barrier_dev; hipkkt_step_enable_genpow;
 *    HIPKKT_PSD_STEP_MAX_DIM / hipkkt_step_enable_psd / hipkkt_psd_set_factors / hipkkt_psd_set_factors_dev;
 *    hipkkt_psd_scaling_enable / hipkkt_psd_get_factors;
 *    hipkkt_cone_set_identity_scaling / hipkkt_cone_margins / hipkkt_cone_shift_to_interior / hipkkt_step_default_start_dev;
 *    HIPKKT_PSD_STEP_LARGE_MAX_DIM / hipkkt_step_enable_psd_large;
 *    hipkkt_step_enable_mixed;
 *    hipkkt_psd_scaling_enable_large / hipkkt_step_default_start_enable_psd_large;
 *    hipkkt_step_enable_mixed_large. */
#define HIPKKT_ABI_VERSION 5
int32_t hipkkt_abi_version(void);
/* releases the process-wide cache of device memory blocks the library keeps between handles (not in the reference: an embedding
 * host under memory pressure may call it at any time; live handles are unaffected) */
int32_t hipkkt_trim_cache(int32_t device_id);

/* ---- construction ------------------------------------------------------------------------ */

/* seam L0.  ref: ctor S{T}(KKT::SparseMatrixCSC{T},Dsigns,settings), directldl_qdldl.jl:6-28 /
 * ext/directldl_pardiso.jl:33-55.  KKT is the N x N :triu CSC image (diagonal present and LAST in
 * every column, as directldl_kkt_assembly.jl:161-165 guarantees).  Symbolic analysis only. */
int32_t hipkkt_create(int32_t device_id, int64_t N, const int64_t *colptr, const int64_t *rowval,
                      const double *nzval, const int64_t *dsigns, const hipkkt_opts *opts,
                      hipkkt_handle *out);

/* seam L1.  ref: DirectLDLKKTSolver{T}(P,A,cones,m,n,settings), kktsolver_directldl.jl:46-92:
 * assembles the :triu KKT image + LDLDataMap (directldl_kkt_assembly.jl:15-175,
 * directldl_datamaps.jl:170-214), Dsigns (kktsolver_directldl.jl:112-126), then the symbolic
 * analysis.  P is n x n :triu CSC, A is m x n CSC.  Per cone: numel, hs_dense (0 = diagonal Hs
 * block, 1 = dense packed-triu block), sparse_kind (HIPKKT_SPARSE_*), dim1 (GenPow only). */
int32_t hipkkt_create_from_parts(int32_t device_id, int64_t n, int64_t m,
                                 const int64_t *Pcolptr, const int64_t *Prowval, const double *Pnzval,
                                 const int64_t *Acolptr, const int64_t *Arowval, const double *Anzval,
                                 int64_t ncones, const int64_t *cone_numel, const int32_t *cone_hs_dense,
                                 const int32_t *cone_sparse_kind, const int64_t *cone_dim1,
                                 const hipkkt_opts *opts, hipkkt_handle *out);

/* ref: finalizer of the Julia wrapper struct (MOI.empty! calls finalize(solver),
 * src/MOI_wrapper/MOI_wrapper.jl:133).  Idempotent on NULL. */
void hipkkt_destroy(hipkkt_handle h);

/* ---- introspection ------------------------------------------------------------------------ */

/* out[0..15] = N, n, m, p, nnzK, nHs, nsparse, nnzP, nnzA, nnzL (strictly-lower entries of L,
 * structural), n_supernodes, n_levels, panel_doubles (supernodal storage incl. padding zeros),
 * n_update_tasks, etree_height (columns), ordering in use (0 minimum degree on K, 1 cone rows first /
 * variables last, 2 user, 3 nested dissection).  (n,m,p,nHs,nnzP,nnzA are 0 for L0 handles.) */
int32_t hipkkt_get_dims(hipkkt_handle h, int64_t *out16);

/* ref: linear_solver_info(ldlsolver) -> LinearSolverInfo(name,threads,direct,nnzA,nnzL),
 * directldl_qdldl.jl:35-42 / src/types.jl:198-206.  name = :hip, threads = 1 (host), direct = true. */
int32_t hipkkt_info(hipkkt_handle h, int64_t *nnzA, int64_t *nnzL);

/* flop / byte model of one numeric factorisation and one solve, from the symbolic factor actually
 * used:  out[0]=sum_j c_j^2+3c_j (factor flops), out[1]=executed factor flops incl.
 * supernode padding, out[2]=solve flops (4 nnzL + N), out[3]=algorithmic factor bytes,
 * out[4]=algorithmic solve bytes, out[5]=spmv bytes, out[6]=dense-update (MFMA) flops, out[7]=the part of out[6] executed by k_update_dense */
int32_t hipkkt_get_cost_model(hipkkt_handle h, double *out8);

/* copies of host-side structures (tests, Julia-side bookkeeping).  Any pointer may be NULL. */
int32_t hipkkt_get_kkt(hipkkt_handle h, int64_t *colptr, int64_t *rowval, double *nzval);
/* perm[k] = index eliminated k-th, of the factorisation IN USE: while the last factorisation lives in the robust-order twin
 * (hipkkt_get_counters out[4]) that is the twin's minimum-degree order, otherwise the handle's own */
int32_t hipkkt_get_perm(hipkkt_handle h, int64_t *perm);
int32_t hipkkt_get_dsigns(hipkkt_handle h, int64_t *dsigns);
/* which: 0 = map.P, 1 = map.A, 2 = map.Hsblocks, 3 = map.diagP, 4 = map.diag_full
 * (ref: LDLDataMap fields, directldl_datamaps.jl:170-181) */
int32_t hipkkt_get_map(hipkkt_handle h, int32_t which, int64_t *out);
/* sparse map i: which 0/1/2 = index vectors (SOC: u,v ; GenPow: q,r,p), 3 = D; *len receives length */
int32_t hipkkt_get_sparse_map(hipkkt_handle h, int64_t i, int32_t which, int64_t *out, int64_t *len);

/* ---- value updates ------------------------------------------------------------------------ */

/* ref: update_values!(ldlsolver,index,values) / scale_values!(ldlsolver,index,scale),
 * directldl_qdldl.jl:46-69, called from kktsolver_directldl.jl:130-188. */
int32_t hipkkt_update_values(hipkkt_handle h, const int64_t *index, const double *values, int64_t k);
int32_t hipkkt_scale_values(hipkkt_handle h, const int64_t *index, int64_t k, double scale);

/* ref: kktsolver_update! first half, kktsolver_directldl.jl:223-228: Hs as produced by
 * get_Hs!(cones,Hsblocks); negated and scattered through map.Hsblocks on the device. */
int32_t hipkkt_set_hs(hipkkt_handle h, const double *hs, int64_t nHs);
/* the _dev form does not synchronise with the host: hs_dev must stay valid until the next synchronising call on this handle
 * (hipkkt_refactor, any solve) has returned */
int32_t hipkkt_set_hs_dev(hipkkt_handle h, const double *hs_dev, int64_t nHs);

/* SURVEY section 8(f) row N1 (first step): the Hs block of PSD triangle cones formed ON THE DEVICE.
 * ref: get_Hs!(::PSDTriangleCone) = pack_triu(skron(R R^T)), coneops_psdtrianglecone.jl:153-161, 502-540.
 * For cone c (c = 0..npsd-1): dim[c] = matrix side n, w_all holds its dense symmetric W = R R^T (n x n, row-major,
 * cones concatenated), hs_off[c] = 0-based offset of the cone's block inside the Hs vector (as used by
 * hipkkt_set_hs).  The packed upper triangle of  W (x)_s W  (numel(numel+1)/2 values, numel = n(n+1)/2) is computed,
 * negated and scattered through map.Hsblocks like hipkkt_set_hs does -- with the same products, sums and rounding
 * as the reference's skron! loop, so K is bit-identical to the host path.  Saves the O(numel^2) host loop and the
 * upload of the block (813 450 doubles per 50 x 50 cone). */
int32_t hipkkt_set_hs_psd(hipkkt_handle h, int64_t npsd, const int64_t *hs_off, const int64_t *dim, const double *w_all);

/* SURVEY section 8(f) row N1 (completion): update_scaling! + get_Hs! of the symmetric cones ON THE DEVICE -- the caller ships the
 * iterate (s, z) (2 m doubles) instead of the Hs vector and the (u, v, eta) of every second-order cone.
 *   hipkkt_set_cone_types   once per handle: kinds[c] = 0 ZeroCone, 1 NonnegativeCone, 2 SecondOrderCone, 3 PSDTriangleCone
 *                           (cone_types.jl:6-67), anything else = a cone the caller keeps updating with hipkkt_set_hs / _set_genpow.
 *                           Checked against the (numel, hs_dense, sparse_kind) the handle was created with.
 *   hipkkt_update_scaling   per IPM iteration, replaces update_scaling!(cones,s,z,mu,PrimalDual) + get_Hs! + the Hs / sparse-cone
 *                           part of _kktsolver_update_inner! (kktsolver_directldl.jl:197-245):
 *      Zero          Hs = 0                                                      coneops_zerocone.jl:91
 *      Nonnegative   lambda = sqrt(s z), w = sqrt(s/z), Hs = w^2 (bit-exact)     coneops_nncone.jl:77-101
 *      SecondOrder   eta, w, lambda, and (d, u, v) of the sparse form or the dense block for dim <= 4, with the reference's
 *                    expressions and association (sums of squares are tree sums)  coneops_socone.jl:75-192
 *      PSDTriangle   psd_R = the cones' R factors (n x n, column-major, concatenated; the Cholesky / SVD of
 *                    coneops_psdtrianglecone.jl:78-143 stay with the caller): W = R R^T and triu(skron(W)) are formed on the
 *                    device (:145-161, :502-540).  psd_R = NULL leaves the PSD blocks to hipkkt_set_hs_psd.
 *    Outputs (any may be NULL): w_out, lambda_out of length m in cone order (NN: w, lambda; SOC: the normalised w and lambda; zero
 *    on other rows) -- what the host loop needs for mul_Hs! / step directions; soc_eta_out[k] = eta of the k-th second-order cone;
 *    *scaling_ok = 0 when a second-order cone's s or z is not interior (update_scaling! returns false, coneops_socone.jl:88-90).
 *    The resident KKT values, w_out, lambda_out and soc_eta_out are then UNSPECIFIED (the other cones have been rewritten, the
 *    failing cone partly): like the reference, which never reaches get_Hs! in that case, the caller must not factor or read them
 *    before a later call has succeeded.
 *   hipkkt_update_scaling_dev  the same with every pointer except scaling_ok in device memory (s, z resident: no PCIe at all). */
int32_t hipkkt_set_cone_types(hipkkt_handle h, int64_t ncones, const int32_t *kinds);
int32_t hipkkt_update_scaling(hipkkt_handle h, const double *s, const double *z, const double *psd_R, double *w_out,
                              double *lambda_out, double *soc_eta_out, int32_t *scaling_ok);
int32_t hipkkt_update_scaling_dev(hipkkt_handle h, const double *s_dev, const double *z_dev, const double *psd_R_dev,
                                  double *w_out_dev, double *lambda_out_dev, double *soc_eta_out_dev, int32_t *scaling_ok);

/* N1 for the NON-SYMMETRIC cones: update_scaling! + get_Hs! + _csc_update_sparsecone of Exponential, Power and Generalized Power cones
 * on the device, next to the symmetric ones.  The two calls above keep their behaviour: hipkkt_set_cone_types treats any kind outside
 * 0..3 as the caller's, hipkkt_update_scaling[_dev] never touches such a cone.
 *   three-row cones, one lane per cone: update_dual_grad_H(z) -> grad, H_dual (coneops_expcone.jl:370-400, coneops_powcone.jl:408-442);
 *     Dual: Hs = mu H_dual (coneops_nonsymmetric_common.jl:71-78); PrimalDual: gradient_primal(s) by Wright omega
 *     (coneops_expcone.jl:284-297, 412-467) resp. the one-sided Newton-Raphson iteration of at most 100 steps (coneops_powcone.jl:288-317,
 *     449-478, coneops_nonsymmetric_common.jl:170-192), then the BFGS form or, on the central path, Hs = (<s, z> / 3) H_dual
 *     (coneops_nonsymmetric_common.jl:82-164).  pack_triu(Hs) goes negated through map.Hsblocks like hipkkt_set_hs.
 *     A block whose 3 x 3 Cholesky (mathutils.jl:427-451) breaks down in rounding -- late iterates, condition numbers beyond 1e16 --
 *     gets the smallest shift 2^k eps max(diag), k = 1 .. 8, on its diagonal with which it goes through (K and the output vector hold
 *     the shifted block); every other block is exactly what the reference's expressions give.
 *   GenPower cones, one wavefront per cone: update_dual_grad_H(z) -> grad, d1, d2, p, q, r (coneops_genpowcone.jl:343-396); the block
 *     -mu d1, -mu d2 (:91-108), the q, r, p columns times -sqrt(mu) and the diagonals (-1, -1, +1) of the expansion
 *     (directldl_datamaps.jl:146-167) through index tables made resident by hipkkt_set_cone_types_ex: no upload and no host
 *     synchronisation per cone.  These cones always take Dual with the caller's mu (coneops_genpowcone.jl:21, 64-80).
 *   Failure: a cone whose z is not strictly inside the dual cone, whose s is not strictly inside the primal cone (PrimalDual), whose
 *     Wright-omega argument is negative or whose result is not finite gives *scaling_ok = 0 (the reference asserts / throws); its slot of
 *     the output vector is filled with NaN, its entries of K are not written; what hipkkt_update_scaling says about the state after
 *     *scaling_ok = 0 holds here too.  The return value stays HIPKKT_OK. */
#define HIPKKT_CONE_EXP 4      /* ExponentialCone,  cone_types.jl */
#define HIPKKT_CONE_POW 5      /* PowerCone(alpha): 1 entry of `alpha` */
#define HIPKKT_CONE_GENPOW 6   /* GenPowerCone(alpha, dim2): dim1 entries of `alpha` */
/* kinds 0..3 as hipkkt_set_cone_types; alpha = the exponents of the Power / GenPow cones concatenated in cone order.  Checked
 * against (numel, hs_dense, sparse_kind, dim1) of the handle: 4 / 5 = numel 3, dense block, no expansion; 6 = sparse_kind
 * HIPKKT_SPARSE_GENPOW, diagonal block, dim1 = its share of alpha, every alpha in (0, 1). */
int32_t hipkkt_set_cone_types_ex(hipkkt_handle h, int64_t ncones, const int32_t *kinds, int64_t nalpha, const double *alpha);
/* doubles in the non-symmetric output vector: 15 per three-row cone (Hs 6, H_dual 6, grad 3; the 3 x 3 matrices in pack_triu order),
 * 3 dim + dim1 + 1 per GenPow cone (grad dim, d1 dim1, d2 1, p dim, q dim1, r dim2), cones in cone order; 0 without such cones */
int32_t hipkkt_get_nonsym_len(hipkkt_handle h, int64_t *len);
/* hipkkt_update_scaling + the cones above.  strategy: 0 PrimalDual, 1 Dual (types.jl:73-76); GenPow cones always take Dual with
 * the caller's mu.  nonsym_out may be NULL.  On a handle without kinds 4..6 the resident K is bit-identical to hipkkt_update_scaling's.
 * hipkkt_update_scaling[_dev] on a handle whose last registration named a kind 4..6 returns HIPKKT_ERR_ARGUMENT (it has no mu). */
int32_t hipkkt_update_scaling_ex(hipkkt_handle h, const double *s, const double *z, const double *psd_R, double mu,
                                 int32_t strategy, double *w_out, double *lambda_out, double *soc_eta_out, double *nonsym_out,
                                 int32_t *scaling_ok);
/* the same with every pointer except scaling_ok in device memory */
int32_t hipkkt_update_scaling_ex_dev(hipkkt_handle h, const double *s_dev, const double *z_dev, const double *psd_R_dev, double mu,
                                     int32_t strategy, double *w_out_dev, double *lambda_out_dev, double *soc_eta_out_dev,
                                     double *nonsym_out_dev, int32_t *scaling_ok);
/* ref: _csc_update_sparsecone(::SecondOrderCone,...), directldl_datamaps.jl:61-79 */
int32_t hipkkt_set_soc(hipkkt_handle h, int64_t sparse_idx, double eta2, const double *u, const double *v,
                       int64_t dim);
/* all sparse SOC cones in one call (same arithmetic; one upload + one launch instead of 5 per cone):
 * eta2[nsoc], u_all / v_all = the cones' u and v vectors concatenated in sparse-map order */
int32_t hipkkt_set_soc_batch(hipkkt_handle h, int64_t nsoc, const double *eta2, const double *u_all,
                             const double *v_all, int64_t total);
/* ref: _csc_update_sparsecone(::GenPowerCone,...), directldl_datamaps.jl:146-167 */
int32_t hipkkt_set_genpow(hipkkt_handle h, int64_t sparse_idx, double sqrtmu, const double *p,
                          const double *q, const double *r);
/* ref: kktsolver_update_P!/A!, kktsolver_directldl.jl:374-386 */
int32_t hipkkt_update_P(hipkkt_handle h, const double *Pnzval, int64_t nnzP);
int32_t hipkkt_update_A(hipkkt_handle h, const double *Anzval, int64_t nnzA);

/* ---- factor ------------------------------------------------------------------------------- */

/* ref: _kktsolver_regularize_and_refactor!, kktsolver_directldl.jl:247-310 with
 * refactor!(ldlsolver,K), directldl_qdldl.jl:72-81.  eps = eps_const + eps_prop*max|diag K|;
 * K_fact = K + eps*diag(Dsigns); numeric LDL^T with the sign-driven dynamic pivot substitution;
 * the unregularised K stays resident for iterative refinement.  Returns 0, or
 * HIPKKT_NUMERICAL_FAILURE when some pivot inverse is non-finite.  eps_used / n_dynamic_reg may be NULL. */
int32_t hipkkt_refactor(hipkkt_handle h, int32_t static_reg_enable, double eps_const, double eps_prop,
                        double *eps_used, int64_t *n_dynamic_reg);

/* ---- solve -------------------------------------------------------------------------------- */

/* ref: kktsolver_setrhs!, kktsolver_directldl.jl:313-327: b = [rhsx; rhsz; 0_p] */
int32_t hipkkt_setrhs(hipkkt_handle h, const double *rhsx, const double *rhsz);
int32_t hipkkt_setrhs_dev(hipkkt_handle h, const double *rhs_dev /* n+m contiguous; not synchronised with the host: valid until the solve has returned */);
/* ref: kktsolver_solve!, kktsolver_directldl.jl:346-371 incl. _iterative_refinement :389-449 and
 * kktsolver_getlhs! :330-343.  lhsx / lhsz may be NULL (Julia `nothing`).  ir_steps may be NULL. */
int32_t hipkkt_solve(hipkkt_handle h, double *lhsx, double *lhsz, int32_t ir_enable, double reltol,
                     double abstol, int64_t max_iter, double stop_ratio, int64_t *ir_steps);
/* same, result left on the device: lhs_dev receives n+m doubles (may be NULL to discard) */
int32_t hipkkt_solve_dev(hipkkt_handle h, double *lhs_dev, int32_t ir_enable, double reltol,
                         double abstol, int64_t max_iter, double stop_ratio, int64_t *ir_steps);
/* SURVEY section 8(f) row N2.  nrhs right-hand sides on ONE factorisation, each refined exactly like hipkkt_solve does,
 * two at a time on concurrent solve contexts (the triangular sweeps are bound by dependency latency, so two of them
 * overlap almost completely).  The caller this serves: kkt_update! leaves the constant-rhs solve of kktsystem.jl:80-92
 * pending and the first kkt_solve! of the iteration (:135-215, affine step) solves [-q; b] and its own right-hand side
 * together.  rhsx = nrhs x n, rhsz = nrhs x m, lhsx / lhsz likewise (row-major, one right-hand side after the other;
 * lhs pointers may be NULL); ir_steps[nrhs] may be NULL.  Returns 0, or HIPKKT_NUMERICAL_FAILURE if any solve failed. */
int32_t hipkkt_solve_multi(hipkkt_handle h, int64_t nrhs, const double *rhsx, const double *rhsz, double *lhsx, double *lhsz,
                           int32_t ir_enable, double reltol, double abstol, int64_t max_iter, double stop_ratio,
                           int64_t *ir_steps);
/* same with everything resident: rhs_dev / lhs_dev = nrhs x (n+m) doubles on the device */
int32_t hipkkt_solve_multi_dev(hipkkt_handle h, int64_t nrhs, const double *rhs_dev, double *lhs_dev, int32_t ir_enable,
                               double reltol, double abstol, int64_t max_iter, double stop_ratio, int64_t *ir_steps);
/* SURVEY section 8(f) row N2, second half.  ref: kkt_solve!(kktsystem, lhs, rhs, data, variables, cones, steptype),
 * src/kktsystem.jl:135-215 -- everything between the caller's cone algebra (the vector c of  Hs dz + ds = -c, :152-163) and
 * mul_Hs! (:203): the solve  K [x1; z1] = [rhs.x; c - rhs.z]  (:167-170), the numerator and denominator of d tau with
 * quad_form(., P, .) (:176-190, mathutils.jl:299-337) from the q, b made resident by hipkkt_set_qb and the resident P values,
 * and  dx = x1 + dtau x2,  dz = z1 + dtau z2  (:194-196).  ONE PCIe round trip and one host synchronisation per kkt_solve!.
 *   rhs_x[n], workz[m] (= c - rhs.z), var_x[n] (= variables.x) in;  scal_in = {variables.tau, variables.kappa, rhs.tau, rhs.kappa}
 *   const_pending != 0: the constant-rhs solve of _kkt_solve_constant_rhs! (:80-92), K [x2; z2] = [-q; b], left pending by
 *     kkt_update!, runs here next to (x1, z1) on the second solve context and its solution becomes the resident (x2, z2);
 *     const_pending == 0: (x2, z2) of the last such call (same factorisation) is used
 *   lhs_x[n], lhs_z[m] out (host; either may be NULL);  scal_out[10] = {dtau, tau_num, tau_den, q.x1, b.z1, xi'P x1, q.x2, b.z2,
 *     (xi - x2)'P(xi - x2), x2'P x2} (host, required);  ir_steps[2] = refinement steps of the (x1, z1) / (x2, z2) solve (may be NULL)
 * The _dev form takes in_dev = [rhs_x | workz | var_x] (2n + m doubles) and writes lhs_dev = [dx | dz] (n + m doubles, may be NULL:
 * the step then stays in the handle and only the scalars cross PCIe).  Returns 0, HIPKKT_NUMERICAL_FAILURE when a solve failed
 * (the reference returns is_success = false), < 0 on usage / device errors (hipkkt_set_qb not called: HIPKKT_ERR_ARGUMENT).
 * ON ANY NON-ZERO RETURN lhs_x / lhs_z / lhs_dev / scal_out ARE UNSPECIFIED: the reduction and the copies of the step are enqueued
 * behind the solves before their outcome is known (that is what makes it one synchronisation), so they may hold a rejected or
 * non-finite iterate.  This differs from hipkkt_solve, which like kktsolver_getlhs! writes lhs only on success; the reference's
 * caller returns at once on is_success = false (kktsystem.jl:172) and never reads lhs. */
int32_t hipkkt_kkt_solve_reduced(hipkkt_handle h, const double *rhs_x, const double *workz, const double *var_x, const double *scal_in4,
                                 int32_t const_pending, double *lhs_x, double *lhs_z, double *scal_out10, int32_t ir_enable,
                                 double reltol, double abstol, int64_t max_iter, double stop_ratio, int64_t *ir_steps2);
int32_t hipkkt_kkt_solve_reduced_dev(hipkkt_handle h, const double *in_dev, const double *scal_in4, int32_t const_pending,
                                     double *lhs_dev, double *scal_out10, int32_t ir_enable, double reltol, double abstol,
                                     int64_t max_iter, double stop_ratio, int64_t *ir_steps2);
/* seam L0.  ref: solve!(ldlsolver,K,x,b), directldl_qdldl.jl:85-96: x = K_fact^{-1} b, length N,
 * no refinement (the Julia-side DirectLDLKKTSolver refines).  x and b must not alias. */
int32_t hipkkt_ldl_solve(hipkkt_handle h, double *x, const double *b);

/* SURVEY section 8(f) row N4 (building block): the sparse products of residuals_update!, residuals.jl:12-25, from the
 * P and A values resident on the device (L1 handles): Px = Symmetric(P) x, ATz = A' z, Ax = A x.
 * x[n], z[m] in; Px[n], ATz[n], Ax[m] out (host memory; any of the outputs may be NULL). */
int32_t hipkkt_block_products(hipkkt_handle h, const double *x, const double *z, double *Px, double *ATz, double *Ax);

/* residuals_update!(residuals, variables, data), residuals.jl:1-37, computed on the device from
 * the resident P and A values (L1 handles).  hipkkt_set_qb makes q[n] and b[m] resident (once per problem, again after
 * update_q!/update_b!).  hipkkt_residuals: x[n], z[m], s[m], tau, kappa in; rx[n], rz[m], rx_inf[n], rz_inf[m], Px[n] out
 * (host memory, any may be NULL); scal5 = {dot_qx, dot_bz, dot_sz, dot_xPx, r_tau} (host, required).  The dot products
 * are summed in a fixed order (deterministic).  The _dev form takes xzs_dev = [x | z | s] and writes
 * out_dev = [rx | rz | rx_inf | rz_inf | Px] (3n + 2m doubles) without touching PCIe except for the five scalars. */
int32_t hipkkt_set_qb(hipkkt_handle h, const double *q, const double *b);
int32_t hipkkt_residuals(hipkkt_handle h, const double *x, const double *z, const double *s, double tau, double kappa,
                         double *rx, double *rz, double *rx_inf, double *rz_inf, double *Px, double *scal5);
int32_t hipkkt_residuals_dev(hipkkt_handle h, const double *xzs_dev, double tau, double kappa, double *out_dev, double *scal5);

/* ---- the interior-point step on the device ------------------------------------------------ */

/* The cone algebra BETWEEN the calls above -- affine_ds!, combined_ds_shift!, Delta_s_from_Delta_z_offset!, mul_Hs!, the step length,
 * variables_add_step! and the norms of info_update! -- for cone sets of ZeroCone, NonnegativeCone and SecondOrderCone (kinds 0..2 of
 * hipkkt_set_cone_types[_ex]).  Every operation works on the (s, z, w, lambda, eta) that the last successful
 * hipkkt_update_scaling[_ex][_dev] left resident; expressions keep the reference's association (Zero / Nonnegative rows are the
 * host's bit for bit), a `dot` of the reference is a tree sum.  No input is modified.
 * All of them return HIPKKT_ERR_ARGUMENT on a handle whose registration names a PSD cone or a kind 4..6 (without the opt-ins below those
 * keep their step algebra with the caller: eigenvalue decompositions, backtracking line search, barriers) and before the first successful scaling; the fused
 * calls also before hipkkt_set_qb.  On any non-zero return the outputs are unspecified, as for hipkkt_kkt_solve_reduced.
 *
 * Opt-in for ExponentialCone / PowerCone (kinds 4, 5): after hipkkt_step_enable_cone3 on a registration of kinds {0, 1, 2, 4, 5} every
 * call of this section serves all rows of that handle, on the (s, z) and the per-cone [Hs | H_dual | grad] that the next successful
 * hipkkt_update_scaling_ex[_dev] leaves resident (a scaling from before the enable does not count).  On the rows of a kind 4 / 5 cone
 *   affine_ds = the resident s; ds_from_dz_offset = ds; mul_hs = the resident 3 x 3 Hs block times x (what the matrix holds);
 *   combined_ds_shift = grad sigma mu - higher_correction(step_s, step_z) (coneops_expcone.jl:319-367, coneops_powcone.jl:329-405;
 *     0 when the 3 x 3 Cholesky of H_dual breaks down, as in the reference);
 *   step length = the composite rule of coneops_compositecone.jl:216-252: the symmetric cones first, then from
 *     alpha0 = min(that, 1 - sqrt(eps)) every kind 4 / 5 cone backtracks alpha <- step alpha separately for z + alpha dz and s + alpha ds
 *     until the point is strictly feasible or alpha < alpha_min, which gives 0 (coneops_nonsymmetric_common.jl:5-33); the result is
 *     the minimum, returned in both slots.  All cones walk the grid alpha0 step^k, so the minimum is the reference's sequential result.
 *     In the fused calls alpha0 also takes min(alpha_tau, alpha_kappa, 1) first, formed on the device (variables.jl:14-43), and
 *     scal_out15[3..4] hold the composite (alpha, alpha) before max_step_fraction.
 * Rows of kinds 0..2 go through the same kernels as without the enable, bit for bit.  Every loop on the device is bounded: the
 * backtracking by ceil(log alpha_min / log step) + 2 trips (at most 4096, else the enable is refused), Newton iterations by the
 * reference's 100 steps; a direction that leaves a cone for every alpha gives alpha = 0, never a trap.
 * Kinds 3 (PSD) and 6 (GenPower) stay refused at hipkkt_step_enable_cone3; kind 6 has its own opt-in, next.
 *
 * Opt-in for GenPowerCone (kind 6): after hipkkt_step_enable_genpow on a registration of kinds {0, 1, 2, 4, 5, 6} with at least one 6
 * every call of this section serves all rows of that handle; the kind 4 / 5 members step as after hipkkt_step_enable_cone3 with the
 * same parameters.  A kind 6 cone works on the resident (s, z), its slot [grad | d1 | d2 | p | q | r] of the scaling's output vector and
 * the mu of that scaling (coneops_genpowcone.jl; the cone always takes the Dual scaling):
 *   affine_ds = the resident s; ds_from_dz_offset = ds; combined_ds_shift = grad sigma mu (no third-order correction, :149-168);
 *   mul_hs = mu (D x + (p.x) p - (q.x1) q - (r.x2) r) (:111-135), the three dots as tree sums;
 *   step length = the same backtracking on the same grid alpha0 step^k with is_dual_feasible / is_primal_feasible of :249-292; the
 *     composite step is the minimum over all kind 4 / 5 / 6 cones;
 *   barrier = barrier_dual + barrier_primal (:209-234, :294-333), the primal gradient from the one-sided Newton iteration of :393-472
 *     (at most 100 steps), one value per (cone, candidate) added to the cone set's barrier.
 * Sums and products over a cone are tree reductions; otherwise expressions keep the reference's association.  A registration without
 * kind 6 computes exactly what it computed before this call existed.  A PSD cone (kind 3) is refused here too.
 *
 * Opt-in for PSDTriangleCone (kind 3): after hipkkt_step_enable_psd on a registration of kinds {0, 1, 2, 3} with at least one 3 and every
 * PSD side <= HIPKKT_PSD_STEP_MAX_DIM, the five hipkkt_cone_* operations, the fused calls and hipkkt_step_get serve all rows of that
 * handle (the barrier calls keep refusing it: the set is symmetric).  The Cholesky / SVD of coneops_psdtrianglecone.jl:78-143 stay
 * with the caller, who hands over (R, Rinv, lambda) per scaling: hipkkt_psd_set_factors[_dev], then a hipkkt_update_scaling[_ex][_dev]
 * with psd_R.  With X = svec_to_mat of a cone's rows and results through mat_to_svec (:469-497):
 *   affine_ds = lambda_k^2 at the diagonal positions, 0 elsewhere (:190-205);
 *   mul_W :N  Y = R' X R, :T  Y = R X R', mul_Winv the same with Rinv (:409-437); mul_hs = W'(W x) (:164-187);
 *   combined_ds_shift: A = W step_z, B = W^-T step_s, svec((B A + A B) / 2) with sigma mu subtracted at the diagonal positions
 *     (coneops_symmetric_common.jl:1-35);
 *   ds_from_dz_offset: X~_ij = 2 DS_ij / (lambda_i + lambda_j), out = R X~ R' (coneops_symmetric_common.jl:39-52);
 *   step length: D = R' dZ R resp. Rinv dS Rinv', M = Lambda^-1/2 D Lambda^-1/2, gamma = lambda_min(M),
 *     alpha = gamma < 0 ? min(1 / -gamma, alpha_max) : alpha_max (:230-254, :439-466); alpha_z and alpha_s each take the minimum with
 *     the pair of the kind 0..2 rows.  gamma comes from a cyclic Jacobi iteration of at most 30 sweeps that stops at
 *     off(M) <= eps |M|_F; an M with a non-finite entry gives a NaN gamma and therefore alpha_max, as the reference's comparison does.
 * One workgroup per cone, matrices in LDS, every k-sum of a product in ascending order (deterministic; the association differs from
 * the host's BLAS, so results agree to rounding, not bit for bit).  Rows of kinds 0..2 go through the same kernels as without the
 * enable, bit for bit.  Kinds 4..6 next to a PSD cone stay refused here; they have their own opt-in, last in this list.
 *
 * Opt-in for PSDTriangleCone of side 65 .. HIPKKT_PSD_STEP_LARGE_MAX_DIM: hipkkt_step_enable_psd_large accepts what hipkkt_step_enable_psd
 * accepts with every PSD side <= HIPKKT_PSD_STEP_LARGE_MAX_DIM, and the same calls then serve all rows of the handle from the same
 * (R, Rinv, lambda) protocol.  A cone of side <= HIPKKT_PSD_STEP_MAX_DIM is computed by the kernels of the paragraph above, bit for
 * bit as after hipkkt_step_enable_psd.  A larger cone is computed with the same arithmetic in another placement: its matrices stay in
 * device memory (a workspace of four n x n matrices per such cone, allocated at the enable), every product is a batch of 16 x 16
 * output tiles over all such cones (and over z / s where an operation has both) whose operands -- a factor, its transpose,
 * svec_to_mat of the rows, the mat_to_svec / svec_to_mat round trip of an intermediate result -- are read from device memory through
 * LDS panels, and the Jacobi iteration runs with one workgroup per cone and side, M alone in LDS (128 x 129 doubles at side 128).
 * Every entry of every product is still one fused multiply-add chain over k in ascending order, the elementwise expressions, the pair
 * schedule, the rotation formulas, the sums of the stop rule and the bound of 30 sweeps are those of the smaller cones: the same
 * input gives the same bits whichever kernels compute a cone.  An operation is a few launches on the handle's stream instead of one;
 * the fused calls keep their single host synchronisation.  The Cholesky / SVD and the default start of such a handle stay with the
 * caller unless their own opt-ins follow: while the registration holds a side above HIPKKT_PSD_STEP_MAX_DIM, hipkkt_psd_scaling_enable
 * returns HIPKKT_ERR_ARGUMENT (its kernel keeps four matrices in LDS; hipkkt_psd_scaling_enable_large is the call for such a handle),
 * and hipkkt_cone_set_identity_scaling, hipkkt_cone_margins, hipkkt_cone_shift_to_interior and hipkkt_step_default_start_dev return
 * HIPKKT_ERR_ARGUMENT until hipkkt_step_default_start_enable_psd_large; with every side <= HIPKKT_PSD_STEP_MAX_DIM they behave as
 * after hipkkt_step_enable_psd.  Sides above HIPKKT_PSD_STEP_LARGE_MAX_DIM keep the host loop.
 *
 * Opt-in for PSDTriangleCone next to kinds 4..6: after hipkkt_step_enable_mixed on a registration (hipkkt_set_cone_types_ex) of kinds
 * {0, .., 6} with at least one 3, at least one of 4 / 5 / 6 and every PSD side <= HIPKKT_PSD_STEP_MAX_DIM, every call of this section
 * serves all rows of that handle.  Each family's rows go through the kernels of its own paragraph above: kinds 0..2 and 4..6 bit for
 * bit as on a handle without the PSD cones, the PSD rows bit for bit as after hipkkt_step_enable_psd, from the same (R, Rinv, lambda)
 * protocol (hipkkt_psd_set_factors[_dev] + psd_R per hipkkt_update_scaling_ex[_dev], or hipkkt_psd_scaling_enable).
 *   step length = the composite rule: the pair of the kind 0..2 rows and of the PSD cones first (the minimum of the PSD paragraph),
 *     then the kind 4 / 5 / 6 cones backtrack from alpha0 = min(that, 1 - sqrt(eps)) on the grid alpha0 step^k as above;
 *   barrier: hipkkt_cone_barrier / hipkkt_step_barrier_dev add, per PSD cone, compute_barrier of coneops_psdtrianglecone.jl:256-290:
 *     Q = svec_to_mat(x + alpha dx), a right-looking lower Cholesky (k-sums in ascending order; a pivot that is not > 0 or not finite
 *     ends it), logdet = dd + dd with dd = sum_j log l_jj in ascending j, +Inf after a failed factorisation, and the cone's term
 *     (0 - logdet_z) - logdet_s, the terms added in PSD-cone order behind the other cones' sum.  As in the reference a shifted point
 *     outside a PSD cone therefore gives -Inf, not +Inf (`barrier -= typemax(T)`); in a solve the step length has bounded alpha inside.
 *     One workgroup per (cone, candidate, z | s), the matrix in LDS: hence the side limit.
 * A PSD side of 65 .. HIPKKT_PSD_STEP_LARGE_MAX_DIM next to a kind 4..6 cone keeps the host loop unless the opt-in of the next paragraph
 * is used, and so does the default start of such a set (the hipkkt_cone_set_identity_scaling group returns HIPKKT_ERR_ARGUMENT): a
 * non-symmetric set starts from the caller's unit initialisation.  Every other hipkkt_step_enable_* keeps refusing such a registration.
 *
 * Opt-in for PSDTriangleCone of side 65 .. HIPKKT_PSD_STEP_LARGE_MAX_DIM next to kinds 4..6: hipkkt_step_enable_mixed_large accepts what
 * hipkkt_step_enable_mixed accepts with every PSD side <= HIPKKT_PSD_STEP_LARGE_MAX_DIM, and the same calls then serve all rows of the
 * handle.  A cone of side <= HIPKKT_PSD_STEP_MAX_DIM and every other family are computed as after hipkkt_step_enable_mixed, bit for
 * bit; a larger cone's rows and its step length by the kernels of hipkkt_step_enable_psd_large, bit for bit as on a handle without the
 * kind 4..6 cones (mul_Hs!, coneops_psdtrianglecone.jl:201-213; step_length, :217-253).  Its barrier (compute_barrier / _logdet_barrier,
 * coneops_psdtrianglecone.jl:256-290) is the computation of the paragraph above expression by expression -- the same load, the same
 * right-looking Cholesky with every entry's subtractions in ascending column order, the same log sum -- by a second kernel behind
 * the first on the same stream: one workgroup of 512 threads per (cone, candidate, z | s) with one 128 x 129 matrix in LDS (132 096
 * bytes, one workgroup per CU); the same input gives the same bits whichever kernel computes a cone.  hipkkt_psd_scaling_enable
 * returns HIPKKT_ERR_ARGUMENT on such a handle while the registration holds a side above HIPKKT_PSD_STEP_MAX_DIM
 * (hipkkt_psd_scaling_enable_large is the call); hipkkt_step_default_start_enable_psd_large and the default-start group keep refusing
 * it.  Sides above HIPKKT_PSD_STEP_LARGE_MAX_DIM keep the host loop.
 *
 * One operation each, host vectors of length m in cone order (the unit-tested surface):
 *   hipkkt_cone_affine_ds            ds = lambda o lambda                  coneops_nncone.jl affine_ds!, coneops_socone.jl:219-228
 *   hipkkt_cone_combined_ds_shift    shift = W^-1 step_s o W step_z - sigma mu e   coneops_symmetric_common.jl:1-36, coneops_socone.jl:300-347
 *   hipkkt_cone_ds_from_dz_offset    out = ds ./ z resp. coneops_socone.jl:241-268
 *   hipkkt_cone_mul_hs               y = Hs x                               coneops_nncone.jl:104-113, coneops_socone.jl:201-216
 *   hipkkt_cone_step_length          alpha_out2 = (alpha_z, alpha_s) <= alpha_max   coneops_nncone.jl:151-170, coneops_socone.jl:270-286,
 *                                    the exact minimum over all cones (coneops_compositecone.jl:216-252) */
int32_t hipkkt_cone_affine_ds(hipkkt_handle h, double *ds_out);
int32_t hipkkt_cone_combined_ds_shift(hipkkt_handle h, const double *step_z, const double *step_s, double sigma_mu, double *shift_out);
int32_t hipkkt_cone_ds_from_dz_offset(hipkkt_handle h, const double *ds, double *out);
int32_t hipkkt_cone_mul_hs(hipkkt_handle h, const double *x, double *y_out);
int32_t hipkkt_cone_step_length(hipkkt_handle h, const double *dz, const double *ds, double alpha_max, double *alpha_out2);
/* enable != 0: HIPKKT_ERR_ARGUMENT unless the last hipkkt_set_cone_types_ex names kinds {0, 1, 2, 4, 5} only with at least one 4 / 5,
 * 0 < linesearch_backtrack_step < 1, min_terminate_step_length > 0 and the implied trip count is at most 4096.  enable == 0 switches
 * it off.  Every hipkkt_set_cone_types[_ex] clears it. */
int32_t hipkkt_step_enable_cone3(hipkkt_handle h, int32_t enable, double linesearch_backtrack_step, double min_terminate_step_length);
/* enable != 0: HIPKKT_ERR_ARGUMENT unless the last hipkkt_set_cone_types_ex names kinds {0, 1, 2, 4, 5, 6} only with at least one 6; the
 * parameter checks, the trip bound and the invalidation of the resident scaling are those of hipkkt_step_enable_cone3.  enable == 0
 * switches the GenPower and the Exponential / Power step off.  Every hipkkt_set_cone_types[_ex] clears it. */
int32_t hipkkt_step_enable_genpow(hipkkt_handle h, int32_t enable, double linesearch_backtrack_step, double min_terminate_step_length);
/* The largest PSD side the device step serves: three n x n double matrices (3 x 32 KiB) fit one workgroup's LDS (160 KiB per CU) with
 * room to spare; larger cones keep the host loop. */
#define HIPKKT_PSD_STEP_MAX_DIM 64
/* enable != 0: HIPKKT_ERR_ARGUMENT unless the last hipkkt_set_cone_types[_ex] names kinds {0, 1, 2, 3} only with at least one 3 and every
 * PSD side <= HIPKKT_PSD_STEP_MAX_DIM.  Enabling invalidates the resident scaling, as hipkkt_step_enable_cone3 does.  enable == 0
 * switches it off.  Every hipkkt_set_cone_types[_ex] clears it. */
int32_t hipkkt_step_enable_psd(hipkkt_handle h, int32_t enable);
/* The largest PSD side hipkkt_step_enable_psd_large serves: the matrix of the step length's Jacobi iteration (128 x 129 doubles, 129 KiB)
 * is the one thing that must fit one workgroup's LDS. */
#define HIPKKT_PSD_STEP_LARGE_MAX_DIM 128
/* hipkkt_step_enable_psd with the side limit HIPKKT_PSD_STEP_LARGE_MAX_DIM: enable != 0 returns HIPKKT_ERR_ARGUMENT and leaves the handle
 * as it was unless the last hipkkt_set_cone_types[_ex] names kinds {0, 1, 2, 3} only with at least one 3 and every PSD side <=
 * HIPKKT_PSD_STEP_LARGE_MAX_DIM.  Enabling invalidates the resident scaling and allocates the larger cones' workspace.  enable == 0
 * does what hipkkt_step_enable_psd(h, 0) does.  Every hipkkt_set_cone_types[_ex] clears it. */
int32_t hipkkt_step_enable_psd_large(hipkkt_handle h, int32_t enable);
/* enable != 0: HIPKKT_ERR_ARGUMENT, and the handle as it was, unless the last hipkkt_set_cone_types_ex names kinds {0, .., 6} only with at
 * least one 3, at least one of 4 / 5 / 6 and every PSD side <= HIPKKT_PSD_STEP_MAX_DIM; the parameter checks, the trip bound and the
 * invalidation of the resident scaling are those of hipkkt_step_enable_cone3, the tables and factor buffers those of
 * hipkkt_step_enable_psd.  enable == 0 switches it off.  Every hipkkt_set_cone_types[_ex] clears it. */
int32_t hipkkt_step_enable_mixed(hipkkt_handle h, int32_t enable, double linesearch_backtrack_step, double min_terminate_step_length);
/* hipkkt_step_enable_mixed with the side limit HIPKKT_PSD_STEP_LARGE_MAX_DIM (compute_barrier of coneops_psdtrianglecone.jl:256-290 for
 * the larger cones next to coneops_compositecone.jl:216-252): enable != 0 returns HIPKKT_ERR_ARGUMENT and leaves the handle as it was
 * unless the last hipkkt_set_cone_types_ex names kinds {0, .., 6} only with at least one 3, at least one of 4 / 5 / 6 and every PSD
 * side <= HIPKKT_PSD_STEP_LARGE_MAX_DIM, and the line-search parameters pass the checks of hipkkt_step_enable_cone3.  Enabling
 * invalidates the resident scaling and allocates the larger cones' workspace, as hipkkt_step_enable_psd_large does.  enable == 0 does
 * what hipkkt_step_enable_mixed(h, 0, ..) does.  Every hipkkt_set_cone_types[_ex] clears it. */
int32_t hipkkt_step_enable_mixed_large(hipkkt_handle h, int32_t enable, double linesearch_backtrack_step,
                                       double min_terminate_step_length);
/* The factors of the PSD cones' scaling for the step (HIPKKT_ERR_ARGUMENT before hipkkt_step_enable_psd / _mixed): Rinv_all = the cones' Rinv, each
 * n x n column-major, concatenated like psd_R; lambda_all = the cones' lambda, n each, concatenated.  They are staged and consumed by
 * the next hipkkt_update_scaling[_ex][_dev]; on an enabled handle that call needs a non-NULL psd_R and factors staged since the last
 * scaling, otherwise it returns HIPKKT_ERR_ARGUMENT and the step calls stay refused until a scaling succeeds.  A lambda entry that is
 * not finite or is <= 0 sets *scaling_ok = 0.  The _dev form does not synchronise with the host; its pointers must stay valid until the
 * next synchronising call on this handle has returned (the rule of hipkkt_set_hs_dev). */
int32_t hipkkt_psd_set_factors(hipkkt_handle h, const double *Rinv_all, const double *lambda_all);
int32_t hipkkt_psd_set_factors_dev(hipkkt_handle h, const double *Rinv_all, const double *lambda_all);
/* Opt-in on top of hipkkt_step_enable_psd / _mixed (HIPKKT_ERR_ARGUMENT before it): the Cholesky / SVD of update_scaling!(::PSDTriangleCone),
 * coneops_psdtrianglecone.jl:78-143, on the device.  On an enabled handle a hipkkt_update_scaling[_ex][_dev] with psd_R == NULL and no
 * factors staged computes, from the (s, z) of that call and per PSD cone (one workgroup each, everything in LDS, same stream, the call
 * keeps its single host synchronisation):
 *   S = L1 L1', Z = L2 L2' (:93-98, lower Cholesky, k-sums in ascending order; a pivot that is not > 0 or not finite fails the cone as
 *     LAPACK's potrf does);
 *   the singular values and vectors of L2' L1 (:107-110) by a one-sided Jacobi iteration on its columns: round-robin sets of disjoint
 *     pairs, a pair rotates when |g_p . g_q| > eps |g_p| |g_q|, at most 40 sweeps, stop after a sweep without a rotation, then one
 *     polishing sweep that rotates every pair;
 *   lambda = the singular values in descending order (:112-113), R = L1 V Sigma^-1/2 (:115-123), Rinv = Sigma^-1/2 U' L2' (:125-131);
 *   one refinement on the (s, z) of the call: lambda_j^2 = (r_j' Z r_j)(q_j' S q_j) / (q_j' r_j)^2 (q_j = row j of Rinv), the three
 *     sums in twice the precision, and r_j, q_j rescaled to r_j' Z r_j = q_j' S q_j = lambda_j, q_j' r_j = 1: lambda is then the
 *     singular value of the exact factors of the float64 (S, Z) to about one eps, whatever cond(S), cond(Z) at an early iterate;
 * and then forms W = R R' and the Hs block as with a caller's psd_R.  R is unique up to column signs (and rotations among equal
 * singular values): R R', lambda and every step operation are what the caller's factors give, to rounding.  The result is the same
 * bits on every run.  A cone that fails (Cholesky, a non-finite entry of s / z, the sweep bound) sets *scaling_ok = 0 with
 * HIPKKT_OK, gets NaN factors and none of its entries of K is written; the other cones are served.  With a non-NULL psd_R and staged
 * factors the call does what it does without this enable.  Enabling or disabling invalidates the resident scaling; enable == 0
 * switches it off, and so do hipkkt_step_enable_psd and every hipkkt_set_cone_types[_ex]. */
int32_t hipkkt_psd_scaling_enable(hipkkt_handle h, int32_t enable);
/* hipkkt_psd_scaling_enable for a handle of hipkkt_step_enable_psd_large or hipkkt_step_enable_mixed_large.  HIPKKT_ERR_ARGUMENT, and the
 * handle as it was, unless the handle is in PSD step mode through hipkkt_step_enable_psd_large or in mixed step mode through
 * hipkkt_step_enable_mixed_large (not after hipkkt_step_enable_psd or _mixed; a side above
 * HIPKKT_PSD_STEP_LARGE_MAX_DIM never gets that far).  Afterwards a hipkkt_update_scaling[_ex][_dev] with psd_R == NULL and no factors
 * staged computes (R, Rinv, lambda) of every PSD cone of the set on the call's stream, with the call's single host synchronisation:
 * the cones hipkkt_step_enable_psd_large routes to its own kernels (side > HIPKKT_PSD_STEP_MAX_DIM) by the algorithm of
 * hipkkt_psd_scaling_enable operation for operation in another placement -- one workgroup of 512 threads per cone, one n x n matrix
 * in LDS, the others in the cone's four matrices of the enable's workspace, the rotations of V applied in device memory -- and the
 * other cones by the kernel of hipkkt_psd_scaling_enable, unchanged; each cone is computed by exactly one of the two.  Every sum runs
 * in the order of the smaller cones' kernel: the same (s, z) give the same bits whichever kernel computes a cone, and on every run.
 * Failures are those of hipkkt_psd_scaling_enable (*scaling_ok = 0 with HIPKKT_OK, NaN factors for that cone, none of its entries of
 * K written, the other cones served); hipkkt_psd_get_factors reads the result back.  With a non-NULL psd_R and staged factors the
 * call does what it does without this enable.  Enabling or disabling invalidates the resident scaling; enable == 0 switches it off,
 * and so do hipkkt_step_enable_psd[_large], hipkkt_step_enable_mixed[_large] and every hipkkt_set_cone_types[_ex]. */
int32_t hipkkt_psd_scaling_enable_large(hipkkt_handle h, int32_t enable);
/* The resident factors of the last scaling of a handle in PSD or mixed step mode, whoever computed them (K.data.R, .Rinv, .lambda of
 * coneops_psdtrianglecone.jl:112-131): R and Rinv n x n column-major per cone, concatenated like psd_R, lambda n per cone.  Host
 * pointers, any may be NULL.  HIPKKT_ERR_ARGUMENT when no scaling call has completed since the enable; after a call that reported
 * *scaling_ok = 0 the failed cones' entries are NaN. */
int32_t hipkkt_psd_get_factors(hipkkt_handle h, double *R_out, double *Rinv_out, double *lambda_out);
/* compute_barrier of the cone set (Zero 0, Nonnegative -sum log((s + a ds)(z + a dz)), coneops_socone.jl:288-305,
 * coneops_expcone.jl:189-248, coneops_powcone.jl:228-251) and dot_shifted (mathutils.jl:23-43) at nalpha <= 8 candidate step lengths:
 * out[2 j] = the barrier, out[2 j + 1] = <z + a_j dz, s + a_j ds>, both summed over fixed slices in a fixed order.  A point outside a
 * cone gives +Inf or what logsafe gives; after hipkkt_step_enable_mixed the PSD cones' -logdet(Z + a dZ) - logdet(S + a dS) is added
 * (coneops_psdtrianglecone.jl:256-290), -Inf for a point outside such a cone.  dz, ds: host vectors of length m; (s, z) are the resident ones.
 * hipkkt_step_barrier_dev: the same for the iterate xzs_dev = [x | z | s] and the resident step of the last fused call; one host
 * synchronisation per call. */
int32_t hipkkt_cone_barrier(hipkkt_handle h, const double *dz, const double *ds, const double *alphas, int64_t nalpha, double *out);
int32_t hipkkt_step_barrier_dev(hipkkt_handle h, const double *xzs_dev, const double *alphas, int64_t nalpha, double *out);
/* once per problem (L1 handles): the equilibration vectors d[n], e[m] of problemdata.jl:133-221 for hipkkt_step_info_norms_dev; the
 * reciprocals are formed on the host as 1 ./ d, 1 ./ e like problemdata.jl does, so they are the caller's dinv / einv bit for bit */
int32_t hipkkt_set_equilibration(hipkkt_handle h, const double *d, const double *e);
/* The fused calls.  xzs_dev = [x | z | s] and res_dev = [rx | rz | rx_inf | rz_inf | Px] are the device buffers of hipkkt_residuals_dev;
 * only scalars cross PCIe and each call synchronises with the host once (hipkkt_step_apply_dev: not at all).  The reduced solve is
 * hipkkt_kkt_solve_reduced_dev's code path (const_pending as there); the step [dx | dz | ds] stays in the handle.
 *   hipkkt_step_affine_dev    variables_affine_step_rhs! (variables.jl:107-121) + kkt_solve!(:affine) (kktsystem.jl:135-215) + the affine
 *     step length (variables.jl:14-43).  scal_in3 = {tau, kappa, r_tau}: rhs.x = rx, workz = s - rz, rhs.tau = r_tau, rhs.kappa = tau kappa;
 *     ds = -(Hs dz + s), dkappa = -(rhs.kappa + kappa dtau) / tau, alpha = min over tau, kappa, 1 and the cones.
 *   hipkkt_step_combined_dev  variables_combined_step_rhs! (variables.jl:124-162) + kkt_solve!(:combined) + the step length times
 *     max_step_fraction.  scal_in9 = {tau, kappa, r_tau, dtau_aff, dkappa_aff, sigma, mu, m_corr, max_step_fraction}; the affine step
 *     must be resident: rhs.kappa = -sigma mu + m_corr dtau_aff dkappa_aff + tau kappa, dz_aff is scaled by m_corr when m_corr != 1,
 *     rhs.s = lambda o lambda + shift, ds_const = Delta_s_from_Delta_z_offset(rhs.s), workz = ds_const - (1 - sigma) rz,
 *     rhs.x = (1 - sigma) rx, rhs.tau = (1 - sigma) r_tau; ds = -(Hs dz + ds_const).
 *   scal_out15 = {alpha, dtau, dkappa, alpha_z, alpha_s of the cones for alpha_max = 1, scal_out10 of hipkkt_kkt_solve_reduced};
 *   ir_steps2 as there (may be NULL).
 *   hipkkt_step_apply_dev     [x | z | s] += alpha [dx | dz | ds] in place; tau and kappa are the caller's, from the scalars it has.
 *     Not synchronised with the host: xzs_dev must stay valid until the next synchronising call on this handle has returned.
 *   hipkkt_step_info_norms_dev  out8 = |d x|, |e z|, |einv s|, |dinv rx|, |einv rz|, |dinv rx_inf|, |einv rz_inf|, |dinv Px| (2-norms of
 *     info_update!, info.jl:1-60), summed in a fixed order.  Needs hipkkt_set_equilibration, no scaling.
 *   hipkkt_step_get           out = the resident step [dx | dz | ds] (n + 2 m doubles, host; tests, debugging) */
int32_t hipkkt_step_affine_dev(hipkkt_handle h, const double *xzs_dev, const double *res_dev, const double *scal_in3, int32_t const_pending,
                               double *scal_out15, int32_t ir_enable, double reltol, double abstol, int64_t max_iter, double stop_ratio,
                               int64_t *ir_steps2);
int32_t hipkkt_step_combined_dev(hipkkt_handle h, const double *xzs_dev, const double *res_dev, const double *scal_in9,
                                 int32_t const_pending, double *scal_out15, int32_t ir_enable, double reltol, double abstol,
                                 int64_t max_iter, double stop_ratio, int64_t *ir_steps2);
int32_t hipkkt_step_apply_dev(hipkkt_handle h, double alpha, double *xzs_dev);
int32_t hipkkt_step_info_norms_dev(hipkkt_handle h, const double *xzs_dev, const double *res_dev, double *out8);
int32_t hipkkt_step_get(hipkkt_handle h, double *out);
/* The default start of a symmetric cone set (solver.jl:383-405) on the device.  Served: L1 handles whose registration is Zero /
 * Nonnegative / SecondOrder only, or holds PSD triangle cones next to them after hipkkt_step_enable_psd[_large] (every side <=
 * HIPKKT_PSD_STEP_MAX_DIM, or <= HIPKKT_PSD_STEP_LARGE_MAX_DIM after hipkkt_step_default_start_enable_psd_large); anything else (a kind 4..6, PSD without the enable, an L0 handle) is HIPKKT_ERR_ARGUMENT.  No scaling is
 * needed.  pd: 0 = primal cone, 1 = dual cone.
 *   hipkkt_cone_set_identity_scaling  set_identity_scaling! (coneops_compositecone.jl:92-101) + get_Hs! (:123-131) + the Hs / sparse-cone
 *     part of _kktsolver_update_inner! (kktsolver_directldl.jl:211-245) for that scaling, written into the resident K; nothing is
 *     uploaded.  K holds the bits hipkkt_set_hs / hipkkt_set_soc_batch leave after the host cones' identity scaling: Zero rows -0,
 *     Nonnegative rows -1, second-order cones their dense (dim <= 4) block or d = 0.5, u = [sqrt 0.5, 0 ...], v = 0, eta^2 = 1
 *     (coneops_socone.jl:57-73, directldl_datamaps.jl:61-79), PSD cones the packed upper triangle of I (coneops_psdtrianglecone.jl:66-75).
 *     The resident scaling and the resident constant-rhs solution are dropped: the step calls are refused until the next successful
 *     hipkkt_update_scaling*.
 *   hipkkt_cone_margins  out2 = (alpha, beta) of margins(::CompositeCone) (coneops_compositecone.jl:49-63) for the host vector v[m]:
 *     Zero (floatmax, 0), Nonnegative (minimum, sum of the positive entries; coneops_nncone.jl:19-38), second-order (z0 - |z1|,
 *     max(0, alpha); coneops_socone.jl:13-22), PSD (smallest eigenvalue, sum of the positive eigenvalues of svec_to_mat;
 *     coneops_psdtrianglecone.jl:8-27; cyclic Jacobi sweeps).  beta is summed over fixed slices in a fixed order (Nonnegative rows,
 *     second-order cones, PSD cones), not in cone order.  min and max propagate a NaN as the reference's do.
 *   hipkkt_cone_shift_to_interior  _shift_to_cone_interior! (variables.jl:180-208) of v[m] in place; out4 = {min_margin, pos_margin,
 *     target, branch}: target = max(1, 0.1 pos_margin / degree) (1 when the degree is 0), branch 0: min_margin <= 0, shift by
 *     -min_margin and then by target (two additions); 1: min_margin < target, shift by target - min_margin; 2: shift by 0 (which
 *     zeroes the Zero rows of a primal vector and turns -0 into +0).  A NaN min_margin takes branch 2.
 *   hipkkt_step_default_start_dev  the fused call: the identity scaling, hipkkt_refactor's code path (robust-order twin included),
 *     kkt_solve_initial_point! (kktsystem.jl:95-132) with the right-hand sides formed from the resident q, b (needs hipkkt_set_qb) --
 *     structural nnz(P) != 0: one refined solve of [-q; b] for (x, z), s = -z; nnz(P) == 0: [0; b] for (x, -s) and [-q; 0] for z on the
 *     two solve contexts -- then variables_symmetric_initialization! (variables.jl:167-208): the primal shift of s and the dual shift of
 *     z.  xzs_dev = [x | z | s] (device, n + 2 m doubles) is written; vectors never cross PCIe.  scal_out8 = {eps_used, n_dynamic_reg,
 *     min_margin_s, pos_margin_s, target_s, min_margin_z, pos_margin_z, target_z}; ir_steps2 (may be NULL) = the refinement steps of
 *     the solve(s).  The cone algebra is enqueued behind the solves and read back with their synchronisation.  Return codes as
 *     hipkkt_step_affine_dev; HIPKKT_NUMERICAL_FAILURE when the factorisation or a solve fails (xzs_dev is then unspecified). */
int32_t hipkkt_cone_set_identity_scaling(hipkkt_handle h);
int32_t hipkkt_cone_margins(hipkkt_handle h, const double *v, int32_t pd, double *out2);
int32_t hipkkt_cone_shift_to_interior(hipkkt_handle h, double *v, int32_t pd, double *out4);
int32_t hipkkt_step_default_start_dev(hipkkt_handle h, double *xzs_dev, int32_t static_reg_enable, double eps_const, double eps_prop,
                                      int32_t ir_enable, double reltol, double abstol, int64_t max_iter, double stop_ratio,
                                      double *scal_out8, int64_t *ir_steps2);
/* The default start for a handle of hipkkt_step_enable_psd_large with a side above HIPKKT_PSD_STEP_MAX_DIM.  HIPKKT_ERR_ARGUMENT, and
 * the handle as it was, unless the handle is in PSD step mode through hipkkt_step_enable_psd_large (a handle of
 * hipkkt_step_enable_mixed_large is refused: a non-symmetric set starts from the caller's unit initialisation).  Afterwards the four calls above
 * serve the handle: the identity scaling does not depend on the side, the margins of a cone of side > HIPKKT_PSD_STEP_MAX_DIM come
 * from a second launch with one 128 x 129 matrix in LDS (the same sweeps: the same bits as the smaller cones' kernel on the same
 * matrix), the shift takes the larger side bound.  Without it they keep refusing such a handle.  enable == 0 switches it off, and so
 * do hipkkt_step_enable_psd[_large] and every hipkkt_set_cone_types[_ex]. */
int32_t hipkkt_step_default_start_enable_psd_large(hipkkt_handle h, int32_t enable);

/* ---- timing (device time on the handle's stream, HIP events) ------------------------------- */
/* out[0] = ms of last refactor (value scatter + numeric LDL), out[1] = ms of last solve call
 * (all LDL solves + SpMVs of the refinement), out[2] = accumulated refactor ms, out[3] = accumulated
 * solve ms, out[4] = #refactors, out[5] = #solve calls, out[6] = #LDL solves, out[7] = ms of the
 * dense-update kernels inside the last refactor (0 unless profiling was enabled) */
int32_t hipkkt_get_timing(hipkkt_handle h, double *out8);
int32_t hipkkt_reset_timing(hipkkt_handle h);
/* last refactorisation run with profiling enabled: out[0] = ms of all Schur-update kernels, out[1] = ms of the
 * k_update_dense<4,4> launches alone (one wavefront per 64x64 tile), out[2] = their algorithmic flops, out[3] = their
 * number; out[4] = ms of the k_front_block launches (one per update batch of a front), out[5] = their number, out[6] = the panels
 * they factor, out[7] = the Schur-update flops of the stages they absorb (not part of out[0]'s kernels), out[8] / out[9] = dense update
 * tiles / their flops that rode in those launches as extra workgroups instead of in their stage's own launch (the partial last round
 * of a front batch's far updates; not part of out[0] .. out[2] either); out[10] = the wide diagonal blocks (> 16 columns) of the last factorisation
 * OUTSIDE the fronts whose explicit inverse has an entry above 64 in magnitude: the solve kernels take one refinement step
 * y += Linv (b - L y)  on these (a product with such an inverse is several times less accurate than the reference's substitution; the
 * 64-column panels of a front are solved by the front sweeps, which never refine, and are not counted; testing build: switch
 * ACCURATE=<threshold>, 0 = never, negative = every wide block), out[11] = factorisations so far with at least one */
int32_t hipkkt_get_profile(hipkkt_handle h, double *out, int64_t cap);   /* writes min(cap, 12) values */
/* the k_update_dense<4,4> launches of that refactorisation one by one: ms[i], algorithmic flops[i], target tiles[i]
 * (any array may be NULL; at most cap entries are written, *count receives the number of launches) */
int32_t hipkkt_get_profile_launches(hipkkt_handle h, double *ms, double *flops, double *tiles, int64_t cap, int64_t *count);
/* 1 = time the update (MFMA) kernels and the k_front_block launches separately inside refactor (eager launches, adds event overhead);
 * 2 = the same with every far update tile kept in its stage's own launch (none riding in the next k_front_block launch): the
 * comparison figure for out[8] / out[9] of hipkkt_get_profile; 0 = off */
int32_t hipkkt_set_profiling(hipkkt_handle h, int32_t enable);

/* robustness counters: out[0] = persistent sweep time-outs seen so far (each one repeats the solve on the per-level
 * kernels and suspends the persistent kernels for a while), out[1] = persistent sweeps currently enabled (0/1),
 * out[2] = factorisations repeated on the robust-order twin, out[3] = twin exists, out[4] = the current factorisation
 * lives in the twin, out[5] = ordering in use (0 minimum degree on K, 1 cone rows first, 2 user), out[6] = #fronts,
 * out[7] = #segments, out[8] = update batches of fronts factored by one launch each (front_block.hip), out[9] = that path is
 * enabled (0 after one of its hand-offs timed out: the handle then keeps one launch per panel), out[10] / out[11] = symbolic plans
 * taken from / not found in the process-wide plan cache (same KKT pattern and options => the analysis of an earlier handle is reused;
 * testing build: switch PLAN_CACHE=0 disables it), out[12] = the pivot chain of the front batches is streamed block by block (front_block2.hip; 0 only in the testing build with
 * the switch FB_STREAM=0), out[13] = factorisations with refined block solves (hipkkt_get_profile out[11]), out[14] = target entries of the per-entry gather lists
 * that every factorisation applies on a side stream next to the levels of the following update batch (round 6).  Writes min(cap, 15) values. */
int32_t hipkkt_get_counters(hipkkt_handle h, int64_t *out, int64_t cap);

/* developer diagnostic, not part of the plugin contract: copies an internal vector of the last LDL solve (what = 0 the
 * permuted right-hand side, 1 z = D^-1 L^-1 b, 2 x in permuted order, 3 the forward update vectors, 4 the unregularised KKT values in nz order, 5 D and 6 1/D of the last factorisation, 7 / 8 the u / v vectors of the sparse second-order cones) or a plan table converted to doubles (10 supernode first
 * columns, 11 levels, 12 rows per supernode, 13 parents, 14 membership in the persistent sweeps; 15 / 16 the stream records / scratch
 * tiles of the front batches, 17 the refinement state of the last refined solve: ||e|| before its last step, ||b||, ||e|| after it, steps; 18 the residual b - K x of
 * the last SpMV on solve context 0 (original ordering), 19 the number of dense triangles of K outside the symmetric view, 20 six values per
 * dense update tile of the plan: stage, tasks, sum of source widths, tasks through a tile map, full-tile flag, sum of rows x columns x
 * width; 21 five values per supernode of the persistent segment sweeps: level, width, rows, longest and mean gather list of its row
 * slots -- tools/dense_stage_stats.py; 22 four values per front, written on the host: its first panel (supernode id), panels, rows,
 * and the panels per super-block of its solve sweeps, 0 = one hop per panel through that panel's inverse (k_front_fwd / k_front_bwd),
 * > 0 = products with the super-blocks' inverses (k_front_fwd_sb / k_front_bwd_sb), 23 the Newton steps of the last hipkkt_update_scaling_ex per
 * Power cone in cone order, 24 the PSD cones step_psd_large.hip serves on this handle, as indices into the registration's PSD cones,
 * read back from the device list -- empty unless hipkkt_step_enable_psd_large / _mixed_large is in place, 25 the work matrices of those cones as the
 * last step operation left them, four of 128 x 128 doubles per served cone, each n x n column-major from its start); *len receives the length, nothing is copied
 * when cap is too small */
int32_t hipkkt_debug_dump(hipkkt_handle h, int32_t what, double *out, int64_t cap, int64_t *len);
/* developer diagnostic, host logic only (no device needed): how many of the `nd` dense tiles of a front batch's far stage -- the
 * first `ncrit` of them belong to the next batch's columns -- ride in the next k_front_block launch, which has `next_blk` workgroups
 * of its own; *per_wave receives the tiles per wavefront there (hipkkt_factor.cpp fb_extra_tiles_of_stage) */
int32_t hipkkt_debug_extra_tiles(int32_t nd, int32_t ncrit, int32_t next_blk, int32_t *per_wave);
/* test / experiment switches -- NOT part of the plugin contract, the Julia glue never calls it.  key = the switch's name ("FB_V2",
 * "SPLIT_K", "ACCURATE", "SPIN_LIMIT", ...: struct DebugOpts in csrc/hipkkt_internal.h lists them), value = its setting as text, NULL =
 * back to the default; key == NULL resets every switch.  A handle reads the switches when it is created.  Only the TESTING build of
 * the library (libclarabel_hipkkt_testing.so, compiled with -DHIPKKT_TESTING; what tests/ load) accepts a setting: the production
 * library returns HIPKKT_ERR_ARGUMENT for every key, contains neither the first form of the front-batch kernel nor the debug flags
 * of the sweeps, and reads no environment variable for any switch (HIPKKT_VERBOSE and HIPKKT_FB_TRACE, which change no result, are
 * the only two it reads).  Process-wide, not thread-safe against concurrent creates. */
int32_t hipkkt_debug_set(const char *key, const char *value);
/* 1 in the testing build, 0 in the production library */
int32_t hipkkt_debug_is_testing_build(void);

/* diagnostic: checks the FP64 matrix-core operand/result lane maps used by the update kernel
 * against a host product with an asymmetric B (returns 0 when they agree to 1e-12) */
int32_t hipkkt_selftest_mfma(int32_t device_id, double *max_err);

/* diagnostic, no handle needed: what the latency-bound kernels of the factorisation (k_front_block, k_factor_panel, the sweeps) depend
 * on and the matrix-core- / memory-bound ones do not.  out[0] = the shader clock (GHz) one busy wavefront really gets (shader cycles
 * against the 100 MHz constant clock), out[1] / out[2] = round trip (ns) of a flag between two workgroups on the SAME / on DIFFERENT
 * XCDs with relaxed agent-scope atomics (the hand-offs of the front kernels; -1 = no such pair), out[3] = XCDs seen, out[4] / out[5] =
 * the runtime's core / memory clock (MHz), out[6] = compute units, out[7] = reserved.  Writes min(cap, 8) values.  bench.py prints it
 * in its JSON line so that a slow line names its cause. */
int32_t hipkkt_box_probe(int32_t device_id, double *out, int64_t cap);

/* last error text for this handle (or for a failed create when h == NULL); never NULL */
const char *hipkkt_last_error(hipkkt_handle h);

#ifdef __cplusplus
}
#endif
#endif
