// The launchers of every .hip file of the library, one heading per file (all work is enqueued on the given stream)
#pragma once
#include <hip/hip_runtime.h>

#include "device_plan.h"

namespace hipkkt {
// values.hip: value updates on the resident K
void launch_scatter_values(hipStream_t st, double *kval, const int64_t *idx, const double *vals, int64_t n, double scale);
void launch_scale_values(hipStream_t st, double *kval, const int64_t *idx, int64_t n, double scale);
void launch_soc_batch(hipStream_t st, double *kval, const int64_t *uidx, const int64_t *vidx, const int *cone_of,
                      const double *u, const double *v, const double *eta2, int64_t n, const int64_t *didx, int nsoc);
// skip != NULL: the launch writes nothing when *skip != 0 (the word of a cone whose device-side scaling failed, scaling_psd.hip)
void launch_psd_hs(hipStream_t st, double *kval, const int64_t *map_hs, int64_t hs_off, const double *W, int n, const int *skip = nullptr);
void launch_zero_words(hipStream_t st, void *p, int nwords);
// kernels.hip: the numeric factorisation
void launch_maxabs_gather(hipStream_t st, const double *v, const int64_t *idx, int64_t n, unsigned long long *slot);
void launch_init_panels(hipStream_t st, const DevPlan &P, int64_t nnz, int static_enable, double eps_const, double eps_prop);
void launch_factor_level(hipStream_t st, const DevPlan &P, int item_begin, int nitems, int wmax, double dyn_eps, double dyn_delta);
void launch_factor_panel(hipStream_t st, const DevPlan &P, int item_begin, int nitems, double dyn_eps, double dyn_delta);
void launch_update_stage(hipStream_t st, const DevPlan &P, int group_begin, int ngroups);
// Up to kDenseStripTiles tiles a dense launch runs the strip kernel (k_update_dense<1,2>, the just-in-time updates), above it one
// wavefront per tile (k_update_dense<4,4>).  full_k: the tiles of this launch carry whole panels of sources (>= 1.5 MFLOP per tile,
// dense_full_k over the stage's nd tiles and their flops): a partial last round is cut into pieces
constexpr int kDenseStripTiles = 384;
constexpr double kFullKFlopsPerTile = 1.5e6;
inline bool dense_full_k(int nd, double flops) { return nd > 0 && flops >= kFullKFlopsPerTile * nd; }
void launch_update_dense(hipStream_t st, const DevPlan &P, int group_begin, int ngroups, bool full_k = false);
// split-K: adds the partial tiles of `n` split target tiles to their targets (fixed order) and clears them (k_split_reduce)
void launch_split_reduce(hipStream_t st, const DevPlan &P, const SplitRec *recs, int n);
void launch_update_gather(hipStream_t st, const DevPlan &P, int64_t ebegin, int64_t n, int64_t hbegin, int64_t nheavy, int max_blocks = 0);
void launch_invert_diag(hipStream_t st, const DevPlan &P, int n_small, int wmax_small, int n_wide);
// solve_sweep.hip: triangular solves over the regular supernodes
void launch_permute_in(hipStream_t st, const double *b, const int *perm, double *y, int n, int *epoch, int *ticks, int nticks, int *zero = nullptr,
                       int nzero = 0);   // zero[0 .. nzero): words cleared by the solve's first kernel for the kernels behind it
void launch_fwd_level(hipStream_t st, const DevPlan &P, int item_begin, int nitems, double *y, double *z);
void launch_bwd_partial(hipStream_t st, const DevPlan &P, int item_begin, int nitems, const double *x);
void launch_bwd_final(hipStream_t st, const DevPlan &P, int sn_begin, int nsn, const double *z, double *x, double *xout);
void launch_fwd_narrow(hipStream_t st, const DevPlan &P, int sn_begin, int n, int wmax, double *y, double *z);
void launch_bwd_narrow(hipStream_t st, const DevPlan &P, int sn_begin, int n, int wmax, const double *z, double *x, double *xout);
void launch_fwd_seg(hipStream_t st, const DevPlan &P, int seg, int item_begin, int nitems, int nsuper, double *y, double *z);
// first: the first backward segment launch of a solve (it re-arms the forward sweeps' counters)
void launch_bwd_seg(hipStream_t st, const DevPlan &P, int seg, int item_begin, int nitems, int nsuper, int first, const double *z,
                    double *x, double *xout);
// front_sweep.hip: sweeps over a front.  launch_front_fwd / _bwd choose between one hop per panel and the super-block sweeps
// (FrontDesc::sb_g > 0), which need the super-block inverses of launch_invert_super
void launch_front_fwd(hipStream_t st, const DevPlan &P, const FrontDesc &F, double *y, double *z);
void launch_front_bwd(hipStream_t st, const DevPlan &P, const FrontDesc &F, const double *z, double *x, double *xout);
void launch_invert_super(hipStream_t st, const DevPlan &P, const FrontDesc &F);
// refine.hip: SpMV, refinement, residuals, reduced system
// e = b - K x and its max norm; x = x0 when rs == nullptr, otherwise the candidate iterate of the refinement state
void launch_spmv_residual(hipStream_t st, const DevPlan &P, const double *b, const RefineState *rs, const double *x0, const double *x1,
                          double *e, int n, unsigned long long *slot);
int long_row_threshold();   // rows of the symmetric CSR view with more entries are taken by k_spmv_long
void launch_norm_inf(hipStream_t st, const double *v, int n, unsigned long long *slot);
void launch_refine_decide(hipStream_t st, RefineState *rs, const double *scal, int phase, double reltol, double abstol, int max_iter,
                          double stop_ratio);
void launch_refine_add(hipStream_t st, const RefineState *rs, double *x0, double *x1, const double *corr, int n);
void launch_refine_copy_out(hipStream_t st, const RefineState *rs, const double *x0, const double *x1, double *out, int nm);
void launch_set_rhs(hipStream_t st, double *b, const double *rhs, int nm, int n);
void launch_check_finite(hipStream_t st, const double *v, int n, int *flags);
void launch_block_products(hipStream_t st, const DevPlan &P, const double *x, const double *z, double *Px, double *ATz,
                           double *Ax, int n, int m);
int residual_blocks(int n, int m);
void launch_residuals(hipStream_t st, const DevPlan &P, const double *x, const double *z, const double *s, const double *q,
                      const double *b, double tau, double kappa, double *out, double *part, double *scal, int n, int m);
// N2: reduced-system algebra of kkt_solve! (part: 8 * residual_blocks(n, m) doubles, scal_out: 10 doubles)
void launch_reduced(hipStream_t st, const DevPlan &P, const double *s1, const double *s2, const double *xv, const double *q,
                    const double *b, double tau, double kappa, double rhs_tau, double rhs_kappa, double *part, double *scal_out,
                    double *lhs, int n, int m);
void launch_const_rhs(hipStream_t st, double *dst, const double *qb, int n, int nm, int N);
// probe.hip
void launch_mfma_probe(hipStream_t st, const double *A, const double *B, double *out);
// front_block.hip
void launch_front_block(hipStream_t st, const DevPlan &P, const FrontBatch &B, int *sync_all, double *scratch_all, double *stream_all,
                        double dyn_eps, double dyn_delta, bool streamed, long long *trace = nullptr);
// front_block2.hip: the same batch with every tile transposed in the accumulators (round 5; the default)
void launch_front_block2(hipStream_t st, const DevPlan &P, const FrontBatch &B, int *sync_all, double *scratch_all, double *stream_all,
                         double dyn_eps, double dyn_delta, long long *trace = nullptr);
// zeroes the sync words of all front batches and fills the stream records of the streamed pivot chain with the "not yet written" sentinel
void launch_fb_reset(hipStream_t st, int *sync_all, int nsync, double *stream_all, int64_t nstream);
// scaling.hip (N1)
void launch_scaling_diag(hipStream_t st, const signed char *row_kind, const int64_t *row_hs, const int64_t *map_hs, const double *s,
                         const double *z, double *w, double *lam, double *kval, int64_t m);
void launch_scaling_soc(hipStream_t st, int nsoc, const int64_t *desc, const int64_t *map_hs, const double *s, const double *z,
                        double *w, double *lam, double *eta_out, double *soc_u, double *soc_v, double *soc_eta2, double *kval,
                        int *fail);
void launch_psd_rrt(hipStream_t st, const double *R, double *W, int n);
// scaling.hip, the non-symmetric cones (hipkkt_update_scaling_ex).  Three-row cones: SoA tables ordered by kind, the first nexp
// entries Exponential, the next npow Power (one launch per kind: a wavefront never mixes the two bodies); strategy 0 PrimalDual,
// 1 Dual; trips (may be NULL) receives the Newton steps per table entry.  Generalized Power: one wavefront per cone, desc = 8 int64 per
// cone, idx = the resident [map.q | map.r | map.p | map.D] tables concatenated.
void launch_scaling_cone3(hipStream_t st, int nexp, int npow, const int64_t *row0, const int64_t *hs0, const int64_t *out0,
                          const double *alpha, const int64_t *map_hs, const double *s, const double *z, double mu, int strategy,
                          double *kval, double *out, int *trips, int *fail);
void launch_scaling_genpow(hipStream_t st, int ngenpow, const int64_t *desc, const double *alpha, const int64_t *idx,
                           const int64_t *map_hs, const double *z, double mu, double sqrtmu, double *kval, double *out, int *fail);
// step.hip: the cone algebra of an interior-point step for Zero / Nonnegative / SecondOrder cones (row_kind, desc: the tables of the
// scaling kernels).  part of launch_step_length: 2 * step_len_pairs(m, nsoc) doubles; of launch_step_info_norms: step_norm_part_doubles()
int64_t step_len_pairs(int64_t m, int nsoc);
int64_t step_norm_part_doubles();
void launch_step_affine_ds(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, const double *lam, double *out,
                           int64_t m);
void launch_step_shift(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, const double *w, const double *eta,
                       const double *dz, const double *ds, double sigma_mu, double *out, int64_t m);
void launch_step_offset(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, const double *z, const double *w,
                        const double *lam, const double *eta, const double *ds, double *out, int64_t m);
// addc != NULL: y = -(Hs x + addc)
void launch_step_mulhs(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, const double *w, const double *eta,
                       const double *x, const double *addc, double *y, int64_t m);
void launch_step_length(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, const double *z, const double *s,
                        const double *dz, const double *ds, double alpha_max, double *part, double *out2, int64_t m);
void launch_step_add_step(hipStream_t st, double *v, const double *dv, double alpha, int64_t len);
void launch_step_scale(hipStream_t st, double *out, const double *in, double f, int64_t len);
void launch_step_add(hipStream_t st, double *acc, const double *b, int64_t len);
// in = [rhs.x | workz | variables.x]: dsc == NULL the affine step (rx, s - rz), otherwise (f rx, dsc - f rz)
void launch_step_rhs(hipStream_t st, double *in, const double *xzs, const double *res, const double *dsc, double f, int64_t n, int64_t m);
// eq = [d | e | dinv | einv]
void launch_step_info_norms(hipStream_t st, const double *xzs, const double *res, const double *eq, double *part, double *out8, int64_t n,
                            int64_t m);
// step_cone3.hip: the same operations on the rows of the Exponential / Power cones (the [Exponential | Power] tables of
// launch_scaling_cone3; nsout = its output vector: Hs 6, H_dual 6, grad 3 per cone), their backtracking step length and the barrier of
// the whole cone set at nalpha <= step3_max_candidates() step lengths
int step3_max_candidates();
int64_t step3_barrier_doubles(int64_t ncones);
void launch_step3_copy(hipStream_t st, int n3, const int64_t *row0, const double *src, double *out);
void launch_step3_mulhs(hipStream_t st, int n3, const int64_t *row0, const int64_t *out0, const double *nsout, const double *x,
                        const double *addc, double *y);
void launch_step3_shift(hipStream_t st, int nexp, int npow, const int64_t *row0, const int64_t *out0, const double *alpha,
                        const double *nsout, const double *z, const double *dz, const double *ds, double sigma_mu, double *out);
void launch_step3_length(hipStream_t st, int nexp, int npow, const int64_t *row0, const double *alpha, const double *z, const double *s,
                         const double *dz, const double *ds, const double *sym2, const double *dtau, double tau, double kappa,
                         double rhs_kappa, double alpha_max, double step, double alpha_min, int trips, double *part, double *out2,
                         int ngp = 0);
void launch_step3_barrier(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, int nexp, int npow,
                          const int64_t *row0, const double *alpha, const double *z, const double *s, const double *dz, const double *ds,
                          const double *alphas, int nalpha, double *work, double *out, int64_t m, int ngp = 0);
// step_genpow.hip: the same operations on the rows of the Generalized Power cones, one wavefront per cone (desc, alpha: the tables of
// launch_scaling_genpow, desc[8 c + 7] = the bits of 1 / <alpha, alpha>; nsout = the scaling's output vector; mu = the mu of that
// scaling).  launch_genpow_length writes one partial per cone to `part`, which launch_step3_length(..., ngp) expects behind its own
// step3_length_parts(nexp, npow) entries; launch_genpow_barrier writes nalpha <= step3_max_candidates() partials per cone (stride 8) to
// cpart = step3_barrier_gppart(work, nsoc, nexp + npow), which launch_step3_barrier(..., ngp) adds to the cone set's barrier
int step3_length_parts(int nexp, int npow);
double *step3_barrier_gppart(double *work, int nsoc, int n3);
void launch_genpow_copy(hipStream_t st, int ngp, const int64_t *desc, const double *src, double *out);
void launch_genpow_shift(hipStream_t st, int ngp, const int64_t *desc, const double *nsout, double sigma_mu, double *out);
void launch_genpow_mulhs(hipStream_t st, int ngp, const int64_t *desc, const double *nsout, double mu, const double *x, const double *addc,
                         double *y);
void launch_genpow_length(hipStream_t st, int ngp, const int64_t *desc, const double *alpha, const double *z, const double *s,
                          const double *dz, const double *ds, const double *sym2, const double *dtau, double tau, double kappa,
                          double rhs_kappa, double alpha_max, double step, double alpha_min, int trips, double *part);
void launch_genpow_barrier(hipStream_t st, int ngp, const int64_t *desc, const double *alpha, const double *z, const double *s,
                           const double *dz, const double *ds, const double *alphas, int nalpha, double *cpart);
// The PSD triangle cones' tables as every launcher below takes them (hipkkt_step.cpp fills one per call): tab = 4 int64 per cone
// [row0 | n | offset of the n x n factors | offset of lambda] (cone_layout.h kPsd*); R, Rinv = the cones' column-major factors
// concatenated, lam = their lambda concatenated; large = the cones of that table step_psd_large.hip serves: lidx = the nlarge cones'
// indices into tab, sides lmin .. psd_step_large_max_dim() (after hipkkt_step_enable_psd_large; lmin = 65 unless the testing switch
// PSD_LARGE_MIN says otherwise), max_n = the largest of their sides, ws = psd_large_ws_doubles(nlarge) doubles (kPsdLargeMats matrices
// of kPsdLargeMatDoubles per large cone).  A launcher reads the fields its operation needs; the default start needs npsd and tab only.
constexpr int kPsdLargeMaxN = 128;                                           // HIPKKT_PSD_STEP_LARGE_MAX_DIM
constexpr int kPsdLargeMats = 4;
constexpr int kPsdLargeMatDoubles = kPsdLargeMaxN * kPsdLargeMaxN;
struct PsdLargeBatch { int nlarge = 0; const int *lidx = nullptr; int lmin = 65, max_n = 0; double *ws = nullptr; };
struct PsdView {
    int npsd = 0;
    const int64_t *tab = nullptr;
    const double *R = nullptr, *Rinv = nullptr, *lam = nullptr;
    PsdLargeBatch large;
};
// step_psd.hip: the same operations on the rows of the PSD triangle cones after hipkkt_step_enable_psd, one workgroup per cone
// (step length: per cone and per z / s), sides <= psd_step_max_dim().  The step length has two halves:
// launch_psd_step_length_cones writes one (alpha_z, alpha_s) pair per cone to `part` (a cone the kernels do not serve gets alpha_max),
// launch_psd_step_length_final writes out2 = the minimum of those pairs and of sym2, the pair launch_step_length left for the Zero /
// Nonnegative / SecondOrder rows; step_psd_large.hip writes its cones' pairs between the two.  launch_psd_step_check sets *fail when
// a lambda is not finite or not positive.
int psd_step_max_dim();
void launch_psd_step_affine_ds(hipStream_t st, const PsdView &P, double *out);
void launch_psd_step_mulhs(hipStream_t st, const PsdView &P, const double *x, const double *addc, double *y);
void launch_psd_step_shift(hipStream_t st, const PsdView &P, const double *dz, const double *ds, double sigma_mu, double *out);
void launch_psd_step_offset(hipStream_t st, const PsdView &P, const double *ds, double *out);
void launch_psd_step_length_cones(hipStream_t st, const PsdView &P, const double *dz, const double *ds, double alpha_max, double *part);
void launch_psd_step_length_final(hipStream_t st, int npsd, const double *sym2, const double *part, double *out2);
void launch_psd_step_check(hipStream_t st, const double *lam, int64_t len, int *fail);
// step_psd_large.hip: the same operations for the cones of P.large, matrices in global memory: products as batched 16 x 16 tile
// launches, the Jacobi iteration of the step length with M alone in LDS.  Same arithmetic as step_psd.hip -- applied to a side <= 64
// the same bits.  launch_psd_large_length writes its cones' pairs to part[2 c + (0 | 1)] and belongs between the two halves above.
// With P.large.nlarge == 0 none of them launches anything.
int psd_step_large_max_dim();
int64_t psd_large_ws_doubles(int nlarge);
void launch_psd_large_affine_ds(hipStream_t st, const PsdView &P, double *out);
void launch_psd_large_mulhs(hipStream_t st, const PsdView &P, const double *x, const double *addc, double *y);
void launch_psd_large_shift(hipStream_t st, const PsdView &P, const double *dz, const double *ds, double sigma_mu, double *out);
void launch_psd_large_offset(hipStream_t st, const PsdView &P, const double *ds, double *out);
void launch_psd_large_length(hipStream_t st, const PsdView &P, const double *dz, const double *ds, double alpha_max, double *part);
// scaling_psd.hip: update_scaling!(::PSDTriangleCone) for the cones of the same table, one workgroup per cone: Cholesky factors of
// svec_to_mat of the cone's rows of (s, z), the SVD of L2' L1 by one-sided Jacobi sweeps, (R, Rinv, lam) written in the layout above.
// A cone that fails sets *fail and bad[cone] (0 otherwise) and gets NaN factors.  A cone of side above min(max_side,
// psd_step_max_dim()) is left alone.
void launch_psd_nt_scaling(hipStream_t st, int npsd, const int64_t *tab, const double *s, const double *z, double *R, double *Rinv,
                           double *lam, int *bad, int *fail, int max_side);
// scaling_psd_large.hip: the same for the cones of P.large (hipkkt_psd_scaling_enable_large), one workgroup of 512 threads per cone,
// one matrix in LDS and the cone's four workspace matrices of P.large.ws; the same arithmetic -- applied to a side <= 64 the same
// bits.  launch_psd_nt_scaling gets max_side = P.large.lmin - 1 in the same call, so each cone is computed by one of the two.
void launch_psd_large_nt_scaling(hipStream_t st, const PsdView &P, const double *s, const double *z, double *R, double *Rinv,
                                 double *lam, int *bad, int *fail);
// barrier_psd.hip: compute_barrier of the PSD triangle cones of the same table (sides <= psd_step_max_dim()) at nalpha <=
// step3_max_candidates() step lengths (host array), for a cone set that holds PSD cones next to non-symmetric ones
// (hipkkt_step_enable_mixed).  launch_psd_barrier leaves [(0 - logdet(Z + a dZ)) | logdet(S + a dS)] per (cone, candidate) in slots =
// psd_barrier_slots(work, nsoc, n3, ngp), 16 doubles per PSD cone of the work buffer of launch_step3_barrier; launch_psd_barrier_add,
// behind launch_step3_barrier on the same stream, adds the cones' (0 - logdet_z) - logdet_s in PSD-cone order to out[2 j].  A shifted
// point outside the cone gives -Inf (the reference subtracts typemax).  launch_psd_barrier_large (hipkkt_step_enable_mixed_large),
// behind launch_psd_barrier on the same stream, overwrites the slots of the cones of P.large (sides up to psd_step_large_max_dim(),
// one 128 x 129 matrix in LDS; the same arithmetic -- applied to a side <= 64 the same bits), for which the first left the failure
// arm; with P.large.nlarge == 0 it launches nothing.
double *psd_barrier_slots(double *work, int nsoc, int n3, int ngp);
void launch_psd_barrier(hipStream_t st, const PsdView &P, const double *z, const double *s, const double *dz, const double *ds,
                        const double *alphas, int nalpha, double *slots);
void launch_psd_barrier_large(hipStream_t st, const PsdView &P, const double *z, const double *s, const double *dz, const double *ds,
                              const double *alphas, int nalpha, double *slots);
void launch_psd_barrier_add(hipStream_t st, int npsd, const double *slots, int nalpha, double *out);
// start.hip: the default start of a symmetric cone set (solver.jl:383-405) on the tables above (P: its npsd and tab).
// launch_start_identity writes the identity scaling's Hs values and sparse second-order terms into kval (psd_hs0 = first Hs entry per
// PSD cone, psd_max_numel = the largest numel among them).  launch_start_margins leaves, for each of nsides vectors (v1 is not read
// when nsides == 1), the record {min_margin, pos_margin, target, branch, a, b, two_stage, 0} at start_decision(work, ncones) + 8 side;
// work has start_work_doubles(ncones) doubles, degree = the cone set's degree.  launch_start_shift applies scaled_unit_shift! twice
// (a, then b when two_stage) to v0 / v1 in place, pd 0 primal (Zero rows become 0) / 1 dual (Zero rows stay).
// launch_start_rhs: mode 1 [0; b; 0], mode 2 [-q; 0; 0].  launch_start_assemble: xzs = [x | z | s] from the solutions sa, sb
// (sb == NULL: z = sa.z, s = -z; otherwise s = -sa.z, z = sb.z).
// psd_large (hipkkt_step_default_start_enable_psd_large): the margins of the cones of P.large come from a second launch with one
// 128 x 129 matrix in LDS behind the first, and the shift serves PSD sides up to psd_step_large_max_dim(); without it both are the
// launches of a handle whose sides are all <= psd_step_max_dim().
int64_t start_work_doubles(int64_t ncones);
double *start_decision(double *work, int64_t ncones);
void launch_start_identity(hipStream_t st, const signed char *row_kind, const int64_t *row_hs, const int64_t *map_hs, int nsoc,
                           const int64_t *desc, double *soc_u, double *soc_v, double *soc_eta2, const PsdView &P,
                           const int64_t *psd_hs0, int64_t psd_max_numel, double *kval, int64_t m);
void launch_start_margins(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, const PsdView &P, const double *v0,
                          const double *v1, int nsides, double degree, double *work, int64_t ncones, int64_t m, bool psd_large);
void launch_start_shift(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, const PsdView &P, const double *dec,
                        double *v0, int pd0, double *v1, int pd1, int nsides, int64_t m, bool psd_large);
void launch_start_rhs(hipStream_t st, double *dst, const double *qb, int n, int nm, int N, int mode);
void launch_start_assemble(hipStream_t st, double *xzs, const double *sa, const double *sb, int64_t n, int64_t m);
}  // namespace hipkkt
