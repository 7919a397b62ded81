// The cone algebra of an interior-point step on the device (step.hip) and its fusion with the reduced solve of hipkkt_solve.cpp:
// hipkkt_cone_* (one operation each, host pointers), hipkkt_set_equilibration, hipkkt_step_* (everything resident, scalars only cross
// PCIe).  Zero, Nonnegative and SecondOrder cones; they work on the (s, z, w, lambda, eta) of the last successful hipkkt_update_scaling.
// After hipkkt_step_enable_cone3 also the Exponential / Power cones of the registration (step_cone3.hip), on the (s, z) and the
// [Hs | H_dual | grad] that hipkkt_update_scaling_ex[_dev] left resident; then hipkkt_cone_barrier / hipkkt_step_barrier_dev as well.
// After hipkkt_step_enable_genpow the Generalized Power cones too (step_genpow.hip), on their slot [grad | d1 | d2 | p | q | r].
// After hipkkt_step_enable_psd the PSD triangle cones of a symmetric registration (step_psd.hip), on the caller's (R, Rinv, lambda);
// after hipkkt_step_enable_psd_large those of side 65 .. 128 as well (step_psd_large.hip).
// After hipkkt_step_enable_mixed PSD triangle cones (sides <= 64) next to Exponential / Power / Generalized Power cones: the launches of
// the families above composed, plus the PSD cones' barrier (barrier_psd.hip); after hipkkt_step_enable_mixed_large sides 65 .. 128 too.
// The default start of a symmetric cone set (start.hip): hipkkt_cone_set_identity_scaling / _margins / _shift_to_interior and the fused
// hipkkt_step_default_start_dev, which need no scaling.
#include "hipkkt_internal.h"

#pragma clang fp contract(off)      // the scalars below repeat the caller's expressions (variables.jl:14-43, :124-162) rounding by rounding

namespace hipkkt_host {

// the cone set and its scaling allow the step entry points
static bool step_ready(hipkkt_solver *S, const char *who) {
    const ConeState &C = S->cones;
    if (!S->l1 || !C.reg.ready || C.step.mode == StepMode::Off) {
        S->err = std::string(who) + ": needs an L1 handle whose registered cones are Zero / Nonnegative / SecondOrder only, or one with "
                                    "Exponential / Power cones next to them after hipkkt_step_enable_cone3, or with Generalized Power cones "
                                    "after hipkkt_step_enable_genpow, or with PSD triangle cones after hipkkt_step_enable_psd[_large], or with PSD "
                                    "triangle cones next to Exponential / Power / Generalized Power cones after hipkkt_step_enable_mixed[_large]";
        return false;
    }
    if (!C.step.scaled) { S->err = std::string(who) + ": no successful hipkkt_update_scaling since the cones were registered"; return false; }
    return true;
}

static void ensure_step_buffers(hipkkt_solver *S) {
    ConeState &C = S->cones;
    if (C.step.step) return;
    const int64_t n = S->img.n, m = S->img.m;
    const int64_t pairs = step_len_pairs(m, (int)S->cone_numel.size());      // (a later registration has at most this many cones)
    C.step.step = S->dalloc<double>(n + 2 * m);
    C.step.in = S->dalloc<double>(2 * n + m);
    C.step.work = S->dalloc<double>(4 * m);
    C.step.part = S->dalloc<double>((size_t)std::max<int64_t>(2 * pairs, step_norm_part_doubles()));
    C.step.out = S->dalloc<double>(kStOutDoubles);      // step lengths, norms, barrier results, the parked symmetric pair (cone_layout.h)
    C.step.bar = S->dalloc<double>((size_t)step3_barrier_doubles((int64_t)S->cone_numel.size()));
    C.step.start = S->dalloc<double>((size_t)start_work_doubles((int64_t)S->cone_numel.size()));
}

struct ConeTables {
    StepMode mode = StepMode::Off;
    const signed char *kind = nullptr; int nsoc = 0; const int64_t *desc = nullptr;
    const double *s = nullptr, *z = nullptr, *w = nullptr, *lam = nullptr, *eta = nullptr;
    int64_t m = 0;
    // Cone3 / GenPow: the Exponential / Power cones, tables [Exponential | Power], the scaling's output vector
    int nexp = 0, npow = 0, n3 = 0;
    const int64_t *row0 = nullptr, *out0 = nullptr;
    const double *alpha = nullptr, *nsout = nullptr;
    // GenPow: the Generalized Power cones' descriptors, exponents, the mu of the last scaling
    int ngp = 0;
    const int64_t *gpdesc = nullptr;
    const double *gpalpha = nullptr;
    double mu = 0.0;
    // Psd / Mixed: the PSD triangle cones' table and factors, and those of them step_psd_large.hip serves (hipkkt_step_enable_psd_large,
    // hipkkt_step_enable_mixed_large; none otherwise: no side above 64)
    PsdView psd;
    // the backtracking line search of the non-symmetric cones decides the step length
    bool line_search() const { return mode == StepMode::Cone3 || mode == StepMode::GenPow || mode == StepMode::Mixed; }
};
static ConeTables tables(hipkkt_solver *S) {
    const ConeState &C = S->cones;
    ConeTables T;
    T.mode = C.step.mode;
    T.m = S->img.m;
    T.kind = C.tab.kind; T.nsoc = C.reg.nsoc; T.desc = C.tab.socdesc;
    T.s = C.tab.sz; T.z = C.tab.sz + T.m; T.w = C.tab.wl; T.lam = C.tab.wl + T.m; T.eta = C.tab.eta;
    if (T.mode == StepMode::Psd || T.mode == StepMode::Mixed) {
        T.psd.npsd = (int)C.reg.psd_n.size(); T.psd.tab = C.tab.psdtab; T.psd.R = C.tab.R; T.psd.Rinv = C.tab.psd_rinv; T.psd.lam = C.tab.psd_lam;
        if (C.step.psd_nlarge > 0) T.psd.large = PsdLargeBatch{C.step.psd_nlarge, C.tab.psd_lidx, C.step.psd_lmin, C.step.psd_lmax, C.tab.psd_ws};
    }
    switch (T.mode) {
        case StepMode::Off:
        case StepMode::Symmetric:
        case StepMode::Psd:
            break;
        case StepMode::Mixed:      // every non-symmetric field
        case StepMode::GenPow:
            T.ngp = C.reg.ngenpow; T.gpdesc = C.tab.gpdesc; T.gpalpha = C.tab.gpalpha; T.mu = C.step.mu;
            [[fallthrough]];      // and the three-row members of the set
        case StepMode::Cone3:
            T.nexp = C.reg.nexp; T.npow = C.reg.npow; T.n3 = T.nexp + T.npow;
            T.row0 = C.tab.row0; T.out0 = C.tab.out0; T.alpha = C.tab.alpha; T.nsout = C.tab.nsout;
            break;
    }
    return T;
}

// every operation: the kernels of step.hip on the Zero / Nonnegative / SecondOrder rows (unchanged), then the Exponential / Power rows,
// then the Generalized Power rows, then the PSD rows (a launcher skips an empty family; only a Mixed set has both non-symmetric and PSD
// members): step_psd.hip leaves a cone of side > 64 alone, step_psd_large.hip computes it
static void op_affine_ds(hipStream_t st, const ConeTables &T, double *out) {
    launch_step_affine_ds(st, T.kind, T.nsoc, T.desc, T.lam, out, T.m);
    launch_step3_copy(st, T.n3, T.row0, T.s, out);
    launch_genpow_copy(st, T.ngp, T.gpdesc, T.s, out);
    launch_psd_step_affine_ds(st, T.psd, out);
    launch_psd_large_affine_ds(st, T.psd, out);
}
static void op_shift(hipStream_t st, const ConeTables &T, const double *dz, const double *ds, double sigma_mu, double *out) {
    launch_step_shift(st, T.kind, T.nsoc, T.desc, T.w, T.eta, dz, ds, sigma_mu, out, T.m);
    if (T.n3) launch_step3_shift(st, T.nexp, T.npow, T.row0, T.out0, T.alpha, T.nsout, T.z, dz, ds, sigma_mu, out);
    launch_genpow_shift(st, T.ngp, T.gpdesc, T.nsout, sigma_mu, out);
    launch_psd_step_shift(st, T.psd, dz, ds, sigma_mu, out);
    launch_psd_large_shift(st, T.psd, dz, ds, sigma_mu, out);
}
static void op_offset(hipStream_t st, const ConeTables &T, const double *ds, double *out) {
    launch_step_offset(st, T.kind, T.nsoc, T.desc, T.z, T.w, T.lam, T.eta, ds, out, T.m);
    launch_step3_copy(st, T.n3, T.row0, ds, out);
    launch_genpow_copy(st, T.ngp, T.gpdesc, ds, out);
    launch_psd_step_offset(st, T.psd, ds, out);
    launch_psd_large_offset(st, T.psd, ds, out);
}
static void op_mulhs(hipStream_t st, const ConeTables &T, const double *x, const double *addc, double *y) {
    launch_step_mulhs(st, T.kind, T.nsoc, T.desc, T.w, T.eta, x, addc, y, T.m);
    launch_step3_mulhs(st, T.n3, T.row0, T.out0, T.nsout, x, addc, y);
    launch_genpow_mulhs(st, T.ngp, T.gpdesc, T.nsout, T.mu, x, addc, y);
    launch_psd_step_mulhs(st, T.psd, x, addc, y);
    launch_psd_large_mulhs(st, T.psd, x, addc, y);
}
// "symmetric cones first" of a set with PSD cones (Psd, Mixed): the symmetric rows' launch as it is, its pair parked at kStOutSymPsd;
// the PSD cones' pairs follow its partials in `part` (2 (ceil(m / 256) + ncones) doubles: second-order and PSD cones together are at
// most ncones); out2 = the minimum over kinds 0..3.  step_psd.hip parks alpha_max for a cone of side > 64, step_psd_large.hip
// overwrites it before the final minimum reads it (without a list of large cones that launcher returns without a launch)
static void length_sym_psd(const ConeState::Step &St, hipStream_t st, const ConeTables &T, const double *dz, const double *ds,
                           double alpha_max, double *out2) {
    double *sym2 = St.out + kStOutSymPsd, *pairs = St.part + 2 * step_len_pairs(T.m, T.nsoc);
    launch_step_length(st, T.kind, T.nsoc, T.desc, T.z, T.s, dz, ds, alpha_max, St.part, sym2, T.m);
    launch_psd_step_length_cones(st, T.psd, dz, ds, alpha_max, pairs);
    launch_psd_large_length(st, T.psd, dz, ds, alpha_max, pairs);
    launch_psd_step_length_final(st, T.psd.npsd, sym2, pairs, out2);
}
// out2 = (alpha_z, alpha_s) of the symmetric cones; with Exponential / Power / Generalized Power cones the composite (alpha, alpha) of
// coneops_compositecone.jl:216-252, started from min(alpha_tau, alpha_kappa, 1) when dtau (device) is given (variables.jl:14-43)
static void op_length(hipkkt_solver *S, hipStream_t st, const ConeTables &T, const double *dz, const double *ds, double alpha_max,
                      const double *dtau, double tau, double kappa, double rhs_kappa, double *out2) {
    const ConeState::Step &St = S->cones.step;
    switch (T.mode) {
        case StepMode::Off:
        case StepMode::Symmetric:
            launch_step_length(st, T.kind, T.nsoc, T.desc, T.z, T.s, dz, ds, alpha_max, St.part, out2, T.m);
            break;
        case StepMode::Psd:
            length_sym_psd(St, st, T, dz, ds, alpha_max, out2);
            break;
        case StepMode::Mixed:
        case StepMode::Cone3:
        case StepMode::GenPow: {
            double *sym2 = St.out + kStOutSym;
            // "symmetric cones first" (coneops_compositecone.jl:216-252) includes the PSD cones of a Mixed set: the pair of kinds 0..3
            // goes to kStOutSym; the partials in St.part are consumed before the line search reuses it
            if (T.mode == StepMode::Mixed) length_sym_psd(St, st, T, dz, ds, alpha_max, sym2);
            else launch_step_length(st, T.kind, T.nsoc, T.desc, T.z, T.s, dz, ds, alpha_max, St.part, sym2, T.m);
            // (St.part holds 2 (ceil(m / 256) + ncones) doubles: room for the three-row workgroups' partials and one per Generalized Power cone)
            launch_genpow_length(st, T.ngp, T.gpdesc, T.gpalpha, T.z, T.s, dz, ds, sym2, dtau, tau, kappa, rhs_kappa, alpha_max,
                                 St.ls_step, St.ls_amin, St.ls_trips, St.part + step3_length_parts(T.nexp, T.npow));
            launch_step3_length(st, T.nexp, T.npow, T.row0, T.alpha, T.z, T.s, dz, ds, sym2, dtau, tau, kappa, rhs_kappa, alpha_max,
                                St.ls_step, St.ls_amin, St.ls_trips, St.part, out2, T.ngp);
            break;
        }
    }
}

// one operation on host vectors of length m: `nin` inputs are staged, op(in0, in1, out) runs, `nout` doubles come back
template <class F>
static int32_t cone_op_host(hipkkt_solver *S, const double *in0, const double *in1, double *out, int64_t nout, F &&op) {
    const int64_t m = S->img.m;
    ensure_step_buffers(S);
    S->ensure_stage(3 * m + 2 + 2 * step3_max_candidates());
    double *d0 = S->d_stage, *d1 = d0 + m, *dout = d1 + m;
    if (in0 && m) HK_CHECK(hipMemcpyAsync(d0, in0, m * sizeof(double), hipMemcpyHostToDevice, S->stream));
    if (in1 && m) HK_CHECK(hipMemcpyAsync(d1, in1, m * sizeof(double), hipMemcpyHostToDevice, S->stream));
    op(d0, d1, dout);
    copy_sync(S->stream, out, dout, (size_t)nout * sizeof(double), hipMemcpyDeviceToHost);
    if (!nout) HK_CHECK(hipStreamSynchronize(S->stream));
    return HIPKKT_OK;
}

struct StepScalars { double tau, kappa, rhs_tau, rhs_kappa; };

// the part of kkt_solve! (kktsystem.jl:135-215) both fused calls share: d_st_in holds [rhs.x | workz | variables.x], addc the constant
// term of ds.  The solve and its reduction are hipkkt_kkt_solve_reduced_dev's; ds = -(Hs dz + addc) (:203-207) and the step length of
// the cones (alpha_max = 1) are enqueued behind every reduction, so the host still synchronises once.
static int32_t fused_solve(hipkkt_solver *S, const StepScalars &sc, const double *addc, int32_t const_pending, double step_fraction,
                           double *scal_out15, const RefineOpts &ir, int64_t *ir_steps2) {
    const int64_t n = S->img.n, m = S->img.m;
    ConeState &C = S->cones;
    const ConeTables T = tables(S);
    if (solve_target(S) != S) HK_CHECK(hipStreamSynchronize(S->stream));      // the robust-order twin solves on its own stream
    static_assert(10 + 2 <= kScalRedDoubles, "the step lengths do not fit behind the ten scalars");
    double *h2 = S->h_scal_red + 10;
    const std::function<void(hipStream_t, const double *)> after = [&](hipStream_t st, const double *d_lhs) {
        double *dz = C.step.step + n, *ds = dz + m;
        HK_CHECK(hipMemcpyAsync(C.step.step, d_lhs, (size_t)(n + m) * sizeof(double), hipMemcpyDeviceToDevice, st));
        op_mulhs(st, T, dz, addc, ds);
        // (with Exponential / Power cones the line search starts from min(alpha_tau, alpha_kappa, 1): dtau is the reduction's first scalar)
        double *out2 = C.step.out + (T.line_search() ? kStOutLen : kStOutSym);
        op_length(S, st, T, dz, ds, 1.0, S->red.d + 3 * (size_t)S->N + n, sc.tau, sc.kappa, sc.rhs_kappa, out2);
        HK_CHECK(hipMemcpyAsync(h2, out2, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    };
    const double scal_in[4] = {sc.tau, sc.kappa, sc.rhs_tau, sc.rhs_kappa};
    double red[10];
    C.step.have_step = false;
    ReducedOut out;
    out.scal_out = red; out.ir_steps = ir_steps2; out.after_reduce = &after;
    const int32_t rc = kkt_solve_reduced_impl(S, ReducedIn::device(C.step.in), {scal_in, const_pending}, out, ir);
    if (rc != HIPKKT_OK) return rc;
    C.step.have_step = true;
    // variables.jl:14-43 (the cones' part ran with alpha_max = 1: the minimum is exact in any order), kktsystem.jl:209
    const double dtau = red[0];
    const double dkappa = -(sc.rhs_kappa + sc.kappa * dtau) / sc.tau;
    const double a_tau = dtau < 0.0 ? -sc.tau / dtau : 1.7976931348623157e308;
    const double a_kap = dkappa < 0.0 ? -sc.kappa / dkappa : 1.7976931348623157e308;
    double alpha = std::min(std::min(a_tau, a_kap), 1.0);
    alpha = std::min(std::min(alpha, h2[0]), h2[1]);
    alpha *= step_fraction;
    scal_out15[0] = alpha; scal_out15[1] = dtau; scal_out15[2] = dkappa; scal_out15[3] = h2[0]; scal_out15[4] = h2[1];
    memcpy(scal_out15 + 5, red, sizeof(red));
    return HIPKKT_OK;
}

}  // namespace hipkkt_host

extern "C" {

int32_t hipkkt_cone_affine_ds(hipkkt_handle h, double *ds_out) {
    HK_ENTER(h)
    if (!step_ready(S, "cone_affine_ds") || (S->img.m && !ds_out)) return HIPKKT_ERR_ARGUMENT;
    const ConeTables T = tables(S);
    return cone_op_host(S, nullptr, nullptr, ds_out, T.m, [&](double *, double *, double *out) {
        op_affine_ds(S->stream, T, out);
    });
    HK_LEAVE
}

int32_t hipkkt_cone_combined_ds_shift(hipkkt_handle h, const double *step_z, const double *step_s, double sigma_mu, double *shift_out) {
    HK_ENTER(h)
    if (!step_ready(S, "cone_combined_ds_shift") || (S->img.m && (!step_z || !step_s || !shift_out))) return HIPKKT_ERR_ARGUMENT;
    const ConeTables T = tables(S);
    return cone_op_host(S, step_z, step_s, shift_out, T.m, [&](double *dz, double *ds, double *out) {
        op_shift(S->stream, T, dz, ds, sigma_mu, out);
    });
    HK_LEAVE
}

int32_t hipkkt_cone_ds_from_dz_offset(hipkkt_handle h, const double *ds, double *out) {
    HK_ENTER(h)
    if (!step_ready(S, "cone_ds_from_dz_offset") || (S->img.m && (!ds || !out))) return HIPKKT_ERR_ARGUMENT;
    const ConeTables T = tables(S);
    return cone_op_host(S, ds, nullptr, out, T.m, [&](double *dds, double *, double *dout) {
        op_offset(S->stream, T, dds, dout);
    });
    HK_LEAVE
}

int32_t hipkkt_cone_mul_hs(hipkkt_handle h, const double *x, double *y_out) {
    HK_ENTER(h)
    if (!step_ready(S, "cone_mul_hs") || (S->img.m && (!x || !y_out))) return HIPKKT_ERR_ARGUMENT;
    const ConeTables T = tables(S);
    return cone_op_host(S, x, nullptr, y_out, T.m, [&](double *dx, double *, double *dy) {
        op_mulhs(S->stream, T, dx, nullptr, dy);
    });
    HK_LEAVE
}

int32_t hipkkt_cone_step_length(hipkkt_handle h, const double *dz, const double *ds, double alpha_max, double *alpha_out2) {
    HK_ENTER(h)
    if (!step_ready(S, "cone_step_length") || !alpha_out2 || (S->img.m && (!dz || !ds))) return HIPKKT_ERR_ARGUMENT;
    const ConeTables T = tables(S);
    return cone_op_host(S, dz, ds, alpha_out2, 2, [&](double *ddz, double *dds, double *dout) {
        op_length(S, S->stream, T, ddz, dds, alpha_max, nullptr, 0.0, 0.0, 0.0, dout);
    });
    HK_LEAVE
}

// the barrier of the cone set and the shifted <z, s> at nalpha candidates: (z, s, dz, ds) and dout are device pointers
// (without the enable T names no Exponential / Power cone: the symmetric cones' barrier).  A Mixed set: the PSD cones' slots before, their
// sum onto out[2 j] behind the two launches every set runs; a set without PSD cones executes exactly those two.  The cones of side
// 65 .. 128 (hipkkt_step_enable_mixed_large) overwrite the failure arm barrier_psd.hip's first kernel left in their slots
static void barrier_impl(hipkkt_solver *S, const ConeTables &T, const double *z, const double *s, const double *dz, const double *ds,
                         const double *alphas, int64_t nalpha, double *dout) {
    // (the work buffer has 16 doubles per registered cone for the per-cone partials: 8 per second-order, three-row and Generalized Power
    // cone, 16 per PSD cone)
    double *bar = S->cones.step.bar;
    double *psd_slots = psd_barrier_slots(bar, T.nsoc, T.n3, T.ngp);
    launch_psd_barrier(S->stream, T.psd, z, s, dz, ds, alphas, (int)nalpha, psd_slots);
    launch_psd_barrier_large(S->stream, T.psd, z, s, dz, ds, alphas, (int)nalpha, psd_slots);
    launch_genpow_barrier(S->stream, T.ngp, T.gpdesc, T.gpalpha, z, s, dz, ds, alphas, (int)nalpha, step3_barrier_gppart(bar, T.nsoc, T.n3));
    launch_step3_barrier(S->stream, T.kind, T.nsoc, T.desc, T.nexp, T.npow, T.row0, T.alpha, z, s, dz, ds, alphas, (int)nalpha, bar, dout,
                         T.m, T.ngp);
    launch_psd_barrier_add(S->stream, T.psd.npsd, psd_slots, (int)nalpha, dout);
}

// the parameter checks, the trip bound and the invalidation both enables share; the handle is in `mode` afterwards
static int32_t enable_line_search(hipkkt_solver *S, const char *who, StepMode mode, double step, double amin) {
    ConeState &C = S->cones;
    if (!(step > 0.0 && step < 1.0) || !(amin > 0.0) || !std::isfinite(amin)) {
        S->err = std::string(who) + ": 0 < linesearch_backtrack_step < 1 and min_terminate_step_length > 0";
        return HIPKKT_ERR_ARGUMENT;
    }
    // alpha0 <= 1, so alpha0 step^k < alpha_min after at most ceil(log alpha_min / log step) multiplications
    const double trips = std::ceil(std::log(amin) / std::log(step)) + 2.0;
    if (!(trips <= 4096.0)) { S->err = std::string(who) + ": the line search would need more than 4096 trips"; return HIPKKT_ERR_ARGUMENT; }
    C.step.ls_step = step; C.step.ls_amin = amin; C.step.ls_trips = (int)std::max(trips, 2.0);
    C.step.mode = mode;
    C.step.scaled = false;      // the step reads the resident (s, z) of a scaling that ran with the enable in place
    C.step.have_step = false;
    return HIPKKT_OK;
}

// enable = 0 of hipkkt_step_enable_cone3 / _genpow: Cone3 and GenPow go off, the other modes stay
static void disable_line_search(ConeState &C) {
    if (C.step.mode == StepMode::Cone3 || C.step.mode == StepMode::GenPow) C.step.mode = StepMode::Off;
}

int32_t hipkkt_step_enable_cone3(hipkkt_handle h, int32_t enable, double linesearch_backtrack_step, double min_terminate_step_length) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    if (!enable) { disable_line_search(C); return HIPKKT_OK; }
    if (!S->l1 || !C.reg.ready || C.reg.cls != ConeClass::Cone3) {
        S->err = "step_enable_cone3: needs an L1 handle whose last hipkkt_set_cone_types_ex names Zero / Nonnegative / SecondOrder / Exponential / "
                 "Power cones only, at least one of the last two";
        return HIPKKT_ERR_ARGUMENT;
    }
    return enable_line_search(S, "step_enable_cone3", StepMode::Cone3, linesearch_backtrack_step, min_terminate_step_length);
    HK_LEAVE
}

int32_t hipkkt_step_enable_genpow(hipkkt_handle h, int32_t enable, double linesearch_backtrack_step, double min_terminate_step_length) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    if (!enable) { disable_line_search(C); return HIPKKT_OK; }
    if (!S->l1 || !C.reg.ready || C.reg.cls != ConeClass::GenPow) {
        S->err = "step_enable_genpow: needs an L1 handle whose last hipkkt_set_cone_types_ex names Zero / Nonnegative / SecondOrder / Exponential / "
                 "Power / GenPower cones only, at least one GenPower";
        return HIPKKT_ERR_ARGUMENT;
    }
    return enable_line_search(S, "step_enable_genpow", StepMode::GenPow, linesearch_backtrack_step, min_terminate_step_length);
    HK_LEAVE
}

// an L1 handle whose registration is of class `cls` with every PSD side <= max_side
static bool psd_class_fits(hipkkt_solver *S, ConeClass cls, int64_t max_side) {
    const ConeState &C = S->cones;
    bool ok = S->l1 && C.reg.ready && C.reg.cls == cls;
    for (size_t c = 0; ok && c < C.reg.psd_n.size(); c++) ok = C.reg.psd_n[c] <= max_side;
    return ok;
}

// what hipkkt_step_enable_psd[_large] and hipkkt_step_enable_mixed[_large] share: the PSD cone table, the factor buffers, the list of the cones
// step_psd_large.hip serves (`large`), the invalidation; the handle is in `mode` afterwards
static void enable_psd_tables(hipkkt_solver *S, StepMode mode, bool large) {
    ConeState &C = S->cones;
    // the cone table and the factor buffers: allocated on the first call, re-used while large enough (as the d_sc_* buffers)
    const int64_t npsd = (int64_t)C.reg.psd_n.size();
    std::vector<int64_t> tab((size_t)(kPsdTab * npsd));
    int64_t foff = 0, loff = 0;
    for (int64_t c = 0; c < npsd; c++) {
        const int64_t n = C.reg.psd_n[c];
        int64_t *t = &tab[kPsdTab * c];
        t[kPsdRow0] = C.reg.psd_row[c]; t[kPsdN] = n; t[kPsdFactor0] = foff; t[kPsdLambda0] = loff;
        foff += n * n; loff += n;
    }
    if (npsd > C.tab.cap_psd_cones) {
        C.tab.psdtab = S->dalloc<int64_t>(kPsdTab * npsd); C.tab.psd_bad = S->dalloc<int>(npsd); C.tab.psd_hs0 = S->dalloc<int64_t>(npsd);
        C.tab.cap_psd_cones = npsd;
    }
    if (foff > C.tab.cap_psd_mat || loff > C.tab.cap_psd_lam) {
        C.tab.psd_rinv = S->dalloc<double>(foff); C.tab.psd_lam = S->dalloc<double>(loff); C.tab.psd_stage = S->dalloc<double>(foff + loff);
        C.tab.cap_psd_mat = foff; C.tab.cap_psd_lam = loff;
    }
    copy_sync(S->stream, C.tab.psdtab, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice);
    copy_sync(S->stream, C.tab.psd_hs0, C.reg.psd_hs.data(), (size_t)npsd * sizeof(int64_t), hipMemcpyHostToDevice);      // (the default start's identity scaling)
    // the cones of step_psd_large.hip: their indices into the table and kPsdLargeMats n x n work matrices each
    std::vector<int> lidx;
    int lmax = 0;
    const int lmin = debug_opts().psd_large_min;      // (65 for ever in the product: hipkkt_debug_set refuses there)
    for (int64_t c = 0; large && c < npsd; c++)
        if (C.reg.psd_n[c] >= lmin) { lidx.push_back((int)c); lmax = std::max(lmax, (int)C.reg.psd_n[c]); }
    if ((int64_t)lidx.size() > C.tab.cap_psd_large) {
        C.tab.psd_lidx = S->dalloc<int>(lidx.size());
        C.tab.psd_ws = S->dalloc<double>((size_t)psd_large_ws_doubles((int)lidx.size()));
        C.tab.cap_psd_large = (int64_t)lidx.size();
    }
    copy_sync(S->stream, C.tab.psd_lidx, lidx.data(), lidx.size() * sizeof(int), hipMemcpyHostToDevice);
    C.step.psd_nlarge = (int)lidx.size(); C.step.psd_lmin = lmin; C.step.psd_lmax = lmax;
    C.step.mode = mode;
    C.step.psd_fresh = false;
    C.step.psd_scaling = C.step.psd_resident = false;
    C.step.psd_large_enabled = large && mode == StepMode::Psd;
    C.step.mixed_large_enabled = large && mode == StepMode::Mixed;
    C.step.psd_scaling_large = C.step.start_psd_large = false;      // (they sit on top of this enable: every call of it clears them)
    C.step.scaled = false;      // the step reads the factors of a scaling that ran with the enable in place
    C.step.have_step = false;
}

// enable = 0 of the entry points below: `mode` goes off, the other modes stay
static void disable_psd_mode(ConeState &C, StepMode mode) {
    if (C.step.mode == mode) {
        C.step.mode = StepMode::Off; C.step.psd_scaling = C.step.psd_resident = false; C.step.psd_nlarge = 0;
        C.step.psd_large_enabled = C.step.mixed_large_enabled = C.step.psd_scaling_large = C.step.start_psd_large = false;
    }
}

// hipkkt_step_enable_psd (large = false: sides <= HIPKKT_PSD_STEP_MAX_DIM) and hipkkt_step_enable_psd_large (sides <=
// HIPKKT_PSD_STEP_LARGE_MAX_DIM; cones of side >= lmin go to step_psd_large.hip, the others to step_psd.hip as after the first)
static int32_t enable_psd_impl(hipkkt_handle h, int32_t enable, bool large) {
    HK_ENTER(h)
    if (!enable) { disable_psd_mode(S->cones, StepMode::Psd); return HIPKKT_OK; }
    if (!psd_class_fits(S, ConeClass::Psd, large ? HIPKKT_PSD_STEP_LARGE_MAX_DIM : HIPKKT_PSD_STEP_MAX_DIM)) {
        S->err = std::string(large ? "step_enable_psd_large" : "step_enable_psd") +
                 ": needs an L1 handle whose last hipkkt_set_cone_types[_ex] names Zero / Nonnegative / SecondOrder / PSD "
                 "triangle cones only, at least one PSD cone, every PSD side <= " +
                 (large ? "HIPKKT_PSD_STEP_LARGE_MAX_DIM" : "HIPKKT_PSD_STEP_MAX_DIM");
        return HIPKKT_ERR_ARGUMENT;
    }
    enable_psd_tables(S, StepMode::Psd, large);
    return HIPKKT_OK;
    HK_LEAVE
}
int32_t hipkkt_step_enable_psd(hipkkt_handle h, int32_t enable) { return enable_psd_impl(h, enable, false); }
int32_t hipkkt_step_enable_psd_large(hipkkt_handle h, int32_t enable) { return enable_psd_impl(h, enable, true); }

// PSD triangle cones next to Exponential / Power / Generalized Power cones: the tables of hipkkt_step_enable_psd[_large] and the line
// search of hipkkt_step_enable_cone3 / _genpow.  hipkkt_step_enable_mixed (large = false: sides <= HIPKKT_PSD_STEP_MAX_DIM, the barrier's
// first kernel keeps its matrix in 64 x 65 doubles of LDS) and hipkkt_step_enable_mixed_large (sides <= HIPKKT_PSD_STEP_LARGE_MAX_DIM;
// cones of side >= lmin go to step_psd_large.hip and to the barrier's second kernel)
static int32_t enable_mixed_impl(hipkkt_handle h, int32_t enable, bool large, double step, double amin) {
    HK_ENTER(h)
    if (!enable) { disable_psd_mode(S->cones, StepMode::Mixed); return HIPKKT_OK; }
    const char *who = large ? "step_enable_mixed_large" : "step_enable_mixed";
    if (!psd_class_fits(S, ConeClass::Mixed, large ? HIPKKT_PSD_STEP_LARGE_MAX_DIM : HIPKKT_PSD_STEP_MAX_DIM)) {
        S->err = std::string(who) +
                 ": needs an L1 handle whose last hipkkt_set_cone_types_ex names Zero / Nonnegative / SecondOrder / PSD "
                 "triangle / Exponential / Power / GenPower cones only, at least one PSD cone and at least one of the last three, every "
                 "PSD side <= " + (large ? "HIPKKT_PSD_STEP_LARGE_MAX_DIM" : "HIPKKT_PSD_STEP_MAX_DIM");
        return HIPKKT_ERR_ARGUMENT;
    }
    // (the parameter checks come first: a refused call leaves the handle as it was)
    const int32_t rc = enable_line_search(S, who, StepMode::Mixed, step, amin);
    if (rc != HIPKKT_OK) return rc;
    enable_psd_tables(S, StepMode::Mixed, large);
    return HIPKKT_OK;
    HK_LEAVE
}
int32_t hipkkt_step_enable_mixed(hipkkt_handle h, int32_t enable, double linesearch_backtrack_step, double min_terminate_step_length) {
    return enable_mixed_impl(h, enable, false, linesearch_backtrack_step, min_terminate_step_length);
}
int32_t hipkkt_step_enable_mixed_large(hipkkt_handle h, int32_t enable, double linesearch_backtrack_step, double min_terminate_step_length) {
    return enable_mixed_impl(h, enable, true, linesearch_backtrack_step, min_terminate_step_length);
}

// the modes whose step reads resident PSD factors (R, Rinv, lambda)
static bool psd_factors_mode(const ConeState &C) { return C.step.mode == StepMode::Psd || C.step.mode == StepMode::Mixed; }

// a handle in PSD or Mixed step mode whose registration holds a side above HIPKKT_PSD_STEP_MAX_DIM (hipkkt_step_enable_psd_large,
// hipkkt_step_enable_mixed_large): the device
// scaling of hipkkt_psd_scaling_enable (scaling_psd.hip) and the default start without its own enable (start.hip) keep their matrices
// in LDS and would leave such a cone alone
static bool psd_side_above_small(const ConeState &C) {
    if (!psd_factors_mode(C)) return false;
    for (int64_t n : C.reg.psd_n) if (n > HIPKKT_PSD_STEP_MAX_DIM) return true;
    return false;
}

static int32_t psd_set_factors_impl(hipkkt_handle h, const double *Rinv_all, const double *lambda_all, bool dev) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    if (!psd_factors_mode(C) || !Rinv_all || !lambda_all) {
        S->err = "psd_set_factors: needs hipkkt_step_enable_psd / _mixed first / null argument";
        return HIPKKT_ERR_ARGUMENT;
    }
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HK_CHECK(hipMemcpyAsync(C.tab.psd_stage, Rinv_all, (size_t)C.reg.psd_total * sizeof(double), kind, S->stream));
    HK_CHECK(hipMemcpyAsync(C.tab.psd_stage + C.reg.psd_total, lambda_all, (size_t)C.reg.psd_lam_total * sizeof(double), kind, S->stream));
    if (!dev) HK_CHECK(hipStreamSynchronize(S->stream));      // (the caller may reuse its host arrays)
    C.step.psd_fresh = true;
    return HIPKKT_OK;
    HK_LEAVE
}
int32_t hipkkt_psd_set_factors(hipkkt_handle h, const double *Rinv_all, const double *lambda_all) {
    return psd_set_factors_impl(h, Rinv_all, lambda_all, false);
}
int32_t hipkkt_psd_set_factors_dev(hipkkt_handle h, const double *Rinv_all, const double *lambda_all) {
    return psd_set_factors_impl(h, Rinv_all, lambda_all, true);
}

// the Cholesky / SVD of the PSD cones' scaling on the device (scaling_psd.hip): hipkkt_update_scaling[_ex][_dev] without psd_R
int32_t hipkkt_psd_scaling_enable(hipkkt_handle h, int32_t enable) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    if (!psd_factors_mode(C)) {
        S->err = "psd_scaling_enable: needs hipkkt_step_enable_psd / _mixed first";
        return HIPKKT_ERR_ARGUMENT;
    }
    if (psd_side_above_small(C)) {
        S->err = "psd_scaling_enable: a PSD side above HIPKKT_PSD_STEP_MAX_DIM keeps its Cholesky / SVD with the caller";
        return HIPKKT_ERR_ARGUMENT;
    }
    C.step.psd_scaling = enable != 0;
    C.step.scaled = false;      // as the other enables: the step reads the factors of a scaling that ran with this setting in place
    C.step.have_step = false;
    C.step.psd_resident = false;
    return HIPKKT_OK;
    HK_LEAVE
}

// what hipkkt_psd_scaling_enable_large and hipkkt_step_default_start_enable_psd_large require: PSD step mode through
// hipkkt_step_enable_psd_large (so the list of the large cones and their workspace exist, and no side exceeds 128); `mixed`: Mixed step
// mode through hipkkt_step_enable_mixed_large serves as well (the scaling; the start of a non-symmetric set stays with the caller)
static bool psd_large_handle(hipkkt_solver *S, const char *who, bool mixed) {
    const ConeState &C = S->cones;
    if (C.step.mode == StepMode::Psd && C.step.psd_large_enabled) return true;
    if (mixed && C.step.mode == StepMode::Mixed && C.step.mixed_large_enabled) return true;
    S->err = std::string(who) + ": needs a handle in PSD step mode through hipkkt_step_enable_psd_large" +
             (mixed ? " or in Mixed step mode through hipkkt_step_enable_mixed_large" : "") + " first";
    return false;
}

// hipkkt_psd_scaling_enable for a handle of hipkkt_step_enable_psd_large / _mixed_large: the cones of step_psd_large.hip through scaling_psd_large.hip,
// the others through scaling_psd.hip
int32_t hipkkt_psd_scaling_enable_large(hipkkt_handle h, int32_t enable) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    if (!psd_large_handle(S, "psd_scaling_enable_large", true)) return HIPKKT_ERR_ARGUMENT;
    C.step.psd_scaling_large = enable != 0;
    C.step.scaled = false;      // as hipkkt_psd_scaling_enable
    C.step.have_step = false;
    C.step.psd_resident = false;
    return HIPKKT_OK;
    HK_LEAVE
}

// the default start (start.hip) of a handle of hipkkt_step_enable_psd_large with a side above HIPKKT_PSD_STEP_MAX_DIM
int32_t hipkkt_step_default_start_enable_psd_large(hipkkt_handle h, int32_t enable) {
    HK_ENTER(h)
    if (!psd_large_handle(S, "step_default_start_enable_psd_large", false)) return HIPKKT_ERR_ARGUMENT;
    S->cones.step.start_psd_large = enable != 0;
    return HIPKKT_OK;
    HK_LEAVE
}

int32_t hipkkt_psd_get_factors(hipkkt_handle h, double *R_out, double *Rinv_out, double *lambda_out) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    if (!psd_factors_mode(C) || !C.step.psd_resident) {
        S->err = "psd_get_factors: no PSD scaling is resident (hipkkt_step_enable_psd / _mixed, then a hipkkt_update_scaling[_ex][_dev])";
        return HIPKKT_ERR_ARGUMENT;
    }
    const size_t nr = (size_t)C.reg.psd_total * sizeof(double), nl = (size_t)C.reg.psd_lam_total * sizeof(double);
    if (R_out) HK_CHECK(hipMemcpyAsync(R_out, C.tab.R, nr, hipMemcpyDeviceToHost, S->stream));
    if (Rinv_out) HK_CHECK(hipMemcpyAsync(Rinv_out, C.tab.psd_rinv, nr, hipMemcpyDeviceToHost, S->stream));
    if (lambda_out) HK_CHECK(hipMemcpyAsync(lambda_out, C.tab.psd_lam, nl, hipMemcpyDeviceToHost, S->stream));
    HK_CHECK(hipStreamSynchronize(S->stream));
    return HIPKKT_OK;
    HK_LEAVE
}

int32_t hipkkt_cone_barrier(hipkkt_handle h, const double *dz, const double *ds, const double *alphas, int64_t nalpha, double *out) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    if (!step_ready(S, "cone_barrier")) return HIPKKT_ERR_ARGUMENT;
    if (C.step.mode == StepMode::Psd) { S->err = "cone_barrier: a set with PSD triangle cones is symmetric and needs no barrier"; return HIPKKT_ERR_ARGUMENT; }
    if (!alphas || !out || nalpha < 1 || nalpha > step3_max_candidates() || (S->img.m && (!dz || !ds))) {
        S->err = "cone_barrier: 1 <= nalpha <= 8 / null argument"; return HIPKKT_ERR_ARGUMENT;
    }
    const ConeTables T = tables(S);
    return cone_op_host(S, dz, ds, out, 2 * nalpha, [&](double *ddz, double *dds, double *dout) {
        barrier_impl(S, T, T.z, T.s, ddz, dds, alphas, nalpha, dout);
    });
    HK_LEAVE
}

int32_t hipkkt_step_barrier_dev(hipkkt_handle h, const double *xzs_dev, const double *alphas, int64_t nalpha, double *out) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    if (!step_ready(S, "step_barrier_dev")) return HIPKKT_ERR_ARGUMENT;
    if (C.step.mode == StepMode::Psd) { S->err = "step_barrier_dev: a set with PSD triangle cones is symmetric and needs no barrier"; return HIPKKT_ERR_ARGUMENT; }
    if (!C.step.have_step || !xzs_dev || !alphas || !out || nalpha < 1 || nalpha > step3_max_candidates()) {
        S->err = "step_barrier_dev: no step resident / 1 <= nalpha <= 8 / null argument"; return HIPKKT_ERR_ARGUMENT;
    }
    const int64_t n = S->img.n, m = S->img.m;
    const ConeTables T = tables(S);
    ensure_step_buffers(S);
    barrier_impl(S, T, xzs_dev + n, xzs_dev + n + m, C.step.step + n, C.step.step + n + m, alphas, nalpha, C.step.out + kStOutBarrier);
    copy_sync(S->stream, out, C.step.out + kStOutBarrier, (size_t)(2 * nalpha) * sizeof(double), hipMemcpyDeviceToHost);
    return HIPKKT_OK;
    HK_LEAVE
}

int32_t hipkkt_set_equilibration(hipkkt_handle h, const double *d, const double *e) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    const int64_t n = S->img.n, m = S->img.m;
    if (!S->l1 || (n && !d) || (m && !e)) { S->err = "set_equilibration: bad arguments / not an L1 handle"; return HIPKKT_ERR_ARGUMENT; }
    // dinv = 1 ./ d, einv = 1 ./ e as problemdata.jl forms them (IEEE division: the caller's bits)
    std::vector<double> eq((size_t)(2 * n + 2 * m) + 1);
    for (int64_t i = 0; i < n; i++) { eq[i] = d[i]; eq[n + m + i] = 1.0 / d[i]; }
    for (int64_t i = 0; i < m; i++) { eq[n + i] = e[i]; eq[2 * n + m + i] = 1.0 / e[i]; }
    if (!C.step.eq) C.step.eq = S->dalloc<double>(2 * n + 2 * m);
    copy_sync(S->stream, C.step.eq, eq.data(), (size_t)(2 * n + 2 * m) * sizeof(double), hipMemcpyHostToDevice);
    return HIPKKT_OK;
    HK_LEAVE
}

int32_t hipkkt_step_affine_dev(hipkkt_handle h, const double *xzs_dev, const double *res_dev, const double *scal_in3, int32_t const_pending,
                               double *scal_out15, int32_t ir_enable, double reltol, double abstol, int64_t max_iter, double stop_ratio,
                               int64_t *ir_steps2) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    if (!step_ready(S, "step_affine_dev")) return HIPKKT_ERR_ARGUMENT;
    if (!S->res.d_qb || !xzs_dev || !res_dev || !scal_in3 || !scal_out15) { S->err = "step_affine_dev: call hipkkt_set_qb first / bad arguments"; return HIPKKT_ERR_ARGUMENT; }
    const int64_t n = S->img.n, m = S->img.m;
    ensure_step_buffers(S);
    const double tau = scal_in3[0], kappa = scal_in3[1], r_tau = scal_in3[2];
    // variables_affine_step_rhs!, variables.jl:107-121; ds_const = s (kktsystem.jl:152-156)
    launch_step_rhs(S->stream, C.step.in, xzs_dev, res_dev, nullptr, 1.0, n, m);
    const StepScalars sc{tau, kappa, r_tau, tau * kappa};
    return fused_solve(S, sc, xzs_dev + n + m, const_pending, 1.0, scal_out15, RefineOpts{ir_enable, reltol, abstol, max_iter, stop_ratio}, ir_steps2);
    HK_LEAVE
}

int32_t hipkkt_step_combined_dev(hipkkt_handle h, const double *xzs_dev, const double *res_dev, const double *scal_in9,
                                 int32_t const_pending, double *scal_out15, int32_t ir_enable, double reltol, double abstol,
                                 int64_t max_iter, double stop_ratio, int64_t *ir_steps2) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    if (!step_ready(S, "step_combined_dev")) return HIPKKT_ERR_ARGUMENT;
    if (!S->res.d_qb || !xzs_dev || !res_dev || !scal_in9 || !scal_out15) { S->err = "step_combined_dev: call hipkkt_set_qb first / bad arguments"; return HIPKKT_ERR_ARGUMENT; }
    if (!C.step.have_step) { S->err = "step_combined_dev: no affine step resident (hipkkt_step_affine_dev comes first)"; return HIPKKT_ERR_ARGUMENT; }
    const int64_t n = S->img.n, m = S->img.m;
    const double tau = scal_in9[0], kappa = scal_in9[1], r_tau = scal_in9[2], dtau_aff = scal_in9[3], dkappa_aff = scal_in9[4];
    const double sigma = scal_in9[5], mu = scal_in9[6], m_corr = scal_in9[7], step_fraction = scal_in9[8];
    const ConeTables T = tables(S);
    hipStream_t st = S->stream;
    // variables_combined_step_rhs!, variables.jl:124-162
    const double sm = sigma * mu, oms = 1.0 - sigma;
    const double rhs_kappa = -sm + m_corr * dtau_aff * dkappa_aff + tau * kappa;
    double *w_dz = C.step.work, *w_rhs_s = w_dz + m, *w_shift = w_rhs_s + m, *w_dsc = w_shift + m;
    const double *dz_aff = C.step.step + n, *ds_aff = dz_aff + m;
    if (m_corr != 1.0) { launch_step_scale(st, w_dz, dz_aff, m_corr, m); dz_aff = w_dz; }
    op_affine_ds(st, T, w_rhs_s);
    op_shift(st, T, dz_aff, ds_aff, sm, w_shift);
    launch_step_add(st, w_rhs_s, w_shift, m);                                                           // rhs.s = lambda o lambda + shift
    op_offset(st, T, w_rhs_s, w_dsc);                                                                   // kktsystem.jl:157-163
    launch_step_rhs(st, C.step.in, xzs_dev, res_dev, w_dsc, oms, n, m);
    const StepScalars sc{tau, kappa, oms * r_tau, rhs_kappa};
    return fused_solve(S, sc, w_dsc, const_pending, step_fraction, scal_out15, RefineOpts{ir_enable, reltol, abstol, max_iter, stop_ratio}, ir_steps2);
    HK_LEAVE
}

int32_t hipkkt_step_apply_dev(hipkkt_handle h, double alpha, double *xzs_dev) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    if (!step_ready(S, "step_apply_dev")) return HIPKKT_ERR_ARGUMENT;
    if (!C.step.have_step || !xzs_dev) { S->err = "step_apply_dev: no step resident / null iterate"; return HIPKKT_ERR_ARGUMENT; }
    launch_step_add_step(S->stream, xzs_dev, C.step.step, alpha, S->img.n + 2 * S->img.m);
    // (no host synchronisation: whatever reads the iterate next runs on the same stream)
    return HIPKKT_OK;
    HK_LEAVE
}

int32_t hipkkt_step_info_norms_dev(hipkkt_handle h, const double *xzs_dev, const double *res_dev, double *out8) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    if (!S->l1 || !C.step.eq || !xzs_dev || !res_dev || !out8) { S->err = "step_info_norms_dev: call hipkkt_set_equilibration first / bad arguments"; return HIPKKT_ERR_ARGUMENT; }
    ensure_step_buffers(S);      // (needs no scaling: the first info_update! of a solve precedes it)
    launch_step_info_norms(S->stream, xzs_dev, res_dev, C.step.eq, C.step.part, C.step.out + kStOutNorms, S->img.n, S->img.m);
    copy_sync(S->stream, out8, C.step.out + kStOutNorms, 8 * sizeof(double), hipMemcpyDeviceToHost);
    return HIPKKT_OK;
    HK_LEAVE
}

int32_t hipkkt_step_get(hipkkt_handle h, double *out) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    if (!S->l1 || !C.step.have_step || !out) { S->err = "step_get: no step resident"; return HIPKKT_ERR_ARGUMENT; }
    copy_sync(S->stream, out, C.step.step, (size_t)(S->img.n + 2 * S->img.m) * sizeof(double), hipMemcpyDeviceToHost);
    return HIPKKT_OK;
    HK_LEAVE
}

// ---- the default start of a symmetric cone set (solver.jl:383-405; start.hip) ------------------------------------------------------
// served: L1 handles in step mode Symmetric (kinds 0..2) or Psd (kinds 0..3 after hipkkt_step_enable_psd; a side above 64 after
// hipkkt_step_default_start_enable_psd_large); needs no scaling
static bool start_ready(hipkkt_solver *S, const char *who) {
    const ConeState &C = S->cones;
    if (!S->l1 || !C.reg.ready || (C.step.mode != StepMode::Symmetric && C.step.mode != StepMode::Psd)) {
        S->err = std::string(who) + ": needs an L1 handle whose registered cones are Zero / Nonnegative / SecondOrder only, or one with PSD "
                                    "triangle cones next to them after hipkkt_step_enable_psd";
        return false;
    }
    if (psd_side_above_small(C) && !C.step.start_psd_large) {
        S->err = std::string(who) + ": a PSD side above HIPKKT_PSD_STEP_MAX_DIM keeps the default start with the caller "
                                    "(hipkkt_step_default_start_enable_psd_large lifts that up to HIPKKT_PSD_STEP_LARGE_MAX_DIM)";
        return false;
    }
    return true;
}

// set_identity_scaling! + get_Hs! + the Hs / sparse-cone part of _kktsolver_update_inner! (kktsolver_directldl.jl:197-245), enqueued
static void start_identity(hipkkt_solver *S) {
    ConeState &C = S->cones;
    const ConeTables T = tables(S);
    int64_t max_numel = 0;
    if (T.psd.npsd) for (int64_t n : C.reg.psd_n) max_numel = std::max(max_numel, n * (n + 1) / 2);
    launch_start_identity(S->stream, C.tab.kind, C.tab.rowhs, S->d_mapHs, T.nsoc, T.desc, S->soc.d_u, S->soc.d_v, S->soc.d_eta2, T.psd,
                          C.tab.psd_hs0, max_numel, S->dp.kval, T.m);
    if (S->soc.n > 0)      // u, v, D entries of the sparse cones (the same kernel hipkkt_set_soc_batch uses)
        launch_soc_batch(S->stream, S->dp.kval, S->soc.d_uidx, S->soc.d_vidx, S->soc.d_cone, S->soc.d_u, S->soc.d_v, S->soc.d_eta2,
                         S->soc.total, S->soc.d_didx, S->soc.n);
    // the resident (w, lambda, eta, R, Rinv) belong to another scaling than K now: the step calls wait for the next hipkkt_update_scaling*
    C.step.scaled = false;
    C.step.psd_resident = false;
    C.step.have_step = false;
    S->red.have_const = false;
}

// margins (and the shift when `shift`) of one host vector: nout doubles of its decision record come back
static int32_t start_host_op(hipkkt_solver *S, double *v, int32_t pd, bool shift, double *out, int nout) {
    ConeState &C = S->cones;
    const ConeTables T = tables(S);
    const int64_t m = T.m, ncones = (int64_t)S->cone_numel.size();
    ensure_step_buffers(S);
    S->ensure_stage(m);
    double *dv = S->d_stage, *dec = start_decision(C.step.start, ncones);
    if (m) HK_CHECK(hipMemcpyAsync(dv, v, m * sizeof(double), hipMemcpyHostToDevice, S->stream));
    const bool large = C.step.start_psd_large;
    launch_start_margins(S->stream, T.kind, T.nsoc, T.desc, T.psd, dv, nullptr, 1, (double)C.reg.degree, C.step.start, ncones, m, large);
    if (shift) {
        launch_start_shift(S->stream, T.kind, T.nsoc, T.desc, T.psd, dec, dv, pd, nullptr, 0, 1, m, large);
        if (m) HK_CHECK(hipMemcpyAsync(v, dv, m * sizeof(double), hipMemcpyDeviceToHost, S->stream));
    }
    copy_sync(S->stream, out, dec, (size_t)nout * sizeof(double), hipMemcpyDeviceToHost);
    return HIPKKT_OK;
}

int32_t hipkkt_cone_set_identity_scaling(hipkkt_handle h) {
    HK_ENTER(h)
    if (!start_ready(S, "cone_set_identity_scaling")) return HIPKKT_ERR_ARGUMENT;
    start_identity(S);
    HK_CHECK(hipStreamSynchronize(S->stream));
    return HIPKKT_OK;
    HK_LEAVE
}

int32_t hipkkt_cone_margins(hipkkt_handle h, const double *v, int32_t pd, double *out2) {
    HK_ENTER(h)
    if (!start_ready(S, "cone_margins")) return HIPKKT_ERR_ARGUMENT;
    if ((pd != 0 && pd != 1) || !out2 || (S->img.m && !v)) { S->err = "cone_margins: pd is 0 (primal) or 1 (dual) / null argument"; return HIPKKT_ERR_ARGUMENT; }
    return start_host_op(S, const_cast<double *>(v), pd, false, out2, 2);
    HK_LEAVE
}

int32_t hipkkt_cone_shift_to_interior(hipkkt_handle h, double *v, int32_t pd, double *out4) {
    HK_ENTER(h)
    if (!start_ready(S, "cone_shift_to_interior")) return HIPKKT_ERR_ARGUMENT;
    if ((pd != 0 && pd != 1) || !out4 || (S->img.m && !v)) { S->err = "cone_shift_to_interior: pd is 0 (primal) or 1 (dual) / null argument"; return HIPKKT_ERR_ARGUMENT; }
    return start_host_op(S, v, pd, true, out4, 4);
    HK_LEAVE
}

int32_t hipkkt_step_default_start_dev(hipkkt_handle h, double *xzs_dev, int32_t static_reg_enable, double eps_const, double eps_prop,
                                      int32_t ir_enable, double reltol, double abstol, int64_t max_iter, double stop_ratio,
                                      double *scal_out8, int64_t *ir_steps2) {
    HK_ENTER(h)
    ConeState &C = S->cones;
    if (!start_ready(S, "step_default_start_dev")) return HIPKKT_ERR_ARGUMENT;
    if (!S->res.d_qb || !xzs_dev || !scal_out8) { S->err = "step_default_start_dev: call hipkkt_set_qb first / bad arguments"; return HIPKKT_ERR_ARGUMENT; }
    const int64_t n = S->img.n, m = S->img.m, ncones = (int64_t)S->cone_numel.size();
    const int nm = (int)(n + m);
    ensure_step_buffers(S);
    for (int k = 0; k < 8; k++) scal_out8[k] = 0.0;
    if (ir_steps2) ir_steps2[0] = ir_steps2[1] = 0;
    // kkt_update! of the identity scaling (kktsystem.jl:62-78): hipkkt_refactor's code path, twin included; it synchronises
    start_identity(S);
    double eps = 0.0;
    int64_t nreg = 0;
    int32_t rc = hipkkt_refactor(h, static_reg_enable, eps_const, eps_prop, &eps, &nreg);
    scal_out8[0] = eps; scal_out8[1] = (double)nreg;
    if (rc != HIPKKT_OK) return rc;
    // kkt_solve_initial_point! (kktsystem.jl:95-132): structural nnz(P) != 0 one solve of [-q; b] for (x, z), s = -z; otherwise
    // [0; b] for (x, -s) and [-q; 0] for z on the two solve contexts
    const ConeTables T = tables(S);
    hipkkt_solver *F = solve_target(S);
    const bool pair = S->img.nnzP == 0, large = C.step.start_psd_large;
    double *sa = C.step.step, *sb = C.step.in;      // (n + m doubles of each are used)
    if (pair) {
        launch_start_rhs(F->ctx[0].stream, F->ctx[0].d_b, S->res.d_qb, (int)n, nm, F->N, 1);
        launch_start_rhs(F->ctx[1].stream, F->ctx[1].d_b, S->res.d_qb, (int)n, nm, F->N, 2);
    } else {
        launch_const_rhs(F->ctx[0].stream, F->ctx[0].d_b, S->res.d_qb, (int)n, nm, F->N);
    }
    // variables_symmetric_initialization! (variables.jl:167-208) behind the solves, read back with their synchronisation
    double *dec = start_decision(C.step.start, ncones), *h16 = S->h_scal_red;
    static_assert(2 * 8 <= kScalRedDoubles, "the two decision records do not fit the pinned read-back area");
    double *s_dev = xzs_dev + n + m, *z_dev = xzs_dev + n;
    const std::function<void(hipStream_t)> after = [&](hipStream_t st) {
        launch_start_assemble(st, xzs_dev, sa, pair ? sb : nullptr, n, m);
        launch_start_margins(st, T.kind, T.nsoc, T.desc, T.psd, s_dev, z_dev, 2, (double)C.reg.degree, C.step.start, ncones, m, large);
        launch_start_shift(st, T.kind, T.nsoc, T.desc, T.psd, dec, s_dev, 0, z_dev, 1, 2, m, large);
        HK_CHECK(hipMemcpyAsync(h16, dec, 2 * 8 * sizeof(double), hipMemcpyDeviceToHost, st));
    };
    double *outs[kNumCtx] = {sa, sb};
    int64_t steps[kNumCtx] = {0, 0};
    rc = solve_many(S, F, pair ? 2 : 1, RefineOpts{ir_enable, reltol, abstol, max_iter, stop_ratio}, steps, outs, nm, &after);
    if (ir_steps2) { ir_steps2[0] = steps[0]; ir_steps2[1] = steps[1]; }
    if (rc != HIPKKT_OK) return rc;
    for (int k = 0; k < 3; k++) { scal_out8[2 + k] = h16[k]; scal_out8[5 + k] = h16[8 + k]; }
    return HIPKKT_OK;
    HK_LEAVE
}

}  // extern "C"
