// LDL solves on a solve context, iterative refinement decided on the device, recovery from a sweep time-out, and the solve entry
// points of the C ABI (see hipkkt_internal.h for the file map).
#include "hipkkt_internal.h"

using namespace hipkkt;
using namespace hipkkt_host;

namespace hipkkt_host {

// in -> out (original ordering on both sides) on context C
static void enqueue_ldl_solve(hipkkt_solver *S, SolveCtx &C, const double *in, double *out, int *zero = nullptr, int nzero = 0) {
    const HostPlan &P = S->plan;
    const SolveSchedule &H = S->sched;
    hipStream_t st = C.stream;
    const DevPlan &D = C.dp;
    launch_permute_in(st, in, D.perm, C.d_y, S->N, D.seg_epoch, D.seg_sync, 2 * H.nseg, zero, nzero);
    // one launch per level (wide bottom levels, and every level on the fallback path: no persistent kernel at all, level lists
    // over every supernode); the leaves of such a level take the thread-per-supernode kernels
    const LevelLists &L = S->persist.use ? H.regular : H.all;
    auto fwd_level = [&](int l) {
        launch_fwd_narrow(st, D, L.reg_ptr[l], L.nnarrow[l], L.wnarrow[l], C.d_y, C.d_z);
        launch_fwd_level(st, D, L.slv_ptr[l], L.slv_ptr[l + 1] - L.slv_ptr[l], C.d_y, C.d_z);
    };
    auto bwd_level = [&](int l) {
        launch_bwd_partial(st, D, L.bwd_ptr[l], L.bwd_ptr[l + 1] - L.bwd_ptr[l], C.d_xp);
        launch_bwd_final(st, D, L.reg_ptr[l] + L.nnarrow[l], L.reg_ptr[l + 1] - L.reg_ptr[l] - L.nnarrow[l], C.d_z, C.d_xp, out);
        launch_bwd_narrow(st, D, L.reg_ptr[l], L.nnarrow[l], L.wnarrow[l], C.d_z, C.d_xp, out);
    };
    if (S->persist.use) {
        // one persistent launch per segment of regular levels, front kernels in between
        for (int g = 0; g < H.nseg; g++) {
            for (int l = H.seg_lo[g]; l < std::min(H.seg_lstar[g], H.seg_hi[g] + 1); l++) fwd_level(l);   // wide bottom levels
            launch_fwd_seg(st, D, g, H.fseg_ptr[2 * g], H.fseg_ptr[2 * g + 1] - H.fseg_ptr[2 * g], P.nsuper, C.d_y, C.d_z);
            for (const FrontDesc &F : P.fronts)
                if (H.seg_of_level[F.level_last] == g) launch_front_fwd(st, D, F, C.d_y, C.d_z);
        }
        bool first = true;    // the first backward launch of a solve re-arms the forward sweeps' counters
        for (int g = H.nseg - 1; g >= 0; g--) {
            for (const FrontDesc &F : P.fronts)
                if (H.seg_of_level[F.level_last] == g) launch_front_bwd(st, D, F, C.d_z, C.d_xp, out);
            const int k = H.nseg - 1 - g;     // launch order index
            const int n = H.bseg_ptr[k + 1] - H.bseg_ptr[k];
            if (n > 0) { launch_bwd_seg(st, D, g, H.bseg_ptr[k], n, P.nsuper, first ? 1 : 0, C.d_z, C.d_xp, out); first = false; }
            for (int l = std::min(H.seg_lstar[g], H.seg_hi[g] + 1) - 1; l >= H.seg_lo[g]; l--) bwd_level(l);
        }
        return;
    }
    for (int l = 0; l < P.nlevels; l++) fwd_level(l);
    for (int l = P.nlevels - 1; l >= 0; l--) bwd_level(l);
}

static void invalidate_solve_graphs(SolveCtx &C) { C.g_ldl.valid = C.g_first.valid = C.g_step.valid = false; }

// the downgrade to per-level kernels after a sweep time-out is temporary
// (hipkkt_reset_timing zeroes the LDL-solve count that retry_at is measured against: a reset postpones the retry)
static void maybe_retry_persistent(hipkkt_solver *S) {
    PersistState &ps = S->persist;
    if (!ps.use && ps.allowed && ps.retry_at >= 0 && S->stats.n_ldlsolves >= ps.retry_at) {
        ps.use = true;
        ps.retry_at = -1;
        for (SolveCtx &C : S->ctx) invalidate_solve_graphs(C);
    }
}

// one refinement step on the device: correction solve, candidate = iterate + correction, its residual, the decision
static void enqueue_refine_step(hipkkt_solver *S, SolveCtx &C, const RefineOpts &ir) {
    hipStream_t st = C.stream;
    enqueue_ldl_solve(S, C, C.d_e, C.d_corr, (int *)(C.dp.scal + SC_NORME), 2);   // (||e|| of the candidate starts from zero)
    launch_refine_add(st, C.d_rs, C.d_x0, C.d_x1, C.d_corr, S->N);
    launch_spmv_residual(st, C.dp, C.d_b, C.d_rs, C.d_x0, C.d_x1, C.d_e, S->N, (unsigned long long *)C.dp.scal + SC_NORME);
    launch_refine_decide(st, C.d_rs, C.dp.scal, 1, ir.reltol, ir.abstol, (int)std::min<int64_t>(ir.max_iter, 1 << 30), ir.stop_ratio);
}

// bit 0: a front sweep / forward segment sweep gave up, bit 2: the backward segment sweep gave up
static inline bool sweep_failed(const SolveCtx &C) {
    if (C.h_flags[FL_FRONTFAIL] & ~7) {   // never written by this library (seen once: a small memset node of a captured
                                           // graph wrote garbage under rocprofv3): report it, do not act on it
        static bool told = false;
        if (!told)
            fprintf(stderr, "hipkkt: unexpected value in the flag words: %x %x %x %x\n", C.h_flags[0], C.h_flags[1], C.h_flags[2], C.h_flags[3]);
        told = true;
    }
    return (C.h_flags[FL_FRONTFAIL] & 7) != 0;
}

// A persistent sweep kernel gave up (bounded spin expired: the workgroups were not dispatched in the order the
// hardware was shared with something that starved a hand-off).  Re-arm every hand-off word, drop to the per-level
// kernels and tell the caller to repeat the solve.  The downgrade is temporary: after 64 further LDL solves (doubling
// with every time-out; debug switch PERSIST_RETRY=<n>: the first interval, 0 = never) the persistent kernels are tried
// again.  Returns false when there is nothing left to fall back to.
static bool recover_from_sweep_failure(hipkkt_solver *S) {
    PersistState &ps = S->persist;
    if (!ps.use) return false;
    for (SolveCtx &C : S->ctx) HK_CHECK(hipStreamSynchronize(C.stream));
    S->stats.n_sweep_timeouts++;
    const int64_t first = debug_opts().persist_retry >= 0 ? debug_opts().persist_retry : 64;
    ps.backoff = ps.backoff > 0 ? 2 * ps.backoff : first;
    ps.retry_at = first > 0 ? S->stats.n_ldlsolves + ps.backoff : -1;
    fprintf(stderr, "hipkkt: a persistent sweep kernel timed out (flags 0x%x 0x%x); per-level solve kernels for the next %lld LDL solves\n",
            S->ctx[0].h_flags[FL_FRONTFAIL], S->ctx[1].h_flags[FL_FRONTFAIL], (long long)(ps.retry_at >= 0 ? ps.backoff : -1));
    const SyncWords nw = sync_words(S);
    for (SolveCtx &C : S->ctx) {
        fill_async(S->stream, C.dp.seg_sync, 0, nw.seg * sizeof(int));
        fill_async(S->stream, C.dp.front_sync, 0, nw.front * sizeof(int));
        fill_async(S->stream, C.dp.flags + FL_FRONTFAIL, 0, sizeof(int));
        C.h_flags[FL_FRONTFAIL] = 0;
        invalidate_solve_graphs(C);
    }
    HK_CHECK(hipStreamSynchronize(S->stream));
    ps.use = false;
    return true;
}

// Runs body (one whole attempt: enqueue, finish; returns whether a persistent sweep timed out in it) at most twice: a time-out that
// recover_from_sweep_failure can answer repeats everything on the per-level kernels.  Returns true when the last attempt timed out.
template <class Body>
static bool with_sweep_retry(hipkkt_solver *T, Body &&body) {
    for (int attempt = 0; attempt < 2; attempt++) {
        maybe_retry_persistent(T);
        if (!body()) return false;
        if (!recover_from_sweep_failure(T)) return true;
    }
    return true;
}

// a negative status wins, then the first positive one
static int32_t merge_rc(int32_t rc, int32_t r) { return (r < 0 || (r > 0 && rc == HIPKKT_OK)) ? (r < 0 ? r : (rc < 0 ? rc : r)) : rc; }

// one solve call of nrhs right-hand sides that took ms on T; booked on the caller's handle S too when the twin solved
static void account_solve(hipkkt_solver *S, hipkkt_solver *T, double ms, int64_t nrhs) {
    for (hipkkt_solver *h : {T, S != T ? S : nullptr})
        if (h) { h->stats.t_last_solve = ms; h->stats.t_acc_solve += ms; h->stats.n_solvecalls++; h->stats.n_rhs_solved += nrhs; }
}

// host right-hand side [rhsx | rhsz | 0] into C.d_b
static void upload_rhs(SolveCtx &C, const double *rhsx, const double *rhsz, int64_t n, int64_t m, int64_t p) {
    if (n) HK_CHECK(hipMemcpyAsync(C.d_b, rhsx, n * sizeof(double), hipMemcpyHostToDevice, C.stream));
    if (m) HK_CHECK(hipMemcpyAsync(C.d_b + n, rhsz, m * sizeof(double), hipMemcpyHostToDevice, C.stream));
    if (p) HK_CHECK(hipMemsetAsync(C.d_b + n + m, 0, p * sizeof(double), C.stream));
}

// ref: kktsolver_solve! + _iterative_refinement (kktsolver_directldl.jl:346-449); C.d_b holds b.  Enqueues the first
// solve, its residual, the device-side decision and ONE refinement step (decided on the device whether it counts), then
// the read-back of the state -- no synchronisation: several contexts can be started before any is finished.
static void solve_begin(hipkkt_solver *S, SolveCtx &C, const RefineOpts &ir) {
    hipStream_t st = C.stream;
    if (S->kval_event_pending && st != S->stream) HK_CHECK(hipStreamWaitEvent(st, S->ev3, 0));   // an asynchronous hipkkt_set_hs_dev on the main stream
    HK_CHECK(hipEventRecord(C.ev_a, st));
    C.ir_used = ir.enable != 0;
    if (ir.enable) {
        const bool same = C.g_opts.same_graph(ir);
        run_graphed(S, st, C.g_first, same, [&] {
            enqueue_ldl_solve(S, C, C.d_b, C.d_x0, (int *)(C.dp.scal + SC_NORMB), 4);       // (||b||, ||e|| start from zero)
            launch_norm_inf(st, C.d_b, S->N, (unsigned long long *)C.dp.scal + SC_NORMB);
            launch_spmv_residual(st, C.dp, C.d_b, nullptr, C.d_x0, C.d_x0, C.d_e, S->N, (unsigned long long *)C.dp.scal + SC_NORME);
            launch_refine_decide(st, C.d_rs, C.dp.scal, 0, ir.reltol, ir.abstol, (int)std::min<int64_t>(ir.max_iter, 1 << 30), ir.stop_ratio);
            if (ir.max_iter > 0) enqueue_refine_step(S, C, ir);
        });
        if (!same) { C.g_step.valid = false; C.g_opts = ir; }
        S->stats.n_ldlsolves += ir.max_iter > 0 ? 2 : 1;
    } else {
        run_graphed(S, st, C.g_ldl, true, [&] {
            enqueue_ldl_solve(S, C, C.d_b, C.d_x0);
            launch_zero_words(st, C.dp.flags, 1);
            launch_check_finite(st, C.d_x0, S->N, C.dp.flags);
        });
        S->stats.n_ldlsolves += 1;
    }
}

// copy the accepted iterate of a started solve to a device buffer (first nm entries), still without synchronising
static void solve_copy_out_dev(hipkkt_solver *S, SolveCtx &C, double *out_dev, int nm) {
    if (!out_dev) return;
    if (C.ir_used) launch_refine_copy_out(C.stream, C.d_rs, C.d_x0, C.d_x1, out_dev, nm);
    else HK_CHECK(hipMemcpyAsync(out_dev, C.d_x0, (size_t)nm * sizeof(double), hipMemcpyDeviceToDevice, C.stream));
}

// waits for a started solve, runs further refinement steps while the device says so, reports like the reference
static int32_t solve_finish(hipkkt_solver *S, SolveCtx &C, int64_t *ir_steps, double *out_dev, int nm) {
    hipStream_t st = C.stream;
    auto readback = [&] {
        if (C.ir_used) HK_CHECK(hipMemcpyAsync(C.h_rs, C.d_rs, sizeof(RefineState), hipMemcpyDeviceToHost, st));
        HK_CHECK(hipMemcpyAsync(C.h_flags, C.dp.flags, FL_COUNT * sizeof(int), hipMemcpyDeviceToHost, st));
        HK_CHECK(hipEventRecord(C.ev_b, st));
        HK_CHECK(hipStreamSynchronize(st));
    };
    readback();
    bool more = false;
    C.extra_steps = false;
    while (C.ir_used && C.h_rs->active && !sweep_failed(C)) {   // rare: more than one step needed
        run_graphed(S, st, C.g_step, true, [&] { enqueue_refine_step(S, C, C.g_opts); });
        S->stats.n_ldlsolves += 1;
        more = true;
        readback();
    }
    C.extra_steps = more;
    if (more && out_dev) {   // the accepted iterate changed after the copy that solve_copy_out_dev enqueued
        solve_copy_out_dev(S, C, out_dev, nm);
        HK_CHECK(hipEventRecord(C.ev_b, st));
        HK_CHECK(hipStreamSynchronize(st));
    }
    float ms = 0;
    HK_CHECK(hipEventElapsedTime(&ms, C.ev_a, C.ev_b));
    C.last_ms = ms;
    if (ir_steps) *ir_steps = C.ir_used ? C.h_rs->steps : 0;
    if (sweep_failed(C)) { S->err = "persistent solve kernel timed out"; return HIPKKT_ERR_DEVICE; }
    const bool ok = C.ir_used ? C.h_rs->fail == 0 : C.h_flags[FL_NONFINITE] == 0;
    return ok ? HIPKKT_OK : HIPKKT_NUMERICAL_FAILURE;
}

// the solver that holds the current factorisation (the robust-order twin after a fallback)
hipkkt_solver *solve_target(hipkkt_solver *S) { return (S->twin.using_fallback && S->twin.fallback) ? S->twin.fallback : S; }

// nrhs (<= kNumCtx) right-hand sides already in T->ctx[c].d_b (T = solve_target(S)): solved concurrently, results optionally
// copied to out_dev[c].  after (hipkkt_step_default_start_dev): work on the copies, enqueued on context 0's stream behind all of them
// before anything is waited for, and once more when a solve took refinement steps beyond the one in its graph (the copies changed);
// the first synchronisation of context 0 then covers it.
int32_t solve_many(hipkkt_solver *S, hipkkt_solver *T, int nrhs, const RefineOpts &ir, int64_t *ir_steps, double *const *out_dev, int nm,
                   const std::function<void(hipStream_t)> *after) {
    int32_t rc = HIPKKT_OK;
    double ms = 0;
    bool redo = false;
    auto run_after = [&] {
        for (int c = 1; c < nrhs; c++) {
            HK_CHECK(hipEventRecord(S->ev2, T->ctx[c].stream));
            HK_CHECK(hipStreamWaitEvent(T->ctx[0].stream, S->ev2, 0));
        }
        (*after)(T->ctx[0].stream);
    };
    const bool gave_up = with_sweep_retry(T, [&] {
        for (int c = 0; c < nrhs; c++) {
            solve_begin(T, T->ctx[c], ir);
            solve_copy_out_dev(T, T->ctx[c], out_dev ? out_dev[c] : nullptr, nm);
        }
        if (after) run_after();
        rc = HIPKKT_OK;
        ms = 0;
        redo = false;
        bool timed_out = false;
        for (int c = 0; c < nrhs; c++) {
            rc = merge_rc(rc, solve_finish(T, T->ctx[c], ir_steps ? ir_steps + c : nullptr, out_dev ? out_dev[c] : nullptr, nm));
            ms = std::max(ms, T->ctx[c].last_ms);
            timed_out = timed_out || sweep_failed(T->ctx[c]);
            redo = redo || T->ctx[c].extra_steps;
        }
        return timed_out;
    });
    if (after && !gave_up && rc == HIPKKT_OK) {
        if (redo) run_after();
        HK_CHECK(hipStreamSynchronize(T->ctx[0].stream));      // (returns at once unless `after` ran again or context 1 finished last)
    }
    account_solve(S, T, ms, nrhs);
    return rc;
}

// SURVEY section 8(f) row N2, second half: kkt_solve! (kktsystem.jl:135-215) between the caller's cone algebra and mul_Hs!.
// Both solves are started before anything is waited for; the reduction (dots, dtau, axpys) and the copies of the step are
// enqueued behind them speculatively; the host synchronises once.  Only if a solve needed more refinement steps than the one that
// is part of its graph (rare) the reduction is repeated after those steps.
// out.after_reduce (hipkkt_step.cpp): work enqueued behind every reduction on the same stream, from the step [dx | dz] it left in d_lhs.
int32_t kkt_solve_reduced_impl(hipkkt_solver *S, const ReducedIn &in, const ReducedScalars &sc, const ReducedOut &out, const RefineOpts &ir) {
    const int64_t n = S->img.n, m = S->img.m, p = S->img.p;
    const int nm = (int)(n + m);
    const int32_t const_pending = sc.const_pending;
    if (!S->red.d) {
        S->red.d = S->dalloc<double>(3 * (size_t)S->N + n + 16);                          // x1z1 | x2z2 | lhs | var_x | scalars
        S->red.d_part = S->dalloc<double>(8 * (size_t)residual_blocks((int)n, (int)m) + 8);
        S->red.have_const = false;
    }
    double *d_s1 = S->red.d, *d_s2 = d_s1 + S->N, *d_lhs = d_s2 + S->N, *d_xv = d_lhs + S->N, *d_sc = d_xv + n;
    if (!const_pending && !S->red.have_const) { S->err = "kkt_solve_reduced: no constant-rhs solution resident (pass const_pending = 1 after a refactorisation)"; return HIPKKT_ERR_ARGUMENT; }
    hipkkt_solver *T = solve_target(S);
    const double tau = sc.scal_in4[0], kappa = sc.scal_in4[1], rhs_tau = sc.scal_in4[2], rhs_kappa = sc.scal_in4[3];
    SolveCtx &A = T->ctx[0], &Bc = T->ctx[1];
    auto reduce = [&]() {
        launch_reduced(A.stream, S->dp, d_s1, d_s2, d_xv, S->res.d_qb, S->res.d_qb + n, tau, kappa, rhs_tau, rhs_kappa, S->red.d_part, d_sc,
                       d_lhs, (int)n, (int)m);
        if (out.lhs_dev) HK_CHECK(hipMemcpyAsync(out.lhs_dev, d_lhs, (size_t)nm * sizeof(double), hipMemcpyDeviceToDevice, A.stream));
        if (out.lhs_x && n) HK_CHECK(hipMemcpyAsync(out.lhs_x, d_lhs, n * sizeof(double), hipMemcpyDeviceToHost, A.stream));
        if (out.lhs_z && m) HK_CHECK(hipMemcpyAsync(out.lhs_z, d_lhs + n, m * sizeof(double), hipMemcpyDeviceToHost, A.stream));
        HK_CHECK(hipMemcpyAsync(S->h_scal_red, d_sc, 10 * sizeof(double), hipMemcpyDeviceToHost, A.stream));
        if (out.after_reduce) (*out.after_reduce)(A.stream, d_lhs);
    };
    // the reduction on A's stream waits for the constant-rhs solve on the other context
    auto join_const = [&]() { HK_CHECK(hipEventRecord(S->ev2, Bc.stream)); HK_CHECK(hipStreamWaitEvent(A.stream, S->ev2, 0)); };
    int64_t st1 = 0, st2 = 0;
    int32_t rc = HIPKKT_OK;
    bool redo = false;
    double ms = 0;
    const bool gave_up = with_sweep_retry(T, [&] {
        // right-hand sides
        if (in.in_dev) {
            launch_set_rhs(A.stream, A.d_b, in.in_dev, nm, T->N);
            HK_CHECK(hipMemcpyAsync(d_xv, in.in_dev + nm, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, A.stream));
        } else {
            upload_rhs(A, in.rhs_x, in.workz, n, m, p);
            if (n) HK_CHECK(hipMemcpyAsync(d_xv, in.var_x, n * sizeof(double), hipMemcpyHostToDevice, A.stream));
        }
        solve_begin(T, A, ir);
        solve_copy_out_dev(T, A, d_s1, nm);
        if (const_pending) {
            launch_const_rhs(Bc.stream, Bc.d_b, S->res.d_qb, (int)n, nm, T->N);
            solve_begin(T, Bc, ir);
            solve_copy_out_dev(T, Bc, d_s2, nm);
            join_const();
        }
        reduce();
        st1 = st2 = 0;
        rc = solve_finish(T, A, &st1, d_s1, nm);
        redo = A.extra_steps;
        ms = A.last_ms;
        if (const_pending) {
            rc = merge_rc(rc, solve_finish(T, Bc, &st2, d_s2, nm));
            redo = redo || Bc.extra_steps;
            ms = std::max(ms, Bc.last_ms);
        }
        return sweep_failed(A) || (const_pending && sweep_failed(Bc));
    });
    if (gave_up) return HIPKKT_ERR_DEVICE;
    if (redo && rc == HIPKKT_OK) {                              // the accepted iterates changed after the speculative reduction
        if (const_pending) join_const();
        reduce();
    }
    HK_CHECK(hipStreamSynchronize(A.stream));
    account_solve(S, T, ms, const_pending ? 2 : 1);
    if (rc == HIPKKT_OK && const_pending) S->red.have_const = true;
    if (out.ir_steps) { out.ir_steps[0] = st1; out.ir_steps[1] = st2; }
    if (out.scal_out) memcpy(out.scal_out, S->h_scal_red, 10 * sizeof(double));
    return rc;
}

}  // namespace hipkkt_host

extern "C" {

// ---- solve -------------------------------------------------------------------------------------

int32_t hipkkt_setrhs(hipkkt_handle h, const double *rhsx, const double *rhsz) {
    HK_ENTER(h)
    const int64_t n = S->img.n, m = S->img.m;
    if (!S->l1 || (n && !rhsx) || (m && !rhsz)) return HIPKKT_ERR_ARGUMENT;
    upload_rhs(S->ctx[0], rhsx, rhsz, n, m, S->img.p);
    HK_CHECK(hipStreamSynchronize(S->stream));
    return HIPKKT_OK;
    HK_LEAVE
}

int32_t hipkkt_setrhs_dev(hipkkt_handle h, const double *rhs_dev) {
    HK_ENTER(h)
    if (!S->l1 || !rhs_dev) return HIPKKT_ERR_ARGUMENT;
    launch_set_rhs(S->stream, S->ctx[0].d_b, rhs_dev, (int)(S->img.n + S->img.m), S->N);
    // (no host synchronisation: the solve that reads d_b runs on the same stream; rhs_dev must stay valid until that solve has returned)
    return HIPKKT_OK;
    HK_LEAVE
}

// the right-hand side that hipkkt_setrhs left in the handle's context 0, handed to the twin when that holds the factorisation
static hipkkt_solver *target_with_rhs(hipkkt_solver *S) {
    hipkkt_solver *T = solve_target(S);
    if (T != S) copy_sync(S->stream, T->ctx[0].d_b, S->ctx[0].d_b, (size_t)S->N * sizeof(double), hipMemcpyDeviceToDevice);
    return T;
}

int32_t hipkkt_solve(hipkkt_handle h, double *lhsx, double *lhsz, int32_t ir_enable, double reltol, double abstol,
                     int64_t max_iter, double stop_ratio, int64_t *ir_steps) {
    HK_ENTER(h)
    if (!S->l1) return HIPKKT_ERR_ARGUMENT;
    hipkkt_solver *T = target_with_rhs(S);
    int32_t rc = solve_many(S, T, 1, RefineOpts{ir_enable, reltol, abstol, max_iter, stop_ratio}, ir_steps, nullptr, 0);
    if (rc == HIPKKT_OK) {  // ref: kktsolver_getlhs! only on success
        const int64_t n = S->img.n, m = S->img.m;
        const double *x = T->ctx[0].result();
        if (lhsx && n) copy_sync(S->stream, lhsx, x, n * sizeof(double), hipMemcpyDeviceToHost);
        if (lhsz && m) copy_sync(S->stream, lhsz, x + n, m * sizeof(double), hipMemcpyDeviceToHost);
    }
    return rc;
    HK_LEAVE
}

int32_t hipkkt_solve_dev(hipkkt_handle h, double *lhs_dev, int32_t ir_enable, double reltol, double abstol,
                         int64_t max_iter, double stop_ratio, int64_t *ir_steps) {
    HK_ENTER(h)
    if (!S->l1) return HIPKKT_ERR_ARGUMENT;
    hipkkt_solver *T = target_with_rhs(S);
    double *outs[1] = {lhs_dev};
    return solve_many(S, T, 1, RefineOpts{ir_enable, reltol, abstol, max_iter, stop_ratio}, ir_steps, outs, (int)(S->img.n + S->img.m));
    HK_LEAVE
}

// several right-hand sides on one factorisation, two at a time on concurrent solve contexts
static int32_t solve_multi_impl(hipkkt_solver *S, int64_t nrhs, const double *rhsx, const double *rhsz, const double *rhs_dev,
                                double *lhsx, double *lhsz, double *lhs_dev, const RefineOpts &ir, int64_t *ir_steps) {
    const int64_t n = S->img.n, m = S->img.m, p = S->img.p;
    hipkkt_solver *T = solve_target(S);
    int32_t rc_all = HIPKKT_OK;
    for (int64_t r0 = 0; r0 < nrhs; r0 += kNumCtx) {
        const int k = (int)std::min<int64_t>(kNumCtx, nrhs - r0);
        double *outs[kNumCtx] = {nullptr, nullptr};
        for (int c = 0; c < k; c++) {
            SolveCtx &C = T->ctx[c];
            const int64_t r = r0 + c;
            if (rhs_dev) launch_set_rhs(C.stream, C.d_b, rhs_dev + r * (n + m), (int)(n + m), T->N);
            else upload_rhs(C, rhsx + r * n, rhsz + r * m, n, m, p);
            if (lhs_dev) outs[c] = lhs_dev + r * (n + m);
        }
        const int32_t rc = solve_many(S, T, k, ir, ir_steps ? ir_steps + r0 : nullptr, lhs_dev ? outs : nullptr, (int)(n + m));
        if (rc < 0) return rc;
        if (rc > 0) rc_all = rc;
        if (rc == HIPKKT_OK && (lhsx || lhsz))
            for (int c = 0; c < k; c++) {
                const double *x = T->ctx[c].result();
                const int64_t r = r0 + c;
                if (lhsx && n) copy_sync(S->stream, lhsx + r * n, x, n * sizeof(double), hipMemcpyDeviceToHost);
                if (lhsz && m) copy_sync(S->stream, lhsz + r * m, x + n, m * sizeof(double), hipMemcpyDeviceToHost);
            }
    }
    return rc_all;
}

int32_t hipkkt_solve_multi(hipkkt_handle h, int64_t nrhs, const double *rhsx, const double *rhsz, double *lhsx, double *lhsz,
                           int32_t ir_enable, double reltol, double abstol, int64_t max_iter, double stop_ratio, int64_t *ir_steps) {
    HK_ENTER(h)
    if (!S->l1 || nrhs < 0 || (nrhs && ((S->img.n && !rhsx) || (S->img.m && !rhsz)))) return HIPKKT_ERR_ARGUMENT;
    return solve_multi_impl(S, nrhs, rhsx, rhsz, nullptr, lhsx, lhsz, nullptr, RefineOpts{ir_enable, reltol, abstol, max_iter, stop_ratio}, ir_steps);
    HK_LEAVE
}

int32_t hipkkt_solve_multi_dev(hipkkt_handle h, int64_t nrhs, const double *rhs_dev, double *lhs_dev, int32_t ir_enable, double reltol,
                               double abstol, int64_t max_iter, double stop_ratio, int64_t *ir_steps) {
    HK_ENTER(h)
    if (!S->l1 || nrhs < 0 || (nrhs && !rhs_dev)) return HIPKKT_ERR_ARGUMENT;
    return solve_multi_impl(S, nrhs, nullptr, nullptr, rhs_dev, nullptr, nullptr, lhs_dev, RefineOpts{ir_enable, reltol, abstol, max_iter, stop_ratio}, ir_steps);
    HK_LEAVE
}

int32_t hipkkt_kkt_solve_reduced(hipkkt_handle h, const double *rhs_x, const double *workz, const double *var_x, const double *scal_in4,
                                 int32_t const_pending, double *lhs_x, double *lhs_z, double *scal_out10, int32_t ir_enable,
                                 double reltol, double abstol, int64_t max_iter, double stop_ratio, int64_t *ir_steps2) {
    HK_ENTER(h)
    const int64_t n = S->img.n, m = S->img.m;
    if (!S->l1 || !S->res.d_qb || !scal_in4 || !scal_out10 || (n && (!rhs_x || !var_x)) || (m && !workz)) {
        S->err = "kkt_solve_reduced: call hipkkt_set_qb first / bad arguments";
        return HIPKKT_ERR_ARGUMENT;
    }
    ReducedOut out;
    out.lhs_x = lhs_x; out.lhs_z = lhs_z; out.scal_out = scal_out10; out.ir_steps = ir_steps2;
    return kkt_solve_reduced_impl(S, ReducedIn::host(rhs_x, workz, var_x), {scal_in4, const_pending}, out, RefineOpts{ir_enable, reltol, abstol, max_iter, stop_ratio});
    HK_LEAVE
}

int32_t hipkkt_kkt_solve_reduced_dev(hipkkt_handle h, const double *in_dev, const double *scal_in4, int32_t const_pending,
                                     double *lhs_dev, double *scal_out10, int32_t ir_enable, double reltol, double abstol,
                                     int64_t max_iter, double stop_ratio, int64_t *ir_steps2) {
    HK_ENTER(h)
    if (!S->l1 || !S->res.d_qb || !scal_in4 || !scal_out10 || !in_dev) {
        S->err = "kkt_solve_reduced_dev: call hipkkt_set_qb first / bad arguments";
        return HIPKKT_ERR_ARGUMENT;
    }
    ReducedOut out;
    out.lhs_dev = lhs_dev; out.scal_out = scal_out10; out.ir_steps = ir_steps2;
    return kkt_solve_reduced_impl(S, ReducedIn::device(in_dev), {scal_in4, const_pending}, out, RefineOpts{ir_enable, reltol, abstol, max_iter, stop_ratio});
    HK_LEAVE
}

int32_t hipkkt_ldl_solve(hipkkt_handle h, double *x, const double *b) {
    if (h && h->twin.using_fallback && h->twin.fallback) return hipkkt_ldl_solve(h->twin.fallback, x, b);
    HK_ENTER(h)
    if (!x || !b) return HIPKKT_ERR_ARGUMENT;
    SolveCtx &C = S->ctx[0];
    HK_CHECK(hipMemcpyAsync(C.d_b, b, (size_t)S->N * sizeof(double), hipMemcpyHostToDevice, C.stream));
    int32_t rc = solve_many(S, S, 1, RefineOpts{0, 0.0, 0.0, 0, 0.0}, nullptr, nullptr, 0);
    if (rc < 0) return rc;
    // ref: solve!(ldlsolver,K,x,b) returns whatever the triangular solves produce; a non-finite result is the caller's to detect
    copy_sync(S->stream, x, C.d_x0, (size_t)S->N * sizeof(double), hipMemcpyDeviceToHost);
    return HIPKKT_OK;
    HK_LEAVE
}

}  // extern "C"
