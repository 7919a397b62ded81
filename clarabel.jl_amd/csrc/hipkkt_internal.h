// Internal declarations shared by the translation units of libclarabel_hipkkt.so's host side:
//   hipkkt_abi.cpp     C entry points: creation / getters / value updates / residuals / diagnostics
//   hipkkt_cones.cpp   cone registration and scaling (hipkkt_set_cone_types[_ex], hipkkt_update_scaling[_ex][_dev])
//   hipkkt_setup.cpp   runtime objects, device residency of a plan, handle creation (finish_create)
//   hipkkt_factor.cpp  the factorisation's launch sequence (enqueue_factor: one walk for the graph and, with a FactorProbe, the profiled
//                      path), hipkkt_refactor and the robust-order twin
//   solve_schedule.cpp the solve schedule of a plan: level lists, segments, item order (host arithmetic only; solve_schedule.h)
//   hipkkt_solve.cpp   LDL solves, device-side iterative refinement, the solve entry points
//   hipkkt_step.cpp    the cone algebra of an interior-point step around the reduced solve (hipkkt_cone_* / hipkkt_step_*), the default start
// hipkkt_parts.h holds the parts a handle is made of besides its cones (hipkkt_cones.h).
// Host orchestration only; all numeric work is in the .hip files: values / kernels / front_block2 (front_block: testing build) /
// solve_sweep / front_sweep / refine / assemble_dev / scaling / step, step_cone3, step_genpow, step_psd / start; kernels.h lists their launchers.
#pragma once
#include "../../include/hipkkt.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "assemble.h"
#include "cone_layout.h"
#include "device_plan.h"
#include "hipkkt_cones.h"
#include "hipkkt_parts.h"
#include "kernels.h"
#include "runtime_pool.h"
#include "solve_schedule.h"
#include "symbolic.h"

namespace hipkkt { int box_probe(int device, double *out); }   // probe.hip
namespace hipkkt_host {
using namespace hipkkt;

extern thread_local std::string g_create_error;

struct DeviceError {
    std::string msg;
};

#define HK_CHECK(expr)                                                                            \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            throw DeviceError{std::string(#expr) + ": " + hipGetErrorString(e_)};                 \
    } while (0)

// Synchronous copy / fill on a handle's OWN stream.  The legacy (NULL) stream is never used: an operation on it from
// one host thread fails while another thread captures a hipGraph ("would make the legacy stream depend on a capturing
// stream"), and handles are meant to be driven concurrently from several threads.
inline void copy_sync(hipStream_t st, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    if (!bytes) return;
    HK_CHECK(hipMemcpyAsync(dst, src, bytes, kind, st));
    HK_CHECK(hipStreamSynchronize(st));
}
inline void fill_async(hipStream_t st, void *dst, int value, size_t bytes) {
    if (bytes) HK_CHECK(hipMemsetAsync(dst, value, bytes, st));
}

// Test / experiment switches (hipkkt_debug_set, include/hipkkt.h).  The library reads NO environment variable for them: a production
// build (libclarabel_hipkkt.so, what the Julia glue and bench.py load) keeps these defaults for ever -- hipkkt_debug_set refuses -- and
// does not even contain the code some of them select (the first form of the front-batch kernel, the debug flags of the sweeps).
// The -DHIPKKT_TESTING build (libclarabel_hipkkt_testing.so, what tests/ load) accepts them; a handle reads them when it is created.
// (Until round 5 every one of them was an environment read inside the product: a HIPKKT_* variable left over in a caller's environment
// silently changed the arithmetic order, or -- DEBUG_FLAGS -- the results.)
struct DebugOpts {
    bool plan_cache = true;        // PLAN_CACHE=0: no process-wide plan cache
    bool fb_extra = true;          // FB_EXTRA=0: every far stage applies all of its tiles in its own launch
    bool fb_stream = true;         // FB_STREAM=0: the round-3 pivot chain (whole-tile hand-off; first form of the kernel only)
    bool fb_v2 = true;             // FB_V2=0: the first form of the front-batch kernel (front_block.hip)
    bool force_twin = false;       // FORCE_TWIN=1: every successful factorisation in the cheap order counts as broken down
    bool no_graph = false;         // NO_GRAPH=1: eager launches
    bool no_persist = false;       // NO_PERSIST=1: per-level solve kernels only
    bool full_tiles = true;        // FULL_TILES=0: the general core for every dense tile
    bool front_block = true;       // FRONT_BLOCK=0: one launch per panel
    bool split_k = true;           // SPLIT_K=0
    bool gather_overlap = true;    // GATHER_OVERLAP=0: big gather stages run whole, in line (no side stream)
    bool gather_sort = true;       // GATHER_SORT=0: the entries of a gather stage stay in target order
    int gather_side_blocks = 512;  // GATHER_SIDE_BLOCKS=<n>: grid bound of the side-stream gather (2 workgroups per compute unit; 0 = unbounded)
    bool dense_tri = true;         // DENSE_TRI=0: dense Hs triangles stay in the symmetric view
    bool ordering_amd = false;     // ORDERING=amd: minimum degree on K only
    bool no_front = false;         // NO_FRONT=1: no persistent front kernels
    bool host_assembly = false;    // HOST_ASSEMBLY=1: the host twin of the assembly kernels
    int front_block_min_rows = -1; // FRONT_BLOCK_MIN_ROWS=<n> (-1: the plan's default)
    int superhop = -1;             // SUPERHOP=<n> (-1: the plan's default)
    int debug_flags = 0;           // DEBUG_FLAGS=<bits>: timing experiments, results are WRONG when set
    long long spin_limit = -1;     // SPIN_LIMIT=<n> (-1: 2^20)
    long long persist_retry = -1;  // PERSIST_RETRY=<n> (-1: 64)
    double accurate = 64.0;        // ACCURATE=<tau>: 0 = never, negative = every wide block
    int fb_extra_pw = 1;           // FB_EXTRA_PW=<tiles per wavefront>,<penalty 1>,<penalty 2>
    double fb_pen1 = 10.0, fb_pen2 = 28.0;
    int psd_large_min = 65;        // PSD_LARGE_MIN=<n>: the smallest PSD side hipkkt_step_enable_psd_large routes to step_psd_large.hip (0 = 65; read at the enable)
};
DebugOpts &debug_opts();
bool verbose();                    // HIPKKT_VERBOSE in the environment: diagnostic lines on stderr (changes no result)

struct GraphSlot {
    hipGraphExec_t exec = nullptr;
    bool valid = false;
    // parameters baked into the captured kernel arguments
    int static_enable = -1;
    double eps_const = 0, eps_prop = 0;
};

}  // namespace hipkkt_host

using namespace hipkkt;        // internal header of one library: the host files all work inside these two namespaces
using namespace hipkkt_host;

// The parameters of iterative refinement as the C entry points receive them (include/hipkkt.h); everything below the ABI passes this.
struct RefineOpts {
    int32_t enable; double reltol, abstol; int64_t max_iter; double stop_ratio;
    // the values baked into a captured refinement graph (enable only picks the graph)
    bool same_graph(const RefineOpts &o) const { return reltol == o.reltol && abstol == o.abstol && max_iter == o.max_iter && stop_ratio == o.stop_ratio; }
};

// One solve context = everything a refined KKT solve mutates: its stream, work vectors, the hand-off / counter words
// of the persistent sweeps (a private copy of those DevPlan pointers), the device-side refinement state and its
// captured graphs.  Two contexts let two right-hand sides be solved CONCURRENTLY on one factorisation (SURVEY
// section 8(f) row N2: the constant-rhs solve and the affine solve of an IPM iteration): the sweeps are bound by
// dependency latency, not by throughput, so two of them overlap almost perfectly.
constexpr int kNumCtx = 2;
constexpr int kScalRedDoubles = 16;   // what h_scal_red may hold: the pinned chunk's second half (hipkkt_setup.cpp init_runtime)
struct SolveCtx {
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevPlan dp{};                 // S->dp with this context's ubuf / pbuf / slots / sync words / scal / flags
    double *d_b = nullptr, *d_x0 = nullptr, *d_x1 = nullptr, *d_e = nullptr, *d_corr = nullptr;
    double *d_y = nullptr, *d_z = nullptr, *d_xp = nullptr;
    RefineState *d_rs = nullptr, *h_rs = nullptr;   // device state, pinned host copy
    int *h_flags = nullptr;                         // pinned copy of dp.flags
    hipkkt_host::GraphSlot g_ldl, g_first, g_step;               // plain LDL solve (d_b -> d_x0) / refined solve incl. its first step / one more step
    RefineOpts g_opts{-1, -1.0, -1.0, -1, -1.0};    // parameters baked into g_first / g_step (no caller passes these: the first comparison fails)
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    double last_ms = 0;
    bool ir_used = false;
    bool extra_steps = false;     // the last solve_finish ran refinement steps beyond the one inside the solve's graph
    const double *result() const { return (ir_used && h_rs->cur) ? d_x1 : d_x0; }
};

struct hipkkt_solver {
    int device = 0;
    SolveCtx ctx[kNumCtx];
    hipStream_t stream = nullptr;
    hipStream_t idle_stream = nullptr;   // never carries work: see init_runtime (hipkkt_setup.cpp)
    hipkkt_opts opts{};
    bool l1 = false;
    KKTImage img;      // L1: assembled image; L0: colptr/rowval/nzval/dsigns copied in
    HostPlan plan;
    PlanOptions plan_opts;       // as used for the current plan
    SolveSchedule sched;         // which supernode goes to which solve launch (solve_schedule.h)
    DevPlan dp{};
    std::vector<std::pair<void *, size_t>> allocs;   // device slabs (RuntimePool blocks: pointer, capacity)
    std::string err;

    int N = 0;
    int64_t nnzK = 0;
    std::chrono::steady_clock::time_point t_created{};   // when the assembly returned
    PersistState persist;
    FrontBatchState fb;
    UpdateSplit split;
    SocTables soc;
    ResidualBuffers res;
    ReducedSolve red;
    TwinState twin;
    SolverStats stats;
    ConeState cones;                     // registration, device tables, resident step (hipkkt_cones.h)
    // refined block solves (kernels.hip k_invert_diag_wide): wide diagonal blocks whose explicit inverse has an entry above the threshold
    double accurate_threshold = 64.0;    // ACCURATE=<threshold> ("0" = never, "-1" = every wide block)
    int last_npolish = 0;                // marked blocks of the last factorisation
    int inv_nsmall = 0, inv_wsmall = 1, inv_nwide = 0;   // split of the diagonal-block inversions (kernels.hip)
    int side_join_level = -1;            // >= 0 while a side-stream gather is in flight: the first level whose update stage must wait for it
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;

    // device index arrays for value updates
    int64_t *d_mapHs = nullptr, *d_mapP = nullptr, *d_mapA = nullptr, *d_diag_full = nullptr;
    // N1: update_scaling! / get_Hs! on the device (hipkkt_set_cone_types + hipkkt_update_scaling, hipkkt_cones.cpp, scaling.hip)
    std::vector<int64_t> cone_numel;                       // as given to hipkkt_create_from_parts
    std::vector<int32_t> cone_hs_dense, cone_sparse_kind;

    double *d_stage = nullptr;   // staging for host-supplied values
    int64_t *d_stage_idx = nullptr;
    int64_t stage_cap = 0;
    double *h_scal = nullptr;    // pinned read-back area
    double *h_scal_red = nullptr;   // ... its second half, kScalRedDoubles doubles: the ten scalars of the reduced solve and the step lengths behind
                                    // them (hipkkt_step.cpp fused_solve), or the two decision records of the default start
    int *h_flags = nullptr;

    hipkkt_host::GraphSlot g_factor;
    bool use_graph = true;
    bool runtime_ready = false;   // init_runtime done (streams, events, pinned areas)
    bool profiling = false;
    bool profiling_no_extra = false;     // hipkkt_set_profiling(h, 2): the profiled refactorisations keep every far tile in its stage's own launch
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    bool kval_event_pending = false;     // ev3 marks an asynchronous value update of the resident K on the main stream (hipkkt_set_hs_dev)
    double last_eps = 0;
    int64_t last_nreg = 0;

    // Device memory comes from a few slabs (bump allocation, 256-byte aligned) instead of one hipMalloc per array:
    // a handle owns ~80 arrays, and on the small problems of a batch the ~160 hipMalloc / hipFree calls were a
    // third of the set-up + tear-down time.
    char *slab_cur = nullptr;
    size_t slab_left = 0;
    template <class T>
    T *dalloc(size_t n) {
        if (n == 0) n = 1;
        const size_t bytes = (n * sizeof(T) + 255) & ~(size_t)255;
        if (bytes > slab_left) {
            size_t slab = std::max<size_t>(bytes, (size_t)8 << 20);
            void *p = RuntimePool::get().dev_alloc(device, slab, &slab);
            if (!p) throw std::bad_alloc();
            allocs.push_back({p, slab});
            slab_cur = (char *)p;
            slab_left = slab;
        }
        void *p = slab_cur;
        slab_cur += bytes;
        slab_left -= bytes;
        return (T *)p;
    }
    template <class T>
    T *upload(const std::vector<T> &v) {
        T *p = dalloc<T>(v.size());
        if (!v.empty()) hipkkt_host::copy_sync(stream, p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        return p;
    }
    void ensure_stage(int64_t n) {
        if (n <= stage_cap) return;
        int64_t cap = std::max<int64_t>(n, 2 * stage_cap);
        d_stage = dalloc<double>(cap);
        d_stage_idx = dalloc<int64_t>(cap);
        stage_cap = cap;
    }
    template <class F>
    void for_each_graph_slot(F &&f) {    // every captured graph of the handle
        f(g_factor); for (SolveCtx &C : ctx) { f(C.g_ldl); f(C.g_first); f(C.g_step); }
    }
    ~hipkkt_solver() {
        if (twin.cancel) twin.cancel->store(true);
        if (twin.go && twin.go->load() == 0) twin.go->store(2);
        if (twin.future.valid()) twin.future.wait();     // the thread reads twin.pending's image (a cancelled one ends at its next phase)
        twin.pending.reset();
        delete twin.fallback;
        (void)hipSetDevice(device);
        // everything below goes back to the process-wide cache (runtime_pool.h): the streams must be idle first
        RuntimePool &rp = RuntimePool::get();
        if (stream) (void)hipStreamSynchronize(stream);
        for (SolveCtx &C : ctx)
            if (C.own_stream && C.stream) (void)hipStreamSynchronize(C.stream);
        for_each_graph_slot([](hipkkt_host::GraphSlot &g) { if (g.exec) (void)hipGraphExecDestroy(g.exec); });
        for (SolveCtx &C : ctx) {
            rp.pinned_free(device, C.h_rs);
            rp.pinned_free(device, C.h_flags);
            for (hipEvent_t e : {C.ev_a, C.ev_b}) rp.event_put(device, e);
            if (C.own_stream) rp.stream_put(device, 2, C.stream);
        }
        for (auto &a : allocs) rp.dev_free(device, a.first, a.second);
        rp.pinned_free(device, h_scal);
        rp.pinned_free(device, h_flags);
        for (hipEvent_t e : {ev0, ev1, ev2, ev3, ev_fork, ev_join}) rp.event_put(device, e);
        rp.stream_put(device, 0, stream);
        rp.stream_put(device, 1, idle_stream);
    }
};

namespace hipkkt_host {

// The words a sweep time-out leaves in an undefined state, per solve context (recover_from_sweep_failure re-arms what
// alloc_solve_scratch cleared): the whole of seg_sync (device_plan.h seg_sync_layout) and of front_sync
struct SyncWords { size_t seg, front; };
inline SyncWords sync_words(const hipkkt_solver *S) {
    return {(size_t)seg_sync_layout(S->sched.nseg, S->plan.nsuper).words, (size_t)std::max(S->plan.front_sync_ints, 16)};
}

// hipkkt_setup.cpp
void plan_cache_counts(int64_t *hits, int64_t *misses);   // process-wide cache of symbolic plans (same pattern + options)
void init_runtime(hipkkt_solver *S);
void setup_device(hipkkt_solver *S);
int32_t finish_create(hipkkt_solver *S, const hipkkt_opts *opts, hipkkt_handle *out);
// hipkkt_solve.cpp
int32_t solve_many(hipkkt_solver *S, hipkkt_solver *T, int nrhs, const RefineOpts &ir, int64_t *ir_steps, double *const *out_dev, int nm,
                   const std::function<void(hipStream_t)> *after = nullptr);
hipkkt_solver *solve_target(hipkkt_solver *S);
// kkt_solve! around the two solves (hipkkt_kkt_solve_reduced*, hipkkt_step_*_dev): input either on the host or [rhs.x | workz | variables.x]
// on the device; outputs whichever of them are set
struct ReducedIn {
    const double *rhs_x, *workz, *var_x, *in_dev;
    static ReducedIn host(const double *rhs_x, const double *workz, const double *var_x) { return {rhs_x, workz, var_x, nullptr}; }
    static ReducedIn device(const double *in_dev) { return {nullptr, nullptr, nullptr, in_dev}; }
};
struct ReducedScalars { const double *scal_in4; int32_t const_pending; };   // tau, kappa, rhs_tau, rhs_kappa
struct ReducedOut {
    double *lhs_x = nullptr, *lhs_z = nullptr, *lhs_dev = nullptr, *scal_out = nullptr;
    int64_t *ir_steps = nullptr;
    const std::function<void(hipStream_t, const double *)> *after_reduce = nullptr;   // enqueued behind every reduction, from the step in d_lhs
};
int32_t kkt_solve_reduced_impl(hipkkt_solver *S, const ReducedIn &in, const ReducedScalars &sc, const ReducedOut &out, const RefineOpts &ir);

template <class F>
void run_graphed(hipkkt_solver *S, hipStream_t stream, GraphSlot &slot, bool reusable, F &&enqueue) {
    if (!S->use_graph) { enqueue(); return; }
    if (!(slot.valid && reusable)) {
        if (slot.exec) { (void)hipGraphExecDestroy(slot.exec); slot.exec = nullptr; slot.valid = false; }
        hipGraph_t graph = nullptr;
        HK_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed));
        try {
            enqueue();
        } catch (...) {
            (void)hipStreamEndCapture(stream, &graph);
            if (graph) (void)hipGraphDestroy(graph);
            throw;
        }
        HK_CHECK(hipStreamEndCapture(stream, &graph));
        hipError_t e = hipGraphInstantiate(&slot.exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { slot.exec = nullptr; S->use_graph = false; enqueue(); return; }
        slot.valid = true;
    }
    HK_CHECK(hipGraphLaunch(slot.exec, stream));
}

}  // namespace hipkkt_host

#define HK_ENTER(h)                                                      \
    if (!(h)) return HIPKKT_ERR_ARGUMENT;                                \
    hipkkt_solver *S = (h);                                              \
    try {                                                                \
        if (hipSetDevice(S->device) != hipSuccess) { S->err = "hipSetDevice failed"; return HIPKKT_ERR_DEVICE; }

#define HK_LEAVE                                                         \
    }                                                                    \
    catch (const DeviceError &e) { S->err = e.msg; return HIPKKT_ERR_DEVICE; } \
    catch (const std::bad_alloc &) { S->err = "out of memory"; return HIPKKT_ERR_ALLOC; } \
    catch (...) { S->err = "internal error"; return HIPKKT_ERR_INTERNAL; }
