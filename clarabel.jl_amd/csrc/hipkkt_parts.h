// The parts a handle (hipkkt_internal.h hipkkt_solver) is made of, next to the ConeState of hipkkt_cones.h.
#pragma once
#include <atomic>
#include <cstdint>
#include <future>
#include <memory>
#include <string>
#include <vector>

#include "device_plan.h"
#include "symbolic.h"

// setup_device (hipkkt_setup.cpp) resets a part as a whole unless its comment says what it keeps.

// the persistent sweep kernels of the solves and the temporary downgrade to per-level kernels after a time-out
struct PersistState {
    bool use = true;
    bool allowed = true;          // false: debug switch NO_PERSIST (never tried)
    int64_t retry_at = -1;        // after a sweep time-out: the LDL-solve count at which the persistent kernels are tried again
    int64_t backoff = 0;          // doubles with every time-out (64, 128, ...); kept across a re-set-up
    void rearm(bool allowed_) { use = allowed = allowed_; retry_at = -1; }
};

// per front batch: what the next batch of the same front needs from this batch's far stage ([columns of the next batch | rest]
// order of the stage's dense tiles, hipkkt_setup.cpp order_far_stages) -- the rest may ride in the next k_front_block launch
struct NextBatch {
    int next_blk = 0;             // workgroups of the next batch's panel kernel
    bool has_next = false;        // the next batch of the same front follows at once: [chain | rest] order valid
    int ncrit = 0;                // far stage: the first ncrit dense groups are the next batch's columns
};

// front batches factored by one launch each (front_block.hip / front_block2.hip)
struct FrontBatchState {
    struct Switches {             // latched from the debug switches by init_runtime: kept across a re-set-up
        bool use = true;          // cleared by a time-out inside a batch: one launch per panel from then on
        bool streamed = true;     // FB_STREAM=0: the round-3 chain (hand-off of the explicit inverse after all 64 pivots)
        bool v2 = true;           // front_block2.hip (tiles transposed in the accumulators, round 5); FB_V2=0: front_block.hip
        bool extra = true;        // the partial last round of a batch's far updates rides in the next k_front_block launch (FB_EXTRA=0: off)
    } sw;
    std::vector<hipkkt::FrontBatch> batches;
    std::vector<int> lvl;         // [nlevels] index of the batch that starts at this level, -2 inside a batch, -1 otherwise
    bool ends_batch(int l) const { return l + 1 >= (int)lvl.size() || lvl[(size_t)l + 1] != -2; }   // l (lvl[l] != -1) is the last level of its batch
    std::vector<int> last_level;  // per batch
    std::vector<NextBatch> next;
    int *d_sync = nullptr;
    double *d_scratch = nullptr;
    // streamed pivot chain of k_front_block: per (batch, panel, 8-pivot block) one record of 528 doubles that the diagonal
    // workgroup publishes as it eliminates and the next diagonal workgroup polls (sentinel-filled before every factorisation)
    double *d_stream = nullptr;
    int64_t stream_doubles = 0;
    long long *d_trace = nullptr; // HIPKKT_FB_TRACE=1: wall-clock stamps of the first 8 workgroups of every batch (debug_dump 9)
    void reset() { const Switches keep = sw; *this = FrontBatchState(); sw = keep; }
};

// How the update stages are cut.  Split-K of stages with few target tiles and long contribution lists (hipkkt_setup.cpp plan_split_k):
// per level, the range of the sub-groups appended to the dense-group records and of the reduce records.  Deferred part of a big
// gather stage (split_gather_stages): the entries of stage l are ordered [targets the next update batch factors or updates | targets
// beyond it]; the second part runs on the side stream next to the levels of the next batch (hipkkt_factor.cpp enqueue_gather / join_side).
struct UpdateSplit {
    int64_t scratch_doubles = 0;  // split-K partial tiles behind the panels in Lx (cleared with them before every factorisation)
    std::vector<int> group_begin, group_count, rec_ptr;
    hipkkt::SplitRec *d_recs = nullptr;
    std::vector<int64_t> heavy_ptr;          // [nlevels+1] into the list of heavy gather entries (kernels.hip k_update_gather_heavy)
    std::vector<int64_t> gath, gath_heavy;   // [l] entries / heavy entries of the first part of gather stage l (gath -1: not split)
};

struct SocTables {                // all sparse SOC cones concatenated
    int64_t total = 0;
    int n = 0;
    std::vector<int64_t> off;     // per sparse map (SOC only) offset into the concatenated arrays
    std::vector<int> of_sparse;   // sparse-map index -> soc ordinal or -1
    int64_t *d_uidx = nullptr, *d_vidx = nullptr, *d_didx = nullptr;
    int *d_cone = nullptr;
    double *d_u = nullptr, *d_v = nullptr, *d_eta2 = nullptr;
};
struct ResidualBuffers {          // residuals_update! on the device (N4)
    double *d_qb = nullptr, *d_in = nullptr, *d_out = nullptr, *d_part = nullptr;
};
struct ReducedSolve {             // reduced-system algebra of kkt_solve! (N2)
    double *d = nullptr, *d_part = nullptr;   // [x1;z1] | [x2;z2] | step | variables.x | scalars
    bool have_const = false;      // (x2, z2) of the current factorisation is resident
};

// robust-order twin (minimum degree on K), created on the first factorisation that fails in the "variables last" order; every
// later factorisation still tries the fast order first.  Never touched by setup_device.
struct hipkkt_solver;
struct TwinState {
    hipkkt_solver *fallback = nullptr;
    bool using_fallback = false;
    bool force = false;           // FORCE_TWIN=1 at create (tests): see hipkkt_refactor
    // the twin's symbolic analysis runs on a host thread from the moment the cheap order is chosen (finish_create)
    bool device_ready = false;    // (a twin:) init_runtime + setup_device already ran on the speculation thread
    std::unique_ptr<hipkkt_solver> pending;
    std::future<std::string> future;
    std::shared_ptr<std::atomic<bool>> cancel;   // set when the twin turns out not to be needed
    std::shared_ptr<std::atomic<int>> go;        // 0: the owner has not chosen its order yet, 1: cheap order chosen (the twin may take device memory), 2: not needed
};

// statistics of a handle's life (hipkkt_get_timing / _get_counters / _get_profile): setup_device keeps them
struct SolverStats {
    double t_init_runtime = 0;           // seconds (HIPKKT_VERBOSE)
    double t_last_factor = 0, t_last_solve = 0, t_acc_factor = 0, t_acc_solve = 0, t_last_update = 0;
    int64_t n_factor = 0, n_solvecalls = 0, n_ldlsolves = 0, n_rhs_solved = 0, n_sweep_timeouts = 0;
    int64_t n_twin_refactors = 0;        // factorisations repeated on the robust-order twin
    int64_t n_accurate_factorisations = 0;   // factorisations with at least one refined block solve
    // last profiled refactorisation: the k_front_block launches; the dense update tiles / flops that rode in them (FB_EXTRA)
    double prof_fb_flops = 0, prof_fb_ms = 0, prof_extra_tiles = 0, prof_extra_flops = 0;
    int prof_fb_launches = 0, prof_fb_panels = 0;
    double prof_dense4_ms = 0, prof_dense4_flops = 0;   // ... k_update_dense<4,4> alone
    int prof_dense4_launches = 0;
    std::vector<double> prof_launch_ms, prof_launch_flops, prof_launch_tiles;   // ... per k_update_dense<4,4> launch
};
