// The schedule of one LDL solve: which supernodes go to which launch, in which order.  Plain host arithmetic on a HostPlan (no HIP):
// hipkkt_setup.cpp uploads it, hipkkt_solve.cpp walks it, tests/support/plan_check.cpp interprets it on the CPU.
#pragma once
#include "device_plan.h"   // kSlvRows, kSegRowTag: what the schedule shares with the solve kernels
#include "symbolic.h"

namespace hipkkt {

constexpr int kPersistMaxItems = 1024;     // a segment's persistent kernels take over from its first level with fewer forward items
// Narrow supernodes of a level go to the thread kernels from 256 on when the whole level is tiny, otherwise (childless supernodes
// only) from 2048 on: only worth it where the workgroup-per-item kernel would need several rounds of the chip.  A thread walks its
// w x (r - w) panel entries one strided load after the other: at most kNarrowMaxPanel of them.
constexpr unsigned kNarrowMinTiny = 256, kNarrowMinLeaves = 2048;
constexpr int kNarrowMaxPanel = 128;
constexpr int kSegRowTagHost = kSegRowTag;   // the name the plan interpreter of tests/support knows the tag by

// Level lists of the per-level solve kernels: ranges into slv_items / bwd_items / lvl_sn.  The first nnarrow[l] supernodes of a
// level's lvl_sn range are NARROW (one thread each, no items); wnarrow[l] is the widest of them.
struct LevelLists { std::vector<int> slv_ptr, bwd_ptr, reg_ptr, nnarrow, wnarrow; };

struct SolveSchedule {
    LevelLists regular;   // without the panels of the fronts (the persistent front kernels solve those)
    LevelLists all;       // EVERY supernode: the path without any persistent kernel, taken after a sweep time-out
    std::vector<FacItem> slv_items, bwd_items;   // blocks of kSlvRows rows (device_plan.h), both families appended
    std::vector<int> lvl_sn;
    std::vector<FacItem> pbwd_items;             // persistent backward sweep: blk == -1 is a supernode's finaliser
    std::vector<int64_t> p_off;                  // [nsuper + 1] partial sums of the backward blocks
    // persistent sweeps over the regular supernodes: segments = level ranges between front kernels
    int nseg = 0;
    std::vector<int> seg_of_level;               // [nlevels]
    std::vector<int> seg_lo, seg_hi, seg_lstar;  // per segment: level range [lo, hi] and the first level handled by the
                                                 // persistent kernels (wide bottom levels keep one launch per level)
    std::vector<int> fseg_ptr;                   // [2g] first persistent item of segment g in slv_items, [2g + 1] end
    std::vector<int> bseg_ptr;                   // [nseg + 1] into pbwd_items, indexed by LAUNCH order (segments descending)
    std::vector<int> sn_nitems, sn_bparent, dep_total, rows_seg;   // per supernode / per row slot: tables of the segment kernels
};

SolveSchedule build_solve_schedule(const HostPlan &P);

}  // namespace hipkkt
