// The solve schedule of a symbolic plan (solve_schedule.h).
#include "solve_schedule.h"

#include <algorithm>

namespace hipkkt {

namespace {
inline int width_of(const HostPlan &P, int s) { return P.sn_first[s + 1] - P.sn_first[s]; }
inline int64_t rows_of(const HostPlan &P, int s) { return P.sn_rowptr[s + 1] - P.sn_rowptr[s]; }
// forward items of a supernode: blocks of kSlvRows rows below its diagonal block
inline int nitems_of(const HostPlan &P, int s) { return (int)std::max<int64_t>(1, (rows_of(P, s) - width_of(P, s) + kSlvRows - 1) / kSlvRows); }

// Segments of the persistent sweeps = level ranges between two front kernels; inside a segment the wide bottom levels (thousands of
// leaf supernodes) are cheaper as one launch per level, the persistent kernels take over from the first level with fewer than
// kPersistMaxItems items (seg_lstar)
void build_segments(const HostPlan &P, SolveSchedule &H) {
    H.seg_of_level.assign(P.nlevels, 0);
    std::vector<char> boundary(P.nlevels + 1, 0);
    for (const FrontDesc &F : P.fronts) boundary[F.level_last] = 1;   // the front runs after regular level level_last
    int sg = 0;
    for (int l = 0; l < P.nlevels; l++) { H.seg_of_level[l] = sg; if (boundary[l]) sg++; }
    H.nseg = sg + 1;
    std::vector<int> lvl_items(P.nlevels, 0);      // forward items of the regular (non-front) supernodes of a level
    for (int s = 0; s < P.nsuper; s++)
        if (P.sn_front[s] < 0) lvl_items[P.sn_level[s]] += nitems_of(P, s);
    H.seg_lo.assign(H.nseg, P.nlevels); H.seg_hi.assign(H.nseg, -1); H.seg_lstar.assign(H.nseg, 0);
    for (int l = P.nlevels - 1; l >= 0; l--) H.seg_lo[H.seg_of_level[l]] = l;
    for (int l = 0; l < P.nlevels; l++) H.seg_hi[H.seg_of_level[l]] = l;
    for (int g = 0; g < H.nseg; g++) {
        int ls = H.seg_lo[g];
        while (ls <= H.seg_hi[g] && lvl_items[ls] >= kPersistMaxItems) ls++;
        H.seg_lstar[g] = ls;
    }
}

// Level lists of the per-level solve kernels, appended to slv_items / bwd_items / lvl_sn.  On a level that gets its own launches the
// NARROW supernodes are listed first and solved one THREAD each (k_fwd_narrow / k_bwd_narrow); they have no items.
void build_level_lists(const HostPlan &P, SolveSchedule &H, const std::vector<char> &has_child, bool with_fronts, LevelLists &L) {
    L.slv_ptr.assign(P.nlevels + 1, (int)H.slv_items.size());
    L.bwd_ptr.assign(P.nlevels + 1, (int)H.bwd_items.size());
    L.reg_ptr.assign(P.nlevels + 1, (int)H.lvl_sn.size());
    L.nnarrow.assign(P.nlevels, 0); L.wnarrow.assign(P.nlevels, 1);
    std::vector<int> nar, reg;
    for (int l = 0; l < P.nlevels; l++) {
        const bool own_launches = with_fronts || l < H.seg_lstar[H.seg_of_level[l]];
        nar.clear(); reg.clear();
        bool all_tiny = true;    // every supernode of the level has <= 4 columns and <= 16 rows below the block
        for (int q = P.lvl_ptr[l]; q < P.lvl_ptr[l + 1]; q++) {
            const int s = P.lvl_sn[q];
            if (!with_fronts && P.sn_front[s] >= 0) continue;      // solved by the persistent front kernels
            all_tiny = all_tiny && width_of(P, s) <= 4 && rows_of(P, s) - width_of(P, s) <= 16;
        }
        for (int q = P.lvl_ptr[l]; q < P.lvl_ptr[l + 1]; q++) {
            const int s = P.lvl_sn[q], w = width_of(P, s);
            if (!with_fronts && P.sn_front[s] >= 0) continue;
            const int64_t r = rows_of(P, s);
            // one thread per supernode pays for every gather of a child's update vector with a serial memory round trip: a level goes
            // to the thread kernels as a whole when all of it is tiny; otherwise only its childless supernodes (leaves: nothing to
            // gather) do, up to kNarrowW x kNarrowR (the thresholds: solve_schedule.h)
            const bool thr = all_tiny || (!has_child[s] && w <= kNarrowW && r - w <= kNarrowR && (int64_t)w * (r - w) <= kNarrowMaxPanel);
            (own_launches && thr ? nar : reg).push_back(s);
        }
        if (nar.size() < (all_tiny ? kNarrowMinTiny : kNarrowMinLeaves)) { reg.insert(reg.end(), nar.begin(), nar.end()); std::sort(reg.begin(), reg.end()); nar.clear(); }
        L.nnarrow[l] = (int)nar.size();
        for (int s : nar) L.wnarrow[l] = std::max(L.wnarrow[l], width_of(P, s));
        H.lvl_sn.insert(H.lvl_sn.end(), nar.begin(), nar.end());
        for (int s : reg) {
            const int nb = nitems_of(P, s);
            for (int b = 0; b < nb; b++) H.slv_items.push_back({s, b});
            if (nb > 1)
                for (int b = 0; b < nb; b++) H.bwd_items.push_back({s, b});
            H.lvl_sn.push_back(s);
        }
        L.slv_ptr[l + 1] = (int)H.slv_items.size();
        L.bwd_ptr[l + 1] = (int)H.bwd_items.size();
        L.reg_ptr[l + 1] = (int)H.lvl_sn.size();
    }
}

// ---- persistent sweeps: dependency counts, row tags, forward ranges, backward item order
void build_segment_sweeps(const HostPlan &P, SolveSchedule &H) {
    auto seg_of = [&](int s) { return H.seg_of_level[P.sn_level[s]]; };
    auto persistent = [&](int s) { return P.sn_level[s] >= H.seg_lstar[seg_of(s)]; };
    H.sn_nitems.assign(P.nsuper, 0); H.sn_bparent.assign(P.nsuper, -1); H.dep_total.assign(P.nsuper, 0);
    for (int c = 0; c < P.nsuper; c++) {
        const int p = P.sn_parent[c];
        if (P.sn_front[c] >= 0) continue;
        H.sn_nitems[c] = nitems_of(P, c);
        if (p >= 0 && P.sn_front[p] < 0 && seg_of(p) == seg_of(c) && persistent(c) && persistent(p)) {
            H.dep_total[p] += H.sn_nitems[c];      // a parent waits for every item of its children of the same launch
            H.sn_bparent[c] = p;
        }
    }
    // tagged hand-off of the persistent backward sweep: mark the rows whose x is produced inside the same launch
    auto in_seg_kernel = [&](int s) { return P.sn_front[s] < 0 && persistent(s); };
    std::vector<int> col_sn(P.N, -1);
    for (int c = 0; c < P.nsuper; c++)
        for (int k = P.sn_first[c]; k < P.sn_first[c + 1]; k++) col_sn[k] = c;
    H.rows_seg.assign(P.sn_rows.begin(), P.sn_rows.end());
    for (int s = 0; s < P.nsuper; s++) {
        if (!in_seg_kernel(s)) continue;
        for (int64_t slot = P.sn_rowptr[s]; slot < P.sn_rowptr[s + 1]; slot++) {
            const int a = col_sn[P.sn_rows[slot]];
            if (a != s && a >= 0 && in_seg_kernel(a) && seg_of(a) == seg_of(s)) H.rows_seg[(size_t)slot] = P.sn_rows[slot] | kSegRowTag;
        }
    }
    // forward segments: slv_items is level-ordered, a segment is a level range
    const LevelLists &L = H.regular;
    H.fseg_ptr.assign(2 * H.nseg, 0);
    for (int g = 0; g < H.nseg; g++) {
        const int ls = std::min(H.seg_lstar[g], P.nlevels);
        H.fseg_ptr[2 * g] = H.seg_hi[g] >= 0 ? L.slv_ptr[std::min(ls, H.seg_hi[g] + 1)] : 0;
        H.fseg_ptr[2 * g + 1] = H.seg_hi[g] >= 0 ? L.slv_ptr[H.seg_hi[g] + 1] : 0;
    }
    // backward items: segments in DESCENDING order of level; inside a segment levels descending, partial blocks before finalisers
    H.bseg_ptr.assign(H.nseg + 1, 0);
    for (int g = H.nseg - 1; g >= 0; g--) {
        for (int l = P.nlevels - 1; l >= 0; l--) {
            if (H.seg_of_level[l] != g || l < H.seg_lstar[g]) continue;
            for (int q = L.reg_ptr[l]; q < L.reg_ptr[l + 1]; q++) {
                const int s = H.lvl_sn[q];
                if (H.sn_nitems[s] > 1)
                    for (int b = 0; b < H.sn_nitems[s]; b++) H.pbwd_items.push_back({s, b});
            }
            for (int q = L.reg_ptr[l]; q < L.reg_ptr[l + 1]; q++) H.pbwd_items.push_back({H.lvl_sn[q], -1});
        }
        H.bseg_ptr[H.nseg - g] = (int)H.pbwd_items.size();
    }
}
}  // namespace

SolveSchedule build_solve_schedule(const HostPlan &P) {
    SolveSchedule H;
    H.p_off.assign(P.nsuper + 1, 0);
    for (int s = 0; s < P.nsuper; s++) H.p_off[s + 1] = H.p_off[s] + (int64_t)nitems_of(P, s) * width_of(P, s);
    build_segments(P, H);
    std::vector<char> has_child(P.nsuper, 0);
    for (int c = 0; c < P.nsuper; c++)
        if (P.sn_parent[c] >= 0) has_child[P.sn_parent[c]] = 1;
    build_level_lists(P, H, has_child, false, H.regular);
    build_level_lists(P, H, has_child, true, H.all);
    build_segment_sweeps(P, H);
    return H;
}

}  // namespace hipkkt
