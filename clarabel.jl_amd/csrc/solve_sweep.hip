// Triangular solves over the REGULAR supernodes (K5; everything that is not a panel of a front: front_sweep.hip):
//   k_permute_in                                first kernel of every LDL solve
//   k_fwd_level / k_bwd_partial / k_bwd_final   one launch per level (wide bottom levels, time-out fallback)
//   k_fwd_narrow / k_bwd_narrow                 one thread per narrow supernode of such a level
//   k_fwd_seg / k_bwd_seg                       persistent, ticket-ordered sweeps over a segment of levels
// The level kernels and the segment kernels run the same arithmetic in different accumulation forms, on purpose.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_plan.h"
#include "kernel_util.h"
#include "kernels.h"
#include "sweep_common.h"

namespace hipkkt {

// ------------------------------------------------------------------------------------------
// K5: triangular solves, level-scheduled ("wavefront") over the supernodal elimination tree.
// forward:  each supernode gathers the updates its descendants left in ubuf (fixed order),
//           solves with the unit-lower L11 inside one wavefront, publishes y_J and z_J = y_J/D,
//           and leaves its own update vector  u_s = L21 * y_J  in ubuf.
// backward: partial dot-products  L21^T x_R  per 256-row block, then a per-supernode finaliser
//           (fixed summation order) + unit-upper solve with L11^T.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_permute_in(const double *__restrict__ b, const int *__restrict__ perm, double *__restrict__ y, int n, int *epoch,
             int *ticks, int nticks, int *zero, int nzero) {
    // first kernel of every LDL solve: a new epoch invalidates the tagged hand-off values of the previous solve
    if (blockIdx.x == 0 && threadIdx.x == 0 && epoch) ((unsigned *)epoch)[0] += 1u;   // wraps after 2^32 solves: any
                                                                                        // two consecutive epochs differ
    // ... and the ticket words of the segment sweeps start from zero.  They are cleared HERE, by a kernel that runs
    // no atomics, and live in cache lines of their own (seg_sync layout): a plain store next to a word that other
    // workgroups are incrementing atomically can lose increments when the writer's L2 writes the line back (seen on
    // MI355X: duplicate tickets => the last items of a launch silently never ran).
    if (blockIdx.x == 0) {
        for (int q = threadIdx.x; q < nticks; q += blockDim.x) ticks[q] = 0;
        // the norm words the refinement kernels BEHIND this solve accumulate into with atomicMax (a launch of their own until round 6)
        for (int q = threadIdx.x; q < nzero; q += blockDim.x) zero[q] = 0;
    }
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) y[k] = b[perm[k]];
}

// One refinement step of a marked block's forward solve against the factored block itself (k_invert_diag_wide explains):
// yv += Linv (rhs - L yv); rhs, yv, scratch in LDS ([w] each), every thread of the workgroup calls it.
__device__ __forceinline__ void polish_fwd(const DevPlan &P, int s, int w, const double *rhs, double *yv, double *scratch) {
    const double *ldg = P.Ldiag + P.sn_diag[s], *li = P.Linv + P.sn_diag[s];
    const int tid = threadIdx.x;
    if (tid < w) {
        double a = rhs[tid] - yv[tid];
        for (int k2 = 0; k2 < tid; k2++) a -= ldg[tid + k2 * w] * yv[k2];
        scratch[tid] = a;
    }
    __syncthreads();
    double c = 0.0;
    if (tid < w)
        for (int k2 = 0; k2 <= tid; k2++) c += li[tid + k2 * w] * scratch[k2];
    __syncthreads();
    if (tid < w) yv[tid] += c;
    __syncthreads();
}
// the same for the backward solve: xv += Linv^T (tv - L^T xv)
__device__ __forceinline__ void polish_bwd(const DevPlan &P, int s, int w, const double *tv, double *xv, double *scratch) {
    const double *ldg = P.Ldiag + P.sn_diag[s], *lit = P.LinvT + P.sn_diag[s];
    const int tid = threadIdx.x;
    if (tid < w) {
        double a = tv[tid] - xv[tid];
        for (int i2 = tid + 1; i2 < w; i2++) a -= ldg[i2 + tid * w] * xv[i2];
        scratch[tid] = a;
    }
    __syncthreads();
    double c = 0.0;
    if (tid < w)
        for (int i2 = tid; i2 < w; i2++) c += lit[tid + i2 * w] * scratch[i2];
    __syncthreads();
    if (tid < w) xv[tid] += c;
    __syncthreads();
}

// Latency model behind these kernels (measured on MI355X, tools/ubench.hip): a dependent f64 FMA
// costs 32 cycles, an LDS round trip 60, an L2 hit ~220, HBM/MALL ~650, and one CU pulls only
// ~10 B/clk from HBM.  Hence: every dot product runs on 4 independent accumulators, and a panel is
// spread over as many workgroups as possible (kSlvRows = 64 rows each, device_plan.h) instead of a few 256-row blocks.

__global__ void __launch_bounds__(256)
k_fwd_level(DevPlan P, int item_begin, double *__restrict__ y, double *__restrict__ z) {
    __shared__ double rhs[kMaxSnWidth];
    __shared__ double part[4][kMaxSnWidth];
    __shared__ double yv[kMaxSnWidth];
    const FacItem it = P.slv_items[item_begin + blockIdx.x];
    const int s = it.sn;
    const int f = P.sn_first[s];
    const int w = P.sn_first[s + 1] - f;
    const int64_t slot0 = P.sn_rowptr[s];
    const int r = (int)(P.sn_rowptr[s + 1] - slot0);
    const double *pan = P.Lx + P.sn_panel[s];
    const double *li = P.Linv + P.sn_diag[s];
    const int tid = threadIdx.x;
    const int i = tid & 63, pq = tid >> 6;
    // right-hand side of the diagonal block: b_J minus what the children pushed onto these rows
    if (tid < w) {
        double acc = 0.0;
        const int64_t g0 = P.g_ptr[slot0 + tid], g1 = P.g_ptr[slot0 + tid + 1];
        for (int64_t g = g0; g < g1; g++) acc += P.ubuf[P.g_idx[g]];
        rhs[tid] = y[f + tid] - acc;
    }
    // prefetch this thread's share of the row GEMV while the diagonal block is being solved
    const int row = w + it.blk * kSlvRows + i;
    double pv[16];
    double gsum = 0.0;
    if (row < r) {
        const double *pr = pan + row;
#pragma unroll
        for (int t = 0; t < 16; t++) {
            const int k = pq + 4 * t;
            pv[t] = k < w ? pr[(int64_t)k * r] : 0.0;
        }
        if (pq == 0) {
            const int64_t g0 = P.g_ptr[slot0 + row], g1 = P.g_ptr[slot0 + row + 1];
            for (int64_t g = g0; g < g1; g++) gsum += P.ubuf[P.g_idx[g]];
        }
    }
    __syncthreads();
    {   // y_J = L11^-1 rhs as a small lower-triangular GEMV (explicit inverse from k_invert_diag)
        double a0 = 0.0, a1 = 0.0;
        if (i < w) {
            int k = pq;
            for (; k + 4 <= i; k += 8) {
                a0 += li[i + k * w] * rhs[k];
                a1 += li[i + (k + 4) * w] * rhs[k + 4];
            }
            if (k <= i) a0 += li[i + k * w] * rhs[k];
        }
        part[pq][i] = a0 + a1;
    }
    __syncthreads();
    if (tid < w) {
        yv[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    } else if (tid < kMaxSnWidth) {
        yv[tid] = 0.0;   // padded columns multiply prefetched zeros: keep them finite
    }
    __syncthreads();
    if (P.sn_polish[s]) polish_fwd(P, s, w, rhs, yv, part[0]);           // (workgroup-uniform)
    if (tid < w && it.blk == 0) z[f + tid] = yv[tid] * P.Dinv[f + tid];   // y keeps the right-hand side: the other block items of
                                                                          // this supernode (same launch) may still have to read it
    // this panel's update vector = children's contributions passed through + L21 * y_J
    {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if (row < r) {
#pragma unroll
            for (int t = 0; t < 16; t += 4) {
                a0 += pv[t] * yv[(pq + 4 * t) & 63];
                a1 += pv[t + 1] * yv[(pq + 4 * t + 4) & 63];
                a2 += pv[t + 2] * yv[(pq + 4 * t + 8) & 63];
                a3 += pv[t + 3] * yv[(pq + 4 * t + 12) & 63];
            }
        }
        __syncthreads();
        part[pq][i] = (a0 + a1) + (a2 + a3);
    }
    __syncthreads();
    if (pq == 0 && row < r)
        P.ubuf[P.u_off[s] + (row - w)] = gsum + (((part[0][i] + part[1][i]) + part[2][i]) + part[3][i]);
}

// partial L21^T x over one block of <=64 off-diagonal rows, from the row-major copy LT:
// lane = column (coalesced), the row's x value is a wave-uniform broadcast.  red[4][64] is LDS.
__device__ __forceinline__ double bwd_block_dot(const DevPlan &P, int s, int w, int r, int blk,
                                                const double *__restrict__ x, double (*red)[kMaxSnWidth]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int *rows = P.sn_rows + P.sn_rowptr[s];
    const double *lt = P.LT + P.lt_off[s];
    const int lo = w + blk * kSlvRows + wave * 16;
    const int hi = min(min(r, lo + 16), w + (blk + 1) * kSlvRows);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (lane < w) {
        int i = lo;
        for (; i + 4 <= hi; i += 4) {
            a0 += lt[(int64_t)(i - w) * w + lane] * x[rows[i]];
            a1 += lt[(int64_t)(i + 1 - w) * w + lane] * x[rows[i + 1]];
            a2 += lt[(int64_t)(i + 2 - w) * w + lane] * x[rows[i + 2]];
            a3 += lt[(int64_t)(i + 3 - w) * w + lane] * x[rows[i + 3]];
        }
        for (; i < hi; i++) a0 += lt[(int64_t)(i - w) * w + lane] * x[rows[i]];
    }
    red[wave][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    return ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// K5 on a level of NARROW supernodes (w <= kNarrowW columns, <= kNarrowR rows below the diagonal block; the
// thousands of 1-2 column leaves of a sparse QP): one THREAD per supernode instead of one 256-thread workgroup --
// a level-0 launch of cfg 2a drops from 17884 workgroups (39 us) to 70.  Same arithmetic as k_fwd_level /
// k_bwd_final, sums taken in index order.
template <int NW>   // NW >= widest supernode of the launch (register arrays)
__global__ void __launch_bounds__(256)
k_fwd_narrow(DevPlan P, int sn_begin, int n, double *__restrict__ y, double *__restrict__ z) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int s = P.lvl_sn[sn_begin + t];
    const int f = P.sn_first[s];
    const int w = P.sn_first[s + 1] - f;
    const int64_t slot0 = P.sn_rowptr[s];
    const int r = (int)(P.sn_rowptr[s + 1] - slot0);
    const double *pan = P.Lx + P.sn_panel[s];
    const double *li = P.Linv + P.sn_diag[s];
    double rhs[NW], yv[NW];
#pragma unroll
    for (int k = 0; k < NW; k++) {
        rhs[k] = 0.0;
        if (k < w) {
            double acc = 0.0;
            for (int64_t g = P.g_ptr[slot0 + k]; g < P.g_ptr[slot0 + k + 1]; g++) acc += P.ubuf[P.g_idx[g]];
            rhs[k] = y[f + k] - acc;
        }
    }
#pragma unroll
    for (int i = 0; i < NW; i++) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k <= i; k++)
            if (i < w) v += li[i + k * w] * rhs[k];
        yv[i] = v;
        if (i < w) z[f + i] = v * P.Dinv[f + i];
    }
    double *u = P.ubuf + P.u_off[s];
    for (int row = w; row < r; row++) {
        double a = 0.0;
        for (int64_t g = P.g_ptr[slot0 + row]; g < P.g_ptr[slot0 + row + 1]; g++) a += P.ubuf[P.g_idx[g]];
#pragma unroll
        for (int k = 0; k < NW; k++)
            if (k < w) a += pan[row + (int64_t)k * r] * yv[k];
        u[row - w] = a;
    }
}

template <int NW>
__global__ void __launch_bounds__(256)
k_bwd_narrow(DevPlan P, int sn_begin, int n, const double *__restrict__ z, double *__restrict__ x, double *__restrict__ xout) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int s = P.lvl_sn[sn_begin + t];
    const int f = P.sn_first[s];
    const int w = P.sn_first[s + 1] - f;
    const int64_t slot0 = P.sn_rowptr[s];
    const int r = (int)(P.sn_rowptr[s + 1] - slot0);
    const int *rows = P.sn_rows + slot0;
    const double *lt = P.LT + P.lt_off[s];          // row-major: lt[(i - w) * w + k]
    const double *lit = P.LinvT + P.sn_diag[s];     // Linv[i][k] at [k + i * w]
    double tv[NW];
#pragma unroll
    for (int k = 0; k < NW; k++) tv[k] = k < w ? z[f + k] : 0.0;
    for (int i = w; i < r; i++) {
        const double xi = x[rows[i]];
#pragma unroll
        for (int k = 0; k < NW; k++)
            if (k < w) tv[k] -= lt[(int64_t)(i - w) * w + k] * xi;
    }
#pragma unroll
    for (int k = 0; k < NW; k++) {
        double v = 0.0;
#pragma unroll
        for (int i = k; i < NW; i++)
            if (i < w) v += lit[k + i * w] * tv[i];
        if (k < w) {
            x[f + k] = v;
            xout[P.perm[f + k]] = v;
        }
    }
}

// panels with more than one 64-row block: per-block partial sums
__global__ void __launch_bounds__(256)
k_bwd_partial(DevPlan P, int item_begin, const double *__restrict__ x) {
    __shared__ double red[4][kMaxSnWidth];
    const FacItem it = P.bwd_items[item_begin + blockIdx.x];
    const int s = it.sn;
    const int w = P.sn_first[s + 1] - P.sn_first[s];
    const int r = (int)(P.sn_rowptr[s + 1] - P.sn_rowptr[s]);
    const double v = bwd_block_dot(P, s, w, r, it.blk, x, red);
    if (threadIdx.x < w) P.pbuf[P.p_off[s] + (int64_t)it.blk * w + threadIdx.x] = v;
}

__global__ void __launch_bounds__(256)
k_bwd_final(DevPlan P, int sn_begin, const double *__restrict__ z, double *__restrict__ x,
            double *__restrict__ xout) {
    __shared__ double red[4][kMaxSnWidth];
    __shared__ double tv[kMaxSnWidth];
    const int s = P.lvl_sn[sn_begin + blockIdx.x];
    const int f = P.sn_first[s];
    const int w = P.sn_first[s + 1] - f;
    const int r = (int)(P.sn_rowptr[s + 1] - P.sn_rowptr[s]);
    const double *lit = P.LinvT + P.sn_diag[s];
    const int tid = threadIdx.x;
    const int k = tid & 63, pq = tid >> 6;
    const int nblk = (r - w + kSlvRows - 1) / kSlvRows;
    double acc = 0.0;
    if (nblk == 1) {
        acc = bwd_block_dot(P, s, w, r, 0, x, red);   // short panel: fused
        __syncthreads();
    } else if (nblk > 1) {
        double a = 0.0;
        if (k < w) {
            const double *pb = P.pbuf + P.p_off[s] + k;
            for (int b = pq; b < nblk; b += 4) a += pb[(int64_t)b * w];
        }
        red[pq][k] = a;
        __syncthreads();
        acc = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
        __syncthreads();
    }
    if (tid < w) tv[tid] = z[f + tid] - acc;
    __syncthreads();
    {   // x_J = L11^-T t :  x_k = sum_{i>=k} Linv[i][k] t_i ; LinvT holds Linv[i][k] at [k + i*w]
        double a0 = 0.0, a1 = 0.0;
        if (k < w) {
            int i = k + pq;
            for (; i + 4 < w; i += 8) {
                a0 += lit[k + i * w] * tv[i];
                a1 += lit[k + (i + 4) * w] * tv[i + 4];
            }
            if (i < w) a0 += lit[k + i * w] * tv[i];
        }
        red[pq][k] = a0 + a1;
    }
    __syncthreads();
    if (P.sn_polish[s]) {                                                 // (workgroup-uniform)
        __shared__ double xv[kMaxSnWidth];
        if (tid < w) xv[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        __syncthreads();
        polish_bwd(P, s, w, tv, xv, red[0]);
        if (tid < w) {
            x[f + tid] = xv[tid];
            xout[P.perm[f + tid]] = xv[tid];
        }
        return;
    }
    if (tid < w) {
        const double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        x[f + tid] = v;
        xout[P.perm[f + tid]] = v;
    }
}

// ------------------------------------------------------------------------------------------
// K5 over the REGULAR supernodes (everything that is not a front panel): level-free persistent sweeps.
// One launch per segment (= the levels between two front kernels) instead of one launch per level
// and kernel: workgroup tickets are handed out in level order, an item first waits for the completion
// counters of the supernodes it depends on (forward: its same-segment children; backward: its parent and,
// for the finaliser, the partial blocks of its own panel), then runs the same arithmetic as the
// level-scheduled kernels.  Data produced inside the launch (update vectors, partial sums, x) is written
// with agent-scope stores and read with agent-scope loads; counters are device-scope atomics.
// Deadlock freedom and bounded spins: as for the front kernels (front_sweep.hip; the give-up rule: sweep_common.h spin_go_on).
// Re-arming: k_permute_in clears the ticket words of every solve, the first backward launch of a solve clears the forward
// completion counters for the next one; the backward sweep has no counters (its hand-offs are keyed with the solve's epoch).
// ------------------------------------------------------------------------------------------
// fdone (device_plan.h seg_sync_layout): kSegSub arrays of nsuper counters.  The items of a child count themselves into its parent's counters, block b into array
// b mod kSegSub: the device serialises atomics on one word at ~11 ns each, and a supernode high in the tree of a random QP waits for
// the ~300 blocks of its children (3 us per level on one word).  The waiting thread adds the kSegSub words up.  Only for supernodes
// that wait for at least kSegSubMin blocks: eight polled words instead of one made the sweeps of the banded QP (2400 waiting
// workgroups, a few blocks per child) 5 % slower.
struct SegSync {
    int *ftick, *btick, *fdone, *err;
};
__device__ __forceinline__ SegSync seg_sync(const DevPlan &P, int nsuper) {
    const SegSyncLayout L = seg_sync_layout(P.nseg, nsuper);
    return {P.seg_sync + L.ftick, P.seg_sync + L.btick, P.seg_sync + L.fdone, P.seg_sync + L.err};
}
// thread 0 waits until the kSegSub counters of supernode s add up to `want` (relaxed polls); false on time-out / foreign failure
__device__ __forceinline__ bool seg_wait_sum(int *ctr, int stride, int want, int *err, int *failflag, unsigned lim) {
    for (unsigned spins = 0;; spins++) {
        int v[kSegSub];
#pragma unroll
        for (int k = 0; k < kSegSub; k++) v[k] = front_ld_flag(ctr + (int64_t)k * stride);
        int sum = 0;
#pragma unroll
        for (int k = 0; k < kSegSub; k++) sum += v[k];
        if (sum >= want) return true;
        if (!spin_go_on(spins + 1u, spins, err, failflag, lim)) return false;
        __builtin_amdgcn_s_sleep(1);
    }
}
// thread 0 waits until *ctr >= want (relaxed polls); false on time-out / foreign failure
__device__ __forceinline__ bool seg_wait(int *ctr, int want, int *err, int *failflag, unsigned lim) {
    for (unsigned spins = 0;; spins++) {
        if (front_ld_flag(ctr) >= want) return true;
        if (!spin_go_on(spins + 1u, spins, err, failflag, lim)) return false;
        __builtin_amdgcn_s_sleep(1);
    }
}
// Tagged hand-off inside a segment sweep: a value produced by one item and consumed by a later item of the SAME
// launch travels as a self-validating 16-byte slot (see FrontSlot) next to its plain copy, keyed with the solve's
// epoch so that the previous solve's slots are invalid without any re-arming.  The consumer polls the very values
// it needs -- no dependency counter, no "stores complete" wait before an atomic, no second round trip.
__device__ __forceinline__ unsigned long long seg_key(const DevPlan &P) {
    return kSlotKey ^ ((unsigned long long)(((const unsigned *)P.seg_epoch)[0] + 1u) * 0x9E3779B97F4A7C15ull);
}
__device__ __forceinline__ void seg_slot_st(FrontSlot *p, double v, unsigned long long key) {
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const unsigned long long b = (unsigned long long)__double_as_longlong(v), h = b ^ key;
    v4u r = {(unsigned)b, (unsigned)(b >> 32), (unsigned)h, (unsigned)(h >> 32)};
    // s_nop: the data VGPRs of a store wider than 64 bits must not be overwritten in the next wait states (the
    // compiler's hazard recogniser does not look inside inline asm and re-used them for an address right away)
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 2" : : "v"(p), "v"(r) : "memory");
}

__global__ void __launch_bounds__(256)
k_fwd_seg(DevPlan P, int seg, int item_begin, int nitems, int nsuper, double *__restrict__ y, double *__restrict__ z) {
    __shared__ double rhs[kMaxSnWidth];
    __shared__ double part[4][kMaxSnWidth];
    __shared__ double yv[kMaxSnWidth];
    __shared__ int tick, sb;              // the item's ticket; 1 = the item's dependencies are met
    const SegSync Y = seg_sync(P, nsuper);
    const int tid = threadIdx.x;
    // item = a ticket taken in arrival order (level order): an item only ever waits for items with lower tickets, whose
    // owners are therefore already running -- forward progress does not depend on the order in which the hardware
    // dispatches workgroups.  One atomic per workgroup (~11 ns each on one word); the wide bottom levels, where that
    // would add up, are not part of the persistent launches (solve_schedule.h kPersistMaxItems).
    if (tid == 0) tick = atomicAdd(Y.ftick + seg, 1);
    __syncthreads();
    const int t = tick;
    if (t >= nitems) return;
    const FacItem it = P.slv_items[item_begin + t];
    const int s = it.sn;
    const int f = P.sn_first[s];
    const int w = P.sn_first[s + 1] - f;
    const int64_t slot0 = P.sn_rowptr[s];
    const int r = (int)(P.sn_rowptr[s + 1] - slot0);
    const double *pan = P.Lx + P.sn_panel[s];
    const double *li = P.Linv + P.sn_diag[s];
    const int i = tid & 63, pq = tid >> 6;
    const int row = w + it.blk * kSlvRows + i;
    // ---- everything that does not depend on other workgroups is fetched BEFORE the dependency wait:
    //      Linv row, panel row, gather-list bounds and first indices, right-hand side
    double liv[16], pv[16];
#pragma unroll
    for (int t2 = 0; t2 < 16; t2++) {
        const int k = pq + 4 * t2;
        liv[t2] = (i < w && k <= i) ? li[i + k * w] : 0.0;
        pv[t2] = (row < r && k < w) ? pan[row + (int64_t)k * r] : 0.0;
    }
    // (kSegGath indices per slot: a row of a supernode high in the tree collects one entry per child that reaches it -- up to 12 on
    // the random QPs of the benchmark -- and every entry past the prefetched ones costs two dependent round trips, index then value,
    // on the critical path of the level)
    constexpr int kSegGath = 12;
    int64_t ga0 = 0, ga1 = 0, gb0 = 0, gb1 = 0;
    int ia[kSegGath], ib[kSegGath];                   // the first gather indices of this thread's slots
#pragma unroll
    for (int q = 0; q < kSegGath; q++) { ia[q] = 0; ib[q] = 0; }
    double yin = 0.0, dinv_own = 0.0;
    if (tid < w) {
        dinv_own = P.Dinv[f + tid];
        ga0 = P.g_ptr[slot0 + tid];
        ga1 = P.g_ptr[slot0 + tid + 1];
#pragma unroll
        for (int q = 0; q < kSegGath; q++)
            if (ga0 + q < ga1) ia[q] = P.g_idx[ga0 + q];
        yin = y[f + tid];
    }
    if (pq == 0 && row < r) {
        gb0 = P.g_ptr[slot0 + row];
        gb1 = P.g_ptr[slot0 + row + 1];
#pragma unroll
        for (int q = 0; q < kSegGath; q++)
            if (gb0 + q < gb1) ib[q] = P.g_idx[gb0 + q];
    }
    // ---- dependencies: every block of every same-segment child has been published; the children count
    //      themselves into THIS supernode's counter, so the wait is one poll loop on one word
    const int want = P.dep_total[s], fpar = P.sn_bparent[s];
    const int fsub = (fpar >= 0 && P.dep_total[fpar] >= kSegSubMin) ? (it.blk & (kSegSub - 1)) : 0;   // (read before the wait)
    if (tid == 0) {
        sb = (want == 0 || (want >= kSegSubMin ? seg_wait_sum(Y.fdone + s, nsuper, want, Y.err, P.flags + FL_FRONTFAIL, P.spin_limit)
                                               : seg_wait(Y.fdone + s, want, Y.err, P.flags + FL_FRONTFAIL, P.spin_limit))) ? 1 : 0;
        asm volatile("" ::: "memory");
    }
    __syncthreads();
    if (!sb) return;
    // the sums run left to right over the list (the first four always take part, absent entries as 0.0: the order of rounds 2 - 5)
    if (tid < w) {
        double u[kSegGath];
#pragma unroll
        for (int q = 0; q < kSegGath; q++) u[q] = ga0 + q < ga1 ? front_ld(P.ubuf + ia[q]) : 0.0;   // in flight together
        double acc = ((u[0] + u[1]) + u[2]) + u[3];
#pragma unroll
        for (int q = 4; q < kSegGath; q++)
            if (ga0 + q < ga1) acc += u[q];
        for (int64_t g = ga0 + kSegGath; g < ga1; g++) acc += front_ld(P.ubuf + P.g_idx[g]);
        rhs[tid] = yin - acc;
    } else if (tid < kMaxSnWidth) {
        rhs[tid] = 0.0;   // padded columns meet zero weights: keep them finite
    }
    double gsum = 0.0;
    if (pq == 0 && row < r) {
        double u[kSegGath];
#pragma unroll
        for (int q = 0; q < kSegGath; q++) u[q] = gb0 + q < gb1 ? front_ld(P.ubuf + ib[q]) : 0.0;
        gsum = ((u[0] + u[1]) + u[2]) + u[3];
#pragma unroll
        for (int q = 4; q < kSegGath; q++)
            if (gb0 + q < gb1) gsum += u[q];
        for (int64_t g = gb0 + kSegGath; g < gb1; g++) gsum += front_ld(P.ubuf + P.g_idx[g]);
    }
    __syncthreads();
    {   // y_J = L11^-1 rhs (explicit inverse; thread (i, pq) owns the columns k = pq + 4t <= i)
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int t2 = 0; t2 < 16; t2 += 2) {
            a0 += liv[t2] * rhs[(pq + 4 * t2) & 63];
            a1 += liv[t2 + 1] * rhs[(pq + 4 * t2 + 4) & 63];
        }
        part[pq][i] = a0 + a1;
    }
    __syncthreads();
    if (tid < w) {
        yv[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    } else if (tid < kMaxSnWidth) {
        yv[tid] = 0.0;
    }
    __syncthreads();
    if (P.sn_polish[s]) polish_fwd(P, s, w, rhs, yv, part[0]);   // (workgroup-uniform)
    if (tid < w && it.blk == 0) z[f + tid] = yv[tid] * dinv_own;   // y is never overwritten (see k_fwd_level)
    {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
        for (int t2 = 0; t2 < 16; t2 += 4) {
            a0 += pv[t2] * yv[(pq + 4 * t2) & 63];
            a1 += pv[t2 + 1] * yv[(pq + 4 * t2 + 4) & 63];
            a2 += pv[t2 + 2] * yv[(pq + 4 * t2 + 8) & 63];
            a3 += pv[t2 + 3] * yv[(pq + 4 * t2 + 12) & 63];
        }
        __syncthreads();
        part[pq][i] = (a0 + a1) + (a2 + a3);
    }
    __syncthreads();
    if (pq == 0 && row < r)
        front_st(P.ubuf + P.u_off[s] + (row - w), gsum + (((part[0][i] + part[1][i]) + part[2][i]) + part[3][i]));
    // publish: the storing wave drains its stores, then one device-scope increment
    if (pq == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0 && fpar >= 0) atomicAdd(Y.fdone + (int64_t)fsub * nsuper + fpar, 1);
}

// backward: item.blk >= 0 = partial dot products of one 64-row block of a long panel, item.blk == -1 = the
// supernode's finaliser (short panels: fused dot product)
__global__ void __launch_bounds__(256)
k_bwd_seg(DevPlan P, int seg, int item_begin, int nitems, int nsuper, int first_launch, const double *__restrict__ z,
          double *__restrict__ x, double *__restrict__ xout) {
    __shared__ double red[4][kMaxSnWidth];
    __shared__ double tv[kMaxSnWidth];
    __shared__ int bad;
    const SegSync Y = seg_sync(P, nsuper);
    const int tid = threadIdx.x;
    __shared__ int tick;
    if (tid == 0) { bad = 0; tick = atomicAdd(Y.btick + seg, 1); }   // see k_fwd_seg
    __syncthreads();                // `bad` may be set by any wave from here on
    const int t = tick;
    if (t >= nitems) return;
    if (first_launch) {             // re-arm the forward sweep's counters for the next solve, every workgroup a share
        for (int q = t * 256 + tid; q < kSegSub * nsuper; q += nitems * 256) Y.fdone[q] = 0;
    }
    const unsigned long long key = seg_key(P);
    const FacItem it = P.pbwd_items[item_begin + t];
    const int s = it.sn;
    const int f = P.sn_first[s];
    const int w = P.sn_first[s + 1] - f;
    const int r = (int)(P.sn_rowptr[s + 1] - P.sn_rowptr[s]);
    const int nblk = (r - w + kSlvRows - 1) / kSlvRows;
    const int lane = tid & 63, wave = tid >> 6;
    const int *rows = P.rows_seg + P.sn_rowptr[s];   // sn_rows with kSegRowTag on the rows solved inside this launch
    const double *lt = P.LT + P.lt_off[s];
    // ---- static data first: the 16 rows x 1 column of L21^T this thread multiplies, their row indices (and the x
    //      values that were final before this launch), the column of Linv^T and z (finaliser)
    const bool dot_here = it.blk >= 0 || nblk == 1;
    const int blk = it.blk >= 0 ? it.blk : 0;
    const int lo = w + blk * kSlvRows + wave * 16;
    double lv[16], xv[16];
    int ri[16];
#pragma unroll
    for (int t2 = 0; t2 < 16; t2++) {
        const int i = lo + t2;
        const bool in = dot_here && i < r && i < w + (blk + 1) * kSlvRows;
        ri[t2] = in ? rows[i] : -1;
        lv[t2] = (in && lane < w) ? lt[(int64_t)(i - w) * w + lane] : 0.0;
        xv[t2] = (ri[t2] >= 0 && !(ri[t2] & kSegRowTag)) ? x[ri[t2]] : 0.0;
    }
    int ri_lane = -1;   // row lo + (lane & 15) of this wave's 16 rows, for the tagged polls
    {
        const int i = lo + (lane & 15);
        if (dot_here && i < r && i < w + (blk + 1) * kSlvRows) ri_lane = rows[i];
    }
    double litv[16];
    double zin = 0.0;
    int perm_own = 0;
    if (it.blk < 0) {
        if (tid < w) perm_own = P.perm[f + tid];
        const double *lit = P.LinvT + P.sn_diag[s];
#pragma unroll
        for (int t2 = 0; t2 < 16; t2++) {
            const int i2 = wave + 4 * t2;
            litv[t2] = (lane < w && i2 >= lane && i2 < w) ? lit[lane + i2 * w] : 0.0;
        }
        if (tid < w) zin = z[f + tid];
    } else {
#pragma unroll
        for (int t2 = 0; t2 < 16; t2++) litv[t2] = 0.0;
    }
    // ---- dependencies = the tagged x values (ancestors solved inside this launch) and partial sums themselves
    bool ok = true;
    double dotv = 0.0;
    if (dot_here) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        {   // lane l < 16 polls the slot of row lo + l (ONE load instruction per round for the wave's 16 rows); the
            // values are then broadcast to all lanes
            const int rl = ri_lane;                       // this lane's row (tagged index) or -1
            const bool mine = lane < 16 && rl >= 0 && (rl & kSegRowTag);
            double myv = 0.0;
            bool got = !mine;
            unsigned spins = 0;
            while (ok) {
                if (!got) {
                    const FrontSlot sl = front_slot_ld(P.xseg + (rl & ~kSegRowTag));
                    if (((unsigned long long)__double_as_longlong(sl.v) ^ sl.h) == key) { myv = sl.v; got = true; }
                }
                if (__ballot(!got) == 0ull) break;
                ++spins;
                ok = spin_go_on(spins, spins, Y.err, P.flags + FL_FRONTFAIL, P.spin_limit);
            }
#pragma unroll
            for (int t2 = 0; t2 < 16; t2++) {
                const double bv = readlane_f64(myv, t2);
                if (ri[t2] >= 0 && (ri[t2] & kSegRowTag)) xv[t2] = bv;
            }
        }
        if (!ok) { bad = 1; atomicOr(P.flags + FL_FRONTFAIL, 4); }   // bit 2: the backward segment sweep gave up
#pragma unroll
        for (int t2 = 0; t2 < 16; t2 += 4) {
            a0 = fma(lv[t2], xv[t2], a0);
            a1 = fma(lv[t2 + 1], xv[t2 + 1], a1);
            a2 = fma(lv[t2 + 2], xv[t2 + 2], a2);
            a3 = fma(lv[t2 + 3], xv[t2 + 3], a3);
        }
        red[wave][lane] = (a0 + a1) + (a2 + a3);
        __syncthreads();
        if (bad) return;
        dotv = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
        __syncthreads();
    }
    if (it.blk >= 0) {   // partial item: its w sums travel to the finaliser as tagged slots
        if (tid < w) seg_slot_st(P.pseg + P.p_off[s] + (int64_t)it.blk * w + tid, dotv, key);
        return;
    }
    double acc = dotv;
    if (nblk > 1) {
        double a = 0.0;
        if (lane < w) {
            // kSegPoll slots per wavefront and round trip (round 6: one dependent poll per block made the finaliser of a 4500-row
            // panel wait 18 round trips after the last partial sum had arrived); the sum still runs over b2 = wave, wave + 4, ... in order
            constexpr int kSegPoll = 8;
            const FrontSlot *pb = P.pseg + P.p_off[s] + lane;
            for (int b0 = wave; b0 < nblk && ok; b0 += 4 * kSegPoll) {
                double v[kSegPoll];
                bool got[kSegPoll];
#pragma unroll
                for (int u = 0; u < kSegPoll; u++) { v[u] = 0.0; got[u] = b0 + 4 * u >= nblk; }
                unsigned spins = 0;
                while (true) {
                    bool all = true;
#pragma unroll
                    for (int u = 0; u < kSegPoll; u++) {
                        if (!got[u]) {
                            const FrontSlot sl = front_slot_ld(pb + (int64_t)(b0 + 4 * u) * w);
                            if (((unsigned long long)__double_as_longlong(sl.v) ^ sl.h) == key) { v[u] = sl.v; got[u] = true; }
                            else all = false;
                        }
                    }
                    if (all) break;
                    ++spins;
                    ok = spin_go_on(spins, spins, Y.err, P.flags + FL_FRONTFAIL, P.spin_limit);
                    if (!ok) break;
                }
#pragma unroll
                for (int u = 0; u < kSegPoll; u++)
                    if (b0 + 4 * u < nblk) a += v[u];
            }
        }
        if (!ok) { bad = 1; atomicOr(P.flags + FL_FRONTFAIL, 4); }   // bit 2: the backward segment sweep gave up
        red[wave][lane] = a;
        __syncthreads();
        if (bad) return;
        acc = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
        __syncthreads();
    }
    if (tid < kMaxSnWidth) tv[tid] = tid < w ? zin - acc : 0.0;
    __syncthreads();
    {   // x_J = Linv^T t
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int t2 = 0; t2 < 16; t2 += 2) {
            s0 = fma(litv[t2], tv[(wave + 4 * t2) & 63], s0);
            s1 = fma(litv[t2 + 1], tv[(wave + 4 * t2 + 4) & 63], s1);
        }
        red[wave][lane] = s0 + s1;
    }
    __syncthreads();
    if (P.sn_polish[s]) {                                                 // (workgroup-uniform; k_invert_diag_wide explains)
        __shared__ double xv[kMaxSnWidth];
        if (tid < w) xv[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        __syncthreads();
        polish_bwd(P, s, w, tv, xv, red[0]);
        if (tid < w) {
            seg_slot_st(P.xseg + f + tid, xv[tid], key);
            x[f + tid] = xv[tid];
            xout[perm_own] = xv[tid];
        }
        return;
    }
    if (tid < w) {   // publish: tagged slot for the descendants solved in this launch, plain copy for everybody else
        const double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        seg_slot_st(P.xseg + f + tid, v, key);
        x[f + tid] = v;
        xout[perm_own] = v;
    }
}

// ------------------------------------------------------------------------------------------
// host-callable launchers (used by the hipkkt_*.cpp host files; all launches go to the handle's stream)
// ------------------------------------------------------------------------------------------
void launch_fwd_narrow(hipStream_t st, const DevPlan &P, int sn_begin, int n, int wmax, double *y, double *z) {
    if (n <= 0) return;
    if (wmax <= 4) hipLaunchKernelGGL(k_fwd_narrow<4>, dim3(nblk(n)), dim3(256), 0, st, P, sn_begin, n, y, z);
    else hipLaunchKernelGGL(k_fwd_narrow<kNarrowW>, dim3(nblk(n)), dim3(256), 0, st, P, sn_begin, n, y, z);
}
void launch_bwd_narrow(hipStream_t st, const DevPlan &P, int sn_begin, int n, int wmax, const double *z, double *x, double *xout) {
    if (n <= 0) return;
    if (wmax <= 4) hipLaunchKernelGGL(k_bwd_narrow<4>, dim3(nblk(n)), dim3(256), 0, st, P, sn_begin, n, z, x, xout);
    else hipLaunchKernelGGL(k_bwd_narrow<kNarrowW>, dim3(nblk(n)), dim3(256), 0, st, P, sn_begin, n, z, x, xout);
}
void launch_permute_in(hipStream_t st, const double *b, const int *perm, double *y, int n, int *epoch, int *ticks, int nticks, int *zero, int nzero) {
    if (n > 0) hipLaunchKernelGGL(k_permute_in, dim3(nblk(n)), dim3(256), 0, st, b, perm, y, n, epoch, ticks, nticks, zero, nzero);
}
void launch_fwd_level(hipStream_t st, const DevPlan &P, int item_begin, int nitems, double *y, double *z) {
    if (nitems > 0) hipLaunchKernelGGL(k_fwd_level, dim3(nitems), dim3(256), 0, st, P, item_begin, y, z);
}
void launch_bwd_partial(hipStream_t st, const DevPlan &P, int item_begin, int nitems, const double *x) {
    if (nitems > 0) hipLaunchKernelGGL(k_bwd_partial, dim3(nitems), dim3(256), 0, st, P, item_begin, x);
}
void launch_bwd_final(hipStream_t st, const DevPlan &P, int sn_begin, int nsn, const double *z, double *x, double *xout) {
    if (nsn > 0) hipLaunchKernelGGL(k_bwd_final, dim3(nsn), dim3(256), 0, st, P, sn_begin, z, x, xout);
}
void launch_fwd_seg(hipStream_t st, const DevPlan &P, int seg, int item_begin, int nitems, int nsuper, double *y, double *z) {
    if (nitems > 0) hipLaunchKernelGGL(k_fwd_seg, dim3(nitems), dim3(256), 0, st, P, seg, item_begin, nitems, nsuper, y, z);
}
void launch_bwd_seg(hipStream_t st, const DevPlan &P, int seg, int item_begin, int nitems, int nsuper, int first, const double *z,
                    double *x, double *xout) {
    if (nitems > 0) hipLaunchKernelGGL(k_bwd_seg, dim3(nitems), dim3(256), 0, st, P, seg, item_begin, nitems, nsuper, first, z, x, xout);
}

}  // namespace hipkkt
