// The numeric factorisation of the KKT path for gfx950 (MI355X / CDNA4).  See DESIGN.md section 5 for the roofline that bounds
// each kernel.  Everything is Float64; indices are int32 except panel offsets (int64).  The other stages of the path: values.hip
// (value updates, K1-K2), solve_sweep.hip and front_sweep.hip (triangular solves, K5), refine.hip (SpMV, refinement, residuals,
// K6-K8), assemble_dev.hip (KKT assembly); front_block2.hip factors the fronts' update batches.
//
//   regulariser      k_maxabs_gather + k_init_panels (+-eps folded into the K -> panel scatter)  (K3)
//   numeric LDL^T     k_factor_panel (w > 8: register-resident, 8-pivot blocks), k_factor_level   (K4, dependency latency)
//                     k_update_dense<NT,NR> (FP64 matrix-core tiles: <4,4> far, <1,2> just in time), k_update_gather
//                     (per-entry lists of the leaves), k_update_stage (relative-index scatter, fallback)   (K4, MFMA)
//                     k_invert_diag / k_invert_diag_wide (explicit inverses of the diagonal blocks for the solves)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "device_plan.h"
#include "kernel_util.h"
#include "kernels.h"
#include "dense_tile.h"

namespace hipkkt {

// ------------------------------------------------------------------------------------------
// K3: static regulariser eps = c + p * max|diag K|  (ref: kktsolver_directldl.jl:297-310)
// scal[SC_MAXDIAG] must be zeroed before the launch
// ------------------------------------------------------------------------------------------
__global__ void k_maxabs_gather(const double *__restrict__ v, const int64_t *__restrict__ idx, int64_t n,
                                unsigned long long *__restrict__ slot) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double a = 0.0;
    if (i < n) a = fabs(idx ? v[idx[i]] : v[i]);
    block_atomic_max_abs(slot, a);
}

// Lx <- scatter(K) with the +-eps shift on the diagonal (the resident Kval stays unregularised:
// kktsolver_directldl.jl:285-291 restores the diagonal for the refinement step)
__global__ void k_init_panels(double *__restrict__ Lx, const double *__restrict__ kval,
                              const int64_t *__restrict__ kmap, const signed char *__restrict__ kdiag_sign,
                              int64_t nnz, const double *__restrict__ scal, int static_enable,
                              double eps_const, double eps_prop) {
    int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nnz) return;
    double v = kval[q];
    int sg = kdiag_sign[q];
    if (static_enable && sg != 0) {
        double maxdiag = __longlong_as_double((long long)((const unsigned long long *)scal)[SC_MAXDIAG]);
        double eps = eps_const + eps_prop * maxdiag;
        v += sg > 0 ? eps : -eps;
    }
    Lx[kmap[q]] = v;
}

// ------------------------------------------------------------------------------------------
// K4a: per-level panel factorisation.  One workgroup per (supernode, 64-row chunk).
// Every workgroup of a supernode refactors the w x w diagonal block redundantly in LDS
// (bit-identical results, no inter-workgroup hand-off inside the launch); chunk 0 publishes
// L11 / D / Dinv, every chunk solves its own rows  L21 = A21 L11^-T D^-1  in place.
// Pivot rule = QDLDL's: if D_k * sign_k < eps then D_k = delta * sign_k   (SURVEY.md App. C).
// ------------------------------------------------------------------------------------------
constexpr int LDT = kFacRows + 8;      // LDS leading dimension of the TRSM tile [k][row]

// dynamic LDS is sized for the widest supernode of the level (wmax): Aw[wmax][wmax+1], dd[wmax], T[wmax][LDT]
__global__ void __launch_bounds__(256)
k_factor_level(DevPlan P, int item_begin, int wmax, double dyn_eps, double dyn_delta) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int LDW = wmax + 1;                  // LDS leading dimension of the diagonal block
    double *Aw = smem;                         // [wmax * LDW]
    double *dd = Aw + wmax * LDW;              // [wmax] pivots
    double *T = dd + wmax;                     // [wmax * LDT]
    const FacItem it = P.fac_items[item_begin + blockIdx.x];
    const int s = it.sn;
    const int f = P.sn_first[s];
    const int w = P.sn_first[s + 1] - f;
    const int r = (int)(P.sn_rowptr[s + 1] - P.sn_rowptr[s]);
    double *pan = P.Lx + P.sn_panel[s];
    const int tid = threadIdx.x;

    for (int idx = tid; idx < w * w; idx += 256) {
        int i = idx % w, j = idx / w;
        Aw[i + j * LDW] = pan[i + (int64_t)j * r];
    }
    __syncthreads();
    // right-looking LDL^T of the lower triangle; thread (ti,tj): row k+1+ti, columns k+1+tj (+4...)
    const int ti = tid & 63, tj = tid >> 6;
    int nreg = 0;
    for (int k = 0; k < w; k++) {
        double d = Aw[k + k * LDW];
        const double sg = (double)P.sgn_perm[f + k];
        if (d * sg < dyn_eps) { d = dyn_delta * sg; nreg++; }
        const double dinv = 1.0 / d;
        if (tid == 0) dd[k] = d;
        const int i = k + 1 + ti;
        if (i < w) {
            const double aik = Aw[i + k * LDW];
            for (int j = k + 1 + tj; j <= i; j += 4) Aw[i + j * LDW] -= aik * (Aw[j + k * LDW] * dinv);
        }
        __syncthreads();
    }
    // scale columns: L11 = A11_lower * D^-1
    for (int idx = tid; idx < w * w; idx += 256) {
        int i = idx % w, k = idx / w;
        if (i > k) Aw[i + k * LDW] /= dd[k];
    }
    __syncthreads();
    if (it.blk == 0) {
        double *ld = P.Ldiag + P.sn_diag[s];
        for (int idx = tid; idx < w * w; idx += 256) {
            int i = idx % w, k = idx / w;
            ld[idx] = i > k ? Aw[i + k * LDW] : (i == k ? 1.0 : 0.0);
        }
        if (tid < w) {
            P.D[f + tid] = dd[tid];
            P.Dinv[f + tid] = 1.0 / dd[tid];
            if (!isfinite(1.0 / dd[tid])) atomicOr(P.flags + FL_NONFINITE, 1);
        }
        if (tid == 0 && nreg) atomicAdd(P.flags + FL_NREG, nreg);
    }
    // TRSM on this chunk's rows: 4 lanes per row, y_k = a_k - sum_{j<k} y_j L11[k][j]
    const int lo = w + it.blk * kFacRows;
    const int nr = min(kFacRows, r - lo);
    if (nr <= 0) return;
    for (int idx = tid; idx < nr * w; idx += 256) {
        int row = idx % nr, k = idx / nr;
        T[k * LDT + row] = pan[(lo + row) + (int64_t)k * r];
    }
    __syncthreads();
    {
        const int q = tid & 3;
        for (int row = tid >> 2; row < nr; row += 64) {
            for (int k = 0; k < w; k++) {
                double acc = 0.0;
                for (int j = q; j < k; j += 4) acc += T[j * LDT + row] * Aw[k + j * LDW];
                acc += __shfl_xor(acc, 1, 64);
                acc += __shfl_xor(acc, 2, 64);
                const double yk = T[k * LDT + row] - acc;
                T[k * LDT + row] = yk;  // all 4 lanes store the same value
            }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < nr * w; idx += 256) {
        int row = idx % nr, k = idx / nr;
        const double v = T[k * LDT + row] / dd[k];
        T[k * LDT + row] = v;
        pan[(lo + row) + (int64_t)k * r] = v;
    }
    __syncthreads();
    // row-major copy (w contiguous doubles per row) for the backward solve's L21^T x
    double *lt = P.LT + P.lt_off[s] + (int64_t)(lo - w) * w;
    for (int idx = tid; idx < nr * w; idx += 256) {
        int k = idx % w, row = idx / w;
        lt[idx] = T[k * LDT + row];
    }
}

// ------------------------------------------------------------------------------------------
// K4a, wide panels (w > 8): register-resident right-looking LDL^T of the whole panel chunk.
// 8 wavefronts: group D (waves 0-3) holds the w x w diagonal block, group O (waves 4-7) the chunk's
// 64 off-diagonal rows; lane = row, wave v of a group owns the columns j = v (mod 4) (16 registers).
// Step k: the owner waves publish column k through LDS (double buffered: one barrier per step),
// every wave forms l_ik = a_ik / d_k for its row and applies  a_ij -= l_ik * a_jk  to its own
// columns j > k.  The panel rows are eliminated with the same steps, so the TRSM costs no extra
// pass: L21[:,k] leaves the kernel at step k.  The critical path per pivot is
// LDS write -> barrier -> LDS read -> 1/d (112 clk) -> mul -> fma  (~400 clk; tools/ubench.hip).
// Pivot rule = QDLDL's.  Every chunk repeats the diagonal block (bit-identical).
// ------------------------------------------------------------------------------------------

// 1/d on the pivot-to-pivot critical path: pivot_rcp / pivot_rcp3 (kernel_util.h) instead of the IEEE division sequence.

// Blocked by 8 pivots: wave v of a group owns the column blocks {v, v+4} (8 columns each).  The owner of block B
// eliminates its 8 columns WITHOUT leaving the wavefront (pivot and the entries a_jk come from the lanes that hold
// them: v_readlane), publishes the block's L columns / raw columns / 1/d through LDS, and after ONE barrier every
// wave applies the rank-8 update to its own live blocks; the chunk rows (group O) follow with the published
// values and a second barrier.  16 barriers per 64-column panel instead of 64, and only the 8x8 triangle of the
// current block sits on the pivot-to-pivot critical path.

// Round 6: TWO workgroups per compute unit (62 KB of LDS instead of 96, <= 128 registers).  A level of many panels -- the 20 cone
// chains of an SDP: 400 items per level on cfg 5 -- ran in two rounds of one workgroup per compute unit, 31 us per level against the
// 15 us one round takes.  What went: the staging tile of the factored diagonal block (its columns now go from the published L columns
// in LDS straight to Ldiag, by a wavefront that is not on the pivot chain, inside the loop -- whose barrier therefore no longer waits
// for global memory: lds_barrier, kernel_util.h).

__global__ void __launch_bounds__(512, 4)                 // (HIP: the second figure is wavefronts per SIMD: 4 = two of these workgroups per compute unit)
k_factor_panel(DevPlan P, int item_begin, double dyn_eps, double dyn_delta) {
    __shared__ double colL[2][8][64];     // l_ik of the diagonal-block rows of block B          (parity B & 1)
    __shared__ double colC[3][8][64];     // raw a_ik = d_k l_ik of the diagonal-block rows        (B % 3: read for two iterations)
    __shared__ double colLO[2][8][64];    // l_ik of the chunk rows                                (parity B & 1)
    __shared__ double dinvs[3][8];
    __shared__ double Yt[64 * 65];        // [row * 65 + k]: L21 of the chunk rows (group O), staged for the panel and its row-major copy
    __shared__ double dsave[64];
    // one self-contained record per item: the panel kernels are the critical path of the factorisation, and the
    // chain  item -> supernode tables -> panel  cost two extra dependent memory round trips per launch
    const FacRec it = P.fac_recs[item_begin + blockIdx.x];
    const int f = it.f, w = it.w, r = it.r;
    double *pan = P.Lx + it.panel_off;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int grp = wv >> 2, v = wv & 3;
    const int lo = w + it.blk * kFacRows;
    const int nr = min(kFacRows, r - lo);
    const int prow = grp ? lo + lane : lane;              // panel row of this lane
    const bool rvalid = grp ? lane < nr : lane < w;
    double a[16];                                         // a[8*h + jj] = column 8*(v + 4h) + jj of this lane's row
#pragma unroll
    for (int c = 0; c < 16; c++) {
        const int j = 8 * (v + 4 * (c >> 3)) + (c & 7);
        a[c] = (rvalid && j < w) ? pan[prow + (int64_t)j * r] : 0.0;
    }
    const unsigned long long spos = __ballot(lane < w && P.sgn_perm[f + (lane < w ? lane : 0)] > 0);
    double *myY = &Yt[lane * 65];                        // (group O only)
    int nreg = 0;
    const int nB = (w + 7) >> 3;
    // Software pipeline with ONE barrier per block: in iteration B the diagonal-row owner eliminates block B while
    // the chunk-row owner eliminates block B-1 with the values published one barrier earlier; after the barrier
    // the diagonal-row waves apply block B and the chunk-row waves apply block B-1 to their live blocks.
    // No global stores inside the loop: __syncthreads() would wait for them every step.
#pragma unroll
    for (int B = 0; B <= 8; B++) {
        if (B <= nB) {                                    // workgroup-uniform
            if (grp == 0 && B < 8 && B < nB && v == (B & 3)) {   // diagonal rows, block B: 8 pivots in-wave
                // Round 5: the lean chain of the front-batch kernels (front_block.hip, front_block2.hip) here as well --
                //   d_k = a_kk - c_{k,k-1}^2 / d_{k-1}  ->  1 / d_k   is one fma, the hardware reciprocal and three more fma;
                //   a_kk and c_{k,k-1} are fetched from the lanes that hold them one pivot EARLIER;
                //   the pivot rule is only TESTED, at the end of the block from the eight pivots (no compare / select / branch on the
                //   chain); a block that needs a substituted pivot is repeated from its saved input with the rule applied;
                //   the pivots / reciprocals are published once per block.
                const int rb = 8 * (B >> 2), pb = B & 1, p3 = B % 3;
                double a_in[8];
#pragma unroll
                for (int q = 0; q < 8; q++) a_in[q] = a[rb + q];
                auto eliminate = [&](auto rule_tag) -> bool {
                    constexpr bool RULE = decltype(rule_tag)::value;
                    double dk[8], dik[8];
                    int nr_ = 0;
                    double akk = readlane_f64(a[rb], 8 * B), csq = 0.0, dinv_prev = 0.0;
#pragma unroll
                    for (int kk = 0; kk < 8; kk++) {
                        const int k = 8 * B + kk;
                        double d = fma(-csq, dinv_prev, akk);
                        double dinv = pivot_rcp3(d);
                        if (RULE) {
                            const double sg = ((spos >> k) & 1ull) ? 1.0 : -1.0;
                            const bool bad = k < w && d * sg < dyn_eps;
                            d = bad ? dyn_delta * sg : d;
                            dinv = bad ? sg / dyn_delta : dinv;
                            nr_ += bad ? 1 : 0;
                        }
                        dinv = k < w ? dinv : 0.0;          // (columns past the panel's width: padding)
                        dk[kk] = d;
                        dik[kk] = dinv;
                        const double reg = a[rb + kk];
                        if (kk < 7) {
                            akk = readlane_f64(a[rb + kk + 1], k + 1);
                            const double cn = readlane_f64(reg, k + 1);
                            csq = cn * cn;
                        }
                        dinv_prev = dinv;
                        const double li = reg * dinv;
                        colL[pb][kk][lane] = li;
                        colC[p3][kk][lane] = k < w ? reg : 0.0;
#pragma unroll
                        for (int jj = kk + 1; jj < 8; jj++) {
                            const double cj = readlane_f64(reg, 8 * B + jj);
                            a[rb + jj] = fma(-li, cj, a[rb + jj]);
                        }
                    }
                    if (!RULE) {
                        bool anybad = false;
#pragma unroll
                        for (int kk = 0; kk < 8; kk++) {
                            const int k = 8 * B + kk;
                            const double sg = ((spos >> k) & 1ull) ? 1.0 : -1.0;
                            anybad = anybad || (k < w && dk[kk] * sg < dyn_eps);
                        }
                        if (__builtin_amdgcn_readfirstlane((int)anybad)) return false;
                    }
                    nreg += nr_;
                    if (lane == 0) {
#pragma unroll
                        for (int kk = 0; kk < 8; kk++) { dsave[8 * B + kk] = dk[kk]; dinvs[p3][kk] = dik[kk]; }
                    }
                    return true;
                };
                if (!eliminate(std::false_type{})) {
#pragma unroll
                    for (int q = 0; q < 8; q++) a[rb + q] = a_in[q];
                    eliminate(std::true_type{});
                }
            }
            if (grp == 1 && B >= 1 && v == ((B - 1) & 3)) {       // chunk rows, block B-1: published operands
                const int Bo = B - 1, rb = 8 * (Bo >> 2), pb = Bo & 1, p3 = Bo % 3;
#pragma unroll
                for (int kk = 0; kk < 8; kk++) {
                    const int k = 8 * Bo + kk;
                    const double li = a[rb + kk] * dinvs[p3][kk];
                    colLO[pb][kk][lane] = li;
                    myY[k] = li;
#pragma unroll
                    for (int jj = kk + 1; jj < 8; jj++) a[rb + jj] = fma(-li, colC[p3][kk][8 * Bo + jj], a[rb + jj]);
                }
            }
            lds_barrier();
            // the factored diagonal block goes to Ldiag from the published columns, by the diagonal-row wavefront that eliminated two
            // blocks ago (not the one that eliminates next); colL[B & 1] stays valid until block B + 2 is published
            if (grp == 0 && it.blk == 0 && B < nB && B < 8 && v == ((B + 2) & 3) && lane < w) {
                double *ld = P.Ldiag + it.diag_off;
#pragma unroll
                for (int kk = 0; kk < 8; kk++) {
                    const int k = 8 * B + kk;
                    if (k < w) ld[lane + k * w] = lane > k ? colL[B & 1][kk][lane] : (lane == k ? 1.0 : 0.0);
                }
            }
            const int Bu = grp == 0 ? B : B - 1;          // block this wave applies now
            if (Bu >= 0 && Bu < nB && Bu < 8) {
                const double(*Lsrc)[64] = grp == 0 ? colL[Bu & 1] : colLO[Bu & 1];
                const int p3 = Bu % 3;
                double lk_[8];
#pragma unroll
                for (int kk = 0; kk < 8; kk++) lk_[kk] = Lsrc[kk][lane];
#pragma unroll
                for (int h = 0; h < 2; h++)
                    if (v + 4 * h > Bu) {
#pragma unroll
                        for (int jj = 0; jj < 8; jj++) {
                            const int j = 8 * (v + 4 * h) + jj;
#pragma unroll
                            for (int kk = 0; kk < 8; kk++) a[8 * h + jj] = fma(-lk_[kk], colC[p3][kk][j], a[8 * h + jj]);
                        }
                    }
            }
        }
    }
    __syncthreads();
    if (it.blk == 0) {
        if (tid < w) {
            const double d = dsave[tid], dinv = 1.0 / d;
            P.D[f + tid] = d;
            P.Dinv[f + tid] = dinv;
            if (!isfinite(dinv)) atomicOr(P.flags + FL_NONFINITE, 1);
        }
        if (grp == 0 && lane == 0 && nreg) atomicAdd(P.flags + FL_NREG, nreg);   // each owner wave counted its own blocks
    }
    if (nr > 0) {
        for (int idx = tid; idx < nr * w; idx += 512) {   // column-major panel rows
            const int row = idx % nr, k = idx / nr;
            pan[(lo + row) + (int64_t)k * r] = Yt[row * 65 + k];
        }
        // row-major copy (w contiguous doubles per row) for the backward solve's L21^T x
        double *lt = P.LT + it.lt_off + (int64_t)(lo - w) * w;
        for (int idx = tid; idx < nr * w; idx += 512) {
            const int k = idx % w, row = idx / w;
            lt[idx] = Yt[row * 65 + k];
        }
    }
}

// ------------------------------------------------------------------------------------------
// after the factorisation: explicit inverses of the unit-lower diagonal blocks (and their
// transposes) so that the solves do small GEMVs instead of w-step substitutions.  One launch.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_invert_diag(DevPlan P, int list_begin, int n) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    if ((int)blockIdx.x >= n) return;
    const int s = P.inv_list[list_begin + blockIdx.x];
    const int w = P.sn_first[s + 1] - P.sn_first[s];
    const int LDL = w | 1;
    double *Ls = smem;              // [w * LDL]
    double *Xs = Ls + w * LDL;      // [w * LDL]
    const double *ld = P.Ldiag + P.sn_diag[s];
    const int tid = threadIdx.x;
    for (int idx = tid; idx < w * w; idx += 64) {
        int i = idx % w, k = idx / w;
        Ls[i + k * LDL] = ld[idx];
        Xs[i + k * LDL] = (i == k) ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid < w) {
        const int j = tid;  // column j of the inverse: solve L x = e_j
        for (int k = j; k < w; k++) {
            const double xk = Xs[k + j * LDL];
            for (int i = k + 1; i < w; i++) Xs[i + j * LDL] -= Ls[i + k * LDL] * xk;
        }
    }
    __syncthreads();
    double *li = P.Linv + P.sn_diag[s];
    double *lit = P.LinvT + P.sn_diag[s];
    for (int idx = tid; idx < w * w; idx += 64) {
        int i = idx % w, j = idx / w;
        li[idx] = Xs[i + j * LDL];     // Linv[i][j], column-major
        lit[idx] = Xs[j + i * LDL];    // LinvT stored so that element (i,j) of Linv sits at [j + i*w]
    }
}

// Wide diagonal blocks (16 < w <= 64, the panels of the fronts): the column-by-column substitution above is a
// 2048-step read-modify-write chain through LDS (~200 us, after the last panel of the factorisation, with nothing
// to overlap it).  Blocked instead, 256 threads: the four 16x16 diagonal blocks are inverted in registers (one
// thread per column), then  X21 = -X22 (L21 X11)  is applied at block size 16 and at block size 32 -- small dense
// products with all operands in LDS.  The block is padded to 64 with the identity.
__global__ void __launch_bounds__(256)
k_invert_diag_wide(DevPlan P, int list_begin) {
    __shared__ double Ls[64 * 65], Xs[64 * 65], Ts[64 * 65];   // [row * 65 + col]
    const int s = P.inv_list[list_begin + blockIdx.x];
    const int w = P.sn_first[s + 1] - P.sn_first[s];
    const double *ld = P.Ldiag + P.sn_diag[s];
    const int tid = threadIdx.x;
    for (int idx = tid; idx < 64 * 64; idx += 256) {
        const int i = idx & 63, k = idx >> 6;
        Ls[i * 65 + k] = (i < w && k < w) ? ld[i + k * w] : (i == k ? 1.0 : 0.0);
        Xs[i * 65 + k] = 0.0;
    }
    __syncthreads();
    if (tid < 64) {   // 16x16 diagonal blocks: thread = column j of block bq, forward substitution in registers
        const int bq = tid >> 4, j = tid & 15, o = 16 * bq;
        double x[16];
#pragma unroll
        for (int c = 0; c < 16; c++) x[c] = c == j ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < 16; k++)
#pragma unroll
            for (int i = k + 1; i < 16; i++) x[i] = fma(-Ls[(o + i) * 65 + o + k], x[k], x[i]);
#pragma unroll
        for (int c = 0; c < 16; c++) Xs[(o + c) * 65 + o + j] = x[c];
    }
    __syncthreads();
    // block size 16: pairs (0,1) and (2,3).  T = L21 X11, then X21 = -X22 T
    for (int e = tid; e < 512; e += 256) {
        const int pr = e >> 8, i = (e >> 4) & 15, j = e & 15, o = 32 * pr;
        double a = 0.0;
#pragma unroll
        for (int m = 0; m < 16; m++) a = fma(Ls[(o + 16 + i) * 65 + o + m], Xs[(o + m) * 65 + o + j], a);
        Ts[(o + 16 + i) * 65 + o + j] = a;
    }
    __syncthreads();
    for (int e = tid; e < 512; e += 256) {
        const int pr = e >> 8, i = (e >> 4) & 15, j = e & 15, o = 32 * pr;
        double a = 0.0;
#pragma unroll
        for (int m = 0; m < 16; m++) a = fma(Xs[(o + 16 + i) * 65 + o + 16 + m], Ts[(o + 16 + m) * 65 + o + j], a);
        Xs[(o + 16 + i) * 65 + o + j] = -a;
    }
    __syncthreads();
    // block size 32: T = L21 X11 (32x32 each, X11 lower triangular), X21 = -X22 T
    for (int e = tid; e < 1024; e += 256) {
        const int i = e >> 5, j = e & 31;
        double a = 0.0;
        for (int m = j; m < 32; m++) a = fma(Ls[(32 + i) * 65 + m], Xs[m * 65 + j], a);
        Ts[(32 + i) * 65 + j] = a;
    }
    __syncthreads();
    for (int e = tid; e < 1024; e += 256) {
        const int i = e >> 5, j = e & 31;
        double a = 0.0;
        for (int m = 0; m <= i; m++) a = fma(Xs[(32 + i) * 65 + 32 + m], Ts[(32 + m) * 65 + j], a);
        Xs[(32 + i) * 65 + j] = -a;
    }
    __syncthreads();
    double *li = P.Linv + P.sn_diag[s];
    double *lit = P.LinvT + P.sn_diag[s];
    double mx = 0.0;
    for (int idx = tid; idx < w * w; idx += 256) {
        const int i = idx % w, j = idx / w;
        li[idx] = Xs[i * 65 + j];      // Linv[i][j], column-major
        lit[idx] = Xs[j * 65 + i];     // LinvT: element (i,j) of Linv at [j + i*w]
        mx = fmax(mx, fabs(Xs[i * 65 + j]));
    }
    // REFINED BLOCK SOLVES.  The solve kernels multiply by this explicit inverse; where it has large entries the product is several
    // times less accurate than the reference's substitution (forward error ~ eps |Linv| |b| against ~ eps |L^-1| |L| |y|) -- on
    // batch seed 324 enough to flip the stop-ratio branch of the iterative refinement and to end the IPM one iteration apart, 1.3e-5
    // off in the objective (round 4).  Established on the CPU with the host interpreter of the plan
    // (tools/seed324_inverse_vs_substitution.py): the first-solve residual is 5.5e-5 with the inverses against substitution's
    // 1.46e-5; one step  y += Linv (b - L y)  on the WIDE blocks (> 16 columns: 16 of that problem's 1361 supernodes) restores
    // 1.46e-5 exactly, on the narrow ones it changes nothing.  So a wide block whose inverse has an entry above DevPlan::polish_tau
    // is marked, and the kernels that solve with regular supernodes take that step on it (k_fwd_level / k_fwd_seg / k_bwd_final /
    // k_bwd_seg).  The fronts' sweeps do not (their panels come in chains whose super-block inverses are a different construction).
    {
        __shared__ double wmx[4];
        mx = wave_max(mx);
        if ((tid & 63) == 0) wmx[tid >> 6] = mx;
        __syncthreads();
        if (tid == 0) {
            const double m = fmax(fmax(wmx[0], wmx[1]), fmax(wmx[2], wmx[3]));
            // every wide block is marked (after a sweep time-out the per-level kernels solve the fronts' panels too, and refine them);
            // COUNTED are the blocks the regular kernels solve (sn_nitems > 0: not a panel of a front) -- the front sweeps never
            // refine, so counting their 64-column panels overstated what is refined (review of round 5)
            const bool big = w > 16 && !(m <= P.polish_tau);
            P.sn_polish[s] = big ? 1 : 0;
            if (big && P.sn_nitems[s] > 0) atomicAdd(P.flags + FL_NPOLISH, 1);
        }
    }
}

// ------------------------------------------------------------------------------------------
// K4b: Schur-complement updates of one stage.  One workgroup owns one 64-row block of one
// target panel (exclusive ownership => deterministic, no atomics) and applies its task list in
// order:   C[rel(i), col(j)] -= sum_k L_s[i,k] * d_k * L_s[j,k]
// The contraction runs on the FP64 matrix core: v_mfma_f64_16x16x4_f64, one 16x16 output tile
// per wave step, operands gathered straight from the source panel (rows are contiguous per k).
// ------------------------------------------------------------------------------------------
constexpr int LDC = kUpdRows + 1;
constexpr int kUpdWaves = 8;   // wavefronts per workgroup in the update kernel

template <int MT>
__device__ __forceinline__ void upd_strip(const double *__restrict__ sp, const double *__restrict__ dv, int r, int K,
                                          int row_lo, int nrows, int tm0, int col_row, int ncols_left, int l15, int lk,
                                          v4f64 (&acc)[4]) {
    // operands gathered straight from the source panel: for a fixed k the 16 rows of a tile are
    // contiguous.  Out-of-range rows are clamped (their outputs are discarded at the scatter);
    // out-of-range k contributes zero through the B operand.
    const double *ap[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) {
        int ai = (tm0 + t) * 16 + l15;
        ai = ai < nrows ? ai : nrows - 1;
        ap[t] = sp + (row_lo + ai);
    }
    int bj = l15 < ncols_left ? l15 : ncols_left - 1;
    const double *bp = sp + (col_row + bj);
#pragma unroll 4
    for (int k0 = 0; k0 < K; k0 += 4) {
        int kk = k0 + lk;
        const double km = kk < K ? 1.0 : 0.0;
        kk = kk < K ? kk : K - 1;
        const int64_t off = (int64_t)kk * r;
        const double b = bp[off] * (dv[kk] * km);
#pragma unroll
        for (int t = 0; t < MT; t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[t][off], b, acc[t], 0, 0, 0);
    }
}

// One workgroup owns one 64-row block of one target panel.  Its task list is cut into wave-tasks
// (one source row range x one 16-column strip); wavefronts take wave-tasks round-robin, run the
// contraction on the FP64 matrix core independently (their load latencies overlap) and then apply
// their results to the LDS-resident target tile strictly in list order (LDS turn counter), so the
// summation order - and therefore every bit of the factor - is fixed.
__global__ void __launch_bounds__(kUpdWaves * 64)
k_update_stage(DevPlan P, int group_begin) {
    __shared__ double Ct[kMaxSnWidth * LDC];
    __shared__ int turn;
    const UpdGroup G = P.upd_groups[group_begin + blockIdx.x];
    const int t = G.tgt;
    const int ft = P.sn_first[t];
    const int wt = P.sn_first[t + 1] - ft;
    const int rt = (int)(P.sn_rowptr[t + 1] - P.sn_rowptr[t]);
    double *tp = P.Lx + P.sn_panel[t];
    const int tid = threadIdx.x;
    const int nrt = min(kUpdRows, rt - G.row_base);
    for (int idx = tid; idx < nrt * wt; idx += kUpdWaves * 64) {
        int row = idx % nrt, col = idx / nrt;
        Ct[col * LDC + row] = tp[(G.row_base + row) + (int64_t)col * rt];
    }
    if (tid == 0) turn = 0;
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lk = lane >> 4;
    int q = G.task_begin;                 // task that contains the current wave-task
    UpdTask T = P.upd_tasks[q];
    for (int v = wave; v < G.nvt; v += kUpdWaves) {
        while (q + 1 < G.task_end) {       // advance to the task holding wave-task v
            const UpdTask Tn = P.upd_tasks[q + 1];
            if (Tn.vt_begin > v) break;
            T = Tn;
            q++;
        }
        const int tn = v - T.vt_begin;     // 16-column strip inside the task
        const int s = T.src;
        const int fs = P.sn_first[s];
        const int K = P.sn_first[s + 1] - fs;
        const int r = (int)(P.sn_rowptr[s + 1] - P.sn_rowptr[s]);
        const double *sp = P.Lx + P.sn_panel[s];
        const double *dv = P.D + fs;
        const int mt = (T.nrows + 15) >> 4;
        const int ncl = T.ncols - tn * 16;
        v4f64 acc[4];
#pragma unroll
        for (int i = 0; i < 4; i++) acc[i] = (v4f64){0.0, 0.0, 0.0, 0.0};
        if (mt == 1) upd_strip<1>(sp, dv, r, K, T.row_lo, T.nrows, 0, T.col_lo + tn * 16, ncl, l15, lk, acc);
        else if (mt == 2) upd_strip<2>(sp, dv, r, K, T.row_lo, T.nrows, 0, T.col_lo + tn * 16, ncl, l15, lk, acc);
        else upd_strip<4>(sp, dv, r, K, T.row_lo, T.nrows, 0, T.col_lo + tn * 16, ncl, l15, lk, acc);
        // target coordinates of this lane's results (C/D layout of the f64 16x16x4 form:
        // col = lane & 15, row = (lane >> 4) + 4 * reg)
        const int *srows = P.sn_rows + P.sn_rowptr[s];
        const int *rel = P.rel + T.rel_off;
        const int jj = tn * 16 + l15;
        const int cp = jj < T.ncols ? srows[T.col_lo + jj] - ft : -1;
        int rp[16];
#pragma unroll
        for (int tmi = 0; tmi < 4; tmi++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int ii = tmi * 16 + lk + 4 * reg;
                rp[tmi * 4 + reg] = (ii < T.nrows && cp >= 0) ? rel[(T.row_lo + ii) - T.col_lo] - G.row_base : -1;
            }
        // ordered application
        while (__atomic_load_n(&turn, __ATOMIC_RELAXED) != v) __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
        for (int tmi = 0; tmi < 4; tmi++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int rr = rp[tmi * 4 + reg];
                if (rr >= 0) Ct[cp * LDC + rr] -= acc[tmi][reg];
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) __atomic_store_n(&turn, v + 1, __ATOMIC_RELAXED);
    }
    __syncthreads();
    for (int idx = tid; idx < nrt * wt; idx += kUpdWaves * 64) {
        int row = idx % nrt, col = idx / nrt;
        tp[(G.row_base + row) + (int64_t)col * rt] = Ct[col * LDC + row];
    }
}

// ------------------------------------------------------------------------------------------
// K4b (dense tiles): one WAVEFRONT owns one 64-row x <=64-column tile of a target panel and keeps it
// in 16 FP64 accumulators (4 x 4 tiles of v_mfma_f64_16x16x4_f64) while it sweeps ALL contributing
// source panels (K = sum of their widths, 256 for the batched updates of a dense front).  The tile is
// loaded once into the accumulators, the product is accumulated with a negated A operand
// (C - sum_k L[j,k] d_k L[i,k]), and stored once.  Operands come straight from the source panels:
// for a fixed k the 16 rows of an MFMA operand are contiguous (128 B), 4 k's per instruction.
// The transposed product is computed (A operand = target COLUMNS, B operand = target ROWS) so that
// the C/D layout (col = lane&15, row = (lane>>4)+4*reg) puts 16 consecutive panel rows in
// consecutive lanes: tile loads / stores are 128-B segments too.
// No LDS, no barriers, no inter-wave communication: 4 independent wavefronts per workgroup.
// ------------------------------------------------------------------------------------------
// Grid-stride over the tiles of a launch (a bounded grid is used by the look-ahead experiments, hipkkt_factor.cpp).
template <int NT, int NR>
__global__ void __launch_bounds__(256, NT == 2 ? 4 : 2)
k_update_dense(DevPlan P, int group_begin, int ngroups) {
    static_assert(NR == 4 || NT == 1, "rows are split only between the workgroups of a one-strip-per-wave launch");
    const int lane = threadIdx.x & 63;
    const int wave = rfl(threadIdx.x >> 6);
    // NT 16-column strips per wavefront: 4/NT wavefronts share a tile, NT tiles per workgroup;
    // NR < 4: 4/NR consecutive workgroups share a tile, each takes NR of its four 16-row blocks
    const int tj0 = (wave % (4 / NT)) * NT;           // first 16-column strip of this wavefront
    if (NR == 4) {
        for (int g = rfl(blockIdx.x * NT + wave / (4 / NT)); g < ngroups; g += gridDim.x * NT)
            dense_tile<NT, NR>(P, P.dgroups + group_begin + g, lane, tj0, 0);
    } else {
        constexpr int RS = 4 / NR;
        for (int u = blockIdx.x; u < ngroups * RS; u += gridDim.x)
            dense_tile<NT, NR>(P, P.dgroups + group_begin + u / RS, lane, tj0, (u % RS) * NR);
    }
}

// A launch of T tiles runs in ceil(T / 1024) rounds of one 64 x 64 tile per SIMD (~60 us each at K = 320): 1128 tiles cost two
// rounds, 2278 three.  Here the r tiles beyond the last FULL round are cut into pieces, one wavefront each, so that the
// partial round costs a fraction of a whole one: four 16-column strips per tile when r <= 256 (one sub-round of ~22 us),
// two 32-column halves when r <= 512 (one sub-round of ~35 us).  Workgroups [0, nfull / 4) take four whole tiles, every
// later workgroup one tile (PIECES = 4) or two tiles (PIECES = 2).  Measured on cfg 2a: 11 launches 1.49 -> 1.33 ms.
template <int PIECES>
__global__ void __launch_bounds__(256, 2)
k_update_dense_tail(DevPlan P, int group_begin, int nfull, int ngroups) {
    const int lane = threadIdx.x & 63;
    const int wave = rfl(threadIdx.x >> 6);
    const int nfw = nfull >> 2;
    if ((int)blockIdx.x < nfw) {
        dense_tile<4, 4>(P, P.dgroups + group_begin + rfl(blockIdx.x * 4 + wave), lane, 0, 0);
    } else if (PIECES == 4) {
        const int g = nfull + ((int)blockIdx.x - nfw);
        if (g < ngroups) dense_tile<1, 4>(P, P.dgroups + group_begin + g, lane, wave, 0);
    } else {
        const int g = nfull + 2 * ((int)blockIdx.x - nfw) + (wave >> 1);
        if (g < ngroups) dense_tile<2, 4>(P, P.dgroups + group_begin + g, lane, (wave & 1) * 2, 0);
    }
}

// ------------------------------------------------------------------------------------------
// K4b (tiny contributions): the leaves of the elimination tree are 1-2 column supernodes whose few
// rows land on scattered single entries of far ancestors (the dense root front).  One thread per
// TARGET ENTRY sums its (source, row i, row j) pairs  sum_k L_s[i,k] d_k L_s[j,k]  in the fixed order
// of the plan's gather list and subtracts once: no atomics, deterministic, fully parallel.
// ------------------------------------------------------------------------------------------
// sum_k L_s[i,k] d_k L_s[j,k] of one pair, added to acc in k order.  The 12 operands of four k's are requested TOGETHER and the
// dependent fma chain runs afterwards (a plain loop waits for the memory round trip of every k).  Same products, same order of
// accumulation as the plain loop.  [Round 6, measured: this does NOT shorten cfg 2a's big gather launch (355 us for 4.0e6 entries,
// 5.5e6 pairs): that launch is bound by the number of scattered memory requests -- adjacent target entries take their operands from
// different small source panels -- not by the dependent chain of its longest thread.]
__device__ __forceinline__ double gath_pair_sum(const DevPlan &P, const GathPair &G, double acc) {
    const double *li = P.Lx + G.src;
    const double *lj = li + G.dj;
    const double *dv = P.D + G.dfirst;
    const int64_t r = G.r;
    const int K = G.K;
    for (int k0 = 0; k0 < K; k0 += 4) {
        double a[4], b[4], d[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int kk = k0 + q < K ? k0 + q : K - 1;      // clamped: loads past the end repeat the last column and are not used
            a[q] = li[kk * r];
            b[q] = lj[kk * r];
            d[q] = dv[kk];
        }
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (k0 + q < K) acc = fma(a[q] * d[q], b[q], acc);
    }
    return acc;
}
__global__ void __launch_bounds__(256)
k_update_gather(DevPlan P, int64_t ebegin, int64_t n) {
    // grid-stride: a launch on the side stream (hipkkt_factor.cpp enqueue_gather) is given a bounded grid so that it leaves wavefront
    // slots and registers on every compute unit to the small kernels of the main stream it runs next to
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p0 = P.gath_pptr[ebegin + e], p1 = P.gath_pptr[ebegin + e + 1];
        if (p1 - p0 > kGathHeavy || p1 <= p0) continue;        // k_update_gather_heavy
        double *tp = P.Lx + P.gath_tgt[ebegin + e];
        const double t0 = *tp;                                 // (requested next to the first record)
        double acc = 0.0;
        GathPair G = P.gath_pairs[p0];
        for (int64_t p = p0; p < p1; p++) {
            const GathPair Gn = P.gath_pairs[p + 1 < p1 ? p + 1 : p];   // the next record is on its way while this pair is summed
            acc = gath_pair_sum(P, G, acc);
            G = Gn;
        }
        *tp = t0 - acc;
    }
}
// target entries with long pair lists (a dense row / column of the root that every leaf touches: 1189 pairs on cfg 3) kept
// ONE thread busy for a millisecond while the rest of the launch had finished: one wavefront each, lane l takes the
// pairs l, l + 64, ... in order and the 64 partial sums are added in a fixed tree -- deterministic, like the thread version
__global__ void __launch_bounds__(256)
k_update_gather_heavy(DevPlan P, int64_t hbegin, int64_t n) {
    const int64_t h = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (h >= n) return;
    const int lane = threadIdx.x & 63;
    const int64_t e = P.gath_heavy[hbegin + h];
    const int64_t p0 = P.gath_pptr[e], p1 = P.gath_pptr[e + 1];
    double acc = 0.0;
    for (int64_t p = p0 + lane; p < p1; p += 64) {
        const GathPair G = P.gath_pairs[p];
        acc = gath_pair_sum(P, G, acc);
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) P.Lx[P.gath_tgt[e]] -= acc;
}

// ------------------------------------------------------------------------------------------
// host-callable launchers (used by the hipkkt_*.cpp host files; all launches go to the handle's stream)
// ------------------------------------------------------------------------------------------
void launch_maxabs_gather(hipStream_t st, const double *v, const int64_t *idx, int64_t n, unsigned long long *slot) {
    if (n > 0) hipLaunchKernelGGL(k_maxabs_gather, dim3(nblk(n)), dim3(256), 0, st, v, idx, n, slot);
}
void launch_init_panels(hipStream_t st, const DevPlan &P, int64_t nnz, int static_enable, double eps_const, double eps_prop) {
    if (nnz > 0)
        hipLaunchKernelGGL(k_init_panels, dim3(nblk(nnz)), dim3(256), 0, st, P.Lx, P.kval, P.kmap, P.kdiag_sign, nnz,
                           P.scal, static_enable, eps_const, eps_prop);
}
static size_t factor_lds_bytes(int wmax) { return sizeof(double) * (size_t)(wmax * (wmax + 1) + wmax + wmax * LDT); }
void launch_factor_level(hipStream_t st, const DevPlan &P, int item_begin, int nitems, int wmax, double dyn_eps, double dyn_delta) {
    if (nitems > 0)
        hipLaunchKernelGGL(k_factor_level, dim3(nitems), dim3(256), factor_lds_bytes(wmax), st, P, item_begin, wmax, dyn_eps,
                           dyn_delta);
}
void launch_factor_panel(hipStream_t st, const DevPlan &P, int item_begin, int nitems, double dyn_eps, double dyn_delta) {
    if (nitems > 0) hipLaunchKernelGGL(k_factor_panel, dim3(nitems), dim3(512), 0, st, P, item_begin, dyn_eps, dyn_delta);
}
void launch_update_stage(hipStream_t st, const DevPlan &P, int group_begin, int ngroups) {
    if (ngroups > 0) hipLaunchKernelGGL(k_update_stage, dim3(ngroups), dim3(kUpdWaves * 64), 0, st, P, group_begin);
}
// Few tiles (<= 384: the just-in-time updates on the critical path): 16-column strips x 32 rows per wavefront, two workgroups per tile
// (measured on cfg 2a, factorisation: 5.81 / 5.65 / 5.65 ms with 64 / 32 / 16 rows per wavefront).  Plenty of tiles: one wavefront per
// tile; full_k launches (whole panels of sources, >= 1.5 MFLOP per tile) cut the tiles of a partial last round into strips / halves.
void launch_update_dense(hipStream_t st, const DevPlan &P, int group_begin, int ngroups, bool full_k) {
    if (ngroups <= 0) return;
    if (ngroups > kDenseStripTiles) {
        const int round = 1024, r = ngroups % round, nfull = ngroups - r;   // nfull: multiple of 1024, hence of 4
        if (full_k && r > 0 && (r <= 256 || (nfull == 0 && r <= 768)))      // (a lone partial round: three strip sub-rounds still beat it)
            hipLaunchKernelGGL(k_update_dense_tail<4>, dim3(nfull / 4 + r), dim3(256), 0, st, P, group_begin, nfull, ngroups);
        else if (full_k && r > 0 && r <= 512)
            hipLaunchKernelGGL(k_update_dense_tail<2>, dim3(nfull / 4 + (r + 1) / 2), dim3(256), 0, st, P, group_begin, nfull, ngroups);
        else
            hipLaunchKernelGGL((k_update_dense<4, 4>), dim3((ngroups + 3) / 4), dim3(256), 0, st, P, group_begin, ngroups);
    } else {
        hipLaunchKernelGGL((k_update_dense<1, 2>), dim3(ngroups * 2), dim3(256), 0, st, P, group_begin, ngroups);
    }
}
// Split-K (hipkkt_setup.cpp plan_split_k): a stage with FEW target tiles and MANY contributions per tile (cfg 5: the 1000 x 1000 block
// of the variables = 136 tiles, each fed by 20 cones x 5 panels per update batch, K = 6400) kept 136 of the 1024 SIMDs busy for 0.7 ms
// per batch.  The contributions of such a tile are cut into up to 16 chunks, each accumulated by a wavefront of its own into a partial
// tile that starts from zero (the unchanged tile code of dense_tile.h on a scratch tile); this kernel adds the partial tiles to the
// target in a FIXED order (deterministic) and clears them for the next stage.
__global__ void __launch_bounds__(256)
k_split_reduce(DevPlan P, const SplitRec *recs) {
    const SplitRec R = recs[blockIdx.x];
    double *tp = P.Lx + R.tile_off, *sc = P.Lx + R.scratch_off;
    for (int idx = threadIdx.x; idx < 4096; idx += 256) {
        const int row = idx & 63, col = idx >> 6;
        double s = 0.0;
        for (int q = 0; q < R.nparts; q++) {
            s += sc[(int64_t)q * 4096 + idx];
            sc[(int64_t)q * 4096 + idx] = 0.0;
        }
        if (row < R.nrt && col < R.wt) tp[row + (int64_t)col * R.rt] += s;
    }
}
void launch_split_reduce(hipStream_t st, const DevPlan &P, const SplitRec *recs, int n) {
    if (n > 0) hipLaunchKernelGGL(k_split_reduce, dim3(n), dim3(256), 0, st, P, recs);
}
void launch_update_gather(hipStream_t st, const DevPlan &P, int64_t ebegin, int64_t n, int64_t hbegin, int64_t nheavy, int max_blocks) {
    if (n > 0) hipLaunchKernelGGL(k_update_gather, dim3(max_blocks > 0 ? std::min<unsigned>(nblk(n), (unsigned)max_blocks) : nblk(n)), dim3(256), 0, st, P, ebegin, n);
    if (nheavy > 0) hipLaunchKernelGGL(k_update_gather_heavy, dim3(nblk(nheavy, 4)), dim3(256), 0, st, P, hbegin, nheavy);
}
// inv_list = [n_small supernodes of width <= wmax_small | n_wide supernodes of width in (16, 64]]
void launch_invert_diag(hipStream_t st, const DevPlan &P, int n_small, int wmax_small, int n_wide) {
    const int ldl = wmax_small | 1;
    if (n_small > 0)
        hipLaunchKernelGGL(k_invert_diag, dim3(n_small), dim3(64), sizeof(double) * 2 * (size_t)wmax_small * ldl, st, P, 0, n_small);
    if (n_wide > 0) hipLaunchKernelGGL(k_invert_diag_wide, dim3(n_wide), dim3(256), 0, st, P, n_small);
}

}  // namespace hipkkt
