// Products with the resident K outside the factorisation (K6-K8, N2, N4), all from the symmetric CSR view of the unregularised K:
//   refinement        k_spmv_residual / k_spmv_long / k_spmv_dense_tri, k_norm_inf, k_refine_decide / _add / _copy_out (decided on the device)
//   residuals (N4)    k_residuals + k_residuals_finish;  k_block_products
//   reduced system    k_reduced_rows + k_reduced_finish + k_reduced_axpy, k_const_rhs  (N2)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_plan.h"
#include "kernel_util.h"
#include "kernels.h"

namespace hipkkt {

// ------------------------------------------------------------------------------------------
// K6-K8: iterative refinement pieces (ref: kktsolver_directldl.jl:389-466)
// e = b - K*xi with the symmetric CSR view of the unregularised K; 8 lanes per row
// ------------------------------------------------------------------------------------------
// Rows longer than kLongRow entries (a budget row 1'x = 1, the expansion columns of big cones, dense PSD blocks) would keep
// their 4 lanes busy for thousands of sequential iterations (cfg 3: 0.3 ms per SpMV for 70 000 nonzeros): they are left
// out here and taken by k_spmv_long, one workgroup each.
constexpr int kLongRow = 192;
__device__ __forceinline__ void spmv_short_rows(const int64_t *__restrict__ rowptr, const int *__restrict__ col,
                                                const int64_t *__restrict__ qidx, const double *__restrict__ kval,
                                                const double *__restrict__ b, const double *__restrict__ xi, double *__restrict__ e,
                                                int n, unsigned long long *__restrict__ norm_slot, const double *__restrict__ dacc) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = gid >> 2, sub = gid & 3;
    double acc = 0.0;
    bool mine = false;
    if (row < n) {
        const int64_t p0 = rowptr[row], p1 = rowptr[row + 1];
        mine = p1 - p0 <= kLongRow;
        if (mine)
            for (int64_t p = p0 + sub; p < p1; p += 4) acc += kval[qidx[p]] * xi[col[p]];
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    double a = 0.0;
    if (mine && sub == 0) {
        if (dacc) acc += dacc[row];         // the row's part inside a dense triangle (k_spmv_dense_tri; 0 for every other row)
        const double ev = b[row] - acc;
        e[row] = ev;
        a = fabs(ev);
    }
    block_atomic_max_abs(norm_slot, a);
}
// one workgroup per long row: fixed partition of the entries over the 256 threads, fixed reduction tree (deterministic)
__device__ __forceinline__ void spmv_long_row(int row, const int64_t *__restrict__ rowptr, const int *__restrict__ col,
                                              const int64_t *__restrict__ qidx, const double *__restrict__ kval,
                                              const double *__restrict__ b, const double *__restrict__ xi, double *__restrict__ e,
                                              unsigned long long *__restrict__ norm_slot, const double *__restrict__ dacc) {
    __shared__ double red[4];
    const int64_t p0 = rowptr[row], p1 = rowptr[row + 1];
    double acc = 0.0;
    for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) acc += kval[qidx[p]] * xi[col[p]];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double ev = b[row] - ((((red[0] + red[1]) + red[2]) + red[3]) + (dacc ? dacc[row] : 0.0));
        e[row] = ev;
        atomic_max_abs(norm_slot, ev);
    }
}
// The three SpMV kernels multiply by x0 when st == nullptr (the first residual of a solve) and otherwise by the CANDIDATE of a
// refinement step, xbuf[1 - cur] (x0 if st->cur else x1); an inactive state makes them return at once: the norm slot keeps its
// previous value, which k_refine_decide ignores when inactive.
__device__ __forceinline__ const double *spmv_operand(const RefineState *st, const double *x0, const double *x1) {
    return st ? (st->cur ? x0 : x1) : x0;
}
__global__ void __launch_bounds__(256)
k_spmv_residual(const int64_t *__restrict__ rowptr, const int *__restrict__ col, const int64_t *__restrict__ qidx,
                const double *__restrict__ kval, const double *__restrict__ b, const RefineState *st,
                const double *__restrict__ x0, const double *__restrict__ x1, double *__restrict__ e, int n,
                unsigned long long *__restrict__ norm_slot, const double *__restrict__ dacc) {
    if (st && !st->active) return;
    spmv_short_rows(rowptr, col, qidx, kval, b, spmv_operand(st, x0, x1), e, n, norm_slot, dacc);
}
__global__ void __launch_bounds__(256)
k_spmv_long(const int *__restrict__ long_rows, const int64_t *__restrict__ rowptr, const int *__restrict__ col,
            const int64_t *__restrict__ qidx, const double *__restrict__ kval, const double *__restrict__ b,
            const RefineState *st, const double *__restrict__ x0, const double *__restrict__ x1, double *__restrict__ e,
            unsigned long long *__restrict__ norm_slot, const double *__restrict__ dacc) {
    if (st && !st->active) return;
    spmv_long_row(long_rows[blockIdx.x], rowptr, col, qidx, kval, b, spmv_operand(st, x0, x1), e, norm_slot, dacc);
}

// The dense triangles of K that left the symmetric view (symbolic.h HostPlan::dtri: the packed upper triangles of PSD-cone Hs blocks,
// column c0 + j = rows c0 .. c0 + j, contiguous in kval from col_off[j]): acc_out[c0 + i] = sum_j H(i, j) x[c0 + j] of the symmetric H.
// One workgroup (8 wavefronts) per 64 rows i0 .. i0 + 63 of a triangle; every stored entry is read twice, both times coalesced:
//   row part     sum_{j >= i} H(i, j) x_j: lane = row, the wavefronts take the columns j = i0 + w, i0 + w + 8, ...  (entry (i, j) sits at
//                col_off[j] + i: 64 consecutive doubles per column and wavefront)
//   column part  sum_{r < i} H(r, i) x_r: column i's rows 0 .. i - 1 are contiguous; every wavefront takes 8 of the strip's columns,
//                lanes stride over the rows, fixed reduction tree
// against 2 x (8 + 4 + 8) bytes per entry through the view (one of the two gathers strided: one value per cache line).  Fixed
// partition and summation order: deterministic.  cfg 5 (20 triangles of 1275): 345 -> 86 us per SpMV (2 x 130 MB at 3.4 TB/s, fabric side).
__global__ void __launch_bounds__(512)
k_spmv_dense_tri(const DenseTriStrip *__restrict__ strips, const int64_t *__restrict__ col_off, const double *__restrict__ kval,
                 const RefineState *st, const double *__restrict__ x0, const double *__restrict__ x1, double *__restrict__ acc_out) {
    if (st && !st->active) return;
    const double *__restrict__ x = spmv_operand(st, x0, x1);
    __shared__ double part[8][64];
    __shared__ double csum[64];
    const DenseTriStrip T = strips[blockIdx.x];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = T.i0 + lane;
    const int64_t *__restrict__ co = col_off + T.col0;
    const double *__restrict__ xb = x + T.c0;
    double a = 0.0;
#pragma unroll 4
    for (int j = T.i0 + w; j < T.d; j += 8) {
        const double v = kval[co[j] + (i <= j ? i : j)];      // (lanes right of the diagonal re-read the diagonal entry: never out of the column)
        a = fma(i <= j ? v : 0.0, xb[j], a);
    }
    part[w][lane] = a;
    for (int c = 0; c < 8; c++) {
        const int ci = T.i0 + 8 * w + c;                      // wave-uniform
        double s = 0.0;
        if (ci < T.d) {
            const double *__restrict__ colv = kval + co[ci];
#pragma unroll 4
            for (int r = lane; r < ci; r += 64) s = fma(colv[r], xb[r], s);
        }
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) csum[8 * w + c] = s;
    }
    __syncthreads();
    if (w == 0 && i < T.d) {
        double t = csum[lane];
#pragma unroll
        for (int q = 0; q < 8; q++) t += part[q][lane];
        acc_out[T.c0 + i] = t;
    }
}

// the three sparse products of residuals_update! (residuals.jl:12-25) from the RESIDENT KKT
// values -- K = [P A'; A -Hs] in the original ordering, symmetric CSR view, 4 lanes per row:
//   rows i < n:        Px_i  = sum_{c < n} K_ic x_c ,   ATz_i = sum_{n <= c < n+m} K_ic z_{c-n}
//   rows n <= i < n+m: Ax_{i-n} = sum_{c < n} K_ic x_c          (the -Hs block and the expansion columns are skipped)
// Deterministic dot products over the rows of a launch, in two steps.  block_dots: the ND per-thread terms d[0 .. ND) of a
// 256-thread workgroup are summed in a fixed order (the wavefront's tree, then wavefronts 0 .. 3) into part[blockIdx][NQ]; the
// columns from ND on pass through (zero).  column_sums, in a single workgroup: thread (which = tid % NQ, slot = tid / NQ) adds the
// blocks slot, slot + 256 / NQ, ... of column `which`, thread c < NQ adds the 256 / NQ slots of column c in order; tot[] is valid
// in thread 0.
template <int ND, int NQ>
__device__ __forceinline__ void block_dots(double (&d)[NQ], double *__restrict__ part) {
    __shared__ double red[4][NQ];
#pragma unroll
    for (int c = 0; c < ND; c++)
        for (int off = 32; off > 0; off >>= 1) d[c] += __shfl_down(d[c], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < NQ; c++) red[wave][c] = d[c];
    __syncthreads();
    if (threadIdx.x < NQ)
        part[(int64_t)blockIdx.x * NQ + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}
template <int NQ>
__device__ __forceinline__ void column_sums(const double *__restrict__ part, int nblocks, double (&tot)[NQ]) {
    constexpr int NS = 256 / NQ;
    __shared__ double buf[NQ][NS];
    const int which = threadIdx.x % NQ, slot = threadIdx.x / NQ;
    double a = 0.0;
    for (int bq = slot; bq < nblocks; bq += NS) a += part[(int64_t)bq * NQ + which];
    buf[which][slot] = a;
    __syncthreads();
    if (threadIdx.x < NQ) {
        double t = 0.0;
        for (int i = 0; i < NS; i++) t += buf[threadIdx.x][i];
        buf[threadIdx.x][0] = t;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NQ; c++) tot[c] = threadIdx.x == 0 ? buf[c][0] : 0.0;
}

// the products of one row, by its 4 lanes (sub = lane & 3; every lane ends up with the sums):
//   ax = sum_{c < n} K_rc x_c ,   az = sum_{n <= c < n+m} K_rc z_{c-n}  (rows < n only)
struct RowProducts { double ax, az; };
__device__ __forceinline__ RowProducts row_products(const int64_t *__restrict__ rowptr, const int *__restrict__ col,
                                                    const int64_t *__restrict__ qidx, const double *__restrict__ kval,
                                                    const double *__restrict__ x, const double *__restrict__ z, int row, int sub,
                                                    int n, int m) {
    double ax = 0.0, az = 0.0;
    if (row < n + m) {
        const int64_t p0 = rowptr[row], p1 = rowptr[row + 1];
        for (int64_t p = p0 + sub; p < p1; p += 4) {
            const int c = col[p];
            const double v = kval[qidx[p]];
            if (c < n) ax += v * x[c];
            else if (row < n && c < n + m) az += v * z[c - n];
        }
    }
    ax += __shfl_xor(ax, 1, 64);
    ax += __shfl_xor(ax, 2, 64);
    az += __shfl_xor(az, 1, 64);
    az += __shfl_xor(az, 2, 64);
    return {ax, az};
}
__global__ void __launch_bounds__(256)
k_block_products(const int64_t *__restrict__ rowptr, const int *__restrict__ col, const int64_t *__restrict__ qidx,
                 const double *__restrict__ kval, const double *__restrict__ x, const double *__restrict__ z,
                 double *__restrict__ Px, double *__restrict__ ATz, double *__restrict__ Ax, int n, int m) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = gid >> 2, sub = gid & 3;
    const auto [ax, az] = row_products(rowptr, col, qidx, kval, x, z, row, sub, n, m);
    if (sub == 0 && row < n + m) {
        if (row < n) { Px[row] = ax; ATz[row] = az; }
        else Ax[row - n] = ax;
    }
}

// residuals_update! (residuals.jl:1-37) from the RESIDENT P and A values -- rows of the symmetric
// CSR view of K, 4 lanes per row (see k_block_products):
//   rows i < n :  Px_i = (P x)_i, rx_inf_i = -(A' z)_i, rx_i = rx_inf_i - Px_i - q_i tau,  partial sums of q.x and x.Px
//   rows n+j   :  rz_inf_j = s_j + (A x)_j,             rz_j = rz_inf_j - b_j tau,         partial sums of b.z and s.z
// The four dot products are reduced per workgroup into part[blockIdx][4] and summed in block order by k_residuals_finish
// (deterministic).  out = [rx | rz | rx_inf | rz_inf | Px]  (n + m + n + m + n doubles).
__global__ void __launch_bounds__(256)
k_residuals(const int64_t *__restrict__ rowptr, const int *__restrict__ col, const int64_t *__restrict__ qidx,
            const double *__restrict__ kval, const double *__restrict__ x, const double *__restrict__ z,
            const double *__restrict__ sv, const double *__restrict__ q, const double *__restrict__ b, double tau,
            double *__restrict__ out, double *__restrict__ part, int n, int m) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = gid >> 2, sub = gid & 3;
    const auto [ax, az] = row_products(rowptr, col, qidx, kval, x, z, row, sub, n, m);
    double d[4] = {0.0, 0.0, 0.0, 0.0};                  // q.x, b.z, s.z, x.Px contributions of this row
    if (sub == 0 && row < n + m) {
        double *rx = out, *rz = out + n, *rxi = rz + m, *rzi = rxi + n, *Px = rzi + m;
        if (row < n) {
            const double xi = x[row], rinf = -az;
            Px[row] = ax;
            rxi[row] = rinf;
            rx[row] = (rinf - ax) - q[row] * tau;
            d[0] = q[row] * xi;
            d[3] = xi * ax;
        } else {
            const int j = row - n;
            const double rinf = sv[j] + ax;
            rzi[j] = rinf;
            rz[j] = rinf - b[j] * tau;
            d[1] = b[j] * z[j];
            d[2] = sv[j] * z[j];
        }
    }
    block_dots<4, 4>(d, part);
}
// scal = [q.x, b.z, s.z, x.Px, r_tau = q.x + b.z + kappa + x.Px / tau]   (residuals.jl:27-34)
__global__ void __launch_bounds__(256)
k_residuals_finish(const double *__restrict__ part, int nblocks, double tau, double kappa, double *__restrict__ scal) {
    double t[4];
    column_sums<4>(part, nblocks, t);
    if (threadIdx.x == 0) {
        const double qx = t[0], bz = t[1], sz = t[2], xPx = t[3];
        scal[0] = qx; scal[1] = bz; scal[2] = sz; scal[3] = xPx;
        scal[4] = qx + bz + kappa + xPx / tau;
    }
}

// ------------------------------------------------------------------------------------------
// SURVEY section 8(f) row N2, second half: the reduced-system algebra of kkt_solve! (kktsystem.jl:170-196) on the device.
// Given the two resident solutions  [x1; z1] (this step's right-hand side)  and  [x2; z2] (the constant right-hand side [-q; b]),
// xi = x / tau and the resident q, b, P:
//   tau_num = rhs.tau - rhs.kappa / tau + q.x1 + b.z1 + 2 xi'P x1
//   tau_den = kappa / tau - q.x2 - b.z2 + (xi - x2)'P(xi - x2) - x2'P x2          (quad_form of mathutils.jl:299-337 = x'(P y), P symmetric)
//   dtau = tau_num / tau_den ;  lhs = [x1; z1] + dtau [x2; z2]
// Rows of the symmetric CSR view of K (4 lanes per row, like k_residuals); the seven dot products are reduced per workgroup into
// part[blockIdx][8] and summed in block order by k_reduced_finish (deterministic).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_reduced_rows(const int64_t *__restrict__ rowptr, const int *__restrict__ col, const int64_t *__restrict__ qidx,
               const double *__restrict__ kval, const double *__restrict__ s1, const double *__restrict__ s2,
               const double *__restrict__ xv, const double *__restrict__ q, const double *__restrict__ b, double tau,
               double *__restrict__ part, int n, int m) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = gid >> 2, sub = gid & 3;
    double a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (row < n) {
        const int64_t p0 = rowptr[row], p1 = rowptr[row + 1];
        for (int64_t p = p0 + sub; p < p1; p += 4) {
            const int c = col[p];
            if (c < n) {
                const double v = kval[qidx[p]];
                a1 += v * s1[c];
                a2 += v * s2[c];
                a3 += v * (xv[c] / tau);
            }
        }
    }
    a1 += __shfl_xor(a1, 1, 64); a1 += __shfl_xor(a1, 2, 64);
    a2 += __shfl_xor(a2, 1, 64); a2 += __shfl_xor(a2, 2, 64);
    a3 += __shfl_xor(a3, 1, 64); a3 += __shfl_xor(a3, 2, 64);
    double d[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // q.x1, b.z1, xi'P x1, q.x2, b.z2, (xi-x2)'P(xi-x2), x2'P x2
    if (sub == 0 && row < n + m) {
        if (row < n) {
            const double xi = xv[row] / tau, x1 = s1[row], x2 = s2[row];
            d[0] = q[row] * x1;
            d[2] = xi * a1;
            d[3] = q[row] * x2;
            d[5] = (xi - x2) * (a3 - a2);
            d[6] = x2 * a2;
        } else {
            const int j = row - n;
            d[1] = b[j] * s1[row];
            d[4] = b[j] * s2[row];
        }
    }
    block_dots<7, 8>(d, part);
}
// scal_in = [tau, kappa, rhs.tau, rhs.kappa];  scal_out = [dtau, tau_num, tau_den, q.x1, b.z1, xi'Px1, q.x2, b.z2, (xi-x2)'P(xi-x2), x2'Px2]
__global__ void __launch_bounds__(256)
k_reduced_finish(const double *__restrict__ part, int nblocks, double tau, double kappa, double rhs_tau, double rhs_kappa,
                 double *__restrict__ scal_out) {
    double t[8];
    column_sums<8>(part, nblocks, t);
    if (threadIdx.x == 0) {
        const double qx1 = t[0], bz1 = t[1], xPx1 = t[2], qx2 = t[3], bz2 = t[4], dPd = t[5], x2Px2 = t[6];
        const double num = rhs_tau - rhs_kappa / tau + qx1 + bz1 + 2.0 * xPx1;         // kktsystem.jl:183
        double den = kappa / tau - qx2 - bz2;                                           // :189
        den += dPd - x2Px2;                                                             // :190
        scal_out[0] = num / den; scal_out[1] = num; scal_out[2] = den;
        scal_out[3] = qx1; scal_out[4] = bz1; scal_out[5] = xPx1; scal_out[6] = qx2; scal_out[7] = bz2; scal_out[8] = dPd; scal_out[9] = x2Px2;
    }
}
// lhs = [x1; z1] + dtau [x2; z2]   (kktsystem.jl:195-196), dtau read from the device
__global__ void k_reduced_axpy(const double *__restrict__ s1, const double *__restrict__ s2, const double *__restrict__ scal,
                               double *__restrict__ lhs, int nm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nm) lhs[i] = s1[i] + scal[0] * s2[i];
}
// the constant right-hand side of _kkt_solve_constant_rhs! (kktsystem.jl:80-92): [-q; b; 0]
__global__ void k_const_rhs(double *__restrict__ dst, const double *__restrict__ qb, int n, int nm, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) dst[i] = i < n ? -qb[i] : (i < nm ? qb[i] : 0.0);
}

__global__ void __launch_bounds__(256)
k_norm_inf(const double *__restrict__ v, int n, unsigned long long *__restrict__ slot) {
    double a = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double t = fabs(v[i]);
        a = (t > a || t != t) ? t : a;
    }
    block_atomic_max_abs(slot, a);
}

// ---- refinement decided on the device (one host synchronisation per refined solve instead of one per step).
// k_refine_decide<phase 0> runs after the first solve and its residual, <phase 1> after every refinement step; both are
// single-thread kernels that replay the branches of kktsolver_directldl.jl:418-446 on the RefineState.
__global__ void k_refine_decide(RefineState *st, const unsigned long long *scal, int phase, double reltol, double abstol,
                                int max_iter, double stop_ratio) {
    if (blockIdx.x || threadIdx.x) return;
    const double norme = __longlong_as_double((long long)scal[SC_NORME]);
    if (phase == 0) {
        const double normb = __longlong_as_double((long long)scal[SC_NORMB]);
        st->cur = 0;
        st->steps = 0;
        st->normb = normb;
        st->norme = norme;
        st->lastnorme = norme;
        st->fail = isfinite(norme) ? 0 : 1;                                        // :414-416
        st->active = (!st->fail && max_iter > 0 && !(norme <= abstol + reltol * normb)) ? 1 : 0;   // :421-426
        return;
    }
    if (!st->active) return;
    st->steps += 1;
    st->norme = norme;
    if (!isfinite(norme)) { st->fail = 1; st->active = 0; return; }               // :433-435
    const double improved = st->lastnorme / norme;                                // :437
    if (improved < stop_ratio) {                                                  // :438-444: insufficient improvement
        if (improved > 1.0) st->cur ^= 1;                                         //           (keep the better of the two)
        st->active = 0;
        return;
    }
    st->cur ^= 1;                                                                 // :445 swap x, dx
    st->lastnorme = norme;
    st->active = (st->steps < max_iter && !(norme <= abstol + reltol * st->normb)) ? 1 : 0;
}
// candidate = iterate + correction  (:430-431: dx = K \ e, dx += x); inactive states leave the candidate alone
__global__ void k_refine_add(const RefineState *st, double *__restrict__ x0, double *__restrict__ x1,
                             const double *__restrict__ corr, int n) {
    if (!st->active) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const double *src = st->cur ? x1 : x0;
    double *dst = st->cur ? x0 : x1;
    if (i < n) dst[i] = src[i] + corr[i];
}
// out = the accepted iterate (first nm entries)
__global__ void k_refine_copy_out(const RefineState *st, const double *__restrict__ x0, const double *__restrict__ x1,
                                  double *__restrict__ out, int nm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const double *src = st->cur ? x1 : x0;
    if (i < nm) out[i] = src[i];
}

__global__ void k_set_rhs(double *__restrict__ b, const double *__restrict__ rhs, int nm, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) b[i] = i < nm ? rhs[i] : 0.0;
}

__global__ void k_check_finite(const double *__restrict__ v, int n, int *__restrict__ flags) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !isfinite(v[i])) atomicOr(flags + FL_NONFINITE, 1);
}

// ------------------------------------------------------------------------------------------
// host-callable launchers (used by the hipkkt_*.cpp host files; all launches go to the handle's stream)
// ------------------------------------------------------------------------------------------
// e = b - K x, ||e||_inf into *slot;  x = x0 when rs == nullptr, otherwise the candidate of the refinement state (spmv_operand)
void launch_spmv_residual(hipStream_t st, const DevPlan &P, const double *b, const RefineState *rs, const double *x0, const double *x1,
                          double *e, int n, unsigned long long *slot) {
    const double *dacc = P.n_dtri_strips > 0 ? P.dense_acc : nullptr;
    if (dacc)
        hipLaunchKernelGGL(k_spmv_dense_tri, dim3(P.n_dtri_strips), dim3(512), 0, st, P.dtri_strips, P.dtri_col, P.kval, rs, x0, x1, P.dense_acc);
    if (n > 0)
        hipLaunchKernelGGL(k_spmv_residual, dim3(nblk((int64_t)n * 4)), dim3(256), 0, st, P.sym_rowptr, P.sym_col, P.sym_q,
                           P.kval, b, rs, x0, x1, e, n, slot, dacc);
    if (P.n_long_rows > 0)
        hipLaunchKernelGGL(k_spmv_long, dim3(P.n_long_rows), dim3(256), 0, st, P.long_rows, P.sym_rowptr, P.sym_col, P.sym_q, P.kval,
                           b, rs, x0, x1, e, slot, dacc);
}
void launch_block_products(hipStream_t st, const DevPlan &P, const double *x, const double *z, double *Px, double *ATz,
                           double *Ax, int n, int m) {
    if (n + m > 0)
        hipLaunchKernelGGL(k_block_products, dim3(nblk((int64_t)(n + m) * 4)), dim3(256), 0, st, P.sym_rowptr, P.sym_col, P.sym_q,
                           P.kval, x, z, Px, ATz, Ax, n, m);
}
void launch_refine_decide(hipStream_t st, RefineState *rs, const double *scal, int phase, double reltol, double abstol, int max_iter,
                          double stop_ratio) {
    hipLaunchKernelGGL(k_refine_decide, dim3(1), dim3(64), 0, st, rs, (const unsigned long long *)scal, phase, reltol, abstol, max_iter,
                       stop_ratio);
}
void launch_refine_add(hipStream_t st, const RefineState *rs, double *x0, double *x1, const double *corr, int n) {
    if (n > 0) hipLaunchKernelGGL(k_refine_add, dim3(nblk(n)), dim3(256), 0, st, rs, x0, x1, corr, n);
}
void launch_refine_copy_out(hipStream_t st, const RefineState *rs, const double *x0, const double *x1, double *out, int nm) {
    if (nm > 0) hipLaunchKernelGGL(k_refine_copy_out, dim3(nblk(nm)), dim3(256), 0, st, rs, x0, x1, out, nm);
}
int long_row_threshold() { return kLongRow; }
int residual_blocks(int n, int m) { return (int)nblk((int64_t)(n + m) * 4); }
void launch_residuals(hipStream_t st, const DevPlan &P, const double *x, const double *z, const double *s, const double *q,
                      const double *b, double tau, double kappa, double *out, double *part, double *scal, int n, int m) {
    if (n + m <= 0) return;
    const int nb = residual_blocks(n, m);
    hipLaunchKernelGGL(k_residuals, dim3(nb), dim3(256), 0, st, P.sym_rowptr, P.sym_col, P.sym_q, P.kval, x, z, s, q, b, tau, out, part, n, m);
    hipLaunchKernelGGL(k_residuals_finish, dim3(1), dim3(256), 0, st, part, nb, tau, kappa, scal);
}
void launch_reduced(hipStream_t st, const DevPlan &P, const double *s1, const double *s2, const double *xv, const double *q,
                    const double *b, double tau, double kappa, double rhs_tau, double rhs_kappa, double *part, double *scal_out,
                    double *lhs, int n, int m) {
    if (n + m <= 0) return;
    const int nb = residual_blocks(n, m);
    hipLaunchKernelGGL(k_reduced_rows, dim3(nb), dim3(256), 0, st, P.sym_rowptr, P.sym_col, P.sym_q, P.kval, s1, s2, xv, q, b, tau, part, n, m);
    hipLaunchKernelGGL(k_reduced_finish, dim3(1), dim3(256), 0, st, part, nb, tau, kappa, rhs_tau, rhs_kappa, scal_out);
    hipLaunchKernelGGL(k_reduced_axpy, dim3(nblk(n + m)), dim3(256), 0, st, s1, s2, scal_out, lhs, n + m);
}
void launch_const_rhs(hipStream_t st, double *dst, const double *qb, int n, int nm, int N) {
    if (N > 0) hipLaunchKernelGGL(k_const_rhs, dim3(nblk(N)), dim3(256), 0, st, dst, qb, n, nm, N);
}
void launch_norm_inf(hipStream_t st, const double *v, int n, unsigned long long *slot) {
    if (n > 0) hipLaunchKernelGGL(k_norm_inf, dim3(min(nblk(n), 64u)), dim3(256), 0, st, v, n, slot);
}
void launch_set_rhs(hipStream_t st, double *b, const double *rhs, int nm, int n) {
    if (n > 0) hipLaunchKernelGGL(k_set_rhs, dim3(nblk(n)), dim3(256), 0, st, b, rhs, nm, n);
}
void launch_check_finite(hipStream_t st, const double *v, int n, int *flags) {
    if (n > 0) hipLaunchKernelGGL(k_check_finite, dim3(nblk(n)), dim3(256), 0, st, v, n, flags);
}

}  // namespace hipkkt
