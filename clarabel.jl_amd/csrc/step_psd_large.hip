// The cone algebra of one interior-point step on the rows of PSD triangle cones of side 65 .. 128 (opt-in, hipkkt_step_enable_psd_large):
// the operations of step_psd.hip with the same arithmetic and another placement.  Three or four n x n matrices of such a cone do not
// fit one workgroup's LDS, so the matrices stay in global memory (a per-handle workspace of kPsdLargeMats matrices per large cone) and
// every product is a batched launch of 16 x 16 output tiles, grid (tile, large cone, z / s), whose operands are read through views:
//   Plain / Trans    a column-major n x n factor or workspace matrix, or its transpose
//   Svec             svec_to_mat of the cone's rows of a vector                                (psd_cone.h svec_entry)
//   RoundTrip        svec_to_mat(mat_to_svec(Y)) of a workspace matrix                         (psd_cone.h round_trip_entry)
//   Offset           the round trip of X~_ij = 2 DS_ij / (lambda_i + lambda_j)                 (step_psd.hip k_psd_offset)
// Every entry of every product is ONE fma chain over k = 0 .. n - 1 in ascending order starting from 0.0, and the elementwise
// expressions are the device functions of psd_cone.h that step_psd.hip calls too; both files are compiled with -ffp-contract=off.  So
// these kernels applied to a cone of side <= 64 give the bits of step_psd.hip (tests/test_gpu_psd_step_large.py holds them to that
// through the testing switch PSD_LARGE_MIN).  A tile stages 16-wide panels of both operands in LDS; that changes where an operand is
// read from, not the order of a sum.
// The smallest eigenvalue of the step length: one 256-thread workgroup per (cone, z / s) with M alone in LDS (128 x 129 doubles at side
// 128, the layout rule of psd_cone.h) and psd_jacobi_sweeps<64, 128> of psd_cone.h: the iteration of k_psd_len with wider lane
// mappings of the two rotation passes (half <= 64, rows <= 128).  The rotations of one set touch disjoint rows / columns: the mapping
// changes no bit.
// No assert, no trap, no waiting between workgroups; every loop has a fixed trip bound.  lidx = the large cones' indices into the table
// of step_psd.hip (cone_layout.h kPsd*); an entry whose side is outside lmin .. kPsdLargeMaxN is left alone (cone_of's lo / hi).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cone_layout.h"
#include "cone_reduce.h"
#include "kernels.h"
#include "psd_cone.h"

namespace hipkkt {

namespace {

constexpr int kMaxN = kPsdLargeMaxN;
constexpr int kTile = 16;
constexpr int kLdsDoubles = kMaxN * (kMaxN + 1);      // M of the Jacobi kernel, leading dimension n + 1 when n % 32 == 0
// (the cone record is cone_of(tab, c, lmin, kMaxN) of psd_cone.h; its K.ld is that LDS layout, the global matrices have ld = n)

enum View { kPlain = 0, kTrans = 1, kSvec = 2, kRoundTrip = 3, kOffset = 4 };
enum Where { kRows = 0, kFactor = 1, kWs0 = 2 };      // kWs0 + w: matrix w of the cone's workspace slot

// one operand of a product: how it is read and where the cone's part of `base` starts
struct Operand { int view; int where; const double *base; };
struct Product { Operand a, b; int out; };              // C = A B into workspace matrix `out`

__device__ __forceinline__ const double *resolve(const Operand &o, const Cone &K, int slot) {
    if (o.where == kRows) return o.base + K.row0;
    if (o.where == kFactor) return o.base + K.foff;
    return o.base + ((int64_t)slot * kPsdLargeMats + (o.where - kWs0)) * kPsdLargeMatDoubles;
}

// entry (i, j) of an operand; i, j < n
__device__ __forceinline__ double view_at(int view, const double *__restrict__ p, const double *__restrict__ lam, int n, int i, int j) {
    switch (view) {
        case kPlain: return p[i + j * n];
        case kTrans: return p[j + i * n];
        case kSvec: return svec_entry(p, i, j);
        case kRoundTrip: return round_trip_entry(p, n, i, j);
        default: {      // kOffset: X = svec_to_mat(ds), X_ij <- 2 X_ij / (lambda_i + lambda_j), then the round trip
            const double x = svec_entry(p, i, j);
            if (i == j) return 2.0 * x / (lam[i] + lam[j]);
            const int r = i < j ? i : j, c = i < j ? j : i;
            const double up = 2.0 * x / (lam[r] + lam[c]), lo = 2.0 * x / (lam[c] + lam[r]);
            return round_trip_pair(up, lo);
        }
    }
}

}  // namespace

// ---- products: C = A B, one 16 x 16 tile per workgroup, blockIdx.z picks the z / s chain --------------------------------------------
__global__ void __launch_bounds__(256)
k_psdl_product(const int64_t *__restrict__ tab, const int *__restrict__ lidx, int lmin, int tiles, Product pz, Product ps,
               const double *__restrict__ lam_all, double *__restrict__ ws) {
    __shared__ double As[kTile * kTile], Bs[kTile * kTile];      // As[k][i], Bs[j][k]
    const int slot = blockIdx.y;
    const Cone K = cone_of(tab, lidx[slot], lmin, kMaxN);
    if (!K.ok) return;
    const int n = K.n, ti = threadIdx.x & (kTile - 1), tj = threadIdx.x >> 4;
    const int i0 = ((int)blockIdx.x % tiles) * kTile, j0 = ((int)blockIdx.x / tiles) * kTile;
    if (i0 >= n || j0 >= n) return;                              // (uniform per workgroup)
    const Product &P = blockIdx.z ? ps : pz;
    const double *pa = resolve(P.a, K, slot), *pb = resolve(P.b, K, slot), *lam = lam_all + K.loff;
    double *out = ws + ((int64_t)slot * kPsdLargeMats + P.out) * kPsdLargeMatDoubles;
    const int i = i0 + ti, j = j0 + tj;
    double acc = 0.0;
    for (int k0 = 0; k0 < n; k0 += kTile) {                      // (at most kMaxN / kTile = 8 panels)
        const int ka = k0 + tj, kb = k0 + ti;
        As[tj * kTile + ti] = (i < n && ka < n) ? view_at(P.a.view, pa, lam, n, i, ka) : 0.0;
        Bs[tj * kTile + ti] = (kb < n && j < n) ? view_at(P.b.view, pb, lam, n, kb, j) : 0.0;
        __syncthreads();
        const int kw = n - k0 < kTile ? n - k0 : kTile;
        for (int k = 0; k < kw; k++) acc = fma(As[k * kTile + ti], Bs[tj * kTile + k], acc);
        __syncthreads();
    }
    if (i < n && j < n) out[i + j * n] = acc;
}

// ---- circ_op of combined_ds_shift: out = (B A + A B) / 2 from the round trips of workspace matrices ia and ib -----------------------------
__global__ void __launch_bounds__(256)
k_psdl_circ(const int64_t *__restrict__ tab, const int *__restrict__ lidx, int lmin, int tiles, int ia, int ib, int iout,
            double *__restrict__ ws) {
    __shared__ double Ai[kTile * kTile], Bi[kTile * kTile], Aj[kTile * kTile], Bj[kTile * kTile];   // A(i, k), B(i, k) as [k][i]; A(k, j), B(k, j) as [j][k]
    const int slot = blockIdx.y;
    const Cone K = cone_of(tab, lidx[slot], lmin, kMaxN);
    if (!K.ok) return;
    const int n = K.n, ti = threadIdx.x & (kTile - 1), tj = threadIdx.x >> 4;
    const int i0 = ((int)blockIdx.x % tiles) * kTile, j0 = ((int)blockIdx.x / tiles) * kTile;
    if (i0 >= n || j0 >= n) return;
    double *base = ws + (int64_t)slot * kPsdLargeMats * kPsdLargeMatDoubles;
    const double *A = base + (int64_t)ia * kPsdLargeMatDoubles, *B = base + (int64_t)ib * kPsdLargeMatDoubles;
    double *out = base + (int64_t)iout * kPsdLargeMatDoubles;
    const int i = i0 + ti, j = j0 + tj;
    double ba = 0.0, ab = 0.0;
    for (int k0 = 0; k0 < n; k0 += kTile) {
        const int ka = k0 + tj, kb = k0 + ti;
        const bool ina = i < n && ka < n, inb = kb < n && j < n;
        Ai[tj * kTile + ti] = ina ? view_at(kRoundTrip, A, nullptr, n, i, ka) : 0.0;
        Bi[tj * kTile + ti] = ina ? view_at(kRoundTrip, B, nullptr, n, i, ka) : 0.0;
        Aj[tj * kTile + ti] = inb ? view_at(kRoundTrip, A, nullptr, n, kb, j) : 0.0;
        Bj[tj * kTile + ti] = inb ? view_at(kRoundTrip, B, nullptr, n, kb, j) : 0.0;
        __syncthreads();
        const int kw = n - k0 < kTile ? n - k0 : kTile;
        for (int k = 0; k < kw; k++) {
            ba = fma(Bi[k * kTile + ti], Aj[tj * kTile + k], ba);
            ab = fma(Ai[k * kTile + ti], Bj[tj * kTile + k], ab);
        }
        __syncthreads();
    }
    if (i < n && j < n) out[i + j * n] = 0.5 * (ba + ab);
}

// ---- out = mat_to_svec(Y) of workspace matrix iy; diag_add goes to the diagonal positions; addc != NULL: out = -(out + addc) ---------------
__global__ void __launch_bounds__(256)
k_psdl_store(const int64_t *__restrict__ tab, const int *__restrict__ lidx, int lmin, int iy, const double *__restrict__ ws,
             double diag_add, const double *__restrict__ addc_all, double *__restrict__ out_all) {
    const int slot = blockIdx.y;
    const Cone K = cone_of(tab, lidx[slot], lmin, kMaxN);
    if (!K.ok) return;
    const int n = K.n;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n * n) return;
    const double *Y = ws + ((int64_t)slot * kPsdLargeMats + iy) * kPsdLargeMatDoubles;
    store_svec_entry(out_all + K.row0, Y, n, n, e, diag_add, addc_all ? addc_all + K.row0 : nullptr);
}

// ---- affine_ds: lambda_k^2 at the diagonal positions, 0 elsewhere -------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_psdl_affine_ds(const int64_t *__restrict__ tab, const int *__restrict__ lidx, int lmin, const double *__restrict__ lam_all,
                 double *__restrict__ out_all) {
    const Cone K = cone_of(tab, lidx[blockIdx.y], lmin, kMaxN);
    if (!K.ok) return;
    const int n = K.n;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n * n) affine_ds_entry(out_all + K.row0, lam_all + K.loff, n, e);
}

// ---- step length: M = Lambda^-1/2 D Lambda^-1/2 from the round trip of workspace matrix id0 + blockIdx.y, its smallest eigenvalue ----------
// blockIdx.y = 0: z, 1: s.  part[2 c + blockIdx.y] = the cone's alpha (c = its index in the table).
__global__ void __launch_bounds__(256)
k_psdl_len(const int64_t *__restrict__ tab, const int *__restrict__ lidx, int lmin, int id0, const double *__restrict__ ws,
           const double *__restrict__ lam_all, double alpha_max, double *__restrict__ part) {
    __shared__ double M[kLdsDoubles];
    __shared__ double red[4];
    // the sweeps' scratch: rs = the rotations' s, rc = their s / (1 + c), rp < rq their index pairs.  One struct fixes the order in
    // LDS: with rq below rp the compiler loads a pair's two indices with one ds_read2st64_b32 in both rotation passes (as separate
    // arrays it did so in one pass only, and k_psdl_len measured 3 % slower with the shared loop than with its own copy)
    __shared__ struct { double rc[kMaxN / 2], rs[kMaxN / 2]; int rq[kMaxN / 2], rp[kMaxN / 2]; } rot;
    double *rc = rot.rc, *rs = rot.rs;
    int *rp = rot.rp, *rq = rot.rq;
    const int slot = blockIdx.x, which = blockIdx.y, t = threadIdx.x;
    const int c = lidx[slot];
    const Cone K = cone_of(tab, c, lmin, kMaxN);
    if (!K.ok) return;
    const int n = K.n, ld = K.ld;
    const double *lam = lam_all + K.loff;
    const double *D = ws + ((int64_t)slot * kPsdLargeMats + id0 + which) * kPsdLargeMatDoubles;
    double tot2 = 0.0;
    for (int e = t; e < n * n; e += 256) {                // M = Lambda^-1/2 D Lambda^-1/2
        const int i = e % n, j = e / n;
        const double v = ((1.0 / sqrt(lam[i])) * view_at(kRoundTrip, D, nullptr, n, i, j)) * (1.0 / sqrt(lam[j]));
        M[i + j * ld] = v;
        tot2 += v * v;
    }
    tot2 = block_sum(tot2, red);                          // (its barriers order the writes above before the reads below)
    // the Jacobi sweeps of psd_cone.h with the lane widths of a side up to 128 (half <= 64, rows <= 128); a non-finite |M|_F skips them
    const bool finite = psd_jacobi_sweeps<64, 128>(M, K, tot2, red, rc, rs, rp, rq);
    double g = finite ? 1.7976931348623157e308 : tot2 - tot2;      // (a non-finite M: gamma = NaN)
    if (finite) for (int i = t; i < n; i += 256) g = nan_min(M[i + i * ld], g);
    g = block_nan_min(g, red);
    if (t == 0) part[2 * c + which] = g < 0.0 ? fmin(1.0 / (-g), alpha_max) : alpha_max;
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
int psd_step_large_max_dim() { return kMaxN; }
int64_t psd_large_ws_doubles(int nlarge) { return (int64_t)nlarge * kPsdLargeMats * kPsdLargeMatDoubles; }

namespace {

// what every launch of one operation shares: the stream, the tables and the tile count of the largest side
struct Batch {
    hipStream_t st; const PsdView &P; const PsdLargeBatch &L; int tiles;
    Batch(hipStream_t st_, const PsdView &P_) : st(st_), P(P_), L(P_.large), tiles((P_.large.max_n + kTile - 1) / kTile) {}
    Operand rows(int view, const double *v) const { return {view, kRows, v}; }
    Operand factor(int view, const double *f) const { return {view, kFactor, f}; }
    Operand mat(int view, int w) const { return {view, kWs0 + w, L.ws}; }
    void product(const Product &pz, const Product *ps) const {
        hipLaunchKernelGGL(k_psdl_product, dim3(tiles * tiles, L.nlarge, ps ? 2 : 1), dim3(256), 0, st, P.tab, L.lidx, L.lmin, tiles, pz,
                           ps ? *ps : pz, P.lam, L.ws);
    }
    void store(int iy, double diag_add, const double *addc, double *out) const {
        const int n = tiles * kTile;
        hipLaunchKernelGGL(k_psdl_store, dim3((n * n + 255) / 256, L.nlarge), dim3(256), 0, st, P.tab, L.lidx, L.lmin, iy, L.ws, diag_add,
                           addc, out);
    }
    // the first two products of both chains: matrix 2 = R' dZ R (z, through matrix 0), matrix 3 = Rinv dS Rinv' (s, through matrix 1)
    void scaled_pair(const double *dz, const double *ds) const {
        const Product z1{rows(kSvec, dz), factor(kPlain, P.R), 0}, s1{rows(kSvec, ds), factor(kTrans, P.Rinv), 1};
        product(z1, &s1);
        const Product z2{factor(kTrans, P.R), mat(kPlain, 0), 2}, s2{factor(kPlain, P.Rinv), mat(kPlain, 1), 3};
        product(z2, &s2);
    }
};

}  // namespace

void launch_psd_large_affine_ds(hipStream_t st, const PsdView &P, double *out) {
    const PsdLargeBatch &L = P.large;
    if (L.nlarge <= 0) return;
    hipLaunchKernelGGL(k_psdl_affine_ds, dim3((L.max_n * L.max_n + 255) / 256, L.nlarge), dim3(256), 0, st, P.tab, L.lidx, L.lmin, P.lam, out);
}
void launch_psd_large_mulhs(hipStream_t st, const PsdView &P, const double *x, const double *addc, double *y) {
    if (P.large.nlarge <= 0) return;
    const Batch B(st, P);
    B.product({B.rows(kSvec, x), B.factor(kPlain, P.R), 0}, nullptr);        // T = X R
    B.product({B.factor(kTrans, P.R), B.mat(kPlain, 0), 1}, nullptr);        // Y = R' T       (W x)
    B.product({B.mat(kRoundTrip, 1), B.factor(kTrans, P.R), 0}, nullptr);    // T = Y R'
    B.product({B.factor(kPlain, P.R), B.mat(kPlain, 0), 1}, nullptr);        // Y = R T        (W' W x)
    B.store(1, 0.0, addc, y);
}
void launch_psd_large_shift(hipStream_t st, const PsdView &P, const double *dz, const double *ds, double sigma_mu, double *out) {
    const PsdLargeBatch &L = P.large;
    if (L.nlarge <= 0) return;
    const Batch B(st, P);
    B.scaled_pair(dz, ds);                                                   // A = W dz in matrix 2, B = W^-T ds in matrix 3
    hipLaunchKernelGGL(k_psdl_circ, dim3(B.tiles * B.tiles, L.nlarge), dim3(256), 0, st, P.tab, L.lidx, L.lmin, B.tiles, 2, 3, 0, L.ws);
    B.store(0, -sigma_mu, nullptr, out);
}
void launch_psd_large_offset(hipStream_t st, const PsdView &P, const double *ds, double *out) {
    if (P.large.nlarge <= 0) return;
    const Batch B(st, P);
    B.product({B.rows(kOffset, ds), B.factor(kTrans, P.R), 0}, nullptr);     // T = X~ R'
    B.product({B.factor(kPlain, P.R), B.mat(kPlain, 0), 1}, nullptr);        // Y = R T
    B.store(1, 0.0, nullptr, out);
}
void launch_psd_large_length(hipStream_t st, const PsdView &P, const double *dz, const double *ds, double alpha_max, double *part) {
    const PsdLargeBatch &L = P.large;
    if (L.nlarge <= 0) return;
    const Batch B(st, P);
    B.scaled_pair(dz, ds);
    hipLaunchKernelGGL(k_psdl_len, dim3(L.nlarge, 2), dim3(256), 0, st, P.tab, L.lidx, L.lmin, 2, L.ws, P.lam, alpha_max, part);
}

}  // namespace hipkkt
