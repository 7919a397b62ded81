// The default start of a symmetric cone set on the device (solver.jl:383-405): what the caller's host loop does before the first
// iteration, on the resident K, q, b and the tables of scaling.hip / step_psd.hip.
//   identity scaling     set_identity_scaling! + get_Hs! + the Hs / sparse-cone part of _kktsolver_update_inner! written straight into
//                        the resident K: Zero -0, Nonnegative -1, second-order cones their dense (dim <= 4) block or d = 0.5,
//                        u = [sqrt 0.5, 0 ...], v = 0, eta^2 = 1 (coneops_socone.jl:57-73, directldl_datamaps.jl:61-79), PSD cones the
//                        packed upper triangle of I (coneops_psdtrianglecone.jl:66-75); every value is the bits hipkkt_set_hs /
//                        hipkkt_set_soc_batch leave after the host cones' set_identity_scaling
//   margins              (alpha, beta) of margins(::CompositeCone), coneops_compositecone.jl:49-63, per cone coneops_zerocone.jl:27-39,
//                        coneops_nncone.jl:19-38, coneops_socone.jl:13-22, coneops_psdtrianglecone.jl:8-27 (eigenvalues by the Jacobi
//                        sweeps of psd_cone.h)
//   decide / shift       _shift_to_cone_interior!, variables.jl:180-208, with scaled_unit_shift! of each cone
//   rhs / assemble       the right-hand sides and the sign flips of kkt_solve_initial_point!, kktsystem.jl:95-132
// blockIdx.y selects the side where a launch serves both vectors of the fused call (s: primal, z: dual).  A NaN keeps to the
// reference's rules: min and max propagate it, `x > 0 ? x : 0` drops it, both comparisons of the shift are false and the last arm
// (shift by 0) is taken.  Sums run over fixed slices in a fixed order: deterministic.  Compiled with -ffp-contract=off: the shift is
// two separately rounded additions.  No assert, no trap, no spin; every loop is bounded by a cone's size or kPsdMaxSweeps.
// PSD sides of 65 .. 128 (hipkkt_step_default_start_enable_psd_large): the identity scaling is indexed by column of the packed triangle
// and does not depend on the side, the margins of such a cone come from k_start_margin_psd_large (one 128 x 129 matrix in LDS, the
// sweeps with the lane widths of k_psdl_len), the shift takes the side bound as an argument.
// Everything is HBM / latency bound: the identity scaling writes nHs doubles through map_hs (8 + 8 bytes per entry), the rest moves a
// few m doubles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cone_layout.h"
#include "cone_reduce.h"
#include "kernels.h"
#include "psd_cone.h"

namespace hipkkt {

namespace {

constexpr double kFloatMax = 1.7976931348623157e308;
constexpr int kSlices = 64;                  // fixed slices of the Nonnegative rows, as k_step_norm_part
constexpr double kSqrtHalf = 0.7071067811865476;      // sqrt(0.5)
constexpr double kSqrt2 = 1.4142135623730951;         // sqrt(2.0)

// max that keeps a NaN (the reference's max)
__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

// partials of one side: [Nonnegative: kSlices x (min, sum of positive)] [second-order: alpha per cone] [PSD: (alpha, beta) per cone]
__host__ __device__ inline int64_t side_doubles(int nsoc, int npsd) { return 2 * kSlices + nsoc + 2 * (int64_t)npsd; }

}  // namespace

// ---- identity scaling ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_start_identity_diag(const signed char *__restrict__ row_kind, const int64_t *__restrict__ row_hs, const int64_t *__restrict__ map_hs,
                      double *__restrict__ kval, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int kind = row_kind[i];
    if (kind == 0) kval[map_hs[row_hs[i]]] = -0.0;
    else if (kind == 1) kval[map_hs[row_hs[i]]] = -1.0;
}
// one workgroup per second-order cone (the descriptors of k_scaling_soc); w = e1, eta = 1
__global__ void __launch_bounds__(256)
k_start_identity_soc(const int64_t *__restrict__ desc, const int64_t *__restrict__ map_hs, double *__restrict__ soc_u,
                     double *__restrict__ soc_v, double *__restrict__ soc_eta2, double *__restrict__ kval) {
    const int c = blockIdx.x, t = threadIdx.x;
    const int64_t dim = desc[kSocDesc * c + kSocDim], hs0 = desc[kSocDesc * c + kSocHs0];
    const int64_t uv0 = desc[kSocDesc * c + kSocUv0], ord = desc[kSocDesc * c + kSocOrd];
    const double eta2 = 1.0;
    if (uv0 >= 0) {
        double *u = soc_u + uv0, *v = soc_v + uv0;
        for (int64_t i = t; i < dim; i += 256) {
            u[i] = i == 0 ? kSqrtHalf : 0.0;
            v[i] = 0.0;
            kval[map_hs[hs0 + i]] = -(i == 0 ? eta2 * 0.5 : eta2);
        }
        if (t == 0) soc_eta2[ord] = eta2;
    } else if (t == 0) {
        // the dense block of coneops_socone.jl:173-189 at w = e1: its first entry is (sqrt 2 - 1)(sqrt 2 + 1) as rounded, not 1
        const double w0 = 1.0;
        int64_t h = 0;
        kval[map_hs[hs0 + h++]] = -(((kSqrt2 * w0 - 1.0) * (kSqrt2 * w0 + 1.0)) * eta2);
        for (int col = 1; col < (int)dim; col++)
            for (int row = 0; row <= col; row++) kval[map_hs[hs0 + h++]] = row == col ? -1.0 : -0.0;
    }
}
// blockIdx.y = PSD cone, blockIdx.x = column b of its packed upper triangle (numel x numel): entries b (b + 1) / 2 + a, a <= b
__global__ void __launch_bounds__(256)
k_start_identity_psd(const int64_t *__restrict__ tab, const int64_t *__restrict__ hs0_all, const int64_t *__restrict__ map_hs,
                     double *__restrict__ kval) {
    const int c = blockIdx.y;
    const int64_t n = tab[kPsdTab * c + kPsdN], numel = n * (n + 1) / 2, b = blockIdx.x;
    if (b >= numel) return;
    const int64_t e0 = hs0_all[c] + b * (b + 1) / 2;
    for (int64_t a = threadIdx.x; a <= b; a += 256) kval[map_hs[e0 + a]] = a == b ? -1.0 : -0.0;
}

// ---- margins -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_start_margin_nn(const signed char *__restrict__ row_kind, const double *__restrict__ v0, const double *__restrict__ v1,
                  double *__restrict__ part, int64_t stride, int64_t m) {
    __shared__ double red[4];
    const double *v = blockIdx.y ? v1 : v0;
    const int64_t len = (m + kSlices - 1) / kSlices, lo = (int64_t)blockIdx.x * len, hi = lo + len < m ? lo + len : m;
    double mn = kFloatMax, sum = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        if (row_kind[i] != 1) continue;
        const double x = v[i];
        mn = nan_min(x, mn);
        sum += x > 0.0 ? x : 0.0;
    }
    mn = block_nan_min(mn, red);
    sum = block_sum(sum, red);
    if (threadIdx.x == 0) { double *p = part + blockIdx.y * stride + 2 * blockIdx.x; p[0] = mn; p[1] = sum; }
}
__global__ void __launch_bounds__(256)
k_start_margin_soc(const int64_t *__restrict__ desc, const double *__restrict__ v0, const double *__restrict__ v1,
                   double *__restrict__ part, int64_t stride) {
    __shared__ double red[4];
    const int c = blockIdx.x;
    const int64_t row0 = desc[kSocDesc * c + kSocRow0], dim = desc[kSocDesc * c + kSocDim];
    const double *z = (blockIdx.y ? v1 : v0) + row0;
    double acc = 0.0;
    for (int64_t i = 1 + threadIdx.x; i < dim; i += 256) acc += z[i] * z[i];
    const double z1 = sqrt(block_sum(acc, red));
    if (threadIdx.x == 0) part[blockIdx.y * stride + 2 * kSlices + c] = z[0] - z1;
}
// (alpha, beta) of one PSD cone from the rows v of its vector: M = svec_to_mat, the Jacobi sweeps of psd_cone.h with the lane widths
// of the caller's largest side, the minimum and the sum of the positive eigenvalues in ascending index order by thread 0
template <int kPairLanes, int kRowLanes>
__device__ __forceinline__ void margin_psd_cone(double *M, const Cone &K, const double *__restrict__ v, double *red, double *rc,
                                                double *rs, int *rp, int *rq, double *out) {
    const int n = K.n, ld = K.ld, t = threadIdx.x;
    load_svec(M, v, K);
    __syncthreads();
    double tot2 = 0.0;
    for (int e = t; e < n * n; e += 256) { const double x = M[e % n + (e / n) * ld]; tot2 += x * x; }
    tot2 = block_sum(tot2, red);
    const bool finite = psd_jacobi_sweeps<kPairLanes, kRowLanes>(M, K, tot2, red, rc, rs, rp, rq);
    if (t != 0) return;
    double a = tot2 - tot2, b = tot2 - tot2;      // (a non-finite matrix: NaN margins)
    if (finite) {
        a = kFloatMax; b = 0.0;
        for (int i = 0; i < n; i++) { const double e = M[i + i * ld]; a = nan_min(e, a); b = e > 0.0 ? b + e : b; }
    }
    out[0] = a; out[1] = b;
}
// one workgroup per (cone, side), ONE matrix in LDS so that several workgroups share a compute unit
__global__ void __launch_bounds__(256)
k_start_margin_psd(const int64_t *__restrict__ tab, const double *__restrict__ v0, const double *__restrict__ v1,
                   double *__restrict__ part, int64_t stride, int nsoc) {
    __shared__ double M[kPsdMatDoubles];
    __shared__ double red[4], rc[kPsdMaxN / 2], rs[kPsdMaxN / 2];
    __shared__ int rp[kPsdMaxN / 2], rq[kPsdMaxN / 2];
    const int c = blockIdx.x, t = threadIdx.x;
    double *out = part + blockIdx.y * stride + 2 * kSlices + nsoc + 2 * (int64_t)c;
    const Cone K = cone_of(tab, c);
    if (!K.ok) { if (t == 0) { out[0] = kFloatMax; out[1] = 0.0; } return; }
    margin_psd_cone<32, 64>(M, K, (blockIdx.y ? v1 : v0) + K.row0, red, rc, rs, rp, rq, out);
}
// the cones of side lmin .. 128 (hipkkt_step_default_start_enable_psd_large; lidx: their indices into tab), one workgroup per (cone,
// side) with the LDS budget of k_psdl_len: launched behind k_start_margin_psd on the same stream, it overwrites the {floatmax, 0} that
// kernel left for a side above 64 (and the same bits for a smaller side the testing switch routes here)
__global__ void __launch_bounds__(256)
k_start_margin_psd_large(const int64_t *__restrict__ tab, const int *__restrict__ lidx, int lmin, const double *__restrict__ v0,
                         const double *__restrict__ v1, double *__restrict__ part, int64_t stride, int nsoc) {
    __shared__ double M[kPsdLargeMaxN * (kPsdLargeMaxN + 1)];
    __shared__ double red[4], rc[kPsdLargeMaxN / 2], rs[kPsdLargeMaxN / 2];
    __shared__ int rp[kPsdLargeMaxN / 2], rq[kPsdLargeMaxN / 2];
    const int c = lidx[blockIdx.x];
    double *out = part + blockIdx.y * stride + 2 * kSlices + nsoc + 2 * (int64_t)c;
    const Cone K = cone_of(tab, c, lmin, kPsdLargeMaxN);
    if (!K.ok) return;
    margin_psd_cone<64, 128>(M, K, (blockIdx.y ? v1 : v0) + K.row0, red, rc, rs, rp, rq, out);
}

// ---- the branch of _shift_to_cone_interior! ---------------------------------------------------------------------------------------
// one workgroup per side; dec[8 side ..] = {min_margin, pos_margin, target, branch, a, b, two_stage}: the shift adds a, then b when
// two_stage.  Nonnegative slices, second-order cones, PSD cones, in this order; within a kind thread t takes the entries t, t + 256, ...
// in ascending order and block_sum adds the 256 results in its fixed tree.
__global__ void __launch_bounds__(256)
k_start_decide(const double *__restrict__ part, int64_t stride, int nsoc, int npsd, double degree, double *__restrict__ dec) {
    __shared__ double red[4];
    const int t = threadIdx.x;
    const double *p = part + blockIdx.x * stride, *ps = p + 2 * kSlices, *pp = ps + nsoc;
    double mn = kFloatMax, bnn = 0.0, bsoc = 0.0, bpsd = 0.0;
    if (t < kSlices) mn = p[2 * t];
    for (int k = t; k < nsoc; k += 256) { const double a = ps[k]; mn = nan_min(a, mn); bsoc += nan_max(a, 0.0); }
    for (int k = t; k < npsd; k += 256) { mn = nan_min(pp[2 * k], mn); bpsd += pp[2 * k + 1]; }
    mn = block_nan_min(mn, red);
    bsoc = block_sum(bsoc, red);
    bpsd = block_sum(bpsd, red);
    if (t != 0) return;
    for (int k = 0; k < kSlices; k++) bnn += p[2 * k + 1];
    const double beta = (bnn + bsoc) + bpsd;
    const double target = degree > 0.0 ? nan_max(0.1 * beta / degree, 1.0) : 1.0;
    double branch = 2.0, a = 0.0, b = 0.0, two = 0.0;
    if (mn <= 0.0) { branch = 0.0; a = -mn; b = target; two = 1.0; }
    else if (mn < target) { branch = 1.0; a = target - mn; }
    double *d = dec + 8 * blockIdx.x;
    d[0] = mn; d[1] = beta; d[2] = target; d[3] = branch; d[4] = a; d[5] = b; d[6] = two; d[7] = 0.0;
}

// ---- scaled_unit_shift! of every cone ---------------------------------------------------------------------------------------------
// blockIdx.x: [0, nrow) one thread per row (Zero / Nonnegative), [nrow, nrow + nsocb) one thread per second-order cone (first row),
// then one workgroup per PSD cone (rows triangular_index(k)); blockIdx.y = side, pd 0 primal / 1 dual
__global__ void __launch_bounds__(256)
k_start_shift(const signed char *__restrict__ row_kind, const int64_t *__restrict__ desc, const int64_t *__restrict__ tab,
              const double *__restrict__ dec, double *__restrict__ v0, int pd0, double *__restrict__ v1, int pd1, int64_t m, int nsoc,
              unsigned nrow, unsigned nsocb, int psd_max_side) {
    const int side = blockIdx.y;
    double *v = side ? v1 : v0;
    const int pd = side ? pd1 : pd0;
    const double a = dec[8 * side + 4], b = dec[8 * side + 5];
    const bool two = dec[8 * side + 6] != 0.0;
    int64_t row = -1;
    if (blockIdx.x < nrow) {
        const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (i >= m) return;
        const int kind = row_kind[i];
        if (kind == 0) { if (pd == 0) v[i] = 0.0; return; }
        if (kind == 1) row = i;
    } else if (blockIdx.x < nrow + nsocb) {
        const int64_t c = (int64_t)(blockIdx.x - nrow) * 256 + threadIdx.x;
        if (c < nsoc) row = desc[kSocDesc * c + kSocRow0];
    } else {
        const int c = blockIdx.x - nrow - nsocb;
        const int64_t n = tab[kPsdTab * c + kPsdN], k = threadIdx.x;
        if (k < n && n <= psd_max_side) row = tab[kPsdTab * c + kPsdRow0] + (k + 1) * (k + 2) / 2 - 1;
    }
    if (row < 0) return;
    double x = v[row];
    x = x + a;
    if (two) x = x + b;
    v[row] = x;
}

// ---- kkt_solve_initial_point! -----------------------------------------------------------------------------------------------------
// mode 1: [0; b; 0], mode 2: [-q; 0; 0] (kktsystem.jl:105-120); [-q; b; 0] is k_const_rhs
__global__ void __launch_bounds__(256)
k_start_rhs(double *__restrict__ dst, const double *__restrict__ qb, int n, int nm, int N, int mode) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double x = 0.0;
    if (i < n) { if (mode == 2) x = -qb[i]; }
    else if (i < nm) { if (mode == 1) x = qb[i]; }
    dst[i] = x;
}
// xzs = [x | z | s] from the solutions sa = [x | .], sb: nnz(P) != 0 (sb == NULL): z = sa.z, s = -z; otherwise s = -sa.z, z = sb.z
__global__ void __launch_bounds__(256)
k_start_assemble(double *__restrict__ xzs, const double *__restrict__ sa, const double *__restrict__ sb, int64_t n, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) xzs[i] = sa[i];
    if (i < m) {
        const double za = sa[n + i];
        xzs[n + i] = sb ? sb[n + i] : za;
        xzs[n + m + i] = -za;
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
static inline dim3 rows_grid(int64_t len) { return dim3((unsigned)((len + 255) / 256)); }

int64_t start_work_doubles(int64_t ncones) { return 2 * side_doubles((int)ncones, (int)ncones) + 16; }

void launch_start_identity(hipStream_t st, const signed char *row_kind, const int64_t *row_hs, const int64_t *map_hs, int nsoc,
                           const int64_t *desc, double *soc_u, double *soc_v, double *soc_eta2, const PsdView &P,
                           const int64_t *psd_hs0, int64_t psd_max_numel, double *kval, int64_t m) {
    if (m > 0) hipLaunchKernelGGL(k_start_identity_diag, rows_grid(m), dim3(256), 0, st, row_kind, row_hs, map_hs, kval, m);
    if (nsoc > 0) hipLaunchKernelGGL(k_start_identity_soc, dim3(nsoc), dim3(256), 0, st, desc, map_hs, soc_u, soc_v, soc_eta2, kval);
    if (P.npsd > 0 && psd_max_numel > 0)
        hipLaunchKernelGGL(k_start_identity_psd, dim3((unsigned)psd_max_numel, P.npsd), dim3(256), 0, st, P.tab, psd_hs0, map_hs, kval);
}

// work: start_work_doubles(ncones) doubles; the decision records of the nsides sides end up at start_decision(work, ncones)
double *start_decision(double *work, int64_t ncones) { return work + 2 * side_doubles((int)ncones, (int)ncones); }

void launch_start_margins(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, const PsdView &P, const double *v0,
                          const double *v1, int nsides, double degree, double *work, int64_t ncones, int64_t m, bool psd_large) {
    const int npsd = P.npsd;
    const int64_t stride = side_doubles(nsoc, npsd);
    hipLaunchKernelGGL(k_start_margin_nn, dim3(kSlices, nsides), dim3(256), 0, st, row_kind, v0, v1, work, stride, m);
    if (nsoc > 0) hipLaunchKernelGGL(k_start_margin_soc, dim3(nsoc, nsides), dim3(256), 0, st, desc, v0, v1, work, stride);
    if (npsd > 0) hipLaunchKernelGGL(k_start_margin_psd, dim3(npsd, nsides), dim3(256), 0, st, P.tab, v0, v1, work, stride, nsoc);
    if (psd_large && P.large.nlarge > 0)
        hipLaunchKernelGGL(k_start_margin_psd_large, dim3(P.large.nlarge, nsides), dim3(256), 0, st, P.tab, P.large.lidx, P.large.lmin, v0,
                           v1, work, stride, nsoc);
    hipLaunchKernelGGL(k_start_decide, dim3(nsides), dim3(256), 0, st, work, stride, nsoc, npsd, degree, start_decision(work, ncones));
}

void launch_start_shift(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, const PsdView &P, const double *dec,
                        double *v0, int pd0, double *v1, int pd1, int nsides, int64_t m, bool psd_large) {
    const unsigned nrow = (unsigned)((m + 255) / 256), nsocb = (unsigned)((nsoc + 255) / 256);
    const unsigned total = nrow + nsocb + (unsigned)P.npsd;
    if (total > 0)
        hipLaunchKernelGGL(k_start_shift, dim3(total, nsides), dim3(256), 0, st, row_kind, desc, P.tab, dec, v0, pd0, v1, pd1, m, nsoc,
                           nrow, nsocb, psd_large ? kPsdLargeMaxN : kPsdMaxN);
}

void launch_start_rhs(hipStream_t st, double *dst, const double *qb, int n, int nm, int N, int mode) {
    if (N > 0) hipLaunchKernelGGL(k_start_rhs, rows_grid(N), dim3(256), 0, st, dst, qb, n, nm, N, mode);
}
void launch_start_assemble(hipStream_t st, double *xzs, const double *sa, const double *sb, int64_t n, int64_t m) {
    const int64_t len = n > m ? n : m;
    if (len > 0) hipLaunchKernelGGL(k_start_assemble, rows_grid(len), dim3(256), 0, st, xzs, sa, sb, n, m);
}

}  // namespace hipkkt
