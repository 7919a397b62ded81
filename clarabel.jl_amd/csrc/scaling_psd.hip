// The Nesterov-Todd scaling of PSD triangle cones on the device (opt-in, hipkkt_psd_scaling_enable on a handle in PSD step mode):
// update_scaling!(::PSDTriangleCone), coneops_psdtrianglecone.jl:78-143, from the (s, z) of the scaling call to the resident
// (R, Rinv, lambda) that step_psd.hip reads.  Per cone, with S = svec_to_mat(s), Z = svec_to_mat(z):
//   S = L1 L1', Z = L2 L2'      lower Cholesky factors (:93-98); a pivot that is not > 0 or not finite fails the cone, as potrf does
//   G = L2' L1 = U Sigma V'     singular values and vectors (:107-110)
//   lambda = sigma              descending, LAPACK's order (:112-113)
//   R = L1 V Sigma^-1/2         (:115-123)
//   Rinv = Sigma^-1/2 U' L2'    (:125-131)
// One 256-thread workgroup per cone, four n x n matrices in LDS (psd_cone.h: column-major, leading dimension n + 1 when n % 32 == 0),
// no communication between workgroups, no spin, every loop with a fixed trip bound.
//
// The SVD is a one-sided (Hestenes) Jacobi iteration on the columns of G with V accumulating the rotations: per sweep np - 1 sets of
// np / 2 disjoint column pairs (the round-robin pairing of k_psd_len, np = n rounded up to even, the index n of an odd n is a dummy).
// The eight lanes t = 8 k .. 8 k + 7 own pair k of a set: lane l sums rows l, l + 8, .. of a = |g_p|^2, b = |g_q|^2, c = g_p . g_q in
// ascending order, a butterfly over the eight lanes gives every one of them the same three sums, and each lane rotates its own rows of
// G and V.  A pair rotates when |c| > eps sqrt(a b), with zeta = (b - a) / 2c, t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)),
// cs = 1 / sqrt(1 + t^2), sn = t cs, in the small-angle form x_p - sn (x_q + r x_p), x_q + sn (x_p - r x_q), r = sn / (1 + cs).  One
// barrier per set.  The iteration stops after a sweep without a rotation (a block sum that every thread receives) and gives up after
// kMaxSweeps.  One polishing sweep follows in which every pair with c != 0 rotates: the threshold leaves |u_p . u_q| up to eps, and
// Rinv = Sigma^-1/2 U' L2' carries that into Rinv S Rinv' and Rinv R at full size where an entry's own scale |Rinv| |R| is far below 1
// (late iterates); quadratic convergence makes the extra sweep bring it down to the rounding of the rotations.  Then sigma_j = |g_j|
// and u_j = g_j / sigma_j: orthogonal to eps whatever the size of sigma_j, no pivoting and no deflation decision anywhere.  The same
// (s, z) give the same bits on every run.
//
// Refinement.  (R, Rinv, sigma) so far carry the rounding of the two Cholesky factors, which at cond(S), cond(Z) = 1e3 already moves a
// lambda by tens of eps.  lambda_j^2 = (r_j' Z r_j)(q_j' S q_j) / (q_j' r_j)^2, with q_j = row j of Rinv, is stationary in r_j and in
// q_j (Z r_j = lambda_j q_j, S q_j = lambda_j r_j), so those errors enter it squared; the three sums are evaluated on the float64
// (S, Z) of the call in twice the precision (dot2, four lanes per column), lambda_j is their value rounded, and r_j, q_j are rescaled so
// that r_j' Z r_j = q_j' S q_j = lambda_j and q_j' r_j = 1.  The sort runs on the refined lambda.  So the lambda that is written is
// this refined value, not |g_j|, and the written factors are L1 V Sigma^-1/2 and Sigma^-1/2 U' L2' only up to that rescaling of their
// columns resp. rows; a refined value that is not finite and positive keeps sigma_j and the unscaled pair.  The unsorted R and Rinv' pass through
// the cone's own slots of the resident arrays on the way (all four LDS matrices are operands of the products that form them).
//
// A cone that fails (Cholesky pivot, non-finite input -- it reaches a pivot --, sweep bound, a sigma that is not finite and positive)
// sets the call's fail word and its own word of `bad`, and its R, Rinv, lambda are filled with NaN: no assert, no trap.  The caller's
// k_psd_hs launches skip a cone whose `bad` word is set, so no K entry of it is written.
// Compiled with -ffp-contract=off: a sum of products is rounded product by product, as tests/psd_scaling_reference.py emulates it (the
// fma calls of dot2 are explicit; the emulation gets the same product errors by Dekker's splitting).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cone_layout.h"
#include "cone_reduce.h"
#include "kernels.h"
#include "psd_cone.h"
#include "psd_nt.h"

namespace hipkkt {

namespace {

constexpr int kMaxSweeps = 40;
constexpr double kEps = 2.220446049250313e-16;

// (pos_finite: psd_cone.h; sum8, dot2_step, dot2_step_pair, sum4_pair: psd_nt.h)

}  // namespace

__global__ void __launch_bounds__(256)
k_psd_nt_scaling(const int64_t *__restrict__ tab, const double *__restrict__ s_all, const double *__restrict__ z_all,
                 double *__restrict__ R_all, double *__restrict__ Rinv_all, double *__restrict__ lam_all, int *__restrict__ bad,
                 int *__restrict__ fail, int hi) {
    __shared__ double A[kPsdMatDoubles], B[kPsdMatDoubles], G[kPsdMatDoubles], V[kPsdMatDoubles];      // L1, L2, G -> U Sigma, V
    __shared__ double red[4], sig[kPsdMaxN], lis[kPsdMaxN], red2[kPsdMaxN];
    __shared__ int rank[kPsdMaxN], flag, sigbad;      // flag: Cholesky / sweep bound; sigbad: a sigma that is not finite and positive
    const int c = blockIdx.x, t = threadIdx.x;
    const Cone K = cone_of(tab, c, 1, hi);      // (hi < kPsdMaxN: scaling_psd_large.hip computes the cones above it)
    if (!K.ok) return;
    const int n = K.n, ld = K.ld;
    double *Rg = R_all + K.foff, *Rig = Rinv_all + K.foff, *lamg = lam_all + K.loff;
    if (t == 0) { flag = 0; sigbad = 0; }
    load_svec(A, s_all + K.row0, K);
    load_svec(B, z_all + K.row0, K);
    __syncthreads();

    // ---- the two Cholesky factors, right-looking, lower triangles in place (the diagonal keeps the pivot until the end); entry (i, k)
    // receives a_ik - l_i0 l_k0 - l_i1 l_k1 - ..: the k-sums in ascending order.  Threads 0..127 work on A, 128..255 on B.
    {
        double *Mx = (t >> 7) ? B : A;
        const int tt = t & 127;
        bool ok = true;
        for (int j = 0; j < n; j++) {
            const double d1 = A[j + j * ld], d2 = B[j + j * ld];      // the same values in every thread: the exit is uniform
            if (!pos_finite(d1) || !pos_finite(d2)) { ok = false; break; }
            const double piv = sqrt((t >> 7) ? d2 : d1);
            for (int i = j + 1 + tt; i < n; i += 128) Mx[i + j * ld] = Mx[i + j * ld] / piv;
            __syncthreads();
            {
                const int i = j + 1 + (tt & 63);
                if (i < n) {
                    const double li = Mx[i + j * ld];
                    for (int k = j + 1 + (tt >> 6); k <= i; k += 2) Mx[i + k * ld] = Mx[i + k * ld] - li * Mx[k + j * ld];
                }
            }
            __syncthreads();
        }
        if (!ok && t == 0) flag = 1;
        __syncthreads();
        if (flag == 0 && t < 2 * n) { double *D = t < n ? A : B; const int i = t < n ? t : t - n; D[i + i * ld] = sqrt(D[i + i * ld]); }
        __syncthreads();
    }

    // ---- G = L2' L1, V = I
    if (flag == 0) {
        for (int e = t; e < n * n; e += 256) {
            const int i = e % n, j = e / n;
            double acc = 0.0;
            for (int k = i > j ? i : j; k < n; k++) acc += B[k + i * ld] * A[k + j * ld];
            G[i + j * ld] = acc;
            V[i + j * ld] = i == j ? 1.0 : 0.0;
        }
    }
    __syncthreads();

    // ---- one-sided Jacobi
    if (flag == 0) {
        const int np = n + (n & 1), half = np / 2;
        const int k = t >> 3, l = t & 7;
        bool converged = false;
        for (int sweep = 0; sweep <= kMaxSweeps; sweep++) {
            // after the sweep without a rotation: one polishing sweep, in which every pair with c != 0 rotates (see the head of the file)
            const bool polish = converged;
            if (!polish && sweep == kMaxSweeps) break;
            double nrot = 0.0;
            for (int r = 0; r < np - 1; r++) {
                // pair k of set r: (np - 1, r) for k = 0, ((r + k) mod (np - 1), (r - k) mod (np - 1)) otherwise
                if (k < half) {
                    const int a_ = k == 0 ? np - 1 : (r + k) % (np - 1), b_ = (r + np - 1 - k) % (np - 1);
                    const int p = a_ < b_ ? a_ : b_, q = a_ < b_ ? b_ : a_;
                    if (q < n) {
                        double *gp = G + p * ld, *gq = G + q * ld;
                        double a = 0.0, b = 0.0, cc = 0.0;
                        for (int i = l; i < n; i += 8) {
                            const double x = gp[i], y = gq[i];
                            a += x * x; b += y * y; cc += x * y;
                        }
                        a = sum8(a); b = sum8(b); cc = sum8(cc);
                        if (polish ? cc != 0.0 : fabs(cc) > kEps * sqrt(a * b)) {
                            const double zeta = (b - a) / (2.0 * cc);
                            const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                            const double cs = 1.0 / sqrt(1.0 + tt * tt);
                            const double sn = tt * cs, rr = sn / (1.0 + cs);
                            double *vp = V + p * ld, *vq = V + q * ld;
                            for (int i = l; i < n; i += 8) {
                                const double x = gp[i], y = gq[i];
                                gp[i] = x - sn * (y + rr * x);
                                gq[i] = y + sn * (x - rr * y);
                                const double u = vp[i], w = vq[i];
                                vp[i] = u - sn * (w + rr * u);
                                vq[i] = w + sn * (u - rr * w);
                            }
                            if (l == 0) nrot += 1.0;
                        }
                    }
                }
                __syncthreads();
            }
            if (polish) break;
            nrot = block_sum(nrot, red);
            if (nrot == 0.0) converged = true;
        }
        if (!converged && t == 0) flag = 1;      // (the same in every thread: block_sum; thread 0 records it)
    }
    __syncthreads();

    // ---- sigma_j = |g_j|, lisqrt_j = 1 / sqrt(sigma_j)
    if (flag == 0) {
        const int l = t & 7;
        for (int j = t >> 3; j < n; j += 32) {
            const double *gj = G + j * ld;
            double a = 0.0;
            for (int i = l; i < n; i += 8) a += gj[i] * gj[i];
            a = sum8(a);
            if (l == 0) {
                const double sg = sqrt(a);
                sig[j] = sg;
                lis[j] = 1.0 / sqrt(sg);
                if (!pos_finite(sg)) sigbad = 1;      // (its own word: flag is only read in this phase)
            }
        }
    }
    __syncthreads();
    if (flag != 0 || sigbad != 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int e = t; e < n * n; e += 256) { Rg[e] = nan; Rig[e] = nan; }
        if (t < n) lamg[t] = nan;
        if (t == 0) { bad[c] = 1; atomicOr(fail, 1); }
        return;
    }
    if (t == 0) bad[c] = 0;

    // ---- R = (L1 V) lisqrt and row j of Rinv = (lisqrt_j / sigma_j) g_j' L2', not sorted yet, through the cone's own slots of the
    // resident arrays (the four LDS matrices are all operands here; the barrier orders the workgroup's global stores and loads)
    for (int e = t; e < n * n; e += 256) {
        const int i = e % n, j = e / n;
        double acc = 0.0;
        for (int k = 0; k <= i; k++) acc += A[i + k * ld] * V[k + j * ld];
        Rg[e] = acc * lis[j];
    }
    for (int e = t; e < n * n; e += 256) {
        const int j = e % n, i = e / n;
        double acc = 0.0;
        for (int k = 0; k <= i; k++) acc += G[k + j * ld] * B[i + k * ld];
        Rig[i + j * n] = acc * (lis[j] / sig[j]);      // (column j of this staging copy = row j of Rinv)
    }
    __syncthreads();
    load_svec(A, s_all + K.row0, K);                   // A = S, B = Z again, G = R, V = Rinv'
    load_svec(B, z_all + K.row0, K);
    for (int e = t; e < n * n; e += 256) { const int i = e % n, j = e / n; G[i + j * ld] = Rg[e]; V[i + j * ld] = Rig[e]; }
    __syncthreads();

    // ---- the refinement of lambda: lambda_j^2 = (r_j' Z r_j)(q_j' S q_j) / (q_j' r_j)^2 is stationary in r_j and in q_j (row j of
    // Rinv), so the rounding of the factors enters it squared; the three sums run in twice the precision (dot2).  Four lanes per
    // column, lane l the rows l, l + 4, ..  Then r_j and q_j are rescaled so that r_j' Z r_j = q_j' S q_j = lambda_j and q_j' r_j = 1.
    {
        const int j = t >> 2, l = t & 3;
        double lamj = 0.0, fa = 1.0, fb = 1.0;
        if (j < n) {
            const double *rj = G + j * ld, *qj = V + j * ld;
            double h1 = 0.0, l1 = 0.0, h2 = 0.0, l2 = 0.0, h3 = 0.0, l3 = 0.0;
            for (int i = l; i < n; i += 4) {
                double yh = 0.0, yl = 0.0, wh = 0.0, wl = 0.0;      // y = (Z r_j)_i, w = (S q_j)_i
                for (int k = 0; k < n; k++) dot2_step(B[i + k * ld], rj[k], yh, yl);
                for (int k = 0; k < n; k++) dot2_step(A[i + k * ld], qj[k], wh, wl);
                dot2_step_pair(rj[i], yh, yl, h1, l1);
                dot2_step_pair(qj[i], wh, wl, h2, l2);
                dot2_step(qj[i], rj[i], h3, l3);
            }
            sum4_pair(h1, l1); sum4_pair(h2, l2); sum4_pair(h3, l3);
            // sqrt of the product of two pairs, then the division by the third
            double p = h1 * h2, e = fma(h1, h2, -p);
            e = e + (h1 * l2 + l1 * h2);
            const double x0 = sqrt(p);
            const double x = x0 + (fma(-x0, x0, p) + e) / (2.0 * x0);
            double v = x / h3;
            v = v - v * (l3 / h3);
            lamj = sig[j];
            if (pos_finite(v) && pos_finite(h1) && pos_finite(h2)) { lamj = v; fa = sqrt(v / h1); fb = sqrt(v / h2); }
        }
        __syncthreads();      // (every read of sig[] above is done)
        if (j < n && l == 0) { sig[j] = lamj; lis[j] = fa; red2[j] = fb; }
    }
    __syncthreads();
    // ---- the descending order by counting (ties by index: a bijection), the outputs to their sorted positions
    if (t < n) {
        const double sj = sig[t];
        int rk = 0;
        for (int i = 0; i < n; i++) rk += (sig[i] > sj || (sig[i] == sj && i < t)) ? 1 : 0;
        rank[t] = rk;
        lamg[rk] = sj;
    }
    __syncthreads();
    for (int e = t; e < n * n; e += 256) {
        const int i = e % n, j = e / n;
        Rg[i + rank[j] * n] = G[i + j * ld] * lis[j];
        Rig[rank[j] + i * n] = V[i + j * ld] * red2[j];
    }
}

void launch_psd_nt_scaling(hipStream_t st, int npsd, const int64_t *tab, const double *s, const double *z, double *R, double *Rinv,
                           double *lam, int *bad, int *fail, int max_side) {
    const int hi = max_side < kPsdMaxN ? max_side : kPsdMaxN;
    if (npsd > 0) hipLaunchKernelGGL(k_psd_nt_scaling, dim3(npsd), dim3(256), 0, st, tab, s, z, R, Rinv, lam, bad, fail, hi);
}

}  // namespace hipkkt
