// Value updates on the resident KKT image (K1-K2; HBM / latency bound): k_scatter_values / k_scale_values / k_soc_batch, the Hs
// block of a PSD triangle cone (k_psd_hs), and k_zero_words for the flag and scalar words of the captured graphs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernel_util.h"
#include "kernels.h"

namespace hipkkt {

// ------------------------------------------------------------------------------------------
// K1/K2: value updates on the resident KKT image (ref: kktsolver_directldl.jl:130-188)
// ------------------------------------------------------------------------------------------
__global__ void k_scatter_values(double *__restrict__ kval, const int64_t *__restrict__ idx,
                                 const double *__restrict__ vals, int64_t n, double scale) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) kval[idx[i]] = vals[i] * scale;
}

__global__ void k_scale_values(double *__restrict__ kval, const int64_t *__restrict__ idx, int64_t n,
                               double scale) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) kval[idx[i]] *= scale;
}

// all sparse SOC cones in one launch (ref: _csc_update_sparsecone, directldl_datamaps.jl:61-79):
// K[u_idx] = u * (-eta^2), K[v_idx] = v * (-eta^2), K[D_idx] = (-eta^2, +eta^2)
__global__ void k_soc_batch(double *__restrict__ kval, const int64_t *__restrict__ uidx, const int64_t *__restrict__ vidx,
                            const int *__restrict__ cone_of, const double *__restrict__ u, const double *__restrict__ v,
                            const double *__restrict__ eta2, int64_t n, const int64_t *__restrict__ didx, int nsoc) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const double sc = -eta2[cone_of[i]];
        kval[uidx[i]] = u[i] * sc;
        kval[vidx[i]] = v[i] * sc;
    }
    if (i < nsoc) {
        kval[didx[2 * i]] = -eta2[i];
        kval[didx[2 * i + 1]] = eta2[i];
    }
}

void launch_scatter_values(hipStream_t st, double *kval, const int64_t *idx, const double *vals, int64_t n, double scale) {
    if (n > 0) hipLaunchKernelGGL(k_scatter_values, dim3(nblk(n)), dim3(256), 0, st, kval, idx, vals, n, scale);
}
void launch_scale_values(hipStream_t st, double *kval, const int64_t *idx, int64_t n, double scale) {
    if (n > 0) hipLaunchKernelGGL(k_scale_values, dim3(nblk(n)), dim3(256), 0, st, kval, idx, n, scale);
}
void launch_soc_batch(hipStream_t st, double *kval, const int64_t *uidx, const int64_t *vidx, const int *cone_of,
                      const double *u, const double *v, const double *eta2, int64_t n, const int64_t *didx, int nsoc) {
    int64_t m = n > nsoc ? n : nsoc;
    if (m > 0)
        hipLaunchKernelGGL(k_soc_batch, dim3(nblk(m)), dim3(256), 0, st, kval, uidx, vidx, cone_of, u, v, eta2, n, didx, nsoc);
}
// zero a few 32-bit words.  Small hipMemsetAsync nodes inside a captured hipGraph are not reliable in every ROCm
// set-up (under rocprofv3 the 16-byte memset of the flag words was seen to write its own arguments instead of
// zeros; under PyTorch's bundled runtime a 56-byte one was seen to do nothing), so the factor / solve graphs
// clear their flag and scalar words with this kernel.
__global__ void k_zero_words(int *p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}
// Hs block of one PSD triangle cone on the device: entry e of the packed (column-major) upper triangle of
// W (x)_s W, e <-> (a <= b), a <-> (i <= j), b <-> (k <= l) in the svec ordering.  The four cases of the reference's
// skron! (coneops_psdtrianglecone.jl:502-540), with its products, association and rounding:
//   i != j, k != l :  W_ik W_jl + W_il W_jk          i == j, k != l :  (sqrt2 W_jl) W_jk
//   i != j, k == l :  (sqrt2 W_il) W_jk               i == j, k == l :  W_jl W_jl
// Explicitly rounded products and sums (no FMA contraction).  The value is negated and scattered through
// map.Hsblocks (kktsolver_directldl.jl:225-228).
__device__ __forceinline__ long long tri_root(long long e) {   // largest t with t(t+1)/2 <= e
    long long t = (long long)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while (t * (t + 1) / 2 > e) t--;
    while ((t + 1) * (t + 2) / 2 <= e) t++;
    return t;
}
__global__ void __launch_bounds__(256)
k_psd_hs(double *__restrict__ kval, const int64_t *__restrict__ map_hs, int64_t hs_off, const double *__restrict__ W, int n,
         int64_t nent, const int *__restrict__ skip) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nent || (skip && *skip != 0)) return;
    const long long b = tri_root(e), a = e - b * (b + 1) / 2;
    const long long j = tri_root(a), i = a - j * (j + 1) / 2;
    const long long l = tri_root(b), k = b - l * (l + 1) / 2;
    const double sqrt2 = sqrt(2.0);
    double v;
    if (i != j && k != l) {
        // products and the sum are rounded one by one like the reference's loop: HIP's `*` followed by `+` is contracted
        // into an FMA by the compiler, so the products pass through an opaque asm before they are added
        double p1 = W[i * n + k] * W[j * n + l];
        double p2 = W[i * n + l] * W[j * n + k];
        asm volatile("" : "+v"(p1), "+v"(p2));
        v = p1 + p2;
    } else if (i == j && k != l) {
        v = (sqrt2 * W[j * n + l]) * W[j * n + k];
    } else if (i != j) {
        v = (sqrt2 * W[i * n + l]) * W[j * n + k];
    } else {
        v = W[j * n + l] * W[j * n + l];
    }
    kval[map_hs[hs_off + e]] = -v;
}
void launch_psd_hs(hipStream_t st, double *kval, const int64_t *map_hs, int64_t hs_off, const double *W, int n, const int *skip) {
    const int64_t numel = (int64_t)n * (n + 1) / 2, nent = numel * (numel + 1) / 2;
    if (nent > 0) hipLaunchKernelGGL(k_psd_hs, dim3(nblk(nent)), dim3(256), 0, st, kval, map_hs, hs_off, W, n, nent, skip);
}
void launch_zero_words(hipStream_t st, void *p, int nwords) {
    if (nwords > 0) hipLaunchKernelGGL(k_zero_words, dim3(nblk(nwords, 64)), dim3(64), 0, st, (int *)p, nwords);
}

}  // namespace hipkkt
