// The cone algebra of one interior-point step for Zero, Nonnegative and SecondOrder cones on the device: what the caller's host loop
// does between the KKT solves (variables.jl:14-43, :107-162, kktsystem.jl:135-215), on the (s, z, w, lambda, eta) that the last
// successful hipkkt_update_scaling[_dev] left resident.
//   affine_ds            lambda o lambda                      coneops_nncone.jl affine_ds!, coneops_socone.jl:219-228 (circ_op :364-378)
//   combined_ds_shift    W^-1 ds o W dz - sigma mu e          coneops_symmetric_common.jl:1-36 with mul_W! / mul_Winv! (coneops_socone.jl:300-347)
//   ds_from_dz_offset    ds ./ z resp. coneops_socone.jl:241-268
//   mul_Hs               w^2 x resp. coneops_socone.jl:201-216
//   step_length          coneops_nncone.jl:151-170, coneops_socone.jl:270-286 with _step_length_soc_component (:443-512);
//                        the minimum over cones is exact, so the order of evaluation does not matter (coneops_compositecone.jl:216-252)
//   add_step             v += alpha dv                         variables.jl variables_add_step!
//   info_norms           the eight scaled 2-norms of info_update!, info.jl:1-60
// One thread per Zero / Nonnegative row, one workgroup per second-order cone (the tables of scaling.hip: row_kind, desc).  Expressions keep
// the reference's association and this file is compiled with -ffp-contract=off, so every row-wise result is the host's bit for bit;
// a `dot` of the reference is a tree sum (block_sum).  Inputs are never written: what the reference keeps in step_z / step_s as
// scratch is recomputed per element here.  No assert, no trap, every loop is bounded by a cone's dimension.
// Everything is HBM / latency bound: a few m doubles per operation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cone_layout.h"
#include "cone_reduce.h"
#include "kernels.h"

namespace hipkkt {

namespace {

constexpr double kFloatMax = 1.7976931348623157e308;

// dot(a[1:], b[1:]) over one cone
__device__ __forceinline__ double tail_dot(const double *a, const double *b, int64_t dim, double *red) {
    double acc = 0.0;
    for (int64_t i = 1 + threadIdx.x; i < dim; i += 256) acc += a[i] * b[i];
    return block_sum(acc, red);
}
// _soc_residual, coneops_socone.jl:395-399: (z0 - |z1|)(z0 + |z1|)
__device__ __forceinline__ double soc_residual(const double *z, int64_t dim, double *red) {
    const double z1 = sqrt(tail_dot(z, z, dim, red));
    return (z[0] - z1) * (z[0] + z1);
}

}  // namespace

// ---- affine_ds --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_step_affine_ds_diag(const signed char *__restrict__ row_kind, const double *__restrict__ lam, double *__restrict__ out, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int kind = row_kind[i];
    if (kind == 0) out[i] = 0.0;
    else if (kind == 1) out[i] = lam[i] * lam[i];
}
__global__ void __launch_bounds__(256)
k_step_affine_ds_soc(const int64_t *__restrict__ desc, const double *__restrict__ lam_all, double *__restrict__ out_all) {
    __shared__ double red[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int64_t row0 = desc[kSocDesc * c + kSocRow0], dim = desc[kSocDesc * c + kSocDim];
    const double *lam = lam_all + row0;
    double *out = out_all + row0;
    double acc = 0.0;
    for (int64_t i = t; i < dim; i += 256) acc += lam[i] * lam[i];
    const double x0 = block_sum(acc, red);
    const double l0 = lam[0];
    for (int64_t i = 1 + t; i < dim; i += 256) out[i] = l0 * lam[i] + l0 * lam[i];
    if (t == 0) out[0] = x0;
}

// ---- combined_ds_shift ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_step_shift_diag(const signed char *__restrict__ row_kind, const double *__restrict__ w, const double *__restrict__ dz,
                  const double *__restrict__ ds, double sigma_mu, double *__restrict__ out, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int kind = row_kind[i];
    if (kind == 0) out[i] = 0.0;
    else if (kind == 1) out[i] = (ds[i] / w[i]) * (dz[i] * w[i]) + (-sigma_mu);
}
__global__ void __launch_bounds__(256)
k_step_shift_soc(const int64_t *__restrict__ desc, const double *__restrict__ w_all, const double *__restrict__ eta_all,
                 const double *__restrict__ dz_all, const double *__restrict__ ds_all, double sigma_mu, double *__restrict__ out_all) {
    __shared__ double red[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int64_t row0 = desc[kSocDesc * c + kSocRow0], dim = desc[kSocDesc * c + kSocDim];
    const double *w = w_all + row0, *dz = dz_all + row0, *ds = ds_all + row0;
    double *out = out_all + row0;
    const double eta = eta_all[c], etainv = 1.0 / eta, w0 = w[0];
    // zW = W dz (mul_W!), sW = W^-1 ds (mul_Winv!)
    const double zeta_z = tail_dot(w, dz, dim, red), zeta_s = tail_dot(w, ds, dim, red);
    const double cz = dz[0] + zeta_z / (1.0 + w0), cs = -ds[0] + zeta_s / (1.0 + w0);
    const double zW0 = eta * (w0 * dz[0] + zeta_z), sW0 = etainv * (w0 * ds[0] - zeta_s);
    // shift = sW o zW (circ_op!), then shift[0] -= sigma mu (scaled_unit_shift!)
    double acc = 0.0;
    for (int64_t i = t; i < dim; i += 256) {
        const double zWi = i == 0 ? zW0 : eta * (dz[i] + cz * w[i]);
        const double sWi = i == 0 ? sW0 : etainv * (ds[i] + cs * w[i]);
        acc += sWi * zWi;
        if (i > 0) out[i] = sW0 * zWi + zW0 * sWi;
    }
    const double x0 = block_sum(acc, red);
    if (t == 0) out[0] = x0 + (-sigma_mu);
}

// ---- ds_from_dz_offset ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_step_offset_diag(const signed char *__restrict__ row_kind, const double *__restrict__ z, const double *__restrict__ ds,
                   double *__restrict__ out, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int kind = row_kind[i];
    if (kind == 0) out[i] = 0.0;
    else if (kind == 1) out[i] = ds[i] / z[i];
}
__global__ void __launch_bounds__(256)
k_step_offset_soc(const int64_t *__restrict__ desc, const double *__restrict__ z_all, const double *__restrict__ w_all,
                  const double *__restrict__ lam_all, const double *__restrict__ eta_all, const double *__restrict__ ds_all,
                  double *__restrict__ out_all) {
    __shared__ double red[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int64_t row0 = desc[kSocDesc * c + kSocRow0], dim = desc[kSocDesc * c + kSocDim];
    const double *z = z_all + row0, *w = w_all + row0, *lam = lam_all + row0, *ds = ds_all + row0;
    double *out = out_all + row0;
    const double eta = eta_all[c];
    const double resz = soc_residual(z, dim, red);
    const double l1ds1 = tail_dot(lam, ds, dim, red), w1ds1 = tail_dot(w, ds, dim, red);
    const double cc = lam[0] * ds[0] - l1ds1;
    const double f = cc / resz, g = w1ds1 / (1.0 + w[0]), linv = 1.0 / lam[0];
    for (int64_t i = t; i < dim; i += 256) {
        double o = i == 0 ? z[0] : -z[i];
        o *= f;
        if (i == 0) o += eta * w1ds1; else o += eta * (ds[i] + g * w[i]);
        out[i] = o * linv;
    }
}

// ---- mul_Hs; with addc != NULL: y = -(Hs x + addc), the ds of kktsystem.jl:203-207 -----------------------------------------------------
__global__ void __launch_bounds__(256)
k_step_mulhs_diag(const signed char *__restrict__ row_kind, const double *__restrict__ w, const double *__restrict__ x,
                  const double *__restrict__ addc, double *__restrict__ y, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int kind = row_kind[i];
    if (kind != 0 && kind != 1) return;
    double v = kind == 0 ? 0.0 : w[i] * (w[i] * x[i]);
    if (addc) v = -(v + addc[i]);
    y[i] = v;
}
__global__ void __launch_bounds__(256)
k_step_mulhs_soc(const int64_t *__restrict__ desc, const double *__restrict__ w_all, const double *__restrict__ eta_all,
                 const double *__restrict__ x_all, const double *__restrict__ addc_all, double *__restrict__ y_all) {
    __shared__ double red[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int64_t row0 = desc[kSocDesc * c + kSocRow0], dim = desc[kSocDesc * c + kSocDim];
    const double *w = w_all + row0, *x = x_all + row0;
    double *y = y_all + row0;
    const double eta2 = eta_all[c] * eta_all[c];
    double acc = 0.0;
    for (int64_t i = t; i < dim; i += 256) acc += w[i] * x[i];
    const double cc = 2.0 * block_sum(acc, red);
    for (int64_t i = t; i < dim; i += 256) {
        double v = i == 0 ? -x[0] : x[i];
        v += cc * w[i];
        v *= eta2;
        if (addc_all) v = -(v + addc_all[row0 + i]);
        y[i] = v;
    }
}

// ---- step_length -------------------------------------------------------------------------------------------------------------------
// part = (alpha_z, alpha_s) pairs: one per workgroup of the row kernel, then one per second-order cone
__global__ void __launch_bounds__(256)
k_step_len_diag(const signed char *__restrict__ row_kind, const double *__restrict__ z, const double *__restrict__ s,
                const double *__restrict__ dz, const double *__restrict__ ds, double alpha_max, double *__restrict__ part, int64_t m) {
    __shared__ double red[4];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double az = alpha_max, as = alpha_max;
    if (i < m && row_kind[i] == 1) {
        if (dz[i] < 0.0) az = fmin(az, -z[i] / dz[i]);
        if (ds[i] < 0.0) as = fmin(as, -s[i] / ds[i]);
    }
    az = block_min(az, red);
    as = block_min(as, red);
    if (threadIdx.x == 0) { part[2 * (int64_t)blockIdx.x] = az; part[2 * (int64_t)blockIdx.x + 1] = as; }
}
// _step_length_soc_component, coneops_socone.jl:443-512; uniform over the workgroup
__device__ double soc_step_component(const double *x, const double *y, int64_t dim, double alpha_max, double *red) {
    if (x[0] >= 0.0 && y[0] < 0.0) alpha_max = fmin(alpha_max, -x[0] / y[0]);
    const double a = soc_residual(y, dim, red);
    const double b = 2.0 * (x[0] * y[0] - tail_dot(x, y, dim, red));
    const double c = fmax(0.0, soc_residual(x, dim, red));
    const double d = b * b - 4.0 * a * c;
    if ((a > 0.0 && b > 0.0) || d < 0.0) return alpha_max;
    if (a == 0.0) return alpha_max;
    if (c == 0.0) return a >= 0.0 ? alpha_max : 0.0;
    const double t = b >= 0.0 ? (-b - sqrt(d)) : (-b + sqrt(d));
    double r1 = (2.0 * c) / t, r2 = t / (2.0 * a);
    if (r1 < 0.0) r1 = kFloatMax;
    if (r2 < 0.0) r2 = kFloatMax;
    return fmin(alpha_max, fmin(r1, r2));
}
__global__ void __launch_bounds__(256)
k_step_len_soc(const int64_t *__restrict__ desc, const double *__restrict__ z_all, const double *__restrict__ s_all,
               const double *__restrict__ dz_all, const double *__restrict__ ds_all, double alpha_max, double *__restrict__ part) {
    __shared__ double red[4];
    const int c = blockIdx.x;
    const int64_t row0 = desc[kSocDesc * c + kSocRow0], dim = desc[kSocDesc * c + kSocDim];
    const double az = soc_step_component(z_all + row0, dz_all + row0, dim, alpha_max, red);
    const double as = soc_step_component(s_all + row0, ds_all + row0, dim, alpha_max, red);
    if (threadIdx.x == 0) { part[2 * c] = az; part[2 * c + 1] = as; }
}
__global__ void __launch_bounds__(256)
k_step_len_final(const double *__restrict__ part, int64_t npairs, double alpha_max, double *__restrict__ out2) {
    __shared__ double red[4];
    double az = alpha_max, as = alpha_max;
    for (int64_t k = threadIdx.x; k < npairs; k += 256) { az = fmin(az, part[2 * k]); as = fmin(as, part[2 * k + 1]); }
    az = block_min(az, red);
    as = block_min(as, red);
    if (threadIdx.x == 0) { out2[0] = az; out2[1] = as; }
}

// ---- row-wise helpers of the fused calls ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_step_add_step(double *__restrict__ v, const double *__restrict__ dv, double alpha, int64_t len) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < len) v[i] = v[i] + alpha * dv[i];
}
__global__ void __launch_bounds__(256)
k_step_scale(double *__restrict__ out, const double *__restrict__ in, double f, int64_t len) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < len) out[i] = in[i] * f;
}
__global__ void __launch_bounds__(256)
k_step_add(double *__restrict__ acc, const double *__restrict__ b, int64_t len) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < len) acc[i] = acc[i] + b[i];
}
// in = [rhs.x | workz | variables.x] of the reduced solve.  affine (dsc == NULL): rhs.x = rx, workz = s - rz (variables.jl:107-121,
// kktsystem.jl:152-163); combined: rhs.x = f rx, workz = dsc - f rz with f = 1 - sigma (variables.jl:124-162)
__global__ void __launch_bounds__(256)
k_step_rhs(double *__restrict__ in, const double *__restrict__ xzs, const double *__restrict__ res, const double *__restrict__ dsc,
           double f, int64_t n, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        in[i] = dsc ? f * res[i] : res[i];
        in[n + m + i] = xzs[i];
    }
    if (i < m) in[n + i] = dsc ? dsc[i] - f * res[n + i] : xzs[n + m + i] - res[n + i];
}

// ---- info_norms ---------------------------------------------------------------------------------------------------------------------
// term k: sum over i of (a_k[i] b_k[i])^2 in kNormBlocks fixed slices, then summed in a fixed order: deterministic
constexpr int kNormBlocks = 64;
struct NormTerms { const double *a[8], *b[8]; int64_t len[8]; };
__global__ void __launch_bounds__(256)
k_step_norm_part(NormTerms T, double *__restrict__ part) {
    __shared__ double red[4];
    const int k = blockIdx.y;
    const double *a = T.a[k], *b = T.b[k];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T.len[k]; i += (int64_t)kNormBlocks * 256) {
        const double v = a[i] * b[i];
        acc += v * v;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) part[k * kNormBlocks + blockIdx.x] = acc;
}
__global__ void __launch_bounds__(64)
k_step_norm_final(const double *__restrict__ part, double *__restrict__ out8) {
    const int k = threadIdx.x;
    if (k >= 8) return;
    double acc = 0.0;
    for (int j = 0; j < kNormBlocks; j++) acc += part[k * kNormBlocks + j];
    out8[k] = sqrt(acc);
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
static inline dim3 rows_grid(int64_t len) { return dim3((unsigned)((len + 255) / 256)); }

int64_t step_len_pairs(int64_t m, int nsoc) { return (m + 255) / 256 + nsoc; }
int64_t step_norm_part_doubles() { return 8 * kNormBlocks; }

void launch_step_affine_ds(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, const double *lam, double *out,
                           int64_t m) {
    if (m > 0) hipLaunchKernelGGL(k_step_affine_ds_diag, rows_grid(m), dim3(256), 0, st, row_kind, lam, out, m);
    if (nsoc > 0) hipLaunchKernelGGL(k_step_affine_ds_soc, dim3(nsoc), dim3(256), 0, st, desc, lam, out);
}
void launch_step_shift(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, const double *w, const double *eta,
                       const double *dz, const double *ds, double sigma_mu, double *out, int64_t m) {
    if (m > 0) hipLaunchKernelGGL(k_step_shift_diag, rows_grid(m), dim3(256), 0, st, row_kind, w, dz, ds, sigma_mu, out, m);
    if (nsoc > 0) hipLaunchKernelGGL(k_step_shift_soc, dim3(nsoc), dim3(256), 0, st, desc, w, eta, dz, ds, sigma_mu, out);
}
void launch_step_offset(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, const double *z, const double *w,
                        const double *lam, const double *eta, const double *ds, double *out, int64_t m) {
    if (m > 0) hipLaunchKernelGGL(k_step_offset_diag, rows_grid(m), dim3(256), 0, st, row_kind, z, ds, out, m);
    if (nsoc > 0) hipLaunchKernelGGL(k_step_offset_soc, dim3(nsoc), dim3(256), 0, st, desc, z, w, lam, eta, ds, out);
}
void launch_step_mulhs(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, const double *w, const double *eta,
                       const double *x, const double *addc, double *y, int64_t m) {
    if (m > 0) hipLaunchKernelGGL(k_step_mulhs_diag, rows_grid(m), dim3(256), 0, st, row_kind, w, x, addc, y, m);
    if (nsoc > 0) hipLaunchKernelGGL(k_step_mulhs_soc, dim3(nsoc), dim3(256), 0, st, desc, w, eta, x, addc, y);
}
// part: 2 * step_len_pairs(m, nsoc) doubles
void launch_step_length(hipStream_t st, const signed char *row_kind, int nsoc, const int64_t *desc, const double *z, const double *s,
                        const double *dz, const double *ds, double alpha_max, double *part, double *out2, int64_t m) {
    const int64_t nblk = (m + 255) / 256;
    if (m > 0) hipLaunchKernelGGL(k_step_len_diag, rows_grid(m), dim3(256), 0, st, row_kind, z, s, dz, ds, alpha_max, part, m);
    if (nsoc > 0) hipLaunchKernelGGL(k_step_len_soc, dim3(nsoc), dim3(256), 0, st, desc, z, s, dz, ds, alpha_max, part + 2 * nblk);
    hipLaunchKernelGGL(k_step_len_final, dim3(1), dim3(256), 0, st, part, nblk + nsoc, alpha_max, out2);
}
void launch_step_add_step(hipStream_t st, double *v, const double *dv, double alpha, int64_t len) {
    if (len > 0) hipLaunchKernelGGL(k_step_add_step, rows_grid(len), dim3(256), 0, st, v, dv, alpha, len);
}
void launch_step_scale(hipStream_t st, double *out, const double *in, double f, int64_t len) {
    if (len > 0) hipLaunchKernelGGL(k_step_scale, rows_grid(len), dim3(256), 0, st, out, in, f, len);
}
void launch_step_add(hipStream_t st, double *acc, const double *b, int64_t len) {
    if (len > 0) hipLaunchKernelGGL(k_step_add, rows_grid(len), dim3(256), 0, st, acc, b, len);
}
void launch_step_rhs(hipStream_t st, double *in, const double *xzs, const double *res, const double *dsc, double f, int64_t n, int64_t m) {
    const int64_t len = n > m ? n : m;
    if (len > 0) hipLaunchKernelGGL(k_step_rhs, rows_grid(len), dim3(256), 0, st, in, xzs, res, dsc, f, n, m);
}
// eq = [d (n) | e (m) | dinv (n) | einv (m)]; out8 = |d x|, |e z|, |einv s|, |dinv rx|, |einv rz|, |dinv rx_inf|, |einv rz_inf|, |dinv Px|
void launch_step_info_norms(hipStream_t st, const double *xzs, const double *res, const double *eq, double *part, double *out8, int64_t n,
                            int64_t m) {
    const double *d = eq, *e = eq + n, *dinv = e + m, *einv = dinv + n;
    NormTerms T;
    const double *a[8] = {d, e, einv, dinv, einv, dinv, einv, dinv};
    const double *b[8] = {xzs, xzs + n, xzs + n + m, res, res + n, res + n + m, res + 2 * n + m, res + 2 * n + 2 * m};
    const int64_t len[8] = {n, m, m, n, m, n, m, n};
    for (int k = 0; k < 8; k++) { T.a[k] = a[k]; T.b[k] = b[k]; T.len[k] = len[k]; }
    hipLaunchKernelGGL(k_step_norm_part, dim3(kNormBlocks, 8), dim3(256), 0, st, T, part);
    hipLaunchKernelGGL(k_step_norm_final, dim3(1), dim3(64), 0, st, part, out8);
}

}  // namespace hipkkt
