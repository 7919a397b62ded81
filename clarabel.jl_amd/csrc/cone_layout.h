// Record layouts shared by the host encoder of the cone tables (hipkkt_cones.cpp, hipkkt_step.cpp) and the kernels that read them
// (scaling.hip, step.hip, step_cone3.hip, step_genpow.hip, step_psd.hip).  Plain C++: the host files include it as well.
// The strides and field indices are `int`, so that an index expression keeps the type it has always had.
#pragma once
#include <stdint.h>

namespace hipkkt {

// second-order cone descriptor (int64): first row, dim, first Hs entry, offset into the concatenated (u, v) of the sparse cones or -1 for
// a dense (dim <= 4) block, ordinal among the sparse cones or -1
constexpr int kSocDesc = 5;
constexpr int kSocRow0 = 0, kSocDim = 1, kSocHs0 = 2, kSocUv0 = 3, kSocOrd = 4;

// Generalized Power cone descriptor (int64): first row, dim1, dim2, first Hs entry, offset of the cone's slot in the output vector, offset
// of its exponents, offset of its index table [map.q (dim1) | map.r (dim2) | map.p (dim) | map.D (3)], the bits of psi = 1 / <alpha, alpha>
constexpr int kGpDesc = 8;
constexpr int kGpRow0 = 0, kGpDim1 = 1, kGpDim2 = 2, kGpHs0 = 3, kGpOut0 = 4, kGpAlpha0 = 5, kGpIdx0 = 6, kGpPsiBits = 7;

// PSD triangle cone table of the step (int64): first row, side n, offset of the n x n factors, offset of lambda
constexpr int kPsdTab = 4;
constexpr int kPsdRow0 = 0, kPsdN = 1, kPsdFactor0 = 2, kPsdLambda0 = 3;

// slot of a three-row cone (Exponential / Power) in the scaling's output vector: pack_triu(Hs) | pack_triu(H_dual) | grad
constexpr int kSlot3 = 15;
constexpr int kSlot3Hs = 0, kSlot3Hdual = 6, kSlot3Grad = 12;

// slot of a Generalized Power cone in the same vector: grad (dim) | d1 (dim1) | d2 (1) | p (dim) | q (dim1) | r (dim2), dim = dim1 + dim2
struct GpSlot { int64_t grad, d1, d2, p, q, r, len; };
constexpr GpSlot gp_slot(int64_t dim1, int64_t dim2) {
    const int64_t dim = dim1 + dim2;
    return GpSlot{0, dim, dim + dim1, dim + dim1 + 1, 2 * dim + dim1 + 1, 2 * dim + 2 * dim1 + 1, 3 * dim + dim1 + 1};
}

// the result buffer of the step entry points (doubles)
constexpr int kStOutSym = 0;        // (alpha_z, alpha_s) of the symmetric rows, from which the non-symmetric cones' line search starts
constexpr int kStOutLen = 2;        // the composite (alpha, alpha) of a set with non-symmetric cones
constexpr int kStOutNorms = 4;      // the eight norms of hipkkt_step_info_norms_dev
constexpr int kStOutBarrier = 12;   // up to 8 (barrier, shifted dot) pairs of hipkkt_step_barrier_dev
constexpr int kStOutSymPsd = 28;    // the symmetric rows' pair next to PSD cones
constexpr int kStOutDoubles = 32;

}  // namespace hipkkt
