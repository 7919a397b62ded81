// What the two Nesterov-Todd scaling kernels of the PSD triangle cones share (scaling_psd.hip: sides <= 64, everything in LDS;
// scaling_psd_large.hip: sides up to 128, one matrix in LDS): the eight-lane sum of a column pair of the one-sided Jacobi iteration
// and the dot2 steps of the refinement.  One definition each: both files are compiled with -ffp-contract=off and
// tests/psd_scaling_reference.py emulates the rounding order of these expressions, so both kernels round alike.
#pragma once
#include <hip/hip_runtime.h>

namespace hipkkt {

constexpr double kPsdNtEps = 2.220446049250313e-16;

// the sum over the eight lanes of a pair (lanes 8 k .. 8 k + 7 of one wavefront); every lane gets the same bits
__device__ __forceinline__ double sum8(double v) {
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

// dot2 (Ogita, Rump, Oishi): (h, l) += a b with the product's and the sum's rounding errors kept in l; h + l is the sum as if
// accumulated in twice the precision.  fma is explicit, so -ffp-contract=off leaves it alone.
__device__ __forceinline__ void dot2_step(double a, double b, double &h, double &l) {
    const double p = a * b, e = fma(a, b, -p);
    const double s = h + p, bb = s - h;
    l = l + (((h - (s - bb)) + (p - bb)) + e);
    h = s;
}
// the same for a (b + bl)
__device__ __forceinline__ void dot2_step_pair(double a, double b, double bl, double &h, double &l) {
    const double p = a * b, e = fma(a, b, -p);
    const double s = h + p, bb = s - h;
    l = l + ((((h - (s - bb)) + (p - bb)) + e) + a * bl);
    h = s;
}
// the sum of the pairs of four neighbouring lanes, normalised (h = the rounded sum); every lane gets the same bits
__device__ __forceinline__ void sum4_pair(double &h, double &l) {
    for (int o = 2; o > 0; o >>= 1) {
        const double h2 = __shfl_xor(h, o), l2 = __shfl_xor(l, o);
        const double s = h + h2, bb = s - h;
        l = (l + l2) + ((h - (s - bb)) + (h2 - bb));
        h = s;
    }
    const double hn = h + l;
    l = l - (hn - h);
    h = hn;
}

}  // namespace hipkkt
