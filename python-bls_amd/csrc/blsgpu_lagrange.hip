// blsgpu_lagrange.hip -- batched Lagrange coefficients at zero over the scalar field (Threshold.lagrange_coeffs_at_zero,
// threshold.py:56-88 of the reference) and the sums sum_j L_j y_j behind interpolate_at_zero (threshold.py:91-101), on the
// arithmetic of fr_scalar.h (included by blsgpu_api.hip, built with blsgpu_g1fix.hip in translation unit 8).
//
// A call holds `groups` groups of k evaluation points, one k per call; one point per LANE.  Lanes are the flat (group, j)
// indices of a workgroup: up to 256 points a workgroup of 256 threads holds 256 / k WHOLE groups (k = 67: three groups on
// 201 of 256 lanes), above that one group on k lanes rounded up to whole wavefronts -- which is the limit on k: a group
// has to fit one workgroup of 1024 threads (BLSGPU_LAGRANGE_MAX_K).  A workgroup's points lie in LDS in Montgomery form,
// 32 bytes each (at most 32 KB); a lane reads the others' as broadcasts.
//   k_lagrange   lane (g, j): p_j = (-x_j) prod_{i != j} (x_j - x_i) -- k subtractions and products -- then its own Fermat
//                inversion shift_j = p_j^-1 (about 450 products; for k = 67 cheaper than a prefix-product exchange through
//                LDS would make it, and every lane does the same work).  The shifts then replace the points in LDS, the
//                first lanes of wavefront 0 add up one group each and invert the sum (one more inversion per WORKGROUP,
//                side by side), and every lane writes L_j = shift_j den as 32 bytes big-endian: the layout
//                blsgpu_g1_msm_dev / blsgpu_g2_msm_dev take as d_scalars.
//                status[g] = 1, or 0 and all-zero coefficients if some x_j is 0 or >= n or two of them are equal: where
//                the reference asserts.  Equal points need no search: p_j = 0.
//   k_fr_dot     lane (g, j): L_j (y_j mod n); the first lanes add up one group each: out[g] = sum_j L_j y_j mod n.
// Every store is a plain C++ store; the status of a group is written by its lane j = 0 only.
// Not constant-time (k_fr_dot handles secrets: the shares y_j): the reductions and zero tests branch on values.
#pragma once
#include "fr_scalar.h"

namespace blsgpu {
namespace lagr {

constexpr uint32_t MAX_K = BLSGPU_LAGRANGE_MAX_K;
static_assert(MAX_K == 1024, "a group is one workgroup: at most 1024 threads");

// (the launch shape for groups of k points, 1 <= k <= MAX_K: keys::lagrange_shape, keys_plan.h)

__global__ void __launch_bounds__(1024) k_lagrange(const uint8_t* __restrict__ x, uint32_t k, uint32_t groups, uint32_t gpb,
                                                   uint8_t* __restrict__ out, uint8_t* __restrict__ status)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    extern __shared__ __align__(16) uint32_t lagr_lds[];
    const uint32_t items = gpb * k, t = threadIdx.x;
    uint32_t* const X = lagr_lds;                                            // items x 8: the points, later the shifts
    uint32_t* const DEN = X + (size_t)items * 8;                             // gpb x 8
    uint32_t* const BAD = DEN + (size_t)gpb * 8;                             // gpb
    const uint32_t gl = t / k, j = t - gl * k;
    const size_t g = (size_t)blockIdx.x * gpb + gl;
    const bool live = t < items && g < groups;
    if (t < gpb) BAD[t] = 0;
    __syncthreads();
    uint32_t v[8];
    frs::set_zero(v);
    if (live && !frs::lagrange_point(x + (g * k + j) * 32, v)) BAD[gl] = 1;
    if (t < items) frs::copy(X + (size_t)t * 8, v);
    __syncthreads();
    if (live) {
        uint32_t p[8];
        frs::lagrange_weight(X + (size_t)gl * k * 8, k, j, p);
        if (frs::is_zero(p)) BAD[gl] = 1;
        frs::inv(v, p);
    }
    __syncthreads();                                                         // every weight has read every point
    if (t < items) frs::copy(X + (size_t)t * 8, v);
    __syncthreads();
    if (t < gpb && (size_t)blockIdx.x * gpb + t < groups) {
        uint32_t den[8];
        frs::lagrange_den(X + (size_t)t * k * 8, k, den);
        frs::copy(DEN + (size_t)t * 8, den);
    }
    __syncthreads();
    if (!live) return;
    const bool bad = BAD[gl] != 0;
    uint32_t l[8];
    frs::mul(l, v, DEN + (size_t)gl * 8);
    frs::from_mont(l, l);
    if (bad) frs::set_zero(l);
    frs::to_be(l, out + (g * k + j) * 32);
    if (j == 0) status[g] = bad ? 0 : 1;
}
#else
;
#endif

__global__ void __launch_bounds__(1024) k_fr_dot(const uint8_t* __restrict__ coeffs, const uint8_t* __restrict__ y, uint32_t k,
                                                 uint32_t groups, uint32_t gpb, uint8_t* __restrict__ out)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    extern __shared__ __align__(16) uint32_t lagr_lds[];
    const uint32_t items = gpb * k, t = threadIdx.x;
    uint32_t* const T = lagr_lds;                                            // items x 8: the terms
    const uint32_t gl = t / k, j = t - gl * k;
    const size_t g = (size_t)blockIdx.x * gpb + gl;
    uint32_t v[8];
    frs::set_zero(v);
    if (t < items && g < groups) frs::dot_term(coeffs + (g * k + j) * 32, y + (g * k + j) * 32, v);
    if (t < items) frs::copy(T + (size_t)t * 8, v);
    __syncthreads();
    const size_t gs = (size_t)blockIdx.x * gpb + t;
    if (t < gpb && gs < groups) {
        uint32_t acc[8];
        frs::set_zero(acc);
        for (uint32_t i = 0; i < k; i++) frs::add(acc, acc, T + ((size_t)t * k + i) * 8);
        frs::to_be(acc, out + gs * 32);
    }
}
#else
;
#endif

}  // namespace lagr
}  // namespace blsgpu
