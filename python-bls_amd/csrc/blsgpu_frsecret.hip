// blsgpu_frsecret.hip -- the scalar-field work of the threshold scheme on SECRET values: a dealing's fragments
// (PrivateKey.new_threshold, keys.py:92-117 of the reference), the recombination of shares (Threshold.interpolate_at_zero,
// threshold.py:91-101) and the scalar lambda_i sk_i of a unit signature (PrivateKey.sign_threshold, keys.py:134-141), on the
// masked forms of fr_scalar.h (included by blsgpu_api.hip, built with blsgpu_lagrange.hip in translation unit 8).
//
// The claim is that of k_fix_mul_secret and k_g2_smul: the sequence of instructions and of memory addresses does not depend
// on the coefficients, shares or keys.  It does depend on t, k, the counts, lane indices and the PUBLIC points x (player
// numbers) and Lagrange coefficients L_j (computed from them by k_lagrange).  Timing inside the hardware is not claimed.
//   k_fr_poly_eval_secret   lane (p, j): out[p][j] = sum_k c[p][k] x_j^k mod n.  A workgroup serves ONE polynomial and a run of
//                           up to 256 points: its threads first reduce the t coefficients (masked), convert them to
//                           Montgomery form and park them in LDS (32 bytes each, t <= 1024: 32 KB); every lane then runs
//                           Horner from the top coefficient, reading coefficient k at step k -- a broadcast whose address
//                           depends on k alone -- t - 1 masked products and additions.  The spare lanes of a polynomial's
//                           last workgroup do the same work on its last point and store nothing.
//   k_fr_dot_secret         k_fr_dot's lane layout and reduction (blsgpu_lagrange.hip) with dot_term_masked and masked
//                           additions: out[g] = sum_j L_j y_j mod n for secret y_j.
//   k_fr_scale_secret       lane i: out_i = L_i (sk_i mod n) mod n, 32 bytes big-endian: the scalar blsgpu_sign_threshold
//                           hands to k_g2_smul.
//   k_fr_sum_secret         out[g] = sum_j y[g k + j] mod n for secret y below 2^256 (a player's share: the fragments it was
//                           dealt, BLS.aggregate_priv_keys): frs::sum_term_masked per term -- a masked reduction and a masked
//                           addition, no Montgomery form, no product -- in k_fr_dot_secret's lane layout: whole groups share a
//                           workgroup of 256 lanes while k <= 256; above that a group has a workgroup to itself and lane l adds
//                           up the terms l, l + 256, ... before the reduction through LDS.  k has no upper limit.
//   k_g2_spread             (public data) session g's point H(m_g) copied to the k slots of its signers.
// Every store is a plain C++ store.
#pragma once
#include "fr_scalar.h"

namespace blsgpu {
namespace frsec {

constexpr uint32_t EVAL_THREADS = 256;                                       // points per workgroup of k_fr_poly_eval_secret
constexpr uint32_t SUM_THREADS = 256;                                        // lanes per workgroup of k_fr_sum_secret

// secrets: coeffs (every line that touches C, v or acc below).  Public: t, n_x, bpp, x.
__global__ void __launch_bounds__(256) k_fr_poly_eval_secret(const uint8_t* __restrict__ coeffs, uint32_t t, const uint8_t* __restrict__ x,
                                                             uint32_t n_x, uint32_t bpp, uint8_t* __restrict__ out)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    extern __shared__ __align__(16) uint32_t frsec_lds[];
    uint32_t* const C = frsec_lds;                                           // t x 8: the coefficients in Montgomery form
    const size_t p = blockIdx.x / bpp;
    const uint32_t run = blockIdx.x - (uint32_t)p * bpp;
    for (uint32_t k = threadIdx.x; k < t; k += EVAL_THREADS) {
        uint32_t v[8];
        frs::poly_coeff_masked(coeffs + (p * t + k) * 32, v);
        frs::copy(C + (size_t)k * 8, v);
    }
    __syncthreads();
    const uint32_t j = run * EVAL_THREADS + threadIdx.x;
    const bool live = j < n_x;
    uint32_t xm[8], r[8];
    frs::poly_point(x + (size_t)(live ? j : n_x - 1) * 32, xm);              // a spare lane: the last point again
    frs::poly_horner_masked(C, t, xm, r);
    if (live) frs::to_be(r, out + (p * n_x + j) * 32);
}
#else
;
#endif

// secrets: y (v, T, acc).  Public: the coefficients, k, groups, gpb.
__global__ void __launch_bounds__(1024) k_fr_dot_secret(const uint8_t* __restrict__ coeffs, const uint8_t* __restrict__ y, uint32_t k,
                                                        uint32_t groups, uint32_t gpb, uint8_t* __restrict__ out)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    extern __shared__ __align__(16) uint32_t frsec_lds[];
    const uint32_t items = gpb * k, t = threadIdx.x;
    uint32_t* const T = frsec_lds;                                           // items x 8: the terms
    const uint32_t gl = t / k, j = t - gl * k;
    const size_t g = (size_t)blockIdx.x * gpb + gl;
    uint32_t v[8];
    frs::set_zero(v);
    if (t < items && g < groups) frs::dot_term_masked(coeffs + (g * k + j) * 32, y + (g * k + j) * 32, v);
    if (t < items) frs::copy(T + (size_t)t * 8, v);
    __syncthreads();
    const size_t gs = (size_t)blockIdx.x * gpb + t;
    if (t < gpb && gs < groups) {
        uint32_t acc[8];
        frs::set_zero(acc);
        for (uint32_t i = 0; i < k; i++) frs::add_masked(acc, acc, T + ((size_t)t * k + i) * 8);
        frs::to_be(acc, out + gs * 32);
    }
}
#else
;
#endif

// secrets: y (v, T, acc).  Public: k, groups, gpb, per (the lanes a group has: min(k, 256)).
__global__ void __launch_bounds__(256) k_fr_sum_secret(const uint8_t* __restrict__ y, size_t k, uint32_t groups, uint32_t gpb, uint32_t per,
                                                       uint8_t* __restrict__ out)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    __shared__ __align__(16) uint32_t T[SUM_THREADS * 8];                    // one partial sum per lane
    const uint32_t items = gpb * per, t = threadIdx.x;
    const uint32_t gl = t / per, j = t - gl * per;
    const size_t g = (size_t)blockIdx.x * gpb + gl;
    uint32_t v[8];
    frs::set_zero(v);
    if (t < items && g < groups)
        for (size_t i = j; i < k; i += per) frs::sum_term_masked(y + (g * k + i) * 32, v);
    frs::copy(T + (size_t)t * 8, v);
    __syncthreads();
    const size_t gs = (size_t)blockIdx.x * gpb + t;
    if (t < gpb && gs < groups) {
        uint32_t acc[8];
        frs::set_zero(acc);
        for (uint32_t i = 0; i < per; i++) frs::add_masked(acc, acc, T + ((size_t)t * per + i) * 8);
        frs::to_be(acc, out + gs * 32);
    }
}
#else
;
#endif

// secrets: sks (v).  Public: the coefficients, n.
__global__ void __launch_bounds__(256) k_fr_scale_secret(const uint8_t* __restrict__ coeffs, const uint8_t* __restrict__ sks, uint32_t n,
                                                         uint8_t* __restrict__ out)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t v[8];
    frs::dot_term_masked(coeffs + i * 32, sks + i * 32, v);
    frs::to_be(v, out + i * 32);
}
#else
;
#endif

// out[i] = pts[(lo + i) / k] for the m scalars [lo, lo + m) of a call: 48 words per G2 point, one word per thread
__global__ void __launch_bounds__(256) k_g2_spread(const uint32_t* __restrict__ pts, uint32_t k, size_t lo, uint32_t m,
                                                   uint32_t* __restrict__ out)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)m * 48) return;
    const size_t i = idx / 48, w = idx - i * 48;
    out[idx] = pts[(lo + i) / k * 48 + w];
}
#else
;
#endif

}  // namespace frsec
}  // namespace blsgpu
