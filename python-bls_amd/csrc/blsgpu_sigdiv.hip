// blsgpu_sigdiv.hip -- batched Signature.divide_by (signature.py:44-103 of the reference): the kernels that turn the
// aggregation-tree exponents of every divisor of a call into its checked quotient scalar, on the arithmetic of sigdiv.h
// (included by blsgpu_api.hip, built with blsgpu_lagrange.hip in translation unit 8).  The sums themselves are
// blsgpu_g2_range_sums / blsgpu_g2_msm_ranges (blsgpu_api.hip sig_divide_dev).
//
// The input is two CSR tables: pt_off[m + 1] over the points -- dividend j owns [pt_off[j], pt_off[j + 1]), its own signature
// first, then its divisors -- and ent_off[n_pts + 1] over the entries, the row of a dividend's own point empty, a divisor's
// with at least one entry.  head: four words of the workspace, zero at the start -- [0] the offsets are refused, [1] the
// number of empty rows, [2] the number of divisors with a quotient other than 1.
//   k_sigdiv_check  one lane per index: the offsets ascend and end where they must, every dividend has a point and its own
//                   row is empty; the empty rows are COUNTED, and with m distinct own rows empty a count of m says that no
//                   divisor's row is (the host compares).  Every later kernel returns at once when head[0] is set, so none of
//                   them follows an offset that was not checked.
//   k_sigdiv_cross  one lane per ENTRY: the owning point by binary search in ent_off (the last p with ent_off[p] <= e: empty
//                   rows share their offset with the next row and own nothing), that divisor's first entry, the cross test
//                   a_e b_0 == a_0 b_e -- four conversions and two products, the same for every lane: one divisor of 100 000
//                   entries costs what 100 000 divisors of one entry cost.  A failing lane stores the byte 1 to mism[owner], a
//                   lane with b_e = 0 mod n to zero[owner]: plain byte stores, every writer writes the same value.
//   k_sigdiv_quot   one lane per POINT: a dividend's own point (an empty row) gets scalar 1 and status 0; a divisor status 2 if
//                   `zero`, else 1 if `mism` (both with scalar 0), else 0 and (n - a_0 / b_0) mod n: ONE Fermat inversion, about
//                   380 products, per divisor.  It also writes the working copy of the points for the plain path -- a divisor
//                   whose quotient is 1 as -P, everything else as it came -- and the byte nonunit[p]; the wavefront's count
//                   of non-unit quotients goes to head[2] in one atomic.  Lanes of own and refused points idle while their
//                   wavefront's divisors invert; a call is mostly divisors.
//   k_sigdiv_fold   one lane per DIVIDEND: the OR of its divisors' statuses (refused[j]) and its range (begin, end) for the
//                   sums.  The trip count is the dividend's number of divisors.
//   k_sigdiv_refuse one lane per dividend, after the sums: a refused dividend gets flag 3 and the output (0,0).
// Every store is a plain C++ store (the counters are atomicOr / atomicAdd); no inline assembly.  MEASURED
// (profiles/sigdiv_probe.txt): with their synchronisation these kernels are 0.5 ms of a 10.5 ms call of 10 000 dividends x 3
// divisors x 4 entries on the scalar path; the plain path takes 3.6 ms.  Register counts: NOT MEASURED (`make resources TU=8`).
// Trees, exponents and signatures are PUBLIC data: NOT constant-time.
#pragma once
#include "sigdiv.h"

namespace blsgpu {
namespace sigdiv {

namespace sd = ::sigdiv;

__global__ void __launch_bounds__(256) k_sigdiv_check(const uint32_t* __restrict__ pt_off, uint32_t m, const uint32_t* __restrict__ ent_off,
                                                      uint32_t n_pts, uint32_t n_ent, uint32_t* __restrict__ head)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i == 0) bad = pt_off[0] != 0u || pt_off[m] != n_pts || ent_off[0] != 0u || ent_off[n_pts] != n_ent;
    if (i < m) {
        const uint32_t b = pt_off[i], e = pt_off[i + 1];
        if (b >= e || e > n_pts) bad = true;                                  // (b < e <= n_pts: row b exists)
        else if (ent_off[b + 1] != ent_off[b]) bad = true;
    }
    bool empty = false;
    if (i < n_pts) {
        const uint32_t b = ent_off[i], e = ent_off[i + 1];
        if (b > e || e > n_ent) bad = true;
        empty = b == e;
    }
    if (bad) atomicOr(head, 1u);
    if (empty) atomicAdd(head + 1, 1u);
}
#else
;
#endif

__global__ void __launch_bounds__(256) k_sigdiv_cross(const uint32_t* __restrict__ head, const uint32_t* __restrict__ ent_off, uint32_t n_pts,
                                                      const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint32_t n_ent,
                                                      uint8_t* __restrict__ mism, uint8_t* __restrict__ zero)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_ent || head[0] != 0u) return;
    uint32_t lo = 0, hi = n_pts;                                              // ent_off[lo] <= e always (ent_off[0] = 0)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ent_off[mid] <= e) lo = mid; else hi = mid;
    }
    const size_t first = ent_off[lo];                                         // <= e < n_ent
    const uint32_t bits = sd::entry_bits(a + 32 * first, b + 32 * first, a + 32 * (size_t)e, b + 32 * (size_t)e);
    if (bits & 1u) mism[lo] = 1;
    if (bits & 2u) zero[lo] = 1;
}
#else
;
#endif

// pts / work: n_pts x 48 words; scalars: n_pts x 32 bytes; status / nonunit: n_pts bytes
__global__ void __launch_bounds__(256) k_sigdiv_quot(uint32_t* __restrict__ head, const uint32_t* __restrict__ ent_off, uint32_t n_pts,
                                                     const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, const uint8_t* __restrict__ mism,
                                                     const uint8_t* __restrict__ zero, const uint32_t* __restrict__ pts, uint8_t* __restrict__ status,
                                                     uint8_t* __restrict__ scalars, uint8_t* __restrict__ nonunit, uint32_t* __restrict__ work)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (head[0] != 0u) return;                                                // (uniform: the ballot below sees whole wavefronts)
    const bool live = p < n_pts;
    bool other = false, negate = false;
    if (live) {
        const uint32_t first = ent_off[p], end = ent_off[p + 1];
        uint8_t* const sc = scalars + 32 * (size_t)p;
        int st = sd::OK;
        if (first == end) {
            sd::scalar_const(1, sc);
        } else {
            st = sd::status_of(mism[p] != 0, zero[p] != 0);
            if (st != sd::OK) {
                sd::scalar_const(0, sc);
            } else {
                negate = sd::quotient_scalar(a + 32 * (size_t)first, b + 32 * (size_t)first, sc);
                other = !negate;
            }
        }
        status[p] = (uint8_t)st;
        nonunit[p] = other ? 1 : 0;
        const uint32_t* const src = pts + 48 * (size_t)p;
        uint32_t* const dst = work + 48 * (size_t)p;
        if (negate) {
            sd::neg_point(src, dst);
        } else {
#pragma unroll
            for (int w = 0; w < 48; w++) dst[w] = src[w];
        }
    }
    const unsigned long long votes = __ballot(other);
    if (votes != 0ull && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)votes) - 1)) atomicAdd(head + 2, (uint32_t)__popcll(votes));
}
#else
;
#endif

// refused: m bytes; ranges: m x (begin, end)
__global__ void __launch_bounds__(256) k_sigdiv_fold(const uint32_t* __restrict__ head, const uint32_t* __restrict__ pt_off, uint32_t m,
                                                     const uint8_t* __restrict__ status, uint8_t* __restrict__ refused, uint32_t* __restrict__ ranges)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m || head[0] != 0u) return;
    const uint32_t b = pt_off[j], e = pt_off[j + 1];
    uint32_t any = 0;
    for (uint32_t p = b + 1u; p < e; p++) any |= status[p];
    refused[j] = any ? 1 : 0;
    ranges[2 * (size_t)j] = b;
    ranges[2 * (size_t)j + 1] = e;
}
#else
;
#endif

// out: m x 48 words; flag: m bytes, over what the sums wrote
__global__ void __launch_bounds__(256) k_sigdiv_refuse(const uint8_t* __restrict__ refused, uint32_t m, uint32_t* __restrict__ out,
                                                       uint8_t* __restrict__ flag)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m || refused[j] == 0) return;
    flag[j] = 3;
    for (uint32_t w = 0; w < 48u; w++) out[(size_t)j * 48 + w] = 0u;
}
#else
;
#endif

}  // namespace sigdiv
}  // namespace blsgpu
