// blsgpu_smul64.hip -- multiplication of a point by a SHORT PUBLIC scalar: out_i = w_i P_i for 64-bit weights, one point per LANE
// (G1) or per LANE PAIR (G2) on SrtG<DEG>'s madd / dbl / add / affine_out (blsgpu_msm.hip), for blsgpu_g1_mul_short /
// blsgpu_g2_mul_short and the leaves of blsgpu_verify_find (included by blsgpu_api.hip, built with blsgpu_msm.hip in translation
// unit 5).  vmgen/smul64_model.py is the specification of the digits and of the window recurrence (tests/test_smul64_model.py).
//   schedule   k_smul's (blsgpu_msm.hip) cut to the 64 bits a weight has: fixed 4-bit windows from the top, SIXTEEN of them --
//              60 doublings, 16 complete additions of a table entry and 14 mixed additions for the table 2P .. 15P (entry 0
//              is infinity, entry 1 the point: the loop has no branch on a digit).  k_smul spends 252, 64 and 14 on the same
//              weight zero-extended to 32 bytes; the result is the same point, and the affine bytes of a point are unique, so
//              the bytes are those of blsgpu_g1_msm / blsgpu_g2_msm(k = 1) on the zero-extended weights.
//   public     the weights are PUBLIC data (the caller's random multipliers): the table entry is fetched at an address the
//              digit chooses.  Nothing here is scalar-independent and nothing is claimed about timing; a secret scalar belongs
//              on secret_window.h's schedule (blsgpu_g2smul.hip, k_fix_mul_secret).
//   table      0 .. 15 P in the L28 projective form in the unit's own piece of HBM workspace, as k_smul keeps it: 16 x 168
//              bytes per G1 lane are 172 KB per wavefront, more than the 160 KB of LDS a CU has, and the accumulator and the
//              operands of a complete addition leave no registers for a register-resident table at two wavefronts per
//              SIMD.  A unit reads its own 168 (336) contiguous bytes per window: 16 + 14 table accesses of ~0.4 KB against
//              ~90 point operations of several thousand instructions each, so the uncoalesced layout is not what bounds the
//              kernel.  A signed-digit table of eight entries would halve the workspace and the table additions at the price
//              of a seventeenth window (w + 0x88..8 carries out of 64 bits) and a negation per window: about 61 against 63
//              addition-equivalents.  NOT MEASURED; the plain nibbles are kept.
//   launch     __launch_bounds__(64, 2): the 256-register budget k_smul, k_sum_chunks and the sorted-bucket kernels run the
//              same point arithmetic under (the compiler's report: 222 registers and no scratch for G1, 230 and 116 bytes
//              of scratch without a spill for G2).  Whether three wavefronts per SIMD (168 registers, the additions
//              spilling) would hide more of the table's latency has NOT been measured for this kernel.  A launch takes at
//              most SRT_LANES / LP units (two wavefronts on every SIMD), which bounds the table at 352 MB whatever the call.
//   input      prep / live: k_lane_prep's points (affine L28, (0, 0) not live); idx (may be NULL): unit i multiplies point
//              idx[i] of the prepared list instead of point i -- blsgpu_verify_find multiplies a key TABLE by per-item weights.
//              A point that is not live, or a zero weight, gives infinity: (0, 0) and out_inf = 1.
//   tail       spare units of the last wavefront repeat the last point and store nothing (k_smul's convention); the unit is
//              the global lane / LP, so both lanes of a G2 pair are spare or neither is.
#pragma once

namespace blsgpu {

constexpr uint32_t SMUL64_WINDOWS = 16;

// weights: n x 8 bytes big-endian; table: units x SMUL_T x G::PJ dwords of this launch's own
template <int DEG>
__global__ void __launch_bounds__(64, 2) k_smul64(const uint32_t* __restrict__ prep, const uint8_t* __restrict__ live,
                                                  const uint32_t* __restrict__ idx, const uint8_t* __restrict__ weights, uint32_t n,
                                                  uint32_t* __restrict__ table, uint32_t* __restrict__ out, uint8_t* __restrict__ out_inf)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    typedef SrtG<DEG> G;
    const uint32_t unit = (blockIdx.x * blockDim.x + threadIdx.x) / G::LP;
    const bool real = unit < n;
    const uint32_t g = real ? unit : n - 1u;
    const size_t pi = idx ? idx[g] : g;
    const uint8_t* wb = weights + (size_t)g * 8;
    const uint32_t hi = ((uint32_t)wb[0] << 24) | ((uint32_t)wb[1] << 16) | ((uint32_t)wb[2] << 8) | wb[3];
    const uint32_t lo = ((uint32_t)wb[4] << 24) | ((uint32_t)wb[5] << 16) | ((uint32_t)wb[6] << 8) | wb[7];
    uint32_t* T = table + (size_t)unit * SMUL_T * G::PJ;
    const bool lv = live[pi] != 0;
    typename G::P m = G::inf();
    G::st(m, T);
#pragma unroll 1
    for (uint32_t d = 1; d < SMUL_T; d++) {
        if (lv) G::madd(m, prep + pi * L28_AFF * DEG, 0u);
        G::st(m, T + (size_t)d * G::PJ);
    }
    typename G::P acc = G::inf();
#pragma unroll 1
    for (int w = (int)SMUL64_WINDOWS - 1; w >= 0; w--) {
        if (w != (int)SMUL64_WINDOWS - 1) {
#pragma unroll 1
            for (int t = 0; t < 4; t++) acc = G::dbl(acc);
        }
        const uint32_t d = ((w >= 8 ? hi : lo) >> (((uint32_t)w & 7u) * 4u)) & 15u;
        acc = G::add(acc, G::ld(T + (size_t)d * G::PJ));
    }
    G::affine_out(acc, out + (size_t)g * 24 * DEG, out_inf ? out_inf + g : nullptr, real);
}
#else
;
#endif

// every instantiation the host side launches: translation unit 5 emits them (blsgpu_tu.h)
#if BLSGPU_TU == BLSGPU_TU_MSM
__attribute__((used)) static const void* const blsgpu_instances_smul64[] = {(const void*)&k_smul64<1>, (const void*)&k_smul64<2>};
#endif

}  // namespace blsgpu
