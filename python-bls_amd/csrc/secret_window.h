// secret_window.h -- the window schedule of the kernels that multiply by SECRET scalars: k_g2_smul (blsgpu_g2smul.hip,
// out_i = s_i P_i on G2) and k_fix_mul_secret (blsgpu_g1fix.hip, out_i = s_i G1).  vmgen/g2smul_model.py (recode, the G2
// schedule) and vmgen/g1fixs_model.py (the G1 table and schedule) are its specification; tests/test_g2smul_model.py and
// tests/test_g1fixs_model.py hold their values against the host's curve arithmetic and their traces == across scalars.
//
// WHAT IS CLAIMED: the sequence of instructions and of memory addresses does not depend on the scalars.  No branch, loop
// bound, load address or store address is computed from a scalar byte:
//   recoding   signed 4-bit digits by the sorted sums' trick (blsgpu_msm.hip, which has a case split for large scalars;
//              this has none): the nibbles of s + C, C = sum_w 8 16^w over 65 windows, minus 8 are digits d_w in [-8, 8)
//              with sum_w d_w 16^w = s for every s < 2^256 (s + C < 16^65).  Nine additions with carry, no branch on a
//              value; the nine words lie in LDS in a column of the scalar's own and are read by the window index (a
//              register array indexed by w >> 3 would go to scratch).
//   window     every window reads ALL EIGHT table entries at addresses formed from the window index, the entry index and
//              the lane alone, and keeps entry |d| - 1 by compare-and-select; y or the normalised -y is kept by select;
//              then ONE complete addition.  A zero digit is handled by select as well (each kernel says how); nothing is
//              skipped, so every scalar, 0 and 2^256 - 1 included, runs the same additions (and doublings, where there are any).
//   output     one fq_inv (fq32.h): 37 batches of 30 division steps, branch-free and of fixed length, 0 -> 0, so infinity
//              leaves as (0, 0).  The compression flag is bls::gt_half_q_mask, a mask, and looks at the result only.
//   tail       spare lanes of the last workgroup repeat the last scalar and store nothing (a matter of the index).
// WHAT IS NOT CLAIMED: data-dependent timing inside the hardware (the duration of an instruction, of a cache or memory
// access as a function of the values it handles), and anything about public inputs (points, messages, HD indices).  The
// scalars are the literal 256-bit integers, not reduced mod the group order.
//
// A kernel on this header declares `__shared__ uint32_t rec[swin::REC_WORDS][COLS]`, one column per scalar of the workgroup,
// and keeps every use of a digit inside sel() / select_entry(): the claim is argued over this file and the few lines of
// each kernel that call it.
#pragma once

namespace blsgpu {
namespace swin {

constexpr uint32_t WINDOWS = 65, TAB = 8, REC_WORDS = 9;        // digits of a scalar, |d| of a table entry, words of s + C

// s + C into column `slot`; s: the scalar's 8 words as they lie in memory (32 bytes big-endian)
template <uint32_t COLS>
__device__ __forceinline__ void recode(uint32_t (&rec)[REC_WORDS][COLS], uint32_t slot, const uint32_t* __restrict__ s) {
    uint64_t t = 0;
#pragma unroll
    for (int j = 0; j < (int)REC_WORDS; j++) {
        t += (uint64_t)(j < 8 ? bswap32(s[7 - j]) : 0u) + (j < 8 ? 0x88888888u : 0x8u);
        rec[j][slot] = (uint32_t)t;
        t >>= 32;
    }
}

struct Digit {
    uint32_t sgn;       // all ones for a negative digit
    uint32_t ad;        // |d|: 0 .. 8
    uint32_t mz;        // all ones for a zero digit
};
template <uint32_t COLS>
__device__ __forceinline__ Digit digit(const uint32_t (&rec)[REC_WORDS][COLS], uint32_t slot, uint32_t w) {
    const int32_t d = (int32_t)((rec[w >> 3][slot] >> (4u * (w & 7u))) & 15u) - 8;
    const uint32_t sgn = (uint32_t)(d >> 31);
    const uint32_t ad = ((uint32_t)d ^ sgn) - sgn;
    return {sgn, ad, 0u - (uint32_t)(ad == 0u)};
}

// a where the mask is all ones, b where it is zero
__device__ __forceinline__ uint32_t sel(uint32_t a, uint32_t b, uint32_t m) { return (a & m) | (b & ~m); }
__device__ __forceinline__ int32_t sel(int32_t a, int32_t b, uint32_t m) { return (int32_t)sel((uint32_t)a, (uint32_t)b, m); }

// q = entry |d| - 1 of a window's TAB entries of DW dwords, dword j of entry e at T[(e DW + j) stride]: every entry is
// read, the mask keeps one.  keep0 is OR-ed into entry 0's mask (a kernel that adds entry 0 for a zero digit passes mz);
// ad = 0 with keep0 = 0 leaves q = 0.  UNROLLED: the eight entries in line (addresses the same in every lane: scalar
// loads), else a loop of eight rounds (addresses per lane: vector loads, one entry's registers at a time).
template <uint32_t DW, bool UNROLLED>
__device__ __forceinline__ void select_entry(uint32_t (&q)[DW], const uint32_t* __restrict__ T, size_t stride, uint32_t ad, uint32_t keep0) {
#pragma unroll
    for (int j = 0; j < (int)DW; j++) q[j] = 0;
#pragma unroll(UNROLLED ? TAB : 1)
    for (uint32_t e = 0; e < TAB; e++) {
        const uint32_t m = (0u - (uint32_t)(ad == e + 1u)) | (e == 0u ? keep0 : 0u);
#pragma unroll
        for (int j = 0; j < (int)DW; j++) q[j] |= T[(size_t)(e * DW + j) * stride] & m;
    }
}

}  // namespace swin
}  // namespace blsgpu
