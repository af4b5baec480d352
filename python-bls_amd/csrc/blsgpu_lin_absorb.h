// blsgpu_lin_absorb.h -- the cross-lane step of a LIN round: a combination split over 2 or 4 adjacent lanes adds the
// partial limb accumulators of the group into its first lane (vmgen/emit.py plan_lin_round).  One text for run_rounds
// (blsgpu_kernels.hip) and for the test-only check library (blsgpu_fq32_check.hip), which runs it on its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace blsgpu {

template <int CTRL>
__device__ __forceinline__ void dpp_quad_absorb(uint64_t& acc, uint32_t mask);
#define BLSGPU_DPP_ABSORB(CTRL, PERM)                                                                            \
    template <>                                                                                                  \
    __device__ __forceinline__ void dpp_quad_absorb<CTRL>(uint64_t& acc, uint32_t mask) {                        \
        uint32_t lo = (uint32_t)acc, hi = (uint32_t)(acc >> 32), t0, t1;                                        \
        asm volatile("v_and_b32_dpp %2, %0, %4 quad_perm:" PERM " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"  \
                     "v_and_b32_dpp %3, %1, %4 quad_perm:" PERM " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"  \
                     "v_add_co_u32 %0, vcc, %0, %2\n\t"                                                          \
                     "v_addc_co_u32 %1, vcc, %1, %3, vcc"                                                        \
                     : "+v"(lo), "+v"(hi), "=&v"(t0), "=&v"(t1)                                                  \
                     : "v"(mask)                                                                                 \
                     : "vcc");                                                                                   \
        acc = ((uint64_t)hi << 32) | lo;                                                                         \
    }
// acc += (the accumulator of another lane of the same quad) & mask, mask = 0 or ~0 of the
// READING lane (the value if the lane absorbs it, else 0): four instructions per limb
BLSGPU_DPP_ABSORB(0xF5, "[1,1,3,3]")       // lanes 0,2 of a quad += lanes 1,3
BLSGPU_DPP_ABSORB(0xAA, "[2,2,2,2]")       // lane 0 += lane 2
#undef BLSGPU_DPP_ABSORB

// w1 = the lane's merge flags (absorb1 << 14 | absorb2 << 15), levels = the round's (wave-uniform, 0 .. 2).
// a combination split over 2 or 4 adjacent lanes: the flagged lanes add their
// neighbours' partial limb accumulators (exact 64-bit integer adds)
__device__ __forceinline__ void lin_absorb(uint64_t (&acc)[12], uint32_t w1, uint32_t levels) {
    if (levels >= 1u) {
        const uint32_t m1 = (uint32_t)((int32_t)(w1 << 17) >> 31);
        asm volatile("s_nop 4");      // the hazard recogniser does not see the DPP reads inside the asm blocks
#pragma unroll
        for (int j = 0; j < 12; j++) dpp_quad_absorb<0xF5>(acc[j], m1);
    }
    if (levels >= 2u) {
        const uint32_t m2 = (uint32_t)((int32_t)(w1 << 16) >> 31);
        asm volatile("s_nop 4");
#pragma unroll
        for (int j = 0; j < 12; j++) dpp_quad_absorb<0xAA>(acc[j], m2);
    }
}

}  // namespace blsgpu
