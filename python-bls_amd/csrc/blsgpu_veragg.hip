// blsgpu_veragg.hip -- the two glue kernels of blsgpu_verify_aggregates (include/blsgpu.h; the schedule is verify_agg_plan.h):
// m aggregate signatures of any shapes verified in one call, between the library's own stages -- hash to G2, the ragged key
// sums, the ragged multi-pairing (included by blsgpu_api.hip, built with blsgpu_mlr.hip in translation unit 9).
//   k_va_pairs    one 16-byte piece per lane, 18 lanes per pair slot (6 of the G1 point, 12 of the G2 point), consecutive lanes
//                 on consecutive pieces: a signature's slot gets (-G1, sig_j), a group's slot (sum_g, H(msg_hashes[grp_msg[g]])),
//                 as the slice's source table says.  The lane of a slot's first G1 piece folds the group's sum flag (2: a key
//                 off the curve) into the aggregate's "undecided" byte, the lane of its first G2 piece the signature's (0,0) test.
//   k_va_status   one aggregate per lane: 1 where the 144 words of its pairing result are Fq12 one, 0 where not, 2 where the
//                 aggregate is undecided.
// Plain C++ with vector loads, stores and atomics; no LDS, no inline assembly; the only early exit is a lane past the table.
// Every index read from a table was checked on the host (verify_agg::plan): nothing outside the buffers is read.
#pragma once

namespace blsgpu {
namespace veragg {

constexpr uint32_t THREADS = 256;
constexpr uint32_t G1_Q = 6, G2_Q = 12, PER = G1_Q + G2_Q;   // 16-byte pieces of an affine G1 / G2 point, of a pair slot
constexpr uint32_t E_Q = BLSGPU_FQ12_BYTES / 16;             // ... of a pairing result
constexpr uint32_t SRC_SIG = 0xFFFFFFFFu;                    // verify_agg::SIG

// total = slots x 18.  src: slots x (a, b, agg) -- (SRC_SIG, j, j) or (g, message, j); und: one byte per aggregate of the CALL,
// zeroed by the host, set through the 32-bit word that holds it
__global__ void __launch_bounds__(256) k_va_pairs(const uint32_t* __restrict__ src, size_t total, const uint4* __restrict__ sigs,
                                                  const uint4* __restrict__ neg_g1, const uint4* __restrict__ sums,
                                                  const uint8_t* __restrict__ sum_flag, const uint4* __restrict__ h,
                                                  uint4* __restrict__ g1, uint4* __restrict__ g2, uint32_t* __restrict__ und)
#if BLSGPU_EMIT(BLSGPU_TU_MLR)
{
    const size_t idx = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t slot = idx / PER;
    const uint32_t piece = (uint32_t)(idx - slot * PER);
    const uint32_t a = src[slot * 3], b = src[slot * 3 + 1], agg = src[slot * 3 + 2];
    const bool sig = a == SRC_SIG;
    bool undecided = false;
    if (piece < G1_Q) {
        g1[slot * G1_Q + piece] = sig ? neg_g1[piece] : sums[(size_t)a * G1_Q + piece];
        undecided = piece == 0 && !sig && sum_flag[a] == 2;
    } else {
        const uint32_t q = piece - G1_Q;
        const uint4* const from = sig ? sigs + (size_t)b * G2_Q : h + (size_t)b * G2_Q;
        g2[slot * G2_Q + q] = from[q];
        if (sig && q == 0) {
            uint32_t any = 0;
#pragma unroll
            for (uint32_t i = 0; i < G2_Q; i++) {
                const uint4 v = from[i];
                any |= v.x | v.y | v.z | v.w;
            }
            undecided = any == 0;
        }
    }
    if (undecided) atomicOr(und + (agg >> 2), 1u << (8 * (agg & 3)));
}
#else
;
#endif

// e: n x 576 bytes, the slice's results; und, status: the slice's first aggregate's bytes
__global__ void __launch_bounds__(256) k_va_status(const uint4* __restrict__ e, const uint8_t* __restrict__ und, uint32_t n,
                                                   uint8_t* __restrict__ status)
#if BLSGPU_EMIT(BLSGPU_TU_MLR)
{
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t diff = 0;
#pragma unroll 4
    for (uint32_t j = 0; j < E_Q; j++) {
        const uint4 v = e[(size_t)i * E_Q + j];
        // Fq12 one: the byte 1 at offset 47 (the last of the first 48-byte coefficient), zeros elsewhere
        diff |= v.x | v.y | v.z | (j == 2 ? v.w ^ 0x01000000u : v.w);
    }
    status[i] = und[i] ? 2 : diff == 0 ? 1 : 0;
}
#else
;
#endif

}  // namespace veragg
}  // namespace blsgpu
