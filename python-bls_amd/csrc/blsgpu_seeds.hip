// blsgpu_seeds.hip -- keys from seeds, one seed per lane (blsgpu_keys_from_seeds; included by blsgpu_api.hip, built in
// translation unit 8): PrivateKey.from_seed and ExtendedPrivateKey.from_seed (keys.py:89-92 and 180-189 of the reference).
//   hd == 0   sk = HMAC-SHA256(key "BLS private key seed", seed) mod n
//   hd == 1   sk = HMAC-SHA256(key "BLS HD seed", seed || 0x00) mod n, chain code = HMAC-SHA256(key "BLS HD seed", seed || 0x01)
// The key is fixed and public: its two midstates (hdk::hmac_key) are computed once on the host and arrive as a kernel
// argument.  The seed is a message of any length up to BLSGPU_SEED_MAX_BYTES: hdk::hmac_long / hmac_long_pair, the blocks
// that hold seed bytes alone hashed once for both HMACs of the HD form.
//
// The claim is that of k_fix_mul_secret and k_hd_path_hmac_secret: the sequence of instructions and of memory addresses does
// not depend on the seeds, the digests or the keys.  It does depend on seed_len (one value per call: every lane runs the
// same number of compressions, no divergence), n, hd, the lane index and which outputs are asked for.  Timing inside the
// hardware is not claimed.
//   seed bytes   lane i reads seeds[i * seed_len + p] for p < seed_len, byte by byte, in the order of p: the address depends on
//                i, seed_len and p.  Neighbouring lanes are seed_len bytes apart -- uncoalesced for short seeds, but a seed
//                of 32 bytes is 32 byte loads beside the 65 mixed additions of its public key (DESIGN.md 2t has the
//                numbers); the bytes are not staged through LDS.
//   digest       i_left -> little-endian words -> hdk::reduce_n_masked (two subtractions kept by mask) -> 32 bytes big-endian,
//                canonical, where k_fix_mul_secret then reads them.
//   registers    w[64] and the state of hdk::sha256_compress stay in registers (fully unrolled, no scratch).
// Every store is a plain C++ store.
#pragma once
#include "hd_derive.h"

namespace blsgpu {
namespace seeds {

constexpr uint32_t PARENT_DW = 40;                          // BLSGPU_HD_PARENT_BYTES / 4: chain code 8, affine key 24, private key 8

// secrets: the seed bytes, il, ir, s.  Public: key, seed_len, n, hd, the pointers.
// sk_out: n x 32 bytes (never NULL: the caller's out_sk or the workspace k_fix_mul_secret reads); chain_out (hd; may be NULL):
// n x 32 bytes; parents (hd; may be NULL): n records of 160 bytes whose chain code and private key are written here.
__global__ void __launch_bounds__(256) k_seed_keys(hdk::HmacKey key, const uint8_t* __restrict__ seed_bytes, uint32_t seed_len, uint32_t n,
                                                   uint32_t hd, uint32_t* __restrict__ sk_out, uint32_t* __restrict__ chain_out,
                                                   uint32_t* __restrict__ parents)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* m = seed_bytes + (size_t)i * seed_len;
    uint32_t il[8], ir[8];
    if (hd) hdk::hmac_long_pair(key, m, seed_len, il, ir);
    else hdk::hmac_long(key, m, seed_len, -1, il);
    uint32_t s[8];
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] = il[7 - j];
    hdk::reduce_n_masked(s);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t v = bswap32(s[7 - j]);
        sk_out[(size_t)i * 8 + j] = v;
        if (parents) parents[(size_t)i * PARENT_DW + 32 + j] = v;
    }
    if (hd) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t v = bswap32(ir[j]);
            if (chain_out) chain_out[(size_t)i * 8 + j] = v;
            if (parents) parents[(size_t)i * PARENT_DW + j] = v;
        }
    }
}
#else
;
#endif

// (public data) the affine public keys k_fix_mul_secret wrote, n x 96 bytes, into the middle of the parent records: one
// word per thread
__global__ void __launch_bounds__(256) k_seed_pack_aff(const uint32_t* __restrict__ aff, uint32_t n, uint32_t* __restrict__ parents)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * 24) return;
    const size_t i = idx / 24, w = idx - i * 24;
    parents[i * PARENT_DW + 8 + w] = aff[idx];
}
#else
;
#endif

}  // namespace seeds
}  // namespace blsgpu
