// blsgpu_hashpks.hip -- the exponents of secure aggregation on the device (util.hash_pks, util.py:36-50 of the reference, as
// BLS.aggregate_sigs_secure, bls.py:28-56, and BLS.aggregate_pub_keys / aggregate_priv_keys, bls.py:203-249, use them), on the
// per-lane steps of hash_pks.h (included by blsgpu_api.hip, built with blsgpu_lagrange.hip in translation unit 8).
//
// A call holds `groups` groups of k serialised public keys (48 bytes each, 16-byte aligned, in the order to be hashed), one k
// per call, and asks for m exponents per group; m is independent of k.
//   k_hash_pks_digest   lane g: digest[g] = SHA256 of group g's 48 k bytes -- a loop over quads of keys (three blocks each)
//                       and the tail and padding cases of hash_pks.h, whose bounds depend on k alone.  One group per LANE:
//                       the work of a lane is 0.75 k compressions in sequence, so the kernel fills the chip from a few
//                       thousand groups on and cannot fill one wavefront below 64 -- there the caller hands in digests from
//                       the host (pk_hash_in of the entry points) and this kernel is not launched.  Workgroups of 64 lanes:
//                       a launch of few wavefronts spreads over the compute units.
//   k_hash_pks_exp      lane (g, i), i < m: t = SHA256(be32(i) || digest[g]) mod n -- one compression and at most two
//                       subtractions of n -- stored as 32 bytes big-endian at out[(g m + i) 32]: the layout blsgpu_g1_msm_dev /
//                       blsgpu_g2_msm_dev take as d_scalars and k_fr_dot_secret as its public coefficients.
// Spare lanes return before they load or store anything.  Every store is a plain C++ store.
// NO kernel here touches a secret: keys, digests and exponents are public, and the branches of hdk::reduce_n are on public
// values.  The private keys of blsgpu_aggregate_priv_keys_secure meet the exponents in k_fr_dot_secret (blsgpu_frsecret.hip).
#pragma once
#include "hash_pks.h"

namespace blsgpu {
namespace hashpks {

constexpr uint32_t DIGEST_THREADS = 64;
constexpr uint32_t EXP_THREADS = 256;

__global__ void __launch_bounds__(64) k_hash_pks_digest(const uint32_t* __restrict__ pks, size_t k, uint32_t groups, uint32_t* __restrict__ digest)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t g = blockIdx.x * DIGEST_THREADS + threadIdx.x;
    if (g >= groups) return;
    uint32_t st[8];
    hpk::digest(pks + (size_t)g * k * 12, k, st);
#pragma unroll
    for (int j = 0; j < 8; j++) digest[(size_t)g * 8 + j] = hpk::bswap(st[j]);
}
#else
;
#endif

__global__ void __launch_bounds__(256) k_hash_pks_exp(const uint32_t* __restrict__ digest, uint32_t m, size_t total, uint32_t* __restrict__ out)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const size_t idx = (size_t)blockIdx.x * EXP_THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t g = idx / m;
    const uint32_t i = (uint32_t)(idx - g * m);
    uint32_t dg[8], t[8];
#pragma unroll
    for (int j = 0; j < 8; j++) dg[j] = hpk::bswap(digest[g * 8 + j]);
    hpk::exponent(dg, i, t);
#pragma unroll
    for (int j = 0; j < 8; j++) out[idx * 8 + j] = hpk::bswap(t[7 - j]);
}
#else
;
#endif

}  // namespace hashpks
}  // namespace blsgpu
