// blsgpu_hashpks.hip -- the exponents of secure aggregation on the device (util.hash_pks, util.py:36-50 of the reference, as
// BLS.aggregate_sigs_secure, bls.py:28-56, and BLS.aggregate_pub_keys / aggregate_priv_keys, bls.py:203-249, use them), on the
// per-lane steps of hash_pks.h (included by blsgpu_api.hip, built with blsgpu_lagrange.hip in translation unit 8).
//
// A call holds `groups` groups of k serialised public keys (48 bytes each, 16-byte aligned, in the order to be hashed), one k
// per call, and asks for m exponents per group; m is independent of k.  (Groups of any sizes in one call: the *_ranges
// kernels at the end of the file.)
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

// ---- groups of ANY sizes in one call (blsgpu_hash_pks_ranges*, blsgpu_aggregate_*_secure_ranges*; host plan: secure_ranges_plan.h).
// Group g hashes the keys [pk_off[g], pk_off[g + 1]) of one list and owns the exponents [exp_off[g], exp_off[g + 1]) of
// another; either table holds groups + 1 uint32 offsets.
//   k_secr_check               lane g: the steps [g, g + 1] of both tables (a table that is NULL is not looked at) -- the first
//                              offset 0, no step down, no end past the list's count: together that is every offset within
//                              the list.  A bad step sets flag[0]; every kernel below returns on a set flag before it
//                              loads anything else, so a bad table is neither followed nor written for.  With `pairs` the
//                              lane also writes (exp_off[g], exp_off[g + 1]), the range table the ragged sums read -- and
//                              (1, 0) where its own steps are bad, which those sums' own check refuses before they write.
//   k_hash_pks_digest_ranges   lane g: digest[g] = SHA256 of the 48 len bytes of its OWN range, len = pk_off[g + 1] - pk_off[g]:
//                              hpk::digest's quad loop, tail and padding cases on the lane's length (len = 0: SHA256 of
//                              nothing).  A wavefront runs as long as its longest group; the groups are taken in the
//                              caller's order (sorting them longest first through a permutation table: NOT MEASURED).
//   k_hash_pks_exp_ranges      lane j < exp_off[groups]: its group by a binary search of exp_off (the last g with
//                              exp_off[g] <= j; at most 31 loads of a table the cache holds against a compression of 64
//                              rounds -- a group-id array would cost a fill kernel, 4 bytes per exponent and its own
//                              search per group), i = j - exp_off[g], t = SHA256(be32(i) || digest[g]) mod n at out[32 j]:
//                              what blsgpu_g?_msm_ranges_dev reads as d_scalars.
// Spare lanes return before they load or store anything.  Every store is a plain C++ store; the flag is set by plain stores
// of the one value 1.  PUBLIC data throughout.
constexpr uint32_t CHECK_THREADS = 256;

__device__ __forceinline__ bool secr_bad_step(const uint32_t* __restrict__ off, uint32_t g, uint32_t count) {
    const uint32_t a = off[g], b = off[g + 1];
    return a > b || b > count || (g == 0 && a != 0);
}

__global__ void __launch_bounds__(256) k_secr_check(const uint32_t* __restrict__ pk_off, uint32_t n_keys, const uint32_t* __restrict__ exp_off,
                                                    uint32_t n_exp, uint32_t groups, uint32_t* __restrict__ flag, uint32_t* __restrict__ pairs)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t g = blockIdx.x * CHECK_THREADS + threadIdx.x;
    if (g >= groups) return;
    bool bad = secr_bad_step(exp_off, g, n_exp);
    if (pk_off) bad |= secr_bad_step(pk_off, g, n_keys);
    if (bad) flag[0] = 1u;
    if (pairs) {
        pairs[2 * (size_t)g] = bad ? 1u : exp_off[g];
        pairs[2 * (size_t)g + 1] = bad ? 0u : exp_off[g + 1];
    }
}
#else
;
#endif

__global__ void __launch_bounds__(64) k_hash_pks_digest_ranges(const uint32_t* __restrict__ pks, const uint32_t* __restrict__ pk_off, uint32_t groups,
                                                               const uint32_t* __restrict__ flag, uint32_t* __restrict__ digest)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t g = blockIdx.x * DIGEST_THREADS + threadIdx.x;
    if (g >= groups) return;
    if (flag[0]) return;
    const uint32_t a = pk_off[g], len = pk_off[g + 1] - a;
    uint32_t st[8];
    hpk::digest(pks + (size_t)a * 12, len, st);
#pragma unroll
    for (int j = 0; j < 8; j++) digest[(size_t)g * 8 + j] = hpk::bswap(st[j]);
}
#else
;
#endif

__global__ void __launch_bounds__(256) k_hash_pks_exp_ranges(const uint32_t* __restrict__ digest, const uint32_t* __restrict__ exp_off, uint32_t groups,
                                                             uint32_t n_exp, const uint32_t* __restrict__ flag, uint32_t* __restrict__ out)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const size_t idx = (size_t)blockIdx.x * EXP_THREADS + threadIdx.x;
    if (idx >= n_exp) return;
    if (flag[0]) return;
    const uint32_t j = (uint32_t)idx;
    if (j >= exp_off[groups]) return;
    uint32_t lo = 0, hi = groups;                                    // exp_off[lo] <= j < exp_off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (exp_off[mid] <= j) lo = mid; else hi = mid;
    }
    uint32_t dg[8], t[8];
#pragma unroll
    for (int q = 0; q < 8; q++) dg[q] = hpk::bswap(digest[(size_t)lo * 8 + q]);
    hpk::exponent(dg, j - exp_off[lo], t);
#pragma unroll
    for (int q = 0; q < 8; q++) out[idx * 8 + q] = hpk::bswap(t[7 - q]);
}
#else
;
#endif

}  // namespace hashpks
}  // namespace blsgpu
