// hash_pks.h -- the per-lane steps of the secure-aggregation exponents (util.hash_pks, util.py:36-50 of the reference):
//     t_i = SHA256(be32(i) || SHA256(ser(pk_0) || ... || ser(pk_{k-1}))) mod n
// on the SHA-256 compression and the scalar reduction of hd_derive.h.  The same source compiles for the host (HD_FN = static
// inline), where tests/test_secure_agg_host.py checks it against hashlib and Python integers, and for gfx950
// (blsgpu_hashpks.hip: one group per lane for the digest, one exponent per lane after it).  Everything here is PUBLIC data:
// public keys, their digest and the exponents; nothing takes a secret.
//
// The digest's message is k serialised keys of 48 bytes, 48 k bytes in all, read as big-endian words from a buffer whose
// keys are 16-byte aligned (a 16-byte aligned base: 48 is a multiple of 16).  FOUR keys are exactly THREE 64-byte blocks,
// so the body is a loop over quads of keys, twelve words per key, with no byte shuffling.  What is left is k mod 4 keys:
//     k mod 4   bytes left   whole blocks   bytes in the last block   0x80 at byte   last block holds
//        0           0            0                  0                     0          padding alone (one pure padding block)
//        1          48            0                 48                    48          12 words, 0x80, zeros, the length
//        2          96            1                 32                    32           8 words, 0x80, zeros, the length
//        3         144            2                 16                    16           4 words, 0x80, zeros, the length
// The 0x80 byte and the 64-bit bit length need 9 bytes; the last block has 64, 16, 32 and 48 bytes free: in all four cases
// the padding fits the block the message ends in (or, for k mod 4 = 0, the one block after a message that ends on a block
// boundary) -- never an extra one.  In words: 12 (k mod 4) words are left, the whole blocks among them are compressed, the
// remaining r = 12 (k mod 4) mod 16 in {0, 12, 8, 4} words open the last block, word r is 0x80000000, words 14 and 15 the
// bit length 384 k.  Every loop bound depends on k alone.
#pragma once
#include <stddef.h>

#include "hd_derive.h"

namespace hpk {

HD_FN uint32_t bswap(uint32_t v) { return __builtin_bswap32(v); }

HD_FN void iv(uint32_t st[8]) {
    const uint32_t v[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    for (int j = 0; j < 8; j++) st[j] = v[j];
}

// SHA-256 of the k keys at `keys` (12 words each as they lie in memory: big-endian bytes) -> st: 8 big-endian words.
// 3 (k / 4) + 12 (k mod 4) / 16 + 1 compressions (k = 2^20: 786 433).
HD_FN void digest(const uint32_t* keys, size_t k, uint32_t st[8]) {
    uint32_t w[16];
    iv(st);
    const uint32_t* p = keys;
    for (size_t q = 0; q < k / 4; q++)                               // a quad of keys: three whole blocks
        for (int b = 0; b < 3; b++, p += 16) {
#pragma unroll
            for (int j = 0; j < 16; j++) w[j] = bswap(p[j]);
            hdk::sha256_compress(st, w);
        }
    const uint32_t left = 12u * (uint32_t)(k & 3);                   // words left: 0, 12, 24, 36 (the table above)
    for (uint32_t b = 0; b < left / 16; b++, p += 16) {              // 0, 0, 1, 2 whole blocks
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = bswap(p[j]);
        hdk::sha256_compress(st, w);
    }
    const uint32_t r = left % 16;                                    // 0, 12, 8, 4 words open the last block
#pragma unroll
    for (uint32_t j = 0; j < 14; j++) w[j] = j < r ? bswap(p[j]) : (j == r ? 0x80000000u : 0u);
    const uint64_t bits = (uint64_t)k * 384u;
    w[14] = (uint32_t)(bits >> 32);
    w[15] = (uint32_t)bits;
    hdk::sha256_compress(st, w);
}

// t_i = SHA256(be32(i) || digest) mod n: the 36-byte message is one block; the 256-bit result is below 2^256 < 3 n, so
// hdk::reduce_n's two conditional subtractions reduce it (the value is public: the branch is fine).
// dg: the digest as 8 big-endian words; t: 8 little-endian words, below n.
HD_FN void exponent(const uint32_t dg[8], uint32_t i, uint32_t t[8]) {
    uint32_t st[8], w[16];
    iv(st);
    w[0] = i;
#pragma unroll
    for (int j = 0; j < 8; j++) w[1 + j] = dg[j];
    w[9] = 0x80000000u;
#pragma unroll
    for (int j = 10; j < 15; j++) w[j] = 0;
    w[15] = 36 * 8;
    hdk::sha256_compress(st, w);
#pragma unroll
    for (int j = 0; j < 8; j++) t[j] = st[7 - j];
    hdk::reduce_n(t);
}

}  // namespace hpk
