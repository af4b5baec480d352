// hd_derive.h -- the byte-level steps of HD child derivation (ExtendedPrivateKey.private_child /
// ExtendedPublicKey.public_child, keys.py:191-215 and 276-296 of the reference): HMAC-SHA256 with the chain code as key
// (util.hmac256, util.py:19-33) and 256-bit scalars mod the group order n.  The same source compiles for the host
// (HD_FN = static inline) so tests/test_hd_host.py and tests/test_hd_paths_host.py check it against Python's hmac, and for gfx950 (blsgpu_g1fix.hip:
// one child per lane).
//
// A child's HMAC message is ser || be32(i) || b, b in {0, 1}: 48 + 4 + 1 = 53 bytes (parent public key, index < 2^31)
// or 32 + 4 + 1 = 37 bytes (parent private key, hardened index).  The key (32 bytes) XOR ipad / opad is one block each,
// whose compressions -- the MIDSTATES -- are the same for every child of a parent: hmac_key computes them once per call.
// After them a message of at most 55 bytes is one padded block, and the outer hash of the 32-byte inner digest one more:
// two compressions per HMAC, four per child.  A PATH (blsgpu_hd_paths: one path per lane, a parent of its own) changes its
// chain code level by level, so there the midstates are per lane and per level -- hmac_key_words, six compressions per
// level -- and the parent fingerprint of the leaf is one more (fingerprint).  A SEED (blsgpu_keys_from_seeds, blsgpu_seeds.hip:
// one seed per lane) is a message of any length under a fixed key: hmac_long / hmac_long_pair (tests/test_seeds_host.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HD_FN __host__ __device__ __forceinline__
#else
#define HD_FN static inline
#endif

namespace hdk {

HD_FN uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// One SHA-256 compression (FIPS 180-4 6.2.2) of the block w_in[16] (big-endian words) into the chaining state st[8].
// The rounds of blsgpu_h2c.hip's sha256_block, which starts from the IV instead.
HD_FN void sha256_compress(uint32_t st[8], const uint32_t w_in[16]) {
    const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
        0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
        0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
        0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
        0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
        0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t w[64];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = w_in[i];
#pragma unroll
    for (int i = 16; i < 64; i++) {
        uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
        uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
        w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], hh = st[7];
#pragma unroll
    for (int i = 0; i < 64; i++) {
        uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25);
        uint32_t ch = (e & f) ^ (~e & g);
        uint32_t t1 = hh + S1 + ch + K[i] + w[i];
        uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22);
        uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
        uint32_t t2 = S0 + mj;
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += hh;
}

// The chaining states after the key blocks (key XOR 0x36.., key XOR 0x5c..) of util.hmac256.
struct HmacKey { uint32_t ipad[8], opad[8]; };

// key: klen <= 64 bytes (a chain code is 32; util.hmac256 hashes longer keys first, which never happens here)
HD_FN void hmac_key(const uint8_t* key, int klen, HmacKey& k) {
    const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint32_t wi[16], wo[16];
    for (int j = 0; j < 16; j++) {
        uint32_t v = 0;
        for (int b = 0; b < 4; b++) v = (v << 8) | (4 * j + b < klen ? key[4 * j + b] : 0u);
        wi[j] = v ^ 0x36363636u;
        wo[j] = v ^ 0x5c5c5c5cu;
    }
    for (int j = 0; j < 8; j++) { k.ipad[j] = iv[j]; k.opad[j] = iv[j]; }
    sha256_compress(k.ipad, wi);
    sha256_compress(k.opad, wo);
}

// HMAC of a message that fits one block behind the key block: `block` is the message, its 0x80 byte and the bit length
// (64 + len) * 8 in word 15 (pad_block).  out: the digest as 8 big-endian words.
HD_FN void hmac_block(const HmacKey& k, const uint32_t block[16], uint32_t out[8]) {
    uint32_t in[8], w[16];
#pragma unroll
    for (int j = 0; j < 8; j++) in[j] = k.ipad[j];
    sha256_compress(in, block);
#pragma unroll
    for (int j = 0; j < 8; j++) { w[j] = in[j]; w[j + 8] = 0; out[j] = k.opad[j]; }
    w[8] = 0x80000000u;
    w[15] = (64 + 32) * 8;
    sha256_compress(out, w);
}

// message bytes m[0 .. len), len <= 55 -> the padded block hmac_block takes
HD_FN void pad_block(const uint8_t* m, int len, uint32_t block[16]) {
    for (int j = 0; j < 16; j++) block[j] = 0;
    for (int i = 0; i < len; i++) block[i >> 2] |= (uint32_t)m[i] << (24 - 8 * (i & 3));
    block[len >> 2] |= 0x80u << (24 - 8 * (len & 3));
    block[15] = (uint32_t)(64 + len) * 8;
}

// The two HMACs of one child (keys.py:202-204 / 284-286 of the reference): ser = sw big-endian words (12: a public key,
// 8: a private key), then be32(index), then b.  i_left / i_right: 8 big-endian words each.
HD_FN void child_hmacs(const HmacKey& k, const uint32_t* ser, int sw, uint32_t index, uint32_t i_left[8], uint32_t i_right[8]) {
    uint32_t block[16];
    for (int j = 0; j < 16; j++) block[j] = j < sw ? ser[j] : 0u;
    block[sw] = index;
    block[15] = (uint32_t)(64 + 4 * sw + 5) * 8;
    block[sw + 1] = 0x00800000u;                                // b = 0, then the 0x80 byte
    hmac_block(k, block, i_left);
    block[sw + 1] = 0x01800000u;                                // b = 1
    hmac_block(k, block, i_right);
}

// ---- paths: the parent changes level by level, so the key midstates are per lane and per level ------------------------
// hmac_key for a chain code held as 8 big-endian words (the i_right of the level before): two compressions.
HD_FN void hmac_key_words(const uint32_t chain[8], HmacKey& k) {
    const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint32_t wi[16], wo[16];
    for (int j = 0; j < 16; j++) {
        const uint32_t v = j < 8 ? chain[j] : 0u;
        wi[j] = v ^ 0x36363636u;
        wo[j] = v ^ 0x5c5c5c5cu;
    }
    for (int j = 0; j < 8; j++) { k.ipad[j] = iv[j]; k.opad[j] = iv[j]; }
    sha256_compress(k.ipad, wi);
    sha256_compress(k.opad, wo);
}

// One level of a path (keys.py:202-204 / 284-286 of the reference) under the chain code `chain`: its two midstates, then
// the two HMACs of child_hmacs -- six compressions.
HD_FN void path_step(const uint32_t chain[8], const uint32_t* ser, int sw, uint32_t index, uint32_t i_left[8], uint32_t i_right[8]) {
    HmacKey k;
    hmac_key_words(chain, k);
    child_hmacs(k, ser, sw, index, i_left, i_right);
}

// PublicKey.get_fingerprint (keys.py:47-49 of the reference): the first four bytes of sha256(ser) for the 48 bytes of
// PublicKey.serialize() as 12 big-endian words -- one padded block, one compression from the IV.
HD_FN uint32_t fingerprint(const uint32_t ser[12]) {
    uint32_t st[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint32_t w[16];
    for (int j = 0; j < 16; j++) w[j] = j < 12 ? ser[j] : 0u;
    w[12] = 0x80000000u;
    w[15] = 48 * 8;
    sha256_compress(st, w);
    return st[0];
}

// ---- seeds: HMAC of a message of any length (PrivateKey.from_seed / ExtendedPrivateKey.from_seed, keys.py:89-92 and 180-189
// of the reference) --------------------------------------------------------------------------------------------------------
// The message is m[0 .. len) followed, when suffix >= 0, by the one byte `suffix`: M = len or len + 1 bytes behind the key
// block.  Standard padding: the 0x80 byte at M, zeros, the bit length (64 + M) * 8 in the last word -- (M + 8) / 64 + 1 blocks.
// Nothing below branches on a message byte or forms an address from one: block counts and byte positions follow from len
// and from whether there is a suffix.  m is read at p < len only (len == 0: never, m may be NULL).
HD_FN uint32_t long_blocks(uint32_t len, int suffix) { return (len + (suffix >= 0 ? 1u : 0u) + 8u) / 64u + 1u; }

// the big-endian word at byte offset off (a multiple of 4) of the padded message without its length field
HD_FN uint32_t long_word(const uint8_t* m, uint32_t len, uint32_t M, uint32_t suffix, uint32_t off) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; b++) {
        const uint32_t p = off + b;
        uint32_t byte = 0;
        if (p < len) byte = m[p];
        else if (p < M) byte = suffix;                          // p == len: the suffix byte
        else if (p == M) byte = 0x80u;
        v = (v << 8) | byte;
    }
    return v;
}

// The inner state after the len / 64 blocks that hold message bytes alone -- the same whatever follows the message, so the
// two HMACs of a seed (suffix 0 and 1) share it.
HD_FN void hmac_long_prefix(const HmacKey& k, const uint8_t* m, uint32_t len, uint32_t in[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) in[j] = k.ipad[j];
    for (uint32_t b = 0; b < len / 64u; b++) {
        uint32_t w[16];
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) w[j] = long_word(m, len, len, 0u, 64u * b + 4u * j);
        sha256_compress(in, w);
    }
}

// From hmac_long_prefix's state `in`: the one or two blocks that are left (the message's last len % 64 bytes, the suffix,
// the padding), then the outer hash.  out: the digest as 8 big-endian words.
HD_FN void hmac_long_finish(const HmacKey& k, const uint32_t in[8], const uint8_t* m, uint32_t len, int suffix, uint32_t out[8]) {
    const uint32_t M = len + (suffix >= 0 ? 1u : 0u), blocks = long_blocks(len, suffix);
    uint32_t st[8], w[16];
#pragma unroll
    for (int j = 0; j < 8; j++) st[j] = in[j];
    for (uint32_t b = len / 64u; b < blocks; b++) {
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) w[j] = long_word(m, len, M, (uint32_t)suffix & 0xffu, 64u * b + 4u * j);
        if (b + 1u == blocks) w[15] = (64u + M) * 8u;           // (the 0x80 byte lies at least nine bytes before the end)
        sha256_compress(st, w);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) { w[j] = st[j]; w[j + 8] = 0; out[j] = k.opad[j]; }
    w[8] = 0x80000000u;
    w[15] = (64 + 32) * 8;
    sha256_compress(out, w);
}

// HMAC-SHA256 under the midstates k of m[0 .. len) (suffix < 0) or of m[0 .. len) || suffix
HD_FN void hmac_long(const HmacKey& k, const uint8_t* m, uint32_t len, int suffix, uint32_t out[8]) {
    uint32_t in[8];
    hmac_long_prefix(k, m, len, in);
    hmac_long_finish(k, in, m, len, suffix, out);
}

// The two HMACs of ExtendedPrivateKey.from_seed: i_left of m || 0x00, i_right of m || 0x01, the shared blocks hashed once
HD_FN void hmac_long_pair(const HmacKey& k, const uint8_t* m, uint32_t len, uint32_t i_left[8], uint32_t i_right[8]) {
    uint32_t in[8];
    hmac_long_prefix(k, m, len, in);
    hmac_long_finish(k, in, m, len, 0, i_left);
    hmac_long_finish(k, in, m, len, 1, i_right);
}

// ---- scalars mod n (the order of G1): 8 little-endian words -----------------------------------------------------------
#define HD_N_WORDS {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u}

// s -= n if s >= n
HD_FN void sub_n_if_ge(uint32_t s[8]) {
    const uint32_t nw[8] = HD_N_WORDS;
    uint32_t t[8];
    uint64_t borrow = 0;
    for (int j = 0; j < 8; j++) {
        const uint64_t d = (uint64_t)s[j] - nw[j] - borrow;
        t[j] = (uint32_t)d;
        borrow = (d >> 32) & 1u;
    }
    if (!borrow)
        for (int j = 0; j < 8; j++) s[j] = t[j];
}
// any s < 2^256 -> s mod n (2^256 < 3n: two conditional subtractions)
HD_FN void reduce_n(uint32_t s[8]) { sub_n_if_ge(s); sub_n_if_ge(s); }
// (a + b) mod n for a, b < n (the sum is below 2^256 as n < 2^255)
HD_FN void add_mod_n(uint32_t r[8], const uint32_t a[8], const uint32_t b[8]) {
    uint64_t c = 0;
    for (int j = 0; j < 8; j++) {
        c += (uint64_t)a[j] + b[j];
        r[j] = (uint32_t)c;
        c >>= 32;
    }
    sub_n_if_ge(r);
}

// ---- the same for SECRET scalars: the subtraction is always computed and kept by a mask, no branch on the borrow --------
// (blsgpu_hd_paths_secret; values equal those of the forms above for every input, tests/test_g1fixs_host.py)
HD_FN void sub_n_if_ge_masked(uint32_t s[8]) {
    const uint32_t nw[8] = HD_N_WORDS;
    uint32_t t[8];
    uint64_t borrow = 0;
    for (int j = 0; j < 8; j++) {
        const uint64_t d = (uint64_t)s[j] - nw[j] - borrow;
        t[j] = (uint32_t)d;
        borrow = (d >> 32) & 1u;
    }
    const uint32_t keep = (uint32_t)borrow - 1u;                // all ones when s >= n
    for (int j = 0; j < 8; j++) s[j] = (t[j] & keep) | (s[j] & ~keep);
}
HD_FN void reduce_n_masked(uint32_t s[8]) { sub_n_if_ge_masked(s); sub_n_if_ge_masked(s); }
HD_FN void add_mod_n_masked(uint32_t r[8], const uint32_t a[8], const uint32_t b[8]) {
    uint64_t c = 0;
    for (int j = 0; j < 8; j++) {
        c += (uint64_t)a[j] + b[j];
        r[j] = (uint32_t)c;
        c >>= 32;
    }
    sub_n_if_ge_masked(r);
}

}  // namespace hdk
