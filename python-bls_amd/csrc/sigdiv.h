// sigdiv.h -- the scalar side of Signature.divide_by (signature.py:44-103 of the reference) on the arithmetic of fr_scalar.h:
// from the aggregation-tree exponents of a divisor to its checked quotient scalar.  The same source compiles for the host
// (HD_FN = static inline) so tests/test_sigdiv_host.py checks it against Python integers, and for gfx950
// (blsgpu_sigdiv.hip: one entry per lane for the test, one divisor per lane for the quotient).
//
// A divisor signature D of a dividend S has k >= 1 tree entries (message hash, public key); entry e carries the dividend's
// exponent a_e and the divisor's exponent b_e of that pair.  The reference computes a_e / b_e mod n for every entry -- one
// Fermat inversion each -- and refuses the divisor unless they are all equal.  Here:
//     q = a_0 b_0^-1 mod n                      one inversion per DIVISOR
//     a_e b_0 == a_0 b_e (mod n), e >= 1        two products per entry: with every b non-zero this is a_e / b_e == a_0 / b_0
// and the scalar the divisor's point is multiplied by is (n - q) mod n, so that S + sum (n - q_D) D is the quotient signature.
// An exponent is 32 bytes big-endian, ANY value below 2^256, taken mod n (hdk::reduce_n: 2^256 < 3 n).  A divisor exponent
// that is 0 mod n is not decided here (status 2): what the reference makes of a division by zero is its own business, and the
// caller's host loop reproduces it.
// Trees, exponents and signatures are PUBLIC data: everything here branches on values.  NOT constant-time.
#pragma once
#include "fr_scalar.h"

namespace sigdiv {

enum { OK = 0, NOT_UNIQUE = 1, ZERO_DIVISOR = 2 };           // a divisor's status; a dividend's own point is always OK

// the base field's modulus, 12 little-endian 32-bit words
#define SIGDIV_Q_WORDS {0xffffaaabu, 0xb9feffffu, 0xb153ffffu, 0x1eabfffeu, 0xf6b0f624u, 0x6730d2a0u, 0xf38512bfu, 0x64774b84u, 0x434bacd7u, 0x4b1ba7b6u, 0x397fe69au, 0x1a0111eau}

// an exponent (32 bytes big-endian, any value) mod n, in Montgomery form: zero exactly when the exponent is 0 mod n
HD_FN void exponent(const uint8_t* be, uint32_t xm[8]) {
    uint32_t x[8];
    frs::from_be(be, x);
    hdk::reduce_n(x);
    frs::to_mont(xm, x);
}
HD_FN bool equal(const uint32_t a[8], const uint32_t b[8]) {
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) d |= a[j] ^ b[j];
    return d == 0;
}
// entry e against the divisor's first entry (all four in Montgomery form): a_e b_0 == a_0 b_e.  Entry 0 passes against itself.
HD_FN bool cross_equal(const uint32_t a0[8], const uint32_t b0[8], const uint32_t ae[8], const uint32_t be[8]) {
    uint32_t l[8], r[8];
    frs::mul(l, ae, b0);
    frs::mul(r, a0, be);
    return equal(l, r);
}
// What one entry contributes to its divisor's verdict, from the bytes: bit 0 the cross test fails, bit 1 b_e is 0 mod n.
HD_FN uint32_t entry_bits(const uint8_t* a0_be, const uint8_t* b0_be, const uint8_t* ae_be, const uint8_t* be_be) {
    uint32_t a0[8], b0[8], ae[8], be[8];
    exponent(a0_be, a0);
    exponent(b0_be, b0);
    exponent(ae_be, ae);
    exponent(be_be, be);
    return (cross_equal(a0, b0, ae, be) ? 0u : 1u) | (frs::is_zero(be) ? 2u : 0u);
}
// The scalar of an accepted divisor from its first entry: (n - a_0 / b_0) mod n as 32 bytes big-endian, the layout
// blsgpu_g2_msm_ranges takes.  Returns whether the quotient is 1 (the divisor then enters as -D: no multiplication).
HD_FN bool quotient_scalar(const uint8_t* a0_be, const uint8_t* b0_be, uint8_t* scalar_be) {
    uint32_t a0[8], b0[8], q[8], one[8];
    exponent(a0_be, a0);
    exponent(b0_be, b0);
    frs::inv(b0, b0);
    frs::mul(q, a0, b0);
    frs::from_mont(q, q);
    frs::set_zero(one);
    one[0] = 1;
    const bool unit = equal(q, one);
    frs::neg(q, q);
    frs::to_be(q, scalar_be);
    return unit;
}
HD_FN void scalar_const(uint32_t v, uint8_t* scalar_be) {    // 0 (a refused divisor) or 1 (a dividend's own point)
    uint32_t s[8];
    frs::set_zero(s);
    s[0] = v;
    frs::to_be(s, scalar_be);
}
// a divisor's status from what its entries stored: a zero exponent outranks a mismatch
HD_FN int status_of(bool mismatch, bool zero) { return zero ? ZERO_DIVISOR : (mismatch ? NOT_UNIQUE : OK); }

// One divisor from end to end, serially (the host test's view of what k_sigdiv_cross spreads over the entries and
// k_sigdiv_quot does per divisor): a, b k x 32 bytes big-endian, k >= 1.  Returns the status; scalar_be gets the scalar, all
// zero for a refused divisor; *nonunit whether an accepted quotient differs from 1.
HD_FN int divisor(const uint8_t* a, const uint8_t* b, size_t k, uint8_t* scalar_be, int* nonunit) {
    uint32_t bits = 0;
    for (size_t e = 0; e < k; e++) bits |= entry_bits(a, b, a + 32 * e, b + 32 * e);
    const int st = status_of((bits & 1u) != 0, (bits & 2u) != 0);
    *nonunit = 0;
    if (st != OK) {
        scalar_const(0, scalar_be);
        return st;
    }
    *nonunit = quotient_scalar(a, b, scalar_be) ? 0 : 1;
    return st;
}

// ---- the point side of the plain path: -P for an affine twist point in the ABI's bytes ---------------------------------------
HD_FN uint32_t bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }
// one coordinate (48 bytes big-endian as 12 words in memory order): q - y, and 0 for 0.  The coordinate is expected below q,
// as every point the library writes is; a larger one gives a value that is not on the twist either.
HD_FN void neg_coord(const uint32_t* in, uint32_t* out) {
    const uint32_t qw[12] = SIGDIV_Q_WORDS;
    uint32_t y[12], any = 0;
#pragma unroll
    for (int w = 0; w < 12; w++) { y[11 - w] = bswap(in[w]); any |= in[w]; }
    uint64_t borrow = 0;
#pragma unroll
    for (int w = 0; w < 12; w++) {
        const uint64_t d = (uint64_t)qw[w] - y[w] - borrow;
        y[w] = any ? (uint32_t)d : 0u;
        borrow = (d >> 32) & 1u;
    }
#pragma unroll
    for (int w = 0; w < 12; w++) out[w] = bswap(y[11 - w]);
}
// a point of 192 bytes (x.c0, x.c1, y.c0, y.c1; 48 words in memory order): (x, -y); (0,0) stays (0,0).  out may be in.
HD_FN void neg_point(const uint32_t* in, uint32_t* out) {
#pragma unroll
    for (int w = 0; w < 24; w++) out[w] = in[w];
    neg_coord(in + 24, out + 24);
    neg_coord(in + 36, out + 36);
}

}  // namespace sigdiv
