// fr_scalar.h -- the scalar field Fr = Z / n (n the order of G1, HD_N_WORDS of hd_derive.h) and the Lagrange coefficients at
// zero over it (Threshold.lagrange_coeffs_at_zero / interpolate_at_zero, threshold.py:56-101 of the reference).  The same
// source compiles for the host (HD_FN = static inline) so tests/test_lagrange_host.py checks it against Python integers and
// the reference's vectors, and for gfx950 (blsgpu_lagrange.hip: one evaluation point per lane).
//
// A value is 8 little-endian 32-bit words, canonical (below n).  The products run in Montgomery form, x R mod n with
// R = 2^256: mul is a hand-written CIOS (coarsely integrated operand scanning) whose inner step
// (uint64_t)a * b + t + carry is one v_mad_u64_u32 on the device; n = 1 mod 2^32, so the quotient word of every
// reduction step is just -t[0].  Nothing here is generated.  The inversion is Fermat's x^(n-2) by square-and-multiply over
// the public bits of n - 2; inv(0) = 0.
// Not constant-time where it matters to a caller: is_zero and the status decisions branch on values.  The forms for secret
// operands -- mul_masked, add_masked, dot_term_masked, the sums and the polynomial evaluation on them -- are at the end of the file.
//
// The Lagrange step, exactly the reference's second barycentric form:
//     w_j = prod_{i != j} (x_j - x_i),  shift_j = w_j^-1 (-x_j)^-1,  den = (sum_j shift_j)^-1,  L_j = shift_j den.
// It is computed as shift_j = (w_j (-x_j))^-1 -- one inversion per point -- and the product w_j (-x_j) is zero exactly
// when x_j = 0 or x_j equals another point, which is where the reference asserts (status 0).  For distinct non-zero points
// sum_j shift_j = 1 / prod_j (-x_j) is never zero.
#pragma once
#include <stddef.h>
#include "hd_derive.h"

namespace frs {

#define FRS_R1_WORDS {0xfffffffeu, 0x00000001u, 0x00034802u, 0x5884b7fau, 0xecbc4ff5u, 0x998c4fefu, 0xacc5056fu, 0x1824b159u}  // R mod n
#define FRS_R2_WORDS {0xf3f29c6du, 0xc999e990u, 0x87925c23u, 0x2b6cedcbu, 0x7254398fu, 0x05d31496u, 0x9f59ff11u, 0x0748d9d9u}  // R^2 mod n
#define FRS_NM2_WORDS {0xffffffffu, 0xfffffffeu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u}  // n - 2

HD_FN void copy(uint32_t r[8], const uint32_t a[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = a[j];
}
HD_FN void set_zero(uint32_t r[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = 0;
}
HD_FN bool is_zero(const uint32_t a[8]) {
    uint32_t z = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) z |= a[j];
    return z == 0;
}
// a < n ?
HD_FN bool below_n(const uint32_t a[8]) {
    const uint32_t nw[8] = HD_N_WORDS;
    uint64_t borrow = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) borrow = (((uint64_t)a[j] - nw[j] - borrow) >> 32) & 1u;
    return borrow != 0;
}

// ---- Montgomery arithmetic: operands and results below n ---------------------------------------------------------------
// r = a b / R mod n (r may be a or b).  After every outer step t < 2n < 2^256: word 8 is a carry within the step only.
HD_FN void mul(uint32_t r[8], const uint32_t a[8], const uint32_t b[8]) {
    const uint32_t nw[8] = HD_N_WORDS;
    uint32_t t[9];
#pragma unroll
    for (int j = 0; j < 9; j++) t[j] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            c += (uint64_t)a[j] * b[i] + t[j];
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        t[8] = (uint32_t)c;
        const uint32_t m = 0u - t[0];                      // -n^-1 = -1 mod 2^32
        c = ((uint64_t)m * nw[0] + t[0]) >> 32;
#pragma unroll
        for (int j = 1; j < 8; j++) {
            c += (uint64_t)m * nw[j] + t[j];
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        t[7] = t[8] + (uint32_t)c;
    }
    hdk::sub_n_if_ge(t);
    copy(r, t);
}
HD_FN void sqr(uint32_t r[8], const uint32_t a[8]) { mul(r, a, a); }
HD_FN void add(uint32_t r[8], const uint32_t a[8], const uint32_t b[8]) { hdk::add_mod_n(r, a, b); }
HD_FN void sub(uint32_t r[8], const uint32_t a[8], const uint32_t b[8]) {
    const uint32_t nw[8] = HD_N_WORDS;
    uint32_t t[8];
    uint64_t borrow = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t d = (uint64_t)a[j] - b[j] - borrow;
        t[j] = (uint32_t)d;
        borrow = (d >> 32) & 1u;
    }
    const uint32_t mask = 0u - (uint32_t)borrow;          // a < b: add n back
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        c += (uint64_t)t[j] + (nw[j] & mask);
        r[j] = (uint32_t)c;
        c >>= 32;
    }
}
HD_FN void neg(uint32_t r[8], const uint32_t a[8]) {
    uint32_t z[8];
    set_zero(z);
    sub(r, z, a);
}
HD_FN void to_mont(uint32_t r[8], const uint32_t a[8]) {
    const uint32_t r2[8] = FRS_R2_WORDS;
    mul(r, a, r2);
}
HD_FN void from_mont(uint32_t r[8], const uint32_t a[8]) {
    uint32_t one[8];
    set_zero(one);
    one[0] = 1;
    mul(r, a, one);
}
// r = a^-1 (Montgomery form in and out; r may be a); inv(0) = 0
HD_FN void inv(uint32_t r[8], const uint32_t a[8]) {
    const uint32_t e[8] = FRS_NM2_WORDS;
    uint32_t base[8], acc[8];
    copy(base, a);
    copy(acc, a);                                          // bit 254, the top bit of n - 2
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int b = 253; b >= 0; b--) {
        sqr(acc, acc);
        if ((e[b >> 5] >> (b & 31)) & 1u) mul(acc, acc, base);
    }
    copy(r, acc);
}

// ---- 32 bytes big-endian <-> words ---------------------------------------------------------------------------------------
HD_FN void from_be(const uint8_t* b, uint32_t s[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++)
        s[7 - j] = ((uint32_t)b[4 * j] << 24) | ((uint32_t)b[4 * j + 1] << 16) | ((uint32_t)b[4 * j + 2] << 8) | b[4 * j + 3];
}
HD_FN void to_be(const uint32_t s[8], uint8_t* b) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t v = s[7 - j];
        b[4 * j] = (uint8_t)(v >> 24); b[4 * j + 1] = (uint8_t)(v >> 16); b[4 * j + 2] = (uint8_t)(v >> 8); b[4 * j + 3] = (uint8_t)v;
    }
}

// ---- the Lagrange step --------------------------------------------------------------------------------------------------
// An evaluation point (32 bytes big-endian) in Montgomery form; false -- and xm = 0 -- if it is 0 or not below n.
HD_FN bool lagrange_point(const uint8_t* be, uint32_t xm[8]) {
    uint32_t x[8];
    from_be(be, x);
    if (is_zero(x) || !below_n(x)) {
        set_zero(xm);
        return false;
    }
    to_mont(xm, x);
    return true;
}
// p = (-x_j) prod_{i != j} (x_j - x_i) over the k points X (Montgomery form, 8 words each): 1 / shift_j; zero exactly when
// x_j = 0 or another point equals x_j
HD_FN void lagrange_weight(const uint32_t* X, uint32_t k, uint32_t j, uint32_t p[8]) {
    const uint32_t one[8] = FRS_R1_WORDS;
    uint32_t xj[8], d[8];
    copy(xj, X + 8 * (size_t)j);
    neg(p, xj);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (uint32_t i = 0; i < k; i++) {
        sub(d, xj, X + 8 * (size_t)i);
        if (i == j) copy(d, one);
        mul(p, p, d);
    }
}
// den = (sum_j shift_j)^-1 over the k shifts S (Montgomery form, 8 words each)
HD_FN void lagrange_den(const uint32_t* S, uint32_t k, uint32_t den[8]) {
    uint32_t acc[8];
    set_zero(acc);
    for (uint32_t i = 0; i < k; i++) add(acc, acc, S + 8 * (size_t)i);
    inv(den, acc);
}
// One group from end to end, serially (the host test's view of the steps k_lagrange spreads over lanes): x and out
// k x 32 bytes big-endian, work 16 k words (the points, then the shifts).  Returns the status: 1 coefficients written,
// 0 (and zeros written) where the reference asserts.
HD_FN int lagrange_group(const uint8_t* x, uint32_t k, uint32_t* work, uint8_t* out) {
    uint32_t* const X = work;
    uint32_t* const S = work + 8 * (size_t)k;
    bool ok = true;
    for (uint32_t j = 0; j < k; j++) ok = lagrange_point(x + 32 * (size_t)j, X + 8 * (size_t)j) && ok;
    for (uint32_t j = 0; j < k; j++) {
        uint32_t p[8];
        lagrange_weight(X, k, j, p);
        ok = ok && !is_zero(p);
        inv(S + 8 * (size_t)j, p);
    }
    uint32_t den[8];
    lagrange_den(S, k, den);
    for (uint32_t j = 0; j < k; j++) {
        uint32_t l[8];
        mul(l, S + 8 * (size_t)j, den);
        from_mont(l, l);
        if (!ok) set_zero(l);
        to_be(l, out + 32 * (size_t)j);
    }
    return ok ? 1 : 0;
}
// t = L (y mod n) for a coefficient L (32 bytes big-endian, below n) and any y < 2^256: one term of interpolate_at_zero
HD_FN void dot_term(const uint8_t* l_be, const uint8_t* y_be, uint32_t t[8]) {
    uint32_t l[8], y[8];
    from_be(l_be, l);
    from_be(y_be, y);
    hdk::reduce_n(y);
    to_mont(l, l);
    mul(t, l, y);                                          // (L R) y / R
}

// ---- the same for SECRET operands (coefficients of a dealing, shares, keys) ----------------------------------------------
// The last subtraction of every step is always computed and kept by a mask (hdk::sub_n_if_ge_masked): no branch, no ?:,
// no early exit and no address that depends on an operand.  frs::sub above is already of this kind.  Values equal those of
// mul / add / dot_term for every input (tests/test_frsecret_host.py).
// mul's operand scanning (straight-line code that looks at no value) with the masked last subtraction
HD_FN void mul_masked(uint32_t r[8], const uint32_t a[8], const uint32_t b[8]) {
    const uint32_t nw[8] = HD_N_WORDS;
    uint32_t t[9];
#pragma unroll
    for (int j = 0; j < 9; j++) t[j] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            c += (uint64_t)a[j] * b[i] + t[j];
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        t[8] = (uint32_t)c;
        const uint32_t m = 0u - t[0];                      // -n^-1 = -1 mod 2^32
        c = ((uint64_t)m * nw[0] + t[0]) >> 32;
#pragma unroll
        for (int j = 1; j < 8; j++) {
            c += (uint64_t)m * nw[j] + t[j];
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        t[7] = t[8] + (uint32_t)c;
    }
    hdk::sub_n_if_ge_masked(t);
    copy(r, t);
}
HD_FN void add_masked(uint32_t r[8], const uint32_t a[8], const uint32_t b[8]) { hdk::add_mod_n_masked(r, a, b); }
HD_FN void to_mont_masked(uint32_t r[8], const uint32_t a[8]) {
    const uint32_t r2[8] = FRS_R2_WORDS;
    mul_masked(r, a, r2);
}
HD_FN void from_mont_masked(uint32_t r[8], const uint32_t a[8]) {
    uint32_t one[8];
    set_zero(one);
    one[0] = 1;
    mul_masked(r, a, one);
}
// dot_term for a PUBLIC coefficient L (below n) and a SECRET y < 2^256
HD_FN void dot_term_masked(const uint8_t* l_be, const uint8_t* y_be, uint32_t t[8]) {
    uint32_t l[8], y[8];
    from_be(l_be, l);
    from_be(y_be, y);
    hdk::reduce_n_masked(y);
    to_mont(l, l);                                         // L is public
    mul_masked(t, l, y);
}

// ---- a player's share: the sum of the fragments it was dealt, sum_j y_j mod n for SECRET y_j below 2^256 ------------------
// acc = acc + (y mod n) for a canonical acc: one masked reduction, one masked addition (no Montgomery form, no product)
HD_FN void sum_term_masked(const uint8_t* y_be, uint32_t acc[8]) {
    uint32_t y[8];
    from_be(y_be, y);
    hdk::reduce_n_masked(y);
    add_masked(acc, acc, y);
}
// One group of k values (32 bytes big-endian each), serially (the host test's view of what k_fr_sum_secret spreads over
// lanes): out = the canonical sum, 32 bytes big-endian.
HD_FN void sum_group_masked(const uint8_t* y, size_t k, uint8_t* out) {
    uint32_t acc[8];
    set_zero(acc);
    for (size_t j = 0; j < k; j++) sum_term_masked(y + 32 * j, acc);
    to_be(acc, out);
}

// ---- a dealing's fragments: P(x) = sum_k c_k x^k mod n for SECRET coefficients and PUBLIC points ---------------------------
// a coefficient (32 bytes big-endian, any value below 2^256) reduced and in Montgomery form
HD_FN void poly_coeff_masked(const uint8_t* be, uint32_t cm[8]) {
    uint32_t c[8];
    from_be(be, c);
    hdk::reduce_n_masked(c);
    to_mont_masked(cm, c);
}
// a point (a player number: public, so the reduction may branch), reduced and in Montgomery form
HD_FN void poly_point(const uint8_t* be, uint32_t xm[8]) {
    uint32_t x[8];
    from_be(be, x);
    hdk::reduce_n(x);
    to_mont(xm, x);
}
// Horner from the top coefficient over the t >= 1 coefficients C (Montgomery form, 8 words each): t - 1 masked products
// and additions; step k reads coefficient k, whatever the values.  r: canonical, not in Montgomery form.
HD_FN void poly_horner_masked(const uint32_t* C, uint32_t t, const uint32_t xm[8], uint32_t r[8]) {
    uint32_t acc[8];
    copy(acc, C + 8 * (size_t)(t - 1));
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (uint32_t k = t - 1; k-- > 0;) {
        mul_masked(acc, acc, xm);
        add_masked(acc, acc, C + 8 * (size_t)k);
    }
    from_mont_masked(r, acc);
}
// One polynomial at n_x points, serially (the host test's view of what k_fr_poly_eval_secret spreads over lanes): coeffs
// t x 32 bytes, x and out n_x x 32 bytes big-endian, work 8 t words.
HD_FN void poly_eval_masked(const uint8_t* coeffs, uint32_t t, const uint8_t* x, uint32_t n_x, uint32_t* work, uint8_t* out) {
    for (uint32_t k = 0; k < t; k++) poly_coeff_masked(coeffs + 32 * (size_t)k, work + 8 * (size_t)k);
    for (uint32_t j = 0; j < n_x; j++) {
        uint32_t xm[8], r[8];
        poly_point(x + 32 * (size_t)j, xm);
        poly_horner_masked(work, t, xm, r);
        to_be(r, out + 32 * (size_t)j);
    }
}

}  // namespace frs
