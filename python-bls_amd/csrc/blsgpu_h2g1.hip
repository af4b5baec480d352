// blsgpu_h2g1.hip -- hash to G1, one message per lane, everything in registers on the 28-bit limbs of fp28.h (included by
// blsgpu_api.hip after blsgpu_h2c.hip, built in its translation unit).
//
// The batch form of the reference's hash_to_point_prehashed_Fq (ec.py:511-520), bls_py/hostmath.py hash_to_g1_prehashed:
//   t_j = int(hash512(m || "G1_j")) mod q, j = 0, 1        k_h2g1<1> only: four one-block SHA-256 compressions of 37-byte
//                                                          messages, hash512(x) = sha256(x || 00) || sha256(x || 01); the
//                                                          512-bit value is reduced as lo + hi 2^384 (k_h2c_swj0's rule)
//   P = sw_encode(t_0) + sw_encode(t_1)                    ec.py:449-507 over Fq, below
//   out = h P, h = 0x396c8c005555e1568c00aaab0000aaab      over the public bits of h: 125 doublings, 47 additions
// k_h2g1<0> takes t_0 || t_1 as 48-byte big-endian integers; any value below 2^384 is taken mod q (r28::from_raw).
//
// sw_encode(t), with its control flow as selects (every lane runs the same instructions):
//   t = 0 -> infinity;  parity = t > q - t;  w = t^2 + 5;  w = 0 -> the generator, negated when parity is set (reachable:
//   -5 is a square mod q);  otherwise w' = s t / w, x1 = -w' t + (s - 1)/2, x2 = -1 - x1, x3 = 1/w'^2 + 1 with s = sqrt(-3);
//   x = the first of x1, x2 whose x^3 + 4 is a square, else x3;  y = the root of x^3 + 4 with (y > q // 2) == parity.
//   x^3 + 4 = 0 does not occur (no point of order 2), so the character is never 0 for a candidate.
// Inversions: 1/w and 1/t of BOTH encodings come from ONE inversion of (w_0 t_0)(w_1 t_1) -- 1/w = t / (w t), 1/w' = w^2 / (s (w t))
// -- with a factor w_j t_j = 0 (the infinity and generator cases, which use neither quotient) replaced by 1; a second
// inversion gives the affine result, Z = 0 -> (0, 0).  Characters: the Jacobi symbol of swl::chi for x1 and x2 (x3 is taken
// unseen, as in the reference); ONE fixed power u^((q-3)/4) per encoding for the root y = u u^((q-3)/4) of the chosen x.
// The sum and the multiplication use the complete formulas of fp28.h (padd, pdbl): infinity, equal and opposite encodings
// take the same path as everything else.
//
// NOT constant-time: every input is public data (message hashes, field elements); the Jacobi routine and nothing else
// here has a data-dependent trip count.
#pragma once

namespace blsgpu {
namespace h2g1 {
using r28::fe;

constexpr uint32_t H_WORDS[4] = {0x0000aaabu, 0x8c00aaabu, 0x5555e156u, 0x396c8c00u};   // the cofactor h, little-endian words
constexpr int H_TOP = 125;                                                              // its highest set bit

__device__ __forceinline__ fe sel(bool c, const fe& a, const fe& b) {
    fe r;
#pragma unroll
    for (int l = 0; l < r28::NL; l++) r.v[l] = c ? a.v[l] : b.v[l];
    return r;
}

// b^((q-3)/4): the sliding-window schedule of k_pow (BLSVM_POW_WIN), odd powers in registers
__device__ __forceinline__ fe pow_e(const fe& b) {
    constexpr int NT = 1 << (BLSVM_POW_WINDOW - 1);
    fe tbl[NT];
    tbl[0] = b;
    const fe t = r28::sqr(b);
#pragma unroll
    for (int i = 1; i < NT; i++) tbl[i] = r28::mul(tbl[i - 1], t);
    auto pick = [&](uint32_t k) {
        fe m = tbl[0];
#pragma unroll
        for (int i = 1; i < NT; i++) m = sel(k == (uint32_t)i, tbl[i], m);
        return m;
    };
    fe a = pick(BLSVM_POW_WIN[0][1]);
#pragma unroll 1
    for (int s = 1; s < BLSVM_POW_STEPS; s++) {
        const uint32_t nsq = BLSVM_POW_WIN[s][0], k = BLSVM_POW_WIN[s][1];
#pragma unroll 1
        for (uint32_t i = 0; i < nsq; i++) a = r28::sqr(a);
        if (k != 255u) a = r28::mul(a, pick(k));
    }
    return a;
}

// t_j of message i: 12 big-endian words (HASH = 0) or the 512-bit hash512(m || "G1_j") (HASH = 1), as a value in (-q, 2q)
template <int HASH>
__device__ __forceinline__ fe field_element(const uint32_t* __restrict__ in, uint32_t i, uint32_t j) {
    uint32_t lo[12];
    if (HASH) {
        uint32_t w[16], be[16];
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = bswap32(in[(size_t)i * 8 + k]);
        w[8] = 0x47315F00u | (0x30u + j);                   // 'G' '1' '_' ('0' + j)
        w[10] = 0; w[11] = 0; w[12] = 0; w[13] = 0; w[14] = 0;
        w[15] = 296;                                        // 37 bytes, in bits
        w[9] = 0x00800000u;                                 // the hash512 selector byte (00, then 01), then the 0x80 padding byte
        sha256_block(w, be);
        w[9] = 0x01800000u;
        sha256_block(w, be + 8);
        uint32_t hi[12];
#pragma unroll
        for (int k = 0; k < 12; k++) { lo[k] = be[15 - k]; hi[k] = k < 4 ? be[3 - k] : 0u; }
        const int32_t c2[r28::NL] = BLS28_WIDE_C2;
        return swl::red(r28::add(r28::from_raw(lo), r28::mul(r28::unpack32(hi), r28::fe_const(c2))));
    }
    const uint32_t* src = in + (size_t)i * 24 + j * 12;
#pragma unroll
    for (int k = 0; k < 12; k++) lo[k] = bswap32(src[11 - k]);
    return r28::from_raw(lo);
}

// in: n x 96 bytes t_0 || t_1 (HASH = 0) or n x 32-byte message hashes (HASH = 1).  out_aff (n x 96 bytes, (0, 0) for
// infinity), out_ser (n x 48 bytes, k_fix_mul's compression) and out_inf (n flag bytes) may each be NULL.
template <int HASH>
__global__ void __launch_bounds__(256) k_h2g1(g1fix::Gen g, const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out_aff,
                                              uint32_t* __restrict__ out_ser, uint8_t* __restrict__ out_inf)
#if BLSGPU_EMIT(BLSGPU_TU_H2C)
{
    using namespace r28;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t s3c[NL] = BLS28_SW_S3, hhc[NL] = BLS28_SW_HH, sic[NL] = BLS28_SW_SINV;
    const fe one = fe_one(), zero = fe_zero(), five = norm(mulc<5>(one)), four = norm(mulc<4>(one));

    // both field elements, w = t^2 + 5 and the factors w t of the shared inversion
    fe t0 = zero, t1 = zero, w0 = zero, w1 = zero, a0 = one, a1 = one;
#pragma unroll 1
    for (uint32_t j = 0; j < 2; j++) {
        const fe t = field_element<HASH>(in, i, j);
        const fe w = swl::red(add(sqr(t), five));
        const fe a = sel(is_zero(t) || is_zero(w), one, mul(w, t));
        t0 = sel(j == 0, t, t0); t1 = sel(j == 0, t1, t);
        w0 = sel(j == 0, w, w0); w1 = sel(j == 0, w1, w);
        a0 = sel(j == 0, a, a0); a1 = sel(j == 0, a1, a);
    }
    const fe inv01 = swl::inv(mul(a0, a1));
    const fe gx = from_raw(g.x), gy = from_raw(g.y);

    ptT<fe> acc = pt_inf<fe>();
#pragma unroll 1
    for (uint32_t j = 0; j < 2; j++) {
        const fe t = sel(j == 0, t0, t1), w = sel(j == 0, w0, w1);
        const fe iwt = mul(inv01, sel(j == 0, a1, a0));                     // 1 / (w t)
        const bool tz = is_zero(t), wz = is_zero(w), parity = swl::sgn(t);
        const fe wp = mul(mul(mul(iwt, t), t), fe_const(s3c));              // w' = s t / w
        const fe x1 = norm(sub(fe_const(hhc), mul(wp, t)));
        const fe x2 = norm(sub(neg(one), x1));
        const fe wpi = mul(mul(mul(iwt, w), w), fe_const(sic));             // 1 / w' = w / (s t)
        const fe x3 = norm(add(sqr(wpi), one));
        // the first of x1, x2 whose x^3 + 4 is a square, else x3 (ec.py:489-500)
        fe x = x3, u = swl::red(add(mul(sqr(x3), x3), four));
#pragma unroll 1
        for (int k = 1; k >= 0; k--) {                                      // x2, then x1: x1 overrides
            const fe xc = k == 0 ? x1 : x2;
            const fe uc = swl::red(add(mul(sqr(xc), xc), four));
            const bool sq = swl::chi(uc) == 1;
            x = sel(sq, xc, x); u = sel(sq, uc, u);
        }
        fe y = mul(pow_e(u), u);                                            // u^((q+1)/4)
        y = sel(swl::sgn(y) != parity, norm(neg(y)), y);
        // w = 0: the generator, negated when parity is set; t = 0: infinity (0 : 1 : 0)
        x = sel(wz, gx, x);
        y = sel(wz, sel(parity, norm(neg(gy)), gy), y);
        const ptT<fe> Q = {sel(tz, zero, x), sel(tz, one, y), sel(tz, zero, one)};
        acc = padd(acc, Q);
    }

    // h (P_0 + P_1) over the bits of h
    const ptT<fe> P = acc;
#pragma unroll 1
    for (int b = H_TOP - 1; b >= 0; b--) {
        acc = pdbl(acc);
        if ((H_WORDS[b >> 5] >> (b & 31)) & 1u) acc = padd(acc, P);
    }
    uint32_t x[12], y[12];
    g1fix::to_affine_raw(acc, x, y);
    if (out_inf) {
        uint32_t any = 0;
#pragma unroll
        for (int k = 0; k < 12; k++) any |= x[k] | y[k];
        out_inf[i] = any ? 0 : 1;
    }
    g1fix::store_result(x, y, i, out_aff, out_ser);
}
#else
;
#endif
#if BLSGPU_TU == BLSGPU_TU_H2C          // the instantiations the host side launches: this translation unit emits them (blsgpu_tu.h)
__attribute__((used)) static const void* const blsgpu_instances_h2g1[] = {(const void*)&k_h2g1<0>, (const void*)&k_h2g1<1>};
#endif

}  // namespace h2g1
}  // namespace blsgpu
