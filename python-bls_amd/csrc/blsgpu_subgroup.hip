// blsgpu_subgroup.hip -- batched membership tests of the order-n subgroups G1 and G2, one affine point per lane (included by
// blsgpu_api.hip, built with blsgpu_g1fix.hip / blsgpu_g1poly.hip in translation unit 8).
//
// Status per point: 1 on the curve and in the order-n subgroup (infinity, the all-zero encoding, included), 2 on the curve
// but outside it, 0 off the curve.  Both tests compare an endomorphism of P with a short scalar multiple of P (Scott, "A note
// on group membership tests for G1, G2 and GT on BLS pairing-friendly curves", 2021), u = -0xd201000000010000:
//   k_g1_subgroup   phi(P) == -[u^2] P with phi(x, y) = (beta x, y): 127 doublings and 16 mixed additions over the bits
//                   of u^2 (against 254 doublings and 127 additions for [n] P, k_poly_subgroup);
//   k_g2_subgroup   psi(Q) == [u] Q = -[|u|] Q with psi(x, y) = (conj(x) psi_x, conj(y) psi_y): 63 doublings and 5 mixed
//                   additions on the twist.  psi_x, psi_y are the cofactor clearing's constants (BLSVM_HC_PSIX / _PSIY of
//                   the VM constant table, blsgpu_h2c.hip).
// Which cube root beta goes with -u^2 is a sign convention; it and the direction of psi are pinned against [n] P == O on the
// host (tests/test_subgroup_host.py).  The RCB formulas of fp28.h are complete on the whole curve (no point of order 2), so
// points outside the subgroup and a multiple that reaches infinity need no branch; the comparison is projective
// (cross-multiplied), with no inversion.  A multiple at infinity is never equal: P != O, so phi(P) != O and psi(Q) != O,
// and (0 : Y : 0) with Y != 0 fails the y comparison.  The loops follow the public bits of u: every lane runs the same
// instructions.
#pragma once

namespace blsgpu {
namespace subgroup {

constexpr uint32_t U2_WORDS[4] = {0x00000000u, 0x00000001u, 0x0001a402u, 0xac45a401u};   // u^2, little-endian words
constexpr int U2_TOP = 127;                                                              // its highest set bit
constexpr uint32_t U_WORDS[2] = {0x00010000u, 0xd2010000u};                              // |u|
constexpr int U_TOP = 63;
// beta: the cube root of unity in Fq with phi(P) = -[u^2] P on G1 (little-endian words of the plain integer)
constexpr uint32_t BETA_WORDS[12] = {0xfffefffeu, 0x2e01ffffu, 0x620a0002u, 0xde17d813u, 0xe6f89688u, 0xddb3a93bu,
                                     0x6a0f77eau, 0xba69c607u, 0xdf76ce51u, 0x5f19672fu, 0x00000000u, 0x00000000u};

// 12 big-endian words at p -> an element of L28 (any value below 2^384, reduced mod q)
__device__ __forceinline__ r28::fe ld_be(const uint32_t* __restrict__ p) {
    uint32_t x[12];
#pragma unroll
    for (int w = 0; w < 12; w++) x[11 - w] = bswap32(p[w]);
    return r28::from_raw(x);
}
__device__ __forceinline__ bool same(const r28::fe& a, const r28::fe& b) {
    const r28::fe x = r28::canon(a), y = r28::canon(b);
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < r28::NL; j++) d |= (uint32_t)(x.v[j] ^ y.v[j]);
    return d == 0;
}
__device__ __forceinline__ bool same(const r28::fe2& a, const r28::fe2& b) { return same(a.a, b.a) && same(a.b, b.b); }

// n affine G1 points (96 bytes each, (0, 0) = infinity) -> n status bytes
__global__ void __launch_bounds__(256) k_g1_subgroup(const uint32_t* __restrict__ pts, uint32_t n, uint8_t* __restrict__ status)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    using namespace r28;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* a = pts + (size_t)i * 24;
    uint32_t z = 0;
#pragma unroll
    for (int w = 0; w < 24; w++) z |= a[w];
    if (z == 0) { status[i] = 1; return; }
    const fe x = ld_be(a), y = ld_be(a + 12);
    const fe one = fe_one(), four = norm(mulc<4>(one));
    if (!same(sqr(y), dot2(sqr(x), x, four, one))) { status[i] = 0; return; }    // y^2 = x^3 + 4
    ptT<fe> R = pt_inf<fe>();
    pmadd(R, x, y);                                                          // the top bit of u^2
#pragma unroll 1
    for (int b = U2_TOP - 1; b >= 0; b--) {
        R = pdbl(R);
        if ((U2_WORDS[b >> 5] >> (b & 31)) & 1u) pmadd(R, x, y);
    }
    // (beta x, y) == -(X : Y : Z)  <=>  X = beta x Z  and  -Y = y Z
    uint32_t braw[12];
#pragma unroll
    for (int w = 0; w < 12; w++) braw[w] = BETA_WORDS[w];
    const fe bx = mul(from_raw(braw), x), ny = norm(neg(y));
    status[i] = same(R.X, mul(bx, R.Z)) && same(R.Y, mul(ny, R.Z)) ? 1 : 2;
}
#else
;
#endif

// n affine G2 points (192 bytes each: x.c0 x.c1 y.c0 y.c1, all zero = infinity) -> n status bytes
__global__ void __launch_bounds__(256) k_g2_subgroup(VmTables T, const uint32_t* __restrict__ pts, uint32_t n, uint8_t* __restrict__ status)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    using namespace r28;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* a = pts + (size_t)i * 48;
    uint32_t z = 0;
#pragma unroll
    for (int w = 0; w < 48; w++) z |= a[w];
    if (z == 0) { status[i] = 1; return; }
    const fe2 x = {ld_be(a), ld_be(a + 12)}, y = {ld_be(a + 24), ld_be(a + 36)};
    const fe one = fe_one(), four = norm(mulc<4>(one));
    const fe2 b = {four, four}, one2 = fe2_one();                            // b' = 4 (1 + u)
    if (!same(sqr(y), dot2(sqr(x), x, b, one2))) { status[i] = 0; return; }     // y^2 = x^3 + 4 (1 + u)
    ptT<fe2> R = pt_inf<fe2>();
    pmadd(R, x, y);                                                          // the top bit of |u|
#pragma unroll 1
    for (int k = U_TOP - 1; k >= 0; k--) {
        R = pdbl(R);
        if ((U_WORDS[k >> 5] >> (k & 31)) & 1u) pmadd(R, x, y);
    }
    // psi(Q) == [u] Q = -(X : Y : Z)  <=>  X = psi_x conj(x) Z  and  -Y = psi_y conj(y) Z
    constexpr uint32_t PSIX = BLSVM_HC_PSIX - BLSVM_HC_SLOT0 + BLSVM_HC_TBL0, PSIY = BLSVM_HC_PSIY - BLSVM_HC_SLOT0 + BLSVM_HC_TBL0;
    const uint32_t* cx = T.consts + PSIX * 12;
    const uint32_t* cy = T.consts + PSIY * 12;
    const fe2 psx = {from_vm(cx), from_vm(cx + 12)}, psy = {from_vm(cy), from_vm(cy + 12)};
    const fe2 px = mul(conj(x), psx), npy = norm(neg(mul(conj(y), psy)));
    status[i] = same(R.X, mul(px, R.Z)) && same(R.Y, mul(npy, R.Z)) ? 1 : 2;
}
#else
;
#endif

}  // namespace subgroup
}  // namespace blsgpu
