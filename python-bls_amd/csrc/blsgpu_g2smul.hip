// blsgpu_g2smul.hip -- G2 scalar multiplication with a schedule that does not look at the scalar: out_i = s_i P_i, one scalar
// per LANE PAIR on sp2's point arithmetic (blsgpu_msm.hip), for blsgpu_g2_mul_secret and blsgpu_sign (included by
// blsgpu_api.hip).  The schedule, the claim and its limits are secret_window.h's; vmgen/g2smul_model.py is the specification
// (tests/test_g2smul_model.py).  Particular to this kernel:
//   table      1P .. 8P per scalar in the L28 projective form (k_g2_smul_table: seven complete additions of P), dword j of
//              entry e of lane t at table[(e 42 + j) stride + t]: the lanes of a wavefront read consecutive dwords (vector
//              loads, a loop of eight rounds).  When every scalar multiplies the same point the table is built once
//              (stride 2) and every pair reads the same entries.
//   window     from the top window down, four complete doublings (RCB algorithm 9), then ONE complete addition (algorithm
//              7) of the selected entry; a zero digit selects nothing and ORs in the constant (0 : 1 : 0) -- the complete
//              addition makes that a no-op.  260 doublings and 65 additions for every scalar.
//   input      an input point (0, 0) enters as (0 : 1 : 0) by select (the point is public all the same).
//   output     (X, Y) / Z through the norm of Z and fq_inv; the compression of Signature.serialize() (ec.py:94-111) is done
//              here by masks.  Nothing is claimed about H(m): the message-dependent hash to G2 that blsgpu_sign runs first
//              is public and keeps its own kernels.  The scalars are the `scalars` of blsgpu_g2_msm.
//
// Slices: a launch takes at most SLICE = 65 536 scalars (two wavefronts on every SIMD of the chip), so the table
// workspace is bounded by 65 536 x 2688 bytes = 168 MiB whatever the size of the call.
#pragma once

#include "secret_window.h"

namespace blsgpu {
namespace g2smul {
using namespace sp2;
using swin::TAB;

constexpr uint32_t PT_DW = 3 * r28::NL;                       // a lane's half of a projective point: X, Y, Z
constexpr uint32_t TABLE_DW = TAB * 2 * PT_DW;                // dwords of one pair's table
constexpr uint32_t PAIRS = 128;                               // lane pairs per 256-thread workgroup
constexpr size_t SLICE = 65536;                               // scalars per launch

// table of point u (n_tab points, 192 bytes affine big-endian each, (0, 0) = infinity): entry e = (e + 1) P
__global__ void __launch_bounds__(256, 2) k_g2_smul_table(const uint32_t* __restrict__ pts, uint32_t n_tab, uint32_t* __restrict__ table)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t u = min(tid >> 1, n_tab - 1u), part = tid & 1u;
    const bool store = (tid >> 1) < n_tab;
    const uint32_t* sx = pts + (size_t)u * 48 + part * 12;
    const uint32_t* sy = sx + 24;
    uint32_t any = 0;
#pragma unroll
    for (int w = 0; w < 12; w++) any |= sx[w] | sy[w];
    any |= (uint32_t)__shfl_xor((int)any, 1);
    const bool inf = any == 0u;
    const h x = load_part(sx), y = load_part(sy);
    const int32_t one[r28::NL] = BLS28_ONE;
    pt P;
#pragma unroll
    for (int j = 0; j < r28::NL; j++) {
        const int32_t o = odd() ? 0 : one[j];
        P.X.v[j] = inf ? 0 : x.v[j];
        P.Y.v[j] = inf ? o : y.v[j];
        P.Z.v[j] = inf ? 0 : o;
    }
    const size_t stride = 2 * (size_t)n_tab;
    uint32_t* T = table + 2 * (size_t)u + part;
    pt acc = P;
#pragma unroll 1
    for (uint32_t e = 0; e < TAB; e++) {
        if (e) acc = padd(acc, P);
        const h* c[3] = {&acc.X, &acc.Y, &acc.Z};
        if (store) {
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
                for (int j = 0; j < r28::NL; j++) T[(size_t)(e * PT_DW + k * r28::NL + j) * stride] = (uint32_t)c[k]->v[j];
        }
    }
}
#else
;
#endif

// out_i = s_i (the table's point) for n <= SLICE scalars (32 bytes big-endian).  table / tstride: k_g2_smul_table's, of n
// points (tstride 2 n) or, shared != 0, of one point (tstride 2).  out_aff: n x 192 bytes ((0, 0) for infinity), out_ser: n x 96
// bytes (Signature.serialize(): x.c0 || x.c1 with 0x80 on the first byte when the imaginary part of y exceeds q // 2; zeros
// for infinity), out_inf: n flags; each may be NULL.
__global__ void __launch_bounds__(256, 2) k_g2_smul(const uint32_t* __restrict__ table, uint32_t tstride, uint32_t shared,
                                                   const uint32_t* __restrict__ scalars, uint32_t n, uint32_t* __restrict__ out_aff,
                                                   uint32_t* __restrict__ out_ser, uint8_t* __restrict__ out_inf)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    __shared__ uint32_t rec[swin::REC_WORDS][PAIRS];
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t g = min(tid >> 1, n - 1u), part = tid & 1u, lp = threadIdx.x >> 1;
    const bool store = (tid >> 1) < n;
    swin::recode(rec, lp, scalars + (size_t)g * 8);                        // both lanes of the pair write the same words
    const uint32_t* T = table + (shared ? part : 2u * g + part);
    const int32_t one[r28::NL] = BLS28_ONE;
    pt acc = pt_inf();
#pragma unroll 1
    for (int w = (int)swin::WINDOWS - 1; w >= 0; w--) {
#pragma unroll 1
        for (int s = 0; s < 4; s++) acc = pdbl(acc);
        const swin::Digit d = swin::digit(rec, lp, (uint32_t)w);
        uint32_t q[PT_DW];
        swin::select_entry<PT_DW, false>(q, T, tstride, d.ad, 0u);
        pt Q;
#pragma unroll
        for (int j = 0; j < r28::NL; j++) {                                // zero digit: q = 0, (0 : 1 : 0)
            Q.X.v[j] = (int32_t)q[j];
            Q.Y.v[j] = (int32_t)(q[r28::NL + j] | ((uint32_t)(odd() ? 0 : one[j]) & d.mz));
            Q.Z.v[j] = (int32_t)q[2 * r28::NL + j];
        }
        const h yn = norm(neg(Q.Y));
#pragma unroll
        for (int j = 0; j < r28::NL; j++) Q.Y.v[j] = swin::sel(yn.v[j], Q.Y.v[j], d.sgn);
        acc = padd(acc, Q);
    }
    // affine: (X, Y) / Z with 1 / Z = conj(Z) / N(Z); Z = 0 gives (0, 0) (the tail of k_msm_horner_quads on a lane pair)
    const h zp = swp(acc.Z);
    r28::fe nz;
    bls28::fp28_dot2(nz.v, acc.Z.v, acc.Z.v, zp.v, zp.v);
    uint32_t nv[12], niv[12];
    r28::to_vm(nv, nz);
    bls::fq_inv(niv, nv);
    const r28::fe ninv = r28::from_vm(niv);
    S<1> zc;
#pragma unroll
    for (int j = 0; j < r28::NL; j++) zc.v[j] = part ? -acc.Z.v[j] : acc.Z.v[j];
    const h zi = mulf(zc, ninv);
    const Rop<1> rzi = right(zi);
    const h xa = mul(left(acc.X), rzi), ya = mul(left(acc.Y), rzi);
    r28::fe tx, ty;
#pragma unroll
    for (int j = 0; j < r28::NL; j++) { tx.v[j] = xa.v[j]; ty.v[j] = ya.v[j]; }
    uint32_t xr[12], yr[12];
    r28::to_raw(xr, tx);
    r28::to_raw(yr, ty);
    uint32_t any = 0;
#pragma unroll
    for (int w = 0; w < 12; w++) any |= xr[w] | yr[w];
    any |= (uint32_t)__shfl_xor((int)any, 1);
    if (out_aff && store) {
#pragma unroll
        for (int w = 0; w < 12; w++) {
            out_aff[(size_t)g * 48 + part * 12 + w] = bswap32(xr[11 - w]);
            out_aff[(size_t)g * 48 + (2 + part) * 12 + w] = bswap32(yr[11 - w]);
        }
    }
    if (out_inf && store && part == 0u) out_inf[g] = any ? 0 : 1;
    if (out_ser) {
        const uint32_t big = bls::gt_half_q_mask(yr);                          // the odd lane's decides: the imaginary part of y
        const uint32_t flag = (uint32_t)__shfl_xor((int)big, 1) & (part ? 0u : 0x80000000u);
        xr[11] |= flag;
        if (store) {
#pragma unroll
            for (int w = 0; w < 12; w++) out_ser[(size_t)g * 24 + part * 12 + w] = bswap32(xr[11 - w]);
        }
    }
}
#else
;
#endif

}  // namespace g2smul
}  // namespace blsgpu
