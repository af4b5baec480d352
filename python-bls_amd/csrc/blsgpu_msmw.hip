// blsgpu_msmw.hip -- the WIDE tail of the sorted-bucket and plain sums in G1 and G2 (round 5): result = sum_i 2^(c i) P_i over a
// short list of projective points, Horner from the top -- the last folds (c = 0), the window sums W_w = sum_b 2^b S_(w,b) (c = 1, one
// wavefront per window) and the sum over the windows sum_w 2^(13 w) W_w (c = 13, one wavefront) of BLS.aggregate_pub_keys(secure)
// and BLS.aggregate_sigs(secure) at scale (bls.py:203-261; the reference's double-and-add summed over the points,
// fields_t.py:705-740).  247 doublings and 19 additions of ONE point are a dependent chain; the wavefront VM ran it on one team with
// every linear combination a round of its own (k_msm_pip_horner<1>: 1.31 ms of a 6.2 ms G1 sum, k_srt_windows another 0.14).
// Included by blsgpu_api.hip after blsgpu_mlw.hip and blsgpu_h2cw.hip.
//
// The machine is k_miller_wide's (blsgpu_mlw.hip: the LDS value file, mlw::wstep<1>: one product per lane, quad sum, scale, a
// multiple of q taken off in the carry pass) and the formulas are DATA: a complete doubling and a complete addition
// (Renes-Costello-Batina, a = 0) in two steps each -- infinity (0 : 1 : 0) anywhere in the list, a doubling inside an addition and
// P + (-P) need no branch, as in csrc/fp28.h pdbl / padd, whose results these are as projective points.  One kernel, two sets of
// constants (HornerCfg): G1 on its own tables (g1w_tables_gfx950.h from vmgen/g1w_model.py; tests/test_g1w_model.py runs them digit
// by digit against the host's integer curve arithmetic), G2 on the tables of the hash clearing (h2cw_tables_gfx950.h: its
// DBL1 / DBL2 / ADD1_0p / ADD2 on the accumulator and slot point 0; vmgen/h2cw_model.horner is this loop on the tables,
// tests/test_h2cw_model.py).  tests/test_gpu_msm.py runs the kernel behind every large sum against the reference's sums.
#pragma once
#include "g1w_tables_gfx950.h"

namespace blsgpu {
namespace msmw {
using r28::fe;
using r28::NL;

// NC coordinates per point (G2: X.re X.im Y.re Y.im Z.re Z.im), the value file, the step records and where the accumulator and
// the addend live in it (coordinate c at + 16 c, its four multiples 4 bytes apart)
template <int DEG> struct HornerCfg;
template <> struct HornerCfg<1> {
    static constexpr uint32_t NC = 3;
    static constexpr int VF_DW = G1W_PAGES * MLW_PAGE_BYTES / 4;
    static constexpr const uint32_t (&REC)[G1W_KINDS][5][64] = G1W_REC;
    static constexpr uint32_t DBL1 = G1W_DBL1, DBL2 = G1W_DBL2, ADD1 = G1W_ADD1, ADD2 = G1W_ADD2;
    static constexpr uint32_t ACC = G1W_AT_AX, ADDEND = G1W_AT_SX;
};
template <> struct HornerCfg<2> {
    static constexpr uint32_t NC = 6;
    static constexpr int VF_DW = h2cw::VF_DW;
    static constexpr const uint32_t (&REC)[H2CW_KINDS][5][64] = H2CW_REC;
    static constexpr uint32_t DBL1 = H2CW_KIND_DBL1, DBL2 = H2CW_KIND_DBL2, ADD1 = H2CW_KIND_ADD1_0p, ADD2 = H2CW_KIND_ADD2;
    static constexpr const uint32_t &ACC = H2CW_POINT[0], &ADDEND = H2CW_POINT[1];      // (the clearing's accumulator and slot point 0)
};

// in: gridDim.x lists of npts projective points in the L28 form (NC x 14 dwords: blsgpu_msm.hip L28_PJ; index 0 the lowest term);
// list g -> sum_i 2^(cbits i) in[g][i].  AFFINE = 0: out = the sum in the same form; AFFINE = 1: out = 96 DEG bytes canonical affine
// per list (x, y -- in G2 x.c0, x.c1, y.c0, y.c1 -- big-endian), (0, 0) and out_inf[g] = 1 for infinity (what k_msm_pip_horner writes).
template <int DEG, int AFFINE>
__global__ void __launch_bounds__(64) k_msm_horner_wide(const uint32_t* __restrict__ in, uint32_t npts, uint32_t cbits, uint32_t* __restrict__ out,
                                                        uint8_t* __restrict__ out_inf)
#if BLSGPU_EMIT(BLSGPU_TU_FXW)
{
    typedef HornerCfg<DEG> C;
    constexpr uint32_t NC = C::NC, PJ_DW = NC * NL;
    __shared__ int32_t vfile[C::VF_DW];
    char* vf = reinterpret_cast<char*>(vfile);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = blockIdx.x;
    for (uint32_t i = lane; i < (uint32_t)C::VF_DW; i += 64u) vfile[i] = 0;
    // quad c < NC stores coordinate c of a point in its four multiples
    const uint32_t qd = lane >> 2, vr = lane & 3u;
    const int32_t variant = mlw::quad_variant(lane);
    const uint32_t* P = in + (size_t)g * npts * PJ_DW + (qd < NC ? qd : 0u) * NL;
    int32_t t[NL], V[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) t[j] = (int32_t)P[(size_t)(npts - 1u) * PJ_DW + j];
    mlw::srn(V, t, variant);
    __syncthreads();                                              // (one wavefront: the zeroing above is done before anything is stored)
    if (qd < NC) mlw::st14(vf, C::ACC + 16u * qd + 4u * vr, V);
    const mlw::Rec d1 = mlw::load_rec(C::REC, C::DBL1, lane), d2 = mlw::load_rec(C::REC, C::DBL2, lane), a1 = mlw::load_rec(C::REC, C::ADD1, lane),
                   a2 = mlw::load_rec(C::REC, C::ADD2, lane);
#pragma unroll 1
    for (int i = (int)npts - 2; i >= 0; i--) {
#pragma unroll
        for (int j = 0; j < NL; j++) t[j] = (int32_t)P[(size_t)i * PJ_DW + j];            // (in flight behind the doublings)
#pragma unroll 1
        for (uint32_t s = 0; s < cbits; s++) {
            mlw::wstep<1, false>(vf, d1);
            mlw::wstep<1, false>(vf, d2);
        }
        mlw::srn(V, t, variant);
        if (qd < NC) mlw::st14(vf, C::ADDEND + 16u * qd + 4u * vr, V);
        mlw::wstep<1, false>(vf, a1);
        mlw::wstep<1, false>(vf, a2);
    }
    if (!AFFINE) {
        if (qd < NC && vr == 0u) {
            const fe c = mlw::ld_fe(vf, C::ACC + 16u * qd);
#pragma unroll
            for (int j = 0; j < NL; j++) out[(size_t)g * PJ_DW + qd * NL + j] = (uint32_t)c.v[j];
        }
        return;
    }
    // affine: lane k < 2 DEG holds part k of (x, y) = (X, Y) / Z, Z = 0 gives (0, 0)
    constexpr uint32_t PARTS = 2 * DEG;
    fe a;
    if (DEG == 1) {
        // every lane holds the same Z: the variable-time division steps of fq32.h (data-dependent control flow is free when the
        // data is wave-uniform)
        const fe z = mlw::ld_fe(vf, C::ACC + 32u);
        uint32_t zv[12], ziv[12];
        r28::to_vm(zv, z);
        bls::fq_inv_var(ziv, zv);
        a = r28::mul(mlw::ld_fe(vf, C::ACC + 16u * (lane & 1u)), r28::from_vm(ziv));
    } else {
        a = h2cw::affine_part(vf, C::ACC, lane & 3u);
    }
    uint32_t y[12];
    r28::to_raw(y, a);
    uint32_t any = 0;
#pragma unroll
    for (int w = 0; w < 12; w++) {
        any |= y[w];
        if (lane < PARTS) out[(size_t)g * (12 * PARTS) + lane * 12u + w] = bswap32(y[11 - w]);
    }
    const uint64_t nz = __ballot(any != 0u && lane < PARTS);
    if (out_inf && lane == 0u) out_inf[g] = nz == 0 ? 1 : 0;
}
#else
;
#endif

#if BLSGPU_TU == BLSGPU_TU_FXW
__attribute__((used)) static const void* const blsgpu_instances_msmw[] = {(const void*)&k_msm_horner_wide<1, 0>, (const void*)&k_msm_horner_wide<1, 1>,
                                                                          (const void*)&k_msm_horner_wide<2, 0>, (const void*)&k_msm_horner_wide<2, 1>};
#endif
}  // namespace msmw
}  // namespace blsgpu
