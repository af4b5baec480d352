// blsgpu_wide_check.hip -- TEST-ONLY device library (libblsgpu_widecheck.so): the step routines of the wide machine
// (mlw:: of blsgpu_mlw.hip, lsw:: of blsgpu_lsw.hip, fxw:: of blsgpu_fexpw.hip) as kernels of their own, operands, records and
// results as raw words in global memory, so that tests/test_gpu_wide.py can compare the COMPILED steps digit for digit with the
// integer model (tests/wide_vectors.py).  Not linked into libblsgpu.so, not declared in include/blsgpu.h, not an ABI.
//
// The routines are the production ones: this file includes the kernel texts the way blsgpu_api.hip does, with a BLSGPU_TU value
// no kernel group has, so no production kernel body is emitted (blsgpu_tu.h).  One kernel per op (a template on the op): each
// step shape is compiled the way the production kernels compile it.  The host function checks every address of every record
// against the value file before anything is launched (-4); the guard records and the return codes are check_runner.h's.
//
//   per lane (256 threads per workgroup, one item per lane):
//     SRN             t[14], s                      -> mlw::srn
//     FXW_SCALE_NORM  t[14], s                      -> fxw::scale_norm
//     STORED_ZERO     d[14]: written to slot (wavefront, lane) of an LDS value file  -> mlw::stored_zero, the 14 words of mlw::ld_fe
//   per wavefront, mlw (an item: a value file image of mlw::VF_DW dwords, then 5 x 64 record words, word i of all lanes side by side):
//     WSTEP_2 / WSTEP_2BS / WSTEP_1 / WSTEP_1OCT    one wavefront per workgroup -> the value file after mlw::wstep<K, BS, OCT>
//     WSTEP_2_X4 / WSTEP_1_X4                       four wavefronts per 256-thread workgroup, each on its own value file
//     TREC_<table>_<shape>  an image and a KIND: the record comes from mlw::load_rec on MLW_REC / H2CW_REC / G1W_REC (a kind past
//                     the table reads kind 0);  LREC_<shape>: the same for lstep through lsw::load_rec<K> on LSW_REC
//     WLOAD           an image, then 64 x 14 digits, 64 destinations and 64 factors sc: every lane stores sc x quad_variant(lane) x its value
//                     (mlw::srn, mlw::st14: how k_miller_wide, k_h2c_clear_wide and k_msm_horner_wide write their inputs)
//   line-stream steps (an item: an image of lsw::VF_DW dwords -- four pairs --, (2 K + 3) x 64 record words, one word: line record or none):
//     LSTEP_2 / LSTEP_3 / LSTEP_4 / LSTEP_4_HAS2 / LSTEP_2_HAS2 / LSTEP_3_HAS2   -> the image, then 4 x 84 words of line records
//   final-exponentiation steps (V, G: 64 x 14 digits in registers):
//     FXW_STEP_VV     V, P1 as 4 x 64 words         -> V          FXW_STEP_VG   V, G, P3 as 9 x 64 words -> V, G
//     FXW_VV_CSQ / FXW_VV_CONJ / FXW_VG_MUL / FXW_VG_FROB / FXW_VG_FROBC: the same through load_p1 / load_p3 on the real tables
//     FXW_TINV        V -> V
#include "check_runner.h"
#define BLSGPU_TU 99                                       // no kernel group: declarations only
#include "blsgpu_tu.h"
#include "blsgpu_kernels.hip"
#include "fp28.h"
#include "blsgpu_ml.hip"
#include "blsgpu_fexp.hip"
#include "blsgpu_fexpw.hip"
#include "blsgpu_mlw.hip"
#include "blsgpu_lsw.hip"
#include "h2cw_tables_gfx950.h"
#include "g1w_tables_gfx950.h"

namespace {
using namespace blsgpu;
using r28::NL;

// every op, once, with its code (tests/wide_vectors.py pins the codes)
#define WIDECHECK_OPS(X) \
    X(SRN, 0) X(FXW_SCALE_NORM, 1) X(STORED_ZERO, 2) \
    X(WSTEP_2, 10) X(WSTEP_2BS, 11) X(WSTEP_1, 12) X(WSTEP_1OCT, 13) X(WSTEP_2_X4, 14) X(WSTEP_1_X4, 15) X(WLOAD, 16) \
    X(LSTEP_2, 20) X(LSTEP_3, 21) X(LSTEP_4, 22) X(LSTEP_4_HAS2, 23) X(LSTEP_2_HAS2, 24) X(LSTEP_3_HAS2, 25) \
    /* the same steps with the record fetched by mlw::load_rec / lsw::load_rec<K> from the real tables: an item names a KIND */ \
    X(TREC_MLW_2, 40) X(TREC_MLW_2BS, 41) X(TREC_MLW_1, 42) X(TREC_MLW_1OCT, 43) X(TREC_H2CW_2, 44) X(TREC_H2CW_2BS, 45) X(TREC_H2CW_1, 46) \
    X(TREC_G1W_1, 47) \
    X(LREC_2, 50) X(LREC_3, 51) X(LREC_4, 52) X(LREC_4_HAS2, 53) X(LREC_2_HAS2, 54) X(LREC_3_HAS2, 55) \
    X(FXW_STEP_VV, 30) X(FXW_STEP_VG, 31) X(FXW_VV_CSQ, 32) X(FXW_VV_CONJ, 33) X(FXW_VG_MUL, 34) X(FXW_VG_FROB, 35) X(FXW_VG_FROBC, 36) \
    X(FXW_TINV, 37)
CHECK_ENUM(WIDECHECK_OPS)
constexpr int MVF = mlw::VF_DW, LVF = lsw::VF_DW, LINES_OUT = 4 * ml::LINE_DW, REGS = 64 * NL;

// words per item in and out, threads per workgroup, items per workgroup
template <int OP> struct Shape;
#define SHAPE(OP, WIN, WOUT, THREADS, PER) template <> struct Shape<OP> { static constexpr int win = WIN, wout = WOUT, threads = THREADS, per = PER; };
SHAPE(SRN, NL + 1, NL, 256, 256) SHAPE(FXW_SCALE_NORM, NL + 1, NL, 256, 256) SHAPE(STORED_ZERO, NL, NL + 1, 256, 256)
SHAPE(WSTEP_2, MVF + 320, MVF, 64, 1) SHAPE(WSTEP_2BS, MVF + 320, MVF, 64, 1) SHAPE(WSTEP_1, MVF + 320, MVF, 64, 1)
SHAPE(WSTEP_1OCT, MVF + 320, MVF, 64, 1) SHAPE(WSTEP_2_X4, MVF + 320, MVF, 256, 4) SHAPE(WSTEP_1_X4, MVF + 320, MVF, 256, 4)
SHAPE(WLOAD, MVF + REGS + 128, MVF, 64, 1)
SHAPE(TREC_MLW_2, MVF + 1, MVF, 64, 1) SHAPE(TREC_MLW_2BS, MVF + 1, MVF, 64, 1) SHAPE(TREC_MLW_1, MVF + 1, MVF, 64, 1) SHAPE(TREC_MLW_1OCT, MVF + 1, MVF, 64, 1)
SHAPE(TREC_H2CW_2, MVF + 1, MVF, 64, 1) SHAPE(TREC_H2CW_2BS, MVF + 1, MVF, 64, 1) SHAPE(TREC_H2CW_1, MVF + 1, MVF, 64, 1) SHAPE(TREC_G1W_1, MVF + 1, MVF, 64, 1)
SHAPE(LREC_2, LVF + 2, LVF + LINES_OUT, 64, 1) SHAPE(LREC_3, LVF + 2, LVF + LINES_OUT, 64, 1) SHAPE(LREC_4, LVF + 2, LVF + LINES_OUT, 64, 1)
SHAPE(LREC_4_HAS2, LVF + 2, LVF + LINES_OUT, 64, 1) SHAPE(LREC_2_HAS2, LVF + 2, LVF + LINES_OUT, 64, 1) SHAPE(LREC_3_HAS2, LVF + 2, LVF + LINES_OUT, 64, 1)
// the step shape of a table-driven op: 0 <2>, 1 <2, BS>, 2 <1>, 3 <1, OCT>
constexpr int trec_shape(int op) { return op == TREC_MLW_2 || op == TREC_H2CW_2 ? 0 : (op == TREC_MLW_2BS || op == TREC_H2CW_2BS ? 1 : (op == TREC_MLW_1OCT ? 3 : 2)); }
constexpr bool is_trec(int op) { return op >= TREC_MLW_2 && op <= TREC_G1W_1; }
// the record of a kind as load_rec gives it, on either side (the tables are plain constants)
template <int OP> __host__ __device__ __forceinline__ mlw::Rec trec_load(uint32_t kind, uint32_t lane) {
    mlw::Rec r;
    if (OP <= TREC_MLW_1OCT) { const uint32_t k = kind < (uint32_t)MLW_KINDS ? kind : 0u; for (int i = 0; i < 5; i++) r.w[i] = MLW_REC[k][i][lane]; }
    else if (OP <= TREC_H2CW_1) { const uint32_t k = kind < (uint32_t)H2CW_KINDS ? kind : 0u; for (int i = 0; i < 5; i++) r.w[i] = H2CW_REC[k][i][lane]; }
    else { const uint32_t k = kind < (uint32_t)G1W_KINDS ? kind : 0u; for (int i = 0; i < 5; i++) r.w[i] = G1W_REC[k][i][lane]; }
    return r;
}
SHAPE(LSTEP_2, LVF + 7 * 64 + 1, LVF + LINES_OUT, 64, 1) SHAPE(LSTEP_3, LVF + 9 * 64 + 1, LVF + LINES_OUT, 64, 1)
SHAPE(LSTEP_4, LVF + 11 * 64 + 1, LVF + LINES_OUT, 64, 1) SHAPE(LSTEP_4_HAS2, LVF + 11 * 64 + 1, LVF + LINES_OUT, 64, 1)
SHAPE(LSTEP_2_HAS2, LVF + 7 * 64 + 1, LVF + LINES_OUT, 64, 1) SHAPE(LSTEP_3_HAS2, LVF + 9 * 64 + 1, LVF + LINES_OUT, 64, 1)
SHAPE(FXW_STEP_VV, REGS + 4 * 64, REGS, 64, 1) SHAPE(FXW_STEP_VG, 2 * REGS + 9 * 64, 2 * REGS, 64, 1)
SHAPE(FXW_VV_CSQ, REGS, REGS, 64, 1) SHAPE(FXW_VV_CONJ, REGS, REGS, 64, 1)
SHAPE(FXW_VG_MUL, 2 * REGS, 2 * REGS, 64, 1) SHAPE(FXW_VG_FROB, 2 * REGS, 2 * REGS, 64, 1) SHAPE(FXW_VG_FROBC, 2 * REGS, 2 * REGS, 64, 1)
SHAPE(FXW_TINV, REGS, REGS, 64, 1)

// ---- per lane -----------------------------------------------------------------------------------------------------------
template <int OP> __device__ __forceinline__ void lane_op(const int32_t* in, int32_t* out, char* vf) {
    int32_t t[NL], V[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) t[j] = in[j];
    if (OP == SRN) mlw::srn(V, t, in[NL]);
    if (OP == FXW_SCALE_NORM) fxw::scale_norm(V, t, in[NL]);
    if (OP == STORED_ZERO) {
        const uint32_t a = (threadIdx.x >> 6) * (uint32_t)MLW_PAGE_BYTES + 4u * (threadIdx.x & 63u);
        mlw::st14(vf, a, t);
        out[NL] = mlw::stored_zero(vf, a) ? 1 : 0;
        const r28::fe x = mlw::ld_fe(vf, a);
#pragma unroll
        for (int j = 0; j < NL; j++) V[j] = x.v[j];
    }
#pragma unroll
    for (int j = 0; j < NL; j++) out[j] = V[j];
}
template <int OP> __global__ void __launch_bounds__(256) k_lane(const int32_t* __restrict__ in, size_t n, int32_t* __restrict__ out) {
    __shared__ int32_t vfile[OP == STORED_ZERO ? MVF : 1];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    lane_op<OP>(in + i * Shape<OP>::win, out + i * Shape<OP>::wout, reinterpret_cast<char*>(vfile));
}

// ---- per wavefront: the value file of blsgpu_mlw.hip ----------------------------------------------------------------------
template <int OP> __global__ void __launch_bounds__(Shape<OP>::threads) k_wave(const int32_t* __restrict__ in, size_t n, int32_t* __restrict__ out) {
    constexpr int PER = Shape<OP>::per;
    __shared__ int32_t vfiles[PER][MVF];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t item_raw = (size_t)blockIdx.x * PER + wv;
    const bool active = item_raw < n;
    const size_t item = active ? item_raw : n - 1;         // (a spare wavefront repeats the last item and writes nothing)
    const int32_t* src = in + item * Shape<OP>::win;
    int32_t* vfile = vfiles[wv];
    char* vf = reinterpret_cast<char*>(vfile);
    for (uint32_t i = lane; i < (uint32_t)MVF; i += 64u) vfile[i] = src[i];
    __syncthreads();
    if (is_trec(OP)) {
        const uint32_t kind = (uint32_t)src[MVF];
        mlw::Rec r;
        if (OP <= TREC_MLW_1OCT) r = mlw::load_rec(MLW_REC, kind, lane);
        else if (OP <= TREC_H2CW_1) r = mlw::load_rec(H2CW_REC, kind, lane);
        else r = mlw::load_rec(G1W_REC, kind, lane);
        if (trec_shape(OP) == 0) mlw::wstep<2, false>(vf, r);
        if (trec_shape(OP) == 1) mlw::wstep<2, true>(vf, r);
        if (trec_shape(OP) == 2) mlw::wstep<1, false>(vf, r);
        if (trec_shape(OP) == 3) mlw::wstep<1, false, true>(vf, r);
    } else if (OP == WLOAD) {
        int32_t t[NL], V[NL];
#pragma unroll
        for (int j = 0; j < NL; j++) t[j] = src[MVF + lane * NL + j];
        const uint32_t dst = (uint32_t)src[MVF + REGS + lane];
        mlw::srn(V, t, src[MVF + REGS + 64 + lane] * mlw::quad_variant(lane));     // (sc x variant: k_miller_wide's -3 px, 3 py)
        mlw::st14(vf, dst, V);
    } else {
        mlw::Rec r;
#pragma unroll
        for (int i = 0; i < 5; i++) r.w[i] = (uint32_t)src[MVF + i * 64 + lane];
        if (OP == WSTEP_2 || OP == WSTEP_2_X4) mlw::wstep<2, false>(vf, r);
        if (OP == WSTEP_2BS) mlw::wstep<2, true>(vf, r);
        if (OP == WSTEP_1 || OP == WSTEP_1_X4) mlw::wstep<1, false>(vf, r);
        if (OP == WSTEP_1OCT) mlw::wstep<1, false, true>(vf, r);
    }
    __syncthreads();
    if (active) {
        int32_t* o = out + item * Shape<OP>::wout;
        for (uint32_t i = lane; i < (uint32_t)MVF; i += 64u) o[i] = vfile[i];
    }
}

// ---- line-stream steps: four pairs of a wavefront in the layout of k_ml_lines_wide's vfiles ----------------------------------
template <int OP> struct LShape;
template <> struct LShape<LSTEP_2> { static constexpr int K = 2; static constexpr bool H = false; };
template <> struct LShape<LSTEP_3> { static constexpr int K = 3; static constexpr bool H = false; };
template <> struct LShape<LSTEP_4> { static constexpr int K = 4; static constexpr bool H = false; };
template <> struct LShape<LSTEP_4_HAS2> { static constexpr int K = 4; static constexpr bool H = true; };
template <> struct LShape<LSTEP_2_HAS2> { static constexpr int K = 2; static constexpr bool H = true; };
template <> struct LShape<LSTEP_3_HAS2> { static constexpr int K = 3; static constexpr bool H = true; };
template <> struct LShape<LREC_2> : LShape<LSTEP_2> {};
template <> struct LShape<LREC_3> : LShape<LSTEP_3> {};
template <> struct LShape<LREC_4> : LShape<LSTEP_4> {};
template <> struct LShape<LREC_4_HAS2> : LShape<LSTEP_4_HAS2> {};
template <> struct LShape<LREC_2_HAS2> : LShape<LSTEP_2_HAS2> {};
template <> struct LShape<LREC_3_HAS2> : LShape<LSTEP_3_HAS2> {};
template <int OP> __global__ void __launch_bounds__(64) k_line(const int32_t* __restrict__ in, size_t n, int32_t* __restrict__ out) {
    constexpr int K = LShape<OP>::K, NW = 2 * K + 3;
    __shared__ int32_t vfile[LVF];
    const uint32_t lane = threadIdx.x & 63u, slot = lane >> 4;
    const int32_t* src = in + (size_t)blockIdx.x * Shape<OP>::win;
    int32_t* o = out + (size_t)blockIdx.x * Shape<OP>::wout;
    for (uint32_t i = lane; i < (uint32_t)LVF; i += 64u) vfile[i] = src[i];
    __syncthreads();
    lsw::RecN<NW> rec;
    bool has_line;
    if (OP >= LREC_2) {
        rec = lsw::load_rec<K>((uint32_t)src[LVF], lane & 15u);
        has_line = src[LVF + 1] != 0;
    } else {
#pragma unroll
        for (int i = 0; i < NW; i++) rec.w[i] = (uint32_t)src[LVF + i * 64 + lane];
        has_line = src[LVF + NW * 64] != 0;
    }
    lsw::lstep<K, LShape<OP>::H>(reinterpret_cast<char*>(vfile) + 4u * slot, rec, has_line ? o + LVF + slot * ml::LINE_DW : nullptr);
    __syncthreads();
    for (uint32_t i = lane; i < (uint32_t)LVF; i += 64u) o[i] = vfile[i];
}

// ---- final-exponentiation steps: V and G in registers ------------------------------------------------------------------------
template <int OP> __global__ void __launch_bounds__(64) k_fxw(const int32_t* __restrict__ in, size_t n, int32_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, quad = lane >> 2;
    const bool home_lane = quad < 12u;
    const int32_t variant = mlw::quad_variant(lane);      // 1, -1, 2, -2: the lane's multiple, as the fxw kernels compute it
    const int32_t* src = in + (size_t)blockIdx.x * Shape<OP>::win;
    int32_t* o = out + (size_t)blockIdx.x * Shape<OP>::wout;
    constexpr bool VG = OP == FXW_STEP_VG || OP == FXW_VG_MUL || OP == FXW_VG_FROB || OP == FXW_VG_FROBC;
    int32_t V[NL], G[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) { V[j] = src[lane * NL + j]; G[j] = VG ? src[REGS + lane * NL + j] : 0; }
    if (OP == FXW_STEP_VV) {
        const int32_t* t = src + REGS;
        const fxw::P1 p = {(uint32_t)t[lane], (uint32_t)t[64 + lane], (uint32_t)t[128 + lane], (uint32_t)t[192 + lane]};
        fxw::step_vv(V, p, variant, home_lane);
    }
    if (OP == FXW_VV_CSQ) fxw::step_vv(V, fxw::load_p1(BLS28W_CSQ, lane), variant, home_lane);
    if (OP == FXW_VV_CONJ) fxw::step_vv(V, fxw::load_p1(BLS28W_CONJ, lane), variant, home_lane);
    if (OP == FXW_STEP_VG) {
        const int32_t* t = src + 2 * REGS;
        fxw::P3 p;
#pragma unroll
        for (int i = 0; i < 3; i++) { p.s1[i] = (uint32_t)t[(3 * i) * 64 + lane]; p.s2[i] = (uint32_t)t[(3 * i + 1) * 64 + lane]; p.s3[i] = (uint32_t)t[(3 * i + 2) * 64 + lane]; }
        fxw::step_vg(V, G, p, variant, home_lane);
    }
    if (OP == FXW_VG_MUL) fxw::step_vg(V, G, fxw::load_p3(BLS28W_MUL, lane), variant, home_lane);
    if (OP == FXW_VG_FROB) fxw::step_vg(V, G, fxw::load_p3(BLS28W_FROB, lane), variant, home_lane);
    if (OP == FXW_VG_FROBC) fxw::step_vg(V, G, fxw::load_p3(BLS28W_FROBC, lane), variant, home_lane);
    if (OP == FXW_TINV) fxw::tinv(V, quad, variant, home_lane);
#pragma unroll
    for (int j = 0; j < NL; j++) {
        o[lane * NL + j] = V[j];
        if (VG) o[REGS + lane * NL + j] = G[j];
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// every byte address a step will use lies inside the value file: limb 13 of the slot at a + 256 x 13 (+ the pair's 12 for lsw)
bool addr_ok(uint32_t a, int vf_dw, uint32_t extra) { return (a & 3u) == 0 && (size_t)a + extra + 256u * (NL - 1) + 4u <= (size_t)vf_dw * 4u; }
template <int OP> bool records_ok(const int32_t* in, size_t n) {
    for (size_t it = 0; it < n; it++) {
        const int32_t* p = in + it * Shape<OP>::win;
        if (OP == WLOAD) {
            for (int l = 0; l < 64; l++)
                if (!addr_ok((uint32_t)p[MVF + REGS + l], MVF, 0)) return false;
        } else if (OP >= WSTEP_2 && OP <= WSTEP_1_X4) {
            const bool bs = OP == WSTEP_2BS;
            const int nops = (OP == WSTEP_1 || OP == WSTEP_1OCT || OP == WSTEP_1_X4) ? 2 : 4;
            for (int l = 0; l < 64; l++) {
                for (int i = 0; i < nops; i++) {
                    const uint32_t w = (uint32_t)p[MVF + i * 64 + l];
                    if (!addr_ok(w & 0xFFFFu, MVF, 0)) return false;
                    if (!(bs && (i & 1)) && !addr_ok(w >> 16, MVF, 0)) return false;      // (a one-slot operand ignores its second address)
                }
                if (!addr_ok((uint32_t)p[MVF + 4 * 64 + l] & 0xFFFFu, MVF, 0)) return false;
            }
        } else if (is_trec(OP)) {
            const int shape = trec_shape(OP), nops = shape >= 2 ? 2 : 4;
            for (int l = 0; l < 64; l++) {
                const mlw::Rec r = trec_load<OP>((uint32_t)p[MVF], (uint32_t)l);
                for (int i = 0; i < nops; i++) {
                    if (!addr_ok(r.w[i] & 0xFFFFu, MVF, 0)) return false;
                    if (!(shape == 1 && (i & 1)) && !addr_ok(r.w[i] >> 16, MVF, 0)) return false;
                }
                if (!addr_ok(r.w[4] & 0xFFFFu, MVF, 0)) return false;
            }
        } else if (OP >= LREC_2 && OP <= LREC_3_HAS2) {
            constexpr int K = LShape<OP >= LREC_2 && OP <= LREC_3_HAS2 ? OP : LREC_2>::K;
            const uint32_t kind = (uint32_t)p[LVF];
            if (kind >= (uint32_t)LSW_KINDS) return false;             // (lsw::load_rec has no clamp)
            for (int l = 0; l < 16; l++) {
                for (int i = 0; i < 2 * K + 2; i++) {
                    const uint32_t w = LSW_REC[kind][i < 2 * K ? i : 8 + i - 2 * K][l];
                    if (!addr_ok(w & 0xFFFFu, LVF, 12) || !addr_ok(w >> 16, LVF, 12)) return false;
                }
                const uint32_t lo = (LSW_REC[kind][10][l] >> 16) & 0xFFu;
                if (lo != 0xFFu && lo >= 6u) return false;
            }
        } else if (OP >= LSTEP_2 && OP <= LSTEP_3_HAS2) {
            const int K = (OP == LSTEP_2 || OP == LSTEP_2_HAS2) ? 2 : ((OP == LSTEP_3 || OP == LSTEP_3_HAS2) ? 3 : 4);
            for (int l = 0; l < 64; l++) {
                for (int i = 0; i < 2 * K + 2; i++) {
                    const uint32_t w = (uint32_t)p[LVF + i * 64 + l];
                    if (!addr_ok(w & 0xFFFFu, LVF, 12) || !addr_ok(w >> 16, LVF, 12)) return false;
                }
                const uint32_t lo = ((uint32_t)p[LVF + (2 * K + 2) * 64 + l] >> 16) & 0xFFu;
                if (lo != 0xFFu && lo >= 6u) return false;
            }
        }
    }
    return true;
}

template <int OP> void launch(const int32_t* din, size_t n, int32_t* dout) {
    const unsigned per = (unsigned)Shape<OP>::per, blocks = (unsigned)((n + per - 1) / per);
    if constexpr (OP <= STORED_ZERO) k_lane<OP><<<dim3(blocks), dim3((unsigned)Shape<OP>::threads)>>>(din, n, dout);
    else if constexpr (OP <= WLOAD || is_trec(OP)) k_wave<OP><<<dim3(blocks), dim3((unsigned)Shape<OP>::threads)>>>(din, n, dout);
    else if constexpr (OP <= LSTEP_3_HAS2 || (OP >= LREC_2 && OP <= LREC_3_HAS2)) k_line<OP><<<dim3(blocks), dim3((unsigned)Shape<OP>::threads)>>>(din, n, dout);
    else k_fxw<OP><<<dim3(blocks), dim3((unsigned)Shape<OP>::threads)>>>(din, n, dout);
}

template <int OP> int run_op(const int32_t* in, size_t words_in, size_t n, int32_t* out, size_t words_out) {
    if (n == 0 || n > (1u << 16) || words_in != n * (size_t)Shape<OP>::win || words_out != n * (size_t)Shape<OP>::wout) return -2;
    if (!records_ok<OP>(in, n)) return -4;
    return check::guarded_run(in, words_in * 4, out, words_out * 4, 0, [=](const int32_t* din, int32_t* dout) { launch<OP>(din, n, dout); });
}
}  // namespace

CHECK_EXPORT(blsgpu_wide_check, int32_t, WIDECHECK_OPS)
