// blsgpu_ml_check.hip -- TEST-ONLY device library (libblsgpu_mlcheck.so): the lane-pair (ml::sp), lane-quad (ml::sq) and
// six-lane-team routines of blsgpu_ml.hip -- the arithmetic of k_ml_lines2 / k_ml_lines4 and of k_ml_accum / k_ml_merge /
// k_ml_small -- as kernels of their own, operands and results as raw limb words in global memory, so that
// tests/test_gpu_ml_steps.py can compare the COMPILED routines word for word with the integer model (tests/ml_vectors.py).
// Not linked into libblsgpu.so, not declared in include/blsgpu.h, not an ABI.
//
// The routines are the production ones: this file includes the kernel texts the way blsgpu_api.hip does, with a BLSGPU_TU
// value no kernel group has, so no production kernel body is emitted (blsgpu_tu.h).  One kernel per op (a template on the op).
// Pair and quad kernels have the launch bounds of k_ml_lines2 and its slab of constants in dynamic LDS, laid out as
// lines_chain lays it out; team kernels have the launch bounds of k_ml_accum.  Spare lanes (past the last item) and the idle
// lanes 60 .. 63 of a team wavefront repeat the last item, run every DPP / ds_bpermute read with the others and store nothing.
// The host function refuses a position outside 0 .. 5 before anything is launched (-4); the guard records and the return codes are
// check_runner.h's.
//
// Lane-pair ops: an item is one lane pair, a value 2 x 14 words (the even lane's part, then the odd lane's), 128 items per
// 256-thread workgroup.  Each op at the ranges of its call sites in blsgpu_ml.hip:
//   MUL_XI, B3          S<1>           tangent_step / sq::tangent_step  E = b3(C)
//   MUL_31              Lop<3> Rop<1>  tangent_step  X = mul(left(A2), right(BmF));  sq::tangent_step m (A2 | widen<3>(B))
//   MUL_11              Lop<1> Rop<1>  tangent_step Z;  chord_step th, la, E, Fz, Gg, X, Z;  lines_chain xxx;  k_ml_exact_fixup
//   DOT2_1111                          chord_step line coefficient 0 and Y3;  k_ml_lines_exact tt
//   SQR_H               h              tangent_step XX, C, B;  chord_step C, D;  sq::tangent_step;  lines_chain yy, xx
//   SQR_HN2             hn + hn        tangent_step (Y + Z)^2, (X + Y)^2: "8 units, the whole column"
//   SQR_M12SQR          h, h           tangent_step Y = G^2 - 12 E^2
//   MULF_1, MULF_3      S<1>, S<3>     tangent_step X^2 (-3 px), 2YZ py (S<3>);  chord_step th (-3 px), la (3 py);  sq::tangent_step lc (S<3>)
//   NORM_2, NORM_4      S<2>, S<4>     chord_step th, la, GH (S<2>), H (S<4>), nE (S<1>);  tangent_step BmF, G (S<4>);  sq:: Y + Z, X + Y, Y
//   MULC_NORM_4_S3                     tangent_step z8 = mulc_norm<4>(H)
//   MULC_NORM_3_S2                     chord_step xq3, nyq3 (on S<1>: the S<2> range contains it)
//   MULC_NORM_12_S2                    b3;  sq::tangent_step 12 E^2 (on S<1>)
//   MULC_NORM_N12_S2                   sqr_m12sqr nue12
//   IS_ZERO2            h              lines_chain (twist test, final Z);  zero2 of k_ml_lines_exact           -> the flag of either lane
//   LOAD_STORE                         lines_chain load_part (3 x 2 x 48 big-endian bytes), store_part for the coefficients 0, 1, 2
//   SP_TANGENT, SP_CHORD               X, Y, Z, then the slab: -3 px (14 words), py (14), xq, yq  ->  X, Y, Z, the 84-word line record
// Lane-quad ops: an item is one quad (64 per workgroup).
//   OTH                 a value per pair -> the other pair's;  PICK  (a, b) per pair -> pair 0: a, pair 1: b
//   SQ_TANGENT          as SP_TANGENT (both pairs load the same inputs, as in lines_chain<true>) -> X, Y, Z of pair 0, the record
//                       (pair 0 stores coefficients 0 and 1, pair 1 the third), then X, Y, Z of pair 1
// Team ops: an item is one team of six lanes, a value 6 x 2 x 14 words (lane c: re, im), ten teams per wavefront, forty per workgroup.
//   SET_ONE;  PUBLISH_RAW / PUBLISH_NORM  publish<false / true>: re, im, nim, xre, xim, nxim of every lane
//   FETCH_0 .. FETCH_5  fetch<J> on publish<true> (mul_dense's): re, im, nim as received;  FETCH2_RT  f, J -> re, im as received
//   MUL3_012, MUL3_345  f, y0, y1, y2 (re, im each) on publish<true>, as mul_dense calls them;  MUL3_012_RAW on publish<false>
//   TEAM_LINE           f, the line record, jA, jB -> mul_line_k3 (k_ml_accum, k_ml_small)
//   TEAM_DENSE          f, g -> mul_dense with GlobalRec (k_ml_merge, k_fexp_team)
//   TEAM_SQUARE         f -> mul_dense with TeamRec on its own value (k_ml_small)
//   TEAM_TEAMREC        f, g per lane -> mul_dense with TeamRec on another value (k_fexp_team)
//   (publish<false> and LdsRec have no production instantiation; LdsRec's body is GlobalRec's.)
#include "check_runner.h"
#define BLSGPU_TU 99                                       // no kernel group: declarations only
#include "blsgpu_tu.h"
#include "blsgpu_kernels.hip"
#include "fp28.h"
#include "blsgpu_ml.hip"

namespace {
using namespace blsgpu;
using r28::NL;
namespace sp = ml::sp;
namespace sq = ml::sq;

// every op, once, with its code (tests/ml_vectors.py pins the codes)
#define MLCHECK_OPS(X) \
    X(MUL_XI, 0) X(B3, 1) X(MUL_31, 2) X(MUL_11, 3) X(DOT2_1111, 4) X(SQR_H, 5) X(SQR_HN2, 6) X(SQR_M12SQR, 7) X(MULF_1, 8) X(MULF_3, 9) \
    X(NORM_2, 10) X(NORM_4, 11) X(MULC_NORM_4_S3, 12) X(MULC_NORM_3_S2, 13) X(MULC_NORM_12_S2, 14) X(MULC_NORM_N12_S2, 15) X(IS_ZERO2, 16) \
    X(LOAD_STORE, 17) X(SP_TANGENT, 18) X(SP_CHORD, 19) \
    X(OTH, 30) X(PICK, 31) X(SQ_TANGENT, 32) \
    X(SET_ONE, 40) X(PUBLISH_RAW, 41) X(PUBLISH_NORM, 42) X(FETCH_0, 43) X(FETCH_1, 44) X(FETCH_2, 45) X(FETCH_3, 46) X(FETCH_4, 47) \
    X(FETCH_5, 48) X(FETCH2_RT, 49) X(MUL3_012, 50) X(MUL3_345, 51) X(MUL3_012_RAW, 52) X(TEAM_LINE, 53) X(TEAM_DENSE, 54) \
    X(TEAM_SQUARE, 55) X(TEAM_TEAMREC, 56)
CHECK_ENUM(MLCHECK_OPS)
constexpr int V2 = 2 * NL, REC = ml::LINE_DW, TV = 6 * V2, STEP_IN = 3 * V2 + 2 * NL + 2 * V2, STEP_OUT = 3 * V2 + REC;

// words per item in and out, lanes per item
template <int OP> struct Shape;
#define SHAPE(OP, WIN, WOUT, LANES) template <> struct Shape<OP> { static constexpr int win = WIN, wout = WOUT, lanes = LANES; };
SHAPE(MUL_XI, V2, V2, 2) SHAPE(B3, V2, V2, 2) SHAPE(MUL_31, 2 * V2, V2, 2) SHAPE(MUL_11, 2 * V2, V2, 2) SHAPE(DOT2_1111, 4 * V2, V2, 2)
SHAPE(SQR_H, V2, V2, 2) SHAPE(SQR_HN2, 2 * V2, V2, 2) SHAPE(SQR_M12SQR, 2 * V2, V2, 2) SHAPE(MULF_1, V2 + NL, V2, 2) SHAPE(MULF_3, V2 + NL, V2, 2)
SHAPE(NORM_2, V2, V2, 2) SHAPE(NORM_4, V2, V2, 2) SHAPE(MULC_NORM_4_S3, V2, V2, 2) SHAPE(MULC_NORM_3_S2, V2, V2, 2)
SHAPE(MULC_NORM_12_S2, V2, V2, 2) SHAPE(MULC_NORM_N12_S2, V2, V2, 2) SHAPE(IS_ZERO2, V2, 2, 2) SHAPE(LOAD_STORE, 3 * 24, REC, 2)
SHAPE(SP_TANGENT, STEP_IN, STEP_OUT, 2) SHAPE(SP_CHORD, STEP_IN, STEP_OUT, 2)
SHAPE(OTH, 2 * V2, 2 * V2, 4) SHAPE(PICK, 4 * V2, 2 * V2, 4) SHAPE(SQ_TANGENT, STEP_IN, STEP_OUT + 3 * V2, 4)
SHAPE(SET_ONE, TV, TV, 6) SHAPE(PUBLISH_RAW, TV, 3 * TV, 6) SHAPE(PUBLISH_NORM, TV, 3 * TV, 6)
SHAPE(FETCH_0, TV, 6 * 3 * NL, 6) SHAPE(FETCH_1, TV, 6 * 3 * NL, 6) SHAPE(FETCH_2, TV, 6 * 3 * NL, 6) SHAPE(FETCH_3, TV, 6 * 3 * NL, 6)
SHAPE(FETCH_4, TV, 6 * 3 * NL, 6) SHAPE(FETCH_5, TV, 6 * 3 * NL, 6) SHAPE(FETCH2_RT, TV + 1, TV, 6)
SHAPE(MUL3_012, TV + 3 * V2, TV, 6) SHAPE(MUL3_345, TV + 3 * V2, TV, 6) SHAPE(MUL3_012_RAW, TV + 3 * V2, TV, 6)
SHAPE(TEAM_LINE, TV + REC + 2, TV, 6) SHAPE(TEAM_DENSE, 2 * TV, TV, 6) SHAPE(TEAM_SQUARE, TV, TV, 6) SHAPE(TEAM_TEAMREC, 2 * TV, TV, 6)

template <class T> __device__ __forceinline__ T ldv(const int32_t* __restrict__ p) { T r;
#pragma unroll
    for (int j = 0; j < NL; j++) r.v[j] = p[j];
    return r; }
template <class T> __device__ __forceinline__ void stv(int32_t* __restrict__ p, const T& x) {
#pragma unroll
    for (int j = 0; j < NL; j++) p[j] = x.v[j];
}

// ---- lane pairs and lane quads ------------------------------------------------------------------------------------------------
// src: the item's words, this lane's part of value k at src + k V2 + part NL; o: the item's output words, or null for a spare lane,
// whose line record goes to `dump` (a record of its own behind the second guard, never read back)
template <int OP> __device__ __forceinline__ void pair_op(const int32_t* __restrict__ src, int32_t* __restrict__ o, int32_t* __restrict__ dump, const sp::Slab& sl) {
    const uint32_t part = threadIdx.x & 1u, pair = (threadIdx.x >> 1) & 1u;
    const int32_t* in = src + part * NL;
    int32_t* out = o ? o + part * NL : nullptr;
    sp::hn r;
    bool plain = true;                                     // the result is one value, stored at out
    if constexpr (OP == MUL_XI) { const sp::S<2> x = sp::mul_xi(ldv<sp::S<1>>(in)); if (out) stv(out, x); plain = false; }
    if constexpr (OP == B3) r = sp::b3(ldv<sp::S<1>>(in));
    if constexpr (OP == MUL_31) r = sp::mul(sp::left(ldv<sp::S<3>>(in)), sp::right(ldv<sp::S<1>>(in + V2)));
    if constexpr (OP == MUL_11) r = sp::mul(sp::left(ldv<sp::S<1>>(in)), sp::right(ldv<sp::S<1>>(in + V2)));
    if constexpr (OP == DOT2_1111)
        r = sp::dot2(sp::left(ldv<sp::S<1>>(in)), sp::right(ldv<sp::S<1>>(in + V2)), sp::left(ldv<sp::S<1>>(in + 2 * V2)), sp::right(ldv<sp::S<1>>(in + 3 * V2)));
    if constexpr (OP == SQR_H) r = sp::sqr(ldv<sp::h>(in));
    if constexpr (OP == SQR_HN2) r = sp::sqr(sp::addn(ldv<sp::hn>(in), ldv<sp::hn>(in + V2)));
    if constexpr (OP == SQR_M12SQR) r = sp::sqr_m12sqr(ldv<sp::h>(in), ldv<sp::h>(in + V2));
    if constexpr (OP == MULF_1) r = sp::mulf(ldv<sp::S<1>>(in), ldv<r28::fe>(src + V2));
    if constexpr (OP == MULF_3) r = sp::mulf(ldv<sp::S<3>>(in), ldv<r28::fe>(src + V2));
    if constexpr (OP == NORM_2) r = sp::norm(ldv<sp::S<2>>(in));
    if constexpr (OP == NORM_4) r = sp::norm(ldv<sp::S<4>>(in));
    if constexpr (OP == MULC_NORM_4_S3) r = sp::mulc_norm<4>(ldv<sp::S<3>>(in));
    if constexpr (OP == MULC_NORM_3_S2) r = sp::mulc_norm<3>(ldv<sp::S<2>>(in));
    if constexpr (OP == MULC_NORM_12_S2) r = sp::mulc_norm<12>(ldv<sp::S<2>>(in));
    if constexpr (OP == MULC_NORM_N12_S2) r = sp::mulc_norm<-12>(ldv<sp::S<2>>(in));
    if constexpr (OP == IS_ZERO2) {
        const bool z = sp::is_zero2(ldv<sp::h>(in));
        if (o) o[part] = z ? 1 : 0;
        plain = false;
    }
    if constexpr (OP == LOAD_STORE) {
        int32_t* rec = o ? o : dump;
#pragma unroll
        for (int c = 0; c < 3; c++) sp::store_part(rec, c, sp::load_part(reinterpret_cast<const uint32_t*>(src) + c * 24 + part * 12));
        plain = false;
    }
    if constexpr (OP == SP_TANGENT || OP == SP_CHORD || OP == SQ_TANGENT) {
        sp::hn X = ldv<sp::hn>(in), Y = ldv<sp::hn>(in + V2), Z = ldv<sp::hn>(in + 2 * V2);
        sl.put(0, ldv<r28::fe>(src + 3 * V2));
        sl.put(1, ldv<r28::fe>(src + 3 * V2 + NL));
        sl.put(2, ldv<sp::h>(in + 3 * V2 + 2 * NL));
        sl.put(3, ldv<sp::h>(in + 4 * V2 + 2 * NL));
        int32_t* rec = o ? o + 3 * V2 : dump;
        if (OP == SP_TANGENT) sp::tangent_step(X, Y, Z, sl, rec);
        if (OP == SP_CHORD) sp::chord_step(X, Y, Z, sl, rec);
        if (OP == SQ_TANGENT) sq::tangent_step(X, Y, Z, sl, rec);
        if (out) {
            int32_t* xyz = OP == SQ_TANGENT && pair ? out + STEP_OUT : out;
            stv(xyz, X); stv(xyz + V2, Y); stv(xyz + 2 * V2, Z);
        }
        plain = false;
    }
    if constexpr (OP == OTH) { const sp::S<1> x = sq::oth(ldv<sp::S<1>>(in + pair * V2)); if (out) stv(out + pair * V2, x); plain = false; }
    if constexpr (OP == PICK) {
        const sp::S<1> x = sq::pick(ldv<sp::S<1>>(in + pair * 2 * V2), ldv<sp::S<1>>(in + pair * 2 * V2 + V2));
        if (out) stv(out + pair * V2, x);
        plain = false;
    }
    if (plain && out) stv(out, r);
}
template <int OP> __global__ void __launch_bounds__(256, BLSGPU_ML_LINES2_WAVES) k_pair(const int32_t* __restrict__ in, uint32_t n, int32_t* __restrict__ out, int32_t* __restrict__ dump) {
    extern __shared__ int32_t ml_slab[];
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t ir = t / (uint32_t)Shape<OP>::lanes;
    const uint32_t item = ir < n ? ir : n - 1u;           // spare lanes repeat the last item
    const sp::Slab sl{(sp::lds_i32*)ml_slab + (threadIdx.x >> 6) * (sp::SLAB_SLOTS * NL * 64) + (threadIdx.x & 63u)};
    pair_op<OP>(in + (size_t)item * Shape<OP>::win, ir < n ? out + (size_t)item * Shape<OP>::wout : nullptr, dump, sl);
}

// ---- teams of six lanes ---------------------------------------------------------------------------------------------------------
template <int OP> __global__ void __launch_bounds__(256, BLSGPU_ML_ACCUM_WAVES) k_team(const int32_t* __restrict__ in, uint32_t n, int32_t* __restrict__ out) {
    const ml::Team t = ml::team_of_lane();
    const uint32_t id = wave_index() * ml::TEAMS + t.slot;
    const bool valid = t.slot < (uint32_t)ml::TEAMS && id < n;
    const uint32_t item = valid ? id : n - 1u;            // spare teams and the idle lanes (c = 0 .. 3 there) repeat the last item
    const int32_t* src = in + (size_t)item * Shape<OP>::win;
    int32_t* o = out + (size_t)item * Shape<OP>::wout;
    int32_t fre[NL], fim[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) { fre[j] = src[t.c * V2 + j]; fim[j] = src[t.c * V2 + NL + j]; }
    if constexpr (OP == SET_ONE) ml::set_one(fre, fim, t);
    if constexpr (OP == PUBLISH_RAW || OP == PUBLISH_NORM) {
        ml::Pub P;
        ml::publish<OP == PUBLISH_NORM>(P, fre, fim);
        if (valid) {
            int32_t* q = o + t.c * 6 * NL;
#pragma unroll
            for (int j = 0; j < NL; j++) {
                q[j] = P.re[j]; q[NL + j] = P.im[j]; q[2 * NL + j] = P.nim[j]; q[3 * NL + j] = P.xre[j]; q[4 * NL + j] = P.xim[j]; q[5 * NL + j] = P.nxim[j];
            }
        }
        return;
    }
    if constexpr (OP >= FETCH_0 && OP <= FETCH_5) {
        ml::Pub P;
        ml::publish<true>(P, fre, fim);
        ml::Xop X;
        ml::fetch<OP - FETCH_0>(X, P, t);
        if (valid) {
            int32_t* q = o + t.c * 3 * NL;
#pragma unroll
            for (int j = 0; j < NL; j++) { q[j] = X.re[j]; q[NL + j] = X.im[j]; q[2 * NL + j] = X.nim[j]; }
        }
        return;
    }
    if constexpr (OP == FETCH2_RT) {
        ml::Pub2 P;
#pragma unroll
        for (int j = 0; j < NL; j++) { P.re[j] = fre[j]; P.im[j] = fim[j]; P.xre[j] = fre[j] - fim[j]; P.xim[j] = fre[j] + fim[j]; }   // (as mul_line_k3)
        ml::Xop2 X;
        ml::fetch2_rt(X, P, t, (uint32_t)src[TV]);
#pragma unroll
        for (int j = 0; j < NL; j++) { fre[j] = X.re[j]; fim[j] = X.im[j]; }
    }
    if constexpr (OP == MUL3_012 || OP == MUL3_345 || OP == MUL3_012_RAW) {
        ml::Pub P;
        ml::publish<OP != MUL3_012_RAW>(P, fre, fim);
        int32_t y[6][NL];
#pragma unroll
        for (int k = 0; k < 6; k++) ml::GlobalRec{src + TV}(y[k], k);
        if (OP == MUL3_345) ml::mul3<3, 4, 5>(fre, fim, P, t, y[0], y[1], y[2], y[3], y[4], y[5]);
        else ml::mul3<0, 1, 2>(fre, fim, P, t, y[0], y[1], y[2], y[3], y[4], y[5]);
    }
    if constexpr (OP == TEAM_LINE) {
        int32_t y[6][NL];
#pragma unroll
        for (int k = 0; k < 6; k++) ml::GlobalRec{src + TV}(y[k], k);
        ml::mul_line_k3(fre, fim, t, (uint32_t)src[TV + REC], (uint32_t)src[TV + REC + 1], y);
    }
    if constexpr (OP == TEAM_DENSE) ml::mul_dense(fre, fim, t, ml::GlobalRec{src + TV});
    if constexpr (OP == TEAM_SQUARE) {
        int32_t cre[NL], cim[NL];
#pragma unroll
        for (int k = 0; k < NL; k++) { cre[k] = fre[k]; cim[k] = fim[k]; }
        ml::mul_dense(fre, fim, t, ml::TeamRec{cre, cim, t.base4});
    }
    if constexpr (OP == TEAM_TEAMREC) {
        int32_t gre[NL], gim[NL];
#pragma unroll
        for (int k = 0; k < NL; k++) { gre[k] = src[TV + t.c * V2 + k]; gim[k] = src[TV + t.c * V2 + NL + k]; }
        ml::mul_dense(fre, fim, t, ml::TeamRec{gre, gim, t.base4});
    }
    if (valid) {
        int32_t* q = o + t.c * V2;
#pragma unroll
        for (int j = 0; j < NL; j++) { q[j] = fre[j]; q[NL + j] = fim[j]; }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// the run-time positions of an item are powers of w: 0 .. 5
template <int OP> bool positions_ok(const int32_t* in, size_t n) {
    for (size_t it = 0; it < n; it++) {
        const int32_t* p = in + it * Shape<OP>::win;
        if (OP == FETCH2_RT && (p[TV] < 0 || p[TV] > 5)) return false;
        if (OP == TEAM_LINE && (p[TV + REC] < 0 || p[TV + REC] > 5 || p[TV + REC + 1] < 0 || p[TV + REC + 1] > 5)) return false;
    }
    return true;
}

constexpr size_t DUMP = REC * 4;                           // behind the second guard: where spare lanes of the step ops put their line record

template <int OP> void launch(const int32_t* din, uint32_t n, int32_t* dout, int32_t* dump) {
    if constexpr (Shape<OP>::lanes == 6) {
        const unsigned waves = (n + ml::TEAMS - 1) / ml::TEAMS, blocks = (waves + 3) / 4;
        k_team<OP><<<dim3(blocks), dim3(256)>>>(din, n, dout);
    } else {
        const unsigned per = 256 / Shape<OP>::lanes, blocks = (n + per - 1) / per;
        k_pair<OP><<<dim3(blocks), dim3(256), 256 * sp::SLAB_BYTES_PER_LANE>>>(din, n, dout, dump);
    }
}

template <int OP> int run_op(const int32_t* in, size_t words_in, size_t n, int32_t* out, size_t words_out) {
    if (n == 0 || n > (1u << 16) || words_in != n * (size_t)Shape<OP>::win || words_out != n * (size_t)Shape<OP>::wout) return -2;
    if (!positions_ok<OP>(in, n)) return -4;
    return check::guarded_run(in, words_in * 4, out, words_out * 4, DUMP, [=](const int32_t* din, int32_t* dout) {
        launch<OP>(din, (uint32_t)n, dout, dout + words_out + check::GUARD / 4);
    });
}
}  // namespace

CHECK_EXPORT(blsgpu_ml_check, int32_t, MLCHECK_OPS)
