// blsgpu_curve_check.hip -- TEST-ONLY device library (libblsgpu_curvecheck.so): the G2 curve arithmetic on lane pairs (sp2) and lane
// quads (sp4) of blsgpu_msm.hip, the group traits SrtG<1> / SrtG<2> and the digit routines of the sums (lane_digit, srt_digit_at,
// srt_key) as kernels of their own, operands and results as raw 32-bit words in global memory, so that tests/test_gpu_curve.py can
// compare the COMPILED routines word for word with the limb model (tests/curve_vectors.py) and check the device's own words as
// points against bls_py.hostmath.  Not linked into libblsgpu.so, not declared in include/blsgpu.h, not an ABI.
//
// The routines are the production ones: this file includes the kernel texts the way blsgpu_api.hip does, with a BLSGPU_TU value no
// kernel group has, so no production kernel body is emitted (blsgpu_tu.h).  One kernel per op (a template on the op), under the
// launch bounds of the tightest production kernel that calls the routine:
//   MSM  64 threads, BLSGPU_MSM_LANE2X_WAVES   k_msm_lane2x: pt_inf, pt_ld / pt_st, ldh, pmadd with norm(neg(y)), padd (the running
//                                              sums), st_vm, lane_digit;  k_pscan_range<2>, k_smul_seg (64, 2): pneg, padd
//   SRT  64 threads, BLSGPU_SRT_WAVES          k_srt_accum<DEG>: SrtG::madd;  k_srt_fix / k_srt_fix_long / k_srt_bits / k_srt_fold
//                                              (64): SrtG::add, xor_lanes;  k_smul / k_sum_chunks (64, 2): SrtG::dbl, madd, affine_out;
//                                              k_srt_count / k_srt_scatter (1024): srt_digit_at, srt_key
//   H2C  256 threads, 2 waves                  k_h2c_clear_pairs: sp2::padd, pdbl, to_jacobian, pdblj, to_homogeneous;  k_h2c_clear_quads
//                                              and k_msm_horner_quads: sp4's;  k_g2_smul / k_g2_smul_table: sp2::padd, pdbl, pmadd
// Spare lanes (past the last item) repeat the last item, run every DPP read with the others and store nothing.  The guard records
// and the return codes are check_runner.h's; the host side refuses, before anything is launched (-4): a `neg` or `store` word that
// is not 0 or 1, an xor_lanes call whose offsets differ, are no power of two below the units of a wavefront or whose count is not
// whole wavefronts, a lane_digit window >= 64, cb outside 5 .. SRT_MAXBITS and a window >= ceil(258 / cb).
//
// An `h` coordinate, when a routine receives it, has one of three forms (the call sites above): from_raw's digits (k_lane_prep,
// k_srt_prep: value in (-q, 2q)), a product's output (mul / dot2 / sqr: digits 0 .. 12 in [0, 2^28), value in (-q, 2q)), or norm's
// output: digits 0 .. 12 in [0, 2^28) and a signed top digit, the value a small sum of such values -- pneg's Y in (-2q, q), sp4::padd /
// sp4::pdbl's sums of two products in (-2q, 4q), pdblj's X = E^2 - 2 D in (-17q, 22q) and Y in (-17q, 10q), which to_homogeneous
// hands on.  So: limbs 0 .. 12 digits, value in (-17q, 22q) (tests/curve_vectors.py CONTRACT); every operand of every set lies in it.
//
// A G2 point is 84 words (pt_st's record: X, Y, Z, each the even lane's 14 limbs then the odd lane's), a G1 point 42.
// Lane-pair ops (one item per pair):
//   PT_INF              (one unused word) -> pt_inf
//   PT_LD_ST            P -> pt_st(pt_ld(P))
//   PNEG, PDBL, PADD    sp2's;  PMADD_NEG  P, x2, y2 -> pmadd(P, x2, norm(neg(y2)))
//   SRTG2_MADD          P, the prepared record x, y, -y, neg -> SrtG<2>::madd;  SRTG2_DBL, SRTG2_ADD
//   SRTG2_XOR_LANES     P, off -> the same part of the pair `off` pairs away (whole wavefronts, every pair another point)
//   TO_JACOBIAN, PDBLJ, TO_HOMOGENEOUS
//   ST_VM               P -> 72 words
//   SRTG2_AFFINE_OUT    P, store -> 48 big-endian words and the flag byte in a 49th word (untouched where store is 0)
// Lane-quad ops (one item per quad; the words of pair 0, then the words of pair 1):
//   SP4_PDBLJ, SP4_PDBL, SP4_PADD, SP4_TO_JACOBIAN, SP4_TO_HOMOGENEOUS
// One-lane ops (one item per lane):  SRTG1_MADD (P, x, y, -y, neg), SRTG1_XOR_LANES (P, off), SRTG1_AFFINE_OUT (P, store -> 24 + 1)
// Chain ops, on pairs (_2) and on quads (_4): every step's point is stored and loaded again before the next step
//   CHAIN_ADD8          P -> inf + P, then + P seven times more (the second step a doubling inside padd)
//   CHAIN_JAC_k         P -> to_jacobian, k x pdblj, to_homogeneous: k + 2 points (k = 1, 2, 16; 60 for the fixed point (1 : 1 : 0))
//   CHAIN_CANCEL        P -> padd(P, pneg(P)), to_jacobian, 2 x pdblj, to_homogeneous: 5 points, then affine_out's 49 words
//   CHAIN_RUNNING       four buckets -> the eight sums of acc += B_j, tot += acc from two infinities, padd's operands selected as
//                       k_msm_lane2x's loop selects them
// Digit ops (one item per lane):
//   LANE_DIGIT          8 scalar words as they lie in memory, window -> digit, big;  LANE_DIGIT_NULL  window, 0 -> digit
//   SRT_DIGIT_KEY       nine record words, w, cb -> biased digit, key, sign, the non-zero flag
// Inline in production kernels and so not callable as routines, covered end to end only: the psi step of k_h2c_clear_pairs /
// k_h2c_clear_quads, k_srt_prep's addition of the bias, and the operand select of the running sums (copied here, not called).
#include "check_runner.h"
#define BLSGPU_TU 99                                       // no kernel group: declarations only
#include "blsgpu_tu.h"
#include "blsgpu_kernels.hip"
#include "fp28.h"
#include "blsgpu_ml.hip"
#include "blsgpu_msm.hip"

namespace {
using namespace blsgpu;
using r28::NL;
using sp2::pt;

// every op, once, with its code (tests/curve_vectors.py pins the codes)
#define CURVECHECK_OPS(X) \
    X(PT_INF, 0) X(PT_LD_ST, 1) X(PNEG, 2) X(PDBL, 3) X(PADD, 4) X(PMADD_NEG, 5) X(SRTG2_MADD, 6) X(SRTG2_DBL, 7) X(SRTG2_ADD, 8) \
    X(SRTG2_XOR_LANES, 9) X(TO_JACOBIAN, 10) X(PDBLJ, 11) X(TO_HOMOGENEOUS, 12) X(ST_VM, 13) X(SRTG2_AFFINE_OUT, 14) \
    X(SP4_PDBLJ, 20) X(SP4_PDBL, 21) X(SP4_PADD, 22) X(SP4_TO_JACOBIAN, 23) X(SP4_TO_HOMOGENEOUS, 24) \
    X(SRTG1_MADD, 30) X(SRTG1_XOR_LANES, 31) X(SRTG1_AFFINE_OUT, 32) \
    X(CHAIN_ADD8_2, 40) X(CHAIN_ADD8_4, 41) X(CHAIN_JAC_1_2, 42) X(CHAIN_JAC_2_2, 43) X(CHAIN_JAC_16_2, 44) X(CHAIN_JAC_60_2, 45) \
    X(CHAIN_JAC_1_4, 46) X(CHAIN_JAC_2_4, 47) X(CHAIN_JAC_16_4, 48) X(CHAIN_JAC_60_4, 49) X(CHAIN_CANCEL_2, 50) X(CHAIN_CANCEL_4, 51) \
    X(CHAIN_RUNNING_2, 52) X(CHAIN_RUNNING_4, 53) \
    X(LANE_DIGIT, 60) X(LANE_DIGIT_NULL, 61) X(SRT_DIGIT_KEY, 62)
CHECK_ENUM(CURVECHECK_OPS)
constexpr int V2 = 2 * NL, PT = 3 * V2, P1 = 3 * NL, AFF2 = 48 + 1, AFF1 = 24 + 1;
enum Site { MSM, SRT, H2C };

// words per item in; words per pair out (quads write them once per pair), words out behind them; lanes per item; launch bounds
template <int OP> struct Shape;
#define SHAPE(OP, WIN, PW, TAIL, LANES, SITE) \
    template <> struct Shape<OP> { static constexpr int win = WIN, pw = PW, lanes = LANES, site = SITE, wout = (LANES == 4 ? 2 : 1) * PW + TAIL; };
SHAPE(PT_INF, 1, PT, 0, 2, MSM) SHAPE(PT_LD_ST, PT, PT, 0, 2, MSM) SHAPE(PNEG, PT, PT, 0, 2, MSM) SHAPE(PDBL, PT, PT, 0, 2, H2C)
SHAPE(PADD, 2 * PT, PT, 0, 2, MSM) SHAPE(PMADD_NEG, PT + 2 * V2, PT, 0, 2, MSM) SHAPE(SRTG2_MADD, PT + 3 * V2 + 1, PT, 0, 2, SRT)
SHAPE(SRTG2_DBL, PT, PT, 0, 2, SRT) SHAPE(SRTG2_ADD, 2 * PT, PT, 0, 2, SRT) SHAPE(SRTG2_XOR_LANES, PT + 1, PT, 0, 2, SRT)
SHAPE(TO_JACOBIAN, PT, PT, 0, 2, H2C) SHAPE(PDBLJ, PT, PT, 0, 2, H2C) SHAPE(TO_HOMOGENEOUS, PT, PT, 0, 2, H2C)
SHAPE(ST_VM, PT, 72, 0, 2, MSM) SHAPE(SRTG2_AFFINE_OUT, PT + 1, 0, AFF2, 2, SRT)
SHAPE(SP4_PDBLJ, PT, PT, 0, 4, H2C) SHAPE(SP4_PDBL, PT, PT, 0, 4, H2C) SHAPE(SP4_PADD, 2 * PT, PT, 0, 4, H2C)
SHAPE(SP4_TO_JACOBIAN, PT, PT, 0, 4, H2C) SHAPE(SP4_TO_HOMOGENEOUS, PT, PT, 0, 4, H2C)
SHAPE(SRTG1_MADD, P1 + 3 * NL + 1, P1, 0, 1, SRT) SHAPE(SRTG1_XOR_LANES, P1 + 1, P1, 0, 1, SRT) SHAPE(SRTG1_AFFINE_OUT, P1 + 1, 0, AFF1, 1, SRT)
SHAPE(CHAIN_ADD8_2, PT, 8 * PT, 0, 2, MSM) SHAPE(CHAIN_ADD8_4, PT, 8 * PT, 0, 4, H2C)
SHAPE(CHAIN_JAC_1_2, PT, 3 * PT, 0, 2, H2C) SHAPE(CHAIN_JAC_2_2, PT, 4 * PT, 0, 2, H2C) SHAPE(CHAIN_JAC_16_2, PT, 18 * PT, 0, 2, H2C)
SHAPE(CHAIN_JAC_60_2, PT, 62 * PT, 0, 2, H2C)
SHAPE(CHAIN_JAC_1_4, PT, 3 * PT, 0, 4, H2C) SHAPE(CHAIN_JAC_2_4, PT, 4 * PT, 0, 4, H2C) SHAPE(CHAIN_JAC_16_4, PT, 18 * PT, 0, 4, H2C)
SHAPE(CHAIN_JAC_60_4, PT, 62 * PT, 0, 4, H2C)
SHAPE(CHAIN_CANCEL_2, PT, 5 * PT, AFF2, 2, H2C) SHAPE(CHAIN_CANCEL_4, PT, 5 * PT, AFF2, 4, H2C)
SHAPE(CHAIN_RUNNING_2, 4 * PT, 8 * PT, 0, 2, MSM) SHAPE(CHAIN_RUNNING_4, 4 * PT, 8 * PT, 0, 4, H2C)
SHAPE(LANE_DIGIT, 9, 0, 2, 1, MSM) SHAPE(LANE_DIGIT_NULL, 2, 0, 1, 1, MSM) SHAPE(SRT_DIGIT_KEY, (int)SRT_SCW + 2, 0, 4, 1, SRT)

// the point routines of a chain on lane pairs and on lane quads
struct A2 {
    static __device__ __forceinline__ pt add(const pt& a, const pt& b) { return sp2::padd(a, b); }
    static __device__ __forceinline__ pt dblj(const pt& a) { return sp2::pdblj(a); }
    static __device__ __forceinline__ pt toj(const pt& a) { return sp2::to_jacobian(a); }
    static __device__ __forceinline__ pt toh(const pt& a) { return sp2::to_homogeneous(a); }
};
struct A4 {
    static __device__ __forceinline__ pt add(const pt& a, const pt& b) { return sp4::padd(a, b); }
    static __device__ __forceinline__ pt dblj(const pt& a) { return sp4::pdblj(a); }
    static __device__ __forceinline__ pt toj(const pt& a) { return sp4::to_jacobian(a); }
    static __device__ __forceinline__ pt toh(const pt& a) { return sp4::to_homogeneous(a); }
};
// a chain's steps: the point goes to the next slot of the lane's pair and comes back from it (a spare lane keeps it)
struct Slots {
    uint32_t* p;
    bool live;
    __device__ __forceinline__ void operator()(pt& P) {
        if (live) { sp2::pt_st(P, p); P = sp2::pt_ld(p); }
        p += PT;
    }
};
template <class A> __device__ __forceinline__ void chain_add8(const pt& P, Slots& st) {
    pt acc = sp2::pt_inf();
#pragma unroll 1
    for (int i = 0; i < 8; i++) { acc = A::add(acc, P); st(acc); }
}
template <class A> __device__ __forceinline__ void chain_jac(pt P, int k, Slots& st) {
    P = A::toj(P); st(P);
#pragma unroll 1
    for (int i = 0; i < k; i++) { P = A::dblj(P); st(P); }
    P = A::toh(P); st(P);
}
template <class A> __device__ __forceinline__ pt chain_cancel(const pt& P0, Slots& st) {
    pt P = A::add(P0, sp2::pneg(P0)); st(P);
    P = A::toj(P); st(P);
#pragma unroll 1
    for (int i = 0; i < 2; i++) { P = A::dblj(P); st(P); }
    P = A::toh(P); st(P);
    return P;
}
// acc += B_j, tot += acc over four buckets: ONE addition, its operands chosen by the step's parity (the loop of k_msm_lane2x)
template <class A> __device__ __forceinline__ void chain_running(const uint32_t* __restrict__ B, Slots& st) {
    pt acc = sp2::pt_inf(), tot = sp2::pt_inf();
    constexpr int nb = 4;
#pragma unroll 1
    for (int it = 0; it < 2 * nb; it++) {
        const bool first = (it & 1) == 0;
        const int j = nb - 1 - (it >> 1);
        const pt Bj = sp2::pt_ld(B + j * PT);
        pt P, Q;
#pragma unroll
        for (int e = 0; e < NL; e++) {
            P.X.v[e] = first ? acc.X.v[e] : tot.X.v[e]; P.Y.v[e] = first ? acc.Y.v[e] : tot.Y.v[e]; P.Z.v[e] = first ? acc.Z.v[e] : tot.Z.v[e];
            Q.X.v[e] = first ? Bj.X.v[e] : acc.X.v[e]; Q.Y.v[e] = first ? Bj.Y.v[e] : acc.Y.v[e]; Q.Z.v[e] = first ? Bj.Z.v[e] : acc.Z.v[e];
        }
        pt R = A::add(P, Q);
        st(R);
        if (first) acc = R; else tot = R;
    }
}

// src: the item's words; o: the item's output words (the last item's for a spare lane, which has live = false and stores nothing)
template <int OP> __device__ __forceinline__ void item_op(const uint32_t* __restrict__ src, uint32_t* __restrict__ o, bool live) {
    typedef Shape<OP> Sh;
    typedef r28::ptT<r28::fe> pt1;
    const uint32_t pair = Sh::lanes == 4 ? (threadIdx.x >> 1) & 1u : 0u;
    uint32_t* op = o + pair * Sh::pw;                      // the points of this lane's pair
    uint32_t* tail = o + (Sh::lanes == 4 ? 2 : 1) * Sh::pw;
    Slots st{op, live};
    (void)tail; (void)st;
    if constexpr (Sh::lanes == 1) {
        if constexpr (OP == SRTG1_MADD) {
            pt1 P = SrtG<1>::ld(src);
            SrtG<1>::madd(P, src + P1, src[P1 + 3 * NL]);
            if (live) SrtG<1>::st(P, o);
        }
        if constexpr (OP == SRTG1_XOR_LANES) {
            const pt1 P = SrtG<1>::ld(src);
            pt1 R;
            SrtG<1>::xor_lanes(R, P, (int)src[P1]);
            if (live) SrtG<1>::st(R, o);
        }
        if constexpr (OP == SRTG1_AFFINE_OUT) SrtG<1>::affine_out(SrtG<1>::ld(src), o, (uint8_t*)(o + 24), live && src[P1] != 0u);
        if constexpr (OP == LANE_DIGIT) {
            bool big;
            const int d = lane_digit(src, 0u, src[8], big);
            if (live) { o[0] = (uint32_t)d; o[1] = big ? 1u : 0u; }
        }
        if constexpr (OP == LANE_DIGIT_NULL) {
            bool big;
            const int d = lane_digit(src[1] ? src : nullptr, 0u, src[0], big);     // (the second word is 0: NULL only at run time, as in the kernels)
            if (live) o[0] = (uint32_t)d;
        }
        if constexpr (OP == SRT_DIGIT_KEY) {
            const uint32_t cb = src[SRT_SCW + 1], v = srt_digit_at(src, src[SRT_SCW], cb);
            uint32_t k, sign;
            const bool nz = srt_key(v, cb, k, sign);
            if (live) { o[0] = v; o[1] = k; o[2] = sign; o[3] = nz ? 1u : 0u; }
        }
    } else {
        pt R;
        bool plain = true;                                 // the result is one point, stored at op
        if constexpr (OP == PT_INF) R = sp2::pt_inf();
        if constexpr (OP == PT_LD_ST) R = sp2::pt_ld(src);
        if constexpr (OP == PNEG) R = sp2::pneg(sp2::pt_ld(src));
        if constexpr (OP == PDBL) R = sp2::pdbl(sp2::pt_ld(src));
        if constexpr (OP == PADD) R = sp2::padd(sp2::pt_ld(src), sp2::pt_ld(src + PT));
        if constexpr (OP == PMADD_NEG) {
            R = sp2::pt_ld(src);
            const sp2::h x2 = sp2::ldh(src + PT), y2 = sp2::norm(sp2::neg(sp2::ldh(src + PT + V2)));
            sp2::pmadd(R, x2, y2);
        }
        if constexpr (OP == SRTG2_MADD) { R = SrtG<2>::ld(src); SrtG<2>::madd(R, src + PT, src[PT + 3 * V2]); }
        if constexpr (OP == SRTG2_DBL) R = SrtG<2>::dbl(SrtG<2>::ld(src));
        if constexpr (OP == SRTG2_ADD) R = SrtG<2>::add(SrtG<2>::ld(src), SrtG<2>::ld(src + PT));
        if constexpr (OP == SRTG2_XOR_LANES) SrtG<2>::xor_lanes(R, SrtG<2>::ld(src), (int)src[PT]);
        if constexpr (OP == TO_JACOBIAN) R = sp2::to_jacobian(sp2::pt_ld(src));
        if constexpr (OP == PDBLJ) R = sp2::pdblj(sp2::pt_ld(src));
        if constexpr (OP == TO_HOMOGENEOUS) R = sp2::to_homogeneous(sp2::pt_ld(src));
        if constexpr (OP == SP4_PDBLJ) R = sp4::pdblj(sp2::pt_ld(src));
        if constexpr (OP == SP4_PDBL) R = sp4::pdbl(sp2::pt_ld(src));
        if constexpr (OP == SP4_PADD) R = sp4::padd(sp2::pt_ld(src), sp2::pt_ld(src + PT));
        if constexpr (OP == SP4_TO_JACOBIAN) R = sp4::to_jacobian(sp2::pt_ld(src));
        if constexpr (OP == SP4_TO_HOMOGENEOUS) R = sp4::to_homogeneous(sp2::pt_ld(src));
        if constexpr (OP == ST_VM) {
            R = sp2::pt_ld(src);
            if (live) sp2::st_vm(R, o);
            plain = false;
        }
        if constexpr (OP == SRTG2_AFFINE_OUT) {
            SrtG<2>::affine_out(SrtG<2>::ld(src), o, (uint8_t*)(o + 48), live && src[PT] != 0u);
            plain = false;
        }
        if constexpr (OP == CHAIN_ADD8_2) { chain_add8<A2>(sp2::pt_ld(src), st); plain = false; }
        if constexpr (OP == CHAIN_ADD8_4) { chain_add8<A4>(sp2::pt_ld(src), st); plain = false; }
        if constexpr (OP == CHAIN_JAC_1_2 || OP == CHAIN_JAC_2_2 || OP == CHAIN_JAC_16_2 || OP == CHAIN_JAC_60_2) {
            chain_jac<A2>(sp2::pt_ld(src), Sh::pw / PT - 2, st);
            plain = false;
        }
        if constexpr (OP == CHAIN_JAC_1_4 || OP == CHAIN_JAC_2_4 || OP == CHAIN_JAC_16_4 || OP == CHAIN_JAC_60_4) {
            chain_jac<A4>(sp2::pt_ld(src), Sh::pw / PT - 2, st);
            plain = false;
        }
        if constexpr (OP == CHAIN_CANCEL_2) {
            SrtG<2>::affine_out(chain_cancel<A2>(sp2::pt_ld(src), st), tail, (uint8_t*)(tail + 48), live);
            plain = false;
        }
        if constexpr (OP == CHAIN_CANCEL_4) {                  // both pairs run the conversion, pair 0 stores (as k_msm_horner_quads)
            SrtG<2>::affine_out(chain_cancel<A4>(sp2::pt_ld(src), st), tail, (uint8_t*)(tail + 48), live && pair == 0u);
            plain = false;
        }
        if constexpr (OP == CHAIN_RUNNING_2) { chain_running<A2>(src, st); plain = false; }
        if constexpr (OP == CHAIN_RUNNING_4) { chain_running<A4>(src, st); plain = false; }
        if (plain && live) sp2::pt_st(R, op);
    }
}

template <int OP> __device__ __forceinline__ void run_lane(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t ir = t / (uint32_t)Shape<OP>::lanes;
    const uint32_t item = ir < n ? ir : n - 1u;           // spare lanes repeat the last item
    item_op<OP>(in + (size_t)item * Shape<OP>::win, out + (size_t)item * Shape<OP>::wout, ir < n);
}
template <int OP> __global__ void __launch_bounds__(64, BLSGPU_MSM_LANE2X_WAVES) k_msm_site(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) { run_lane<OP>(in, n, out); }
template <int OP> __global__ void __launch_bounds__(64, BLSGPU_SRT_WAVES) k_srt_site(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) { run_lane<OP>(in, n, out); }
template <int OP> __global__ void __launch_bounds__(256, 2) k_h2c_site(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) { run_lane<OP>(in, n, out); }

// ---- host side ---------------------------------------------------------------------------------------------------------------
// what a routine would index memory or shift with is checked here, before the launch
template <int OP> bool items_ok(const uint32_t* in, size_t n) {
    constexpr int win = Shape<OP>::win;
    constexpr uint32_t per_wave = 64u / (uint32_t)Shape<OP>::lanes;
    if ((OP == SRTG2_XOR_LANES || OP == SRTG1_XOR_LANES) && n % per_wave != 0) return false;
    for (size_t it = 0; it < n; it++) {
        const uint32_t* p = in + it * win;
        const uint32_t last = p[win - 1];
        if ((OP == SRTG2_MADD || OP == SRTG1_MADD || OP == SRTG2_AFFINE_OUT || OP == SRTG1_AFFINE_OUT) && last > 1u) return false;
        if ((OP == SRTG2_XOR_LANES || OP == SRTG1_XOR_LANES) && (last == 0u || (last & (last - 1u)) != 0u || last >= per_wave || last != in[win - 1])) return false;
        if (OP == LANE_DIGIT && last >= (uint32_t)PIP_W) return false;
        if (OP == LANE_DIGIT_NULL && (p[0] >= (uint32_t)PIP_W || p[1] != 0u)) return false;
        if (OP == SRT_DIGIT_KEY) {
            const uint32_t w = p[SRT_SCW], cb = p[SRT_SCW + 1];
            if (cb < 5u || cb > SRT_MAXBITS || w >= (258u + cb - 1u) / cb) return false;
        }
    }
    return true;
}

template <int OP> void launch(const uint32_t* din, uint32_t n, uint32_t* dout) {
    constexpr unsigned threads = Shape<OP>::site == H2C ? 256 : 64, per = threads / Shape<OP>::lanes;
    const unsigned blocks = (n + per - 1) / per;
    if constexpr (Shape<OP>::site == MSM) k_msm_site<OP><<<dim3(blocks), dim3(threads)>>>(din, n, dout);
    if constexpr (Shape<OP>::site == SRT) k_srt_site<OP><<<dim3(blocks), dim3(threads)>>>(din, n, dout);
    if constexpr (Shape<OP>::site == H2C) k_h2c_site<OP><<<dim3(blocks), dim3(threads)>>>(din, n, dout);
}

template <int OP> int run_op(const uint32_t* in, size_t words_in, size_t n, uint32_t* out, size_t words_out) {
    if (n == 0 || n > (1u << 16) || words_in != n * (size_t)Shape<OP>::win || words_out != n * (size_t)Shape<OP>::wout) return -2;
    if (!items_ok<OP>(in, n)) return -4;
    return check::guarded_run(in, words_in * 4, out, words_out * 4, 0, [=](const uint32_t* din, uint32_t* dout) { launch<OP>(din, (uint32_t)n, dout); });
}
}  // namespace

CHECK_EXPORT(blsgpu_curve_check, uint32_t, CURVECHECK_OPS)
