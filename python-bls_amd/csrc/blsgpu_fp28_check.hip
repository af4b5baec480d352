// blsgpu_fp28_check.hip -- TEST-ONLY device library (libblsgpu_fp28check.so): every primitive of fp28.h and
// fp28_mul_gfx950.h as a kernel of its own, one item per lane, operands and results as raw limb words in global
// memory, so that tests/test_gpu_fp28.py can compare the COMPILED arithmetic limb for limb with the integer model
// (tests/fp28_vectors.py).  Not linked into libblsgpu.so, not declared in include/blsgpu.h, not an ABI.
//
// One kernel per op (a template on the op): each op is compiled the way the kernels compile it, not as one switch
// with every product alive at once.  Raw products run 64 lanes per workgroup, everything else 256; spare lanes of
// the last workgroup store nothing.  The guard records and the return codes are check_runner.h's.
//
// Ranges.  The limb arithmetic of add / sub / neg / mulc / norm / mulc_norm / conj / mul_xi is the same code for every
// F<LO, HI>; the type only says which inputs are admitted.  Each linear op is therefore instantiated here at a range
// that CONTAINS the widest one the kernels use (the sites below), and the typed products at F<0, 1> and at ranges
// whose ColumnsFit sum is the largest that compiles (pos = 8, neg = 9).  Typed r28:: sites (file:line, widest first):
//   add        F<0,1> + F<0,5>            blsgpu_h2c.hip:437, :580 (t^2 + b' + 1);  F<0,1> + F<0,1>  fp28.h padd z3, pdbl;
//                                          F2<0,1> + F2<0,1> fp28.h pmadd t4                        -> here F<4,4> + F<4,4>
//   sub        F<0,1> - F<0,3> -> F<3,1>  fp28.h pdbl d;  F<1,1> - F<0,1> -> F<2,1>  fp28.h padd t3 / t4 / t5, pmadd t3;
//              F<1,0> - F<0,1>            blsgpu_h2c.hip:446, :589                                   -> here F<4,4> - F<4,4>
//   neg        F<2,1>                     fp28.h padd neg(t4);  F<0,1>  blsgpu_g1fix.hip:174, blsgpu_g1poly.hip:198,
//                                          blsgpu_msm.hip:579, :1117, blsgpu_h2c.hip:530, :681, :797, :909,
//                                          blsgpu_subgroup.hip:73, :108, blsgpu_g2smul.hip:107     -> here F<7,7> (F<8,.> is refused)
//   mulc<3>    F<0,1>                     fp28.h pdbl;  mulc<4>, mulc<5> of one  blsgpu_h2c.hip:437, :450, :580, :598,
//                                          blsgpu_subgroup.hip:60, :93                              -> here mulc<3> F<2,2>
//   norm       F<0,6>                     blsgpu_h2c.hip:437, :580;  F<3,1> fp28.h pdbl tight (twist);  F<2,1> fp28.h
//                                          padd tight(t3), tight(t4), blsgpu_ml.hip:918;  F<0,2> blsgpu_ml.hip:768, :844,
//                                          :913, blsgpu_h2c.hip:423, :565;  F<1,1> blsgpu_fexp.hip:202  -> here F<7,7> (F<8,8> is refused)
//   mulc_norm  <12> F<4,3>                fp28.h b3 on the twist (mul_xi of padd's t5, F2<2,1>);  <12> F<2,1> b3 on G1;
//              <3> F<0,1>                 fp28.h padd / pmadd x3;  <3> F<1,0> blsgpu_ml.hip:392;  <8> F<0,1> fp28.h pdbl z8
//                                                                                                   -> here <3>, <8>, <12> F<8,8>
//   canon, is_zero  fe                    blsgpu_g1poly.hip:84, :137, :138, :252, :253, blsgpu_subgroup.hip:39,
//                                          blsgpu_ml.hip:220, :641, blsgpu_h2c.hip:461, :605, fp28.h to_vm / to_raw
//   mul        F<0,2> x F<0,2> (4)        fp28.h padd t3 / t4 / t5;  sqr F<0,1>;  dot2 on G1 at most pos 4 / neg 6
//                                          (fp28.h padd R.Z)                   -> here also 8x1, 4x2, 3x3 (neg 9), 2x2 + 2x2 ...
//   Fq2 dot2   F2<2,1> F2<1,1> F2<1,2> F2<0,1>: pos 8, neg 7  fp28.h padd R.X on the twist -- the full column, and the
//                                          same instantiation here (op F2_DOT2_W)
//   mul_xi / b3  F2<2,1>                  fp28.h padd b3(t5);  F2<0,2> pmadd                       -> here F2<4,4>
//   conj       F2<0,1>                    blsgpu_subgroup.hip:108                                   -> here F2<7,7>
//   from_raw / to_raw / to_vm / unpack32  blsgpu_h2c.hip:313, :326, :387, :423, :565, blsgpu_subgroup.hip:73
//   padd / pmadd / pdbl / pneg / padd_fn / pdbl_fn  fe and fe2: blsgpu_g1fix.hip, blsgpu_g1poly.hip, blsgpu_g2smul.hip,
//                                          blsgpu_subgroup.hip, blsgpu_h2c.hip:797 - :930, blsgpu_msm.hip:579
// (blsgpu_ml.hip and blsgpu_msm.hip keep lane-pair types of their own, S<A> / h, over the same fp28_dotK products.)
#include "check_runner.h"
#include "fp28.h"

namespace {
using namespace blsgpu::r28;

// every op, once, with its code (tests/fp28_vectors.py pins the codes)
#define FP28CHECK_OPS(X) \
    /* raw products */ \
    X(RAW_DOT1, 0) X(RAW_DOT2, 1) X(RAW_DOT3, 2) X(RAW_DOT4, 3) X(RAW_DOT6, 4) X(RAW_SQR1, 5) X(RAW_SQR2, 6) \
    /* linear / carry */ \
    X(LIN_ADD, 10) X(LIN_SUB, 11) X(LIN_NEG, 12) X(LIN_MULC3, 13) X(LIN_NORM, 14) X(LIN_MULC_NORM3, 15) X(LIN_MULC_NORM8, 16) \
    X(LIN_MULC_NORM12, 17) X(LIN_CANON, 18) X(LIN_IS_ZERO, 19) \
    /* typed products */ \
    X(T_MUL, 20) X(T_MUL_8x1, 21) X(T_MUL_4x2, 22) X(T_MUL_2x4, 23) X(T_MUL_NEG9, 24) X(T_SQR, 25) X(T_SQR_2, 26) X(T_DOT2, 27) \
    X(T_DOT2_2222, 28) X(T_DOT2_4122, 29) X(T_DOT4, 30) X(T_DOT4_21, 31) \
    /* boundaries */ \
    X(B_UNPACK32, 40) X(B_PACK32, 41) X(B_FROM_VM, 42) X(B_TO_VM, 43) X(B_FROM_RAW, 44) X(B_TO_RAW, 45) X(B_VM_MUL28, 46) \
    /* Fq2 */ \
    X(F2_MUL, 50) X(F2_MUL_W, 51) X(F2_SQR, 52) X(F2_SQR_W, 53) X(F2_DOT2, 54) X(F2_DOT2_W, 55) X(F2_MUL_XI, 56) X(F2_CONJ, 57) \
    X(F2_B3, 58) X(F2_NORM, 59) X(F2_CANON, 60) X(F2_IS_ZERO, 61) \
    /* curve: G1 at 70, the twist at 80 */ \
    X(G1_PADD, 70) X(G1_PMADD, 71) X(G1_PDBL, 72) X(G1_PNEG, 73) X(G1_PADD_FN, 74) X(G1_PDBL_FN, 75) X(G1_CHAIN8, 76) \
    X(G2_PADD, 80) X(G2_PMADD, 81) X(G2_PDBL, 82) X(G2_PNEG, 83) X(G2_PADD_FN, 84) X(G2_PDBL_FN, 85) X(G2_CHAIN8, 86)
CHECK_ENUM(FP28CHECK_OPS)

template <int LO, int HI> __device__ __forceinline__ F<LO, HI> ldF(const int32_t* p) {
    F<LO, HI> r;
#pragma unroll
    for (int j = 0; j < NL; j++) r.v[j] = p[j];
    return r;
}
template <int LO, int HI> __device__ __forceinline__ F2<LO, HI> ldF2(const int32_t* p) { return {ldF<LO, HI>(p), ldF<LO, HI>(p + NL)}; }
template <int LO, int HI> __device__ __forceinline__ void stF(const F<LO, HI>& x, int32_t* p) {
#pragma unroll
    for (int j = 0; j < NL; j++) p[j] = x.v[j];
}
template <int LO, int HI> __device__ __forceinline__ void stF(const F2<LO, HI>& x, int32_t* p) { stF(x.a, p); stF(x.b, p + NL); }
__device__ __forceinline__ void ldraw(int32_t* d, const int32_t* p) {
#pragma unroll
    for (int j = 0; j < NL; j++) d[j] = p[j];
}
template <class E> __device__ __forceinline__ ptT<E> ldpt(const int32_t* p) { return pt_ld<E>((const uint32_t*)p); }
template <class E> __device__ __forceinline__ void stpt(const ptT<E>& P, int32_t* p) { pt_st(P, (uint32_t*)p); }

// in / out words per item and the op's body
template <int OP> struct Do;
#define CHECK_OP(OP, WIN, WOUT) \
    template <> struct Do<OP> { static constexpr int win = WIN, wout = WOUT; static __device__ __forceinline__ void run(const int32_t* in, int32_t* out); }; \
    __device__ __forceinline__ void Do<OP>::run(const int32_t* in, int32_t* out)

// ---- raw products ---------------------------------------------------------------------------------------------
#define RAW_LOAD(K) int32_t x[K][NL]; _Pragma("unroll") for (int t = 0; t < K; t++) ldraw(x[t], in + t * NL); int32_t r[NL]
#define RAW_STORE _Pragma("unroll") for (int j = 0; j < NL; j++) out[j] = r[j]
CHECK_OP(RAW_DOT1, 2 * NL, NL) { RAW_LOAD(2); bls28::fp28_dot1(r, x[0], x[1]); RAW_STORE; }
CHECK_OP(RAW_DOT2, 4 * NL, NL) { RAW_LOAD(4); bls28::fp28_dot2(r, x[0], x[1], x[2], x[3]); RAW_STORE; }
CHECK_OP(RAW_DOT3, 6 * NL, NL) { RAW_LOAD(6); bls28::fp28_dot3(r, x[0], x[1], x[2], x[3], x[4], x[5]); RAW_STORE; }
CHECK_OP(RAW_DOT4, 8 * NL, NL) { RAW_LOAD(8); bls28::fp28_dot4(r, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]); RAW_STORE; }
CHECK_OP(RAW_DOT6, 12 * NL, NL) { RAW_LOAD(12); bls28::fp28_dot6(r, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], x[9], x[10], x[11]); RAW_STORE; }
CHECK_OP(RAW_SQR1, NL, NL) { RAW_LOAD(1); bls28::fp28_sqr1(r, x[0]); RAW_STORE; }
CHECK_OP(RAW_SQR2, 3 * NL, NL) { RAW_LOAD(3); bls28::fp28_sqr2(r, x[0], x[1], x[2]); RAW_STORE; }

// ---- linear / carry -------------------------------------------------------------------------------------------
CHECK_OP(LIN_ADD, 2 * NL, NL) { stF(add(ldF<4, 4>(in), ldF<4, 4>(in + NL)), out); }
CHECK_OP(LIN_SUB, 2 * NL, NL) { stF(sub(ldF<4, 4>(in), ldF<4, 4>(in + NL)), out); }
CHECK_OP(LIN_NEG, NL, NL) { stF(neg(ldF<7, 7>(in)), out); }
CHECK_OP(LIN_MULC3, NL, NL) { stF(mulc<3>(ldF<2, 2>(in)), out); }
CHECK_OP(LIN_NORM, NL, NL) { stF(norm(ldF<7, 7>(in)), out); }
CHECK_OP(LIN_MULC_NORM3, NL, NL) { stF(mulc_norm<3>(ldF<8, 8>(in)), out); }
CHECK_OP(LIN_MULC_NORM8, NL, NL) { stF(mulc_norm<8>(ldF<8, 8>(in)), out); }
CHECK_OP(LIN_MULC_NORM12, NL, NL) { stF(mulc_norm<12>(ldF<8, 8>(in)), out); }
CHECK_OP(LIN_CANON, NL, NL) { stF(canon(ldF<0, 1>(in)), out); }
CHECK_OP(LIN_IS_ZERO, NL, 1) { out[0] = is_zero(ldF<0, 1>(in)) ? 1 : 0; }

// ---- typed products -------------------------------------------------------------------------------------------
CHECK_OP(T_MUL, 2 * NL, NL) { stF(mul(ldF<0, 1>(in), ldF<0, 1>(in + NL)), out); }
CHECK_OP(T_MUL_8x1, 2 * NL, NL) { stF(mul(ldF<8, 8>(in), ldF<1, 1>(in + NL)), out); }
CHECK_OP(T_MUL_4x2, 2 * NL, NL) { stF(mul(ldF<4, 4>(in), ldF<2, 2>(in + NL)), out); }
CHECK_OP(T_MUL_2x4, 2 * NL, NL) { stF(mul(ldF<2, 2>(in), ldF<4, 4>(in + NL)), out); }
CHECK_OP(T_MUL_NEG9, 2 * NL, NL) { stF(mul(ldF<3, 0>(in), ldF<0, 3>(in + NL)), out); }
CHECK_OP(T_SQR, NL, NL) { stF(sqr(ldF<0, 1>(in)), out); }
CHECK_OP(T_SQR_2, NL, NL) { stF(sqr(ldF<2, 2>(in)), out); }
CHECK_OP(T_DOT2, 4 * NL, NL) { stF(dot2(ldF<0, 1>(in), ldF<0, 1>(in + NL), ldF<0, 1>(in + 2 * NL), ldF<0, 1>(in + 3 * NL)), out); }
CHECK_OP(T_DOT2_2222, 4 * NL, NL) { stF(dot2(ldF<2, 2>(in), ldF<2, 2>(in + NL), ldF<2, 2>(in + 2 * NL), ldF<2, 2>(in + 3 * NL)), out); }
CHECK_OP(T_DOT2_4122, 4 * NL, NL) { stF(dot2(ldF<4, 4>(in), ldF<1, 1>(in + NL), ldF<2, 2>(in + 2 * NL), ldF<2, 2>(in + 3 * NL)), out); }
CHECK_OP(T_DOT4, 8 * NL, NL) {
    stF(dot4(ldF<0, 1>(in), ldF<0, 1>(in + NL), ldF<0, 1>(in + 2 * NL), ldF<0, 1>(in + 3 * NL),
             ldF<0, 1>(in + 4 * NL), ldF<0, 1>(in + 5 * NL), ldF<0, 1>(in + 6 * NL), ldF<0, 1>(in + 7 * NL)), out);
}
CHECK_OP(T_DOT4_21, 8 * NL, NL) {
    stF(dot4(ldF<2, 2>(in), ldF<1, 1>(in + NL), ldF<2, 2>(in + 2 * NL), ldF<1, 1>(in + 3 * NL),
             ldF<2, 2>(in + 4 * NL), ldF<1, 1>(in + 5 * NL), ldF<2, 2>(in + 6 * NL), ldF<1, 1>(in + 7 * NL)), out);
}

// ---- boundaries -----------------------------------------------------------------------------------------------
CHECK_OP(B_UNPACK32, 12, NL) { uint32_t w[12];
#pragma unroll
    for (int j = 0; j < 12; j++) w[j] = (uint32_t)in[j];
    stF(unpack32(w), out); }
CHECK_OP(B_PACK32, NL, 12) { uint32_t w[12]; pack32(w, ldF<0, 1>(in));
#pragma unroll
    for (int j = 0; j < 12; j++) out[j] = (int32_t)w[j]; }
CHECK_OP(B_FROM_VM, 12, NL) { uint32_t w[12];
#pragma unroll
    for (int j = 0; j < 12; j++) w[j] = (uint32_t)in[j];
    stF(from_vm(w), out); }
CHECK_OP(B_TO_VM, NL, 12) { uint32_t w[12]; to_vm(w, ldF<0, 1>(in));
#pragma unroll
    for (int j = 0; j < 12; j++) out[j] = (int32_t)w[j]; }
CHECK_OP(B_FROM_RAW, 12, NL) { uint32_t w[12];
#pragma unroll
    for (int j = 0; j < 12; j++) w[j] = (uint32_t)in[j];
    stF(from_raw(w), out); }
CHECK_OP(B_TO_RAW, NL, 12) { uint32_t w[12]; to_raw(w, ldF<0, 1>(in));
#pragma unroll
    for (int j = 0; j < 12; j++) out[j] = (int32_t)w[j]; }
CHECK_OP(B_VM_MUL28, 24, 12) { uint32_t a[12], b[12], d[12];
#pragma unroll
    for (int j = 0; j < 12; j++) { a[j] = (uint32_t)in[j]; b[j] = (uint32_t)in[12 + j]; }
    vm_mul28(d, a, b);
#pragma unroll
    for (int j = 0; j < 12; j++) out[j] = (int32_t)d[j]; }

// ---- Fq2 --------------------------------------------------------------------------------------------------------
constexpr int N2 = 2 * NL;
CHECK_OP(F2_MUL, 2 * N2, N2) { stF(mul(ldF2<0, 1>(in), ldF2<0, 1>(in + N2)), out); }
CHECK_OP(F2_MUL_W, 2 * N2, N2) { stF(mul(ldF2<2, 2>(in), ldF2<2, 2>(in + N2)), out); }
CHECK_OP(F2_SQR, N2, N2) { stF(sqr(ldF2<0, 1>(in)), out); }
CHECK_OP(F2_SQR_W, N2, N2) { stF(sqr(ldF2<0, 2>(in)), out); }
CHECK_OP(F2_DOT2, 4 * N2, N2) { stF(dot2(ldF2<0, 1>(in), ldF2<0, 1>(in + N2), ldF2<0, 1>(in + 2 * N2), ldF2<0, 1>(in + 3 * N2)), out); }
CHECK_OP(F2_DOT2_W, 4 * N2, N2) { stF(dot2(ldF2<2, 1>(in), ldF2<1, 1>(in + N2), ldF2<1, 2>(in + 2 * N2), ldF2<0, 1>(in + 3 * N2)), out); }
CHECK_OP(F2_MUL_XI, N2, N2) { stF(mul_xi(ldF2<4, 4>(in)), out); }
CHECK_OP(F2_CONJ, N2, N2) { stF(conj(ldF2<7, 7>(in)), out); }
CHECK_OP(F2_B3, N2, N2) { stF(b3(ldF2<4, 4>(in)), out); }
CHECK_OP(F2_NORM, N2, N2) { stF(norm(ldF2<7, 7>(in)), out); }
CHECK_OP(F2_CANON, N2, N2) { stF(canon(ldF2<0, 1>(in)), out); }
CHECK_OP(F2_IS_ZERO, N2, 1) { out[0] = is_zero(ldF2<0, 1>(in)) ? 1 : 0; }

// ---- curve: a point is X, Y, Z (3 x DW words); pmadd takes P and then x2, y2; chain8 takes P and eight Q -----------------
template <class E> struct Curve {
    static constexpr int DW = Elem<E>::DW, PW = 3 * DW;
    static __device__ __forceinline__ void do_padd(const int32_t* in, int32_t* out) { stpt(padd(ldpt<E>(in), ldpt<E>(in + PW)), out); }
    static __device__ __forceinline__ void do_pmadd(const int32_t* in, int32_t* out) {
        ptT<E> P = ldpt<E>(in);
        const E x2 = Elem<E>::load((const uint32_t*)in + PW), y2 = Elem<E>::load((const uint32_t*)in + PW + DW);
        pmadd(P, x2, y2);
        stpt(P, out);
    }
    static __device__ __forceinline__ void do_pdbl(const int32_t* in, int32_t* out) { stpt(pdbl(ldpt<E>(in)), out); }
    static __device__ __forceinline__ void do_pneg(const int32_t* in, int32_t* out) { stpt(pneg(ldpt<E>(in)), out); }
    static __device__ __forceinline__ void do_padd_fn(const int32_t* in, int32_t* out) { stpt(padd_fn<E>(ldpt<E>(in), ldpt<E>(in + PW)), out); }
    static __device__ __forceinline__ void do_pdbl_fn(const int32_t* in, int32_t* out) { stpt(pdbl_fn<E>(ldpt<E>(in)), out); }
    // eight additions in a row, nothing canonical in between: the accumulator stays in product form (-q, 2q)
    static __device__ __forceinline__ void do_chain8(const int32_t* in, int32_t* out) {
        ptT<E> A = ldpt<E>(in);
#pragma unroll 1
        for (int k = 1; k <= 8; k++) A = padd(A, ldpt<E>(in + k * PW));
        stpt(A, out);
    }
};
#define CURVE_OPS(G, E) \
    CHECK_OP(G##_PADD, 2 * Curve<E>::PW, Curve<E>::PW) { Curve<E>::do_padd(in, out); } \
    CHECK_OP(G##_PMADD, Curve<E>::PW + 2 * Curve<E>::DW, Curve<E>::PW) { Curve<E>::do_pmadd(in, out); } \
    CHECK_OP(G##_PDBL, Curve<E>::PW, Curve<E>::PW) { Curve<E>::do_pdbl(in, out); } \
    CHECK_OP(G##_PNEG, Curve<E>::PW, Curve<E>::PW) { Curve<E>::do_pneg(in, out); } \
    CHECK_OP(G##_PADD_FN, 2 * Curve<E>::PW, Curve<E>::PW) { Curve<E>::do_padd_fn(in, out); } \
    CHECK_OP(G##_PDBL_FN, Curve<E>::PW, Curve<E>::PW) { Curve<E>::do_pdbl_fn(in, out); } \
    CHECK_OP(G##_CHAIN8, 9 * Curve<E>::PW, Curve<E>::PW) { Curve<E>::do_chain8(in, out); }
CURVE_OPS(G1, fe)
CURVE_OPS(G2, fe2)

template <int OP> __global__ void __launch_bounds__(OP < LIN_ADD ? 64 : 256) k_check(const int32_t* __restrict__ in, size_t n, int32_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Do<OP>::run(in + i * Do<OP>::win, out + i * Do<OP>::wout);
}

template <int OP> int run_op(const int32_t* in, size_t words_in, size_t n, int32_t* out, size_t words_out) {
    if (words_in != n * (size_t)Do<OP>::win || words_out != n * (size_t)Do<OP>::wout || n == 0 || n > (1u << 20)) return -2;
    const unsigned threads = OP < LIN_ADD ? 64u : 256u;
    return check::guarded_run(in, words_in * 4, out, words_out * 4, 0, [=](const int32_t* din, int32_t* dout) {
        k_check<OP><<<dim3((unsigned)((n + threads - 1) / threads)), dim3(threads)>>>(din, n, dout);
    });
}
}  // namespace

CHECK_EXPORT(blsgpu_fp28_check, int32_t, FP28CHECK_OPS)
