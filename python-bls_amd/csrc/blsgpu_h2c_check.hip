// blsgpu_h2c_check.hip -- TEST-ONLY device library (libblsgpu_h2ccheck.so): the register layer behind hash to G2, hash to G1 and
// decompression -- namespace swl and the fixed-exponent powers of blsgpu_h2c.hip, the helpers of blsgpu_h2g1.hip and the SHA-256
// block both share -- as kernels of their own, one item per lane, operands and results as 32-bit words in global memory, so that
// tests/test_gpu_h2c_check.py can compare the COMPILED routines word for word with the limb model (tests/h2c_vectors.py) and check
// the device's own words in plain integers.  Not linked into libblsgpu.so, not declared in include/blsgpu.h, not an ABI.
//
// The routines are the production ones: this file includes the kernel texts the way blsgpu_api.hip does, with a BLSGPU_TU value no
// kernel group has, so no production kernel body is emitted (blsgpu_tu.h).  One kernel per op (a template on the op); spare lanes
// of the last workgroup store nothing.  The guard records and the return codes are check_runner.h's; at most 4096 items per call.
// Where a routine returns an fe, the op stores the 14 raw limbs AND the 12 words of to_vm (FE = 26 words).
//
// No routine here has a host build: fp28.h is device code only and every routine below is __device__, so the op bodies are too
// (tests/test_h2c_vectors_model.py compiles this file for the device with -fsyntax-only; the model stands in for a host build).
//
// TWO LOOPS ARE INLINE in their kernels and cannot be called, so their bodies are COPIED here, not called: k_pow's window loop
// (POW_LOOP_WIN) and k_pow2's two-wave base-4 loop (POW_LOOP_B4).  The kernels themselves run in tests/test_gpu_h2c_check.py through
// two engines (BLSGPU_POW2_MAX = 0 and above any size).  FE1_REDUCE is a third copy: the last statement of field_element<1>, on
// digests the caller chooses (no 512-bit value with hi = 0 or lo = q can be found through SHA-256).
//
// Every F<A, B> the call sites hand to chi, sgn, inv, pow_e and sel is fe = F<0, 1> (the result of a product or of norm): the sites
// differ in the VALUE that type carries, not in the instantiation.  red is instantiated at F<0, 2> and F<1, 1>, stv at F<0, 1> (products,
// constants) and F<0, 2> (add(one, mul(...)) of k_h2c_sw2 / swj2) and nowhere with negative digits.  Ops, call sites and the value
// range each site delivers (digits 0 .. 12 in [0, 2^28) throughout):
//   JACOBI_BIN       12 canonical words -> 1.  swl::jacobi: chi's answer to fq_jacobi_var = 2, and chi itself under
//                    BLSGPU_H2C_BINARY_JACOBI; the operand is to_raw's output: canonical
//   CHI              14 limbs -> 1.  k_h2c_swj0 nc (dot2), k_h2c_swj1 dp (mul), k_h2g1 uc (red): products, (-q, 2q)
//   SGN              14 limbs -> 1.  k_h2c_sw0 / swj0 tv.b: from_raw (-q, 2q) or, WIDE, norm of a sum of two products (-2q, 4q);
//                    k_h2c_sw2 / swj2 x1c (mul); k_h2g1 t (from_raw or red) and y (mul; norm(neg(y)) is never passed)
//   RED_02, RED_11   14 limbs -> FE.  red<0, 2>: add of two fe (k_h2c_sw0 / swj0 u, k_h2c_sw1 inner, k_h2c_sw2 / swj2 x0 + x0, k_h2g1 w,
//                    uc, field_element<1>): (-2q, 4q);  red<1, 1>: sub of two fe (k_h2c_sw1 p1 - p2, k_h2c_sw2 / swj2 y0 - 1): (-3q, 3q)
//   INV              14 limbs -> FE.  k_h2c_sw0 / swj0 (dot2), k_h2c_sw2 / swj2 (red), k_h2g1 (mul): (-q, 2q); 0 -> 0
//   SCALE            fe2, fe -> 2 FE.  k_h2c_sw0 / swj0: products
//   LDV_STV          slot a, slot b, slot z, 14 limbs -> an image of H1_IMG x 12 words: stv<0, 2> at a, ldv from a, stv<0, 1> of that at
//                    b, st_zero at z; every other word of the image stays as the runner filled it.  The kernels name slots
//                    BLSVM_H1_T (= STATE0, k_h2c_sw0) .. BLSVM_H1_S + 5 NE - 1 (= STATE1 - 1, k_h2c_sw2 / swj2)
//   POW_E            14 limbs -> FE.  k_h2g1 u (red): (-q, 2q)
//   POW_LOOP_WIN     12 words (the VM's form, any value below 2^384) -> FE.  k_pow: slots BASE of the image, written by stv
//                    (canonical) or by the VM (below 2q)
//   POW_LOOP_B4      the same through k_pow2's loop: 256-thread workgroups, two sets of 64 values, LDS posts; spare lanes repeat
//                    the last value (vr < total ? vr : total - 1)
//   FIELD_ELEMENT_0  24 words (t_0 || t_1, 48 bytes big-endian each) -> 2 FE (j = 0, 1): any value below 2^384
//   FIELD_ELEMENT_1  8 words (a message hash) -> 2 FE (j = 0, 1)
//   FE1_REDUCE       16 words (a 64-byte digest as sha256_block leaves it: word 0 most significant) -> FE   (copied)
//   SEL              c, fe, fe -> 14 limbs; c differs between lanes
//   SHA256_BLOCK     16 words -> 8
// Launch bounds are the tightest of an op's call sites: (256, 2) of k_h2c_swj0 for CHI, SGN, RED_*, INV, SCALE and LDV_STV (the
// k_h2c_sw* kernels' (64) and the other sites' (256) allow more registers), (256) of k_h2g1 / k_pow / k_pow2 for the rest.
// The host side refuses, before anything is launched (-4): an LDV_STV slot outside [BLSVM_H1_STATE0, BLSVM_H1_STATE1).
#include "check_runner.h"
#define BLSGPU_TU 99                                       // no kernel group: declarations only
#include "blsgpu_tu.h"
#include "blsgpu_kernels.hip"
#include "fp28.h"
#include "blsgpu_ml.hip"
#include "blsgpu_msm.hip"                                  // sp2 / sp4, the point arithmetic blsgpu_h2c.hip's clearing kernels name
#include "blsgpu_g1fix.hip"                                // g1fix::Gen of k_h2g1
#include "blsgpu_h2c.hip"
#include "blsgpu_h2g1.hip"

namespace {
using namespace blsgpu;
using r28::NL;
using r28::fe;

// every op, once, with its code (tests/h2c_vectors.py pins the codes)
#define H2CCHECK_OPS(X) \
    X(JACOBI_BIN, 0) X(CHI, 1) X(SGN, 2) X(RED_02, 3) X(RED_11, 4) X(INV, 5) X(SCALE, 6) X(LDV_STV, 7) \
    X(POW_E, 10) X(POW_LOOP_WIN, 11) X(POW_LOOP_B4, 12) \
    X(FIELD_ELEMENT_0, 20) X(FIELD_ELEMENT_1, 21) X(FE1_REDUCE, 22) X(SEL, 23) X(SHA256_BLOCK, 24)
CHECK_ENUM(H2CCHECK_OPS)
constexpr int FE = NL + 12, IMG_DW = (int)H1_IMG * 12;
constexpr size_t MAX_ITEMS = 1u << 12;

template <int A, int B> __device__ __forceinline__ r28::F<A, B> ldF(const int32_t* p) {
    r28::F<A, B> r;
#pragma unroll
    for (int j = 0; j < NL; j++) r.v[j] = p[j];
    return r;
}
__device__ __forceinline__ void ldw(uint32_t* d, const int32_t* p, int n) {
#pragma unroll
    for (int j = 0; j < n; j++) d[j] = (uint32_t)p[j];
}
// an fe result: the limbs as they are, then the words of to_vm
__device__ __forceinline__ void stFE(const fe& x, int32_t* p) {
    uint32_t y[12];
    r28::to_vm(y, x);
#pragma unroll
    for (int j = 0; j < NL; j++) p[j] = x.v[j];
#pragma unroll
    for (int j = 0; j < 12; j++) p[NL + j] = (int32_t)y[j];
}

// in / out words per item and the op's body
template <int OP> struct Do;
#define CHECK_OP(OP, WIN, WOUT) \
    template <> struct Do<OP> { static constexpr int win = WIN, wout = WOUT; static __device__ __forceinline__ void run(const int32_t* in, int32_t* out); }; \
    __device__ __forceinline__ void Do<OP>::run(const int32_t* in, int32_t* out)

CHECK_OP(JACOBI_BIN, 12, 1) { uint32_t a[12]; ldw(a, in, 12); out[0] = swl::jacobi(a); }
CHECK_OP(CHI, NL, 1) { out[0] = swl::chi(ldF<0, 1>(in)); }
CHECK_OP(SGN, NL, 1) { out[0] = swl::sgn(ldF<0, 1>(in)) ? 1 : 0; }
CHECK_OP(RED_02, NL, FE) { stFE(swl::red(ldF<0, 2>(in)), out); }
CHECK_OP(RED_11, NL, FE) { stFE(swl::red(ldF<1, 1>(in)), out); }
CHECK_OP(INV, NL, FE) { stFE(swl::inv(ldF<0, 1>(in)), out); }
CHECK_OP(SCALE, 3 * NL, 2 * FE) {
    const r28::fe2 x = {ldF<0, 1>(in), ldF<0, 1>(in + NL)};
    const r28::fe2 r = swl::scale(x, ldF<0, 1>(in + 2 * NL));
    stFE(r.a, out); stFE(r.b, out + FE);
}
CHECK_OP(LDV_STV, 3 + NL, IMG_DW) {
    uint32_t* img = (uint32_t*)out;
    swl::stv(img, (uint32_t)in[0], ldF<0, 2>(in + 3));
    const fe x = swl::ldv(img, (uint32_t)in[0]);
    swl::stv(img, (uint32_t)in[1], x);
    swl::st_zero(img, (uint32_t)in[2]);
}
CHECK_OP(POW_E, NL, FE) { stFE(h2g1::pow_e(ldF<0, 1>(in)), out); }
CHECK_OP(POW_LOOP_WIN, 12, FE) {                           // (copied from k_pow: from_vm, the window loop; to_vm is stFE's)
    constexpr int NT = 1 << (BLSVM_POW_WINDOW - 1);
    r28::fe tbl[NT], a;
    {
        uint32_t x[12];
        ldw(x, in, 12);
        tbl[0] = r28::from_vm(x);
    }
    const r28::fe t = r28::sqr(tbl[0]);
#pragma unroll
    for (int i = 1; i < NT; i++) tbl[i] = r28::mul(tbl[i - 1], t);
    auto pick = [&](uint32_t k) {
        r28::fe m;
#pragma unroll
        for (int j = 0; j < r28::NL; j++) {
            m.v[j] = tbl[0].v[j];
#pragma unroll
            for (int i = 1; i < NT; i++) m.v[j] = (k == (uint32_t)i) ? tbl[i].v[j] : m.v[j];
        }
        return m;
    };
    a = pick(BLSVM_POW_WIN[0][1]);
#pragma unroll 1
    for (int s = 1; s < BLSVM_POW_STEPS; s++) {
        const uint32_t nsq = BLSVM_POW_WIN[s][0], k = BLSVM_POW_WIN[s][1];
#pragma unroll 1
        for (uint32_t i = 0; i < nsq; i++) a = r28::sqr(a);
        if (k != 255u) a = r28::mul(a, pick(k));
    }
    stFE(a, out);
}
template <> struct Do<POW_LOOP_B4> { static constexpr int win = 12, wout = FE; };      // (its body is its kernel below)
CHECK_OP(FIELD_ELEMENT_0, 24, 2 * FE) {
    stFE(h2g1::field_element<0>((const uint32_t*)in, 0, 0), out);
    stFE(h2g1::field_element<0>((const uint32_t*)in, 0, 1), out + FE);
}
CHECK_OP(FIELD_ELEMENT_1, 8, 2 * FE) {
    stFE(h2g1::field_element<1>((const uint32_t*)in, 0, 0), out);
    stFE(h2g1::field_element<1>((const uint32_t*)in, 0, 1), out + FE);
}
CHECK_OP(FE1_REDUCE, 16, FE) {                             // (copied from field_element<1>: what follows the two sha256_block calls)
    uint32_t be[16], lo[12], hi[12];
    ldw(be, in, 16);
#pragma unroll
    for (int k = 0; k < 12; k++) { lo[k] = be[15 - k]; hi[k] = k < 4 ? be[3 - k] : 0u; }
    const int32_t c2[r28::NL] = BLS28_WIDE_C2;
    stFE(swl::red(r28::add(r28::from_raw(lo), r28::mul(r28::unpack32(hi), r28::fe_const(c2)))), out);
}
CHECK_OP(SEL, 1 + 2 * NL, NL) {
    const fe r = h2g1::sel(in[0] != 0, ldF<0, 1>(in + 1), ldF<0, 1>(in + 1 + NL));
#pragma unroll
    for (int j = 0; j < NL; j++) out[j] = r.v[j];
}
CHECK_OP(SHA256_BLOCK, 16, 8) {
    uint32_t w[16], d[8];
    ldw(w, in, 16);
    sha256_block(w, d);
#pragma unroll
    for (int j = 0; j < 8; j++) out[j] = (int32_t)d[j];
}

constexpr bool swj0_site(int op) { return op == CHI || op == SGN || op == RED_02 || op == RED_11 || op == INV || op == SCALE || op == LDV_STV; }

template <int OP> __global__ void __launch_bounds__(256, swj0_site(OP) ? 2 : 1) k_check(const int32_t* __restrict__ in, uint32_t n, int32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Do<OP>::run(in + (size_t)i * Do<OP>::win, out + (size_t)i * Do<OP>::wout);
}
// (copied from k_pow2: value v of `total` is item v; set, wave, posts, digits and the four final products as there)
template <> __global__ void __launch_bounds__(256) k_check<POW_LOOP_B4>(const int32_t* __restrict__ in, uint32_t total, int32_t* __restrict__ out) {
    __shared__ int32_t posts[2][2][r28::NL][64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t set = wv >> 1, wave = wv & 1u;
    int32_t (*post)[r28::NL][64] = posts[set];
    const uint32_t vr = (blockIdx.x * 2u + set) * 64u + lane;
    const uint32_t v = vr < total ? vr : total - 1u;
    const int32_t* src = in + (size_t)v * 12;
    int32_t* dst = out + (size_t)v * FE;
    constexpr uint32_t DIGITS = (BLSVM_POW_E_BITS + 1) / 2;
    auto digit = [&](uint32_t j) { return (BLSVM_POW_E[(2u * j) >> 5] >> ((2u * j) & 31u)) & 3u; };
    r28::fe p;
    if (wave == 0u) {
        uint32_t x[12];
        ldw(x, src, 12);
        p = r28::from_vm(x);
    }
    r28::fe B1 = r28::fe_one(), B2 = r28::fe_one(), B3 = r28::fe_one();
#pragma unroll 1
    for (uint32_t j = 0; j < DIGITS; j++) {
        if (wave == 0u) {
#pragma unroll
            for (int l = 0; l < r28::NL; l++) post[j & 1u][l][lane] = p.v[l];
        }
        __syncthreads();
        if (wave == 0u) {
            if (j + 1u < DIGITS) p = r28::sqr(r28::sqr(p));
        } else {
            const uint32_t d = digit(j);
            if (d != 0u) {
                r28::fe q;
#pragma unroll
                for (int l = 0; l < r28::NL; l++) q.v[l] = post[j & 1u][l][lane];
                if (d == 1u) B1 = r28::mul(B1, q);
                else if (d == 2u) B2 = r28::mul(B2, q);
                else B3 = r28::mul(B3, q);
            }
        }
    }
    if (wave == 1u) {
        r28::fe run = r28::mul(B3, B2);
        r28::fe acc = r28::mul(B3, run);
        run = r28::mul(run, B1);
        acc = r28::mul(acc, run);
        if (vr < total) stFE(acc, dst);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
template <int OP> bool args_ok(const int32_t* in, size_t n) {
    if (OP != LDV_STV) return true;
    for (size_t it = 0; it < n; it++)
        for (int s = 0; s < 3; s++) {
            const int32_t slot = in[it * Do<OP>::win + s];
            if (slot < (int32_t)BLSVM_H1_STATE0 || slot >= (int32_t)BLSVM_H1_STATE1) return false;
        }
    return true;
}

template <int OP> int run_op(const int32_t* in, size_t words_in, size_t n, int32_t* out, size_t words_out) {
    if (n == 0 || n > MAX_ITEMS || words_in != n * (size_t)Do<OP>::win || words_out != n * (size_t)Do<OP>::wout) return -2;
    if (!args_ok<OP>(in, n)) return -4;
    const unsigned blocks = OP == POW_LOOP_B4 ? (unsigned)((n + 127) / 128) : (unsigned)((n + 255) / 256);
    return check::guarded_run(in, words_in * 4, out, words_out * 4, 0, [=](const int32_t* din, int32_t* dout) {
        k_check<OP><<<dim3(blocks), dim3(256)>>>(din, (uint32_t)n, dout);
    });
}
}  // namespace

CHECK_EXPORT(blsgpu_h2c_check, int32_t, H2CCHECK_OPS)
