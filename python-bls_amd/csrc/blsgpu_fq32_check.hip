// blsgpu_fq32_check.hip -- TEST-ONLY device library (libblsgpu_fq32check.so): every primitive of fq32.h and
// fq_mul_gfx950.h, and the LIN-round helpers of run_rounds, as a kernel of its own, one item per lane, operands and
// results as raw 32-bit words in global memory, so that tests/test_gpu_fq32.py can compare the COMPILED arithmetic word
// for word with Python integers (tests/fq32_vectors.py).  This is the layer where the device and the host compile
// different code: fq_mul_dev<> / fq_sqr_dev (inline-assembly columns), fat_reduce's device branch, inv_mad32, the
// addc / subc builtins and the DPP absorb.  Not linked into libblsgpu.so, not declared in include/blsgpu.h, not an ABI.
//
// One kernel per op (a template on the op), 256 lanes per workgroup; spare lanes of the last workgroup store nothing.
// The guard records and the return codes are check_runner.h's.  The op bodies (struct Do<OP>) also compile for the host:
// tests/test_fq32_vectors_model.py includes this file with the host compiler and runs the same bodies on fq32.h's host code
// (LIN_ABSORB and the kernels are device only).
//
// Item layouts (32-bit words):
//   a field value                     12 words, least significant first
//   a fat accumulator                 24 words: limb j is word 2j (low) and word 2j + 1 (high)
//   a LIN share (ops LIN, LIN_ABSORB) MN, K, merge flags (bits 14 / 15), levels, 30 coefficients, 30 operands of 12 words;
//                                     micro-ops 0 .. MN - 1 are the negative terms, MN .. K - 1 the positive ones, run as
//                                     run_rounds runs them: plain sums, fat_flip where it flips, plain sums, fat_reduce
//   LIN_ABSORB                        the same, then lin_absorb (blsgpu_lin_absorb.h: the kernel's own text) before the
//                                     reduce.  MN, K and levels are the ROUND's: the kernel takes them from the first lane
//                                     of the wavefront, as run_rounds takes them from the round header, so all items of a
//                                     wavefront carry the same three words.  Spare lanes run a share of zero coefficients
//                                     (they flip with the rest) and store nothing: no lane leaves before the DPP reads.
//   FQ_INV_UNI, FQ_INV_VAR_UNI        eight values per item, inverted one after the other: the caller gives every lane
//                                     of a wavefront the same item, the case fq_inv_var was written for
#include "check_runner.h"
#include "fq32.h"
#if defined(__HIPCC__)
#include "blsgpu_lin_absorb.h"
#endif

namespace {

// every op, once, with its code (tests/fq32_vectors.py pins the codes): those that also build for the host, then the device-only one
#define FQ32CHECK_HOST_OPS(X) \
    /* products */ \
    X(FQ_MUL, 0) X(FQ_MUL_RELAXED, 1) X(FQ_SQR_RELAXED, 2) \
    /* linear */ \
    X(FQ_ADD_MOD, 10) X(FQ_NEG_RAW, 11) X(FQ_SUB_MOD, 12) X(FQ_CANON, 13) X(FQ_IS_ZERO, 14) \
    /* fat accumulators and LIN shares */ \
    X(FAT_MAC_PLAIN, 20) X(FAT_FLIP, 21) X(FAT_REDUCE, 22) X(LIN, 23) \
    /* decisions */ \
    X(FQ_SGN, 30) X(GT_HALF_Q_MASK, 31) X(FQ_JACOBI_VAR, 32) \
    /* inversions */ \
    X(FQ_INV, 40) X(FQ_INV_VAR, 41) X(FQ_INV_UNI, 42) X(FQ_INV_VAR_UNI, 43)
#define FQ32CHECK_DEVICE_OPS(X) X(LIN_ABSORB, 24)
#define FQ32CHECK_OPS(X) FQ32CHECK_HOST_OPS(X) FQ32CHECK_DEVICE_OPS(X)
CHECK_ENUM(FQ32CHECK_OPS)

constexpr int NW = 12, FATW = 24;
constexpr int LIN_MAXK = 30, LIN_HDR = 4, LIN_OPS = LIN_HDR + LIN_MAXK, LIN_WIN = LIN_OPS + LIN_MAXK * NW;
constexpr int UNI = 8;

CHECK_FN void ld12(uint32_t* d, const uint32_t* p) {
#pragma unroll
    for (int j = 0; j < NW; j++) d[j] = p[j];
}
CHECK_FN void st12(const uint32_t* x, uint32_t* p) {
#pragma unroll
    for (int j = 0; j < NW; j++) p[j] = x[j];
}
CHECK_FN void ldfat(uint64_t* a, const uint32_t* p) {
#pragma unroll
    for (int j = 0; j < NW; j++) a[j] = (uint64_t)p[2 * j] | ((uint64_t)p[2 * j + 1] << 32);
}
CHECK_FN void stfat(const uint64_t* a, uint32_t* p) {
#pragma unroll
    for (int j = 0; j < NW; j++) { p[2 * j] = (uint32_t)a[j]; p[2 * j + 1] = (uint32_t)(a[j] >> 32); }
}

// one lane's share of a LIN round, in run_rounds' order: micro-ops 0 .. MN - 1, the flip, micro-ops MN .. K - 1
// (K >= 1); a lane that is not live runs zero coefficients on zero operands and reads nothing
CHECK_FN void lin_share(uint64_t (&acc)[NW], const uint32_t* in, uint32_t MN, uint32_t K, bool live) {
#pragma unroll
    for (int j = 0; j < NW; j++) acc[j] = 0;
#pragma unroll 1
    for (uint32_t p = 0; p < K; p++) {
        uint32_t S[NW], cf = 0;
#pragma unroll
        for (int j = 0; j < NW; j++) S[j] = 0;
        if (live) {
            cf = in[LIN_HDR + p] & 31u;
            ld12(S, in + LIN_OPS + p * NW);
        }
        if (p > 0 && p == MN) bls::fat_flip(acc);
        bls::fat_mac_plain(acc, S, cf);
    }
    if (MN == K) bls::fat_flip(acc);
}

// in / out words per item and the op's body
template <int OP> struct Do;
#define CHECK_OP(OP, WIN, WOUT) \
    template <> struct Do<OP> { static constexpr int win = WIN, wout = WOUT; static CHECK_MEMBER void run(const uint32_t* in, uint32_t* out); }; \
    CHECK_MEMBER void Do<OP>::run(const uint32_t* in, uint32_t* out)

// ---- products ---------------------------------------------------------------------------------------------------
CHECK_OP(FQ_MUL, 2 * NW, NW) { uint32_t a[NW], b[NW], r[NW]; ld12(a, in); ld12(b, in + NW); bls::fq_mul(r, a, b); st12(r, out); }
CHECK_OP(FQ_MUL_RELAXED, 2 * NW, NW) { uint32_t a[NW], b[NW], r[NW]; ld12(a, in); ld12(b, in + NW); bls::fq_mul_relaxed(r, a, b); st12(r, out); }
CHECK_OP(FQ_SQR_RELAXED, NW, NW) { uint32_t a[NW], r[NW]; ld12(a, in); bls::fq_sqr_relaxed(r, a); st12(r, out); }

// ---- linear -----------------------------------------------------------------------------------------------------
CHECK_OP(FQ_ADD_MOD, 2 * NW, NW) { uint32_t a[NW], s[NW]; ld12(a, in); ld12(s, in + NW); bls::fq_add_mod(a, s); st12(a, out); }
CHECK_OP(FQ_NEG_RAW, NW, NW) { uint32_t s[NW]; ld12(s, in); bls::fq_neg_raw(s); st12(s, out); }
CHECK_OP(FQ_SUB_MOD, 2 * NW, NW) { uint32_t x[NW], y[NW]; ld12(x, in); ld12(y, in + NW); bls::fq_sub_mod(x, y); st12(x, out); }
CHECK_OP(FQ_CANON, NW, NW) { uint32_t x[NW]; ld12(x, in); bls::fq_canon(x); st12(x, out); }
CHECK_OP(FQ_IS_ZERO, NW, 1) { uint32_t x[NW]; ld12(x, in); out[0] = bls::fq_is_zero(x) ? 1u : 0u; }

// ---- fat accumulators ---------------------------------------------------------------------------------------------
CHECK_OP(FAT_MAC_PLAIN, FATW + NW + 1, FATW) { uint64_t acc[NW]; uint32_t s[NW]; ldfat(acc, in); ld12(s, in + FATW);
    bls::fat_mac_plain(acc, s, in[FATW + NW]); stfat(acc, out); }
CHECK_OP(FAT_FLIP, FATW, FATW) { uint64_t acc[NW]; ldfat(acc, in); bls::fat_flip(acc); stfat(acc, out); }
CHECK_OP(FAT_REDUCE, FATW, NW) { uint64_t acc[NW]; uint32_t r[NW]; ldfat(acc, in); bls::fat_reduce(r, acc); st12(r, out); }
CHECK_OP(LIN, LIN_WIN, NW) { uint64_t acc[NW]; uint32_t r[NW]; const uint32_t K = in[1] < (uint32_t)LIN_MAXK ? in[1] : (uint32_t)LIN_MAXK;   // (a record holds 30 micro-ops)
    lin_share(acc, in, in[0], K, true); bls::fat_reduce(r, acc); st12(r, out); }
// (LIN_ABSORB has a kernel of its own below: spare lanes take part in it)
template <> struct Do<LIN_ABSORB> { static constexpr int win = LIN_WIN, wout = NW; };

// ---- decisions ----------------------------------------------------------------------------------------------------
CHECK_OP(FQ_SGN, NW, NW) { uint32_t a[NW], r[NW]; ld12(a, in); bls::fq_sgn(r, a); st12(r, out); }
CHECK_OP(GT_HALF_Q_MASK, NW, 1) { uint32_t y[NW]; ld12(y, in); out[0] = bls::gt_half_q_mask(y); }
CHECK_OP(FQ_JACOBI_VAR, NW, 1) { uint32_t a[NW]; ld12(a, in); out[0] = (uint32_t)bls::fq_jacobi_var(a); }

// ---- inversions ---------------------------------------------------------------------------------------------------
CHECK_OP(FQ_INV, NW, NW) { uint32_t a[NW], r[NW]; ld12(a, in); bls::fq_inv(r, a); st12(r, out); }
CHECK_OP(FQ_INV_VAR, NW, NW) { uint32_t a[NW], r[NW]; ld12(a, in); bls::fq_inv_var(r, a); st12(r, out); }
CHECK_OP(FQ_INV_UNI, UNI * NW, UNI * NW) {
#pragma unroll 1
    for (int t = 0; t < UNI; t++) { uint32_t a[NW], r[NW]; ld12(a, in + t * NW); bls::fq_inv(r, a); st12(r, out + t * NW); }
}
CHECK_OP(FQ_INV_VAR_UNI, UNI * NW, UNI * NW) {
#pragma unroll 1
    for (int t = 0; t < UNI; t++) { uint32_t a[NW], r[NW]; ld12(a, in + t * NW); bls::fq_inv_var(r, a); st12(r, out + t * NW); }
}

#if defined(__HIPCC__)
template <int OP> __global__ void __launch_bounds__(256) k_check(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Do<OP>::run(in + i * Do<OP>::win, out + i * Do<OP>::wout);
}
// every lane of the workgroup stays to the end: the DPP reads of lin_absorb must find their neighbours running
template <> __global__ void __launch_bounds__(256) k_check<LIN_ABSORB>(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    const uint32_t* rec = in + (live ? i : 0) * LIN_WIN;
    // the round's MN, K and levels: from the wavefront's first lane (always live), wave-uniform as in run_rounds
    const uint32_t MN = __builtin_amdgcn_readfirstlane(rec[0]), K1 = __builtin_amdgcn_readfirstlane(rec[1]);
    const uint32_t K = K1 < (uint32_t)LIN_MAXK ? K1 : (uint32_t)LIN_MAXK;
    const uint32_t levels = __builtin_amdgcn_readfirstlane(rec[3]);
    const uint32_t w1 = live ? rec[2] : 0u;
    uint64_t acc[NW];
    lin_share(acc, rec, MN, K, live);
    // lin_absorb's DPP reads need two wait states after a VALU write of their source, and the hazard recogniser does not
    // look inside its asm blocks: every limb is settled in its register pair HERE, ahead of the helper's s_nop 4, so that
    // no register copy is left to land between the blocks (tools/dpp_hazard_scan.py checks the built code object)
#pragma unroll
    for (int j = 0; j < NW; j++) asm volatile("" : "+v"(acc[j]));
    blsgpu::lin_absorb(acc, w1, levels);
    uint32_t r[NW];
    bls::fat_reduce(r, acc);
    if (live) st12(r, out + i * NW);
}

template <int OP> int run_op(const uint32_t* in, size_t words_in, size_t n, uint32_t* out, size_t words_out) {
    if (words_in != n * (size_t)Do<OP>::win || words_out != n * (size_t)Do<OP>::wout || n == 0 || n > (1u << 20)) return -2;
    const unsigned threads = 256u;
    return check::guarded_run(in, words_in * 4, out, words_out * 4, 0, [=](const uint32_t* din, uint32_t* dout) {
        k_check<OP><<<dim3((unsigned)((n + threads - 1) / threads)), dim3(threads)>>>(din, n, dout);
    });
}
#endif
}  // namespace

#if defined(__HIPCC__)
CHECK_EXPORT(blsgpu_fq32_check, uint32_t, FQ32CHECK_OPS)
#else
CHECK_HOST_ENTRY(fq32check_host, FQ32CHECK_HOST_OPS)   // (tests/test_fq32_vectors_model.py)
#endif
