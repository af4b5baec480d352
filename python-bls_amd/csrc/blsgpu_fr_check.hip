// blsgpu_fr_check.hip -- TEST-ONLY device library (libblsgpu_frcheck.so): every routine of the scalar-field and byte-hashing
// layer -- fr_scalar.h, hd_derive.h, hash_pks.h, sigdiv.h, secret_window.h -- as a kernel of its own, one item per lane,
// operands and results as raw 32-bit words in global memory, so that tests/test_gpu_fr.py can compare the COMPILED routines
// word for word with Python integers, hashlib / hmac and the window models (tests/fr_vectors.py).  The host tests of these
// headers (test_lagrange_host, test_frsecret_host, test_hd_host, test_seeds_host, test_secure_agg_host, test_sigdiv_host)
// compile them with the host compiler; the device compiles v_mad_u64_u32 chains, loops held by `#pragma unroll 1`,
// dynamically indexed constant arrays (e[b >> 5], K[64]), byte loads at any alignment, lanes of one wavefront with different
// block counts and the masked selects.  secret_window.h has no host build at all.
// Not linked into libblsgpu.so, not declared in include/blsgpu.h, not an ABI.
//
// One kernel per op (a template on the op), 256 lanes per workgroup; spare lanes of the last workgroup store nothing.  The
// guard records and the return codes are check_runner.h's.
// The op bodies (struct Do<OP>) also compile for the host: tests/test_fr_vectors_model.py includes this file with the host
// compiler and runs the same bodies on the same records (the `window` group and the kernels are device only).
//
// Item layouts (32-bit words).  A SCALAR is 8 words, least significant first.  BYTES are the bytes as they lie in memory,
// four to a word (so 32 bytes big-endian are 8 words); a byte pointer is the record's own address.
//   LAGRANGE_WEIGHT   k, j, then MAXK points of 8 words      LAGRANGE_DEN   k, then MAXK shifts
//   POLY_HORNER       t, xm, then MAXT coefficients          SUM_TERM       y (bytes), acc
//   SHA_COMPRESS      state, block                           HMAC_KEY       klen, 64 key bytes -> ipad, opad
//   PAD_HMAC_BLOCK    len, ipad, opad, 56 message bytes -> the padded block, the digest
//   CHILD_HMACS       sw, index, ipad, opad, ser[12]         PATH_STEP      sw, index, chain, ser[12]   -> i_left, i_right
//   LONG_WORD         len, 1 with a suffix, suffix, off, shift, message   HMAC_LONG      len, suffix, shift, ipad, opad, message
//   HMAC_LONG_PAIR    len, shift, ipad, opad, message        (the message begins `shift` bytes, 0 .. 3, into its MSGW words)
//   HPK_DIGEST        k, three words of padding (the keys start on 16 bytes), MAXKEYS keys of 12 words
//   RECODE_G1 / _G2   a scalar (32 bytes big-endian) -> sgn, ad, mz of the digits w = 0 .. 64, through a column of LDS:
//                     _G1 with COLS = 256 and one scalar per lane (k_fix_mul_secret, k_poly_eval_secret), _G2 with COLS =
//                     g2smul::PAIRS and one scalar per lane PAIR, both lanes writing the column (k_g2_smul); the even lane stores
//   SELECT_G1         ad, keep0, a table of TAB x ENTRY_DW words at stride 1 -> select_entry<g1fix::ENTRY_DW, true>
//   SELECT_G2         select_entry<g2smul::PT_DW, false> on the lane-strided layout of k_g2_smul_table: the call's input is
//                     ad, keep0 of every item (2 n words), then dword d of item i's table at word 2 n + d n + i
//
// CALL SITES and the operand range each can deliver (the `below n` contract of fr_scalar.h, settled here):
//   frs::mul(r, a, b)     every outer step leaves t < a + n (t' = (t + a b_i + m n) / 2^32 with b_i, m < 2^32), so with
//                         a < n the running sum stays below 2n < 2^256 WHATEVER b is, the one subtraction makes it canonical
//                         and the result is the integer a b / R mod n.  With a >= n the sum can pass 2^256 and the carry
//                         out of `t[8] + (uint32_t)c` is lost: a must be below n, b may be any 256-bit value.  The class
//                         `wide_b` (b in [n, 2^256), a below n) holds that; `a >= n` is outside the contract and is asked of
//                         no call site:
//       k_lagrange            lagrange_weight p (p, d: results of neg / sub / mul / the constant R mod n: below n);
//                             l = mul(shift, den) (results of inv: below n)
//       inv / sqr             results of mul and the caller's a: lagrange_weight's p, lagrange_den's sum of add results,
//                             sigdiv::exponent's result -- all below n
//       to_mont(a) = mul(a, R^2)   lagrange_point (refuses x = 0 and x >= n BEFORE converting: status 0 for a caller's
//                             point at or above n); dot_term / dot_term_masked's coefficient l (below); poly_point,
//                             poly_coeff_masked, sigdiv::exponent (reduce_n / reduce_n_masked first: any 256-bit value
//                             arrives below n); k_share_weights r (a 64-bit weight)
//       from_mont(a) = mul(a, 1)   results of mul
//       dot_term(l, y), dot_term_masked(l, y)   y: caller bytes, reduced first.  l: NEVER caller bytes -- k_fr_dot and
//                             k_fr_scale_secret read the workspace k_lagrange wrote (from_mont results, or zeros for a refused
//                             group), k_fr_dot_secret that workspace or the exponents k_hash_pks_exp wrote (hpk::exponent
//                             ends in reduce_n); no export takes coefficients for a dot product from its caller
//       k_share_weights       mul(w, l): w = to_mont(r) below n, l from k_lagrange's workspace
//       sigdiv::cross_equal, quotient_scalar   operands from sigdiv::exponent
//       poly_horner_masked    mul_masked(acc, xm): acc a coefficient from poly_coeff_masked or an add_masked result, xm from
//                             poly_point
//     So no site hands mul an `a` at or above n, and no caller's unchecked bytes reach an operand of mul, mul_masked, to_mont
//     or the coefficient of a dot_term: every path reduces (reduce_n, 2^256 < 3n) or refuses (lagrange_point) first.
//   hdk::sub_n_if_ge      mul's t (below 2n), add_mod_n's sum (below 2n), reduce_n (any value below 2^256 < 3n)
//   hdk::reduce_n / _masked   caller bytes of any value: HMAC halves (k_hd_hmac, k_hd_path_hmac), seeds' digests (k_seed_keys),
//                         shares, keys, coefficients, exponents, SHA-256 digests (hpk::exponent)
//   hdk::add_mod_n / _masked, frs::add / add_masked   reduced values; partial sums (below n)
//   frs::sub, neg         below n (Montgomery-form points and products); neg(0) = 0
//   hdk::sha256_compress  any state and block.  hmac_key: klen 20 and 11 (the seed keys) and 32 (a chain code), on the host
//                         side only (blsgpu_api.hip); <= 64 by contract.  pad_block: len <= 55 (host tests only).
//   hdk::child_hmacs, path_step   sw 12 (a public key) or 8 (a private key), any index.  fingerprint: 12 words.
//   hdk::hmac_long, hmac_long_pair   k_seed_keys: len up to BLSGPU_SEED_MAX_BYTES, suffix -1 (hmac_long) or 0 and 1 (the pair),
//                         a message at any byte address (seed i at i * len)
//   hpk::digest           k >= 1 keys on a 16-byte aligned base;  hpk::exponent  any digest, any i
//   sigdiv::exponent, entry_bits, quotient_scalar   caller bytes of any value;  neg_coord / neg_point  coordinates below q
//   swin::recode          any 256-bit scalar (NOT reduced): digits in [-8, 8), the top digit (w = 64) is 0 or +1 -- s + C <
//                         2^256 + 8 (16^65 - 1) / 15 < 2 * 16^64 so its nibble is 8 or 9 -- never negative
//   swin::select_entry    ad 0 .. 8; keep0 = 0 (k_g2_smul) or the digit's mz (k_fix_mul_secret, k_poly_eval_secret)
#include "check_runner.h"
#if defined(__HIPCC__)
#define BLSGPU_TU 99                                       // no kernel group: declarations only
#include "blsgpu_tu.h"
#include "blsgpu_kernels.hip"                              // bswap32 for secret_window.h
#include "fp28.h"
#include "blsgpu_ml.hip"
#include "blsgpu_msm.hip"                                  // sp2, the point arithmetic blsgpu_g2smul.hip names
#include "blsgpu_g1fix.hip"                                // g1fix::ENTRY_DW, secret_window.h
#include "blsgpu_g2smul.hip"                               // g2smul::PT_DW, g2smul::PAIRS
#endif
#include "fr_scalar.h"
#include "sigdiv.h"
#include "hash_pks.h"

namespace frcheck {

// every op, once, with its code (tests/fr_vectors.py pins the codes): those that also build for the host, then the device-only ones
#define FRCHECK_HOST_OPS(X) \
    /* reduce */ \
    X(SUB_N_IF_GE, 0) X(REDUCE_N, 1) X(ADD_MOD_N, 2) X(SUB_N_IF_GE_MASKED, 3) X(REDUCE_N_MASKED, 4) X(ADD_MOD_N_MASKED, 5) X(BELOW_N, 6) \
    X(IS_ZERO, 7) X(SUB, 8) X(NEG, 9) X(ADD, 10) X(ADD_MASKED, 11) \
    /* products */ \
    X(MUL, 20) X(MUL_MASKED, 21) X(SQR, 22) X(TO_MONT, 23) X(FROM_MONT, 24) X(TO_MONT_MASKED, 25) X(FROM_MONT_MASKED, 26) \
    /* inversions */ \
    X(INV, 30) X(INV_UNI, 31) X(QUOTIENT_SCALAR, 32) \
    /* lagrange */ \
    X(LAGRANGE_POINT, 40) X(LAGRANGE_WEIGHT, 41) X(LAGRANGE_DEN, 42) X(DOT_TERM, 43) X(DOT_TERM_MASKED, 44) X(SUM_TERM_MASKED, 45) \
    X(POLY_COEFF_MASKED, 46) X(POLY_POINT, 47) X(POLY_HORNER_MASKED, 48) \
    /* sigdiv */ \
    X(SD_EXPONENT, 50) X(SD_CROSS_EQUAL, 51) X(SD_ENTRY_BITS, 52) X(SD_STATUS_OF, 53) X(SD_NEG_COORD, 54) X(SD_NEG_POINT, 55) \
    /* sha */ \
    X(SHA_COMPRESS, 60) X(HMAC_KEY, 61) X(HMAC_KEY_WORDS, 62) X(PAD_HMAC_BLOCK, 63) X(CHILD_HMACS, 64) X(PATH_STEP, 65) X(FINGERPRINT, 66) \
    X(LONG_BLOCKS, 67) X(LONG_WORD, 68) X(HMAC_LONG, 69) X(HMAC_LONG_PAIR, 70) X(HPK_DIGEST, 71) X(HPK_EXPONENT, 72)
// window (device only)
#define FRCHECK_DEVICE_OPS(X) X(RECODE_G1, 80) X(RECODE_G2, 81) X(SEL, 82) X(SELECT_G1, 83) X(SELECT_G2, 84)
#define FRCHECK_OPS(X) FRCHECK_HOST_OPS(X) FRCHECK_DEVICE_OPS(X)
CHECK_ENUM(FRCHECK_OPS)

constexpr int W = 8, MAXK = 67, MAXT = 16, MSGW = 52, MAXKEYS = 9, DIGITS = 65;

CHECK_FN void ld(uint32_t* d, const uint32_t* p, int n = W) { for (int j = 0; j < n; j++) d[j] = p[j]; }
CHECK_FN void st(const uint32_t* x, uint32_t* p, int n = W) { for (int j = 0; j < n; j++) p[j] = x[j]; }
CHECK_FN const uint8_t* bytes(const uint32_t* p) { return (const uint8_t*)p; }
CHECK_FN void ldkey(hdk::HmacKey& k, const uint32_t* p) { ld(k.ipad, p); ld(k.opad, p + W); }

// in / out words per item and the op's body
template <int OP> struct Do;
#define CHECK_OP(OP, WIN, WOUT) \
    template <> struct Do<OP> { static constexpr int win = WIN, wout = WOUT; static CHECK_MEMBER void run(const uint32_t* in, uint32_t* out); }; \
    CHECK_MEMBER void Do<OP>::run(const uint32_t* in, uint32_t* out)
#define OP1(OP, CALL) CHECK_OP(OP, W, W) { uint32_t s[W]; ld(s, in); CALL; st(s, out); }
#define OP2(OP, CALL) CHECK_OP(OP, 2 * W, W) { uint32_t a[W], b[W], r[W]; ld(a, in); ld(b, in + W); CALL; st(r, out); }

// ---- reduce -------------------------------------------------------------------------------------------------------------
OP1(SUB_N_IF_GE, hdk::sub_n_if_ge(s))
OP1(REDUCE_N, hdk::reduce_n(s))
OP2(ADD_MOD_N, hdk::add_mod_n(r, a, b))
OP1(SUB_N_IF_GE_MASKED, hdk::sub_n_if_ge_masked(s))
OP1(REDUCE_N_MASKED, hdk::reduce_n_masked(s))
OP2(ADD_MOD_N_MASKED, hdk::add_mod_n_masked(r, a, b))
CHECK_OP(BELOW_N, W, 1) { uint32_t a[W]; ld(a, in); out[0] = frs::below_n(a) ? 1u : 0u; }
CHECK_OP(IS_ZERO, W, 1) { uint32_t a[W]; ld(a, in); out[0] = frs::is_zero(a) ? 1u : 0u; }
OP2(SUB, frs::sub(r, a, b))
CHECK_OP(NEG, W, W) { uint32_t a[W], r[W]; ld(a, in); frs::neg(r, a); st(r, out); }
OP2(ADD, frs::add(r, a, b))
OP2(ADD_MASKED, frs::add_masked(r, a, b))

// ---- products -----------------------------------------------------------------------------------------------------------
OP2(MUL, frs::mul(r, a, b))
OP2(MUL_MASKED, frs::mul_masked(r, a, b))
CHECK_OP(SQR, W, W) { uint32_t a[W], r[W]; ld(a, in); frs::sqr(r, a); st(r, out); }
CHECK_OP(TO_MONT, W, W) { uint32_t a[W], r[W]; ld(a, in); frs::to_mont(r, a); st(r, out); }
CHECK_OP(FROM_MONT, W, W) { uint32_t a[W], r[W]; ld(a, in); frs::from_mont(r, a); st(r, out); }
CHECK_OP(TO_MONT_MASKED, W, W) { uint32_t a[W], r[W]; ld(a, in); frs::to_mont_masked(r, a); st(r, out); }
CHECK_OP(FROM_MONT_MASKED, W, W) { uint32_t a[W], r[W]; ld(a, in); frs::from_mont_masked(r, a); st(r, out); }

// ---- inversions ---------------------------------------------------------------------------------------------------------
CHECK_OP(INV, W, W) { uint32_t a[W], r[W]; ld(a, in); frs::inv(r, a); st(r, out); }
CHECK_OP(INV_UNI, W, W) { uint32_t a[W], r[W]; ld(a, in); frs::inv(r, a); st(r, out); }   // (the caller gives a wavefront one value)
CHECK_OP(QUOTIENT_SCALAR, 2 * W, W + 1) { out[W] = sigdiv::quotient_scalar(bytes(in), bytes(in + W), (uint8_t*)out) ? 1u : 0u; }

// ---- lagrange -----------------------------------------------------------------------------------------------------------
CHECK_OP(LAGRANGE_POINT, W, W + 1) { uint32_t xm[W]; out[W] = frs::lagrange_point(bytes(in), xm) ? 1u : 0u; st(xm, out); }
CHECK_OP(LAGRANGE_WEIGHT, 2 + MAXK * W, W) { uint32_t p[W]; const uint32_t k = in[0] < (uint32_t)MAXK ? in[0] : (uint32_t)MAXK;   // (a record holds MAXK points)
    frs::lagrange_weight(in + 2, k, in[1] < k ? in[1] : 0u, p); st(p, out); }
CHECK_OP(LAGRANGE_DEN, 1 + MAXK * W, W) { uint32_t d[W]; frs::lagrange_den(in + 1, in[0] < (uint32_t)MAXK ? in[0] : (uint32_t)MAXK, d); st(d, out); }
CHECK_OP(DOT_TERM, 2 * W, W) { uint32_t t[W]; frs::dot_term(bytes(in), bytes(in + W), t); st(t, out); }
CHECK_OP(DOT_TERM_MASKED, 2 * W, W) { uint32_t t[W]; frs::dot_term_masked(bytes(in), bytes(in + W), t); st(t, out); }
CHECK_OP(SUM_TERM_MASKED, 2 * W, W) { uint32_t acc[W]; ld(acc, in + W); frs::sum_term_masked(bytes(in), acc); st(acc, out); }
CHECK_OP(POLY_COEFF_MASKED, W, W) { uint32_t c[W]; frs::poly_coeff_masked(bytes(in), c); st(c, out); }
CHECK_OP(POLY_POINT, W, W) { uint32_t x[W]; frs::poly_point(bytes(in), x); st(x, out); }
CHECK_OP(POLY_HORNER_MASKED, 1 + W + MAXT * W, W) { uint32_t xm[W], r[W]; ld(xm, in + 1);
    const uint32_t t = in[0] < 1u ? 1u : (in[0] < (uint32_t)MAXT ? in[0] : (uint32_t)MAXT);                                      // (1 .. MAXT coefficients)
    frs::poly_horner_masked(in + 1 + W, t, xm, r); st(r, out); }

// ---- sigdiv -------------------------------------------------------------------------------------------------------------
CHECK_OP(SD_EXPONENT, W, W) { uint32_t x[W]; sigdiv::exponent(bytes(in), x); st(x, out); }
CHECK_OP(SD_CROSS_EQUAL, 4 * W, 1) { uint32_t a0[W], b0[W], ae[W], be[W]; ld(a0, in); ld(b0, in + W); ld(ae, in + 2 * W); ld(be, in + 3 * W);
    out[0] = sigdiv::cross_equal(a0, b0, ae, be) ? 1u : 0u; }
CHECK_OP(SD_ENTRY_BITS, 4 * W, 1) { out[0] = sigdiv::entry_bits(bytes(in), bytes(in + W), bytes(in + 2 * W), bytes(in + 3 * W)); }
CHECK_OP(SD_STATUS_OF, 2, 1) { out[0] = (uint32_t)sigdiv::status_of(in[0] != 0, in[1] != 0); }
CHECK_OP(SD_NEG_COORD, 12, 12) { sigdiv::neg_coord(in, out); }
CHECK_OP(SD_NEG_POINT, 48, 48) { sigdiv::neg_point(in, out); }

// ---- sha ----------------------------------------------------------------------------------------------------------------
CHECK_OP(SHA_COMPRESS, W + 16, W) { uint32_t s[W], w[16]; ld(s, in); ld(w, in + W, 16); hdk::sha256_compress(s, w); st(s, out); }
CHECK_OP(HMAC_KEY, 1 + 16, 2 * W) { hdk::HmacKey k; hdk::hmac_key(bytes(in + 1), (int)(in[0] < 64u ? in[0] : 64u), k); st(k.ipad, out); st(k.opad, out + W); }
CHECK_OP(HMAC_KEY_WORDS, W, 2 * W) { hdk::HmacKey k; uint32_t c[W]; ld(c, in); hdk::hmac_key_words(c, k); st(k.ipad, out); st(k.opad, out + W); }
CHECK_OP(PAD_HMAC_BLOCK, 1 + 2 * W + 14, 16 + W) { hdk::HmacKey k; ldkey(k, in + 1); uint32_t block[16], d[W];
    hdk::pad_block(bytes(in + 1 + 2 * W), (int)(in[0] < 55u ? in[0] : 55u), block); hdk::hmac_block(k, block, d); st(block, out, 16); st(d, out + 16); }
CHECK_OP(CHILD_HMACS, 2 + 2 * W + 12, 2 * W) { hdk::HmacKey k; ldkey(k, in + 2); uint32_t ser[12], il[W], ir[W]; ld(ser, in + 2 + 2 * W, 12);
    hdk::child_hmacs(k, ser, in[0] == 8u ? 8 : 12, in[1], il, ir); st(il, out); st(ir, out + W); }
CHECK_OP(PATH_STEP, 2 + W + 12, 2 * W) { uint32_t chain[W], ser[12], il[W], ir[W]; ld(chain, in + 2); ld(ser, in + 2 + W, 12);
    hdk::path_step(chain, ser, in[0] == 8u ? 8 : 12, in[1], il, ir); st(il, out); st(ir, out + W); }
CHECK_OP(FINGERPRINT, 12, 1) { uint32_t ser[12]; ld(ser, in, 12); out[0] = hdk::fingerprint(ser); }
CHECK_OP(LONG_BLOCKS, 2, 1) { out[0] = hdk::long_blocks(in[0], (int)in[1]); }
// a record's message: `shift` bytes into its MSGW words, len bytes long at the most that fit
CHECK_FN uint32_t fit(uint32_t len, uint32_t shift) { const uint32_t room = 4u * MSGW - (shift & 3u); return len < room ? len : room; }
CHECK_OP(LONG_WORD, 5 + MSGW, 1) { const uint32_t len = fit(in[0], in[4]);
    out[0] = hdk::long_word(bytes(in + 5) + (in[4] & 3u), len, len + (in[1] ? 1u : 0u), in[2] & 0xffu, in[3]); }
CHECK_OP(HMAC_LONG, 3 + 2 * W + MSGW, W) { hdk::HmacKey k; ldkey(k, in + 3); uint32_t d[W];
    hdk::hmac_long(k, bytes(in + 3 + 2 * W) + (in[2] & 3u), fit(in[0], in[2]), (int)in[1] < 0 ? -1 : (int)(in[1] & 0xffu), d); st(d, out); }
CHECK_OP(HMAC_LONG_PAIR, 2 + 2 * W + MSGW, 2 * W) { hdk::HmacKey k; ldkey(k, in + 2); uint32_t il[W], ir[W];
    hdk::hmac_long_pair(k, bytes(in + 2 + 2 * W) + (in[1] & 3u), fit(in[0], in[1]), il, ir); st(il, out); st(ir, out + W); }
CHECK_OP(HPK_DIGEST, 4 + MAXKEYS * 12, W) { uint32_t d[W]; hpk::digest(in + 4, in[0] < (uint32_t)MAXKEYS ? in[0] : (uint32_t)MAXKEYS, d); st(d, out); }
CHECK_OP(HPK_EXPONENT, 1 + W, W) { uint32_t dg[W], t[W]; ld(dg, in + 1); hpk::exponent(dg, in[0], t); st(t, out); }

#if defined(__HIPCC__)
// ---- window (the bodies of RECODE_* and SELECT_G2 are their kernels below) ----------------------------------------------
using blsgpu::g1fix::ENTRY_DW;
using blsgpu::g2smul::PT_DW;
using blsgpu::g2smul::PAIRS;
namespace swin = blsgpu::swin;
constexpr int G1_COLS = 256;                               // `rec` of k_fix_mul_secret and k_poly_eval_secret
static_assert(swin::WINDOWS == DIGITS && swin::TAB == 8, "the records hold 65 digits and 8 entries");
template <> struct Do<RECODE_G1> { static constexpr int win = W, wout = 3 * DIGITS; };
template <> struct Do<RECODE_G2> { static constexpr int win = W, wout = 3 * DIGITS; };
CHECK_OP(SEL, 3, 2) { out[0] = swin::sel(in[0], in[1], in[2]); out[1] = (uint32_t)swin::sel((int32_t)in[0], (int32_t)in[1], in[2]); }
CHECK_OP(SELECT_G1, 2 + 8 * (int)ENTRY_DW, (int)ENTRY_DW) { uint32_t q[ENTRY_DW];
    swin::select_entry<ENTRY_DW, true>(q, in + 2, 1, in[0], in[1]); st(q, out, (int)ENTRY_DW); }
template <> struct Do<SELECT_G2> { static constexpr int win = 2 + 8 * (int)PT_DW, wout = (int)PT_DW; };

template <int OP> __global__ void __launch_bounds__(256) k_check(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Do<OP>::run(in + i * Do<OP>::win, out + i * Do<OP>::wout);
}
__device__ __forceinline__ void store_digit(const swin::Digit& d, uint32_t* out) { out[0] = d.sgn; out[1] = d.ad; out[2] = d.mz; }
// one scalar per lane, a column of its own; a spare lane repeats the last scalar and stores nothing (as the kernels do)
template <> __global__ void __launch_bounds__(256) k_check<RECODE_G1>(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
    __shared__ uint32_t rec[swin::REC_WORDS][G1_COLS];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, g = i < n ? i : n - 1;
    swin::recode(rec, threadIdx.x, in + g * W);
#pragma unroll 1
    for (uint32_t w = 0; w < swin::WINDOWS; w++) {
        const swin::Digit d = swin::digit(rec, threadIdx.x, w);
        if (i < n) store_digit(d, out + i * (3 * DIGITS) + 3 * w);
    }
}
// one scalar per lane pair, both lanes writing the pair's column (k_g2_smul); the even lane stores
template <> __global__ void __launch_bounds__(256) k_check<RECODE_G2>(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
    __shared__ uint32_t rec[swin::REC_WORDS][PAIRS];
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, i = tid >> 1, g = i < n ? i : n - 1;
    const uint32_t lp = threadIdx.x >> 1;
    swin::recode(rec, lp, in + g * W);
#pragma unroll 1
    for (int w = (int)swin::WINDOWS - 1; w >= 0; w--) {
        const swin::Digit d = swin::digit(rec, lp, (uint32_t)w);
        if (i < n && (tid & 1u) == 0) store_digit(d, out + i * (3 * DIGITS) + 3 * w);
    }
}
template <> __global__ void __launch_bounds__(256) k_check<SELECT_G2>(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t q[PT_DW];
    swin::select_entry<PT_DW, false>(q, in + 2 * n + i, n, in[2 * i], in[2 * i + 1]);
    st(q, out + i * PT_DW, (int)PT_DW);
}

template <int OP> int run_op(const uint32_t* in, size_t words_in, size_t n, uint32_t* out, size_t words_out) {
    if (words_in != n * (size_t)Do<OP>::win || words_out != n * (size_t)Do<OP>::wout || n == 0 || n > (1u << 20)) return -2;
    const unsigned threads = 256u;
    const size_t lanes = OP == RECODE_G2 ? 2 * n : n;
    return check::guarded_run(in, words_in * 4, out, words_out * 4, 0, [=](const uint32_t* din, uint32_t* dout) {
        k_check<OP><<<dim3((unsigned)((lanes + threads - 1) / threads)), dim3(threads)>>>(din, n, dout);
    });
}
#endif
}  // namespace frcheck

using namespace frcheck;
#if defined(__HIPCC__)
CHECK_EXPORT(blsgpu_fr_check, uint32_t, FRCHECK_OPS)
#else
CHECK_HOST_ENTRY(frcheck_host, FRCHECK_HOST_OPS)        // (tests/test_fr_vectors_model.py)
#endif
