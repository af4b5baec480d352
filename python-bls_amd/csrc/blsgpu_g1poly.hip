// blsgpu_g1poly.hip -- batched Feldman share checks  (s_i mod n) G1 == sum_k x_i^k C[poly_i][k]  (Threshold.verify_secret_fragment
// of the reference, threshold.py:104-125) and the Horner values behind them (included by blsgpu_api.hip, built with
// blsgpu_g1fix.hip in translation unit 8).
//
// A call holds n_polys polynomials of t commitments each and n fragments (poly_i, x_i, s_i); one fragment per lane.
//   k_poly_prep      the commitments, once per call: 96-byte affine -> L28 entries (the 112-byte layout of the fixed-base
//                    table); (0, 0) = infinity stays all-zero limbs (no point of the curve has x = y = 0).
//   k_poly_subgroup  one commitment C_k (k >= 1) per lane: [n] C_k == O by double-and-add over the public bits of n;
//                    a polynomial with one that fails is flagged (an ordinary store of 1).
//   k_poly_eval      x = x_i mod n; Horner in the exponent R = C_{t-1}; R = x R + C_k for k = t-2 .. 0, x R by left-to-right
//                    double-and-add over the bits of x (players 1 .. N: a few doublings per step, not 255); the left-hand
//                    side (s_i mod n) G1 on the fixed-base table (g1fix::fix_sum); a projective comparison, no inversion.
// The RCB formulas of fp28.h are complete on all of E(Fq) (h n is odd: no point of order 2), so points outside the order-n
// subgroup, infinity and doubling need no branch.  The one branch is an infinity COMMITMENT, which the mixed addition
// cannot take as its affine operand: it is skipped.
//
// Why the subgroup flag: Horner computes sum_k x^k C_k, the reference sum_k (x^k mod n) C_k.  The two agree when every
// C_k (k >= 1) has order dividing n; otherwise the kernel does not decide and the fragment gets status 2 (the caller
// decides it exactly, bls_py.threshold).  C_0 is multiplied by 1 on both sides and is not checked.
// Not constant-time: the loops follow the bits of the public player values and the table gathers follow the digits of
// the secret fragments (as k_fix_mul does).  k_poly_eval_secret (the section "the check for SECRET fragments" below) is the
// form whose schedule does not look at the fragments.
#pragma once

namespace blsgpu {
namespace g1poly {

using g1fix::ENTRY_DW;
constexpr uint32_t N_WORDS[8] = HD_N_WORDS;                                  // the group order, little-endian words
constexpr int N_TOP = 254;                                                   // its highest set bit

// an L28 affine entry with all-zero limbs is infinity
__device__ __forceinline__ bool entry_inf(const uint32_t* __restrict__ p) {
    uint32_t z = 0;
#pragma unroll
    for (int j = 0; j < (int)ENTRY_DW; j++) z |= p[j];
    return z == 0;
}
// P += the entry at p (nothing for infinity)
__device__ __forceinline__ void add_entry(r28::ptT<r28::fe>& P, const uint32_t* __restrict__ p) {
    if (!entry_inf(p)) r28::pmadd(P, r28::ld(p), r28::ld(p + r28::NL));
}
// 8 big-endian words -> little-endian words mod n
__device__ __forceinline__ void ld_scalar_mod_n(const uint32_t* __restrict__ be, uint32_t s[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] = bswap32(be[7 - j]);
    hdk::reduce_n(s);
}

// m commitments (96 bytes big-endian each) -> m L28 entries
__global__ void __launch_bounds__(256) k_poly_prep(const uint32_t* __restrict__ commit, uint32_t m, uint32_t* __restrict__ l28)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m) return;
    const uint32_t* a = commit + (size_t)e * 24;
    uint32_t x[12], y[12];
#pragma unroll
    for (int w = 0; w < 12; w++) { x[11 - w] = bswap32(a[w]); y[11 - w] = bswap32(a[12 + w]); }
    r28::st(r28::from_raw(x), l28 + (size_t)e * ENTRY_DW);                  // from_raw(0) is all-zero limbs
    r28::st(r28::from_raw(y), l28 + (size_t)e * ENTRY_DW + r28::NL);
}
#else
;
#endif

// bad[p] = 1 if [n] C[p][k] != O for some k in 1 .. t-1 (one (p, k) per lane; bad cleared by the caller)
__global__ void __launch_bounds__(256) k_poly_subgroup(const uint32_t* __restrict__ l28, uint32_t n_polys, uint32_t t, uint32_t* __restrict__ bad)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 2 || e >= n_polys * (t - 1)) return;
    const uint32_t p = e / (t - 1), k = 1 + e % (t - 1);
    const uint32_t* c = l28 + ((size_t)p * t + k) * ENTRY_DW;
    if (entry_inf(c)) return;
    const r28::fe cx = r28::ld(c), cy = r28::ld(c + r28::NL);
    r28::ptT<r28::fe> acc = r28::pt_inf<r28::fe>();
    r28::pmadd(acc, cx, cy);                                                 // the top bit of n
#pragma unroll 1
    for (int b = N_TOP - 1; b >= 0; b--) {
        acc = r28::pdbl(acc);
        if ((N_WORDS[b >> 5] >> (b & 31)) & 1u) r28::pmadd(acc, cx, cy);
    }
    if (!r28::is_zero(acc.Z)) bad[p] = 1u;
}
#else
;
#endif

// fragment i of m: R = sum_k (x_i mod n)^k C[poly_i][k] by Horner; status[i] = 2 if bad[poly_i], else 1 if R == (s_i mod n) G1
// and 0 if not (s and status NULL together: evaluation only); out_aff[i] = R affine (96 bytes, (0, 0) for infinity) if asked.
__global__ void __launch_bounds__(256) k_poly_eval(const uint32_t* __restrict__ table, const uint32_t* __restrict__ l28,
                                                   const uint32_t* __restrict__ bad, uint32_t n_polys, uint32_t t,
                                                   const uint32_t* __restrict__ poly, const uint32_t* __restrict__ xs,
                                                   const uint32_t* __restrict__ ss, uint32_t m, uint8_t* __restrict__ status,
                                                   uint32_t* __restrict__ out_aff)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t p = poly[i];
    if (p >= n_polys) return;                                                // (the host checked every index before the launch)
    const uint32_t* C = l28 + (size_t)p * t * ENTRY_DW;
    uint32_t x[8];
    ld_scalar_mod_n(xs + (size_t)i * 8, x);
    int top = -1;                                                            // highest set bit of x
#pragma unroll
    for (int j = 7; j >= 0; j--)
        if (top < 0 && x[j]) top = 32 * j + 31 - __builtin_clz(x[j]);

    r28::ptT<r28::fe> R = r28::pt_inf<r28::fe>();
    add_entry(R, C + (size_t)(t - 1) * ENTRY_DW);
#pragma unroll 1
    for (int k = (int)t - 2; k >= 0; k--) {
        if (top < 0) {
            R = r28::pt_inf<r28::fe>();
        } else {
            r28::ptT<r28::fe> acc = R;                                       // the top bit of x
#pragma unroll 1
            for (int b = top - 1; b >= 0; b--) {
                acc = r28::pdbl(acc);
                if ((x[b >> 5] >> (b & 31)) & 1u) acc = r28::padd(acc, R);
            }
            R = acc;
        }
        add_entry(R, C + (size_t)k * ENTRY_DW);
    }

    if (status) {
        uint8_t st = 2;
        if (!bad[p]) {
            uint32_t s[8];
            ld_scalar_mod_n(ss + (size_t)i * 8, s);
            r28::ptT<r28::fe> L = r28::pt_inf<r28::fe>();
            g1fix::fix_sum(table, s, L);
            // (X1 : Y1 : Z1) == (X2 : Y2 : Z2)  <=>  X1 Z2 = X2 Z1 and Y1 Z2 = Y2 Z1 (infinity is (0 : Y : 0), Y != 0)
            const r28::fe a = r28::canon(r28::mul(R.X, L.Z)), b = r28::canon(r28::mul(L.X, R.Z));
            const r28::fe c = r28::canon(r28::mul(R.Y, L.Z)), d = r28::canon(r28::mul(L.Y, R.Z));
            uint32_t diff = 0;
#pragma unroll
            for (int j = 0; j < r28::NL; j++) diff |= (uint32_t)(a.v[j] ^ b.v[j]) | (uint32_t)(c.v[j] ^ d.v[j]);
            st = diff == 0 ? 1 : 0;
        }
        status[i] = st;
    }
    if (out_aff) {
        uint32_t ax[12], ay[12];
        g1fix::to_affine_raw(R, ax, ay);
        g1fix::store_result(ax, ay, i, out_aff, nullptr);
    }
}
#else
;
#endif

// ---- the check for SECRET fragments (blsgpu_g1_poly_check_secret) ----------------------------------------------------------
// k_poly_eval with the left-hand side on secret_window.h's schedule -- the claim and its limits are stated there: the sequence
// of instructions and of memory addresses does not depend on the fragments s_i.  It does depend on t, the counts, lane
// indices, the commitments, the players x_i and the polynomial indices, which are public, and the status that is stored is
// the OUTCOME of the check, which a player publishes (a complaint).
//   left       L = s_i G1 for the LITERAL 256-bit s_i (no reduction mod n: G1 has order n, so this is (s_i mod n) G1):
//              swin::recode into the lane's column of LDS, then the 65 windows of k_fix_mul_secret on the context's signed
//              4-bit table -- all eight entries of a window read at addresses formed from the window alone, one kept by
//              select, one r28::pmadd, a zero digit dropped by select.  No inversion.  The loop is written out a second
//              time here: shared with k_fix_mul_secret through an inline function it changed that kernel's scalar-register
//              spills (9 -> 5), and the existing kernels keep their allocation.  The finished L is parked in LDS, in a
//              column of the lane's own, while the right-hand side runs (R, the accumulator of x R and a table entry
//              would not sit in registers together).
//   right      k_poly_eval's Horner over the bits of the public x_i, the skip of an infinity commitment and the top < 0
//              case included.
//   compare    four products, canon, an OR of the differences; 2 where bad[poly_i].
//   tail       spare lanes of the last workgroup repeat the last fragment and store nothing; no lane leaves before the end.
// SECRET: ss, and with it rec, L and lhs (the lines marked below); a, b, c, d and diff mix it with public values, and what is
// stored of them is the status.  Every store is a plain C++ store.
__global__ void __launch_bounds__(256) k_poly_eval_secret(const uint32_t* __restrict__ table, const uint32_t* __restrict__ l28,
                                                          const uint32_t* __restrict__ bad, uint32_t n_polys, uint32_t t,
                                                          const uint32_t* __restrict__ poly, const uint32_t* __restrict__ xs,
                                                          const uint32_t* __restrict__ ss, uint32_t m, uint8_t* __restrict__ status,
                                                          uint32_t* __restrict__ out_aff)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    __shared__ uint32_t rec[swin::REC_WORDS][256];
    __shared__ int32_t lhs[3 * r28::NL][256];
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x;
    const uint32_t i = min(tid, m - 1u);
    const bool store = tid < m;
    {
        swin::recode(rec, lane, ss + (size_t)i * 8);                         // secret
        r28::ptT<r28::fe> L = r28::pt_inf<r28::fe>();
#pragma unroll 1
        for (uint32_t w = 0; w < swin::WINDOWS; w++) {                       // k_fix_mul_secret's window, line for line
            const swin::Digit d = swin::digit(rec, lane, w);                 // secret from here to the end of the block
            uint32_t q[ENTRY_DW];
            swin::select_entry<ENTRY_DW, true>(q, table + (size_t)w * (swin::TAB * ENTRY_DW), 1, d.ad, d.mz);
            r28::fe ex, ey;
#pragma unroll
            for (int j = 0; j < r28::NL; j++) { ex.v[j] = (int32_t)q[j]; ey.v[j] = (int32_t)q[r28::NL + j]; }
            const r28::fe yn = r28::norm(r28::neg(ey));
#pragma unroll
            for (int j = 0; j < r28::NL; j++) ey.v[j] = swin::sel(yn.v[j], ey.v[j], d.sgn);
            const r28::ptT<r28::fe> old = L;
            r28::pmadd(L, ex, ey);
#pragma unroll
            for (int j = 0; j < r28::NL; j++) {                              // a zero digit: the sum is dropped
                L.X.v[j] = swin::sel(old.X.v[j], L.X.v[j], d.mz);
                L.Y.v[j] = swin::sel(old.Y.v[j], L.Y.v[j], d.mz);
                L.Z.v[j] = swin::sel(old.Z.v[j], L.Z.v[j], d.mz);
            }
        }
#pragma unroll
        for (int j = 0; j < r28::NL; j++) {                                  // lane-indexed addresses
            lhs[j][lane] = L.X.v[j];
            lhs[r28::NL + j][lane] = L.Y.v[j];
            lhs[2 * r28::NL + j][lane] = L.Z.v[j];
        }
    }
    const uint32_t p = min(poly[i], n_polys - 1u);                           // (the host checked every index before the launch)
    const uint32_t* C = l28 + (size_t)p * t * ENTRY_DW;
    uint32_t x[8];
    ld_scalar_mod_n(xs + (size_t)i * 8, x);
    int top = -1;                                                            // highest set bit of x
#pragma unroll
    for (int j = 7; j >= 0; j--)
        if (top < 0 && x[j]) top = 32 * j + 31 - __builtin_clz(x[j]);

    r28::ptT<r28::fe> R = r28::pt_inf<r28::fe>();
    add_entry(R, C + (size_t)(t - 1) * ENTRY_DW);
#pragma unroll 1
    for (int k = (int)t - 2; k >= 0; k--) {
        if (top < 0) {
            R = r28::pt_inf<r28::fe>();
        } else {
            r28::ptT<r28::fe> acc = R;                                       // the top bit of x
#pragma unroll 1
            for (int b = top - 1; b >= 0; b--) {
                acc = r28::pdbl(acc);
                if ((x[b >> 5] >> (b & 31)) & 1u) acc = r28::padd(acc, R);
            }
            R = acc;
        }
        add_entry(R, C + (size_t)k * ENTRY_DW);
    }

    r28::ptT<r28::fe> L;
#pragma unroll
    for (int j = 0; j < r28::NL; j++) {                                      // secret
        L.X.v[j] = lhs[j][lane];
        L.Y.v[j] = lhs[r28::NL + j][lane];
        L.Z.v[j] = lhs[2 * r28::NL + j][lane];
    }
    // (X1 : Y1 : Z1) == (X2 : Y2 : Z2)  <=>  X1 Z2 = X2 Z1 and Y1 Z2 = Y2 Z1 (infinity is (0 : Y : 0), Y != 0)
    const r28::fe a = r28::canon(r28::mul(R.X, L.Z)), b = r28::canon(r28::mul(L.X, R.Z));
    const r28::fe c = r28::canon(r28::mul(R.Y, L.Z)), d = r28::canon(r28::mul(L.Y, R.Z));
    uint32_t diff = 0;
#pragma unroll
    for (int j = 0; j < r28::NL; j++) diff |= (uint32_t)(a.v[j] ^ b.v[j]) | (uint32_t)(c.v[j] ^ d.v[j]);
    const uint8_t st = bad[p] ? 2 : (diff == 0 ? 1 : 0);                     // the outcome: public from here on
    if (store) status[i] = st;
    if (out_aff) {
        uint32_t ax[12], ay[12];
        g1fix::to_affine_raw(R, ax, ay);
        g1fix::store_result(ax, ay, i, store ? out_aff : nullptr, nullptr);
    }
}
#else
;
#endif

// flag[0] |= 1 if any of the m polynomial indices is >= n_polys (the _dev form checks before it writes)
__global__ void __launch_bounds__(256) k_poly_check(const uint32_t* __restrict__ poly, uint32_t m, uint32_t n_polys, uint32_t* __restrict__ flag)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m && poly[i] >= n_polys) atomicOr(flag, 1u);
}
#else
;
#endif

}  // namespace g1poly
}  // namespace blsgpu
