// blsgpu_g1fix.hip -- fixed-base G1 multiplication  out_i = s_i G1 (+ A_i), batched HD child derivation and batched HD
// PATH derivation with a parent per lane (included by blsgpu_api.hip).
//
// Every s G1 of the other entries is a variable-base multiplication (k_smul: a table of the point's own multiples per
// lane, 252 doublings, 64 complete additions).  The generator is fixed, so its multiples are computed ONCE per context:
// unsigned 8-bit windows, entry (w, d) = d 2^(8w) G1 for w < 32, 1 <= d <= 255, affine (x, y) in the L28 form of fp28.h --
// 32 x 255 x 112 bytes = 0.9 MB, inside one XCD's 4 MB L2.  A scalar is then s = sum_w d_w 2^(8w) and s G1 = sum_w
// T[w][d_w]: 32 complete mixed additions (r28::pmadd, none for a zero digit), no doubling, then one inversion for the
// affine result.  One scalar per lane; the lanes of a wavefront gather from the same window's 28 KB at each step.
// The table is indexed by secret digits: not constant-time (neither is k_smul).
//
// HD paths (blsgpu_hd_paths): one path per lane, one level per pair of launches -- k_hd_path_hmac (the lane's own chain
// code as HMAC key: two midstate compressions and four HMAC compressions per level) and k_fix_mul on the scalars it
// leaves -- over state that stays in device memory between the levels.  Like k_hd_hmac and k_fix_mul it is NOT
// constant-time: the table gathers follow the digits of secret keys, and lanes branch on hardened indices.
// blsgpu_g1_mul_gen_secret and blsgpu_hd_paths_secret run k_fix_mul_secret instead: a second, signed 4-bit table read whole
// per window, a schedule that does not look at the scalar (the section "multiplication by SECRET scalars" below).
#pragma once

#include "hd_derive.h"
#include "secret_window.h"

namespace blsgpu {
namespace g1fix {

constexpr uint32_t WINDOWS = 32, DIGITS = 255;
constexpr uint32_t ENTRY_DW = 2 * r28::NL;                                   // affine (x, y), L28
constexpr uint32_t ENTRIES = WINDOWS * DIGITS;
constexpr size_t TABLE_BYTES = (size_t)ENTRIES * ENTRY_DW * 4;
constexpr uint32_t S_ENTRIES = swin::WINDOWS * swin::TAB;                     // the signed 4-bit table of k_fix_mul_secret
constexpr size_t S_TABLE_BYTES = (size_t)S_ENTRIES * ENTRY_DW * 4;

struct Gen { uint32_t x[12], y[12]; };                                        // an affine point, little-endian words

// (X : Y : Z) -> canonical x, y (little-endian words; (0, 0) for Z = 0 since fq_inv(0) = 0), one inversion
__device__ __forceinline__ void to_affine_raw(const r28::ptT<r28::fe>& a, uint32_t x[12], uint32_t y[12]) {
    uint32_t zv[12], ziv[12];
    r28::to_vm(zv, a.Z);
    bls::fq_inv(ziv, zv);
    const r28::fe zi = r28::from_vm(ziv);
    r28::to_raw(x, r28::mul(a.X, zi));
    r28::to_raw(y, r28::mul(a.Y, zi));
}

// acc += s G1 for s < 2^256 given as 8 little-endian words (reduce mod n first for s mod n): one complete mixed addition
// per non-zero 8-bit digit, gathered from the table (k_fix_mul, and the left-hand side of k_poly_eval in blsgpu_g1poly.hip)
__device__ __forceinline__ void fix_sum(const uint32_t* __restrict__ table, const uint32_t s[8], r28::ptT<r28::fe>& acc) {
#pragma unroll 1
    for (uint32_t w = 0; w < WINDOWS; w++) {
        const uint32_t d = (s[w >> 2] >> ((w & 3u) * 8u)) & 255u;
        if (d) {
            const uint32_t* p = table + (size_t)(w * DIGITS + d - 1u) * ENTRY_DW;
            r28::pmadd(acc, r28::ld(p), r28::ld(p + r28::NL));
        }
    }
}

// PublicKey.serialize() of a canonical affine point (ec.py:94-111 of the reference), in place on x: 0x80 in the top byte
// when y > q // 2 (most significant word first).  Infinity is (0, 0): y = 0, so x stays 0.
__device__ __forceinline__ void ser_flag(uint32_t x[12], const uint32_t y[12]) { x[11] |= bls::gt_half_q_mask(y) & 0x80000000u; }

// The result of lane i, canonical (x, y): out_aff 96 bytes big-endian ((0, 0) for infinity), out_ser 48 bytes
// (PublicKey.serialize()); each may be NULL
__device__ __forceinline__ void store_result(uint32_t x[12], const uint32_t y[12], uint32_t i, uint32_t* __restrict__ out_aff,
                                             uint32_t* __restrict__ out_ser) {
    if (out_aff) {
#pragma unroll
        for (int w = 0; w < 12; w++) { out_aff[(size_t)i * 24 + w] = bswap32(x[11 - w]); out_aff[(size_t)i * 24 + 12 + w] = bswap32(y[11 - w]); }
    }
    if (out_ser) {
        ser_flag(x, y);
#pragma unroll
        for (int w = 0; w < 12; w++) out_ser[(size_t)i * 12 + w] = bswap32(x[11 - w]);
    }
}

// The tables, WBITS bits per window: entry e = w * PER + d - 1 holds d 2^(WBITS w) G1 -- one entry per lane, double-and-add
// over the WBITS bits of d, then WBITS w doublings, then the affine form.  Once per context (a few hundred microseconds);
// nothing here depends on a scalar.  <8>: 32 windows of the digits 1 .. 255 (fix_sum); <4>: swin::WINDOWS windows of
// |d| = 1 .. swin::TAB (k_fix_mul_secret).
template <uint32_t WBITS>
__global__ void __launch_bounds__(64) k_fix_table_t(Gen g, uint32_t* __restrict__ table)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    static_assert(WBITS == 8 || WBITS == 4, "unsigned 8-bit or signed 4-bit windows");
    constexpr uint32_t PER = WBITS == 8 ? DIGITS : swin::TAB, N = WBITS == 8 ? ENTRIES : S_ENTRIES;
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    const uint32_t w = e / PER, d = e % PER + 1u;
    const r28::fe gx = r28::from_raw(g.x), gy = r28::from_raw(g.y);
    r28::ptT<r28::fe> acc = r28::pt_inf<r28::fe>();
#pragma unroll 1
    for (int b = (int)WBITS - 1; b >= 0; b--) {
        acc = r28::pdbl(acc);
        if ((d >> b) & 1u) r28::pmadd(acc, gx, gy);
    }
#pragma unroll 1
    for (uint32_t t = 0; t < WBITS * w; t++) acc = r28::pdbl(acc);
    uint32_t x[12], y[12];
    to_affine_raw(acc, x, y);
    r28::st(r28::from_raw(x), table + (size_t)e * ENTRY_DW);
    r28::st(r28::from_raw(y), table + (size_t)e * ENTRY_DW + r28::NL);
}
#else
;
#endif
#if BLSGPU_TU == BLSGPU_TU_FIX          // the instantiations the host side launches: this translation unit emits them (blsgpu_tu.h)
__attribute__((used)) static const void* const blsgpu_instances_fix[] = {(const void*)&k_fix_table_t<8>, (const void*)&k_fix_table_t<4>};
#endif

// out_i = (s_i mod n) G1 + A_i.  scalars: n x 32 bytes big-endian; add: NULL, one point (add_per = 0) or n points (add_per = 1),
// 96 bytes affine big-endian, (0, 0) = infinity; out_aff (n x 96 bytes, (0, 0) for infinity) and out_ser (n x 48 bytes, the
// reference's compression ec.py:94-111: x with 0x80 when y > q // 2, 48 zero bytes for infinity) may each be NULL.
// s mod n gives the same point as s (G1 has order n); the complete additions need no special case for A = +-s G1.
__global__ void __launch_bounds__(256) k_fix_mul(const uint32_t* __restrict__ table, const uint32_t* __restrict__ scalars, uint32_t n,
                                                 const uint32_t* __restrict__ add, uint32_t add_per, uint32_t* __restrict__ out_aff,
                                                 uint32_t* __restrict__ out_ser)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t s[8];
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] = bswap32(scalars[(size_t)i * 8 + 7 - j]);
    hdk::reduce_n(s);
    r28::ptT<r28::fe> acc = r28::pt_inf<r28::fe>();
    if (add) {
        const uint32_t* a = add + (size_t)(add_per ? i : 0u) * 24;
        uint32_t x[12], y[12], any = 0;
#pragma unroll
        for (int w = 0; w < 12; w++) { x[11 - w] = bswap32(a[w]); y[11 - w] = bswap32(a[12 + w]); any |= x[11 - w] | y[11 - w]; }
        if (any) r28::pmadd(acc, r28::from_raw(x), r28::from_raw(y));
    }
    fix_sum(table, s, acc);
    uint32_t x[12], y[12];
    to_affine_raw(acc, x, y);
    store_result(x, y, i, out_aff, out_ser);
}
#else
;
#endif

// ---- multiplication by SECRET scalars (blsgpu_g1_mul_gen_secret, blsgpu_hd_paths_secret) ---------------------------------
// out_i = s_i G1 on secret_window.h's schedule -- the claim and its limits are stated there; vmgen/g1fixs_model.py is the
// specification of the table and of the window schedule.  Particular to this kernel, cheaper than k_g2_smul because the
// point is fixed and public:
//   table      a SECOND table per context: entry (w, e) = (e + 1) 16^w G1 for w < 65, e < 8, affine (x, y) in L28 form --
//              520 x 112 bytes = 58 240 bytes, built once (k_fix_table_t<4>).  The 8-bit table above is not used.  The powers
//              of 16 are in the table: 65 mixed additions (r28::pmadd) and NO doubling for every scalar.
//   window     the address of window w's eight entries depends on w alone, the same for every lane (the compiler issues
//              them as scalar loads).  A zero digit cannot be an affine addend: entry 0 is selected and added all the same
//              and the old accumulator kept by a per-limb select.
//   output     to_affine_raw, then store_result as k_fix_mul: s G1 = (s mod n) G1, so the bytes are those of k_fix_mul.
// out_i = s_i G1 for n >= 1 scalars (32 bytes big-endian).  out_aff (n x 96 bytes, (0, 0) for infinity) and out_ser (n x 48
// bytes, PublicKey.serialize()) as k_fix_mul writes them; each may be NULL.
__global__ void __launch_bounds__(256) k_fix_mul_secret(const uint32_t* __restrict__ table, const uint32_t* __restrict__ scalars, uint32_t n,
                                                        uint32_t* __restrict__ out_aff, uint32_t* __restrict__ out_ser)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    __shared__ uint32_t rec[swin::REC_WORDS][256];
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x;
    const uint32_t i = min(tid, n - 1u);
    const bool store = tid < n;
    swin::recode(rec, lane, scalars + (size_t)i * 8);
    r28::ptT<r28::fe> acc = r28::pt_inf<r28::fe>();
#pragma unroll 1
    for (uint32_t w = 0; w < swin::WINDOWS; w++) {
        const swin::Digit d = swin::digit(rec, lane, w);
        uint32_t q[ENTRY_DW];
        swin::select_entry<ENTRY_DW, true>(q, table + (size_t)w * (swin::TAB * ENTRY_DW), 1, d.ad, d.mz);
        r28::fe x, y;
#pragma unroll
        for (int j = 0; j < r28::NL; j++) { x.v[j] = (int32_t)q[j]; y.v[j] = (int32_t)q[r28::NL + j]; }
        const r28::fe yn = r28::norm(r28::neg(y));
#pragma unroll
        for (int j = 0; j < r28::NL; j++) y.v[j] = swin::sel(yn.v[j], y.v[j], d.sgn);
        const r28::ptT<r28::fe> old = acc;
        r28::pmadd(acc, x, y);
#pragma unroll
        for (int j = 0; j < r28::NL; j++) {                                // a zero digit: the sum is dropped
            acc.X.v[j] = swin::sel(old.X.v[j], acc.X.v[j], d.mz);
            acc.Y.v[j] = swin::sel(old.Y.v[j], acc.Y.v[j], d.mz);
            acc.Z.v[j] = swin::sel(old.Z.v[j], acc.Z.v[j], d.mz);
        }
    }
    uint32_t x[12], y[12];
    to_affine_raw(acc, x, y);
    store_result(x, y, i, store ? out_aff : nullptr, store ? out_ser : nullptr);
}
#else
;
#endif

// One call's parent: the HMAC key midstates of the chain code, the parent's serialised keys as big-endian words and, for
// private derivation, its key mod n (little-endian words).
struct HdParent {
    hdk::HmacKey key;
    uint32_t pk_ser[12];        // PublicKey.serialize() of the parent (the message of an index < 2^31)
    uint32_t sk_ser[8];         // PrivateKey.serialize() (the message of a hardened index; private mode)
    uint32_t sk[8];             // parent key mod n (private mode)
    uint32_t priv;              // 1: private derivation
};

// Child i of the parent, one per lane (keys.py:191-215 / 276-296 of the reference): i_left, i_right = the two HMACs;
// chain[i] = i_right; scal[i] = i_left (public mode: the fixed-base kernel reduces it and adds the parent key) or the child
// key (i_left + sk) mod n (private mode).  chain / scal: n x 32 bytes.
__global__ void __launch_bounds__(256) k_hd_hmac(HdParent P, const uint32_t* __restrict__ idx, uint32_t n, uint32_t* __restrict__ chain,
                                                 uint32_t* __restrict__ scal)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t index = idx[i];
    const bool hardened = (index >> 31) != 0u;              // only in private mode (the host refuses them in public mode)
    uint32_t il[8], ir[8];
    if (P.priv && hardened) hdk::child_hmacs(P.key, P.sk_ser, 8, index, il, ir);
    else hdk::child_hmacs(P.key, P.pk_ser, 12, index, il, ir);
#pragma unroll
    for (int j = 0; j < 8; j++) chain[(size_t)i * 8 + j] = bswap32(ir[j]);
    if (P.priv) {
        uint32_t a[8], r[8];
#pragma unroll
        for (int j = 0; j < 8; j++) a[j] = il[7 - j];
        hdk::reduce_n(a);
        hdk::add_mod_n(r, a, P.sk);
#pragma unroll
        for (int j = 0; j < 8; j++) scal[(size_t)i * 8 + j] = bswap32(r[7 - j]);
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) scal[(size_t)i * 8 + j] = bswap32(il[j]);
    }
}
#else
;
#endif

// flag[0] |= 1 if any of the n indices is >= 2^31 (the _dev form of public derivation checks before it writes)
__global__ void __launch_bounds__(256) k_hd_check(const uint32_t* __restrict__ idx, uint32_t n, uint32_t* __restrict__ flag)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (idx[i] >> 31)) atomicOr(flag, 1u);
}
#else
;
#endif

// One level of n paths, one path per lane (keys.py:191-215 / 276-296 of the reference with the lane's OWN parent).  The
// lane's parent is record `src` of (chain_in, aff_in, sk_in): 32 bytes chain code, 96 bytes affine public key, 32 bytes
// private key (private mode), every array with a stride of rec_dw words -- 40 for the caller's parent records (first
// level: src = parent_of[p], or 0 without parent_of), or rec_dw = 0 for the state of the level before (strides 8 / 24 / 8,
// src = p).  The chain code is the HMAC key, so its two midstates are computed here, per lane and per level
// (hdk::hmac_key_words); the message is the parent key's serialisation (ser_flag, as k_fix_mul writes it) or, for a
// hardened index in private mode, the private key's bytes.  chain_out[p] = i_right; scal_out[p] = (i_left + sk) mod n
// (private) or i_left (public: k_fix_mul reduces it and adds the parent key).  chain_out / scal_out may be the state
// arrays this lane read (no other lane touches them).  aff_copy (or NULL): the parent key's 96 bytes per lane, the `add`
// of the first public level's k_fix_mul.  fp_out (or NULL): PublicKey.get_fingerprint of the parent key, 4 bytes
// big-endian -- the last level's parent_fingerprint.
// SECRET (k_hd_path_hmac_secret, private mode): the reductions mod n keep their subtraction by mask (hd_derive.h); the branch
// on a hardened index stays, indices are public.
template <bool SECRET>
__device__ __forceinline__ void hd_path_level(const uint32_t* chain_in, const uint32_t* sk_in, const uint32_t* __restrict__ aff_in,
                                              uint32_t rec_dw, const uint32_t* __restrict__ parent_of, uint32_t first,
                                              const uint32_t* __restrict__ idx, uint32_t idx_stride, uint32_t n, uint32_t priv,
                                              uint32_t* chain_out, uint32_t* scal_out, uint32_t* __restrict__ aff_copy,
                                              uint32_t* __restrict__ fp_out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const size_t src = first ? (parent_of ? parent_of[p] : 0u) : p;
    const uint32_t* a = aff_in + src * (rec_dw ? rec_dw : 24u);
    const uint32_t* c = chain_in + src * (rec_dw ? rec_dw : 8u);
    const uint32_t index = idx[(size_t)p * idx_stride];
    const bool hardened = (index >> 31) != 0u;              // only in private mode (refused in public mode before any launch)
    uint32_t x[12], y[12], ser[12], chain[8], sk_ser[8];
#pragma unroll
    for (int w = 0; w < 12; w++) {
        const uint32_t xw = a[w], yw = a[12 + w];
        if (aff_copy) { aff_copy[(size_t)p * 24 + w] = xw; aff_copy[(size_t)p * 24 + 12 + w] = yw; }
        x[11 - w] = bswap32(xw);
        y[11 - w] = bswap32(yw);
    }
    ser_flag(x, y);
#pragma unroll
    for (int w = 0; w < 12; w++) ser[w] = x[11 - w];
#pragma unroll
    for (int j = 0; j < 8; j++) chain[j] = bswap32(c[j]);
    if (priv) {
        const uint32_t* s = sk_in + src * (rec_dw ? rec_dw : 8u);
#pragma unroll
        for (int j = 0; j < 8; j++) sk_ser[j] = bswap32(s[j]);
    }
    if (fp_out) fp_out[p] = bswap32(hdk::fingerprint(ser));
    hdk::HmacKey key;
    hdk::hmac_key_words(chain, key);
    uint32_t il[8], ir[8];
    if (priv && hardened) hdk::child_hmacs(key, sk_ser, 8, index, il, ir);
    else hdk::child_hmacs(key, ser, 12, index, il, ir);
#pragma unroll
    for (int j = 0; j < 8; j++) chain_out[(size_t)p * 8 + j] = bswap32(ir[j]);
    if (priv) {
        uint32_t l[8], k[8], r[8];
#pragma unroll
        for (int j = 0; j < 8; j++) { l[j] = il[7 - j]; k[j] = sk_ser[7 - j]; }
        if (SECRET) {
            hdk::reduce_n_masked(l);
            hdk::reduce_n_masked(k);
            hdk::add_mod_n_masked(r, l, k);
        } else {
            hdk::reduce_n(l);
            hdk::reduce_n(k);
            hdk::add_mod_n(r, l, k);
        }
#pragma unroll
        for (int j = 0; j < 8; j++) scal_out[(size_t)p * 8 + j] = bswap32(r[7 - j]);
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) scal_out[(size_t)p * 8 + j] = bswap32(il[j]);
    }
}
#define BLSGPU_HD_PATH_ARGS                                                                                                       \
    const uint32_t *chain_in, const uint32_t *sk_in, const uint32_t *__restrict__ aff_in, uint32_t rec_dw,                        \
        const uint32_t *__restrict__ parent_of, uint32_t first, const uint32_t *__restrict__ idx, uint32_t idx_stride, uint32_t n, \
        uint32_t priv, uint32_t *chain_out, uint32_t *scal_out, uint32_t *__restrict__ aff_copy, uint32_t *__restrict__ fp_out
__global__ void __launch_bounds__(256) k_hd_path_hmac(BLSGPU_HD_PATH_ARGS)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    hd_path_level<false>(chain_in, sk_in, aff_in, rec_dw, parent_of, first, idx, idx_stride, n, priv, chain_out, scal_out, aff_copy, fp_out);
}
#else
;
#endif
__global__ void __launch_bounds__(256) k_hd_path_hmac_secret(BLSGPU_HD_PATH_ARGS)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    hd_path_level<true>(chain_in, sk_in, aff_in, rec_dw, parent_of, first, idx, idx_stride, n, priv, chain_out, scal_out, aff_copy, fp_out);
}
#else
;
#endif
#undef BLSGPU_HD_PATH_ARGS

// The validity scan of blsgpu_hd_paths_dev, one path per lane: flag[0] |= 2 if parent_of[p] >= n_parents, |= 1 if (pub)
// any of the path's `depth` indices is >= 2^31
__global__ void __launch_bounds__(256) k_hd_path_check(const uint32_t* __restrict__ parent_of, uint32_t n_parents,
                                                       const uint32_t* __restrict__ idx, uint32_t depth, uint32_t pub, uint32_t n,
                                                       uint32_t* __restrict__ flag)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (parent_of && parent_of[p] >= n_parents) atomicOr(flag, 2u);
    if (pub) {
        uint32_t any = 0;
        for (uint32_t l = 0; l < depth; l++) any |= idx[(size_t)p * depth + l];
        if (any >> 31) atomicOr(flag, 1u);
    }
}
#else
;
#endif

}  // namespace g1fix
}  // namespace blsgpu
