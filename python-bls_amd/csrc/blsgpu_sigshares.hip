// blsgpu_sigshares.hip -- the glue kernels of blsgpu_sig_shares_check (include/blsgpu.h): signature shares of threshold
// sessions checked on the device, a whole session by ONE random linear combination, and only the sessions that fail
// bisected down to the shares that are wrong (included by blsgpu_api.hip, built with blsgpu_lagrange.hip in translation
// unit 8).  The expensive steps are the library's own kernels on their _dev paths -- subgroup checks, hash to G2, Lagrange
// coefficients, the G1 / G2 sums, the two-pair pairings --; the four kernels here join them:
//   k_share_weights   one share per lane, on fr_scalar.h: r_i (the caller's 64-bit weight, a zero weight taken as 1) and
//                     w_i = r_i lambda_i mod n (scaled) or r_i, both as the 32-byte big-endian scalars the sums take; the
//                     share's key copied next to it (the G1 sum wants its points in the order of its scalars); and the
//                     share SETTLED where it cannot enter a sum: status 0 for a share off the twist, outside G2, at
//                     infinity or in a session whose player set blsgpu_lagrange_at_zero refuses, status 2 for a key off
//                     the curve or outside G1 (a bad share with a bad key is 0: it is invalid whatever the key).  Every
//                     other share is ELIGIBLE and starts as 1: only a failing leaf test takes that back.  Lane j = 0 of a
//                     session also notes whether H(m) is the point at infinity.
//   k_share_gather    one 16-byte piece of one slot per lane: the leaves A_i = r_i sigma_i and B_i = w_i PK_i of this
//                     round's nodes (session, offset; all of one length, a power of two) packed node after node; a slot
//                     past the session's k shares or of a share that is not eligible is (0, 0), the sums' infinity.
//   k_share_pairs     one 16-byte piece per lane: the pairs (-G1, S_node), (P_node, H(m_session)) of every node.  A sum at
//                     infinity is never fed to the pairing: such a node (or one whose H(m) is infinity) gets the placeholder
//                     (-G1, G2) twice, whose result k_share_verdict does not look at.
//   k_share_verdict   one node per lane: 1 if the node's equation e(G1, S) = e(P, H(m)) holds, else 0 -- the one byte per
//                     node the host reads back.  Every point is in its prime-order subgroup here, so with H(m) != O: both
//                     sums at infinity pass, exactly one fails, neither: the pairing result is compared with one.  With
//                     H(m) = O the node passes iff S = O.  In the round of leaves a failing node writes its share's
//                     status 0.
// What is claimed, and nothing stronger: a FAILING leaf test is exact -- r_i != 0 mod n (0 < r_i < 2^64), so the leaf's
// equation holds iff the share's does --; a node that PASSES although one of its eligible shares is invalid does so with
// probability at most 2^-64 over the caller's weights, per node.
// Every store is a plain C++ store; no LDS, no inline assembly.
#pragma once
#include "fr_scalar.h"

namespace blsgpu {
namespace sigsh {

constexpr uint32_t THREADS = 256;
constexpr uint32_t G1_Q = 6, G2_Q = 12;                      // 16-byte pieces of an affine G1 / G2 point
struct Node { uint32_t session, offset; };

// -G1 and the generator of G2 (ec.py:394-403 of the reference) as the ABI's bytes, read as little-endian words
#define SIGSH_NEG_G1_WORDS { \
    0xa7d3f117u, 0x94d79731u, 0x8c639526u, 0x0faca94fu, 0x4f8c68c3u, 0x05b97497u, 0x3f3a4ea1u, 0x58ac1b17u, 0x3fe8556cu, 0xef1a7af9u, \
    0x0af03afbu, 0xbbc622dbu, 0x681d4d11u, 0xa845d555u, 0xc8767daau, 0xf2212ecfu, 0xef6a8167u, 0xc907b51du, 0xd5b95566u, 0x3642accau, \
    0xba386f4eu, 0x1b75cb0eu, 0xd6dc54adu, 0xcac239b9u}
#define SIGSH_G1_GEN_WORDS { /* G1: -G1's x, q minus its y (the cancelling couples of blsgpu_pscan.hip k_fold_fill) */ \
    0xa7d3f117u, 0x94d79731u, 0x8c639526u, 0x0faca94fu, 0x4f8c68c3u, 0x05b97497u, 0x3f3a4ea1u, 0x58ac1b17u, 0x3fe8556cu, 0xef1a7af9u, \
    0x0af03afbu, 0xbbc622dbu, 0x81f4b308u, 0xf1a0aae3u, 0xed309ea0u, 0xe48a1d74u, 0x95e0f5fcu, 0xf60ad0d5u, 0xcb18db00u, 0xedb3042cu, \
    0x44c73cd0u, 0xe48a88a2u, 0x2923aa0cu, 0xe1e7c546u}
#define SIGSH_G2_GEN_WORDS { \
    0xb2a24a02u, 0x910a8ff0u, 0x27050826u, 0x5110c52du, 0xd47ae4c6u, 0x023b40fau, 0x640b51b4u, 0x77d1e37au, 0x2603ac0bu, 0xefbb05a8u, \
    0xc85680d4u, 0xb8bd21c1u, 0x602be013u, 0x609f7152u, 0xa0d3ac7du, 0x654f2788u, 0xd0d06b59u, 0x1ab62099u, 0xbb61dab5u, 0x49507fdcu, \
    0x12f14c33u, 0x575d9413u, 0x057dace5u, 0x7e2b045du, 0x27d5e50cu, 0x116e7d72u, 0xc6cdc98cu, 0x1a352edau, 0xaa9bfdadu, 0xa7d3bd8cu, \
    0x699a426du, 0x2cd16051u, 0xccc93a92u, 0x89a2ac3bu, 0x865493e1u, 0x0128b808u, 0xa0c40606u, 0xcc34a72eu, 0xb0d2ac32u, 0x998bc22bu, \
    0x7e283ecbu, 0xaf63a785u, 0xab927426u, 0xab992e57u, 0x270d373fu, 0xa11dec5cu, 0x5f07a9aau, 0xbe795ff0u}

__device__ __forceinline__ uint4 neg_g1_piece(uint32_t piece) {
    const uint32_t w[24] = SIGSH_NEG_G1_WORDS;
    return make_uint4(w[4 * piece], w[4 * piece + 1], w[4 * piece + 2], w[4 * piece + 3]);
}
__device__ __forceinline__ uint4 g1_gen_piece(uint32_t piece) {
    const uint32_t w[24] = SIGSH_G1_GEN_WORDS;
    return make_uint4(w[4 * piece], w[4 * piece + 1], w[4 * piece + 2], w[4 * piece + 3]);
}
__device__ __forceinline__ uint4 g2_gen_piece(uint32_t piece) {
    const uint32_t w[48] = SIGSH_G2_GEN_WORDS;
    return make_uint4(w[4 * piece], w[4 * piece + 1], w[4 * piece + 2], w[4 * piece + 3]);
}

// n = sessions x k shares of one slice.  sig_st / key_st: the bytes of k_g2_subgroup / k_g1_subgroup; lambda, sess_st: NULL
// when not scaled; h: sessions x 48 words.
__global__ void __launch_bounds__(256) k_share_weights(const uint32_t* __restrict__ sigs, const uint8_t* __restrict__ sig_st,
                                                       const uint32_t* __restrict__ keys, const uint8_t* __restrict__ key_st,
                                                       const uint32_t* __restrict__ key_idx, const uint8_t* __restrict__ lambda,
                                                       const uint8_t* __restrict__ sess_st, const uint8_t* __restrict__ weights,
                                                       const uint32_t* __restrict__ h, uint32_t k, uint32_t n, uint8_t* __restrict__ r_be,
                                                       uint8_t* __restrict__ w_be, uint32_t* __restrict__ pk, uint8_t* __restrict__ elig,
                                                       uint8_t* __restrict__ h_inf, uint8_t* __restrict__ status)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = i / k;
    uint32_t r[8], w[8];
    frs::set_zero(r);
    const uint8_t* wb = weights + (size_t)i * 8;
    r[1] = ((uint32_t)wb[0] << 24) | ((uint32_t)wb[1] << 16) | ((uint32_t)wb[2] << 8) | wb[3];
    r[0] = ((uint32_t)wb[4] << 24) | ((uint32_t)wb[5] << 16) | ((uint32_t)wb[6] << 8) | wb[7];
    if ((r[0] | r[1]) == 0) r[0] = 1;                                        // a zero weight is taken as 1
    frs::copy(w, r);
    if (lambda) {
        uint32_t l[8];
        frs::from_be(lambda + (size_t)i * 32, l);                            // canonical, below n
        frs::to_mont(w, r);
        frs::mul(w, w, l);                                                   // (r R) lambda / R
    }
    frs::to_be(r, r_be + (size_t)i * 32);
    frs::to_be(w, w_be + (size_t)i * 32);
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < 48; j++) any |= sigs[(size_t)i * 48 + j];
    const bool share_ok = sig_st[i] == 1 && any != 0 && (!sess_st || sess_st[g] == 1);
    const uint32_t ki = key_idx[i];
    const bool ok = share_ok && key_st[ki] == 1;
#pragma unroll
    for (int j = 0; j < 24; j++) pk[(size_t)i * 24 + j] = ok ? keys[(size_t)ki * 24 + j] : 0u;
    elig[i] = ok ? 1 : 0;
    status[i] = !share_ok ? 0 : (ok ? 1 : 2);
    if (i == g * k) {
        uint32_t hz = 0;
#pragma unroll
        for (int j = 0; j < 48; j++) hz |= h[(size_t)g * 48 + j];
        h_inf[g] = hz == 0 ? 1 : 0;
    }
}
#else
;
#endif

// total = nodes x len x 18 pieces (len = 1 << lg); a, b: the leaves of the slice, share (s, i) at s * k + i
__global__ void __launch_bounds__(256) k_share_gather(const Node* __restrict__ nodes, uint32_t lg, size_t total, uint32_t k,
                                                      const uint4* __restrict__ a, const uint4* __restrict__ b,
                                                      const uint8_t* __restrict__ elig, uint4* __restrict__ ga, uint4* __restrict__ gb)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const size_t idx = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t slot = idx / (G2_Q + G1_Q);
    const uint32_t piece = (uint32_t)(idx - slot * (G2_Q + G1_Q));
    const uint32_t ses = nodes[slot >> lg].session, first = nodes[slot >> lg].offset;
    const uint32_t leaf = first + (uint32_t)(slot & (((size_t)1 << lg) - 1));
    const size_t src = (size_t)ses * k + leaf;
    const bool a_side = piece < G2_Q;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (leaf < k && elig[src] != 0) v = a_side ? a[src * G2_Q + piece] : b[src * G1_Q + (piece - G2_Q)];
    if (a_side) ga[slot * G2_Q + piece] = v;
    else gb[slot * G1_Q + (piece - G2_Q)] = v;
}
#else
;
#endif

// total = nodes x 36 pieces: g1 nodes x 2 x 96 bytes, g2 nodes x 2 x 192 bytes in the layout of blsgpu_pairing_multi_batch_dev
__global__ void __launch_bounds__(256) k_share_pairs(const Node* __restrict__ nodes, size_t total, const uint4* __restrict__ s,
                                                     const uint8_t* __restrict__ s_inf, const uint4* __restrict__ p,
                                                     const uint8_t* __restrict__ p_inf, const uint4* __restrict__ h,
                                                     const uint8_t* __restrict__ h_inf, uint4* __restrict__ g1, uint4* __restrict__ g2)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    constexpr uint32_t PER = 2 * G1_Q + 2 * G2_Q;
    const size_t idx = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t node = idx / PER;
    const uint32_t piece = (uint32_t)(idx - node * PER);
    const uint32_t ses = nodes[node].session;
    const bool held = s_inf[node] != 0 || p_inf[node] != 0 || h_inf[ses] != 0;          // the placeholder pair instead
    if (piece < G1_Q) {
        g1[node * 2 * G1_Q + piece] = neg_g1_piece(piece);
    } else if (piece < 2 * G1_Q) {
        const uint32_t q = piece - G1_Q;
        g1[node * 2 * G1_Q + piece] = held ? neg_g1_piece(q) : p[node * G1_Q + q];
    } else if (piece < 2 * G1_Q + G2_Q) {
        const uint32_t q = piece - 2 * G1_Q;
        g2[node * 2 * G2_Q + q] = held ? g2_gen_piece(q) : s[node * G2_Q + q];
    } else {
        const uint32_t q = piece - 2 * G1_Q - G2_Q;
        g2[node * 2 * G2_Q + G2_Q + q] = held ? g2_gen_piece(q) : h[(size_t)ses * G2_Q + q];
    }
}
#else
;
#endif

// one node per lane; e: nodes x 576 bytes, the results of the pairings; leaves: the nodes have length 1
__global__ void __launch_bounds__(256) k_share_verdict(const Node* __restrict__ nodes, uint32_t n_nodes, const uint4* __restrict__ e,
                                                       const uint8_t* __restrict__ s_inf, const uint8_t* __restrict__ p_inf,
                                                       const uint8_t* __restrict__ h_inf, uint32_t leaves, uint32_t k,
                                                       uint8_t* __restrict__ verdict, uint8_t* __restrict__ status)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_nodes) return;
    const Node nd = nodes[i];
    const bool si = s_inf[i] != 0, pi = p_inf[i] != 0;
    bool pass;
    if (h_inf[nd.session]) {
        pass = si;
    } else if (si || pi) {
        pass = si && pi;
    } else {
        // Fq12 one: the byte 1 at offset 47 (the last of the first 48-byte coefficient), zeros elsewhere
        uint32_t diff = 0;
#pragma unroll 4
        for (uint32_t j = 0; j < BLSGPU_FQ12_BYTES / 16; j++) {
            const uint4 v = e[(size_t)i * (BLSGPU_FQ12_BYTES / 16) + j];
            diff |= v.x | v.y | v.z | (j == 2 ? v.w ^ 0x01000000u : v.w);
        }
        pass = diff == 0;
    }
    verdict[i] = pass ? 1 : 0;
    if (leaves && !pass && nd.offset < k) status[(size_t)nd.session * k + nd.offset] = 0;
}
#else
;
#endif

}  // namespace sigsh
}  // namespace blsgpu
