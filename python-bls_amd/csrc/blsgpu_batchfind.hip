// blsgpu_batchfind.hip -- the glue kernels of blsgpu_verify_find (include/blsgpu.h): ordinary signatures with their own keys
// and messages checked on the device, all of them by ONE random linear combination, and only what fails bisected down to the
// signatures that are wrong (included by blsgpu_api.hip, built with blsgpu_sigshares.hip in translation unit 8).  The structure
// is blsgpu_sigshares.hip's with two differences: every item has its own H(h), so a node is a multi-pairing of its items' pairs
// and only the G2 side is summed; and the nodes are cut from the DENSE order of the eligible items, so no slot is padded.
// The expensive steps are the library's own kernels -- subgroup checks, hash to G2, k_smul64 for the leaves, the plain G2 group
// sum, blsgpu_pairing_multi_batch_dev --; the five kernels here join them:
//   k_find_settle    one item per lane: the item SETTLED where it cannot enter a sum -- status 0 for a signature off the twist,
//                    outside G2 or at infinity (whatever its key), status 2 for a key off the curve, outside G1 or at infinity
//                    or an H(h) at infinity --; every other item is ELIGIBLE and starts as 1: only a failing leaf test takes
//                    that back.  The item's weight copied with a zero weight taken as 1.
//   k_find_dense     one workgroup: the eligible items' indices in input order (a ballot scan, 1024 items a step) and their
//                    count n_e, which the host reads once.
//   k_find_gather    one 16-byte piece per lane: the leaves A_i = r_i sig_i of this launch's nodes (offset; all of one length)
//                    packed node after node for the G2 group sum S_node.
//   k_find_pairs     one 16-byte piece per lane: per node the pairs (-G1, S_node), (B_i, H(h_i)) for its items, B_i = r_i P_i,
//                    in the layout of blsgpu_pairing_multi_batch_dev.  A sum at infinity is never fed to the pairing: a node
//                    with S = O gets (-G1, G2) in that place, and its result is compared with e(-G1, G2) instead of one (unit:
//                    that constant, computed by the pairing itself once per context) -- the node is decided by
//                    prod e(B_i, H(h_i)) = 1 alone.  With 0 < r_i < 2^64 < n, the key in G1 and not infinity and H != O,
//                    neither B_i nor H(h_i) is ever at infinity, and a LEAF's S = r_i sig_i is not either.
//   k_find_verdict   one node per lane: 1 if the node's equation holds, else 0 -- the one byte per node the host reads back.  In
//                    the round of leaves it writes the item's status 0 or 1 itself.
// What is claimed, and nothing stronger: a FAILING leaf test is exact -- r_i != 0 mod n, so the leaf's equation holds iff the
// item's does --; a node that PASSES although it holds an invalid eligible item does so with probability at most 2^-64 over the
// caller's weights, per node (blsgpu_sigshares.hip's argument with delta_i = sig_i - sk_i H(h_i)).
// Every store is a plain C++ store; no inline assembly.
#pragma once

namespace blsgpu {
namespace bfind {

constexpr uint32_t THREADS = 256, DENSE_THREADS = 1024;
constexpr uint32_t G1_Q = 6, G2_Q = 12;                      // 16-byte pieces of an affine G1 / G2 point
constexpr uint32_t E_Q = BLSGPU_FQ12_BYTES / 16;             // ... of a pairing result

// sig_st / key_st: the bytes of k_g2_subgroup over the items / k_g1_subgroup over the key table; h: n_msgs x 48 words
__global__ void __launch_bounds__(256) k_find_settle(const uint32_t* __restrict__ sigs, const uint8_t* __restrict__ sig_st,
                                                     const uint32_t* __restrict__ keys, const uint8_t* __restrict__ key_st,
                                                     const uint32_t* __restrict__ key_idx, const uint32_t* __restrict__ h,
                                                     const uint32_t* __restrict__ msg_idx, const uint8_t* __restrict__ weights, uint32_t n,
                                                     uint8_t* __restrict__ r_be, uint8_t* __restrict__ elig, uint8_t* __restrict__ status)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t wz = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) wz |= weights[(size_t)i * 8 + j];
#pragma unroll
    for (int j = 0; j < 8; j++) r_be[(size_t)i * 8 + j] = (j == 7 && wz == 0) ? 1 : weights[(size_t)i * 8 + j];   // a zero weight is taken as 1
    uint32_t sa = 0, ka = 0, ha = 0;
#pragma unroll
    for (int j = 0; j < 48; j++) sa |= sigs[(size_t)i * 48 + j];
    const uint32_t ki = key_idx[i], mi = msg_idx[i];
#pragma unroll
    for (int j = 0; j < 24; j++) ka |= keys[(size_t)ki * 24 + j];
#pragma unroll
    for (int j = 0; j < 48; j++) ha |= h[(size_t)mi * 48 + j];
    const bool sig_ok = sig_st[i] == 1 && sa != 0;
    const bool ok = sig_ok && key_st[ki] == 1 && ka != 0 && ha != 0;
    elig[i] = ok ? 1 : 0;
    status[i] = !sig_ok ? 0 : (ok ? 1 : 2);
}
#else
;
#endif

// dense[0 .. n_e) = the i with elig[i] != 0 in input order; *n_e their count.  One workgroup of DENSE_THREADS lanes.
__global__ void __launch_bounds__(1024) k_find_dense(const uint8_t* __restrict__ elig, uint32_t n, uint32_t* __restrict__ dense,
                                                     uint32_t* __restrict__ n_e)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    __shared__ uint32_t wsum[DENSE_THREADS / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    uint32_t run = 0;
    for (uint32_t base = 0; base < n; base += DENSE_THREADS) {
        const uint32_t i = base + t;
        const bool f = i < n && elig[i] != 0;
        const unsigned long long b = __ballot(f);
        if (lane == 0) wsum[wv] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t j = 0; j < DENSE_THREADS / 64; j++) {
            before += j < wv ? wsum[j] : 0u;
            total += wsum[j];
        }
        if (f) dense[run + before + (uint32_t)__popcll(b & (((unsigned long long)1 << lane) - 1ull))] = i;
        run += total;
        __syncthreads();
    }
    if (t == 0) *n_e = run;
}
#else
;
#endif

// total = nodes x len x 12 pieces; offsets: the nodes' first positions in the dense order; a: the leaves A by item
__global__ void __launch_bounds__(256) k_find_gather(const uint32_t* __restrict__ offsets, uint32_t len, size_t total,
                                                     const uint32_t* __restrict__ dense, const uint4* __restrict__ a, uint4* __restrict__ ga)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const size_t idx = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t slot = idx / G2_Q;
    const uint32_t piece = (uint32_t)(idx - slot * G2_Q);
    const size_t node = slot / len;
    const uint32_t item = dense[offsets[node] + (uint32_t)(slot - node * len)];
    ga[idx] = a[(size_t)item * G2_Q + piece];
}
#else
;
#endif

// total = nodes x (len + 1) x 18 pieces: g1 nodes x (len + 1) x 96 bytes, g2 nodes x (len + 1) x 192 bytes
__global__ void __launch_bounds__(256) k_find_pairs(const uint32_t* __restrict__ offsets, uint32_t len, size_t total,
                                                    const uint32_t* __restrict__ dense, const uint4* __restrict__ s,
                                                    const uint8_t* __restrict__ s_inf, const uint4* __restrict__ b,
                                                    const uint4* __restrict__ h, const uint32_t* __restrict__ msg_idx,
                                                    uint4* __restrict__ g1, uint4* __restrict__ g2)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    constexpr uint32_t PER = G1_Q + G2_Q;
    const size_t idx = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t pair = idx / PER;
    const uint32_t piece = (uint32_t)(idx - pair * PER);
    const size_t node = pair / (len + 1u);
    const uint32_t j = (uint32_t)(pair - node * (len + 1u));
    if (j == 0) {
        if (piece < G1_Q) g1[pair * G1_Q + piece] = sigsh::neg_g1_piece(piece);
        else g2[pair * G2_Q + (piece - G1_Q)] = s_inf[node] != 0 ? sigsh::g2_gen_piece(piece - G1_Q) : s[node * G2_Q + (piece - G1_Q)];
        return;
    }
    const uint32_t item = dense[offsets[node] + j - 1u];
    if (piece < G1_Q) g1[pair * G1_Q + piece] = b[(size_t)item * G1_Q + piece];
    else g2[pair * G2_Q + (piece - G1_Q)] = h[(size_t)msg_idx[item] * G2_Q + (piece - G1_Q)];
}
#else
;
#endif

// one node per lane; e: nodes x 576 bytes, the results of the pairings; unit: e(-G1, G2), what a node with S = O is compared
// with; leaves: the nodes have length 1 and their verdict is their item's status
__global__ void __launch_bounds__(256) k_find_verdict(const uint32_t* __restrict__ offsets, uint32_t n_nodes, const uint4* __restrict__ e,
                                                      const uint8_t* __restrict__ s_inf, const uint4* __restrict__ unit, uint32_t leaves,
                                                      const uint32_t* __restrict__ dense, uint8_t* __restrict__ verdict,
                                                      uint8_t* __restrict__ status)
#if BLSGPU_EMIT(BLSGPU_TU_FIX)
{
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_nodes) return;
    const bool si = s_inf[i] != 0;
    uint32_t diff = 0;
#pragma unroll 4
    for (uint32_t j = 0; j < E_Q; j++) {
        const uint4 v = e[(size_t)i * E_Q + j];
        if (si) {
            const uint4 u = unit[j];
            diff |= (v.x ^ u.x) | (v.y ^ u.y) | (v.z ^ u.z) | (v.w ^ u.w);
        } else {
            // Fq12 one: the byte 1 at offset 47 (the last of the first 48-byte coefficient), zeros elsewhere
            diff |= v.x | v.y | v.z | (j == 2 ? v.w ^ 0x01000000u : v.w);
        }
    }
    const bool pass = diff == 0;
    verdict[i] = pass ? 1 : 0;
    if (leaves) status[dense[offsets[i]]] = pass ? 1 : 0;
}
#else
;
#endif

}  // namespace bfind
}  // namespace blsgpu
