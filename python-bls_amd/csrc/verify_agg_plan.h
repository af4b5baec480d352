// verify_agg_plan.h -- the whole schedule of blsgpu_verify_aggregates* (blsgpu_api.hip, kernels in blsgpu_veragg.hip) as
// arithmetic on host integers (plain C++, no HIP: compiled for the host and compared with tests/verify_agg_model.py by
// tests/test_verify_agg_plan_host.py).  From the caller's three HOST tables (grp_off, grp_msg, agg_off), the sizes and the
// knobs: the validation, the key ranges of the sums, the pair slots, the cut into slices, each slice's range table (and the
// plan of its ragged multi-pairing, pairing_ranges_plan.h), the source table k_va_pairs reads, the sizes of the buffers and
// the grids.  Nothing is read back from the device.
//
//   groups   group g sums the keys [grp_off[g], grp_off[g + 1]) and is paired with H(msg_hashes[grp_msg[g]]); its key range
//            goes to the ragged sums as it is.  ALL groups are summed, and all n_msgs hashes mapped, once ahead of the slices.
//   slots    aggregate j owns the groups [agg_off[j], agg_off[j + 1]) and the pair slots [slot(j), slot(j + 1)),
//            slot(j) = agg_off[j] - agg_off[0] + j: the first is the signature's pair (-G1, sig_j), the others its groups' in
//            order.  (With agg_off[0] == 0, as callers write it, that is [agg_off[j] + j, agg_off[j + 1] + j + 1).)
//   slices   cut on AGGREGATE boundaries: a slice takes aggregates while its pairs stay within Limits::ls_max_pairs (the test
//            hook BLSGPU_TEST_SLICE_CAP shortens it); an aggregate longer than that is a slice of its own, and the ragged
//            multi-pairing cuts its pair list further.  Per slice one launch of k_va_pairs, one ragged multi-pairing with a
//            range per aggregate, one launch of k_va_status.
//   sources  per slot three uint32: (SIG, j, j) for a signature's slot, (g, grp_msg[g], j) for a group's.
//   tables   ONE upload: -G1 | the key ranges | per slice its source table and the table image of its multi-pairing.
#pragma once
#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "layout.h"
#include "pairing_ranges_plan.h"
#include "ragged_plan.h"

namespace verify_agg {

constexpr uint32_t SIG = 0xFFFFFFFFu;                        // a source entry's first word: the slot is a signature's
constexpr size_t MAX_MSGS = 0x03FFFFF0ull;                   // as the hash to G2
constexpr size_t MAX_AGGS = 0x3FFFFFF0ull;                   // every aggregate is a pair at least
constexpr size_t SRC_BYTES = 12;                             // a source entry: three uint32
constexpr size_t G1_BYTES = 96, G2_BYTES = 192, GT_BYTES = 576;
constexpr size_t PIECES = (G1_BYTES + G2_BYTES) / 16;        // 16-byte moves per slot: a lane of k_va_pairs each
constexpr size_t THREADS = 256;

enum Refusal { OK, TOO_LARGE, GRP_OFF_DOWN, GRP_OFF_END, AGG_OFF_DOWN, AGG_OFF_END, BAD_MSG, REFUSALS };
inline int refusal_code(Refusal r) { return r == OK ? 0 : -EINVAL; }
inline const char* refusal_text(Refusal r) {
    switch (r) {
    case TOO_LARGE: return "batch too large";
    case GRP_OFF_DOWN: return "grp_off steps down";
    case GRP_OFF_END: return "grp_off does not end at n_keys";
    case AGG_OFF_DOWN: return "agg_off steps down";
    case AGG_OFF_END: return "agg_off does not end at n_grp";
    case BAD_MSG: return "grp_msg out of range";
    default: return "";
    }
}

struct Src { uint32_t a, b, agg; };                          // (SIG, j, j) or (g, grp_msg[g], j)
static_assert(sizeof(Src) == SRC_BYTES, "the table is uploaded as it is");

struct Slice {
    size_t agg0, aggs;                 // the aggregates [agg0, agg0 + aggs)
    size_t slot0, pairs;               // their slots [slot0, slot0 + pairs) of the call: slot 0 of the slice's pair list is slot0
    std::vector<uint32_t> ranges;      // aggs x (begin, end) within the slice's pair list
    pairing_ranges::Plan pr;           // the ragged multi-pairing of those ranges
    size_t src_off, prtab_off;         // its source table and the image of pr's tables in the workspace
    unsigned g_pairs, g_status;        // workgroups of k_va_pairs (a lane per 16-byte piece) and k_va_status (a lane per aggregate)
};

struct Plan {
    Refusal refusal;
    size_t bad;                        // the first offending entry: g of grp_off[g] > grp_off[g + 1] / of grp_msg[g]; j of agg_off[j] > agg_off[j + 1]; n_grp / m for the ends
    size_t m, n_grp, n_keys, n_msgs, pairs, cap;             // pairs: slots in all; cap: pairs per slice as used
    std::vector<uint32_t> key_ranges;  // n_grp x (begin, end): what the sums take
    std::vector<Src> src;              // slot after slot, slice after slice
    std::vector<Slice> slices;
    size_t max_pairs, max_aggs;        // of one slice
    size_t lines_bytes, bad_bytes, degen_bytes, pairr_bytes; // the largest of the slices' multi-pairings: grown once, before the first launch
    // the workspace: the sums and their flags, the hashed points, the undecided bytes, one slice's pair list and results, then
    // every table ([o_tables, ws_bytes) is ONE upload)
    size_t o_sum, o_flag, o_h, o_und, o_g1, o_g2, o_gt, o_tables, o_neg, o_kr, ws_bytes;
    // the image of [o_tables, ws_bytes): dst holds ws_bytes - o_tables bytes; neg_g1: the 96 bytes of -G1
    void fill_tables(void* dst, const void* neg_g1) const {
        char* d = (char*)dst;
        memset(d, 0, ws_bytes - o_tables);
        memcpy(d + (o_neg - o_tables), neg_g1, G1_BYTES);
        if (n_grp) memcpy(d + (o_kr - o_tables), key_ranges.data(), n_grp * 8);
        for (const Slice& s : slices) {
            memcpy(d + (s.src_off - o_tables), src.data() + s.slot0, s.pairs * SRC_BYTES);
            s.pr.fill_tables(d + (s.prtab_off - o_tables));
        }
    }
};

// grp_off: n_grp + 1, grp_msg: n_grp, agg_off: m + 1 entries (m > 0).  A refused plan holds no table.
inline Plan plan(const uint32_t* grp_off, const uint32_t* grp_msg, size_t n_grp, const uint32_t* agg_off, size_t m, size_t n_keys,
                 size_t n_msgs, const pairing_ranges::Knobs& rk, const pairing::Knobs& pk, const pairing::Consts& K, const pairing::Limits& L,
                 const msm::Consts& MK) {
    Plan p{};
    p.m = m, p.n_grp = n_grp, p.n_keys = n_keys, p.n_msgs = n_msgs;
    p.cap = L.ls_max_pairs ? L.ls_max_pairs : 1;
    if (m > MAX_AGGS || n_grp > MAX_AGGS || m + n_grp > pairing_ranges::MAX_PAIRS || n_msgs > MAX_MSGS || ragged::too_large(MK, n_keys, n_grp)) {
        p.refusal = TOO_LARGE;
        return p;
    }
    for (size_t g = 0; g < n_grp; g++)
        if (grp_off[g] > grp_off[g + 1]) { p.refusal = GRP_OFF_DOWN, p.bad = g; return p; }
    if (grp_off[n_grp] != n_keys) { p.refusal = GRP_OFF_END, p.bad = n_grp; return p; }
    for (size_t j = 0; j < m; j++)
        if (agg_off[j] > agg_off[j + 1]) { p.refusal = AGG_OFF_DOWN, p.bad = j; return p; }
    if (agg_off[m] != n_grp) { p.refusal = AGG_OFF_END, p.bad = m; return p; }
    for (size_t g = 0; g < n_grp; g++)
        if (grp_msg[g] >= n_msgs) { p.refusal = BAD_MSG, p.bad = g; return p; }

    p.key_ranges.resize(2 * n_grp);
    for (size_t g = 0; g < n_grp; g++) p.key_ranges[2 * g] = grp_off[g], p.key_ranges[2 * g + 1] = grp_off[g + 1];
    const size_t first = agg_off[0];
    auto slot = [&](size_t j) { return (size_t)agg_off[j] - first + j; };
    p.pairs = slot(m);
    p.src.resize(p.pairs);
    for (size_t j = 0; j < m; j++) {
        size_t at = slot(j);
        p.src[at++] = {SIG, (uint32_t)j, (uint32_t)j};
        for (size_t g = agg_off[j]; g < agg_off[j + 1]; g++) p.src[at++] = {(uint32_t)g, grp_msg[g], (uint32_t)j};
    }
    // the slices: whole aggregates while the pairs stay within the cap
    for (size_t j = 0; j < m;) {
        Slice s{};
        s.agg0 = j, s.slot0 = slot(j);
        do j++; while (j < m && slot(j + 1) - s.slot0 <= p.cap);
        s.aggs = j - s.agg0, s.pairs = slot(j) - s.slot0;
        s.ranges.resize(2 * s.aggs);
        for (size_t i = 0; i < s.aggs; i++)
            s.ranges[2 * i] = (uint32_t)(slot(s.agg0 + i) - s.slot0), s.ranges[2 * i + 1] = (uint32_t)(slot(s.agg0 + i + 1) - s.slot0);
        s.pr = pairing_ranges::plan(s.pairs, s.ranges.data(), s.aggs, rk, pk, K, L);
        if (s.pr.refusal) {                                  // (2^31 chunks: not within MAX_PAIRS pairs, every range holding one at least)
            Plan r{};
            r.refusal = TOO_LARGE;
            return r;
        }
        s.g_pairs = (unsigned)((s.pairs * PIECES + THREADS - 1) / THREADS), s.g_status = (unsigned)((s.aggs + THREADS - 1) / THREADS);
        if (s.pairs > p.max_pairs) p.max_pairs = s.pairs;
        if (s.aggs > p.max_aggs) p.max_aggs = s.aggs;
        if (s.pr.lines_bytes > p.lines_bytes) p.lines_bytes = s.pr.lines_bytes;
        if (s.pr.bad_bytes > p.bad_bytes) p.bad_bytes = s.pr.bad_bytes;
        if (s.pr.degen_bytes > p.degen_bytes) p.degen_bytes = s.pr.degen_bytes;
        if (s.pr.ws_bytes > p.pairr_bytes) p.pairr_bytes = s.pr.ws_bytes;
        p.slices.push_back(std::move(s));
    }
    ws::Layout w{256, 0};
    p.o_sum = w.take(n_grp * G1_BYTES), p.o_flag = w.take(n_grp), p.o_h = w.take(n_msgs * G2_BYTES), p.o_und = w.take(m);
    p.o_g1 = w.take(p.max_pairs * G1_BYTES), p.o_g2 = w.take(p.max_pairs * G2_BYTES), p.o_gt = w.take(p.max_aggs * GT_BYTES);
    p.o_tables = w.off;
    p.o_neg = w.take(G1_BYTES), p.o_kr = w.take(n_grp * 8);
    for (Slice& s : p.slices) s.src_off = w.take(s.pairs * SRC_BYTES), s.prtab_off = w.take(s.pr.ws_bytes - s.pr.o_tables);
    p.ws_bytes = w.off;
    return p;
}

}   // namespace verify_agg
