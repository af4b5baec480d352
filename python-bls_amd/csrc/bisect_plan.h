// bisect_plan.h -- everything about a bisecting check that is arithmetic on host integers (plain C++, no HIP: compiled for the
// host and compared with tests/bisect_model.py by tests/test_bisect_plan_host.py).  A check tests aligned NODES (offset,
// length) of a sequence of `limit` leaves, all nodes of a round of one length, from the top length ceil_pow2(limit) down; a
// node that failed is halved.  run() owns the loop; blsgpu_api.hip's bisect_rounds adds the verdict read-back, and its three
// callers lay out and launch a round.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "layout.h"

namespace bisect {

using ws::Layout;

// the top length: n rounded up to a power of two
inline size_t ceil_pow2(size_t n) { size_t K = 1; while (K < n) K <<= 1; return K; }

// a node is its offset (the verify_find forms) or a record with an `offset` that carries more (the share check: the session)
inline uint32_t offset_of(uint32_t node) { return node; }
inline uint32_t moved(uint32_t node, uint32_t by) { return node + by; }
template <class N> uint32_t offset_of(const N& node) { return node.offset; }
template <class N> N moved(N node, uint32_t by) { node.offset += by; return node; }

// The halving rule: a node of length `len` that failed (verdict byte 0) gives itself and its second half at length len / 2, in
// this order and in the order of `nodes`; a second half that begins at or past `limit` holds nothing and is dropped.
template <class N>
void halve(const std::vector<N>& nodes, const uint8_t* verdict, size_t len, size_t limit, std::vector<N>& next) {
    next.clear();
    for (size_t i = 0; i < nodes.size(); i++)
        if (!verdict[i]) {
            next.push_back(nodes[i]);
            if ((size_t)offset_of(nodes[i]) + len / 2 < limit) next.push_back(moved(nodes[i], (uint32_t)(len / 2)));
        }
}

// The rounds over `b.nodes`, from length `top` halving: `round(nodes, len, verdict)` tests the nodes -- it may reorder them first
// -- and fills one verdict byte per node, in their order (nonzero: return it); the nodes that failed are halved against `limit`,
// until the leaves or until nothing failed.  The counts run on across calls (the slices of one check).
template <class N>
struct State {
    std::vector<N> nodes, next;
    std::vector<uint8_t> verdict;
    uint64_t rounds = 0, tests = 0, pairs = 0;                               // pairs fed: counted by the rounds that have them
    // the `stats` of a check (may be NULL): rounds, node tests and, with n = 3, pairs
    void report(uint64_t* stats, int n) const {
        const uint64_t v[3] = {rounds, tests, pairs};
        if (stats) std::copy(v, v + n, stats);
    }
};
template <class N, class Round>
int run(State<N>& b, size_t top, size_t limit, Round round) {
    for (size_t len = top;; len >>= 1) {
        b.verdict.resize(b.nodes.size());
        if (int rc = round(b.nodes, len, b.verdict.data())) return rc;
        b.rounds++;
        b.tests += b.nodes.size();
        if (len == 1) return 0;
        halve(b.nodes, b.verdict.data(), len, limit, b.next);
        if (b.next.empty()) return 0;
        b.nodes.swap(b.next);
    }
}

// The plain round of verify_find: every node begins before n_e, so at most one crosses n_e.  `nodes` is reordered to the full
// nodes, in their order, then that one; part[0] are the full nodes at length L, part[1] the short one at length n_e - offset.
struct Part { size_t nodes, len; };
inline void plain_round(std::vector<uint32_t>& nodes, size_t L, uint32_t n_e, Part part[2]) {
    size_t ls = 0;
    for (size_t i = 0; i < nodes.size() && !ls; i++)
        if ((size_t)nodes[i] + L > n_e) {
            ls = n_e - nodes[i];
            std::rotate(nodes.begin() + i, nodes.begin() + i + 1, nodes.end());
        }
    part[0] = {nodes.size() - (ls ? 1 : 0), L};
    part[1] = {ls ? (size_t)1 : 0, ls};
}

// The run table of a folded slice, as the device wrote it: run r is the leaves [rb[r], rb[r + 1]) of message rmsg[r], the runs
// tile [0, n_e), and the arrays have `cap` entries
inline bool run_table_ok(uint32_t n_e, uint32_t n_runs, size_t cap, const uint32_t* rb) {
    return !(n_runs == 0 || n_runs >= cap || rb[0] != 0 || rb[n_runs] != n_e);
}

// The folded round of verify_find_folded.  A node (off, L), end = min(off + L, n_e), has one pair for its S and one per run that
// meets [off, end); every pair is a SLOT, node after node, the nodes stably ordered by their pair count (so the nodes of one
// count are one multi-pairing batch), and `nodes` is reordered to match.  `tab` is what goes to the device: first[nn + 1] (a
// node's first slot), off[nn], rng2[2 nn] (off, end: the range of S), node_of[slots], slot_msg[slots] and rng1[2 nb]: the ranges
// of the B sums, one per slot that is not a node's head -- node i's slot sl has the sum sl - i - 1 --, the run clipped to the node.
struct NodeRec { uint32_t off, r0, cnt; };                                   // a node, its first run and its pair count
struct FoldPlan {
    std::vector<NodeRec> order;
    std::vector<uint32_t> tab;
    size_t slots, nb, t_first, t_off, t_rng2, t_node, t_msg, t_rng1;         // nb = slots - nn; word offsets into tab
};
inline void fold_round(std::vector<uint32_t>& nodes, size_t L, uint32_t n_e, const uint32_t* rb, const uint32_t* rmsg, uint32_t n_runs,
                       FoldPlan& p) {
    auto end_of = [&](uint32_t o) { return (size_t)o + L < n_e ? (uint32_t)(o + L) : n_e; };
    p.order.clear();
    for (uint32_t o : nodes) {
        const uint32_t r0 = (uint32_t)(std::upper_bound(rb, rb + n_runs, o) - rb) - 1u;
        uint32_t r1 = r0;
        while (rb[r1 + 1] < end_of(o)) r1++;
        p.order.push_back({o, r0, r1 - r0 + 2u});
    }
    std::stable_sort(p.order.begin(), p.order.end(), [](const NodeRec& a, const NodeRec& b) { return a.cnt < b.cnt; });
    const size_t nn = p.order.size();
    p.slots = 0;
    for (const NodeRec& nd : p.order) p.slots += nd.cnt;
    p.nb = p.slots - nn;
    Layout t{64, 0};
    p.t_first = t.take(nn + 1), p.t_off = t.take(nn), p.t_rng2 = t.take(2 * nn), p.t_node = t.take(p.slots), p.t_msg = t.take(p.slots),
    p.t_rng1 = t.take(2 * p.nb);
    p.tab.assign(t.off, 0u);
    uint32_t* const tab = p.tab.data();
    size_t sl = 0;
    for (size_t i = 0; i < nn; i++) {
        const NodeRec& nd = p.order[i];
        const uint32_t end = end_of(nd.off);
        nodes[i] = nd.off;
        tab[p.t_first + i] = (uint32_t)sl;
        tab[p.t_off + i] = nd.off;
        tab[p.t_rng2 + 2 * i] = nd.off;
        tab[p.t_rng2 + 2 * i + 1] = end;
        for (uint32_t j = 0; j < nd.cnt; j++, sl++) {
            tab[p.t_node + sl] = (uint32_t)i;
            if (j == 0) continue;                                            // the head slot: (-G1, S)
            const uint32_t r = nd.r0 + j - 1u;
            const size_t bi = sl - i - 1;
            tab[p.t_msg + sl] = rmsg[r];
            tab[p.t_rng1 + 2 * bi] = rb[r] > nd.off ? rb[r] : nd.off;
            tab[p.t_rng1 + 2 * bi + 1] = rb[r + 1] < end ? rb[r + 1] : end;
        }
    }
    tab[p.t_first + nn] = (uint32_t)sl;
}

}   // namespace bisect
