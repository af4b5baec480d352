// find_plan.h -- everything about the three forgery finders of blsgpu_api.hip -- the share check (sig_shares_dev), the batch
// verification that names the forgeries (verify_find_dev) and its form that folds shared messages (verify_find_folded_dev) --
// that is arithmetic on host integers (plain C++, no HIP: compiled for the host and compared with tests/find_plan_model.py by
// tests/test_find_plan_host.py): the refusals, the slice rule, every workspace and every round with its grids.  bisect_plan.h owns
// the loop over the rounds; blsgpu_api.hip grows each buffer to a plan's total and launches what the plan says.
//
// Each check keeps one workspace over the rounds of a slice (B_SHR_WS, B_FIND_WS) and lays out a second one afresh in every
// round (B_SHR_ROUND, B_FIND_ROUND).  Every array of either is ONE line of a region list below: its name, the unit it is counted
// in and its bytes per unit.  The offsets (regions on 256 bytes) and the bytes per item of the slice rule are both computed from
// the lists, so an array added to a list moves the offsets, the total and the slice together.
//
// THE SLICE RULE AND ITS 2 GB.  Items (sessions) go in slices so that what a slice keeps, and its largest possible round -- every
// leaf a node --, take at most BUDGET = 2 GB each.  Nothing in the kernels of blsgpu_batchfind.hip, blsgpu_sigshares.hip and
// blsgpu_pscan.hip needs that figure: every one of them forms its addresses in 64 bits (size_t piece and slot indices), their
// counts are 32-bit ITEM counts that the refusals below bound on their own, and a 2 GB array of 16-byte pieces is 2^19
// workgroups, far from any launch limit.  What the slices protect is
//   * the device memory of the context: both buffers only grow and stay for the context's life, and the round's bytes per item are
//     five times the kept ones -- unsliced, the 2^31 items the refusal admits would ask for 3.3 TB;
//   * the callees' own refusals, by a wide margin rather than by design: the hash to G2 takes at most 0x03FFFFF0 hashes, the
//     subgroup tests 0x3FFFFFF0 points, the sums and the pairing 0xFFFFFFF0 points or pairs a call, and the folded form's prefix
//     sums run as ONE slice of the scan (ragged::PSCAN_RECORD_BYTES: 6.3 M points in G2), where the natural slices here are 1.39 M
//     and 1.08 M items and at most 1.31 M sessions.
// The finders divide BUDGET - 1 MB, which pays for the rounding of every region to 256 bytes, and tests/test_find_plan_host.py
// holds both of their totals below 2 GB (less the per-call arrays of the keys and the messages, which no slice can shrink).  The
// share check divides the flat 2 GB and its round sum counts three of a node's four G1 points (SHR_ROUND_UNCOUNTED), so its round
// of leaves CAN pass 2 GB: by 5.8 % at the most (1739 bytes a leaf where the rule counts 1643, plus the rounding): 125 477 376 bytes, at k = 1.
// The rule is kept as it stands -- a slice length is behaviour --; the test asserts that overshoot as an upper bound.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bisect_plan.h"
#include "layout.h"
#include "msm_plan.h"

namespace find {

using msm::Knobs;

// ---- what the plans take from include/blsgpu.h and the three kernel files (held to their names by static_asserts in
// blsgpu_api.hip): the bytes of an affine G1 / G2 point and of a pairing result, of a sigsh::Node, the lanes of a workgroup of the
// glue kernels and the 16-byte pieces of a point
constexpr size_t G1 = 96, G2 = 192, FQ12 = 576, NODE_BYTES = 8, THREADS = 256, G1_Q = 6, G2_Q = 12;
constexpr size_t BUDGET = (size_t)2 << 30, FIND_SLACK = (size_t)1 << 20;
inline unsigned blocks(size_t items) { return (unsigned)((items + THREADS - 1) / THREADS); }

// ---- regions.  What an array is counted in; a Counts gives the number of each for one layout or one per-item sum
enum Unit {
    KEY, MSG,                          // per call: the key table, the distinct messages
    ITEM,                              // per item of a slice (share check: per share)
    DENSE, RUN,                        // folded form only: per item again, per entry of the run table
    LAM,                               // share check, scaled form only: per share
    SESSION,                           // share check: per session of a slice
    NODE,                              // per node of a round
    LEAF,                              // per leaf under the nodes of a round (plain finder: of one part)
    PAIR,                              // plain finder: per pair of a part, a node's leaves + 1
    SLOT, NB,                          // folded form: per slot (pair) of a round, per slot that is not a node's head
    TABW,                              // folded form: per word of bisect::FoldPlan::tab
    UNITS
};
struct Counts { size_t n[UNITS]; };
struct Region { const char* name; Unit unit; size_t bytes; };
// a list is a macro LIST(X) of X(name, unit, bytes) lines; from it come the offset fields of a struct, the table of regions ...
#define FIND_PLAN_FIELD(name, unit, bytes) size_t o_##name;
#define FIND_PLAN_ENTRY(name, unit, bytes) {#name, unit, bytes},
#define FIND_PLAN_TAKE(name, unit, bytes) w.o_##name = l.take(c.n[unit] * (bytes));
#define FIND_PLAN_LIST(Struct, TABLE, LIST)                                            \
    struct Struct { LIST(FIND_PLAN_FIELD) size_t bytes; };                              \
    constexpr Region TABLE[] = {LIST(FIND_PLAN_ENTRY)};                                 \
    inline void lay(Struct& w, const Counts& c, ws::Layout& l) { LIST(FIND_PLAN_TAKE) w.bytes = l.off; }
// ... and the bytes the list takes for `c` with nothing rounded: the per-item sums of the slice rule
template <size_t N>
constexpr size_t packed(const Region (&list)[N], const Counts& c) {
    size_t s = 0;
    for (size_t i = 0; i < N; i++) s += c.n[list[i].unit] * list[i].bytes;
    return s;
}
constexpr Counts counts() { return Counts{}; }
template <class... Rest>
constexpr Counts counts(Unit u, size_t n, Rest... rest) { Counts c = counts(rest...); c.n[u] = n; return c; }

// ---- the one slice rule: the items whose kept bytes and whose largest round stay within budget - slack each, at least one, under
// the knobs' test cap, and no more than there are (`count`: the finders' n, the share check's sessions)
inline size_t slice_of(const Knobs& c, size_t budget, size_t slack, size_t keep_per, size_t round_per, size_t count) {
    size_t s = (budget - slack) / (keep_per > round_per ? keep_per : round_per);
    s = msm::slice_len(c, s < 1 ? 1 : s);
    return s < count ? s : count;
}

// ======================================================================= the share check (blsgpu_sigshares.hip) ==
// B_SHR_WS, [0, 4): the flag word of the index scan (scan_indices writes, the host reads).  A slice is `slice` sessions of k shares.
#define FIND_SHR_KEEP(X)                                                                                                          \
    X(keyst, KEY, 1)      /* a key's subgroup flag: subgroup_dev writes once per call, k_share_weights reads                   */ \
    X(sigst, ITEM, 1)     /* a share's subgroup flag: subgroup_dev per slice, k_share_weights reads                            */ \
    X(h, SESSION, G2)     /* H(m) of a session: the hash to G2 per slice; k_share_weights (is it O?) and k_share_pairs read    */ \
    X(hinf, SESSION, 1)   /* H(m) = O: k_share_weights writes, k_share_pairs and k_share_verdict read                          */ \
    X(lam, LAM, 32)       /* the Lagrange coefficients (scaled form; the slice rule counts them in both): k_lagrange writes,   */ \
                          /* k_share_weights reads                                                                             */ \
    X(r, ITEM, 32)        /* the scalar r_i of A_i: k_share_weights writes, the G2 sum of the leaves reads                     */ \
    X(w, ITEM, 32)        /* the scalar r_i (lambda_i) of B_i: k_share_weights writes, the G1 sum of the leaves reads          */ \
    X(pk, ITEM, G1)       /* the share's key, copied by key_idx: k_share_weights writes, the G1 sum of the leaves reads        */ \
    X(elig, ITEM, 1)      /* the share may enter a sum: k_share_weights writes, k_share_gather reads                           */ \
    X(a, ITEM, G2)        /* the leaf A_i = r_i sig_i: msm_dev<2> writes per slice, k_share_gather reads in every round        */ \
    X(b, ITEM, G1)        /* the leaf B_i = w_i PK_i: msm_dev<1> writes per slice, k_share_gather reads in every round         */
FIND_PLAN_LIST(SharesWs, SHR_KEEP, FIND_SHR_KEEP)
// B_SHR_ROUND: a round of nn nodes of `len` leaves
#define FIND_SHR_ROUND(X)                                                                                                         \
    X(nodes, NODE, NODE_BYTES) /* (session, offset): the host uploads, the four kernels of the round read                      */ \
    X(ga, LEAF, G2)       /* the leaves A under the nodes (O where not eligible): k_share_gather writes, msm_dev<2> reads      */ \
    X(gb, LEAF, G1)       /* ... and the leaves B: k_share_gather writes, msm_dev<1> reads                                     */ \
    X(s, NODE, G2)        /* a node's sum S of its A: msm_dev<2> writes, k_share_pairs reads                                   */ \
    X(p, NODE, G1)        /* ... and P of its B: msm_dev<1> writes, k_share_pairs reads                                        */ \
    X(sinf, NODE, 1)      /* S = O: msm_dev<2> writes, k_share_pairs and k_share_verdict read                                  */ \
    X(pinf, NODE, 1)      /* P = O: msm_dev<1> writes, k_share_pairs and k_share_verdict read                                  */ \
    X(g1, NODE, 2 * G1)   /* the G1 sides of a node's two pairs: k_share_pairs writes, the pairing reads                       */ \
    X(g2, NODE, 2 * G2)   /* ... and their G2 sides                                                                            */ \
    X(e, NODE, FQ12)      /* the pairing's result: blsgpu_pairing_multi_batch_dev writes, k_share_verdict reads                */ \
    X(v, NODE, 1)         /* the verdict byte: k_share_verdict writes, the host reads it back (bisect_rounds)                  */
FIND_PLAN_LIST(SharesRoundWs, SHR_ROUND, FIND_SHR_ROUND)
// The rule as it stands counts three of the four G1 points of a node (gb, p and ONE of g1's two); see the head of the file
constexpr size_t SHR_ROUND_UNCOUNTED = G1;
constexpr size_t shares_keep_per(size_t k) { return packed(SHR_KEEP, counts(ITEM, k, LAM, k, SESSION, 1)); }
constexpr size_t shares_round_per(size_t K) { return K * (packed(SHR_ROUND, counts(NODE, 1, LEAF, 1)) - SHR_ROUND_UNCOUNTED); }   // every leaf a node
static_assert(shares_keep_per(1) == 675 && shares_round_per(1) == 1643, "the share check's slice rule changed");
static_assert(shares_keep_per(67) == 67 * 482 + 193 && shares_round_per(128) == 128 * 1643, "the share check's slice rule changed");

// "batch too large": sessions and keys are 32-bit signed counts in the kernels, shares index 32-bit words
inline bool shares_too_large(size_t k, size_t groups, size_t n_keys) {
    return groups > 0x7FFFFFFFull || n_keys > 0x7FFFFFFFull || k * groups > 0xFFFFFFF0ull;
}
struct SharesSlice { size_t n; unsigned g_weights; };                        // the shares of m sessions; k_share_weights: a share per lane
struct SharesPlan {
    size_t k, K, keep_per, round_per, slice, n0;                             // K: the top length; n0: the shares of a whole slice
    SharesWs w;
    SharesSlice at(size_t m) const { return {m * k, blocks(m * k)}; }
};
inline SharesPlan plan_shares(const Knobs& c, size_t k, size_t groups, size_t n_keys, bool scaled) {
    SharesPlan p{};
    p.k = k, p.K = bisect::ceil_pow2(k), p.keep_per = shares_keep_per(k), p.round_per = shares_round_per(p.K);
    p.slice = slice_of(c, BUDGET, 0, p.keep_per, p.round_per, groups), p.n0 = p.slice * k;
    ws::Layout l{256, 256};
    lay(p.w, counts(KEY, n_keys, ITEM, p.n0, LAM, scaled ? p.n0 : 0, SESSION, p.slice), l);
    return p;
}
// a round: gtotal / ptotal are the 16-byte pieces k_share_gather / k_share_pairs move, one per lane; k_share_verdict: a node per lane
struct SharesRound {
    size_t nn, slots, gtotal, ptotal;
    uint32_t lg;                                                             // log2 len
    unsigned g_gather, g_pairs, g_verdict;
    SharesRoundWs w;
};
inline SharesRound shares_round(size_t nn, size_t len, size_t k) {
    (void)k;                                                                 // (a node past the k shares is the kernels' business, not the layout's)
    SharesRound r{};
    r.nn = nn, r.slots = nn * len, r.lg = (uint32_t)__builtin_ctzll(len);
    r.gtotal = r.slots * (G1_Q + G2_Q), r.ptotal = nn * (2 * G1_Q + 2 * G2_Q);
    r.g_gather = blocks(r.gtotal), r.g_pairs = blocks(r.ptotal), r.g_verdict = blocks(nn);
    ws::Layout l{256, 0};
    lay(r.w, counts(NODE, nn, LEAF, r.slots), l);
    return r;
}

// ======================================================== the two finders (blsgpu_batchfind.hip, blsgpu_pscan.hip) ==
// B_FIND_WS, [0, 4): the flag word of the index scan, [4, 8): n_e (k_find_dense writes; the host, k_fold_runs and k_fold_leaves
// read), [8, 12): the number of runs (k_fold_runs writes, the host reads).  A slice is `slice` items.
#define FIND_KEEP(X)                                                                                                              \
    X(keyst, KEY, 1)      /* a key's subgroup flag: subgroup_dev writes once per call, k_find_settle reads                     */ \
    X(h, MSG, G2)         /* H(h) of a distinct message: the hash to G2 once per call; k_find_settle, k_find_pairs, k_fold_fill */ \
    X(sigst, ITEM, 1)     /* a signature's subgroup flag: subgroup_dev per slice, k_find_settle reads                          */ \
    X(r, ITEM, 8)         /* the weight, zero taken as 1: k_find_settle writes, both k_smul64 launches read                    */ \
    X(elig, ITEM, 1)      /* the item may enter a sum: k_find_settle writes, k_find_dense reads                                */ \
    X(dense, ITEM, 4)     /* the eligible items in input order: k_find_dense writes; k_find_gather, k_find_pairs, k_find_verdict, */ \
                          /* k_fold_runs and k_fold_leaves read                                                                */ \
    X(a, ITEM, G2)        /* the leaf A_i = r_i sig_i by item: k_smul64<2> writes; k_find_gather or k_fold_leaves reads        */ \
    X(b, ITEM, G1)        /* the leaf B_i = r_i P_i by item: k_smul64<1> writes; k_find_pairs or k_fold_leaves reads           */ \
    X(ad, DENSE, G2)      /* folded: the leaves A in the dense order: k_fold_leaves writes, the G2 prefix scan reads           */ \
    X(bd, DENSE, G1)      /* folded: the leaves B in the dense order: k_fold_leaves writes, the G1 prefix scan reads           */ \
    X(rb, RUN, 4)         /* folded: the first leaf of every run, and n_e after the last: k_fold_runs writes, the host reads   */ \
    X(rmsg, RUN, 4)       /* folded: the message of every run: k_fold_runs writes, the host reads                              */
FIND_PLAN_LIST(FindWs, KEEP, FIND_KEEP)
// B_FIND_ROUND of the plain finder: the head, then the two parts of bisect::plain_round (the full nodes, the one cut short)
#define FIND_PLAIN_HEAD(X)                                                                                                        \
    X(off, NODE, 4)       /* the nodes' first positions in the dense order: the host uploads, the three kernels read           */ \
    X(v, NODE, 1)         /* the verdict bytes: k_find_verdict writes, the host reads them back (bisect_rounds)                */
#define FIND_PLAIN_PART(X)                                                                                                        \
    X(ga, LEAF, G2)       /* the leaves A under the part's nodes: k_find_gather writes, msm_dev<2> reads                       */ \
    X(s, NODE, G2)        /* a node's sum S: msm_dev<2> writes, k_find_pairs reads                                             */ \
    X(sinf, NODE, 1)      /* S = O: msm_dev<2> writes, k_find_pairs and k_find_verdict read                                    */ \
    X(g1, PAIR, G1)       /* the G1 sides of a node's len + 1 pairs: k_find_pairs writes, the pairing reads                    */ \
    X(g2, PAIR, G2)       /* ... and their G2 sides                                                                            */ \
    X(e, NODE, FQ12)      /* the pairing's result: blsgpu_pairing_multi_batch_dev writes, k_find_verdict reads                 */
FIND_PLAN_LIST(PlainHeadWs, PLAIN_HEAD, FIND_PLAIN_HEAD)
FIND_PLAN_LIST(PlainPartWs, PLAIN_PART, FIND_PLAIN_PART)
// B_FIND_ROUND of the folded form: nn nodes, `slots` pairs, nb of them no node's head (bisect::fold_round)
#define FIND_FOLD_ROUND(X)                                                                                                        \
    X(tab, TABW, 4)       /* bisect::FoldPlan::tab: the host uploads; the range kernels, k_fold_codes, k_fold_fill, k_find_verdict */ \
    X(code, SLOT, 1)      /* a slot's pair is replaced by (-G1, G2): k_fold_codes writes, k_fold_fill reads                    */ \
    X(bflag, NB, 1)       /* the flag of a B sum (1: O): k_pscan_range<1> writes, k_fold_codes reads                           */ \
    X(b, NB, G1)          /* the B sum of a run inside a node: k_pscan_range<1> writes, k_fold_fill reads                      */ \
    X(sflag, NODE, 1)     /* the flag of a node's S: k_pscan_range<2> writes, k_fold_codes reads                               */ \
    X(odd, NODE, 1)       /* the node is compared with e(-G1, G2), not one: k_fold_codes writes, k_find_verdict reads          */ \
    X(v, NODE, 1)         /* the verdict bytes: k_find_verdict writes, the host reads them back (bisect_rounds)                */ \
    X(s, NODE, G2)        /* a node's sum S: k_pscan_range<2> writes, k_fold_fill reads                                        */ \
    X(g1, SLOT, G1)       /* the G1 side of every slot: k_fold_fill writes, the pairing reads                                  */ \
    X(g2, SLOT, G2)       /* ... and the G2 side                                                                               */ \
    X(e, NODE, FQ12)      /* the pairing's results: blsgpu_pairing_multi_batch_dev writes, k_find_verdict reads                */
FIND_PLAN_LIST(FoldRoundWs, FOLD_ROUND, FIND_FOLD_ROUND)
// the words of FoldPlan::tab (bisect_plan.h): first (+ 1), off and rng2 by node; node_of and slot_msg by slot, rng1 by B sum
constexpr Region FOLD_TAB[] = {{"first", NODE, 1}, {"off", NODE, 1}, {"rng2", NODE, 2}, {"node_of", SLOT, 1}, {"slot_msg", SLOT, 1}, {"rng1", NB, 2}};

// The per-item sums.  Plain: a kept item; a round in which every leaf is a node -- a node, a leaf and two pairs an item.
constexpr size_t PLAIN_KEEP_PER = packed(KEEP, counts(ITEM, 1));
constexpr size_t PLAIN_ROUND_PER = packed(PLAIN_HEAD, counts(NODE, 1)) + packed(PLAIN_PART, counts(NODE, 1, LEAF, 1, PAIR, 2));
// Folded: an entry of the run table an item (rcap <= slice + 1).  Its round is a BOUND, not a sum: a round has at most one node an
// item, and slots <= 2 nodes + runs <= 3 items, because a node has a head slot and a slot per run that meets it, and a run met by
// two nodes of a round is cut by the boundary between them: slots <= nodes + (runs + nodes - 1).  tests/test_find_plan_host.py
// sweeps it.
constexpr size_t FOLD_KEEP_PER = packed(KEEP, counts(ITEM, 1, DENSE, 1, RUN, 1));
constexpr size_t FOLD_SLOT_PER = packed(FOLD_ROUND, counts(SLOT, 1, NB, 1, TABW, packed(FOLD_TAB, counts(SLOT, 1, NB, 1))));
constexpr size_t FOLD_NODE_PER = packed(FOLD_ROUND, counts(NODE, 1, TABW, packed(FOLD_TAB, counts(NODE, 1))));
constexpr size_t FOLD_SLOTS_PER_ITEM = 3;
constexpr size_t FOLD_ROUND_PER = FOLD_SLOTS_PER_ITEM * FOLD_SLOT_PER + FOLD_NODE_PER;
static_assert(PLAIN_KEEP_PER == 302 && PLAIN_ROUND_PER == 1542, "the plain finder's slice rule changed");
static_assert(FOLD_KEEP_PER == 598 && FOLD_SLOT_PER == 402 && FOLD_ROUND_PER == 1993, "the folded finder's slice rule changed");

// "batch too large": items and keys are 32-bit counts in the kernels (the items with room for the + 1 records of the folded form);
// the distinct hashes' H(h) take BUDGET at most -- they are kept for the whole call, so no slice can bound them
inline bool find_too_large(size_t n, size_t n_keys, size_t n_msgs) {
    return n > 0x7FFFFFF0ull || n_keys > 0x7FFFFFFFull || n_msgs > BUDGET / G2;
}
// a slice of m items: k_find_settle an item per lane; folded: ltotal = the 16-byte pieces k_fold_leaves moves, rn = the entries of
// the run table the host reads back
struct FindSlice { size_t m, rn, ltotal; unsigned g_settle, g_leaves; };
struct FindPlan {
    size_t n_msgs, keep_per, round_per, slice, rcap;                         // rcap: entries of the run table (folded), else 0
    FindWs w;
    FindSlice at(size_t m) const {
        const size_t ltotal = m * (G1_Q + G2_Q);
        return {m, rcap ? (m < n_msgs ? m : n_msgs) + 1 : 0, ltotal, blocks(m), blocks(ltotal)};
    }
};
inline FindPlan plan_find(const Knobs& c, size_t n, size_t n_keys, size_t n_msgs, bool folded) {
    FindPlan p{};
    p.n_msgs = n_msgs, p.keep_per = folded ? FOLD_KEEP_PER : PLAIN_KEEP_PER, p.round_per = folded ? FOLD_ROUND_PER : PLAIN_ROUND_PER;
    p.slice = slice_of(c, BUDGET, FIND_SLACK, p.keep_per, p.round_per, n);
    p.rcap = folded ? (p.slice < n_msgs ? p.slice : n_msgs) + 1 : 0;         // a run per message and per item at most, and the end
    ws::Layout l{256, 256};
    lay(p.w, counts(KEY, n_keys, MSG, n_msgs, ITEM, p.slice, DENSE, folded ? p.slice : 0, RUN, p.rcap), l);
    return p;
}
// the plain round: per part its nodes, their first index in `off` and `v`, the pieces k_find_gather (gtotal) and k_find_pairs
// (ptotal) move, the pairs it feeds (gsz pairs a node) and the grids; a part of no nodes launches nothing
struct PlainPart {
    size_t nodes, len, first, gsz, pairs, gtotal, ptotal;
    unsigned g_gather, g_pairs, g_verdict;
    PlainPartWs w;
};
struct PlainRound { size_t nn, bytes; PlainHeadWs head; PlainPart part[2]; };
inline PlainRound plain_round(const bisect::Part shape[2]) {
    PlainRound r{};
    r.nn = shape[0].nodes + shape[1].nodes;
    ws::Layout l{256, 0};
    lay(r.head, counts(NODE, r.nn), l);
    size_t first = 0;
    for (int i = 0; i < 2; i++) {
        PlainPart& p = r.part[i];
        p.nodes = shape[i].nodes, p.len = shape[i].len, p.first = first, p.gsz = p.len + 1, p.pairs = p.nodes * p.gsz;
        p.gtotal = p.nodes * p.len * G2_Q, p.ptotal = p.pairs * (G1_Q + G2_Q);
        p.g_gather = blocks(p.gtotal), p.g_pairs = blocks(p.ptotal), p.g_verdict = blocks(p.nodes);
        lay(p.w, counts(NODE, p.nodes, LEAF, p.nodes * p.len, PAIR, p.pairs), l);
        first += p.nodes;
    }
    r.bytes = l.off;
    return r;
}
// the folded round: ftotal = the pieces k_fold_fill moves; k_fold_codes and k_find_verdict a node per lane
struct FoldRound {
    size_t nn, slots, nb, ftotal;
    unsigned g_codes, g_fill, g_verdict;
    FoldRoundWs w;
    // where the pairs of a multi-pairing batch begin (its first slot) and where its results go (its first node)
    size_t g1_at(size_t slot) const { return w.o_g1 + slot * G1; }
    size_t g2_at(size_t slot) const { return w.o_g2 + slot * G2; }
    size_t e_at(size_t node) const { return w.o_e + node * FQ12; }
};
inline FoldRound folded_round(const bisect::FoldPlan& t) {
    FoldRound r{};
    r.nn = t.order.size(), r.slots = t.slots, r.nb = t.nb, r.ftotal = t.slots * (G1_Q + G2_Q);
    r.g_codes = r.g_verdict = blocks(r.nn), r.g_fill = blocks(r.ftotal);
    ws::Layout l{256, 0};
    lay(r.w, counts(TABW, t.tab.size(), NODE, r.nn, SLOT, r.slots, NB, r.nb), l);
    return r;
}

}   // namespace find
