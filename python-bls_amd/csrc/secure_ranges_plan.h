// secure_ranges_plan.h -- everything about the ragged secure aggregation (blsgpu_hash_pks_ranges*, blsgpu_aggregate_pub_keys_secure_ranges*,
// blsgpu_aggregate_sigs_secure_ranges* of blsgpu_api.hip, kernels in blsgpu_hashpks.hip) that is arithmetic on host integers
// (plain C++, no HIP: compiled for the host and compared with tests/secure_ranges_model.py by
// tests/test_secure_ranges_plan_host.py): the refusals, the offset validation of the host-buffer forms, the grids, the
// workspace and the cut of a host-buffer call into staged slices.
//
// A call holds `groups` groups.  Group g hashes the keys [pk_off[g], pk_off[g + 1]) of one list of n_keys serialised keys and
// owns the exponents [exp_off[g], exp_off[g + 1]) of one list of n_exp exponents; both tables hold groups + 1 uint32 values,
// begin at 0, never step down and end within their list.  Either range may be empty.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "layout.h"
#include "msm_plan.h"

namespace secure_ranges {

constexpr size_t CHECK_THREADS = 256;                        // k_secr_check: a group per lane
constexpr size_t DIGEST_THREADS = 64;                        // k_hash_pks_digest_ranges: a group per lane
constexpr size_t EXP_THREADS = 256;                          // k_hash_pks_exp_ranges: an exponent per lane
constexpr uint64_t MAX_ITEMS = (uint64_t)1 << 31;            // keys and exponents of a call stay below this
constexpr uint64_t MAX_GROUPS = (uint64_t)1 << 30;           // ... and its groups below this: a group is two words of the pair table, and a lane pair of the G2 sums
constexpr size_t SLICE_ITEMS = (size_t)1 << 18;              // keys, exponents (points) and groups per staged slice of the host-buffer forms: 48 MB of G2 points

// "batch too large"
inline bool too_large(uint64_t n_keys, uint64_t n_exp, uint64_t groups) {
    return n_keys >= MAX_ITEMS || n_exp >= MAX_ITEMS || groups >= MAX_GROUPS;
}

// What is refused of ONE offset table over a list of `count` items, in the order it is looked for: a first offset that is
// not 0, then group by group a step down, then a last offset past the list.  groups == 0: nothing is read.  `at` (may be
// NULL): the group, `groups` for PAST_END.  The device check (k_secr_check) refuses the same tables.
enum Verdict { OK = 0, FIRST_NOT_ZERO = 1, DECREASING = 2, PAST_END = 3 };
inline Verdict validate(const uint32_t* off, size_t groups, uint64_t count, size_t* at = nullptr) {
    size_t where = 0;
    Verdict v = OK;
    if (groups && off[0] != 0) v = FIRST_NOT_ZERO;
    for (size_t g = 0; v == OK && g < groups; g++)
        if (off[g] > off[g + 1]) v = DECREASING, where = g;
    if (v == OK && groups && off[groups] > count) v = PAST_END, where = groups;
    if (at) *at = where;
    return v;
}
inline const char* verdict_text(Verdict v) {
    switch (v) {
        case FIRST_NOT_ZERO: return "the first offset is not 0";
        case DECREASING: return "offsets decrease";
        case PAST_END: return "the last offset lies past the buffer";
        default: return "";
    }
}

// the three launches of a call: the check (and the pair table), the digests, the exponents.  The exponent kernel is launched
// over the n_exp slots of the caller's list; a lane at or past exp_off[groups] returns.
struct Grids { unsigned check, digest, exp; };
inline Grids grids(size_t groups, size_t n_exp) {
    return {(unsigned)((groups + CHECK_THREADS - 1) / CHECK_THREADS), (unsigned)((groups + DIGEST_THREADS - 1) / DIGEST_THREADS),
            (unsigned)((n_exp + EXP_THREADS - 1) / EXP_THREADS)};
}

// B_HPK_WS of a ragged call (bytes, regions on 256): the head words (word 0: the verdict of k_secr_check) | the digests, when
// they are neither the caller's input nor its output | the exponents, when they go to the sums and not to the caller | the
// (begin, end) pair table of the sums.
struct Workspace { size_t head, digests, exps, pairs, total; };
inline Workspace workspace(size_t groups, size_t n_exp, bool own_digests, bool own_exps, bool pair_table) {
    ws::Layout l{256, 0};
    Workspace w;
    w.head = l.take(16);
    w.digests = l.take(own_digests ? groups * 32 : 0);
    w.exps = l.take(own_exps ? n_exp * 32 : 0);
    w.pairs = l.take(pair_table ? groups * 8 : 0);
    w.total = l.off;
    return w;
}

// ---- the fixed-shape forms (blsgpu_hash_pks*, blsgpu_aggregate_*_secure*): every group hashes k keys and owns m exponents.  Their
// launches are grids(groups, groups * m)'s digest and exp.
// "batch too large"; groups >= 1
inline bool fixed_too_large(size_t k, size_t m, size_t groups) {
    return groups > 0x7FFFFFFFull || m > 0xFFFFFFFFull || m * groups > 0xFFFFFFF0ull || k > (~(size_t)0 >> 6) / groups;
}
// ... and on top of it for blsgpu_aggregate_priv_keys_secure*, whose keys are k_fr_dot_secret's lanes
inline bool fixed_priv_too_large(size_t k, size_t groups) { return k * groups > 0xFFFFFFF0ull; }
// B_HPK_WS of a fixed-shape call (bytes): the digests | the exponents (m == 0: the caller's buffer takes them)
struct FixedWorkspace { size_t digests, exps, total; };
inline FixedWorkspace fixed_workspace(size_t m, size_t groups) {
    ws::Layout l{256, 0};
    FixedWorkspace w;
    w.digests = l.take(groups * 32);
    l.unit = 32;
    w.exps = l.take(groups * m * 32);
    w.total = l.off;
    return w;
}

// ---- the host-buffer forms: staged slices on GROUP boundaries
// items per slice: SLICE_ITEMS, or what the test hook BLSGPU_TEST_SLICE_CAP sets
inline size_t slice_cap(const msm::Knobs& c) { return msm::slice_len(c, SLICE_ITEMS); }

// The cut of validated tables: a slice takes groups while its keys, its exponents and its groups all stay within `cap`; its
// first group is always taken, so a group longer than the cap is a slice of its own.  pk_off NULL (the caller hands in the
// digests): the keys do not count.
struct Slice { size_t lo, hi; };
inline void cut(const uint32_t* pk_off, const uint32_t* exp_off, size_t groups, size_t cap, std::vector<Slice>& out) {
    out.clear();
    for (size_t lo = 0; lo < groups;) {
        size_t hi = lo + 1;
        while (hi < groups && hi + 1 - lo <= cap && (!pk_off || (size_t)(pk_off[hi + 1] - pk_off[lo]) <= cap) &&
               (size_t)(exp_off[hi + 1] - exp_off[lo]) <= cap)
            hi++;
        out.push_back({lo, hi});
        lo = hi;
    }
}
// what the staging of a cut has to hold: the most groups, keys and exponents of a slice
struct Extent { size_t groups, keys, exps; };
inline Extent extent(const uint32_t* pk_off, const uint32_t* exp_off, const std::vector<Slice>& slices) {
    Extent e{0, 0, 0};
    for (const Slice& s : slices) {
        const size_t k = pk_off ? pk_off[s.hi] - pk_off[s.lo] : 0, x = exp_off[s.hi] - exp_off[s.lo];
        if (s.hi - s.lo > e.groups) e.groups = s.hi - s.lo;
        if (k > e.keys) e.keys = k;
        if (x > e.exps) e.exps = x;
    }
    return e;
}
// a slice's own table: off[lo .. hi] with off[lo] taken off, so that it begins at 0 like a call's
inline void rebase(const uint32_t* off, const Slice& s, std::vector<uint32_t>& out) {
    out.resize(s.hi - s.lo + 1);
    for (size_t g = s.lo; g <= s.hi; g++) out[g - s.lo] = off[g] - off[s.lo];
}

}   // namespace secure_ranges
