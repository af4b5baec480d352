// keys_plan.h -- everything about the calls that handle key material (the fixed-base G1 forms, blsgpu_hd_children*, blsgpu_hd_paths*,
// blsgpu_keys_from_seeds*, blsgpu_g1_poly_check*, the Lagrange family, blsgpu_fr_sum_secret*, blsgpu_threshold_deal_secret*,
// blsgpu_g2_mul_secret*, blsgpu_sign*, blsgpu_sign_threshold* of blsgpu_api.hip) that is arithmetic on host integers (plain C++, no
// HIP: compiled for the host and compared with tests/keys_plan_model.py by tests/test_keys_plan_host.py): the refusals, the slice
// lengths, the grids, the workspaces and what a slice of a loop adds to the caller's arrays.  blsgpu_api.hip grows the buffers to a
// plan's totals and launches what the plan says.  (The fixed-shape secure aggregation's B_HPK_WS: secure_ranges_plan.h.)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "layout.h"
#include "msm_plan.h"

namespace keys {

constexpr size_t FIX_SLICE = (size_t)1 << 22;          // items per launch of the _dev forms
constexpr size_t FIX_HOST_SLICE = (size_t)1 << 18;     // items per staged slice of the host-buffer forms (<= 76 MB of staging)
constexpr size_t SEED_SLICE = (size_t)1 << 20;         // seeds per launch of the _dev form (<= 128 MB of workspace)
constexpr size_t STAGE_TARGET = (size_t)1 << 26;       // "about 64 MB of staging" of the forms whose items have no fixed size
constexpr size_t THREADS = 256;                        // workgroup of the lane-per-item kernels
constexpr size_t G1 = 96, G2 = 192, FR = 32;           // bytes of an affine point of either group and of a scalar

// ---- what the plans take from the kernel files: blsgpu_api.hip fills a Consts from the kernels' own names; GFX950 repeats the
// values for the host test, and a static_assert there holds the two together
struct Consts {
    size_t smul_slice, smul_pairs, table_dw;           // blsgpu_g2smul.hip: SLICE, PAIRS, TABLE_DW
    size_t sum_threads, eval_threads;                  // blsgpu_frsecret.hip: SUM_THREADS, EVAL_THREADS
    size_t entry_dw, parent_dw, max_k, parent_bytes;   // g1poly::ENTRY_DW, seeds::PARENT_DW, lagr::MAX_K, BLSGPU_HD_PARENT_BYTES
};
constexpr Consts GFX950 = {65536, 128, 672, 256, 256, 28, 40, 1024, 160};
constexpr bool same(const Consts& a, const Consts& b) {
    return a.smul_slice == b.smul_slice && a.smul_pairs == b.smul_pairs && a.table_dw == b.table_dw && a.sum_threads == b.sum_threads &&
           a.eval_threads == b.eval_threads && a.entry_dw == b.entry_dw && a.parent_dw == b.parent_dw && a.max_k == b.max_k &&
           a.parent_bytes == b.parent_bytes;
}

// ---- grids
inline unsigned blocks(size_t items, size_t threads = THREADS) { return (unsigned)((items + threads - 1) / threads); }   // a lane per item
inline unsigned pack_aff_blocks(size_t m) { return blocks(m * 24); }     // k_seed_pack_aff: a lane per word of an affine key
inline unsigned spread_blocks(size_t m) { return blocks(m * 48); }       // k_g2_spread: a lane per word of a G2 point
inline unsigned smul_blocks(const Consts& K, size_t m) { return blocks(m, K.smul_pairs); }   // k_g2_smul / k_g2_smul_table: a lane pair per scalar
inline size_t eval_bpp(const Consts& K, size_t n_x) { return (n_x + K.eval_threads - 1) / K.eval_threads; }   // k_fr_poly_eval_secret: workgroups per polynomial
inline unsigned eval_blocks(const Consts& K, size_t n_polys, size_t n_x) { return (unsigned)(n_polys * eval_bpp(K, n_x)); }
// the launch shape of k_lagrange / k_fr_dot / k_fr_dot_secret for groups of k points (1 <= k <= max_k): up to 256 points a
// workgroup of 256 threads holds 256 / k whole groups, above that one group on k lanes rounded up to whole wavefronts
struct LagrShape {
    uint32_t threads, gpb;                             // gpb: groups per workgroup
    size_t lds;                                        // points / shifts, one den and one flag per group
    unsigned grid(size_t groups) const { return blocks(groups, gpb); }
};
inline LagrShape lagrange_shape(uint32_t k) {
    LagrShape s;
    s.threads = k <= 256 ? 256u : (k + 63u) / 64u * 64u;
    s.gpb = k <= 256 ? 256u / k : 1u;
    s.lds = ((size_t)s.gpb * k + s.gpb) * 32 + (size_t)s.gpb * 4;
    return s;
}
// k_fr_sum_secret: `per` lanes a group, gpb groups a workgroup
struct SumShape {
    uint32_t per, gpb;
    unsigned grid(size_t groups) const { return blocks(groups, gpb); }
};
inline SumShape sum_shape(const Consts& K, size_t k) {
    const uint32_t per = k <= K.sum_threads ? (uint32_t)k : (uint32_t)K.sum_threads;
    return {per, (uint32_t)K.sum_threads / per};
}

// ---- "batch too large" (and poly_args' "too many commitments"), each what its entry points refuse
inline bool bad_k(const Consts& K, size_t k) { return k == 0 || k > K.max_k; }                        // "k (t) must be 1 .. BLSGPU_LAGRANGE_MAX_K"
inline bool too_many_lanes(size_t n) { return n > 0xFFFFFFFFull; }                                    // hd_children_dev, seeds_args
inline bool hd_paths_too_large(size_t n, size_t n_parents) { return too_many_lanes(n) || too_many_lanes(n_parents); }
inline bool poly_too_many(size_t n_polys, size_t t) { return n_polys > 0x7FFFFFFFull / t; }            // t >= 1
inline bool lagrange_too_large(size_t k, size_t groups) { return groups > 0x7FFFFFFFull || k * groups > 0xFFFFFFF0ull; }
inline bool fr_sum_too_large(size_t k, size_t groups) { return groups > 0x7FFFFFFFull || k > (~(size_t)0 >> 6) / groups; }   // groups >= 1
inline bool deal_too_large(const Consts& K, size_t n_polys, size_t t, size_t n_x, bool frag) {
    return n_polys > 0x7FFFFFFFull || n_x > 0xFFFFFF00ull || (frag && n_polys * eval_bpp(K, n_x) > 0x7FFFFFFFull) || n_polys * t > 0xFFFFFFF0ull;
}
inline bool g2_smul_too_large(size_t n) { return n > 0xFFFFFFF0ull; }

// ---- slices
// the staged slice of a host-buffer form (and what a _dev form holds state for): min(n, slice_len(knobs, natural))
inline size_t staged_slice(const msm::Knobs& c, size_t n, size_t natural) {
    const size_t s = msm::slice_len(c, natural);
    return n < s ? n : s;
}
// the 64 MB rule of the forms whose items have no fixed size: slice_len(knobs, target / bytes per item), never zero, at most n
inline size_t staged_fit(const msm::Knobs& c, size_t n, size_t item_bytes) {
    const size_t fit = msm::slice_len(c, STAGE_TARGET / item_bytes);
    return n < fit ? n : (fit ? fit : 1);
}
// ... and what an item of each stages: a polynomial's coefficients and commitments and its fragments, a group's shares and its
// sum with both forms of its key, a seed and every output of it
constexpr size_t deal_item_bytes(size_t t, size_t n_x, bool frag) { return t * (FR + G1) + (frag ? n_x * FR : 0); }
constexpr size_t fr_sum_item_bytes(size_t k) { return k * FR + 176; }
constexpr size_t seeds_item_bytes(size_t seed_len) { return seed_len + 368; }
// items [lo, lo + m) of a loop over n items in runs of `step`
inline size_t run_len(size_t n, size_t step, size_t lo) { return n - lo < step ? n - lo : step; }

// ---- the fixed-base G1 launches (k_fix_mul, k_fix_mul_secret, k_poly_eval*): FIX_SLICE scalars each; word offsets
struct FixAt { size_t m, scalars, add, aff, ser; unsigned grid; };
inline size_t fix_step(const msm::Knobs& c) { return msm::slice_len(c, FIX_SLICE); }
inline FixAt fix_at(size_t n, size_t step, size_t lo) {
    const size_t m = run_len(n, step, lo);
    return {m, lo * 8, lo * 24, lo * 24, lo * 12, blocks(m)};
}

// ---- B_FIX_WS of blsgpu_hd_children* (bytes): the parent key | the flag of the scan | in public mode one slice of i_left
struct ChildrenAt { size_t m, idx, chain, sk, aff, ser; unsigned grid; };   // words, but aff and ser: bytes
struct ChildrenPlan {
    size_t n, step;                                    // public: the slice the workspace holds; private: FIX_SLICE, nothing held
    size_t o_parent, o_flag, o_ileft, bytes;
    ChildrenAt at(size_t lo) const {
        const size_t m = run_len(n, step, lo);
        return {m, lo, lo * 8, lo * 8, lo * G1, lo * 48, blocks(m)};
    }
};
inline ChildrenPlan plan_children(const msm::Knobs& c, size_t n, bool pub) {
    ChildrenPlan p{};
    const size_t slice = pub ? staged_slice(c, n, FIX_HOST_SLICE) : 0;
    p.n = n, p.step = pub ? slice : fix_step(c);
    ws::Layout l{128, 0};
    p.o_parent = l.take(G1), p.o_flag = l.take(4);
    l.unit = FR;
    p.o_ileft = l.take(slice * FR), p.bytes = l.off;
    return p;
}

// ---- B_HDP_WS of blsgpu_hd_paths* (bytes): the flag of the scan | per path of a slice the chain code | the key (private) or i_left
// (public) | the affine key | in public mode a second one (k_fix_mul reads the parent key while it writes the child's): 160 bytes
// a path in private mode, 256 in public
struct PathsAt { size_t m, parent_of, idx, chain, sk, aff, ser, fp; unsigned grid; };   // words, but aff and ser: bytes
struct PathsPlan {
    size_t n, depth, S;
    size_t o_flag, o_chain, o_scal, o_aff[2], bytes;
    PathsAt at(size_t lo) const {
        const size_t m = run_len(n, S, lo);
        return {m, lo, lo * depth, lo * 8, lo * 8, lo * G1, lo * 48, lo, blocks(m)};
    }
};
inline PathsPlan plan_paths(const msm::Knobs& c, size_t n, size_t depth, bool priv) {
    PathsPlan p{};
    p.n = n, p.depth = depth, p.S = staged_slice(c, n, FIX_HOST_SLICE);
    ws::Layout l{256, 0};
    p.o_flag = l.take(4);
    l.unit = FR;
    p.o_chain = l.take(p.S * FR), p.o_scal = l.take(p.S * FR), p.o_aff[0] = l.take(p.S * G1), p.o_aff[1] = l.take(priv ? 0 : p.S * G1);
    p.bytes = l.off;
    return p;
}

// ---- B_SEED_WS of blsgpu_keys_from_seeds* (bytes): one slice of the keys when out_sk is NULL | of the affine keys when the records
// are wanted without out_pk_aff
struct SeedsAt { size_t m, seeds, sk, chain, par, aff, ser; unsigned grid, g_pack; };   // words, but seeds and ser: bytes
struct SeedsPlan {
    size_t n, seed_len, parent_dw, S, o_sk, o_aff, bytes;
    SeedsAt at(size_t lo) const {
        const size_t m = run_len(n, S, lo);
        return {m, lo * seed_len, lo * 8, lo * 8, lo * parent_dw, lo * 24, lo * 48, blocks(m), pack_aff_blocks(m)};
    }
};
inline SeedsPlan plan_seeds(const msm::Knobs& c, const Consts& K, size_t seed_len, size_t n, bool out_sk, bool out_aff, bool out_parents) {
    SeedsPlan p{};
    p.n = n, p.seed_len = seed_len, p.parent_dw = K.parent_dw, p.S = staged_slice(c, n, SEED_SLICE);
    ws::Layout l{FR, 0};
    p.o_sk = l.take(out_sk ? 0 : p.S * FR), p.o_aff = l.take(out_parents && !out_aff ? p.S * G1 : 0), p.bytes = l.off;
    return p;
}

// ---- B_POLY_WS of blsgpu_g1_poly_check* (bytes): the flag of the index scan | the subgroup flags, a word per polynomial | the
// commitments in L28 form
struct PolyPlan {
    size_t m, mk;                                      // commitments; those the subgroup check reads (none when t == 1)
    size_t o_flag, o_sub, o_l28, bytes, sub_bytes;
    unsigned g_prep, g_sub;
};
inline PolyPlan plan_poly(const Consts& K, size_t n_polys, size_t t) {
    PolyPlan p{};
    p.m = n_polys * t, p.mk = n_polys * (t - 1), p.sub_bytes = n_polys * 4;
    ws::Layout l{256, 0};
    p.o_flag = l.take(4), p.o_sub = l.take(p.sub_bytes);
    l.unit = 4;
    p.o_l28 = l.take(p.m * K.entry_dw * 4), p.bytes = l.off;
    p.g_prep = blocks(p.m), p.g_sub = blocks(p.mk);
    return p;
}

// ---- B_LAGR_WS: the coefficients of `groups` groups of k points
inline size_t coeff_bytes(size_t k, size_t groups) { return groups * k * FR; }

// ---- k_g2_smul over n scalars (g2_smul_launch): smul_slice scalars a launch; word offsets, but inf: bytes
struct SmulAt { size_t m, pts, scalars, aff, ser, inf; unsigned grid; };
inline size_t smul_step(const msm::Knobs& c, const Consts& K) { return msm::slice_len(c, K.smul_slice); }
inline SmulAt smul_at(const Consts& K, size_t n, size_t step, size_t lo) {
    const size_t m = run_len(n, step, lo);
    return {m, lo * 48, lo * 8, lo * 48, lo * 24, lo, smul_blocks(K, m)};
}
// points whose tables are held at a time: one when the point is shared, else a launch's
inline size_t smul_held(const msm::Knobs& c, const Consts& K, bool shared, size_t n) { return shared ? 1 : staged_slice(c, n, K.smul_slice); }
// B_SMUL_WS of blsgpu_g2_mul_secret_dev: the tables of the held points
inline size_t smul_table_bytes(const Consts& K, size_t held) { return held * K.table_dw * 4; }

// ---- blsgpu_sign_dev.  B_SMUL_WS (bytes): H(m) of the held slice | its tables.  One message: hashed once, one table, and the outer
// loop is a single slice of n (g2_smul_launch cuts it)
struct SignAt { size_t m, msgs, hashes, sks, aff, ser; };                // bytes
struct SignPlan {
    size_t n, held, step;
    bool shared;
    size_t o_pts, o_table, bytes;
    SignAt at(size_t lo) const {
        const size_t m = run_len(n, step, lo);
        return {m, shared ? 1 : m, shared ? 0 : lo * FR, lo * FR, lo * G2, lo * 96};
    }
};
inline SignPlan plan_sign(const msm::Knobs& c, const Consts& K, size_t n_msg, size_t n) {
    SignPlan p{};
    p.n = n, p.shared = n_msg == 1, p.held = smul_held(c, K, p.shared, n), p.step = p.shared ? n : p.held;
    ws::Layout l{256, 0};
    p.o_pts = l.take(p.held * G2);
    l.unit = 4;
    p.o_table = l.take(smul_table_bytes(K, p.held)), p.bytes = l.off;
    return p;
}

// ---- blsgpu_sign_threshold_dev for `groups` sessions of k signers.  B_LAGR_WS: the coefficients.  B_FRS_WS (bytes): the scalars
// lambda_i sk_i of the call | with a message per session the point copies of the held slice.  B_SMUL_WS (bytes): H(m) per message |
// the tables of the held slice (one with ONE message)
struct ThresholdAt { size_t m, sc, aff, ser, inf; unsigned g_spread; };  // bytes
struct ThresholdPlan {
    size_t n, held;
    bool shared;
    size_t lagr_bytes, o_sc, o_rep, frs_bytes, o_hm, o_table, smul_bytes;
    unsigned g_scale;
    ThresholdAt at(size_t lo) const {
        const size_t m = run_len(n, held, lo);
        return {m, lo * FR, lo * G2, lo * 96, lo, spread_blocks(m)};
    }
};
inline ThresholdPlan plan_threshold(const msm::Knobs& c, const Consts& K, size_t k, size_t groups, size_t n_msg) {
    ThresholdPlan p{};
    p.n = k * groups, p.shared = n_msg == 1, p.held = smul_held(c, K, p.shared, p.n);
    p.lagr_bytes = coeff_bytes(k, groups), p.g_scale = blocks(p.n);
    ws::Layout f{256, 0};
    p.o_sc = f.take(p.n * FR);
    f.unit = 1;
    p.o_rep = f.take(p.shared ? 0 : p.held * G2), p.frs_bytes = f.off;
    ws::Layout s{256, 0};
    p.o_hm = s.take(n_msg * G2);
    s.unit = 4;
    p.o_table = s.take(smul_table_bytes(K, p.held)), p.smul_bytes = s.off;
    return p;
}

}   // namespace keys
