// pairing_plan.h -- everything about a pairing call (the Miller stage, the reduce chain and the final exponentiation in
// blsgpu_api.hip) that is arithmetic on host integers (plain C++, no HIP: compiled for the host and compared with
// tests/pairing_plan_model.py by tests/test_pairing_plan_host.py): the knobs, which kernel runs, how many partials come out per
// group, chunks and merge levels of the line-stream stage, the levels of the reduce chain, the sizes of the buffers and where a
// call is cut into slices.  blsgpu_api.hip grows the buffers to a plan's totals and launches what the plan says.
#pragma once
#include <errno.h>
#include <stddef.h>
#include <stdint.h>

namespace pairing {

// ---- the knobs of the pairing path (blsgpu_ctx derives from this; blsgpu_ctx.h's KNOBS names the environment variable of each)
struct Knobs {
    size_t miller_wide3_max = 256;     // ... with the accumulator split over two wavefronts (three per pair) up to this many pairs: three SIMDs per pair are free
    size_t miller_wide_max = 1536;     // calls of at most this many pairs run the wide Miller loop (blsgpu_mlw.hip: one pair per two-wavefront workgroup, a product per lane); 0: never
    size_t mp_threshold = 4096;        // pairs from which k_miller_mp is used
    size_t mp3_threshold = (size_t)-1; // ... with three pairs per wavefront from here on, two below; -1: the measured schedule
    bool test_ls_nomem = false;        // test hook (BLSGPU_TEST_LS_NOMEM=1): the line-stream workspace "cannot be allocated"
    // line-stream multi-pairing (blsgpu_ml.hip): used from ls_threshold pairs per call when every group has at least
    // ls_min_group pairs
    size_t ls_threshold = 2304;        // measured crossover (tools/ls_wide_sweep.py, round 5 with the point chains sixteen lanes per pair): 2048 pairs 1.70 (VM) vs 1.70 ms, 3072 pairs 1.93 vs 1.79; 5120 in round 4, 16 384 in round 3
    size_t ls_min_group = 64;
    size_t ls_teams = 163840;          // accumulators k_ml_accum aims at (10 per wavefront: 8 wavefronts per place at two per SIMD)
    bool vm_exact_lanes = true;        // degenerate blocks of the VM kernels through the lane kernels (k_ml_lines_exact / k_ml_small) instead of k_miller_slow
    bool miller_exact_lanes = true;    // blsgpu_miller_loop_batch (one exact Fq12 per pair) on the lane kernels (k_ml_lines_exact + k_ml_small, round 5) instead of the VM's k_miller_exact
    bool miller_exact_fast = true;     // ... from the FAST lines: the line-stream kernels + one Fq2 factor per pair (k_ml_exact_fixup) instead of the reference's 73 affine slopes per pair; false: k_ml_lines_exact for every pair
    size_t ls_merge_wide_max = 16384;  // merge levels with at most this many outputs run one wavefront per output
    size_t ls_wide_max = 5120;         // calls of at most this many pairs run the point chains sixteen lanes per pair with the values in LDS (k_ml_lines_wide, blsgpu_lsw.hip); 0: never
    size_t ls_quad_max = 20480;        // calls of at most this many pairs run the point chains on lane QUADS (k_ml_lines4: 0.6 of the depth while lane pairs leave SIMDs empty)
    size_t fexp_team_threshold = 5120; // results per call from which the final exponentiations run six lanes each (blsgpu_fexp.hip); below: one result per wavefront (measured crossover, tools/fexp_latency.py)
    bool fexp_wide = true;             // fewer results than that: one result per wavefront, a product per lane (blsgpu_fexpw.hip); false: the VM program
    size_t fexp_wide_max_partials = 8; // ... which also multiplies up to this many partials per result itself (a dense product is ~2.5 us)
};

// ---- what the plans take from the kernel files: blsgpu_api.hip fills a Consts from the kernels' own names; GFX950 repeats the
// values for the host test, and a static_assert there holds the two together.
struct Consts {
    size_t lines, line_dw, dense_dw, teams, slab_bytes_per_lane;           // blsgpu_ml.hip: ml::LINES, LINE_DW, DENSE_DW, TEAMS, sp::SLAB_BYTES_PER_LANE
    size_t mp_g, team_bytes, mp_team_bytes, slow_team_bytes, fexp_nslots;  // BLSVM_MP_G, TEAM_BYTES, MP_TEAM_BYTES, SLOW_TEAM_BYTES, BLS28_FEXP_NSLOTS
    size_t miller_waves, reduce_waves, reduce_per_block;                   // teams per workgroup of k_miller and of k_reduce; partials folded by one k_reduce block
    size_t batch_tree_min_group, merge_fan, slow_grid;                     // see plan_batch, plan_ls, plan_miller
};
constexpr Consts GFX950 = {68, 84, 168, 10, 224, 3, 10176, 10176, 10176, 5, 4, 8, 64, 24, 8, 3072};
constexpr bool same(const Consts& a, const Consts& b) {
    return a.lines == b.lines && a.line_dw == b.line_dw && a.dense_dw == b.dense_dw && a.teams == b.teams &&
           a.slab_bytes_per_lane == b.slab_bytes_per_lane && a.mp_g == b.mp_g && a.team_bytes == b.team_bytes &&
           a.mp_team_bytes == b.mp_team_bytes && a.slow_team_bytes == b.slow_team_bytes && a.fexp_nslots == b.fexp_nslots &&
           a.miller_waves == b.miller_waves && a.reduce_waves == b.reduce_waves && a.reduce_per_block == b.reduce_per_block &&
           a.batch_tree_min_group == b.batch_tree_min_group && a.merge_fan == b.merge_fan && a.slow_grid == b.slow_grid;
}

// ---- the three slice lengths of the pairing path (blsgpu_api.hip: slice_len of 32768, 1 << 20, 262144).  Every workspace size
// that depends on a slice length is computed from these values, so loop and buffer cannot disagree.
struct Limits {
    size_t max_groups;                 // groups ride on gridDim.y: larger batches go in slices
    size_t ls_max_pairs;               // pairs per line-stream launch sequence: 24 GB of line records at 1 << 20
    size_t exact_slice;                // pairs per slice of blsgpu_miller_loop_batch: keeps the line records below 6 GB
};

constexpr size_t cdiv(size_t a, size_t b) { return (a + b - 1) / b; }
constexpr size_t PARTIAL_BYTES = 576;  // a partial is 144 x u32 (BLSGPU_FQ12_BYTES)

// ---- what a plan refuses, with the error code and text the call returns
enum Refusal { OK, BATCH_TOO_LARGE, PARTIALS_TOO_SMALL, WORK_LIST_TOO_SMALL, TOO_MANY_GROUPS, WORKSPACE_TOO_SMALL };
inline int refusal_code(Refusal r) { return r == OK ? 0 : (r == BATCH_TOO_LARGE || r == TOO_MANY_GROUPS) ? -EINVAL : -ENOMEM; }
inline const char* refusal_text(Refusal r) {
    switch (r) {
    case BATCH_TOO_LARGE: return "batch too large";
    case PARTIALS_TOO_SMALL: return "partial buffer too small for the Miller kernel's blocks";
    case WORK_LIST_TOO_SMALL: return "work list too small";
    case TOO_MANY_GROUPS: return "too many groups";
    case WORKSPACE_TOO_SMALL: return "workspace too small; call blsgpu_ctx_reserve";
    default: return "";
    }
}

// Partials a call of `pairs` pairs takes on the wavefront-VM kernels: one per Miller block -- at most a team of two pairs
// (k_miller_mp<2>) -- plus the levels of the reduce chain.
inline size_t pairs_partials(const Consts& K, size_t pairs) { return (pairs + 1) / 2 + cdiv(pairs, K.miller_waves) + 1; }
// ... a batch of n pairs whose every launch leaves at most one partial per PAIR; m independent final exponentiations (one per
// element is written)
inline size_t batch_partials(size_t n) { return 3 * (n + 1) + 1; }
inline size_t fexp_batch_partials(size_t m) { return 3 * m + 1; }
// the product of m x groups partials of the caller's: the first level of the reduce chain leaves a partial per reduce_per_block of a group's
inline size_t product_partials(const Consts& K, size_t m, size_t groups) { return cdiv(m, K.reduce_per_block) * groups + 1; }
// the work list that goes with partial buffers of part_cap partials: one entry per Miller block at most (+ the counter)
inline size_t degen_bytes(size_t part_cap) { return (part_cap + 2) * sizeof(uint32_t); }
// workgroups of k_final_groups / k_bytes_to_partials for `groups` results
inline unsigned final_blocks(const Consts& K, size_t groups) { return (unsigned)cdiv(groups, K.reduce_waves); }

// ---- the final exponentiation of `groups` results, each the product of m partials: six lanes per result (k_fexp_team), one
// result per wavefront (k_fexp_wide: fewer results than the team form wants, the latency form), or neither (the VM's program)
enum FexpKind { FEXP_NONE, FEXP_TEAM, FEXP_WIDE };
struct FexpForm {
    FexpKind kind;
    size_t waves, ws_bytes_per_wave;   // TEAM: wavefronts asked of wave_shape; bytes of B_FEXP_WS per LAUNCHED wavefront
};
inline FexpForm fexp_form(const Knobs& c, const Consts& K, size_t m, size_t groups) {
    if (groups >= c.fexp_team_threshold && m <= 64) return {FEXP_TEAM, cdiv(groups, K.teams), (K.teams + 1) * K.fexp_nslots * K.dense_dw * 4};
    if (c.fexp_wide && groups < c.fexp_team_threshold && m >= 1 && m <= c.fexp_wide_max_partials && groups <= 0x7FFFFFFFull) return {FEXP_WIDE, 0, 0};
    return {FEXP_NONE, 0, 0};
}

// ---- Miller loops of `groups` runs of gsz pairs on the wide machine or the wavefront VM: bpg partials come out per group
// Batches of at least mp_threshold pairs use the multi-pair program (k_miller_mp: fewer instructions per pairing, longer
// per-batch latency); smaller ones the one-pair-per-wavefront program (k_miller).
inline bool use_mp(const Knobs& c, size_t n) { return n >= c.mp_threshold; }
// Two or three pairs per wavefront?  Three costs fewest instructions per pairing (large batches), two fills the
// chip sooner: 4096 teams are one "round" of the chip, so teams of two win while the batch is a little under a
// multiple of 8192 pairs and teams of three where it is a little under a multiple of 12288 -- measured crossovers
// (tools/mp_threshold_sweep.py, profiles/r02_schedule_experiments.txt); from ~20 000 pairs on blocks flow
// continuously and three wins by 8 %.
inline bool use_mp2(const Knobs& c, size_t n) {
    if (c.mp3_threshold != (size_t)-1) return n < c.mp3_threshold;
    return n <= 8704 || (n > 9728 && n <= 11264) || (n > 14336 && n <= 18432);
}
enum MillerKernel { M_WIDE3, M_WIDE2, M_MP2, M_MP3, M_VM };   // k_miller_wide<3>, <2>, k_miller_mp<2>, <BLSVM_MP_G>, k_miller
struct MillerPlan {
    MillerKernel kernel;
    size_t per_block, bpg, blocks, pairs;       // pairs per block; partials per group; bpg x groups; gsz x groups
    unsigned grid, threads;
    size_t lds;
    // The listed (degenerate) blocks once more, exactly: on the lane kernels (k_ml_lines_exact in block mode + k_ml_small in list
    // mode) when exact_lanes -- and their buffers can be had -- else k_miller_slow on slow_grid wavefronts
    size_t nv;                                  // virtual pairs: every block could be listed
    bool exact_lanes;
    size_t lines_bytes, bad_bytes;
    unsigned small_grid;
    Refusal refusal;
};
// team: 0 = choose by batch size; 2 / 3 = k_miller_mp with that many pairs per wavefront (groups of two or three pairs: one team
// per group, the group's product comes out of the Miller kernel).  own_partials: the partials go to the context's own buffers,
// of part_cap partials; degen_cap: entries of the work list.
inline MillerPlan plan_miller(const Knobs& c, const Consts& K, size_t gsz, size_t groups, bool one_per_block, int team, bool own_partials,
                              size_t part_cap, size_t degen_cap) {
    MillerPlan p{};
    const size_t n = p.pairs = gsz * groups;
    // a few pairs: one pair per two-wavefront workgroup with a product per lane (blsgpu_mlw.hip), every pair its own partial
    // (where the one-pair-per-wavefront k_miller ran: calls below the throughput kernels' threshold)
    const bool wide = !team && n <= c.miller_wide_max && !use_mp(c, n);
    const bool mp = team ? true : (!wide && !one_per_block && use_mp(c, n));
    const bool mp2 = team ? team == 2 : (mp && use_mp2(c, n));   // a few thousand pairs: teams of two fill the chip
    p.per_block = (one_per_block || wide) ? 1 : (mp ? (mp2 ? (size_t)2 : K.mp_g) : K.miller_waves);
    p.bpg = cdiv(gsz, p.per_block);
    p.blocks = p.bpg * groups;
    p.kernel = wide ? (n <= c.miller_wide3_max ? M_WIDE3 : M_WIDE2) : mp2 ? M_MP2 : mp ? M_MP3 : M_VM;
    p.refusal = p.blocks > 0x7FFFFFFFull ? BATCH_TOO_LARGE : (own_partials && p.blocks > part_cap) ? PARTIALS_TOO_SMALL
              : p.blocks + 2 > degen_cap ? WORK_LIST_TOO_SMALL : OK;
    if (p.refusal) return p;
    switch (p.kernel) {
    case M_WIDE3: p.grid = (unsigned)p.blocks, p.threads = 192, p.lds = 0; break;
    case M_WIDE2: p.grid = (unsigned)((p.blocks + 1) / 2), p.threads = 256, p.lds = 0; break;
    case M_MP2: case M_MP3: p.grid = (unsigned)p.blocks, p.threads = 64, p.lds = K.mp_team_bytes; break;
    case M_VM: p.grid = (unsigned)p.blocks, p.threads = (unsigned)p.per_block * 64, p.lds = p.per_block * K.team_bytes; break;
    }
    p.nv = p.blocks * p.per_block;
    p.exact_lanes = c.vm_exact_lanes && p.nv <= ((size_t)1 << 16);
    if (p.exact_lanes) p.lines_bytes = p.nv * K.lines * K.line_dw * 4, p.bad_bytes = p.nv, p.small_grid = (unsigned)cdiv(p.blocks, K.teams);
    return p;
}

// ---- the line-stream form of the Miller stage (blsgpu_ml.hip): ONE partial per group comes out.  Asked for from ls_threshold
// pairs per call.
inline bool use_ls(const Knobs& c, size_t gsz, size_t groups) {
    return gsz >= 1 && gsz * groups >= c.ls_threshold && gsz * groups <= 0x3FFFFFF0ull;
}
enum ChainKernel { L_WIDE16, L_QUAD, L_PAIR };               // k_ml_lines_wide, k_ml_lines4, k_ml_lines2
struct Merge {                         // a merge level: runs of merge_fan partial products per output, from lsp(src) to lsp(dst)
    size_t cpg, cpo, teams, waves;     // chunks per group before and after; outputs; wavefronts of k_ml_merge
    bool wide;                         // few outputs: k_ml_merge_wide, one wavefront each (grid = teams)
    int src, dst;
};
constexpr int MAX_MERGES = 12;         // (2^26 chunks merge to one in nine levels)
struct LsPlan {
    size_t n, chunk, cpg;
    bool small;                        // one accumulator per group runs the whole loop (k_ml_small)
    size_t lines_bytes, lsp0_bytes, lsp1_bytes, bad_bytes, degen_bytes;
    ChainKernel chain;
    unsigned chain_grid;               // L_WIDE16
    size_t chain_waves;                // L_QUAD, L_PAIR (wave_shape; dynamic LDS = threads x slab_bytes_per_lane)
    size_t small_waves;                // k_ml_small
    size_t accum_teams, accum_waves;   // k_ml_accum
    int nmerges;
    Merge merge[MAX_MERGES];
    int last;                          // the lsp buffer k_ml_horner_fexp reads
    bool fuse;                         // ... which goes on to the final exponentiation of each group's product in place
};
// gsz >= 1.  one_per_group: one accumulator per group whatever ls_min_group says (blsgpu_miller_loop_batch_dev: a group is a
// pair).  want_fused: the caller wants nothing but the final exponentiation of each group's product.
inline LsPlan plan_ls(const Knobs& c, const Consts& K, size_t gsz, size_t groups, bool one_per_group, bool want_fused) {
    LsPlan p{};
    const size_t n = p.n = gsz * groups;
    // chunks: equal runs of a group's pairs, one accumulator each per line index, sized so that about ls_teams
    // accumulators exist (a wavefront of ten then runs a few hundred products: many short wavefronts per SIMD, so the
    // last round of the launch costs little) but never fewer than 16 pairs (the merge is a dense product per chunk)
    // ... and fewer, longer chunks for mid-size calls (at least 128 pairs each while 40 960 accumulators -- two wavefronts per
    // SIMD -- remain): the merge tree over the chunks is latency, 65 536 pairs 7.05 -> 6.8 ms (tools/c3_probe.py)
    size_t aim = n * K.lines / 128;
    if (aim < 40960) aim = 40960;
    if (aim > c.ls_teams) aim = c.ls_teams;
    size_t want = cdiv(n * K.lines, aim);
    if (want < 16) want = 16;
    if (want > gsz) want = gsz;
    size_t cpg = cdiv(gsz, want);
    p.chunk = cdiv(gsz, cpg);
    p.cpg = cpg = cdiv(gsz, p.chunk);
    p.small = one_per_group || gsz < c.ls_min_group;
    p.lines_bytes = n * K.lines * K.line_dw * 4, p.bad_bytes = n, p.degen_bytes = (n + 2) * 4;
    if (!p.small) {
        p.lsp0_bytes = groups * cpg * K.lines * K.dense_dw * 4;
        p.lsp1_bytes = groups * cdiv(cpg, K.merge_fan) * K.lines * K.dense_dw * 4;
    }
    // a few thousand pairs: sixteen lanes each, the values in LDS, a product per lane; few pairs: four lanes each, the tangent
    // step's levels shared by the two pairs
    p.chain = n <= c.ls_wide_max ? L_WIDE16 : n <= c.ls_quad_max ? L_QUAD : L_PAIR;
    p.chain_grid = (unsigned)cdiv(n, 16);
    p.chain_waves = p.chain == L_QUAD ? (4 * n + 63) / 64 : (2 * n + 63) / 64;
    p.small_waves = cdiv(groups, K.teams);
    if (p.small) return p;
    p.accum_teams = groups * cpg * K.lines, p.accum_waves = cdiv(p.accum_teams, K.teams);
    int cur = 0;
    while (cpg > 1) {
        const size_t cpo = cdiv(cpg, K.merge_fan), teams = groups * cpo * K.lines;
        p.merge[p.nmerges++] = {cpg, cpo, teams, cdiv(teams, K.teams), teams <= c.ls_merge_wide_max, cur, cur ^ 1};
        cpg = cpo;
        cur ^= 1;
    }
    p.last = cur;
    p.fuse = want_fused && fexp_form(c, K, 1, groups).kind == FEXP_WIDE;
    return p;
}

// ---- the reduce chain: for each of `groups` groups fold its m partials down to one, reduce_per_block per k_reduce block and
// level.  It ends in the register final exponentiation as soon as few enough partials per group are left (R_REG: reads m
// partials per group with the strides below), after the level that leaves one partial per group (R_HAND_OVER: one more launch,
// but the VM's final exponentiation inside k_reduce is 1.25 ms of one wavefront), or inside the last k_reduce (R_REDUCE: its
// final flag, or one partial per group to the caller).
enum ReduceBuf { RB_IN, RB_PART0, RB_PART1, RB_OUT };        // the caller's input, the context's two buffers, the caller's partial output
enum ReduceEnd { R_REG, R_HAND_OVER, R_REDUCE };
struct ReduceLevel {
    size_t blocks, m, istride, gstride;
    ReduceBuf dst;
    bool final_flag;
    int timer;                         // KernelTimer kind: 1 k_reduce, 2 with the final exponentiation
};
constexpr int MAX_REDUCE_LEVELS = 8;   // (2^32 partials fold to one in six)
struct ReducePlan {
    Refusal refusal;
    int nlevels;
    ReduceLevel level[MAX_REDUCE_LEVELS];
    ReduceEnd end;
    FexpForm fexp;                     // R_REG, R_HAND_OVER: the form, reading fm partials per group from fsrc
    ReduceBuf fsrc;
    size_t fm, fistride, fgstride;
    size_t lds;
};
// from_part0: the input is the context's first partial buffer (the levels then begin with the second)
inline ReducePlan plan_reduce(const Knobs& c, const Consts& K, size_t m, size_t groups, size_t istride, size_t gstride, bool do_final,
                              bool from_part0, size_t part_cap) {
    ReducePlan p{};
    p.lds = K.reduce_waves * K.team_bytes;
    if (groups > 65535) { p.refusal = TOO_MANY_GROUPS; return p; }
    ReduceBuf src = from_part0 ? RB_PART0 : RB_IN;
    int pp = from_part0 ? 1 : 0;
    while (true) {
        if (do_final && fexp_form(c, K, m, groups).kind != FEXP_NONE) {
            p.end = R_REG, p.fexp = fexp_form(c, K, m, groups), p.fsrc = src, p.fm = m, p.fistride = istride, p.fgstride = gstride;
            return p;
        }
        size_t blocks = cdiv(m, K.reduce_per_block);
        if (blocks == 0) blocks = 1;
        const bool last = blocks == 1;
        const bool hand_over = last && do_final && fexp_form(c, K, 1, groups).kind != FEXP_NONE && groups <= part_cap;
        const ReduceBuf dst = (last && !hand_over) ? RB_OUT : pp ? RB_PART1 : RB_PART0;
        if (!last && blocks * groups > part_cap) { p.refusal = WORKSPACE_TOO_SMALL; return p; }
        const bool fin = last && do_final && !hand_over;
        p.level[p.nlevels++] = {blocks, m, istride, gstride, dst, fin, fin ? 2 : 1};
        if (hand_over) {
            p.end = R_HAND_OVER, p.fexp = fexp_form(c, K, 1, groups), p.fsrc = dst, p.fm = p.fistride = p.fgstride = 1;
            return p;
        }
        if (last) break;
        src = dst, m = blocks, istride = 1, gstride = blocks, pp ^= 1;
    }
    p.end = R_REDUCE;
    return p;
}

// ---- Miller loops + per-group product (grouped_pairing): final exponentiation iff want_bytes, one partial per group to the
// caller iff want_partial
enum LsMode {
    LS_OFF,                            // the wide machine / the wavefront VM (plan_miller)
    LS_WHOLE,                          // one line-stream launch sequence
    LS_GROUP_SLICES,                   // slices of `per` whole groups
    LS_RUN_SLICES,                     // ONE long group: `runs` runs of its pairs, each leaves a partial for the product
    LS_VM_LONG_GROUPS                  // several groups longer than a slice: the VM kernels
};
struct GroupedPlan {
    size_t outer;                      // more than max_groups groups: the call goes in slices of this many groups, each planned on its own; else 0
    size_t partials;                   // to ensure in each partial buffer
    LsMode ls;
    size_t per, runs, run_len;
    bool direct;                       // LS_WHOLE: the stage writes straight into the caller's partial buffer (no copying pass of k_reduce behind it)
    size_t ls_bpg, vm_bpg;             // partials per group the reduce chain gets after the line-stream stage / after plan_miller's kernels
};
inline GroupedPlan plan_grouped(const Knobs& c, const Consts& K, const Limits& L, size_t gsz, size_t groups, bool want_bytes, bool want_partial) {
    GroupedPlan p{};
    if (groups > L.max_groups) { p.outer = L.max_groups; return p; }
    // every group rounds its team count up; the wide Miller loop leaves one partial per pair
    const size_t partials = pairs_partials(K, (gsz + 3) * groups);
    p.vm_bpg = gsz ? plan_miller(c, K, gsz, groups, false, 0, false, 0, (size_t)-1).bpg : 0;
    const size_t vm_blocks = p.vm_bpg * groups;
    p.partials = partials > vm_blocks ? partials : vm_blocks;
    if (!use_ls(c, gsz, groups)) return p;
    // The line records are 22.8 KB per pair: a call is cut into slices of at most ls_max_pairs pairs -- whole groups,
    // or, for ONE long group, runs of its pairs that each leave a partial for the product.
    p.ls_bpg = 1;
    if (gsz * groups <= L.ls_max_pairs) p.ls = LS_WHOLE, p.direct = want_partial && !want_bytes;
    else if (gsz <= L.ls_max_pairs) p.ls = LS_GROUP_SLICES, p.per = L.ls_max_pairs / gsz;
    else if (groups == 1) p.ls = LS_RUN_SLICES, p.run_len = L.ls_max_pairs, p.ls_bpg = p.runs = cdiv(gsz, L.ls_max_pairs);
    else p.ls = LS_VM_LONG_GROUPS, p.ls_bpg = 0;
    return p;
}

// ---- `groups` independent multi-pairings of gsz pairs each (blsgpu_pairing_multi_batch_dev)
enum BatchRoute {
    B_TREE,                            // groups of at least batch_tree_min_group pairs: plan_grouped's per-group product tree
    B_LS_SMALL,                        // a large batch of small groups: point chains, then one accumulator per group (plan_ls)
    B_TEAM_GROUPS,                     // groups of two or three pairs in a batch large enough for the team kernels: the group IS the team, one partial per group
    B_ONE_PER_BLOCK                    // one partial per pair
};
struct BatchFinal { size_t m, istride, gstride; FexpForm fexp; unsigned blocks; };   // what the final stage reads; fexp NONE: k_final_groups on `blocks` workgroups
struct BatchPlan {
    BatchRoute route, fallback;        // fallback: the route when B_LS_SMALL finds no memory for its line records
    size_t partials, n;
    BatchFinal fin, fallback_fin;
};
inline BatchFinal batch_final(const Knobs& c, const Consts& K, BatchRoute r, size_t gsz, size_t groups) {
    const size_t m = r == B_ONE_PER_BLOCK ? gsz : 1;
    return {m, 1, m, fexp_form(c, K, m, groups), final_blocks(K, groups)};
}
inline BatchPlan plan_batch(const Knobs& c, const Consts& K, const Limits& L, size_t gsz, size_t groups) {
    BatchPlan p{};
    const size_t n = p.n = gsz * groups;
    if (gsz >= K.batch_tree_min_group) { p.route = p.fallback = B_TREE; return p; }
    p.partials = batch_partials(n);
    p.fallback = ((gsz == 2 || gsz == K.mp_g) && use_mp(c, n) && groups <= 0x7FFFFFFFull) ? B_TEAM_GROUPS : B_ONE_PER_BLOCK;
    p.route = (use_ls(c, gsz, groups) && n <= L.ls_max_pairs) ? B_LS_SMALL : p.fallback;
    p.fin = batch_final(c, K, p.route, gsz, groups), p.fallback_fin = batch_final(c, K, p.fallback, gsz, groups);
    return p;
}

// ---- one exact Miller value per pair (blsgpu_miller_loop_batch_dev) in slices of L.exact_slice pairs: the fast form (line-stream
// kernels with one accumulator per pair + k_ml_exact_fixup), the lane form (k_ml_lines_exact for every pair + k_ml_small), the VM
struct ExactSlice { size_t m; unsigned g_flags, g_fixup, g_list, g_bytes; size_t small_waves; };   // grids of k_ml_exact_flags, k_ml_exact_fixup, k_ml_list_all, k_ml_partials_to_bytes; wavefronts of k_ml_small
struct ExactPlan {
    size_t n, slice, m0;
    size_t partials;                   // both forms
    size_t exflags_bytes;              // fast form (the line-stream buffers are plan_ls(1, m, one_per_group)'s)
    size_t lines_bytes, bad_bytes, degen_bytes;   // lane form
    unsigned vm_grid;
    ExactSlice at(size_t lo) const {
        const size_t m = n - lo < slice ? n - lo : slice;
        return {m, (unsigned)cdiv(m, 256), (unsigned)cdiv(2 * m, 256), (unsigned)cdiv(m, 256), (unsigned)cdiv(m * 12, 256), cdiv(m, teams)};
    }
    size_t teams;
};
inline ExactPlan plan_exact(const Consts& K, const Limits& L, size_t n) {
    ExactPlan p{};
    p.n = n, p.slice = L.exact_slice, p.teams = K.teams;
    const size_t m0 = p.m0 = n < p.slice ? n : p.slice;
    p.partials = m0 + (m0 + 1) / 2 + 1;
    p.exflags_bytes = 2 * m0;
    p.lines_bytes = m0 * K.lines * K.line_dw * 4, p.bad_bytes = m0, p.degen_bytes = (m0 + 2) * 4;
    p.vm_grid = (unsigned)(n < 16384 ? n : 16384);
    return p;
}

// ---- blsgpu_ctx_reserve(max_pairs): the partials of a call of that size on the VM kernels and, from ls_threshold pairs, the
// line-stream stage's buffers as well (a call of that size takes them): line records of one slice, the flags and the work list,
// and dense partial products for the usual chunking (ls_teams accumulators plus `lines` per group of at least ls_min_group
// pairs); a call that needs more grows them itself (plan_ls)
struct ReservePlan {
    size_t partials;
    bool ls;
    size_t lines_bytes, bad_bytes, degen_bytes, lsp0_bytes, lsp1_bytes;
};
inline ReservePlan plan_reserve(const Knobs& c, const Consts& K, const Limits& L, size_t max_pairs) {
    ReservePlan p{};
    p.partials = pairs_partials(K, max_pairs);
    p.ls = max_pairs >= c.ls_threshold;
    if (!p.ls) return p;
    const size_t n = max_pairs < L.ls_max_pairs ? max_pairs : L.ls_max_pairs;
    const size_t teams = c.ls_teams + K.lines * (n / (c.ls_min_group ? c.ls_min_group : 1) + 1);
    p.lines_bytes = n * K.lines * K.line_dw * 4, p.bad_bytes = n, p.degen_bytes = (n + 2) * 4;
    p.lsp0_bytes = teams * K.dense_dw * 4, p.lsp1_bytes = (teams / 8 + K.lines) * K.dense_dw * 4;
    return p;
}

// ---- where slice [lo, ...) of a call's arrays begins, in bytes: `lo` counts pairs for the points and the flags (two flag bytes
// per pair), `res` results for the partials (576 bytes each, also the size of a final result)
struct SliceOffsets { size_t g1, g2, inf, res; };
inline SliceOffsets slice_offsets(size_t lo_pairs, size_t lo_results) { return {lo_pairs * 96, lo_pairs * 192, lo_pairs * 2, lo_results * PARTIAL_BYTES}; }

}   // namespace pairing
