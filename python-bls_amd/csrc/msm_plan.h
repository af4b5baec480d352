// msm_plan.h -- everything about a G1 / G2 sum (msm_dev in blsgpu_api.hip) that is arithmetic on host integers (plain C++, no HIP:
// compiled for the host and compared with tests/msm_plan_model.py by tests/test_msm_plan_host.py): the knobs, which kernel family
// serves a call (next_route), and one plan per family -- window bits, chunk lengths, fold levels, grid sizes and the layout of the
// two workspace buffers the sums share.  blsgpu_api.hip grows the buffers to a plan's totals and launches what the plan says.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "layout.h"

namespace msm {

// ---- the knobs of the sums (blsgpu_ctx derives from this; blsgpu_ctx.h's KNOBS names the environment variable of each)
struct Knobs {
    size_t pip_threshold = 4096;       // points from which a single sum uses the bucket method
    size_t pip_group_threshold = 48;   // points per sum from which a batch of sums does
    size_t pip_chunks = 0;             // chunks one large bucket-method sum is cut into (BLSGPU_PIP_CHUNKS); 0: 256, or 3072 on the lane path
    size_t msm_sort_threshold = 1;     // points from which one G1 sum with scalars uses sorted buckets (k_srt_*): since the tail runs on the wide machine (round 5) they win at every size -- 1 point 1.24 ms against 1.63, 8192 points 1.45 against 2.59 (profiles/r05_c5_window_bits.txt)
    size_t msm_sort2_threshold = 1;    // the same for ONE G2 sum with scalars (round 5: BLS.aggregate_sigs(secure) as a multi-scalar sum)
    size_t sort_bits = 0;              // window bits of the sorted-bucket G1 sum (BLSGPU_MSM_SORT_BITS); 0: the measured schedule (plan_sorted)
    size_t sort2_bits = 0;             // ... of the G2 sum (BLSGPU_MSM_SORT2_BITS); 0: msm_sort2_bits(n)
    static uint32_t msm_sort2_bits(size_t n) { return n >= 16384 ? 13 : (n >= 512 ? 11 : 9); }   // window bits of the G2 path by size (tools/g2_single_sum_probe.py, profiles/r05_g2_single_sum.txt)
    size_t msm_plain_threshold = 2;    // points from which ONE plain sum (no scalars) runs on the register kernels (k_sum_chunks + folds; round 5) instead of the wavefront VM's k_msm
    size_t smul_min_groups = 4096;     // sums per call from which a batch of SMALL sums with scalars (scalar multiplications: groups x 1 point) runs one group per lane / lane pair (k_smul, round 5) instead of the wavefront VM's k_msm
    size_t smul_max_k = 8;             // ... for sums of up to this many points
    bool msm_wide_tail = true;         // the sorted-bucket G1 sum: window sums and the Horner over the windows on the wide machine (blsgpu_msmw.hip k_msm_horner_wide<1, .>: 0.9 ms against the wavefront VM's 1.45); false: k_srt_windows + k_msm_pip_horner<1>
    size_t msm_lane_threshold = 65536; // points from which the bucket sums run one (group, chunk, window) per lane
    bool msm_lane_pairs = true;        // G2: every (group, chunk, window) on a lane PAIR (k_msm_lane2x) instead of one lane
    size_t horner_np_threshold = 1024; // G2 sums per call from which the window Horner runs several sums per team
    size_t horner_quads_threshold = 2; // G2 sums per call (lane-pair bucket kernel) from which the window Horner runs one sum per lane quad
    size_t test_slice_cap = 0;         // test hook (BLSGPU_TEST_SLICE_CAP=items): the host loops cut their work into slices of at most this many items (slice_len), so a test crosses every slice boundary with a few items; 0: the natural slice lengths
};

// The slice length of a host loop: `natural` -- unless the test hook caps it (test_slice_cap), then at most the cap rounded up to a
// whole number of `unit`s and never less than one unit.  Every workspace size that follows from a slice length is derived from
// this value, so loop and buffer cannot disagree.
inline size_t slice_len(const Knobs& c, size_t natural, size_t unit = 1) {
    if (!c.test_slice_cap) return natural;
    const size_t cap = (c.test_slice_cap + unit - 1) / unit * unit;
    const size_t s = natural < cap ? natural : cap;
    return s < unit ? unit : s;
}

// ---- what the plans take from the kernel files: blsgpu_api.hip fills a Consts from the kernels' own names; GFX950 repeats the
// values for the host test, and a static_assert there holds the two together.  The arrays are indexed by DEG - 1.
struct Consts {
    size_t srt_lanes, srt_scw, srt_bitadds, srt_maxbits, srt_slice;        // blsgpu_msm.hip: SRT_*
    size_t smul_t, pip_w, pip_nb, l28_aff, l28_pj;                         // SMUL_T, PIP_W, PIP_NB, L28_AFF, L28_PJ
    size_t msm_waves, hmsm2_np;                                            // wavefronts per workgroup of k_msm / k_msm_prep / k_msm_finish; BLSVM_HMSM2_NP
    size_t np[2], lp[2], aff[2], pj[2];                                    // MsmCfg<DEG>::NP, SrtG<DEG>::{LP, AFF, PJ}
};
constexpr Consts GFX950 = {2048 * 64, 9, 8, 14, 65536, 16, 64, 16, 28, 42, 4, 5, {6, 2}, {1, 2}, {42, 84}, {42, 84}};
constexpr bool same(const size_t (&a)[2], const size_t (&b)[2]) { return a[0] == b[0] && a[1] == b[1]; }
constexpr bool same(const Consts& a, const Consts& b) {
    return a.srt_lanes == b.srt_lanes && a.srt_scw == b.srt_scw && a.srt_bitadds == b.srt_bitadds && a.srt_maxbits == b.srt_maxbits &&
           a.srt_slice == b.srt_slice && a.smul_t == b.smul_t && a.pip_w == b.pip_w && a.pip_nb == b.pip_nb && a.l28_aff == b.l28_aff &&
           a.l28_pj == b.l28_pj && a.msm_waves == b.msm_waves && a.hmsm2_np == b.hmsm2_np && same(a.np, b.np) && same(a.lp, b.lp) &&
           same(a.aff, b.aff) && same(a.pj, b.pj);
}

// ---- the kernel families, in the order msm_dev asks them.  SMALL_GROUPS says "not me" when its tables find no room, SORTED when
// its key list does not fit 32 bits (SortedPlan::not_me); the router then asks for the next route.
enum Route { START = -1, EMPTY, PLAIN, SMALL_GROUPS, SORTED, BUCKET_VM, BUCKET_LANE, VM, END };

// the refusal "msm too large" (an empty sum has no size to refuse)
inline bool too_large(size_t k, size_t groups) {
    return k && (k > 0x7FFFFFFFull || groups > 0x7FFFFFFFull || k * groups > 0xFFFFFFF0ull);
}

inline bool serves(const Knobs& c, int DEG, size_t k, size_t groups, bool has_scalars, Route r) {
    if (k == 0) return r == EMPTY;                  // empty sums: infinity
    // bucket method: one large sum is cut into about 256 chunks; a batch of sums uses one chunk per group
    const bool bucket = (groups == 1 && k >= c.pip_threshold) || (groups > 1 && groups <= 65535 && k >= c.pip_group_threshold);
    // enough points for one (group, chunk, window) per lane to fill the chip?  (3 waves per SIMD = 3072 chunks)
    const bool lane_path = k * groups >= c.msm_lane_threshold;
    switch (r) {
    case PLAIN: return groups == 1 && !has_scalars && k >= c.msm_plain_threshold;
    case SMALL_GROUPS: return has_scalars && groups >= c.smul_min_groups && k <= c.smul_max_k;
    case SORTED: return groups == 1 && has_scalars && k >= (DEG == 1 ? c.msm_sort_threshold : c.msm_sort2_threshold);
    case BUCKET_VM: return bucket && !lane_path;
    case BUCKET_LANE: return bucket && lane_path;
    case VM: return true;
    default: return false;
    }
}
// the first route after `after` that serves the call (START: the first of all); END after VM
inline Route next_route(const Knobs& c, int DEG, size_t k, size_t groups, bool has_scalars, Route after) {
    for (int r = after + 1; r < END; r++)
        if (serves(c, DEG, k, groups, has_scalars, (Route)r)) return (Route)r;
    return END;
}

// ---- fold levels: runs of 8 partial sums per unit, from the array at word `src` to the one at `dst` (the two buffers alternate)
enum FoldKernel { F_HORNER_WIDE, F_SRT_FOLD, F_LANE_FOLD };              // k_msm_horner_wide<DEG, 0>, k_srt_fold<DEG>, k_msm_lane_fold<1>
struct Fold {
    FoldKernel kernel;
    size_t cur, nfold, ftotal;         // partial sums per (window, bit) before and after; runs of the level
    uint32_t npts, last;               // F_HORNER_WIDE: points per run; F_LANE_FOLD: 1 on the last fold (the VM's form for the VM's tail)
    unsigned grid;
    size_t src, dst;
};
constexpr int MAX_FOLDS = 8;           // (131 072 units fold to 8 in five levels)
inline unsigned unit_blocks(size_t nunits, size_t LP) { return (unsigned)((nunits * LP + 63) / 64); }   // 64-lane workgroups for nunits units of LP lanes

// ---- one sum with scalars by sorted buckets (blsgpu_msm.hip, k_srt_*; G1 a unit per lane, G2 per lane pair)
struct SortedPlan {
    bool bad_bits, not_me;             // "BLSGPU_MSM_SORT_BITS out of range"; the key list would not fit 32 bits: the fixed-window path
    uint32_t cb, kb, nwin;
    size_t nkeys, nch, nsum, units, btotal;
    bool wide, pass5;                  // pass5: 5-bit windows on the VM's tail -- nothing to fold, but the VM's tail reads its own form
    uint32_t bias[9];                  // SrtBias (SRT_SCW words)
    // workspace: prep | recoded scalars | cnt | start (+1) | cursor | maxcnt, total | idx | bsum | headpart | headkey | bit sums (two buffers) | winsums
    size_t o_prep, o_rec, o_cnt, o_start, o_cur, o_max, o_idx, o_bsum, o_hp, o_hk, o_b0, o_b1, o_win, o_live, o_wtot, o_long, words;
    int nfolds;
    Fold fold[MAX_FOLDS];
    size_t src;                        // where the tail reads the (window, bit) sums
    unsigned g_prep, g_slices, g_accum, g_fix, g_bits, g_pass5;
};
inline SortedPlan plan_sorted(const Knobs& c, const Consts& K, int DEG, size_t n) {
    SortedPlan p{};
    const size_t LP = K.lp[DEG - 1], PJ = K.pj[DEG - 1];
    // Window bits: with 131 072 equal pieces a run covers 131072 / (keys per window x windows) pieces whatever n is, and a run of
    // more than three pieces costs a whole wavefront in k_srt_fix_long.  With signed digits (2^(cb-1) keys per window) 13 bits are
    // the best width at every size the sorted path serves (tools/c5_probe.py under BLSGPU_MSM_SORT_BITS, profiles/r05_c5_window_bits.txt:
    // 2^20 points 5.71 / 5.42 / 5.46 ms for 12 / 13 / 14 bits, 16 384 points 1.88 / 1.52 / 1.68).
    const size_t pinned = DEG == 1 ? c.sort_bits : c.sort2_bits;
    if (pinned && (pinned < 5 || pinned > K.srt_maxbits)) { p.bad_bits = true; return p; }
    const uint32_t cb = pinned ? (uint32_t)pinned : DEG == 1 ? (n < 512 ? 7u : 13u) : c.msm_sort2_bits(n);   // (a few points: 37 windows of 64 keys, 1.06 ms for one point against 1.24)
    // signed digits (blsgpu_msm.hip): 2^(cb-1) keys per window; 258 <= cb x windows keeps the recoded scalar inside the windows
    const uint32_t kb = cb - 1, nwin = (258 + cb - 1) / cb;
    p.cb = cb, p.kb = kb, p.nwin = nwin;
    const size_t nkeys = p.nkeys = (size_t)nwin << kb;
    if ((size_t)nwin * n > 0xFFFFFFF0ull || n >= 0x80000000ull) { p.not_me = true; return p; }
    const size_t nch = p.nch = ((size_t)1 << (cb - 2)) / K.srt_bitadds, nsum = p.nsum = (size_t)nwin * cb;
    const size_t units = p.units = K.srt_lanes / LP;
    p.wide = DEG == 2 || c.msm_wide_tail;                     // (G2 has no tail on the wavefront VM)
    ws::Layout l{4, 0};
    p.o_prep = l.take(n * K.aff[DEG - 1]), p.o_rec = l.take(n * K.srt_scw), p.o_cnt = l.take(nkeys), p.o_start = l.take(nkeys + 1),
    p.o_cur = l.take(nkeys), p.o_max = l.take(4), p.o_idx = l.take((size_t)nwin * n), p.o_bsum = l.take(nkeys * PJ), p.o_hp = l.take(units * PJ),
    p.o_hk = l.take(units), p.o_b0 = l.take(nsum * nch * PJ), p.o_b1 = l.take(nsum * ((nch + 7) / 8) * PJ + PJ), p.o_win = l.take((size_t)nwin * PJ),
    p.o_live = l.take((n + 3) / 4), p.o_wtot = l.take(2 * (size_t)nwin), p.o_long = l.take(nkeys + 4);
    p.words = l.off;
    for (uint32_t w = 0; w < nwin; w++) {
        const uint32_t pos = cb * w + cb - 1;
        p.bias[pos >> 5] |= 1u << (pos & 31);
    }
    p.g_prep = (unsigned)((n + 255) / 256), p.g_slices = (unsigned)((n + K.srt_slice - 1) / K.srt_slice);
    p.g_accum = unit_blocks(units, LP), p.g_fix = unit_blocks(nkeys, LP);
    p.btotal = nsum * nch, p.g_bits = unit_blocks(p.btotal, LP);
    size_t src = p.o_b0, dst = p.o_b1;
    if (nch == 1 && !p.wide) {
        p.pass5 = true, p.g_pass5 = (unsigned)((nsum + 63) / 64);
        src = dst;
    }
    for (size_t cur = nch; cur > 1;) {                        // runs of 8 partial sums per unit until one is left per (window, bit)
        const size_t nfold = (cur + 7) / 8, ftotal = nsum * nfold;
        Fold& f = p.fold[p.nfolds++];
        f = {F_LANE_FOLD, cur, nfold, ftotal, (uint32_t)(cur < 8 ? cur : 8), nfold == 1 ? 1u : 0u, (unsigned)((ftotal + 63) / 64), src, dst};
        if (p.wide && ftotal <= 4096 && (cur <= 8 || cur % 8 == 0))
            // few runs left: one wavefront per run, an addition two steps of the wide machine (a lane's own addition is ~6000 instructions)
            f.kernel = F_HORNER_WIDE, f.grid = (unsigned)ftotal;
        else if (p.wide)
            f.kernel = F_SRT_FOLD, f.grid = unit_blocks(ftotal, LP);
        const size_t t = src; src = dst; dst = t;
        cur = nfold;
    }
    p.src = src;
    return p;
}

// ---- one plain sum of n points (no scalars): a chunk of the list per unit (k_sum_chunks), then runs of eight partial sums until
// eight are left (k_srt_fold, or one wavefront per run on the wide machine once at most 4096 runs are left), then the last run
struct PlainPlan {
    size_t U, chunk, o_prep, o_live, o_b0, o_b1, words;
    int nfolds;
    Fold fold[MAX_FOLDS];
    size_t src;
    uint32_t last_n;                   // partial sums the last Horner takes
    unsigned g_prep, g_chunks;
};
inline PlainPlan plan_plain(const Consts& K, int DEG, size_t n) {
    PlainPlan p{};
    const size_t LP = K.lp[DEG - 1], PJ = K.pj[DEG - 1], units_max = K.srt_lanes / LP;
    size_t U = (n + 3) / 4;                                   // four points per unit while units are free (a small sum is a latency)
    if (U > units_max) U = units_max;
    p.chunk = (n + U - 1) / U;
    p.U = U = (n + p.chunk - 1) / p.chunk;
    ws::Layout l{4, 0};
    p.o_prep = l.take(n * K.l28_aff * DEG), p.o_live = l.take((n + 3) / 4), p.o_b0 = l.take(U * PJ), p.o_b1 = l.take(((U + 7) / 8) * PJ + PJ);
    p.words = l.off;
    p.g_prep = (unsigned)((n + 255) / 256), p.g_chunks = unit_blocks(U, LP);
    size_t src = p.o_b0, dst = p.o_b1, cur = U;
    while (cur > 8) {
        const size_t nfold = (cur + 7) / 8;
        Fold& f = p.fold[p.nfolds++];
        f = {F_SRT_FOLD, cur, nfold, nfold, 8u, 0u, unit_blocks(nfold, LP), src, dst};
        if (nfold <= 4096 && cur % 8 == 0) f.kernel = F_HORNER_WIDE, f.grid = (unsigned)nfold;
        const size_t t = src; src = dst; dst = t;
        cur = nfold;
    }
    p.src = src, p.last_n = (uint32_t)cur;
    return p;
}

// ---- a batch of scalar multiplications / of small sums with scalars: one group per unit (k_smul), in slices of groups whose
// tables (16 projective multiples per point) stay below 2 GB: 2^20 groups of eight G2 points would ask for 45 GB
// The slice rule of the kernels that run one item per unit on a table of SMUL_T projective multiples per point (k_smul here,
// k_smul_seg and k_smul64 in ragged_plan.h): whole wavefronts of units whose tables stay below 2 GB, at least one wavefront.
// `ceiling`: units one launch may take (0: none -- k_smul's grid is not bound to SRT_LANES); `cap_unit`: what the test cap is
// rounded up to (a wavefront of units, or 1 where the cap counts single items).
inline size_t unit_slice(const Knobs& c, const Consts& K, int DEG, size_t pts_per_unit, size_t ceiling, size_t cap_unit) {
    const size_t upw = 64 / K.lp[DEG - 1], per_unit = pts_per_unit * K.smul_t * K.pj[DEG - 1] * 4;
    size_t slice = ((size_t)2 << 30) / per_unit / upw * upw;
    if (slice < upw) slice = upw;
    if (ceiling && slice > ceiling) slice = ceiling;
    return slice_len(c, slice, cap_unit);
}
struct SmallSlice { size_t m, n, units, pts, scalars, out; unsigned g_prep, g_smul; };   // pts, scalars, out: words into the caller's arrays
struct SmallPlan {
    size_t upw, slice, units0, o_prep, o_live, o_tab, words;
    size_t k, groups, LP, DEG;
    SmallSlice at(size_t lo) const {                          // the slice that begins at group lo
        const size_t m = groups - lo < slice ? groups - lo : slice, n = k * m, units = (m + upw - 1) / upw * upw;
        return {m, n, units, lo * k * 24 * DEG, lo * k * 8, lo * 24 * DEG, (unsigned)((n + 255) / 256), (unsigned)(units * LP / 64)};
    }
};
inline SmallPlan plan_small_groups(const Knobs& c, const Consts& K, int DEG, size_t k, size_t groups) {
    SmallPlan p{};
    const size_t LP = K.lp[DEG - 1], PJ = K.pj[DEG - 1];
    const size_t upw = p.upw = 64 / LP;
    size_t slice = unit_slice(c, K, DEG, k, 0, upw);
    if (slice > groups) slice = groups;                       // (the ragged plans keep their slice and clamp the units instead)
    p.slice = slice, p.k = k, p.groups = groups, p.LP = LP, p.DEG = (size_t)DEG;
    p.units0 = (slice + upw - 1) / upw * upw;
    const size_t n0 = k * slice;
    ws::Layout l{4, 0};
    p.o_prep = l.take(n0 * K.l28_aff * DEG), p.o_live = l.take((n0 + 3) / 4), p.o_tab = l.take(p.units0 * k * K.smul_t * PJ);
    p.words = l.off;
    return p;
}

// ---- the bucket method, buckets in LDS (BUCKET_VM: k_msm_pip) or one (group, chunk, window) per lane with buckets in HBM
// (BUCKET_LANE: k_msm_lane / k_msm_lane2x, then k_msm_lane_fold when a sum has more than 96 chunks)
enum Tail { T_HORNER_QUADS, T_HORNER_NP, T_PIP_HORNER };
struct BucketPlan {
    bool lane_path;
    size_t n, chunk, chunks, fold_n;
    // B_MSM_PART: partials -- the VM's form (36 DEG dwords) except between the lane kernel and its fold (L28: 42 DEG) -- | window
    // sums | prep: the VM's projective triples (36 DEG) or the lane path's affine L28 points (28 DEG) + live flags (o_live)
    size_t part_words, o_win, o_prep, o_live;
    // B_BUCKETS (lane path): buckets | the folded partials
    size_t bucket_words, o_fold;
    size_t lanes, ftotal, wchunks;     // ftotal: runs of the fold; wchunks: partials per window that k_msm_pip_windows reads
    bool pairs;                        // k_msm_lane2x (G2 on lane pairs), not k_msm_lane<DEG>
    uint32_t lane_last;                // its last argument: 1 when it writes the VM's form itself (no fold, no quad Horner)
    Tail tail;
    unsigned g_prep, g_lane, g_fold, g_np;
    size_t quad_waves;                 // wavefronts of k_msm_horner_quads (wave_shape)
};
inline BucketPlan plan_bucket(const Knobs& c, const Consts& K, int DEG, size_t k, size_t groups) {
    BucketPlan p{};
    const size_t NP = K.np[DEG - 1], PJ28 = K.l28_pj * DEG, W = K.pip_w;
    const size_t n = p.n = k * groups;
    const bool lane_path = p.lane_path = n >= c.msm_lane_threshold;
    const size_t want = c.pip_chunks ? c.pip_chunks : (lane_path ? 3072 : 256);
    size_t chunk = (groups > 1) ? k : (k + want - 1) / want;
    if (!lane_path && chunk < 64 * NP && groups == 1) chunk = 64 * NP;
    if (!lane_path) chunk = ((chunk + NP - 1) / NP) * NP;
    if (chunk == 0) chunk = 1;
    const size_t chunks = p.chunks = (k + chunk - 1) / chunk;
    p.chunk = chunk;
    p.fold_n = (lane_path && chunks > 96) ? (chunks + 63) / 64 : 0;
    ws::Layout part{1, 0};
    part.take(chunks * groups * W * PJ28), p.o_win = part.take(groups * W * PJ28), p.o_prep = part.take(n * 36 * DEG + (n + 3) / 4 + 4);
    p.part_words = part.off, p.o_live = p.o_prep + n * K.l28_aff * DEG;
    p.wchunks = chunks;
    bool horner_quads = false;
    if (lane_path) {
        p.lanes = groups * chunks * W;
        ws::Layout b{1, 0};
        b.take(p.lanes * (K.pip_nb - 1) * PJ28), p.o_fold = b.take(p.fold_n * groups * W * 36 * DEG);
        p.bucket_words = b.off;
        // a batch of G2 sums (one chunk each): the window sums stay in the L28 form and the Horner runs one sum per lane quad
        horner_quads = DEG == 2 && c.msm_lane_pairs && chunks == 1 && groups >= c.horner_quads_threshold;
        p.pairs = DEG == 2 && c.msm_lane_pairs;
        p.lane_last = p.pairs ? ((p.fold_n || horner_quads) ? 0u : 1u) : (p.fold_n ? 0u : 1u);
        p.g_prep = (unsigned)((n + 255) / 256), p.g_lane = (unsigned)(((p.pairs ? 2 : 1) * p.lanes + 63) / 64);
        if (p.fold_n) {                                       // many chunks: fold runs of 64 partials per lane first
            p.ftotal = groups * W * p.fold_n, p.g_fold = (unsigned)((p.ftotal + 63) / 64);
            p.wchunks = p.fold_n;
        }
        p.quad_waves = (4 * groups + 63) / 64;
    } else {
        p.g_prep = (unsigned)((n + K.msm_waves * NP - 1) / (K.msm_waves * NP));
    }
    // (a batch of G2 sums: BLSVM_HMSM2_NP sums per team)
    p.tail = horner_quads ? T_HORNER_QUADS : (DEG == 2 && groups >= c.horner_np_threshold) ? T_HORNER_NP : T_PIP_HORNER;
    p.g_np = (unsigned)((groups + K.hmsm2_np - 1) / K.hmsm2_np);
    return p;
}

// ---- double-and-add on the wavefront VM (k_msm + k_msm_finish).  Points per block: whole group when small, else chunks that give
// >= ~2k blocks
struct VmPlan { size_t chunk, bpg, blocks, words, fblocks; };
inline VmPlan plan_vm(const Consts& K, int DEG, size_t k, size_t groups) {
    VmPlan p{};
    const size_t per_pass = K.msm_waves * K.np[DEG - 1];
    p.chunk = k;
    if (groups < 1024 && k > 4 * per_pass) {
        const size_t want_blocks = 2048 / groups + 1;
        p.chunk = (k + want_blocks - 1) / want_blocks;
        p.chunk = ((p.chunk + per_pass - 1) / per_pass) * per_pass;
        if (p.chunk > k) p.chunk = k;
    }
    p.bpg = (k + p.chunk - 1) / p.chunk;
    p.blocks = p.bpg * groups;
    ws::Layout l{1, 0};
    l.take(p.blocks * 36 * DEG);
    p.words = l.off;
    p.fblocks = (groups + K.msm_waves - 1) / K.msm_waves;
    return p;
}

}   // namespace msm
