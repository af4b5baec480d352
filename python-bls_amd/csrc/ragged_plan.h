// ragged_plan.h -- everything about the point prefix / range sums (range_sums_run), the ragged multi-scalar sums (msm_ranges_dev),
// the short-scalar multiplications (smul64_launch) and the batched signature division (sig_divide_dev) of blsgpu_api.hip that is
// arithmetic on host integers (plain C++, no HIP: compiled for the host and compared with tests/ragged_plan_model.py by
// tests/test_ragged_plan_host.py): the shared refusals, slices, grids and the layout of every workspace.  blsgpu_api.hip grows
// the buffers to a plan's totals and launches what the plan says.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "layout.h"
#include "msm_plan.h"

namespace ragged {

using msm::Knobs;

// ---- what the plans take from blsgpu_pscan.hip and blsgpu_msmr.hip beyond msm::Consts (held to the kernels' names by a
// static_assert in blsgpu_api.hip)
struct Consts { size_t pscan_chunk, pscan_mid_threads, msmr_chunk, msmr_scan_threads; };
constexpr Consts GFX950 = {16, 128, 8, 1024};
constexpr bool same(const Consts& a, const Consts& b) {
    return a.pscan_chunk == b.pscan_chunk && a.pscan_mid_threads == b.pscan_mid_threads && a.msmr_chunk == b.msmr_chunk &&
           a.msmr_scan_threads == b.msmr_scan_threads;
}
inline unsigned blocks(size_t items, size_t threads = 256) { return (unsigned)((items + threads - 1) / threads); }
inline size_t whole(size_t items, size_t unit) { return (items + unit - 1) / unit * unit; }

// ---- the shared refusals.  "batch too large": n points (and n_ent entries) index 32-bit words with room for the + 1 records, m
// ranges run on lane pairs in G2
inline bool too_large(const msm::Consts& K, size_t n, size_t m, size_t n_ent = 0) {
    return n > 0xFFFFFFF0ull || n_ent > 0xFFFFFFF0ull || m > 0x7FFFFFF0ull / K.lp[1];
}
// the first range of a host table that is out of order or ends past the n points; NONE when every range is fine
constexpr size_t NONE = ~(size_t)0;
inline size_t first_bad_range(const uint32_t* ranges, size_t m, size_t n) {
    for (size_t i = 0; i < m; i++)
        if (ranges[2 * i] > ranges[2 * i + 1] || ranges[2 * i + 1] > n) return i;
    return NONE;
}

// ---- point prefix sums and range sums (blsgpu_pscan.hip)
constexpr size_t PSCAN_RECORD_BYTES = ((size_t)2 << 30) - ((size_t)1 << 20);    // what the prefix records of one slice may take
// one launch sequence of the scan over m points (k_lane_prep, k_pscan_totals, k_pscan_mid, k_pscan_replay): a chunk per lane
struct ScanGrids { size_t chunks; unsigned g_prep, g_chunks; };
inline ScanGrids scan_grids(const Consts& R, size_t m) {
    const size_t chunks = m ? (m + R.pscan_chunk - 1) / R.pscan_chunk : 1;
    return {chunks, blocks(m), blocks(chunks, 64)};
}
inline unsigned range_blocks(const msm::Consts& K, int DEG, size_t m) { return blocks(m * K.lp[DEG - 1], 64); }   // k_pscan_range: a range per unit
// B_PSCAN_G1 / B_PSCAN_G2 for `pts` points (bytes): the prepared points, their live and kind bytes, the chunk totals and counts,
// the pts + 1 prefix records and counts, and the carry into the next slice
struct ScanWs { size_t o_prep, o_live, o_kind, o_ct, o_cb, o_s, o_cnt, o_carry, o_cc, bytes; };
inline ScanWs scan_ws(const msm::Consts& K, const Consts& R, int DEG, size_t pts) {
    const size_t PJ = K.l28_pj * DEG, chunks = scan_grids(R, pts).chunks;
    ws::Layout l{256, 0};
    ScanWs w{};
    w.o_prep = l.take(pts * K.l28_aff * DEG * 4), w.o_live = l.take(pts), w.o_kind = l.take(pts), w.o_ct = l.take(chunks * PJ * 4),
    w.o_cb = l.take(chunks * 4), w.o_s = l.take((pts + 1) * PJ * 4), w.o_cnt = l.take((pts + 1) * 4), w.o_carry = l.take(PJ * 4), w.o_cc = l.take(4);
    w.bytes = l.off;
    return w;
}
// the range sums of m ranges over n points: slices of SL points whose records carry on from the slice before.  With more than
// one slice the record at a range's begin is kept beside the range in B_PSCAN_RANGE: the flag word | base | basec
struct ScanSlice { size_t lo, len, hi; bool first, more, last; };
struct ScanPlan {
    size_t n, SL, S;                   // S: the points the workspace holds at a time
    bool single;
    ScanWs ws;                         // scan_ws of S points
    size_t o_base, o_basec, range_bytes;
    size_t begin_total;                // words k_pscan_begin copies
    unsigned g_check, g_begin, g_range;
    ScanSlice at(size_t lo) const {    // the slice that begins at point lo (n = 0: one empty slice)
        const size_t len = n - lo < SL ? n - lo : SL;
        return {lo, len, lo + len, lo == 0, lo + len != n, lo + len == n};
    }
};
inline ScanPlan plan_scan(const Knobs& c, const msm::Consts& K, const Consts& R, int DEG, size_t n, size_t m) {
    ScanPlan p{};
    const size_t PJ = K.l28_pj * DEG;
    p.n = n, p.SL = msm::slice_len(c, PSCAN_RECORD_BYTES / (PJ * 4) - 1), p.single = n <= p.SL;
    p.S = n < p.SL ? n : p.SL, p.ws = scan_ws(K, R, DEG, p.S);
    ws::Layout l{256, 0};
    l.take(4), p.o_base = l.take(p.single ? 0 : m * PJ * 4), p.o_basec = l.off;
    p.range_bytes = p.o_basec + (p.single ? 0 : m * 4);
    p.begin_total = m * PJ;
    p.g_check = blocks(m), p.g_begin = blocks(p.begin_total), p.g_range = range_blocks(K, DEG, m);
    return p;
}

// ---- the ragged multi-scalar sums (blsgpu_msmr.hip).  The number of chunks is known after the one read-back: heads before it,
// body after.  B_MSM_PART (words, regions on 256 bytes): the head words | chunk counts | first[] (+ 1) | the chunk ranges
struct MsmrHeads { size_t h_cnt, h_first, h_cr, words; unsigned g_count; };
inline MsmrHeads plan_msmr_heads(size_t m) {
    ws::Layout l{64, 0};
    MsmrHeads p{};
    l.take(4), p.h_cnt = l.take(m), p.h_first = l.take(m + 1), p.h_cr = l.take(2 * m);
    p.words = l.off, p.g_count = blocks(m);
    return p;
}
// B_BUCKETS (words): the prepared points | live | the chunk table | the partials | the counts | their prefix sums | one slice's tables
struct MsmrSlice { size_t k, units, tab, part, bad; unsigned g_smul; };
struct MsmrBody {
    bool too_many;                     // "too many chunks"
    size_t total, slice, units0, o_prep, o_live, o_tab, o_part, o_bad, o_bpre, o_table, words;
    size_t upw, LP, DEG;
    unsigned g_fill, g_prep, g_offcurve;
    MsmrSlice at(size_t lo) const {    // the slice that begins at chunk lo
        const size_t k = total - lo < slice ? total - lo : slice, units = whole(k, upw);
        return {k, units, o_tab + 2 * lo, o_part + lo * 24 * DEG, o_bad + lo, (unsigned)(units * LP / 64)};
    }
};
inline MsmrBody plan_msmr_body(const Knobs& c, const msm::Consts& K, const Consts& R, int DEG, size_t n, size_t m, uint64_t total) {
    MsmrBody p{};
    if (total >= ((uint64_t)1 << 31)) { p.too_many = true; return p; }
    const size_t LP = K.lp[DEG - 1], upw = 64 / LP;
    p.total = (size_t)total, p.upw = upw, p.LP = LP, p.DEG = (size_t)DEG;
    p.slice = msm::unit_slice(c, K, DEG, R.msmr_chunk, K.srt_lanes / LP, upw);
    p.units0 = whole(p.total < p.slice ? p.total : p.slice, upw);
    ws::Layout l{64, 0};
    p.o_prep = l.take(n * K.l28_aff * DEG), p.o_live = l.take((n + 3) / 4), p.o_tab = l.take(2 * p.total), p.o_part = l.take(p.total * 24 * DEG),
    p.o_bad = l.take(p.total), p.o_bpre = l.take(p.total + 1), p.o_table = l.off;
    p.words = p.o_table + p.units0 * R.msmr_chunk * K.smul_t * K.pj[DEG - 1];
    p.g_fill = blocks(p.total > m ? p.total : m), p.g_prep = blocks(n), p.g_offcurve = blocks(m);
    return p;
}

// ---- short public scalars (blsgpu_smul64.hip): n weights in slices of S, each launch with tables of its own in B_SM64_WS
// (words): the prepared points | live | the tables.  `indexed`: the n_pts points are prepared once and every launch indexes them
struct Smul64Slice { size_t m, units, pts, w, out; unsigned g_prep, g_smul; };   // pts, out: words; w: bytes into the weights
struct Smul64Plan {
    size_t n, S, units0, np0, o_prep, o_live, o_tab, words;
    size_t upw, LP, DEG;
    unsigned g_prep_all;               // k_lane_prep over all n_pts points (indexed)
    Smul64Slice at(size_t lo) const {
        const size_t m = n - lo < S ? n - lo : S, units = whole(m, upw);
        return {m, units, lo * 24 * DEG, lo * 8, lo * 24 * DEG, blocks(m), (unsigned)(units * LP / 64)};
    }
};
inline Smul64Plan plan_smul64(const Knobs& c, const msm::Consts& K, int DEG, size_t n_pts, size_t n, bool indexed) {
    Smul64Plan p{};
    const size_t LP = K.lp[DEG - 1], upw = 64 / LP;
    p.n = n, p.upw = upw, p.LP = LP, p.DEG = (size_t)DEG;
    // the test cap counts items, not wavefronts of them: tests/test_gpu_slices.py puts items at the edges of slices of five
    p.S = msm::unit_slice(c, K, DEG, 1, K.srt_lanes / LP, 1);
    const size_t m0 = n < p.S ? n : p.S;
    p.units0 = whole(m0, upw), p.np0 = indexed ? n_pts : m0;
    ws::Layout l{4, 0};
    p.o_prep = l.take(p.np0 * K.l28_aff * DEG), p.o_live = l.take((p.np0 + 3) / 4), p.o_tab = l.take(p.units0 * K.smul_t * K.pj[DEG - 1]);
    p.words = l.off, p.g_prep_all = blocks(n_pts);
    return p;
}

// ---- batched Signature.divide_by (blsgpu_sigdiv.hip).  B_SIGDIV_WS (bytes): the head words | mism | zero | nonunit | status (a
// byte per point) | refused (per dividend) | the ranges | the scalars | the working copy of the points
struct SigdivPlan {
    size_t o_mism, o_zero, o_nonunit, o_status, o_refused, o_ranges, o_scalars, o_work, bytes;
    size_t memset_bytes;               // the head words, mism and zero
    unsigned g_check, g_cross, g_quot, g_fold, g_refuse;
};
inline SigdivPlan plan_sigdiv(size_t n_pts, size_t m, size_t n_ent) {
    SigdivPlan p{};
    ws::Layout l{256, 0};
    l.take(16), p.o_mism = l.take(n_pts), p.o_zero = l.take(n_pts), p.o_nonunit = l.take(n_pts), p.o_status = l.take(n_pts), p.o_refused = l.take(m),
    p.o_ranges = l.take(8 * m), p.o_scalars = l.take(32 * n_pts), p.o_work = l.take(192 * n_pts);
    p.bytes = l.off, p.memset_bytes = p.o_nonunit;
    p.g_check = blocks((m > n_pts ? m : n_pts) + 1), p.g_cross = blocks(n_ent), p.g_quot = blocks(n_pts), p.g_fold = p.g_refuse = blocks(m);
    return p;
}

}   // namespace ragged
