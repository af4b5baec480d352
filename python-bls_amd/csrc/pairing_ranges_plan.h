// pairing_ranges_plan.h -- the whole schedule of blsgpu_pairing_multi_ranges* (blsgpu_api.hip, kernels in blsgpu_mlr.hip) as
// arithmetic on host integers (plain C++, no HIP: compiled for the host and compared with tests/pairing_ranges_model.py by
// tests/test_pairing_ranges_plan_host.py).  From (n, ranges, m, knobs, limits): the validation of the ranges, the slices of the
// pair list, the chunks of every range, each slice's chunk table, the fold levels, the sizes of the buffers and the grids.
// Nothing is read back from the device: the range table is the caller's HOST memory in both forms of the call.
//
//   slices   the pair list is cut at multiples of Limits::ls_max_pairs (line records cost 22.8 KB per pair; the test hook
//            BLSGPU_TEST_SLICE_CAP shortens it): slice s holds the pairs [s S, min(n, (s + 1) S)).  A slice runs the point chains
//            over ALL its pairs when a chunk with pairs lies in it, and nothing when none does.
//   chunks   range j = [b, e) is cut into chunks of at most C = pair_ranges_chunk consecutive pairs that never cross a slice
//            boundary; an empty range is one chunk of length 0 (its accumulator stays one).  One six-lane team of k_ml_ranges runs
//            the Miller loop of one chunk and leaves one partial.
//   slots    one array of partials.  Slot j < m is range j's product.  A range of ONE chunk writes slot j straight from
//            k_ml_ranges; a range of k > 1 chunks owns k consecutive slots behind the first m, in the order of its pairs
//            (whichever slices they lie in), and every fold level gives it cdiv(k, merge_fan) new consecutive slots -- or slot j
//            when that is one.
//   folds    level l is a table of (first source slot, count, destination slot), 1 <= count <= merge_fan, one team of
//            k_ml_fold_ranges each; levels go on until every range with more than one chunk has reached its slot j.
#pragma once
#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "layout.h"
#include "pairing_plan.h"

namespace pairing_ranges {

// ---- the knob of the ragged multi-pairing (blsgpu_ctx derives from this; blsgpu_ctx.h's KNOBS names BLSGPU_PAIR_RANGES_CHUNK)
struct Knobs {
    size_t pair_ranges_chunk = 16;     // C: pairs per chunk at most.  NOT MEASURED: the value is plan_ls's rule "never fewer than 16 pairs: the merge is a dense product per chunk"; tools/pair_ranges_probe.py runs 8, 16, 32 and 64
};

constexpr size_t MAX_PAIRS = 0x3FFFFFF0ull;                  // as blsgpu_pairing_multi_batch
constexpr uint64_t MAX_CHUNKS = (uint64_t)1 << 31;           // 2^31 chunks or more are refused
constexpr size_t ENTRY_BYTES = 12;                           // a chunk or a fold entry: three uint32

enum Refusal { OK, TOO_MANY_PAIRS, BAD_RANGE, TOO_MANY_CHUNKS };
inline int refusal_code(Refusal r) { return r == OK ? 0 : -EINVAL; }
inline const char* refusal_text(Refusal r) {
    switch (r) {
    case TOO_MANY_PAIRS: return "batch too large";
    case BAD_RANGE: return "a range with begin > end or end > n";
    case TOO_MANY_CHUNKS: return "2^31 chunks or more";
    default: return "";
    }
}

struct Chunk { uint32_t first, len, dest; };                 // first pair within the slice, pairs, destination slot
struct Fold { uint32_t src, count, dest; };                  // first source slot, partials, destination slot
struct Slice {
    size_t lo, pairs;                  // the pairs [lo, lo + pairs) of the list
    size_t chunk0, nchunks;            // its rows of Plan::chunks
    bool chains;                       // a chunk with pairs lies in it: the point chains run (ls), else k_ml_ranges alone -- or nothing (nchunks == 0)
    size_t waves;                      // wavefronts of k_ml_ranges: `teams` chunks each
    size_t tab_off;                    // its chunk table in the workspace
    pairing::LsPlan ls;                // chains: the chain kernel and its grid, the bytes of line records, flags and work list
};
struct Level { size_t fold0, nfolds, waves, tab_off; };      // rows of Plan::folds; wavefronts of k_ml_fold_ranges; its table in the workspace

struct Plan {
    Refusal refusal;
    size_t bad_range;                  // BAD_RANGE: the first such range
    size_t n, m, chunk, slice_pairs;   // C and S as used
    uint64_t nchunks;
    size_t slots;                      // partials in all: m + the slots of the folds
    std::vector<Slice> slices;
    std::vector<Chunk> chunks;         // slice after slice
    std::vector<Level> levels;
    std::vector<Fold> folds;           // level after level
    size_t lines_bytes, bad_bytes, degen_bytes;              // the largest of the slices': grown once, before the first launch
    size_t o_partials, o_tables, ws_bytes;                   // the workspace: the partials, then every table ([o_tables, ws_bytes) is ONE upload)
    size_t final_step;                 // results per launch of the final exponentiation
    // the image of [o_tables, ws_bytes): dst holds ws_bytes - o_tables bytes
    void fill_tables(void* dst) const {
        char* d = (char*)dst;
        memset(d, 0, ws_bytes - o_tables);
        for (const Slice& s : slices)
            if (s.nchunks) memcpy(d + (s.tab_off - o_tables), chunks.data() + s.chunk0, s.nchunks * ENTRY_BYTES);
        for (const Level& l : levels) memcpy(d + (l.tab_off - o_tables), folds.data() + l.fold0, l.nfolds * ENTRY_BYTES);
    }
};
static_assert(sizeof(Chunk) == ENTRY_BYTES && sizeof(Fold) == ENTRY_BYTES, "the tables are uploaded as they are");

// chunks of the non-empty range [b, e): per slice touched, its pairs in runs of C
inline uint64_t chunks_of(size_t b, size_t e, size_t C, size_t S) {
    const size_t s0 = b / S, s1 = (e - 1) / S;
    if (s0 == s1) return pairing::cdiv(e - b, C);
    return (uint64_t)pairing::cdiv((s0 + 1) * S - b, C) + (uint64_t)(s1 - s0 - 1) * pairing::cdiv(S, C) + pairing::cdiv(e - s1 * S, C);
}

// ranges: m x 2 uint32 (begin, end).  A refused plan holds no table.
inline Plan plan(size_t n, const uint32_t* ranges, size_t m, const Knobs& k, const pairing::Knobs& pk, const pairing::Consts& K,
                 const pairing::Limits& L) {
    Plan p{};
    const size_t C = p.chunk = k.pair_ranges_chunk ? k.pair_ranges_chunk : 1;
    const size_t S = p.slice_pairs = L.ls_max_pairs ? L.ls_max_pairs : 1;
    p.n = n, p.m = m, p.final_step = L.max_groups ? L.max_groups : 1;
    if (n > MAX_PAIRS) { p.refusal = TOO_MANY_PAIRS; return p; }
    for (size_t j = 0; j < m; j++) {
        const size_t b = ranges[2 * j], e = ranges[2 * j + 1];
        if (b > e || e > n) { p.refusal = BAD_RANGE, p.bad_range = j; return p; }
        p.nchunks += b == e ? 1 : chunks_of(b, e, C, S);
        if (p.nchunks >= MAX_CHUNKS) { p.refusal = TOO_MANY_CHUNKS; return p; }
    }
    // the slices and how many chunks each takes
    const size_t ns = n ? pairing::cdiv(n, S) : 1;
    p.slices.resize(ns);
    for (size_t s = 0; s < ns; s++) p.slices[s].lo = s * S, p.slices[s].pairs = n - s * S < S ? n - s * S : S;
    auto slice_of_empty = [&](size_t b) { return b / S < ns ? b / S : ns - 1; };
    for (size_t j = 0; j < m; j++) {
        const size_t b = ranges[2 * j], e = ranges[2 * j + 1];
        if (b == e) { p.slices[slice_of_empty(b)].nchunks++; continue; }
        for (size_t s = b / S; s <= (e - 1) / S; s++) {
            const size_t lo = b > s * S ? b : s * S, hi = e < (s + 1) * S ? e : (s + 1) * S;
            p.slices[s].nchunks += pairing::cdiv(hi - lo, C);
            p.slices[s].chains = true;
        }
    }
    std::vector<size_t> cur(ns);
    size_t at = 0;
    for (size_t s = 0; s < ns; s++) p.slices[s].chunk0 = cur[s] = at, at += p.slices[s].nchunks;
    p.chunks.resize(at);
    // the chunks, and the ranges that fold: (range, first slot, slots)
    struct Run { size_t j, base, k; };
    std::vector<Run> runs, next;
    size_t slots = m;
    for (size_t j = 0; j < m; j++) {
        const size_t b = ranges[2 * j], e = ranges[2 * j + 1];
        if (b == e) { p.chunks[cur[slice_of_empty(b)]++] = {0u, 0u, (uint32_t)j}; continue; }
        const size_t kj = (size_t)chunks_of(b, e, C, S), base = kj == 1 ? j : slots;
        if (kj > 1) runs.push_back({j, base, kj}), slots += kj;
        size_t i = 0;
        for (size_t q = b; q < e; i++) {
            const size_t s = q / S;
            size_t hi = q + C < e ? q + C : e;
            if (hi > (s + 1) * S) hi = (s + 1) * S;
            p.chunks[cur[s]++] = {(uint32_t)(q - s * S), (uint32_t)(hi - q), (uint32_t)(kj == 1 ? j : base + i)};
            q = hi;
        }
    }
    // the fold levels
    const size_t fan = K.merge_fan;
    while (!runs.empty()) {
        Level lv{p.folds.size(), 0, 0, 0};
        next.clear();
        for (const Run& r : runs) {
            const size_t ko = pairing::cdiv(r.k, fan), nb = ko == 1 ? r.j : slots;
            if (ko > 1) next.push_back({r.j, nb, ko}), slots += ko;
            for (size_t i = 0; i < ko; i++) {
                const size_t left = r.k - i * fan;
                p.folds.push_back({(uint32_t)(r.base + i * fan), (uint32_t)(left < fan ? left : fan), (uint32_t)(ko == 1 ? r.j : nb + i)});
            }
        }
        lv.nfolds = p.folds.size() - lv.fold0, lv.waves = pairing::cdiv(lv.nfolds, K.teams);
        p.levels.push_back(lv);
        runs.swap(next);
    }
    p.slots = slots;
    // sizes, grids and the layout of the workspace
    ws::Layout w{256, 0};
    p.o_partials = w.take(slots * pairing::PARTIAL_BYTES);
    p.o_tables = w.off;
    for (Slice& s : p.slices) {
        s.waves = pairing::cdiv(s.nchunks, K.teams);
        if (s.nchunks) s.tab_off = w.take(s.nchunks * ENTRY_BYTES);
        if (!s.chains) continue;
        s.ls = pairing::plan_ls(pk, K, 1, s.pairs, true, false);
        if (s.ls.lines_bytes > p.lines_bytes) p.lines_bytes = s.ls.lines_bytes;
        if (s.ls.bad_bytes > p.bad_bytes) p.bad_bytes = s.ls.bad_bytes;
        if (s.ls.degen_bytes > p.degen_bytes) p.degen_bytes = s.ls.degen_bytes;
    }
    for (Level& l : p.levels) l.tab_off = w.take(l.nfolds * ENTRY_BYTES);
    p.ws_bytes = w.off;
    return p;
}

}   // namespace pairing_ranges
