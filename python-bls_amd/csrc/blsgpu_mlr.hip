// blsgpu_mlr.hip -- the accumulate and fold stages of the RAGGED multi-pairing (blsgpu_pairing_multi_ranges*): ranges of any
// lengths over one list of pairs in one launch sequence.  The point chains (k_ml_lines2 / k_ml_lines4 / k_ml_lines_wide, then
// k_ml_lines_exact) leave line records and `bad` flags per PAIR, whatever range a pair belongs to; only the stages here know
// about ranges, and they read them from tables the host wrote (csrc/pairing_ranges_plan.h is the whole schedule).
//
// Both kernels are k_ml_small's shape: six lanes per accumulator, ten teams per wavefront, the production routines of namespace
// ml.  Those routines exchange operands across the lanes of a team (ds_bpermute), so every lane of a wavefront runs every one
// of them the same number of times:
//   * the trip count of a loop whose bound differs per team is WAVE-UNIFORM -- `__any(i < len)`, the largest bound among the
//     wavefront's teams;
//   * a team past its own bound computes and discards (select), its loads clamped to addresses inside the buffers;
//   * no lane leaves before the last exchange unless its whole wavefront does.
#pragma once

namespace blsgpu {
namespace ml {

// One chunk per team: tab[3 id ..] = (first pair within the slice, length, destination slot).  The team runs the loop
// f <- f^2 prod_i l_{i,L} over its pairs [first, first + len) for the 68 line indices and stores f in the VM word format at
// partials[dest * 144].  lines / bad: one slice's records and flags, n pairs (every chunk lies inside: first + len <= n); a
// launch whose chunks are all empty (n may be 0) reads neither.
__global__ void __launch_bounds__(256, 2) k_ml_ranges(const int32_t* __restrict__ lines, const uint8_t* __restrict__ bad, uint32_t n,
                                                     const uint32_t* __restrict__ tab, uint32_t nchunks, uint32_t* __restrict__ partials)
#if BLSGPU_EMIT(BLSGPU_TU_MLR)
{
    const Team t = team_of_lane();
    if (wave_index() * TEAMS >= nchunks) return;              // the whole wavefront
    const uint32_t id = wave_index() * TEAMS + t.slot;
    const bool valid = t.slot < (uint32_t)TEAMS && id < nchunks;
    const uint32_t idc = valid ? id : wave_index() * TEAMS;   // (a row of the table either way)
    const uint32_t first = tab[3 * (size_t)idc], len = valid ? tab[3 * (size_t)idc + 1] : 0u, dest = tab[3 * (size_t)idc + 2];
    const uint32_t last = n ? n - 1u : 0u;
    int32_t fre[NL], fim[NL];
    set_one(fre, fim, t);
#pragma unroll 1
    for (uint32_t L = 0; L < (uint32_t)LINES; L++) {
        if (L > 0 && line_is_tangent(L)) {
            int32_t cre[NL], cim[NL];
#pragma unroll
            for (int k = 0; k < NL; k++) { cre[k] = fre[k]; cim[k] = fim[k]; }
            mul_dense(fre, fim, t, TeamRec{cre, cim, t.base4});
        }
        const int32_t* base = lines + (size_t)L * n * LINE_DW;
#pragma unroll 1
        for (uint32_t i = 0; __any(i < len); i++) {           // the wavefront's longest chunk
            const bool use = i < len;
            const uint32_t pi = min(first + (use ? i : 0u), last);   // a team past its chunk: a pair of the slice, read and discarded
            uint32_t jA, jB;
            line_positions(L, bad[pi], jA, jB);
            const int4* rec = reinterpret_cast<const int4*>(base + (size_t)pi * LINE_DW);
            int32_t y[6][NL];
            {
                int4 q[LINE_DW / 4];
#pragma unroll
                for (int k = 0; k < LINE_DW / 4; k++) q[k] = rec[k];
#pragma unroll
                for (int k = 0; k < LINE_DW / 4; k++) {
                    const int e = 4 * k;
                    y[e / NL][e % NL] = q[k].x; y[(e + 1) / NL][(e + 1) % NL] = q[k].y;
                    y[(e + 2) / NL][(e + 2) % NL] = q[k].z; y[(e + 3) / NL][(e + 3) % NL] = q[k].w;
                }
            }
            int32_t re[NL], im[NL];
#pragma unroll
            for (int k = 0; k < NL; k++) { re[k] = fre[k]; im[k] = fim[k]; }
            mul_line_k3(re, im, t, jA, jB, y);
#pragma unroll
            for (int k = 0; k < NL; k++) { fre[k] = use ? re[k] : fre[k]; fim[k] = use ? im[k] : fim[k]; }
        }
    }
    if (valid) {
        const uint32_t flat = (t.c & 1u) ? 3u + (t.c >> 1) : (t.c >> 1);
        uint32_t* o = partials + (size_t)dest * 144 + flat * 24u;
        fe a, b;
#pragma unroll
        for (int k = 0; k < NL; k++) { a.v[k] = fre[k]; b.v[k] = fim[k]; }
        uint32_t w[12];
        r28::to_vm(w, a);
#pragma unroll
        for (int k = 0; k < 12; k++) o[k] = w[k];
        r28::to_vm(w, b);
#pragma unroll
        for (int k = 0; k < 12; k++) o[12 + k] = w[k];
    }
}
#else
;
#endif

// One fold entry per team: tab[3 id ..] = (first source slot, count, destination slot), 1 <= count.  The team multiplies the
// partials [src, src + count) of `partials` (VM words) densely and writes the product to slot dest.  No destination of a launch
// is a source of it (pairing_ranges_plan.h: a level's outputs are new slots, or slots below m that nothing reads).
__global__ void __launch_bounds__(256, 2) k_ml_fold_ranges(uint32_t* partials, const uint32_t* __restrict__ tab, uint32_t nfolds)
#if BLSGPU_EMIT(BLSGPU_TU_MLR)
{
    const Team t = team_of_lane();
    if (wave_index() * TEAMS >= nfolds) return;               // the whole wavefront
    const uint32_t id = wave_index() * TEAMS + t.slot;
    const bool valid = t.slot < (uint32_t)TEAMS && id < nfolds;
    const uint32_t idc = valid ? id : wave_index() * TEAMS;
    const uint32_t src = tab[3 * (size_t)idc], count = valid ? tab[3 * (size_t)idc + 1] : 0u, dest = tab[3 * (size_t)idc + 2];
    const uint32_t flat = (t.c & 1u) ? 3u + (t.c >> 1) : (t.c >> 1);
    // the partial at slot q: the lane's part, from the VM words
    auto load = [&](uint32_t q, int32_t* __restrict__ re, int32_t* __restrict__ im) {
        const uint32_t* p = partials + (size_t)q * 144 + flat * 24u;
        uint32_t w[12];
#pragma unroll
        for (int j = 0; j < 12; j++) w[j] = p[j];
        const fe a = r28::from_vm(w);
#pragma unroll
        for (int j = 0; j < 12; j++) w[j] = p[12 + j];
        const fe b = r28::from_vm(w);
#pragma unroll
        for (int j = 0; j < NL; j++) { re[j] = a.v[j]; im[j] = b.v[j]; }
    };
    int32_t fre[NL], fim[NL];
    load(src, fre, fim);                                      // count >= 1 (a team of no entry: the slot of its wavefront's first row, discarded)
#pragma unroll 1
    for (uint32_t i = 1; __any(i < count); i++) {             // the wavefront's longest entry
        const bool act = i < count;
        int32_t yre[NL], yim[NL], nre[NL], nim[NL];
        load(src + (act ? i : 0u), yre, yim);                 // past its count: its first source again, read and discarded
#pragma unroll
        for (int j = 0; j < NL; j++) { nre[j] = fre[j]; nim[j] = fim[j]; }
        mul_dense(nre, nim, t, TeamRec{yre, yim, t.base4});
#pragma unroll
        for (int j = 0; j < NL; j++) { fre[j] = act ? nre[j] : fre[j]; fim[j] = act ? nim[j] : fim[j]; }
    }
    if (valid) {
        uint32_t* o = partials + (size_t)dest * 144 + flat * 24u;
        fe a, b;
#pragma unroll
        for (int k = 0; k < NL; k++) { a.v[k] = fre[k]; b.v[k] = fim[k]; }
        uint32_t w[12];
        r28::to_vm(w, a);
#pragma unroll
        for (int k = 0; k < 12; k++) o[k] = w[k];
        r28::to_vm(w, b);
#pragma unroll
        for (int k = 0; k < 12; k++) o[12 + k] = w[k];
    }
}
#else
;
#endif

}  // namespace ml
}  // namespace blsgpu
