// blsgpu_msmr.hip -- RAGGED multi-scalar sums: out_j = sum_{i in [begin_j, end_j)} s_i P_i for m ranges of ANY lengths over n
// points of G1 (DEG 1) or of the twist (DEG 2) with 256-bit PUBLIC scalars, nothing padded (blsgpu_g1_msm_ranges /
// blsgpu_g2_msm_ranges; included by blsgpu_api.hip, built with blsgpu_msm.hip in translation unit 5).  vmgen/msmr_model.py is
// the specification of the chunk table, of a chunk's window recurrence and of the per-range combination
// (tests/test_msmr_model.py).
//   schedule   every range is cut into CHUNKS of at most CHUNK = 8 consecutive points (ceil(L / 8) chunks for a range of L
//              points, none for an empty range); ONE CHUNK PER UNIT -- a lane for G1, a lane pair for G2, unit = global lane /
//              LP -- on k_smul's schedule (blsgpu_msm.hip) for the unit's own (first point, count <= 8): the table 0 .. 15 P of
//              each point by 14 mixed additions (entry 0 infinity, entry 1 the point), then 64 windows of 4 bits from the top,
//              4 doublings between windows and one complete addition of the digit-selected entry per point: 252 doublings per
//              CHUNK and 14 + 64 additions per POINT, where k = 1 calls spend the 252 per point.  The chunk's partial sum
//              leaves through SrtG's affine_out into a chunk-indexed array; the chunks of range j are the consecutive chunks
//              [first_chunk[j], first_chunk[j + 1]), so the per-range sums are blsgpu_pscan.hip's range sums over the partials
//              (blsgpu_api.hip msm_ranges_dev).  The scalars are the 256-bit integers they are, NOT reduced, as in k_smul.
//              Why 8: it is k_smul's BLSGPU_SMUL_MAX_K, the longest group that kernel is sent; a longer chunk saves
//              doublings (252 / count per point against 78 additions) and costs table workspace and units for short ranges.
//              Other chunk lengths: NOT MEASURED.
//   public     points, scalars and ranges are PUBLIC data: NOT constant-time.  The table entry is fetched at an address the
//              digit chooses, the trip counts follow the range lengths and the on-curve test branches.  A secret scalar
//              belongs on secret_window.h's schedule.
//   off curve  before a table is built the unit tests the point with pscan::on_curve; a point that is neither (0, 0) nor on
//              the curve enters as infinity (every table entry infinity, like a point that is not live) and is counted in the
//              chunk's entry of `bad`.  On a G2 pair both lanes test the whole Fq2 point, so the outcome is uniform per pair.
//   control    sp2's arithmetic exchanges values between the two lanes of a pair; both lanes share `unit`, hence the chunk and
//              its count.  The loops over a chunk's points run to the UNIT'S OWN count (a per-unit branch, uniform per pair):
//              a unit with a short chunk idles while its wavefront finishes the longest one.  The alternative -- the
//              wavefront's maximum as the trip count, a unit past its count building an all-infinity table and taking digit
//              0 -- is BLSGPU_MSMR_WAVE_UNIFORM=1 at compile time; it executes the same number of point operations per
//              wavefront and adds table stores (make libblsgpu_msmru.so builds it for tools/msm_ranges_probe.py).  MEASURED,
//              both libraries in one session (profiles/msm_ranges_probe.txt and msm_ranges_probe_msmru.txt, the same bytes):
//              the uniform trip count is equal on the skewed G1 shape (9.01 against 9.00 ms) and 1 to 3 % slower on every
//              other shape of both groups, never faster.  The per-unit branch ships.
//   table      count x 16 projective records in the unit's own piece of HBM workspace, 8 x 16 records of room per unit
//              (21.5 KB G1, 43 KB G2) whatever the count, as k_smul keeps it (k_smul64's header: neither LDS nor registers
//              hold it at two wavefronts per SIMD).  A table packed by count: NOT MEASURED.
//   launch     __launch_bounds__(64, 2), the budget of every SrtG kernel.  The compiler's report for gfx950: see
//              MSMR_RESOURCES below.  A launch takes at most SRT_LANES / LP units and at most 2 GB of tables
//              (blsgpu_api.hip slices the chunks).  Three wavefronts per SIMD: NOT MEASURED.
//   input      prep / live: k_lane_prep's points (affine L28, (0, 0) not live); scalars: n x 32 bytes big-endian; tab: per
//              chunk (first point, count), 1 <= count <= 8, first + count <= n (k_msmr_fill writes it from checked ranges).
//   tail       spare units of the last wavefront repeat the last chunk and store nothing (k_smul's convention); the unit is
//              the global lane / LP, so both lanes of a G2 pair are spare or neither is.
// MSMR_RESOURCES (the compiler's kernel-resource-usage report for gfx950, per-unit branch): k_smul_seg<1> 217 registers and no
// scratch; k_smul_seg<2> 250 registers and 116 bytes of scratch without a spill (k_smul: 214 / 0 and 234 / 116); two
// wavefronts per SIMD both.  The glue kernels (k_msmr_count, k_msmr_scan, k_msmr_fill, k_msmr_offcurve) take 4 to 14 registers.
// Every store is a plain C++ store; no inline assembly.
#pragma once

#ifndef BLSGPU_MSMR_WAVE_UNIFORM
#define BLSGPU_MSMR_WAVE_UNIFORM 0
#endif

namespace blsgpu {
namespace msmr {

constexpr uint32_t CHUNK = 8;                                // points per unit: k_smul's BLSGPU_SMUL_MAX_K
constexpr uint32_t SCAN_THREADS = 1024;

// head[0] |= 1 if one of the m ranges has begin > end or end > n; cnt[i] = ceil(len_i / CHUNK) (0 for a bad range) and their
// sum in the 64-bit counter at head + 2 (it cannot wrap: m < 2^31 ranges of at most 2^29 chunks)
__global__ void __launch_bounds__(256) k_msmr_count(const uint32_t* __restrict__ ranges, uint32_t m, uint32_t n, uint32_t* __restrict__ head,
                                                    uint32_t* __restrict__ cnt)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t b = ranges[2 * (size_t)i], e = ranges[2 * (size_t)i + 1];
    const bool bad = b > e || e > n;
    const uint32_t k = bad ? 0u : (e - b) / CHUNK + ((e - b) % CHUNK ? 1u : 0u);
    cnt[i] = k;
    if (bad) atomicOr(head, 1u);
    if (k) atomicAdd(reinterpret_cast<unsigned long long*>(head + 2), (unsigned long long)k);
}
#else
;
#endif

// out[0 .. n] = the exclusive prefix sums of in[0 .. n) and their total: ONE workgroup, a run of ceil(n / 1024) entries per
// lane, the lane sums scanned through LDS (k_srt_scan_window's Hillis-Steele), the run replayed from its carry-in.  It runs
// over the m counts and again over the chunks' off-curve counts, reading its input twice, serially per lane: a few microseconds
// at the probe's sizes, but about two million dependent loads a lane near the limit of 2^31 chunks.  Its cost at such sizes, and
// a multi-workgroup scan in its place: NOT MEASURED.
__global__ void __launch_bounds__(1024) k_msmr_scan(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    __shared__ uint32_t part[SCAN_THREADS];
    const uint32_t t = threadIdx.x, per = (n + SCAN_THREADS - 1u) / SCAN_THREADS;
    const uint32_t lo = (uint64_t)t * per < n ? t * per : n, hi = n - lo < per ? n : lo + per;
    uint32_t s = 0;
    for (uint32_t k = lo; k < hi; k++) s += in[k];
    part[t] = s;
    __syncthreads();
    for (uint32_t off = 1; off < SCAN_THREADS; off <<= 1) {
        const uint32_t v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (uint32_t k = lo; k < hi; k++) {
        const uint32_t own = in[k];
        out[k] = run;
        run += own;
    }
    if (t == SCAN_THREADS - 1u) out[n] = part[t];
}
#else
;
#endif

// The chunk table from first[0 .. m] (k_msmr_scan of the counts): chunk c belongs to the LAST range j < m with first[j] <= c
// (empty ranges share their first with the next one and own nothing); its points are begin_j + 8 (c - first[j]) .. , at most 8
// and not past end_j.  Lanes c < m also write range c's chunk range (first[c], first[c + 1]) for the range-sum passes.
__global__ void __launch_bounds__(256) k_msmr_fill(const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ first, uint32_t m,
                                                   uint32_t total, uint32_t* __restrict__ tab, uint32_t* __restrict__ cr)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m) {
        cr[2 * (size_t)c] = first[c];
        cr[2 * (size_t)c + 1] = first[c + 1];
    }
    if (c >= total) return;
    uint32_t lo = 0, hi = m;                                 // first[lo] <= c always (first[0] = 0)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (first[mid] <= c) lo = mid; else hi = mid;
    }
    const uint32_t p = ranges[2 * (size_t)lo] + (c - first[lo]) * CHUNK, left = ranges[2 * (size_t)lo + 1] - p;
    tab[2 * (size_t)c] = p;
    tab[2 * (size_t)c + 1] = left < CHUNK ? left : CHUNK;
}
#else
;
#endif

// tab: nchunks x (first point, count); table: units x CHUNK x SMUL_T x G::PJ dwords of this launch's own; out: nchunks affine
// points (24 DEG dwords each); bad: nchunks counts of points off the curve
template <int DEG>
__global__ void __launch_bounds__(64, 2) k_smul_seg(const uint32_t* __restrict__ prep, const uint8_t* __restrict__ live,
                                                    const uint32_t* __restrict__ scalars, const uint32_t* __restrict__ tab, uint32_t nchunks,
                                                    uint32_t* __restrict__ table, uint32_t* __restrict__ out, uint32_t* __restrict__ bad)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    typedef SrtG<DEG> G;
    typedef typename pscan::Cfg<DEG>::E E;
    const uint32_t unit = (blockIdx.x * blockDim.x + threadIdx.x) / G::LP;
    const bool real = unit < nchunks;
    const uint32_t g = real ? unit : nchunks - 1u;
    const uint32_t first = tab[2 * (size_t)g], count = tab[2 * (size_t)g + 1];
#if BLSGPU_MSMR_WAVE_UNIFORM
    uint32_t trip = count;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) trip = max(trip, (uint32_t)__shfl_xor((int)trip, off));
#else
    const uint32_t trip = count;
#endif
    uint32_t* T = table + (size_t)unit * CHUNK * SMUL_T * G::PJ;
    uint32_t nbad = 0;
#pragma unroll 1
    for (uint32_t i = 0; i < trip; i++) {
        const size_t pi = (size_t)first + (i < count ? i : 0u);
        const uint32_t* p = prep + pi * L28_AFF * DEG;
        bool lv = i < count && live[pi] != 0;
        if (lv && !pscan::on_curve(r28::Elem<E>::load(p), r28::Elem<E>::load(p + pscan::Cfg<DEG>::DW))) {
            lv = false;
            nbad++;
        }
        typename G::P m = G::inf();
        G::st(m, T + (size_t)i * SMUL_T * G::PJ);
#pragma unroll 1
        for (uint32_t d = 1; d < SMUL_T; d++) {
            if (lv) G::madd(m, p, 0u);
            G::st(m, T + ((size_t)i * SMUL_T + d) * G::PJ);
        }
    }
    typename G::P acc = G::inf();
#pragma unroll 1
    for (int w = 63; w >= 0; w--) {
        if (w != 63) {
#pragma unroll 1
            for (int t = 0; t < 4; t++) acc = G::dbl(acc);
        }
#pragma unroll 1
        for (uint32_t i = 0; i < trip; i++) {
            const uint32_t word = bswap32(scalars[((size_t)first + (i < count ? i : 0u)) * 8 + 7u - ((uint32_t)w >> 3)]);
            const uint32_t d = i < count ? (word >> (((uint32_t)w & 7u) * 4u)) & 15u : 0u;
            acc = G::add(acc, G::ld(T + ((size_t)i * SMUL_T + d) * G::PJ));
        }
    }
    G::affine_out(acc, out + (size_t)g * 24 * DEG, nullptr, real);
    if (real && (G::LP == 1 || (threadIdx.x & 1u) == 0)) bad[g] = nbad;
}
#else
;
#endif

// badpre[0 .. total]: the exclusive prefix sums of the chunks' counts of points off the curve; a range whose chunks
// [first[j], first[j + 1]) hold one gets flag 2 and the output (0, 0), over what the range-sum pass wrote
template <int DEG>
__global__ void __launch_bounds__(256) k_msmr_offcurve(const uint32_t* __restrict__ badpre, const uint32_t* __restrict__ first, uint32_t m,
                                                       uint32_t* __restrict__ out, uint8_t* __restrict__ flag)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m || badpre[first[j + 1]] == badpre[first[j]]) return;
    flag[j] = 2;
    for (uint32_t w = 0; w < 24u * DEG; w++) out[(size_t)j * 24 * DEG + w] = 0u;
}
#else
;
#endif

// every instantiation the host side launches: translation unit 5 emits them (blsgpu_tu.h)
#if BLSGPU_TU == BLSGPU_TU_MSM
__attribute__((used)) static const void* const blsgpu_instances_msmr[] = {(const void*)&k_smul_seg<1>, (const void*)&k_smul_seg<2>,
                                                                          (const void*)&k_msmr_offcurve<1>, (const void*)&k_msmr_offcurve<2>};
#endif

}  // namespace msmr
}  // namespace blsgpu
