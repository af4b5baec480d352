// blsgpu_pscan.hip -- PREFIX SUMS over curve points and sums over RANGES of unequal length: S[j] = sum_{i<j} P_i for n affine
// points of G1 (DEG 1) or of the twist (DEG 2), kept as projective records in workspace, and any number of range sums
// S[end] - S[begin], each ONE point subtraction (blsgpu_g1_range_sums / blsgpu_g2_range_sums, and the node sums of
// blsgpu_verify_find_folded; included by blsgpu_api.hip, built with blsgpu_msm.hip in translation unit 5).
// vmgen/pscan_model.py is the specification of the three passes and of the range difference (tests/test_pscan_model.py).
//
// Why no case analysis is needed.  The scan runs on fp28.h's ptT<E> with the COMPLETE formulas of Renes-Costello-Batina for
// a = 0 (pt_inf, pt_ld, pt_st, padd, pmadd).  They are complete on every curve WITHOUT A POINT OF ORDER TWO, and both
// E(Fq): y^2 = x^3 + 4 and the twist E'(Fq2): y^2 = x^3 + 4 (1 + u) have ODD order: #E = h1 r and #E' = h2 r with r odd, and
// both cofactors are odd because the curve parameter z = -0xd201000000010000 is even (h1 = (z - 1)^2 / 3,
// h2 = (z^8 - 4 z^7 + 5 z^6 - 4 z^4 + 6 z^3 - 4 z^2 - 4 z + 13) / 9: an odd numerator over an odd denominator).  So the formulas
// hold for every pair of points of either curve, not only of the prime-order subgroups:
//   * S[b] - S[a] meets P + (-P) whenever the range sums to infinity,
//   * it meets P + P (through the negation, P + (-(-P))) whenever the two prefixes are negatives of one another, and the scan
//     meets P + P whenever two adjacent inputs are equal,
//   * an input may itself be infinity ((0, 0)): it is skipped, which is adding (0 : 1 : 0).
// An input that is neither (0, 0) nor on the curve is outside that argument: it is COUNTED (an integer prefix count beside the
// point scan) and enters the sums as infinity, so a range knows whether it holds one.  Nothing is checked for the subgroup.
//
// The passes over n points, CHUNK consecutive points per lane (M = ceil(n / CHUNK) chunks, at least one):
//   k_pscan_totals   lane t: the on-curve test of its points (kind 0 infinity, 1 added, 2 off the curve), its chunk total by
//                    complete mixed additions and its count of points off the curve.
//   k_pscan_mid      ONE workgroup of MID_THREADS lanes: the exclusive scan of the M chunk totals and counts in place, from the
//                    carry of the slice before (NULL: infinity and zero).  A lane sums ceil(M / MID_THREADS) consecutive totals,
//                    the lane sums are scanned through LDS (Kogge-Stone: log2 MID_THREADS steps of one complete addition), and
//                    the lane replays its totals from its carry-in.  A projective record of the twist is 336 bytes: 128 of them
//                    are 43 KB of LDS, inside the 64 KB a workgroup gets without asking; 256 would not be.
//   k_pscan_replay   lane t: its chunk again from its carry-in, every prefix S[i] and count stored before point i is added; the
//                    lane of the last chunk stores S[n] as well.
// About 2 n mixed additions and 2 M / MID_THREADS + log2 MID_THREADS sequential complete additions in the middle.  CHUNK = 16
// balances the two at n = 32 768 (2 x 16 mixed additions a lane against 39 additions in the middle) and leaves 2048 lanes;
// at 2^20 points the middle is the longer part (1031 additions).  Other chunk lengths and a recursive middle: NOT MEASURED.
// The lane passes run under __launch_bounds__(64, 2), the register budget of the other point kernels (k_smul64's header).
//   k_pscan_check    the _dev form's scan of the ranges: begin <= end <= n, before anything is written.
//   k_pscan_begin    one dword per lane: the record and count at a range's begin copied beside the range -- only when the
//                    points take more than one SLICE of records (blsgpu_api.hip), so that the record is still there when the
//                    slice that holds the range's end is scanned.
//   k_pscan_range    one range per lane (G1) or lane pair (G2), on SrtG<DEG> as k_smul64: S[end] + (-S[begin]) by ONE complete
//                    addition, then SrtG's affine_out -- canonical affine bytes, (0, 0) for infinity.  flag 0 finite, 1
//                    infinity, 2 when the counts at end and begin differ (a point off the curve inside: the output is (0, 0)).
//                    sp2's lane-pair record of a twist point is the same 84 dwords that pt_st<fe2> writes.
// The glue kernels of blsgpu_verify_find_folded are at the end of the file.
// Every store is a plain C++ store; no inline assembly.
#pragma once

namespace blsgpu {
namespace pscan {

constexpr uint32_t CHUNK = 16;                               // points per lane
constexpr uint32_t MID_THREADS = 128;                        // lanes of the middle scan's one workgroup

template <int DEG> struct Cfg {
    typedef typename LaneElem<DEG>::E E;
    static constexpr uint32_t AFF = L28_AFF * DEG, PJ = L28_PJ * DEG, DW = r28::NL * DEG;
};
// the curve's b in the form a product takes: 4 on G1, 4 (1 + u) on the twist
__device__ __forceinline__ r28::fe curve_b(const r28::fe&) { return r28::mulc_norm<4>(r28::fe_one()); }
__device__ __forceinline__ r28::fe2 curve_b(const r28::fe2&) { return {r28::mulc_norm<4>(r28::fe_one()), r28::mulc_norm<4>(r28::fe_one())}; }
// y^2 = x^3 + b: the difference through one product by one, which is what is_zero takes
template <class E> __device__ __forceinline__ bool on_curve(const E& x, const E& y) {
    const auto d = r28::sub(r28::sub(r28::sqr(y), r28::mul(r28::sqr(x), x)), curve_b(x));
    return r28::is_zero(r28::mul(r28::norm(d), r28::Elem<E>::one()));
}

// prep / live: k_lane_prep's points; kind: n bytes; ct: M records; cb: M counts
template <int DEG>
__global__ void __launch_bounds__(64, 2) k_pscan_totals(const uint32_t* __restrict__ prep, const uint8_t* __restrict__ live, uint32_t n,
                                                        uint8_t* __restrict__ kind, uint32_t* __restrict__ ct, uint32_t* __restrict__ cb)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    typedef typename Cfg<DEG>::E E;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, chunks = n ? (n + CHUNK - 1) / CHUNK : 1u;
    if (t >= chunks) return;
    const uint32_t lo = t * CHUNK, hi = n - lo < CHUNK ? n : lo + CHUNK;
    r28::ptT<E> acc = r28::pt_inf<E>();
    uint32_t bad = 0;
#pragma unroll 1
    for (uint32_t i = lo; i < hi; i++) {
        uint8_t k = 0;
        if (live[i]) {
            const uint32_t* p = prep + (size_t)i * Cfg<DEG>::AFF;
            const E x = r28::Elem<E>::load(p), y = r28::Elem<E>::load(p + Cfg<DEG>::DW);
            if (on_curve(x, y)) {
                r28::pmadd(acc, x, y);
                k = 1;
            } else {
                bad++;
                k = 2;
            }
        }
        kind[i] = k;
    }
    r28::pt_st(acc, ct + (size_t)t * Cfg<DEG>::PJ);
    cb[t] = bad;
}
#else
;
#endif

// ct / cb: the chunk totals and counts, replaced by their exclusive prefixes (+ the carry); carry_pt / carry_cnt may be NULL
template <int DEG>
__global__ void __launch_bounds__(MID_THREADS) k_pscan_mid(uint32_t* __restrict__ ct, uint32_t* __restrict__ cb, uint32_t chunks,
                                                           const uint32_t* __restrict__ carry_pt, const uint32_t* __restrict__ carry_cnt)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    typedef typename Cfg<DEG>::E E;
    constexpr uint32_t PJ = Cfg<DEG>::PJ;
    __shared__ uint32_t sp[MID_THREADS * PJ];
    __shared__ uint32_t sc[MID_THREADS];
    const uint32_t t = threadIdx.x, per = (chunks + MID_THREADS - 1) / MID_THREADS;
    const uint32_t lo = t * per < chunks ? t * per : chunks, hi = chunks - lo < per ? chunks : lo + per;
    r28::ptT<E> v = r28::pt_inf<E>();
    uint32_t cnt = 0;
#pragma unroll 1
    for (uint32_t j = lo; j < hi; j++) {
        v = r28::padd_fn(v, r28::pt_ld<E>(ct + (size_t)j * PJ));
        cnt += cb[j];
    }
#pragma unroll 1
    for (uint32_t d = 1; d < MID_THREADS; d <<= 1) {
        r28::pt_st(v, sp + t * PJ);
        sc[t] = cnt;
        __syncthreads();
        if (t >= d) {
            v = r28::padd_fn(r28::pt_ld<E>(sp + (t - d) * PJ), v);
            cnt += sc[t - d];
        }
        __syncthreads();
    }
    r28::pt_st(v, sp + t * PJ);
    sc[t] = cnt;
    __syncthreads();
    r28::ptT<E> run = t ? r28::pt_ld<E>(sp + (t - 1) * PJ) : r28::pt_inf<E>();
    uint32_t c = t ? sc[t - 1] : 0u;
    if (carry_pt) {
        run = r28::padd_fn(r28::pt_ld<E>(carry_pt), run);
        c += *carry_cnt;
    }
#pragma unroll 1
    for (uint32_t j = lo; j < hi; j++) {
        const r28::ptT<E> own = r28::pt_ld<E>(ct + (size_t)j * PJ);
        const uint32_t oc = cb[j];
        r28::pt_st(run, ct + (size_t)j * PJ);
        cb[j] = c;
        run = r28::padd_fn(run, own);
        c += oc;
    }
}
#else
;
#endif

// s: n + 1 records; cnt: n + 1 counts
template <int DEG>
__global__ void __launch_bounds__(64, 2) k_pscan_replay(const uint32_t* __restrict__ prep, const uint8_t* __restrict__ kind, uint32_t n,
                                                        const uint32_t* __restrict__ ct, const uint32_t* __restrict__ cb,
                                                        uint32_t* __restrict__ s, uint32_t* __restrict__ cnt)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    typedef typename Cfg<DEG>::E E;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, chunks = n ? (n + CHUNK - 1) / CHUNK : 1u;
    if (t >= chunks) return;
    const uint32_t lo = t * CHUNK, hi = n - lo < CHUNK ? n : lo + CHUNK;
    r28::ptT<E> run = r28::pt_ld<E>(ct + (size_t)t * Cfg<DEG>::PJ);
    uint32_t c = cb[t];
#pragma unroll 1
    for (uint32_t i = lo; i < hi; i++) {
        r28::pt_st(run, s + (size_t)i * Cfg<DEG>::PJ);
        cnt[i] = c;
        const uint8_t k = kind[i];
        if (k == 1) {
            const uint32_t* p = prep + (size_t)i * Cfg<DEG>::AFF;
            const E x = r28::Elem<E>::load(p), y = r28::Elem<E>::load(p + Cfg<DEG>::DW);
            r28::pmadd(run, x, y);
        }
        c += k == 2 ? 1u : 0u;
    }
    if (hi == n) {
        r28::pt_st(run, s + (size_t)n * Cfg<DEG>::PJ);
        cnt[n] = c;
    }
}
#else
;
#endif

// Record index j of the whole input lies in the slice [lo, hi] of records s[0 .. hi - lo] when lo <= j < hi, or j = hi in the
// LAST slice (the record hi of another slice is the record lo of the next).
__device__ __forceinline__ bool in_slice(uint32_t j, uint32_t lo, uint32_t hi, uint32_t last) { return j >= lo && (j < hi || (last && j == hi)); }

// total = m x PJ dwords; base: m records; basec: m counts
template <int DEG>
__global__ void __launch_bounds__(256) k_pscan_begin(const uint32_t* __restrict__ s, const uint32_t* __restrict__ cnt, uint32_t lo, uint32_t hi,
                                                     uint32_t last, const uint32_t* __restrict__ ranges, size_t total,
                                                     uint32_t* __restrict__ base, uint32_t* __restrict__ basec)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    constexpr uint32_t PJ = Cfg<DEG>::PJ;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const size_t r = idx / PJ;
    const uint32_t w = (uint32_t)(idx - r * PJ), b = ranges[2 * r];
    if (!in_slice(b, lo, hi, last)) return;
    base[idx] = s[(size_t)(b - lo) * PJ + w];
    if (w == 0) basec[r] = cnt[b - lo];
}
#else
;
#endif

// flag[0] |= 1 if one of the m ranges has begin > end or end > n (the _dev form checks before it writes)
__global__ void __launch_bounds__(256) k_pscan_check(const uint32_t* __restrict__ ranges, uint32_t m, uint32_t n, uint32_t* __restrict__ flag)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m && (ranges[2 * (size_t)i] > ranges[2 * (size_t)i + 1] || ranges[2 * (size_t)i + 1] > n)) atomicOr(flag, 1u);
}
#else
;
#endif

__device__ __forceinline__ r28::ptT<r28::fe> neg_pt(const r28::ptT<r28::fe>& p) { return r28::pneg(p); }
__device__ __forceinline__ sp2::pt neg_pt(const sp2::pt& p) { return sp2::pneg(p); }

// ranges: m x (begin, end); the ranges whose END lies in the slice are finished; base / basec NULL: the begin is in the slice too
template <int DEG>
__global__ void __launch_bounds__(64, 2) k_pscan_range(const uint32_t* __restrict__ s, const uint32_t* __restrict__ cnt, uint32_t lo, uint32_t hi,
                                                       uint32_t last, const uint32_t* __restrict__ ranges, uint32_t m,
                                                       const uint32_t* __restrict__ base, const uint32_t* __restrict__ basec,
                                                       uint32_t* __restrict__ out, uint8_t* __restrict__ flag)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    typedef SrtG<DEG> G;
    const uint32_t unit = (blockIdx.x * blockDim.x + threadIdx.x) / G::LP;
    const uint32_t g = unit < m ? unit : m - 1u;
    const uint32_t b = ranges[2 * (size_t)g], e = ranges[2 * (size_t)g + 1];
    const bool real = unit < m && in_slice(e, lo, hi, last);
    bool bad = false;
    typename G::P acc = G::inf();
    if (real) {
        const uint32_t cb = base ? basec[g] : cnt[b - lo];
        bad = cnt[e - lo] != cb;
        if (!bad) acc = G::add(G::ld(s + (size_t)(e - lo) * G::PJ), neg_pt(G::ld(base ? base + (size_t)g * G::PJ : s + (size_t)(b - lo) * G::PJ)));
    }
    uint8_t* f = flag + g;
    G::affine_out(acc, out + (size_t)g * 24 * DEG, f, real);
    if (real && bad && (G::LP == 1 || (threadIdx.x & 1u) == 0)) *f = 2;
}
#else
;
#endif

// ---- the glue of blsgpu_verify_find_folded (blsgpu_api.hip verify_find_folded_dev) -----------------------------------------
constexpr uint32_t THREADS = 256, RUN_THREADS = 1024;

// flag[0] |= 2 if idx[i] < idx[i - 1] for an i of [first, first + m), first + m <= n (the items of one launch; i = 0 has no
// predecessor): the folded call's precondition, scanned beside the index ranges
__global__ void __launch_bounds__(256) k_fold_mono(const uint32_t* __restrict__ idx, uint32_t first, uint32_t m, uint32_t* __restrict__ flag)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    const uint32_t i = first + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < first + m && i > 0 && idx[i] < idx[i - 1]) atomicOr(flag, 2u);
}
#else
;
#endif

// The RUN TABLE of the dense order, one workgroup (k_find_dense's ballot scan): position p begins a run when p = 0 or its item
// names another message than the item before it.  rb[r]: the run's first position, rb[n_runs] = n_e; rmsg[r]: its message.
__global__ void __launch_bounds__(1024) k_fold_runs(const uint32_t* __restrict__ dense, const uint32_t* __restrict__ n_e_ptr,
                                                    const uint32_t* __restrict__ msg_idx, uint32_t* __restrict__ rb,
                                                    uint32_t* __restrict__ rmsg, uint32_t* __restrict__ n_runs)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    __shared__ uint32_t wsum[RUN_THREADS / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6, n = *n_e_ptr;
    uint32_t run = 0;
    for (uint32_t base = 0; base < n; base += RUN_THREADS) {
        const uint32_t p = base + t;
        const uint32_t mine = p < n ? msg_idx[dense[p]] : 0u;
        const bool f = p < n && (p == 0 || mine != msg_idx[dense[p - 1]]);
        const unsigned long long bal = __ballot(f);
        if (lane == 0) wsum[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t j = 0; j < RUN_THREADS / 64; j++) {
            before += j < wv ? wsum[j] : 0u;
            total += wsum[j];
        }
        if (f) {
            const uint32_t r = run + before + (uint32_t)__popcll(bal & (((unsigned long long)1 << lane) - 1ull));
            rb[r] = p;
            rmsg[r] = mine;
        }
        run += total;
        __syncthreads();
    }
    if (t == 0) {
        rb[run] = n;
        *n_runs = run;
    }
}
#else
;
#endif

// total = n x 18 pieces, of which the first *n_e_ptr x 18 are copied: the leaves in the DENSE order, ad[p] = a[dense[p]] (12
// pieces), bd[p] = b[dense[p]] (6) -- once per call; no round gathers anything
__global__ void __launch_bounds__(256) k_fold_leaves(const uint32_t* __restrict__ dense, const uint32_t* __restrict__ n_e_ptr, size_t total,
                                                     const uint4* __restrict__ a, const uint4* __restrict__ b, uint4* __restrict__ ad,
                                                     uint4* __restrict__ bd)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    const size_t idx = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t p = idx / 18;
    if (p >= *n_e_ptr) return;
    const uint32_t piece = (uint32_t)(idx - p * 18), item = dense[p];
    if (piece < 12) ad[p * 12 + piece] = a[(size_t)item * 12 + piece];
    else bd[p * 6 + (piece - 12)] = b[(size_t)item * 6 + (piece - 12)];
}
#else
;
#endif

// One node per lane.  first[node] .. first[node + 1]: its slots -- slot 0 the pair (-G1, S), the others (B_r, H(h_r)).  A sum
// at infinity never reaches the pairing as a point: the slots whose sum is at infinity (or holds a bad point, which cannot
// happen with the leaves of eligible items) take (G1, G2) and (-G1, G2) IN TURN -- code 1, 2, 1, 2 ... -- a couple that
// cancels; when their number is odd the last one is (-G1, G2) alone and the node's result is compared with e(-G1, G2)
// (odd[node] = 1: k_find_verdict's unit) instead of one.  code 0: the slot keeps its own pair.  bflag: the flags of the B sums,
// which are kept WITHOUT the head slots -- node i's slot sl > first[i] has the sum sl - i - 1.
__global__ void __launch_bounds__(256) k_fold_codes(const uint32_t* __restrict__ first, uint32_t n_nodes, const uint8_t* __restrict__ bflag,
                                                    const uint8_t* __restrict__ sflag, uint8_t* __restrict__ code, uint8_t* __restrict__ odd)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_nodes) return;
    const uint32_t lo = first[i], hi = first[i + 1];
    uint32_t k = 0;
    for (uint32_t sl = hi; sl-- > lo;) {                                     // from the end: the unpaired one, if any, is found first
        const bool at_inf = (sl == lo ? sflag[i] : bflag[sl - i - 1u]) != 0;                // B sums: one per slot that is no head
        code[sl] = at_inf ? (uint8_t)(2u - (k & 1u)) : (uint8_t)0;
        k += at_inf ? 1u : 0u;
    }
    odd[i] = (uint8_t)(k & 1u);
}
#else
;
#endif

// total = slots x 18 pieces: the pairs in the layout of blsgpu_pairing_multi_batch_dev.  g1: -G1 in a node's head slot, the
// range sum B (b: the sums without the head slots) elsewhere, the couple's point where the code says so; g2: S of the node, H of
// the slot's message, or G2.
__global__ void __launch_bounds__(256) k_fold_fill(const uint32_t* __restrict__ node_of, const uint32_t* __restrict__ first,
                                                   const uint32_t* __restrict__ slot_msg, size_t total, const uint8_t* __restrict__ code,
                                                   const uint4* __restrict__ b, const uint4* __restrict__ s, const uint4* __restrict__ h,
                                                   uint4* __restrict__ g1, uint4* __restrict__ g2)
#if BLSGPU_EMIT(BLSGPU_TU_MSM)
{
    const size_t idx = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= total) return;
    const size_t sl = idx / 18;
    const uint32_t piece = (uint32_t)(idx - sl * 18), node = node_of[sl], cd = code[sl];
    const bool head = sl == first[node];
    if (piece < 6) {
        g1[sl * 6 + piece] = cd == 1 ? sigsh::g1_gen_piece(piece)
                                     : (cd == 2 || head ? sigsh::neg_g1_piece(piece) : b[(sl - node - 1u) * 6 + piece]);
    } else {
        const uint32_t q = piece - 6;
        g2[sl * 12 + q] = cd != 0 ? sigsh::g2_gen_piece(q) : (head ? s[(size_t)node * 12 + q] : h[(size_t)slot_msg[sl] * 12 + q]);
    }
}
#else
;
#endif

// every instantiation the host side launches: translation unit 5 emits them (blsgpu_tu.h)
#if BLSGPU_TU == BLSGPU_TU_MSM
__attribute__((used)) static const void* const blsgpu_instances_pscan[] = {
    (const void*)&k_pscan_totals<1>, (const void*)&k_pscan_totals<2>, (const void*)&k_pscan_mid<1>, (const void*)&k_pscan_mid<2>,
    (const void*)&k_pscan_replay<1>, (const void*)&k_pscan_replay<2>, (const void*)&k_pscan_begin<1>, (const void*)&k_pscan_begin<2>,
    (const void*)&k_pscan_range<1>, (const void*)&k_pscan_range<2>};
#endif

}  // namespace pscan
}  // namespace blsgpu
