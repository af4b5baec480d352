// blsgpu_api.hip -- host side of the C ABI declared in include/blsgpu.h.
// Pure HIP runtime: no torch types, no CPU fallback.  If no GPU is usable the
// context cannot be created and every entry point fails loudly.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <optional>
#include <string>
#include <vector>

#include "../../include/blsgpu.h"
#include "blsgpu_tu.h"
#include "blsgpu_kernels.hip"
#include "fp28.h"
#include "blsgpu_ml.hip"
#include "blsgpu_mlr.hip"
#include "blsgpu_veragg.hip"
#include "blsgpu_fexp.hip"
#include "blsgpu_fexpw.hip"
#include "blsgpu_mlw.hip"
#include "blsgpu_lsw.hip"
#include "blsgpu_msm.hip"
#include "blsgpu_g1fix.hip"
#include "blsgpu_seeds.hip"
#include "blsgpu_g1poly.hip"
#include "blsgpu_subgroup.hip"
#include "blsgpu_lagrange.hip"
#include "blsgpu_sigdiv.hip"
#include "blsgpu_frsecret.hip"
#include "blsgpu_hashpks.hip"
#include "blsgpu_sigshares.hip"
#include "blsgpu_batchfind.hip"
#include "blsgpu_g2smul.hip"
#include "blsgpu_smul64.hip"
#include "blsgpu_pscan.hip"
#include "blsgpu_msmr.hip"
#include "blsgpu_h2c.hip"
#include "blsgpu_h2g1.hip"
#include "blsgpu_h2cw.hip"
#include "blsgpu_msmw.hip"
#include "blsgpu_probe.hip"

#if BLSGPU_EMIT(BLSGPU_TU_HOST)
#include "bisect_plan.h"
#include "find_plan.h"
#include "keys_plan.h"
#include "msm_plan.h"
#include "pairing_plan.h"
#include "pairing_ranges_plan.h"
#include "ragged_plan.h"
#include "secure_ranges_plan.h"
#include "verify_agg_plan.h"
#include "blsgpu_ctx.h"

// Which kernels a pairing call runs, its partials, chunks, levels, slices and buffer sizes are pairing_plan.h (host-only: tested
// without a GPU); the pairing functions below grow the buffers to a plan's totals and launch what it says.
namespace {
constexpr int MILLER_WAVES = 4;        // teams (pairings) per workgroup in k_miller
constexpr int REDUCE_WAVES = 8;        // teams per workgroup in k_reduce
constexpr size_t BATCH_TREE_MIN_GROUP = 24;   // batches of groups at least this long use the per-group product tree
constexpr int REDUCE_PER_BLOCK = 64;   // partials folded by one k_reduce block
constexpr size_t LS_MERGE_FAN = 8;     // partial products a merge level of the line-stream stage multiplies per output
constexpr unsigned SLOW_GRID = 3072;   // k_miller_slow: three wavefronts per SIMD (166 VGPRs, 10 KB of LDS each)
constexpr pairing::Consts PAIRING_CONSTS = {blsgpu::ml::LINES, blsgpu::ml::LINE_DW, blsgpu::ml::DENSE_DW, blsgpu::ml::TEAMS,
                                            blsgpu::ml::sp::SLAB_BYTES_PER_LANE, BLSVM_MP_G, blsgpu::TEAM_BYTES, blsgpu::MP_TEAM_BYTES,
                                            blsgpu::SLOW_TEAM_BYTES, BLS28_FEXP_NSLOTS, MILLER_WAVES, REDUCE_WAVES, REDUCE_PER_BLOCK,
                                            BATCH_TREE_MIN_GROUP, LS_MERGE_FAN, SLOW_GRID};
static_assert(pairing::same(PAIRING_CONSTS, pairing::GFX950), "pairing_plan.h: GFX950 (the host test's values) differs from the kernel files");
static_assert(pairing::PARTIAL_BYTES == BLSGPU_FQ12_BYTES && BLSGPU_G1_BYTES == 96 && BLSGPU_G2_BYTES == 192, "pairing_plan.h: slice_offsets");
// the slice lengths of the pairing path: groups per call of the grouped kernels (they ride on gridDim.y), pairs per line-stream
// launch sequence (24 GB of line records), pairs per slice of blsgpu_miller_loop_batch (6 GB)
pairing::Limits pairing_limits(const blsgpu_ctx* c) { return {slice_len(c, 32768), slice_len(c, (size_t)1 << 20), slice_len(c, 262144)}; }
int refuse(pairing::Refusal r) { return fail(pairing::refusal_code(r), pairing::refusal_text(r)); }
}  // namespace

// Room for `partials` partials in each partial buffer, and one work-list entry per Miller block at most (+ the counter).
static int ensure_partials(blsgpu_ctx* c, size_t partials) {
    for (BufId b : {B_PART0, B_PART1})
        if (int rc = c->grow(b, partials * BLSGPU_FQ12_BYTES)) return rc;
    return c->grow(B_DEGEN, pairing::degen_bytes(c->part_cap()));
}

// fixed-exponent powers on a stage image (blsgpu_h2c.hip)
static int launch_pow(blsgpu_ctx* c, uint32_t* img, uint32_t img_slots, uint32_t base_off, uint32_t acc_off, size_t teams, uint32_t cnt,
                      hipStream_t st) {
    size_t total = teams * cnt;
    if (total <= c->pow2_max)          // a batch that leaves SIMDs empty: two wavefronts per 64 values (the squarings a chain of their own)
        hipLaunchKernelGGL(blsgpu::k_pow2, dim3((unsigned)((total + 127) / 128)), dim3(256), 0, st, img, img_slots, base_off, acc_off, cnt,
                           (uint32_t)total);
    else
        hipLaunchKernelGGL(blsgpu::k_pow, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, img, img_slots, base_off, acc_off, cnt,
                           (uint32_t)total);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------ decompression --
namespace {
template <int DEG>
int decompress_dev(blsgpu_ctx* c, const void* d_in, size_t n, void* d_out, void* d_ok, hipStream_t st) {
    using C = blsgpu::DecompCfg<DEG>;
    if (n == 0) return 0;
    StreamGuard sg(c, st);
    if (n > 0x0FFFFFF0ull) return fail(-EINVAL, "batch too large");
    const size_t teams = (n + C::NE - 1) / C::NE;
    size_t need = teams * C::IMG * 12;
    if (int rc_ = c->grow(B_MSM_PART, need * 4)) return rc_;
    uint32_t* img = c->at<uint32_t>(B_MSM_PART);
    const size_t lds = (size_t)C::SLOTS * 48;
    constexpr uint32_t BASE = C::BASE - C::STATE0, ACC = C::ACC - C::STATE0;
    hipLaunchKernelGGL((blsgpu::k_decompress<DEG, 0>), dim3((unsigned)teams), dim3(64), lds, st, c->tabs, (const uint32_t*)d_in,
                       (uint32_t)n, img, (uint32_t*)d_out, (uint8_t*)d_ok);
    HIP_TRY(hipGetLastError());
    int rc = launch_pow(c, img, C::IMG, BASE, ACC, teams, C::NE, st);
    if (rc) return rc;
    if (DEG == 2) {
        hipLaunchKernelGGL((blsgpu::k_decompress<DEG, 1>), dim3((unsigned)teams), dim3(64), lds, st, c->tabs, (const uint32_t*)d_in,
                           (uint32_t)n, img, (uint32_t*)d_out, (uint8_t*)d_ok);
        HIP_TRY(hipGetLastError());
        rc = launch_pow(c, img, C::IMG, BASE, ACC, teams, 2 * C::NE, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL((blsgpu::k_decompress<DEG, 2>), dim3((unsigned)teams), dim3(64), lds, st, c->tabs, (const uint32_t*)d_in,
                       (uint32_t)n, img, (uint32_t*)d_out, (uint8_t*)d_ok);
    HIP_TRY(hipGetLastError());
    return 0;
}
template <int DEG>
int decompress_host(blsgpu_ctx* c, const uint8_t* in, size_t n, uint8_t* out, uint8_t* ok) {
    if (!c || (n && (!in || !out || !ok))) return fail(-EINVAL, "NULL argument");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int din = s.in(in, n * 48 * DEG), dout = s.out(out, n * 96 * DEG), dok = s.out(ok, n);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = decompress_dev<DEG>(c, s.at(din), n, s.at(dout), s.at(dok), nullptr)) return rc;
    return s.down();
}
}  // namespace

// ---------------------------------------------------------------- MSM -------
// Which kernel family serves a sum, and every size, offset, window, chunk and grid of it, is msm_plan.h (host-only: tested without a
// GPU); the functions here grow the two shared buffers to a plan's totals and launch what it says.
namespace {
constexpr int MSM_WAVES = 4;
constexpr msm::Consts MSM_CONSTS = {blsgpu::SRT_LANES, blsgpu::SRT_SCW, blsgpu::SRT_BITADDS, blsgpu::SRT_MAXBITS, blsgpu::SRT_SLICE,
                                    blsgpu::SMUL_T, blsgpu::PIP_W, blsgpu::PIP_NB, blsgpu::L28_AFF, blsgpu::L28_PJ, MSM_WAVES, BLSVM_HMSM2_NP,
                                    {blsgpu::MsmCfg<1>::NP, blsgpu::MsmCfg<2>::NP}, {blsgpu::SrtG<1>::LP, blsgpu::SrtG<2>::LP},
                                    {blsgpu::SrtG<1>::AFF, blsgpu::SrtG<2>::AFF}, {blsgpu::SrtG<1>::PJ, blsgpu::SrtG<2>::PJ}};
static_assert(msm::same(MSM_CONSTS, msm::GFX950), "msm_plan.h: GFX950 (the host test's values) differs from the kernel files");
static_assert(sizeof(msm::SortedPlan::bias) == sizeof(blsgpu::SrtBias), "msm_plan.h: SortedPlan::bias is not SRT_SCW words");
// ... and ragged_plan.h (the range sums, the ragged sums, the short scalars and the signature division below)
constexpr ragged::Consts RAGGED_CONSTS = {blsgpu::pscan::CHUNK, blsgpu::pscan::MID_THREADS, blsgpu::msmr::CHUNK, blsgpu::msmr::SCAN_THREADS};
static_assert(ragged::same(RAGGED_CONSTS, ragged::GFX950), "ragged_plan.h: GFX950 (the host test's values) differs from the kernel files");
// ... and find_plan.h (the three forgery finders below)
static_assert(find::G1 == BLSGPU_G1_BYTES && find::G2 == BLSGPU_G2_BYTES && find::FQ12 == BLSGPU_FQ12_BYTES &&
                  find::NODE_BYTES == sizeof(blsgpu::sigsh::Node) && find::THREADS == blsgpu::sigsh::THREADS &&
                  find::THREADS == blsgpu::bfind::THREADS && find::THREADS == blsgpu::pscan::THREADS && find::G1_Q == blsgpu::bfind::G1_Q &&
                  find::G2_Q == blsgpu::bfind::G2_Q && find::G1_Q == blsgpu::sigsh::G1_Q && find::G2_Q == blsgpu::sigsh::G2_Q,
              "find_plan.h: its constants (the host test's values) differ from blsgpu.h or the kernel files");

// The wide machine's Horner (blsgpu_msmw.hip): list g of `lists` -> sum_i 2^(cbits i) in[g][i], one wavefront per list; AFFINE = 0
// leaves projective sums for the next step, AFFINE = 1 writes the caller's affine point and its infinity flag.
template <int DEG, int AFFINE>
static void horner_wide(hipStream_t st, size_t lists, const uint32_t* in, uint32_t npts, uint32_t cbits, uint32_t* out, uint8_t* out_inf) {
    hipLaunchKernelGGL((blsgpu::msmw::k_msm_horner_wide<DEG, AFFINE>), dim3((unsigned)lists), dim3(64), 0, st, in, npts, cbits, out, out_inf);
}

// the fold levels of a sorted or a plain sum in the workspace W
template <int DEG>
static int run_folds(hipStream_t st, uint32_t* W, const msm::Fold* fold, int nfolds) {
    for (const msm::Fold* f = fold; f != fold + nfolds; f++) {
        if (f->kernel == msm::F_HORNER_WIDE)
            horner_wide<DEG, 0>(st, f->ftotal, W + f->src, f->npts, 0u, W + f->dst, nullptr);
        else if (f->kernel == msm::F_SRT_FOLD)
            hipLaunchKernelGGL(blsgpu::k_srt_fold<DEG>, dim3(f->grid), dim3(64), 0, st, W + f->src, (uint32_t)f->cur, 8u, (uint32_t)f->nfold,
                               (uint32_t)f->ftotal, W + f->dst);
        else
            hipLaunchKernelGGL(blsgpu::k_msm_lane_fold<1>, dim3(f->grid), dim3(64), 0, st, W + f->src, (uint32_t)f->cur, 8u, (uint32_t)f->nfold,
                               (uint32_t)f->ftotal, W + f->dst, f->last);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// One sum with scalars by sorted buckets (blsgpu_msm.hip, k_srt_*; G1 a unit per lane, G2 per lane pair): enqueues on `st` and
// returns, like every _dev path (no synchronisation, usable under stream capture).  Returns 1 only when the key list would not fit
// 32 bits; the caller then takes the fixed-window path.
template <int DEG>
static int msm_sorted(blsgpu_ctx* c, const void* d_pts, const void* d_scalars, size_t n, void* d_out, void* d_out_inf, hipStream_t st) {
    const msm::SortedPlan p = msm::plan_sorted(*c, MSM_CONSTS, DEG, n);
    if (p.bad_bits) return fail(-EINVAL, "BLSGPU_MSM_SORT_BITS out of range");
    if (p.not_me) return 1;
    if (int rc_ = c->grow(B_BUCKETS, p.words * 4)) return rc_;
    uint32_t* W = c->at<uint32_t>(B_BUCKETS);
    HIP_TRY(hipMemsetAsync(W + p.o_cnt, 0, p.nkeys * 4, st));
    HIP_TRY(hipMemsetAsync(W + p.o_long, 0, 16, st));        // counter of the long runs (the key list follows it)
    uint8_t* live = (uint8_t*)(W + p.o_live);
    blsgpu::SrtBias bias;
    memcpy(bias.w, p.bias, sizeof(bias.w));
    const uint32_t cb = p.cb, kb = p.kb, nwin = p.nwin, nkeys = (uint32_t)p.nkeys, units = (uint32_t)p.units;
    hipLaunchKernelGGL(blsgpu::k_srt_prep<DEG>, dim3(p.g_prep), dim3(256), 0, st, (const uint32_t*)d_pts, (const uint32_t*)d_scalars, (uint32_t)n,
                       bias, W + p.o_prep, live, W + p.o_rec);
    HIP_TRY(hipGetLastError());
    const uint32_t* sc = W + p.o_rec;
    const dim3 sgrid(p.g_slices, nwin);
    hipLaunchKernelGGL(blsgpu::k_srt_count, sgrid, dim3(1024), 0, st, sc, live, (uint32_t)n, cb, W + p.o_cnt);
    hipLaunchKernelGGL(blsgpu::k_srt_scan_window, dim3(nwin), dim3(1024), 0, st, W + p.o_cnt, kb, W + p.o_start, W + p.o_wtot, W + p.o_wtot + nwin);
    hipLaunchKernelGGL(blsgpu::k_srt_scan_add, dim3(nwin), dim3(1024), 0, st, nwin, kb, W + p.o_wtot, W + p.o_wtot + nwin, W + p.o_start, W + p.o_cur,
                       W + p.o_max);
    HIP_TRY(hipGetLastError());
    // No read-back, no host decision (round 3): whatever the digit distribution, a long run is finished by a wavefront of
    // k_srt_fix_long -- all-equal scalars cost ~100 additions per lane there (a millisecond), and only a batch whose scalars
    // leave all windows but one empty is slow (still correct, and still faster than the fixed windows it used to fall back to).
    hipLaunchKernelGGL(blsgpu::k_srt_scatter, sgrid, dim3(1024), 0, st, sc, live, (uint32_t)n, cb, W + p.o_cur, W + p.o_idx);
    hipLaunchKernelGGL(blsgpu::k_srt_accum<DEG>, dim3(p.g_accum), dim3(64), 0, st, W + p.o_prep, W + p.o_idx, W + p.o_start, nkeys, units,
                       W + p.o_bsum, W + p.o_hp, W + p.o_hk);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(blsgpu::k_srt_fix<DEG>, dim3(p.g_fix), dim3(64), 0, st, W + p.o_start, nkeys, units, W + p.o_hp, W + p.o_hk, W + p.o_bsum,
                       W + p.o_long, W + p.o_long + 4);
    hipLaunchKernelGGL(blsgpu::k_srt_fix_long<DEG>, dim3(1024), dim3(64), 0, st, W + p.o_start, nkeys, units, W + p.o_hp, W + p.o_bsum, W + p.o_long,
                       W + p.o_long + 4);
    hipLaunchKernelGGL(blsgpu::k_srt_bits<DEG>, dim3(p.g_bits), dim3(64), 0, st, W + p.o_bsum, nwin, cb, (uint32_t)p.btotal, W + p.o_b0);
    HIP_TRY(hipGetLastError());
    if (p.pass5)                                              // (5-bit windows: nothing to fold, but the VM's tail reads its own form)
        hipLaunchKernelGGL(blsgpu::k_msm_lane_fold<1>, dim3(p.g_pass5), dim3(64), 0, st, W + p.o_b0, 1u, 1u, 1u, (uint32_t)p.nsum, W + p.o_b1, 1u);
    if (int rc_ = run_folds<DEG>(st, W, p.fold, p.nfolds)) return rc_;
    if (p.wide) {
        // W_w = sum_b 2^b S_(w,b), one wavefront per window; then sum_w 2^(cb w) W_w on one wavefront
        horner_wide<DEG, 0>(st, nwin, W + p.src, cb, 1u, W + p.o_win, nullptr);
        horner_wide<DEG, 1>(st, 1, W + p.o_win, nwin, cb, (uint32_t*)d_out, (uint8_t*)d_out_inf);
    } else {
        hipLaunchKernelGGL(blsgpu::k_srt_windows, dim3(nwin), dim3(64), (size_t)blsgpu::TEAM_BYTES, st, c->tabs, W + p.src, cb, W + p.o_win);
        hipLaunchKernelGGL(blsgpu::k_msm_pip_horner<1>, dim3(1), dim3(64), (size_t)blsgpu::TEAM_BYTES, st, c->tabs, W + p.o_win, nwin, cb,
                           (uint32_t*)d_out, (uint8_t*)d_out_inf);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// One plain sum of n points (no scalars) -- BLS.aggregate_pub_keys / aggregate_sigs without exponents (bls.py:203-261): a chunk of
// the list per unit (k_sum_chunks: complete mixed additions in registers), the fold levels, then the last run with the affine
// conversion.  Enqueues on `st` and returns.
template <int DEG>
static int msm_plain(blsgpu_ctx* c, const void* d_pts, size_t n, void* d_out, void* d_out_inf, hipStream_t st) {
    const msm::PlainPlan p = msm::plan_plain(MSM_CONSTS, DEG, n);
    if (int rc_ = c->grow(B_BUCKETS, p.words * 4)) return rc_;
    uint32_t* W = c->at<uint32_t>(B_BUCKETS);
    uint8_t* live = (uint8_t*)(W + p.o_live);
    hipLaunchKernelGGL(blsgpu::k_lane_prep<DEG>, dim3(p.g_prep), dim3(256), 0, st, (const uint32_t*)d_pts, (uint32_t)n, W + p.o_prep, live);
    hipLaunchKernelGGL(blsgpu::k_sum_chunks<DEG>, dim3(p.g_chunks), dim3(64), 0, st, W + p.o_prep, live, (uint32_t)n, (uint32_t)p.chunk, (uint32_t)p.U,
                       W + p.o_b0);
    HIP_TRY(hipGetLastError());
    if (int rc_ = run_folds<DEG>(st, W, p.fold, p.nfolds)) return rc_;
    horner_wide<DEG, 1>(st, 1, W + p.src, p.last_n, 0u, (uint32_t*)d_out, (uint8_t*)d_out_inf);
    HIP_TRY(hipGetLastError());
    return 0;
}

// A batch of scalar multiplications / of small sums with scalars: one group per unit (k_smul).  Enqueues on `st` and returns.
template <int DEG>
static int msm_small_groups(blsgpu_ctx* c, const void* d_pts, const void* d_scalars, size_t k, size_t groups, void* d_out, void* d_out_inf, hipStream_t st) {
    const msm::SmallPlan p = msm::plan_small_groups(*c, MSM_CONSTS, DEG, k, groups);
    if (c->grow(B_BUCKETS, p.words * 4)) {
        (void)hipGetLastError();
        return 1;                                              // no room: the caller's other kernels
    }
    uint32_t* W = c->at<uint32_t>(B_BUCKETS);
    uint8_t* live = (uint8_t*)(W + p.o_live);
    for (size_t lo = 0; lo < groups; lo += p.slice) {
        const msm::SmallSlice s = p.at(lo);
        hipLaunchKernelGGL(blsgpu::k_lane_prep<DEG>, dim3(s.g_prep), dim3(256), 0, st, (const uint32_t*)d_pts + s.pts, (uint32_t)s.n, W + p.o_prep, live);
        hipLaunchKernelGGL(blsgpu::k_smul<DEG>, dim3(s.g_smul), dim3(64), 0, st, W + p.o_prep, live, (const uint32_t*)d_scalars + s.scalars,
                           (uint32_t)k, (uint32_t)s.m, W + p.o_tab, (uint32_t*)d_out + s.out, d_out_inf ? (uint8_t*)d_out_inf + lo : nullptr);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// The bucket method: one large sum is cut into chunks, a batch of sums uses one chunk per group; buckets in LDS (k_msm_pip) or one
// (group, chunk, window) per lane with the buckets in HBM (k_msm_lane / k_msm_lane2x).
template <int DEG>
static int msm_bucket(blsgpu_ctx* c, const void* d_pts, const void* d_scalars, size_t k, size_t groups, void* d_out, void* d_out_inf, hipStream_t st) {
    using P = blsgpu::PipCfg<DEG>;
    const msm::BucketPlan p = msm::plan_bucket(*c, MSM_CONSTS, DEG, k, groups);
    if (int rc_ = c->grow(B_MSM_PART, p.part_words * 4)) return rc_;
    uint32_t* const d_part = c->at<uint32_t>(B_MSM_PART);
    uint32_t *d_win = d_part + p.o_win, *d_prep = d_part + p.o_prep;
    if (p.lane_path) {
        uint8_t* d_live = (uint8_t*)(d_part + p.o_live);
        hipLaunchKernelGGL(blsgpu::k_lane_prep<DEG>, dim3(p.g_prep), dim3(256), 0, st, (const uint32_t*)d_pts, (uint32_t)p.n, d_prep, d_live);
        HIP_TRY(hipGetLastError());
        if (int rc_ = c->grow(B_BUCKETS, p.bucket_words * 4)) return rc_;
        uint32_t* const d_buckets = c->at<uint32_t>(B_BUCKETS);
        if (p.pairs)
            hipLaunchKernelGGL(blsgpu::k_msm_lane2x, dim3(p.g_lane), dim3(64), 0, st, d_prep, d_live, (const uint32_t*)d_scalars, (uint32_t)k,
                               (uint32_t)p.chunk, (uint32_t)p.chunks, (uint32_t)p.lanes, d_buckets, d_part, p.lane_last);
        else
            hipLaunchKernelGGL(blsgpu::k_msm_lane<DEG>, dim3(p.g_lane), dim3(64), 0, st, d_prep, d_live, (const uint32_t*)d_scalars, (uint32_t)k,
                               (uint32_t)p.chunk, (uint32_t)p.chunks, (uint32_t)p.lanes, d_buckets, d_part, p.lane_last);
        HIP_TRY(hipGetLastError());
        if (p.tail == msm::T_HORNER_QUADS) {
            const WaveShape ws = wave_shape(c, p.quad_waves);
            hipLaunchKernelGGL(blsgpu::k_msm_horner_quads, dim3(ws.blocks), dim3(ws.threads), 0, st, d_part,
                               (uint32_t)blsgpu::PIP_W, (uint32_t)blsgpu::PIP_C, (uint32_t)groups, (uint32_t*)d_out, (uint8_t*)d_out_inf);
            HIP_TRY(hipGetLastError());
            return 0;
        }
        const uint32_t* winsrc = d_part;
        if (p.fold_n) {                                      // many chunks: fold runs of 64 partials per lane first
            uint32_t* d_fold = d_buckets + p.o_fold;
            hipLaunchKernelGGL(blsgpu::k_msm_lane_fold<DEG>, dim3(p.g_fold), dim3(64), 0, st, d_part, (uint32_t)p.chunks, 64u, (uint32_t)p.fold_n,
                               (uint32_t)p.ftotal, d_fold, 1u);
            HIP_TRY(hipGetLastError());
            winsrc = d_fold;
        }
        hipLaunchKernelGGL(blsgpu::k_msm_pip_windows<DEG>, dim3(blsgpu::PIP_W, (unsigned)groups), dim3(64), (size_t)blsgpu::TEAM_BYTES, st,
                           c->tabs, winsrc, (uint32_t)p.wchunks, d_win);
        HIP_TRY(hipGetLastError());
    } else {
        hipLaunchKernelGGL(blsgpu::k_msm_prep<DEG>, dim3(p.g_prep), dim3(MSM_WAVES * 64), (size_t)MSM_WAVES * blsgpu::TEAM_BYTES,
                           st, c->tabs, (const uint32_t*)d_pts, (uint32_t)p.n, d_prep);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(blsgpu::k_msm_pip<DEG>, dim3((unsigned)p.chunks, blsgpu::PIP_W, (unsigned)groups), dim3(64), (size_t)P::SLOTS * 48,
                           st, c->tabs, d_prep, (const uint32_t*)d_scalars, (uint32_t)k, (uint32_t)p.chunk, d_part);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(blsgpu::k_msm_pip_windows<DEG>, dim3(blsgpu::PIP_W, (unsigned)groups), dim3(64), (size_t)blsgpu::TEAM_BYTES, st,
                           c->tabs, d_part, (uint32_t)p.chunks, d_win);
        HIP_TRY(hipGetLastError());
    }
    if (p.tail == msm::T_HORNER_NP) {                        // a batch of G2 sums: BLSVM_HMSM2_NP sums per team
        hipLaunchKernelGGL(blsgpu::k_msm_horner_np, dim3(p.g_np), dim3(64),
                           (size_t)BLSVM_HMSM2_SLOTS * 48, st, c->tabs, d_win, (uint32_t)blsgpu::PIP_W, (uint32_t)blsgpu::PIP_C,
                           (uint32_t)groups, (uint32_t*)d_out, (uint8_t*)d_out_inf);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(blsgpu::k_msm_pip_horner<DEG>, dim3((unsigned)groups), dim3(64), (size_t)blsgpu::TEAM_BYTES, st, c->tabs, d_win,
                       (uint32_t)blsgpu::PIP_W, (uint32_t)blsgpu::PIP_C, (uint32_t*)d_out, (uint8_t*)d_out_inf);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Double-and-add on the wavefront VM: every sum the other families do not serve.
template <int DEG>
static int msm_vm(blsgpu_ctx* c, const void* d_pts, const void* d_scalars, size_t k, size_t groups, void* d_out, void* d_out_inf, hipStream_t st) {
    const msm::VmPlan p = msm::plan_vm(MSM_CONSTS, DEG, k, groups);
    if (int rc_ = c->grow(B_MSM_PART, p.words * 4)) return rc_;
    size_t lds = (size_t)MSM_WAVES * blsgpu::TEAM_BYTES;
    hipLaunchKernelGGL(blsgpu::k_msm<DEG>, dim3((unsigned)p.blocks), dim3(MSM_WAVES * 64), lds, st, c->tabs,
                       (const uint32_t*)d_pts, (const uint32_t*)d_scalars, (uint32_t)k, (uint32_t)p.chunk, (uint32_t)p.bpg,
                       c->at<uint32_t>(B_MSM_PART));
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(blsgpu::k_msm_finish<DEG>, dim3((unsigned)p.fblocks), dim3(MSM_WAVES * 64), lds, st, c->tabs,
                       c->at<uint32_t>(B_MSM_PART), (uint32_t)p.bpg, (uint32_t)groups, (uint32_t*)d_out, (uint8_t*)d_out_inf);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int DEG>
int msm_dev(blsgpu_ctx* c, const void* d_pts, const void* d_scalars, size_t k, size_t groups, void* d_out,
            void* d_out_inf, hipStream_t st) {
    if (groups == 0) return 0;
    StreamGuard sg(c, st);
    if (msm::too_large(k, groups)) return fail(-EINVAL, "msm too large");
    // a route that answers 1 is not the one ("not me": msm_plan.h); the next one is asked
    for (msm::Route r = msm::START; (r = msm::next_route(*c, DEG, k, groups, d_scalars != nullptr, r)) != msm::END;) {
        int rc_ = 1;
        switch (r) {
        case msm::EMPTY:                            // empty sums: infinity
            HIP_TRY(hipMemsetAsync(d_out, 0, groups * 96 * DEG, st));
            if (d_out_inf) HIP_TRY(hipMemsetAsync(d_out_inf, 1, groups, st));
            return 0;
        case msm::PLAIN: rc_ = msm_plain<DEG>(c, d_pts, k, d_out, d_out_inf, st); break;
        case msm::SMALL_GROUPS: rc_ = msm_small_groups<DEG>(c, d_pts, d_scalars, k, groups, d_out, d_out_inf, st); break;
        case msm::SORTED: rc_ = msm_sorted<DEG>(c, d_pts, d_scalars, k, d_out, d_out_inf, st); break;
        case msm::BUCKET_VM:
        case msm::BUCKET_LANE: rc_ = msm_bucket<DEG>(c, d_pts, d_scalars, k, groups, d_out, d_out_inf, st); break;
        default: rc_ = msm_vm<DEG>(c, d_pts, d_scalars, k, groups, d_out, d_out_inf, st);
        }
        if (rc_ != 1) return rc_;
    }
    return fail(-EINVAL, "msm: no route");          // (not reached: VM serves every call)
}

template <int DEG>
int msm_host(blsgpu_ctx* c, const uint8_t* pts, const uint8_t* scalars, size_t k, size_t groups, uint8_t* out,
             uint8_t* out_inf) {
    if (!c || !out) return fail(-EINVAL, "NULL argument");
    size_t n = k * groups;
    if (n && !pts) return fail(-EINVAL, "NULL point buffer");
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int dp = s.in(pts, n * 96 * DEG), ds = s.in(scalars, n * 32), dout = s.out(out, groups * 96 * DEG), dinf = s.out_kept(out_inf, groups);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = msm_dev<DEG>(c, s.at(dp), s.opt(ds), k, groups, s.at(dout), s.at(dinf), 0)) return rc;
    return s.down();
}

// ------------------------------------------------------------ fixed-base G1, HD derivation (blsgpu_g1fix.hip, keys_plan.h) --
using keys::FIX_SLICE;
using keys::FIX_HOST_SLICE;
constexpr keys::Consts KEYS_CONSTS = {blsgpu::g2smul::SLICE, blsgpu::g2smul::PAIRS, blsgpu::g2smul::TABLE_DW, blsgpu::frsec::SUM_THREADS,
                                      blsgpu::frsec::EVAL_THREADS, blsgpu::g1poly::ENTRY_DW, blsgpu::seeds::PARENT_DW, blsgpu::lagr::MAX_K,
                                      BLSGPU_HD_PARENT_BYTES};
static_assert(keys::same(KEYS_CONSTS, keys::GFX950), "keys_plan.h: GFX950 (the host test's values) differs from the kernel files");
static_assert(keys::G1 == BLSGPU_G1_BYTES && keys::G2 == BLSGPU_G2_BYTES, "keys_plan.h: the point sizes");
// blsgpu_keys_from_seeds' staged slice is never zero: the longest seed and its outputs fit the staging target many times
static_assert(keys::STAGE_TARGET / keys::seeds_item_bytes(BLSGPU_SEED_MAX_BYTES) >= 1, "keys_plan.h: staged_fit of the seeds form");

// G1, ec.py:394-396 (little-endian words)
blsgpu::g1fix::Gen g1_generator() {
    return {{0xdb22c6bbu, 0xfb3af00au, 0xf97a1aefu, 0x6c55e83fu, 0x171bac58u, 0xa14e3a3fu, 0x9774b905u, 0xc3688c4fu, 0x4fa9ac0fu,
                    0x2695638cu, 0x3197d794u, 0x17f1d3a7u},
                   {0x46c5e7e1u, 0x0caa2329u, 0xa2888ae4u, 0xd03cc744u, 0x2c04b3edu, 0x00db18cbu, 0xd5d00af6u, 0xfcf5e095u, 0x741d8ae4u,
                    0xa09e30edu, 0xe3aaa0f1u, 0x08b3f481u}};
}

// a context's table, built on `st` the first time it is needed: d 2^(8w) G1 for k_fix_mul (fix_sum), or `secret`: the
// (e + 1) 16^w G1 that k_fix_mul_secret reads whole, window by window
int fix_table(blsgpu_ctx* c, hipStream_t st, bool secret = false) {
    using namespace blsgpu::g1fix;
    uint32_t*& slot = secret ? c->d_fix_table_secret : c->d_fix_table;
    if (slot) return 0;
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, secret ? S_TABLE_BYTES : TABLE_BYTES));
    if (secret)
        hipLaunchKernelGGL(k_fix_table_t<4>, dim3((S_ENTRIES + 63) / 64), dim3(64), 0, st, g1_generator(), (uint32_t*)p);
    else
        hipLaunchKernelGGL(k_fix_table_t<8>, dim3((ENTRIES + 63) / 64), dim3(64), 0, st, g1_generator(), (uint32_t*)p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        (void)hipFree(p);
        return fail(-EIO, std::string(secret ? "k_fix_table_secret: " : "k_fix_table: ") + hipGetErrorString(e));
    }
    slot = (uint32_t*)p;
    return 0;
}

int check_n_add(size_t n, size_t n_add, const void* add) {
    if (n_add != 0 && n_add != 1 && n_add != n) return fail(-EINVAL, "n_add must be 0, 1 or n");
    if (n_add && !add) return fail(-EINVAL, "NULL add buffer");
    return 0;
}

// an optional array of the caller at a plan's offset: NULL stays NULL
uint32_t* at_words(void* d, size_t words) { return d ? (uint32_t*)d + words : nullptr; }
char* at_bytes(void* d, size_t bytes) { return d ? (char*)d + bytes : nullptr; }

// enqueues out_i = s_i G1 (+ A) on `st` (caller: StreamGuard, table built)
int fix_mul_launch(blsgpu_ctx* c, const void* d_scalars, size_t n, const void* d_add, size_t n_add, void* d_out_aff, void* d_out_ser,
                   hipStream_t st) {
    const bool per = n_add == n && n_add > 1;
    const size_t step = keys::fix_step(*c);
    return for_slices(n, step, [&](size_t lo, size_t) {
        const keys::FixAt a = keys::fix_at(n, step, lo);
        hipLaunchKernelGGL(blsgpu::g1fix::k_fix_mul, dim3(a.grid), dim3(256), 0, st, (const uint32_t*)c->d_fix_table,
                           (const uint32_t*)d_scalars + a.scalars, (uint32_t)a.m, n_add ? (const uint32_t*)d_add + (per ? a.add : 0) : nullptr,
                           per ? 1u : 0u, at_words(d_out_aff, a.aff), at_words(d_out_ser, a.ser));
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

// enqueues out_i = s_i G1 on the scalar-independent schedule on `st` (caller: StreamGuard, fix_table(secret))
int fix_mul_secret_launch(blsgpu_ctx* c, const void* d_scalars, size_t n, void* d_out_aff, void* d_out_ser, hipStream_t st) {
    KernelTimer kt(c, st, 9);
    const size_t step = keys::fix_step(*c);
    return for_slices(n, step, [&](size_t lo, size_t) {
        const keys::FixAt a = keys::fix_at(n, step, lo);
        hipLaunchKernelGGL(blsgpu::g1fix::k_fix_mul_secret, dim3(a.grid), dim3(256), 0, st, (const uint32_t*)c->d_fix_table_secret,
                           (const uint32_t*)d_scalars + a.scalars, (uint32_t)a.m, at_words(d_out_aff, a.aff), at_words(d_out_ser, a.ser));
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

int g1_mul_gen_secret_dev(blsgpu_ctx* c, const void* d_scalars, size_t n, void* d_out_aff, void* d_out_ser, hipStream_t st) {
    if (n == 0) return 0;
    if (!d_scalars || (!d_out_aff && !d_out_ser)) return fail(-EINVAL, "NULL argument");
    StreamGuard sg(c, st);
    if (int rc = fix_table(c, st, true)) return rc;
    return fix_mul_secret_launch(c, d_scalars, n, d_out_aff, d_out_ser, st);
}

int g1_mul_gen_dev(blsgpu_ctx* c, const void* d_scalars, size_t n, const void* d_add, size_t n_add, void* d_out_aff, void* d_out_ser,
                   hipStream_t st) {
    if (n == 0) return 0;
    if (!d_scalars) return fail(-EINVAL, "NULL scalar buffer");
    if (int rc = check_n_add(n, n_add, d_add)) return rc;
    StreamGuard sg(c, st);
    if (int rc = fix_table(c, st)) return rc;
    return fix_mul_launch(c, d_scalars, n, d_add, n_add, d_out_aff, d_out_ser, st);
}

uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
// y > q // 2 for 48 big-endian bytes
bool y_gt_half_q(const uint8_t y[48]) {
    uint32_t w[12];
    for (int j = 0; j < 12; j++) w[11 - j] = be32(y + 4 * j);
    return bls::gt_half_q_mask(w) != 0;
}

// the per-call constants of a parent: HMAC midstates of the chain code, PublicKey.serialize() of the parent key
// (ec.py:94-111; (0, 0) -> 48 zero bytes), and for private derivation its key's bytes and value mod n
blsgpu::g1fix::HdParent hd_parent(const uint8_t chain_code[32], const uint8_t parent_pk_aff[96], const uint8_t* parent_sk) {
    blsgpu::g1fix::HdParent P;
    memset(&P, 0, sizeof(P));
    hdk::hmac_key(chain_code, 32, P.key);
    for (int j = 0; j < 12; j++) P.pk_ser[j] = be32(parent_pk_aff + 4 * j);
    if (y_gt_half_q(parent_pk_aff + 48)) P.pk_ser[0] |= 0x80000000u;
    if (parent_sk) {
        for (int j = 0; j < 8; j++) { P.sk_ser[j] = be32(parent_sk + 4 * j); P.sk[7 - j] = P.sk_ser[j]; }
        hdk::reduce_n(P.sk);
        P.priv = 1;
    }
    return P;
}

// The validity scans of the _dev forms: clears the flag word, runs `launch` (which enqueues the scan kernel on `st`) and
// reads the word back -- one synchronisation, before anything is written
template <class F>
int scan_flag(void* d_flag, hipStream_t st, uint32_t& flag, F launch) {
    HIP_TRY(hipMemsetAsync(d_flag, 0, 4, st));
    launch((uint32_t*)d_flag);
    HIP_TRY(hipGetLastError());
    flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// The rounds of a bisecting check on `st` (bisect::run owns the loop).  `round(nodes, len, d_verdict)` enqueues one round -- it may
// reorder `nodes` first -- and names the device bytes that get one verdict per node, in the order of `nodes`; they come back here,
// the one synchronisation of a round.  What a round uploads asynchronously from the host is `nodes` itself or storage that only
// `round` writes: nothing touches `nodes` between a round and its synchronisation, and `round` runs again only after it.
template <class N, class Round>
int bisect_rounds(bisect::State<N>& b, size_t top, size_t limit, hipStream_t st, Round round) {
    return bisect::run(b, top, limit, [&](std::vector<N>& nodes, size_t len, uint8_t* verdict) {
        const void* d_verdict = nullptr;
        if (int rc = round(nodes, len, d_verdict)) return rc;
        HIP_TRY(hipMemcpyAsync(verdict, d_verdict, nodes.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return 0;
    });
}
// the validity scan of the three checks' _dev forms: key_idx < n_keys and, with d_msg_idx, msg_idx < n_msgs (bit 0 of `bad`)
// over n entries in launches of FIX_SLICE; `mono`: that msg_idx does not decrease as well (another bit)
int scan_indices(blsgpu_ctx* c, void* d_flag, const void* d_key_idx, size_t n_keys, const void* d_msg_idx, size_t n_msgs, size_t n, bool mono,
                 uint32_t& bad, hipStream_t st) {
    const size_t FS = keys::fix_step(*c);
    return scan_flag(d_flag, st, bad, [&](uint32_t* flag) {
        for (size_t lo = 0; lo < n; lo += FS) {
            const size_t m = keys::run_len(n, FS, lo);
            const dim3 grid(keys::blocks(m));
            hipLaunchKernelGGL(blsgpu::g1poly::k_poly_check, grid, dim3(256), 0, st, (const uint32_t*)d_key_idx + lo, (uint32_t)m,
                               (uint32_t)n_keys, flag);
            if (d_msg_idx)
                hipLaunchKernelGGL(blsgpu::g1poly::k_poly_check, grid, dim3(256), 0, st, (const uint32_t*)d_msg_idx + lo, (uint32_t)m,
                                   (uint32_t)n_msgs, flag);
            if (mono)
                hipLaunchKernelGGL(blsgpu::pscan::k_fold_mono, grid, dim3(256), 0, st, (const uint32_t*)d_msg_idx, (uint32_t)lo, (uint32_t)m, flag);
        }
    });
}

// n children of one parent on `st`; public mode (parent_sk NULL) with `check`: a device scan of the indices and one
// synchronising read of its flag first, -EINVAL before anything is written if one is hardened
int hd_children_dev(blsgpu_ctx* c, const uint8_t chain_code[32], const uint8_t parent_pk_aff[96], const uint8_t* parent_sk, const void* d_idx,
                    size_t n, void* d_chain, void* d_sk, void* d_pk_aff, void* d_pk_ser, bool check, hipStream_t st) {
    if (n == 0) return 0;
    if (!chain_code || !parent_pk_aff || !d_idx || !d_chain) return fail(-EINVAL, "NULL argument");
    if (parent_sk && !d_sk) return fail(-EINVAL, "private derivation needs out_sk");
    if (keys::too_many_lanes(n)) return fail(-EINVAL, "batch too large");
    const blsgpu::g1fix::HdParent P = hd_parent(chain_code, parent_pk_aff, parent_sk);
    StreamGuard sg(c, st);
    const bool pub = parent_sk == nullptr;
    const keys::ChildrenPlan p = keys::plan_children(*c, n, pub);
    if (int rc = c->grow(B_FIX_WS, p.bytes)) return rc;
    char* ws = c->at<char>(B_FIX_WS);
    if (pub && check) {
        uint32_t flag;
        if (int rc = scan_flag(ws + p.o_flag, st, flag, [&](uint32_t* d_flag) {
                hipLaunchKernelGGL(blsgpu::g1fix::k_hd_check, dim3(keys::blocks(n)), dim3(256), 0, st, (const uint32_t*)d_idx, (uint32_t)n, d_flag);
            }))
            return rc;
        if (flag) return fail(-EINVAL, "Cannot derive hardened children from public key");
    }
    const bool pk_out = d_pk_aff || d_pk_ser;
    if (pk_out) {
        if (int rc = fix_table(c, st)) return rc;
    }
    if (pub) HIP_TRY(hipMemcpyAsync(ws + p.o_parent, parent_pk_aff, 96, hipMemcpyHostToDevice, st));
    return for_slices(n, p.step, [&](size_t lo, size_t) {
        const keys::ChildrenAt a = p.at(lo);
        uint32_t* scal = pub ? (uint32_t*)(ws + p.o_ileft) : (uint32_t*)d_sk + a.sk;
        hipLaunchKernelGGL(blsgpu::g1fix::k_hd_hmac, dim3(a.grid), dim3(256), 0, st, P, (const uint32_t*)d_idx + a.idx, (uint32_t)a.m,
                           (uint32_t*)d_chain + a.chain, scal);
        HIP_TRY(hipGetLastError());
        if (!pk_out) return 0;
        return fix_mul_launch(c, scal, a.m, pub ? ws + p.o_parent : nullptr, pub ? 1 : 0, at_bytes(d_pk_aff, a.aff), at_bytes(d_pk_ser, a.ser), st);
    });
}
// blsgpu_hd_paths*: the arguments every form checks before anything is written (after n == 0)
int hd_paths_args(const void* parents, size_t n_parents, int priv, const void* indices, size_t depth, size_t n, const void* chain,
                  const void* sk, const void* aff, const void* ser) {
    if (depth == 0 || depth > 255) return fail(-EINVAL, "depth must be 1 .. 255");
    if (n_parents == 0) return fail(-EINVAL, "no parent records");
    if (!parents || !indices || !chain) return fail(-EINVAL, "NULL argument");
    if (priv && !sk) return fail(-EINVAL, "private derivation needs out_sk");
    if (!aff && !ser) return fail(-EINVAL, "ask for out_pk_aff or out_pk_ser");
    if (keys::hd_paths_too_large(n, n_parents)) return fail(-EINVAL, "batch too large");
    return 0;
}

// n paths of `depth` levels on `st`, every buffer in device memory: per slice and level k_hd_path_hmac, then k_fix_mul, over
// the state of one slice in B_HDP_WS (keys::PathsPlan).
// `check`: the device scan of parent_of and (public mode) the indices and one synchronising read of its flag first.
// `secret` (private mode only, blsgpu_hd_paths_secret): k_hd_path_hmac_secret and k_fix_mul_secret in their places.
int hd_paths_dev(blsgpu_ctx* c, const void* d_parents, size_t n_parents, int priv, const void* d_parent_of, const void* d_idx, size_t depth,
                 size_t n, void* d_chain, void* d_sk, void* d_pk_aff, void* d_pk_ser, void* d_fp, bool check, hipStream_t st,
                 bool secret = false) {
    using namespace blsgpu::g1fix;
    if (n == 0) return 0;
    if (int rc = hd_paths_args(d_parents, n_parents, priv, d_idx, depth, n, d_chain, d_sk, d_pk_aff, d_pk_ser)) return rc;
    StreamGuard sg(c, st);
    const keys::PathsPlan p = keys::plan_paths(*c, n, depth, priv != 0);
    if (int rc = c->grow(B_HDP_WS, p.bytes)) return rc;
    char* ws = c->at<char>(B_HDP_WS);
    if (check && (d_parent_of || !priv)) {
        uint32_t flag;
        if (int rc = scan_flag(ws + p.o_flag, st, flag, [&](uint32_t* d_flag) {
                hipLaunchKernelGGL(k_hd_path_check, dim3(keys::blocks(n)), dim3(256), 0, st, (const uint32_t*)d_parent_of, (uint32_t)n_parents,
                                   (const uint32_t*)d_idx, (uint32_t)depth, priv ? 0u : 1u, (uint32_t)n, d_flag);
            }))
            return rc;
        if (flag & 2u) return fail(-EINVAL, "parent index out of range");
        if (flag & 1u) return fail(-EINVAL, "Cannot derive hardened children from public key");
    }
    if (int rc = fix_table(c, st, secret)) return rc;
    uint32_t* ws_chain = (uint32_t*)(ws + p.o_chain);
    uint32_t* ws_scal = (uint32_t*)(ws + p.o_scal);
    uint32_t* ws_aff[2] = {(uint32_t*)(ws + p.o_aff[0]), (uint32_t*)(ws + p.o_aff[1])};
    const uint32_t* par = (const uint32_t*)d_parents;
    return for_slices(n, p.S, [&](size_t lo, size_t m) {
        const keys::PathsAt a = p.at(lo);
        int cur = 0;                                                       // ws_aff[cur]: the keys the next level derives from
        for (size_t l = 0; l < depth; l++) {
            const bool first = l == 0, last = l + 1 == depth;
            uint32_t* chain_out = last ? (uint32_t*)d_chain + a.chain : ws_chain;
            uint32_t* scal_out = last && priv ? (uint32_t*)d_sk + a.sk : ws_scal;
            hipLaunchKernelGGL(secret ? k_hd_path_hmac_secret : k_hd_path_hmac, dim3(a.grid), dim3(256), 0, st, first ? par : ws_chain,
                               first ? par + 32 : ws_scal, first ? par + 8 : ws_aff[cur], first ? 40u : 0u,
                               d_parent_of ? (const uint32_t*)d_parent_of + a.parent_of : nullptr, first ? 1u : 0u,
                               (const uint32_t*)d_idx + a.idx + l, (uint32_t)depth, (uint32_t)m, priv ? 1u : 0u, chain_out, scal_out,
                               first && !priv ? ws_aff[0] : nullptr, last ? at_words(d_fp, a.fp) : nullptr);
            HIP_TRY(hipGetLastError());
            const int next = priv ? 0 : cur ^ 1;
            void* aff_out = last ? at_bytes(d_pk_aff, a.aff) : (char*)ws_aff[next];
            void* ser_out = last ? at_bytes(d_pk_ser, a.ser) : nullptr;
            if (int rc = secret ? fix_mul_secret_launch(c, scal_out, m, aff_out, ser_out, st)
                                : fix_mul_launch(c, scal_out, m, priv ? nullptr : ws_aff[cur], priv ? 0 : m, aff_out, ser_out, st))
                return rc;
            cur = next;
        }
        return 0;
    });
}
// ------------------------------------------------------------ keys from seeds (blsgpu_seeds.hip) --
// the midstates of the two fixed keys (public constants), computed once: [0] "BLS private key seed", [1] "BLS HD seed"
const hdk::HmacKey& seed_key(int hd) {
    static const struct Keys {
        hdk::HmacKey k[2];
        Keys() {
            hdk::hmac_key((const uint8_t*)"BLS private key seed", 20, k[0]);
            hdk::hmac_key((const uint8_t*)"BLS HD seed", 11, k[1]);
        }
    } keys;
    return keys.k[hd];
}

// blsgpu_keys_from_seeds*: the arguments every form checks before anything is written; 1: nothing to do
int seeds_args(const blsgpu_ctx* c, const void* seeds, size_t seed_len, size_t n, int hd, const void* sk, const void* chain, const void* aff,
               const void* ser, const void* parents) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (hd != 0 && hd != 1) return fail(-EINVAL, "hd must be 0 or 1");
    if (seed_len > BLSGPU_SEED_MAX_BYTES) return fail(-EINVAL, "seeds are at most BLSGPU_SEED_MAX_BYTES bytes");
    if (!hd && (chain || parents)) return fail(-EINVAL, "out_chain and out_parents belong to hd = 1");
    if (n == 0) return 1;
    if (!seeds && seed_len) return fail(-EINVAL, "NULL seed buffer");
    if (!sk && !chain && !aff && !ser && !parents) return fail(-EINVAL, "ask for at least one output");
    if (keys::too_many_lanes(n)) return fail(-EINVAL, "batch too large");
    return 0;
}

// n keys from n seeds of seed_len bytes on `st`, every buffer in device memory (caller: seeds_args): per slice k_seed_keys
// (timing kind 13), then -- when a public key is asked for -- k_fix_mul_secret on the keys where k_seed_keys left them (the
// caller's out_sk or B_SEED_WS, keys::SeedsPlan) and k_seed_pack_aff for the records.
int keys_from_seeds_dev(blsgpu_ctx* c, const void* d_seeds, size_t seed_len, size_t n, int hd, void* d_sk, void* d_chain, void* d_pk_aff,
                        void* d_pk_ser, void* d_parents, hipStream_t st) {
    using namespace blsgpu::seeds;
    StreamGuard sg(c, st);
    const bool pk = d_pk_aff || d_pk_ser || d_parents;
    const keys::SeedsPlan p = keys::plan_seeds(*c, KEYS_CONSTS, seed_len, n, d_sk != nullptr, d_pk_aff != nullptr, d_parents != nullptr);
    if (int rc = c->grow(B_SEED_WS, p.bytes)) return rc;                   // (nothing to hold: nothing grows)
    if (pk) {
        if (int rc = fix_table(c, st, true)) return rc;
    }
    char* ws = c->at<char>(B_SEED_WS);
    return for_slices(n, p.S, [&](size_t lo, size_t) {
        const keys::SeedsAt a = p.at(lo);
        uint32_t* sk = d_sk ? (uint32_t*)d_sk + a.sk : (uint32_t*)(ws + p.o_sk);
        uint32_t* par = at_words(d_parents, a.par);
        {
            KernelTimer kt(c, st, 13);
            hipLaunchKernelGGL(k_seed_keys, dim3(a.grid), dim3(256), 0, st, seed_key(hd), (const uint8_t*)d_seeds + a.seeds, (uint32_t)seed_len,
                               (uint32_t)a.m, (uint32_t)hd, sk, at_words(d_chain, a.chain), par);
            HIP_TRY(hipGetLastError());
        }
        if (!pk) return 0;
        uint32_t* aff = d_pk_aff ? (uint32_t*)d_pk_aff + a.aff : (par ? (uint32_t*)(ws + p.o_aff) : nullptr);
        if (int rc = fix_mul_secret_launch(c, sk, a.m, aff, at_bytes(d_pk_ser, a.ser), st)) return rc;
        if (par) {
            hipLaunchKernelGGL(k_seed_pack_aff, dim3(a.g_pack), dim3(256), 0, st, (const uint32_t*)aff, (uint32_t)a.m, par);
            HIP_TRY(hipGetLastError());
        }
        return 0;
    });
}

// ------------------------------------------------------------ Feldman share checks (blsgpu_g1poly.hip) --
// the arguments every form checks before anything is written (after t == 0 and n == 0)
int poly_args(size_t n_polys, size_t t, const void* commit, const void* poly, const void* x, const void* s, const void* status,
              const void* out_aff) {
    if (!commit || !poly || !x) return fail(-EINVAL, "NULL argument");
    if (!s != !status) return fail(-EINVAL, "s and status must be NULL together");
    if (!status && !out_aff) return fail(-EINVAL, "ask for status or out_aff");
    if (n_polys == 0) return fail(-EINVAL, "polynomial index out of range");
    if (keys::poly_too_many(n_polys, t)) return fail(-EINVAL, "too many commitments");
    return 0;
}

// B_POLY_WS of the call (keys::PolyPlan)
int poly_ws(blsgpu_ctx* c, size_t n_polys, size_t t) { return c->grow(B_POLY_WS, keys::plan_poly(KEYS_CONSTS, n_polys, t).bytes); }

// the commitments of the call, once: L28 entries, then the subgroup flags (caller: StreamGuard, poly_ws); `table`: the
// left-hand sides need the fixed-base table -- `secret`: the signed 4-bit one of k_poly_eval_secret
int poly_prep(blsgpu_ctx* c, const void* d_commit, size_t n_polys, size_t t, bool table, hipStream_t st, bool secret = false) {
    using namespace blsgpu::g1poly;
    if (table) {
        if (int rc = fix_table(c, st, secret)) return rc;
    }
    char* ws = c->at<char>(B_POLY_WS);
    const keys::PolyPlan p = keys::plan_poly(KEYS_CONSTS, n_polys, t);
    uint32_t* l28 = (uint32_t*)(ws + p.o_l28);
    HIP_TRY(hipMemsetAsync(ws + p.o_sub, 0, p.sub_bytes, st));
    hipLaunchKernelGGL(k_poly_prep, dim3(p.g_prep), dim3(256), 0, st, (const uint32_t*)d_commit, (uint32_t)p.m, l28);
    HIP_TRY(hipGetLastError());
    if (t > 1) {
        hipLaunchKernelGGL(k_poly_subgroup, dim3(p.g_sub), dim3(256), 0, st, (const uint32_t*)l28, (uint32_t)n_polys, (uint32_t)t,
                           (uint32_t*)(ws + p.o_sub));
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// n fragments against the prepared commitments, FIX_SLICE per launch (caller: StreamGuard, poly_prep); `secret`:
// k_poly_eval_secret on the signed 4-bit table (timing kind 9, one record per call)
int poly_eval_launch(blsgpu_ctx* c, size_t n_polys, size_t t, const void* d_poly, const void* d_x, const void* d_s, size_t n, void* d_status,
                     void* d_out_aff, hipStream_t st, bool secret = false) {
    char* ws = c->at<char>(B_POLY_WS);
    const keys::PolyPlan p = keys::plan_poly(KEYS_CONSTS, n_polys, t);
    const size_t step = keys::fix_step(*c);
    auto launches = [&]() {
        return for_slices(n, step, [&](size_t lo, size_t) {
            const keys::FixAt a = keys::fix_at(n, step, lo);                // (x and s: scalars; the polynomial index and the status: an entry an item)
            hipLaunchKernelGGL(secret ? blsgpu::g1poly::k_poly_eval_secret : blsgpu::g1poly::k_poly_eval, dim3(a.grid), dim3(256), 0, st,
                               (const uint32_t*)(secret ? c->d_fix_table_secret : c->d_fix_table), (const uint32_t*)(ws + p.o_l28),
                               (const uint32_t*)(ws + p.o_sub), (uint32_t)n_polys, (uint32_t)t, (const uint32_t*)d_poly + lo,
                               (const uint32_t*)d_x + a.scalars, d_s ? (const uint32_t*)d_s + a.scalars : nullptr, (uint32_t)a.m,
                               (uint8_t*)at_bytes(d_status, lo), at_words(d_out_aff, a.aff));
            HIP_TRY(hipGetLastError());
            return 0;
        });
    };
    if (!secret) return launches();
    KernelTimer kt(c, st, 9);
    return launches();
}

// the _dev form: a device scan of the indices and one synchronising read of its flag first (-EINVAL before anything is written)
// (`secret`: blsgpu_g1_poly_check_secret_dev -- s and status are required)
int poly_check_dev(blsgpu_ctx* c, const void* d_commit, size_t n_polys, size_t t, const void* d_poly, const void* d_x, const void* d_s,
                   size_t n, void* d_status, void* d_out_aff, hipStream_t st, bool secret = false) {
    if (t == 0) return fail(-EINVAL, "t must be at least 1");
    if (n == 0) return 0;
    if (secret && (!d_s || !d_status)) return fail(-EINVAL, "s and status are required");
    if (int rc = poly_args(n_polys, t, d_commit, d_poly, d_x, d_s, d_status, d_out_aff)) return rc;
    StreamGuard sg(c, st);
    if (int rc = poly_ws(c, n_polys, t)) return rc;
    uint32_t bad;
    if (int rc = scan_indices(c, c->at<char>(B_POLY_WS) + keys::plan_poly(KEYS_CONSTS, n_polys, t).o_flag, d_poly, n_polys, nullptr, 0, n, false, bad, st))
        return rc;
    if (bad) return fail(-EINVAL, "polynomial index out of range");
    if (int rc = poly_prep(c, d_commit, n_polys, t, d_status != nullptr, st, secret)) return rc;
    return poly_eval_launch(c, n_polys, t, d_poly, d_x, d_s, n, d_status, d_out_aff, st, secret);
}
// ------------------------------------------------------------ subgroup membership (blsgpu_subgroup.hip) --
// n affine points of G1 (g = 1, 96 B each) or G2 (g = 2, 192 B each) -> n status bytes, FIX_SLICE per launch
int subgroup_dev(blsgpu_ctx* c, int g, const void* d_pts, size_t n, void* d_status, hipStream_t st) {
    if (n == 0) return 0;
    if (!d_pts || !d_status) return fail(-EINVAL, "NULL argument");
    StreamGuard sg(c, st);
    const size_t dw = g == 1 ? 24 : 48, FS = slice_len(c, FIX_SLICE);
    for (size_t lo = 0; lo < n; lo += FS) {
        const size_t m = n - lo < FS ? n - lo : FS;
        const dim3 grid((unsigned)((m + 255) / 256));
        const uint32_t* p = (const uint32_t*)d_pts + lo * dw;
        uint8_t* s = (uint8_t*)d_status + lo;
        if (g == 1)
            hipLaunchKernelGGL(blsgpu::subgroup::k_g1_subgroup, grid, dim3(256), 0, st, p, (uint32_t)m, s);
        else
            hipLaunchKernelGGL(blsgpu::subgroup::k_g2_subgroup, grid, dim3(256), 0, st, c->tabs, p, (uint32_t)m, s);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
// the host-buffer form: FIX_HOST_SLICE points per staged slice
int subgroup_host(blsgpu_ctx* c, int g, const uint8_t* pts, size_t n, uint8_t* status) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    if (!pts || !status) return fail(-EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t HS = slice_len(c, FIX_HOST_SLICE), S = n < HS ? n : HS;
    Staging s(c);
    const int dp = s.in(pts, S, g == 1 ? 96 : 192), dst = s.out(status, S, 1);
    if (int rc = s.alloc()) return rc;
    return for_slices(n, S, [&](size_t lo, size_t m) {
        if (int rc = s.up(lo, m)) return rc;
        if (int rc = subgroup_dev(c, g, s.at(dp), m, s.at(dst), nullptr)) return rc;
        return s.down(lo, m);
    });
}
// ------------------------------------------------------------ Lagrange coefficients (blsgpu_lagrange.hip) --
// the argument checks the three entry-point pairs share (before anything is written); 1: nothing to do
int lagrange_args(const blsgpu_ctx* c, size_t k, size_t groups, bool null_buffer) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (keys::bad_k(KEYS_CONSTS, k)) return fail(-EINVAL, "k must be 1 .. BLSGPU_LAGRANGE_MAX_K");
    if (groups == 0) return 1;
    if (null_buffer) return fail(-EINVAL, "NULL argument");
    if (keys::lagrange_too_large(k, groups)) return fail(-EINVAL, "batch too large");
    return 0;
}
// coefficients and status of `groups` groups of k points (checked by lagrange_args), all on the device
int lagrange_launch(blsgpu_ctx* c, const void* d_x, size_t k, size_t groups, void* d_coeffs, void* d_status, hipStream_t st) {
    const keys::LagrShape sh = keys::lagrange_shape((uint32_t)k);
    hipLaunchKernelGGL(blsgpu::lagr::k_lagrange, dim3(sh.grid(groups)), dim3(sh.threads), sh.lds, st, (const uint8_t*)d_x, (uint32_t)k,
                       (uint32_t)groups, sh.gpb, (uint8_t*)d_coeffs, (uint8_t*)d_status);
    HIP_TRY(hipGetLastError());
    return 0;
}
// ... into B_LAGR_WS (caller: StreamGuard)
int lagrange_to_ws(blsgpu_ctx* c, const void* d_x, size_t k, size_t groups, void* d_status, hipStream_t st) {
    if (int rc = c->grow(B_LAGR_WS, keys::coeff_bytes(k, groups))) return rc;
    return lagrange_launch(c, d_x, k, groups, c->at<void>(B_LAGR_WS), d_status, st);
}
// out[g] = sum_j L_j y_j with the coefficients of B_LAGR_WS: k_fr_dot, or `secret`: k_fr_dot_secret's masked sums (timing kind 10)
int fr_interpolate_dev(blsgpu_ctx* c, const void* d_x, const void* d_y, size_t k, size_t groups, void* d_out, void* d_status, hipStream_t st,
                       bool secret = false) {
    StreamGuard sg(c, st);
    if (int rc = lagrange_to_ws(c, d_x, k, groups, d_status, st)) return rc;
    const keys::LagrShape sh = keys::lagrange_shape((uint32_t)k);
    std::optional<KernelTimer> kt;
    if (secret) kt.emplace(c, st, 10);
    hipLaunchKernelGGL(secret ? blsgpu::frsec::k_fr_dot_secret : blsgpu::lagr::k_fr_dot, dim3(sh.grid(groups)), dim3(sh.threads), sh.lds, st,
                       c->at<uint8_t>(B_LAGR_WS), (const uint8_t*)d_y, (uint32_t)k, (uint32_t)groups, sh.gpb, (uint8_t*)d_out);
    HIP_TRY(hipGetLastError());
    return 0;
}
// the coefficients into the workspace, then the G2 sums of blsgpu_g2_msm_dev with them as its device scalars (a group
// with status 0 has all-zero scalars: infinity)
int threshold_combine_dev(blsgpu_ctx* c, const void* d_sigs, const void* d_x, size_t k, size_t groups, void* d_out, void* d_out_inf,
                          void* d_status, hipStream_t st) {
    {
        StreamGuard sg(c, st);
        if (int rc = lagrange_to_ws(c, d_x, k, groups, d_status, st)) return rc;
    }
    return msm_dev<2>(c, d_sigs, c->at<void>(B_LAGR_WS), k, groups, d_out, d_out_inf, st);
}

// ------------------------------------------------------------ signature shares (blsgpu_sigshares.hip) --
// the argument checks of blsgpu_sig_shares_check* (before anything is written); 1: nothing to do
int sig_shares_args(const blsgpu_ctx* c, size_t k, size_t groups, size_t n_keys, bool null_buffer) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (k == 0 || k > blsgpu::lagr::MAX_K) return fail(-EINVAL, "k must be 1 .. BLSGPU_LAGRANGE_MAX_K");
    if (groups == 0) return 1;
    if (n_keys == 0) return fail(-EINVAL, "key index out of range");
    if (null_buffer) return fail(-EINVAL, "NULL argument");
    if (find::shares_too_large(k, groups, n_keys)) return fail(-EINVAL, "batch too large");
    return 0;
}
// Sessions in slices (find::plan_shares: the slice and B_SHR_WS; find::shares_round: B_SHR_ROUND and the grids of a round); per
// slice the once-per-call stages into B_SHR_WS, then the rounds (bisect_rounds): the nodes of a round
// (all of one length) go up and their verdict bytes come back.  A node's second half that lies past the session's k shares holds
// nothing and is not tested.  `scan`: the _dev form's device scan of the key indices first.  stats (host, may be NULL): rounds,
// node tests.
int sig_shares_dev(blsgpu_ctx* c, const void* d_sigs, const void* d_keys, size_t n_keys, const void* d_key_idx, const void* d_x,
                   const void* d_hashes, const void* d_weights, int scaled, size_t k, size_t groups, void* d_status, void* d_sess,
                   uint64_t* stats, bool scan, hipStream_t st) {
    using namespace blsgpu::sigsh;
    const find::SharesPlan p = find::plan_shares(*c, k, groups, n_keys, scaled != 0);
    const find::SharesWs& w = p.w;
    const size_t slice = p.slice, K = p.K;
    StreamGuard sg(c, st);
    if (int rc = c->grow(B_SHR_WS, w.bytes)) return rc;
    char* const W = c->at<char>(B_SHR_WS);
    if (scan) {
        uint32_t bad = 0;
        if (int rc = scan_indices(c, W, d_key_idx, n_keys, nullptr, 0, groups * k, false, bad, st)) return rc;
        if (bad) return fail(-EINVAL, "key index out of range");
    }
    if (int rc = subgroup_dev(c, 1, d_keys, n_keys, W + w.o_keyst, st)) return rc;
    if (!scaled) HIP_TRY(hipMemsetAsync(d_sess, 1, groups, st));
    bisect::State<Node> bis;
    int rc = for_slices(groups, slice, [&](size_t lo, size_t m) {
        const size_t n = p.at(m).n;
        const char* sigs = (const char*)d_sigs + lo * k * BLSGPU_G2_BYTES;
        uint8_t* status = (uint8_t*)d_status + lo * k;
        if (int rc = subgroup_dev(c, 2, sigs, n, W + w.o_sigst, st)) return rc;
        if (int rc = blsgpu_hash_to_g2_dev(c, (const char*)d_hashes + lo * 32, m, W + w.o_h, st)) return rc;
        if (scaled) {
            if (int rc = lagrange_launch(c, (const char*)d_x + lo * k * 32, k, m, W + w.o_lam, (uint8_t*)d_sess + lo, st)) return rc;
        }
        hipLaunchKernelGGL(k_share_weights, dim3(p.at(m).g_weights), dim3(THREADS), 0, st, (const uint32_t*)sigs,
                           (const uint8_t*)(W + w.o_sigst), (const uint32_t*)d_keys, (const uint8_t*)(W + w.o_keyst),
                           (const uint32_t*)d_key_idx + lo * k, scaled ? (const uint8_t*)(W + w.o_lam) : nullptr,
                           scaled ? (const uint8_t*)d_sess + lo : nullptr, (const uint8_t*)d_weights + lo * k * 8,
                           (const uint32_t*)(W + w.o_h), (uint32_t)k, (uint32_t)n, (uint8_t*)(W + w.o_r), (uint8_t*)(W + w.o_w),
                           (uint32_t*)(W + w.o_pk), (uint8_t*)(W + w.o_elig), (uint8_t*)(W + w.o_hinf), status);
        HIP_TRY(hipGetLastError());
        // the leaves: scalar multiplications as sums of one point with device scalars
        if (int rc = msm_dev<2>(c, sigs, W + w.o_r, 1, n, W + w.o_a, nullptr, st)) return rc;
        if (int rc = msm_dev<1>(c, W + w.o_pk, W + w.o_w, 1, n, W + w.o_b, nullptr, st)) return rc;
        bis.nodes.resize(m);
        for (size_t s = 0; s < m; s++) bis.nodes[s] = {(uint32_t)s, 0u};
        return bisect_rounds(bis, K, k, st, [&](std::vector<Node>& cur, size_t len, const void*& d_verdict) {
            const size_t nn = cur.size();
            const find::SharesRound r = find::shares_round(nn, len, k);
            if (int rc = c->grow(B_SHR_ROUND, r.w.bytes)) return rc;
            char* const R = c->at<char>(B_SHR_ROUND);
            const Node* d_nodes = (const Node*)(R + r.w.o_nodes);
            HIP_TRY(hipMemcpyAsync(R + r.w.o_nodes, cur.data(), nn * sizeof(Node), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_share_gather, dim3(r.g_gather), dim3(THREADS), 0, st, d_nodes, r.lg, r.gtotal,
                               (uint32_t)k, (const uint4*)(W + w.o_a), (const uint4*)(W + w.o_b), (const uint8_t*)(W + w.o_elig),
                               (uint4*)(R + r.w.o_ga), (uint4*)(R + r.w.o_gb));
            HIP_TRY(hipGetLastError());
            if (int rc = msm_dev<2>(c, R + r.w.o_ga, nullptr, len, nn, R + r.w.o_s, R + r.w.o_sinf, st)) return rc;
            if (int rc = msm_dev<1>(c, R + r.w.o_gb, nullptr, len, nn, R + r.w.o_p, R + r.w.o_pinf, st)) return rc;
            hipLaunchKernelGGL(k_share_pairs, dim3(r.g_pairs), dim3(THREADS), 0, st, d_nodes, r.ptotal,
                               (const uint4*)(R + r.w.o_s), (const uint8_t*)(R + r.w.o_sinf), (const uint4*)(R + r.w.o_p), (const uint8_t*)(R + r.w.o_pinf),
                               (const uint4*)(W + w.o_h), (const uint8_t*)(W + w.o_hinf), (uint4*)(R + r.w.o_g1), (uint4*)(R + r.w.o_g2));
            HIP_TRY(hipGetLastError());
            if (int rc = blsgpu_pairing_multi_batch_dev(c, R + r.w.o_g1, R + r.w.o_g2, nullptr, 2, nn, R + r.w.o_e, st)) return rc;
            hipLaunchKernelGGL(k_share_verdict, dim3(r.g_verdict), dim3(THREADS), 0, st, d_nodes, (uint32_t)nn,
                               (const uint4*)(R + r.w.o_e), (const uint8_t*)(R + r.w.o_sinf), (const uint8_t*)(R + r.w.o_pinf),
                               (const uint8_t*)(W + w.o_hinf), len == 1 ? 1u : 0u, (uint32_t)k, (uint8_t*)(R + r.w.o_v), status);
            HIP_TRY(hipGetLastError());
            d_verdict = R + r.w.o_v;
            return 0;
        });
    });
    if (!rc) bis.report(stats, 2);
    return rc;
}

// ------------------------------------------------------------ short public scalars (blsgpu_smul64.hip) --
// enqueues out_i = w_i P_(d_idx ? idx[i] : i) on `st` for n 64-bit weights (caller: StreamGuard, arguments checked, idx in
// range): launches of at most SRT_LANES / LP units, each with tables of its own in B_SM64_WS.  With d_idx the n_pts points are
// prepared once and every launch indexes them; without, a launch prepares its own points.
template <int DEG>
int smul64_launch(blsgpu_ctx* c, const void* d_pts, size_t n_pts, const void* d_idx, const void* d_w, size_t n, void* d_out, void* d_out_inf,
                  hipStream_t st) {
    const ragged::Smul64Plan p = ragged::plan_smul64(*c, MSM_CONSTS, DEG, n_pts, n, d_idx != nullptr);
    if (int rc = c->grow(B_SM64_WS, p.words * 4)) return rc;
    uint32_t* W = c->at<uint32_t>(B_SM64_WS);
    uint8_t* live = (uint8_t*)(W + p.o_live);
    if (d_idx) {
        hipLaunchKernelGGL(blsgpu::k_lane_prep<DEG>, dim3(p.g_prep_all), dim3(256), 0, st, (const uint32_t*)d_pts, (uint32_t)n_pts, W + p.o_prep, live);
        HIP_TRY(hipGetLastError());
    }
    return for_slices(n, p.S, [&](size_t lo, size_t) {
        const ragged::Smul64Slice s = p.at(lo);
        if (!d_idx)
            hipLaunchKernelGGL(blsgpu::k_lane_prep<DEG>, dim3(s.g_prep), dim3(256), 0, st, (const uint32_t*)d_pts + s.pts, (uint32_t)s.m, W + p.o_prep, live);
        hipLaunchKernelGGL(blsgpu::k_smul64<DEG>, dim3(s.g_smul), dim3(64), 0, st, W + p.o_prep, live,
                           d_idx ? (const uint32_t*)d_idx + lo : nullptr, (const uint8_t*)d_w + s.w, (uint32_t)s.m, W + p.o_tab,
                           (uint32_t*)d_out + s.out, d_out_inf ? (uint8_t*)d_out_inf + lo : nullptr);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}
// the argument checks of blsgpu_g?_mul_short* (before anything is written); 1: nothing to do
int mul_short_args(const blsgpu_ctx* c, const void* pts, const void* w, size_t n, const void* out) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 1;
    if (!pts || !w || !out) return fail(-EINVAL, "NULL argument");
    if (n > 0x7FFFFFFFull) return fail(-EINVAL, "batch too large");
    return 0;
}
template <int DEG>
int mul_short_dev(blsgpu_ctx* c, const void* d_pts, const void* d_w, size_t n, void* d_out, void* d_out_inf, hipStream_t st) {
    if (int rc = mul_short_args(c, d_pts, d_w, n, d_out)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    StreamGuard sg(c, st);
    return smul64_launch<DEG>(c, d_pts, n, nullptr, d_w, n, d_out, d_out_inf, st);
}
// the host-buffer form: FIX_HOST_SLICE points per staged slice
template <int DEG>
int mul_short_host(blsgpu_ctx* c, const uint8_t* pts, const uint8_t* w, size_t n, uint8_t* out, uint8_t* out_inf) {
    if (int rc = mul_short_args(c, pts, w, n, out)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    const size_t HS = slice_len(c, FIX_HOST_SLICE), S = n < HS ? n : HS;
    Staging s(c);
    const int dp = s.in(pts, S, 96 * DEG), dw = s.in(w, S, 8), dout = s.out(out, S, 96 * DEG), dinf = s.out(out_inf, S, 1);
    if (int rc = s.alloc()) return rc;
    return for_slices(n, S, [&](size_t lo, size_t m) {
        if (int rc = s.up(lo, m)) return rc;
        {
            StreamGuard sg(c, nullptr);
            if (int rc = smul64_launch<DEG>(c, s.at(dp), m, nullptr, s.at(dw), m, s.at(dout), s.opt(dinf), nullptr)) return rc;
        }
        return s.down(lo, m);
    });
}

// ------------------------------------------------------------ batch verification that names the forgeries (blsgpu_batchfind.hip) --
// the argument checks of blsgpu_verify_find* (before anything is written); 1: nothing to do
int verify_find_args(const blsgpu_ctx* c, size_t n, size_t n_keys, size_t n_msgs, bool null_buffer) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 1;
    if (null_buffer) return fail(-EINVAL, "NULL argument");
    if (n_keys == 0) return fail(-EINVAL, "key index out of range");
    if (n_msgs == 0) return fail(-EINVAL, "message index out of range");
    if (find::find_too_large(n, n_keys, n_msgs)) return fail(-EINVAL, "batch too large");
    return 0;
}
// e(-G1, G2) in B_FIND_UNIT (+512), from the pairing itself, once per context: what k_find_verdict compares a node with S = O with
int find_unit(blsgpu_ctx* c, hipStream_t st) {
    if (c->find_unit_ready) return 0;
    static const uint32_t neg_g1[24] = SIGSH_NEG_G1_WORDS, g2_gen[48] = SIGSH_G2_GEN_WORDS;
    if (int rc = c->grow(B_FIND_UNIT, 512 + BLSGPU_FQ12_BYTES)) return rc;
    char* const U = c->at<char>(B_FIND_UNIT);
    HIP_TRY(hipMemcpyAsync(U, neg_g1, sizeof(neg_g1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(U + 256, g2_gen, sizeof(g2_gen), hipMemcpyHostToDevice, st));
    if (int rc = blsgpu_pairing_multi_batch_dev(c, U, U + 256, nullptr, 1, 1, U + 512, st)) return rc;
    c->find_unit_ready = true;
    return 0;
}
// What the two verify_find forms share: find::plan_find gives the slice and B_FIND_WS, find::plain_round / find::folded_round
// B_FIND_ROUND and the grids of a round (find_plan.h).
using find::FindWs;
// once per call: the workspace, the _dev form's device scan of the indices (`scan`; `mono`: the folded form's precondition too),
// e(-G1, G2), the key subgroup flags and the distinct hashes, once each
int find_call_stages(blsgpu_ctx* c, const FindWs& w, const void* d_keys, size_t n_keys, const void* d_key_idx, const void* d_hashes,
                     size_t n_msgs, const void* d_msg_idx, size_t n, bool scan, bool mono, hipStream_t st) {
    if (int rc = c->grow(B_FIND_WS, w.bytes)) return rc;
    char* const W = c->at<char>(B_FIND_WS);
    if (scan) {
        uint32_t bad = 0;
        if (int rc = scan_indices(c, W, d_key_idx, n_keys, d_msg_idx, n_msgs, n, mono, bad, st)) return rc;
        if (mono ? bad & 1u : bad) return fail(-EINVAL, "key or message index out of range");
        if (bad) return fail(-EINVAL, "message indices decrease");
    }
    if (int rc = find_unit(c, st)) return rc;
    if (int rc = subgroup_dev(c, 1, d_keys, n_keys, W + w.o_keyst, st)) return rc;
    return blsgpu_hash_to_g2_dev(c, d_hashes, n_msgs, W + w.o_h, st);
}
// once per slice of m items from `lo`: the signature subgroup flags, the weights, eligibility and status bytes (k_find_settle),
// the dense order and n_e (k_find_dense), what `after_dense` enqueues, and the leaves A_i = r_i sig_i, B_i = r_i keys[key_idx[i]]
// by item (those of items that are not eligible are never read)
struct FindSlice { const char* sigs; const uint32_t *kidx, *midx, *dense; uint8_t* status; find::FindSlice at; };
template <class F>
int find_slice_stages(blsgpu_ctx* c, const find::FindPlan& p, char* W, const void* d_sigs, const void* d_keys, size_t n_keys,
                      const void* d_key_idx, const void* d_msg_idx, const void* d_weights, void* d_status, size_t lo, size_t m, hipStream_t st,
                      FindSlice& s, F after_dense) {
    using namespace blsgpu::bfind;
    const FindWs& w = p.w;
    s = {(const char*)d_sigs + lo * BLSGPU_G2_BYTES, (const uint32_t*)d_key_idx + lo, (const uint32_t*)d_msg_idx + lo,
         (const uint32_t*)(W + w.o_dense), (uint8_t*)d_status + lo, p.at(m)};
    if (int rc = subgroup_dev(c, 2, s.sigs, m, W + w.o_sigst, st)) return rc;
    hipLaunchKernelGGL(k_find_settle, dim3(s.at.g_settle), dim3(THREADS), 0, st, (const uint32_t*)s.sigs,
                       (const uint8_t*)(W + w.o_sigst), (const uint32_t*)d_keys, (const uint8_t*)(W + w.o_keyst), s.kidx,
                       (const uint32_t*)(W + w.o_h), s.midx, (const uint8_t*)d_weights + lo * 8, (uint32_t)m, (uint8_t*)(W + w.o_r),
                       (uint8_t*)(W + w.o_elig), s.status);
    hipLaunchKernelGGL(k_find_dense, dim3(1), dim3(DENSE_THREADS), 0, st, (const uint8_t*)(W + w.o_elig), (uint32_t)m,
                       (uint32_t*)(W + w.o_dense), (uint32_t*)(W + 4));
    after_dense();
    HIP_TRY(hipGetLastError());
    if (int rc = smul64_launch<2>(c, s.sigs, m, nullptr, W + w.o_r, m, W + w.o_a, nullptr, st)) return rc;
    return smul64_launch<1>(c, d_keys, n_keys, s.kidx, W + w.o_r, m, W + w.o_b, nullptr, st);
}

// Items in slices; per slice the shared stages into B_FIND_WS and ONE read of n_e, then the rounds (bisect_rounds) over aligned
// nodes (offset, length L) of the dense order, L from ceil_pow2(n_e) halving: the full nodes of a round go through one
// multi-pairing batch of L + 1 pairs each, the one node that crosses n_e through a call of its own size (bisect::plain_round), a
// node wholly past n_e does not exist.  `scan`: the _dev form's device scan of the indices first.  stats (host, may be NULL):
// rounds, node tests, pairs fed.
int verify_find_dev(blsgpu_ctx* c, const void* d_sigs, const void* d_keys, size_t n_keys, const void* d_key_idx, const void* d_hashes,
                    size_t n_msgs, const void* d_msg_idx, const void* d_weights, size_t n, void* d_status, uint64_t* stats, bool scan,
                    hipStream_t st) {
    using namespace blsgpu::bfind;
    const find::FindPlan plan = find::plan_find(*c, n, n_keys, n_msgs, false);
    const FindWs& w = plan.w;
    StreamGuard sg(c, st);
    if (int rc = find_call_stages(c, w, d_keys, n_keys, d_key_idx, d_hashes, n_msgs, d_msg_idx, n, scan, false, st)) return rc;
    char* const W = c->at<char>(B_FIND_WS);
    const uint4* d_unit = (const uint4*)(c->at<char>(B_FIND_UNIT) + 512);
    bisect::State<uint32_t> bis;
    int rc = for_slices(n, plan.slice, [&](size_t lo, size_t m) {
        FindSlice s;
        if (int rc = find_slice_stages(c, plan, W, d_sigs, d_keys, n_keys, d_key_idx, d_msg_idx, d_weights, d_status, lo, m, st, s, [] {})) return rc;
        uint32_t n_e = 0;
        HIP_TRY(hipMemcpyAsync(&n_e, W + 4, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (n_e == 0) return 0;
        bis.nodes.assign(1, 0u);
        return bisect_rounds(bis, bisect::ceil_pow2(n_e), n_e, st, [&](std::vector<uint32_t>& order, size_t L, const void*& d_verdict) {
            bisect::Part shape[2];
            bisect::plain_round(order, L, n_e, shape);
            const find::PlainRound r = find::plain_round(shape);
            if (int rc = c->grow(B_FIND_ROUND, r.bytes)) return rc;
            char* const R = c->at<char>(B_FIND_ROUND);
            HIP_TRY(hipMemcpyAsync(R + r.head.o_off, order.data(), r.nn * 4, hipMemcpyHostToDevice, st));
            for (const find::PlainPart& p : r.part) {
                if (p.nodes == 0) continue;
                const uint32_t* d_off = (const uint32_t*)(R + r.head.o_off) + p.first;
                hipLaunchKernelGGL(k_find_gather, dim3(p.g_gather), dim3(THREADS), 0, st, d_off, (uint32_t)p.len, p.gtotal, s.dense,
                                   (const uint4*)(W + w.o_a), (uint4*)(R + p.w.o_ga));
                HIP_TRY(hipGetLastError());
                if (int rc = msm_dev<2>(c, R + p.w.o_ga, nullptr, p.len, p.nodes, R + p.w.o_s, R + p.w.o_sinf, st)) return rc;
                hipLaunchKernelGGL(k_find_pairs, dim3(p.g_pairs), dim3(THREADS), 0, st, d_off, (uint32_t)p.len, p.ptotal, s.dense,
                                   (const uint4*)(R + p.w.o_s), (const uint8_t*)(R + p.w.o_sinf), (const uint4*)(W + w.o_b),
                                   (const uint4*)(W + w.o_h), s.midx, (uint4*)(R + p.w.o_g1), (uint4*)(R + p.w.o_g2));
                HIP_TRY(hipGetLastError());
                if (int rc = blsgpu_pairing_multi_batch_dev(c, R + p.w.o_g1, R + p.w.o_g2, nullptr, p.gsz, p.nodes, R + p.w.o_e, st)) return rc;
                hipLaunchKernelGGL(k_find_verdict, dim3(p.g_verdict), dim3(THREADS), 0, st, d_off, (uint32_t)p.nodes, (const uint4*)(R + p.w.o_e),
                                   (const uint8_t*)(R + p.w.o_sinf), d_unit, L == 1 ? 1u : 0u, s.dense, (uint8_t*)(R + r.head.o_v) + p.first,
                                   s.status);
                HIP_TRY(hipGetLastError());
                bis.pairs += p.pairs;
            }
            d_verdict = R + r.head.o_v;
            return 0;
        });
    });
    if (!rc) bis.report(stats, 3);
    return rc;
}

// ------------------------------------------------------------ point prefix sums and range sums (blsgpu_pscan.hip) --
// One scan's workspace (B_PSCAN_G1 / B_PSCAN_G2): the prepared points of a slice, their live and kind bytes, the chunk totals
// and counts, the n + 1 prefix records and counts, and the carry into the next slice.
struct PscanWs { uint32_t *prep, *ct, *cb, *s, *cnt, *carry, *carryc; uint8_t *live, *kind; };
template <int DEG>
int pscan_ws(blsgpu_ctx* c, size_t pts, PscanWs& w) {
    const ragged::ScanWs o = ragged::scan_ws(MSM_CONSTS, RAGGED_CONSTS, DEG, pts);
    const BufId id = DEG == 1 ? B_PSCAN_G1 : B_PSCAN_G2;
    if (int rc = c->grow(id, o.bytes)) return rc;
    char* const W = c->at<char>(id);
    w = {(uint32_t*)(W + o.o_prep), (uint32_t*)(W + o.o_ct), (uint32_t*)(W + o.o_cb), (uint32_t*)(W + o.o_s), (uint32_t*)(W + o.o_cnt),
         (uint32_t*)(W + o.o_carry), (uint32_t*)(W + o.o_cc), (uint8_t*)(W + o.o_live), (uint8_t*)(W + o.o_kind)};
    return 0;
}
// enqueues the prefix records of the m points at d_pts (one slice) into w; `first`: no carry comes in; `more`: the last record
// is kept as the carry of the next slice
template <int DEG>
int pscan_launch(const PscanWs& w, const void* d_pts, size_t m, bool first, bool more, hipStream_t st) {
    namespace ps = blsgpu::pscan;
    const size_t PJ = blsgpu::L28_PJ * DEG;
    const ragged::ScanGrids g = ragged::scan_grids(RAGGED_CONSTS, m);
    if (m) hipLaunchKernelGGL(blsgpu::k_lane_prep<DEG>, dim3(g.g_prep), dim3(256), 0, st, (const uint32_t*)d_pts, (uint32_t)m, w.prep, w.live);
    hipLaunchKernelGGL(ps::k_pscan_totals<DEG>, dim3(g.g_chunks), dim3(64), 0, st, w.prep, w.live, (uint32_t)m, w.kind, w.ct, w.cb);
    hipLaunchKernelGGL(ps::k_pscan_mid<DEG>, dim3(1), dim3(ps::MID_THREADS), 0, st, w.ct, w.cb, (uint32_t)g.chunks, first ? nullptr : w.carry,
                       first ? nullptr : w.carryc);
    hipLaunchKernelGGL(ps::k_pscan_replay<DEG>, dim3(g.g_chunks), dim3(64), 0, st, w.prep, w.kind, (uint32_t)m, w.ct, w.cb, w.s, w.cnt);
    HIP_TRY(hipGetLastError());
    if (more) {
        HIP_TRY(hipMemcpyAsync(w.carry, w.s + m * PJ, PJ * 4, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(w.carryc, w.cnt + m, 4, hipMemcpyDeviceToDevice, st));
    }
    return 0;
}
// enqueues the sums of the m ranges whose end lies among the records [lo, hi] of w (base / basec: the records at the begins, NULL
// when every begin lies there too)
template <int DEG>
int pscan_ranges_launch(const PscanWs& w, size_t lo, size_t hi, bool last, const void* d_ranges, size_t m, const uint32_t* base,
                        const uint32_t* basec, void* d_out, void* d_flag, hipStream_t st) {
    hipLaunchKernelGGL(blsgpu::pscan::k_pscan_range<DEG>, dim3(ragged::range_blocks(MSM_CONSTS, DEG, m)), dim3(64), 0, st, w.s, w.cnt, (uint32_t)lo, (uint32_t)hi,
                       last ? 1u : 0u, (const uint32_t*)d_ranges, (uint32_t)m, base, basec, (uint32_t*)d_out, (uint8_t*)d_flag);
    HIP_TRY(hipGetLastError());
    return 0;
}
// the argument checks of blsgpu_g?_range_sums* (before anything is written); 1: nothing to do
int range_sums_args(const blsgpu_ctx* c, const void* pts, size_t n, const void* ranges, size_t m, const void* out, const void* flag) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if ((n && !pts) || (m && (!ranges || !out || !flag))) return fail(-EINVAL, "NULL argument");
    if (ragged::too_large(MSM_CONSTS, n, m)) return fail(-EINVAL, "batch too large");
    return m == 0 ? 1 : 0;
}
// Points in slices (ragged::plan_scan) whose records carry on from the slice before; a range is finished in the slice that
// holds its end.  With more than one slice the record at a range's begin is copied beside the range (B_PSCAN_RANGE) while its
// slice is there.  `scan`: the _dev form's device scan of the ranges first -- one synchronisation, before anything is written.
template <int DEG>
int range_sums_run(blsgpu_ctx* c, const void* d_pts, size_t n, const void* d_ranges, size_t m, void* d_out, void* d_flag, bool scan, hipStream_t st);
template <int DEG>
int range_sums_dev(blsgpu_ctx* c, const void* d_pts, size_t n, const void* d_ranges, size_t m, void* d_out, void* d_flag, bool scan,
                   hipStream_t st) {
    StreamGuard sg(c, st);
    return range_sums_run<DEG>(c, d_pts, n, d_ranges, m, d_out, d_flag, scan, st);
}
// ... the same inside a caller's StreamGuard (msm_ranges_dev sums its chunk partials with scan = false)
template <int DEG>
int range_sums_run(blsgpu_ctx* c, const void* d_pts, size_t n, const void* d_ranges, size_t m, void* d_out, void* d_flag, bool scan,
                   hipStream_t st) {
    namespace ps = blsgpu::pscan;
    const ragged::ScanPlan p = ragged::plan_scan(*c, MSM_CONSTS, RAGGED_CONSTS, DEG, n, m);
    if (int rc = c->grow(B_PSCAN_RANGE, p.range_bytes)) return rc;
    char* const R = c->at<char>(B_PSCAN_RANGE);
    if (scan) {
        uint32_t bad = 0;
        if (int rc = scan_flag(R, st, bad, [&](uint32_t* flag) {
                hipLaunchKernelGGL(ps::k_pscan_check, dim3(p.g_check), dim3(256), 0, st, (const uint32_t*)d_ranges, (uint32_t)m, (uint32_t)n, flag);
            }))
            return rc;
        if (bad) return fail(-EINVAL, "range out of order or past the points");
    }
    PscanWs w;
    if (int rc = pscan_ws<DEG>(c, p.S, w)) return rc;
    uint32_t* const base = p.single ? nullptr : (uint32_t*)(R + p.o_base);
    uint32_t* const basec = p.single ? nullptr : (uint32_t*)(R + p.o_basec);
    size_t lo = 0;
    do {
        const ragged::ScanSlice s = p.at(lo);
        if (int rc = pscan_launch<DEG>(w, (const char*)d_pts + s.lo * 96 * DEG, s.len, s.first, s.more, st)) return rc;
        if (!p.single)
            hipLaunchKernelGGL(ps::k_pscan_begin<DEG>, dim3(p.g_begin), dim3(256), 0, st, w.s, w.cnt, (uint32_t)s.lo, (uint32_t)s.hi, s.last ? 1u : 0u,
                               (const uint32_t*)d_ranges, p.begin_total, base, basec);
        if (int rc = pscan_ranges_launch<DEG>(w, s.lo, s.hi, s.last, d_ranges, m, base, basec, d_out, d_flag, st)) return rc;
        lo = s.hi;
    } while (lo < n);
    return 0;
}
template <int DEG>
int range_sums_host(blsgpu_ctx* c, const uint8_t* pts, size_t n, const uint32_t* ranges, size_t m, uint8_t* out, uint8_t* flag) {
    if (int rc = range_sums_args(c, pts, n, ranges, m, out, flag)) return rc < 0 ? rc : 0;
    if (ragged::first_bad_range(ranges, m, n) != ragged::NONE) return fail(-EINVAL, "range out of order or past the points");
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int dp = s.in(n ? pts : nullptr, n * 96 * DEG), dr = s.in(ranges, m * 8), dout = s.out(out, m * 96 * DEG), df = s.out(flag, m);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = range_sums_dev<DEG>(c, s.opt(dp), n, s.at(dr), m, s.at(dout), s.at(df), false, nullptr)) return rc;
    return s.down();
}

// ------------------------------------------------------------ ragged multi-scalar sums (blsgpu_msmr.hip) --
// the argument checks of blsgpu_g?_msm_ranges* (before anything is written); 1: nothing to do
int msm_ranges_args(const blsgpu_ctx* c, const void* pts, const void* scalars, size_t n, const void* ranges, size_t m, const void* out,
                    const void* flag) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if ((n && (!pts || !scalars)) || (m && (!ranges || !out || !flag))) return fail(-EINVAL, "NULL argument");
    if (ragged::too_large(MSM_CONSTS, n, m)) return fail(-EINVAL, "batch too large");
    return m == 0 ? 1 : 0;
}
// The ranges are checked and cut into chunks of at most eight points on the device (k_msmr_count, k_msmr_scan, k_msmr_fill); ONE
// synchronisation reads the check flag and the number of chunks, before anything is written to the outputs.  Then the n points
// are prepared once, the chunks go through k_smul_seg in slices whose tables stay below 2 GB and whose launches take at most
// SRT_LANES / LP units, and the chunk partials -- affine points in chunk order, range j's being the chunks [first[j],
// first[j + 1]) -- are summed per range by the range-sum passes (range_sums_run without its scan).  A range one of whose chunks
// counted a point off the curve gets flag 2 last (k_msmr_offcurve over the prefix sums of the counts).  A range of a single
// chunk takes the same passes (writing it straight from k_smul_seg: NOT MEASURED).
// Workspace: B_MSM_PART holds the head words, the chunk counts, first[] and the chunk ranges; B_BUCKETS the prepared points, the
// chunk table, the partials, the counts with their prefix sums and one slice's tables.
template <int DEG>
int msm_ranges_dev(blsgpu_ctx* c, const void* d_pts, const void* d_scalars, size_t n, const void* d_ranges, size_t m, void* d_out,
                   void* d_flag, hipStream_t st) {
    namespace mr = blsgpu::msmr;
    StreamGuard sg(c, st);
    const ragged::MsmrHeads h = ragged::plan_msmr_heads(m);
    if (int rc = c->grow(B_MSM_PART, h.words * 4)) return rc;
    uint32_t* const Hd = c->at<uint32_t>(B_MSM_PART);
    HIP_TRY(hipMemsetAsync(Hd, 0, 16, st));
    hipLaunchKernelGGL(mr::k_msmr_count, dim3(h.g_count), dim3(256), 0, st, (const uint32_t*)d_ranges, (uint32_t)m, (uint32_t)n, Hd, Hd + h.h_cnt);
    hipLaunchKernelGGL(mr::k_msmr_scan, dim3(1), dim3(mr::SCAN_THREADS), 0, st, Hd + h.h_cnt, (uint32_t)m, Hd + h.h_first);
    HIP_TRY(hipGetLastError());
    uint32_t head[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(head, Hd, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (head[0]) return fail(-EINVAL, "range out of order or past the points");
    const ragged::MsmrBody p = ragged::plan_msmr_body(*c, MSM_CONSTS, RAGGED_CONSTS, DEG, n, m, (uint64_t)head[2] | ((uint64_t)head[3] << 32));
    if (p.too_many) return fail(-EINVAL, "too many chunks");
    const size_t total = p.total;
    if (int rc = c->grow(B_BUCKETS, p.words * 4)) return rc;
    uint32_t* const W = c->at<uint32_t>(B_BUCKETS);
    uint8_t* const live = (uint8_t*)(W + p.o_live);
    hipLaunchKernelGGL(mr::k_msmr_fill, dim3(p.g_fill), dim3(256), 0, st, (const uint32_t*)d_ranges, Hd + h.h_first, (uint32_t)m, (uint32_t)total,
                       W + p.o_tab, Hd + h.h_cr);
    HIP_TRY(hipGetLastError());
    if (total) {
        hipLaunchKernelGGL(blsgpu::k_lane_prep<DEG>, dim3(p.g_prep), dim3(256), 0, st, (const uint32_t*)d_pts, (uint32_t)n, W + p.o_prep, live);
        HIP_TRY(hipGetLastError());
        if (int rc = for_slices(total, p.slice, [&](size_t lo, size_t) {
                const ragged::MsmrSlice s = p.at(lo);
                hipLaunchKernelGGL(mr::k_smul_seg<DEG>, dim3(s.g_smul), dim3(64), 0, st, W + p.o_prep, live, (const uint32_t*)d_scalars, W + s.tab,
                                   (uint32_t)s.k, W + p.o_table, W + s.part, W + s.bad);
                HIP_TRY(hipGetLastError());
                return 0;
            }))
            return rc;
        hipLaunchKernelGGL(mr::k_msmr_scan, dim3(1), dim3(mr::SCAN_THREADS), 0, st, W + p.o_bad, (uint32_t)total, W + p.o_bpre);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = range_sums_run<DEG>(c, W + p.o_part, total, Hd + h.h_cr, m, d_out, d_flag, false, st)) return rc;
    if (total) {
        hipLaunchKernelGGL(mr::k_msmr_offcurve<DEG>, dim3(p.g_offcurve), dim3(256), 0, st, W + p.o_bpre, Hd + h.h_first, (uint32_t)m,
                           (uint32_t*)d_out, (uint8_t*)d_flag);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
template <int DEG>
int msm_ranges_host(blsgpu_ctx* c, const uint8_t* pts, const uint8_t* scalars, size_t n, const uint32_t* ranges, size_t m, uint8_t* out,
                    uint8_t* flag) {
    if (int rc = msm_ranges_args(c, pts, scalars, n, ranges, m, out, flag)) return rc < 0 ? rc : 0;
    if (ragged::first_bad_range(ranges, m, n) != ragged::NONE) return fail(-EINVAL, "range out of order or past the points");
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int dp = s.in(n ? pts : nullptr, n * 96 * DEG), dsc = s.in(n ? scalars : nullptr, n * 32), dr = s.in(ranges, m * 8),
              dout = s.out(out, m * 96 * DEG), df = s.out(flag, m);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = msm_ranges_dev<DEG>(c, s.opt(dp), s.opt(dsc), n, s.at(dr), m, s.at(dout), s.at(df), nullptr)) return rc;
    return s.down();
}

// ------------------------------------------------------------ batched Signature.divide_by (blsgpu_sigdiv.hip) --
// the argument checks of blsgpu_sig_divide* (before anything is written); 1: nothing to do
int sig_divide_args(const blsgpu_ctx* c, const void* pts, size_t n_pts, const void* pt_off, size_t m, const void* ent_off, const void* ea,
                    const void* eb, size_t n_ent, const void* out, const void* flag, const void* status) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (m == 0) return 1;
    if (!pts || !pt_off || !ent_off || !out || !flag || !status || (n_ent && (!ea || !eb))) return fail(-EINVAL, "NULL argument");
    if (ragged::too_large(MSM_CONSTS, n_pts, m, n_ent)) return fail(-EINVAL, "batch too large");
    if (n_pts < m) return fail(-EINVAL, "a dividend without a point");
    return 0;
}
// The offsets are checked on the device (k_sigdiv_check), the entries tested (k_sigdiv_cross), the scalars, statuses and the
// working copy written into the WORKSPACE (k_sigdiv_quot, k_sigdiv_fold), and ONE synchronisation reads the head words: the
// verdict on the offsets and the number of non-unit quotients.  Only then do the statuses and scalars go to the caller and
// the sums run: the plain sums of the working copy when no accepted quotient differs from 1 (and the knob allows it), the
// ragged multi-scalar sums of the points as given otherwise.  A refused dividend gets flag 3 and (0,0) last.
int sig_divide_dev(blsgpu_ctx* c, const void* d_pts, size_t n_pts, const void* d_pt_off, size_t m, const void* d_ent_off, const void* d_ea,
                   const void* d_eb, size_t n_ent, void* d_out, void* d_flag, void* d_status, void* d_scalars, uint32_t* stats, hipStream_t st) {
    namespace sd = blsgpu::sigdiv;
    StreamGuard sg(c, st);
    const ragged::SigdivPlan p = ragged::plan_sigdiv(n_pts, m, n_ent);
    if (int rc = c->grow(B_SIGDIV_WS, p.bytes)) return rc;
    char* const W = c->at<char>(B_SIGDIV_WS);
    uint32_t* const head = (uint32_t*)W;
    HIP_TRY(hipMemsetAsync(W, 0, p.memset_bytes, st));                         // the head words, mism and zero
    hipLaunchKernelGGL(sd::k_sigdiv_check, dim3(p.g_check), dim3(256), 0, st, (const uint32_t*)d_pt_off, (uint32_t)m, (const uint32_t*)d_ent_off,
                       (uint32_t)n_pts, (uint32_t)n_ent, head);
    if (n_ent)
        hipLaunchKernelGGL(sd::k_sigdiv_cross, dim3(p.g_cross), dim3(256), 0, st, head, (const uint32_t*)d_ent_off, (uint32_t)n_pts,
                           (const uint8_t*)d_ea, (const uint8_t*)d_eb, (uint32_t)n_ent, (uint8_t*)(W + p.o_mism), (uint8_t*)(W + p.o_zero));
    hipLaunchKernelGGL(sd::k_sigdiv_quot, dim3(p.g_quot), dim3(256), 0, st, head, (const uint32_t*)d_ent_off, (uint32_t)n_pts, (const uint8_t*)d_ea,
                       (const uint8_t*)d_eb, (const uint8_t*)(W + p.o_mism), (const uint8_t*)(W + p.o_zero), (const uint32_t*)d_pts,
                       (uint8_t*)(W + p.o_status), (uint8_t*)(W + p.o_scalars), (uint8_t*)(W + p.o_nonunit), (uint32_t*)(W + p.o_work));
    hipLaunchKernelGGL(sd::k_sigdiv_fold, dim3(p.g_fold), dim3(256), 0, st, head, (const uint32_t*)d_pt_off, (uint32_t)m,
                       (const uint8_t*)(W + p.o_status), (uint8_t*)(W + p.o_refused), (uint32_t*)(W + p.o_ranges));
    HIP_TRY(hipGetLastError());
    uint32_t h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, head, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h[0]) return fail(-EINVAL, "offsets out of order, a dividend without a point or with entries of its own");
    if (h[1] != m) return fail(-EINVAL, "a divisor without entries");
    const bool plain = c->sigdiv_plain && h[2] == 0;
    if (stats) {
        stats[0] = plain ? 0u : 1u;
        stats[1] = h[2];
    }
    HIP_TRY(hipMemcpyAsync(d_status, W + p.o_status, n_pts, hipMemcpyDeviceToDevice, st));
    if (d_scalars) HIP_TRY(hipMemcpyAsync(d_scalars, W + p.o_scalars, 32 * n_pts, hipMemcpyDeviceToDevice, st));
    if (plain) {
        if (int rc = range_sums_run<2>(c, W + p.o_work, n_pts, W + p.o_ranges, m, d_out, d_flag, false, st)) return rc;
    } else {
        if (int rc = msm_ranges_dev<2>(c, d_pts, W + p.o_scalars, n_pts, W + p.o_ranges, m, d_out, d_flag, st)) return rc;
    }
    hipLaunchKernelGGL(sd::k_sigdiv_refuse, dim3(p.g_refuse), dim3(256), 0, st, (const uint8_t*)(W + p.o_refused), (uint32_t)m, (uint32_t*)d_out,
                       (uint8_t*)d_flag);
    HIP_TRY(hipGetLastError());
    return 0;
}
int sig_divide_host(blsgpu_ctx* c, const uint8_t* pts, size_t n_pts, const uint32_t* pt_off, size_t m, const uint32_t* ent_off, const uint8_t* ea,
                    const uint8_t* eb, size_t n_ent, uint8_t* out, uint8_t* flag, uint8_t* status, uint8_t* scalars, uint32_t* stats) {
    if (int rc = sig_divide_args(c, pts, n_pts, pt_off, m, ent_off, ea, eb, n_ent, out, flag, status)) return rc < 0 ? rc : 0;
    if (pt_off[0] != 0 || pt_off[m] != n_pts || ent_off[0] != 0 || ent_off[n_pts] != n_ent) return fail(-EINVAL, "offsets do not span the lists");
    for (size_t p = 0; p < n_pts; p++)
        if (ent_off[p] > ent_off[p + 1] || ent_off[p + 1] > n_ent) return fail(-EINVAL, "entry offsets out of order");
    for (size_t j = 0; j < m; j++) {
        if (pt_off[j] >= pt_off[j + 1] || pt_off[j + 1] > n_pts) return fail(-EINVAL, "point offsets out of order or a dividend without a point");
        if (ent_off[pt_off[j]] != ent_off[pt_off[j] + 1]) return fail(-EINVAL, "a dividend with entries of its own");
        for (size_t p = pt_off[j] + 1; p < pt_off[j + 1]; p++)
            if (ent_off[p] == ent_off[p + 1]) return fail(-EINVAL, "a divisor without entries");
    }
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int dp = s.in(pts, n_pts * 192), dpo = s.in(pt_off, (m + 1) * 4), deo = s.in(ent_off, (n_pts + 1) * 4),
              da = s.in(n_ent ? ea : nullptr, n_ent * 32), db = s.in(n_ent ? eb : nullptr, n_ent * 32), dout = s.out(out, m * 192), df = s.out(flag, m),
              dst = s.out(status, n_pts), dsc = s.out(scalars, n_pts * 32);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = sig_divide_dev(c, s.at(dp), n_pts, s.at(dpo), m, s.at(deo), s.opt(da), s.opt(db), n_ent, s.at(dout), s.at(df), s.at(dst), s.opt(dsc),
                                stats, nullptr))
        return rc;
    return s.down();
}

// ------------------------------------------------------------ batch verification that folds shared messages (blsgpu_pscan.hip) --
// verify_find_dev with the items of one message FOLDED inside every node.  msg_idx is non-decreasing, so in the dense order
// every message is one contiguous run.  Once per slice, beyond verify_find_dev's stages: the run table (k_fold_runs; the host
// reads it with n_e in the same synchronisation), the leaves in the dense order (k_fold_leaves) and their prefix records SA
// (G2) and SB (G1).  A round's node (off, L), end = min(off + L, n_e), is e(-G1, SA[end] - SA[off]) prod_r e(SB[min(end,
// rb[r+1])] - SB[max(off, rb[r])], H(h_r)) = 1 over the runs r that meet it: the host lays out one SLOT per pair -- node after
// node, the nodes of a round ordered by their pair count --, the two range kernels give the sums (the B sums of the slots that are
// no head, the S of the nodes), k_fold_codes / k_fold_fill lay out the pairs, and the nodes of EQUAL pair count go through one blsgpu_pairing_multi_batch_dev each: nothing is padded.
int verify_find_folded_dev(blsgpu_ctx* c, const void* d_sigs, const void* d_keys, size_t n_keys, const void* d_key_idx, const void* d_hashes,
                           size_t n_msgs, const void* d_msg_idx, const void* d_weights, size_t n, void* d_status, uint64_t* stats, bool scan,
                           hipStream_t st) {
    using namespace blsgpu::bfind;
    namespace ps = blsgpu::pscan;
    const find::FindPlan fp = find::plan_find(*c, n, n_keys, n_msgs, true);
    const FindWs& w = fp.w;
    StreamGuard sg(c, st);
    if (int rc = find_call_stages(c, w, d_keys, n_keys, d_key_idx, d_hashes, n_msgs, d_msg_idx, n, scan, true, st)) return rc;
    char* const W = c->at<char>(B_FIND_WS);
    const uint4* d_unit = (const uint4*)(c->at<char>(B_FIND_UNIT) + 512);
    bisect::State<uint32_t> bis;
    bisect::FoldPlan plan;                                                   // plan.tab goes up in every round: written by the round alone
    std::vector<uint32_t> rb(fp.rcap), rmsg(fp.rcap);
    int rc = for_slices(n, fp.slice, [&](size_t lo, size_t m) {
        FindSlice s;
        if (int rc = find_slice_stages(c, fp, W, d_sigs, d_keys, n_keys, d_key_idx, d_msg_idx, d_weights, d_status, lo, m, st, s, [&] {
                hipLaunchKernelGGL(ps::k_fold_runs, dim3(1), dim3(ps::RUN_THREADS), 0, st, s.dense, (const uint32_t*)(W + 4), s.midx,
                                   (uint32_t*)(W + w.o_rb), (uint32_t*)(W + w.o_rmsg), (uint32_t*)(W + 8));
            }))
            return rc;
        // the leaves of the eligible items in the dense order
        hipLaunchKernelGGL(ps::k_fold_leaves, dim3(s.at.g_leaves), dim3(ps::THREADS), 0, st, s.dense, (const uint32_t*)(W + 4), s.at.ltotal,
                           (const uint4*)(W + w.o_a), (const uint4*)(W + w.o_b), (uint4*)(W + w.o_ad), (uint4*)(W + w.o_bd));
        HIP_TRY(hipGetLastError());
        uint32_t head[2] = {0, 0};                                           // n_e, the number of runs
        const size_t rn = s.at.rn;
        HIP_TRY(hipMemcpyAsync(head, W + 4, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(rb.data(), W + w.o_rb, rn * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(rmsg.data(), W + w.o_rmsg, rn * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint32_t n_e = head[0], n_runs = head[1];
        if (n_e == 0) return 0;
        if (!bisect::run_table_ok(n_e, n_runs, rn, rb.data())) return fail(-EIO, "run table inconsistent");
        PscanWs wa, wb;
        if (int rc = pscan_ws<2>(c, n_e, wa)) return rc;
        if (int rc = pscan_ws<1>(c, n_e, wb)) return rc;
        if (int rc = pscan_launch<2>(wa, W + w.o_ad, n_e, true, false, st)) return rc;
        if (int rc = pscan_launch<1>(wb, W + w.o_bd, n_e, true, false, st)) return rc;
        bis.nodes.assign(1, 0u);
        return bisect_rounds(bis, bisect::ceil_pow2(n_e), n_e, st, [&](std::vector<uint32_t>& nodes, size_t L, const void*& d_verdict) {
            bisect::fold_round(nodes, L, n_e, rb.data(), rmsg.data(), n_runs, plan);
            const bisect::FoldPlan& t = plan;
            const find::FoldRound r = find::folded_round(t);
            const size_t nn = r.nn;
            if (int rc = c->grow(B_FIND_ROUND, r.w.bytes)) return rc;
            char* const R = c->at<char>(B_FIND_ROUND);
            const uint32_t* const T = (const uint32_t*)(R + r.w.o_tab);
            HIP_TRY(hipMemcpyAsync(R + r.w.o_tab, t.tab.data(), t.tab.size() * 4, hipMemcpyHostToDevice, st));
            if (int rc = pscan_ranges_launch<1>(wb, 0, n_e, true, T + t.t_rng1, r.nb, nullptr, nullptr, R + r.w.o_b, R + r.w.o_bflag, st)) return rc;
            if (int rc = pscan_ranges_launch<2>(wa, 0, n_e, true, T + t.t_rng2, nn, nullptr, nullptr, R + r.w.o_s, R + r.w.o_sflag, st)) return rc;
            hipLaunchKernelGGL(ps::k_fold_codes, dim3(r.g_codes), dim3(ps::THREADS), 0, st, T + t.t_first, (uint32_t)nn,
                               (const uint8_t*)(R + r.w.o_bflag), (const uint8_t*)(R + r.w.o_sflag), (uint8_t*)(R + r.w.o_code),
                               (uint8_t*)(R + r.w.o_odd));
            hipLaunchKernelGGL(ps::k_fold_fill, dim3(r.g_fill), dim3(ps::THREADS), 0, st, T + t.t_node, T + t.t_first, T + t.t_msg, r.ftotal,
                               (const uint8_t*)(R + r.w.o_code), (const uint4*)(R + r.w.o_b), (const uint4*)(R + r.w.o_s),
                               (const uint4*)(W + w.o_h), (uint4*)(R + r.w.o_g1), (uint4*)(R + r.w.o_g2));
            HIP_TRY(hipGetLastError());
            for (size_t i = 0; i < nn;) {                                    // the nodes of one pair count: one multi-pairing batch
                size_t j = i;
                while (j < nn && t.order[j].cnt == t.order[i].cnt) j++;
                const size_t s0 = t.tab[t.t_first + i];
                if (int rc = blsgpu_pairing_multi_batch_dev(c, R + r.g1_at(s0), R + r.g2_at(s0), nullptr, t.order[i].cnt, j - i, R + r.e_at(i), st))
                    return rc;
                i = j;
            }
            hipLaunchKernelGGL(k_find_verdict, dim3(r.g_verdict), dim3(THREADS), 0, st, T + t.t_off, (uint32_t)nn, (const uint4*)(R + r.w.o_e),
                               (const uint8_t*)(R + r.w.o_odd), d_unit, L == 1 ? 1u : 0u, s.dense, (uint8_t*)(R + r.w.o_v), s.status);
            HIP_TRY(hipGetLastError());
            bis.pairs += r.slots;
            d_verdict = R + r.w.o_v;
            return 0;
        });
    });
    if (!rc) bis.report(stats, 3);
    return rc;
}

// ------------------------------------------------------------ scalar-field work on secrets (blsgpu_frsecret.hip) --
// (blsgpu_fr_interpolate_at_zero_secret: fr_interpolate_dev with `secret`)
// the argument checks of blsgpu_fr_sum_secret* (before anything is written); 1: nothing to do
int fr_sum_args(const blsgpu_ctx* c, const void* y, size_t k, size_t groups, const void* out) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (k == 0) return fail(-EINVAL, "k must be at least 1");
    if (groups == 0) return 1;
    if (!y || !out) return fail(-EINVAL, "NULL argument");
    if (keys::fr_sum_too_large(k, groups)) return fail(-EINVAL, "batch too large");
    return 0;
}
// out[g] = sum_j y[g k + j] mod n (k_fr_sum_secret, timing kind 10), then the public key of every sum from k_fix_mul_secret
// reading `d_out` where it lies, all on the device
int fr_sum_secret_dev(blsgpu_ctx* c, const void* d_y, size_t k, size_t groups, void* d_out, void* d_out_pk_aff, void* d_out_pk_ser,
                      hipStream_t st) {
    using namespace blsgpu::frsec;
    StreamGuard sg(c, st);
    const bool pk = d_out_pk_aff || d_out_pk_ser;
    if (pk) {
        if (int rc = fix_table(c, st, true)) return rc;
    }
    const keys::SumShape sh = keys::sum_shape(KEYS_CONSTS, k);
    {
        KernelTimer kt(c, st, 10);
        hipLaunchKernelGGL(k_fr_sum_secret, dim3(sh.grid(groups)), dim3(SUM_THREADS), 0, st, (const uint8_t*)d_y, k, (uint32_t)groups, sh.gpb,
                           sh.per, (uint8_t*)d_out);
        HIP_TRY(hipGetLastError());
    }
    return pk ? fix_mul_secret_launch(c, d_out, groups, d_out_pk_aff, d_out_pk_ser, st) : 0;
}

// ------------------------------------------------------------ secure aggregation (blsgpu_hashpks.hip) --
// the argument checks of blsgpu_hash_pks* and blsgpu_aggregate_*_secure* (before anything is written); 1: nothing to do.
// k: keys hashed per group, m: exponents per group
int hash_pks_args(const blsgpu_ctx* c, size_t k, size_t m, size_t groups, bool null_buffer) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (k == 0 || m == 0) return fail(-EINVAL, "k and m must be at least 1");
    if (groups == 0) return 1;
    if (null_buffer) return fail(-EINVAL, "NULL argument");
    if (secure_ranges::fixed_too_large(k, m, groups)) return fail(-EINVAL, "batch too large");
    return 0;
}
// the workspace of a call: the digests, then the exponents (when they are not the caller's buffers; secure_ranges::FixedWorkspace)
struct HashPksWs { uint32_t* digest; uint32_t* ts; };
int hash_pks_ws(blsgpu_ctx* c, size_t m, size_t groups, HashPksWs& w) {
    const secure_ranges::FixedWorkspace p = secure_ranges::fixed_workspace(m, groups);
    if (int rc = c->grow(B_HPK_WS, p.total)) return rc;
    w.digest = (uint32_t*)(c->at<char>(B_HPK_WS) + p.digests);
    w.ts = (uint32_t*)(c->at<char>(B_HPK_WS) + p.exps);
    return 0;
}
// enqueues the digests of `groups` groups of k keys (k_hash_pks_digest, timing kind 11; skipped when the caller has them:
// d_pk_hash_in) and m exponents per group into d_ts (k_hash_pks_exp, kind 12) on `st` (caller: StreamGuard, arguments
// checked by hash_pks_args).  d_digest_ws: groups x 32 bytes the digests go to when they are computed here.
int hash_pks_launch(blsgpu_ctx* c, const void* d_pks_ser, size_t k, size_t groups, const void* d_pk_hash_in, size_t m, void* d_ts,
                    void* d_digest_ws, hipStream_t st) {
    using namespace blsgpu::hashpks;
    const void* d_digest = d_pk_hash_in;
    const size_t total = groups * m;
    const secure_ranges::Grids g = secure_ranges::grids(groups, total);
    if (!d_digest) {
        KernelTimer kt(c, st, 11);
        hipLaunchKernelGGL(k_hash_pks_digest, dim3(g.digest), dim3(DIGEST_THREADS), 0, st, (const uint32_t*)d_pks_ser, k, (uint32_t)groups,
                           (uint32_t*)d_digest_ws);
        HIP_TRY(hipGetLastError());
        d_digest = d_digest_ws;
    }
    KernelTimer kt(c, st, 12);
    hipLaunchKernelGGL(k_hash_pks_exp, dim3(g.exp), dim3(EXP_THREADS), 0, st, (const uint32_t*)d_digest, (uint32_t)m, total, (uint32_t*)d_ts);
    HIP_TRY(hipGetLastError());
    return 0;
}
// blsgpu_hash_pks_dev: the exponents into the caller's buffer, the digests into the caller's if it asks for them
int hash_pks_dev(blsgpu_ctx* c, const void* d_pks_ser, size_t k, size_t groups, const void* d_pk_hash_in, size_t m, void* d_out_ts,
                 void* d_out_pk_hash, hipStream_t st) {
    StreamGuard sg(c, st);
    void* d_digest_ws = d_out_pk_hash;
    if (!d_pk_hash_in && !d_digest_ws) {
        HashPksWs w;
        if (int rc = hash_pks_ws(c, 0, groups, w)) return rc;
        d_digest_ws = w.digest;
    }
    if (d_pk_hash_in && d_out_pk_hash && d_pk_hash_in != d_out_pk_hash)
        HIP_TRY(hipMemcpyAsync(d_out_pk_hash, d_pk_hash_in, groups * 32, hipMemcpyDeviceToDevice, st));
    return hash_pks_launch(c, d_pks_ser, k, groups, d_pk_hash_in, m, d_out_ts, d_digest_ws, st);
}
// the exponents of `groups` groups (m each, from k_pks keys each) into the workspace, then the sums of msm_dev<DEG> over
// groups x k points with them as its device scalars (m == k)
template <int DEG>
int aggregate_secure_dev(blsgpu_ctx* c, const void* d_pts, size_t k, const void* d_pks_ser, size_t k_pks, const void* d_pk_hash_in,
                         size_t groups, void* d_out, void* d_out_inf, hipStream_t st) {
    HashPksWs w;
    {
        StreamGuard sg(c, st);
        if (int rc = hash_pks_ws(c, k, groups, w)) return rc;
        if (int rc = hash_pks_launch(c, d_pks_ser, k_pks, groups, d_pk_hash_in, k, w.ts, w.digest, st)) return rc;
    }
    return msm_dev<DEG>(c, d_pts, w.ts, k, groups, d_out, d_out_inf, st);
}
// the exponents into the workspace, out[g] = sum_i t_gi sks[g k + i] mod n by k_fr_dot_secret (the exponents are its public
// coefficients, the keys its secret y; timing kind 10), then the public key of every sum from k_fix_mul_secret reading
// `d_out` where it lies
int aggregate_priv_keys_secure_dev(blsgpu_ctx* c, const void* d_sks, const void* d_pks_ser, const void* d_pk_hash_in, size_t k, size_t groups,
                                   void* d_out, void* d_out_pk_aff, void* d_out_pk_ser, hipStream_t st) {
    StreamGuard sg(c, st);
    const bool pk = d_out_pk_aff || d_out_pk_ser;
    if (pk) {
        if (int rc = fix_table(c, st, true)) return rc;
    }
    HashPksWs w;
    if (int rc = hash_pks_ws(c, k, groups, w)) return rc;
    if (int rc = hash_pks_launch(c, d_pks_ser, k, groups, d_pk_hash_in, k, w.ts, w.digest, st)) return rc;
    const keys::LagrShape sh = keys::lagrange_shape((uint32_t)k);
    {
        KernelTimer kt(c, st, 10);
        hipLaunchKernelGGL(blsgpu::frsec::k_fr_dot_secret, dim3(sh.grid(groups)), dim3(sh.threads), sh.lds, st, (const uint8_t*)w.ts,
                           (const uint8_t*)d_sks, (uint32_t)k, (uint32_t)groups, sh.gpb, (uint8_t*)d_out);
        HIP_TRY(hipGetLastError());
    }
    return pk ? fix_mul_secret_launch(c, d_out, groups, d_out_pk_aff, d_out_pk_ser, st) : 0;
}
// blsgpu_aggregate_priv_keys_secure*: hash_pks_args and the limit on k of k_fr_dot_secret (a group is one workgroup)
int aggregate_priv_args(const blsgpu_ctx* c, size_t k, size_t groups, bool null_buffer) {
    if (c && k > blsgpu::lagr::MAX_K) return fail(-EINVAL, "k must be 1 .. BLSGPU_LAGRANGE_MAX_K");
    if (int rc = hash_pks_args(c, k, k, groups, null_buffer)) return rc;
    if (secure_ranges::fixed_priv_too_large(k, groups)) return fail(-EINVAL, "batch too large");
    return 0;
}

// ------------------------------------------------------------ ragged secure aggregation (blsgpu_hashpks.hip, secure_ranges_plan.h) --
static_assert(secure_ranges::CHECK_THREADS == blsgpu::hashpks::CHECK_THREADS && secure_ranges::DIGEST_THREADS == blsgpu::hashpks::DIGEST_THREADS &&
                  secure_ranges::EXP_THREADS == blsgpu::hashpks::EXP_THREADS,
              "secure_ranges_plan.h: the grids differ from the kernels of blsgpu_hashpks.hip");
// the argument checks of blsgpu_hash_pks_ranges* and blsgpu_aggregate_*_secure_ranges* (before anything is written); 1: nothing to do
int secr_args(const blsgpu_ctx* c, size_t n_keys, size_t n_exp, size_t groups, bool null_buffer) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (groups == 0) return 1;
    if (null_buffer) return fail(-EINVAL, "NULL argument");
    if (secure_ranges::too_large(n_keys, n_exp, groups)) return fail(-EINVAL, "batch too large");
    return 0;
}
// the host tables of a host-buffer form, before anything is staged (pk_off NULL: the caller hands in the digests)
int secr_validate(const uint32_t* pk_off, size_t n_keys, const uint32_t* exp_off, size_t n_exp, size_t groups) {
    namespace sr = secure_ranges;
    if (pk_off)
        if (const sr::Verdict v = sr::validate(pk_off, groups, n_keys)) return fail(-EINVAL, std::string("pk_off: ") + sr::verdict_text(v));
    if (const sr::Verdict v = sr::validate(exp_off, groups, n_exp)) return fail(-EINVAL, std::string("exponent offsets: ") + sr::verdict_text(v));
    return 0;
}
constexpr const char* SECR_BAD_TABLE = "offsets decrease, do not begin at 0 or end past their buffer";
// Enqueues the check of both tables (k_secr_check, which also writes the pair table of the sums when W.pairs is wanted), the
// digests of the groups' own key ranges (k_hash_pks_digest_ranges, timing kind 11; skipped when the caller has them) and the
// exponents (k_hash_pks_exp_ranges, kind 12) on `st` (caller: StreamGuard, arguments checked by secr_args).  Both kernels
// return on the check's flag, W.head word 0.  d_digest_ws / d_ts: where the digests and the exponents go.
int secr_launch(blsgpu_ctx* c, const void* d_pks_ser, size_t n_keys, const void* d_pk_off, const void* d_exp_off, size_t n_exp, size_t groups,
                const void* d_pk_hash_in, uint32_t* d_flag, void* d_digest_ws, void* d_ts, uint32_t* d_pairs, hipStream_t st) {
    using namespace blsgpu::hashpks;
    const secure_ranges::Grids g = secure_ranges::grids(groups, n_exp);
    HIP_TRY(hipMemsetAsync(d_flag, 0, 16, st));
    hipLaunchKernelGGL(k_secr_check, dim3(g.check), dim3(CHECK_THREADS), 0, st, d_pk_hash_in ? nullptr : (const uint32_t*)d_pk_off, (uint32_t)n_keys,
                       (const uint32_t*)d_exp_off, (uint32_t)n_exp, (uint32_t)groups, d_flag, d_pairs);
    HIP_TRY(hipGetLastError());
    const void* d_digest = d_pk_hash_in;
    if (!d_digest) {
        KernelTimer kt(c, st, 11);
        hipLaunchKernelGGL(k_hash_pks_digest_ranges, dim3(g.digest), dim3(DIGEST_THREADS), 0, st, (const uint32_t*)d_pks_ser, (const uint32_t*)d_pk_off,
                           (uint32_t)groups, (const uint32_t*)d_flag, (uint32_t*)d_digest_ws);
        HIP_TRY(hipGetLastError());
        d_digest = d_digest_ws;
    }
    if (n_exp) {
        KernelTimer kt(c, st, 12);
        hipLaunchKernelGGL(k_hash_pks_exp_ranges, dim3(g.exp), dim3(EXP_THREADS), 0, st, (const uint32_t*)d_digest, (const uint32_t*)d_exp_off,
                           (uint32_t)groups, (uint32_t)n_exp, (const uint32_t*)d_flag, (uint32_t*)d_ts);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
// blsgpu_hash_pks_ranges_dev: the exponents into the caller's buffer, the digests into the caller's if it asks for them.  This
// call has no sums behind it whose synchronisation it could share: it reads the check's flag itself -- ONE synchronisation,
// before anything is written to an output (the kernels are enqueued first and return on the flag; the copy of the caller's
// digests waits for the verdict).
int hash_pks_ranges_dev(blsgpu_ctx* c, const void* d_pks_ser, size_t n_keys, const void* d_pk_off, const void* d_exp_off, size_t n_exp, size_t groups,
                        const void* d_pk_hash_in, void* d_out_ts, void* d_out_pk_hash, hipStream_t st) {
    StreamGuard sg(c, st);
    const secure_ranges::Workspace w = secure_ranges::workspace(groups, n_exp, !d_pk_hash_in && !d_out_pk_hash, false, false);
    if (int rc = c->grow(B_HPK_WS, w.total)) return rc;
    char* const W = c->at<char>(B_HPK_WS);
    uint32_t* const d_flag = (uint32_t*)(W + w.head);
    if (int rc = secr_launch(c, d_pks_ser, n_keys, d_pk_off, d_exp_off, n_exp, groups, d_pk_hash_in, d_flag, d_out_pk_hash ? d_out_pk_hash : W + w.digests,
                             d_out_ts, nullptr, st))
        return rc;
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, d_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad) return fail(-EINVAL, SECR_BAD_TABLE);
    if (d_pk_hash_in && d_out_pk_hash && d_pk_hash_in != d_out_pk_hash)
        HIP_TRY(hipMemcpyAsync(d_out_pk_hash, d_pk_hash_in, groups * 32, hipMemcpyDeviceToDevice, st));
    return 0;
}
// The exponents of all groups into the workspace, then the sums of msm_ranges_dev<DEG> over the n_exp points with them as its
// device scalars and the pair table k_secr_check wrote as its ranges.  No synchronisation of its own: a bad table poisons
// the pair table, so msm_ranges_dev's one read-back refuses the call before anything is written to the outputs; only then --
// on the failure path -- is the flag read, to tell whose refusal it was.
template <int DEG>
int aggregate_secure_ranges_dev(blsgpu_ctx* c, const void* d_pts, size_t n_exp, const void* d_exp_off, const void* d_pks_ser, size_t n_keys,
                                const void* d_pk_off, size_t groups, const void* d_pk_hash_in, void* d_out, void* d_flag_out, hipStream_t st) {
    const secure_ranges::Workspace w = secure_ranges::workspace(groups, n_exp, !d_pk_hash_in, true, true);
    char* W;
    {
        StreamGuard sg(c, st);
        if (int rc = c->grow(B_HPK_WS, w.total)) return rc;
        W = c->at<char>(B_HPK_WS);
        if (int rc = secr_launch(c, d_pks_ser, n_keys, d_pk_off, d_exp_off, n_exp, groups, d_pk_hash_in, (uint32_t*)(W + w.head), W + w.digests, W + w.exps,
                                 (uint32_t*)(W + w.pairs), st))
            return rc;
    }
    const int rc = msm_ranges_dev<DEG>(c, d_pts, W + w.exps, n_exp, W + w.pairs, groups, d_out, d_flag_out, st);
    if (rc == -EINVAL) {
        const std::string theirs = g_err;
        uint32_t bad = 0;
        HIP_TRY(hipMemcpyAsync(&bad, W + w.head, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return fail(-EINVAL, bad ? SECR_BAD_TABLE : theirs);
    }
    return rc;
}
// The host-buffer forms: the tables are validated on the host, the groups cut into slices (secure_ranges::cut, the test hook
// BLSGPU_TEST_SLICE_CAP shortening them) and every slice staged, run as a call of its own on tables that begin at 0, and
// read back.  DEG 0: blsgpu_hash_pks_ranges (out: the exponents; out2: the digests, may be NULL); DEG 1 / 2: the aggregates
// (pts: the n_exp points; out: the sums; out2: the flags).
template <int DEG>
int secure_ranges_host(blsgpu_ctx* c, const uint8_t* pts, size_t n_exp, const uint32_t* exp_off, const uint8_t* pks_ser, size_t n_keys,
                       const uint32_t* pk_off, size_t groups, const uint8_t* pk_hash_in, uint8_t* out, uint8_t* out2) {
    namespace sr = secure_ranges;
    if (pk_hash_in) pk_off = nullptr, pks_ser = nullptr;     // (with the digests given the keys are not read: they stay on the host)
    if (int rc = secr_validate(pk_off, n_keys, exp_off, n_exp, groups)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<sr::Slice> slices;
    sr::cut(pk_off, exp_off, groups, sr::slice_cap(*c), slices);
    const sr::Extent e = sr::extent(pk_off, exp_off, slices);
    constexpr size_t PT = DEG ? 96 * DEG : 0, OUT = DEG ? 96 * DEG : 0;
    Staging s(c);
    const int dpts = s.scratch(e.exps * PT), dpk = s.scratch(e.keys * 48), dko = s.scratch(pk_off ? (e.groups + 1) * 4 : 0),
              deo = s.scratch((e.groups + 1) * 4), dh = s.scratch(pk_hash_in ? e.groups * 32 : 0),
              dout = s.scratch(DEG ? e.groups * OUT : e.exps * 32), dout2 = s.scratch(DEG ? e.groups : (out2 ? e.groups * 32 : 0));
    if (int rc = s.alloc()) return rc;
    std::vector<uint32_t> ko, eo;
    for (const sr::Slice& sl : slices) {
        const size_t m = sl.hi - sl.lo, e0 = exp_off[sl.lo], ne = exp_off[sl.hi] - e0, k0 = pk_off ? pk_off[sl.lo] : 0, nk = pk_off ? pk_off[sl.hi] - k0 : 0;
        sr::rebase(exp_off, sl, eo);
        HIP_TRY(hipMemcpyAsync(s.at(deo), eo.data(), (m + 1) * 4, hipMemcpyHostToDevice, 0));
        if (pk_off) {
            sr::rebase(pk_off, sl, ko);
            HIP_TRY(hipMemcpyAsync(s.at(dko), ko.data(), (m + 1) * 4, hipMemcpyHostToDevice, 0));
            if (nk) HIP_TRY(hipMemcpyAsync(s.at(dpk), pks_ser + k0 * 48, nk * 48, hipMemcpyHostToDevice, 0));
        }
        if (pk_hash_in) HIP_TRY(hipMemcpyAsync(s.at(dh), pk_hash_in + sl.lo * 32, m * 32, hipMemcpyHostToDevice, 0));
        if (DEG && ne) HIP_TRY(hipMemcpyAsync(s.at(dpts), pts + e0 * PT, ne * PT, hipMemcpyHostToDevice, 0));
        const void* d_ko = pk_off ? s.at(dko) : nullptr;
        const void* d_pk = pk_off ? s.at(dpk) : nullptr;
        const void* d_h = pk_hash_in ? s.at(dh) : nullptr;
        if constexpr (DEG == 0) {
            if (int rc = hash_pks_ranges_dev(c, d_pk, nk, d_ko, s.at(deo), ne, m, d_h, s.at(dout), out2 ? s.at(dout2) : nullptr, nullptr)) return rc;
            if (ne) HIP_TRY(hipMemcpy(out + e0 * 32, s.at(dout), ne * 32, hipMemcpyDeviceToHost));
            if (out2) HIP_TRY(hipMemcpy(out2 + sl.lo * 32, s.at(dout2), m * 32, hipMemcpyDeviceToHost));
        } else {
            if (int rc = aggregate_secure_ranges_dev<DEG>(c, s.at(dpts), ne, s.at(deo), d_pk, nk, d_ko, m, d_h, s.at(dout), s.at(dout2), nullptr))
                return rc;
            HIP_TRY(hipMemcpy(out + sl.lo * OUT, s.at(dout), m * OUT, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(out2 + sl.lo, s.at(dout2), m, hipMemcpyDeviceToHost));
        }
    }
    return 0;
}

// the argument checks of blsgpu_threshold_deal_secret* (before anything is written); 1: nothing to do
int deal_args(const blsgpu_ctx* c, const void* coeffs, size_t n_polys, size_t t, const void* x, size_t n_x, const void* out_commit,
              const void* out_frag) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (keys::bad_k(KEYS_CONSTS, t)) return fail(-EINVAL, "t must be 1 .. BLSGPU_LAGRANGE_MAX_K");
    if (n_polys == 0) return 1;
    if (!coeffs) return fail(-EINVAL, "NULL argument");
    if (!out_commit && !out_frag) return fail(-EINVAL, "out_commit_aff and out_frag are both NULL");
    if (out_frag && (n_x == 0 || !x)) return fail(-EINVAL, "fragments need at least one point");
    if (keys::deal_too_large(KEYS_CONSTS, n_polys, t, n_x, out_frag != nullptr)) return fail(-EINVAL, "batch too large");
    return 0;
}
// commitments c_k G1 (k_fix_mul_secret) and fragments P(x_j) (k_fr_poly_eval_secret) of n_polys polynomials, all on the device
int deal_secret_dev(blsgpu_ctx* c, const void* d_coeffs, size_t n_polys, size_t t, const void* d_x, size_t n_x, void* d_out_commit,
                    void* d_out_frag, hipStream_t st) {
    StreamGuard sg(c, st);
    if (d_out_commit) {
        if (int rc = fix_table(c, st, true)) return rc;
        if (int rc = fix_mul_secret_launch(c, d_coeffs, n_polys * t, d_out_commit, nullptr, st)) return rc;
    }
    if (d_out_frag) {
        KernelTimer kt(c, st, 10);
        hipLaunchKernelGGL(blsgpu::frsec::k_fr_poly_eval_secret, dim3(keys::eval_blocks(KEYS_CONSTS, n_polys, n_x)), dim3(blsgpu::frsec::EVAL_THREADS),
                           t * keys::FR, st, (const uint8_t*)d_coeffs, (uint32_t)t, (const uint8_t*)d_x, (uint32_t)n_x,
                           (uint32_t)keys::eval_bpp(KEYS_CONSTS, n_x), (uint8_t*)d_out_frag);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// the argument checks of blsgpu_sign_threshold* (before anything is written); 1: nothing to do
int sign_threshold_args(const blsgpu_ctx* c, size_t k, size_t groups, size_t n_msg, bool null_buffer, const void* out_aff, const void* out_ser) {
    if (int rc = lagrange_args(c, k, groups, null_buffer)) return rc;
    if (n_msg != 1 && n_msg != groups) return fail(-EINVAL, "n_msg must be 1 or groups");
    if (!out_aff && !out_ser) return fail(-EINVAL, "out_aff and out_ser are both NULL");
    return 0;
}
}  // namespace


#define BLSGPU_EXPORT __attribute__((visibility("default")))

extern "C" {

BLSGPU_EXPORT const char* blsgpu_version(void) { return "blsgpu/1 gfx950 vm-tables " BLSVM_TABLE_HASH; }
BLSGPU_EXPORT const char* blsgpu_last_error(void) { return g_err.c_str(); }

BLSGPU_EXPORT int blsgpu_ctx_create(int device, blsgpu_ctx** out) {
    if (!out) return fail(-EINVAL, "out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(-ENODEV, std::string("no HIP device available (") + hipGetErrorString(e) +
                                 "); blsgpu has no CPU fallback");
    if (device < 0 || device >= count) return fail(-EINVAL, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    blsgpu_ctx* c = new blsgpu_ctx();
    c->device = device;
    read_knobs(c);
    // pack all tables into one device allocation (16-byte aligned pieces)
    auto al = [](size_t x) { return (x + 15) & ~size_t(15); };
    size_t o_m = 0;
    size_t o_mp = o_m + al(sizeof(BLSVM_MILLER_FLAT));
    size_t o_mp2 = o_mp + al(sizeof(BLSVM_MP_FLAT));
    size_t o_h2 = o_mp2 + al(sizeof(BLSVM_MP2_FLAT));
    size_t o_f = o_h2 + al(sizeof(BLSVM_H2_FLAT));
    size_t o_sl = o_f + al(sizeof(BLSVM_FEXP_FLAT));
    size_t o_s = o_sl + al(sizeof(BLSVM_SLOW_FLAT));
    size_t o_data = o_s + al(sizeof(BLSVM_SEG_FLAT));
    size_t o_c = o_data + al(sizeof(BLSVM_DATA));
    size_t total = o_c + al(sizeof(BLSVM_CONSTS));
    if (hipMalloc(&c->d_tables, total) != hipSuccess) {
        delete c;
        return fail(-ENOMEM, "hipMalloc(tables) failed");
    }
    char* base = (char*)c->d_tables;
    struct { size_t off; const void* src; size_t len; } parts[] = {
        {o_m, BLSVM_MILLER_FLAT, sizeof(BLSVM_MILLER_FLAT)}, {o_mp, BLSVM_MP_FLAT, sizeof(BLSVM_MP_FLAT)},
        {o_mp2, BLSVM_MP2_FLAT, sizeof(BLSVM_MP2_FLAT)},
        {o_h2, BLSVM_H2_FLAT, sizeof(BLSVM_H2_FLAT)},
        {o_f, BLSVM_FEXP_FLAT, sizeof(BLSVM_FEXP_FLAT)},
        {o_sl, BLSVM_SLOW_FLAT, sizeof(BLSVM_SLOW_FLAT)},
        {o_s, BLSVM_SEG_FLAT, sizeof(BLSVM_SEG_FLAT)},       {o_data, BLSVM_DATA, sizeof(BLSVM_DATA)},
        {o_c, BLSVM_CONSTS, sizeof(BLSVM_CONSTS)}};
    for (auto& p : parts) {
        if (hipMemcpy(base + p.off, p.src, p.len, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(c->d_tables);
            delete c;
            return fail(-EIO, "hipMemcpy(tables) failed");
        }
    }
    c->tabs.mflat = (const uint2*)(base + o_m);
    c->tabs.mpflat = (const uint2*)(base + o_mp);
    c->tabs.mp2flat = (const uint2*)(base + o_mp2);
    c->tabs.h2flat = (const uint2*)(base + o_h2);
    c->tabs.fflat = (const uint2*)(base + o_f);
    c->tabs.sflat = (const uint2*)(base + o_sl);
    c->tabs.segflat = (const uint2*)(base + o_s);
    c->tabs.data = (const uint16_t*)(base + o_data);
    c->tabs.consts = (const uint32_t*)(base + o_c);
    c->tabs.stamps = nullptr;
#ifdef BLSGPU_STAMPS
    {
        void* p = nullptr;
        if (hipMalloc(&p, 128) == hipSuccess) { (void)hipMemset(p, 0, 128); c->tabs.stamps = (unsigned long long*)p; }
    }
#endif
    if (hipMalloc((void**)&c->d_out, BLSGPU_FQ12_BYTES) != hipSuccess) {
        (void)hipFree(c->d_tables);
        delete c;
        return fail(-ENOMEM, "hipMalloc(out) failed");
    }
    // the kernels need more than the default 64 KiB of dynamic LDS
    (void)hipFuncSetAttribute((const void*)blsgpu::k_miller, hipFuncAttributeMaxDynamicSharedMemorySize,
                              MILLER_WAVES * blsgpu::TEAM_BYTES);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_reduce, hipFuncAttributeMaxDynamicSharedMemorySize,
                              REDUCE_WAVES * blsgpu::TEAM_BYTES);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_h2c_stage<0, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, blsgpu::H1_TEAM_DW * 4);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_h2c_stage<0, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, blsgpu::H1_TEAM_DW * 4);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_h2c_stage<1, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, blsgpu::H1_TEAM_DW * 4);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_h2c_stage<2, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, blsgpu::H1_TEAM_DW * 4);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_h2c_clear, hipFuncAttributeMaxDynamicSharedMemorySize,
                              blsgpu::H2_TEAM_DW * 4);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_decompress<1, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, BLSVM_D1_SLOTS * 48);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_decompress<1, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, BLSVM_D1_SLOTS * 48);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_decompress<2, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, BLSVM_D2_SLOTS * 48);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_decompress<2, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, BLSVM_D2_SLOTS * 48);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_decompress<2, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, BLSVM_D2_SLOTS * 48);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_miller_mp<BLSVM_MP_G>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              blsgpu::MP_TEAM_BYTES);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_miller_mp<2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              blsgpu::MP_TEAM_BYTES);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_final_groups, hipFuncAttributeMaxDynamicSharedMemorySize,
                              REDUCE_WAVES * blsgpu::TEAM_BYTES);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_bytes_to_partials, hipFuncAttributeMaxDynamicSharedMemorySize,
                              REDUCE_WAVES * blsgpu::TEAM_BYTES);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_msm_prep<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * blsgpu::TEAM_BYTES);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_msm_prep<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * blsgpu::TEAM_BYTES);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_msm_pip<1>, hipFuncAttributeMaxDynamicSharedMemorySize, blsgpu::PipCfg<1>::SLOTS * 48);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_msm_pip<2>, hipFuncAttributeMaxDynamicSharedMemorySize, blsgpu::PipCfg<2>::SLOTS * 48);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_msm<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * blsgpu::TEAM_BYTES);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_msm<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * blsgpu::TEAM_BYTES);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_msm_finish<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * blsgpu::TEAM_BYTES);
    (void)hipFuncSetAttribute((const void*)blsgpu::k_msm_finish<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * blsgpu::TEAM_BYTES);
    int rc = ensure_partials(c, pairing::pairs_partials(PAIRING_CONSTS, 4096));
    if (!rc && hipEventCreateWithFlags(&c->last_event, hipEventDisableTiming) != hipSuccess) rc = fail(-EIO, "hipEventCreate failed");
    if (rc) {
        blsgpu_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return 0;
}

BLSGPU_EXPORT void blsgpu_ctx_destroy(blsgpu_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->d_tables) (void)hipFree(c->d_tables);
    if (c->d_out) (void)hipFree(c->d_out);
    if (c->d_fix_table) (void)hipFree(c->d_fix_table);
    if (c->d_fix_table_secret) (void)hipFree(c->d_fix_table_secret);
    for (const Buf& b : c->buf)
        if (b.p) (void)hipFree(b.p);
    for (void* q : c->retired) (void)hipFree(q);
    if (c->last_event) (void)hipEventDestroy(c->last_event);
    if (c->pin_event) (void)hipEventDestroy(c->pin_event);
    if (c->pin) (void)hipHostFree(c->pin);
    if (c->ev0) {
        for (int i = 0; i < blsgpu_ctx::TIMING_SLOTS; i++) { (void)hipEventDestroy(c->ev0[i]); (void)hipEventDestroy(c->ev1[i]); }
        delete[] c->ev0; delete[] c->ev1; delete[] c->ev_kind;
    }
    delete c;
}

BLSGPU_EXPORT int blsgpu_timing_enable(blsgpu_ctx* c, int enable) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    if (enable && !c->ev0) {
        c->ev0 = new hipEvent_t[blsgpu_ctx::TIMING_SLOTS];
        c->ev1 = new hipEvent_t[blsgpu_ctx::TIMING_SLOTS];
        c->ev_kind = new int[blsgpu_ctx::TIMING_SLOTS];
        for (int i = 0; i < blsgpu_ctx::TIMING_SLOTS; i++) { HIP_TRY(hipEventCreate(&c->ev0[i])); HIP_TRY(hipEventCreate(&c->ev1[i])); }
    }
    c->timing = enable != 0;
    c->ev_count = 0;
    return 0;
}

BLSGPU_EXPORT int blsgpu_timing_read(blsgpu_ctx* c, float* ms, int* kind, size_t cap, size_t* count) {
    if (!c || !count) return fail(-EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    size_t n = c->ev_count < cap ? c->ev_count : cap;
    for (size_t i = 0; i < n; i++) {
        HIP_TRY(hipEventSynchronize(c->ev1[i]));
        HIP_TRY(hipEventElapsedTime(&ms[i], c->ev0[i], c->ev1[i]));
        kind[i] = c->ev_kind[i];
    }
    *count = n;
    c->ev_count = 0;
    return 0;
}

// The chip's v_mad_i64_i32 rate right now: a probe kernel of about `target_ms` milliseconds (2048 workgroups x 256 threads, eight
// independent multiply-add chains per lane), timed with HIP events on `stream`; *tmacs = 10^12 multiply-adds per second.
BLSGPU_EXPORT int blsgpu_timing_mad_probe(blsgpu_ctx* c, double target_ms, double* tmacs, void* stream) {
    if (!c || !tmacs) return fail(-EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    constexpr unsigned BLOCKS = 2048, THREADS = 256;
    if (int rc = c->grow(B_IO, (size_t)BLOCKS * THREADS * 4)) return rc;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    double rate = 0.0;
    uint32_t iters = 20000;                                   // ~2.4 ms at 34 T/s: calibrates the second launch
    for (int pass = 0; pass < 2; pass++) {
        HIP_TRY(hipEventRecord(e0, st));
        hipLaunchKernelGGL(blsgpu::probe::k_mad_probe, dim3(BLOCKS), dim3(THREADS), 0, st, c->at<uint32_t>(B_IO), iters, (uint32_t)pass);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(e1, st));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        rate = (double)BLOCKS * THREADS * 8.0 * iters / (ms * 1e-3) / 1e12;
        if (pass == 0 && ms > 0.f) {
            double want = (double)iters * target_ms / ms;
            iters = want < 1000.0 ? 1000u : (want > 4e6 ? 4000000u : (uint32_t)want);
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *tmacs = rate;
    return 0;
}

// One dispatch of an empty kernel (blsgpu::probe::k_mark) on `stream`: a caller brackets its timed region with two of them so that
// a profile of the run can be cut to that region (the counters of rocprofv3 --pmc are per dispatch).
BLSGPU_EXPORT int blsgpu_timing_mark(blsgpu_ctx* c, unsigned tag, void* stream) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(blsgpu::probe::k_mark, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint32_t)tag);
    HIP_TRY(hipGetLastError());
    return 0;
}

BLSGPU_EXPORT int blsgpu_ctx_set_mp_threshold(blsgpu_ctx* c, size_t pairs) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    c->mp_threshold = pairs;
    return 0;
}
// Calls of at least `pairs` pairs whose groups all have at least `min_group` pairs run the line-stream kernels
// (blsgpu_ml.hip); (size_t)-1 for `pairs` keeps every call on the wavefront-VM kernels.
BLSGPU_EXPORT int blsgpu_ctx_set_ls_threshold(blsgpu_ctx* c, size_t pairs, size_t min_group) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    c->ls_threshold = pairs;
    c->ls_min_group = min_group ? min_group : 1;
    return 0;
}
// The caller's event (or NULL: none) is recorded on the call's stream right after the last kernel of a Miller stage that
// fills the chip; what follows (Horner, the product of the partials, the final exponentiation) occupies a few dozen
// wavefronts.  A server that pipelines calls over several contexts lets the next call's stream wait for this event
// instead of the end of the call.
// Calls with at least `results` final exponentiations run them six lanes per result on the register arithmetic
// (blsgpu_fexp.hip); fewer keep one wavefront each on the VM (lower latency).  (size_t)-1: never.
BLSGPU_EXPORT int blsgpu_ctx_set_fexp_team_threshold(blsgpu_ctx* c, size_t results) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    c->fexp_team_threshold = results;
    return 0;
}
// Diagnostic (tools/exact_trace.py): copies the first `bytes` bytes of the line records of the last line-stream call.
BLSGPU_EXPORT int blsgpu_debug_read_lines(blsgpu_ctx* c, void* host_buf, size_t bytes) {
    if (!c || !host_buf) return fail(-EINVAL, "NULL argument");
    if (bytes > c->buf[B_LINES].cap) return fail(-EINVAL, "more than the buffer holds");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_buf, c->buf[B_LINES].p, bytes, hipMemcpyDeviceToHost));
    return 0;
}
// Diagnostic (tools/fexp_trace.py): device buffer of BLS28_FEXP_NOPS x 576 bytes that receives the accumulator of
// result 0 after every operation of the batched final exponentiation's script, or NULL.
BLSGPU_EXPORT int blsgpu_ctx_set_fexp_trace(blsgpu_ctx* c, void* d_buf) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    c->d_fexp_dbg = d_buf;
    return 0;
}
// Diagnostic (tools/fexpw_stamps.py): device buffer of (BLS28_FEXP_NOPS + 1) x 8 bytes that receives the cycle counter of result 0
// before the one-result-per-wavefront final exponentiation's script and after every operation of it, or NULL.
BLSGPU_EXPORT int blsgpu_ctx_set_fexpw_stamps(blsgpu_ctx* c, void* d_buf) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    c->d_fexpw_stamps = d_buf;
    return 0;
}
BLSGPU_EXPORT int blsgpu_ctx_set_bulk_event(blsgpu_ctx* c, void* event) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    c->bulk_event = (hipEvent_t)event;
    return 0;
}
// accumulators (six lanes each) the line-stream product kernel aims at; decides the chunk of pairs per accumulator
BLSGPU_EXPORT int blsgpu_ctx_set_ls_teams(blsgpu_ctx* c, size_t teams) {
    if (!c || teams == 0) return fail(-EINVAL, "bad argument");
    c->ls_teams = teams;
    return 0;
}
// Calls of at most `pairs` pairs (that do not take the line-stream kernels) run the wide Miller loop; 0: never.
BLSGPU_EXPORT int blsgpu_ctx_set_miller_wide_max(blsgpu_ctx* c, size_t pairs) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    c->miller_wide_max = pairs;
    return 0;
}
BLSGPU_EXPORT int blsgpu_ctx_set_mp3_threshold(blsgpu_ctx* c, size_t pairs) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    c->mp3_threshold = pairs;
    return 0;
}

BLSGPU_EXPORT int blsgpu_ctx_reserve(blsgpu_ctx* c, size_t max_pairs) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    const pairing::ReservePlan p = pairing::plan_reserve(*c, PAIRING_CONSTS, pairing_limits(c), max_pairs);
    if (int rc = ensure_partials(c, p.partials)) return rc;
    // the line-stream stage's buffers as well (a call of that size takes them); a call that needs more grows them itself
    if (p.ls && (c->grow(B_LINES, p.lines_bytes) || c->grow(B_BAD, p.bad_bytes) || c->grow(B_DEGEN, p.degen_bytes) ||
                 c->grow(B_LSP0, p.lsp0_bytes) || c->grow(B_LSP1, p.lsp1_bytes))) {
        (void)hipGetLastError();
        return fail(-ENOMEM, "no memory for the line-stream workspace (calls of that size will use the wavefront-VM kernels)");
    }
    return 0;
}

// Bytes of HBM the context holds, by purpose (grow-only buffers: the high-water mark of the calls made so far).
BLSGPU_EXPORT int blsgpu_ctx_workspace_bytes(blsgpu_ctx* c, size_t out[BLSGPU_WS_FIELDS]) {
    if (!c || !out) return fail(-EINVAL, "NULL argument");
    for (int i = 0; i < BLSGPU_WS_FIELDS; i++) out[i] = 0;
    size_t total = (c->d_fix_table ? blsgpu::g1fix::TABLE_BYTES : 0) + (c->d_fix_table_secret ? blsgpu::g1fix::S_TABLE_BYTES : 0);
    for (int b = 0; b < B_COUNT; b++) {
        const size_t bytes = c->buf[b].cap / BUF_INFO[b].unit * BUF_INFO[b].unit;
        if (BUF_INFO[b].ws_field != BLSGPU_WS_TOTAL) out[BUF_INFO[b].ws_field] += bytes;
        total += bytes;
    }
    out[BLSGPU_WS_TOTAL] = total;
    return 0;
}

// Waits for the context's enqueued work and releases the buffers that larger ones replaced.
BLSGPU_EXPORT int blsgpu_ctx_trim(blsgpu_ctx* c) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    if (c->used && c->last_event) HIP_TRY(hipEventSynchronize(c->last_event));
    for (void* q : c->retired) (void)hipFree(q);
    c->retired.clear();
    return 0;
}

// `groups` results at once: product of the m partials of each group (partial i of group g at
// d_in[(i * istride + g * gstride) * 144]) and its final exponentiation in registers, in the form pairing::fexp_form chose:
// six lanes per result (blsgpu_fexp.hip), or -- fewer results than the team form wants -- one result per wavefront
// (blsgpu_fexpw.hip), the latency form.
static int launch_fexp(blsgpu_ctx* c, const pairing::FexpForm& f, const uint32_t* d_in, size_t m, size_t istride, size_t gstride, size_t groups,
                       void* d_out_bytes, hipStream_t st) {
    using namespace blsgpu;
    if (f.kind == pairing::FEXP_TEAM) {
        const WaveShape ws = wave_shape(c, f.waves);
        // every launched wavefront owns rows of the workspace
        if (int rc = c->grow(B_FEXP_WS, (size_t)ws.blocks * (ws.threads / 64) * f.ws_bytes_per_wave)) return rc;
        KernelTimer kt(c, st, 2);
        hipLaunchKernelGGL(fx::k_fexp_team, dim3(ws.blocks), dim3(ws.threads), 0, st, d_in, (uint32_t)m, (uint32_t)istride, (uint32_t)gstride,
                           (uint32_t)groups, c->at<int32_t>(B_FEXP_WS), (uint32_t*)d_out_bytes, (uint32_t*)c->d_fexp_dbg);
    } else {
        KernelTimer kt(c, st, 2);
        hipLaunchKernelGGL(fxw::k_fexp_wide, dim3((unsigned)groups), dim3(64), 0, st, d_in, (uint32_t)m, (uint32_t)istride,
                           (uint32_t)gstride, (uint32_t*)d_out_bytes, (unsigned long long*)c->d_fexpw_stamps);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
// ... in that form, or where there is none on the VM (k_final_groups: one wavefront per result, m partials side by side);
// timed: the VM's launch is timed too
static int launch_final(blsgpu_ctx* c, const pairing::FexpForm& f, const uint32_t* d_in, size_t m, size_t istride, size_t gstride, size_t groups,
                        void* d_out_bytes, hipStream_t st, bool timed = true) {
    if (f.kind != pairing::FEXP_NONE) return launch_fexp(c, f, d_in, m, istride, gstride, groups, d_out_bytes, st);
    {
        std::optional<KernelTimer> kt;
        if (timed) kt.emplace(c, st, 2);
        hipLaunchKernelGGL(blsgpu::k_final_groups, dim3(pairing::final_blocks(PAIRING_CONSTS, groups)), dim3(REDUCE_WAVES * 64),
                           (size_t)REDUCE_WAVES * blsgpu::TEAM_BYTES, st, c->tabs, d_in, (uint32_t)m, (uint32_t)groups, (uint32_t*)d_out_bytes);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// For each of `groups` groups fold its m partials down to one (pairing::plan_reduce); the last launch
// optionally applies the final exponentiation and writes 576 bytes per group to
// d_out_bytes, otherwise one partial per group to d_out_partial.  Partial i of
// group g is read from d_in[(i * istride + g * gstride) * 144].
static int reduce_chain(blsgpu_ctx* c, const uint32_t* d_in, size_t m, size_t groups, size_t istride, size_t gstride,
                        bool do_final, uint32_t* d_out_partial, void* d_out_bytes, hipStream_t st) {
    const pairing::ReducePlan p = pairing::plan_reduce(*c, PAIRING_CONSTS, m, groups, istride, gstride, do_final, d_in == c->part(0), c->part_cap());
    if (p.refusal) return refuse(p.refusal);
    const uint32_t* const bufs[] = {d_in, c->part(0), c->part(1), d_out_partial};
    const uint32_t* src = d_in;
    for (const pairing::ReduceLevel* l = p.level; l != p.level + p.nlevels; l++) {
        uint32_t* dst = (uint32_t*)bufs[l->dst];
        {
            KernelTimer kt(c, st, l->timer);
            hipLaunchKernelGGL(blsgpu::k_reduce, dim3((unsigned)l->blocks, (unsigned)groups), dim3(REDUCE_WAVES * 64), p.lds, st, c->tabs,
                               src, (uint32_t)l->m, (uint32_t)REDUCE_PER_BLOCK, (uint32_t)l->istride, (uint32_t)l->gstride, dst,
                               (uint32_t)l->final_flag, (uint32_t*)d_out_bytes);
        }
        HIP_TRY(hipGetLastError());
        src = dst;
    }
    if (p.end == pairing::R_REDUCE) return 0;
    return launch_fexp(c, p.fexp, bufs[p.fsrc], p.fm, p.fistride, p.fgstride, groups, d_out_bytes, st);
}

// Miller loops of `groups` runs of gsz pairs on the kernel pairing::plan_miller chose; *bpg_out: the partials per group.
// Then the blocks that met a degenerate pair once more with the reference-faithful program (normally none: every wavefront
// leaves at once).
// The caller has sized the workspace for plan_miller(...).bpg x groups partials (ensure_partials) BEFORE it took d_partials:
// nothing grows here -- a grown buffer would leave that pointer on a retired one -- and a launch that does not fit fails.
static int launch_miller(blsgpu_ctx* c, const void* d_g1, const void* d_g2, const void* d_inf, size_t gsz, size_t groups, bool one_per_block,
                         uint32_t* d_partials, hipStream_t st, size_t* bpg_out, int team = 0) {
    using namespace pairing;
    const MillerPlan p = plan_miller(*c, PAIRING_CONSTS, gsz, groups, one_per_block, team, d_partials == c->part(0) || d_partials == c->part(1),
                                     c->part_cap(), c->degen_cap());
    *bpg_out = p.bpg;
    if (p.refusal) return refuse(p.refusal);
    const uint32_t *g1 = (const uint32_t*)d_g1, *g2 = (const uint32_t*)d_g2;
    blsgpu::DegenList dg{c->at<uint32_t>(B_DEGEN), c->at<uint32_t>(B_DEGEN) + 1, (const uint8_t*)d_inf};
    HIP_TRY(hipMemsetAsync(c->at<uint32_t>(B_DEGEN), 0, sizeof(uint32_t), st));
    {
        KernelTimer kt(c, st, 0);
        switch (p.kernel) {
        case M_WIDE3: hipLaunchKernelGGL(blsgpu::mlw::k_miller_wide<3>, dim3(p.grid), dim3(p.threads), p.lds, st, g1, g2, (uint32_t)p.pairs, d_partials, dg); break;
        case M_WIDE2: hipLaunchKernelGGL(blsgpu::mlw::k_miller_wide<2>, dim3(p.grid), dim3(p.threads), p.lds, st, g1, g2, (uint32_t)p.pairs, d_partials, dg); break;
        case M_MP2:
            hipLaunchKernelGGL(blsgpu::k_miller_mp<2>, dim3(p.grid), dim3(p.threads), p.lds, st, c->tabs, g1, g2, (uint32_t)gsz, (uint32_t)p.bpg, d_partials, dg);
            break;
        case M_MP3:
            hipLaunchKernelGGL(blsgpu::k_miller_mp<BLSVM_MP_G>, dim3(p.grid), dim3(p.threads), p.lds, st, c->tabs, g1, g2, (uint32_t)gsz, (uint32_t)p.bpg, d_partials, dg);
            break;
        case M_VM:
            hipLaunchKernelGGL(blsgpu::k_miller, dim3(p.grid), dim3(p.threads), p.lds, st, c->tabs, g1, g2, (uint32_t)gsz, (uint32_t)p.bpg, d_partials, dg);
            break;
        }
    }
    HIP_TRY(hipGetLastError());
    if (c->bulk_event) HIP_TRY(hipEventRecord(c->bulk_event, st));
    // The listed blocks once more, exactly: the reference's own line values of their pairs on lane pairs
    // (k_ml_lines_exact, block mode) and one six-lane accumulator per block over them (k_ml_small, list mode) -- 1.5 ms
    // where the VM's slow program (k_miller_slow: one pair at a time per wavefront, 68 lane-serial inversions each)
    // takes 6 ms per PAIR.  Both kernels leave at once when the list is empty.
    if (p.exact_lanes && !c->grow(B_LINES, p.lines_bytes) && !c->grow(B_BAD, p.bad_bytes)) {
        KernelTimer kt(c, st, 3);
        hipLaunchKernelGGL(blsgpu::ml::k_ml_lines_exact, dim3(1024), dim3(64), 0, st, g1, g2, (uint32_t)p.nv,
                           c->at<int32_t>(B_LINES), c->at<uint8_t>(B_BAD), dg, (uint32_t)gsz, (uint32_t)p.bpg, (uint32_t)p.per_block);
        hipLaunchKernelGGL(blsgpu::ml::k_ml_small, dim3(p.small_grid), dim3(64), 0, st,
                           c->at<int32_t>(B_LINES), c->at<uint8_t>(B_BAD), (uint32_t)p.nv, (uint32_t)p.per_block, (uint32_t)p.blocks,
                           d_partials, 144u, (const uint32_t*)dg.count, (const uint32_t*)dg.blocks);
    } else {
        (void)hipGetLastError();
        KernelTimer kt(c, st, 3);
        hipLaunchKernelGGL(blsgpu::k_miller_slow, dim3(SLOW_GRID), dim3(64), (size_t)blsgpu::SLOW_TEAM_BYTES, st, c->tabs,
                           g1, g2, (uint32_t)gsz, (uint32_t)p.bpg, (uint32_t)p.per_block, d_partials, dg);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// The chain part of the line-stream stage, shared by launch_miller_ls and the ragged multi-pairing: room for the line records,
// the flags and the work list of p.n pairs, the work list reset, the point chains on the kernel plan_ls chose and the listed
// pairs once more with the reference's own formulas.  Leaves 68 line records and a `bad` flag per pair in B_LINES / B_BAD.
// -ENOMEM (nothing enqueued): the buffers cannot be had.
static int launch_ls_chains(blsgpu_ctx* c, const pairing::LsPlan& p, const void* d_g1, const void* d_g2, const void* d_inf, hipStream_t st) {
    using namespace blsgpu;
    if (c->test_ls_nomem ||                                // tests/test_gpu_alternate_forms.py: the callers' -ENOMEM paths, without exhausting a GPU
        c->grow(B_LINES, p.lines_bytes) || c->grow(B_BAD, p.bad_bytes) || c->grow(B_DEGEN, p.degen_bytes)) {
        (void)hipGetLastError();
        return -ENOMEM;
    }
    const uint32_t *g1 = (const uint32_t*)d_g1, *g2 = (const uint32_t*)d_g2, n = (uint32_t)p.n;
    int32_t* const lines = c->at<int32_t>(B_LINES);
    uint8_t* const bad = c->at<uint8_t>(B_BAD);
    DegenList dg{c->at<uint32_t>(B_DEGEN), c->at<uint32_t>(B_DEGEN) + 1, (const uint8_t*)d_inf};
    HIP_TRY(hipMemsetAsync(c->at<uint32_t>(B_DEGEN), 0, sizeof(uint32_t), st));
    {
        KernelTimer kt(c, st, 4);
        if (p.chain == pairing::L_WIDE16) {              // a few thousand pairs: sixteen lanes each, the values in LDS, a product per lane
            hipLaunchKernelGGL(lsw::k_ml_lines_wide, dim3(p.chain_grid), dim3(256), 0, st, g1, g2, n, lines, bad, dg);
        } else {                                         // four lanes each (few pairs), or two
            const WaveShape ws = wave_shape(c, p.chain_waves);
            if (p.chain == pairing::L_QUAD)
                hipLaunchKernelGGL(ml::k_ml_lines4, dim3(ws.blocks), dim3(ws.threads), ws.threads * ml::sp::SLAB_BYTES_PER_LANE, st, g1, g2, n, lines, bad, dg);
            else
                hipLaunchKernelGGL(ml::k_ml_lines2, dim3(ws.blocks), dim3(ws.threads), ws.threads * ml::sp::SLAB_BYTES_PER_LANE, st, g1, g2, n, lines, bad, dg);
        }
    }
    HIP_TRY(hipGetLastError());
    {   // the listed pairs once more with the reference's own formulas: their line records are rewritten (leaves at once
        // when the list is empty)
        KernelTimer kt(c, st, 3);
        hipLaunchKernelGGL(ml::k_ml_lines_exact, dim3(2048), dim3(64), 0, st, g1, g2, n, lines, bad, dg, 0u, 0u, 0u);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// The line-stream form of launch_miller (blsgpu_ml.hip, pairing::plan_ls): ONE partial per group comes out (bpg = 1).
// d_fused_out (optional): the caller wants nothing but the final exponentiation of each group's product -- the kernel
// that ends the stage (k_ml_horner_fexp) then goes on to it in place: no partial, no further launch; *fused tells.
// one_per_group: one accumulator per group whatever ls_min_group says (blsgpu_miller_loop_batch_dev: a group is a pair).
static int launch_miller_ls(blsgpu_ctx* c, const void* d_g1, const void* d_g2, const void* d_inf, size_t gsz, size_t groups,
                            uint32_t* d_partials, hipStream_t st, void* d_fused_out = nullptr, bool* fused = nullptr,
                            bool one_per_group = false) {
    using namespace blsgpu;
    const pairing::LsPlan p = pairing::plan_ls(*c, PAIRING_CONSTS, gsz, groups, one_per_group, d_fused_out != nullptr);
    if (!c->test_ls_nomem && (c->grow(B_LSP0, p.lsp0_bytes) || c->grow(B_LSP1, p.lsp1_bytes))) {
        (void)hipGetLastError();
        return -ENOMEM;                                    // the caller falls back to the wavefront-VM kernels
    }
    if (int rc = launch_ls_chains(c, p, d_g1, d_g2, d_inf, st)) return rc;   // (-ENOMEM likewise)
    const uint32_t n = (uint32_t)p.n;
    int32_t* const lines = c->at<int32_t>(B_LINES);
    uint8_t* const bad = c->at<uint8_t>(B_BAD);
    if (p.small) {
        {
            KernelTimer kt(c, st, 5);
            const WaveShape ws = wave_shape(c, p.small_waves);
            hipLaunchKernelGGL(ml::k_ml_small, dim3(ws.blocks), dim3(ws.threads), 0, st, lines, bad, n, (uint32_t)gsz, (uint32_t)groups, d_partials, 144u,
                               (const uint32_t*)nullptr, (const uint32_t*)nullptr);
        }
        HIP_TRY(hipGetLastError());
        if (c->bulk_event) HIP_TRY(hipEventRecord(c->bulk_event, st));
        return 0;
    }
    {
        KernelTimer kt(c, st, 5);
        const WaveShape ws = wave_shape(c, p.accum_waves);
        hipLaunchKernelGGL(ml::k_ml_accum, dim3(ws.blocks), dim3(ws.threads), 0, st, lines, bad, n, (uint32_t)gsz, (uint32_t)p.chunk, (uint32_t)p.cpg,
                           (uint32_t)p.accum_teams, c->lsp(0));
    }
    HIP_TRY(hipGetLastError());
    for (const pairing::Merge* m = p.merge; m != p.merge + p.nmerges; m++) {
        KernelTimer kt(c, st, 6);
        if (m->wide)                                       // few outputs: one wavefront each, a product per lane
            hipLaunchKernelGGL(fxw::k_ml_merge_wide, dim3((unsigned)m->teams), dim3(64), 0, st, c->lsp(m->src), (uint32_t)m->cpg,
                               (uint32_t)LS_MERGE_FAN, (uint32_t)m->cpo, c->lsp(m->dst));
        else {
            const WaveShape ws = wave_shape(c, m->waves);
            hipLaunchKernelGGL(ml::k_ml_merge, dim3(ws.blocks), dim3(ws.threads), 0, st, c->lsp(m->src), (uint32_t)m->cpg, (uint32_t)LS_MERGE_FAN,
                               (uint32_t)m->cpo, (uint32_t)m->teams, c->lsp(m->dst));
        }
        HIP_TRY(hipGetLastError());
    }
    if (c->bulk_event) HIP_TRY(hipEventRecord(c->bulk_event, st));
    {
        KernelTimer kt(c, st, p.fuse ? 2 : 7);
        hipLaunchKernelGGL(fxw::k_ml_horner_fexp, dim3((unsigned)groups), dim3(64), 0, st, c->lsp(p.last), d_partials, 144u,
                           (uint32_t*)(p.fuse ? d_fused_out : nullptr));
        if (fused) *fused = p.fuse;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// A call's arrays from pair `lo` on -- the points and the flags (when given) -- and an array of 576-byte partials or results
// (when given) from result `res` on
struct PairArrays { const char *g1, *g2, *inf; };
static PairArrays pairs_at(const void* d_g1, const void* d_g2, const void* d_inf, size_t lo) {
    const pairing::SliceOffsets o = pairing::slice_offsets(lo, 0);
    return {(const char*)d_g1 + o.g1, (const char*)d_g2 + o.g2, d_inf ? (const char*)d_inf + o.inf : nullptr};
}
static char* result_at(void* d, size_t res) { return d ? (char*)d + pairing::slice_offsets(0, res).res : nullptr; }

// Miller loops + per-group product; final exponentiation iff d_out_bytes (pairing::plan_grouped)
static int grouped_pairing(blsgpu_ctx* c, const void* d_g1, const void* d_g2, const void* d_inf, size_t gsz, size_t groups,
                           uint32_t* d_out_partial, void* d_out_bytes, hipStream_t st) {
    const pairing::GroupedPlan p = pairing::plan_grouped(*c, PAIRING_CONSTS, pairing_limits(c), gsz, groups, d_out_bytes != nullptr, d_out_partial != nullptr);
    if (p.outer)                                           // groups ride on gridDim.y: larger batches go in slices
        return for_slices(groups, p.outer, [&](size_t g0, size_t gn) {
            const PairArrays a = pairs_at(d_g1, d_g2, d_inf, g0 * gsz);
            return grouped_pairing(c, a.g1, a.g2, a.inf, gsz, gn, (uint32_t*)result_at(d_out_partial, g0), result_at(d_out_bytes, g0), st);
        });
    if (int rc = ensure_partials(c, p.partials)) return rc;
    // the line-stream stage: a slice that finds no memory for its line records (-ENOMEM) leaves the call to the VM kernels
    int rc = -ENOMEM;
    switch (p.ls) {
    case pairing::LS_OFF: case pairing::LS_VM_LONG_GROUPS: break;
    case pairing::LS_WHOLE: {
        bool fused = false;
        uint32_t* target = p.direct ? d_out_partial : c->part(0);
        rc = launch_miller_ls(c, d_g1, d_g2, d_inf, gsz, groups, target, st, d_out_bytes, &fused);
        if (rc == 0 && (fused || p.direct)) return 0;      // (fused: the stage's last kernel ran the final exponentiations too)
        break;
    }
    case pairing::LS_GROUP_SLICES:
        rc = for_slices(groups, p.per, [&](size_t g0, size_t gn) {
            const PairArrays a = pairs_at(d_g1, d_g2, d_inf, g0 * gsz);
            return launch_miller_ls(c, a.g1, a.g2, a.inf, gsz, gn, (uint32_t*)result_at(c->part(0), g0), st);
        });
        break;
    case pairing::LS_RUN_SLICES:
        rc = for_slices(gsz, p.run_len, [&](size_t p0, size_t pn) {
            const PairArrays a = pairs_at(d_g1, d_g2, d_inf, p0);
            return launch_miller_ls(c, a.g1, a.g2, a.inf, pn, 1, (uint32_t*)result_at(c->part(0), p0 / p.run_len), st);
        });
        break;
    }
    size_t bpg = p.ls_bpg;
    if (rc == -ENOMEM) {
        bpg = 0;
        if (gsz > 0)
            if (int rc2 = launch_miller(c, d_g1, d_g2, d_inf, gsz, groups, false, c->part(0), st, &bpg)) return rc2;
    } else if (rc) {
        return rc;
    }
    return reduce_chain(c, c->part(0), bpg, groups, 1, bpg, d_out_bytes != nullptr, d_out_partial, d_out_bytes, st);
}

BLSGPU_EXPORT int blsgpu_miller_product_dev(blsgpu_ctx* c, const void* d_g1, const void* d_g2, const void* d_inf, size_t n,
                              void* d_partial, void* stream) {
    return blsgpu_miller_product_batch_dev(c, d_g1, d_g2, d_inf, n, 1, d_partial, stream);
}

BLSGPU_EXPORT int blsgpu_miller_product_batch_dev(blsgpu_ctx* c, const void* d_g1, const void* d_g2, const void* d_inf, size_t gsz,
                                                  size_t groups, void* d_partials, void* stream) {
    if (!c || (groups && !d_partials)) return fail(-EINVAL, "NULL argument");
    if (groups == 0) return 0;
    if (gsz > 0 && (!d_g1 || !d_g2)) return fail(-EINVAL, "NULL point buffer");
    if (gsz > 0xFFFFFFF0ull || gsz * groups > 0xFFFFFFF0ull) return fail(-EINVAL, "batch too large");
    HIP_TRY(hipSetDevice(c->device));
    StreamGuard sg(c, (hipStream_t)stream);
    return grouped_pairing(c, d_g1, d_g2, d_inf, gsz, groups, (uint32_t*)d_partials, nullptr, (hipStream_t)stream);
}

BLSGPU_EXPORT int blsgpu_final_exp_product_dev(blsgpu_ctx* c, const void* d_partials, size_t m, void* d_out, void* stream) {
    return blsgpu_final_exp_product_batch_dev(c, d_partials, m, 1, d_out, stream);
}

// d_partials holds m x groups partials, partial (i, g) at index i * groups + g: the
// layout an all-gather of every rank's `groups` partials produces.
BLSGPU_EXPORT int blsgpu_final_exp_product_batch_dev(blsgpu_ctx* c, const void* d_partials, size_t m, size_t groups, void* d_out,
                                                     void* stream) {
    if (!c || (groups && !d_out)) return fail(-EINVAL, "NULL argument");
    if (groups == 0) return 0;
    if (m > 0 && !d_partials) return fail(-EINVAL, "NULL partials");
    HIP_TRY(hipSetDevice(c->device));
    StreamGuard sg(c, (hipStream_t)stream);
    if (int rc = ensure_partials(c, pairing::product_partials(PAIRING_CONSTS, m, groups))) return rc;
    return reduce_chain(c, (const uint32_t*)d_partials, m, groups, groups, 1, true, nullptr, d_out, (hipStream_t)stream);
}

BLSGPU_EXPORT int blsgpu_pairing_multi_dev(blsgpu_ctx* c, const void* d_g1, const void* d_g2, const void* d_inf, size_t n,
                             void* d_out, void* stream) {
    if (!c || !d_out) return fail(-EINVAL, "NULL argument");
    if (n > 0 && (!d_g1 || !d_g2)) return fail(-EINVAL, "NULL point buffer");
    if (n > 0xFFFFFFF0ull) return fail(-EINVAL, "n too large");
    HIP_TRY(hipSetDevice(c->device));
    StreamGuard sg(c, (hipStream_t)stream);
    return grouped_pairing(c, d_g1, d_g2, d_inf, n, 1, nullptr, d_out, (hipStream_t)stream);
}

BLSGPU_EXPORT int blsgpu_pairing_multi(blsgpu_ctx* c, const uint8_t* g1, const uint8_t* g2, const uint8_t* inf, size_t n,
                                       uint8_t out[576]) {
    if (!c || !out) return fail(-EINVAL, "NULL argument");
    if (n > 0 && (!g1 || !g2)) return fail(-EINVAL, "NULL point buffer");
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int d1 = s.in(g1, n * BLSGPU_G1_BYTES), d2 = s.in(g2, n * BLSGPU_G2_BYTES), di = s.in(inf, n * 2);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = blsgpu_pairing_multi_dev(c, s.at(d1), s.at(d2), s.opt(di), n, c->d_out, nullptr)) return rc;
    HIP_TRY(hipMemcpy(out, c->d_out, BLSGPU_FQ12_BYTES, hipMemcpyDeviceToHost));
    return 0;
}

// fq_miller_loop (fields_t.py:1091-1111) of every pair: n x 576 bytes, the reference's own
// Miller values (not multiples of them).
BLSGPU_EXPORT int blsgpu_miller_loop_batch_dev(blsgpu_ctx* c, const void* d_g1, const void* d_g2, const void* d_inf, size_t n,
                                               void* d_out, void* stream) {
    if (!c || (n && (!d_g1 || !d_g2 || !d_out))) return fail(-EINVAL, "NULL argument");
    if (n == 0) return 0;
    if (n > 0x7FFFFFF0ull) return fail(-EINVAL, "n too large");
    HIP_TRY(hipSetDevice(c->device));
    StreamGuard sg(c, (hipStream_t)stream);
    using namespace blsgpu;
    const hipStream_t st = (hipStream_t)stream;
    const pairing::ExactPlan p = pairing::plan_exact(PAIRING_CONSTS, pairing_limits(c), n);
    // slice [lo, lo + m) of the call: its points as words, its flags, its results
    struct Slice { pairing::ExactSlice s; const uint32_t *p1, *p2; const uint8_t* inf; uint32_t* out; };
    const auto slice = [&](size_t lo) {
        const PairArrays a = pairs_at(d_g1, d_g2, d_inf, lo);
        return Slice{p.at(lo), (const uint32_t*)a.g1, (const uint32_t*)a.g2, (const uint8_t*)a.inf, (uint32_t*)result_at(d_out, lo)};
    };
    if (c->miller_exact_lanes) {
        // Round 5: the lane kernels instead of the VM's reference-faithful program (one pair per wavefront, 68 lane-serial inversions:
        // 7 ms for one pair, 158 k pairs/s): every pair on the work list, k_ml_lines_exact writes its 68 lines with the reference's
        // own formulas (a pair per lane pair), k_ml_small multiplies them up with one six-lane accumulator per pair, in slices that
        // keep the line records below 6 GB.
        if (c->miller_exact_fast && c->grow(B_EXFLAGS, p.exflags_bytes) == 0 && ensure_partials(c, p.partials) == 0) {
            // the ordinary line-stream kernels with one accumulator per pair, then one Fq2 factor per pair turns the fast value into the
            // reference's (k_ml_exact_fixup: 73 dependent inversions per pair become one); a pair the fast formulas are not valid for
            // -- or whose py is 0, which the factor divides by -- takes the reference's own lines inside the same launches
            const int rc = for_slices(n, p.slice, [&](size_t lo, size_t m) {
                const Slice s = slice(lo);
                hipLaunchKernelGGL(ml::k_ml_exact_flags, dim3(s.s.g_flags), dim3(256), 0, st, s.p1, s.inf, (uint32_t)m, c->at<uint8_t>(B_EXFLAGS));
                const int rc_ = launch_miller_ls(c, s.p1, s.p2, c->at<uint8_t>(B_EXFLAGS), 1, m, c->part(0), st, nullptr, nullptr, true);
                if (rc_ == -ENOMEM && lo == 0) return 1;                   // no room for the line records: the forms below
                if (rc_) return rc_;
                hipLaunchKernelGGL(ml::k_ml_exact_fixup, dim3(s.s.g_fixup), dim3(256), 0, st, s.p1, c->at<int32_t>(B_LINES),
                                   c->at<uint8_t>(B_BAD), c->part(0), (uint32_t)m, s.out);
                HIP_TRY(hipGetLastError());
                return 0;
            });
            if (rc != 1) return rc;
        }
        if (c->grow(B_LINES, p.lines_bytes) == 0 && c->grow(B_BAD, p.bad_bytes) == 0 && c->grow(B_DEGEN, p.degen_bytes) == 0 &&
            ensure_partials(c, p.partials) == 0)
            return for_slices(n, p.slice, [&](size_t lo, size_t m) {
                const Slice s = slice(lo);
                DegenList dg{c->at<uint32_t>(B_DEGEN), c->at<uint32_t>(B_DEGEN) + 1, s.inf};
                hipLaunchKernelGGL(ml::k_ml_list_all, dim3(s.s.g_list), dim3(256), 0, st, (uint32_t)m, c->at<uint32_t>(B_DEGEN), c->at<uint32_t>(B_DEGEN) + 1);
                hipLaunchKernelGGL(ml::k_ml_lines_exact, dim3(2048), dim3(64), 0, st, s.p1, s.p2, (uint32_t)m, c->at<int32_t>(B_LINES), c->at<uint8_t>(B_BAD), dg, 0u, 0u, 0u);
                const WaveShape ws = wave_shape(c, s.s.small_waves);
                hipLaunchKernelGGL(ml::k_ml_small, dim3(ws.blocks), dim3(ws.threads), 0, st, c->at<int32_t>(B_LINES), c->at<uint8_t>(B_BAD), (uint32_t)m, 1u,
                                   (uint32_t)m, c->part(0), 144u, (const uint32_t*)nullptr, (const uint32_t*)nullptr);
                hipLaunchKernelGGL(ml::k_ml_partials_to_bytes, dim3(s.s.g_bytes), dim3(256), 0, st, c->part(0), (uint32_t)(m * 12), s.out);
                HIP_TRY(hipGetLastError());
                return 0;
            });
        (void)hipGetLastError();                               // no room for the line records: the VM's program below
    }
    hipLaunchKernelGGL(blsgpu::k_miller_exact, dim3(p.vm_grid), dim3(64), (size_t)blsgpu::SLOW_TEAM_BYTES, st, c->tabs,
                       (const uint32_t*)d_g1, (const uint32_t*)d_g2, (const uint8_t*)d_inf, (uint32_t)n, (uint32_t*)d_out);
    HIP_TRY(hipGetLastError());
    return 0;
}
BLSGPU_EXPORT int blsgpu_miller_loop_batch(blsgpu_ctx* c, const uint8_t* g1, const uint8_t* g2, const uint8_t* inf, size_t n,
                                           uint8_t* out) {
    if (!c || (n && (!g1 || !g2 || !out))) return fail(-EINVAL, "NULL argument");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int d1 = s.in(g1, n * BLSGPU_G1_BYTES), d2 = s.in(g2, n * BLSGPU_G2_BYTES), di = s.in(inf, n * 2), dout = s.out(out, n * BLSGPU_FQ12_BYTES);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = blsgpu_miller_loop_batch_dev(c, s.at(d1), s.at(d2), s.opt(di), n, s.at(dout), nullptr)) return rc;
    return s.down();
}

// fq2_double_line_eval (q == NULL) / fq2_add_line_eval on n (R, [Q,] P) triples
BLSGPU_EXPORT int blsgpu_line_eval_batch(blsgpu_ctx* c, const uint8_t* r, const uint8_t* q, const uint8_t* p, size_t n, uint8_t* out) {
    if (!c || (n && (!r || !p || !out))) return fail(-EINVAL, "NULL argument");
    if (n == 0) return 0;
    if (n > 0x00FFFFF0ull) return fail(-EINVAL, "n too large");
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int dr = s.in(r, n * BLSGPU_G2_BYTES), dq = s.in(q, n * BLSGPU_G2_BYTES), dp = s.in(p, n * BLSGPU_G1_BYTES), dout = s.out(out, n * BLSGPU_FQ12_BYTES);
    if (int rc = s.alloc()) return rc;
    StreamGuard sg(c, nullptr);
    if (int rc = s.up()) return rc;
    const unsigned grid = (unsigned)(n < 16384 ? n : 16384);
    hipLaunchKernelGGL(blsgpu::k_line_eval, dim3(grid), dim3(64), (size_t)blsgpu::SLOW_TEAM_BYTES, 0, c->tabs, (const uint32_t*)s.at(dr),
                       (const uint32_t*)s.opt(dq), (const uint32_t*)s.at(dp), (uint32_t)n, (uint32_t*)s.at(dout));
    HIP_TRY(hipGetLastError());
    return s.down();
}

// Fq12 field operations on n elements (op: 0 add, 1 sub, 2 mul, 3 neg, 4 invert), or a^e for one exponent
namespace {
int fq12_op_host(blsgpu_ctx* c, uint32_t op, const uint8_t* a, const uint8_t* b, const uint8_t* ebits, size_t nbits, size_t n, uint8_t* out) {
    if (!c || (n && (!a || !out)) || (n && op <= 2 && !b)) return fail(-EINVAL, "NULL argument");
    if (n == 0) return 0;
    if (n > 0x00FFFFF0ull || nbits > 0x10000) return fail(-EINVAL, "too large");
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int da = s.in(a, n * BLSGPU_FQ12_BYTES), db = s.in(op <= 2 ? b : nullptr, n * BLSGPU_FQ12_BYTES), de = s.in(nbits ? ebits : nullptr, nbits),
              dout = s.out(out, n * BLSGPU_FQ12_BYTES);
    if (int rc = s.alloc()) return rc;
    StreamGuard sg(c, nullptr);
    if (int rc = s.up()) return rc;
    const unsigned grid = (unsigned)(n < 16384 ? n : 16384);
    hipLaunchKernelGGL(blsgpu::k_fq12_op, dim3(grid), dim3(64), (size_t)blsgpu::SLOW_TEAM_BYTES, 0, c->tabs, op, (const uint32_t*)s.at(da),
                       (const uint32_t*)s.at(db), (const uint8_t*)s.at(de), (uint32_t)nbits, (uint32_t)n, (uint32_t*)s.at(dout));
    HIP_TRY(hipGetLastError());
    return s.down();
}
}  // namespace
BLSGPU_EXPORT int blsgpu_fq12_op_batch(blsgpu_ctx* c, int op, const uint8_t* a, const uint8_t* b, size_t n, uint8_t* out) {
    if (op < 0 || op > 4) return fail(-EINVAL, "bad op");
    return fq12_op_host(c, (uint32_t)op, a, b, nullptr, 0, n, out);
}
BLSGPU_EXPORT int blsgpu_fq12_pow_batch(blsgpu_ctx* c, const uint8_t* a, const uint8_t* e_be, size_t e_len, size_t n, uint8_t* out) {
    if (n && (!e_be && e_len)) return fail(-EINVAL, "NULL exponent");
    // exponent bytes (big-endian) -> bits, most significant first, leading zeros dropped
    std::vector<uint8_t> bits;
    bool started = false;
    for (size_t i = 0; i < e_len; i++)
        for (int k = 7; k >= 0; k--) {
            const uint8_t bit = (e_be[i] >> k) & 1;
            started = started || bit;
            if (started) bits.push_back(bit);
        }
    return fq12_op_host(c, 5u, a, nullptr, bits.data(), bits.size(), n, out);
}

// m independent final exponentiations: fq12_final_exp on each 576-byte element
BLSGPU_EXPORT int blsgpu_final_exp_batch(blsgpu_ctx* c, const uint8_t* in, size_t m, uint8_t* out) {
    if (!c || (m && (!in || !out))) return fail(-EINVAL, "NULL argument");
    if (m == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int din = s.in(in, m * 576), dout = s.out(out, m * 576);
    if (int rc = s.alloc()) return rc;
    if (int rc = ensure_partials(c, pairing::fexp_batch_partials(m))) return rc;
    StreamGuard sg(c, nullptr);
    if (int rc = s.up()) return rc;
    hipLaunchKernelGGL(blsgpu::k_bytes_to_partials, dim3(pairing::final_blocks(PAIRING_CONSTS, m)), dim3(REDUCE_WAVES * 64),
                       (size_t)REDUCE_WAVES * blsgpu::TEAM_BYTES, 0, c->tabs, (const uint32_t*)s.at(din), (uint32_t)m, c->part(1));
    HIP_TRY(hipGetLastError());
    if (int rc = launch_final(c, pairing::fexp_form(*c, PAIRING_CONSTS, 1, m), c->part(1), 1, 1, 1, m, s.at(dout), 0, false)) return rc;
    return s.down();
}

BLSGPU_EXPORT int blsgpu_final_exp(blsgpu_ctx* c, const uint8_t in[576], uint8_t out[576]) {
    return blsgpu_final_exp_batch(c, in, 1, out);
}

// `groups` independent multi-pairings of gsz pairs each (pairs stored group after
// group): out[g] = fq_ate_pairing_multi of group g.  One wavefront per pair for
// the Miller loops, one wavefront per group for product + final exponentiation.
BLSGPU_EXPORT int blsgpu_pairing_multi_batch_dev(blsgpu_ctx* c, const void* d_g1, const void* d_g2, const void* d_inf, size_t gsz,
                                                 size_t groups, void* d_out, void* stream) {
    if (!c || (groups && !d_out)) return fail(-EINVAL, "NULL argument");
    if (groups == 0) return 0;
    size_t n = gsz * groups;
    if (n && (!d_g1 || !d_g2)) return fail(-EINVAL, "NULL point buffer");
    if (n > 0x3FFFFFF0ull) return fail(-EINVAL, "batch too large");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    StreamGuard sg(c, st);
    const pairing::BatchPlan p = pairing::plan_batch(*c, PAIRING_CONSTS, pairing_limits(c), gsz, groups);
    if (p.route == pairing::B_TREE) return grouped_pairing(c, d_g1, d_g2, d_inf, gsz, groups, nullptr, d_out, st);
    // every launch below leaves at most one partial per PAIR (plan_miller: bpg x groups <= n whichever kernel runs)
    if (int rc = ensure_partials(c, p.partials)) return rc;
    bool ls = p.route == pairing::B_LS_SMALL;
    if (ls) {
        // a large batch of small groups: point chains on lane pairs, then one accumulator per group (blsgpu_ml.hip)
        const int rc = launch_miller_ls(c, d_g1, d_g2, d_inf, gsz, groups, c->part(0), st);
        if (rc && rc != -ENOMEM) return rc;
        ls = rc == 0;                                      // no memory for the line records: the fallback route
    }
    const pairing::BatchFinal& fin = ls ? p.fin : p.fallback_fin;
    if (n && !ls) {
        // groups of two or three pairs in a batch large enough for the team kernels: the group IS the team (one
        // accumulator, its squarings shared), one partial per group; otherwise one partial per pair
        size_t bpg = 0;
        const int rc = p.fallback == pairing::B_TEAM_GROUPS ? launch_miller(c, d_g1, d_g2, d_inf, gsz, groups, false, c->part(0), st, &bpg, (int)gsz)
                                                            : launch_miller(c, d_g1, d_g2, d_inf, n, 1, true, c->part(0), st, &bpg);
        if (rc) return rc;
    }
    return launch_final(c, fin.fexp, c->part(0), fin.m, fin.istride, fin.gstride, groups, d_out, st);
}

BLSGPU_EXPORT int blsgpu_pairing_multi_batch(blsgpu_ctx* c, const uint8_t* g1, const uint8_t* g2, const uint8_t* inf, size_t gsz,
                                             size_t groups, uint8_t* out) {
    if (!c || (groups && !out)) return fail(-EINVAL, "NULL argument");
    if (groups == 0) return 0;
    size_t n = gsz * groups;
    if (n && (!g1 || !g2)) return fail(-EINVAL, "NULL point buffer");
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int d1 = s.in(g1, n * BLSGPU_G1_BYTES), d2 = s.in(g2, n * BLSGPU_G2_BYTES), di = s.in(inf, n * 2), dout = s.out(out, groups * 576);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = blsgpu_pairing_multi_batch_dev(c, s.at(d1), s.at(d2), s.opt(di), gsz, groups, s.at(dout), nullptr)) return rc;
    return s.down();
}

// The RAGGED multi-pairing: out[j] = fq_ate_pairing_multi of the pairs [begin_j, end_j) of one list, for m ranges of any lengths
// in one launch sequence (pairing_ranges_plan.h is the whole schedule, host arithmetic on the caller's HOST range table; nothing
// is read back).  Per slice of the pair list the point chains and k_ml_ranges -- one six-lane team per chunk of at most
// pair_ranges_chunk pairs --, after the last slice the fold levels, then the final exponentiation of one partial per range.
namespace {
// the argument checks, before anything is written; 1: nothing to do
int pairing_ranges_args(const blsgpu_ctx* c, const void* g1, const void* g2, size_t n, const uint32_t* ranges, size_t m, const void* out) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (m == 0) return 1;
    if (!ranges || !out) return fail(-EINVAL, "NULL argument");
    if (n && (!g1 || !g2)) return fail(-EINVAL, "NULL point buffer");
    return 0;
}
int pairing_ranges_refuse(const pairing_ranges::Plan& p) { return fail(pairing_ranges::refusal_code(p.refusal), pairing_ranges::refusal_text(p.refusal)); }

// every buffer of every slice before the first launch: a later slice cannot fail after an earlier one wrote.  No memory for
// the line records is this call's error -- it has no wavefront-VM form to fall back to.
int pairing_ranges_reserve(blsgpu_ctx* c, const pairing_ranges::Plan& p) {
    if (p.lines_bytes && (c->test_ls_nomem || c->grow(B_LINES, p.lines_bytes) || c->grow(B_BAD, p.bad_bytes) || c->grow(B_DEGEN, p.degen_bytes))) {
        (void)hipGetLastError();
        return fail(-ENOMEM, "no memory for the line records");
    }
    if (int rc = c->grow(B_PAIRR_WS, p.ws_bytes)) return rc;
    const pairing::FexpForm form = pairing::fexp_form(*c, PAIRING_CONSTS, 1, p.m < p.final_step ? p.m : p.final_step);
    if (form.kind == pairing::FEXP_TEAM) {                   // (launch_fexp grows it again: nothing to do then)
        const WaveShape ws = wave_shape(c, form.waves);
        if (int rc = c->grow(B_FEXP_WS, (size_t)ws.blocks * (ws.threads / 64) * form.ws_bytes_per_wave)) return rc;
    }
    return 0;
}

// d_tables: the image of the plan's tables already in device memory (blsgpu_verify_aggregates uploads those of all its slices
// in one copy), or NULL: written here to pinned memory and uploaded
int pairing_ranges_launch(blsgpu_ctx* c, const pairing_ranges::Plan& p, const void* d_g1, const void* d_g2, const void* d_inf, void* d_out,
                          hipStream_t st, const void* d_tables = nullptr) {
    using namespace blsgpu;
    if (int rc = pairing_ranges_reserve(c, p)) return rc;
    char* const W = c->at<char>(B_PAIRR_WS);
    uint32_t* const partials = (uint32_t*)(W + p.o_partials);
    if (d_tables) {
        HIP_TRY(hipMemcpyAsync(W + p.o_tables, d_tables, p.ws_bytes - p.o_tables, hipMemcpyDeviceToDevice, st));
    } else {   // the tables: written to pinned memory that outlives the enqueue, one asynchronous upload
        PinnedTables pin(c);
        void* image = nullptr;
        if (int rc = pin.take(p.ws_bytes - p.o_tables, &image)) return rc;
        p.fill_tables(image);
        if (int rc = pin.upload(W + p.o_tables, p.ws_bytes - p.o_tables, st)) return rc;
    }
    for (const pairing_ranges::Slice& s : p.slices) {
        if (!s.nchunks) continue;
        if (s.chains) {
            const PairArrays a = pairs_at(d_g1, d_g2, d_inf, s.lo);
            if (int rc = launch_ls_chains(c, s.ls, a.g1, a.g2, a.inf, st)) return rc == -ENOMEM ? fail(rc, "no memory for the line records") : rc;
        }
        {
            KernelTimer kt(c, st, 5);
            const WaveShape ws = wave_shape(c, s.waves);
            hipLaunchKernelGGL(ml::k_ml_ranges, dim3(ws.blocks), dim3(ws.threads), 0, st, c->at<int32_t>(B_LINES), c->at<uint8_t>(B_BAD),
                               (uint32_t)(s.chains ? s.pairs : 0), (const uint32_t*)(W + s.tab_off), (uint32_t)s.nchunks, partials);
        }
        HIP_TRY(hipGetLastError());
    }
    if (c->bulk_event) HIP_TRY(hipEventRecord(c->bulk_event, st));
    for (const pairing_ranges::Level& l : p.levels) {
        KernelTimer kt(c, st, 6);
        const WaveShape ws = wave_shape(c, l.waves);
        hipLaunchKernelGGL(ml::k_ml_fold_ranges, dim3(ws.blocks), dim3(ws.threads), 0, st, partials, (const uint32_t*)(W + l.tab_off), (uint32_t)l.nfolds);
        HIP_TRY(hipGetLastError());
    }
    // one partial per result; more results than one launch takes go in slices (as the groups of blsgpu_pairing_multi_batch)
    return for_slices(p.m, p.final_step, [&](size_t lo, size_t mm) {
        return launch_final(c, pairing::fexp_form(*c, PAIRING_CONSTS, 1, mm), (const uint32_t*)result_at(partials, lo), 1, 1, 1, mm, result_at(d_out, lo), st);
    });
}
}  // namespace

BLSGPU_EXPORT int blsgpu_pairing_multi_ranges_dev(blsgpu_ctx* c, const void* d_g1, const void* d_g2, const void* d_inf, size_t n,
                                                  const uint32_t* ranges, size_t m, void* d_out, void* stream) {
    if (int rc = pairing_ranges_args(c, d_g1, d_g2, n, ranges, m, d_out)) return rc < 0 ? rc : 0;
    const pairing_ranges::Plan p = pairing_ranges::plan(n, ranges, m, *c, *c, PAIRING_CONSTS, pairing_limits(c));
    if (p.refusal) return pairing_ranges_refuse(p);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    StreamGuard sg(c, st);
    return pairing_ranges_launch(c, p, d_g1, d_g2, d_inf, d_out, st);
}

BLSGPU_EXPORT int blsgpu_pairing_multi_ranges(blsgpu_ctx* c, const uint8_t* g1, const uint8_t* g2, const uint8_t* inf, size_t n,
                                              const uint32_t* ranges, size_t m, uint8_t* out) {
    if (int rc = pairing_ranges_args(c, g1, g2, n, ranges, m, out)) return rc < 0 ? rc : 0;
    const pairing_ranges::Plan p = pairing_ranges::plan(n, ranges, m, *c, *c, PAIRING_CONSTS, pairing_limits(c));
    if (p.refusal) return pairing_ranges_refuse(p);
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int d1 = s.in(g1, n * BLSGPU_G1_BYTES), d2 = s.in(g2, n * BLSGPU_G2_BYTES), di = s.in(inf, n * 2), dout = s.out(out, m * 576);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    {
        StreamGuard sg(c, nullptr);
        if (int rc = pairing_ranges_launch(c, p, s.at(d1), s.at(d2), s.opt(di), s.at(dout), nullptr)) return rc;
    }
    return s.down();
}

BLSGPU_EXPORT int blsgpu_g1_msm(blsgpu_ctx* c, const uint8_t* pts, const uint8_t* scalars, size_t k, size_t groups,
                                uint8_t* out, uint8_t* out_inf) {
    return msm_host<1>(c, pts, scalars, k, groups, out, out_inf);
}
BLSGPU_EXPORT int blsgpu_g2_msm(blsgpu_ctx* c, const uint8_t* pts, const uint8_t* scalars, size_t k, size_t groups,
                                uint8_t* out, uint8_t* out_inf) {
    return msm_host<2>(c, pts, scalars, k, groups, out, out_inf);
}
BLSGPU_EXPORT int blsgpu_g1_msm_dev(blsgpu_ctx* c, const void* d_pts, const void* d_scalars, size_t k, size_t groups,
                                    void* d_out, void* d_out_inf, void* stream) {
    if (!c || !d_out) return fail(-EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    return msm_dev<1>(c, d_pts, d_scalars, k, groups, d_out, d_out_inf, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_g2_msm_dev(blsgpu_ctx* c, const void* d_pts, const void* d_scalars, size_t k, size_t groups,
                                    void* d_out, void* d_out_inf, void* stream) {
    if (!c || !d_out) return fail(-EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    return msm_dev<2>(c, d_pts, d_scalars, k, groups, d_out, d_out_inf, (hipStream_t)stream);
}

// ------------------------------------------------------------ hash to G2 -----
// t: n x 192 bytes = (t0.c0, t0.c1, t1.c0, t1.c1) canonical big-endian, the four
// hash512 values of ec.py:531-534 reduced mod q; out: n x 192 bytes affine G2.
// from_hashes: d_in = message hashes (n x 32 bytes), else t values (n x 192 bytes)
static int map_to_g2_impl(blsgpu_ctx* c, const void* d_in, size_t n, void* d_out, hipStream_t st, bool from_hashes) {
    if (n == 0) return 0;
    if (n > 0x03FFFFF0ull) return fail(-EINVAL, "batch too large");
    StreamGuard sg(c, st);
    const size_t teams = (2 * n + BLSVM_H1_NE - 1) / BLSVM_H1_NE;
    size_t need = teams * blsgpu::H1_IMG * 12 + (from_hashes ? n * 64 : 0);     // stage image (+ digests), u32
    if (int rc_ = c->grow(B_MSM_PART, need * 4)) return rc_;
    uint32_t* img = c->at<uint32_t>(B_MSM_PART);
    const size_t lds = (size_t)blsgpu::H1_TEAM_DW * 4;
    constexpr uint32_t BASE = BLSVM_H1_BASE - BLSVM_H1_STATE0, ACC = BLSVM_H1_ACC - BLSVM_H1_STATE0;
    const bool lanes = n >= c->h2c_lane_threshold;         // the three encoding stages one encoding per lane (k_h2c_sw*)
    const uint32_t total = (uint32_t)(teams * BLSVM_H1_NE);
    const unsigned lgrid = (unsigned)((total + 63) / 64);
    const WaveShape lsh = wave_shape(c, lgrid);            // the division-step kernels (k_h2c_swj*): any workgroup size
    if (from_hashes) {
        uint32_t* d_dig = img + teams * blsgpu::H1_IMG * 12;
        hipLaunchKernelGGL(blsgpu::k_h2c_hash, dim3((unsigned)((8 * n + 255) / 256)), dim3(256), 0, st, (const uint32_t*)d_in,
                           (uint32_t)n, d_dig);
        HIP_TRY(hipGetLastError());
        if (lanes && c->h2c_jacobi && n >= c->h2c_jacobi_threshold)
            hipLaunchKernelGGL(blsgpu::k_h2c_swj0<1>, dim3(lsh.blocks), dim3(lsh.threads), 0, st, (const uint32_t*)d_dig, (uint32_t)(2 * n), total, img);
        else if (lanes)
            hipLaunchKernelGGL(blsgpu::k_h2c_sw0<1>, dim3(lgrid), dim3(64), 0, st, (const uint32_t*)d_dig, (uint32_t)(2 * n), total, img);
        else
            hipLaunchKernelGGL((blsgpu::k_h2c_stage<0, 1>), dim3((unsigned)teams), dim3(64), lds, st, c->tabs, (const uint32_t*)d_dig,
                               (uint32_t)(2 * n), img);
    } else if (lanes && c->h2c_jacobi && n >= c->h2c_jacobi_threshold) {
        hipLaunchKernelGGL(blsgpu::k_h2c_swj0<0>, dim3(lsh.blocks), dim3(lsh.threads), 0, st, (const uint32_t*)d_in, (uint32_t)(2 * n), total, img);
    } else if (lanes) {
        hipLaunchKernelGGL(blsgpu::k_h2c_sw0<0>, dim3(lgrid), dim3(64), 0, st, (const uint32_t*)d_in, (uint32_t)(2 * n), total, img);
    } else {
        hipLaunchKernelGGL((blsgpu::k_h2c_stage<0, 0>), dim3((unsigned)teams), dim3(64), lds, st, c->tabs, (const uint32_t*)d_in,
                           (uint32_t)(2 * n), img);
    }
    HIP_TRY(hipGetLastError());
    const bool jac = lanes && c->h2c_jacobi && n >= c->h2c_jacobi_threshold;   // two powers per encoding instead of five (swl::jacobi)
    int rc = launch_pow(c, img, blsgpu::H1_IMG, BASE, ACC, teams, (jac ? 1 : 3) * BLSVM_H1_NE, st);
    if (rc) return rc;
    if (jac)
        hipLaunchKernelGGL(blsgpu::k_h2c_swj1, dim3(lsh.blocks), dim3(lsh.threads), 0, st, total, img);
    else if (lanes)
        hipLaunchKernelGGL(blsgpu::k_h2c_sw1, dim3(lgrid), dim3(64), 0, st, total, img);
    else
        hipLaunchKernelGGL((blsgpu::k_h2c_stage<1, 0>), dim3((unsigned)teams), dim3(64), lds, st, c->tabs, (const uint32_t*)nullptr,
                           (uint32_t)(2 * n), img);
    HIP_TRY(hipGetLastError());
    rc = launch_pow(c, img, blsgpu::H1_IMG, BASE, ACC, teams, (jac ? 1 : 2) * BLSVM_H1_NE, st);
    if (rc) return rc;
    if (jac)
        hipLaunchKernelGGL(blsgpu::k_h2c_swj2, dim3(lsh.blocks), dim3(lsh.threads), 0, st, total, img);
    else if (lanes)
        hipLaunchKernelGGL(blsgpu::k_h2c_sw2, dim3(lgrid), dim3(64), 0, st, total, img);
    else
        hipLaunchKernelGGL((blsgpu::k_h2c_stage<2, 0>), dim3((unsigned)teams), dim3(64), lds, st, c->tabs, (const uint32_t*)nullptr,
                           (uint32_t)(2 * n), img);
    HIP_TRY(hipGetLastError());
    if (n <= c->h2c_wide_max && n < c->h2c_reg_threshold) {   // a few messages: one per wavefront, a product per lane (the latency form)
        hipLaunchKernelGGL(blsgpu::h2cw::k_h2c_clear_wide, dim3((unsigned)n), dim3(64), 0, st, c->tabs, img, (uint32_t)n, (uint32_t*)d_out);
    } else if (n < c->h2c_reg_threshold) { // the VM form (BLSVM_H2_NM messages per wavefront)
        unsigned b2 = (unsigned)((n + BLSVM_H2_NM - 1) / BLSVM_H2_NM);
        hipLaunchKernelGGL(blsgpu::k_h2c_clear, dim3(b2), dim3(64), (size_t)blsgpu::H2_TEAM_DW * 4, st, c->tabs, img, (uint32_t)n,
                           (uint32_t*)d_out);
    } else if (n <= c->h2c_quad_max) {   // a batch that leaves SIMDs empty on lane pairs: one message per lane QUAD
        const WaveShape ws = wave_shape(c, (4 * n + 63) / 64);                   // every launched lane owns rows of the workspace
        if (int rc2 = c->grow(B_H2C_WS, (size_t)ws.blocks * ws.threads * BLS28_H2C_NSLOTS * 3 * blsgpu::r28::NL * 4)) return rc2;
        hipLaunchKernelGGL(blsgpu::k_h2c_clear_quads, dim3(ws.blocks), dim3(ws.threads), 0, st, c->tabs, img, (uint32_t)n,
                           c->at<uint32_t>(B_H2C_WS), (uint32_t*)d_out);
    } else {                               // one message per lane pair, the point operations as a script
        const WaveShape ws = wave_shape(c, (2 * n + 63) / 64);
        if (int rc2 = c->grow(B_H2C_WS, (size_t)ws.blocks * ws.threads * BLS28_H2C_NSLOTS * 3 * blsgpu::r28::NL * 4)) return rc2;
        hipLaunchKernelGGL(blsgpu::k_h2c_clear_pairs, dim3(ws.blocks), dim3(ws.threads), 0, st, c->tabs, img, (uint32_t)n,
                           c->at<uint32_t>(B_H2C_WS), (uint32_t*)d_out);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

BLSGPU_EXPORT int blsgpu_map_to_g2_dev(blsgpu_ctx* c, const void* d_t, size_t n, void* d_out, void* stream) {
    if (!c || (n && (!d_t || !d_out))) return fail(-EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    return map_to_g2_impl(c, d_t, n, d_out, (hipStream_t)stream, false);
}

// The whole hash_to_point_prehashed_Fq2 (ec.py:528-550) for 32-byte message hashes.
BLSGPU_EXPORT int blsgpu_hash_to_g2_dev(blsgpu_ctx* c, const void* d_msg_hashes, size_t n, void* d_out, void* stream) {
    if (!c || (n && (!d_msg_hashes || !d_out))) return fail(-EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    return map_to_g2_impl(c, d_msg_hashes, n, d_out, (hipStream_t)stream, true);
}

// ---- the device work of BLS.verify (bls.py:153-201) in one call ----------------------------------------------------------
// d_g1: (n + 1) x 96 bytes, slot 0 = -G1, slots 1 .. n = the per-message keys (given, or written here by the key sums);
// d_g2: (n + 1) x 192 bytes, slot 0 = the aggregate signature, slots 1 .. n written here by the hash to G2.
BLSGPU_EXPORT int blsgpu_verify_pipeline_dev(blsgpu_ctx* c, void* d_g1, void* d_g2, const void* d_msg_hashes, size_t n, const void* d_key_pts,
                                             const void* d_key_scalars, size_t k, void* d_out, void* stream) {
    if (!c || !d_g1 || !d_g2 || !d_out || (n && !d_msg_hashes)) return fail(-EINVAL, "NULL argument");
    if (k && (!d_key_pts || !d_key_scalars)) return fail(-EINVAL, "NULL key buffer");
    if (n > 0x03FFFFF0ull) return fail(-EINVAL, "batch too large");
    HIP_TRY(hipSetDevice(c->device));
    if (n) {
        if (int rc = map_to_g2_impl(c, d_msg_hashes, n, (char*)d_g2 + BLSGPU_G2_BYTES, (hipStream_t)stream, true)) return rc;
        if (k)
            if (int rc = msm_dev<1>(c, d_key_pts, d_key_scalars, k, n, (char*)d_g1 + BLSGPU_G1_BYTES, nullptr, (hipStream_t)stream)) return rc;
    }
    return blsgpu_pairing_multi_dev(c, d_g1, d_g2, nullptr, n + 1, d_out, stream);
}

// Host buffers: ONE upload (points, hashes, keys), the three stages on the device, 576 bytes back.
BLSGPU_EXPORT int blsgpu_verify_pipeline(blsgpu_ctx* c, const uint8_t neg_g1[96], const uint8_t sig[192], const uint8_t* msg_hashes, size_t n,
                                         const uint8_t* keys_affine, const uint8_t* key_pts, const uint8_t* key_scalars, size_t k,
                                         uint8_t out[576]) {
    if (!c || !neg_g1 || !sig || !out || (n && !msg_hashes)) return fail(-EINVAL, "NULL argument");
    if (n && !keys_affine && !(k && key_pts && key_scalars)) return fail(-EINVAL, "neither keys nor key sums given");
    if (n > 0x03FFFFF0ull) return fail(-EINVAL, "batch too large");
    HIP_TRY(hipSetDevice(c->device));
    const bool sums = n && !keys_affine;
    // the two point arrays: slot 0 comes from the host; the rest is keys_affine, or written on the device
    Staging s(c);
    const int d1 = s.scratch((n + 1) * BLSGPU_G1_BYTES), d2 = s.scratch((n + 1) * BLSGPU_G2_BYTES), dh = s.in(msg_hashes, n * 32),
              dkp = s.in(sums ? key_pts : nullptr, n * k * BLSGPU_G1_BYTES), dks = s.in(sums ? key_scalars : nullptr, n * k * 32), dout = s.out(out, 576);
    if (int rc = s.alloc()) return rc;
    // the VM kernels round their team counts up: reserve as a call of n + 1 pairs does
    if (int rc = ensure_partials(c, pairing::batch_partials(n + 3))) return rc;
    {
        StreamGuard sg(c, nullptr);
        HIP_TRY(hipMemcpyAsync(s.at(d1), neg_g1, BLSGPU_G1_BYTES, hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemcpyAsync(s.at(d2), sig, BLSGPU_G2_BYTES, hipMemcpyHostToDevice, nullptr));
        if (int rc = s.up()) return rc;
        if (n && !sums) HIP_TRY(hipMemcpyAsync(s.at(d1) + BLSGPU_G1_BYTES, keys_affine, n * BLSGPU_G1_BYTES, hipMemcpyHostToDevice, nullptr));
    }
    if (int rc = blsgpu_verify_pipeline_dev(c, s.at(d1), s.at(d2), s.at(dh), n, s.opt(dkp), s.opt(dks), sums ? k : 0, s.at(dout), nullptr)) return rc;
    return s.down();
}

// ---- m aggregates of any shapes in one call (blsgpu_veragg.hip; verify_agg_plan.h is the whole schedule) -----------------
// Once per call: the tables (one upload), the key sums of ALL groups -- msm_ranges_dev with exponents, which synchronises the
// stream once to read its chunk count, range_sums_dev (no scan: the plan checked the ranges) without --, and the hash of all
// n_msgs message hashes.  Then per slice of whole aggregates: k_va_pairs, the ragged multi-pairing with a range per aggregate,
// k_va_status.  Nothing of the caller's is written before the first slice's k_va_status, and every buffer the slices take is
// sized before the first launch.
namespace {
// the argument checks, before anything is written; 1: nothing to do
int veragg_args(const blsgpu_ctx* c, const void* sigs, const void* msg_hashes, size_t n_msgs, const void* keys, size_t n_keys,
                const uint32_t* grp_off, const uint32_t* grp_msg, size_t n_grp, const uint32_t* agg_off, size_t m, const void* status) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (m == 0) return 1;
    if (!sigs || !status || !agg_off || !grp_off || (n_grp && !grp_msg) || (n_keys && !keys) || (n_msgs && !msg_hashes))
        return fail(-EINVAL, "NULL argument");
    return 0;
}
verify_agg::Plan veragg_plan(const blsgpu_ctx* c, const uint32_t* grp_off, const uint32_t* grp_msg, size_t n_grp, const uint32_t* agg_off,
                             size_t m, size_t n_keys, size_t n_msgs) {
    return verify_agg::plan(grp_off, grp_msg, n_grp, agg_off, m, n_keys, n_msgs, *c, *c, PAIRING_CONSTS, pairing_limits(c), MSM_CONSTS);
}
int veragg_refuse(const verify_agg::Plan& p) {
    return fail(verify_agg::refusal_code(p.refusal), std::string(verify_agg::refusal_text(p.refusal)) + " (entry " + std::to_string(p.bad) + ")");
}

int veragg_launch(blsgpu_ctx* c, const verify_agg::Plan& p, const void* d_sigs, const void* d_hashes, const void* d_keys, const void* d_exps,
                  void* d_status, void* d_out_gt, hipStream_t st) {
    namespace va = blsgpu::veragg;
    static_assert(va::PER == verify_agg::PIECES && va::THREADS == verify_agg::THREADS && va::SRC_SIG == verify_agg::SIG &&
                      verify_agg::GT_BYTES == BLSGPU_FQ12_BYTES,
                  "verify_agg_plan.h differs from blsgpu_veragg.hip");
    static const uint32_t neg_g1[24] = SIGSH_NEG_G1_WORDS;
    for (const verify_agg::Slice& s : p.slices)
        if (int rc = pairing_ranges_reserve(c, s.pr)) return rc;
    if (int rc = c->grow(B_VERAGG_WS, p.ws_bytes)) return rc;
    char* const W = c->at<char>(B_VERAGG_WS);
    {
        PinnedTables pin(c);
        void* image = nullptr;
        if (int rc = pin.take(p.ws_bytes - p.o_tables, &image)) return rc;
        p.fill_tables(image, neg_g1);
        if (int rc = pin.upload(W + p.o_tables, p.ws_bytes - p.o_tables, st)) return rc;
    }
    HIP_TRY(hipMemsetAsync(W + p.o_und, 0, (p.m + 3) & ~(size_t)3, st));
    if (p.n_grp) {
        if (d_exps) {
            if (int rc = msm_ranges_dev<1>(c, d_keys, d_exps, p.n_keys, W + p.o_kr, p.n_grp, W + p.o_sum, W + p.o_flag, st)) return rc;
        } else if (int rc = range_sums_dev<1>(c, d_keys, p.n_keys, W + p.o_kr, p.n_grp, W + p.o_sum, W + p.o_flag, false, st)) {
            return rc;
        }
    }
    if (int rc = map_to_g2_impl(c, d_hashes, p.n_msgs, W + p.o_h, st, true)) return rc;
    for (const verify_agg::Slice& s : p.slices) {
        char* const gt = d_out_gt ? (char*)d_out_gt + s.agg0 * BLSGPU_FQ12_BYTES : W + p.o_gt;
        hipLaunchKernelGGL(va::k_va_pairs, dim3(s.g_pairs), dim3(va::THREADS), 0, st, (const uint32_t*)(W + s.src_off), s.pairs * va::PER,
                           (const uint4*)d_sigs, (const uint4*)(W + p.o_neg), (const uint4*)(W + p.o_sum), (const uint8_t*)(W + p.o_flag),
                           (const uint4*)(W + p.o_h), (uint4*)(W + p.o_g1), (uint4*)(W + p.o_g2), (uint32_t*)(W + p.o_und));
        HIP_TRY(hipGetLastError());
        if (int rc = pairing_ranges_launch(c, s.pr, W + p.o_g1, W + p.o_g2, nullptr, gt, st, W + s.prtab_off)) return rc;
        hipLaunchKernelGGL(va::k_va_status, dim3(s.g_status), dim3(va::THREADS), 0, st, (const uint4*)gt, (const uint8_t*)(W + p.o_und + s.agg0),
                           (uint32_t)s.aggs, (uint8_t*)d_status + s.agg0);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
}  // namespace

BLSGPU_EXPORT int blsgpu_verify_aggregates_dev(blsgpu_ctx* c, const void* d_sigs, const void* d_msg_hashes, size_t n_msgs, const void* d_keys,
                                               const void* d_exps, size_t n_keys, const uint32_t* grp_off, const uint32_t* grp_msg, size_t n_grp,
                                               const uint32_t* agg_off, size_t m, void* d_status, void* d_out_gt, void* stream) {
    if (int rc = veragg_args(c, d_sigs, d_msg_hashes, n_msgs, d_keys, n_keys, grp_off, grp_msg, n_grp, agg_off, m, d_status)) return rc < 0 ? rc : 0;
    const verify_agg::Plan p = veragg_plan(c, grp_off, grp_msg, n_grp, agg_off, m, n_keys, n_msgs);
    if (p.refusal) return veragg_refuse(p);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    StreamGuard sg(c, st);
    return veragg_launch(c, p, d_sigs, d_msg_hashes, d_keys, d_exps, d_status, d_out_gt, st);
}

BLSGPU_EXPORT int blsgpu_verify_aggregates(blsgpu_ctx* c, const uint8_t* sigs, const uint8_t* msg_hashes, size_t n_msgs, const uint8_t* keys,
                                           const uint8_t* exps, size_t n_keys, const uint32_t* grp_off, const uint32_t* grp_msg, size_t n_grp,
                                           const uint32_t* agg_off, size_t m, uint8_t* status, uint8_t* out_gt) {
    if (int rc = veragg_args(c, sigs, msg_hashes, n_msgs, keys, n_keys, grp_off, grp_msg, n_grp, agg_off, m, status)) return rc < 0 ? rc : 0;
    const verify_agg::Plan p = veragg_plan(c, grp_off, grp_msg, n_grp, agg_off, m, n_keys, n_msgs);
    if (p.refusal) return veragg_refuse(p);
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int ds = s.in(sigs, m * BLSGPU_G2_BYTES), dh = s.in(n_msgs ? msg_hashes : nullptr, n_msgs * 32),
              dk = s.in(n_keys ? keys : nullptr, n_keys * BLSGPU_G1_BYTES), de = s.in(n_keys ? exps : nullptr, n_keys * 32),
              dst = s.out(status, m), dgt = s.out(out_gt, m * BLSGPU_FQ12_BYTES);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    {
        StreamGuard sg(c, nullptr);
        if (int rc = veragg_launch(c, p, s.at(ds), s.opt(dh), s.opt(dk), s.opt(de), s.at(dst), s.opt(dgt), nullptr)) return rc;
    }
    return s.down();
}

BLSGPU_EXPORT int blsgpu_hash_to_g2(blsgpu_ctx* c, const uint8_t* msg_hashes, size_t n, uint8_t* out) {
    if (!c || (n && (!msg_hashes || !out))) return fail(-EINVAL, "NULL argument");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int din = s.in(msg_hashes, n * 32), dout = s.out(out, n * 192);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = map_to_g2_impl(c, s.at(din), n, s.at(dout), nullptr, true)) return rc;
    return s.down();
}

BLSGPU_EXPORT int blsgpu_map_to_g2(blsgpu_ctx* c, const uint8_t* t, size_t n, uint8_t* out) {
    if (!c || (n && (!t || !out))) return fail(-EINVAL, "NULL argument");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int din = s.in(t, n * 192), dout = s.out(out, n * 192);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = blsgpu_map_to_g2_dev(c, s.at(din), n, s.at(dout), nullptr)) return rc;
    return s.down();
}

// ------------------------------------------------------------ hash to G1 (blsgpu_h2g1.hip) --
// One kernel per slice and nothing between the slices: a message lives in one lane's registers from its bytes to its point, so
// these calls take no workspace.  `hash`: n x 32-byte message hashes (the SHA-256 chain on the device), otherwise n x 96 bytes
// t0 || t1.  The argument checks come before anything is written.
static int h2g1_dev(blsgpu_ctx* c, bool hash, const void* d_in, size_t n, void* d_out_aff, void* d_out_ser, void* d_out_inf, hipStream_t st) {
    if (n == 0) return 0;
    if (!d_in || (!d_out_aff && !d_out_ser)) return fail(-EINVAL, "NULL argument");
    StreamGuard sg(c, st);
    const size_t in_dw = hash ? 8 : 24;
    return for_slices(n, slice_len(c, FIX_SLICE), [&](size_t lo, size_t m) {
        const dim3 grid((unsigned)((m + 255) / 256));
        const uint32_t* in = (const uint32_t*)d_in + lo * in_dw;
        uint32_t* aff = d_out_aff ? (uint32_t*)d_out_aff + lo * 24 : nullptr;
        uint32_t* ser = d_out_ser ? (uint32_t*)d_out_ser + lo * 12 : nullptr;
        uint8_t* inf = d_out_inf ? (uint8_t*)d_out_inf + lo : nullptr;
        if (hash)
            hipLaunchKernelGGL(blsgpu::h2g1::k_h2g1<1>, grid, dim3(256), 0, st, g1_generator(), in, (uint32_t)m, aff, ser, inf);
        else
            hipLaunchKernelGGL(blsgpu::h2g1::k_h2g1<0>, grid, dim3(256), 0, st, g1_generator(), in, (uint32_t)m, aff, ser, inf);
        HIP_TRY(hipGetLastError());
        return 0;
    });
}
// the host-buffer forms: FIX_HOST_SLICE messages per staged slice
static int h2g1_host(blsgpu_ctx* c, bool hash, const uint8_t* in, size_t n, uint8_t* out_aff, uint8_t* out_ser, uint8_t* out_inf) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    if (!in || (!out_aff && !out_ser)) return fail(-EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t HS = slice_len(c, FIX_HOST_SLICE), S = n < HS ? n : HS;
    Staging s(c);
    const int din = s.in(in, S, hash ? 32 : 96), daff = s.out(out_aff, S, 96), dser = s.out(out_ser, S, 48), dinf = s.out(out_inf, S, 1);
    if (int rc = s.alloc()) return rc;
    return for_slices(n, S, [&](size_t lo, size_t m) {
        if (int rc = s.up(lo, m)) return rc;
        if (int rc = h2g1_dev(c, hash, s.at(din), m, s.opt(daff), s.opt(dser), s.opt(dinf), nullptr)) return rc;
        return s.down(lo, m);
    });
}
BLSGPU_EXPORT int blsgpu_map_to_g1(blsgpu_ctx* c, const uint8_t* t, size_t n, uint8_t* out_aff, uint8_t* out_ser, uint8_t* out_inf) {
    return h2g1_host(c, false, t, n, out_aff, out_ser, out_inf);
}
BLSGPU_EXPORT int blsgpu_map_to_g1_dev(blsgpu_ctx* c, const void* d_t, size_t n, void* d_out_aff, void* d_out_ser, void* d_out_inf,
                                       void* stream) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return h2g1_dev(c, false, d_t, n, d_out_aff, d_out_ser, d_out_inf, (hipStream_t)stream);
}
// The whole hash_to_point_prehashed_Fq (ec.py:511-520) for 32-byte message hashes.
BLSGPU_EXPORT int blsgpu_hash_to_g1(blsgpu_ctx* c, const uint8_t* msg_hashes, size_t n, uint8_t* out_aff, uint8_t* out_ser,
                                    uint8_t* out_inf) {
    return h2g1_host(c, true, msg_hashes, n, out_aff, out_ser, out_inf);
}
BLSGPU_EXPORT int blsgpu_hash_to_g1_dev(blsgpu_ctx* c, const void* d_msg_hashes, size_t n, void* d_out_aff, void* d_out_ser,
                                        void* d_out_inf, void* stream) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return h2g1_dev(c, true, d_msg_hashes, n, d_out_aff, d_out_ser, d_out_inf, (hipStream_t)stream);
}

// ------------------------------------------------------------ G2 multiplication by secret scalars, signing (blsgpu_g2smul.hip) --
// enqueues out_i = s_i P_(n_pts == 1 ? 0 : i) on `st` in slices of g2smul::SLICE scalars (caller: StreamGuard); table: room for
// the tables of one slice (of one point when n_pts == 1: built once, read by every slice)
static int g2_smul_launch(blsgpu_ctx* c, const void* d_pts, size_t n_pts, const void* d_scalars, size_t n, void* d_out_aff, void* d_out_ser,
                          void* d_out_inf, uint32_t* table, hipStream_t st) {
    using namespace blsgpu::g2smul;
    const bool shared = n_pts == 1;
    KernelTimer kt(c, st, 8);
    if (shared) {
        hipLaunchKernelGGL(k_g2_smul_table, dim3(1), dim3(256), 0, st, (const uint32_t*)d_pts, 1u, table);
        HIP_TRY(hipGetLastError());
    }
    const size_t step = keys::smul_step(*c, KEYS_CONSTS);
    return for_slices(n, step, [&](size_t lo, size_t) {
        const keys::SmulAt a = keys::smul_at(KEYS_CONSTS, n, step, lo);
        const uint32_t m = (uint32_t)a.m;
        if (!shared) hipLaunchKernelGGL(k_g2_smul_table, dim3(a.grid), dim3(256), 0, st, (const uint32_t*)d_pts + a.pts, m, table);
        hipLaunchKernelGGL(k_g2_smul, dim3(a.grid), dim3(256), 0, st, (const uint32_t*)table, shared ? 2u : 2 * m, shared ? 1u : 0u,
                           (const uint32_t*)d_scalars + a.scalars, m, at_words(d_out_aff, a.aff), at_words(d_out_ser, a.ser),
                           (uint8_t*)at_bytes(d_out_inf, a.inf));
        HIP_TRY(hipGetLastError());
        return 0;
    });
}
static int g2_smul_args(size_t n_sel, size_t n, const void* a, const void* b, const void* out_aff, const void* out_ser, const char* what) {
    if (n_sel != 1 && n_sel != n) return fail(-EINVAL, std::string(what) + " must be 1 or n");
    if (!a || !b) return fail(-EINVAL, "NULL argument");
    if (!out_aff && !out_ser) return fail(-EINVAL, "out_aff and out_ser are both NULL");
    if (keys::g2_smul_too_large(n)) return fail(-EINVAL, "batch too large");
    return 0;
}

BLSGPU_EXPORT int blsgpu_g2_mul_secret_dev(blsgpu_ctx* c, const void* d_pts, size_t n_pts, const void* d_scalars, size_t n, void* d_out_aff,
                                           void* d_out_ser, void* d_out_inf, void* stream) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    if (int rc = g2_smul_args(n_pts, n, d_pts, d_scalars, d_out_aff, d_out_ser, "n_pts")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    StreamGuard sg(c, (hipStream_t)stream);
    if (int rc = c->grow(B_SMUL_WS, keys::smul_table_bytes(KEYS_CONSTS, keys::smul_held(*c, KEYS_CONSTS, n_pts == 1, n)))) return rc;
    return g2_smul_launch(c, d_pts, n_pts, d_scalars, n, d_out_aff, d_out_ser, d_out_inf, c->at<uint32_t>(B_SMUL_WS), (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_g2_mul_secret(blsgpu_ctx* c, const uint8_t* pts, size_t n_pts, const uint8_t* scalars, size_t n, uint8_t* out_aff,
                                       uint8_t* out_ser, uint8_t* out_inf) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    if (int rc = g2_smul_args(n_pts, n, pts, scalars, out_aff, out_ser, "n_pts")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t S = keys::staged_slice(*c, n, KEYS_CONSTS.smul_slice);
    const bool per = n_pts != 1;
    Staging s(c);
    const int dp = per ? s.in(pts, S, 192) : s.in(pts, 192), dsc = s.in(scalars, S, 32), daff = s.out(out_aff, S, 192),
              dser = s.out(out_ser, S, 96), dinf = s.out(out_inf, S, 1);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    return for_slices(n, S, [&](size_t lo, size_t m) {
        if (int rc = s.up(lo, m)) return rc;
        if (int rc = blsgpu_g2_mul_secret_dev(c, s.at(dp), per ? m : 1, s.at(dsc), m, s.opt(daff), s.opt(dser), s.opt(dinf), nullptr)) return rc;
        return s.down(lo, m);
    });
}

// PrivateKey.sign_prehashed's device work: the hash to G2 of a slice of messages into the workspace, then k_g2_smul on
// those points; one message (n_msg == 1) is hashed once and its table shared
BLSGPU_EXPORT int blsgpu_sign_dev(blsgpu_ctx* c, const void* d_sks, const void* d_msg_hashes, size_t n_msg, size_t n, void* d_out_aff,
                                  void* d_out_ser, void* stream) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    if (int rc = g2_smul_args(n_msg, n, d_sks, d_msg_hashes, d_out_aff, d_out_ser, "n_msg")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const keys::SignPlan p = keys::plan_sign(*c, KEYS_CONSTS, n_msg, n);
    if (int rc = c->grow(B_SMUL_WS, p.bytes)) return rc;
    char* d_hm = c->at<char>(B_SMUL_WS) + p.o_pts;
    uint32_t* table = (uint32_t*)(c->at<char>(B_SMUL_WS) + p.o_table);
    return for_slices(n, p.step, [&](size_t lo, size_t) {
        const keys::SignAt a = p.at(lo);
        if (int rc = map_to_g2_impl(c, (const char*)d_msg_hashes + a.hashes, a.msgs, d_hm, st, true)) return rc;
        StreamGuard sg(c, st);
        return g2_smul_launch(c, d_hm, a.msgs, (const char*)d_sks + a.sks, a.m, at_bytes(d_out_aff, a.aff), at_bytes(d_out_ser, a.ser), nullptr,
                              table, st);
    });
}
BLSGPU_EXPORT int blsgpu_sign(blsgpu_ctx* c, const uint8_t* sks, const uint8_t* msg_hashes, size_t n_msg, size_t n, uint8_t* out_aff,
                              uint8_t* out_ser) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    if (int rc = g2_smul_args(n_msg, n, sks, msg_hashes, out_aff, out_ser, "n_msg")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t S = keys::staged_slice(*c, n, KEYS_CONSTS.smul_slice);
    const bool per = n_msg != 1;
    Staging s(c);
    const int dsk = s.in(sks, S, 32), dh = per ? s.in(msg_hashes, S, 32) : s.in(msg_hashes, 32), daff = s.out(out_aff, S, 192),
              dser = s.out(out_ser, S, 96);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    return for_slices(n, S, [&](size_t lo, size_t m) {
        if (int rc = s.up(lo, m)) return rc;
        if (int rc = blsgpu_sign_dev(c, s.at(dsk), s.at(dh), per ? m : 1, m, s.opt(daff), s.opt(dser), nullptr)) return rc;
        return s.down(lo, m);
    });
}

// ------------------------------------------------------------ decompression --
BLSGPU_EXPORT int blsgpu_g1_decompress(blsgpu_ctx* c, const uint8_t* in, size_t n, uint8_t* out, uint8_t* ok) {
    return decompress_host<1>(c, in, n, out, ok);
}
BLSGPU_EXPORT int blsgpu_g2_decompress(blsgpu_ctx* c, const uint8_t* in, size_t n, uint8_t* out, uint8_t* ok) {
    return decompress_host<2>(c, in, n, out, ok);
}
BLSGPU_EXPORT int blsgpu_g1_decompress_dev(blsgpu_ctx* c, const void* d_in, size_t n, void* d_out, void* d_ok, void* stream) {
    if (!c || (n && (!d_in || !d_out || !d_ok))) return fail(-EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    return decompress_dev<1>(c, d_in, n, d_out, d_ok, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_g2_decompress_dev(blsgpu_ctx* c, const void* d_in, size_t n, void* d_out, void* d_ok, void* stream) {
    if (!c || (n && (!d_in || !d_out || !d_ok))) return fail(-EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    return decompress_dev<2>(c, d_in, n, d_out, d_ok, (hipStream_t)stream);
}

// ------------------------------------------------------------ fixed-base G1, HD derivation --
// the host-buffer forms of out_i = s_i G1: digit-indexed with the optional addend, or `secret` (no addend)
static int g1_mul_gen_host(blsgpu_ctx* c, const uint8_t* scalars, size_t n, const uint8_t* add, size_t n_add, uint8_t* out_aff,
                           uint8_t* out_ser, bool secret) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    if (!scalars || (!out_aff && !out_ser)) return fail(-EINVAL, "NULL argument");
    if (!secret)
        if (int rc = check_n_add(n, n_add, add)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t S = keys::staged_slice(*c, n, FIX_HOST_SLICE);
    const bool per = n_add == n && n_add > 1;
    Staging s(c);
    const int dsc = s.in(scalars, S, 32), dadd = per ? s.in(add, S, 96) : s.in(n_add ? add : nullptr, 96), daff = s.out(out_aff, S, 96),
              dser = s.out(out_ser, S, 48);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    return for_slices(n, S, [&](size_t lo, size_t m) {
        if (int rc = s.up(lo, m)) return rc;
        if (int rc = secret ? g1_mul_gen_secret_dev(c, s.at(dsc), m, s.opt(daff), s.opt(dser), nullptr)
                            : g1_mul_gen_dev(c, s.at(dsc), m, s.opt(dadd), per ? m : n_add, s.opt(daff), s.opt(dser), nullptr))
            return rc;
        return s.down(lo, m);
    });
}
BLSGPU_EXPORT int blsgpu_g1_mul_gen(blsgpu_ctx* c, const uint8_t* scalars, size_t n, const uint8_t* add, size_t n_add, uint8_t* out_aff,
                                    uint8_t* out_ser) {
    return g1_mul_gen_host(c, scalars, n, add, n_add, out_aff, out_ser, false);
}
BLSGPU_EXPORT int blsgpu_g1_mul_gen_dev(blsgpu_ctx* c, const void* d_scalars, size_t n, const void* d_add, size_t n_add, void* d_out_aff,
                                        void* d_out_ser, void* stream) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return g1_mul_gen_dev(c, d_scalars, n, d_add, n_add, d_out_aff, d_out_ser, (hipStream_t)stream);
}

BLSGPU_EXPORT int blsgpu_g1_mul_gen_secret(blsgpu_ctx* c, const uint8_t* scalars, size_t n, uint8_t* out_aff, uint8_t* out_ser) {
    return g1_mul_gen_host(c, scalars, n, nullptr, 0, out_aff, out_ser, true);
}
BLSGPU_EXPORT int blsgpu_g1_mul_gen_secret_dev(blsgpu_ctx* c, const void* d_scalars, size_t n, void* d_out_aff, void* d_out_ser,
                                               void* stream) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return g1_mul_gen_secret_dev(c, d_scalars, n, d_out_aff, d_out_ser, (hipStream_t)stream);
}

BLSGPU_EXPORT int blsgpu_hd_children(blsgpu_ctx* c, const uint8_t chain_code[32], const uint8_t parent_pk_aff[96], const uint8_t* parent_sk,
                                     const uint32_t* indices, size_t n, uint8_t* out_chain, uint8_t* out_sk, uint8_t* out_pk_aff,
                                     uint8_t* out_pk_ser) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    if (!chain_code || !parent_pk_aff || !indices || !out_chain) return fail(-EINVAL, "NULL argument");
    if (parent_sk && !out_sk) return fail(-EINVAL, "private derivation needs out_sk");
    if (!parent_sk)
        for (size_t i = 0; i < n; i++)
            if (indices[i] >> 31) return fail(-EINVAL, "Cannot derive hardened children from public key");
    HIP_TRY(hipSetDevice(c->device));
    const size_t S = keys::staged_slice(*c, n, FIX_HOST_SLICE);
    Staging s(c);
    const int didx = s.in(indices, S, 4), dchain = s.out(out_chain, S, 32), dsk = s.out(parent_sk ? out_sk : nullptr, S, 32),
              daff = s.out(out_pk_aff, S, 96), dser = s.out(out_pk_ser, S, 48);
    if (int rc = s.alloc()) return rc;
    return for_slices(n, S, [&](size_t lo, size_t m) {
        if (int rc = s.up(lo, m)) return rc;
        if (int rc = hd_children_dev(c, chain_code, parent_pk_aff, parent_sk, s.at(didx), m, s.at(dchain), s.opt(dsk), s.opt(daff), s.opt(dser),
                                     false, nullptr)) return rc;
        return s.down(lo, m);
    });
}
BLSGPU_EXPORT int blsgpu_hd_children_dev(blsgpu_ctx* c, const uint8_t chain_code[32], const uint8_t parent_pk_aff[96], const uint8_t* parent_sk,
                                         const void* d_indices, size_t n, void* d_out_chain, void* d_out_sk, void* d_out_pk_aff,
                                         void* d_out_pk_ser, void* stream) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return hd_children_dev(c, chain_code, parent_pk_aff, parent_sk, d_indices, n, d_out_chain, d_out_sk, d_out_pk_aff, d_out_pk_ser, true,
                           (hipStream_t)stream);
}

static int hd_paths_host(blsgpu_ctx* c, const uint8_t* parents, size_t n_parents, int priv, const uint32_t* parent_of,
                         const uint32_t* indices, size_t depth, size_t n, uint8_t* out_chain, uint8_t* out_sk, uint8_t* out_pk_aff,
                         uint8_t* out_pk_ser, uint8_t* out_parent_fp, bool secret) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (depth == 0 || depth > 255) return fail(-EINVAL, "depth must be 1 .. 255");
    if (n == 0) return 0;
    if (int rc = hd_paths_args(parents, n_parents, priv, indices, depth, n, out_chain, out_sk, out_pk_aff, out_pk_ser)) return rc;
    if (parent_of)
        for (size_t i = 0; i < n; i++)
            if (parent_of[i] >= n_parents) return fail(-EINVAL, "parent index out of range");
    if (!priv)
        for (size_t i = 0; i < n * depth; i++)
            if (indices[i] >> 31) return fail(-EINVAL, "Cannot derive hardened children from public key");
    HIP_TRY(hipSetDevice(c->device));
    const size_t S = keys::staged_slice(*c, n, FIX_HOST_SLICE);
    Staging s(c);
    const int dpar = s.in(parents, n_parents * BLSGPU_HD_PARENT_BYTES), dof = s.in(parent_of, S, 4), didx = s.in(indices, S, depth * 4),
              dchain = s.out(out_chain, S, 32), dsk = s.out(priv ? out_sk : nullptr, S, 32), daff = s.out(out_pk_aff, S, 96),
              dser = s.out(out_pk_ser, S, 48), dfp = s.out(out_parent_fp, S, 4);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    return for_slices(n, S, [&](size_t lo, size_t m) {
        if (int rc = s.up(lo, m)) return rc;
        if (int rc = hd_paths_dev(c, s.at(dpar), n_parents, priv, s.opt(dof), s.at(didx), depth, m, s.at(dchain), s.opt(dsk), s.opt(daff),
                                  s.opt(dser), s.opt(dfp), false, nullptr, secret)) return rc;
        return s.down(lo, m);
    });
}
BLSGPU_EXPORT int blsgpu_hd_paths(blsgpu_ctx* c, const uint8_t* parents, size_t n_parents, int priv, const uint32_t* parent_of,
                                  const uint32_t* indices, size_t depth, size_t n, uint8_t* out_chain, uint8_t* out_sk, uint8_t* out_pk_aff,
                                  uint8_t* out_pk_ser, uint8_t* out_parent_fp) {
    return hd_paths_host(c, parents, n_parents, priv, parent_of, indices, depth, n, out_chain, out_sk, out_pk_aff, out_pk_ser, out_parent_fp,
                         false);
}
BLSGPU_EXPORT int blsgpu_hd_paths_secret(blsgpu_ctx* c, const uint8_t* parents, size_t n_parents, const uint32_t* parent_of,
                                         const uint32_t* indices, size_t depth, size_t n, uint8_t* out_chain, uint8_t* out_sk,
                                         uint8_t* out_pk_aff, uint8_t* out_pk_ser, uint8_t* out_parent_fp) {
    return hd_paths_host(c, parents, n_parents, 1, parent_of, indices, depth, n, out_chain, out_sk, out_pk_aff, out_pk_ser, out_parent_fp,
                         true);
}
BLSGPU_EXPORT int blsgpu_hd_paths_dev(blsgpu_ctx* c, const void* d_parents, size_t n_parents, int priv, const void* d_parent_of,
                                      const void* d_indices, size_t depth, size_t n, void* d_out_chain, void* d_out_sk, void* d_out_pk_aff,
                                      void* d_out_pk_ser, void* d_out_parent_fp, void* stream) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (depth == 0 || depth > 255) return fail(-EINVAL, "depth must be 1 .. 255");
    HIP_TRY(hipSetDevice(c->device));
    return hd_paths_dev(c, d_parents, n_parents, priv, d_parent_of, d_indices, depth, n, d_out_chain, d_out_sk, d_out_pk_aff, d_out_pk_ser,
                        d_out_parent_fp, true, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_hd_paths_secret_dev(blsgpu_ctx* c, const void* d_parents, size_t n_parents, const void* d_parent_of,
                                             const void* d_indices, size_t depth, size_t n, void* d_out_chain, void* d_out_sk,
                                             void* d_out_pk_aff, void* d_out_pk_ser, void* d_out_parent_fp, void* stream) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (depth == 0 || depth > 255) return fail(-EINVAL, "depth must be 1 .. 255");
    HIP_TRY(hipSetDevice(c->device));
    return hd_paths_dev(c, d_parents, n_parents, 1, d_parent_of, d_indices, depth, n, d_out_chain, d_out_sk, d_out_pk_aff, d_out_pk_ser,
                        d_out_parent_fp, true, (hipStream_t)stream, true);
}

// ------------------------------------------------------------ keys from seeds --
BLSGPU_EXPORT int blsgpu_keys_from_seeds_dev(blsgpu_ctx* c, const void* d_seeds, size_t seed_len, size_t n, int hd, void* d_out_sk,
                                             void* d_out_chain, void* d_out_pk_aff, void* d_out_pk_ser, void* d_out_parents, void* stream) {
    if (int rc = seeds_args(c, d_seeds, seed_len, n, hd, d_out_sk, d_out_chain, d_out_pk_aff, d_out_pk_ser, d_out_parents)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return keys_from_seeds_dev(c, d_seeds, seed_len, n, hd, d_out_sk, d_out_chain, d_out_pk_aff, d_out_pk_ser, d_out_parents,
                               (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_keys_from_seeds(blsgpu_ctx* c, const uint8_t* seeds, size_t seed_len, size_t n, int hd, uint8_t* out_sk,
                                         uint8_t* out_chain, uint8_t* out_pk_aff, uint8_t* out_pk_ser, uint8_t* out_parents) {
    if (int rc = seeds_args(c, seeds, seed_len, n, hd, out_sk, out_chain, out_pk_aff, out_pk_ser, out_parents)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    const size_t S = keys::staged_fit(*c, n, keys::seeds_item_bytes(seed_len));
    Staging s(c);
    const int dseed = s.in(seed_len ? seeds : nullptr, S, seed_len), dsk = s.out(out_sk, S, 32), dchain = s.out(out_chain, S, 32),
              daff = s.out(out_pk_aff, S, 96), dser = s.out(out_pk_ser, S, 48), dpar = s.out(out_parents, S, BLSGPU_HD_PARENT_BYTES);
    if (int rc = s.alloc()) return rc;
    return for_slices(n, S, [&](size_t lo, size_t m) {
        if (int rc = s.up(lo, m)) return rc;
        if (int rc = keys_from_seeds_dev(c, s.opt(dseed), seed_len, m, hd, s.opt(dsk), s.opt(dchain), s.opt(daff), s.opt(dser), s.opt(dpar),
                                         nullptr))
            return rc;
        return s.down(lo, m);
    });
}

// ------------------------------------------------------------ Feldman share checks --
static int poly_check_host(blsgpu_ctx* c, const uint8_t* commit, size_t n_polys, size_t t, const uint32_t* poly, const uint8_t* x,
                           const uint8_t* s, size_t n, uint8_t* status, uint8_t* out_aff, bool secret) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (t == 0) return fail(-EINVAL, "t must be at least 1");
    if (n == 0) return 0;
    if (secret && (!s || !status)) return fail(-EINVAL, "s and status are required");
    if (int rc = poly_args(n_polys, t, commit, poly, x, s, status, out_aff)) return rc;
    for (size_t i = 0; i < n; i++)
        if (poly[i] >= n_polys) return fail(-EINVAL, "polynomial index out of range");
    HIP_TRY(hipSetDevice(c->device));
    const size_t S = keys::staged_slice(*c, n, FIX_HOST_SLICE);
    Staging st(c);
    const int dcommit = st.in(commit, n_polys * t * 96), dpoly = st.in(poly, S, 4), dx = st.in(x, S, 32), ds = st.in(s, S, 32),
              dstatus = st.out(status, S, 1), daff = st.out(out_aff, S, 96);
    if (int rc = st.alloc()) return rc;
    if (int rc = st.up()) return rc;
    {
        StreamGuard sg(c, nullptr);
        if (int rc = poly_ws(c, n_polys, t)) return rc;
        if (int rc = poly_prep(c, st.at(dcommit), n_polys, t, status != nullptr, nullptr, secret)) return rc;
    }
    return for_slices(n, S, [&](size_t lo, size_t m) {
        if (int rc = st.up(lo, m)) return rc;
        {
            StreamGuard sg(c, nullptr);
            if (int rc = poly_eval_launch(c, n_polys, t, st.at(dpoly), st.at(dx), st.opt(ds), m, st.opt(dstatus), st.opt(daff), nullptr, secret))
                return rc;
        }
        return st.down(lo, m);
    });
}
BLSGPU_EXPORT int blsgpu_g1_poly_check(blsgpu_ctx* c, const uint8_t* commit, size_t n_polys, size_t t, const uint32_t* poly, const uint8_t* x,
                                       const uint8_t* s, size_t n, uint8_t* status, uint8_t* out_aff) {
    return poly_check_host(c, commit, n_polys, t, poly, x, s, n, status, out_aff, false);
}
BLSGPU_EXPORT int blsgpu_g1_poly_check_secret(blsgpu_ctx* c, const uint8_t* commit, size_t n_polys, size_t t, const uint32_t* poly,
                                              const uint8_t* x, const uint8_t* s, size_t n, uint8_t* status, uint8_t* out_aff) {
    return poly_check_host(c, commit, n_polys, t, poly, x, s, n, status, out_aff, true);
}
BLSGPU_EXPORT int blsgpu_g1_poly_check_dev(blsgpu_ctx* c, const void* d_commit, size_t n_polys, size_t t, const void* d_poly, const void* d_x,
                                           const void* d_s, size_t n, void* d_status, void* d_out_aff, void* stream) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return poly_check_dev(c, d_commit, n_polys, t, d_poly, d_x, d_s, n, d_status, d_out_aff, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_g1_poly_check_secret_dev(blsgpu_ctx* c, const void* d_commit, size_t n_polys, size_t t, const void* d_poly,
                                                  const void* d_x, const void* d_s, size_t n, void* d_status, void* d_out_aff, void* stream) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    return poly_check_dev(c, d_commit, n_polys, t, d_poly, d_x, d_s, n, d_status, d_out_aff, (hipStream_t)stream, true);
}

// ------------------------------------------------------------ subgroup membership --
BLSGPU_EXPORT int blsgpu_g1_subgroup_check(blsgpu_ctx* c, const uint8_t* pts, size_t n, uint8_t* status) {
    return subgroup_host(c, 1, pts, n, status);
}
BLSGPU_EXPORT int blsgpu_g2_subgroup_check(blsgpu_ctx* c, const uint8_t* pts, size_t n, uint8_t* status) {
    return subgroup_host(c, 2, pts, n, status);
}
BLSGPU_EXPORT int blsgpu_g1_subgroup_check_dev(blsgpu_ctx* c, const void* d_pts, size_t n, void* d_status, void* stream) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    return subgroup_dev(c, 1, d_pts, n, d_status, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_g2_subgroup_check_dev(blsgpu_ctx* c, const void* d_pts, size_t n, void* d_status, void* stream) {
    if (!c) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    return subgroup_dev(c, 2, d_pts, n, d_status, (hipStream_t)stream);
}

// ------------------------------------------------------------ threshold recovery --
BLSGPU_EXPORT int blsgpu_lagrange_at_zero_dev(blsgpu_ctx* c, const void* d_x, size_t k, size_t groups, void* d_out_coeffs, void* d_status,
                                              void* stream) {
    if (int rc = lagrange_args(c, k, groups, !d_x || !d_out_coeffs || !d_status)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    StreamGuard sg(c, (hipStream_t)stream);
    return lagrange_launch(c, d_x, k, groups, d_out_coeffs, d_status, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_lagrange_at_zero(blsgpu_ctx* c, const uint8_t* x, size_t k, size_t groups, uint8_t* out_coeffs, uint8_t* status) {
    if (int rc = lagrange_args(c, k, groups, !x || !out_coeffs || !status)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int dx = s.in(x, groups * k * 32), dco = s.out(out_coeffs, groups * k * 32), dst = s.out(status, groups);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = blsgpu_lagrange_at_zero_dev(c, s.at(dx), k, groups, s.at(dco), s.at(dst), nullptr)) return rc;
    return s.down();
}
BLSGPU_EXPORT int blsgpu_fr_interpolate_at_zero_dev(blsgpu_ctx* c, const void* d_x, const void* d_y, size_t k, size_t groups, void* d_out,
                                                    void* d_status, void* stream) {
    if (int rc = lagrange_args(c, k, groups, !d_x || !d_y || !d_out || !d_status)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return fr_interpolate_dev(c, d_x, d_y, k, groups, d_out, d_status, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_fr_interpolate_at_zero(blsgpu_ctx* c, const uint8_t* x, const uint8_t* y, size_t k, size_t groups, uint8_t* out,
                                                uint8_t* status) {
    if (int rc = lagrange_args(c, k, groups, !x || !y || !out || !status)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int dx = s.in(x, groups * k * 32), dy = s.in(y, groups * k * 32), dout = s.out(out, groups * 32), dst = s.out(status, groups);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = fr_interpolate_dev(c, s.at(dx), s.at(dy), k, groups, s.at(dout), s.at(dst), nullptr)) return rc;
    return s.down();
}
BLSGPU_EXPORT int blsgpu_threshold_combine_dev(blsgpu_ctx* c, const void* d_sigs_affine, const void* d_x, size_t k, size_t groups, void* d_out,
                                               void* d_out_inf, void* d_status, void* stream) {
    if (int rc = lagrange_args(c, k, groups, !d_sigs_affine || !d_x || !d_out || !d_status)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return threshold_combine_dev(c, d_sigs_affine, d_x, k, groups, d_out, d_out_inf, d_status, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_threshold_combine(blsgpu_ctx* c, const uint8_t* sigs_affine, const uint8_t* x, size_t k, size_t groups, uint8_t* out,
                                           uint8_t* out_inf, uint8_t* status) {
    if (int rc = lagrange_args(c, k, groups, !sigs_affine || !x || !out || !status)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int dsig = s.in(sigs_affine, groups * k * BLSGPU_G2_BYTES), dx = s.in(x, groups * k * 32), dout = s.out(out, groups * BLSGPU_G2_BYTES),
              dinf = s.out(out_inf, groups), dst = s.out(status, groups);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = threshold_combine_dev(c, s.at(dsig), s.at(dx), k, groups, s.at(dout), s.opt(dinf), s.at(dst), nullptr)) return rc;
    return s.down();
}

// ------------------------------------------------------------ signature shares --
BLSGPU_EXPORT int blsgpu_sig_shares_check_dev(blsgpu_ctx* c, const void* d_sigs, const void* d_keys, size_t n_keys, const void* d_key_idx,
                                              const void* d_x, const void* d_msg_hashes, const void* d_weights, int scaled, size_t k,
                                              size_t groups, void* d_status, void* d_session_status, uint64_t* stats, void* stream) {
    if (int rc = sig_shares_args(c, k, groups, n_keys, !d_sigs || !d_keys || !d_key_idx || (scaled && !d_x) || !d_msg_hashes || !d_weights ||
                                                           !d_status || !d_session_status))
        return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return sig_shares_dev(c, d_sigs, d_keys, n_keys, d_key_idx, d_x, d_msg_hashes, d_weights, scaled, k, groups, d_status, d_session_status,
                          stats, true, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_sig_shares_check(blsgpu_ctx* c, const uint8_t* sigs, const uint8_t* keys, size_t n_keys, const uint32_t* key_idx,
                                          const uint8_t* x, const uint8_t* msg_hashes, const uint8_t* weights, int scaled, size_t k,
                                          size_t groups, uint8_t* status, uint8_t* session_status, uint64_t* stats) {
    if (int rc = sig_shares_args(c, k, groups, n_keys, !sigs || !keys || !key_idx || (scaled && !x) || !msg_hashes || !weights || !status ||
                                                           !session_status))
        return rc < 0 ? rc : 0;
    const size_t n = groups * k;
    for (size_t i = 0; i < n; i++)
        if (key_idx[i] >= n_keys) return fail(-EINVAL, "key index out of range");
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int dsig = s.in(sigs, n * BLSGPU_G2_BYTES), dkey = s.in(keys, n_keys * BLSGPU_G1_BYTES), didx = s.in(key_idx, n * 4),
              dx = s.in(scaled ? x : nullptr, n * 32), dh = s.in(msg_hashes, groups * 32), dw = s.in(weights, n * 8),
              dst = s.out(status, n), dss = s.out(session_status, groups);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = sig_shares_dev(c, s.at(dsig), s.at(dkey), n_keys, s.at(didx), s.opt(dx), s.at(dh), s.at(dw), scaled, k, groups, s.at(dst),
                                s.at(dss), stats, false, nullptr))
        return rc;
    return s.down();
}

// ------------------------------------------------------------ short public scalars, batch verification that names the forgeries --
BLSGPU_EXPORT int blsgpu_g1_mul_short(blsgpu_ctx* c, const uint8_t* pts, const uint8_t* w, size_t n, uint8_t* out_aff, uint8_t* out_inf) {
    return mul_short_host<1>(c, pts, w, n, out_aff, out_inf);
}
BLSGPU_EXPORT int blsgpu_g2_mul_short(blsgpu_ctx* c, const uint8_t* pts, const uint8_t* w, size_t n, uint8_t* out_aff, uint8_t* out_inf) {
    return mul_short_host<2>(c, pts, w, n, out_aff, out_inf);
}
BLSGPU_EXPORT int blsgpu_g1_mul_short_dev(blsgpu_ctx* c, const void* d_pts, const void* d_w, size_t n, void* d_out_aff, void* d_out_inf,
                                          void* stream) {
    return mul_short_dev<1>(c, d_pts, d_w, n, d_out_aff, d_out_inf, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_g2_mul_short_dev(blsgpu_ctx* c, const void* d_pts, const void* d_w, size_t n, void* d_out_aff, void* d_out_inf,
                                          void* stream) {
    return mul_short_dev<2>(c, d_pts, d_w, n, d_out_aff, d_out_inf, (hipStream_t)stream);
}
// blsgpu_verify_find* and blsgpu_verify_find_folded*: `find` is verify_find_dev or verify_find_folded_dev; the host form checks
// the indices itself and, with `mono` (the folded form), refuses message indices that decrease
typedef int FindDev(blsgpu_ctx*, const void*, const void*, size_t, const void*, const void*, size_t, const void*, const void*, size_t, void*,
                    uint64_t*, bool, hipStream_t);
int verify_find_abi_dev(FindDev* find, blsgpu_ctx* c, const void* d_sigs, const void* d_keys, size_t n_keys, const void* d_key_idx,
                        const void* d_msg_hashes, size_t n_msgs, const void* d_msg_idx, const void* d_weights, size_t n, void* d_status,
                        uint64_t* stats, void* stream) {
    if (int rc = verify_find_args(c, n, n_keys, n_msgs, !d_sigs || !d_keys || !d_key_idx || !d_msg_hashes || !d_msg_idx || !d_weights || !d_status))
        return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return find(c, d_sigs, d_keys, n_keys, d_key_idx, d_msg_hashes, n_msgs, d_msg_idx, d_weights, n, d_status, stats, true, (hipStream_t)stream);
}
int verify_find_abi_host(FindDev* find, bool mono, blsgpu_ctx* c, const uint8_t* sigs, const uint8_t* keys, size_t n_keys, const uint32_t* key_idx,
                         const uint8_t* msg_hashes, size_t n_msgs, const uint32_t* msg_idx, const uint8_t* weights, size_t n, uint8_t* status,
                         uint64_t* stats) {
    if (int rc = verify_find_args(c, n, n_keys, n_msgs, !sigs || !keys || !key_idx || !msg_hashes || !msg_idx || !weights || !status))
        return rc < 0 ? rc : 0;
    for (size_t i = 0; i < n; i++) {
        if (key_idx[i] >= n_keys) return fail(-EINVAL, "key index out of range");
        if (msg_idx[i] >= n_msgs) return fail(-EINVAL, "message index out of range");
        if (mono && i && msg_idx[i] < msg_idx[i - 1]) return fail(-EINVAL, "message indices decrease");
    }
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int dsig = s.in(sigs, n * BLSGPU_G2_BYTES), dkey = s.in(keys, n_keys * BLSGPU_G1_BYTES), dki = s.in(key_idx, n * 4),
              dh = s.in(msg_hashes, n_msgs * 32), dmi = s.in(msg_idx, n * 4), dw = s.in(weights, n * 8), dst = s.out(status, n);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = find(c, s.at(dsig), s.at(dkey), n_keys, s.at(dki), s.at(dh), n_msgs, s.at(dmi), s.at(dw), n, s.at(dst), stats, false, nullptr))
        return rc;
    return s.down();
}
BLSGPU_EXPORT int blsgpu_verify_find_dev(blsgpu_ctx* c, const void* d_sigs, const void* d_keys, size_t n_keys, const void* d_key_idx,
                                         const void* d_msg_hashes, size_t n_msgs, const void* d_msg_idx, const void* d_weights, size_t n,
                                         void* d_status, uint64_t* stats, void* stream) {
    return verify_find_abi_dev(verify_find_dev, c, d_sigs, d_keys, n_keys, d_key_idx, d_msg_hashes, n_msgs, d_msg_idx, d_weights, n, d_status,
                               stats, stream);
}
BLSGPU_EXPORT int blsgpu_verify_find(blsgpu_ctx* c, const uint8_t* sigs, const uint8_t* keys, size_t n_keys, const uint32_t* key_idx,
                                     const uint8_t* msg_hashes, size_t n_msgs, const uint32_t* msg_idx, const uint8_t* weights, size_t n,
                                     uint8_t* status, uint64_t* stats) {
    return verify_find_abi_host(verify_find_dev, false, c, sigs, keys, n_keys, key_idx, msg_hashes, n_msgs, msg_idx, weights, n, status, stats);
}

// ------------------------------------------------------------ point range sums, batch verification that folds shared messages --
BLSGPU_EXPORT int blsgpu_g1_range_sums(blsgpu_ctx* c, const uint8_t* pts, size_t n, const uint32_t* ranges, size_t m, uint8_t* out_aff,
                                       uint8_t* out_flag) {
    return range_sums_host<1>(c, pts, n, ranges, m, out_aff, out_flag);
}
BLSGPU_EXPORT int blsgpu_g2_range_sums(blsgpu_ctx* c, const uint8_t* pts, size_t n, const uint32_t* ranges, size_t m, uint8_t* out_aff,
                                       uint8_t* out_flag) {
    return range_sums_host<2>(c, pts, n, ranges, m, out_aff, out_flag);
}
BLSGPU_EXPORT int blsgpu_g1_range_sums_dev(blsgpu_ctx* c, const void* d_pts, size_t n, const void* d_ranges, size_t m, void* d_out_aff,
                                           void* d_out_flag, void* stream) {
    if (int rc = range_sums_args(c, d_pts, n, d_ranges, m, d_out_aff, d_out_flag)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return range_sums_dev<1>(c, d_pts, n, d_ranges, m, d_out_aff, d_out_flag, true, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_g2_range_sums_dev(blsgpu_ctx* c, const void* d_pts, size_t n, const void* d_ranges, size_t m, void* d_out_aff,
                                           void* d_out_flag, void* stream) {
    if (int rc = range_sums_args(c, d_pts, n, d_ranges, m, d_out_aff, d_out_flag)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return range_sums_dev<2>(c, d_pts, n, d_ranges, m, d_out_aff, d_out_flag, true, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_g1_msm_ranges(blsgpu_ctx* c, const uint8_t* pts, const uint8_t* scalars, size_t n, const uint32_t* ranges, size_t m,
                                       uint8_t* out_aff, uint8_t* out_flag) {
    return msm_ranges_host<1>(c, pts, scalars, n, ranges, m, out_aff, out_flag);
}
BLSGPU_EXPORT int blsgpu_g2_msm_ranges(blsgpu_ctx* c, const uint8_t* pts, const uint8_t* scalars, size_t n, const uint32_t* ranges, size_t m,
                                       uint8_t* out_aff, uint8_t* out_flag) {
    return msm_ranges_host<2>(c, pts, scalars, n, ranges, m, out_aff, out_flag);
}
BLSGPU_EXPORT int blsgpu_g1_msm_ranges_dev(blsgpu_ctx* c, const void* d_pts, const void* d_scalars, size_t n, const void* d_ranges, size_t m,
                                           void* d_out_aff, void* d_out_flag, void* stream) {
    if (int rc = msm_ranges_args(c, d_pts, d_scalars, n, d_ranges, m, d_out_aff, d_out_flag)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return msm_ranges_dev<1>(c, d_pts, d_scalars, n, d_ranges, m, d_out_aff, d_out_flag, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_g2_msm_ranges_dev(blsgpu_ctx* c, const void* d_pts, const void* d_scalars, size_t n, const void* d_ranges, size_t m,
                                           void* d_out_aff, void* d_out_flag, void* stream) {
    if (int rc = msm_ranges_args(c, d_pts, d_scalars, n, d_ranges, m, d_out_aff, d_out_flag)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return msm_ranges_dev<2>(c, d_pts, d_scalars, n, d_ranges, m, d_out_aff, d_out_flag, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_sig_divide(blsgpu_ctx* c, const uint8_t* pts, size_t n_pts, const uint32_t* pt_off, size_t m, const uint32_t* ent_off,
                                    const uint8_t* ent_dividend, const uint8_t* ent_divisor, size_t n_ent, uint8_t* out_aff, uint8_t* out_flag,
                                    uint8_t* out_status, uint8_t* out_scalars, uint32_t stats[2]) {
    return sig_divide_host(c, pts, n_pts, pt_off, m, ent_off, ent_dividend, ent_divisor, n_ent, out_aff, out_flag, out_status, out_scalars, stats);
}
BLSGPU_EXPORT int blsgpu_sig_divide_dev(blsgpu_ctx* c, const void* d_pts, size_t n_pts, const void* d_pt_off, size_t m, const void* d_ent_off,
                                        const void* d_ent_dividend, const void* d_ent_divisor, size_t n_ent, void* d_out_aff, void* d_out_flag,
                                        void* d_out_status, void* d_out_scalars, uint32_t stats[2], void* stream) {
    if (int rc = sig_divide_args(c, d_pts, n_pts, d_pt_off, m, d_ent_off, d_ent_dividend, d_ent_divisor, n_ent, d_out_aff, d_out_flag, d_out_status))
        return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return sig_divide_dev(c, d_pts, n_pts, d_pt_off, m, d_ent_off, d_ent_dividend, d_ent_divisor, n_ent, d_out_aff, d_out_flag, d_out_status,
                          d_out_scalars, stats, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_verify_find_folded_dev(blsgpu_ctx* c, const void* d_sigs, const void* d_keys, size_t n_keys, const void* d_key_idx,
                                                const void* d_msg_hashes, size_t n_msgs, const void* d_msg_idx, const void* d_weights, size_t n,
                                                void* d_status, uint64_t* stats, void* stream) {
    return verify_find_abi_dev(verify_find_folded_dev, c, d_sigs, d_keys, n_keys, d_key_idx, d_msg_hashes, n_msgs, d_msg_idx, d_weights, n,
                               d_status, stats, stream);
}
BLSGPU_EXPORT int blsgpu_verify_find_folded(blsgpu_ctx* c, const uint8_t* sigs, const uint8_t* keys, size_t n_keys, const uint32_t* key_idx,
                                            const uint8_t* msg_hashes, size_t n_msgs, const uint32_t* msg_idx, const uint8_t* weights, size_t n,
                                            uint8_t* status, uint64_t* stats) {
    return verify_find_abi_host(verify_find_folded_dev, true, c, sigs, keys, n_keys, key_idx, msg_hashes, n_msgs, msg_idx, weights, n, status,
                                stats);
}

// ------------------------------------------------------------ threshold dealing, recovery and share signing for secrets --
BLSGPU_EXPORT int blsgpu_threshold_deal_secret_dev(blsgpu_ctx* c, const void* d_coeffs, size_t n_polys, size_t t, const void* d_x, size_t n_x,
                                                   void* d_out_commit_aff, void* d_out_frag, void* stream) {
    if (int rc = deal_args(c, d_coeffs, n_polys, t, d_x, n_x, d_out_commit_aff, d_out_frag)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return deal_secret_dev(c, d_coeffs, n_polys, t, d_x, n_x, d_out_commit_aff, d_out_frag, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_threshold_deal_secret(blsgpu_ctx* c, const uint8_t* coeffs, size_t n_polys, size_t t, const uint8_t* x, size_t n_x,
                                               uint8_t* out_commit_aff, uint8_t* out_frag) {
    if (int rc = deal_args(c, coeffs, n_polys, t, x, n_x, out_commit_aff, out_frag)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    const size_t S = keys::staged_fit(*c, n_polys, keys::deal_item_bytes(t, n_x, out_frag != nullptr));   // whole polynomials per staged slice
    Staging s(c);
    const int dco = s.in(coeffs, S, t * 32), dx = s.in(out_frag ? x : nullptr, n_x * 32), dcm = s.out(out_commit_aff, S, t * 96),
              dfr = s.out(out_frag, S, n_x * 32);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    return for_slices(n_polys, S, [&](size_t lo, size_t m) {
        if (int rc = s.up(lo, m)) return rc;
        if (int rc = deal_secret_dev(c, s.at(dco), m, t, s.opt(dx), n_x, s.opt(dcm), s.opt(dfr), nullptr)) return rc;
        return s.down(lo, m);
    });
}

BLSGPU_EXPORT int blsgpu_fr_interpolate_at_zero_secret_dev(blsgpu_ctx* c, const void* d_x, const void* d_y, size_t k, size_t groups, void* d_out,
                                                           void* d_status, void* stream) {
    if (int rc = lagrange_args(c, k, groups, !d_x || !d_y || !d_out || !d_status)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return fr_interpolate_dev(c, d_x, d_y, k, groups, d_out, d_status, (hipStream_t)stream, true);
}
BLSGPU_EXPORT int blsgpu_fr_interpolate_at_zero_secret(blsgpu_ctx* c, const uint8_t* x, const uint8_t* y, size_t k, size_t groups, uint8_t* out,
                                                       uint8_t* status) {
    if (int rc = lagrange_args(c, k, groups, !x || !y || !out || !status)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int dx = s.in(x, groups * k * 32), dy = s.in(y, groups * k * 32), dout = s.out(out, groups * 32), dst = s.out(status, groups);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = fr_interpolate_dev(c, s.at(dx), s.at(dy), k, groups, s.at(dout), s.at(dst), nullptr, true)) return rc;
    return s.down();
}

BLSGPU_EXPORT int blsgpu_fr_sum_secret_dev(blsgpu_ctx* c, const void* d_y, size_t k, size_t groups, void* d_out, void* d_out_pk_aff,
                                           void* d_out_pk_ser, void* stream) {
    if (int rc = fr_sum_args(c, d_y, k, groups, d_out)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return fr_sum_secret_dev(c, d_y, k, groups, d_out, d_out_pk_aff, d_out_pk_ser, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_fr_sum_secret(blsgpu_ctx* c, const uint8_t* y, size_t k, size_t groups, uint8_t* out, uint8_t* out_pk_aff,
                                       uint8_t* out_pk_ser) {
    if (int rc = fr_sum_args(c, y, k, groups, out)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    const size_t S = keys::staged_fit(*c, groups, keys::fr_sum_item_bytes(k));                           // whole groups per staged slice
    Staging s(c);
    const int dy = s.in(y, S, k * 32), dout = s.out(out, S, 32), daff = s.out(out_pk_aff, S, 96), dser = s.out(out_pk_ser, S, 48);
    if (int rc = s.alloc()) return rc;
    return for_slices(groups, S, [&](size_t lo, size_t m) {
        if (int rc = s.up(lo, m)) return rc;
        if (int rc = fr_sum_secret_dev(c, s.at(dy), k, m, s.at(dout), s.opt(daff), s.opt(dser), nullptr)) return rc;
        return s.down(lo, m);
    });
}

// PrivateKey.sign_threshold's device work for `groups` sessions of k signers: the coefficients (k_lagrange) into the
// workspace, lambda_i sk_i mod n (k_fr_scale_secret) beside them, H(m) per message, then k_g2_smul -- with ONE message its
// table is built once and shared; with a message per session, session g's point is copied to its k slots slice by slice
BLSGPU_EXPORT int blsgpu_sign_threshold_dev(blsgpu_ctx* c, const void* d_sks, const void* d_x, size_t k, size_t groups, const void* d_msg_hashes,
                                            size_t n_msg, void* d_out_aff, void* d_out_ser, void* d_out_inf, void* d_status, void* stream) {
    if (int rc = sign_threshold_args(c, k, groups, n_msg, !d_sks || !d_x || !d_msg_hashes || !d_status, d_out_aff, d_out_ser)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const keys::ThresholdPlan p = keys::plan_threshold(*c, KEYS_CONSTS, k, groups, n_msg);
    if (int rc = c->grow(B_LAGR_WS, p.lagr_bytes)) return rc;
    if (int rc = c->grow(B_FRS_WS, p.frs_bytes)) return rc;
    if (int rc = c->grow(B_SMUL_WS, p.smul_bytes)) return rc;
    char* d_sc = c->at<char>(B_FRS_WS) + p.o_sc;
    char* d_rep = c->at<char>(B_FRS_WS) + p.o_rep;
    char* d_hm = c->at<char>(B_SMUL_WS) + p.o_hm;
    uint32_t* table = (uint32_t*)(c->at<char>(B_SMUL_WS) + p.o_table);
    {
        StreamGuard sg(c, st);
        if (int rc = lagrange_launch(c, d_x, k, groups, c->at<void>(B_LAGR_WS), d_status, st)) return rc;
        KernelTimer kt(c, st, 10);
        hipLaunchKernelGGL(blsgpu::frsec::k_fr_scale_secret, dim3(p.g_scale), dim3(256), 0, st, c->at<uint8_t>(B_LAGR_WS), (const uint8_t*)d_sks,
                           (uint32_t)p.n, (uint8_t*)d_sc);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = map_to_g2_impl(c, d_msg_hashes, n_msg, d_hm, st, true)) return rc;
    StreamGuard sg(c, st);
    if (p.shared) return g2_smul_launch(c, d_hm, 1, d_sc, p.n, d_out_aff, d_out_ser, d_out_inf, table, st);
    return for_slices(p.n, p.held, [&](size_t lo, size_t) {
        const keys::ThresholdAt a = p.at(lo);
        hipLaunchKernelGGL(blsgpu::frsec::k_g2_spread, dim3(a.g_spread), dim3(256), 0, st, (const uint32_t*)d_hm, (uint32_t)k, lo, (uint32_t)a.m,
                           (uint32_t*)d_rep);
        HIP_TRY(hipGetLastError());
        return g2_smul_launch(c, d_rep, a.m, d_sc + a.sc, a.m, at_bytes(d_out_aff, a.aff), at_bytes(d_out_ser, a.ser), at_bytes(d_out_inf, a.inf),
                              table, st);
    });
}
BLSGPU_EXPORT int blsgpu_sign_threshold(blsgpu_ctx* c, const uint8_t* sks, const uint8_t* x, size_t k, size_t groups, const uint8_t* msg_hashes,
                                        size_t n_msg, uint8_t* out_aff, uint8_t* out_ser, uint8_t* out_inf, uint8_t* status) {
    if (int rc = sign_threshold_args(c, k, groups, n_msg, !sks || !x || !msg_hashes || !status, out_aff, out_ser)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = k * groups;
    Staging s(c);
    const int dsk = s.in(sks, n * 32), dx = s.in(x, n * 32), dh = s.in(msg_hashes, n_msg * 32), daff = s.out(out_aff, n * BLSGPU_G2_BYTES),
              dser = s.out(out_ser, n * 96), dinf = s.out(out_inf, n), dst = s.out(status, groups);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = blsgpu_sign_threshold_dev(c, s.at(dsk), s.at(dx), k, groups, s.at(dh), n_msg, s.opt(daff), s.opt(dser), s.opt(dinf), s.at(dst),
                                           nullptr)) return rc;
    return s.down();
}

// ------------------------------------------------------------ secure aggregation: hash_pks exponents and the three sums --
BLSGPU_EXPORT int blsgpu_hash_pks_dev(blsgpu_ctx* c, const void* d_pks_ser, size_t k, size_t groups, const void* d_pk_hash_in, size_t m,
                                      void* d_out_ts, void* d_out_pk_hash, void* stream) {
    if (int rc = hash_pks_args(c, k, m, groups, (!d_pks_ser && !d_pk_hash_in) || !d_out_ts)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return hash_pks_dev(c, d_pks_ser, k, groups, d_pk_hash_in, m, d_out_ts, d_out_pk_hash, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_hash_pks(blsgpu_ctx* c, const uint8_t* pks_ser, size_t k, size_t groups, const uint8_t* pk_hash_in, size_t m,
                                  uint8_t* out_ts, uint8_t* out_pk_hash) {
    if (int rc = hash_pks_args(c, k, m, groups, (!pks_ser && !pk_hash_in) || !out_ts)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    // (with the digests given the keys are not read: they stay on the host)
    const int dpk = s.in(pk_hash_in ? nullptr : pks_ser, groups * k * 48), dh = s.in(pk_hash_in, groups * 32), dts = s.out(out_ts, groups * m * 32),
              ddg = s.out(out_pk_hash, groups * 32);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = hash_pks_dev(c, s.opt(dpk), k, groups, s.opt(dh), m, s.at(dts), s.opt(ddg), nullptr)) return rc;
    return s.down();
}
BLSGPU_EXPORT int blsgpu_aggregate_pub_keys_secure_dev(blsgpu_ctx* c, const void* d_pts_aff, const void* d_pks_ser, const void* d_pk_hash_in,
                                                       size_t k, size_t groups, void* d_out_aff, void* d_out_inf, void* stream) {
    if (int rc = hash_pks_args(c, k, k, groups, !d_pts_aff || (!d_pks_ser && !d_pk_hash_in) || !d_out_aff)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return aggregate_secure_dev<1>(c, d_pts_aff, k, d_pks_ser, k, d_pk_hash_in, groups, d_out_aff, d_out_inf, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_aggregate_pub_keys_secure(blsgpu_ctx* c, const uint8_t* pts_aff, const uint8_t* pks_ser, const uint8_t* pk_hash_in,
                                                   size_t k, size_t groups, uint8_t* out_aff, uint8_t* out_inf) {
    if (int rc = hash_pks_args(c, k, k, groups, !pts_aff || (!pks_ser && !pk_hash_in) || !out_aff)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int dp = s.in(pts_aff, groups * k * BLSGPU_G1_BYTES), dpk = s.in(pk_hash_in ? nullptr : pks_ser, groups * k * 48),
              dh = s.in(pk_hash_in, groups * 32), dout = s.out(out_aff, groups * BLSGPU_G1_BYTES), dinf = s.out(out_inf, groups);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = aggregate_secure_dev<1>(c, s.at(dp), k, s.opt(dpk), k, s.opt(dh), groups, s.at(dout), s.opt(dinf), nullptr)) return rc;
    return s.down();
}
BLSGPU_EXPORT int blsgpu_aggregate_sigs_secure_dev(blsgpu_ctx* c, const void* d_sigs_aff, size_t k, const void* d_pks_ser, size_t k_pks,
                                                   const void* d_pk_hash_in, size_t groups, void* d_out_aff, void* d_out_inf, void* stream) {
    if (int rc = hash_pks_args(c, k_pks, k, groups, !d_sigs_aff || (!d_pks_ser && !d_pk_hash_in) || !d_out_aff)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return aggregate_secure_dev<2>(c, d_sigs_aff, k, d_pks_ser, k_pks, d_pk_hash_in, groups, d_out_aff, d_out_inf, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_aggregate_sigs_secure(blsgpu_ctx* c, const uint8_t* sigs_aff, size_t k, const uint8_t* pks_ser, size_t k_pks,
                                               const uint8_t* pk_hash_in, size_t groups, uint8_t* out_aff, uint8_t* out_inf) {
    if (int rc = hash_pks_args(c, k_pks, k, groups, !sigs_aff || (!pks_ser && !pk_hash_in) || !out_aff)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int dp = s.in(sigs_aff, groups * k * BLSGPU_G2_BYTES), dpk = s.in(pk_hash_in ? nullptr : pks_ser, groups * k_pks * 48),
              dh = s.in(pk_hash_in, groups * 32), dout = s.out(out_aff, groups * BLSGPU_G2_BYTES), dinf = s.out(out_inf, groups);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = aggregate_secure_dev<2>(c, s.at(dp), k, s.opt(dpk), k_pks, s.opt(dh), groups, s.at(dout), s.opt(dinf), nullptr)) return rc;
    return s.down();
}
BLSGPU_EXPORT int blsgpu_aggregate_priv_keys_secure_dev(blsgpu_ctx* c, const void* d_sks, const void* d_pks_ser, const void* d_pk_hash_in, size_t k,
                                                        size_t groups, void* d_out, void* d_out_pk_aff, void* d_out_pk_ser, void* stream) {
    if (int rc = aggregate_priv_args(c, k, groups, !d_sks || (!d_pks_ser && !d_pk_hash_in) || !d_out)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return aggregate_priv_keys_secure_dev(c, d_sks, d_pks_ser, d_pk_hash_in, k, groups, d_out, d_out_pk_aff, d_out_pk_ser, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_aggregate_priv_keys_secure(blsgpu_ctx* c, const uint8_t* sks, const uint8_t* pks_ser, const uint8_t* pk_hash_in, size_t k,
                                                    size_t groups, uint8_t* out, uint8_t* out_pk_aff, uint8_t* out_pk_ser) {
    if (int rc = aggregate_priv_args(c, k, groups, !sks || (!pks_ser && !pk_hash_in) || !out)) return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    Staging s(c);
    const int dsk = s.in(sks, groups * k * 32), dpk = s.in(pk_hash_in ? nullptr : pks_ser, groups * k * 48), dh = s.in(pk_hash_in, groups * 32),
              dout = s.out(out, groups * 32), daff = s.out(out_pk_aff, groups * 96), dser = s.out(out_pk_ser, groups * 48);
    if (int rc = s.alloc()) return rc;
    if (int rc = s.up()) return rc;
    if (int rc = aggregate_priv_keys_secure_dev(c, s.at(dsk), s.opt(dpk), s.opt(dh), k, groups, s.at(dout), s.opt(daff), s.opt(dser), nullptr))
        return rc;
    return s.down();
}

// ------------------------------------------------------------ ragged secure aggregation: groups of any sizes in one call --
BLSGPU_EXPORT int blsgpu_hash_pks_ranges_dev(blsgpu_ctx* c, const void* d_pks_ser, size_t n_keys, const void* d_pk_off, const void* d_exp_off,
                                             size_t n_exp, size_t groups, const void* d_pk_hash_in, void* d_out_ts, void* d_out_pk_hash, void* stream) {
    if (int rc = secr_args(c, d_pk_hash_in ? 0 : n_keys, n_exp, groups, (!d_pk_hash_in && (!d_pks_ser || !d_pk_off)) || !d_exp_off || !d_out_ts))
        return rc < 0 ? rc : 0;
    HIP_TRY(hipSetDevice(c->device));
    return hash_pks_ranges_dev(c, d_pks_ser, n_keys, d_pk_off, d_exp_off, n_exp, groups, d_pk_hash_in, d_out_ts, d_out_pk_hash, (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_hash_pks_ranges(blsgpu_ctx* c, const uint8_t* pks_ser, size_t n_keys, const uint32_t* pk_off, const uint32_t* exp_off,
                                         size_t groups, const uint8_t* pk_hash_in, uint8_t* out_ts, uint8_t* out_pk_hash) {
    const bool null_buffer = (!pk_hash_in && (!pks_ser || !pk_off)) || !exp_off || !out_ts;
    const size_t n_exp = groups && c && !null_buffer ? exp_off[groups] : 0;
    if (int rc = secr_args(c, pk_hash_in ? 0 : n_keys, n_exp, groups, null_buffer)) return rc < 0 ? rc : 0;
    return secure_ranges_host<0>(c, nullptr, n_exp, exp_off, pks_ser, n_keys, pk_off, groups, pk_hash_in, out_ts, out_pk_hash);
}
// (the sums' own limits on top of secr_args': msm_ranges_args)
BLSGPU_EXPORT int blsgpu_aggregate_pub_keys_secure_ranges_dev(blsgpu_ctx* c, const void* d_pts_aff, const void* d_pks_ser, size_t n_keys,
                                                              const void* d_pk_off, size_t groups, const void* d_pk_hash_in, void* d_out_aff,
                                                              void* d_out_flag, void* stream) {
    if (int rc = secr_args(c, n_keys, n_keys, groups, !d_pts_aff || !d_pk_off || (!d_pks_ser && !d_pk_hash_in) || !d_out_aff || !d_out_flag))
        return rc < 0 ? rc : 0;
    if (ragged::too_large(MSM_CONSTS, n_keys, groups)) return fail(-EINVAL, "batch too large");
    HIP_TRY(hipSetDevice(c->device));
    return aggregate_secure_ranges_dev<1>(c, d_pts_aff, n_keys, d_pk_off, d_pks_ser, n_keys, d_pk_off, groups, d_pk_hash_in, d_out_aff, d_out_flag,
                                          (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_aggregate_pub_keys_secure_ranges(blsgpu_ctx* c, const uint8_t* pts_aff, const uint8_t* pks_ser, size_t n_keys,
                                                          const uint32_t* pk_off, size_t groups, const uint8_t* pk_hash_in, uint8_t* out_aff,
                                                          uint8_t* out_flag) {
    if (int rc = secr_args(c, n_keys, n_keys, groups, !pts_aff || !pk_off || (!pks_ser && !pk_hash_in) || !out_aff || !out_flag)) return rc < 0 ? rc : 0;
    if (ragged::too_large(MSM_CONSTS, n_keys, groups)) return fail(-EINVAL, "batch too large");
    return secure_ranges_host<1>(c, pts_aff, n_keys, pk_off, pks_ser, n_keys, pk_off, groups, pk_hash_in, out_aff, out_flag);
}
BLSGPU_EXPORT int blsgpu_aggregate_sigs_secure_ranges_dev(blsgpu_ctx* c, const void* d_sigs_aff, size_t n_sigs, const void* d_sig_off,
                                                          const void* d_pks_ser, size_t n_keys, const void* d_pk_off, size_t groups,
                                                          const void* d_pk_hash_in, void* d_out_aff, void* d_out_flag, void* stream) {
    if (int rc = secr_args(c, d_pk_hash_in ? 0 : n_keys, n_sigs, groups,
                           !d_sigs_aff || !d_sig_off || (!d_pk_hash_in && (!d_pks_ser || !d_pk_off)) || !d_out_aff || !d_out_flag))
        return rc < 0 ? rc : 0;
    if (ragged::too_large(MSM_CONSTS, n_sigs, groups)) return fail(-EINVAL, "batch too large");
    HIP_TRY(hipSetDevice(c->device));
    return aggregate_secure_ranges_dev<2>(c, d_sigs_aff, n_sigs, d_sig_off, d_pks_ser, n_keys, d_pk_off, groups, d_pk_hash_in, d_out_aff, d_out_flag,
                                          (hipStream_t)stream);
}
BLSGPU_EXPORT int blsgpu_aggregate_sigs_secure_ranges(blsgpu_ctx* c, const uint8_t* sigs_aff, size_t n_sigs, const uint32_t* sig_off,
                                                      const uint8_t* pks_ser, size_t n_keys, const uint32_t* pk_off, size_t groups,
                                                      const uint8_t* pk_hash_in, uint8_t* out_aff, uint8_t* out_flag) {
    if (int rc = secr_args(c, pk_hash_in ? 0 : n_keys, n_sigs, groups,
                           !sigs_aff || !sig_off || (!pk_hash_in && (!pks_ser || !pk_off)) || !out_aff || !out_flag))
        return rc < 0 ? rc : 0;
    if (ragged::too_large(MSM_CONSTS, n_sigs, groups)) return fail(-EINVAL, "batch too large");
    return secure_ranges_host<2>(c, sigs_aff, n_sigs, sig_off, pks_ser, n_keys, pk_off, groups, pk_hash_in, out_aff, out_flag);
}

#ifdef BLSGPU_STAMPS
// diagnostic build: {cycles MUL, LIN, INV, rounds MUL, LIN, INV} of block 0 / wave 0, then reset
BLSGPU_EXPORT int blsgpu_debug_stamps(blsgpu_ctx* c, unsigned long long out[9]) {
    if (!c || !c->tabs.stamps) return fail(-EINVAL, "no stamps");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, c->tabs.stamps, 72, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(c->tabs.stamps, 0, 128));
    return 0;
}
// (running a program round by round against vmgen/tablesim.py needs no diagnostic build: tools/trace_rounds.py does it through
// the test-only libblsgpu_vmcheck.so)
#endif

}  // extern "C"
#endif  // BLSGPU_TU_HOST
