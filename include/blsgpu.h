/*
 * blsgpu.h -- C ABI of the MI355X (gfx950) BLS12-381 multi-pairing engine.
 *
 * Drop-in boundary: this library replaces the reference's only native
 * component for the aggregate-verify path, the Cython/GMP module
 * bls_py.fields_t_c (extmod/bls_py/fields_t_c.pyx), whose functions shadow the
 * pure-Python ones of bls_py/fields_t.py at import (fields_t.py:1218-1265).
 * Each entry point names the reference function it stands in for.
 *
 * Byte conventions = the reference's own serialisation:
 *   Fq    48-byte big-endian canonical residue           (fields.py:87-88)
 *   Fq12  12 x Fq in flat "ZT" order, 576 bytes          (fields.py:624-629, 273-278)
 *   G1    affine x || y, 96 bytes    -- the (x, y) of fq_ate_pairing_multi's Ps
 *   G2    affine x.c0 || x.c1 || y.c0 || y.c1, 192 bytes -- the ((x0,x1),(y0,y1)) of Qs
 * Infinity is the reference's coordinate encoding (0,0) (fields_t.py:609-622).
 *   inf   optional n x 2 bytes, (P flag, Q flag) per pair -- the third member of the
 *         (x, y, inf) tuples fq_ate_pairing_multi takes (fields_t_c.pyx:2333-2346); NULL = all
 *         False.  As in the reference only Q's flag has an effect (fields_t.py:676-677).
 * Coordinates must be canonical residues (< q), as the reference assumes (no check there
 * either).  For EVERY such input -- points of the wrong order, off the curve, zero
 * coordinates, flags -- the pairing entry points return the reference's bytes: pairs on
 * which the reference's special cases decide (0^-1 := 0, fields_t.py:47-55; the branches of
 * fq2_add_line_eval :1062-1065 and fq2_add_points :673-686) are detected on the GPU and
 * recomputed there by a reference-faithful program (k_miller_slow).
 *
 * All functions return 0 on success or a negative errno-style code;
 * blsgpu_last_error() describes the last failure on the calling thread.
 * Buffers are caller-allocated; nothing owned by the library crosses the ABI
 * except the opaque context.
 *
 * Threading and streams.  A context is used by ONE host thread at a time (the reference's
 * native module is not re-entrant either: module-global scratch pools,
 * fields_t_c.pyx:2401-2412); different contexts are independent.  Every `_dev` entry point
 * enqueues on the caller's stream and returns; all of a context's work shares one
 * workspace, so a call on another stream than the context's previous call first waits (on
 * the device) for that earlier work -- for concurrency use one context per stream.  The
 * workspace only grows: a buffer that a larger one replaces is kept until
 * blsgpu_ctx_trim / blsgpu_ctx_destroy, so growth never invalidates enqueued work and never
 * synchronises the device inside a pipeline; blsgpu_ctx_reserve sizes it up front.
 */
#ifndef BLSGPU_H
#define BLSGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLSGPU_FQ_BYTES 48
#define BLSGPU_G1_BYTES 96
#define BLSGPU_G2_BYTES 192
#define BLSGPU_FQ12_BYTES 576
#define BLSGPU_PARTIAL_WORDS 144   /* one Fq12 in Montgomery limb form, uint32 */

typedef struct blsgpu_ctx blsgpu_ctx;

/* Library / table identification string (static storage). */
const char *blsgpu_version(void);
const char *blsgpu_last_error(void);

/* Create a context on HIP device `device` (uploads the schedule tables).
 * Fails with -ENODEV (-19) when no gfx950-class GPU is usable: there is no CPU
 * fallback in this library. */
int blsgpu_ctx_create(int device, blsgpu_ctx **out);
void blsgpu_ctx_destroy(blsgpu_ctx *ctx);
/* Pre-size the per-context workspace for batches of up to max_pairs pairs. */
int blsgpu_ctx_reserve(blsgpu_ctx *ctx, size_t max_pairs);
/* Bytes of device memory the context's grow-only workspace holds right now, by purpose (the high-water mark of the
 * calls made so far; the line-stream stage keeps 68 x 336 bytes of line records per pair of its largest call, the
 * counterpart of the n-arrays of mpz_t the reference mallocs per call, fields_t_c.pyx:2348-2388).  out[BLSGPU_WS_TOTAL]
 * is the sum (which also counts the fixed-base G1 table and the HD derivation slice, blsgpu_g1_mul_gen /
 * blsgpu_hd_children, the per-path state of blsgpu_hd_paths, the commitments of blsgpu_g1_poly_check and the Lagrange
 * coefficients of blsgpu_threshold_combine / blsgpu_fr_interpolate_at_zero, the table of blsgpu_g1_mul_gen_secret, the
 * point tables of blsgpu_g2_mul_secret / blsgpu_sign, the scalars and point copies of blsgpu_sign_threshold, the leaves and
 * round buffers of blsgpu_sig_shares_check, and the keys blsgpu_keys_from_seeds holds back; they have no field of their own).
 * BLSGPU_WS_FLAGS_AND_LISTS counts the flag copy of blsgpu_miller_loop_batch's fast form as well (2 bytes per pair of a
 * slice).  No device call is made. */
enum { BLSGPU_WS_PARTIALS = 0, BLSGPU_WS_STAGING, BLSGPU_WS_LINES, BLSGPU_WS_LINE_PRODUCTS, BLSGPU_WS_FLAGS_AND_LISTS,
       BLSGPU_WS_GROUP_SUMS, BLSGPU_WS_SLOTS, BLSGPU_WS_TOTAL, BLSGPU_WS_FIELDS };
int blsgpu_ctx_workspace_bytes(blsgpu_ctx *ctx, size_t out[BLSGPU_WS_FIELDS]);
/* Wait for the context's enqueued work and free the buffers that larger ones replaced.  The fixed-base G1 table of
 * blsgpu_g1_mul_gen stays (0.9 MB, built once), and so does the 58 KB table of blsgpu_g1_mul_gen_secret: blsgpu_ctx_destroy
 * frees them. */
int blsgpu_ctx_trim(blsgpu_ctx *ctx);
/* Batches of at least `pairs` pairs run the throughput-oriented Miller kernel
 * (several pairs per wavefront sharing one accumulator); smaller batches the
 * latency-oriented one (one pair per wavefront).  Default 4096; 0 = always the
 * throughput kernel.  Results are identical either way. */
int blsgpu_ctx_set_mp_threshold(blsgpu_ctx *ctx, size_t pairs);
/* Measurement aid (bench.py): the chip's 32 x 32 + 64-bit multiply-add rate (v_mad_i64_i32) measured NOW by a probe kernel of
 * about `target_ms` milliseconds on `stream`; *tmacs = 10^12 multiply-adds per second.  The roofline of this path is that
 * instruction's issue rate (integer VALU, not HBM or MFMA), and the clock the package's power limit leaves differs
 * by a few per cent between boxes. */
int blsgpu_timing_mad_probe(blsgpu_ctx *ctx, double target_ms, double *tmacs, void *stream);
/* Measurement aid: one dispatch of an empty kernel (blsgpu::probe::k_mark) on `stream`.  bench.py brackets every timed region
 * with two of them; tools/collect_profiles.py cuts the per-dispatch counters of a rocprofv3 --pmc run to the dispatches between
 * the marks (the HBM traffic per step of roofline.traffic). */
int blsgpu_timing_mark(blsgpu_ctx *ctx, unsigned tag, void *stream);
/* Calls of at most `pairs` pairs (below the line-stream threshold) run the WIDE Miller loop (csrc/blsgpu_mlw.hip): one pair
 * per workgroup of two wavefronts with a field product per lane -- the loop of fq_miller_loop (fields_t.py:1091-1111) at
 * the depth of one wavefront's instruction stream, the latency form for BLS.verify of a few signatures
 * (bls.py:197-201).  Default 1536 (measured crossover against the wavefront-VM kernel, tools/miller_wide_probe.py); 0 = never (the wavefront-VM kernels).  Results are identical either way.
 * Any value is valid: the loop leaves one partial per pair, and the workspace of a call follows the kernel it takes. */
int blsgpu_ctx_set_miller_wide_max(blsgpu_ctx *ctx, size_t pairs);
/* The throughput kernel runs three pairs per wavefront from `pairs` pairs per call on and two pairs per
 * wavefront below (a call of a few thousand pairs fills the chip with teams of two and each finishes sooner).
 * 0 = always three; (size_t)-1 = the measured schedule (default: two up to ~8.7 k pairs and in the pockets
 * where teams of two quantise better, three elsewhere).  Results are identical either way. */
int blsgpu_ctx_set_mp3_threshold(blsgpu_ctx *ctx, size_t pairs);
/* Calls of at least `pairs` pairs whose groups all have at least `min_group` pairs run the LINE-STREAM form of
 * the Miller loops (csrc/blsgpu_ml.hip: the twist-point chains alone, their 68 lines per pair through
 * HBM, the accumulator products six lanes each, Horner over the line indices) -- the same loop as
 * fq_miller_loop, fields_t.py:1091-1111, cut where the data dependency allows.  Default 2304 / 64 (the measured
 * crossover, tools/ls_wide_sweep.py; calls of up to 5120 pairs run the point chains sixteen lanes per pair with the values in
 * LDS -- csrc/blsgpu_lsw.hip --, up to 20 480 pairs four lanes per pair, above that two); (size_t)-1
 * keeps every call on the wavefront-VM kernels.  Results are identical either way. */
int blsgpu_ctx_set_ls_threshold(blsgpu_ctx *ctx, size_t pairs, size_t min_group);
/* Number of accumulators the line-stream product kernel aims at (default 163840): a group's pairs are cut into equal
 * chunks of at least 16 pairs, one accumulator per (chunk, line index); the chunks' products are merged by a tree of
 * dense products.  A tuning knob; results are identical for every value. */
int blsgpu_ctx_set_ls_teams(blsgpu_ctx *ctx, size_t teams);
/* `event` (a hipEvent_t, or NULL for none) is recorded on the call's stream right after the last kernel of a Miller
 * stage that fills the chip; what follows (Horner over the line products, the product of the partials, the final
 * exponentiation) occupies a few dozen wavefronts.  A caller that pipelines calls over several contexts lets the
 * next call's stream wait for this event instead of the end of the call (bench.py does). */
int blsgpu_ctx_set_bulk_event(blsgpu_ctx *ctx, void *event);
/* Calls that end in at least `results` final exponentiations (fq12_final_exp, fields_t.py:1124-1128) run them six
 * lanes per result, ten results per wavefront, on the register arithmetic (csrc/blsgpu_fexp.hip: the fewest
 * instructions per result, 2.6 ms of latency).  Fewer results run ONE PER WAVEFRONT with every Fq product of a step
 * on its own lane (csrc/blsgpu_fexpw.hip: 0.70 ms for one result against 1.25 ms of the wavefront-VM program of
 * rounds 1 - 3, which BLSGPU_FEXP_WIDE=0 in the environment brings back).  Default 5120 (the measured crossover: 4096 results 3.55 against 4.04 ms, 6144 results 5.09 against 4.77 ms);
 * (size_t)-1: never.  Results are identical either way. */
int blsgpu_ctx_set_fexp_team_threshold(blsgpu_ctx *ctx, size_t results);
/* Diagnostic: a device buffer of (script length) x 576 bytes that receives the accumulator of result 0 after every
 * operation of the batched final exponentiation's script -- the six-lanes-per-result form k_fexp_team only; force it with
 * blsgpu_ctx_set_fexp_team_threshold(ctx, 1) -- (tools/fexp_trace.py compares it with the integer model), or
 * NULL (default). */
int blsgpu_ctx_set_fexp_trace(blsgpu_ctx *ctx, void *d_buf);
/* Diagnostic: a device buffer of (script length + 1) x 8 bytes that receives the GPU cycle counter of result 0 before the
 * one-result-per-wavefront final exponentiation's script (csrc/blsgpu_fexpw.hip) and after every operation of it
 * (tools/fexpw_stamps.py), or NULL (default).  (A buffer of its own: blsgpu_ctx_set_fexp_trace's holds field elements and is
 * written by the six-lanes-per-result form only.) */
int blsgpu_ctx_set_fexpw_stamps(blsgpu_ctx *ctx, void *d_buf);
/* Diagnostic: the first `bytes` bytes of the line records the last line-stream call left in the workspace
 * (lines[(L * n + pair) * 84] int32, csrc/blsgpu_ml.hip); tools/exact_trace.py compares them with the integer model. */
int blsgpu_debug_read_lines(blsgpu_ctx *ctx, void *host_buf, size_t bytes);

/* The device work of BLS.verify (bls.py:153-201) in ONE call:  e(-G1, sig) * prod_i e(P_i, H(m_i))  for n distinct
 * message hashes (32 bytes each) -- hash_to_point_prehashed_Fq2 of every hash (bls.py:194-195, ec.py:528-550), the
 * per-message key P_i either given (keys_affine: n x 96 bytes) or folded here as sum_j t_ij pk_ij (bls.py:177-192:
 * key_pts n x k x 96 bytes, key_scalars n x k x 32 bytes big-endian), then the (n + 1)-pair multi-pairing in the
 * reference's order Ps[0] = -G1, Qs[0] = sig (bls.py:197-199).  One upload, nothing returns to the host between the
 * stages, 576 bytes back: the caller compares them with Fq12 one.  The scheme logic around it (grouping keys by
 * message, the False of a missing tree key, bls.py:181-190) stays with the caller. */
int blsgpu_verify_pipeline(blsgpu_ctx *ctx, const uint8_t neg_g1[BLSGPU_G1_BYTES], const uint8_t sig[BLSGPU_G2_BYTES],
                           const uint8_t *msg_hashes, size_t n, const uint8_t *keys_affine, const uint8_t *key_pts,
                           const uint8_t *key_scalars, size_t k, uint8_t out[BLSGPU_FQ12_BYTES]);
/* The same on device-resident buffers, enqueued on `stream`: d_g1 = (n + 1) x 96 bytes with slot 0 = -G1 and slots
 * 1 .. n the keys (k == 0) or left for the key sums to fill (k > 0); d_g2 = (n + 1) x 192 bytes with slot 0 = sig,
 * slots 1 .. n filled by the hash; d_out receives 576 bytes. */
int blsgpu_verify_pipeline_dev(blsgpu_ctx *ctx, void *d_g1, void *d_g2, const void *d_msg_hashes, size_t n,
                               const void *d_key_pts, const void *d_key_scalars, size_t k, void *d_out, void *stream);

/* BLS.verify of m aggregates of ANY shapes in ONE call (csrc/blsgpu_veragg.hip; csrc/verify_agg_plan.h is its schedule): the
 * bytes and three tables go up once, nothing returns to the host between the stages, m status bytes come back.
 *   sigs        m x 192 bytes, the aggregates' signatures, affine G2
 *   msg_hashes  n_msgs x 32 bytes; each is hashed to G2 ONCE per call, however many groups name it (an entry no group names
 *               is hashed too)
 *   keys, exps  n_keys x 96 bytes affine G1 and n_keys x 32 bytes big-endian exponents, or exps == NULL: every exponent is 1
 *   grp_off     n_grp + 1 offsets into keys: group g sums the keys [grp_off[g], grp_off[g + 1])
 *   grp_msg     n_grp indices into msg_hashes
 *   agg_off     m + 1 offsets into the groups: aggregate j owns the groups [agg_off[j], agg_off[j + 1])
 * For aggregate j the value computed is fq_ate_pairing_multi of the pairs (-G1, sig_j), (sum_i e_i pk_i over group g,
 * H(msg_hashes[grp_msg[g]])) for g in j's groups in order -- the pair order of bls.py:197-199; -G1 is the library's own.
 * status[j]: 1 the value is Fq12 one, 0 it is not, 2 NOT DECIDED here (the caller runs its exact path): the signature is (0,0)
 * -- an infinity signature carries the one flag the reference's Miller loop reads --, or one of j's groups holds a key that is
 * neither (0,0) nor on the curve (flag 2 of the sums).  A key sum at infinity is NOT status 2: its (0,0) goes into the pair
 * list with no flag, exactly as blsgpu_verify_pipeline_dev hands it on.  An aggregate with no groups is the one-pair product.
 * out_gt: m x 576 bytes, the value of every aggregate (unspecified where status is 2), or NULL.
 * Stages: the key sums of all groups -- blsgpu_g1_msm_ranges' implementation with exps, blsgpu_g1_range_sums' without (the same
 * bytes for unit exponents) --, the hash to G2 of all n_msgs hashes, then per slice of whole aggregates (pair lists of at most
 * 2^20 pairs; a longer aggregate is a slice of its own) k_va_pairs gathers the pair list in 16-byte moves, the ragged
 * multi-pairing (blsgpu_pairing_multi_ranges' implementation) runs a range per aggregate, and k_va_status writes the bytes.
 * The call inherits what its stages cost: the serial chain of the ragged sums on a long group and the ragged multi-pairing's
 * loss on one long range (README).  Measured (profiles/verify_aggregates_probe.txt, one run, host buffers, medians of 3): 32 768
 * single-key signatures over distinct messages 28.9 ms, 1000 aggregates of 2 .. 201 messages 33.9 ms, one message with 1024 keys
 * plus 1024 messages with one key 21.4 ms.  The _dev form alone: NOT MEASURED.
 * The three tables are HOST memory in BOTH forms: validation and the whole schedule are host arithmetic on them, the derived
 * tables go up in one copy, and they may be released or changed as soon as the call returns.  The workspace counts in
 * BLSGPU_WS_TOTAL, the line records in BLSGPU_WS_LINES; every buffer of every slice is sized before the first launch.
 * -EINVAL before anything is written: a NULL required buffer (sigs, status, agg_off, grp_off with m > 0; grp_msg with
 * n_grp > 0; keys with n_keys > 0; msg_hashes with n_msgs > 0), a table that steps down, grp_off[n_grp] != n_keys,
 * agg_off[m] != n_grp, grp_msg[g] >= n_msgs (blsgpu_last_error names the first offending entry), m + n_grp > 0x3FFFFFF0,
 * n_msgs > 0x03FFFFF0, n_keys > 0xFFFFFFF0.  -ENOMEM when the line records cannot be allocated.  m == 0 writes nothing and
 * returns 0.  All of this is PUBLIC data: not constant-time. */
int blsgpu_verify_aggregates(blsgpu_ctx *ctx, const uint8_t *sigs, const uint8_t *msg_hashes, size_t n_msgs, const uint8_t *keys,
                             const uint8_t *exps, size_t n_keys, const uint32_t *grp_off, const uint32_t *grp_msg, size_t n_grp,
                             const uint32_t *agg_off, size_t m, uint8_t *status, uint8_t *out_gt);
/* The same with the points, hashes, exponents, status and out_gt in device memory (points and out_gt 16-byte aligned), on
 * `stream`; the three tables stay HOST memory.  With exps the call inherits the ONE synchronisation of that stream by which the
 * ragged multi-scalar sums read their chunk count (before anything is written to status or out_gt); with exps == NULL it
 * does not synchronise. */
int blsgpu_verify_aggregates_dev(blsgpu_ctx *ctx, const void *d_sigs, const void *d_msg_hashes, size_t n_msgs, const void *d_keys,
                                 const void *d_exps, size_t n_keys, const uint32_t *grp_off, const uint32_t *grp_msg, size_t n_grp,
                                 const uint32_t *agg_off, size_t m, void *d_status, void *d_out_gt, void *stream);

/* fq_ate_pairing_multi(Ps, Qs) -- fields_t.py:1114-1121 / fields_t_c.pyx:2333-2391.
 * Host buffers in, 576 result bytes out; synchronous.  n == 0 returns one. */
int blsgpu_pairing_multi(blsgpu_ctx *ctx, const uint8_t *g1, const uint8_t *g2, const uint8_t *inf,
                         size_t n, uint8_t out[BLSGPU_FQ12_BYTES]);

/* Same computation on device-resident buffers, enqueued on `stream`
 * (a hipStream_t, or NULL for the default stream); asynchronous.
 * d_out receives 576 bytes. */
int blsgpu_pairing_multi_dev(blsgpu_ctx *ctx, const void *d_g1, const void *d_g2, const void *d_inf,
                             size_t n, void *d_out, void *stream);

/* fq_miller_loop(px, py, pinf, qx, qy, qinf) -- fields_t.py:1091-1111 / fields_t_c.pyx:2295-2319
 * (pairing.miller_loop, pairing.py:51-65) for n pairs at once: out receives n x 576 bytes,
 * the reference's own Miller values bit for bit (computed by the reference-faithful program:
 * affine twist point, one inversion per step; the throughput path is blsgpu_pairing_multi). */
int blsgpu_miller_loop_batch(blsgpu_ctx *ctx, const uint8_t *g1, const uint8_t *g2, const uint8_t *inf,
                             size_t n, uint8_t *out);
int blsgpu_miller_loop_batch_dev(blsgpu_ctx *ctx, const void *d_g1, const void *d_g2, const void *d_inf,
                                 size_t n, void *d_out, void *stream);

/* fq2_double_line_eval(R, P) -- fields_t.py:1035-1049 / fields_t_c.pyx:1416-1445 (q == NULL) and
 * fq2_add_line_eval(R, Q, P) -- fields_t.py:1052-1078 / fields_t_c.pyx:1448-1511 (pairing.double_line_eval,
 * pairing.add_line_eval, pairing.py:16-48), for n triples at once: r, q: n x 192 bytes (twist
 * points), p: n x 96 bytes; out: n x 576 bytes, the reference's Fq12 line values. */
int blsgpu_line_eval_batch(blsgpu_ctx *ctx, const uint8_t *r, const uint8_t *q, const uint8_t *p, size_t n,
                           uint8_t *out);

/* The Fq12 arithmetic of the reference's native module on n elements at once (576 bytes each; an Fq, Fq2 or
 * Fq6 element is an Fq12 element whose other coefficients are zero):
 *   op 0 fq12_add (fields_t.py:339-343), 1 fq12_sub (:346-350), 2 fq12_mul (:503-554 / fields_t_c.pyx:824-875),
 *      3 fq12_neg (:321-325), 4 fq12_invert (:328-337; 0 -> 0 as fq_invert :47-55);  b is ignored for 3 and 4.
 * blsgpu_fq12_pow_batch: fq12_pow(a_i, e) (:340-353 / fields_t_c.pyx:771-821) for ONE exponent e given as
 * e_len big-endian bytes. */
int blsgpu_fq12_op_batch(blsgpu_ctx *ctx, int op, const uint8_t *a, const uint8_t *b, size_t n, uint8_t *out);
int blsgpu_fq12_pow_batch(blsgpu_ctx *ctx, const uint8_t *a, const uint8_t *e_be, size_t e_len, size_t n,
                          uint8_t *out);

/* Sharded form (one rank per GPU).  Step 1: the product of the n Miller-loop
 * values of this shard (fq_miller_loop, fields_t.py:1091-1111, folded with
 * fq12_mul as in :1119-1120) as ONE partial of BLSGPU_PARTIAL_WORDS uint32.
 * Step 2, after the partials of all ranks were gathered: their product and the
 * final exponentiation (fq12_final_exp, fields_t.py:1124-1128) -> 576 bytes. */
int blsgpu_miller_product_dev(blsgpu_ctx *ctx, const void *d_g1, const void *d_g2, const void *d_inf,
                              size_t n, void *d_partial, void *stream);
int blsgpu_final_exp_product_dev(blsgpu_ctx *ctx, const void *d_partials, size_t m,
                                 void *d_out, void *stream);

/* fq12_final_exp(t) on a host element (fields_t.py:1124-1128). */
int blsgpu_final_exp(blsgpu_ctx *ctx, const uint8_t in[BLSGPU_FQ12_BYTES],
                     uint8_t out[BLSGPU_FQ12_BYTES]);

/* m independent fq12_final_exp (fields_t.py:1124-1128), host buffers m x 576 bytes. */
int blsgpu_final_exp_batch(blsgpu_ctx *ctx, const uint8_t *in, size_t m, uint8_t *out);

/* `groups` independent fq_ate_pairing_multi calls of gsz pairs each, in one
 * launch sequence (e.g. 10 000 threshold verifications of 2 pairs: BLS.verify,
 * bls.py:153-201, once per group).  Pairs are stored group after group;
 * out receives groups x 576 bytes. */
int blsgpu_pairing_multi_batch(blsgpu_ctx *ctx, const uint8_t *g1, const uint8_t *g2, const uint8_t *inf,
                               size_t gsz, size_t groups, uint8_t *out);
int blsgpu_pairing_multi_batch_dev(blsgpu_ctx *ctx, const void *d_g1, const void *d_g2, const void *d_inf,
                                   size_t gsz, size_t groups, void *d_out, void *stream);

/* RAGGED multi-pairing (csrc/blsgpu_mlr.hip; csrc/pairing_ranges_plan.h is its schedule):
 * out[j] = fq_ate_pairing_multi of the pairs [begin_j, end_j) of ONE list of n pairs, for m ranges of ANY lengths, in one launch
 * sequence and with nothing padded -- where blsgpu_pairing_multi_batch takes runs of one and the same gsz.  g1, g2, inf: the n
 * pairs and their flag bytes, laid out as in blsgpu_pairing_multi_batch (inf may be NULL).  ranges: m x 2 uint32 (begin, end),
 * begin <= end <= n; ranges may overlap, repeat or be empty, and each pays for its own chunks.  An empty range gives Fq12 one,
 * as blsgpu_pairing_multi does for n == 0.  out: m x 576 bytes.  Every input the reference accepts (infinity, off-curve, zero
 * and flagged points) gives the reference's bytes, as in every other pairing call.
 * Every range is cut into chunks of at most 16 consecutive pairs (BLSGPU_PAIR_RANGES_CHUNK at context creation); the point
 * chains of the line-stream stage run once per PAIR of the list (whether or not a range holds it: hand in the pairs the ranges
 * use), one six-lane accumulator runs the Miller loop of one chunk, the chunks' partials of a range are multiplied in levels of
 * 8, and one final exponentiation per range ends the call.  The pair list is processed in slices of 2^20 pairs (the line
 * records cost 22.8 KB per pair); a range may span slices.
 * The range table is a HOST pointer in BOTH forms: the whole schedule -- validation, chunks, fold levels, buffer sizes -- is
 * host arithmetic on it, nothing is read back from the device and the _dev form does not synchronise.  The table may be
 * released or changed as soon as the call returns.  The workspace (partials and tables) counts in BLSGPU_WS_TOTAL, the line
 * records in BLSGPU_WS_LINES.
 * -EINVAL before anything is written: a NULL required buffer (g1 or g2 with n > 0; ranges or out with m > 0), a range with
 * begin > end or end > n, n > 0x3FFFFFF0, 2^31 chunks or more in all.  -ENOMEM when the line records cannot be allocated (this
 * call has no other form to fall back to); every buffer is sized before the first launch.  m == 0 writes nothing and
 * returns 0.  All of this is PUBLIC data: not constant-time. */
int blsgpu_pairing_multi_ranges(blsgpu_ctx *ctx, const uint8_t *g1, const uint8_t *g2, const uint8_t *inf, size_t n,
                                const uint32_t *ranges, size_t m, uint8_t *out);
/* The same with the pairs, the flags and the results in device memory (points 16-byte aligned), on `stream`; `ranges` stays
 * HOST memory. */
int blsgpu_pairing_multi_ranges_dev(blsgpu_ctx *ctx, const void *d_g1, const void *d_g2, const void *d_inf, size_t n,
                                    const uint32_t *ranges, size_t m, void *d_out, void *stream);

/* Sharded form of the batch: every rank holds gsz pairs of each of the `groups`
 * multi-pairings.  Step 1 writes one partial per group (groups x
 * BLSGPU_PARTIAL_WORDS uint32).  Step 2 takes the all-gathered buffer of m ranks
 * (partial of rank i, group g at index i * groups + g), multiplies per group and
 * applies fq12_final_exp (fields_t.py:1116-1121 per group) -> groups x 576 bytes. */
int blsgpu_miller_product_batch_dev(blsgpu_ctx *ctx, const void *d_g1, const void *d_g2, const void *d_inf,
                                    size_t gsz, size_t groups, void *d_partials, void *stream);
int blsgpu_final_exp_product_batch_dev(blsgpu_ctx *ctx, const void *d_partials, size_t m,
                                       size_t groups, void *d_out, void *stream);

/* Multi-scalar sums  out[g] = sum_{i<k} scalars[g*k+i] * pts[g*k+i]  for `groups`
 * independent groups of k points: the loops of BLS.aggregate_pub_keys
 * (bls.py:203-223, G1), BLS.aggregate_sigs* (bls.py:12-151, G2) and
 * Threshold.aggregate_unit_sigs (threshold.py:127-136, G2), i.e. the reference's
 * fq_/fq2_scalar_mult_jacobian + *_add_points_jacobian (fields_t.py:705-875).
 * pts: affine big-endian coordinates (96 B per G1 point, 192 B per G2 point,
 * (0,0) = infinity); scalars: 32 bytes big-endian each, or NULL for plain sums;
 * out: affine bytes per group ((0,0) for infinity); out_inf (may be NULL): 1 if
 * the group's sum is the point at infinity. */
int blsgpu_g1_msm(blsgpu_ctx *ctx, const uint8_t *pts, const uint8_t *scalars, size_t k,
                  size_t groups, uint8_t *out, uint8_t *out_inf);
int blsgpu_g2_msm(blsgpu_ctx *ctx, const uint8_t *pts, const uint8_t *scalars, size_t k,
                  size_t groups, uint8_t *out, uint8_t *out_inf);
int blsgpu_g1_msm_dev(blsgpu_ctx *ctx, const void *d_pts, const void *d_scalars, size_t k,
                      size_t groups, void *d_out, void *d_out_inf, void *stream);
int blsgpu_g2_msm_dev(blsgpu_ctx *ctx, const void *d_pts, const void *d_scalars, size_t k,
                      size_t groups, void *d_out, void *d_out_inf, void *stream);

/* Hash to G2 after the SHA-256 step: hash_to_point_prehashed_Fq2 (ec.py:528-550)
 * from the two Fq2 elements t0, t1 (the four hash512 values of ec.py:531-534,
 * reduced mod q) onwards: sw_encode twice (ec.py:449-507), their sum, cofactor
 * clearing with psi.  t: n x 192 bytes (t0.c0, t0.c1, t1.c0, t1.c1 big-endian
 * canonical); out: n x 192 bytes affine G2, (0,0) for infinity.  t = 0 encodes
 * to infinity as in ec.py:450-452; a candidate x whose x^3 + b' has zero imaginary part is skipped
 * as the reference's bare `except` skips it (ec.py:489-498).  Where the reference's sw_encode itself
 * raises (its LAST candidate is of that kind -- never for hashed input) the output is unspecified. */
int blsgpu_map_to_g2(blsgpu_ctx *ctx, const uint8_t *t, size_t n, uint8_t *out);
int blsgpu_map_to_g2_dev(blsgpu_ctx *ctx, const void *d_t, size_t n, void *d_out, void *stream);

/* The whole hash_to_point_prehashed_Fq2(m) (ec.py:528-550) for n 32-byte messages m
 * (the message hashes of AggregationInfo, bls.py:194-195): the four hash512 values
 * (util.py:13-16, SHA-256 on the GPU) reduced mod q, then as blsgpu_map_to_g2.
 * msg_hashes: n x 32 bytes; out: n x 192 bytes affine G2. */
int blsgpu_hash_to_g2(blsgpu_ctx *ctx, const uint8_t *msg_hashes, size_t n, uint8_t *out);
int blsgpu_hash_to_g2_dev(blsgpu_ctx *ctx, const void *d_msg_hashes, size_t n, void *d_out, void *stream);

/* Hash to G1 after the SHA-256 step: hash_to_point_prehashed_Fq (ec.py:511-520) from the two field elements t0, t1
 * onwards -- sw_encode over Fq twice (ec.py:449-507), their sum, multiplication by the cofactor
 * h = 0x396c8c005555e1568c00aaab0000aaab -- one message per lane in registers (k_h2g1, blsgpu_h2g1.hip).
 * t: n x 96 bytes, t0 || t1 as 48-byte big-endian integers; any value below 2^384 is taken mod q, as Fq(q, v) does.
 * t = 0 encodes to infinity (ec.py:450-452); t^2 = -5 (reachable: -5 is a square mod q) encodes to the generator, negated
 * when t > q - t (ec.py:466-473).  out_aff: n x 96 bytes affine, (0, 0) for infinity; out_ser: n x 48 bytes, the compression
 * blsgpu_g1_mul_gen writes (x with 0x80 on the first byte when y > q // 2, 48 zero bytes for infinity); out_inf (may be
 * NULL): n flags, 1 for infinity.  out_aff and out_ser may each be NULL, not both: both NULL, or a NULL input, with n > 0
 * is -EINVAL before anything is written.  n == 0 writes nothing and returns 0.  The calls take no workspace; the host-buffer
 * form stages slices of 262 144 messages.  Every input is public data: NOT constant-time. */
int blsgpu_map_to_g1(blsgpu_ctx *ctx, const uint8_t *t, size_t n, uint8_t *out_aff, uint8_t *out_ser, uint8_t *out_inf);
/* The same with every buffer in device memory, enqueued on `stream` (no synchronisation). */
int blsgpu_map_to_g1_dev(blsgpu_ctx *ctx, const void *d_t, size_t n, void *d_out_aff, void *d_out_ser, void *d_out_inf, void *stream);

/* The whole hash_to_point_prehashed_Fq(m) (ec.py:511-520) for n 32-byte messages m: t_j = hash512(m || "G1_j") mod q for
 * j = 0, 1 (util.py:13-16: four one-block SHA-256 compressions per message, in the same kernel -- the digests never visit
 * the host), then as blsgpu_map_to_g1.  msg_hashes: n x 32 bytes; outputs and argument rules as blsgpu_map_to_g1. */
int blsgpu_hash_to_g1(blsgpu_ctx *ctx, const uint8_t *msg_hashes, size_t n, uint8_t *out_aff, uint8_t *out_ser, uint8_t *out_inf);
/* The same with every buffer in device memory, enqueued on `stream` (no synchronisation). */
int blsgpu_hash_to_g1_dev(blsgpu_ctx *ctx, const void *d_msg_hashes, size_t n, void *d_out_aff, void *d_out_ser, void *d_out_inf, void *stream);

/* Batched point decompression: PublicKey.from_bytes (keys.py:28-40) and
 * Signature.from_bytes (signature.py:21-38) from the serialised bytes: mask the top
 * three bits (`& 0x1f`), y_for_x (ec.py:255-269; square roots fields.py:199-205 and
 * 463-482), and the reference's choice between y and -y by bit 0x80 (G2: on the
 * imaginary part only, signature.py:31-35).  in: n x 48 (G1) / n x 96 (G2) bytes;
 * out: n x 96 / n x 192 bytes affine; ok[i] = 1 iff the reference accepts encoding i (it raises
 * otherwise -- ValueError, or for a G2 x whose x^3 + 4(1+i) has zero imaginary part the AffinePoint
 * constructor's Exception, because Fq2.modsqrt returns an Fq there, fields.py:466-467; out bytes of
 * such an entry are unspecified). */
int blsgpu_g1_decompress(blsgpu_ctx *ctx, const uint8_t *in, size_t n, uint8_t *out, uint8_t *ok);
int blsgpu_g2_decompress(blsgpu_ctx *ctx, const uint8_t *in, size_t n, uint8_t *out, uint8_t *ok);
int blsgpu_g1_decompress_dev(blsgpu_ctx *ctx, const void *d_in, size_t n, void *d_out, void *d_ok, void *stream);
int blsgpu_g2_decompress_dev(blsgpu_ctx *ctx, const void *d_in, size_t n, void *d_out, void *d_ok, void *stream);

/* Fixed-base multiplication by the generator:  out_i = (s_i mod n) G1 (+ A_i)  for n scalars at once -- the
 * PrivateKey.get_public_key of the reference (keys.py:104-105, G1 * sk with the generator of ec.py:394-396) and, with A,
 * the public derivation step sk_left.get_public_key().value + self.public_key.value (keys.py:292-293).  A scalar is 32 bytes
 * big-endian, any value below 2^256 (reduced mod the group order on the device: the same point); its product is a sum of
 * 32 entries of a table of d 2^(8w) G1 (8-bit windows, 0.9 MB) that the context builds on first use and keeps until
 * blsgpu_ctx_destroy -- no doubling, one inversion per scalar (csrc/blsgpu_g1fix.hip).  The table is indexed by the
 * scalar's digits: NOT constant-time (nor is the variable-base path of blsgpu_g1_msm); blsgpu_g1_mul_gen_secret below is
 * the form for private keys.
 * add: NULL (n_add = 0), one point added to every product (n_add = 1) or one per scalar (n_add = n); 96 bytes affine,
 * (0, 0) = infinity.  out_aff: n x 96 bytes affine ((0, 0) for infinity); out_ser: n x 48 bytes, PublicKey.serialize()
 * (ec.py:94-111: x big-endian with 0x80 when y > q // 2; 48 zero bytes for infinity); either may be NULL, not both.
 * n == 0 writes nothing. */
int blsgpu_g1_mul_gen(blsgpu_ctx *ctx, const uint8_t *scalars, size_t n, const uint8_t *add, size_t n_add, uint8_t *out_aff,
                      uint8_t *out_ser);
int blsgpu_g1_mul_gen_dev(blsgpu_ctx *ctx, const void *d_scalars, size_t n, const void *d_add, size_t n_add, void *d_out_aff,
                          void *d_out_ser, void *stream);
/* The same product for SECRET scalars (a private key's public key):  out_i = s_i G1  with a schedule independent of s
 * (csrc/blsgpu_g1fix.hip k_fix_mul_secret; vmgen/g1fixs_model.py is its specification).  s_i is the literal 256-bit integer
 * of 32 big-endian bytes; G1 has order n, so the bytes equal those of blsgpu_g1_mul_gen.  There is no `add`: the added
 * point belongs to public derivation.
 * The claim is exactly that of blsgpu_g2_mul_secret: the sequence of instructions and of memory addresses does not depend
 * on the scalars.  One scalar per lane; signed 4-bit digits of s + C over 65 windows (plain carries); a second per-context
 * table of (e + 1) 16^w G1, w < 65, e < 8 (affine, 58 240 bytes, built on first use, kept until blsgpu_ctx_destroy, counted
 * in BLSGPU_WS_TOTAL only); per window every lane reads all eight entries -- the address depends on the window alone --
 * keeps one by compare-and-select, its sign by a select between y and -y, and runs one complete mixed addition; for a zero
 * digit entry 0 is added all the same and the old accumulator kept by select.  65 additions, no doubling, nothing skipped;
 * the affine conversion is the fixed-length branch-free inversion.  NOT claimed: data-dependent timing inside the hardware
 * (how long an instruction or a memory access takes for given values).
 * out_aff / out_ser as in blsgpu_g1_mul_gen: each may be NULL, not both.  A NULL input or both outputs NULL with n > 0 is
 * -EINVAL before anything is written; n == 0 writes nothing and returns 0. */
int blsgpu_g1_mul_gen_secret(blsgpu_ctx *ctx, const uint8_t *scalars, size_t n, uint8_t *out_aff, uint8_t *out_ser);
/* The same with every buffer in device memory, enqueued on `stream` (no synchronisation). */
int blsgpu_g1_mul_gen_secret_dev(blsgpu_ctx *ctx, const void *d_scalars, size_t n, void *d_out_aff, void *d_out_ser,
                                 void *stream);

/* HD child derivation of n siblings of one parent (keys.py:167-316 of the reference): for every index i,
 * i_left = hmac256(ser || be32(i) || 0, chain_code), i_right = hmac256(ser || be32(i) || 1, chain_code) (util.hmac256;
 * ser = PublicKey.serialize() of parent_pk_aff, or for an index >= 2^31 in private mode the 32 bytes of parent_sk); the
 * child's chain code is i_right, and
 *   public mode (parent_sk NULL; ExtendedPublicKey.public_child, keys.py:276-296): child key (i_left mod n) G1 + parent key;
 *   private mode (ExtendedPrivateKey.private_child, keys.py:191-215): child sk = (i_left + parent_sk) mod n into out_sk,
 *   child key sk G1.
 * Both HMACs run on the device (midstates of the key blocks computed once per call), the keys on blsgpu_g1_mul_gen's table.
 * parent_pk_aff: 96 bytes affine (in private mode the parent sk's public key); parent_sk: 32 bytes big-endian or NULL.
 * out_chain: n x 32 bytes; out_sk: n x 32 bytes (private mode; ignored in public mode); out_pk_aff (n x 96 bytes) and
 * out_pk_ser (n x 48 bytes) as in blsgpu_g1_mul_gen, either may be NULL.  In public mode an index >= 2^31 fails the whole
 * call with -EINVAL ("Cannot derive hardened children from public key") before anything is written.  Not constant-time. */
int blsgpu_hd_children(blsgpu_ctx *ctx, const uint8_t chain_code[32], const uint8_t parent_pk_aff[BLSGPU_G1_BYTES],
                       const uint8_t *parent_sk, const uint32_t *indices, size_t n, uint8_t *out_chain, uint8_t *out_sk,
                       uint8_t *out_pk_aff, uint8_t *out_pk_ser);
/* The same with the indices and outputs in device memory, enqueued on `stream`; chain_code, parent_pk_aff and parent_sk
 * are host buffers.  Public mode first scans the indices on the device and synchronises the stream once to read the
 * result of that check. */
int blsgpu_hd_children_dev(blsgpu_ctx *ctx, const uint8_t chain_code[32], const uint8_t parent_pk_aff[BLSGPU_G1_BYTES],
                           const uint8_t *parent_sk, const void *d_indices, size_t n, void *d_out_chain, void *d_out_sk,
                           void *d_out_pk_aff, void *d_out_pk_ser, void *stream);

/* HD derivation of n PATHS at once, every path from a parent of its own: path p starts at record parent_of[p] of
 * `parents` and folds the reference's step -- ExtendedPrivateKey.private_child (keys.py:191-215; priv != 0) or
 * ExtendedPublicKey.public_child (keys.py:276-296; priv == 0) -- over indices[p * depth .. (p + 1) * depth).  Every level
 * runs on the device with the path's current chain code as HMAC key (its two key-block midstates per path and level,
 * util.hmac256, util.py:19-33), the current serialised public key (or, for an index >= 2^31 in private mode, the current
 * private key) as message and blsgpu_g1_mul_gen's table for the key; nothing returns to the host between levels.  The
 * outputs are those of `depth` chained blsgpu_hd_children calls, byte for byte.
 * parents: n_parents records of BLSGPU_HD_PARENT_BYTES: chain code (32), public key affine (96; in private mode the
 * private key's public key), private key (32, big-endian; ignored when priv == 0).  parent_of: n uint32, or NULL: every
 * path starts at record 0.  indices: n x depth uint32, path-major; depth: 1 .. 255, the same for every path of a call.
 * Outputs, of the LEAF of each path: out_chain n x 32; out_sk n x 32 (required when priv, ignored otherwise); out_pk_aff
 * n x 96 and out_pk_ser n x 48 as in blsgpu_hd_children (either may be NULL, not both); out_parent_fp (may be NULL) n x 4:
 * the first four bytes of sha256(PublicKey.serialize()) of the key one level above the leaf -- the parent_fingerprint the
 * reference stores in the child (PublicKey.get_fingerprint, keys.py:47-49); for depth == 1 that of the input parent.
 * -EINVAL before anything is written: depth == 0 or > 255, n_parents == 0 with n > 0, a NULL required buffer, a parent_of
 * entry >= n_parents, and in public mode an index >= 2^31 at any level ("Cannot derive hardened children from public
 * key").  n == 0 writes nothing.  Not constant-time (private keys: blsgpu_hd_paths_secret below). */
#define BLSGPU_HD_PARENT_BYTES 160
int blsgpu_hd_paths(blsgpu_ctx *ctx, const uint8_t *parents, size_t n_parents, int priv, const uint32_t *parent_of,
                    const uint32_t *indices, size_t depth, size_t n, uint8_t *out_chain, uint8_t *out_sk, uint8_t *out_pk_aff,
                    uint8_t *out_pk_ser, uint8_t *out_parent_fp);
/* The same with every buffer in device memory, enqueued on `stream`.  With parent_of, and in public mode, the call first
 * scans parent_of and the indices on the device and synchronises the stream once to read the result of that check; the
 * levels then run without another synchronisation. */
int blsgpu_hd_paths_dev(blsgpu_ctx *ctx, const void *d_parents, size_t n_parents, int priv, const void *d_parent_of,
                        const void *d_indices, size_t depth, size_t n, void *d_out_chain, void *d_out_sk, void *d_out_pk_aff,
                        void *d_out_pk_ser, void *d_out_parent_fp, void *stream);
/* blsgpu_hd_paths in private mode for SECRET keys: the same arguments without `priv`, the same validation and the same
 * outputs, byte for byte.  Every level's child key comes from k_fix_mul_secret (blsgpu_g1_mul_gen_secret above), and
 * i_left mod n and (i_left + sk) mod n keep their subtraction by a mask instead of a branch on the borrow.  The claim and
 * its limits are those of blsgpu_g1_mul_gen_secret: the sequence of instructions and of memory addresses does not depend on
 * the keys (it does depend on the indices, which are public: a hardened index takes the private key as HMAC message);
 * timing inside the hardware is not claimed.  One parent with depth 1 is the secret form of blsgpu_hd_children. */
int blsgpu_hd_paths_secret(blsgpu_ctx *ctx, const uint8_t *parents, size_t n_parents, const uint32_t *parent_of,
                           const uint32_t *indices, size_t depth, size_t n, uint8_t *out_chain, uint8_t *out_sk,
                           uint8_t *out_pk_aff, uint8_t *out_pk_ser, uint8_t *out_parent_fp);
int blsgpu_hd_paths_secret_dev(blsgpu_ctx *ctx, const void *d_parents, size_t n_parents, const void *d_parent_of,
                               const void *d_indices, size_t depth, size_t n, void *d_out_chain, void *d_out_sk,
                               void *d_out_pk_aff, void *d_out_pk_ser, void *d_out_parent_fp, void *stream);

/* Keys from seeds, n at once, one seed per lane (csrc/blsgpu_seeds.hip k_seed_keys): the first step of a key's life on the
 * device, so that seeds -> masters -> leaves never visits the host.
 *   hd == 0  PrivateKey.from_seed (keys.py:89-92 of the reference): sk = hmac256(seed, "BLS private key seed") mod n;
 *            out_chain and out_parents must be NULL.
 *   hd == 1  ExtendedPrivateKey.from_seed (keys.py:180-189): sk = hmac256(seed || 0x00, "BLS HD seed") mod n, chain code =
 *            hmac256(seed || 0x01, "BLS HD seed"); the blocks that hold seed bytes alone are hashed once for both.
 * seeds: n x seed_len bytes, 0 <= seed_len <= BLSGPU_SEED_MAX_BYTES, one length per call (seed_len == 0: seeds may be NULL;
 * the reference accepts b"").  The midstates of the two fixed keys are public constants computed once on the host.
 * Outputs, any of them NULL but not all: out_sk n x 32 bytes big-endian, canonical (below n); out_chain n x 32; out_pk_aff
 * n x 96 and out_pk_ser n x 48 as blsgpu_g1_mul_gen_secret writes them, from k_fix_mul_secret reading the keys where
 * k_seed_keys left them (no multiplication is launched when none of out_pk_aff, out_pk_ser, out_parents is asked for);
 * out_parents n records of BLSGPU_HD_PARENT_BYTES (chain code, public key affine, private key), exactly what
 * blsgpu_hd_paths_secret reads as `parents`.  Keys and affine public keys that the caller does not ask for but a later
 * step needs lie in the workspace (counted in BLSGPU_WS_TOTAL).
 * The claim and its limits are those of blsgpu_g1_mul_gen_secret: the sequence of instructions and of memory addresses does
 * not depend on the seeds, digests or keys (i_left mod n keeps its subtractions by a mask).  It does depend on seed_len, n,
 * hd and which outputs are asked for; timing inside the hardware is not claimed.
 * -EINVAL before anything is written: seed_len above the limit; hd not 0 or 1; out_chain or out_parents given with hd == 0;
 * and with n > 0: seeds NULL with seed_len > 0, all outputs NULL.  n == 0 writes nothing and returns 0. */
#define BLSGPU_SEED_MAX_BYTES 1024
int blsgpu_keys_from_seeds(blsgpu_ctx *ctx, const uint8_t *seeds, size_t seed_len, size_t n, int hd, uint8_t *out_sk,
                           uint8_t *out_chain, uint8_t *out_pk_aff, uint8_t *out_pk_ser, uint8_t *out_parents);
/* The same with every buffer in device memory, enqueued on `stream` (no synchronisation). */
int blsgpu_keys_from_seeds_dev(blsgpu_ctx *ctx, const void *d_seeds, size_t seed_len, size_t n, int hd, void *d_out_sk,
                               void *d_out_chain, void *d_out_pk_aff, void *d_out_pk_ser, void *d_out_parents, void *stream);

/* Feldman share check (Threshold.verify_secret_fragment, threshold.py:104-125 of the reference) for n fragments at once.
 * commit: n_polys x t affine G1 points (96 B, (0,0) = infinity; caller guarantees on-curve);
 * poly: n uint32 polynomial indices; x, s: n x 32 B big-endian (any value < 2^256, reduced mod n on the device).
 * status[i] = 1 if (s_i mod n)G1 == sum_k x_i^k C[poly_i][k], 0 if not, 2 if poly_i has a commitment C_k (k >= 1)
 * outside the order-n subgroup (not decided on the device).  out_aff (NULL or n x 96 B): the Horner value.
 * s/status may be NULL together (evaluation only); out_aff and status not both NULL. t == 0 or a poly index >= n_polys:
 * -EINVAL before anything is written. n == 0 writes nothing.
 * The commitments are prepared once per call (csrc/blsgpu_g1poly.hip): L28 form, and a check [n] C_k == O per commitment;
 * then one fragment per lane: Horner in the exponent over the bits of x_i mod n, (s_i mod n) G1 on blsgpu_g1_mul_gen's
 * table, a projective comparison.  Sort the fragments by polynomial: a wavefront then reads one polynomial.  The loops
 * follow the bits of the (public) x_i and the table gathers the digits of s_i: NOT constant-time.  A player checking the
 * fragments it was dealt uses blsgpu_g1_poly_check_secret below; the dealer's side is blsgpu_threshold_deal_secret. */
int blsgpu_g1_poly_check(blsgpu_ctx *ctx, const uint8_t *commit, size_t n_polys, size_t t, const uint32_t *poly,
                         const uint8_t *x, const uint8_t *s, size_t n, uint8_t *status, uint8_t *out_aff);
/* The same with every buffer in device memory, enqueued on `stream`.  The indices are first scanned on the device and the
 * stream is synchronised once to read the result of that check. */
int blsgpu_g1_poly_check_dev(blsgpu_ctx *ctx, const void *d_commit, size_t n_polys, size_t t, const void *d_poly,
                             const void *d_x, const void *d_s, size_t n, void *d_status, void *d_out_aff, void *stream);

/* Subgroup membership for n affine points at once: pts is n x 96 B (G1: x || y) or n x 192 B (G2: x.c0 x.c1 y.c0 y.c1),
 * big-endian, all zero = infinity.  status[i] = 1 if point i is on the curve and in the order-n subgroup (infinity
 * included), 2 if it is on the curve but outside the subgroup, 0 if it is off the curve.  n == 0 writes nothing and
 * returns 0; NULL pts or status with n > 0: -EINVAL before anything is written.
 * One point per lane (csrc/blsgpu_subgroup.hip): G1 tests phi(P) == -[u^2] P (127 doublings, 16 additions), G2 tests
 * psi(Q) == [u] Q (63 doublings, 5 additions on the twist); projective comparison, no inversion.  The work follows the
 * public bits of u only. */
int blsgpu_g1_subgroup_check(blsgpu_ctx *ctx, const uint8_t *pts, size_t n, uint8_t *status);
int blsgpu_g2_subgroup_check(blsgpu_ctx *ctx, const uint8_t *pts, size_t n, uint8_t *status);
/* The same with both buffers in device memory, enqueued on `stream` (no synchronisation). */
int blsgpu_g1_subgroup_check_dev(blsgpu_ctx *ctx, const void *d_pts, size_t n, void *d_status, void *stream);
int blsgpu_g2_subgroup_check_dev(blsgpu_ctx *ctx, const void *d_pts, size_t n, void *d_status, void *stream);

/* Threshold recovery for `groups` signer sets of k players at once (csrc/blsgpu_lagrange.hip on the scalar-field
 * arithmetic of csrc/fr_scalar.h): one k per call, 1 <= k <= BLSGPU_LAGRANGE_MAX_K -- a group is one workgroup, one
 * evaluation point per lane, so a larger k is refused with -EINVAL and left to the caller's host loop.
 * x: groups x k evaluation points, 32 bytes big-endian each.
 * Lagrange coefficients at zero (Threshold.lagrange_coeffs_at_zero, threshold.py:56-88 of the reference: the second
 * barycentric form, w_j = prod_{i != j} (x_j - x_i), shift_j = w_j^-1 (-x_j)^-1, L_j = shift_j / sum_i shift_i):
 * out_coeffs: groups x k x 32 bytes big-endian, the canonical integers below n the reference computes -- the layout the
 * multi-scalar sums take as `scalars`.  status[g] = 1 if group g's coefficients were written; 0 if some x_j is 0 or not
 * below n, or two of them are equal (where the reference asserts, threshold.py:66): its coefficients are all zero.
 * groups == 0 writes nothing and returns 0; k == 0, k above the limit or a NULL buffer with groups > 0: -EINVAL before
 * anything is written.  The points are public: the work does not depend on them except through the status. */
#define BLSGPU_LAGRANGE_MAX_K 1024
int blsgpu_lagrange_at_zero(blsgpu_ctx *ctx, const uint8_t *x, size_t k, size_t groups, uint8_t *out_coeffs,
                            uint8_t *status);
/* The same with every buffer in device memory, enqueued on `stream` (no synchronisation). */
int blsgpu_lagrange_at_zero_dev(blsgpu_ctx *ctx, const void *d_x, size_t k, size_t groups, void *d_out_coeffs,
                                void *d_status, void *stream);
/* Threshold.interpolate_at_zero (threshold.py:91-101): out[g] = sum_j L_j y_j mod n, 32 bytes big-endian per group, with
 * the coefficients of group g computed as above into the context's workspace; y: groups x k x 32 bytes big-endian, any
 * value below 2^256 (reduced mod n on the device).  A group with status 0 yields 0.  The y_j are secrets (shares): the
 * reductions branch on their values, NOT constant-time; blsgpu_fr_interpolate_at_zero_secret below is the form for shares. */
int blsgpu_fr_interpolate_at_zero(blsgpu_ctx *ctx, const uint8_t *x, const uint8_t *y, size_t k, size_t groups,
                                  uint8_t *out, uint8_t *status);
int blsgpu_fr_interpolate_at_zero_dev(blsgpu_ctx *ctx, const void *d_x, const void *d_y, size_t k, size_t groups,
                                      void *d_out, void *d_status, void *stream);
/* Threshold.aggregate_unit_sigs (threshold.py:127-136) per group: out[g] = sum_j L_j sigs[g*k+j], the coefficients
 * computed into the workspace and handed to the G2 multi-scalar sum on the device -- the internal path of the G2 sum with
 * device scalars, no host round trip.  sigs_affine: groups x k x 192 bytes as the G2 sums take them; out: groups x 192
 * bytes; out_inf (may be NULL): 1 for the point at infinity.  A group with status 0 yields the all-zero point with
 * out_inf = 1. */
int blsgpu_threshold_combine(blsgpu_ctx *ctx, const uint8_t *sigs_affine, const uint8_t *x, size_t k, size_t groups,
                             uint8_t *out, uint8_t *out_inf, uint8_t *status);
int blsgpu_threshold_combine_dev(blsgpu_ctx *ctx, const void *d_sigs_affine, const void *d_x, size_t k, size_t groups,
                                 void *d_out, void *d_out_inf, void *d_status, void *stream);

/* Signature shares of `groups` threshold sessions of k shares each, checked on the device, and the wrong ones named
 * (csrc/blsgpu_sigshares.hip; one k per call, 1 <= k <= BLSGPU_LAGRANGE_MAX_K).  Share i of a session with message hash h is
 * VALID iff
 *   scaled = 1:  e(G1, sig_i) = e(lambda_i PK_i, H(h))  -- a unit signature of PrivateKey.sign_threshold (keys.py:134-141 of the
 *                reference), lambda the Lagrange coefficients at zero of the session's players x;
 *   scaled = 0:  e(G1, sig_i) = e(PK_i, H(h))           -- a plain share, secret_share.sign(m), as Threshold.aggregate_unit_sigs
 *                (threshold.py:127-136) combines them;
 * PK_i = sk_i G1 the player's share public key, H = hash_to_point_prehashed_Fq2 (ec.py:528-550).
 * sigs: groups x k x 192 bytes affine G2, (0,0) = infinity.  keys: n_keys x 96 bytes affine G1; key_idx: groups x k uint32 into
 * keys (as `poly` of blsgpu_g1_poly_check).  x: groups x k x 32 bytes big-endian player numbers, required when scaled, ignored
 * (may be NULL) otherwise.  msg_hashes: groups x 32 bytes.  weights: groups x k x 8 bytes big-endian, the random 64-bit
 * multipliers of the check, drawn by the CALLER (as BLS.verify_batch_randomized draws them: unpredictable to whoever made the
 * shares); a ZERO weight is taken as 1 on the device.
 * status: groups x k bytes -- 1 valid; 0 invalid, which includes a share off the twist, outside the order-n subgroup or at
 * infinity (whatever its key); 2 not decided: the share's key is off the curve or outside G1.  session_status: groups bytes --
 * 0 where blsgpu_lagrange_at_zero refuses the player set (a zero, a value >= n, a repeated x): all of that session's shares
 * are then 0; 1 otherwise, and always 1 when not scaled.  stats (HOST memory in both forms, may be NULL): [0] the rounds run,
 * summed over the slices of the call, [1] the node tests (two-pair pairings) performed.
 * Once per call: the subgroup checks of keys and shares, H(h), the coefficients, k_share_weights (w_i = r_i lambda_i mod n,
 * or r_i), and the leaves A_i = r_i sig_i, B_i = w_i PK_i from the G2 / G1 sums with device scalars.  Then rounds over NODES
 * (session, offset, length): round 0 tests every session whole; a node's leaves are gathered, summed by the plain G2 / G1
 * group sums to S and P, and e(-G1, S) e(P, H(h)) = 1 is tested by blsgpu_pairing_multi_batch_dev (two pairs per node).  A sum
 * at infinity is never fed to the pairing: with H(h) != O a node whose two sums are both at infinity passes and one with
 * exactly one at infinity fails (every point is in its prime-order subgroup); with H(h) = O it passes iff S = O.  The host
 * reads ONE byte per node and round, halves the nodes that failed and stops at the leaves: at most log2 K + 1 rounds (K: k
 * rounded up to a power of two), one stream synchronisation each -- the calls are NOT asynchronous.  Sessions are processed in
 * slices that keep the leaves, and the largest round, below 2 GB each (counted in BLSGPU_WS_TOTAL).
 * What is claimed: a failing leaf test is exact (0 < r_i < 2^64 is not 0 mod n); a node that passes although it holds an
 * invalid eligible share does so with probability at most 2^-64 over the weights, per node.  Nothing stronger.
 * -EINVAL before anything is written: k == 0 or above the limit (also with groups == 0), n_keys == 0, a key_idx >= n_keys, a
 * NULL required buffer.  groups == 0 writes nothing and returns 0.  All of this is PUBLIC data: not constant-time. */
int blsgpu_sig_shares_check(blsgpu_ctx *ctx, const uint8_t *sigs, const uint8_t *keys, size_t n_keys, const uint32_t *key_idx,
                            const uint8_t *x, const uint8_t *msg_hashes, const uint8_t *weights, int scaled, size_t k,
                            size_t groups, uint8_t *status, uint8_t *session_status, uint64_t *stats);
/* The same with every buffer but stats in device memory (16-byte aligned where it holds points, 4-byte otherwise), on
 * `stream`.  The key indices are first scanned on the device and the stream is synchronised once to read the result of that
 * check; then once per round. */
int blsgpu_sig_shares_check_dev(blsgpu_ctx *ctx, const void *d_sigs, const void *d_keys, size_t n_keys, const void *d_key_idx,
                                const void *d_x, const void *d_msg_hashes, const void *d_weights, int scaled, size_t k,
                                size_t groups, void *d_status, void *d_session_status, uint64_t *stats, void *stream);

/* Multiplication by SHORT PUBLIC scalars:  out_i = w_i P_i  for 64-bit weights (csrc/blsgpu_smul64.hip k_smul64;
 * vmgen/smul64_model.py is its specification).  pts: n x 96 (G1) / n x 192 (G2) bytes affine, (0,0) = infinity; w: n x 8 bytes
 * big-endian; out_aff: n points likewise, (0,0) for infinity; out_inf (may be NULL): n flags, 1 for infinity.  w = 0 gives
 * infinity.  One point per lane (G1) or lane pair (G2), 4-bit windows from the top: 16 windows -- 60 doublings and 16
 * additions against the 252 and 64 that blsgpu_g1_msm / blsgpu_g2_msm(k = 1, groups = n) spend on the same weight zero-extended
 * to 32 bytes, whose result bytes this call reproduces byte for byte for every input those calls accept.  The weights are
 * PUBLIC data: the schedule reads a table entry the digit chooses and is NOT scalar-independent (secret scalars:
 * blsgpu_g2_mul_secret, blsgpu_g1_mul_gen_secret).  A launch takes 131 072 G1 / 65 536 G2 points, which bounds the table
 * workspace at 352 MB (counted in BLSGPU_WS_TOTAL).  n == 0 writes nothing and returns 0; a NULL required buffer is -EINVAL
 * before anything is written. */
int blsgpu_g1_mul_short(blsgpu_ctx *ctx, const uint8_t *pts, const uint8_t *w, size_t n, uint8_t *out_aff, uint8_t *out_inf);
int blsgpu_g2_mul_short(blsgpu_ctx *ctx, const uint8_t *pts, const uint8_t *w, size_t n, uint8_t *out_aff, uint8_t *out_inf);
/* The same with every buffer in device memory (points 16-byte aligned), enqueued on `stream` (no synchronisation). */
int blsgpu_g1_mul_short_dev(blsgpu_ctx *ctx, const void *d_pts, const void *d_w, size_t n, void *d_out_aff, void *d_out_inf,
                            void *stream);
int blsgpu_g2_mul_short_dev(blsgpu_ctx *ctx, const void *d_pts, const void *d_w, size_t n, void *d_out_aff, void *d_out_inf,
                            void *stream);

/* Batch verification that NAMES the forgeries (csrc/blsgpu_batchfind.hip): n signatures with their own keys and messages,
 * all of them checked by one random linear combination and only what fails bisected.  Item i is (sig_i,
 * P_i = keys[key_idx[i]], h_i = msg_hashes[msg_idx[i]]); it is VALID iff e(G1, sig_i) = e(P_i, H(h_i)),
 * H = hash_to_point_prehashed_Fq2 (ec.py:528-550 of the reference).
 * sigs: n x 192 bytes affine G2, (0,0) = infinity.  keys: n_keys x 96 bytes affine G1; key_idx: n uint32 into keys.
 * msg_hashes: n_msgs x 32 bytes; msg_idx: n uint32 into them -- a hash is mapped to G2 ONCE however many items name it.
 * weights: n x 8 bytes big-endian, the random 64-bit multipliers r_i, drawn by the CALLER (unpredictable to whoever made the
 * signatures); a ZERO weight is taken as 1 on the device.
 * status: n bytes -- 1 valid; 0 invalid, which includes a signature off the twist, outside G2 or at infinity (whatever its
 * key); 2 not decided: the key is off the curve, outside G1 or at infinity, or H(h) is at infinity.  stats (HOST memory in
 * both forms, may be NULL): [0] the rounds run, summed over the slices of the call, [1] the node tests, [2] the pairs fed to
 * the pairing by those tests.
 * Once per call: k_g1_subgroup over the key table, k_g2_subgroup over the signatures, H of the n_msgs hashes, k_find_settle
 * (the items that cannot enter a sum get their status; the others are ELIGIBLE), the dense order of the n_e eligible items
 * (input order kept; the host reads n_e: one synchronisation), and the leaves A_i = r_i sig_i, B_i = r_i P_i from k_smul64.
 * Then rounds over aligned NODES (offset, length L) of the dense order, L from K = 2^ceil(log2 n_e) halving: a node's test is
 * e(-G1, S) prod_(i in node) e(B_i, H(h_i)) = 1 with S = sum A_i from the plain G2 group sum; the full nodes of a round go
 * through one blsgpu_pairing_multi_batch_dev of L + 1 pairs each, the one node that crosses n_e through a call of its own size
 * (no flagged pair pads it), a node wholly past n_e is not tested.  A sum at infinity is never fed to the pairing: a node with
 * S = O carries (-G1, G2) in that place and its result is compared with e(-G1, G2) (computed by the pairing once per context),
 * so it is decided by prod e(B_i, H(h_i)) = 1 alone; B_i and H(h_i) of an eligible item are never at infinity, nor is a leaf's
 * S.  The host reads ONE byte per node and round, halves the nodes that failed -- both halves are tested -- and in the round
 * L = 1 the verdict is the item's status: at most log2 K + 1 rounds, one stream synchronisation each; the calls are NOT
 * asynchronous.  One forgery costs at most 1 + 2 log2 K node tests.  Items are processed in slices that keep the leaves, and
 * the largest round, below 2 GB each (counted in BLSGPU_WS_TOTAL).
 * What is claimed: a failing leaf test is exact (0 < r_i < 2^64 is not 0 mod n); a node that passes although it holds an
 * invalid eligible item does so with probability at most 2^-64 over the weights, per node.  Nothing stronger.
 * -EINVAL before anything is written: a NULL required buffer, n_keys == 0 or n_msgs == 0 with n > 0, a key_idx >= n_keys or a
 * msg_idx >= n_msgs.  n == 0 writes nothing and returns 0.  All of this is PUBLIC data: not constant-time. */
int blsgpu_verify_find(blsgpu_ctx *ctx, const uint8_t *sigs, const uint8_t *keys, size_t n_keys, const uint32_t *key_idx,
                       const uint8_t *msg_hashes, size_t n_msgs, const uint32_t *msg_idx, const uint8_t *weights, size_t n,
                       uint8_t *status, uint64_t *stats);
/* The same with every buffer but stats in device memory (16-byte aligned where it holds points, 4-byte otherwise), on
 * `stream`.  The indices are first scanned on the device and the stream is synchronised once to read the result of that
 * check; then once for n_e and once per round. */
int blsgpu_verify_find_dev(blsgpu_ctx *ctx, const void *d_sigs, const void *d_keys, size_t n_keys, const void *d_key_idx,
                           const void *d_msg_hashes, size_t n_msgs, const void *d_msg_idx, const void *d_weights, size_t n,
                           void *d_status, uint64_t *stats, void *stream);

/* Sums over RANGES of a list of points (csrc/blsgpu_pscan.hip; vmgen/pscan_model.py is its specification):
 * out_j = sum of pts[begin_j .. end_j) for m ranges of ANY lengths over n points, from prefix sums S[i] = sum_{k<i} pts[k] kept
 * as projective records on the device: three passes of about 2 n mixed additions, then ONE complete addition
 * S[end] + (-S[begin]) and one inversion per range.
 * pts: n x 96 (G1) / n x 192 (G2) bytes affine, (0,0) = infinity.  ranges: m x 2 uint32 (begin, end), begin <= end <= n; ranges
 * may overlap, repeat or be empty.  out_aff: m points likewise, (0,0) for infinity.  out_flag: m bytes -- 0 a finite sum, 1
 * infinity (an empty range gives infinity), 2 the range holds a point that is neither (0,0) nor on the curve: its output is
 * (0,0).  Such a point is counted and enters every sum as infinity, so the ranges that do not hold it are not disturbed.
 * A coordinate that is not below q is taken mod q, as blsgpu_g1_msm / blsgpu_g2_msm take it: x + q is accepted as x.
 * The arithmetic is the complete formulas of Renes-Costello-Batina; both curves have odd order, so the formulas hold for every
 * point of either curve and the points are NOT checked for (and need not lie in) the prime-order subgroups.  Equal-length
 * ranges [j k, (j + 1) k) give the bytes of blsgpu_g1_msm / blsgpu_g2_msm(scalars = NULL, k, groups).
 * More points than keep the prefix records below 2 GB (12.7 M in G1, 6.3 M in G2) are processed in slices; the carry goes into
 * the next slice and a range is finished in the slice that holds its end.  The workspace counts in BLSGPU_WS_TOTAL.
 * -EINVAL before anything is written: a NULL required buffer (pts with n > 0; ranges, out_aff, out_flag with m > 0), a range
 * with begin > end or end > n.  m == 0 writes nothing and returns 0; n == 0 with every range empty writes m times (0,0) and
 * flag 1.  All of this is PUBLIC data: not constant-time. */
int blsgpu_g1_range_sums(blsgpu_ctx *ctx, const uint8_t *pts, size_t n, const uint32_t *ranges, size_t m, uint8_t *out_aff,
                         uint8_t *out_flag);
int blsgpu_g2_range_sums(blsgpu_ctx *ctx, const uint8_t *pts, size_t n, const uint32_t *ranges, size_t m, uint8_t *out_aff,
                         uint8_t *out_flag);
/* The same with every buffer in device memory (points 16-byte aligned, ranges 4-byte), on `stream`.  The ranges are first
 * scanned on the device and the stream is synchronised once to read the result of that check; the rest is enqueued. */
int blsgpu_g1_range_sums_dev(blsgpu_ctx *ctx, const void *d_pts, size_t n, const void *d_ranges, size_t m, void *d_out_aff,
                             void *d_out_flag, void *stream);
int blsgpu_g2_range_sums_dev(blsgpu_ctx *ctx, const void *d_pts, size_t n, const void *d_ranges, size_t m, void *d_out_aff,
                             void *d_out_flag, void *stream);

/* RAGGED multi-scalar sums (csrc/blsgpu_msmr.hip; vmgen/msmr_model.py is its specification):
 * out_j = sum_{i in [begin_j, end_j)} scalars[i] * pts[i] for m ranges of ANY lengths over n points, in one call and with
 * nothing padded.  Every range is cut into chunks of at most 8 consecutive points; one chunk runs on one lane (G1) or lane pair
 * (G2) on the fixed 4-bit windows of blsgpu_g1_msm's small-group kernel -- 252 doublings per chunk, 14 mixed and 64 complete
 * additions per point --, and the chunks' partial sums are summed per range by the passes of blsgpu_g?_range_sums.
 * pts: n x 96 (G1) / n x 192 (G2) bytes affine, (0,0) = infinity.  scalars: n x 32 bytes big-endian, taken as the 256-bit
 * integers they are (not reduced).  ranges: m x 2 uint32 (begin, end), begin <= end <= n; ranges may overlap, repeat or be empty,
 * and each pays for its own chunks.  out_aff: m points, (0,0) for infinity.  out_flag: m bytes -- 0 a finite sum, 1 infinity
 * (an empty range, a range of (0,0) points, zero scalars, terms that cancel), 2 the range holds a point that is neither (0,0)
 * nor on the curve: its output is (0,0).  Such a point enters every sum as infinity, so the ranges that do not hold it are not
 * disturbed.  The points are not checked for the prime-order subgroups (both curves have odd order: the complete formulas
 * hold for every point of either curve).
 * Equal-length ranges [j k, (j + 1) k) over on-curve points give the bytes of blsgpu_g1_msm / blsgpu_g2_msm(scalars, k, groups),
 * and out_inf == (flag == 1).
 * Both forms check the ranges and count the chunks on the device and synchronise ONCE to read the result, before anything is
 * written to the outputs; the rest is enqueued.  The chunks are processed in slices whose tables stay below 2 GB (at most 99 840
 * chunks in G1, 49 920 in G2, a launch); the workspace counts in BLSGPU_WS_TOTAL.
 * -EINVAL before anything is written: a NULL required buffer (pts or scalars with n > 0; ranges, out_aff or out_flag with
 * m > 0; scalars == NULL is an error here: plain sums are blsgpu_g?_range_sums' business), a range with begin > end or end > n,
 * 2^31 chunks or more in all.  m == 0 writes nothing and returns 0; n == 0 with every range empty writes m times (0,0) and
 * flag 1.  All of this is PUBLIC data: not constant-time. */
int blsgpu_g1_msm_ranges(blsgpu_ctx *ctx, const uint8_t *pts, const uint8_t *scalars, size_t n, const uint32_t *ranges, size_t m,
                         uint8_t *out_aff, uint8_t *out_flag);
int blsgpu_g2_msm_ranges(blsgpu_ctx *ctx, const uint8_t *pts, const uint8_t *scalars, size_t n, const uint32_t *ranges, size_t m,
                         uint8_t *out_aff, uint8_t *out_flag);
/* The same with every buffer in device memory (points 16-byte aligned, scalars and ranges 4-byte), on `stream`; the one
 * synchronisation is of that stream. */
int blsgpu_g1_msm_ranges_dev(blsgpu_ctx *ctx, const void *d_pts, const void *d_scalars, size_t n, const void *d_ranges, size_t m,
                             void *d_out_aff, void *d_out_flag, void *stream);
int blsgpu_g2_msm_ranges_dev(blsgpu_ctx *ctx, const void *d_pts, const void *d_scalars, size_t n, const void *d_ranges, size_t m,
                             void *d_out_aff, void *d_out_flag, void *stream);

/* Batched Signature.divide_by (signature.py:44-103 of the reference; csrc/sigdiv.h, csrc/blsgpu_sigdiv.hip): m dividends, each
 * with any number of divisors, in one call.  The caller has done the dictionary work: for every entry (message hash, public
 * key) of every divisor's aggregation tree it hands in the dividend's exponent a and the divisor's exponent b of that entry.
 *   out_aff[j] = pts[first of j] + sum over j's divisors d of (-q_d) pts[d],   q_d = a_0 / b_0 mod n from d's FIRST entry,
 * and every further entry e of d is held against it by a_e b_0 == a_0 b_e (mod n): with every b non-zero that is the
 * reference's `quotient != new_quotient`.  One inversion mod n per divisor, two products per entry.
 * pts: n_pts x 192 bytes affine G2, (0,0) = infinity.  pt_off: m + 1 uint32, dividend j owns the points [pt_off[j], pt_off[j+1]):
 * the first is its own signature, the others its divisors.  ent_off: n_pts + 1 uint32, point p owns the entries [ent_off[p],
 * ent_off[p+1]): none for a dividend's own point, at least one for a divisor.  ent_dividend / ent_divisor: n_ent x 32 bytes
 * big-endian each, any value below 2^256, taken mod n.
 * out_aff: m points, (0,0) for infinity.  out_flag: m bytes -- 0 finite, 1 infinity, 2 the range holds a point that is neither
 * (0,0) nor on the twist (as blsgpu_g2_msm_ranges reports it), 3 a divisor of j has status 1 or 2: the output is (0,0).
 * out_status: n_pts bytes -- 0 fine (always for a dividend's own point), 1 the pairs of this divisor are not unique (an entry
 * fails the test above), 2 an exponent b of this divisor is 0 mod n: not decided here (the reference divides by zero its own
 * way; the caller's host loop decides it).  out_scalars (may be NULL): n_pts x 32 bytes big-endian, the scalar of every point
 * in the layout blsgpu_g2_msm_ranges takes -- 1 for a dividend's own point, (n - q_d) mod n for a divisor, 0 for a refused one.
 * stats (may be NULL; host memory in BOTH forms): [0] 0 the plain path ran, 1 the scalar path; [1] the divisors with q != 1.
 * The plain path: when every accepted quotient of the call is 1 -- aggregates that were never merged securely, the common
 * case -- the sums are blsgpu_g2_range_sums over a working copy of the points in which every divisor is replaced by its
 * negative; no scalar multiplication runs.  Otherwise the sums are blsgpu_g2_msm_ranges over the points as given with the
 * scalars above.  Both give the same bytes; BLSGPU_SIGDIV_PLAIN=0 at context creation sends every call down the scalar path.
 * Both forms check the offsets on the device and synchronise ONCE, reading that check and the number of non-unit quotients
 * together, before anything is written to the outputs (the sums then synchronise once more for their own plan where
 * blsgpu_g2_msm_ranges does).  The workspace -- the scalars, the working copy, the statuses and the ranges -- counts in
 * BLSGPU_WS_TOTAL.
 * -EINVAL before anything is written: a NULL required buffer (everything but out_scalars and stats; ent_dividend / ent_divisor
 * with n_ent > 0), offsets that decrease, pt_off[0] != 0, pt_off[m] != n_pts, ent_off[0] != 0, ent_off[n_pts] != n_ent, an
 * empty dividend range, a dividend's own row with entries, a divisor's row with none.  m == 0 writes nothing and returns 0.
 * Signatures, trees and exponents are PUBLIC data: not constant-time. */
int blsgpu_sig_divide(blsgpu_ctx *ctx, const uint8_t *pts, size_t n_pts, const uint32_t *pt_off, size_t m, const uint32_t *ent_off,
                      const uint8_t *ent_dividend, const uint8_t *ent_divisor, size_t n_ent, uint8_t *out_aff, uint8_t *out_flag,
                      uint8_t *out_status, uint8_t *out_scalars, uint32_t stats[2]);
/* The same with every buffer but stats in device memory (points 16-byte aligned, offsets and exponents 4-byte), on `stream`. */
int blsgpu_sig_divide_dev(blsgpu_ctx *ctx, const void *d_pts, size_t n_pts, const void *d_pt_off, size_t m, const void *d_ent_off,
                          const void *d_ent_dividend, const void *d_ent_divisor, size_t n_ent, void *d_out_aff, void *d_out_flag,
                          void *d_out_status, void *d_out_scalars, uint32_t stats[2], void *stream);

/* blsgpu_verify_find with the items of one message FOLDED inside every node: arguments, status bytes and stats as there, with
 * ONE precondition -- msg_idx is non-decreasing over the items (a decrease is -EINVAL before anything is written; the _dev form
 * finds it in the device scan that checks the indices).  The dense order keeps input order, so every message is one
 * contiguous run of it, and by bilinearity a node (off, L), end = min(off + L, n_e), is tested as
 *   e(-G1, SA[end] - SA[off])  prod_r e(SB[min(end, rb[r+1])] - SB[max(off, rb[r])], H(h_r)) = 1
 * over the runs r (begins rb) that meet it: one pair per distinct message in the node plus one, where blsgpu_verify_find takes
 * one per item plus one.  SA / SB are the prefix sums of the leaves A_i = r_i sig_i (G2) / B_i = r_i P_i (G1) in the dense
 * order, scanned once per call; every sum of every round is one point subtraction (blsgpu_g?_range_sums' kernels).  A sum at
 * infinity never reaches the pairing as a point: the pairs whose sum is at infinity take (G1, G2) and (-G1, G2) in turn -- a
 * couple that cancels -- and when their number is odd the node's result is compared with e(-G1, G2) instead of one.  The
 * nodes of a round that have the SAME pair count go through one blsgpu_pairing_multi_batch_dev; nothing is padded, and
 * stats[2] counts exactly the pairs fed.  A batch without a forgery costs (messages among the eligible items) + 1 pairs.
 * Bisection, leaf verdicts, slicing, synchronisations (one for n_e and the run table, one per round) and what is claimed about
 * the 2^-64 bound are blsgpu_verify_find's. */
int blsgpu_verify_find_folded(blsgpu_ctx *ctx, const uint8_t *sigs, const uint8_t *keys, size_t n_keys, const uint32_t *key_idx,
                              const uint8_t *msg_hashes, size_t n_msgs, const uint32_t *msg_idx, const uint8_t *weights, size_t n,
                              uint8_t *status, uint64_t *stats);
int blsgpu_verify_find_folded_dev(blsgpu_ctx *ctx, const void *d_sigs, const void *d_keys, size_t n_keys, const void *d_key_idx,
                                  const void *d_msg_hashes, size_t n_msgs, const void *d_msg_idx, const void *d_weights, size_t n,
                                  void *d_status, uint64_t *stats, void *stream);

/* G2 scalar multiplication for SECRET scalars:  out_i = s_i P_(n_pts == 1 ? 0 : i)  with a schedule independent of s
 * (csrc/blsgpu_g2smul.hip k_g2_smul; vmgen/g2smul_model.py is its specification).  s_i is the literal 256-bit integer of
 * 32 big-endian bytes, NOT reduced mod the group order -- exactly the `scalars` of blsgpu_g2_msm, whose results this call
 * reproduces byte for byte.
 * The claim is exactly this: the sequence of instructions and of memory addresses does not depend on the scalars.  One
 * scalar per lane pair; signed 4-bit digits of s + C over 65 windows (plain carries); a table 1P .. 8P per scalar in the
 * workspace (built once when n_pts == 1 and read by every pair); per window four complete doublings and one complete
 * addition of an entry that is picked by reading all eight and keeping one by compare-and-select, its sign by a select
 * between y and -y, a zero digit by the constant (0 : 1 : 0) -- nothing is skipped; an input (0, 0) enters as (0 : 1 : 0)
 * by select; the affine conversion is the fixed-length branch-free safegcd inversion (37 x 30 division steps).
 * NOT claimed: data-dependent timing inside the hardware (how long an instruction or a memory access takes for given
 * values), and anything about the points -- in blsgpu_sign the message-dependent H(m), which is public.
 * pts: n_pts x 192 bytes affine (x.c0 x.c1 y.c0 y.c1, (0, 0) = infinity; on the twist, the subgroup is not required).
 * out_aff: n x 192 bytes ((0, 0) for infinity); out_ser: n x 96 bytes, Signature.serialize() (ec.py:94-111: x.c0 || x.c1
 * with 0x80 on the first byte when the imaginary part of y exceeds q // 2; 96 zero bytes for infinity) -- the compression
 * runs in the kernel; out_inf (may be NULL): n flags, 1 for infinity.  out_aff and out_ser may each be NULL, not both.
 * n_pts must be 1 or n: anything else, a NULL input or both outputs NULL is -EINVAL before anything is written.  n == 0
 * writes nothing and returns 0.  Calls are processed in slices of 65 536 scalars, which bounds the table workspace at
 * 168 MiB (counted in BLSGPU_WS_TOTAL). */
int blsgpu_g2_mul_secret(blsgpu_ctx *ctx, const uint8_t *pts, size_t n_pts, const uint8_t *scalars, size_t n,
                         uint8_t *out_aff, uint8_t *out_ser, uint8_t *out_inf);
/* The same with every buffer in device memory, enqueued on `stream` (no synchronisation). */
int blsgpu_g2_mul_secret_dev(blsgpu_ctx *ctx, const void *d_pts, size_t n_pts, const void *d_scalars, size_t n,
                             void *d_out_aff, void *d_out_ser, void *d_out_inf, void *stream);
/* Signing, the device work of PrivateKey.sign_prehashed (keys.py:128-132 of the reference):
 * sig_i = sk_i H(h_(n_msg == 1 ? 0 : i)).  sks: n x 32 bytes big-endian; msg_hashes: n_msg x 32 bytes.  The call enqueues
 * blsgpu_hash_to_g2_dev into the workspace and then k_g2_smul on those points: nothing returns to the host in between, and
 * the private keys meet only the scalar-independent schedule described above (same claim, same limits; H(m) is public).
 * n_msg == 1: every key signs the same message (a committee, a threshold session) -- one hash, one shared table.
 * out_aff / out_ser as in blsgpu_g2_mul_secret; n_msg must be 1 or n (-EINVAL before anything is written otherwise). */
int blsgpu_sign(blsgpu_ctx *ctx, const uint8_t *sks, const uint8_t *msg_hashes, size_t n_msg, size_t n, uint8_t *out_aff,
                uint8_t *out_ser);
int blsgpu_sign_dev(blsgpu_ctx *ctx, const void *d_sks, const void *d_msg_hashes, size_t n_msg, size_t n, void *d_out_aff,
                    void *d_out_ser, void *stream);

/* The threshold scheme's work on SECRET scalars (csrc/blsgpu_frsecret.hip on the masked forms of csrc/fr_scalar.h, and
 * k_poly_eval_secret of csrc/blsgpu_g1poly.hip).  The claim of the five calls below is exactly that of blsgpu_g1_mul_gen_secret
 * and blsgpu_g2_mul_secret: the sequence of instructions and of memory addresses does not depend on the coefficients,
 * fragments, shares or keys.  It does depend on t, k, the counts and the evaluation points x (player numbers), which are
 * public -- and so do the Lagrange coefficients computed from them -- and, in the share check, on the commitments, the
 * polynomial indices and the OUTCOME of the check: the status is what a player publishes as a complaint.  NOT claimed:
 * data-dependent timing inside the hardware (how long an instruction or a memory access takes for given values).
 *
 * Joint-Feldman dealing (PrivateKey.new_threshold, keys.py:92-117 of the reference) of n_polys polynomials of t coefficients
 * at once.  coeffs: n_polys x t x 32 bytes big-endian, coefficient k of polynomial p at index p * t + k, any value below
 * 2^256; x: n_x x 32 bytes big-endian, the points the fragments are taken at (1 .. N in the reference), any value below 2^256
 * (reduced mod n).  out_commit_aff: n_polys x t x 96 bytes, c_k G1 from k_fix_mul_secret (the bytes of blsgpu_g1_mul_gen);
 * out_frag: n_polys x n_x x 32 bytes big-endian canonical, P_p(x_j) = sum_k c[p][k] x_j^k mod n at index p * n_x + j, from
 * k_fr_poly_eval_secret: one lane per (p, j), the polynomial's coefficients reduced by mask, in Montgomery form in LDS, Horner
 * from the top coefficient with t - 1 masked products and additions, coefficient k read at step k by every lane.  Either
 * output may be NULL, not both; without out_frag, x and n_x are ignored.  -EINVAL before anything is written: t == 0 or
 * t > BLSGPU_LAGRANGE_MAX_K (a polynomial's coefficients fit one workgroup's LDS), a NULL required buffer, n_x == 0 with
 * out_frag given.  n_polys == 0 writes nothing and returns 0. */
int blsgpu_threshold_deal_secret(blsgpu_ctx *ctx, const uint8_t *coeffs, size_t n_polys, size_t t, const uint8_t *x, size_t n_x,
                                 uint8_t *out_commit_aff, uint8_t *out_frag);
/* The same with every buffer in device memory, enqueued on `stream` (no synchronisation). */
int blsgpu_threshold_deal_secret_dev(blsgpu_ctx *ctx, const void *d_coeffs, size_t n_polys, size_t t, const void *d_x, size_t n_x,
                                     void *d_out_commit_aff, void *d_out_frag, void *stream);
/* blsgpu_fr_interpolate_at_zero for SECRET y_j (recombining shares into a private key): the same arguments, validation and
 * bytes, status 0 groups included.  k_lagrange on the public points, then k_fr_dot_secret: y_j mod n, L_j y_j and the sum
 * over the group keep every subtraction by a mask.  The claim and its limits are stated above. */
int blsgpu_fr_interpolate_at_zero_secret(blsgpu_ctx *ctx, const uint8_t *x, const uint8_t *y, size_t k, size_t groups,
                                         uint8_t *out, uint8_t *status);
int blsgpu_fr_interpolate_at_zero_secret_dev(blsgpu_ctx *ctx, const void *d_x, const void *d_y, size_t k, size_t groups,
                                             void *d_out, void *d_status, void *stream);
/* blsgpu_g1_poly_check for SECRET fragments s_i (step 2 of Joint-Feldman: a player checks what it was dealt): the same
 * arguments, validation and layout, and for every s below 2^256 the same status and out_aff bytes.  s and status are
 * required -- NULL with n > 0 is -EINVAL before anything is written; there is no evaluation-only mode -- and out_aff may be
 * NULL.  The commitments are prepared as in blsgpu_g1_poly_check (k_poly_prep, k_poly_subgroup); then k_poly_eval_secret, one
 * fragment per lane: the left-hand side is s_i G1 for the LITERAL 256-bit s_i (no reduction mod n; G1 has order n) on the
 * schedule and the 58 KB table of blsgpu_g1_mul_gen_secret -- 65 windows, all eight entries of a window read and one kept by
 * select, one complete addition each, no inversion -- and the right-hand side and the projective comparison are those of
 * k_poly_eval over the bits of the public x_i.  The claim and its limits are stated above. */
int blsgpu_g1_poly_check_secret(blsgpu_ctx *ctx, const uint8_t *commit, size_t n_polys, size_t t, const uint32_t *poly,
                                const uint8_t *x, const uint8_t *s, size_t n, uint8_t *status, uint8_t *out_aff);
/* The same with every buffer in device memory, enqueued on `stream`; the one synchronisation of the index scan stays. */
int blsgpu_g1_poly_check_secret_dev(blsgpu_ctx *ctx, const void *d_commit, size_t n_polys, size_t t, const void *d_poly,
                                    const void *d_x, const void *d_s, size_t n, void *d_status, void *d_out_aff,
                                    void *stream);
/* A player's share (step 3 of Joint-Feldman, BLS.aggregate_priv_keys without secure aggregation) for `groups` players at
 * once: out[g] = sum_j y[g * k + j] mod n, the canonical integer below n, 32 bytes big-endian.  y: groups x k x 32 bytes
 * big-endian, any value below 2^256; k >= 1 has no upper limit.  k_fr_sum_secret: a masked reduction and a masked addition per
 * term (no Montgomery form, no product); whole groups share a workgroup of 256 lanes while k <= 256, above that a group has a
 * workgroup to itself and its lanes stride over the terms.  out (groups x 32) is required.  out_pk_aff (groups x 96) and
 * out_pk_ser (groups x 48) may each be NULL: the public key of every sum as blsgpu_g1_mul_gen_secret writes it, from
 * k_fix_mul_secret reading the sums where the first kernel left them -- nothing returns to the host in between.  -EINVAL
 * before anything is written: k == 0, or a NULL required buffer with groups > 0.  groups == 0 writes nothing and returns 0.
 * The claim and its limits are stated above. */
int blsgpu_fr_sum_secret(blsgpu_ctx *ctx, const uint8_t *y, size_t k, size_t groups, uint8_t *out, uint8_t *out_pk_aff,
                         uint8_t *out_pk_ser);
/* The same with every buffer in device memory, enqueued on `stream` (no synchronisation). */
int blsgpu_fr_sum_secret_dev(blsgpu_ctx *ctx, const void *d_y, size_t k, size_t groups, void *d_out, void *d_out_pk_aff,
                             void *d_out_pk_ser, void *stream);
/* Unit signatures of `groups` threshold sessions of k signers each (PrivateKey.sign_threshold, keys.py:134-141 of the
 * reference): out[g * k + j] = (lambda_gj sk_gj mod n) H(h_(n_msg == 1 ? 0 : g)) with lambda_g the Lagrange coefficients at
 * zero of session g's players.  sks and x: groups x k x 32 bytes big-endian (share and player number of signer j of session
 * g; sk any value below 2^256); msg_hashes: n_msg x 32 bytes, n_msg = 1 (every session signs the same message) or groups.
 * The call enqueues k_lagrange, then k_fr_scale_secret (lambda sk mod n with the masked reduction and product, into the
 * workspace), blsgpu_hash_to_g2_dev of the n_msg hashes, then k_g2_smul -- on ONE shared table when n_msg == 1, otherwise
 * session g's point is copied to its k slots and the per-scalar tables are used; nothing returns to the host between the
 * stages, and a call is processed in the slices of 65 536 scalars of blsgpu_g2_mul_secret.  1 <= k <= BLSGPU_LAGRANGE_MAX_K.
 * status: groups bytes as in blsgpu_lagrange_at_zero; a session with status 0 has all-zero coefficients, hence scalar 0 and
 * the point at infinity for each of its signers.  out_aff (groups x k x 192), out_ser (groups x k x 96), out_inf (groups x
 * k, may be NULL) as in blsgpu_g2_mul_secret: out_aff and out_ser may each be NULL, not both.  -EINVAL before anything is
 * written: k == 0 or above the limit, n_msg neither 1 nor groups, a NULL required buffer.  groups == 0 writes nothing and
 * returns 0.  The claim is the one stated above; H(m) and the players are public. */
int blsgpu_sign_threshold(blsgpu_ctx *ctx, const uint8_t *sks, const uint8_t *x, size_t k, size_t groups,
                          const uint8_t *msg_hashes, size_t n_msg, uint8_t *out_aff, uint8_t *out_ser, uint8_t *out_inf,
                          uint8_t *status);
/* The same with every buffer in device memory, enqueued on `stream` (no synchronisation). */
int blsgpu_sign_threshold_dev(blsgpu_ctx *ctx, const void *d_sks, const void *d_x, size_t k, size_t groups,
                              const void *d_msg_hashes, size_t n_msg, void *d_out_aff, void *d_out_ser, void *d_out_inf,
                              void *d_status, void *stream);

/* Secure aggregation (util.hash_pks, util.py:36-50 of the reference; BLS.aggregate_sigs_secure, bls.py:28-56;
 * BLS.aggregate_pub_keys and BLS.aggregate_priv_keys, bls.py:203-249) for `groups` independent groups at once, the exponents
 *     t_gi = SHA256(be32(i) || SHA256(ser(pk_g0) || ... || ser(pk_g,k-1))) mod n
 * computed on the device (csrc/blsgpu_hashpks.hip on csrc/hash_pks.h) and handed to the sums without a host round trip.
 * pks_ser: groups x k x 48 bytes, PublicKey.serialize() of every key IN THE ORDER TO BE HASHED (the reference sorts the keys
 * before it hashes them in aggregate_pub_keys and does not in aggregate_sigs_secure / aggregate_priv_keys: the order is the
 * caller's), 16-byte aligned; one k per call.  pk_hash_in (may be NULL): groups x 32 bytes, the inner SHA-256 of every group
 * computed by the caller; then k_hash_pks_digest is not launched and pks_ser is not read (it may be NULL).  One group per lane
 * is 0.75 k compressions in sequence: below 64 groups the kernel cannot fill one wavefront, and a single group of 2^20 keys
 * is 786 433 sequential compressions -- there the host's SHA-256 is the right tool and the caller passes its digest.
 * k_hash_pks_exp then writes one exponent per lane, 32 bytes big-endian, below n.  All of this is PUBLIC data.
 * Common to the entries below: -EINVAL before anything is written for k == 0 or m == 0 (also with groups == 0), a NULL
 * context, a NULL required buffer with groups > 0 (pks_ser and pk_hash_in both NULL included); groups == 0 writes nothing and
 * returns 0.  The _dev forms take every buffer in device memory (4-byte aligned, pks_ser 16) and enqueue on `stream` without
 * synchronising.
 *
 * blsgpu_hash_pks (util.py:36-50): out_ts[(g * m + i) * 32 ..] = t_gi for i < m -- m, the reference's num_outputs, is
 * independent of k.  out_pk_hash (may be NULL): groups x 32 bytes, the inner digests (computed or copied from pk_hash_in). */
int blsgpu_hash_pks(blsgpu_ctx *ctx, const uint8_t *pks_ser, size_t k, size_t groups, const uint8_t *pk_hash_in, size_t m,
                    uint8_t *out_ts, uint8_t *out_pk_hash);
int blsgpu_hash_pks_dev(blsgpu_ctx *ctx, const void *d_pks_ser, size_t k, size_t groups, const void *d_pk_hash_in, size_t m,
                        void *d_out_ts, void *d_out_pk_hash, void *stream);
/* BLS.aggregate_pub_keys(keys, secure=True) (bls.py:203-223): out[g] = sum_i t_gi P_gi.  pts_aff: groups x k x 96 bytes, the
 * affine points of the same keys in the same order as pks_ser (the caller has both: sorting needs the serialisations; taking
 * both means no decompression step and no new failure mode).  The exponents (m = k) go to the context's workspace, then the
 * sums are those of blsgpu_g1_msm_dev over the same groups x k layout: out_aff (groups x 96, (0,0) for infinity) and out_inf
 * (groups flags, may be NULL) as there.  The order is the caller's: the reference sorts the keys first. */
int blsgpu_aggregate_pub_keys_secure(blsgpu_ctx *ctx, const uint8_t *pts_aff, const uint8_t *pks_ser, const uint8_t *pk_hash_in,
                                     size_t k, size_t groups, uint8_t *out_aff, uint8_t *out_inf);
int blsgpu_aggregate_pub_keys_secure_dev(blsgpu_ctx *ctx, const void *d_pts_aff, const void *d_pks_ser, const void *d_pk_hash_in,
                                         size_t k, size_t groups, void *d_out_aff, void *d_out_inf, void *stream);
/* BLS.aggregate_sigs_secure (bls.py:28-56; the colliding part of BLS.aggregate_sigs, bls.py:58-151): out[g] = sum_{i<k}
 * t_gi S_gi for k signatures per group (sigs_aff: groups x k x 192 bytes affine, in the order the exponents multiply them:
 * the reference sorts them by (message hash, key, signature)) with the m = k exponents hashed over k_pks keys per group --
 * BLS.aggregate_sigs hashes a different number of keys than it has signatures.  Then blsgpu_g2_msm_dev: out_aff
 * (groups x 192), out_inf (may be NULL). */
int blsgpu_aggregate_sigs_secure(blsgpu_ctx *ctx, const uint8_t *sigs_aff, size_t k, const uint8_t *pks_ser, size_t k_pks,
                                 const uint8_t *pk_hash_in, size_t groups, uint8_t *out_aff, uint8_t *out_inf);
int blsgpu_aggregate_sigs_secure_dev(blsgpu_ctx *ctx, const void *d_sigs_aff, size_t k, const void *d_pks_ser, size_t k_pks,
                                     const void *d_pk_hash_in, size_t groups, void *d_out_aff, void *d_out_inf, void *stream);
/* BLS.aggregate_priv_keys(keys, public_keys, secure=True) (bls.py:225-249): out[g] = sum_i t_gi sks[g * k + i] mod n, the
 * canonical integer below n, 32 bytes big-endian.  sks: groups x k x 32 bytes big-endian, any value below 2^256;
 * sks[g * k + i] is the key that t_gi multiplies, pks_ser is in the order to be hashed -- in the reference these two orders
 * DIFFER (the pairs are sorted by public key, bls.py:239-240, the exponents hashed over the keys as given, bls.py:241), so no
 * permutation between them is assumed.  The exponents go to the workspace; k_fr_dot_secret takes them as its public
 * coefficients and the keys as its secret y (masked reduction, product and additions); out_pk_aff (groups x 96) and
 * out_pk_ser (groups x 48) may each be NULL: the public key of every sum from k_fix_mul_secret reading the sums where they
 * were left, as in blsgpu_fr_sum_secret.  1 <= k <= BLSGPU_LAGRANGE_MAX_K as in blsgpu_fr_interpolate_at_zero_secret (a group
 * is one workgroup of k_fr_dot_secret); beyond it -EINVAL with a blsgpu_last_error text.
 * The claim is the one stated above for the calls on secrets: the sequence of instructions and of memory addresses does not
 * depend on sks.  It does depend on k, groups and the public keys.  Timing inside the hardware is not claimed.  The two hash
 * kernels touch no secret. */
int blsgpu_aggregate_priv_keys_secure(blsgpu_ctx *ctx, const uint8_t *sks, const uint8_t *pks_ser, const uint8_t *pk_hash_in,
                                      size_t k, size_t groups, uint8_t *out, uint8_t *out_pk_aff, uint8_t *out_pk_ser);
int blsgpu_aggregate_priv_keys_secure_dev(blsgpu_ctx *ctx, const void *d_sks, const void *d_pks_ser, const void *d_pk_hash_in,
                                          size_t k, size_t groups, void *d_out, void *d_out_pk_aff, void *d_out_pk_ser,
                                          void *stream);

/* RAGGED secure aggregation: groups of ANY sizes in one call (csrc/blsgpu_hashpks.hip's *_ranges kernels on csrc/hash_pks.h; host
 * plan csrc/secure_ranges_plan.h).  The three entries above take one k per call, so a caller with groups of many sizes --
 * committees, colliding-message sets, signer subsets -- pays a call, a host assembly and a synchronisation per distinct size;
 * these take them all at once.  Group g hashes the keys [pk_off[g], pk_off[g + 1]) of ONE list of n_keys serialised keys
 * (pks_ser: n_keys x 48 bytes in the order to be hashed, 16-byte aligned) and owns the exponents [exp_off[g], exp_off[g + 1]) of
 * one list: exponent i of group g is t_gi = SHA256(be32(i) || SHA256(the group's keys)) mod n (util.py:36-50), i counted
 * from the group's own begin.  Either table holds groups + 1 uint32 offsets: the first is 0, they never step down, and the last
 * is at most its list's count (keys or points past it belong to no group).  A group may be empty on either side: no keys
 * hashes nothing (SHA256 of the empty string), no exponents gives none -- and, in the aggregates, infinity with flag 1.  The
 * two tables are separate because BLS.aggregate_sigs hashes a different number of keys than it has signatures (bls.py:58-151), the
 * reason the uniform call has k and k_pks and blsgpu_hash_pks' m is independent of k.
 * pk_hash_in (may be NULL): groups x 32 bytes, the inner SHA-256 of every group computed by the caller; then the digest
 * kernel is not launched and pks_ser / pk_off are not read (they may be NULL) -- the advice on few groups and very long groups
 * above holds here as well, and a wavefront of k_hash_pks_digest_ranges runs as long as its longest group (the groups are
 * taken in the caller's order).
 * k_secr_check checks both tables on the device (the host-buffer forms have checked them on the host already) and writes the
 * (begin, end) range table of the sums; the kernels behind it return on its flag, so a bad table is neither followed nor
 * written for.  -EINVAL with a blsgpu_last_error text BEFORE ANYTHING IS WRITTEN to an output: a NULL context, a NULL required
 * buffer with groups > 0, a bad offset table, n_keys or the number of exponents 2^31 or more, 2^30 groups or more.
 * groups == 0 writes nothing and returns 0.  The host-buffer forms stage their groups in slices of at most 2^18 keys,
 * exponents and groups (cut on group boundaries; a longer group is a slice of its own), each a call of its own.  The
 * workspace counts in BLSGPU_WS_TOTAL.  All of this is PUBLIC data: not constant-time.
 *
 * blsgpu_hash_pks_ranges (util.py:36-50 per group): out_ts[32 j ..] for j in [exp_off[g], exp_off[g + 1]) = t_g,j-exp_off[g] --
 * exp_off[groups] exponents in all, 32 bytes big-endian each, below n: the layout blsgpu_g?_msm_ranges take as scalars.
 * out_pk_hash (may be NULL): groups x 32 bytes, the inner digests (computed or copied from pk_hash_in).  The _dev form takes
 * n_exp, the exponents d_out_ts has room for (exp_off[groups] <= n_exp is checked), and synchronises `stream` ONCE to read
 * the verdict on the tables. */
int blsgpu_hash_pks_ranges(blsgpu_ctx *ctx, const uint8_t *pks_ser, size_t n_keys, const uint32_t *pk_off, const uint32_t *exp_off,
                           size_t groups, const uint8_t *pk_hash_in, uint8_t *out_ts, uint8_t *out_pk_hash);
int blsgpu_hash_pks_ranges_dev(blsgpu_ctx *ctx, const void *d_pks_ser, size_t n_keys, const void *d_pk_off, const void *d_exp_off,
                               size_t n_exp, size_t groups, const void *d_pk_hash_in, void *d_out_ts, void *d_out_pk_hash,
                               void *stream);
/* BLS.aggregate_pub_keys(keys, secure=True) (bls.py:203-223) per group: out[g] = sum_i t_gi P_i over the group's own keys,
 * exp_off = pk_off.  pts_aff: n_keys x 96 bytes, the affine points of the keys of pks_ser in the same order (the reference
 * sorts a group's keys first: the order is the caller's).  pk_off is required with pk_hash_in too: it counts the exponents.
 * The exponents and the range table go to the workspace, then the sums are blsgpu_g1_msm_ranges_dev's: out_aff (groups x 96,
 * (0,0) for infinity) and out_flag (groups bytes, required: 0 finite, 1 infinity, 2 the group holds a point that is neither
 * (0,0) nor on the curve and its output is (0,0); such a point enters as infinity, the other groups are not disturbed).
 * Equal-length groups give the bytes of blsgpu_aggregate_pub_keys_secure, out_inf == (flag == 1).  The _dev form makes no
 * synchronisation beyond the ONE of blsgpu_g1_msm_ranges_dev, whose check also refuses a bad offset table. */
int blsgpu_aggregate_pub_keys_secure_ranges(blsgpu_ctx *ctx, const uint8_t *pts_aff, const uint8_t *pks_ser, size_t n_keys,
                                            const uint32_t *pk_off, size_t groups, const uint8_t *pk_hash_in, uint8_t *out_aff,
                                            uint8_t *out_flag);
int blsgpu_aggregate_pub_keys_secure_ranges_dev(blsgpu_ctx *ctx, const void *d_pts_aff, const void *d_pks_ser, size_t n_keys,
                                                const void *d_pk_off, size_t groups, const void *d_pk_hash_in, void *d_out_aff,
                                                void *d_out_flag, void *stream);
/* BLS.aggregate_sigs_secure (bls.py:28-56; the colliding part of BLS.aggregate_sigs, bls.py:58-151) per group: out[g] =
 * sum_i t_gi S_i over the signatures [sig_off[g], sig_off[g + 1]) of sigs_aff (n_sigs x 192 bytes affine, in the order the
 * exponents multiply them: the reference sorts them by (message hash, key, signature)), the exponents counted by sig_off and
 * hashed over the keys [pk_off[g], pk_off[g + 1]).  The sums are blsgpu_g2_msm_ranges_dev's: out_aff (groups x 192), out_flag
 * as above.  Equal-length groups give the bytes of blsgpu_aggregate_sigs_secure. */
int blsgpu_aggregate_sigs_secure_ranges(blsgpu_ctx *ctx, const uint8_t *sigs_aff, size_t n_sigs, const uint32_t *sig_off,
                                        const uint8_t *pks_ser, size_t n_keys, const uint32_t *pk_off, size_t groups,
                                        const uint8_t *pk_hash_in, uint8_t *out_aff, uint8_t *out_flag);
int blsgpu_aggregate_sigs_secure_ranges_dev(blsgpu_ctx *ctx, const void *d_sigs_aff, size_t n_sigs, const void *d_sig_off,
                                            const void *d_pks_ser, size_t n_keys, const void *d_pk_off, size_t groups,
                                            const void *d_pk_hash_in, void *d_out_aff, void *d_out_flag, void *stream);

/* Measurement aid (bench.py): when enabled, HIP events are recorded on the
 * launch stream around every kernel this context launches (up to 1024 launches
 * between reads).  blsgpu_timing_read waits for them and returns, per launch,
 * the duration in ms and the kernel kind: 0 = k_miller (Miller loops + workgroup
 * product), 1 = k_reduce (partial products), 2 = k_reduce with the final
 * exponentiation, 3 = k_miller_slow (degenerate pairs; empty work list normally); the line-stream stages use 4 .. 7, and
 * 8 = k_g2_smul with its table kernel (one record per blsgpu_g2_mul_secret / per slice of blsgpu_sign),
 * 9 = the G1 kernels on secrets: k_fix_mul_secret (one record per blsgpu_g1_mul_gen_secret_dev call / per level of
 * blsgpu_hd_paths_secret / per blsgpu_fr_sum_secret_dev call with keys) and k_poly_eval_secret (one record per
 * blsgpu_g1_poly_check_secret_dev call / per staged slice of the host form),
 * 10 = the scalar kernels on secrets: k_fr_poly_eval_secret, k_fr_dot_secret, k_fr_scale_secret, k_fr_sum_secret (one record
 * per call of blsgpu_threshold_deal_secret_dev with fragments, blsgpu_fr_interpolate_at_zero_secret_dev,
 * blsgpu_sign_threshold_dev, blsgpu_fr_sum_secret_dev, blsgpu_aggregate_priv_keys_secure_dev; the G1 / G2 halves of those
 * calls keep their kinds 9 and 8),
 * 11 = k_hash_pks_digest and 12 = k_hash_pks_exp (one record each per blsgpu_hash_pks_dev / blsgpu_aggregate_*_secure_dev
 * call; no record of kind 11 when the caller hands in the digests; the *_ranges forms record their digest and exponent kernels
 * under the same kinds),
 * 13 = k_seed_keys (one record per slice of 2^20 seeds of blsgpu_keys_from_seeds_dev / per staged slice of the host form; the
 * multiplication behind it keeps kind 9, the copy into the parent records has no record).
 * Reading resets the ring. */
int blsgpu_timing_enable(blsgpu_ctx *ctx, int enable);
int blsgpu_timing_read(blsgpu_ctx *ctx, float *ms, int *kind, size_t cap, size_t *count);

#ifdef __cplusplus
}
#endif
#endif
