// blsgpu_ctx.h -- the context behind the C ABI of include/blsgpu.h: every workspace buffer and every tuning knob of the
// library, and the helpers the host side (blsgpu_api.hip) shares -- error reporting, kernel timing, stream ordering, launch
// shapes and the staging of the host-buffer entry points.  Included by blsgpu_api.hip in the host translation unit only.
#pragma once

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail(-EIO, std::string(#expr) + ": " + hipGetErrorString(_e));             \
    } while (0)

// A workspace buffer: device memory that only ever GROWS.  The buffer a larger one replaces goes to `retired` and is kept
// until the context is destroyed (or trimmed by blsgpu_ctx_trim on an idle context), so work already enqueued on it stays
// valid and no hipFree -- a device-wide synchronisation -- happens inside a pipeline.
struct Buf {
    void* p = nullptr;
    size_t cap = 0;                                          // bytes
    template <class T> T* as() const { return (T*)p; }
    // at least `bytes`; contents are scratch, not copied
    int grow(std::vector<void*>& retired, size_t bytes) {
        if (bytes <= cap) return 0;
        size_t want = bytes + bytes / 4;                     // headroom: fewer regrowths
        void* n = nullptr;
        if (hipMalloc(&n, want) != hipSuccess) {
            (void)hipGetLastError();                         // the failed attempt must not show up in a later launch check
            want = bytes;
            HIP_TRY(hipMalloc(&n, want));
        }
        if (p) retired.push_back(p);
        p = n;
        cap = want;
        return 0;
    }
};

// The buffers of a context (blsgpu_ctx::buf) and the field of blsgpu_ctx_workspace_bytes each one counts under.
enum BufId {
    B_PART0, B_PART1,    // partials: 144 x u32 (BLSGPU_FQ12_BYTES) each, ping-pong over the levels of the reduce chain
    B_IO,                // staging for the host-buffer entry points (Staging)
    B_LINES,             // 68 x pairs line records
    B_LSP0, B_LSP1,      // dense partial products (ping-pong over the merge levels)
    B_BAD,               // one byte per pair: left to the slow program
    B_DEGEN,             // u32 [0] count, [1 ..] block indices of degenerate pairs (k_miller_slow's work list)
    B_EXFLAGS,           // blsgpu_miller_loop_batch's fast form: the caller's flags with "py = 0" marked (2 bytes per pair)
    B_MSM_PART,          // MSM partials; the stage images of decompression and hash to G2; blsgpu_g?_msm_ranges*: the head words, the chunk counts, first_chunk[] and the chunk ranges
    B_BUCKETS,           // the bucket sums' buckets (HBM); the workspace of the sorted, plain and small-group sums; blsgpu_g?_msm_ranges*: the prepared points, the chunk table, the partials, the off-curve counts and one slice's tables (k_smul_seg)
    B_FEXP_WS,           // the slots of k_fexp_team
    B_H2C_WS,            // the lane-private point slots of k_h2c_clear_pairs
    B_FIX_WS,            // blsgpu_hd_children*: the parent key, a flag word and one slice of HMAC outputs (keys_plan.h, ChildrenPlan)
    B_POLY_WS,           // blsgpu_g1_poly_check*: a flag word, the subgroup flags and the commitments in L28 form (keys_plan.h, PolyPlan)
    B_LAGR_WS,           // blsgpu_threshold_combine* / blsgpu_fr_interpolate_at_zero* / blsgpu_sign_threshold*: the coefficients of a call (keys_plan.h, coeff_bytes)
    B_HDP_WS,            // blsgpu_hd_paths*: a flag word and one slice of per-path state (keys_plan.h, PathsPlan)
    B_SMUL_WS,           // blsgpu_g2_mul_secret* / blsgpu_sign* / blsgpu_sign_threshold*: H(m) points and one slice of tables 1P .. 8P of k_g2_smul (keys_plan.h: smul_table_bytes, SignPlan, ThresholdPlan)
    B_FRS_WS,            // blsgpu_sign_threshold*: the scalars lambda_i sk_i of a call and, with a message per session, one slice of H(m) copies (keys_plan.h, ThresholdPlan)
    B_HPK_WS,            // blsgpu_hash_pks* / blsgpu_aggregate_*_secure*: the digests, then the exponents (secure_ranges_plan.h, FixedWorkspace); the *_ranges forms: the head words, the digests, the exponents and the range table of the sums (secure_ranges_plan.h, Workspace)
    B_SHR_WS,            // blsgpu_sig_shares_check*: what one slice of sessions keeps over its rounds -- a flag word, the subgroup flags, H(m), the scalars r and w, the key copies and the leaves A, B (every array, its writer and readers: find_plan.h, FIND_SHR_KEEP)
    B_SHR_ROUND,         // ... and what one round of it takes: the node table, the gathered leaves, the node sums, the pairs, the pairing results and the verdict bytes (find_plan.h, FIND_SHR_ROUND)
    B_SEED_WS,           // blsgpu_keys_from_seeds*: one slice of the keys and of their affine public keys where the caller does not ask for them (keys_plan.h, SeedsPlan)
    B_SM64_WS,           // blsgpu_g1_mul_short* / blsgpu_g2_mul_short* and the leaves of blsgpu_verify_find*: the prepared points, their live flags and one launch's tables 0 .. 15 P (k_smul64)
    B_FIND_WS,           // blsgpu_verify_find* / blsgpu_verify_find_folded* (which adds the leaves in the dense order and the run table): what one slice of items keeps over its rounds -- a flag word, n_e, the subgroup flags, H(h), the weights, the dense order and the leaves A, B (find_plan.h, FIND_KEEP)
    B_FIND_ROUND,        // ... and what one round of it takes: the node offsets, the gathered leaves, the node sums, the pairs, the pairing results and the verdict bytes (find_plan.h: FIND_PLAIN_HEAD and FIND_PLAIN_PART, or FIND_FOLD_ROUND)
    B_FIND_UNIT,         // ... and e(-G1, G2) with the pair it comes from, computed once per context (find_unit_ready)
    B_PSCAN_G1,          // blsgpu_g1_range_sums* and SB of blsgpu_verify_find_folded*: one slice of prepared points, their live and kind bytes, the chunk totals and counts, the prefix records and counts, the carry (blsgpu_pscan.hip)
    B_PSCAN_G2,          // ... the same for blsgpu_g2_range_sums* and SA
    B_PSCAN_RANGE,       // blsgpu_g?_range_sums*: a flag word and, when the points take several slices, the record and count at every range's begin
    B_SIGDIV_WS,         // blsgpu_sig_divide*: the head words, the mismatch / zero / non-unit / status bytes per point, the refused byte and the range per dividend, the scalars and the working copy of the points
    B_PAIRR_WS,          // blsgpu_pairing_multi_ranges*: the partials (a slot per range, then the slots of the folds), every slice's chunk table and every fold level's table (pairing_ranges_plan.h)
    B_VERAGG_WS,         // blsgpu_verify_aggregates*: the key sums and their flags, the hashed points, the undecided bytes, one slice's pair list and results, and every table of the call (verify_agg_plan.h)
    B_COUNT
};
// (unit: what the buffer is counted in -- whole partials, whole u32 entries, bytes)
struct BufInfo { int ws_field; size_t unit; };
constexpr BufInfo BUF_INFO[B_COUNT] = {
    {BLSGPU_WS_PARTIALS, BLSGPU_FQ12_BYTES}, {BLSGPU_WS_PARTIALS, BLSGPU_FQ12_BYTES}, {BLSGPU_WS_STAGING, 1}, {BLSGPU_WS_LINES, 1},
    {BLSGPU_WS_LINE_PRODUCTS, 1}, {BLSGPU_WS_LINE_PRODUCTS, 1}, {BLSGPU_WS_FLAGS_AND_LISTS, 1}, {BLSGPU_WS_FLAGS_AND_LISTS, 4},
    {BLSGPU_WS_FLAGS_AND_LISTS, 1}, {BLSGPU_WS_GROUP_SUMS, 4}, {BLSGPU_WS_GROUP_SUMS, 4}, {BLSGPU_WS_SLOTS, 1}, {BLSGPU_WS_SLOTS, 1},
    {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1},
    {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}, {BLSGPU_WS_TOTAL, 1}};   // no field of their own: they count in the total only

}  // namespace

// (the knobs of the G1 / G2 sums are msm::Knobs, msm_plan.h; those of the pairing path pairing::Knobs, pairing_plan.h, and
// pairing_ranges::Knobs, pairing_ranges_plan.h; verify_agg_plan.h has none of its own)
struct blsgpu_ctx : msm::Knobs, pairing::Knobs, pairing_ranges::Knobs {
    int device = 0;
    blsgpu::VmTables tabs{};
    void* d_tables = nullptr;          // one allocation holding every table
    uint32_t* d_out = nullptr;         // 576-byte result staging
    uint32_t* d_fix_table = nullptr;   // the fixed-base G1 table (blsgpu_g1fix.hip), built on first use; freed by blsgpu_ctx_destroy only
    uint32_t* d_fix_table_secret = nullptr;   // the signed 4-bit table of k_fix_mul_secret (58 240 bytes), likewise
    bool find_unit_ready = false;      // B_FIND_UNIT holds e(-G1, G2) (blsgpu_verify_find), enqueued on first use
    Buf buf[B_COUNT];
    std::vector<void*> retired;        // Buf::grow
    int grow(BufId id, size_t bytes) { return buf[id].grow(retired, bytes); }
    template <class T> T* at(BufId id) const { return buf[id].as<T>(); }
    uint32_t* part(int i) const { return buf[B_PART0 + i].as<uint32_t>(); }
    int32_t* lsp(int i) const { return buf[B_LSP0 + i].as<int32_t>(); }
    // capacity of each partial buffer, in partials, and of the work list, in entries
    size_t part_cap() const { return (buf[B_PART0].cap < buf[B_PART1].cap ? buf[B_PART0].cap : buf[B_PART1].cap) / BLSGPU_FQ12_BYTES; }
    size_t degen_cap() const { return buf[B_DEGEN].cap / sizeof(uint32_t); }

    // ---- tuning knobs: the defaults are the measured ones; KNOBS below names the environment variable of each, read once
    // by blsgpu_ctx_create
    size_t pow2_max = 32768;           // fixed-exponent powers (hash to G2, decompression): up to this many values per launch two wavefronts per 64 values (k_pow2: 0.32 ms against 0.47); 0: never
    size_t h2c_wide_max = 2048;        // up to this many messages the cofactor clearing runs one message per WAVEFRONT with a product per lane (blsgpu_h2cw.hip: the latency form); 0: never
    size_t h2c_reg_threshold = 8192;   // messages from which cofactor clearing runs in registers (one message per lane PAIR; measured: DESIGN.md 2c)
    size_t h2c_lane_threshold = 2048;  // messages from which the three encoding stages run one encoding per lane (k_h2c_sw0/1/2)
    bool h2c_jacobi = true;            // ... with the quadratic characters decided by a Jacobi-symbol routine: two powers per encoding, not five
    size_t h2c_jacobi_threshold = 16384;   // ... from this many messages (below, five parallel powers finish sooner than three serial symbol loops)
    size_t h2c_quad_max = 16384;       // ... on lane QUADS up to this many messages (k_h2c_clear_quads: half the depth while the chip is not full)
    bool sigdiv_plain = true;           // blsgpu_sig_divide*: a call whose accepted quotients are all 1 sums the negated divisors (blsgpu_g2_range_sums' passes) and multiplies nothing; false: every call takes the scalars through blsgpu_g2_msm_ranges' kernels (the tests hold the two against each other)
    size_t wg256_max_waves = 4096;     // register kernels: launches of up to this many wavefronts go out as 256-thread workgroups (blsgpu_tu.h)

    void* d_fexp_dbg = nullptr;        // tools/fexp_trace.py: the accumulator of result 0 after every operation of the script (k_fexp_team)
    void* d_fexpw_stamps = nullptr;    // tools/fexpw_stamps.py: cycle counter of result 0 around every operation of the script (k_fexp_wide)
    hipEvent_t bulk_event = nullptr;   // caller's event, recorded after the last chip-filling kernel of a Miller stage
    // optional per-kernel timing (blsgpu_timing_enable): HIP events recorded on
    // the launch stream around every kernel, ring of TIMING_SLOTS launches
    bool timing = false;
    static constexpr int TIMING_SLOTS = 1024;
    hipEvent_t* ev0 = nullptr;
    hipEvent_t* ev1 = nullptr;
    int* ev_kind = nullptr;            // 0 k_miller, 1 k_reduce, 2 k_reduce with final exponentiation
    size_t ev_count = 0;
    // The workspace is shared by everything a context launches: a call on another stream than
    // the previous one first waits for that one's work (StreamGuard).
    hipStream_t last_stream = nullptr;
    hipEvent_t last_event = nullptr;
    bool used = false;
    // Pinned host memory for tables a call computes on the host and uploads with hipMemcpyAsync (PinnedTables): it outlives
    // the enqueue, and pin_event -- recorded behind the copy -- is waited for before the next call writes it again.
    void* pin = nullptr;
    size_t pin_cap = 0;
    hipEvent_t pin_event = nullptr;
    bool pin_busy = false;
};

namespace {

// Every knob once: blsgpu_ctx_create sets the field from the variable when it is set -- sizes by strtoull (base 10),
// switches by atoi != 0.
struct Knob {
    const char* env;
    size_t blsgpu_ctx::* size;
    bool blsgpu_ctx::* flag;
    constexpr Knob(const char* e, size_t blsgpu_ctx::* s) : env(e), size(s), flag(nullptr) {}
    constexpr Knob(const char* e, bool blsgpu_ctx::* f) : env(e), size(nullptr), flag(f) {}
};
const Knob KNOBS[] = {
    {"BLSGPU_MP_THRESHOLD", &blsgpu_ctx::mp_threshold},
    {"BLSGPU_MILLER_WIDE3_MAX", &blsgpu_ctx::miller_wide3_max},
    {"BLSGPU_MILLER_WIDE_MAX", &blsgpu_ctx::miller_wide_max},
    {"BLSGPU_MP3_THRESHOLD", &blsgpu_ctx::mp3_threshold},
    {"BLSGPU_LS_THRESHOLD", &blsgpu_ctx::ls_threshold},
    {"BLSGPU_LS_MIN_GROUP", &blsgpu_ctx::ls_min_group},
    {"BLSGPU_LS_TEAMS", &blsgpu_ctx::ls_teams},
    {"BLSGPU_FEXP_TEAM_THRESHOLD", &blsgpu_ctx::fexp_team_threshold},
    {"BLSGPU_FEXP_WIDE", &blsgpu_ctx::fexp_wide},
    {"BLSGPU_FEXP_WIDE_MAX_PARTIALS", &blsgpu_ctx::fexp_wide_max_partials},
    {"BLSGPU_VM_EXACT_LANES", &blsgpu_ctx::vm_exact_lanes},
    {"BLSGPU_LS_MERGE_WIDE_MAX", &blsgpu_ctx::ls_merge_wide_max},
    {"BLSGPU_LS_WIDE_MAX", &blsgpu_ctx::ls_wide_max},
    {"BLSGPU_LS_QUAD_MAX", &blsgpu_ctx::ls_quad_max},
    {"BLSGPU_PIP_THRESHOLD", &blsgpu_ctx::pip_threshold},
    {"BLSGPU_PIP_GROUP_THRESHOLD", &blsgpu_ctx::pip_group_threshold},
    {"BLSGPU_PIP_CHUNKS", &blsgpu_ctx::pip_chunks},
    {"BLSGPU_POW2_MAX", &blsgpu_ctx::pow2_max},
    {"BLSGPU_MSM_WIDE_TAIL", &blsgpu_ctx::msm_wide_tail},
    {"BLSGPU_H2C_WIDE_MAX", &blsgpu_ctx::h2c_wide_max},
    {"BLSGPU_H2C_REG_THRESHOLD", &blsgpu_ctx::h2c_reg_threshold},
    {"BLSGPU_H2C_QUAD_MAX", &blsgpu_ctx::h2c_quad_max},
    {"BLSGPU_TEST_LS_NOMEM", &blsgpu_ctx::test_ls_nomem},
    {"BLSGPU_TEST_SLICE_CAP", &blsgpu_ctx::test_slice_cap},
    {"BLSGPU_H2C_JACOBI", &blsgpu_ctx::h2c_jacobi},
    {"BLSGPU_H2C_JACOBI_THRESHOLD", &blsgpu_ctx::h2c_jacobi_threshold},
    {"BLSGPU_H2C_LANE_THRESHOLD", &blsgpu_ctx::h2c_lane_threshold},
    {"BLSGPU_MSM_SORT_THRESHOLD", &blsgpu_ctx::msm_sort_threshold},
    {"BLSGPU_MSM_SORT2_THRESHOLD", &blsgpu_ctx::msm_sort2_threshold},
    {"BLSGPU_MSM_SORT_BITS", &blsgpu_ctx::sort_bits},
    {"BLSGPU_MSM_SORT2_BITS", &blsgpu_ctx::sort2_bits},
    {"BLSGPU_MILLER_EXACT_LANES", &blsgpu_ctx::miller_exact_lanes},
    {"BLSGPU_MILLER_EXACT_FAST", &blsgpu_ctx::miller_exact_fast},
    {"BLSGPU_MSM_PLAIN_THRESHOLD", &blsgpu_ctx::msm_plain_threshold},
    {"BLSGPU_SMUL_MIN_GROUPS", &blsgpu_ctx::smul_min_groups},
    {"BLSGPU_SMUL_MAX_K", &blsgpu_ctx::smul_max_k},
    {"BLSGPU_HORNER_NP_THRESHOLD", &blsgpu_ctx::horner_np_threshold},
    {"BLSGPU_HORNER_QUADS_THRESHOLD", &blsgpu_ctx::horner_quads_threshold},
    {"BLSGPU_WG256_MAX_WAVES", &blsgpu_ctx::wg256_max_waves},
    {"BLSGPU_MSM_LANE_THRESHOLD", &blsgpu_ctx::msm_lane_threshold},
    {"BLSGPU_MSM_LANE_PAIRS", &blsgpu_ctx::msm_lane_pairs},
    {"BLSGPU_SIGDIV_PLAIN", &blsgpu_ctx::sigdiv_plain},
    {"BLSGPU_PAIR_RANGES_CHUNK", &blsgpu_ctx::pair_ranges_chunk},
};
void read_knobs(blsgpu_ctx* c) {
    for (const Knob& k : KNOBS)
        if (const char* e = getenv(k.env)) {
            if (k.size) c->*k.size = (size_t)strtoull(e, nullptr, 10);
            else c->*k.flag = atoi(e) != 0;
        }
}

struct KernelTimer {
    blsgpu_ctx* c; hipStream_t st; int slot;
    KernelTimer(blsgpu_ctx* c_, hipStream_t st_, int kind) : c(c_), st(st_), slot(-1) {
        if (c->timing && c->ev_count < (size_t)blsgpu_ctx::TIMING_SLOTS) {
            slot = (int)c->ev_count++;
            c->ev_kind[slot] = kind;
            (void)hipEventRecord(c->ev0[slot], st);
        }
    }
    ~KernelTimer() { if (slot >= 0) (void)hipEventRecord(c->ev1[slot], st); }
};

// Serialises the use of the context's workspace across streams (blsgpu_ctx::last_stream).
struct StreamGuard {
    blsgpu_ctx* c; hipStream_t st;
    StreamGuard(blsgpu_ctx* c_, hipStream_t st_) : c(c_), st(st_) {
        if (c->used && c->last_stream != st && c->last_event) (void)hipStreamWaitEvent(st, c->last_event, 0);
    }
    ~StreamGuard() {
        if (c->last_event) (void)hipEventRecord(c->last_event, st);
        c->last_stream = st;
        c->used = true;
    }
};

// Grid and workgroup size for `waves` independent wavefronts of a register kernel (blsgpu_tu.h: wave_index()): four
// wavefronts per workgroup -- one per SIMD of a CU -- while the launch does not fill the chip several times over.
struct WaveShape { unsigned blocks, threads; };
WaveShape wave_shape(const blsgpu_ctx* c, size_t waves) {
    const unsigned per = (waves <= c->wg256_max_waves) ? 4u : 1u;
    return {(unsigned)((waves + per - 1) / per), per * 64u};
}

// The layout of B_IO for one host-buffer call: the entry point declares its regions once, in the order their copies are
// issued; every region starts on a 256-byte boundary.  A WHOLE region is copied by up() / down(); a region of ITEMS holds
// one slice and is copied by up(lo, m) / down(lo, m), items [lo, lo + m) of the host array.  Uploads are asynchronous on
// the null stream, downloads synchronous: the host-buffer forms return with their results.
struct Staging {
    struct Region { size_t off, bytes, item; const char* src; char* dst; bool absent; };
    blsgpu_ctx* c;
    Region r[10];
    int n = 0;
    size_t total = 0;
    explicit Staging(blsgpu_ctx* c_) : c(c_) {}
    int add(bool absent, size_t bytes, size_t item, const void* src, void* dst) {
        r[n] = {total, absent ? 0 : bytes, item, (const char*)src, (char*)dst, absent};
        total += (r[n].bytes + 255) & ~(size_t)255;
        return n++;
    }
    // an input that is not given (NULL) takes no room and is not copied: opt() of it is NULL
    int in(const void* src, size_t bytes) { return add(!src, bytes, 0, src, nullptr); }
    int in(const void* src, size_t items, size_t item) { return add(!src, items * item, item, src, nullptr); }
    // likewise an output that is not asked for -- unless the device form writes it regardless (out_kept)
    int out(void* dst, size_t bytes) { return add(!dst, bytes, 0, nullptr, dst); }
    int out_kept(void* dst, size_t bytes) { return add(false, bytes, 0, nullptr, dst); }
    int out(void* dst, size_t items, size_t item) { return add(!dst, items * item, item, nullptr, dst); }
    int scratch(size_t bytes) { return add(false, bytes, 0, nullptr, nullptr); }
    int alloc() { return c->grow(B_IO, total); }
    char* at(int i) const { return c->at<char>(B_IO) + r[i].off; }
    char* opt(int i) const { return r[i].absent ? nullptr : at(i); }
    int up(size_t lo = 0, size_t m = 0) const {
        for (int i = 0; i < n; i++) {
            const size_t bytes = m ? m * r[i].item : (r[i].item ? 0 : r[i].bytes);
            if (r[i].src && bytes) HIP_TRY(hipMemcpyAsync(at(i), r[i].src + lo * r[i].item, bytes, hipMemcpyHostToDevice, 0));
        }
        return 0;
    }
    int down(size_t lo = 0, size_t m = 0) const {
        for (int i = 0; i < n; i++) {
            const size_t bytes = m ? m * r[i].item : (r[i].item ? 0 : r[i].bytes);
            if (r[i].dst && bytes) HIP_TRY(hipMemcpy(r[i].dst + lo * r[i].item, at(i), bytes, hipMemcpyDeviceToHost));
        }
        return 0;
    }
};

// Tables written by the host for an asynchronous upload: take(bytes) waits for the previous upload from the context's pinned
// block, grows it if need be and hands it out; upload() copies it to the device on `st` and records the event the next take()
// waits for.  The block is freed by blsgpu_ctx_destroy alone, so it outlives everything enqueued from it.
struct PinnedTables {
    blsgpu_ctx* c;
    explicit PinnedTables(blsgpu_ctx* c_) : c(c_) {}
    int take(size_t bytes, void** out) {
        if (c->pin_busy) { HIP_TRY(hipEventSynchronize(c->pin_event)); c->pin_busy = false; }
        if (bytes > c->pin_cap) {
            void* n = nullptr;
            HIP_TRY(hipHostMalloc(&n, bytes + bytes / 4, hipHostMallocDefault));
            if (c->pin) (void)hipHostFree(c->pin);
            c->pin = n, c->pin_cap = bytes + bytes / 4;
        }
        if (!c->pin_event) HIP_TRY(hipEventCreateWithFlags(&c->pin_event, hipEventDisableTiming));
        *out = c->pin;
        return 0;
    }
    int upload(void* d_dst, size_t bytes, hipStream_t st) {
        HIP_TRY(hipMemcpyAsync(d_dst, c->pin, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(c->pin_event, st));
        c->pin_busy = true;
        return 0;
    }
};

// The slice length of a host loop (msm_plan.h: `natural`, unless the test hook caps it)
size_t slice_len(const blsgpu_ctx* c, size_t natural, size_t unit = 1) { return msm::slice_len(*c, natural, unit); }

// body(lo, m) over [0, n) in runs of at most `step` items
template <class F>
int for_slices(size_t n, size_t step, F body) {
    for (size_t lo = 0; lo < n; lo += step)
        if (int rc = body(lo, n - lo < step ? n - lo : step)) return rc;
    return 0;
}

}  // namespace
