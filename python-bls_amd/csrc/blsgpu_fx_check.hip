// blsgpu_fx_check.hip -- TEST-ONLY device library (libblsgpu_fxcheck.so): the routines of blsgpu_fexp.hip, namespace fx -- the steps of
// k_fexp_team, the six-lanes-per-result final exponentiation -- as kernels of their own, operands and results as raw limb words in
// global memory, so that tests/test_gpu_fx.py can compare the COMPILED routines word for word with the limb model
// (tests/fx_vectors.py) and check the device's own words in plain integers mod q.  Not linked into libblsgpu.so, not declared in
// include/blsgpu.h, not an ABI.
//
// The routines are the production ones: this file includes the kernel texts the way blsgpu_api.hip does, with a BLSGPU_TU value no
// kernel group has, so no production kernel body is emitted (blsgpu_tu.h).  One kernel per op (a template on the op), under
// k_fexp_team's launch bounds (256, 2).  Team ops use the ml check's layout: an item is one team of six lanes, a value 6 x 2 x 14
// words (lane c: re, im), ten teams per wavefront, forty per workgroup; spare teams and the idle lanes 60 .. 63 repeat the last item,
// take part in every ds_bpermute and store nothing.  Per-lane ops hold one item per lane.  The guard records and the return codes are
// check_runner.h's; at most 4096 items per call.
//
// Two operations are INLINE in k_fexp_team and cannot be called, so their bodies are COPIED here, not called: op 5 (CONJ) and the
// slot traffic of ops 3 / 1 (ST, then MUL through the slot).  The script dispatch itself, LD, and the kernel's own slot pointer are
// covered by the traced run of tests/test_gpu_fx.py only.
//
// Ops, the call sites in k_fexp_team and the operand range each site delivers (derived from vmgen/fexp_model.script() by
// tests/fx_vectors.py script_sites(); "dense" is mul_dense's output: digits 0 .. 12 in [0, 2^28), value in (-2q, 4q); "small" is
// reduce_small's: digits, value in (-2q, 2q); "fe" a product's: digits, value in (-q, 2q)):
//   REDUCE_SMALL    14 words -> 14 words.  cyc_sqr's two calls: x = 3 t -+ 2 f, t a dot3 output (fe), f dense or small: limbs 0 .. 12
//                   in (-2^29, 2^28 + 2^30), value in (-11q, 14q)  (3 (-q, 2q) -+ 2 (-2q, 4q))
//   CYC_SQR         team -> team.  Script op 2 (CSQ).  Every CSQ run is entered from a MUL output (dense), from an ST of one (the
//                   accumulator is unchanged) or from an LD of a dense value; inside a run the operand is a cyc_sqr output (small)
//   CYC_SQR_CHAIN   team, n -> the team after n squarings, then the team after the first and after the second: the kernel's
//                   `#pragma unroll 1` loop with the run-time count (n uniform per call, at most 64; the script's longest run is 32)
//   FROB            team, j3 -> team.  Script op 6, j3 = arg (uniform).  Entered from ST of a dense value (j3 = 1), from LD of a
//                   dense value (j3 = 0, 1, 2): always dense
//   TINV            team -> team.  Script op 7, once: entered from a MUL output (dense); only coefficient 0 is read
//   FQ_INVERSE      14 words -> 14 words.  tinv's BLSGPU_FEXP_FERMAT branch: the norm, a dot2 output (fe)
//   CONJ            team -> team.  Script op 5: entered from ST of the input (from_vm's products: fe), from a CSQ run (small) and
//                   from LD of a dense value: the widest is dense
//   SLOT_ROUNDTRIP  teams f, g -> f g.  Script ops 3 and 1: every lane stores its part of g to slot BLS28_FEXP_NSLOTS - 1 of its
//                   team's slot area (release fence), mul_dense with GlobalRec reads the record back (acquire fence); the area is
//                   indexed as the kernel indexes it, the idle lanes' team 10 included, and lies behind the second guard.  f and g
//                   are dense, small (after CSQ), frob's or CONJ's outputs (fe): the widest is dense
// The host side refuses, before anything is launched (-4): a CYC_SQR_CHAIN count that differs between items, is negative or exceeds
// 64; a FROB j3 that differs between items or is outside 0 .. 2.
#include "check_runner.h"
#define BLSGPU_TU 99                                       // no kernel group: declarations only
#include "blsgpu_tu.h"
#include "blsgpu_kernels.hip"
#include "fp28.h"
#include "blsgpu_ml.hip"
#include "blsgpu_fexp.hip"

namespace {
using namespace blsgpu;
using r28::NL;

// every op, once, with its code (tests/fx_vectors.py pins the codes)
#define FXCHECK_OPS(X) \
    X(REDUCE_SMALL, 0) X(FQ_INVERSE, 1) \
    X(CYC_SQR, 10) X(CYC_SQR_CHAIN, 11) X(FROB, 12) X(TINV, 13) X(CONJ, 14) X(SLOT_ROUNDTRIP, 15)
CHECK_ENUM(FXCHECK_OPS)
constexpr int V2 = 2 * NL, TV = 6 * V2, MAX_CHAIN = 64, RT_SLOT = BLS28_FEXP_NSLOTS - 1;
constexpr size_t MAX_ITEMS = 1u << 12;
constexpr size_t AREA_DW = (size_t)(ml::TEAMS + 1) * BLS28_FEXP_NSLOTS * ml::DENSE_DW;    // slot words of one wavefront

// words per item in and out, lanes per item
template <int OP> struct Shape;
#define SHAPE(OP, WIN, WOUT, LANES) template <> struct Shape<OP> { static constexpr int win = WIN, wout = WOUT, lanes = LANES; };
SHAPE(REDUCE_SMALL, NL, NL, 1) SHAPE(FQ_INVERSE, NL, NL, 1)
SHAPE(CYC_SQR, TV, TV, 6) SHAPE(CYC_SQR_CHAIN, TV + 1, 3 * TV, 6) SHAPE(FROB, TV + 1, TV, 6) SHAPE(TINV, TV, TV, 6) SHAPE(CONJ, TV, TV, 6)
SHAPE(SLOT_ROUNDTRIP, 2 * TV, TV, 6)

// ---- one item per lane ---------------------------------------------------------------------------------------------------------
template <int OP> __global__ void __launch_bounds__(256, 2) k_lane(const int32_t* __restrict__ in, uint32_t n, int32_t* __restrict__ out) {
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t item = id < n ? id : n - 1u;           // spare lanes repeat the last item
    const int32_t* src = in + (size_t)item * NL;
    int32_t x[NL], r[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) x[j] = src[j];
    if constexpr (OP == REDUCE_SMALL) fx::reduce_small(r, x);
    if constexpr (OP == FQ_INVERSE) {
        r28::fe a;
#pragma unroll
        for (int j = 0; j < NL; j++) a.v[j] = x[j];
        const r28::fe b = fx::fq_inverse(a);
#pragma unroll
        for (int j = 0; j < NL; j++) r[j] = b.v[j];
    }
    if (id < n) {
        int32_t* o = out + (size_t)item * NL;
#pragma unroll
        for (int j = 0; j < NL; j++) o[j] = r[j];
    }
}

// ---- teams of six lanes ----------------------------------------------------------------------------------------------------------
template <int OP> __global__ void __launch_bounds__(256, 2) k_team(const int32_t* __restrict__ in, uint32_t n, int32_t* __restrict__ out, int32_t* __restrict__ ws) {
    const ml::Team t = ml::team_of_lane();
    const uint32_t id = wave_index() * ml::TEAMS + t.slot;
    const bool valid = t.slot < (uint32_t)ml::TEAMS && id < n;
    const uint32_t item = valid ? id : n - 1u;            // spare teams and the idle lanes (c = 0 .. 3 there) repeat the last item
    const int32_t* src = in + (size_t)item * Shape<OP>::win;
    int32_t* o = out + (size_t)item * Shape<OP>::wout;
    int32_t fre[NL], fim[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) { fre[j] = src[t.c * V2 + j]; fim[j] = src[t.c * V2 + NL + j]; }
    if constexpr (OP == CYC_SQR) fx::cyc_sqr(fre, fim, t);
    if constexpr (OP == CYC_SQR_CHAIN) {
        const uint32_t arg = (uint32_t)__builtin_amdgcn_readfirstlane(src[TV]);       // uniform, as the script's arg is
#pragma unroll 1
        for (uint32_t i = 0; i < arg; i++) {
            fx::cyc_sqr(fre, fim, t);
            if (i < 2u && valid) {
                int32_t* q = o + (1 + i) * TV + t.c * V2;
#pragma unroll
                for (int j = 0; j < NL; j++) { q[j] = fre[j]; q[NL + j] = fim[j]; }
            }
        }
    }
    if constexpr (OP == FROB) fx::frob(fre, fim, t, (uint32_t)__builtin_amdgcn_readfirstlane(src[TV]));
    if constexpr (OP == TINV) fx::tinv(fre, fim, t);
    if constexpr (OP == CONJ) {                            // (copied from k_fexp_team, op 5)
        r28::F<1, 1> a, b;
#pragma unroll
        for (int j = 0; j < NL; j++) { a.v[j] = (t.c & 1u) ? -fre[j] : fre[j]; b.v[j] = (t.c & 1u) ? -fim[j] : fim[j]; }
        const r28::fe na = r28::norm(a), nb = r28::norm(b);
#pragma unroll
        for (int j = 0; j < NL; j++) { fre[j] = na.v[j]; fim[j] = nb.v[j]; }
    }
    if constexpr (OP == SLOT_ROUNDTRIP) {                  // (copied from k_fexp_team: the slot pointer, op 3 on g, op 1 on f)
        int32_t* slots = ws + (size_t)(wave_index() * (ml::TEAMS + 1) + t.slot) * BLS28_FEXP_NSLOTS * ml::DENSE_DW;
        const uint32_t arg = RT_SLOT;
        {
            int32_t* q = slots + arg * ml::DENSE_DW + t.c * 2 * NL;
#pragma unroll
            for (int j = 0; j < NL; j++) { q[j] = src[TV + t.c * V2 + j]; q[NL + j] = src[TV + t.c * V2 + NL + j]; }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        ml::mul_dense(fre, fim, t, ml::GlobalRec{slots + arg * ml::DENSE_DW});
    }
    if (valid) {
        int32_t* q = o + t.c * V2;
#pragma unroll
        for (int j = 0; j < NL; j++) { q[j] = fre[j]; q[NL + j] = fim[j]; }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// the run-time words of a call are uniform, as the script's arg is in production, and inside what the routine indexes or loops with
template <int OP> bool args_ok(const int32_t* in, size_t n) {
    if (OP != CYC_SQR_CHAIN && OP != FROB) return true;
    const int32_t first = in[TV], most = OP == FROB ? 2 : MAX_CHAIN;
    if (first < 0 || first > most) return false;
    for (size_t it = 1; it < n; it++)
        if (in[it * Shape<OP>::win + TV] != first) return false;
    return true;
}

constexpr unsigned team_blocks(size_t n) { return (unsigned)(((n + ml::TEAMS - 1) / ml::TEAMS + 3) / 4); }

template <int OP> int run_op(const int32_t* in, size_t words_in, size_t n, int32_t* out, size_t words_out) {
    if (n == 0 || n > MAX_ITEMS || words_in != n * (size_t)Shape<OP>::win || words_out != n * (size_t)Shape<OP>::wout) return -2;
    if (!args_ok<OP>(in, n)) return -4;
    // the slot areas of every wavefront launched, behind the second guard
    const size_t extra = OP == SLOT_ROUNDTRIP ? (size_t)team_blocks(n) * 4 * AREA_DW * sizeof(int32_t) : 0;
    return check::guarded_run(in, words_in * 4, out, words_out * 4, extra, [=](const int32_t* din, int32_t* dout) {
        if constexpr (Shape<OP>::lanes == 6) k_team<OP><<<dim3(team_blocks(n)), dim3(256)>>>(din, (uint32_t)n, dout, dout + words_out + check::GUARD / 4);
        else k_lane<OP><<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(din, (uint32_t)n, dout);
    });
}
}  // namespace

CHECK_EXPORT(blsgpu_fx_check, int32_t, FXCHECK_OPS)
