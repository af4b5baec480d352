// blsgpu_vm_check.hip -- TEST-ONLY device library (libblsgpu_vmcheck.so): run_rounds, the round interpreter under every wavefront-VM
// kernel (blsgpu_kernels.hip), on an UPLOADED program and uploaded scratchpad images, so that tests/test_gpu_vm.py can compare every
// slot of every image with the word machine of tests/vm_vectors.py and with vmgen/tablesim.py.  Not linked into libblsgpu.so, not
// declared in include/blsgpu.h, not an ABI.
//
// run_rounds is the production text: this file includes the kernel texts the way blsgpu_api.hip does, with a BLSGPU_TU value no
// kernel group has, so no production kernel body is emitted (blsgpu_tu.h).  The kernel builds a VmTables whose `data` is the uploaded
// record table (run_rounds reads no other member) and passes the uploaded round headers as `seq`.  The program is shared by all
// teams of a call; every team has its own image.  Input and output layout: vm_check_plan.h.
//
// Ops:
//   RUN_FULL          run_rounds<false>: kinds 2 / 3 are INV / SGN
//   RUN_LIGHT         run_rounds<true>, stash = nullptr: kinds 2 / 3 do nothing
//   RUN_LIGHT_STASH   run_rounds<true> with three stash registers per lane, as k_miller_mp has them: kinds 2 / 3 are SAVE / RESTORE
//   RUN_FULL_CHK, RUN_LIGHT_CHK   with the header's check_at and a functor that counts its calls and answers "slot chk_slot of my
//                     team is not zero mod q" through the production slots_nonzero: it reads LDS, so its answer depends on the rounds
//                     before it having been fenced
// each in the three geometries production uses, chosen by the header's teams-per-workgroup word: 64 threads, one team at base16 0
// (k_fq12_op, k_h2c_stage; __launch_bounds__(64)); 256 threads, four teams at wave * nslots * 3 (k_miller; (256, BLSGPU_MILLER_WPS));
// 512 threads, eight teams (k_reduce / k_final_groups; (512)).  Dynamic LDS = teams x nslots x 48 bytes, raised with
// hipFuncSetAttribute.  n is a multiple of the teams per workgroup, at most 64 teams per call.
//
// THE HOST SIDE MAKES A BAD TABLE IMPOSSIBLE TO LAUNCH (vmcheck::verify, vm_check_plan.h; -4 before the launch).  Every global load
// of run_rounds, and why it lies inside the uploaded arrays (nr = n >= 1 rounds, headers H[0 .. nr), table of ndata u16):
//   * ld2(seq, 0), ld2(seq, n > 1 ? 1 : 0), ld2(seq, n > 2 ? 2 : 0): indices below nr.
//   * ld2(seq, i + 3) in round i: only under `i + 3 < n`.
//   * the record fetch before the loop: 64 records of rec_len(H[0].meta) u16 from H[0].data_off; chunk c of lane l is the 8 bytes
//     at u16 data_off + l len + 4 c, c < len / 4.  verify() refuses a round unless data_off is a multiple of 4 (8-byte alignment;
//     the table itself starts 32 + 8 nr bytes into a hipMalloc'ed buffer) and data_off + 64 len <= ndata.  len <= 32 because
//     K <= 30, so c < LIN_CHUNKS = 8 always covers it.
//   * the record fetch inside round i uses h0 AFTER the shift h0 <- h1 <- hraw.  For i + 1 < n that is H[i + 1].  In the last
//     round (i = n - 1) it is whatever the pipeline still holds: n = 1: H[0]; n = 2: H[0] (hraw was loaded from index 0);
//     n >= 3: H[n - 1] again (hraw is not reloaded once i + 3 >= n).  In every case a header OF THIS PROGRAM, and verify() holds
//     every header's 64 records inside the table -- a SAVE / RESTORE header too (data_off + 256 <= ndata), whose records are
//     fetched and never used.  No run depends on an out-of-range read being harmless.
//   * T.stamps is read only under -DBLSGPU_STAMPS, which this library is never built with.
// LDS: a MUL lane loads slots ra and rb whether it stores or not, a LIN lane its K operands (positions K .. 29 are masked to slot 0),
// INV / SGN lanes ra; verify() holds all of these and every destination below 3 nslots, destinations multiples of 3 and distinct
// among the live lanes of a round, the SAVE / RESTORE window K .. K + 11 below nslots, chk_slot below nslots; K in 1 .. 30 and
// MN <= K keep BLSGPU_UOP inside ch[0 .. 8).  nslots <= 1023 and teams x nslots x 48 <= 65536 bound the allocation.
#include "check_runner.h"
#include "vm_check_plan.h"
#define BLSGPU_TU 99                                       // no kernel group: declarations only
#include "blsgpu_tu.h"
#include "blsgpu_kernels.hip"

namespace {
using namespace blsgpu;

// every op, once, with its code (tests/vm_vectors.py pins the codes)
#define VMCHECK_OPS(X) X(RUN_FULL, 0) X(RUN_LIGHT, 1) X(RUN_LIGHT_STASH, 2) X(RUN_FULL_CHK, 3) X(RUN_LIGHT_CHK, 4)
CHECK_ENUM(VMCHECK_OPS)
constexpr bool is_light(int op) { return op == RUN_LIGHT || op == RUN_LIGHT_STASH || op == RUN_LIGHT_CHK; }

struct CountingCheck {                       // "slot `slot` of my team is not zero"; counts its calls
    uint32_t base16, slot, lane;
    uint32_t* calls;
    __device__ __forceinline__ bool operator()() const {
        ++*calls;
        return slots_nonzero(base16, slot, 1, lane) != 0;
    }
};

template <int OP> __device__ __forceinline__ void vm_body(const uint32_t* __restrict__ in, uint32_t nr, uint32_t nslots, uint32_t ndata,
                                                          uint32_t check_at, uint32_t chk_slot, uint32_t n, uint32_t* __restrict__ out) {
    uint32_t* smem = reinterpret_cast<uint32_t*>(smem4);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t item = blockIdx.x * (blockDim.x >> 6) + wave;              // < n: n is a multiple of the teams per workgroup
    const uint32_t team_dw = nslots * 12u;
    uint32_t* team = smem + wave * team_dw;
    const uint32_t base16 = wave * nslots * 3u;
    const uint2* seq = reinterpret_cast<const uint2*>(in + vmcheck::HDR);
    VmTables T = {};
    T.data = reinterpret_cast<const uint16_t*>(in + vmcheck::HDR + 2u * nr);
    const uint32_t* img = in + vmcheck::HDR + 2u * nr + (ndata + 1u) / 2u + (size_t)item * team_dw;
    for (uint32_t i = lane; i < team_dw; i += 64) team[i] = img[i];
    wave_fence();
    uint32_t stash[3] = {0u, 0u, 0u}, calls = 0;
    bool ret = true;
    if constexpr (OP == RUN_FULL) ret = run_rounds(T, seq, nr, base16, lane);
    if constexpr (OP == RUN_LIGHT) ret = run_rounds<true>(T, seq, nr, base16, lane);
    if constexpr (OP == RUN_LIGHT_STASH) ret = run_rounds<true>(T, seq, nr, base16, lane, stash);
    if constexpr (OP == RUN_FULL_CHK) ret = run_rounds<false>(T, seq, nr, base16, lane, nullptr, check_at, CountingCheck{base16, chk_slot, lane, &calls});
    if constexpr (OP == RUN_LIGHT_CHK) ret = run_rounds<true>(T, seq, nr, base16, lane, nullptr, check_at, CountingCheck{base16, chk_slot, lane, &calls});
    wave_fence();
    uint32_t* o = out + (size_t)item * team_dw;
    for (uint32_t i = lane; i < team_dw; i += 64) o[i] = team[i];
    uint32_t* tr = out + (size_t)n * team_dw + (size_t)item * vmcheck::TRAILER;
    if (lane == 0) { tr[0] = ret ? 1u : 0u; tr[1] = calls; }
#pragma unroll
    for (int j = 0; j < 3; j++) tr[2 + 64 * j + lane] = stash[j];
}

// one kernel per op and geometry, under the launch bounds of the production kernels of that geometry
#define VM_KERNEL(NAME, BOUNDS) \
    template <int OP> __global__ void BOUNDS NAME(const uint32_t* __restrict__ in, uint32_t nr, uint32_t nslots, uint32_t ndata, \
                                                  uint32_t check_at, uint32_t chk_slot, uint32_t n, uint32_t* __restrict__ out) { \
        vm_body<OP>(in, nr, nslots, ndata, check_at, chk_slot, n, out); \
    }
VM_KERNEL(k_vm1, __launch_bounds__(64))
VM_KERNEL(k_vm4, __launch_bounds__(256, BLSGPU_MILLER_WPS))
VM_KERNEL(k_vm8, __launch_bounds__(512))

template <int OP> int run_op(const uint32_t* in, size_t words_in, size_t n, uint32_t* out, size_t words_out) {
    vmcheck::Header h;
    const int v = vmcheck::verify(is_light(OP), in, words_in, n, words_out, &h);
    if (v != 0) return v;
    const int lds = (int)(h.tpw * h.nslots * 48u);
    auto kernel = h.tpw == 1 ? k_vm1<OP> : h.tpw == 4 ? k_vm4<OP> : k_vm8<OP>;
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
    return check::guarded_run(in, words_in * 4, out, words_out * 4, 0, [=](const uint32_t* din, uint32_t* dout) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)(n / h.tpw)), dim3(64u * h.tpw), (size_t)lds, 0,
                           din, h.nr, h.nslots, h.ndata, h.check_at, h.chk_slot, (uint32_t)n, dout);
    });
}
}  // namespace

CHECK_EXPORT(blsgpu_vm_check, uint32_t, VMCHECK_OPS)
