// check_runner.h -- TEST-ONLY: the host side the check libraries share (blsgpu_fp28_check.hip, blsgpu_fq32_check.hip,
// blsgpu_wide_check.hip, blsgpu_ml_check.hip, blsgpu_fr_check.hip, blsgpu_curve_check.hip, blsgpu_fx_check.hip, blsgpu_vm_check.hip, blsgpu_h2c_check.hip).  Not part of
// libblsgpu.so, not an ABI.
//
// Every library exports ONE function, int blsgpu_<layer>_check(op, in, words_in, n, out, words_out), over 32-bit words.
// It returns
//    0    the op ran; `out` holds its words
//   > 0   a HIP error code
//   -1    unknown op
//   -2    sizes that do not match the op (or n = 0, or n above the library's limit)
//   -3    a guard record was written: the device output lies between two records of GUARD bytes of 0xAA, and a lane stored
//         outside its own record
//   -4    a record the library refuses before launching (an address outside the value file, a position outside 0 .. 5, a loop count
//         or table index that is too large or differs between the items of a call, a VM program that vm_check_plan.h refuses, an image slot
//         outside the stage image)
// and launches nothing unless it returns 0, -3 or a HIP error.
//
// Each library names its ops ONCE, in an X-macro LIB_OPS(X) of entries X(NAME, code); the enum, the exported switch and the
// host build's switch are generated from it (CHECK_ENUM, CHECK_EXPORT, CHECK_HOST_ENTRY).
#pragma once
#include <stddef.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
// the qualifiers of op bodies that also compile for the host (a plain C++ compiler includes the check file itself)
#define CHECK_FN __device__ __forceinline__
#define CHECK_MEMBER __device__ __forceinline__
#else
#define CHECK_FN static inline
#define CHECK_MEMBER inline
#endif

namespace check {
constexpr size_t GUARD = 256;                              // bytes of 0xAA on either side of the output

// back: the front guard, bytes_out bytes of output, the back guard, as they came back from the device
inline bool guards_intact(const unsigned char* back, size_t bytes_out) {
    for (size_t j = 0; j < GUARD; j++)
        if (back[j] != 0xAA || back[GUARD + bytes_out + j] != 0xAA) return false;
    return true;
}

#if defined(__HIPCC__)
// One guarded call: upload `in`, fill guard | output | guard | bytes_extra with 0xAA, launch(device in, device out past the
// first guard), wait, read output and guards back.  bytes_extra lie behind the second guard and are never read back (the ml
// check's dump record).  Both buffers are freed on every path.
template <class W, class Launch> int guarded_run(const W* in, size_t bytes_in, W* out, size_t bytes_out, size_t bytes_extra, Launch launch) {
    char *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc((void**)&din, bytes_in);
    if (e == hipSuccess) e = hipMalloc((void**)&dout, bytes_out + 2 * GUARD + bytes_extra);
    if (e == hipSuccess) e = hipMemcpy(din, in, bytes_in, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0xAA, bytes_out + 2 * GUARD + bytes_extra);
    if (e == hipSuccess) {
        launch((const W*)din, (W*)(dout + GUARD));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    std::vector<unsigned char> back(bytes_out + 2 * GUARD);
    if (e == hipSuccess) e = hipMemcpy(back.data(), dout, back.size(), hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    if (e != hipSuccess) return (int)e;
    if (!guards_intact(back.data(), bytes_out)) return -3;   // a lane stored outside its record
    memcpy(out, back.data() + GUARD, bytes_out);
    return 0;
}
#endif
}  // namespace check

// ---- what is generated from a library's op list ---------------------------------------------------------------------------
#define CHECK_ENUM_ENTRY(OP, CODE) OP = CODE,
#define CHECK_ENUM(OPS) enum Op { OPS(CHECK_ENUM_ENTRY) };
// the exported function: run_op<OP> of the library for an op of the list, -1 for any other code
#define CHECK_RUN_CASE(OP, CODE) case OP: return run_op<OP>(in, words_in, n, out, words_out);
#define CHECK_EXPORT(NAME, WORD, OPS) \
    extern "C" __attribute__((visibility("default"))) int NAME(int op, const WORD* in, size_t words_in, size_t n, WORD* out, size_t words_out) { \
        switch (op) { OPS(CHECK_RUN_CASE) } \
        return -1; \
    }
// the host build's entry: one item of a lane-layout op through Do<OP>::run; false for an op the list does not have
#define CHECK_HOST_CASE(OP, CODE) case OP: Do<OP>::run(in, out); return true;
#define CHECK_HOST_ENTRY(NAME, OPS) \
    static inline bool NAME(int op, const uint32_t* in, uint32_t* out) { \
        switch (op) { OPS(CHECK_HOST_CASE) } \
        return false; \
    }
