// msghash_plan.h -- everything about hashing packed messages of different lengths in one device call that is arithmetic on host
// integers (plain C++, no HIP: compiled for the host and compared with tests/msghash_model.py by
// tests/test_msghash_plan_host.py).  Message i of a call is the bytes [off[i], off[i + 1]) of one packed buffer, `off` holding
// n + 1 values; the kernel this plans for hashes one message per lane, 256 lanes per workgroup.  The header is the host layer
// alone: no kernel and no entry point of the library uses it yet.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "layout.h"

namespace msghash {

using ws::Layout;

constexpr size_t LANES = 256;                                // messages per workgroup of the kernel
constexpr size_t DIGEST = 32;
constexpr uint64_t MAX_LEN = (uint64_t)1 << 32;              // a message is shorter than this: the kernel's byte counts are 32 bits
constexpr size_t SLICE_BYTES = (size_t)1 << 26;              // message bytes per staged slice of the host-buffer forms (blsgpu_keys_from_seeds' staging size)
constexpr size_t SLICE_MSGS = (size_t)1 << 20;              // ... and messages per slice of a call that returns digests alone: its staging per message is a digest and an offset

// SHA-256 compressions of a message of len bytes: the len / 64 blocks of message bytes alone, then one or two that hold the
// rest, the 0x80 byte and the bit length
inline uint64_t blocks(uint64_t len) { return (len + 8) / 64 + 1; }

// workgroups for n messages
inline size_t grid(size_t n) { return (n + LANES - 1) / LANES; }

// What the host-buffer forms refuse before anything is written, in the order it is looked for: message by message a step down
// or a length of MAX_LEN or more, then a last offset past the buffer.  n == 0: nothing is read.  `at` (may be NULL): the
// message, n for PAST_END.
enum Verdict { OK = 0, DECREASING = 1, TOO_LONG = 2, PAST_END = 3 };
inline Verdict validate(const uint64_t* off, size_t n, uint64_t msgs_bytes, size_t* at = nullptr) {
    if (n == 0) return OK;
    for (size_t i = 0; i < n; i++) {
        if (off[i] > off[i + 1] || off[i + 1] - off[i] >= MAX_LEN) {
            if (at) *at = i;
            return off[i] > off[i + 1] ? DECREASING : TOO_LONG;
        }
    }
    if (off[n] > msgs_bytes) {
        if (at) *at = n;
        return PAST_END;
    }
    return OK;
}
inline const char* verdict_text(Verdict v) {
    switch (v) {
        case DECREASING: return "offsets decrease";
        case TOO_LONG: return "a message of 2^32 bytes or more";
        case PAST_END: return "the last offset lies past the message buffer";
        default: return "";
    }
}

// The cut of a validated table into staged slices: messages [lo, hi), whose bytes are [off[lo], off[hi]).  A slice takes
// messages while their bytes stay within `target`; its first message that is not empty is always taken, so a message longer
// than the target is a slice of its own; an empty message never starts a slice after the first, it belongs to the slice of its
// predecessor -- unless that one already holds max_msgs messages, the bound the per-message outputs of a call set (>= 1).
struct Slice { size_t lo, hi; };
inline void cut(const uint64_t* off, size_t n, uint64_t target, size_t max_msgs, std::vector<Slice>& out) {
    out.clear();
    for (size_t lo = 0; lo < n;) {
        size_t hi = lo;
        uint64_t bytes = 0;
        while (hi < n && hi - lo < max_msgs) {
            const uint64_t len = off[hi + 1] - off[hi];
            if (len && bytes && bytes + len > target) break;
            bytes += len;
            hi++;
        }
        out.push_back({lo, hi});
        lo = hi;
    }
}
// what the staging of a cut has to hold: the most messages and the most message bytes of a slice
struct Extent { size_t msgs; uint64_t bytes; };
inline Extent extent(const uint64_t* off, const std::vector<Slice>& slices) {
    Extent e{0, 0};
    for (const Slice& s : slices) {
        if (s.hi - s.lo > e.msgs) e.msgs = s.hi - s.lo;
        if (off[s.hi] - off[s.lo] > e.bytes) e.bytes = off[s.hi] - off[s.lo];
    }
    return e;
}

// The workspace of a device-buffer call that feeds the digests to hash to G2, hash to G1 or signing: the
// digests of the call's messages where the caller does not take them (out_hashes NULL); with out_hashes they are written
// there and the call needs none.
struct Workspace { size_t digests, total; };
inline Workspace workspace(size_t n_msg, bool caller_takes_digests) {
    Layout l{256, 0};
    Workspace w;
    w.digests = l.take(caller_takes_digests ? 0 : n_msg * DIGEST);
    w.total = l.off;
    return w;
}

}   // namespace msghash
