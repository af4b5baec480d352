// vm_check_plan.h -- TEST-ONLY: the decision the VM check library (blsgpu_vm_check.hip) makes BEFORE it launches: is every load,
// store and loop bound of run_rounds inside the uploaded arrays for this program?  Plain C++, no HIP: tests/test_vm_check_host.py
// compiles it with a host compiler.  Not part of libblsgpu.so, not an ABI.
//
// A call's input, 32-bit words:
//   [0 .. 8)    header: nr (rounds), nslots, ndata (length of the record table in u16), check_at, chk_slot (the slot the check
//               functor looks at), tpw (teams per workgroup: 1, 4 or 8), 0, 0
//   then        nr round headers {data_off, meta}                              (2 nr words)
//   then        the record table, two u16 per word, low half first             ((ndata + 1) / 2 words)
//   then        one scratchpad image of nslots x 12 words for each of the n teams
// and its output: the n images after the run, then per team {run_rounds' return value, calls of the functor, 3 x 64 stash words
// (register j of lane l at 64 j + l)}.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace vmcheck {
constexpr uint32_t HDR = 8;
constexpr uint32_t MAX_ROUNDS = 1u << 16;                  // nr and check_at
constexpr uint32_t MAX_TEAMS = 64;
constexpr uint32_t MAX_SLOTS = 1023;                       // a micro-op's slot field is 10 bits
constexpr uint32_t MAX_DATA = 1u << 24;                    // u16 entries of the table
constexpr uint32_t MAX_LIN_K = 30;                         // 4 * LIN_CHUNKS - 2 (blsgpu_kernels.hip)
constexpr uint32_t LDS_MAX = 65536;                        // dynamic LDS a workgroup of any geometry may ask for
constexpr uint32_t INACTIVE = 0xFFFFu;
constexpr uint32_t TRAILER = 2 + 3 * 64;                   // per team behind the images

struct Header { uint32_t nr, nslots, ndata, check_at, chk_slot, tpw; };

// per-lane record length of a round in u16 (the same rule as blsgpu_kernels.hip rec_len)
inline uint32_t rec_len(uint32_t meta) {
    if ((meta & 3u) != 1u) return 4u;
    return (((meta >> 8) & 0xFFu) + 2u + 3u) & ~3u;
}
inline size_t words_in(const Header& h, size_t n) { return HDR + 2 * (size_t)h.nr + ((size_t)h.ndata + 1) / 2 + n * (size_t)h.nslots * 12; }
inline size_t words_out(const Header& h, size_t n) { return n * ((size_t)h.nslots * 12 + TRAILER); }

// 0: the program may be launched; -2: sizes; -4: a table the interpreter must not be given.  light: kinds 2 / 3 are SAVE / RESTORE
// of the 12-slot window at slot K (run_rounds<true>), else INV / SGN.
inline int verify(bool light, const uint32_t* in, size_t nwords_in, size_t n, size_t nwords_out, Header* out = nullptr) {
    if (in == nullptr || nwords_in < HDR || n == 0 || n > MAX_TEAMS) return -2;
    const Header h = {in[0], in[1], in[2], in[3], in[4], in[5]};
    if (h.nr == 0 || h.nslots == 0 || h.ndata > MAX_DATA || in[6] != 0 || in[7] != 0) return -2;
    if (h.tpw != 1 && h.tpw != 4 && h.tpw != 8) return -2;
    if (n % h.tpw != 0) return -2;
    if (h.nr > MAX_ROUNDS || h.check_at > MAX_ROUNDS || h.nslots > MAX_SLOTS) return -4;
    if (nwords_in != words_in(h, n) || nwords_out != words_out(h, n)) return -2;
    if ((size_t)h.tpw * h.nslots * 48 > LDS_MAX) return -4;
    if (h.chk_slot >= h.nslots) return -4;
    const uint32_t* seq = in + HDR;
    const uint32_t* tab = seq + 2 * (size_t)h.nr;
    auto d16 = [&](size_t i) -> uint32_t { return (tab[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu; };
    const uint32_t ref_end = 3 * h.nslots;
    std::vector<uint8_t> written(h.nslots);
    for (uint32_t r = 0; r < h.nr; r++) {
        const uint32_t off = seq[2 * r], meta = seq[2 * r + 1], kind = meta & 3u, len = rec_len(meta);
        if (off % 4 != 0 || (uint64_t)off + 64ull * len > h.ndata) return -4;      // (also the look-ahead fetch of a SAVE / RESTORE round)
        written.assign(h.nslots, 0);
        // a destination: INACTIVE, or a multiple of 3 below 3 nslots that no other live lane of the round has
        auto dst_ok = [&](uint32_t rd) -> bool {
            if (rd == INACTIVE) return true;
            if (rd % 3 != 0 || rd >= ref_end || written[rd / 3]) return false;
            written[rd / 3] = 1;
            return true;
        };
        if (kind == 1u) {
            const uint32_t K = (meta >> 8) & 0xFFu, levels = (meta >> 16) & 3u, MN = (meta >> 18) & 0xFFu;
            if (K == 0 || K > MAX_LIN_K || MN > K || levels > 2 || (meta >> 26) != 0 || (meta & 0xFCu) != 0) return -4;
            for (uint32_t lane = 0; lane < 64; lane++) {
                const size_t rec = (size_t)off + (size_t)lane * len;
                if (!dst_ok(d16(rec))) return -4;
                if ((d16(rec + 1) & 0x3FFFu) != 0) return -4;                      // merge flags: bits 14 and 15 only
                for (uint32_t p = 0; p < K; p++) {                                   // every lane loads its K operands, a live one or not
                    const uint32_t u = d16(rec + 2 + p);
                    if (u >> 15 || (u & 1023u) >= h.nslots) return -4;
                }
            }
        } else if (light && kind >= 2u) {
            const uint32_t K = (meta >> 8) & 0xFFu;
            if ((meta >> 16) != 0 || (meta & 0xFCu) != 0 || K + 12 > h.nslots) return -4;
        } else {
            if ((meta >> 2) != 0) return -4;
            for (uint32_t lane = 0; lane < 64; lane++) {
                const size_t rec = (size_t)off + 4 * (size_t)lane;
                const uint32_t ra = d16(rec), rb = d16(rec + 1), rd = d16(rec + 2);
                // a MUL lane loads both operands whether it stores or not
                if (ra % 3 != 0 || ra >= ref_end || rb % 3 != 0 || rb >= ref_end || !dst_ok(rd)) return -4;
            }
        }
    }
    if (out) *out = h;
    return 0;
}
}  // namespace vmcheck
