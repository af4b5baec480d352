"""The host plan of message pre-hashing, csrc/msghash_plan.h (offset validation, the slice cut on message boundaries, blocks per
message, the grid, the workspace of the fused calls), compiled for the host as a stand-alone program -- once with -O2, once
under AddressSanitizer and UBSan, the offset tables in heap blocks of exactly their length -- and compared with
tests/msghash_model.py."""
import hashlib
import os
import subprocess

import pytest

import msghash_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")

# one case per line
#   blocks len                        -> blocks
#   grid n                            -> workgroups
#   ws n_msg caller_takes_digests     -> offset total
#   validate msgs_bytes n off[n + 1]  -> verdict where
#   cut target max_msgs n off[n + 1]  -> lo hi lo hi .. : most messages, most bytes
HOST_TEST = r'''
#include "msghash_plan.h"
#include <stdio.h>
#include <iostream>
#include <sstream>
#include <string>
// a heap block of exactly n values
static uint64_t* some(std::istream& in, size_t n) { uint64_t* v = new uint64_t[n]; for (size_t i = 0; i < n; i++) in >> v[i]; return v; }
int main() {
    std::string line, op;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        in >> op;
        if (op == "blocks") { uint64_t len; in >> len; printf("%llu\n", (unsigned long long)msghash::blocks(len)); }
        else if (op == "grid") { size_t n; in >> n; printf("%zu\n", msghash::grid(n)); }
        else if (op == "ws") {
            size_t n; int takes;
            in >> n >> takes;
            const msghash::Workspace w = msghash::workspace(n, takes != 0);
            printf("%zu %zu\n", w.digests, w.total);
        } else if (op == "validate") {
            uint64_t msgs_bytes; size_t n;
            in >> msgs_bytes >> n;
            uint64_t* off = n ? some(in, n + 1) : nullptr;
            size_t at = 0;
            const msghash::Verdict v = msghash::validate(off, n, msgs_bytes, &at);
            if (msghash::validate(off, n, msgs_bytes) != v || (v != msghash::OK) != (msghash::verdict_text(v)[0] != 0)) return 3;
            printf("%d %zu\n", (int)v, at);
            delete[] off;
        } else if (op == "cut") {
            uint64_t target; size_t max_msgs, n;
            in >> target >> max_msgs >> n;
            uint64_t* off = some(in, n + 1);
            std::vector<msghash::Slice> slices;
            slices.push_back({7, 9});                                        // cut() clears what is there
            msghash::cut(off, n, target, max_msgs, slices);
            for (const msghash::Slice& s : slices) printf("%zu %zu ", s.lo, s.hi);
            const msghash::Extent e = msghash::extent(off, slices);
            printf(": %zu %llu\n", e.msgs, (unsigned long long)e.bytes);
            delete[] off;
        }
    }
    return 0;
}
'''

BUILDS = {"O2": ["-O2"], "sanitizers": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}

BLOCK_LENGTHS = [0, 55, 56, 63, 64, 119, 120] + M.PAD_LENGTHS + [(1 << 32) - 1]
GRIDS = [1, 255, 256, 257, 512, 513]
WS = [(n, t) for n in (1, 8, 9, 65, 257) for t in (0, 1)]

GOOD = [[0], [0, 0], [5, 5, 5], [0, 1, 1, 70, 200], [3, 3, 10, 10, 10, 4000], [0, (1 << 32) - 1]]
# (offsets, msgs_bytes): one decreasing step, a last offset past the end, a length of 2^32
BAD = [([0, 10, 9, 20], 20), ([4, 3], 100), ([0, 10, 20], 19), ([0, 0], 0), ([7, 7], 6), ([0, 1 << 32], 1 << 32),
       ([0, 5, 5 + (1 << 32), 6 + (1 << 32)], 1 << 40), ([0, 9, 3, 3 + (1 << 32)], 1 << 40)]
VALIDATE = [(off, off[-1]) for off in GOOD] + [(off, off[-1] + 3) for off in GOOD] + BAD

# length tables with empty messages at both ends and in runs, a message longer than every target but 1000's, sums that land on
# a target exactly (64) and one past it (65)
TABLES = [
    [0, 0, 10, 0, 0, 0, 30, 24, 1, 0, 200, 0, 0, 5, 0],
    [0] * 5,
    [64, 64, 65, 1, 63, 0, 1, 64],
    [1] * 70,
    [0, 1000, 0, 1001, 999, 1, 0, 0],
    [300],
    [10, 20, 30, 4, 0, 0, 0, 0, 0, 0, 60, 5],
]
TARGETS = [1, 64, 65, 1000]
CUTS = [(lens, t, cap) for lens in TABLES for t in TARGETS for cap in (1 << 20, 3)]


def offsets_of(lens, start=0):
    off = [start]
    for v in lens:
        off.append(off[-1] + v)
    return off


def case_lines():
    j = lambda v: " ".join(map(str, v))
    lines = ["blocks %d" % v for v in BLOCK_LENGTHS] + ["grid %d" % n for n in GRIDS] + ["ws %d %d" % w for w in WS]
    lines += ["validate %d %d %s" % (mb, len(off) - 1, j(off if len(off) > 1 else [])) for off, mb in VALIDATE]
    lines += ["cut %d %d %d %s" % (t, cap, len(lens), j(offsets_of(lens, 11))) for lens, t, cap in CUTS]
    return "\n".join(lines) + "\n"


def ints(s):
    return [int(x) for x in s.split()]


@pytest.fixture(scope="module", params=sorted(BUILDS))
def out(request, tmp_path_factory):
    """the program's output lines, from the plain and from the sanitizer build"""
    d = tmp_path_factory.mktemp("msghash_" + request.param)
    src, exe = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, *BUILDS[request.param], "-o", str(exe), str(src)])
    res = subprocess.run([str(exe)], input=case_lines(), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
    return iter(res.stdout.split("\n")[:-1])


def test_against_the_model(out):
    for v in BLOCK_LENGTHS:
        assert int(next(out)) == M.blocks(v)
    for n in GRIDS:
        assert int(next(out)) == M.grid(n)
    for n, t in WS:
        assert tuple(ints(next(out))) == M.workspace(n, bool(t))
    for off, mb in VALIDATE:
        verdict, at = ints(next(out))
        assert (verdict, at) == M.validate(off, mb), (off, mb)
    for lens, t, cap in CUTS:
        off = offsets_of(lens, 11)
        left, right = next(out).split(":")
        flat = ints(left)
        slices = list(zip(flat[::2], flat[1::2]))
        assert slices == M.cut(off, t, cap), (lens, t, cap)
        assert tuple(ints(right)) == M.extent(off, slices)
    assert next(out, None) is None


def test_the_model_alone():
    """the properties the rule is stated in, on the model: the verdicts by construction, the slices a partition in order, none
    over the target unless it is one message's bytes, no slice beginning with an empty message but the first, and the block
    counts against a padding written out"""
    assert [M.blocks(v) for v in (0, 55, 56, 63, 64, 119, 120)] == [1, 1, 2, 2, 2, 2, 3]
    for v in BLOCK_LENGTHS[:-1]:
        padded = b"\x00" * v + b"\x80" + b"\x00" * ((55 - v) % 64) + (8 * v).to_bytes(8, "big")
        assert len(padded) % 64 == 0 and M.blocks(v) == len(padded) // 64
    assert all(M.validate(off, off[-1])[0] == M.OK for off in GOOD)
    assert [M.validate(off, mb)[0] for off, mb in BAD] == [M.DECREASING, M.DECREASING, M.PAST_END, M.OK, M.PAST_END, M.TOO_LONG,
                                                           M.TOO_LONG, M.DECREASING]
    for lens, t, cap in CUTS:
        off = offsets_of(lens)
        slices = M.cut(off, t, cap)
        assert [lo for lo, _ in slices] == [0] + [hi for _, hi in slices[:-1]] and slices[-1][1] == len(lens)
        for k, (lo, hi) in enumerate(slices):
            held = [v for v in lens[lo:hi] if v]
            assert 0 < hi - lo <= cap and (sum(held) <= t or len(held) == 1)
            if k and cap > len(lens):
                assert lens[lo] > 0                                         # an empty message stays with its predecessor
    assert M.cut(offsets_of(TABLES[0]), 64, 1 << 20) == [(0, 8), (8, 10), (10, 13), (13, 15)]    # 10 + 30 + 24 = 64 fits
    assert M.cut(offsets_of(TABLES[4]), 1000, 1 << 20) == [(0, 3), (3, 4), (4, 8)]
    msgs, covered = M.padding_list()
    assert covered == {(v, r) for v in M.PAD_LENGTHS for r in range(4)}
    off = M.offsets(msgs)
    assert {(len(m), off[i] % 4) for i, m in enumerate(msgs)} >= covered and all(0 < len(m) < 4 or len(m) in M.PAD_LENGTHS for m in msgs)
    assert M.digests([b"abc"]) == hashlib.sha256(b"abc").digest()
