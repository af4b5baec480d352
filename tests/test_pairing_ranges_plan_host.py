"""The host plan of the ragged multi-pairing, csrc/pairing_ranges_plan.h (range validation, slices, chunks, chunk tables, fold
levels, buffer sizes, grids, refusals), compiled for the host as a stand-alone program -- once with -O2, once under
AddressSanitizer and UBSan, the range table and the table image in heap blocks of exactly their length -- and compared with
tests/pairing_ranges_model.py; the invariants of a schedule are asserted on every table the program prints."""
import os
import random
import subprocess

import pytest

import pairing_plan_model as P
import pairing_ranges_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")

# one case per line:   plan C S max_groups n m  b0 e0 b1 e1 ..   -> the numbers of pairing_ranges_model.plan
#                      refusals                                   -> code and text of every refusal
HOST_TEST = r'''
#include "pairing_ranges_plan.h"
#include <stdio.h>
#include <iostream>
#include <sstream>
#include <string>
namespace R = pairing_ranges;
int main() {
    static_assert(R::Knobs().pair_ranges_chunk == 16, "the default chunk");
    std::string line, op;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        in >> op;
        if (op == "refusals") {
            for (int r = 0; r < 4; r++) printf("%d|%s\n", R::refusal_code((R::Refusal)r), R::refusal_text((R::Refusal)r));
            continue;
        }
        R::Knobs k;
        pairing::Limits L{};
        size_t n, m;
        in >> k.pair_ranges_chunk >> L.ls_max_pairs >> L.max_groups >> n >> m;
        uint32_t* ranges = m ? new uint32_t[2 * m] : nullptr;                // a heap block of exactly the table
        for (size_t i = 0; i < 2 * m; i++) in >> ranges[i];
        const R::Plan p = R::plan(n, ranges, m, k, pairing::Knobs(), pairing::GFX950, L);
        delete[] ranges;
        printf("%d %zu", (int)p.refusal, p.bad_range);
        if (p.refusal) {
            if (!p.chunks.empty() || !p.folds.empty() || !p.slices.empty()) return 3;    // a refused plan holds no table
            printf("\n");
            continue;
        }
        printf(" %zu %zu %zu %zu %llu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", p.n, p.m, p.chunk, p.slice_pairs, (unsigned long long)p.nchunks,
               p.slots, p.lines_bytes, p.bad_bytes, p.degen_bytes, p.o_partials, p.o_tables, p.ws_bytes, p.final_step, p.slices.size(),
               p.levels.size());
        for (const R::Slice& s : p.slices) {
            printf(" %zu %zu %zu %zu %d %zu %zu", s.lo, s.pairs, s.chunk0, s.nchunks, (int)s.chains, s.waves, s.tab_off);
            if (s.chains) printf(" %d %u %zu %zu %zu %zu", (int)s.ls.chain, s.ls.chain_grid, s.ls.chain_waves, s.ls.lines_bytes, s.ls.bad_bytes, s.ls.degen_bytes);
            else printf(" 0 0 0 0 0 0");
        }
        for (const R::Chunk& c : p.chunks) printf(" %u %u %u", c.first, c.len, c.dest);
        for (const R::Level& l : p.levels) printf(" %zu %zu %zu %zu", l.fold0, l.nfolds, l.waves, l.tab_off);
        for (const R::Fold& f : p.folds) printf(" %u %u %u", f.src, f.count, f.dest);
        const size_t bytes = p.ws_bytes - p.o_tables;
        char* image = new char[bytes];                                       // exactly the upload
        p.fill_tables(image);
        unsigned long long sum = 0;
        for (size_t i = 0; i < bytes / 4; i++) { uint32_t w; memcpy(&w, image + 4 * i, 4); sum += (unsigned long long)(i + 1) * w; }
        delete[] image;
        printf(" %llu\n", sum);
    }
    return 0;
}
'''

BUILDS = {"O2": ["-O2"],
          "sanitizers": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D_GLIBCXX_SANITIZE_VECTOR"]}

FAN = M.FAN
BIG = 1 << 20


def lengths_case(C):
    """every length 0, 1, C-1, C, C+1, 2C+1 side by side, an empty range first, in the middle and last"""
    lens = [0, 1, C - 1, C, 0, C + 1, 2 * C + 1, 0]
    ranges, at = [], 0
    for v in lens:
        ranges.append((at, at + v))
        at += v
    return at, ranges


def random_case(rng):
    n = rng.randrange(0, 200)
    C, S = rng.choice([1, 2, 3, 5, 16]), rng.choice([1, 4, 7, 16, 50, BIG])
    ranges = []
    for _ in range(rng.randrange(0, 12)):
        b = rng.randrange(0, n + 1)
        ranges.append((b, rng.randrange(b, n + 1) if rng.random() < 0.8 else b))
    return C, S, 32768, n, ranges


def cases():
    out = []
    for C in (16, 4, 1, 2):
        n, ranges = lengths_case(C)
        out.append((C, BIG, 32768, n, ranges))
        out.append((C, 5, 3, n, ranges))                                     # ... across slices of 5 pairs, three results per final launch
    # overlapping and repeated ranges, ranges that end at n, an empty range at n
    out.append((16, BIG, 32768, 100, [(0, 65), (10, 30), (0, 65), (64, 100), (99, 100), (100, 100), (0, 100)]))
    out.append((4, 10, 32768, 40, [(0, 40), (5, 25), (5, 25), (40, 40), (10, 10), (9, 11), (20, 30)]))
    # a range across a slice boundary; a boundary inside a chunk-sized run; n a multiple of S with an empty range at n
    out.append((16, 24, 32768, 60, [(20, 30), (0, 60), (23, 25), (24, 24), (47, 49)]))
    out.append((16, 20, 32768, 40, [(40, 40), (0, 0), (20, 20)]))
    # merge_fan, merge_fan + 1 and merge_fan^2 + 1 chunks in one range (C = 2), alone and together
    for k in (FAN, FAN + 1, FAN * FAN, FAN * FAN + 1):
        out.append((2, BIG, 32768, 2 * k + 3, [(0, 2 * k)]))
        out.append((2, BIG, 32768, 2 * k + 3, [(1, 2 * k + 1), (0, 1), (0, 2 * k), (3, 3)]))
    out.append((2, 64, 32768, 2 * (FAN * FAN + 1), [(0, 2 * (FAN * FAN + 1))]))
    # no pairs, no ranges
    out += [(16, BIG, 32768, 0, []), (16, BIG, 32768, 0, [(0, 0), (0, 0)]), (16, BIG, 32768, 7, []), (0, 0, 0, 3, [(0, 3)])]
    # the chain kernels of plan_ls: sixteen lanes, quads, pairs
    out += [(16, BIG, 32768, 5121, [(0, 5121)]), (16, BIG, 32768, 20481, [(0, 17), (20000, 20481)]), (64, 4096, 32768, 9000, [(100, 9000)])]
    # refusals: begin > end, end > n (the first such range is named), too many pairs, 2^31 chunks
    out += [(16, BIG, 32768, 10, [(0, 3), (5, 4), (0, 11)]), (16, BIG, 32768, 10, [(0, 10), (0, 11)]), (16, BIG, 32768, 0, [(0, 1)]),
            (16, BIG, 32768, 0x3FFFFFF1, [(0, 1)]), (1, BIG, 32768, BIG, [(0, BIG)] * 2048)]
    rng = random.Random(20261021)
    out += [random_case(rng) for _ in range(60)]
    return out


CASES = cases()


def case_lines():
    lines = ["refusals"]
    for C, S, mg, n, ranges in CASES:
        lines.append("plan %d %d %d %d %d %s" % (C, S, mg, n, len(ranges), " ".join("%d %d" % r for r in ranges)))
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module", params=sorted(BUILDS))
def out(request, tmp_path_factory):
    """the program's output lines, from the plain and from the sanitizer build"""
    d = tmp_path_factory.mktemp("pairranges_" + request.param)
    src, exe = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, *BUILDS[request.param], "-o", str(exe), str(src)])
    res = subprocess.run([str(exe)], input=case_lines(), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
    return iter(res.stdout.split("\n")[:-1])


def test_against_the_model_and_the_invariants(out):
    for r in range(4):
        code, text = next(out).split("|")
        assert (int(code), text) == M.REFUSALS[r]
    refused = 0
    for C, S, mg, n, ranges in CASES:
        got = [int(x) for x in next(out).split()]
        assert got == M.plan(n, ranges, C, S, mg), (C, S, n, ranges[:8])
        if got[0] == M.OK:
            M.check_invariants(got, ranges)
        else:
            refused += 1
    assert refused == 5
    assert next(out, None) is None


def test_the_model_alone():
    """the rules on the model, with the numbers written out"""
    # lengths 0, 1, 15, 16, 0, 17, 33, 0 with C = 16: 1 + 1 + 1 + 1 + 1 + 2 + 3 + 1 chunks, five folded slots, one level
    n, ranges = lengths_case(16)
    s = M.schedule(n, ranges, 16, BIG)
    assert s["nchunks"] == 11 and s["slots"] == 8 + 5 and len(s["levels"]) == 1
    assert s["slices"][0][2] == [(0, 0, 0), (0, 1, 1), (1, 15, 2), (16, 16, 3), (0, 0, 4), (32, 16, 8), (48, 1, 9), (49, 16, 10), (65, 16, 11),
                                 (81, 1, 12), (0, 0, 7)]
    assert s["levels"] == [[(8, 2, 5), (10, 3, 6)]]
    # a slice boundary at 24 inside the range [20, 30): two chunks, in two slices, folded
    s = M.schedule(60, [(20, 30)], 16, 24)
    assert [sl[2] for sl in s["slices"]] == [[(20, 4, 1)], [(0, 6, 2)], []] and s["levels"] == [[(1, 2, 0)]]
    # FAN^2 + 1 chunks: 9 entries, then 2, then the one into slot 0; FAN^2 chunks: 8, then that one
    s = M.schedule(200, [(0, 2 * (FAN * FAN + 1))], 2, BIG)
    assert [len(l) for l in s["levels"]] == [FAN + 1, 2, 1] and s["levels"][-1][-1][2] == 0
    s = M.schedule(200, [(0, 2 * FAN * FAN)], 2, BIG)
    assert [len(l) for l in s["levels"]] == [FAN, 1]
    # refusals, in their order
    assert M.schedule(10, [(0, 3), (5, 4), (0, 11)], 16, BIG) == (M.BAD_RANGE, 1)
    assert M.schedule(M.MAX_PAIRS + 1, [(5, 4)], 16, BIG) == (M.TOO_MANY_PAIRS, 0)
    assert M.schedule(BIG, [(0, BIG)] * 2048, 1, BIG) == (M.TOO_MANY_CHUNKS, 0)
    for case in CASES[:30]:
        C, S, mg, n, ranges = case
        nums = M.plan(n, ranges, C, S, mg)
        if nums[0] == M.OK:
            M.check_invariants(nums, ranges)
    assert P.LITERALS[1] == BIG and M.DEFAULT_CHUNK == 16
