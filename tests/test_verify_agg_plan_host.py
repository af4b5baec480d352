"""The host plan of blsgpu_verify_aggregates*, csrc/verify_agg_plan.h (validation of the three tables, key ranges, pair slots,
slices on aggregate boundaries, range and source tables, workspace, grids, refusals with the first offending entry), compiled
for the host as a stand-alone program -- once with -O2, once under AddressSanitizer and UBSan, the three tables and the table
image in heap blocks of exactly their length -- and compared with tests/verify_agg_model.py; the invariants of a schedule are
asserted on every plan the program prints."""
import os
import random
import subprocess

import pytest

import verify_agg_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")

# one case per line:   plan cap max_groups n_keys n_msgs m n_grp  L go..  L gm..  L ao..   (L: the entries of the table that follows;
#                      0 entries: a NULL table, for the refusals that read none)  -> the numbers of verify_agg_model.plan
#                      refusals                                                    -> code and text of every refusal
HOST_TEST = r'''
#include "verify_agg_plan.h"
#include <stdio.h>
#include <iostream>
#include <sstream>
#include <string>
namespace V = verify_agg;
static uint32_t* table(std::istringstream& in) {              // a heap block of exactly the table
    size_t len;
    in >> len;
    uint32_t* t = len ? new uint32_t[len] : nullptr;
    for (size_t i = 0; i < len; i++) in >> t[i];
    return t;
}
int main() {
    std::string line, op;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        in >> op;
        if (op == "refusals") {
            for (int r = 0; r < V::REFUSALS; r++) printf("%d|%s\n", V::refusal_code((V::Refusal)r), V::refusal_text((V::Refusal)r));
            continue;
        }
        pairing::Limits L{};
        size_t n_keys, n_msgs, m, n_grp;
        in >> L.ls_max_pairs >> L.max_groups >> n_keys >> n_msgs >> m >> n_grp;
        uint32_t *go = table(in), *gm = table(in), *ao = table(in);
        const V::Plan p = V::plan(go, gm, n_grp, ao, m, n_keys, n_msgs, pairing_ranges::Knobs(), pairing::Knobs(), pairing::GFX950, L, msm::GFX950);
        delete[] go, delete[] gm, delete[] ao;
        printf("%d %zu", (int)p.refusal, p.bad);
        if (p.refusal) {
            if (!p.slices.empty() || !p.src.empty() || !p.key_ranges.empty()) return 3;      // a refused plan holds no table
            printf("\n");
            continue;
        }
        printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", p.m, p.n_grp, p.n_keys, p.n_msgs, p.pairs, p.cap, p.max_pairs, p.max_aggs,
               p.lines_bytes, p.bad_bytes, p.degen_bytes, p.pairr_bytes);
        printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", p.o_sum, p.o_flag, p.o_h, p.o_und, p.o_g1, p.o_g2, p.o_gt, p.o_tables, p.o_neg,
               p.o_kr, p.ws_bytes, p.slices.size());
        for (uint32_t v : p.key_ranges) printf(" %u", v);
        for (const V::Src& e : p.src) printf(" %u %u %u", e.a, e.b, e.agg);
        uint32_t neg[24];
        for (uint32_t i = 0; i < 24; i++) neg[i] = i + 1;
        const size_t bytes = p.ws_bytes - p.o_tables;
        char* image = new char[bytes];                                       // exactly the upload
        p.fill_tables(image, neg);
        for (const V::Slice& s : p.slices) {
            // the multi-pairing's tables in the image are its own image; its sum is printed, and the region left out of the sum
            const size_t pb = s.pr.ws_bytes - s.pr.o_tables;
            char* own = new char[pb];
            s.pr.fill_tables(own);
            if (memcmp(own, image + (s.prtab_off - p.o_tables), pb)) return 4;
            unsigned long long psum = 0;
            for (size_t i = 0; i < pb / 4; i++) { uint32_t w; memcpy(&w, own + 4 * i, 4); psum += (unsigned long long)(i + 1) * w; }
            delete[] own;
            memset(image + (s.prtab_off - p.o_tables), 0, pb);
            printf(" %zu %zu %zu %zu %zu %zu %u %u %zu %zu %llu %zu %llu", s.agg0, s.aggs, s.slot0, s.pairs, s.src_off, s.prtab_off, s.g_pairs,
                   s.g_status, s.pr.o_tables, s.pr.ws_bytes, (unsigned long long)s.pr.nchunks, s.pr.slots, psum);
            for (uint32_t v : s.ranges) printf(" %u", v);
        }
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
BIG = 1 << 20


def build(shapes, n_msgs=None):
    """the three tables of aggregates given as lists of (message, keys) groups"""
    go, gm, ao = [0], [], [0]
    for groups in shapes:
        for msg, k in groups:
            gm.append(msg)
            go.append(go[-1] + k)
        ao.append(len(gm))
    return go, gm, ao, go[-1], (max(gm) + 1 if gm else 0) if n_msgs is None else n_msgs


def random_shapes(rng):
    n_msgs = rng.randrange(1, 9)
    return [[(rng.randrange(n_msgs), rng.choice([0, 1, 1, 2, 8, 9])) for _ in range(rng.choice([0, 1, 1, 2, 3, 7, 16, 17]))]
            for _ in range(rng.randrange(1, 9))], n_msgs


def cases():
    """(cap, max_groups, n_keys, n_msgs, m, n_grp, grp_off, grp_msg, agg_off)"""
    out = []

    def add(shapes, caps=(1, 5, BIG), n_msgs=None, mg=32768):
        go, gm, ao, n_keys, nm = build(shapes, n_msgs)
        for cap in caps:
            out.append((cap, mg, n_keys, nm, len(ao) - 1, len(gm), go, gm, ao))
    # aggregates of 0, 1, 2, 15, 16 and 17 messages; groups of 1, 2, 8 and 9 keys; a shared message and an unused one
    add([[(i, 1) for i in range(k)] for k in (0, 1, 2, 15, 16, 17)])
    add([[(0, 1), (1, 2)], [(2, 8)], [(1, 9), (0, 0)], []], n_msgs=5)
    add([[(0, 1), (1, 1)], [(2, 1), (3, 1)], [(i, 1) for i in range(6)]], mg=2)     # 3, 3 and 7 pairs: caps 5 and 6 cut them apart
    add([[(0, 1), (1, 1)], [(2, 1), (3, 1)], [(i, 1) for i in range(6)]], caps=(6, 7, 13))
    add([[]], n_msgs=0)
    add([[], [], []], n_msgs=3)
    # tables that do not begin at zero: the keys and groups before them belong to nobody
    go, gm, ao, n_keys, nm = build([[(0, 2)], [(1, 1), (0, 3)], [(1, 1)]])
    out.append((BIG, 32768, n_keys + 4, nm, 2, len(gm), [4] + [v + 4 for v in go[1:]], gm, ao[1:]))
    # refusals, each naming its first entry: sizes (no table is read), grp_off down, its end, agg_off down, its end, a message
    out += [(BIG, 32768, 0, 0, M.MAX_AGGS + 1, 0, [], [], []), (BIG, 32768, 0, M.MAX_MSGS + 1, 1, 0, [], [], []),
            (BIG, 32768, 0xFFFFFFF1, 1, 1, 1, [], [], []), (BIG, 32768, 0, 1, M.MAX_AGGS - 3, 4, [], [], []),
            (BIG, 32768, 6, 2, 2, 3, [0, 2, 1, 6], [0, 1, 0], [0, 1, 3]), (BIG, 32768, 6, 2, 2, 3, [0, 2, 1, 0], [0, 1, 0], [0, 1, 3]),
            (BIG, 32768, 7, 2, 2, 3, [0, 2, 4, 6], [0, 1, 0], [0, 1, 3]), (BIG, 32768, 6, 2, 2, 3, [0, 2, 4, 6], [0, 1, 0], [0, 2, 1]),
            (BIG, 32768, 6, 2, 2, 3, [0, 2, 4, 6], [0, 1, 0], [2, 1, 3]), (BIG, 32768, 6, 2, 2, 3, [0, 2, 4, 6], [0, 1, 0], [0, 1, 2]),
            (BIG, 32768, 6, 2, 2, 3, [0, 2, 4, 6], [0, 2, 5], [0, 1, 3]), (BIG, 32768, 6, 0, 2, 3, [0, 2, 4, 6], [0, 0, 0], [0, 1, 3])]
    rng = random.Random(20261021)
    for _ in range(40):
        shapes, n_msgs = random_shapes(rng)
        add(shapes, caps=(rng.choice([1, 2, 3, 5, 8, 18, BIG]),), n_msgs=n_msgs)
    return out


CASES = cases()
REFUSED = [(M.TOO_LARGE, 0)] * 4 + [(M.GRP_OFF_DOWN, 1), (M.GRP_OFF_DOWN, 1), (M.GRP_OFF_END, 3), (M.AGG_OFF_DOWN, 1), (M.AGG_OFF_DOWN, 0),
                                    (M.AGG_OFF_END, 2), (M.BAD_MSG, 1), (M.BAD_MSG, 0)]


def case_lines():
    tab = lambda t: "%d %s" % (len(t), " ".join(map(str, t)))
    lines = ["refusals"]
    for cap, mg, n_keys, n_msgs, m, n_grp, go, gm, ao in CASES:
        lines.append("plan %d %d %d %d %d %d %s %s %s" % (cap, mg, n_keys, n_msgs, m, n_grp, tab(go), tab(gm), tab(ao)))
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module", params=sorted(BUILDS))
def out(request, tmp_path_factory):
    """the program's output lines, from the plain and from the sanitizer build"""
    d = tmp_path_factory.mktemp("veragg_" + request.param)
    src, exe = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, *BUILDS[request.param], "-o", str(exe), str(src)])
    res = subprocess.run([str(exe)], input=case_lines(), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
    return iter(res.stdout.split("\n")[:-1])


def test_against_the_model_and_the_invariants(out):
    for r in range(7):
        code, text = next(out).split("|")
        assert (int(code), text) == M.REFUSALS[r]
    refused = []
    for cap, mg, n_keys, n_msgs, m, n_grp, go, gm, ao in CASES:
        got = [int(x) for x in next(out).split()]
        assert got == M.plan(go, gm, ao, n_keys, n_msgs, cap, mg, m=m, n_grp=n_grp), (cap, go[:8], gm[:8], ao[:8])
        if got[0] == M.OK:
            M.check_invariants(got, gm, ao)
        else:
            refused.append(tuple(got))
    assert refused == REFUSED
    assert next(out, None) is None


def test_the_model_alone():
    """the rules on the model, with the numbers written out"""
    go, gm, ao, n_keys, n_msgs = build([[(0, 1), (1, 1)], [(2, 1), (3, 1)], [(i, 1) for i in range(6)]])
    assert ao == [0, 2, 4, 10] and M.slots(ao) == [0, 3, 6, 13]
    assert M.sources(gm, ao)[:4] == [(M.SIG, 0, 0), (0, 0, 0), (1, 1, 0), (M.SIG, 1, 1)]
    # aggregates of 3, 3 and 7 pairs: a cap of 5 takes them one by one (the last one past the cap, alone), 6 the first two
    assert M.slices(ao, 5) == [(0, 1, 0, 3), (1, 1, 3, 3), (2, 1, 6, 7)]
    assert M.slices(ao, 6) == [(0, 2, 0, 6), (2, 1, 6, 7)] and M.slices(ao, 12) == M.slices(ao, 6)
    assert M.slices(ao, 13) == [(0, 3, 0, 13)] and M.slices(ao, 1) == M.slices(ao, 5)
    # the workspace of that call, unsliced: 10 sums, 10 flags, 6 hashed points, 3 undecided bytes, 13 pairs, 3 results
    nums = M.plan(go, gm, ao, n_keys, n_msgs)
    assert nums[14:21] == [0, 1024, 1280, 2560, 2816, 4096, 6656] and nums[21] == 6656 + 1792
    M.check_invariants(nums, gm, ao)
    # an aggregate without groups is one pair; tables that begin past zero leave what lies before them to nobody
    assert M.slots([0, 0, 0]) == [0, 1, 2] and M.slots([2, 3, 5]) == [0, 2, 5]
    assert M.validate([0, 2, 1, 6], [0, 1, 0], [0, 1, 3], 2, 3, 6, 2) == (M.GRP_OFF_DOWN, 1)
    assert M.validate([0, 2, 4, 6], [0, 1, 0], [0, 1, 2], 2, 3, 6, 2) == (M.AGG_OFF_END, 2)
    assert M.validate([0, 2, 4, 6], [0, 2, 5], [0, 1, 3], 2, 3, 6, 2) == (M.BAD_MSG, 1)
