"""The host plan of the ragged secure aggregation, csrc/secure_ranges_plan.h (the refusals, the validation of the offset tables,
the grids, the workspace, the cut of a host-buffer call into staged slices on group boundaries), compiled for the host as a
stand-alone program -- once with -O2, once under AddressSanitizer and UBSan, the offset tables in heap blocks of exactly their
length -- and compared with tests/secure_ranges_model.py over a few hundred seeded tables."""
import os
import random
import subprocess

import pytest

import secure_ranges_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")

# one case per line
#   large n_keys n_exp groups                          -> 0 | 1
#   grids groups n_exp                                 -> check digest exp
#   ws groups n_exp own_digests own_exps pair_table    -> head digests exps pairs total
#   fixed k m groups                                   -> too large, too large for the private keys, digests exps total
#   cap test_slice_cap                                 -> items per slice
#   validate count groups off[groups + 1]              -> verdict where
#   cut test_slice_cap has_pk groups [pk_off[groups + 1]] exp_off[groups + 1]
#                                                      -> lo hi lo hi .. : most groups, keys, exponents : the rebased tables of the last slice
HOST_TEST = r'''
#include "secure_ranges_plan.h"
#include <stdio.h>
#include <iostream>
#include <sstream>
#include <string>
namespace sr = secure_ranges;
// a heap block of exactly n values
static uint32_t* some(std::istream& in, size_t n) { uint32_t* v = new uint32_t[n]; for (size_t i = 0; i < n; i++) in >> v[i]; return v; }
int main() {
    std::string line, op;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        in >> op;
        if (op == "large") { uint64_t a, b, g; in >> a >> b >> g; printf("%d\n", sr::too_large(a, b, g) ? 1 : 0); }
        else if (op == "grids") {
            size_t groups, n_exp;
            in >> groups >> n_exp;
            const sr::Grids g = sr::grids(groups, n_exp);
            printf("%u %u %u\n", g.check, g.digest, g.exp);
        } else if (op == "ws") {
            size_t groups, n_exp; int a, b, c;
            in >> groups >> n_exp >> a >> b >> c;
            const sr::Workspace w = sr::workspace(groups, n_exp, a != 0, b != 0, c != 0);
            printf("%zu %zu %zu %zu %zu\n", w.head, w.digests, w.exps, w.pairs, w.total);
        } else if (op == "fixed") {
            size_t k, m, groups;
            in >> k >> m >> groups;
            const sr::FixedWorkspace w = sr::fixed_workspace(m, groups);
            printf("%d %d %zu %zu %zu\n", sr::fixed_too_large(k, m, groups) ? 1 : 0, sr::fixed_priv_too_large(k, groups) ? 1 : 0, w.digests, w.exps, w.total);
        } else if (op == "cap") {
            msm::Knobs k;
            in >> k.test_slice_cap;
            printf("%zu\n", sr::slice_cap(k));
        } else if (op == "validate") {
            uint64_t count; size_t groups;
            in >> count >> groups;
            uint32_t* off = groups ? some(in, groups + 1) : nullptr;
            size_t at = 77;
            const sr::Verdict v = sr::validate(off, groups, count, &at);
            if (sr::validate(off, groups, count) != v || (v != sr::OK) != (sr::verdict_text(v)[0] != 0)) return 3;
            printf("%d %zu\n", (int)v, at);
            delete[] off;
        } else if (op == "cut") {
            msm::Knobs k; int has_pk; size_t groups;
            in >> k.test_slice_cap >> has_pk >> groups;
            uint32_t* pk_off = has_pk ? some(in, groups + 1) : nullptr;
            uint32_t* exp_off = some(in, groups + 1);
            std::vector<sr::Slice> slices;
            slices.push_back({7, 9});                                        // cut() clears what is there
            sr::cut(pk_off, exp_off, groups, sr::slice_cap(k), slices);
            for (const sr::Slice& s : slices) printf("%zu %zu ", s.lo, s.hi);
            const sr::Extent e = sr::extent(pk_off, exp_off, slices);
            printf(": %zu %zu %zu :", e.groups, e.keys, e.exps);
            if (!slices.empty()) {
                std::vector<uint32_t> t(3, 5u);                              // rebase() resizes
                if (pk_off) { sr::rebase(pk_off, slices.back(), t); for (uint32_t v : t) printf(" %u", v); }
                printf(" |");
                sr::rebase(exp_off, slices.back(), t);
                for (uint32_t v : t) printf(" %u", v);
            }
            printf("\n");
            delete[] pk_off;
            delete[] exp_off;
        }
    }
    return 0;
}
'''

BUILDS = {"O2": ["-O2"], "sanitizers": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}

B31, B30 = 1 << 31, 1 << 30
# totals at the 2^31 bound (keys, exponents) and the 2^30 bound (groups): the last value taken, the first refused
LARGE = [(0, 0, 0), (B31 - 1, B31 - 1, B30 - 1), (B31, 0, 1), (0, B31, 1), (B31 - 1, B31, 1), (5, 5, B30), (5, 5, B30 - 1), (1 << 40, 0, 0),
         (0, (1 << 32) - 1, 3), (B31 - 1, 0, B30)]
GRIDS = [(0, 0), (1, 0), (1, 1), (64, 256), (65, 257), (255, 511), (256, 512), (257, 513), (70, 1000)]
WS = [(g, x, a, b, c) for g, x in ((1, 0), (8, 8), (9, 7), (65, 400), (70, 0)) for a, b, c in ((0, 0, 0), (1, 0, 0), (1, 1, 1), (0, 1, 1))]
CAPS = [0, 1, 3, 64, 1 << 18, 1 << 19]
# the fixed-shape forms (k keys, m exponents a group): layouts with 7, 8 and 9 digests (256 bytes are eight) and without
# exponents of its own (m = 0: blsgpu_hash_pks_dev), and on every term of the bound the last value taken and the first refused
K58 = ((1 << 64) - 1) >> 6
FIXED = [(1, 0, 1), (3, 3, 7), (3, 3, 8), (67, 67, 9), (2, 5, 1000), (1, 1, B31 - 1), (1, 1, B31), (1, (1 << 32) - 1, 1), (1, 1 << 32, 1),
         (1, 2, 0x7FFFFFF8), (1, 2, 0x7FFFFFF9), (K58 // 3, 1, 3), (K58 // 3 + 1, 1, 3), (1024, 1024, 4194303), (1024, 1024, 4194304),
         (2, 1, 0x7FFFFFF8), (2, 1, 0x7FFFFFF9)]

# (offsets, count) the header takes ...
GOOD = [([0, 0], 0), ([0, 5], 5), ([0, 5], 9), ([0, 0, 0, 0], 0), ([0, 1, 1, 70, 200], 200), ([0, B31 - 1], B31 - 1), ([0, 3, 3, 3, 10], 11)]
# ... and refuses: a step down, a first offset that is not 0 (whatever follows), a last offset past the buffer
BAD = [([0, 10, 9, 20], 20), ([0, 4, 3], 100), ([1, 1], 5), ([3, 2, 1], 0), ([7, 7], 7), ([0, 10, 20], 19), ([0, 0, 1], 0),
       ([0, 5, 4, 100], 50), ([0, (1 << 32) - 1], B31)]
BAD_VERDICTS = [M.DECREASING, M.DECREASING, M.FIRST_NOT_ZERO, M.FIRST_NOT_ZERO, M.FIRST_NOT_ZERO, M.PAST_END, M.PAST_END, M.DECREASING,
                M.PAST_END]


def seeded_tables():
    """a few hundred tables of random group lengths with runs of empty groups and lone long ones; some damaged: one step turned
    down, the first offset moved, the count set below the last offset"""
    rng = random.Random(20240611)
    out = []
    for t in range(240):
        groups = rng.choice([1, 2, 3, 7, 64, 65, 70])
        lens = [rng.choice([0, 0, 1, 2, 3, 4, 5, 7, 8, 9, 67, rng.randrange(300)]) for _ in range(groups)]
        off = M.offsets(lens)
        count = off[-1] + rng.choice([0, 0, 3])
        kind = t % 4
        if kind == 1:
            i = next((i for i in range(1, groups) if off[i] > 0), None)    # an interior offset above 0: its successor goes below it
            if i is not None:
                off[i + 1] = off[i] - 1
        elif kind == 2:
            off[0] = rng.choice([1, 5])
        elif kind == 3 and off[-1]:
            count = off[-1] - 1
        out.append((off, count))
    return out


SEEDED = seeded_tables()
VALIDATE = GOOD + BAD + SEEDED


def cut_cases():
    """(test_slice_cap, pk_off | None, exp_off): the caps of the device tests and the natural length, tables with equal and
    with different key and exponent counts, and with the digests handed in (no key table)"""
    rng = random.Random(777)
    fixed = [M.LENGTHS * 7, [0] * 5, [1] * 70, [64, 64, 65, 1, 63, 0, 1, 64], [300], [0, 1000, 0, 3, 3, 0, 0], [2, 1, 0, 0, 0, 0, 3, 3, 3, 4]]
    tables = [(lens, lens) for lens in fixed]
    for _ in range(40):
        groups = rng.choice([1, 2, 5, 33, 70])
        tables.append(([rng.choice([0, 1, 2, 3, 4, 5, 67]) for _ in range(groups)], [rng.choice([0, 1, 2, 3, 9, 70]) for _ in range(groups)]))
    out = []
    for kl, el in tables:
        for cap in (1, 3, 64, 0):
            out.append((cap, M.offsets(kl), M.offsets(el)))
        out.append((3, None, M.offsets(el)))
    return out


CUTS = cut_cases()


def case_lines():
    j = lambda v: " ".join(map(str, v))
    lines = ["large %d %d %d" % v for v in LARGE] + ["grids %d %d" % v for v in GRIDS] + ["ws %d %d %d %d %d" % w for w in WS]
    lines += ["fixed %d %d %d" % v for v in FIXED] + ["cap %d" % c for c in CAPS]
    lines += ["validate %d %d %s" % (count, len(off) - 1, j(off)) for off, count in VALIDATE] + ["validate 9 0"]
    lines += ["cut %d %d %d %s %s" % (cap, pk is not None, len(ex) - 1, j(pk or []), j(ex)) for cap, pk, ex in CUTS]
    return "\n".join(lines) + "\n"


def ints(s):
    return [int(x) for x in s.split()]


@pytest.fixture(scope="module", params=sorted(BUILDS))
def out(request, tmp_path_factory):
    """the program's output lines, from the plain and from the sanitizer build"""
    d = tmp_path_factory.mktemp("secure_ranges_" + request.param)
    src, exe = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, *BUILDS[request.param], "-o", str(exe), str(src)])
    res = subprocess.run([str(exe)], input=case_lines(), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
    return iter(res.stdout.split("\n")[:-1])


def test_against_the_model(out):
    for v in LARGE:
        assert int(next(out)) == int(M.too_large(*v)), v
    for v in GRIDS:
        assert tuple(ints(next(out))) == M.grids(*v)
    for g, x, a, b, c in WS:
        assert tuple(ints(next(out))) == M.workspace(g, x, bool(a), bool(b), bool(c))
    for k, m, g in FIXED:
        assert tuple(ints(next(out))) == (int(M.fixed_too_large(k, m, g)), int(M.fixed_priv_too_large(k, g))) + M.fixed_workspace(m, g), (k, m, g)
    for c in CAPS:
        assert int(next(out)) == M.slice_len(c, M.SLICE_ITEMS)
    for off, count in VALIDATE:
        assert tuple(ints(next(out))) == M.validate(off, count), (off, count)
    assert ints(next(out)) == [M.OK, 0]                                     # no group: nothing is read
    for cap, pk, ex in CUTS:
        left, mid, right = next(out).split(":")
        flat = ints(left)
        slices = list(zip(flat[::2], flat[1::2]))
        assert slices == M.cut(pk, ex, M.slice_len(cap, M.SLICE_ITEMS)), (cap, pk, ex)
        assert tuple(ints(mid)) == M.extent(pk, ex, slices)
        lo, hi = slices[-1]
        pk_part, ex_part = right.split("|")
        assert ints(pk_part) == (M.rebase(pk, lo, hi) if pk is not None else []) and ints(ex_part) == M.rebase(ex, lo, hi)
    assert next(out, None) is None


def test_the_model_alone():
    """the properties the rules are stated in, on the model: the verdicts by construction, the bounds, the slices a partition in
    order with every count within the cap unless the slice is one group, and no slice that its successor's first group would
    still have fitted"""
    assert [M.too_large(*v) for v in LARGE] == [False, False, True, True, True, True, False, True, True, True]
    assert all(M.validate(off, count) == (M.OK, 0) for off, count in GOOD)
    assert [M.validate(off, count)[0] for off, count in BAD] == BAD_VERDICTS
    assert M.validate([0, 10, 9, 20], 20) == (M.DECREASING, 1) and M.validate([0, 10, 20], 19) == (M.PAST_END, 2)
    verdicts = [M.validate(off, count)[0] for off, count in SEEDED]
    assert len(SEEDED) >= 200 and all(verdicts.count(v) >= 20 for v in (M.OK, M.FIRST_NOT_ZERO, M.DECREASING, M.PAST_END))
    for off, count in SEEDED:                                               # the verdict against the definition, not the walk
        v = M.validate(off, count)[0]
        fine = off[0] == 0 and all(a <= b for a, b in zip(off, off[1:])) and off[-1] <= count
        assert (v == M.OK) == fine
    assert [M.slice_len(c, M.SLICE_ITEMS) for c in CAPS] == [1 << 18, 1, 3, 64, 1 << 18, 1 << 18]
    for cap, pk, ex in CUTS:
        cap = M.slice_len(cap, M.SLICE_ITEMS)
        slices = M.cut(pk, ex, cap)
        groups = len(ex) - 1
        assert [lo for lo, _ in slices] == [0] + [hi for _, hi in slices[:-1]] and slices[-1][1] == groups
        count = lambda lo, hi: (hi - lo, pk[hi] - pk[lo] if pk is not None else 0, ex[hi] - ex[lo])
        for k, (lo, hi) in enumerate(slices):
            assert hi > lo and (hi - lo == 1 or max(count(lo, hi)) <= cap)
            if hi < groups:
                assert max(count(lo, hi + 1)) > cap                         # greedy: the next group did not fit
    lens = M.LENGTHS * 7
    assert len(M.cut(M.offsets(lens), M.offsets(lens), 1)) == 70                          # cap 1: a group a slice, the empty ones too
    assert M.cut(M.offsets([2, 1, 0, 3]), M.offsets([2, 1, 0, 3]), 3) == [(0, 3), (3, 4)]
    assert M.workspace(65, 400, True, True, True) == (0, 256, 256 + 2304, 256 + 2304 + 12800, 256 + 2304 + 12800 + 768)
    # (the bound on m alone never decides: m x groups passes 0xFFFFFFF0 first -- both values around 2^32 are refused)
    assert [M.fixed_too_large(*v) for v in FIXED] == [False] * 6 + [True, True, True, False, True, False, True, False, True, False, False]
    assert [M.fixed_priv_too_large(k, g) for k, _, g in FIXED[-4:]] == [False, True, False, True]
    assert M.fixed_workspace(3, 7) == (0, 256, 256 + 672) and M.fixed_workspace(67, 9) == (0, 512, 512 + 9 * 67 * 32) and M.fixed_workspace(0, 1) == (0, 256, 256)
    # the fixed-shape launches are the ragged grids over groups x m exponents
    assert M.grids(9, 9 * 67) == (1, 1, 3)
    import hashlib
    dg, ts = M.hash_pks_ranges(b"", [0, 0], [0, 1])
    assert dg == hashlib.sha256(b"").digest() and int.from_bytes(ts, "big") == int.from_bytes(hashlib.sha256(bytes(4) + dg).digest(), "big") % M.N
