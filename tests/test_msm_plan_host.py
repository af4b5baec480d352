"""The host plan of the G1 / G2 sums, csrc/msm_plan.h (the knobs, the order of the kernel families, one plan per family: window
bits, chunks, fold levels, grids and the layout of the two shared buffers), compiled for the host as a stand-alone program -- once
with -O2, once under AddressSanitizer and UBSan -- and compared word for word with tests/msm_plan_model.py, which states what
msm_dev did before the header existed.  The invariants below hold for every plan whatever the model says, and the mutants show
that the grid of cases tells a wrong model from the right one."""
import os
import subprocess

import pytest

import msm_plan_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")

# first line: `consts` -> the values of msm::GFX950; then one case per line: deg scalars k groups and the 16 knobs in the order of
# msm_plan_model.KNOBS -> `too_large`, or one line per route asked (its name and the numbers of its plan) and `end`
HOST_TEST = r'''
#include "msm_plan.h"
#include <stdio.h>
#include <iostream>
#include <sstream>
#include <string>
static void put(size_t v) { printf(" %zu", v); }
static void put_folds(const msm::Fold* f, int n) {
    put((size_t)n);
    for (int i = 0; i < n; i++)
        for (size_t v : {(size_t)f[i].kernel, f[i].cur, f[i].nfold, f[i].ftotal, (size_t)f[i].npts, (size_t)f[i].last, (size_t)f[i].grid, f[i].src, f[i].dst}) put(v);
}
int main() {
    const msm::Consts K = msm::GFX950;
    static const char* const NAMES[] = {"EMPTY", "PLAIN", "SMALL_GROUPS", "SORTED", "BUCKET_VM", "BUCKET_LANE", "VM"};
    static_assert(sizeof(NAMES) / sizeof(NAMES[0]) == msm::END, "a route without a name");
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line == "consts") {
            printf("consts");
            for (size_t v : {K.srt_lanes, K.srt_scw, K.srt_bitadds, K.srt_maxbits, K.srt_slice, K.smul_t, K.pip_w, K.pip_nb, K.l28_aff, K.l28_pj,
                             K.msm_waves, K.hmsm2_np, K.np[0], K.np[1], K.lp[0], K.lp[1], K.aff[0], K.aff[1], K.pj[0], K.pj[1]}) put(v);
            printf("\n");
            continue;
        }
        std::istringstream in(line);
        int deg, sc;
        size_t k, groups, wide_tail, lane_pairs;
        msm::Knobs c;
        in >> deg >> sc >> k >> groups >> c.pip_threshold >> c.pip_group_threshold >> c.pip_chunks >> c.msm_sort_threshold >> c.msm_sort2_threshold >>
            c.sort_bits >> c.sort2_bits >> c.msm_plain_threshold >> c.smul_min_groups >> c.smul_max_k >> wide_tail >> c.msm_lane_threshold >>
            lane_pairs >> c.horner_np_threshold >> c.horner_quads_threshold >> c.test_slice_cap;
        c.msm_wide_tail = wide_tail != 0, c.msm_lane_pairs = lane_pairs != 0;
        if (msm::too_large(k, groups)) { printf("too_large\n"); continue; }
        bool more = true;
        for (msm::Route r = msm::START; more && (r = msm::next_route(c, deg, k, groups, sc != 0, r)) != msm::END;) {
            printf("%s", NAMES[r]);
            more = false;
            switch (r) {
            case msm::START: case msm::END: case msm::EMPTY: break;
            case msm::PLAIN: {
                const msm::PlainPlan p = msm::plan_plain(K, deg, k);
                for (size_t v : {p.U, p.chunk, p.o_prep, p.o_live, p.o_b0, p.o_b1, p.words, p.src, (size_t)p.last_n, (size_t)p.g_prep, (size_t)p.g_chunks}) put(v);
                put_folds(p.fold, p.nfolds);
                break;
            }
            case msm::SMALL_GROUPS: {
                const msm::SmallPlan p = msm::plan_small_groups(c, K, deg, k, groups);
                for (size_t v : {p.upw, p.slice, p.units0, p.o_prep, p.o_live, p.o_tab, p.words, (groups + p.slice - 1) / p.slice}) put(v);
                for (size_t lo = 0; lo < groups; lo += p.slice) {
                    const msm::SmallSlice s = p.at(lo);
                    for (size_t v : {lo, s.m, s.n, s.units, s.pts, s.scalars, s.out, (size_t)s.g_prep, (size_t)s.g_smul}) put(v);
                }
                more = true;                                   // (its tables may find no room)
                break;
            }
            case msm::SORTED: {
                const msm::SortedPlan p = msm::plan_sorted(c, K, deg, k);
                put(p.bad_bits);
                if (p.bad_bits) break;
                for (size_t v : {(size_t)p.not_me, (size_t)p.cb, (size_t)p.kb, (size_t)p.nwin, p.nkeys}) put(v);
                more = p.not_me;
                if (p.not_me) break;
                for (size_t v : {p.nch, p.nsum, p.units, p.btotal, (size_t)p.wide, (size_t)p.pass5}) put(v);
                for (uint32_t v : p.bias) put(v);
                for (size_t v : {p.o_prep, p.o_rec, p.o_cnt, p.o_start, p.o_cur, p.o_max, p.o_idx, p.o_bsum, p.o_hp, p.o_hk, p.o_b0, p.o_b1, p.o_win, p.o_live,
                                 p.o_wtot, p.o_long, p.words, p.src, (size_t)p.g_prep, (size_t)p.g_slices, (size_t)p.g_accum, (size_t)p.g_fix, (size_t)p.g_bits,
                                 (size_t)p.g_pass5}) put(v);
                put_folds(p.fold, p.nfolds);
                break;
            }
            case msm::BUCKET_VM: case msm::BUCKET_LANE: {
                const msm::BucketPlan p = msm::plan_bucket(c, K, deg, k, groups);
                for (size_t v : {(size_t)p.lane_path, p.n, p.chunk, p.chunks, p.fold_n, p.part_words, p.o_win, p.o_prep, p.o_live, p.bucket_words, p.o_fold,
                                 p.lanes, p.ftotal, p.wchunks, (size_t)p.pairs, (size_t)p.lane_last, (size_t)p.tail, (size_t)p.g_prep, (size_t)p.g_lane,
                                 (size_t)p.g_fold, (size_t)p.g_np, p.quad_waves}) put(v);
                break;
            }
            case msm::VM: {
                const msm::VmPlan p = msm::plan_vm(K, deg, k, groups);
                for (size_t v : {p.chunk, p.bpg, p.blocks, p.words, p.fblocks}) put(v);
                break;
            }
            }
            printf("\n");
        }
        printf("end\n");
    }
    return 0;
}
'''

BUILDS = {"O2": ["-O2"], "sanitizers": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}

BIG = 1 << 40
FIXED_WINDOW = dict(msm_sort_threshold=BIG, msm_sort2_threshold=BIG, msm_plain_threshold=BIG, smul_min_groups=BIG)
# default knobs, and every setting the device tests and tools/*probe*.py use
SETTINGS = [{}, FIXED_WINDOW,
            dict(FIXED_WINDOW, pip_threshold=1, pip_group_threshold=1),
            dict(FIXED_WINDOW, pip_threshold=1, pip_group_threshold=1, msm_lane_threshold=1),
            dict(FIXED_WINDOW, pip_threshold=1, pip_group_threshold=1, msm_lane_threshold=1, msm_lane_pairs=0),
            dict(FIXED_WINDOW, pip_threshold=1, pip_group_threshold=1, msm_lane_threshold=1, pip_chunks=97),
            dict(FIXED_WINDOW, pip_threshold=1, pip_group_threshold=1, pip_chunks=97),
            dict(FIXED_WINDOW, pip_group_threshold=1, horner_np_threshold=1),
            dict(pip_threshold=1, pip_group_threshold=1, msm_lane_threshold=1, horner_np_threshold=1, horner_quads_threshold=10 ** 9,
                 msm_sort_threshold=BIG, msm_sort2_threshold=BIG),
            dict(msm_lane_threshold=1), dict(msm_lane_pairs=0), dict(pip_group_threshold=2), dict(msm_wide_tail=0), dict(msm_wide_tail=0, sort_bits=5),
            dict(smul_min_groups=1), dict(smul_min_groups=2), dict(smul_min_groups=2, test_slice_cap=1), dict(pip_chunks=97)]
SETTINGS += [dict(sort_bits=b, sort2_bits=b) for b in range(4, 16)]
SETTINGS += [dict(test_slice_cap=cap) for cap in (1, 3, 64)]
GROUPS = [1, 2, 3, 47, 48, 4095, 4096, 65535, 65536]
KS = [0, 1, 2, 8, 9, 47, 48, 511, 512, 4095, 4096, 16383, 16384, 65535, 65536, 1 << 20]
CASES = [(M.knobs(**s), deg, k, groups, sc) for s in SETTINGS for deg in (1, 2) for sc in (1, 0) for groups in GROUPS for k in KS]
# the sizes at which SORTED answers "not me": 20 windows (13 bits) x n over 2^32 - 16, and n = 2^31
CASES += [(M.knobs(), deg, k, 1, 1) for deg in (1, 2) for k in (214748364, 214748365, (1 << 31) - 1)]
CASES += [(M.knobs(sort_bits=14, sort2_bits=14), deg, k, 1, 1) for deg in (1, 2) for k in (226050909, 226050910, 226050911)]


def case_line(c, deg, k, groups, sc):
    return " ".join(map(str, [deg, sc, k, groups] + [int(c[name]) for name in M.KNOBS]))


@pytest.fixture(scope="module", params=sorted(BUILDS))
def out(request, tmp_path_factory):
    """the program's output lines, from the plain and from the sanitizer build"""
    d = tmp_path_factory.mktemp("msm_plan_" + request.param)
    src, exe = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, *BUILDS[request.param], "-o", str(exe), str(src)])
    res = subprocess.run([str(exe)], input="consts\n" + "".join(case_line(*c) + "\n" for c in CASES), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
    return res.stdout.split("\n")[:-1]


def answers(out):
    """the lines of each case"""
    it = iter(out[1:])
    res = []
    for _ in CASES:
        got = []
        for line in it:
            got.append(line)
            if line in ("end", "too_large"):
                break
        res.append(got)
    assert next(it, None) is None
    return res


def test_against_the_model(out):
    assert out[0].split() == ["consts"] + [str(v) for v in M.CONSTS]
    got = answers(out)
    seen = set()
    for case, lines in zip(CASES, got):
        assert lines == M.lines(*case), case
        seen.update(line.split()[0] for line in lines)
    # every route, the refusal, both "not me" answers and the refused window bits occur in the grid
    assert seen == set(M.ROUTES) | {"end", "too_large"}
    assert any(ls[0].startswith("SORTED 0 1") for ls in got) and any(ls[0] == "SORTED 1" for ls in got)
    assert any(ls[0].startswith("SMALL_GROUPS") and len(ls) == 3 for ls in got)


def regions(p, names):
    """[(offset, size)] of the named regions"""
    return [(p[x], p["sizes"][x]) for x in names]


def check_regions(regs, total, unit):
    at = 0
    for off, size in regs:
        assert off >= at and off % unit == 0, (regs, total)
        at = off + size
    assert at <= total


def fits32(*values):
    assert all(0 <= v < 1 << 32 for v in values), values


def check_folds(p, ends_at):
    a, b = p["o_b0"], p["o_b1"]
    src = p["o_b1"] if p.get("pass5") else a
    for f in p["folds"]:
        assert f["src"] == src and f["dst"] == (b if src == a else a) and f["nfold"] == M.cdiv(f["cur"], 8)
        assert 0 < f["grid"] < 1 << 31
        fits32(f["cur"], f["nfold"], f["ftotal"], f["npts"])
        if f["kernel"] == M.HORNER_WIDE:
            assert f["npts"] == min(f["cur"], 8) and (f["cur"] <= 8 or f["cur"] % 8 == 0) and f["grid"] == f["ftotal"] <= 4096
        src = f["dst"]
    for f, g in zip(p["folds"], p["folds"][1:]):
        assert g["cur"] == f["nfold"]
    assert p["src"] == src
    last = p["folds"][-1]["nfold"] if p["folds"] else None
    assert ends_at(last)


def check_plan(c, deg, k, groups, route, p):
    """what must hold of a plan whatever the model says (the numbers are the model's, which the header equals word for word)"""
    n = k * groups
    if route == "SORTED":
        pinned = c["sort_bits"] if deg == 1 else c["sort2_bits"]
        assert p["bad_bits"] == int(pinned != 0 and not 5 <= pinned <= 14)
        if p["bad_bits"]:
            return
        assert 258 <= p["cb"] * p["nwin"] and p["nkeys"] == p["nwin"] << p["kb"] and p["kb"] == p["cb"] - 1
        assert p["not_me"] == int(p["nwin"] * k > 0xFFFFFFF0 or k >= 1 << 31)
        if p["not_me"]:
            return
        check_regions(regions(p, M.SORTED_OFFSETS[:-1]), p["words"], 4)
        assert p["bias_rest"] == 0 and sum(bin(w).count("1") for w in p["bias"]) == p["nwin"]
        check_folds(p, lambda last: last == 1 if p["nch"] > 1 else last is None)
        assert p["pass5"] == int(p["nch"] == 1 and not p["wide"])
        if p["folds"] and not p["wide"]:
            assert [f["last"] for f in p["folds"]] == [0] * (len(p["folds"]) - 1) + [1]
        fits32(k, p["nkeys"], p["units"], p["btotal"], p["nsum"], p["nwin"] * k)
        for g in ("g_prep", "g_slices", "g_accum", "g_fix", "g_bits"):
            assert 0 < p[g] < 1 << 31
        assert p["nwin"] <= 65535                                                        # the y of the count and scatter grids
        assert p["sizes"]["o_b1"] >= max([f["ftotal"] for f in p["folds"][0::2]] + [p["nsum"] if p["pass5"] else 0]) * M.PJ[deg]
        assert p["sizes"]["o_b0"] >= max([f["ftotal"] for f in p["folds"][1::2]] + [p["btotal"]]) * M.PJ[deg]
    elif route == "PLAIN":
        check_regions(regions(p, ("o_prep", "o_live", "o_b0", "o_b1")), p["words"], 4)
        check_folds(p, lambda last: last is None or last <= 8)
        assert 1 <= p["last_n"] <= 8 and p["U"] * p["chunk"] >= k > (p["U"] - 1) * p["chunk"] and p["U"] <= M.SRT_LANES // M.LP[deg]
        fits32(k, p["chunk"], p["U"])
        assert 0 < p["g_prep"] < 1 << 31 and 0 < p["g_chunks"] < 1 << 31
        assert p["sizes"]["o_b1"] >= max([f["nfold"] for f in p["folds"][0::2]] + [0]) * M.PJ[deg]
    elif route == "SMALL_GROUPS":
        check_regions(regions(p, ("o_prep", "o_live", "o_tab")), p["words"], 4)
        ss = p["slices"]
        assert ss[0]["lo"] == 0 and all(a["lo"] + a["m"] == b["lo"] for a, b in zip(ss, ss[1:])) and ss[-1]["lo"] + ss[-1]["m"] == groups
        table = p["units0"] * k * M.SMUL_T * M.PJ[deg] * 4
        assert table <= 2 << 30 or p["units0"] == p["upw"]                               # 2 GB, unless one wavefront's worth exceeds it
        for s in ss:
            assert 0 < s["m"] <= p["slice"] and s["m"] <= s["units"] <= p["units0"] and s["units"] % p["upw"] == 0 and s["n"] == k * s["m"] <= k * p["slice"]
            assert 0 < s["g_prep"] < 1 << 31 and 0 < s["g_smul"] < 1 << 31 and s["g_smul"] * 64 == s["units"] * M.LP[deg]
            fits32(s["n"], s["m"], k)
    elif route in ("BUCKET_VM", "BUCKET_LANE"):
        assert (route == "BUCKET_LANE") == bool(p["lane_path"]) and p["n"] == n
        assert p["chunk"] * p["chunks"] >= k > p["chunk"] * (p["chunks"] - 1)
        pj28 = M.L28_PJ * deg
        prep = n * M.L28_AFF * deg + M.cdiv(n, 4) if p["lane_path"] else n * 36 * deg
        check_regions([(0, p["chunks"] * groups * M.PIP_W * pj28), (p["o_win"], groups * M.PIP_W * pj28), (p["o_prep"], prep)], p["part_words"], 1)
        assert p["o_live"] == p["o_prep"] + n * M.L28_AFF * deg
        fits32(n, k, p["chunk"], p["chunks"], p["lanes"], p["fold_n"], p["ftotal"], p["wchunks"], groups)
        assert groups <= 65535 and 0 < p["g_prep"] < 1 << 31 and 0 < p["g_np"] < 1 << 31
        if p["lane_path"]:
            check_regions([(0, p["lanes"] * (M.PIP_NB - 1) * pj28), (p["o_fold"], p["fold_n"] * groups * M.PIP_W * 36 * deg)], p["words"], 1)
            assert (p["fold_n"] > 0) == (p["chunks"] > 96) and p["fold_n"] * 64 >= p["chunks"] * bool(p["fold_n"])
            assert p["wchunks"] == (p["fold_n"] or p["chunks"]) and 0 < p["g_lane"] < 1 << 31
            assert p["lane_last"] == int(not p["fold_n"] and p["tail"] != M.T_QUADS)
            assert p["tail"] != M.T_QUADS or (deg == 2 and p["pairs"] and p["chunks"] == 1)
        else:
            assert p["chunk"] % M.NP[deg] == 0 and p["chunks"] <= 65535 and p["tail"] != M.T_QUADS and p["words"] == 0   # (x of k_msm_pip's grid)
    elif route == "VM":
        assert p["chunk"] * p["bpg"] >= k > p["chunk"] * (p["bpg"] - 1) and p["blocks"] == p["bpg"] * groups
        assert p["part_words"] == p["blocks"] * 36 * deg and 0 < p["blocks"] < 1 << 31 and 0 < p["fblocks"] < 1 << 31
        fits32(k, p["chunk"], p["bpg"], groups)


def test_invariants_of_every_plan(out):
    assert out[0].split()[1:] == [str(v) for v in M.CONSTS]                              # (the numbers below are the header's: test_against_the_model)
    for c, deg, k, groups, sc in CASES:
        r = M.msm_dev(c, deg, k, groups, sc)
        if r == "too_large":
            assert k > 0x7FFFFFFF or groups > 0x7FFFFFFF or k * groups > 0xFFFFFFF0
            continue
        for route, p in r:
            check_plan(c, deg, k, groups, route, p)


def test_every_route_has_a_case(out):
    """a Route value the header gains must be named by the program (its static_assert), printed by it and met by the grid"""
    got = answers(out)
    met = {line.split()[0] for lines in got for line in lines} - {"end", "too_large"}
    assert met == set(M.ROUTES)


# ---- mutants: the model with one thing wrong; each must differ from the right model somewhere on the grid
def _mutant(name):
    import types
    m = types.ModuleType("mutant")
    with open(M.__file__) as f:
        src = f.read()
    a, b = MUTANTS[name]
    assert src.count(a) == 1, (name, src.count(a))
    exec(compile(src.replace(a, b), M.__file__, "exec"), m.__dict__)
    return m


MUTANTS = {
    "plain threshold strict": ('k >= c["msm_plain_threshold"]', 'k > c["msm_plain_threshold"]'),
    "small groups k strict": ('k <= c["smul_max_k"]', 'k < c["smul_max_k"]'),
    "pip group threshold strict": ('k >= c["pip_group_threshold"])', 'k > c["pip_group_threshold"])'),
    "groups 65535 excluded": ("1 < groups <= 65535", "1 < groups < 65535"),
    "cb for kb": ("nkeys = nwin << kb", "nkeys = nwin << cb"),
    "dropped + PJ": ("nsum * cdiv(nch, 8) * pj + pj", "nsum * cdiv(nch, 8) * pj"),
    "fold_n at 96": ("lane_path and chunks > 96", "lane_path and chunks >= 96"),
    "unrounded VM bucket chunk": ("        chunk = cdiv(chunk, NP[deg]) * NP[deg]\n    if chunk == 0", "        pass\n    if chunk == 0"),
    "7-bit windows below 513": ("7 if n < 512 else 13", "7 if n <= 512 else 13"),
    "wide fold at any run count": ("wide and ftotal <= 4096 and", "wide and"),
    "lane threshold strict": ('n >= c["msm_lane_threshold"]', 'n > c["msm_lane_threshold"]'),
    "slice not capped": ("    slice_ = slice_len(c, slice_, upw)\n", ""),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_the_grid_catches_a_wrong_model(name):
    m = _mutant(name)
    assert any(m.lines(*case) != M.lines(*case) for case in CASES), name
