"""The host plan of the pairing path, csrc/pairing_plan.h (the knobs, the Miller kernel and its partials, chunks and merge levels
of the line-stream stage, the levels of the reduce chain, the form of the final exponentiation, buffer sizes and slices),
compiled for the host as a stand-alone program -- once with -O2, once under AddressSanitizer and UBSan -- and compared number
for number with tests/pairing_plan_model.py, which states what blsgpu_api.hip did before the header existed.  The invariants
below hold for every plan whatever the model says, and the mutants show that the grid of cases tells a wrong model from the
right one."""
import os
import subprocess

import pytest

import pairing_plan_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")

# first line: `consts` -> the values of pairing::GFX950, `refusals` -> code and text of each; then one case per line: the 17 knobs
# in the order of pairing_plan_model.KNOBS, the three limits, part_cap, gsz, groups -> one line per plan (pairing_plan_model.lines)
HOST_TEST = r'''
#include "pairing_plan.h"
#include <stdio.h>
#include <iostream>
#include <sstream>
#include <string>
using namespace pairing;
static void put(size_t v) { printf(" %zu", v); }
static void put(const FexpForm& f) { put(f.kind), put(f.waves), put(f.ws_bytes_per_wave); }
static void put(const BatchFinal& f) { put(f.m), put(f.istride), put(f.gstride), put(f.fexp), put(f.blocks); }
int main() {
    const Consts K = GFX950;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line == "consts") {
            printf("consts");
            for (size_t v : {K.lines, K.line_dw, K.dense_dw, K.teams, K.slab_bytes_per_lane, K.mp_g, K.team_bytes, K.mp_team_bytes, K.slow_team_bytes,
                             K.fexp_nslots, K.miller_waves, K.reduce_waves, K.reduce_per_block, K.batch_tree_min_group, K.merge_fan, K.slow_grid}) put(v);
            printf("\n");
            continue;
        }
        if (line == "refusals") {
            for (int r = OK; r <= WORKSPACE_TOO_SMALL; r++) printf("%d %d %s\n", r, refusal_code((Refusal)r), refusal_text((Refusal)r));
            continue;
        }
        std::istringstream in(line);
        Knobs c;
        Limits L;
        size_t fw, vel, mel, mef, nomem, part_cap, gsz, groups;
        in >> c.miller_wide3_max >> c.miller_wide_max >> c.mp_threshold >> c.mp3_threshold >> c.ls_threshold >> c.ls_min_group >> c.ls_teams >>
            c.ls_merge_wide_max >> c.ls_wide_max >> c.ls_quad_max >> c.fexp_team_threshold >> fw >> c.fexp_wide_max_partials >> vel >> mel >> mef >>
            nomem >> L.max_groups >> L.ls_max_pairs >> L.exact_slice >> part_cap >> gsz >> groups;
        c.fexp_wide = fw != 0, c.vm_exact_lanes = vel != 0, c.miller_exact_lanes = mel != 0, c.miller_exact_fast = mef != 0, c.test_ls_nomem = nomem != 0;
        const size_t n = gsz * groups;
        printf("fexp"), put(fexp_form(c, K, gsz, groups)), put(fexp_form(c, K, 1, groups)), printf("\n");
        for (int v = 0; v < 3; v++) {
            if (v == 2 && gsz != 2 && gsz != K.mp_g) continue;
            const MillerPlan p = plan_miller(c, K, gsz, groups, v == 1, v == 2 ? (int)gsz : 0, v != 1, part_cap, part_cap + 2);   // (v == 1: a buffer of the caller's)
            printf("miller");
            for (size_t x : {(size_t)p.kernel, p.per_block, p.bpg, p.blocks, p.pairs, (size_t)p.refusal}) put(x);
            if (!p.refusal)
                for (size_t x : {(size_t)p.grid, (size_t)p.threads, p.lds, p.nv, (size_t)p.exact_lanes, p.lines_bytes, p.bad_bytes, (size_t)p.small_grid}) put(x);
            printf("\n");
        }
        if (gsz >= 1 && n <= 0x3FFFFFF0ull)
            for (int v = 0; v < 2; v++) {
                const LsPlan p = plan_ls(c, K, gsz, groups, v == 1, v == 0);
                printf("ls");
                for (size_t x : {p.n, p.chunk, p.cpg, (size_t)p.small, p.lines_bytes, p.lsp0_bytes, p.lsp1_bytes, p.bad_bytes, p.degen_bytes, (size_t)p.chain,
                                 (size_t)p.chain_grid, p.chain_waves, p.small_waves, p.accum_teams, p.accum_waves, (size_t)p.nmerges}) put(x);
                for (int i = 0; i < p.nmerges; i++)
                    for (size_t x : {p.merge[i].cpg, p.merge[i].cpo, p.merge[i].teams, p.merge[i].waves, (size_t)p.merge[i].wide, (size_t)p.merge[i].src,
                                     (size_t)p.merge[i].dst}) put(x);
                put((size_t)p.last), put((size_t)p.fuse), printf("\n");
            }
        for (int v = 0; v < 3; v++) {
            const ReducePlan p = v < 2 ? plan_reduce(c, K, gsz, groups, 1, gsz, v == 0, true, part_cap) : plan_reduce(c, K, gsz, groups, groups, 1, true, false, part_cap);
            printf("reduce"), put((size_t)p.refusal);
            if (!p.refusal) {
                put((size_t)p.nlevels);
                for (int i = 0; i < p.nlevels; i++)
                    for (size_t x : {p.level[i].blocks, p.level[i].m, p.level[i].istride, p.level[i].gstride, (size_t)p.level[i].dst,
                                     (size_t)p.level[i].final_flag, (size_t)p.level[i].timer}) put(x);
                put((size_t)p.end), put(p.fexp);
                for (size_t x : {(size_t)p.fsrc, p.fm, p.fistride, p.fgstride, p.lds}) put(x);
            }
            printf("\n");
        }
        for (int v = 0; v < 2; v++) {
            const GroupedPlan p = plan_grouped(c, K, L, gsz, groups, v == 0, v == 1);
            printf("grouped");
            for (size_t x : {p.outer, p.partials, (size_t)p.ls, p.per, p.runs, p.run_len, (size_t)p.direct, p.ls_bpg, p.vm_bpg}) put(x);
            printf("\n");
        }
        {
            const BatchPlan p = plan_batch(c, K, L, gsz, groups);
            printf("batch"), put((size_t)p.route), put((size_t)p.fallback), put(p.partials), put(p.n), put(p.fin), put(p.fallback_fin), printf("\n");
        }
        {
            const ExactPlan p = plan_exact(K, L, gsz);
            printf("exact");
            for (size_t x : {p.n, p.slice, p.m0, p.partials, p.exflags_bytes, p.lines_bytes, p.bad_bytes, p.degen_bytes, (size_t)p.vm_grid}) put(x);
            const size_t slices = cdiv(p.n, p.slice);
            put(slices > 8 ? 7 : slices);
            for (size_t i = 0; i < slices; i++) {
                if (slices > 8 && i >= 4 && i + 3 < slices) continue;            // many slices: the first four and the last three
                const ExactSlice s = p.at(i * p.slice);
                for (size_t x : {i * p.slice, s.m, (size_t)s.g_flags, (size_t)s.g_fixup, (size_t)s.g_list, (size_t)s.g_bytes, s.small_waves}) put(x);
            }
            printf("\n");
        }
        {
            const ReservePlan p = plan_reserve(c, K, L, gsz);
            printf("reserve");
            for (size_t x : {p.partials, (size_t)p.ls, p.lines_bytes, p.bad_bytes, p.degen_bytes, p.lsp0_bytes, p.lsp1_bytes}) put(x);
            printf("\n");
        }
        printf("end\n");
    }
    return 0;
}
'''

BUILDS = {"O2": ["-O2"], "sanitizers": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}

BIG = 1 << 40
# default knobs, and every setting tests/test_gpu_alternate_forms.py, test_gpu_miller_wide.py, test_gpu_slices.py and
# tools/*probe*.py / *sweep*.py use (environment variables and blsgpu_ctx_set_* calls)
SETTINGS = [{}, dict(ls_wide_max=0, ls_quad_max=0), dict(ls_wide_max=0), dict(ls_merge_wide_max=0), dict(vm_exact_lanes=0), dict(miller_wide3_max=0),
            dict(miller_wide_max=0), dict(test_ls_nomem=1), dict(fexp_wide=0), dict(miller_exact_lanes=0), dict(miller_exact_fast=0),
            dict(ls_threshold=1, ls_min_group=1), dict(ls_threshold=1, ls_min_group=64), dict(ls_threshold=1, ls_min_group=2),
            dict(ls_threshold=1, ls_min_group=1, ls_wide_max=0, ls_quad_max=0), dict(ls_threshold=1, ls_min_group=1, ls_merge_wide_max=0),
            dict(ls_threshold=M.NEVER), dict(ls_threshold=16384), dict(fexp_team_threshold=1), dict(fexp_team_threshold=M.NEVER),
            dict(miller_wide_max=1 << 30), dict(miller_wide_max=1 << 30, mp_threshold=BIG), dict(mp_threshold=0), dict(mp_threshold=BIG),
            dict(mp_threshold=0, mp3_threshold=0), dict(mp_threshold=0, mp3_threshold=BIG), dict(ls_threshold=M.NEVER, mp3_threshold=10000),
            dict(ls_teams=40960), dict(ls_teams=1), dict(ls_wide_max=1 << 30)]
GSZ = [0, 1, 2, 3, 4, 15, 16, 17, 23, 24, 63, 64, 65, 127, 128, 2303, 2304, 4095, 4096, 8704, 8705, 9728, 11264, 14336, 18432, 20480, 65536,
       1 << 20, (1 << 20) + 1]
GROUPS = [1, 2, 3, 7, 8, 9, 64, 5119, 5120, 32768, 32769, 65535, 65536]
LIMITS = [M.LITERALS, (5, 5, 5)]
ROOMY = 1 << 50                                              # a workspace that refuses nothing
CASES = [(M.knobs(**s), L, ROOMY, gsz, groups) for s in SETTINGS for L in LIMITS for gsz in GSZ for groups in GROUPS]
# the refusals: a workspace of 1000 partials (and 1002 work-list entries), one that holds a reduce level but no Miller block, none
CASES += [(M.knobs(**s), M.LITERALS, cap, gsz, groups) for s in ({}, dict(fexp_wide=0, fexp_team_threshold=M.NEVER)) for cap in (1000, 8, 0)
          for gsz in GSZ for groups in GROUPS]
# the device cases of tests/test_gpu_slices.py
SLICED = M.knobs(ls_threshold=1, ls_min_group=2)
CASES += [(SLICED, (5, 5, 5), ROOMY, gsz, groups) for gsz, groups in [(23, 1), (20, 1), (6, 1), (5, 1), (2, 7), (1, 23), (7, 3), (24, 2), (1, 20), (1, 6), (1, 5)]]


def case_line(c, L, part_cap, gsz, groups):
    return " ".join(map(str, [int(c[name]) for name in M.KNOBS] + list(L) + [part_cap, gsz, groups]))


@pytest.fixture(scope="module", params=sorted(BUILDS))
def out(request, tmp_path_factory):
    """the program's output lines, from the plain and from the sanitizer build"""
    d = tmp_path_factory.mktemp("pairing_plan_" + request.param)
    src, exe = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, *BUILDS[request.param], "-o", str(exe), str(src)])
    res = subprocess.run([str(exe)], input="consts\nrefusals\n" + "".join(case_line(*c) + "\n" for c in CASES), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
    return res.stdout.split("\n")[:-1]


HEAD = 1 + len(M.REFUSALS)


def answers(out):
    """the lines of each case, without its `end`"""
    it = iter(out[HEAD:])
    res = []
    for _ in CASES:
        got = []
        for line in it:
            if line == "end":
                break
            got.append(line)
        res.append(got)
    assert next(it, None) is None
    return res


@pytest.fixture(scope="module")
def expected():
    """the model's lines of every case, computed once"""
    return [M.lines(*case) for case in CASES]


def test_against_the_model(out, expected):
    assert out[0].split() == ["consts"] + [str(v) for v in M.CONSTS]
    assert out[1:HEAD] == [("%d %d %s" % (r, code, text)).rstrip(" ") if text else "%d %d " % (r, code) for r, (code, text) in sorted(M.REFUSALS.items())]
    for case, lines, want in zip(CASES, answers(out), expected):
        assert lines == want, case[1:]


def rows(lines, name):
    return [[int(x) for x in line.split()[1:]] for line in lines if line.split()[0] == name]


def test_the_grid_meets_every_form(expected):
    """every kernel, route, mode, ending and refusal occurs"""
    met = {name: set() for name in ("miller", "refusal", "chain", "end", "mode", "route", "fexp", "merge_wide")}
    for lines in expected:
        for r in rows(lines, "miller"):
            met["miller"].add(r[0]), met["refusal"].add(r[5])
        for r in rows(lines, "ls"):
            met["chain"].add(r[9])
            met["merge_wide"].update(r[16 + 7 * i + 4] for i in range(r[15]))
        for r in rows(lines, "reduce"):
            met["refusal"].add(r[0])
            if r[0] == M.OK:
                met["end"].add(r[2 + 7 * r[1]])
        for r in rows(lines, "grouped"):
            met["mode"].add(r[2])
        for r in rows(lines, "batch"):
            met["route"].add(r[0])
        for r in rows(lines, "fexp"):
            met["fexp"].update((r[0], r[3]))
    assert met == dict(miller=set(range(5)), refusal=set(range(6)), chain=set(range(3)), end=set(range(3)), mode=set(range(5)), route=set(range(4)),
                       fexp=set(range(3)), merge_wide={0, 1})


def reduce_outputs(c, bpg, groups, do_final, part_cap):
    """partials each level of the reduce chain writes into the context's buffers"""
    r = M.reduce(c, bpg, groups, 1, bpg, do_final, 1, part_cap)
    assert r[0] == M.OK
    return [r[2 + 7 * i] * groups for i in range(r[1]) if r[2 + 7 * i + 4] in (M.RB_PART0, M.RB_PART1)]


def check_grids(*grids):
    assert all(0 < g < 1 << 31 for g in grids), grids


def check_ls(c, gsz, groups, r):
    n, chunk, cpg, small = r[:4]
    assert n == gsz * groups and chunk * cpg >= gsz > chunk * (cpg - 1)
    check_grids(r[10], r[11], r[12], groups)                 # (k_ml_horner_fexp: a workgroup per group)
    if small:
        return
    assert r[5] >= r[13] * M.DENSE_DW * 4 and r[13] == groups * cpg * M.LINES
    check_grids(r[14])
    levels = [r[16 + 7 * i:23 + 7 * i] for i in range(r[15])]
    cur, src = cpg, 0
    for lcpg, cpo, teams, waves, wide, s, d in levels:
        assert lcpg == cur and cpo == M.cdiv(cur, M.FAN) and s == src and d == 1 - s and teams == groups * cpo * M.LINES
        assert (r[6] if d else r[5]) >= teams * M.DENSE_DW * 4
        check_grids(teams if wide else waves)
        cur, src = cpo, d
    assert cur == 1 and r[-2] == src


def test_invariants_of_every_plan():
    """what must hold of a plan whatever the model says (the numbers are the model's, which the header equals number for number)"""
    for c, L, part_cap, gsz, groups in CASES:
        if part_cap != ROOMY:
            continue
        n = gsz * groups
        # slices tile the call exactly; every slice is planned on its own
        g = M.grouped(c, L, gsz, groups, 1, 0)
        parts = [(gsz, groups)] if not g[0] else [(gsz, min(g[0], groups - g0)) for g0 in range(0, groups, g[0])]
        assert sum(p[1] for p in parts) == groups and all(0 < p[1] <= L[0] for p in parts)
        for gsz_, gn in set(parts):
            for wb in (1, 0):
                outer, partials, mode, per, runs, run_len, direct, ls_bpg, vm_bpg = M.grouped(c, L, gsz_, gn, wb, 1 - wb)
                assert outer == 0 and direct == int(mode == M.LS_WHOLE and not wb)
                bpgs = [vm_bpg]                              # (the VM kernels also take over when the line records find no memory)
                if mode == M.LS_WHOLE:
                    stages = [(gsz_, gn)]
                elif mode == M.LS_GROUP_SLICES:
                    stages = [(gsz_, min(per, gn - g0)) for g0 in range(0, gn, per)]
                    assert per >= 1 and sum(s[1] for s in stages) == gn
                elif mode == M.LS_RUN_SLICES:
                    stages = [(min(run_len, gsz_ - p0), 1) for p0 in range(0, gsz_, run_len)]
                    assert gn == 1 and sum(s[0] for s in stages) == gsz_ and len(stages) == runs == ls_bpg
                else:
                    stages = []
                    assert ls_bpg == 0 and (mode == M.LS_OFF) == (not M.use_ls(c, gsz_, gn))
                if stages:
                    bpgs.append(ls_bpg)
                    assert len(set(stages)) <= 2 and all(a * b <= L[1] for a, b in stages)
                    for a, b in set(stages):
                        check_ls(c, a, b, M.ls(c, a, b, False, bool(wb)))
                for bpg in bpgs:
                    assert partials >= bpg * gn
                    if gn <= 65535:
                        assert all(partials >= o for o in reduce_outputs(c, bpg, gn, wb, partials))
                if gsz_:
                    m = M.miller(c, gsz_, gn, 0, 0, True, partials, partials + 2)
                    assert m[5] == (M.BATCH_TOO_LARGE if m[3] >= 1 << 31 else M.OK)     # (never for want of room)
                    if m[5] == M.OK:
                        check_grids(m[6], m[13] or 1)
        # the batch entry
        b = M.batch(c, L, gsz, groups)
        if b[0] != M.B_TREE:
            assert b[2] >= n and gsz < M.BATCH_TREE_MIN_GROUP      # (one partial per pair at most, and per group only where it has a pair)
            if n and n < 1 << 31:
                m = M.miller(c, gsz, groups, 0, gsz, True, b[2], b[2] + 2) if b[1] == M.B_TEAM_GROUPS else M.miller(c, n, 1, 1, 0, True, b[2], b[2] + 2)
                assert m[5] == M.OK and m[3] <= b[2] and (m[2] == 1 or b[1] == M.B_ONE_PER_BLOCK)
                check_grids(m[6], b[10], b[17])
            if b[0] == M.B_LS_SMALL:
                check_ls(c, gsz, groups, M.ls(c, gsz, groups, False, False))
        # blsgpu_miller_loop_batch: the slices tile n, each within the sizes of the first
        e = M.exact(L, gsz)
        if gsz:
            sl = [e[10 + 7 * i:17 + 7 * i] for i in range(e[9])]
            assert sl[0][0] == 0 and sl[-1][0] + sl[-1][1] == gsz and all(0 < s[1] <= e[2] for s in sl) and e[2] == min(gsz, L[2])
            assert all(a[0] + a[1] == b[0] for a, b in zip(sl, sl[1:])) or len(sl) == 7
            assert e[3] >= e[2] and e[4] == 2 * e[2]
            for s in sl:
                check_grids(*s[2:])
                check_ls(c, 1, s[1], M.ls(c, 1, s[1], True, False))
            assert M.ls(c, 1, e[2], True, False)[4] == e[5]  # (the lane form's line records are the fast form's)


def test_reserve_covers_one_group_at_the_default_knobs():
    c = M.knobs()
    for n in sorted(set(GSZ) | {2305, 5000, 40960, 100000, 163840, 300000, (1 << 20) - 1}):
        r = M.reserve(c, M.LITERALS, n)
        if not M.use_ls(c, n, 1) or n > M.LITERALS[1]:
            continue
        need = M.ls(c, n, 1, False, True)
        assert r[1] == 1 and all(have >= want for have, want in zip(r[2:], [need[4], need[7], need[8], need[5], need[6]])), n


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
    "wide max strict": ('n <= c["miller_wide_max"]', 'n < c["miller_wide_max"]'),
    "wide3 max strict": ('n <= c["miller_wide3_max"]', 'n < c["miller_wide3_max"]'),
    "group rounding + 2": ("pairs_partials((gsz + 3) * groups)", "pairs_partials((gsz + 2) * groups)"),
    "chunk floor 15": ("want = max(want, 16)", "want = max(want, 15)"),
    "fan-in 4": ("BATCH_TREE_MIN_GROUP, FAN, SLOW_GRID = 4, 8, 64, 24, 8, 3072", "BATCH_TREE_MIN_GROUP, FAN, SLOW_GRID = 4, 8, 64, 24, 4, 3072"),
    "hand over whatever the room": (" and groups <= part_cap", ""),
    "per rounded up": ("ls_max_pairs // gsz", "cdiv(ls_max_pairs, gsz)"),
    "whole call strict": ("if gsz * groups <= ls_max_pairs:", "if gsz * groups < ls_max_pairs:"),
    "runs miss the short one": ("len(range(0, gsz, ls_max_pairs))", "gsz // ls_max_pairs"),
    "mp2 schedule edge": ("n <= 8704 or", "n < 8704 or"),
    "tree from 25": ("if gsz >= BATCH_TREE_MIN_GROUP:", "if gsz > BATCH_TREE_MIN_GROUP:"),
    "team groups of four": ("(gsz == 2 or gsz == MP_G)", "(gsz == 2 or gsz == MP_G + 1)"),
    "exact lanes past 65536": ("nv <= 1 << 16", "nv <= 1 << 17"),
    "fexp team with 65 partials": ("and m <= 64", "and m <= 65"),
    "min group strict": ('gsz < c["ls_min_group"]', 'gsz <= c["ls_min_group"]'),
    "exact slice ignored": ("    step = L[2]\n", "    step = 262144\n"),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_the_grid_catches_a_wrong_model(name, expected):
    m = _mutant(name)
    assert any(m.lines(*case) != want for case, want in zip(CASES, expected)), name
