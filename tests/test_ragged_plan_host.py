"""The host plan of the range sums, the ragged multi-scalar sums, the short-scalar multiplications and the signature division,
csrc/ragged_plan.h (the shared refusals, slices, grids and the layout of every workspace), compiled for the host as a
stand-alone program -- once with -O2, once under AddressSanitizer and UBSan -- and compared number for number with
tests/ragged_plan_model.py, which states what blsgpu_api.hip did before the header existed.  The invariants below hold for every
plan whatever the model says, and the mutants show that the grid of cases tells a wrong model from the right one."""
import os
import subprocess
import types

import pytest

import ragged_plan_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")

# one case per line, its kind first; the answer repeats the kind (msmr answers with two lines: heads, body).  Of many slices the
# program prints the first three and the last two (ragged_plan_model.shown).
HOST_TEST = r'''
#include "ragged_plan.h"
#include <stdio.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
static void put(size_t v) { printf(" %zu", v); }
template <class P, class F> static void put_slices(const P& p, size_t items, size_t step, bool one_if_empty, F show) {
    const size_t k = items ? (items + step - 1) / step : (one_if_empty ? 1 : 0);
    put(k);
    for (size_t i = 0; i < k; i++)
        if (k <= 6 || i < 3 || i + 2 >= k) show(p.at(i * step), i * step);
}
int main() {
    const msm::Consts K = msm::GFX950;
    const ragged::Consts R = ragged::GFX950;
    std::string line, kind;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        in >> kind;
        printf("%s", kind.c_str());
        msm::Knobs c;
        int deg;
        size_t n, m;
        if (kind == "consts") {
            for (size_t v : {R.pscan_chunk, R.pscan_mid_threads, R.msmr_chunk, R.msmr_scan_threads}) put(v);
        } else if (kind == "scan") {
            in >> c.test_slice_cap >> deg >> n >> m;
            const ragged::ScanPlan p = ragged::plan_scan(c, K, R, deg, n, m);
            const ragged::ScanWs& w = p.ws;
            for (size_t v : {p.SL, p.S, (size_t)p.single, w.o_prep, w.o_live, w.o_kind, w.o_ct, w.o_cb, w.o_s, w.o_cnt, w.o_carry, w.o_cc, w.bytes, p.o_base,
                             p.o_basec, p.range_bytes, p.begin_total, (size_t)p.g_check, (size_t)p.g_begin, (size_t)p.g_range}) put(v);
            put_slices(p, n, p.SL, true, [&](const ragged::ScanSlice& s, size_t) {
                const ragged::ScanGrids g = ragged::scan_grids(R, s.len);
                for (size_t v : {s.lo, s.len, s.hi, (size_t)s.first, (size_t)s.more, (size_t)s.last, g.chunks, (size_t)g.g_prep, (size_t)g.g_chunks}) put(v);
            });
        } else if (kind == "msmr") {
            uint64_t total;
            in >> c.test_slice_cap >> deg >> n >> m >> total;
            const ragged::MsmrHeads h = ragged::plan_msmr_heads(m);
            printf("heads");
            for (size_t v : {h.h_cnt, h.h_first, h.h_cr, h.words, (size_t)h.g_count}) put(v);
            printf("\nbody");
            const ragged::MsmrBody p = ragged::plan_msmr_body(c, K, R, deg, n, m, total);
            put(p.too_many);
            if (!p.too_many) {
                for (size_t v : {p.total, p.slice, p.units0, p.o_prep, p.o_live, p.o_tab, p.o_part, p.o_bad, p.o_bpre, p.o_table, p.words, (size_t)p.g_fill,
                                 (size_t)p.g_prep, (size_t)p.g_offcurve}) put(v);
                put_slices(p, p.total, p.slice, false, [&](const ragged::MsmrSlice& s, size_t lo) {
                    for (size_t v : {lo, s.k, s.units, s.tab, s.part, s.bad, (size_t)s.g_smul}) put(v);
                });
            }
        } else if (kind == "smul64") {
            size_t n_pts, indexed;
            in >> c.test_slice_cap >> deg >> n_pts >> n >> indexed;
            const ragged::Smul64Plan p = ragged::plan_smul64(c, K, deg, n_pts, n, indexed != 0);
            for (size_t v : {p.S, p.units0, p.np0, p.o_prep, p.o_live, p.o_tab, p.words, (size_t)p.g_prep_all}) put(v);
            put_slices(p, n, p.S, false, [&](const ragged::Smul64Slice& s, size_t lo) {
                for (size_t v : {lo, s.m, s.units, s.pts, s.w, s.out, (size_t)s.g_prep, (size_t)s.g_smul}) put(v);
            });
        } else if (kind == "sigdiv") {
            size_t n_ent;
            in >> n >> m >> n_ent;
            const ragged::SigdivPlan p = ragged::plan_sigdiv(n, m, n_ent);
            for (size_t v : {p.o_mism, p.o_zero, p.o_nonunit, p.o_status, p.o_refused, p.o_ranges, p.o_scalars, p.o_work, p.bytes, p.memset_bytes,
                             (size_t)p.g_check, (size_t)p.g_cross, (size_t)p.g_quot, (size_t)p.g_fold, (size_t)p.g_refuse}) put(v);
        } else if (kind == "large") {
            size_t n_ent;
            in >> n >> m >> n_ent;
            put(ragged::too_large(K, n, m, n_ent));
            if (n_ent == 0) put(ragged::too_large(K, n, m));   // (the form of the two callers without entries)
        } else if (kind == "ranges") {
            in >> n;
            std::vector<uint32_t> r;                           // (exactly 2 m words on the heap: a read past them is the sanitizer's)
            for (uint32_t v; in >> v;) r.push_back(v);
            put(ragged::first_bad_range(r.data(), r.size() / 2, n));
        } else if (kind == "unit") {                           // msm::unit_slice as the three callers ask it
            size_t pts, ceiling, cap_unit;
            in >> c.test_slice_cap >> deg >> pts >> ceiling >> cap_unit;
            put(msm::unit_slice(c, K, deg, pts, ceiling, cap_unit));
        }
        printf("\n");
    }
    return 0;
}
'''

BUILDS = {"O2": ["-O2"], "sanitizers": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}

CAPS = [0, 1, 5, 16, 64]
SL = {d: M.PSCAN_RECORD_BYTES // (M.L28_PJ * d * 4) - 1 for d in (1, 2)}                 # the natural slice of the scan
LANES = {d: M.SRT_LANES // M.LP[d] for d in (1, 2)}                                      # ... of the chunk slices and of smul64
CHUNK_SLICE = {d: (2 << 30) // (M.MSMR_CHUNK * M.SMUL_T * M.PJ[d] * 4) // (64 // M.LP[d]) * (64 // M.LP[d]) for d in (1, 2)}   # 2 GB of tables
SMALL = [0, 1, 2, 15, 16, 17, 63, 64, 65]
TOTALS = [0, 1, 63, 64, 65, 127, 128, 129, 520]
N_MAX, M_MAX = 0xFFFFFFF0, 0x7FFFFFF0 // 2

CASES = [("consts",)]
for deg in (1, 2):
    for cap in CAPS:
        CASES += [("scan", cap, deg, n, m) for n in SMALL + [100, 520] for m in (0, 1, 64, 65)]
        CASES += [("msmr", cap, deg, n, m, total) for n, m in ((0, 1), (1, 1), (65, 37), (65, 64), (520, 39)) for total in TOTALS]
        # chunk totals around the natural chunk slice (set by the 2 GB rule in both groups: below the lane ceiling) and the ceiling
        CASES += [("msmr", cap, deg, 1 << 20, 65, t + d) for t in (CHUNK_SLICE[deg], 2 * CHUNK_SLICE[deg], LANES[deg]) for d in (-1, 0, 1)]
        CASES += [("smul64", cap, deg, n_pts, n, ix) for n_pts, ix in ((0, 0), (3, 1), (1000, 1)) for n in SMALL + [23, 1000]]
        CASES += [("smul64", cap, deg, 7, LANES[deg] + d, ix) for d in (-1, 0, 1) for ix in (0, 1)]
    # arithmetic only: the natural slice of the scan at its edges, several slices of it, n and m at the refusal limits
    CASES += [("scan", 0, deg, SL[deg] + d, m) for d in (-1, 0, 1) for m in (1, 65)]
    CASES += [("scan", 0, deg, n, M_MAX) for n in (3 * SL[deg] + 7, N_MAX)] + [("scan", 1, deg, N_MAX, M_MAX)]
    CASES += [("msmr", cap, deg, N_MAX, M_MAX, total) for cap in (0, 5) for total in ((1 << 31) - 1, 1 << 31, (1 << 31) + 1, 1 << 40)]
    CASES += [("smul64", cap, deg, N_MAX, 0x7FFFFFFF, ix) for cap in (0, 5) for ix in (0, 1)]
    # the slice rule as k_smul (no ceiling, any k), k_smul_seg and k_smul64 ask it; k = 5000 in G2: one wavefront's tables pass 2 GB
    CASES += [("unit", cap, deg, k, 0, 64 // M.LP[deg]) for cap in CAPS for k in (1, 2, 8, 9, 1000, 5000, 100000)]
    CASES += [("unit", cap, deg, M.MSMR_CHUNK, LANES[deg], 64 // M.LP[deg]) for cap in CAPS]
    CASES += [("unit", cap, deg, 1, LANES[deg], 1) for cap in CAPS]
CASES += [("sigdiv", n_pts, m, n_ent) for n_pts in SMALL + [255, 256, 257] for m in (1, 64, 65, 256, 257) for n_ent in (0, 1, 256, 257)]
CASES += [("sigdiv", N_MAX, M_MAX, N_MAX)]
# the refusals, each at its boundary value and one below
CASES += [("large", n, m, e) for n in (N_MAX, N_MAX + 1) for m in (M_MAX, M_MAX + 1) for e in (0, N_MAX, N_MAX + 1)] + [("large", 0, 0, 0)]
CASES += [("ranges", 10) + r for r in ((), (0, 0), (0, 10), (10, 10), (0, 11), (5, 4), (0, 3, 2, 10), (0, 3, 5, 4), (0, 3, 2, 11), (11, 11, 0, 1),
                                       (0, 1, 1, 2, 2, 3, 4, 3))]
CASES += [("ranges", 0, 0, 0), ("ranges", 0, 0, 1), ("ranges", 0xFFFFFFF0, 0, 0xFFFFFFF0, 0xFFFFFFF0, 0xFFFFFFF1)]


def unit_slice(c, deg, pts, ceiling, cap_unit):
    """the three slice computations of before the header, told apart by what they did not share"""
    if ceiling == 0:
        return M.slice_len(c, max((2 << 30) // (pts * M.SMUL_T * M.PJ[deg] * 4) // cap_unit * cap_unit, cap_unit), cap_unit)   # plan_small_groups
    if cap_unit == 1:
        return M.smul64(c, deg, 0, 0, False)["S"]
    return M.msmr_body(c, deg, 0, 0, 0)["slice"]


def lines(model, case):
    """what the model says the program prints for a case"""
    kind, a = case[0], case[1:]
    if kind == "consts":
        return [model.join("consts", model.CONSTS)]
    if kind == "large":
        return [model.join("large", [model.too_large(*a)] * (2 if a[2] == 0 else 1))]
    if kind == "ranges":
        return [model.join("ranges", [model.first_bad_range(list(zip(a[1::2], a[2::2])), a[0])])]
    if kind == "sigdiv":
        return [model.sigdiv_line(*a)]
    c = model.knobs(test_slice_cap=a[0])
    if kind == "unit":
        return [model.join("unit", [unit_slice(c, *a[1:])])]
    if kind == "msmr":
        heads, body = model.msmr_lines(c, *a[1:])
        return ["msmr" + heads, body]
    return [{"scan": model.scan_line, "smul64": model.smul64_line}[kind](c, *a[1:])]


@pytest.fixture(scope="module", params=sorted(BUILDS))
def out(request, tmp_path_factory):
    """the program's output lines, from the plain and from the sanitizer build"""
    d = tmp_path_factory.mktemp("ragged_plan_" + request.param)
    src, exe = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, *BUILDS[request.param], "-o", str(exe), str(src)])
    res = subprocess.run([str(exe)], input="".join(" ".join(map(str, c)) + "\n" for c in CASES), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
    return res.stdout.split("\n")[:-1]


def test_against_the_model(out):
    it = iter(out)
    for case in CASES:
        want = lines(M, case)
        assert [next(it) for _ in want] == want, case
    assert next(it, None) is None
    # both answers of every refusal, one slice and many, the single and the many-slice scan occur in the grid
    assert {"large 0 0", "large 1 1", "large 0", "large 1", "body 1", "ranges %d" % M.NONE, "ranges 0", "ranges 1", "ranges 3"} <= set(out)
    assert {int(line.split()[3]) for line in out if line.startswith("scan ")} == {0, 1}


def check_regions(p, names, total, unit, packed_last=False):
    """every region on its unit, none overlapping the next, the total the end of the last"""
    at = 0
    for x in names:
        assert p[x] >= at and p[x] % unit == 0, (x, p)
        at = p[x] + p["sizes"][x]
    assert at <= total < at + unit and (not packed_last or total == at), (p, total)


def check_slices(p, size, empty_ok=False):
    """the slices tile [0, items) in order; none is empty (but the scan's one slice of no points)"""
    k, step, items = p["nslices"], p["step"], p["items"]
    assert (k - 1) * step < items <= k * step or (items == 0 and k == (1 if empty_ok else 0))
    idx = range(k) if k <= 300 else [0, 1, 2, k // 2, k - 2, k - 1]
    for i in idx:
        s = p["at"](i * step)
        assert s["lo"] == i * step and 0 < s[size] <= step or (items == 0 and empty_ok)
        assert s["lo"] + s[size] == (items if i == k - 1 else (i + 1) * step)
        yield i, s


def fits32(*values):
    assert all(0 <= v < 1 << 32 for v in values), values


def check_case(case):
    kind, a = case[0], case[1:]
    if kind == "sigdiv":
        n_pts, m, n_ent = a
        p = M.sigdiv(*a)
        check_regions(p, M.SIGDIV, p["bytes"], 256)
        assert p["o_mism"] >= 16 and p["memset_bytes"] >= p["o_zero"] + n_pts and p["memset_bytes"] <= p["o_nonunit"]
        for g, items in (("g_check", max(m, n_pts) + 1), ("g_cross", n_ent), ("g_quot", n_pts), ("g_fold", m), ("g_refuse", m)):
            assert p[g] * 256 >= items and p[g] < 1 << 31
        return
    if kind not in ("scan", "msmr", "smul64"):
        return
    c, deg = M.knobs(test_slice_cap=a[0]), a[1]
    lp, upw, pj = M.LP[deg], 64 // M.LP[deg], M.PJ[deg]
    if kind == "scan":
        n, m = a[2:]
        p = M.scan_plan(c, deg, n, m)
        w = p["ws"]
        check_regions(w, M.SCAN_WS, w["bytes"], 256)
        assert (p["SL"] + 1) * pj * 4 <= M.PSCAN_RECORD_BYTES and w["sizes"]["o_s"] == (p["S"] + 1) * pj * 4 and p["S"] == min(n, p["SL"])
        assert p["single"] == int(p["nslices"] == 1) and 4 <= p["o_base"] <= p["o_basec"] <= p["range_bytes"]
        if not p["single"]:
            assert p["o_base"] % 256 == 0 == p["o_basec"] % 256 and p["o_basec"] - p["o_base"] >= m * pj * 4 and p["range_bytes"] == p["o_basec"] + 4 * m
        assert p["g_check"] * 256 >= m and p["g_begin"] * 256 >= p["begin_total"] == m * pj and p["g_range"] * 64 >= m * lp
        fits32(n, m, p["g_begin"])
        for i, s in check_slices(p, "len", empty_ok=True):
            assert s["first"] == int(i == 0) and s["more"] == 1 - s["last"] and s["last"] == int(i == p["nslices"] - 1) and s["len"] <= p["S"]
            assert s["chunks"] * M.PSCAN_CHUNK >= s["len"] and s["g_prep"] * 256 >= s["len"] and s["g_chunks"] * 64 >= s["chunks"] >= 1
            assert s["chunks"] * pj * 4 <= w["sizes"]["o_ct"]
    elif kind == "msmr":
        n, m, total = a[2:]
        h = M.msmr_heads(m)
        check_regions(h, ("h_cnt", "h_first", "h_cr"), h["words"], 64)
        assert h["h_cnt"] >= 4 and h["g_count"] * 256 >= m
        p = M.msmr_body(c, deg, n, m, total)
        assert p["too_many"] == int(total >= 1 << 31)
        if p["too_many"]:
            return
        check_regions(p, M.MSMR_BODY, p["words"], 64, packed_last=True)
        table = p["units0"] * M.MSMR_CHUNK * M.SMUL_T * pj * 4
        assert p["slice"] % upw == 0 and upw <= p["slice"] <= M.SRT_LANES // lp and table <= 2 << 30 and p["sizes"]["o_table"] * 4 == table
        assert p["g_fill"] * 256 >= max(total, m) and p["g_prep"] * 256 >= n and p["g_offcurve"] * 256 >= m
        for i, s in check_slices(p, "k"):
            assert s["k"] <= s["units"] <= p["units0"] and s["units"] % upw == 0 and s["g_smul"] * 64 == s["units"] * lp
            assert s["tab"] + 2 * s["k"] <= p["o_part"] and s["part"] + s["k"] * 24 * deg <= p["o_bad"] and s["bad"] + s["k"] <= p["o_bpre"]
            fits32(s["k"])
    else:
        n_pts, n, indexed = a[2:]
        p = M.smul64(c, deg, n_pts, n, indexed)
        check_regions(p, ("o_prep", "o_live", "o_tab"), p["words"], 4)
        assert p["np0"] == (n_pts if indexed else min(n, p["S"])) and p["S"] <= M.SRT_LANES // lp and p["g_prep_all"] * 256 >= n_pts
        for i, s in check_slices(p, "m"):
            assert s["m"] <= s["units"] <= p["units0"] and s["units"] % upw == 0 and s["g_smul"] * 64 == s["units"] * lp and s["g_prep"] * 256 >= s["m"]
            assert indexed or s["m"] <= p["np0"]
            assert (s["pts"], s["w"], s["out"]) == (s["lo"] * 24 * deg, s["lo"] * 8, s["lo"] * 24 * deg)


def test_invariants_of_every_plan(out):
    assert out[0] == lines(M, ("consts",))[0]                                            # (the numbers below are the header's: test_against_the_model)
    for case in CASES:
        check_case(case)
    # the 2 GB rule, not the lane ceiling, sets the natural chunk slice in both groups; the ceiling sets k_smul64's
    for deg in (1, 2):
        assert M.msmr_body(M.knobs(), deg, 0, 0, 0)["slice"] == CHUNK_SLICE[deg] < LANES[deg] == M.smul64(M.knobs(), deg, 0, 0, False)["S"]


def test_the_three_slice_rules_are_one(out):
    """k_smul64's slice has no 2 GB clause and k_smul_seg's no floor of one wavefront: the shared rule has both, and gives the
    numbers of before for every cap and degree (a unit's tables are fixed there, so these are all the inputs there are)"""
    asked, said = [c for c in CASES if c[0] == "unit"], [line for line in out if line.startswith("unit ")]
    got = {tuple(c[1:]): int(line.split()[1]) for c, line in zip(asked, said)}
    assert len(asked) == len(said)
    for (cap, deg, pts, ceiling, cap_unit), v in got.items():
        assert v == unit_slice(M.knobs(test_slice_cap=cap), deg, pts, ceiling, cap_unit)
    assert len(got) == 2 * len(CAPS) * 9


# ---- mutants: the model with one thing wrong; each must differ from the right model somewhere on the grid
MUTANTS = {
    "n records for n + 1": ("(pts + 1) * pj * 4, (pts + 1) * 4", "pts * pj * 4, (pts + 1) * 4"),
    "n counts for n + 1": ("(pts + 1) * pj * 4, (pts + 1) * 4", "(pts + 1) * pj * 4, pts * 4"),
    "o_basec without the rounding": ("o_base + ((0 if single else m * pj * 4 + 255) & ~255)", "o_base + (0 if single else m * pj * 4)"),
    "single strict": ("single = n <= SL", "single = n < SL"),
    "no chunk of no points": ("chunks = cdiv(m, PSCAN_CHUNK) if m else 1", "chunks = cdiv(m, PSCAN_CHUNK)"),
    "chunk slice not rounded to units": ("    slice_ = slice_len(c, slice_, upw)\n", "    slice_ = slice_len(c, slice_)\n"),
    "units not rounded": ("units0 = cdiv(min(total, slice_), upw) * upw\n    sizes = (n * L28_AFF", "units0 = min(total, slice_)\n    sizes = (n * L28_AFF"),
    "2 GB of tables counted in words": ("per_unit = 64 // LP[deg], MSMR_CHUNK * SMUL_T * PJ[deg] * 4", "per_unit = 64 // LP[deg], MSMR_CHUNK * SMUL_T * PJ[deg]"),
    "too many chunks strict": ("if total >= 1 << 31", "if total > 1 << 31"),
    "first[] without its + 1": ("h_cr = h_first + words64(m + 1)", "h_cr = h_first + words64(m)"),
    "prefix counts without their + 1": ("total, total + 1, units0", "total, total, units0"),
    "fill grid over the ranges only": ("g_fill=cdiv(max(total, m), 256)", "g_fill=cdiv(m, 256)"),
    "index grid without its + 1": ("cdiv(max(m, n_pts) + 1, 256)", "cdiv(max(m, n_pts), 256)"),
    "index grid over the dividends only": ("cdiv(max(m, n_pts) + 1, 256)", "cdiv(m + 1, 256)"),
    "memset past nonunit": ('memset_bytes=p["o_nonunit"]', 'memset_bytes=p["o_status"]'),
    "smul64 prepares a slice when indexed": ("np0 = n_pts if indexed else m0", "np0 = m0"),
    "smul64 cap in wavefronts": ("S = slice_len(c, SRT_LANES // LP[deg])", "S = slice_len(c, SRT_LANES // LP[deg], upw)"),
    "m limit for G1 lanes": ("m > 0x7FFFFFF0 // LP[2]", "m > 0x7FFFFFF0 // LP[1]"),
    "n limit strict": ("return n > 0xFFFFFFF0 or", "return n >= 0xFFFFFFF0 or"),
    "range may not end at n": ("if b > e or e > n", "if b > e or e >= n"),
}


def _mutant(name):
    m = types.ModuleType("mutant")
    with open(M.__file__) as f:
        src = f.read()
    a, b = MUTANTS[name]
    assert src.count(a) == 1, (name, src.count(a))
    exec(compile(src.replace(a, b), M.__file__, "exec"), m.__dict__)
    return m


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_the_grid_catches_a_wrong_model(name):
    m = _mutant(name)
    assert any(lines(m, case) != lines(M, case) for case in CASES if case[0] != "unit"), name
