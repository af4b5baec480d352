"""The host plan of the calls that handle key material, csrc/keys_plan.h (the refusals, the staged slices and the 64 MB rule, the
grids, every workspace and what a slice adds to the caller's arrays), compiled for the host as a stand-alone program -- once with
-O2, once under AddressSanitizer and UBSan -- and compared number for number with tests/keys_plan_model.py, which states what
blsgpu_api.hip did before the header existed.  The invariants below hold for every plan whatever the model says, and the mutants
show that the grid of cases tells a wrong model from the right one.

The grid.  Item counts 0, 1, cap - 1, cap, cap + 1 and a multiple of the cap for the caps 0 (natural), 1, 5 and 64 of
BLSGPU_TEST_SLICE_CAP; the natural slice lengths 2^18, 2^22, 2^20 and 65536, each - 1, + 0, + 1; k and t 1, 2, 255, 256, 257, 1023,
1024 and 1025 (refused); depth 1, 2, 255; seed lengths 0 and BLSGPU_SEED_MAX_BYTES; every combination of priv, out_sk, out_pk_aff
with out_parents, n_msg == 1 against one per item, out_frag; for each refusal the last value taken and the first refused."""
import itertools
import os
import subprocess
import types

import pytest

import keys_plan_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")

# one case per line, its kind first; the answer repeats the kind.  A sliced plan prints its first and its last slice.
HOST_TEST = r'''
#include "keys_plan.h"
#include <stdio.h>
#include <iostream>
#include <sstream>
#include <string>
static void put(size_t v) { printf(" %zu", v); }
static const keys::Consts& K = keys::GFX950;
// at(lo) of the first and the last slice of a loop over n items in runs of `step`
template <class F> static void slices(size_t n, size_t step, F f) {
    if (!n || !step) return;
    f((size_t)0);
    f((n - 1) / step * step);
}
int main() {
    std::string line, kind;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        in >> kind;
        printf("%s", kind.c_str());
        msm::Knobs c;
        if (kind == "large") {
            std::string which; size_t a = 0, b = 0, d = 0, e = 0;
            in >> which >> a >> b >> d >> e;
            put(which == "k" ? keys::bad_k(K, a) : which == "lanes" ? keys::too_many_lanes(a) : which == "paths" ? keys::hd_paths_too_large(a, b) :
                which == "poly" ? keys::poly_too_many(a, b) : which == "lagrange" ? keys::lagrange_too_large(a, b) :
                which == "frsum" ? keys::fr_sum_too_large(a, b) : which == "deal" ? keys::deal_too_large(K, a, b, d, e != 0) : keys::g2_smul_too_large(a));
        } else if (kind == "staged") {
            size_t n, natural;
            in >> c.test_slice_cap >> n >> natural;
            put(keys::staged_slice(c, n, natural));
        } else if (kind == "fit") {
            std::string which; size_t n, a = 0, b = 0, d = 0;
            in >> c.test_slice_cap >> n >> which >> a >> b >> d;
            const size_t item = which == "deal" ? keys::deal_item_bytes(a, b, d != 0) : which == "frsum" ? keys::fr_sum_item_bytes(a) : keys::seeds_item_bytes(a);
            put(item), put(keys::staged_fit(c, n, item));
        } else if (kind == "lagr") {
            size_t k, groups;
            in >> k >> groups;
            const keys::LagrShape s = keys::lagrange_shape((uint32_t)k);
            for (size_t v : {(size_t)s.threads, (size_t)s.gpb, s.lds, (size_t)s.grid(groups), keys::coeff_bytes(k, groups)}) put(v);
        } else if (kind == "sum") {
            size_t k, groups;
            in >> k >> groups;
            const keys::SumShape s = keys::sum_shape(K, k);
            put(s.per), put(s.gpb), put(s.grid(groups));
        } else if (kind == "eval") {
            size_t n_polys, n_x;
            in >> n_polys >> n_x;
            put(keys::eval_bpp(K, n_x)), put(keys::eval_blocks(K, n_polys, n_x));
        } else if (kind == "fix") {
            size_t n;
            in >> c.test_slice_cap >> n;
            const size_t step = keys::fix_step(c);
            put(step);
            slices(n, step, [&](size_t lo) { const keys::FixAt a = keys::fix_at(n, step, lo); for (size_t v : {a.m, a.scalars, a.add, a.aff, a.ser, (size_t)a.grid}) put(v); });
        } else if (kind == "children") {
            size_t n, pub;
            in >> c.test_slice_cap >> n >> pub;
            const keys::ChildrenPlan p = keys::plan_children(c, n, pub != 0);
            for (size_t v : {p.step, p.o_parent, p.o_flag, p.o_ileft, p.bytes}) put(v);
            slices(n, p.step, [&](size_t lo) { const keys::ChildrenAt a = p.at(lo); for (size_t v : {a.m, a.idx, a.chain, a.sk, a.aff, a.ser, (size_t)a.grid}) put(v); });
        } else if (kind == "paths") {
            size_t n, depth, priv;
            in >> c.test_slice_cap >> n >> depth >> priv;
            const keys::PathsPlan p = keys::plan_paths(c, n, depth, priv != 0);
            for (size_t v : {p.S, p.o_flag, p.o_chain, p.o_scal, p.o_aff[0], p.o_aff[1], p.bytes}) put(v);
            slices(n, p.S, [&](size_t lo) { const keys::PathsAt a = p.at(lo); for (size_t v : {a.m, a.parent_of, a.idx, a.chain, a.sk, a.aff, a.ser, a.fp, (size_t)a.grid}) put(v); });
        } else if (kind == "seeds") {
            size_t seed_len, n, sk, aff, par;
            in >> c.test_slice_cap >> seed_len >> n >> sk >> aff >> par;
            const keys::SeedsPlan p = keys::plan_seeds(c, K, seed_len, n, sk != 0, aff != 0, par != 0);
            for (size_t v : {p.S, p.o_sk, p.o_aff, p.bytes}) put(v);
            slices(n, p.S, [&](size_t lo) { const keys::SeedsAt a = p.at(lo); for (size_t v : {a.m, a.seeds, a.sk, a.chain, a.par, a.aff, a.ser, (size_t)a.grid, (size_t)a.g_pack}) put(v); });
        } else if (kind == "poly") {
            size_t n_polys, t;
            in >> n_polys >> t;
            const keys::PolyPlan p = keys::plan_poly(K, n_polys, t);
            for (size_t v : {p.m, p.mk, p.o_flag, p.o_sub, p.o_l28, p.bytes, p.sub_bytes, (size_t)p.g_prep, (size_t)p.g_sub}) put(v);
        } else if (kind == "smul") {
            size_t shared, n;
            in >> c.test_slice_cap >> shared >> n;
            const size_t step = keys::smul_step(c, K), held = keys::smul_held(c, K, shared != 0, n);
            put(step), put(held), put(keys::smul_table_bytes(K, held));
            slices(n, step, [&](size_t lo) { const keys::SmulAt a = keys::smul_at(K, n, step, lo); for (size_t v : {a.m, a.pts, a.scalars, a.aff, a.ser, a.inf, (size_t)a.grid}) put(v); });
        } else if (kind == "sign") {
            size_t n_msg, n;
            in >> c.test_slice_cap >> n_msg >> n;
            const keys::SignPlan p = keys::plan_sign(c, K, n_msg, n);
            for (size_t v : {p.held, p.step, (size_t)p.shared, p.o_pts, p.o_table, p.bytes}) put(v);
            slices(n, p.step, [&](size_t lo) { const keys::SignAt a = p.at(lo); for (size_t v : {a.m, a.msgs, a.hashes, a.sks, a.aff, a.ser}) put(v); });
        } else if (kind == "threshold") {
            size_t k, groups, n_msg;
            in >> c.test_slice_cap >> k >> groups >> n_msg;
            const keys::ThresholdPlan p = keys::plan_threshold(c, K, k, groups, n_msg);
            for (size_t v : {p.n, p.held, (size_t)p.shared, p.lagr_bytes, p.o_sc, p.o_rep, p.frs_bytes, p.o_hm, p.o_table, p.smul_bytes, (size_t)p.g_scale}) put(v);
            slices(p.n, p.held, [&](size_t lo) { const keys::ThresholdAt a = p.at(lo); for (size_t v : {a.m, a.sc, a.aff, a.ser, a.inf, (size_t)a.g_spread}) put(v); });
        }
        printf("\n");
    }
    return 0;
}
'''

BUILDS = {"O2": ["-O2"], "sanitizers": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}

CAPS = [0, 1, 5, 64]
NATURALS = [M.FIX_HOST_SLICE, M.FIX_SLICE, M.SEED_SLICE, M.SMUL_SLICE]
KS = [1, 2, 255, 256, 257, 1023, 1024]
DEPTHS = [1, 2, 255]
SEED_LENS = [0, M.SEED_MAX_BYTES]
B32, B31 = 1 << 32, 1 << 31


def counts(cap, natural):
    """0, 1, the slice length - 1, + 0, + 1 and three slices"""
    s = M.slice_len(cap, natural)
    return sorted({0, 1, max(s - 1, 0), s, s + 1, 3 * s})


CASES = [("large", "k", k) for k in [0] + KS + [1025]]
# each refusal: the last value taken and the first refused, on every term of its bound
CASES += [("large", "lanes", n) for n in (B32 - 1, B32)]
CASES += [("large", "paths", n, p) for n in (B32 - 1, B32) for p in (B32 - 1, B32)]
CASES += [("large", "poly", n, t) for t in (1, 2, 1024) for n in (0x7FFFFFFF // t, 0x7FFFFFFF // t + 1)]
CASES += [("large", "lagrange", k, g) for k, g in ((1, B31 - 1), (1, B31), (2, 0x7FFFFFF8), (2, 0x7FFFFFF9), (1024, 4194303), (1024, 4194304))]
CASES += [("large", "frsum", k, g) for k, g in ((1, B31 - 1), (1, B31), ((M.SIZE_MAX >> 6) // 3, 3), ((M.SIZE_MAX >> 6) // 3 + 1, 3), (M.SIZE_MAX >> 6, 1), ((M.SIZE_MAX >> 6) + 1, 1))]
CASES += [("large", "deal", n, t, x, f) for f in (0, 1) for n, t, x in ((B31 - 1, 1, 1), (B31, 1, 1), (1, 1, 0xFFFFFF00), (1, 1, 0xFFFFFF01), (4194303, 1024, 1),
                                                                     (4194304, 1024, 1), (B31 // 2 - 1, 1, 257), (B31 // 2, 1, 257), (B31 // 2, 1, 256))]
CASES += [("large", "smul", n) for n in (0xFFFFFFF0, 0xFFFFFFF1)]
CASES += [("staged", cap, n, nat) for nat in NATURALS for cap in CAPS for n in counts(cap, nat)]
CASES += [("fit", cap, n, "seeds", ln) for cap in CAPS for ln in SEED_LENS for n in counts(cap, M.STAGE_TARGET // M.seeds_item_bytes(ln))]
CASES += [("fit", cap, n, "frsum", k) for cap in CAPS for k in KS + [(1 << 21) - 6, 1 << 21, 1 << 40] for n in (1, 5, 6, 1 << 19, 1 << 20)]   # an item of 64 MB - 16, of more: never zero
CASES += [("fit", cap, n, "deal", t, x, f) for cap in CAPS for t in (1, 67, 1024) for x, f in ((0, 0), (1, 1), (1000, 1), (1000, 0), (1 << 22, 1)) for n in (1, 5, 6, 1 << 20)]
CASES += [("lagr", k, g) for k in KS for g in (1, 2, 255, 256, 257, 4194303 // k + 1)]
CASES += [("sum", k, g) for k in KS + [1 << 20] for g in (1, 2, 255, 256, 257, B31 - 1)]
CASES += [("eval", n, x) for n in (1, 3, 1000) for x in (0, 1, 255, 256, 257, 1000)] + [("eval", B31 // 2 - 1, 257), ("eval", 1, 0xFFFFFF00)]
CASES += [("fix", cap, n) for cap in CAPS for n in counts(cap, M.FIX_SLICE)]
CASES += [("children", cap, n, pub) for pub in (0, 1) for cap in CAPS for n in counts(cap, M.FIX_HOST_SLICE if pub else M.FIX_SLICE)[1:]] + [("children", 0, B32 - 1, 1)]
CASES += [("paths", cap, n, d, priv) for priv in (0, 1) for d in DEPTHS for cap in CAPS for n in counts(cap, M.FIX_HOST_SLICE)[1:]] + [("paths", 0, B32 - 1, 255, 0)]
CASES += [("seeds", cap, ln, n, sk, aff, par) for cap in CAPS for ln in SEED_LENS for sk in (0, 1) for aff, par in itertools.product((0, 1), (0, 1))
          for n in counts(cap, M.SEED_SLICE)[1:]] + [("seeds", 0, 1024, B32 - 1, 0, 0, 1)]
CASES += [("poly", n, t) for t in KS for n in (1, 2, 63, 64, 65, 1000)] + [("poly", 0x7FFFFFFF // t, t) for t in (1, 2, 1024)]
CASES += [("smul", cap, sh, n) for sh in (0, 1) for cap in CAPS for n in counts(cap, M.SMUL_SLICE)[1:]] + [("smul", 0, 0, 0xFFFFFFF0)]
CASES += [("sign", cap, 1 if sh else n, n) for sh in (0, 1) for cap in CAPS for n in counts(cap, M.SMUL_SLICE)[1:]] + [("sign", 0, 1, 0xFFFFFFF0), ("sign", 0, 0xFFFFFFF0, 0xFFFFFFF0)]
CASES += [("threshold", cap, k, g, 1 if sh else g) for sh in (0, 1) for cap in CAPS for k in KS for g in (1, 2, 5, 6, 70)]
CASES += [("threshold", 0, k, g, n_msg) for k, g in ((1, 65535), (1, 65536), (1, 65537), (2, 0x7FFFFFF8), (1024, 4194303)) for n_msg in (1, g)]


@pytest.fixture(scope="module", params=sorted(BUILDS))
def out(request, tmp_path_factory):
    """the program's output lines, from the plain and from the sanitizer build"""
    d = tmp_path_factory.mktemp("keys_plan_" + request.param)
    src, exe = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, *BUILDS[request.param], "-o", str(exe), str(src)])
    res = subprocess.run([str(exe)], input="".join(" ".join(map(str, c)) + "\n" for c in CASES), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
    return res.stdout.split("\n")[:-1]


def test_against_the_model(out):
    assert len(out) == len(CASES)
    for case, got in zip(CASES, out):
        assert got == M.line(case), case
    # both answers of every refusal occur, and so do one slice and many of every sliced plan
    for which in ("k", "lanes", "paths", "poly", "lagrange", "frsum", "deal", "smul"):
        assert {M.line(c) for c in CASES if c[:2] == ("large", which)} == {"large 0", "large 1"}, which
    assert M.line(("large", "k", 1024)) == "large 0" and M.line(("large", "k", 1025)) == "large 1"


def fits32(*values):
    assert all(0 <= v < 1 << 32 for v in values), values


def check_regions(p, regions, total, units):
    """the regions in order, none overlapping the next, each on its unit of the layout, the last ending at the total"""
    at = 0
    for (name, size), unit in zip(regions, units):
        assert p[name] >= at and p[name] % unit == 0, (name, p)
        at = p[name] + size
    assert at == total, (regions, total)


def check_slices(n, step, at):
    """-> [(lo, at(lo))]: the slices cover [0, n) once and in order, none empty, none longer than the first"""
    out, end = [], 0
    for lo, m in M.runs(n, step):
        a = at(lo)
        assert lo == end and a["m"] == m and 1 <= m <= step
        end = lo + m
        out.append((lo, a))
    assert end == n
    return out[:2] + out[-2:]                                                            # (a slice's figures are linear in lo: the ends tell)


def test_invariants_of_every_plan(out):
    """The invariants are checked on the MODEL's plans, as in the sibling tests: they say something about the header only
    because test_against_the_model holds the header equal to the model on these very cases, line for line -- restated here,
    so that this test does not pass on its own where the two differ.  (The mutants below likewise hold one model against
    another: they test the grid, not the header.)"""
    assert out == [M.line(case) for case in CASES]
    for case in CASES:
        kind, a = case[0], case[1:]
        if kind == "staged":
            cap, n, nat = a
            s = M.staged_slice(cap, n, nat)
            assert s <= n and (s >= 1 or n == 0) and s <= nat and (cap == 0 or s <= cap)
        elif kind == "fit":
            cap, n = a[:2]
            item, s = [int(x) for x in M.line(case).split()[1:]]
            assert s <= n and (s >= 1 or n == 0) and (cap == 0 or s <= cap)
            assert s == 1 or s * item <= M.STAGE_TARGET                                  # 64 MB, unless one item alone is more
        elif kind == "lagr":
            k, groups = a
            threads, gpb, lds = M.lagrange_shape(k)
            grid = M.blocks(groups, gpb)
            assert threads % 64 == 0 and gpb * k <= threads <= 1024 and grid * gpb >= groups and lds <= 65536
            fits32(k, groups, gpb, k * groups)
        elif kind == "sum":
            k, groups = a
            per, gpb = M.sum_shape(k)
            assert 1 <= per <= k and per * gpb <= M.SUM_THREADS and M.blocks(groups, gpb) * gpb >= groups
            fits32(groups, gpb, per)
        elif kind == "eval":
            n_polys, n_x = a
            bpp = M.eval_bpp(n_x)
            assert bpp * M.EVAL_THREADS >= n_x
            fits32(n_x, bpp, n_polys * bpp)
        elif kind == "fix":
            cap, n = a
            step = M.slice_len(cap, M.FIX_SLICE)
            for lo, s in check_slices(n, step, lambda lo: M.fix_at(n, step, lo)):
                assert s["grid"] * 256 >= s["m"] and s["scalars"] == lo * 8 and s["aff"] == lo * 24 and s["ser"] == lo * 12
                fits32(s["m"])
        elif kind == "children":
            cap, n, pub = a
            p = M.plan_children(cap, n, pub)
            check_regions(p, p["regions"], p["bytes"], (128, 128, 32))
            for lo, s in check_slices(n, p["step"], p["at"]):
                assert s["grid"] * 256 >= s["m"] and (not pub or s["m"] * 32 <= dict(p["regions"])["o_ileft"])
                fits32(s["m"], n)
        elif kind == "paths":
            cap, n, depth, priv = a
            p = M.plan_paths(cap, n, depth, priv)
            check_regions(p, p["regions"], p["bytes"], (256, 32, 32, 32, 32))
            assert p["bytes"] == 256 + p["S"] * (160 if priv else 256)
            size = dict(p["regions"])
            for lo, s in check_slices(n, p["S"], p["at"]):
                assert s["m"] * 32 <= size["o_chain"] == size["o_scal"] and s["m"] * 96 <= size["o_aff0"] and (priv or s["m"] * 96 <= size["o_aff1"])
                assert s["grid"] * 256 >= s["m"] and s["idx"] == lo * depth and s["aff"] == lo * 96
                fits32(s["m"], n, depth)
        elif kind == "seeds":
            cap, ln, n, sk, aff, par = a
            p = M.plan_seeds(cap, ln, n, sk, aff, par)
            check_regions(p, p["regions"], p["bytes"], (32, 32))
            size = dict(p["regions"])
            assert (size["o_sk"] == 0) == bool(sk) and (size["o_aff"] != 0) == bool(par and not aff)
            for lo, s in check_slices(n, p["S"], p["at"]):
                assert (sk or s["m"] * 32 <= size["o_sk"]) and (aff or not par or s["m"] * 96 <= size["o_aff"])
                assert s["grid"] * 256 >= s["m"] and s["g_pack"] * 256 >= s["m"] * 24 and s["seeds"] == lo * ln
                fits32(s["m"], ln)
        elif kind == "poly":
            p = M.plan_poly(*a)
            check_regions(p, p["regions"], p["bytes"], (256, 256, 256))
            assert p["g_prep"] * 256 >= p["m"] and p["g_sub"] * 256 >= p["mk"] and p["sub_bytes"] == dict(p["regions"])["o_sub"]
            fits32(p["m"], a[0], a[1])
        elif kind == "smul":
            cap, shared, n = a
            step, held = M.slice_len(cap, M.SMUL_SLICE), M.smul_held(cap, shared, n)
            for lo, s in check_slices(n, step, lambda lo: M.smul_at(n, step, lo)):
                assert s["grid"] * M.SMUL_PAIRS >= s["m"] and (shared or s["m"] <= held)
                fits32(2 * s["m"])
        elif kind == "sign":
            cap, n_msg, n = a
            p = M.plan_sign(cap, n_msg, n)
            check_regions(p, p["regions"], p["bytes"], (256, 256))
            size = dict(p["regions"])
            for lo, s in check_slices(n, p["step"], p["at"]):
                assert s["msgs"] * 192 <= size["o_pts"] and s["msgs"] * M.TABLE_DW * 4 <= size["o_table"] and s["msgs"] in (1, s["m"])
                assert s["hashes"] + s["msgs"] * 32 <= n_msg * 32 and s["sks"] == lo * 32
        elif kind == "threshold":
            cap, k, groups, n_msg = a
            p = M.plan_threshold(cap, k, groups, n_msg)
            check_regions(p, p["frs_regions"], p["frs_bytes"], (256, 256))
            check_regions(p, p["smul_regions"], p["smul_bytes"], (256, 256))
            assert p["lagr_bytes"] == p["n"] * 32 and p["g_scale"] * 256 >= p["n"]
            fits32(p["n"], k, groups)
            frs, smul = dict(p["frs_regions"]), dict(p["smul_regions"])
            if not p["shared"]:
                for lo, s in check_slices(p["n"], p["held"], p["at"]):
                    assert s["m"] * 192 <= frs["o_rep"] and s["m"] * M.TABLE_DW * 4 <= smul["o_table"] and s["sc"] + s["m"] * 32 <= frs["o_sc"]
                    assert s["g_spread"] * 256 >= s["m"] * 48
                    fits32(lo, s["m"])
            else:
                assert frs["o_rep"] == 0 and smul["o_table"] == M.TABLE_DW * 4


# ---- mutants: the model with one thing wrong; each must differ from the right model somewhere on the grid
MUTANTS = {
    "a staged slice one too long": ("return min(n, slice_len(cap, natural))", "return min(n, slice_len(cap, natural) + 1)"),
    "the 64 MB rule may give zero": ("return n if n < fit else max(fit, 1)", "return n if n < fit else fit"),
    "the seed's outputs one byte short": ("return seed_len + 368", "return seed_len + 367"),
    "fragments staged when not asked for": ("(n_x * 32 if frag else 0)", "n_x * 32"),
    "the public and private HD strides swapped": ("(160 if priv else 256)", "(256 if priv else 160)"),
    "chain codes and scalars swapped": ("o_chain=chain, o_scal=scal", "o_chain=scal, o_scal=chain"),
    "the flag of B_FIX_WS on the parent key": ("o_flag=128, o_ileft=256", "o_flag=96, o_ileft=256"),
    "keys held although out_sk is given": ("ws_sk = 0 if out_sk else S * 32", "ws_sk = S * 32"),
    "affine keys held without records": ("S * 96 if out_parents and not out_aff else 0", "0 if out_aff else S * 96"),
    "the subgroup flags not rounded up": ("l28 = 256 + up(n_polys * 4)", "l28 = 256 + n_polys * 4"),
    "a table per item with one message": ("return 1 if shared else staged_slice(cap, n, SMUL_SLICE)", "return staged_slice(cap, n, SMUL_SLICE)"),
    "the sign loop in held slices with one message": ("step = n if shared else held", "step = held"),
    "point copies with one message": ("rep = 0 if shared else held * 192", "rep = held * 192"),
    "a lane per scalar in k_g2_smul": ("grid=blocks(m, SMUL_PAIRS)", "grid=blocks(m)"),
    "lagrange bound strict": ("k * groups > 0xFFFFFFF0\n", "k * groups >= 0xFFFFFFF0\n"),
    "commitment bound moved by one": ("n_polys > 0x7FFFFFFF // t", "n_polys >= 0x7FFFFFFF // t"),
    "deal bound without the fragments' grid": ("bool(frag and n_polys * eval_bpp(n_x) > 0x7FFFFFFF)", "False"),
    "k up to 1025": ("k > MAX_K", "k > MAX_K + 1"),
    "groups per workgroup one short": ("gpb = 256 // k if k <= 256 else 1", "gpb = max(256 // k - 1, 1) if k <= 256 else 1"),
    "a path's indices not strided by the depth": ("idx=lo * depth", "idx=lo"),
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
    assert any(m.line(case) != M.line(case) for case in CASES), name
