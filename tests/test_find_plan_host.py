"""The host plan of the three forgery finders, csrc/find_plan.h (the refusals, the one slice rule, every workspace and every
round with its grids, all derived from the header's region lists), compiled for the host as a stand-alone program -- once with
-O2, once under AddressSanitizer and UBSan -- and compared number for number with tests/find_plan_model.py, which states what
blsgpu_api.hip did before the header existed, hand-added sums included.  The invariants below hold for every plan whatever the
model says -- among them what the 2 GB of the slice rule really bounds --, the sweep checks the folded round's bound on every
small input there is, and the mutants show that the grid of cases tells a wrong model from the right one."""
import itertools
import os
import subprocess
import types

import pytest

import bisect_model as B
import find_plan_model as M
from test_bisect_plan_host import run_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")

# one case per line, its kind first; the answer repeats the kind.  A plan prints its first and its last slice.
HOST_TEST = r'''
#include "find_plan.h"
#include <stdio.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
static void put(size_t v) { printf(" %zu", v); }
template <class T> std::vector<T> some(std::istream& in, size_t n) { std::vector<T> v(n); for (T& x : v) in >> x; v.shrink_to_fit(); return v; }
template <class T> std::vector<T> rest(std::istream& in) { std::vector<T> v; T x; while (in >> x) v.push_back(x); v.shrink_to_fit(); return v; }
static size_t last_len(size_t items, size_t step) { return items && step ? items - ((items + step - 1) / step - 1) * step : 0; }
#define PUT_OFFSET(name, unit, bytes) put(w.o_##name);
// the exhaustive sweep of the folded round over n_e leaves: every run table, every forged subset of up to three leaves
struct Sweep { size_t rounds = 0, bad_slots = 0, bad_bytes = 0, bad_nodes = 0; };
static void sweep_one(uint32_t n_e, const std::vector<uint32_t>& rb, const std::vector<uint32_t>& rmsg, const std::vector<uint32_t>& forged, Sweep& s) {
    const size_t rounding = 11 * 255 + 6 * 63 * 4 + 4;                       // eleven regions, the table's six arrays and first's + 1
    bisect::State<uint32_t> b;
    bisect::FoldPlan p;
    b.nodes.assign(1, 0u);
    bisect::run(b, bisect::ceil_pow2(n_e), n_e, [&](std::vector<uint32_t>& nodes, size_t L, uint8_t* verdict) {
        bisect::fold_round(nodes, L, n_e, rb.data(), rmsg.data(), (uint32_t)rmsg.size(), p);
        const find::FoldRound r = find::folded_round(p);
        s.rounds++;
        s.bad_nodes += r.nn > n_e;
        s.bad_slots += r.slots > 2 * r.nn + rmsg.size() || r.slots > find::FOLD_SLOTS_PER_ITEM * n_e;
        s.bad_bytes += r.w.bytes > find::FOLD_ROUND_PER * n_e + rounding;
        for (size_t i = 0; i < nodes.size(); i++) {
            verdict[i] = 1;
            for (uint32_t f : forged) if (f >= nodes[i] && f < nodes[i] + L) verdict[i] = 0;
        }
        return 0;
    });
}
int main() {
    std::string line, kind;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        in >> kind;
        printf("%s", kind.c_str());
        msm::Knobs c;
        if (kind == "consts") {
            for (size_t v : {find::PLAIN_KEEP_PER, find::PLAIN_ROUND_PER, find::FOLD_KEEP_PER, find::FOLD_SLOT_PER, find::FOLD_NODE_PER, find::FOLD_ROUND_PER,
                             find::shares_keep_per(1), find::shares_round_per(1), find::shares_keep_per(67), find::shares_round_per(128),
                             find::SHR_ROUND_UNCOUNTED, find::BUDGET, find::FIND_SLACK}) put(v);
        } else if (kind == "find") {
            size_t n, n_keys, n_msgs, folded;
            in >> c.test_slice_cap >> n >> n_keys >> n_msgs >> folded;
            const find::FindPlan p = find::plan_find(c, n, n_keys, n_msgs, folded != 0);
            const find::FindWs& w = p.w;
            for (size_t v : {p.keep_per, p.round_per, p.slice, p.rcap, w.o_keyst, w.o_h, w.o_sigst, w.o_r, w.o_elig, w.o_dense, w.o_a, w.o_b}) put(v);
            if (folded) for (size_t v : {w.o_ad, w.o_bd, w.o_rb, w.o_rmsg}) put(v);
            put(w.bytes);
            for (size_t m : {p.slice, last_len(n, p.slice)}) {
                const find::FindSlice s = p.at(m);
                for (size_t v : {s.m, s.rn, s.ltotal, (size_t)s.g_settle, (size_t)s.g_leaves}) put(v);
            }
        } else if (kind == "shares") {
            size_t k, groups, n_keys, scaled;
            in >> c.test_slice_cap >> k >> groups >> n_keys >> scaled;
            const find::SharesPlan p = find::plan_shares(c, k, groups, n_keys, scaled != 0);
            const find::SharesWs& w = p.w;
            for (size_t v : {p.K, p.keep_per, p.round_per, p.slice, p.n0}) put(v);
            FIND_SHR_KEEP(PUT_OFFSET)
            put(w.bytes);
            for (size_t m : {p.slice, last_len(groups, p.slice)}) { put(p.at(m).n); put(p.at(m).g_weights); }
        } else if (kind == "shround") {
            size_t nn, len, k;
            in >> nn >> len >> k;
            const find::SharesRound r = find::shares_round(nn, len, k);
            const find::SharesRoundWs& w = r.w;
            for (size_t v : {r.nn, r.slots, r.gtotal, r.ptotal, (size_t)r.lg, (size_t)r.g_gather, (size_t)r.g_pairs, (size_t)r.g_verdict}) put(v);
            FIND_SHR_ROUND(PUT_OFFSET)
            put(w.bytes);
        } else if (kind == "plainr") {
            uint32_t n_e; size_t L;
            in >> n_e >> L;
            std::vector<uint32_t> nodes = rest<uint32_t>(in);
            bisect::Part shape[2];
            bisect::plain_round(nodes, L, n_e, shape);
            const find::PlainRound r = find::plain_round(shape);
            for (uint32_t o : nodes) put(o);
            for (size_t v : {r.nn, r.bytes, r.head.o_off, r.head.o_v}) put(v);
            for (const find::PlainPart& q : r.part) {
                const find::PlainPartWs& w = q.w;
                for (size_t v : {q.nodes, q.len, q.first, q.gsz, q.pairs, q.gtotal, q.ptotal, (size_t)q.g_gather, (size_t)q.g_pairs, (size_t)q.g_verdict}) put(v);
                FIND_PLAIN_PART(PUT_OFFSET)
            }
        } else if (kind == "foldr") {
            uint32_t n_e, n_runs; size_t L;
            in >> n_e >> n_runs;
            const std::vector<uint32_t> rb = some<uint32_t>(in, n_runs + 1), rmsg = some<uint32_t>(in, n_runs);
            in >> L;
            std::vector<uint32_t> nodes = rest<uint32_t>(in);
            bisect::FoldPlan p;
            bisect::fold_round(nodes, L, n_e, rb.data(), rmsg.data(), n_runs, p);
            const find::FoldRound r = find::folded_round(p);
            const find::FoldRoundWs& w = r.w;
            for (size_t v : {r.nn, r.slots, r.nb, r.ftotal, (size_t)r.g_codes, (size_t)r.g_fill, (size_t)r.g_verdict}) put(v);
            FIND_FOLD_ROUND(PUT_OFFSET)
            put(w.bytes);
            if (r.slots) { put(r.g1_at(r.slots - 1) + find::G1 <= w.o_g2); put(r.g2_at(r.slots - 1) + find::G2 <= w.o_e); put(r.e_at(r.nn - 1) + find::FQ12 <= w.bytes); }
        } else if (kind == "large") {
            std::string which; size_t a, b, d;
            in >> which >> a >> b >> d;
            put(which == "find" ? find::find_too_large(a, b, d) : find::shares_too_large(a, b, d));
        } else if (kind == "sweep") {
            uint32_t n_e;
            in >> n_e;
            Sweep s;
            for (uint32_t cuts = 0; cuts < (1u << (n_e - 1)); cuts++) {       // bit i: a run begins at leaf i + 1
                std::vector<uint32_t> rb(1, 0u), rmsg;
                for (uint32_t i = 1; i < n_e; i++) if (cuts >> (i - 1) & 1u) rb.push_back(i);
                rb.push_back(n_e);
                for (size_t r = 0; r + 1 < rb.size(); r++) rmsg.push_back((uint32_t)(3 * r + 1));
                rb.shrink_to_fit(), rmsg.shrink_to_fit();
                sweep_one(n_e, rb, rmsg, {}, s);
                for (uint32_t a = 0; a < n_e; a++) {
                    sweep_one(n_e, rb, rmsg, {a}, s);
                    for (uint32_t b = a + 1; b < n_e; b++) {
                        sweep_one(n_e, rb, rmsg, {a, b}, s);
                        for (uint32_t d = b + 1; d < n_e; d++) sweep_one(n_e, rb, rmsg, {a, b, d}, s);
                    }
                }
            }
            for (size_t v : {s.rounds, s.bad_slots, s.bad_bytes, s.bad_nodes}) put(v);
        }
        printf("\n");
    }
    return 0;
}
'''

BUILDS = {"O2": ["-O2"], "sanitizers": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
SWEEP_MAX = 12

GB2 = 2 << 30
CAPS = [0, 1, 5, 64]
NAT = {0: (GB2 - (1 << 20)) // 1542, 1: (GB2 - (1 << 20)) // 1993}                       # the natural slice of the plain and the folded form
N_LIM, KEY_LIM, MSG_LIM = 0x7FFFFFF0, 0x7FFFFFFF, GB2 // 192
K_ONE = [1 << 21, 5_000_000]                                                              # one session alone passes 2 GB: by its round, by both

CASES = [("consts",)]
for folded in (0, 1):
    CASES += [("find", cap, n, nk, nm, folded) for cap in CAPS for n in (0, 1, 2, 63, 64, 65, 1000) for nk in (1, 2, 300) for nm in (1, 2, 300)]
    # arithmetic only: n around the natural slice and several slices of it, n and n_msgs at the refusal limits and one past them
    CASES += [("find", 0, NAT[folded] + d, 300, nm, folded) for d in (-1, 0, 1) for nm in (1, NAT[folded] - 1, NAT[folded], NAT[folded] + 1)]
    CASES += [("find", cap, n, KEY_LIM, nm, folded) for cap in (0, 5) for n in (3 * NAT[folded] + 7, N_LIM, N_LIM + 1) for nm in (MSG_LIM, MSG_LIM + 1)]
    # n_msgs below, at and above a capped slice: both branches of rcap and rn
    CASES += [("find", 5, 12, 12, nm, folded) for nm in (2, 4, 5, 6, 7)]
for scaled in (0, 1):
    CASES += [("shares", cap, k, groups, nk, scaled) for cap in CAPS for k in (1, 2, 3, 4, 5, 64, 65, 1000) + tuple(K_ONE) for groups in (1, 2, 1000)
              for nk in (1, 1000)]
    CASES += [("shares", 0, k, GB2 // (1643 * B.ceil_pow2(k)) + d, 1000, scaled) for k in (1, 3, 64, 67, 1000) for d in (-1, 0, 1, 7)]
CASES += [("shround", nn, ln, k) for nn in (1, 2, 65) for ln in (1, 2, 64) for k in (1, 67)]
CASES += [("shround", GB2 // 1643, 1, 1), ("shround", (GB2 // (1643 * 128)) * 67, 1, 67)]
# plain rounds with and without a node that crosses n_e; a round of nothing but leaves at the natural slice
CASES += [("plainr", 8, 4, 0, 4), ("plainr", 7, 4, 0, 4), ("plainr", 7, 4, 4), ("plainr", 5, 8, 0), ("plainr", 13, 2, 0, 2, 6, 12, 8), ("plainr", 13, 1, 3, 12),
          ("plainr", 1000, 1) + tuple(range(0, 1000, 3)), ("plainr", 1, 1, 0), ("plainr", 600, 2) + tuple(range(0, 600, 2))]


def fold_rounds():
    """every round of the bisections of tests/test_bisect_plan_host.py's message patterns, each round once"""
    seen = []
    for n_e in (1, 2, 3, 5, 8, 9, 16, 17, 33):
        for msgs in run_tables(n_e):
            for forged in ((), (0,), (n_e - 1,), (0, n_e // 2, n_e - 1), tuple(range(n_e))):
                for L, nodes in B.folded(msgs, sorted(set(forged)))["rounds"]:
                    if (msgs, L, nodes) not in seen:
                        seen.append((msgs, L, nodes))
    return seen


FOLD_ROUNDS = fold_rounds()
for msgs, L, nodes in FOLD_ROUNDS:
    rb, rmsg = B.runs_of(msgs)
    CASES.append(("foldr", len(msgs), len(rmsg)) + tuple(rb) + tuple(rmsg) + (L,) + tuple(nodes))
CASES += [("large", "find", n, nk, nm) for n in (N_LIM, N_LIM + 1) for nk in (KEY_LIM, KEY_LIM + 1) for nm in (MSG_LIM, MSG_LIM + 1)]
CASES += [("large", "shares", k, g, nk) for k, g in ((1, 0x7FFFFFFF), (1, 0x80000000), (2, 0x7FFFFFF8), (2, 0x7FFFFFF9), (1024, 4194303), (1024, 4194304))
          for nk in (KEY_LIM, KEY_LIM + 1)]
N_PLAN_LINES = len(CASES)


def lines(model, case):
    """what the model says the program prints for a case"""
    kind, a = case[0], case[1:]
    if kind == "consts":
        one, big = model.plan_shares(model.knobs(), 1, 1, 1, 1), model.plan_shares(model.knobs(), 67, 1, 1, 1)
        p, f = model.plan_find(model.knobs(), 1, 1, 1, 0), model.plan_find(model.knobs(), 1, 1, 1, 1)
        slot_per = (f["round_per"] - 787) // 3
        return model.join("consts", [p["keep_per"], p["round_per"], f["keep_per"], slot_per, f["round_per"] - 3 * slot_per, f["round_per"], one["keep_per"],
                                     one["round_per"], big["keep_per"], big["round_per"], 96, GB2, 1 << 20])
    if kind == "find":
        return model.find_line(model.knobs(test_slice_cap=a[0]), *a[1:])
    if kind == "shares":
        return model.shares_line(model.knobs(test_slice_cap=a[0]), *a[1:])
    if kind == "shround":
        return model.shround_line(*a)
    if kind == "plainr":
        return model.plainr_line(a[0], a[1], list(a[2:]))
    if kind == "foldr":
        msgs, L, nodes = FOLD_ROUNDS[[c for c in CASES if c[0] == "foldr"].index(case)]
        return model.foldr_line(msgs, L, nodes) + " 1 1 1"
    which, x, y, z = a
    return model.join("large", [model.find_too_large(x, y, z) if which == "find" else model.shares_too_large(x, y, z)])


@pytest.fixture(scope="module", params=sorted(BUILDS))
def out(request, tmp_path_factory):
    """the program's output lines, from the plain and from the sanitizer build"""
    d = tmp_path_factory.mktemp("find_plan_" + request.param)
    src, exe = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, *BUILDS[request.param], "-o", str(exe), str(src)])
    sweeps = ["sweep %d\n" % n_e for n_e in range(1, SWEEP_MAX + 1)]
    res = subprocess.run([str(exe)], input="".join(" ".join(map(str, c)) + "\n" for c in CASES) + "".join(sweeps), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
    return res.stdout.split("\n")[:-1]


def test_against_the_model(out):
    assert len(out) == N_PLAN_LINES + SWEEP_MAX
    for case, got in zip(CASES, out):
        assert got == lines(M, case), case
    # both answers of both refusals, one slice and many, a clamped share slice, both branches of rcap occur in the grid
    assert {"large 0", "large 1"} <= set(out)
    finds = [(c, M.plan_find(M.knobs(test_slice_cap=c[1]), *c[2:])) for c in CASES if c[0] == "find"]
    assert {(c[5], p["slice"] < c[4], p["slice"] < c[2]) for c, p in finds} == set(itertools.product((0, 1), (False, True), (False, True)))
    shares = [M.plan_shares(M.knobs(test_slice_cap=c[1]), *c[2:]) for c in CASES if c[0] == "shares"]
    assert any(p["slice"] == 1 and p["round_per"] > GB2 >= p["keep_per"] for p in shares) and any(p["keep_per"] > GB2 for p in shares)


def check_regions(w, names, total, start=0):
    """every region on 256 bytes, none overlapping the next, the total the end of the last"""
    at = start
    for x in names:
        assert w[x] >= at and w[x] % 256 == 0, (x, w)
        at = w[x] + w["sizes"][x]
    assert at <= total < at + 256 and total % 256 == 0, (w, total)


# What the share check's round of leaves takes beyond 2 GB at the most, over the whole grid: the rule divides a flat 2 GB by 1643
# bytes a leaf where the layout takes 1739 (a node's fourth G1 point is not counted) and rounds eleven regions up.  An upper
# bound, reached at k = 1 -- not a claim that it is harmless; the rule is left as it is (csrc/find_plan.h).
SHARE_ROUND_OVERSHOOT = 125_477_376


def test_invariants_of_every_plan(out):
    assert out[0] == lines(M, ("consts",))                                               # (the numbers below are the header's: test_against_the_model)
    over = 0
    for case in CASES:
        kind, a = case[0], case[1:]
        if kind == "find":
            cap, n, n_keys, n_msgs, folded = a
            p = M.plan_find(M.knobs(test_slice_cap=cap), n, n_keys, n_msgs, folded)
            w, s = p["w"], p["slice"]
            check_regions(w, M.FOLD_WS if folded else M.FIND_WS, w["bytes"], 256)
            assert s <= n and (s >= 1 or n == 0) and (cap == 0 or s <= cap)
            assert p["rcap"] == (min(s, n_msgs) + 1 if folded else 0) and p["at"](s)["rn"] <= p["rcap"]
            last = p["at"](M.last_len(n, s))
            assert last["m"] <= s and last["rn"] <= p["rcap"] and last["g_settle"] * 256 >= last["m"] and last["g_leaves"] * 256 >= last["ltotal"]
            # what a slice keeps -- all but the per-call arrays of the keys and the messages -- stays below 2 GB, and so does the
            # worst round: of the plain form every leaf a node; of the folded form the bound the sweep below establishes
            assert w["bytes"] - w["sigst"] < GB2
            worst = p["round_per"] * s + 11 * 255 + 6 * 63 * 4 + 4 if folded else M.plain_round([(s, 1), (0, 0)])["bytes"]
            assert worst < GB2, (case, worst)
        elif kind == "shares":
            cap, k, groups, n_keys, scaled = a
            p = M.plan_shares(M.knobs(test_slice_cap=cap), k, groups, n_keys, scaled)
            w, s = p["w"], p["slice"]
            check_regions(w, M.SHR_WS, w["bytes"], 256)
            assert 1 <= s <= groups and (cap == 0 or s <= cap) and p["n0"] == s * k and (scaled or w["sizes"]["lam"] == 0)
            if p["round_per"] <= GB2:                                                    # (else one session alone passes 2 GB: slice 1)
                assert w["bytes"] - w["sigst"] < GB2
                worst = M.shares_round(s * k, 1, k)["w"]["bytes"]                        # every leaf a node
                assert worst <= s * k * 1739 + 11 * 255 and worst - GB2 <= SHARE_ROUND_OVERSHOOT, (case, worst - GB2)
                over = max(over, worst - GB2)
        elif kind == "shround":
            r = M.shares_round(*a)
            check_regions(r["w"], M.SHR_ROUND, r["w"]["bytes"])
            assert r["g_gather"] * 256 >= r["gtotal"] == r["slots"] * 18 and r["g_pairs"] * 256 >= r["ptotal"] == r["nn"] * 36
            assert r["g_verdict"] * 256 >= r["nn"] and 1 << r["lg"] == a[1]
        elif kind == "plainr":
            order, parts = M.plain_parts(list(a[2:]), a[1], a[0])
            r = M.plain_round(parts)
            check_regions(r["w"], r["names"], r["bytes"])
            assert sum(p["pairs"] for p in r["part"]) == sum(min(o + a[1], a[0]) - o + 1 for o in order)
            for p in r["part"]:
                assert p["g_gather"] * 256 >= p["gtotal"] and p["g_pairs"] * 256 >= p["ptotal"] == p["pairs"] * 18 and p["g_verdict"] * 256 >= p["nodes"]
        elif kind == "foldr":
            msgs, L, nodes = FOLD_ROUNDS[[c for c in CASES if c[0] == "foldr"].index(case)]
            nn, slots, nb, words = M.fold_shape(msgs, nodes, L)
            r = M.folded_round(nn, slots, nb, words)
            check_regions(r["w"], M.FOLD_ROUND, r["w"]["bytes"])
            assert slots <= 2 * nn + len(set(msgs)) and slots <= 3 * len(msgs) and nn <= len(msgs)
            assert r["g_fill"] * 256 >= r["ftotal"] == slots * 18 and r["g_codes"] * 256 >= nn
    assert over == SHARE_ROUND_OVERSHOOT                                                 # the bound is the overshoot the grid finds, not a guess


def test_the_folded_bound_on_every_small_input(out):
    """over every round of every bisection of up to 12 leaves, any run table, any forged subset of up to three leaves: a node an
    item at most, slots <= 2 nodes + runs <= 3 items, and the round's total within round_per n_e + the regions' rounding"""
    sweeps = [[int(x) for x in line.split()[1:]] for line in out[N_PLAN_LINES:]]
    assert len(sweeps) == SWEEP_MAX
    for n_e, (rounds, bad_slots, bad_bytes, bad_nodes) in enumerate(sweeps, 1):
        tables, subsets = 1 << (n_e - 1), sum(len(list(itertools.combinations(range(n_e), r))) for r in range(4))
        assert rounds >= tables * subsets and (bad_slots, bad_bytes, bad_nodes) == (0, 0, 0), n_e
    assert sweeps[1][0] == 2 * (1 + 2 + 2 + 2)                                           # n_e = 2: a round, or two where something is forged


# ---- mutants: the model with one thing wrong; each must differ from the right model somewhere on the grid
MUTANTS = {
    "the dense order dropped from the kept sum": ("keep_per = 1 + 8 + 1 + 4 + G2 + G1", "keep_per = 1 + 8 + 1 + G2 + G1"),
    "the verdict byte dropped from the round sum": ("round_per = 4 + 2 * G2 + 1 + 2 * G1 + 2 * G2 + FQ12 + 1", "round_per = 4 + 2 * G2 + 1 + 2 * G1 + 2 * G2 + FQ12"),
    "a node's fourth G1 point counted": ("round_per = K * (NODE + 3 * G1 + 4 * G2 + FQ12 + 3)", "round_per = K * (NODE + 4 * G1 + 4 * G2 + FQ12 + 3)"),
    "slack applied to the share check": ("slice_ = (2 << 30) // max(keep_per, round_per)", "slice_ = ((2 << 30) - (1 << 20)) // max(keep_per, round_per)"),
    "no slack for the finders": ("slice_len(c, ((2 << 30) - (1 << 20)) // max(keep_per, round_per))", "slice_len(c, (2 << 30) // max(keep_per, round_per))"),
    "rcap without the + 1": ("rcap = min(slice_, n_msgs) + 1 if folded else 0", "rcap = min(slice_, n_msgs) if folded else 0"),
    "rn of the slice, not of its items": ("rn=min(m, n_msgs) + 1 if folded else 0", "rn=min(n, n_msgs) + 1 if folded else 0"),
    "share slice not clamped to one": ("    slice_ = max(slice_, 1)\n", ""),
    "share slice not clamped to the sessions": ("    slice_ = min(slice_, groups)\n", ""),
    "the coefficients kept when not scaled": ("n0 * 32 if scaled else 0", "n0 * 32"),
    "one pair a node in the share round": ("nn * 2 * G1, nn * 2 * G2", "nn * G1, nn * 2 * G2"),
    "a part's pairs without the node's own": ("nodes * (ln + 1) * G1, nodes * (ln + 1) * G2", "nodes * ln * G1, nodes * (ln + 1) * G2"),
    "B sums per slot": ("sizes = (tab_words * 4, slots, nb, nb * G1", "sizes = (tab_words * 4, slots, nb, slots * G1"),
    "n_msgs limit in G1 points": ("n_msgs > (2 << 30) // G2", "n_msgs > (2 << 30) // G1"),
    "share limit strict": ("k * groups > 0xFFFFFFF0", "k * groups >= 0xFFFFFFF0"),
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
    assert any(lines(m, case) != lines(M, case) for case in CASES), name
