"""The host plan of the three bisecting checks, csrc/bisect_plan.h (the layout helper, the halving rule and the round loop, the
plain and the folded round plan, the run-table check), compiled for the host as a stand-alone program -- once with -O2, once
under AddressSanitizer and UBSan, the run table in heap blocks of exactly its length -- and compared with tests/bisect_model.py:
whole bisections under the verdict rule "a node fails iff it holds a forged position", the `stats` values the device tests pin,
and the invariants of every folded table."""
import itertools
import os
import subprocess

import pytest

import bisect_model as M
from test_gpu_batch_find import lg, positions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")

# one case per line; a case prints one line per round and a last line `end <rounds> <tests> <pairs> : <leaves named>`
#   pow2 n | layout unit start counts.. | runs n_e n_runs cap rb[cap]
#   plain n_e forged..                       round: `L : nodes.. : full nodes, L, short nodes, its length`
#   fold n_e n_runs rb[n_runs + 1] rmsg[n_runs] forged..
#                                            round: `L : nodes.. : pair counts.. : slots nb 6 offsets : the table`
#   share k sessions (count forged..) per session    round: `len : session offset ..`
HOST_TEST = r'''
#include "bisect_plan.h"
#include <stdio.h>
#include <iostream>
#include <sstream>
#include <string>
struct SNode { uint32_t session, offset; };
template <class T> std::vector<T> some(std::istream& in, size_t n) { std::vector<T> v(n); for (T& x : v) in >> x; v.shrink_to_fit(); return v; }
template <class T> std::vector<T> rest(std::istream& in) { std::vector<T> v; T x; while (in >> x) v.push_back(x); return v; }
static bool holds(const std::vector<uint32_t>& f, size_t lo, size_t hi) { for (uint32_t x : f) if (x >= lo && x < hi) return true; return false; }
template <class N> void finish(const bisect::State<N>& b, const std::vector<uint32_t>& named, int n) {
    uint64_t st[3] = {0, 0, 0};
    b.report(st, n);
    b.report(nullptr, n);
    printf("end %llu %llu %llu :", (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2]);
    for (uint32_t x : named) printf(" %u", x);
    printf("\n");
}
int main() {
    std::string line, op;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        in >> op;
        if (op == "pow2") { size_t n; in >> n; printf("%zu\n", bisect::ceil_pow2(n)); }
        else if (op == "layout") {
            size_t unit, start;
            in >> unit >> start;
            bisect::Layout l{unit, start};
            for (size_t x : rest<size_t>(in)) printf("%zu ", l.take(x));
            printf("%zu\n", l.off);
        } else if (op == "runs") {
            uint32_t n_e, n_runs; size_t cap;
            in >> n_e >> n_runs >> cap;
            const std::vector<uint32_t> rb = some<uint32_t>(in, cap);
            printf("%d\n", bisect::run_table_ok(n_e, n_runs, cap, rb.data()) ? 1 : 0);
        } else if (op == "plain" || op == "fold") {
            const bool fold = op == "fold";
            uint32_t n_e, n_runs = 0;
            in >> n_e;
            if (fold) in >> n_runs;
            const std::vector<uint32_t> rb = some<uint32_t>(in, fold ? n_runs + 1 : 0), rmsg = some<uint32_t>(in, n_runs), forged = rest<uint32_t>(in);
            std::vector<uint32_t> named;
            bisect::State<uint32_t> b;
            bisect::FoldPlan p;
            b.nodes.assign(1, 0u);
            bisect::run(b, bisect::ceil_pow2(n_e), n_e, [&](std::vector<uint32_t>& nodes, size_t L, uint8_t* verdict) {
                printf("%zu :", L);
                if (fold) {
                    bisect::fold_round(nodes, L, n_e, rb.data(), rmsg.data(), n_runs, p);
                    for (uint32_t o : nodes) printf(" %u", o);
                    printf(" :");
                    for (const bisect::NodeRec& nd : p.order) printf(" %u", nd.cnt);
                    printf(" : %zu %zu %zu %zu %zu %zu %zu %zu :", p.slots, p.nb, p.t_first, p.t_off, p.t_rng2, p.t_node, p.t_msg, p.t_rng1);
                    for (uint32_t x : p.tab) printf(" %u", x);
                    b.pairs += p.slots;
                } else {
                    bisect::Part part[2];
                    bisect::plain_round(nodes, L, n_e, part);
                    for (uint32_t o : nodes) printf(" %u", o);
                    printf(" : %zu %zu %zu %zu", part[0].nodes, part[0].len, part[1].nodes, part[1].len);
                    for (const bisect::Part& q : part) b.pairs += q.nodes * (q.len + 1);
                }
                printf("\n");
                for (size_t i = 0; i < nodes.size(); i++) {
                    verdict[i] = holds(forged, nodes[i], nodes[i] + L) ? 0 : 1;
                    if (L == 1 && !verdict[i]) named.push_back(nodes[i]);
                }
                return 0;
            });
            finish(b, named, 3);
        } else if (op == "share") {
            uint32_t k, sessions;
            in >> k >> sessions;
            std::vector<std::vector<uint32_t>> forged;
            for (uint32_t s = 0; s < sessions; s++) { size_t cnt; in >> cnt; forged.push_back(some<uint32_t>(in, cnt)); }
            std::vector<uint32_t> named;
            bisect::State<SNode> b;
            for (uint32_t s = 0; s < sessions; s++) b.nodes.push_back({s, 0u});
            bisect::run(b, bisect::ceil_pow2(k), k, [&](std::vector<SNode>& nodes, size_t len, uint8_t* verdict) {
                printf("%zu :", len);
                for (size_t i = 0; i < nodes.size(); i++) {
                    printf(" %u %u", nodes[i].session, nodes[i].offset);
                    verdict[i] = holds(forged[nodes[i].session], nodes[i].offset, nodes[i].offset + len) ? 0 : 1;
                    if (len == 1 && !verdict[i]) named.push_back(nodes[i].session * k + nodes[i].offset);
                }
                printf("\n");
                return 0;
            });
            finish(b, named, 2);
        }
    }
    return 0;
}
'''

BUILDS = {"O2": ["-O2"], "sanitizers": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def ints(s):
    return [int(x) for x in s.split()]


def subsets(n):
    return [p for r in range(n + 1) for p in itertools.combinations(range(n), r)]


def forged_sets(n_e):
    return subsets(n_e) if n_e <= 8 else positions(n_e)


def run_tables(n_e):
    """the messages of n_e leaves: one message, n_e messages, an uneven split (runs of 1, 2, 3, .. leaves, the messages not
    consecutive numbers)"""
    uneven = [7 * r + 2 for r in range(n_e) for _ in range(r + 1)][:n_e]
    out = []
    for msgs in ([5] * n_e, list(range(n_e)), uneven):
        if msgs not in out:
            out.append(msgs)
    return out


SIZES = list(range(1, 9)) + [9, 15, 16, 17, 33]
PLAIN = [(n_e, f) for n_e in SIZES for f in forged_sets(n_e)]
FOLD = [(msgs, f) for n_e in SIZES for msgs in run_tables(n_e) for f in forged_sets(n_e)]
SHARE = [(k, [pats[(s + c) % len(pats)] for s in range(sessions)]) for k in (1, 2, 3, 5, 8) for sessions in (1, 3)
         for pats in [subsets(k) if k <= 5 else positions(k)] for c in range(len(pats))]
LAYOUTS = [(256, 256, [0, 1, 255, 256, 257, 1000, 96 * 33]), (256, 0, [4, 0, 512]), (64, 0, [1, 64, 65, 0, 130, 2]), (4, 0, [3, 4, 5])]
# run tables the check refuses: no run, more runs than entries, a first run that does not begin at 0, a last that does not end at n_e
RUNS = [((5, 2, 3, [0, 3, 5]), 1), ((5, 1, 2, [0, 5]), 1), ((5, 0, 3, [0, 3, 5]), 0), ((5, 3, 3, [0, 3, 5]), 0), ((5, 2, 3, [1, 3, 5]), 0),
        ((5, 2, 3, [0, 3, 4]), 0)]


def case_lines():
    j = lambda v: " ".join(map(str, v))
    lines = ["pow2 %d" % n for n in range(1, 70)]
    lines += ["layout %d %d %s" % (u, s, j(c)) for u, s, c in LAYOUTS]
    lines += ["runs %d %d %d %s" % (n_e, n_runs, cap, j(rb)) for (n_e, n_runs, cap, rb), _ in RUNS]
    lines += ["plain %d %s" % (n_e, j(f)) for n_e, f in PLAIN]
    for msgs, f in FOLD:
        rb, rmsg = M.runs_of(msgs)
        lines.append("fold %d %d %s %s %s" % (len(msgs), len(rmsg), j(rb), j(rmsg), j(f)))
    lines += ["share %d %d %s" % (k, len(fs), " ".join("%d %s" % (len(f), j(f)) for f in fs)) for k, fs in SHARE]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module", params=sorted(BUILDS))
def out(request, tmp_path_factory):
    """the program's output lines, from the plain and from the sanitizer build"""
    d = tmp_path_factory.mktemp("bisect_" + request.param)
    src, exe = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, *BUILDS[request.param], "-o", str(exe), str(src)])
    res = subprocess.run([str(exe)], input=case_lines(), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
    return iter(res.stdout.split("\n")[:-1])


def bisection(out):
    """-> the rounds' lines, each split at its colons, and (stats, named leaves)"""
    rounds = []
    for line in out:
        parts = [ints(p) for p in line.replace("end", "").split(":")]
        if line.startswith("end"):
            return rounds, (tuple(parts[0]), parts[1])
        rounds.append(parts)
    raise AssertionError("no end line")


def check_table(msgs, L, nodes, cnts, head, tab):
    """the invariants of a folded table, and its content against the model's ranges"""
    n_e, nn = len(msgs), len(nodes)
    slots, nb, *offs = head
    assert slots == sum(cnts) and nb == slots - nn and cnts == sorted(cnts)                    # pair counts are non-decreasing
    assert (offs, len(tab)) == M.layout(64, 0, [nn + 1, nn, 2 * nn, slots, slots, 2 * nb])
    t_first, t_off, t_rng2, t_node, t_msg, t_rng1 = offs
    first = tab[t_first:t_first + nn + 1]
    assert all(a < b for a, b in zip(first, first[1:])) and first[0] == 0 and first[nn] == slots
    assert tab[t_off:t_off + nn] == nodes
    for i, off in enumerate(nodes):
        end = min(off + L, n_e)
        assert tab[t_rng2 + 2 * i:t_rng2 + 2 * i + 2] == [off, end]
        assert first[i + 1] - first[i] == cnts[i]
        assert tab[t_node + first[i]:t_node + first[i + 1]] == [i] * cnts[i]                   # node_of agrees with first
        got = []
        for sl in range(first[i] + 1, first[i + 1]):
            bi = sl - i - 1
            got.append((tab[t_msg + sl], tab[t_rng1 + 2 * bi], tab[t_rng1 + 2 * bi + 1]))
        # the ranges are not empty, adjacent, and together [off, end); each slot's message is its run's
        assert all(lo < hi for _, lo, hi in got) and got[0][1] == off and got[-1][2] == end
        assert all(a[2] == b[1] for a, b in zip(got, got[1:]))
        assert all(msgs[lo:hi] == [m] * (hi - lo) for m, lo, hi in got)
        assert got == M.pair_ranges(msgs, off, end)


def test_against_the_model(out):
    assert [int(next(out)) for _ in range(1, 70)] == [M.ceil_pow2(n) for n in range(1, 70)]
    for u, s, c in LAYOUTS:
        offs, end = M.layout(u, s, c)
        assert ints(next(out)) == offs + [end]
    for (n_e, n_runs, cap, rb), want in RUNS:
        assert int(next(out)) == want == int(M.run_table_ok(n_e, n_runs, cap, rb))
    for n_e, f in PLAIN:
        m = M.plain(n_e, f)
        rounds, (stats, named) = bisection(out)
        assert sorted(named) == list(f) == sorted(m["named"]) and stats == m["stats"]
        assert [(r[0][0], r[1]) for r in rounds] == m["rounds"]
        for (L,), nodes, (nf, lf, ns, ls) in rounds:
            short = [o for o in nodes if o + L > n_e]
            assert (nf, lf, ns) == (len(nodes) - len(short), L, len(short)) and ns <= 1 and nodes[nf:] == short
            assert ls == (n_e - short[0] if short else 0)
        if not f:
            assert stats == (1, 1, n_e + 1)
        if len(f) == 1:
            assert stats[1] <= 1 + 2 * lg(n_e) and stats[0] <= lg(n_e) + 1
        if n_e == 8 and len(f) == 8:
            assert stats[:2] == (4, 15)
    for msgs, f in FOLD:
        m = M.folded(msgs, f)
        rounds, (stats, named) = bisection(out)
        assert sorted(named) == list(f) == sorted(m["named"]) and stats == m["stats"]
        assert [(r[0][0], r[1]) for r in rounds] == m["rounds"]
        for (L,), nodes, cnts, head, tab in rounds:
            check_table(msgs, L, nodes, cnts, head, tab)
        if not f:
            assert stats == (1, 1, len(set(msgs)) + 1)
    for k, fs in SHARE:
        m = M.shares(k, fs)
        rounds, (stats, named) = bisection(out)
        assert named == [s * k + j for s, f in enumerate(fs) for j in f] and m["named"] == [set(f) for f in fs]
        assert stats == m["stats"] + (0,)
        assert [(r[0][0], list(zip(r[1][::2], r[1][1::2]))) for r in rounds] == m["rounds"]
        if not any(fs):
            assert stats == (1, len(fs), 0)
    assert next(out, None) is None


def test_the_values_the_device_tests_pin():
    """the model alone: the `stats` that tests/test_gpu_batch_find.py, test_gpu_verify_find_folded.py and test_gpu_sigshares.py
    assert on the device"""
    assert M.plain(2, (1,))["stats"] == (2, 3, 7) and M.plain(2, ())["stats"] == (1, 1, 3)
    assert M.folded([0, 0], ())["stats"] == (1, 1, 2)
    assert M.folded([0, 0], (1,))["stats"] == M.folded([0, 0], (0,))["stats"] == (2, 3, 6)
    assert M.folded([0, 1], (1,))["stats"] == (2, 3, 7)
    assert M.plain(8, range(8))["stats"][:2] == (4, 15)
    assert M.shares(2, [(1,)])["stats"] == (2, 3) and M.shares(64, [()] * 5)["stats"] == (1, 5)
    for n in (64, 100):
        for at in range(n):
            rounds, tests, _ = M.plain(n, (at,))["stats"]
            assert tests <= 1 + 2 * lg(n) and rounds <= lg(n) + 1
