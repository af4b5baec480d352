"""Batched threshold recovery without a GPU: the scalar-field arithmetic and the Lagrange routine of csrc/fr_scalar.h
compiled for the host against Python integers and the reference's vectors (tests/golden/lagrange.json), and the three
Threshold.*_batch methods and PrivateKey.sign_threshold_batch -- their assertions and routing -- under a provider without
the device entry points (the host loop) and under a host provider of them (tests/lagrange_vectors.HostLagrange)."""
import os
import random
import subprocess

import pytest

from lagrange_vectors import (HostLagrange, N, be32, check_batches, group_coeffs, group_players, host_coeffs, ints32,
                              unit_signatures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")
R = 2**256

HOST_TEST = r'''
#include "fr_scalar.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
static void le(const char* h, uint32_t s[8]) { for (int j = 0; j < 8; j++) { char b[9]; memcpy(b, h + 8 * (7 - j), 8); b[8] = 0; s[j] = (uint32_t)strtoul(b, 0, 16); } }
static void pl(const uint32_t s[8]) { for (int j = 7; j >= 0; j--) printf("%08x", s[j]); }
static char op[16], a[70000], b[70000];
int main() {
    while (scanf("%15s %69999s %69999s", op, a, b) == 3) {
        if (!strcmp(op, "lag")) {                        // k points of 64 hex digits -> status, k coefficients
            uint32_t k = (uint32_t)strlen(a) / 64;
            uint8_t* xb = (uint8_t*)malloc(32 * k); uint8_t* ob = (uint8_t*)malloc(32 * k); uint32_t* w = (uint32_t*)malloc(64 * k);
            for (uint32_t i = 0; i < 32 * k; i++) { unsigned v; sscanf(a + 2 * i, "%2x", &v); xb[i] = (uint8_t)v; }
            printf("%d ", frs::lagrange_group(xb, k, w, ob));
            for (uint32_t i = 0; i < 32 * k; i++) printf("%02x", ob[i]);
            free(xb); free(ob); free(w);
        } else if (!strcmp(op, "dot")) {                 // L, y as 32 bytes big-endian -> L (y mod n)
            uint8_t lb[32], yb[32]; uint32_t t[8];
            for (int i = 0; i < 32; i++) { unsigned v; sscanf(a + 2 * i, "%2x", &v); lb[i] = (uint8_t)v; sscanf(b + 2 * i, "%2x", &v); yb[i] = (uint8_t)v; }
            frs::dot_term(lb, yb, t); pl(t);
        } else {
            uint32_t x[8], y[8], r[8];
            le(a, x); le(b, y);
            if (!strcmp(op, "mul")) { frs::to_mont(x, x); frs::to_mont(y, y); frs::mul(r, x, y); frs::from_mont(r, r); pl(r); }
            else if (!strcmp(op, "mraw")) { frs::mul(r, x, y); pl(r); }            // a b / R
            else if (!strcmp(op, "tom")) { frs::to_mont(r, x); pl(r); }
            else if (!strcmp(op, "sqr")) { frs::to_mont(x, x); frs::sqr(r, x); frs::from_mont(r, r); pl(r); }
            else if (!strcmp(op, "inv")) { frs::to_mont(x, x); frs::inv(r, x); frs::from_mont(r, r); pl(r); }
            else if (!strcmp(op, "add")) { frs::add(r, x, y); pl(r); }
            else if (!strcmp(op, "sub")) { frs::sub(r, x, y); pl(r); }
            else if (!strcmp(op, "neg")) { frs::neg(r, x); pl(r); }
            else if (!strcmp(op, "zero")) { printf("%d%d", (int)frs::is_zero(x), (int)frs::below_n(x)); }
        }
        printf("\n");
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def fr_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("fr")
    src, exe = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, "-o", str(exe), str(src)])
    return str(exe)


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return out[:len(lines)]


@pytest.fixture(scope="module")
def lag(golden):
    return golden("lagrange.json")


def test_montgomery_arithmetic_matches_python_ints(fr_exe):
    rnd = random.Random(31)
    edge = [0, 1, 2, N - 1, N - 2, R % N, R * R % N, (N + 1) // 2, 2**255 % N, 2**32 - 1, 2**32]
    vals = edge + [rnd.randrange(N) for _ in range(60)]
    lines, want = [], []
    for a in vals:
        for b in edge + vals[-4:]:
            for op, w in (("mul", a * b % N), ("mraw", a * b * pow(R, -1, N) % N), ("add", (a + b) % N), ("sub", (a - b) % N)):
                lines.append("%s %064x %064x" % (op, a, b))
                want.append(w)
        for op, w in (("sqr", a * a % N), ("inv", pow(a, N - 2, N)), ("neg", -a % N), ("tom", a * R % N)):
            lines.append("%s %064x %064x" % (op, a, 0))
            want.append(w)
    got = _run(fr_exe, lines)
    assert [int(g, 16) for g in got] == want
    # inverses really invert; is_zero / below_n on the boundary
    assert all(a * pow(a, N - 2, N) % N == 1 for a in vals if a)
    probe = [0, 1, N - 1, N, N + 1, 2**256 - 1]
    assert _run(fr_exe, ["zero %064x %064x" % (v, 0) for v in probe]) == ["11", "01", "01", "00", "00", "00"]
    ys = [0, 1, N - 1, N, N + 5, 2**256 - 1] + [rnd.randrange(2**256) for _ in range(40)]
    ls = [rnd.randrange(N) for _ in ys]
    got = _run(fr_exe, ["dot %064x %064x" % (l, y) for l, y in zip(ls, ys)])
    assert [int(g, 16) for g in got] == [l * y % N for l, y in zip(ls, ys)]


def test_header_lagrange_routine_on_every_fixture_group(fr_exe, lag):
    assert sorted({g["k"] for g in lag["groups"]}) == [1, 2, 3, 5, 63, 64, 65, 67, 128, 200]
    assert {g["kind"] for g in lag["groups"]} == {"small", "u32", "2^200", "top", "mixed"}
    got = _run(fr_exe, ["lag %s -" % be32(group_players(g)).hex() for g in lag["groups"]])
    for g, line in zip(lag["groups"], got):
        st, co = line.split()
        assert st == "1" and ints32(bytes.fromhex(co)) == group_coeffs(g), (g["k"], g["kind"])
    # where the reference asserts: status 0 and zeros
    assert all(a["raises"] for a in lag["asserts"])
    got = _run(fr_exe, ["lag %s -" % be32([int(x, 16) for x in a["X"]]).hex() for a in lag["asserts"]])
    for a, line in zip(lag["asserts"], got):
        st, co = line.split()
        assert st == "0" and set(co) == {"0"}, a["what"]


def test_host_mirror_and_host_provider_agree_with_the_fixture(lag):
    from bls_py.threshold import Threshold
    for g in lag["groups"]:
        if g["k"] > 67:
            continue
        X = group_players(g)
        assert [int(l) for l in Threshold.lagrange_coeffs_at_zero(X)] == group_coeffs(g)
        assert host_coeffs(X) == (group_coeffs(g), 1)


@pytest.fixture
def plain_provider():
    """a provider WITHOUT the device entry points (what the CPU oracle provider of the scheme tests is): the host loop"""
    from bls_py import backend
    old = backend._provider

    class Plain:
        calls = []

        def g2_msm(self, pts, scalars, k, groups=1):
            self.calls.append(("g2_msm", k, groups))
            return HostLagrange._g2_msm(pts, scalars, k, groups)
    p = Plain()
    backend.use(p)
    yield p
    backend.use(old)


@pytest.fixture
def host_lagrange():
    from bls_py import backend
    old = backend._provider
    p = HostLagrange(None)
    backend.use(p)
    yield p
    backend.use(old)


def test_batches_take_the_host_loop_without_the_entry_points(lag, plain_provider):
    check_batches(lag)
    assert {c[0] for c in plain_provider.calls} == {"g2_msm"}              # (aggregate_unit_sigs' own sum, one per subset)
    assert len(plain_provider.calls) == 10


def test_batches_through_the_device_contract(lag, host_lagrange):
    check_batches(lag, shuffle_seed=4)
    ks = sorted({g["k"] for g in lag["groups"]})
    per_k = {k: sum(1 for g in lag["groups"] if g["k"] == k) for k in ks}
    lagr = [c for c in host_lagrange.calls if c[0] == "lagrange_at_zero"]
    assert sorted(lagr) == sorted(("lagrange_at_zero", k, per_k[k]) for k in ks)         # one call per distinct k
    dots = [c for c in host_lagrange.calls if c[0] == "fr_interpolate_at_zero"]
    assert sorted(dots) == sorted(("fr_interpolate_at_zero", k, per_k[k]) for k in ks)
    assert [c for c in host_lagrange.calls if c[0] == "threshold_combine"] == [("threshold_combine", 3, 10)]
    assert not [c for c in host_lagrange.calls if c[0] == "g2_msm"]


def test_assertion_cases_raise_before_device_work(lag, host_lagrange):
    from bls_py.threshold import Threshold
    cb = lag["combine"]
    unit = unit_signatures(cb)
    good = [1, 2, 3]
    for a in lag["asserts"]:
        X = [int(x, 16) for x in a["X"]]
        with pytest.raises(AssertionError):
            Threshold.lagrange_coeffs_at_zero(X)
        host_lagrange.calls.clear()
        with pytest.raises(AssertionError):
            Threshold.lagrange_coeffs_at_zero_batch([good, X, good])
        with pytest.raises(AssertionError):
            Threshold.interpolate_at_zero_batch([good, X], [[1, 2, 3], [4] * len(X)])
        with pytest.raises(AssertionError):
            Threshold.aggregate_unit_sigs_batch([unit[:3], unit[:len(X)]], [good, X], 3)
        assert host_lagrange.calls == [], a["what"]
    assert Threshold.lagrange_coeffs_at_zero_batch([]) == []
    assert Threshold.interpolate_at_zero_batch([], []) == []
    assert Threshold.aggregate_unit_sigs_batch([], [], 3) == []
    assert host_lagrange.calls == []


def test_host_path_routing(lag, host_lagrange):
    from bls_py.ec import EC, default_ec
    from bls_py.fields import Fq
    from bls_py.threshold import Threshold
    big = list(range(1, HostLagrange.LAGRANGE_MAX_K + 2))                     # k above the device limit
    Xs = [[1, 2, 3], [5, -2, 7], [], [4, 9], [True, 2, 3], [Fq(N, 6), 1], [2**200, N - 1], [7]]
    want = [Threshold.lagrange_coeffs_at_zero(X) for X in Xs]
    host_lagrange.calls.clear()
    assert Threshold.lagrange_coeffs_at_zero_batch(Xs) == want
    # device: [1, 2, 3] (k = 3), [4, 9] and [2^200, n - 1] (k = 2), [7] (k = 1); the negative player, the empty group, the
    # bool and the Fq take the host loop
    assert sorted(host_lagrange.calls) == [("lagrange_at_zero", 1, 1), ("lagrange_at_zero", 2, 2), ("lagrange_at_zero", 3, 1)]
    host_lagrange.calls.clear()
    got = Threshold.lagrange_coeffs_at_zero_batch([big[:5], big])
    assert host_lagrange.calls == [("lagrange_at_zero", 5, 1)]
    assert [int(l) for l in got[1][:3]] == [int(l) for l in Threshold.lagrange_coeffs_at_zero(big)[:3]]
    # another curve object: the host loop
    other = EC(*default_ec)
    host_lagrange.calls.clear()
    assert Threshold.lagrange_coeffs_at_zero_batch([[1, 2, 3]], other) == [Threshold.lagrange_coeffs_at_zero([1, 2, 3], other)]
    assert host_lagrange.calls == []
    # interpolate: a value list of another length, or holding an Fq of another modulus, is the host loop's
    Ys = [[10, 20, 30], [1, 2, 3], [], [Fq(N, 5), 6], [1, 2, 3], [1, 2], [3, 4, 5], [Fq(N, 9)]]
    want = [Threshold.interpolate_at_zero(X, Y) for X, Y in zip(Xs, Ys)]
    host_lagrange.calls.clear()
    assert Threshold.interpolate_at_zero_batch(Xs, Ys) == want
    assert sorted(host_lagrange.calls) == [("fr_interpolate_at_zero", 1, 1), ("fr_interpolate_at_zero", 2, 1),
                                           ("fr_interpolate_at_zero", 3, 1)]
    # aggregate: mismatched lengths go to the single call (which sums over the shorter list on the host provider)
    cb = lag["combine"]
    unit = unit_signatures(cb)
    sub = cb["subsets"][0]
    sig_groups = [[unit[p - 1] for p in sub["players"]], [unit[0], unit[1]], [unit[0], unit[1], unit[2]]]
    player_groups = [sub["players"], [1, 2, 3], [1, -5 % N - N, 3]]
    host_lagrange.calls.clear()
    got = Threshold.aggregate_unit_sigs_batch(sig_groups, player_groups, 99)       # T is unused
    assert host_lagrange.calls[0] == ("threshold_combine", 3, 1)
    assert got[0].serialize().hex() == sub["aggregate"]
    assert [c[0] for c in host_lagrange.calls[1:]] == ["g2_msm", "g2_msm"]         # the two host-loop groups
    assert got[2] == Threshold.aggregate_unit_sigs(sig_groups[2], player_groups[2], 3)


def test_sign_threshold_batch_equals_sign_threshold(lag, host_lagrange):
    from bls_py.keys import PrivateKey
    from bls_py.threshold import Threshold
    cb = lag["combine"]
    shares = [int(s, 16) for s in cb["shares"]]
    msg = bytes.fromhex(cb["msg"])
    for sub in cb["subsets"][:3]:
        players = sub["players"]
        sks = [PrivateKey(shares[p - 1]) for p in players]
        host_lagrange.calls.clear()
        out = PrivateKey.sign_threshold_batch(sks, msg, players)
        assert [c[0] for c in host_lagrange.calls] == ["lagrange_at_zero", "hash_to_g2", "g2_msm"]
        assert host_lagrange.calls[2] == ("g2_msm", 1, 3)
        lam = Threshold.lagrange_coeffs_at_zero(players)
        unit = unit_signatures(cb)
        for sig, p, l in zip(out, players, lam):
            assert sig.value == unit[p - 1].value * int(l)                      # lambda_p share_p H(m)
        total = out[0].value + out[1].value + out[2].value
        from bls_py.signature import Signature
        assert Signature.from_g2(total).serialize().hex() == cb["master"]
    with pytest.raises(ValueError):
        PrivateKey.sign_threshold_batch([PrivateKey(1)], msg, [1, 2])
    assert PrivateKey.sign_threshold_batch([], msg, []) == []
