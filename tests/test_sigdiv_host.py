"""Signature.divide_by's scalar side without a GPU: csrc/sigdiv.h compiled for the host against Python integers -- the
quotient scalar (n - a_0 / b_0) mod n, the cross test a_e b_0 == a_0 b_e of every further entry, the statuses, and the point
negation of the plain path."""
import os
import random
import subprocess

import pytest

from bls_py import hostmath as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")
N = H.N
EDGE = [0, 1, N - 1, N, N + 1, 2**256 - 1]

HOST_TEST = r'''
#include "sigdiv.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
static char op[16], a[70000], b[70000];
static uint8_t* unhex(const char* h, size_t* n) {
    *n = strlen(h) / 2;
    uint8_t* o = (uint8_t*)malloc(*n + 1);
    for (size_t i = 0; i < *n; i++) { unsigned v; sscanf(h + 2 * i, "%2x", &v); o[i] = (uint8_t)v; }
    return o;
}
int main() {
    while (scanf("%15s %69999s %69999s", op, a, b) == 3) {
        size_t na, nb;
        uint8_t* xa = unhex(a, &na); uint8_t* xb = unhex(b, &nb);
        if (!strcmp(op, "div")) {                         // k dividend and k divisor exponents -> status nonunit scalar
            uint8_t sc[32]; int nonunit = -1;
            const int st = sigdiv::divisor(xa, xb, na / 32, sc, &nonunit);
            printf("%d %d ", st, nonunit);
            for (int i = 0; i < 32; i++) printf("%02x", sc[i]);
        } else if (!strcmp(op, "neg")) {                  // a 192-byte point -> its negative (b is ignored)
            uint32_t in[48], out[48];
            memcpy(in, xa, 192);
            sigdiv::neg_point(in, out);
            const uint8_t* o = (const uint8_t*)out;
            for (int i = 0; i < 192; i++) printf("%02x", o[i]);
            sigdiv::neg_point(in, in);                    // in place gives the same
            printf(" %d", memcmp(in, out, 192));
        }
        printf("\n");
        free(xa); free(xb);
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("sigdiv")
    src, out = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, "-o", str(out), str(src)])
    return str(out)


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return out[:len(lines)]


def hex32(vals):
    return "".join("%064x" % v for v in vals)


def model(a, b):
    """(status, nonunit, scalar) of a divisor with the exponents a, b (any values below 2^256), from Python integers: the
    reference's quotient per entry, compared as it compares them"""
    if any(x % N == 0 for x in b):
        return 2, 0, 0
    qs = [x * pow(y, -1, N) % N for x, y in zip(a, b)]
    if any(q != qs[0] for q in qs):
        return 1, 0, 0
    return 0, int(qs[0] != 1), -qs[0] % N


def check(exe, cases):
    got = _run(exe, ["div %s %s" % (hex32(a), hex32(b)) for a, b in cases])
    for (a, b), line in zip(cases, got):
        st, nonunit, sc = model(a, b)
        assert line == "%d %d %064x" % (st, nonunit, sc), (a[:3], b[:3], len(a))


def test_single_entries_over_the_edge_exponents(exe):
    rnd = random.Random(44)
    vals = EDGE + [rnd.randrange(2**256) for _ in range(6)] + [rnd.randrange(1, N) for _ in range(6)]
    check(exe, [([a], [b]) for a in vals for b in vals])


def test_two_entries_over_the_edge_exponents(exe):
    """every pair of edge values as the second entry of a divisor whose first entry is (3, 7), (0, 5) or (N - 1, N - 1)"""
    check(exe, [([a0, a], [b0, b]) for a0, b0 in ((3, 7), (0, 5), (N - 1, N - 1), (2**256 - 1, N + 1)) for a in EDGE for b in EDGE])


@pytest.mark.parametrize("q", [1, N - 1, 0x1234567, 2])
def test_a_divisor_of_257_entries(exe, q):
    rnd = random.Random(q)
    b = [rnd.randrange(1, N) for _ in range(257)]
    a = [q * y % N for y in b]
    cases = [(a, b)]
    for e in (1, 256):                                       # a single mismatch, early and in the last entry
        bad = list(a)
        bad[e] = (bad[e] + 1) % N
        cases.append((bad, b))
    for e, z in ((0, 0), (0, N), (1, 0), (256, N), (128, 0)):   # b = 0 and b = n: status 2, wherever it stands
        zb = list(b)
        zb[e] = z
        cases.append((a, zb))
    mixed = list(b)                                          # a zero outranks a mismatch
    mixed[200] = N
    bad = list(a)
    bad[3] = (bad[3] + 1) % N
    cases.append((bad, mixed))
    # unreduced forms of the same exponents give the same scalar
    cases.append(([x + N if x + N < 2**256 else x for x in a], [y + N if y + N < 2**256 else y for y in b]))
    check(exe, cases)
    st, nonunit, sc = model(a, b)
    assert (st, nonunit, sc) == (0, int(q != 1), N - q)


def test_negation_of_twist_points(exe):
    rnd = random.Random(45)
    P = H.Q
    pts = [bytes(192)]
    for _ in range(4):
        x = [rnd.randrange(P), rnd.randrange(P)]
        pts.append(b"".join(v.to_bytes(48, "big") for v in x + [rnd.randrange(1, P), rnd.randrange(1, P)]))
    pts.append(b"".join(v.to_bytes(48, "big") for v in (5, 6, 0, 7)))          # a zero component stays zero
    pts.append(b"".join(v.to_bytes(48, "big") for v in (5, 6, 1, P - 1)))
    got = _run(exe, ["neg %s 00" % p.hex() for p in pts])
    for p, line in zip(pts, got):
        v = [int.from_bytes(p[48 * i:48 * (i + 1)], "big") for i in range(4)]
        want = b"".join(c.to_bytes(48, "big") for c in (v[0], v[1], -v[2] % P, -v[3] % P))
        assert line == want.hex() + " 0"
