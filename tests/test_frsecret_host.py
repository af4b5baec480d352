"""The scalar-field work on secrets without a GPU: the masked forms of csrc/fr_scalar.h (mul_masked, add_masked,
dot_term_masked and the polynomial evaluation on them) compiled for the host against Python integers and against the
branching forms beside them, the serial rendering of k_fr_poly_eval_secret against every dealer of tests/golden/dkg.json,
and the secret=True keyword of the three threshold calls -- under a provider without the entries (it raises) and under a
host provider of them (tests/frsecret_vectors.HostFrSecret)."""
import os
import random
import subprocess

import pytest

from frsecret_vectors import HostFrSecret, N, R, be32, dealers, ints32
from lagrange_vectors import HostLagrange, group_players, group_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")

HOST_TEST = r'''
#include "fr_scalar.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
static void le(const char* h, uint32_t s[8]) { for (int j = 0; j < 8; j++) { char b[9]; memcpy(b, h + 8 * (7 - j), 8); b[8] = 0; s[j] = (uint32_t)strtoul(b, 0, 16); } }
static void pl(const uint32_t s[8]) { for (int j = 7; j >= 0; j--) printf("%08x", s[j]); }
static uint8_t* bytes(const char* h, size_t* n) {
    *n = strlen(h) / 2;
    uint8_t* b = (uint8_t*)malloc(*n + 1);
    for (size_t i = 0; i < *n; i++) { unsigned v; sscanf(h + 2 * i, "%2x", &v); b[i] = (uint8_t)v; }
    return b;
}
static char op[16], a[70000], b[70000];
int main() {
    while (scanf("%15s %69999s %69999s", op, a, b) == 3) {
        if (!strcmp(op, "poly")) {                       // t coefficients, n_x points (64 hex digits each) -> n_x values
            size_t cn, xn;
            uint8_t* cb = bytes(a, &cn); uint8_t* xb = bytes(b, &xn);
            uint32_t t = (uint32_t)(cn / 32), n_x = (uint32_t)(xn / 32);
            uint32_t* w = (uint32_t*)malloc(32 * t); uint8_t* ob = (uint8_t*)malloc(32 * n_x);
            frs::poly_eval_masked(cb, t, xb, n_x, w, ob);
            for (uint32_t i = 0; i < 32 * n_x; i++) printf("%02x", ob[i]);
            free(cb); free(xb); free(w); free(ob);
        } else if (!strcmp(op, "dot") || !strcmp(op, "dotm")) {          // L, y as 32 bytes big-endian -> L (y mod n)
            size_t n; uint8_t* lb = bytes(a, &n); uint8_t* yb = bytes(b, &n); uint32_t t[8];
            if (op[3]) frs::dot_term_masked(lb, yb, t); else frs::dot_term(lb, yb, t);
            pl(t); free(lb); free(yb);
        } else {
            uint32_t x[8], y[8], r[8];
            le(a, x); le(b, y);
            if (!strcmp(op, "mul")) { frs::mul(r, x, y); pl(r); }                  // a b / R
            else if (!strcmp(op, "mulm")) { frs::mul_masked(r, x, y); pl(r); }
            else if (!strcmp(op, "add")) { frs::add(r, x, y); pl(r); }
            else if (!strcmp(op, "addm")) { frs::add_masked(r, x, y); pl(r); }
            else if (!strcmp(op, "tomm")) { frs::to_mont_masked(r, x); pl(r); }
            else if (!strcmp(op, "frmm")) { frs::from_mont_masked(r, x); pl(r); }
        }
        printf("\n");
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def fr_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("frsecret")
    src, exe = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, "-o", str(exe), str(src)])
    return str(exe)


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return out[:len(lines)]


def test_masked_forms_match_python_ints_and_the_branching_forms(fr_exe):
    rnd = random.Random(0x6672)
    rinv = pow(R, -1, N)
    vals = [0, 1, N - 1, R % N, R * R % N] + [rnd.randrange(N) for _ in range(60)]
    lines, want = [], []
    for a in vals:
        for b in vals[:5] + vals[-4:]:
            for op, w in (("mulm", a * b * rinv % N), ("mul", a * b * rinv % N), ("addm", (a + b) % N), ("add", (a + b) % N)):
                lines.append("%s %064x %064x" % (op, a, b))
                want.append(w)
        for op, w in (("tomm", a * R % N), ("frmm", a * rinv % N)):
            lines.append("%s %064x %064x" % (op, a, 0))
            want.append(w)
    got = _run(fr_exe, lines)
    assert [int(g, 16) for g in got] == want
    # dot_term: any y below 2^256 is reduced first
    ys = [N, N + 1, 2 * N, 2**256 - 1] + vals
    ls = vals[:5] + [rnd.randrange(N) for _ in range(len(ys) - 5)]
    for op in ("dotm", "dot"):
        got = _run(fr_exe, ["%s %064x %064x" % (op, l, y) for l, y in zip(ls, ys)])
        assert [int(g, 16) for g in got] == [l * y % N for l, y in zip(ls, ys)], op


def test_host_rendering_of_the_horner_evaluation_on_every_dealer(fr_exe, golden):
    dkg = golden("dkg.json")
    shapes, lines, want = [], [], []
    for T, n_players, ds in dealers(dkg):
        shapes.append((T, n_players))
        for d in ds:
            assert len(d["coefficients"]) == T and len(d["fragments"]) == n_players
            lines.append("poly %s %s" % ("".join(d["coefficients"]), be32(range(1, n_players + 1)).hex()))
            want.append("".join(d["fragments"]))
    assert shapes == [(1, 1), (2, 3), (3, 5), (5, 7)]
    assert _run(fr_exe, lines) == want
    # coefficients and points at and above n, a zero polynomial, the top coefficient zero
    rnd = random.Random(9)
    edge = [0, 1, N - 1, N, N + 1, 2**255, 2**256 - 1]
    polys = [edge, [0] * 4, [5, 0, 0], [rnd.randrange(2**256) for _ in range(67)]]
    xs = edge + [rnd.randrange(2**256) for _ in range(3)]
    got = _run(fr_exe, ["poly %s %s" % (be32(p).hex(), be32(xs).hex()) for p in polys])
    for p, g in zip(polys, got):
        assert ints32(bytes.fromhex(g)) == [sum(c * pow(x, i, N) for i, c in enumerate(p)) % N for x in xs]


@pytest.fixture
def without_the_entries():
    """a provider with the default paths only: secret=True has nowhere to go"""
    from bls_py import backend
    old = backend._provider
    p = HostLagrange(None)
    backend.use(p)
    yield p
    backend.use(old)


@pytest.fixture
def host_provider():
    from bls_py import backend
    old = backend._provider
    p = HostFrSecret(None)
    backend.use(p)
    yield p
    backend.use(old)


def test_secret_raises_without_the_entries(without_the_entries):
    from bls_py.keys import PrivateKey
    from bls_py.threshold import Threshold
    with pytest.raises(NotImplementedError):
        PrivateKey.new_threshold_batch(2, 3, 2, secret=True)
    with pytest.raises(NotImplementedError):
        Threshold.interpolate_at_zero_batch([[1, 2, 3]], [[4, 5, 6]], secret=True)
    with pytest.raises(NotImplementedError):
        PrivateKey.sign_threshold_batch([PrivateKey(5), PrivateKey(6)], b"m", [1, 2], secret=True)
    assert without_the_entries.calls == []
    # the defaults are still there
    assert int(Threshold.interpolate_at_zero_batch([[1, 2, 3]], [[4, 5, 6]])[0]) == int(Threshold.interpolate_at_zero([1, 2, 3], [4, 5, 6]))


class _Seeded(random.Random):
    """keys.RNG for a test: seeded, and it counts its draws"""
    draws = 0

    def randint(self, a, b):
        self.draws += 1
        return super().randint(a, b)


def test_new_threshold_batch_secret_draws_and_returns_the_same(host_provider, monkeypatch):
    from bls_py import keys
    from bls_py.fields import Fq
    from bls_py.keys import PrivateKey
    from bls_py.threshold import Threshold
    out = {}
    for secret in (False, True):
        rng = _Seeded(77)
        monkeypatch.setattr(keys, "RNG", rng)
        out[secret] = PrivateKey.new_threshold_batch(3, 5, 4, secret=secret)
        assert rng.draws == 12
        out[secret, "next"] = rng.randint(1, N - 1)
    assert out[True, "next"] == out[False, "next"]
    assert [c[0] for c in host_provider.calls] == ["g1_mul_gen", "threshold_deal_secret"]
    assert host_provider.calls[1] == ("threshold_deal_secret", 4, 3, 5)
    assert len(out[True]) == 4
    for (sk_a, com_a, frag_a), (sk_b, com_b, frag_b) in zip(out[True], out[False]):
        assert sk_a == sk_b and com_a == com_b and frag_a == frag_b
        assert all(type(f) is Fq and f.Q == N for f in frag_a)
        assert all(Threshold.verify_secret_fragment(3, f, j + 1, com_a) for j, f in enumerate(frag_a[:2]))
    assert PrivateKey.new_threshold_batch(1, 1, 0, secret=True) == []


def test_interpolate_and_sign_secret_routing(host_provider, golden):
    from bls_py.fields import Fq
    from bls_py.keys import PrivateKey
    from bls_py.threshold import Threshold
    lag = golden("lagrange.json")
    groups = [g for g in lag["groups"] if g["k"] <= 67]
    Xs = [group_players(g) for g in groups]
    Ys = [[Fq(N, y) if i % 2 else y for i, y in enumerate(group_values(g))] for g in groups]
    vals = Threshold.interpolate_at_zero_batch(Xs, Ys, secret=True)
    assert [int(v) for v in vals] == [int(g["interpolate"], 16) for g in groups]
    assert all(type(v) is Fq and v.Q == N for v in vals)
    assert {c[0] for c in host_provider.calls} == {"fr_interpolate_at_zero_secret"}          # one call per distinct k, no host loop
    assert len(host_provider.calls) == len({g["k"] for g in groups})
    # what the device cannot take raises instead of taking the host loop; the reference's assertion comes first
    host_provider.calls.clear()
    wide = list(range(1, HostFrSecret.LAGRANGE_MAX_K + 2))
    for X, Y in ((wide, wide), ([1, -2], [3, 4]), ([], []), ([1, 2], [3])):
        with pytest.raises(ValueError):
            Threshold.interpolate_at_zero_batch([[1, 2], X], [[5, 6], Y], secret=True)
    with pytest.raises(AssertionError):
        Threshold.interpolate_at_zero_batch([[1, 1]], [[5, 6]], secret=True)
    assert host_provider.calls == []
    assert Threshold.interpolate_at_zero_batch([], [], secret=True) == []
    # signing: one call for the session, the default call's signatures
    cb = lag["combine"]
    shares = [int(s, 16) for s in cb["shares"]]
    msg = bytes.fromhex(cb["msg"])
    players = cb["subsets"][0]["players"]
    sks = [PrivateKey(shares[p - 1]) for p in players]
    want = PrivateKey.sign_threshold_batch(sks, msg, players)
    host_provider.calls.clear()
    got = PrivateKey.sign_threshold_batch(sks, msg, players, secret=True)
    assert host_provider.calls == [("sign_threshold", 3, 1, 1)]
    assert got == want and [s.serialize() for s in got] == [s.serialize() for s in want]
    with pytest.raises(ValueError):
        PrivateKey.sign_threshold_batch([PrivateKey(1)], msg, [1, 2], secret=True)
    with pytest.raises(AssertionError):
        PrivateKey.sign_threshold_batch([PrivateKey(1), PrivateKey(2)], msg, [4, 4], secret=True)
    assert PrivateKey.sign_threshold_batch([], msg, [], secret=True) == []
