"""The masked scalar helpers of csrc/hd_derive.h (reduce_n_masked, add_mod_n_masked: the subtraction kept by a mask, no
branch on the borrow -- blsgpu_hd_paths_secret) compiled for the host against Python integers and against the branching
forms beside them; the y > q // 2 test of the compressed forms (fq32.h gt_half_q_mask, shared by the G1 and G2 kernels and
the host) at its tie and single-word cases; and the secret=True keyword of the key methods on a provider that lacks the
device calls."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")
N = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001

HOST_TEST = r'''
#include "hd_derive.h"
#include <stdio.h>
#include <string.h>
static void le(const char* h, uint32_t s[8]) { for (int j = 0; j < 8; j++) { unsigned v; sscanf(h + 8 * j, "%8x", &v); s[7 - j] = v; } }
static void pl(const uint32_t s[8]) { for (int j = 7; j >= 0; j--) printf("%08x", s[j]); }
int main() {
    char op[8], a[80], b[80];
    while (scanf("%7s %79s %79s", op, a, b) == 3) {
        uint32_t x[8], y[8], r[8], x2[8], r2[8];
        le(a, x); le(a, x2);
        if (!strcmp(op, "red")) { hdk::reduce_n_masked(x); hdk::reduce_n(x2); pl(x); printf(" "); pl(x2);
        } else if (!strcmp(op, "addn")) { le(b, y); hdk::add_mod_n_masked(r, x, y); hdk::add_mod_n(r2, x, y); pl(r); printf(" "); pl(r2); }
        printf("\n");
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("g1fixs")
    src, out = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, "-o", str(out), str(src)])
    return str(out)


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return [tuple(int(v, 16) for v in ln.split()) for ln in out[:len(lines)]]


EDGES = [0, N - 1, N, N + 1, 2 * N, 2 * N + 1, 2**256 - 1]


def test_masked_reduction(exe):
    rnd = random.Random(31)
    vals = EDGES + [1, 2 * N - 1, 2**255] + [rnd.randrange(2**256) for _ in range(1000)]
    got = _run(exe, ["red %064x -" % v for v in vals])
    assert [g[0] for g in got] == [v % N for v in vals]
    assert all(g[0] == g[1] for g in got)                    # the branching form beside it


def test_masked_addition(exe):
    rnd = random.Random(32)
    small = [v for v in EDGES if v < N]
    pairs = [(a, b) for a in small for b in small] + [(N - 1, 1), (N - 1, N - 1), (1, N - 2)]
    pairs += [(rnd.randrange(N), rnd.randrange(N)) for _ in range(1000)]
    got = _run(exe, ["addn %064x %064x" % p for p in pairs])
    assert [g[0] for g in got] == [(a + b) % N for a, b in pairs]
    assert all(g[0] == g[1] for g in got)
    # the step of the kernel: (i_left mod n + sk mod n) mod n for the edge values on either side
    red = {v: r[0] for v, r in zip(EDGES, _run(exe, ["red %064x -" % v for v in EDGES]))}
    combos = [(a, b) for a in EDGES for b in EDGES]
    got = _run(exe, ["addn %064x %064x" % (red[a], red[b]) for a, b in combos])
    assert [g[0] for g in got] == [(a + b) % N for a, b in combos]


HALF_Q_TEST = r'''
#include "fq32.h"
#include <stdio.h>
int main() {
    char a[128];
    while (scanf("%127s", a) == 1) {
        uint32_t y[12];
        for (int j = 0; j < 12; j++) { unsigned v; sscanf(a + 8 * j, "%8x", &v); y[11 - j] = v; }
        printf("%08x\n", bls::gt_half_q_mask(y));
    }
    return 0;
}
'''
Q = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab


def test_gt_half_q_mask(tmp_path):
    """all ones exactly when y > q // 2: the ends, the tie and its neighbours, and values that differ from q // 2 in one
    word only (the lowest, the highest, one in the middle), below and above -- cases no curve coordinate of the device tests
    reaches"""
    src, out = tmp_path / "h.cpp", tmp_path / "h"
    src.write_text(HALF_Q_TEST)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, "-o", str(out), str(src)])
    half = Q // 2
    low, high = half & 0xFFFFFFFF, half >> 352

    def word(j, v):
        return (half & ~(0xFFFFFFFF << (32 * j))) | (v << (32 * j))
    vals = [0, half - 1, half, half + 1, Q - 1]
    vals += [word(0, 0), word(0, low - 0x1000), word(0, low + 1), word(0, 0xFFFFFFFF)]
    vals += [word(11, 0), word(11, high - 1), word(11, high + 1), word(11, Q >> 352)]
    mid = (half >> 160) & 0xFFFFFFFF
    vals += [word(5, mid - 1), word(5, mid + 1)]
    rnd = random.Random(33)
    vals += [rnd.randrange(Q) for _ in range(200)]
    assert all(0 <= v < 1 << 384 for v in vals)
    res = subprocess.run([str(out)], input="\n".join("%096x" % v for v in vals) + "\n", capture_output=True, text=True, check=True)
    got = [int(ln, 16) for ln in res.stdout.split()]
    assert got == [0xFFFFFFFF if v > half else 0 for v in vals]
    assert sum(1 for g in got if g) > 50 and sum(1 for g in got if not g) > 50


class _DigitIndexedOnly:
    """a provider with the digit-indexed calls alone"""
    def g1_mul_gen(self, scalars, add=None, n_add=0):
        raise AssertionError("secret=True must not reach the digit-indexed path")

    def hd_children(self, *a):
        raise AssertionError("secret=True must not reach the digit-indexed path")

    def hd_paths(self, *a):
        raise AssertionError("secret=True must not reach the digit-indexed path")


def test_secret_keyword_never_falls_back():
    from bls_py import backend
    from bls_py.keys import ExtendedPrivateKey, PrivateKey
    old = backend._provider
    backend.use(_DigitIndexedOnly())
    try:
        sk = PrivateKey(5)
        with pytest.raises(NotImplementedError, match="g1_mul_gen_secret"):
            PrivateKey.get_public_key_batch([sk], secret=True)
        esk = ExtendedPrivateKey(1, 0, 0, 0, bytes(32), sk)
        for call in (lambda: esk.private_child_batch([1], secret=True), lambda: esk.private_path_batch([[1, 2]], secret=True),
                     lambda: ExtendedPrivateKey.private_paths_from([esk], [0], [[1]], secret=True)):
            with pytest.raises(NotImplementedError, match="_secret"):
                call()
        assert PrivateKey.get_public_key_batch([], secret=True) == []
    finally:
        backend.use(old)
