"""Secure aggregation without a GPU: the per-lane steps of csrc/hash_pks.h compiled for the host against hashlib and
Python integers, and the batch forms of bls_py (util.hash_pks_batch, BLS.aggregate_pub_keys_batch,
BLS.aggregate_sigs_secure_batch, BLS.aggregate_priv_keys_batch(secure_with=...)) through a recording host provider of the
four device operations (tests/secure_agg_vectors.HostSecureAgg) against vectors generated from the reference
(tests/golden/secure_agg.json) and against the per-call loop."""
import hashlib
import os
import random
import subprocess

import pytest

from secure_agg_vectors import HostSecureAgg, N, Pool, check_hash_pks, check_priv_keys, check_pub_keys, check_sigs, seeded_keys
from rxsecret_vectors import HostRxSecret

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")

# stdin: "dig <k> <hex of k keys>" -> the digest; "exp <digest hex> <i hex>" -> the exponent, 32 bytes big-endian
HOST_TEST = r'''
#include "hash_pks.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
static void pw(const uint32_t* w, int n) { for (int i = 0; i < n; i++) printf("%08x", w[i]); }
int main() {
    static char op[8], a[72], h[48 * 2 * 300];
    while (scanf("%7s %71s %28799s", op, a, h) == 3) {
        if (!strcmp(op, "dig")) {
            const size_t k = strtoul(a, nullptr, 10);
            uint8_t* buf = (uint8_t*)aligned_alloc(16, 48 * k + 16);       // exactly the keys: a read past them is out of bounds
            for (size_t i = 0; i < 48 * k; i++) { unsigned v; sscanf(h + 2 * i, "%2x", &v); buf[i] = (uint8_t)v; }
            uint32_t st[8]; hpk::digest((const uint32_t*)buf, k, st); pw(st, 8);
            free(buf);
        } else {
            uint32_t dg[8], t[8]; unsigned i;
            for (int j = 0; j < 8; j++) { unsigned v; sscanf(a + 8 * j, "%8x", &v); dg[j] = v; }
            sscanf(h, "%x", &i);
            hpk::exponent(dg, i, t);
            for (int j = 7; j >= 0; j--) printf("%08x", t[j]);
        }
        printf("\n");
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def hpk_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("hpk")
    src, exe = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, "-o", str(exe), str(src)])
    return str(exe)


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return out[:len(lines)]


def test_digest_matches_hashlib(hpk_exe):
    """every k mod 4 with zero, one and several quads before it, and lengths whose bit count needs more than 16 bits"""
    ks = list(range(1, 14)) + [64, 65, 255, 256, 257]
    keys = [seeded_keys(500 + k, k) for k in ks]
    got = _run(hpk_exe, ["dig %d %s" % (k, b.hex()) for k, b in zip(ks, keys)])
    assert got == [hashlib.sha256(b).hexdigest() for b in keys]


def test_exponent_matches_python_integers(hpk_exe):
    rnd = random.Random(77)
    cases = [(rnd.randbytes(32), rnd.choice((0, 1, 2, 255, 256, 2**31, 2**32 - 1, rnd.randrange(2**32)))) for _ in range(320)]
    outer = [int.from_bytes(hashlib.sha256(i.to_bytes(4, "big") + d).digest(), "big") for d, i in cases]
    # all three cases of the reduction occur (about 45 %, 45 % and 9 % of the digests: 2^256 = 2.21 n)
    zones = [sum(1 for v in outer if lo <= v < hi) for lo, hi in ((0, N), (N, 2 * N), (2 * N, 2**256))]
    assert min(zones) >= 10 and sum(zones) == len(cases) >= 300, zones
    got = _run(hpk_exe, ["exp %s %x" % (d.hex(), i) for d, i in cases])
    assert [int(g, 16) for g in got] == [v % N for v in outer]


# ---- the Python batch forms ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx(golden):
    return golden("secure_agg.json")


def _provider(cls):
    from bls_py import backend
    old = backend._provider
    p = cls(None)
    backend.use(p)
    return p, old


@pytest.fixture
def host_agg():
    from bls_py import backend
    p, old = _provider(HostSecureAgg)
    yield p
    backend.use(old)


@pytest.fixture
def host_without():
    """a provider WITHOUT the four entries"""
    from bls_py import backend
    p, old = _provider(HostRxSecret)
    yield p
    backend.use(old)


@pytest.fixture(scope="module")
def pool(fx):
    from bls_py import backend
    p, old = _provider(HostSecureAgg)
    try:
        return Pool(fx)
    finally:
        backend.use(old)


NEW = ("hash_pks", "aggregate_pub_keys_secure", "aggregate_sigs_secure", "aggregate_priv_keys_secure")


def _new_calls(p):
    return [c for c in p.calls if c[0] in NEW]


def test_fixture_size(fx):
    path = os.path.join(ROOT, "tests", "golden", "secure_agg.json")
    assert 10_000 < os.path.getsize(path) < 100_000


def test_hash_pks_batch(fx, pool, host_agg):
    check_hash_pks(fx, pool)
    host_agg.calls.clear()
    from bls_py.util import hash_pks_batch
    groups = [[pool.pks[i] for i in r["keys"]] for r in fx["hash_pks"]]
    hash_pks_batch(2, groups + groups[:3])
    assert sorted(_new_calls(host_agg)) == sorted(("hash_pks", k, 2, 2 if k <= 3 else 1) for k in list(range(1, 10)) + [64, 65])
    host_agg.calls.clear()
    assert hash_pks_batch(0, groups[:2]) == [[], []] and hash_pks_batch(3, []) == [] and len(hash_pks_batch(3, [[]])[0]) == 3
    assert host_agg.calls == []


def test_pub_keys_batch(fx, pool, host_agg):
    check_pub_keys(fx, pool)
    host_agg.calls.clear()
    from bls_py.bls import BLS
    groups = [[pool.pks[i] for i in r["keys"]] for r in fx["pub_keys"]]
    BLS.aggregate_pub_keys_batch(groups + groups[1:2], True)
    assert sorted(_new_calls(host_agg)) == [("aggregate_pub_keys_secure", k, 2 if k == 2 else 1) for k in (1, 2, 3, 5, 9)]
    with pytest.raises(Exception, match="Invalid number of keys"):
        BLS.aggregate_pub_keys_batch([groups[0], []], True)


def test_sigs_batch(fx, pool, host_agg):
    check_sigs(fx, pool)
    from bls_py.bls import BLS
    assert sorted(c for c in _new_calls(host_agg) if c[0] == "aggregate_sigs_secure") == \
        [("aggregate_sigs_secure", 1, 1, 1), ("aggregate_sigs_secure", 2, 2, 1), ("aggregate_sigs_secure", 3, 3, 1), ("aggregate_sigs_secure", 5, 5, 2)]
    with pytest.raises(Exception, match="Invalid number of keys"):
        BLS.aggregate_sigs_secure_batch([[]], [[pool.pks[0]]], [[]])
    assert BLS.aggregate_sigs_secure_batch([[]], [[]], [[]])[0].value.infinity


def test_priv_keys_batch(fx, pool, host_agg):
    check_priv_keys(fx, pool, secret=True)
    assert ("aggregate_priv_keys_secure", 9, 1, True) in host_agg.calls and ("aggregate_priv_keys_secure", 9, 1, False) in host_agg.calls
    host_agg.calls.clear()
    check_priv_keys(fx, pool, secret=False)                # the host loop
    assert _new_calls(host_agg) == []
    from bls_py.bls import BLS
    with pytest.raises(Exception, match="Must include public keys"):
        BLS.aggregate_priv_keys_batch([[pool.sks[0]]], secret=True, secure_with=[[]])
    with pytest.raises(Exception, match="Invalid number of keys"):
        BLS.aggregate_priv_keys_batch([[pool.sks[0]]], secret=True, secure_with=[pool.pks[:2]])
    with pytest.raises(ValueError):
        BLS.aggregate_priv_keys_batch([[pool.sks[0]]], secret=True, secure_with=[])
    # without secure_with nothing changes
    assert BLS.aggregate_priv_keys_batch([pool.sks[:3]])[0].value == sum(sk.value for sk in pool.sks[:3]) % N


def test_a_provider_without_the_entries(fx, pool, host_without):
    """the loops run and reproduce the fixture; secret=True raises instead of falling back"""
    check_hash_pks(fx, pool)
    check_pub_keys(fx, pool)
    check_sigs(fx, pool)
    check_priv_keys(fx, pool, secret=False)
    assert _new_calls(host_without) == []
    from bls_py.bls import BLS
    with pytest.raises(NotImplementedError):
        BLS.aggregate_priv_keys_batch([pool.sks[:2]], secret=True, secure_with=[pool.pks[:2]])
