"""Keys from seeds, the host side: the long-message HMAC of csrc/hd_derive.h (hmac_long, hmac_long_pair: blsgpu_keys_from_seeds
runs it one seed per lane) compiled for the host against Python's hmac -- once more under AddressSanitizer and UBSan, since
block indexing at the padding boundaries is where an overrun would sit -- the fixture tests/golden/seeds.json against the
repository's own from_seed, and PrivateKey.from_seed_batch / ExtendedPrivateKey.from_seed_batch with backend.extension on a
recording stand-in provider."""
import json
import os
import random
import subprocess

import pytest

from bls_py import backend
from bls_py.keys import ExtendedPrivateKey, PrivateKey
from seeds_vectors import KEYS, LENGTHS, SEED_MAX, HostSeeds, by_length, host_keys, load, mac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")
H31 = 2**31

# one line per case: <op> <key index> <suffix: -1, 0, 1> <hex of the message, or - for none>; op `one`: hmac_long, `pair`:
# hmac_long_pair (two digests).  The message lies in a heap block of exactly its length.
HOST_TEST = r'''
#include "hd_derive.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
static char hex[4096];
static void pd(const uint32_t d[8]) { for (int j = 0; j < 8; j++) printf("%08x", d[j]); }
int main() {
    hdk::HmacKey K[2];
    hdk::hmac_key((const uint8_t*)"BLS private key seed", 20, K[0]);
    hdk::hmac_key((const uint8_t*)"BLS HD seed", 11, K[1]);
    char op[8];
    int key, suffix;
    while (scanf("%7s %d %d %4095s", op, &key, &suffix, hex) == 4) {
        const uint32_t len = hex[0] == '-' ? 0u : (uint32_t)strlen(hex) / 2u;
        uint8_t* m = len ? (uint8_t*)malloc(len) : nullptr;
        for (uint32_t i = 0; i < len; i++) { unsigned v; sscanf(hex + 2 * i, "%2x", &v); m[i] = (uint8_t)v; }
        uint32_t a[8], b[8];
        if (!strcmp(op, "pair")) { hdk::hmac_long_pair(K[key], m, len, a, b); pd(a); printf(" "); pd(b); }
        else { hdk::hmac_long(K[key], m, len, suffix, a); pd(a); }
        printf("\n");
        free(m);
    }
    return 0;
}
'''
HOST_LENGTHS = list(range(201)) + [1023, 1024]


@pytest.fixture(scope="module")
def hmac_cases():
    rnd = random.Random(0x5eed)
    lines, want = [], []
    for L in HOST_LENGTHS:
        m = rnd.randbytes(L)
        h = m.hex() or "-"
        for k in (0, 1):
            lines.append("one %d -1 %s" % (k, h))
            want.append(mac(KEYS[k], m).hex())
            for s in (0, 1):
                lines.append("one %d %d %s" % (k, s, h))
                want.append(mac(KEYS[k], m + bytes([s])).hex())
            lines.append("pair %d 0 %s" % (k, h))
            want.append(mac(KEYS[k], m + b"\x00").hex() + " " + mac(KEYS[k], m + b"\x01").hex())
    return "\n".join(lines) + "\n", want


def _build_and_run(tmp_path, flags, text):
    src, exe = tmp_path / "t.cpp", tmp_path / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, *flags, "-o", str(exe), str(src)])
    return subprocess.run([str(exe)], input=text, capture_output=True, text=True)


def test_hmac_long_against_python(tmp_path, hmac_cases):
    text, want = hmac_cases
    res = _build_and_run(tmp_path, ["-O2"], text)
    assert res.returncode == 0
    assert res.stdout.split("\n")[:-1] == want


def test_hmac_long_under_sanitizers(tmp_path, hmac_cases):
    """the same program and cases with AddressSanitizer and UBSan (CPU only): every message is a heap block of exactly its
    length, so a read past a seed's last byte is reported"""
    text, want = hmac_cases
    res = _build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], text)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
    assert res.stdout.split("\n")[:-1] == want


# ---- the fixture against the repository's own single-seed calls -------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return load()


def test_fixture_against_from_seed(fx):
    for r in fx["seeds"]:
        seed = bytes.fromhex(r["seed"])
        sk = PrivateKey.from_seed(seed)
        esk = ExtendedPrivateKey.from_seed(seed)
        assert "%064x" % sk.value == r["plain"]["sk"]
        assert "%064x" % esk.private_key.value == r["hd"]["sk"] and esk.chain_code.hex() == r["hd"]["chain"]
        for mode, hd in (("plain", False), ("hd", True)):
            skb, chain, cls = host_keys(seed, hd)
            assert skb.hex() == r[mode]["sk"] and cls == r[mode]["cls"] and (not hd or chain.hex() == r["hd"]["chain"])


# ---- the batch methods on a recording stand-in -----------------------------------------------------------------------------
@pytest.fixture
def host():
    old = backend._provider
    prov = HostSeeds()
    backend.use(prov)
    yield prov
    backend.use(old)


def test_fixture_public_keys_and_path_leaves(fx, host):
    """the public keys and the path leaves of the fixture through the batch methods (the stand-in multiplies on the host)"""
    recs = by_length(fx)
    picked = [r for L in (0, 32, 64, 1024) for r in recs[L]]
    seeds = [bytes.fromhex(r["seed"]) for r in picked]
    sks = PrivateKey.from_seed_batch(seeds)
    assert [sk.get_public_key().serialize().hex() for sk in sks] == [r["plain"]["ser"] for r in picked]
    masters = ExtendedPrivateKey.from_seed_batch(seeds)
    assert [m.get_public_key().serialize().hex() for m in masters] == [r["hd"]["ser"] for r in picked]
    assert [m._public_key().serialize().hex() for m in masters] == [r["hd"]["ser"] for r in picked]
    roots = ExtendedPrivateKey.from_seed_batch([bytes.fromhex(p["seed"]) for p in fx["paths"]])
    del host.calls[:]
    leaves = ExtendedPrivateKey.private_paths_from(roots, list(range(len(roots))), [fx["path"]] * len(roots), secret=True)
    assert [k.serialize().hex() for k in leaves] == [p["leaf"] for p in fx["paths"]]
    assert [k.get_public_key().serialize().hex() for k in leaves] == [p["leaf_pk"] for p in fx["paths"]]
    # the masters came with their public keys: the path call is the only one
    assert host.calls == [("hd_paths_secret", len(roots))]


def test_batch_equals_the_loop(host):
    rnd = random.Random(0x5eed5)
    lengths = [32, 0, 64, 32, 1, 55, 64, 32, 56, 0, 1024]
    seeds = [rnd.randbytes(L) for L in lengths]
    sks = PrivateKey.from_seed_batch(seeds)
    assert sks == [PrivateKey.from_seed(s) for s in seeds] and all(type(k) is PrivateKey for k in sks)
    # one call per distinct length, in the order the lengths first appear, the results back in input order
    first = list(dict.fromkeys(lengths))
    assert host.calls == [("keys_from_seeds", L, lengths.count(L), False) for L in first]
    for sk in sks:
        assert sk.__dict__["_pk_point"] is not None
        assert sk.get_public_key().serialize() == PrivateKey(sk.value).get_public_key().serialize()
    del host.calls[:]
    masters = ExtendedPrivateKey.from_seed_batch(seeds)
    loop = [ExtendedPrivateKey.from_seed(s) for s in seeds]
    assert masters == loop and [m.serialize() for m in masters] == [m.serialize() for m in loop]
    assert host.calls == [("keys_from_seeds", L, lengths.count(L), True) for L in first]
    for m, l in zip(masters, loop):
        assert (m.version, m.depth, m.parent_fingerprint, m.child_number) == (1, 0, 0, 0)
        assert m.__dict__["_pk"]._ser == l.get_public_key().serialize() and m.__dict__["_pk"].value is m.private_key.__dict__["_pk_point"]
        assert m.get_extended_public_key().serialize() == l.get_extended_public_key().serialize()
    del host.calls[:]
    assert PrivateKey.from_seed_batch([]) == [] and ExtendedPrivateKey.from_seed_batch([]) == [] and host.calls == []


def test_masters_need_no_multiplication_of_their_own(host):
    rnd = random.Random(0x5eed6)
    seeds = [rnd.randbytes(32) for _ in range(5)]
    masters = ExtendedPrivateKey.from_seed_batch(seeds)
    seed_of = [0, 1, 2, 3, 4, 4, 0]
    paths = [[H31 + 44, 0, j] for j in range(len(seed_of))]
    del host.calls[:]
    leaves = ExtendedPrivateKey.private_paths_from(masters, seed_of, paths, secret=True)
    assert not [c for c in host.calls if c[0] == "g1_mul_gen_secret"]
    assert host.calls == [("hd_paths_secret", len(paths))]
    # masters from the single calls have no key yet: there the multiplication is made
    cold = [ExtendedPrivateKey.from_seed(s) for s in seeds]
    del host.calls[:]
    again = ExtendedPrivateKey.private_paths_from(cold, seed_of, paths, secret=True)
    assert host.calls == [("g1_mul_gen_secret", len(seeds)), ("hd_paths_secret", len(paths))]
    assert [k.serialize() for k in leaves] == [k.serialize() for k in again]


def test_over_limit_seeds_take_the_single_calls(host):
    rnd = random.Random(0x5eed7)
    seeds = [rnd.randbytes(SEED_MAX + 1), rnd.randbytes(SEED_MAX), rnd.randbytes(3000), rnd.randbytes(SEED_MAX)]
    assert PrivateKey.from_seed_batch(seeds) == [PrivateKey.from_seed(s) for s in seeds]
    assert ExtendedPrivateKey.from_seed_batch(seeds) == [ExtendedPrivateKey.from_seed(s) for s in seeds]
    assert host.calls == [("keys_from_seeds", SEED_MAX, 2, False), ("keys_from_seeds", SEED_MAX, 2, True)]
    del host.calls[:]
    assert PrivateKey.from_seed_batch(seeds[::2]) == [PrivateKey.from_seed(s) for s in seeds[::2]] and host.calls == []


def test_str_seeds_as_the_reference_treats_them(host):
    assert PrivateKey.from_seed_batch(["seed é", b"x"]) == [PrivateKey.from_seed("seed é"), PrivateKey.from_seed(b"x")]
    assert PrivateKey.from_seed("seed é") == PrivateKey.from_seed("seed é".encode("utf-8"))
    assert host.calls == [("keys_from_seeds", 7, 1, False), ("keys_from_seeds", 1, 1, False)]
    del host.calls[:]
    with pytest.raises(TypeError):
        ExtendedPrivateKey.from_seed("seed")
    with pytest.raises(TypeError):
        ExtendedPrivateKey.from_seed_batch([b"fine", "seed"])
    assert host.calls == []                                     # refused before any device work
    assert ExtendedPrivateKey.from_seed_batch([bytearray(b"ab")]) == [ExtendedPrivateKey.from_seed(b"ab")]


def test_a_provider_without_the_extension_takes_the_loop():
    class Bare:
        pass
    old = backend._provider
    backend.use(Bare())
    try:
        assert backend.extension("keys_from_seeds") is None
        seeds = [b"", b"one", bytes(64)]
        assert PrivateKey.from_seed_batch(seeds) == [PrivateKey.from_seed(s) for s in seeds]
        assert ExtendedPrivateKey.from_seed_batch(seeds) == [ExtendedPrivateKey.from_seed(s) for s in seeds]
        assert not hasattr(PrivateKey.from_seed_batch(seeds)[0], "_pk_point")
    finally:
        backend.use(old)


def test_extension_lookup(host):
    assert backend.extension("keys_from_seeds").__self__ is host             # a stand-in's own attribute
    assert backend.extension("no_such_extension") is None
    # a HipProvider: the function of the extension module bound to that provider's engine (no GPU call is made here)
    from bls_py import _native_seeds
    p = backend.HipProvider.__new__(backend.HipProvider)
    p._eng = object()
    backend.use(p)
    fn = backend.extension("keys_from_seeds")
    assert fn.func is _native_seeds.keys_from_seeds and fn.args == (p._eng,)
    assert backend.extension("no_such_extension") is None
    assert set(backend.EXTENSIONS) == {"keys_from_seeds"}


def test_the_fixed_method_sets_gained_no_name():
    """the engine's methods are the ones with recorded marshalling cases, the provider's names its PROVIDER_METHODS: the new
    call lives in a module of its own and is reached through backend.extension"""
    from bls_py import _native
    assert sorted(n for n in dir(backend.HipProvider) if not n.startswith("_")) == sorted(backend.PROVIDER_METHODS + ("LAGRANGE_MAX_K",))
    with open(os.path.join(ROOT, "tests", "golden", "native_marshalling.json")) as f:
        recorded = list(json.load(f)["engine"])
    public = [n for n, v in vars(_native.Engine).items() if not n.startswith("_") and callable(v)]
    assert all(any(cid.startswith(n) for cid in recorded) for n in public)
    assert not [n for n in dir(_native.Engine) + dir(backend.HipProvider) if "seed" in n]
    assert {"blsgpu_keys_from_seeds", "blsgpu_keys_from_seeds_dev"} <= set(_native.PROTOTYPES)
