"""HD path derivation without a GPU: the per-level helpers of csrc/hd_derive.h (key midstates from a chain code held in
words, one level of a path, the fingerprint block) compiled for the host against Python's hmac / hashlib, and the object
logic of the *_path_batch / *_paths_from methods of bls_py.keys through a host provider of hd_paths
(tests/hd_paths_vectors.HostHDPaths) against vectors generated from the reference (tests/golden/hd_paths.json)."""
import hashlib
import hmac
import os
import random
import subprocess

import pytest

from hd_paths_vectors import HostHDPaths, check_grid_record, check_private_record, check_public_record
from hd_vectors import HostHD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")
H31 = 2**31

HOST_TEST = r'''
#include "hd_derive.h"
#include <stdio.h>
#include <string.h>
static int unhex(const char* h, uint8_t* b) { int n = (int)strlen(h) / 2; for (int i = 0; i < n; i++) { unsigned v; sscanf(h + 2 * i, "%2x", &v); b[i] = (uint8_t)v; } return n; }
static int words(const char* h, uint32_t* w) { uint8_t b[64]; int n = unhex(h, b) / 4; for (int j = 0; j < n; j++) w[j] = ((uint32_t)b[4*j] << 24) | (b[4*j+1] << 16) | (b[4*j+2] << 8) | b[4*j+3]; return n; }
static void pw(const uint32_t* w, int n) { for (int i = 0; i < n; i++) printf("%08x", w[i]); }
int main() {
    char op[8], a[260], b[2100];
    while (scanf("%7s %259s %2099s", op, a, b) == 3) {
        if (!strcmp(op, "fp")) {                         // 48 bytes of a serialised key
            uint32_t s[12]; words(a, s); printf("%08x", hdk::fingerprint(s));
        } else if (!strcmp(op, "key")) {                 // chain code: hmac_key_words against hmac_key
            uint32_t c[8]; words(a, c); uint8_t k[32]; unhex(a, k);
            hdk::HmacKey K1, K2; hdk::hmac_key_words(c, K1); hdk::hmac_key(k, 32, K2);
            printf("%d", !memcmp(&K1, &K2, sizeof(K1))); pw(K1.ipad, 8); pw(K1.opad, 8);
        } else if (!strcmp(op, "chain")) {               // chain code, then per level "ser(64 or 96 hex):index(hex)," -- the chain
            uint32_t c[8]; words(a, c);                  // code of a level is the i_right of the level before
            for (char* t = strtok(b, ","); t; t = strtok(NULL, ",")) {
                char* colon = strchr(t, ':'); *colon = 0;
                uint32_t s[12], l[8], r[8]; int sw = words(t, s); unsigned idx; sscanf(colon + 1, "%x", &idx);
                hdk::path_step(c, s, sw, idx, l, r); pw(l, 8);
                for (int j = 0; j < 8; j++) c[j] = r[j];
            }
            pw(c, 8);
        }
        printf("\n");
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def hdp_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("hdp")
    src, exe = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, "-o", str(exe), str(src)])
    return str(exe)


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return out[:len(lines)]


def test_fingerprint_block_matches_sha256(hdp_exe):
    rnd = random.Random(21)
    sers = [bytes(48), b"\xff" * 48, b"\x80" + bytes(47)] + [rnd.randbytes(48) for _ in range(200)]
    got = _run(hdp_exe, ["fp %s -" % s.hex() for s in sers])
    assert got == [hashlib.sha256(s).digest()[:4].hex() for s in sers]


def test_key_midstates_from_words(hdp_exe):
    rnd = random.Random(22)
    chains = [bytes(32), b"\xff" * 32] + [rnd.randbytes(32) for _ in range(50)]
    got = _run(hdp_exe, ["key %s -" % c.hex() for c in chains])
    assert all(g[0] == "1" and len(g) == 129 for g in got)           # the same midstates as hmac_key of the bytes


def test_multi_level_chain_matches_python_hmac(hdp_exe):
    rnd = random.Random(23)
    lines, want = [], []
    for _ in range(120):
        chain = rnd.randbytes(32)
        levels = [(rnd.randbytes(rnd.choice((32, 48))), rnd.choice((0, 1, H31 - 1, H31, 2**32 - 1, rnd.randrange(2**32))))
                  for _ in range(rnd.randrange(1, 9))]
        lines.append("chain %s %s" % (chain.hex(), ",".join("%s:%x" % (s.hex(), i) for s, i in levels)))
        w = ""
        for s, i in levels:
            msg = s + i.to_bytes(4, "big")
            w += hmac.new(chain, msg + b"\x00", hashlib.sha256).hexdigest()
            chain = hmac.new(chain, msg + b"\x01", hashlib.sha256).digest()
        want.append(w + chain.hex())
    assert _run(hdp_exe, lines) == want


# ---- the Python surface over a host provider ----------------------------------------------------------------------
@pytest.fixture
def host_paths():
    from bls_py import backend
    old = backend._provider
    p = HostHDPaths(old)
    backend.use(p)
    yield p
    backend.use(old)


@pytest.fixture
def host_no_paths():
    """a provider WITHOUT hd_paths: the methods chain the single steps"""
    from bls_py import backend
    old = backend._provider
    p = HostHD(None)
    backend.use(p)
    yield p
    backend.use(old)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("hd_paths.json")


def test_fixture_shape(fx):
    assert len(fx["private"]) == 2
    for rec in fx["private"]:
        paths = rec["paths"]
        assert len(paths) == 256 and {len(p) for p in paths} == set(range(1, 7))
        for d in range(1, 7):
            assert any(len(p) == d and all(i >= H31 for i in p) for p in paths)
            assert any(len(p) == d and all(i < H31 for i in p) for p in paths)
        assert any(any(i >= H31 for i in p) and any(i < H31 for i in p) for p in paths)
    pub = fx["public"]["paths"]
    assert len(pub) == 256 and {len(p) for p in pub} == set(range(1, 7)) and all(i < H31 for p in pub for i in p)
    assert fx["grid"]["accounts"] == fx["grid"]["addresses"] == 32 and fx["grid"]["epk"]["count"] == 1024


def test_fixture_private_paths_sampled(fx, host_paths):
    for rec in fx["private"]:
        check_private_record(rec, full=False)


def test_fixture_public_paths_sampled(fx, host_paths):
    check_public_record(fx["public"], full=False)


def test_fixture_grid_sampled(fx, host_paths):
    check_grid_record(fx["grid"], full=False)


def _keys():
    from bls_py.keys import ExtendedPrivateKey
    esk = ExtendedPrivateKey.from_seed(b"paths")
    return esk, esk.get_extended_public_key()


def test_mixed_lengths_keep_input_order(host_paths):
    from bls_py.keys import ExtendedPrivateKey, ExtendedPublicKey
    esk, epk = _keys()
    paths = [[5, H31 + 1, 7], [3], [], [H31 + 2, 4], [9], [1, 2, 3], [H31 + 8]]
    host_paths.calls.clear()
    got = esk.private_path_batch(paths)
    assert host_paths.calls == [("hd_paths", 3, 1), ("hd_paths", 1, 2), ("hd_paths", 2, 3)]     # one call per distinct length
    for k, p in zip(got, paths):
        want = esk
        for i in p:
            want = want.private_child(i)
        assert k.serialize() == want.serialize(), p
        assert k.get_extended_public_key().serialize() == want.get_extended_public_key().serialize(), p
        assert (k.depth, k.child_number, k.parent_fingerprint) == (want.depth, want.child_number, want.parent_fingerprint)
    assert [k.serialize() for k in esk.public_path_batch(paths)] == [k.get_extended_public_key().serialize() for k in got]
    soft = [[5, 1, 7], [], [3], [2, 4], [1, 2, 3, 4]]
    pgot = epk.public_path_batch(soft)
    for k, p in zip(pgot, soft):
        want = epk
        for i in p:
            want = want.public_child(i)
        assert k.serialize() == want.serialize(), p
    assert pgot == esk.public_path_batch(soft)
    # many parents: parent j's own paths, in input order
    kids = esk.private_child_batch([H31, H31 + 1, 2])
    parent_of = [2, 0, 1, 0, 2]
    pp = [[1, H31], [4], [], [6, 7, 8], [9]]
    many = ExtendedPrivateKey.private_paths_from(kids, parent_of, pp)
    for k, a, p in zip(many, parent_of, pp):
        want = kids[a]
        for i in p:
            want = want.private_child(i)
        assert k.serialize() == want.serialize(), (a, p)
    xkids = [k.get_extended_public_key() for k in kids]
    xp = [[1, 5], [4], [], [6, 7, 8], [9]]
    xmany = ExtendedPublicKey.public_paths_from(xkids, parent_of, xp)
    for k, a, p in zip(xmany, parent_of, xp):
        want = xkids[a]
        for i in p:
            want = want.public_child(i)
        assert k.serialize() == want.serialize(), (a, p)
    assert ExtendedPublicKey.public_paths_from(xkids, None, [[3]])[0] == xkids[0].public_child(3)      # None: parent 0


def test_empty_path_and_empty_batch(host_paths):
    from bls_py.keys import ExtendedPrivateKey, ExtendedPublicKey
    esk, epk = _keys()
    kid = esk.private_child(H31 + 4)
    host_paths.calls.clear()
    assert [k.serialize() for k in kid.private_path_batch([[], []])] == [kid.serialize()] * 2
    assert kid.public_path_batch([[]])[0] == kid.get_extended_public_key()
    assert kid.get_extended_public_key().public_path_batch([[]])[0] == kid.get_extended_public_key()
    assert esk.private_path_batch([]) == [] and epk.public_path_batch([]) == [] and esk.public_path_batch([]) == []
    assert ExtendedPrivateKey.private_paths_from([], [], []) == [] and ExtendedPublicKey.public_paths_from([epk], [], []) == []
    assert host_paths.calls == []                                    # no device work for any of these


def test_exceptions_before_device_work(host_paths):
    from bls_py.keys import ExtendedPrivateKey, ExtendedPublicKey
    esk, epk = _keys()
    host_paths.calls.clear()
    with pytest.raises(Exception, match="Cannot derive hardened children from public key"):
        epk.public_path_batch([[1, 2], [3, H31]])
    with pytest.raises(Exception, match="Cannot derive hardened children from public key"):
        epk.public_path_batch([[2**32]])
    with pytest.raises(Exception, match="Cannot derive hardened children from public key"):
        ExtendedPublicKey.public_paths_from([epk, epk], [0, 1], [[1], [H31 + 1, 0]])
    for bad in (-1, 2**32, 2**40):
        with pytest.raises(OverflowError):
            esk.private_path_batch([[0], [1, bad]])
        with pytest.raises(OverflowError):
            esk.public_path_batch([[bad]])
    with pytest.raises(OverflowError):
        epk.public_path_batch([[0, -1]])
    deep = ExtendedPrivateKey(1, 253, 0, 0, esk.chain_code, esk.private_key)
    for paths in ([[1, 2, 3]], [[1], [1, 2], [H31, 1, 2]]):
        with pytest.raises(Exception, match="Cannot go further than 255 levels"):
            deep.private_path_batch(paths)
        with pytest.raises(Exception, match="Cannot go further than 255 levels"):
            deep.public_path_batch(paths)
        with pytest.raises(Exception, match="Cannot go further than 255 levels"):
            deep.get_extended_public_key().public_path_batch([[i % H31 for i in p] for p in paths])
    with pytest.raises(Exception, match="Cannot go further than 255 levels"):
        ExtendedPrivateKey.private_paths_from([esk, deep], [0, 1], [[1, 2, 3], [1, 2, 3]])
    with pytest.raises(IndexError):
        ExtendedPrivateKey.private_paths_from([esk], [0, 1], [[1], [2]])
    with pytest.raises(ValueError):
        ExtendedPublicKey.public_paths_from([epk], [0], [[1], [2]])
    assert host_paths.calls == []
    assert len(deep.private_path_batch([[1, 2], [5]])) == 2            # 255 itself is reachable


def test_fallback_without_hd_paths(fx, host_no_paths):
    from bls_py import backend
    from bls_py.keys import ExtendedPrivateKey, ExtendedPublicKey
    assert not hasattr(backend.get(), "hd_paths")
    esk, epk = _keys()
    paths = [[5, H31 + 1], [], [3], [1, 2, 3]]
    got = esk.private_path_batch(paths)
    assert [k.serialize() for k in got] == [esk.private_child(5).private_child(H31 + 1).serialize(), esk.serialize(),
                                            esk.private_child(3).serialize(),
                                            esk.private_child(1).private_child(2).private_child(3).serialize()]
    assert all(c[0] in ("hd_children", "g1_mul_gen") for c in host_no_paths.calls)
    soft = [[5, 1], [], [3]]
    assert [k.serialize() for k in epk.public_path_batch(soft)] == [epk.public_child(5).public_child(1).serialize(), epk.serialize(),
                                                                    epk.public_child(3).serialize()]
    assert ExtendedPublicKey.public_paths_from([epk], [0], [[7]])[0] == epk.public_child(7)
    assert ExtendedPrivateKey.private_paths_from([esk], None, [[7]])[0] == esk.private_child(7)
    with pytest.raises(Exception, match="Cannot derive hardened children from public key"):
        epk.public_path_batch([[H31]])
    check_public_record({"xpub": fx["public"]["xpub"], "paths": fx["public"]["paths"],
                         "epk": dict(fx["public"]["epk"], every16={k: v for k, v in list(fx["public"]["epk"]["every16"].items())[:4]})},
                        full=False)
