"""Shared by tests/test_seeds_host.py and tests/test_gpu_seeds.py: the keys-from-seeds vectors of tests/golden/seeds.json
(generated from the reference by tests/golden/make_golden_seeds.py), the byte-level definition the device call is compared
with (hmac / hashlib and Python integers), and a host-only provider with the keys_from_seeds extension and the secret forms
behind it (hostmath) for the CPU tests."""
import hashlib
import hmac
import json
import os

from bls_py import hostmath as H

from hd_paths_vectors import HostHDPaths

N = H.N
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = (b"BLS private key seed", b"BLS HD seed")
LENGTHS = [0, 1, 31, 32, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 128, 1023, 1024]
SEED_MAX = 1024


def load():
    with open(os.path.join(GOLDEN, "seeds.json")) as f:
        fx = json.load(f)
    assert fx["lengths"] == LENGTHS and fx["path"] == [2**31 + 44, 0, 5]
    seeds = [bytes.fromhex(r["seed"]) for r in fx["seeds"]]
    assert [len(s) for s in seeds[:4 * len(LENGTHS)]] == [L for L in LENGTHS for _ in range(4)]
    for mode in ("plain", "hd"):                                  # every class of the raw digest: below n, in [n, 2n), above
        assert {r[mode]["cls"] for r in fx["seeds"]} == {0, 1, 2}
    return fx


def by_length(fx):
    """{L: [records]} of the fixture, in its order"""
    out = {}
    for r in fx["seeds"]:
        out.setdefault(len(r["seed"]) // 2, []).append(r)
    return out


def mac(key, msg):
    return hmac.new(key, msg, hashlib.sha256).digest()


def host_keys(seed, hd):
    """(key as 32 bytes, chain code or None, class of the raw digest) by hmac and Python integers"""
    il = mac(KEYS[1], seed + b"\x00") if hd else mac(KEYS[0], seed)
    raw = int.from_bytes(il, "big")
    return (raw % N).to_bytes(32, "big"), mac(KEYS[1], seed + b"\x01") if hd else None, raw // N


def expected(recs, mode):
    """the fixture's bytes for records of one length: (sk, chain|None, aff, ser, parents|None)"""
    cat = lambda k: b"".join(bytes.fromhex(r[mode][k]) for r in recs)
    hd = mode == "hd"
    par = b"".join(bytes.fromhex(r["hd"]["chain"] + r["hd"]["aff"] + r["hd"]["sk"]) for r in recs) if hd else None
    return cat("sk"), cat("chain") if hd else None, cat("aff"), cat("ser"), par


class HostSeeds(HostHDPaths):
    """HostHDPaths with the keys_from_seeds extension of bls_py.backend on the host, by the device's contract, and the two
    secret forms the masters then meet (g1_mul_gen_secret, hd_paths_secret: the bytes of the plain forms), the calls
    recorded"""

    def _quiet(self, fn, *args):
        calls, self.calls = self.calls, []
        try:
            return fn(*args)
        finally:
            self.calls = calls

    def keys_from_seeds(self, seeds, seed_len, n, hd=False):
        self.calls.append(("keys_from_seeds", seed_len, n, bool(hd)))
        assert seed_len <= SEED_MAX and len(seeds) == seed_len * n
        got = [host_keys(seeds[seed_len * i:seed_len * (i + 1)], hd) for i in range(n)]
        sks = b"".join(g[0] for g in got)
        aff, ser = self._quiet(self.g1_mul_gen, sks)
        return sks, b"".join(g[1] for g in got) if hd else None, aff, ser, None

    def g1_mul_gen_secret(self, scalars):
        self.calls.append(("g1_mul_gen_secret", len(scalars) // 32))
        return self._quiet(self.g1_mul_gen, scalars)

    def hd_paths_secret(self, parents, parent_of, paths):
        self.calls.append(("hd_paths_secret", len(paths)))
        return self._quiet(self.hd_paths, parents, True, parent_of, paths)


__all__ = ["H", "HostSeeds", "KEYS", "LENGTHS", "N", "SEED_MAX", "by_length", "expected", "host_keys", "load", "mac"]
