"""Shared by tests/test_secure_agg_host.py and tests/test_gpu_secure_agg.py: the secure-aggregation vectors of
tests/golden/secure_agg.json (generated from the reference by tests/golden/make_golden_secure_agg.py) checked through
whatever provider bls_py.backend holds, the byte-level compositions the device calls are compared with, and a host-only
provider of the four device operations (hashlib + hostmath + Python integers) for the CPU tests."""
import hashlib
import random

from bls_py import hostmath as H

from lagrange_vectors import be32, ints32
from rxsecret_vectors import HostRxSecret

N = H.N


def host_digests(pks_ser, k, groups):
    return b"".join(hashlib.sha256(pks_ser[48 * k * g:48 * k * (g + 1)]).digest() for g in range(groups))


def host_ts(pks_ser, k, m, groups, digests=None):
    """the exponents of `groups` groups of k serialised keys as ints, group by group: hashlib and Python integers"""
    dg = digests if digests is not None else host_digests(pks_ser, k, groups)
    return [int.from_bytes(hashlib.sha256(i.to_bytes(4, "big") + dg[32 * g:32 * (g + 1)]).digest(), "big") % N
            for g in range(groups) for i in range(m)]


def seeded_keys(seed, count):
    """`count` strings of 48 bytes that stand for serialised keys (hash_pks hashes bytes; they need not be points)"""
    rnd = random.Random(seed)
    return b"".join(rnd.randbytes(48) for _ in range(count))


class HostSecureAgg(HostRxSecret):
    """hash_pks, aggregate_pub_keys_secure, aggregate_sigs_secure and aggregate_priv_keys_secure of
    bls_py.backend.HipProvider on the host, by the device's contract, with the calls recorded; the rest from HostRxSecret
    (which has none of the four: it is the provider WITHOUT the entries)."""

    def hash_pks(self, pks_ser, k, m, groups=1):
        self.calls.append(("hash_pks", k, m, groups))
        assert k >= 1 and m >= 1 and len(pks_ser) == 48 * k * groups
        return be32(host_ts(bytes(pks_ser), k, m, groups))

    def aggregate_pub_keys_secure(self, pts_aff, pks_ser, k, groups=1):
        self.calls.append(("aggregate_pub_keys_secure", k, groups))
        assert len(pts_aff) == 96 * k * groups
        return self._quiet(HostRxSecret.g1_msm, pts_aff, host_ts(bytes(pks_ser), k, k, groups), k, groups)

    def aggregate_sigs_secure(self, sigs_aff, k, pks_ser, k_pks, groups=1):
        self.calls.append(("aggregate_sigs_secure", k, k_pks, groups))
        assert len(sigs_aff) == 192 * k * groups
        return self._g2_msm(sigs_aff, host_ts(bytes(pks_ser), k_pks, k, groups), k, groups)

    def aggregate_priv_keys_secure(self, sks, pks_ser, k, groups=1, pk=False):
        self.calls.append(("aggregate_priv_keys_secure", k, groups, bool(pk)))
        ys, ts = ints32(bytes(sks)), host_ts(bytes(pks_ser), k, k, groups)
        assert 1 <= k <= self.LAGRANGE_MAX_K and len(ys) == k * groups
        out = be32([sum(t * y for t, y in zip(ts[g * k:(g + 1) * k], ys[g * k:(g + 1) * k])) % N for g in range(groups)])
        aff, ser = self._quiet(HostRxSecret.g1_mul_gen, out) if pk else (None, None)
        return out, aff, ser


# ---- the fixture through the Python entry points ---------------------------------------------------------------------------
class Pool:
    """the fixture's 65 keys as PrivateKey / PublicKey objects (the public keys multiplied by the installed provider and
    checked against the fixture's serialisations)"""

    def __init__(self, fx):
        from bls_py.keys import PrivateKey
        self.sks = [PrivateKey(int(h, 16)) for h in fx["pool"]["sks"]]
        self.pks = PrivateKey.get_public_key_batch(self.sks)
        assert [pk.serialize().hex() for pk in self.pks] == fx["pool"]["pks"]


def signature(h):
    """Signature from the fixture's 192-byte affine hex"""
    from bls_py.ec import JacobianPoint
    from bls_py.signature import Signature
    return Signature.from_g2(JacobianPoint._from(H.F2, H.aff_to_jac(H.F2, H.g2_from_abi(bytes.fromhex(h)))))


def check_hash_pks(fx, pool):
    from bls_py.util import hash_pks, hash_pks_batch
    assert [r["k"] for r in fx["hash_pks"]] == list(range(1, 10)) + [64, 65]
    groups = [[pool.pks[i] for i in r["keys"]] for r in fx["hash_pks"]]
    for which in range(3):
        for m in sorted({r["num_outputs"][which] for r in fx["hash_pks"]}):
            sel = [j for j, r in enumerate(fx["hash_pks"]) if r["num_outputs"][which] == m]
            got = hash_pks_batch(m, [groups[j] for j in sel])
            assert got == [[int(t, 16) for t in fx["hash_pks"][j]["ts"][:m]] for j in sel]
            assert got == [hash_pks(m, groups[j]) for j in sel]
    # one call over every group with one num_outputs: one device call per distinct length
    assert hash_pks_batch(4, groups) == [[int(t, 16) for t in r["ts"][:4]] for r in fx["hash_pks"]]


def check_pub_keys(fx, pool):
    from bls_py.bls import BLS
    groups = [[pool.pks[i] for i in r["keys"]] for r in fx["pub_keys"]]
    before = [list(g) for g in groups]
    got = BLS.aggregate_pub_keys_batch(groups, True)
    assert [pk.serialize().hex() for pk in got] == [r["aggregate"] for r in fx["pub_keys"]]
    assert all(a is b for g, h in zip(groups, before) for a, b in zip(g, h)), "the caller's lists were reordered"
    assert got == [BLS.aggregate_pub_keys(list(g), True) for g in groups]
    assert BLS.aggregate_pub_keys_batch(groups, False) == [BLS.aggregate_pub_keys(list(g), False) for g in groups]


def check_sigs(fx, pool):
    from bls_py.bls import BLS
    from bls_py.util import hash256
    sig_groups = [[signature(h) for h in r["sigs"]] for r in fx["sigs"]]
    pk_groups = [[pool.pks[i] for i in r["keys"]] for r in fx["sigs"]]
    mh_groups = [[hash256(bytes.fromhex(m)) for m in r["msgs"]] for r in fx["sigs"]]
    assert {r["kind"] for r in fx["sigs"]} == {"one", "distinct", "mixed"}
    got = BLS.aggregate_sigs_secure_batch(sig_groups, pk_groups, mh_groups)
    assert [s.serialize().hex() for s in got] == [r["aggregate"] for r in fx["sigs"]]
    assert got == [BLS.aggregate_sigs_secure(s, p, m) for s, p, m in zip(sig_groups, pk_groups, mh_groups)]


def check_priv_keys(fx, pool, secret):
    from bls_py.bls import BLS
    groups = [[pool.sks[i] for i in r["sks"]] for r in fx["priv_keys"]]
    pk_groups = [[pool.pks[i] for i in r["pks"]] for r in fx["priv_keys"]]
    # the quirk is in the fixture: some group's public keys are not in sorted order, one group's are not the keys' own
    assert any([pk.serialize() for pk in p] != sorted(pk.serialize() for pk in p) for p in pk_groups)
    assert any(r["sks"] != r["pks"] for r in fx["priv_keys"])
    before = [list(g) for g in groups], [list(p) for p in pk_groups]
    keys, pks = BLS.aggregate_priv_keys_batch(groups, secret=secret, public_keys=True, secure_with=pk_groups)
    assert ["%064x" % k.value for k in keys] == [r["aggregate"] for r in fx["priv_keys"]]
    loop = [BLS.aggregate_priv_keys(g, p, True) for g, p in zip(groups, pk_groups)]
    assert [k.value for k in keys] == [k.value for k in loop]
    assert pks == [k.get_public_key() for k in loop] and [p.serialize() for p in pks] == [k.get_public_key().serialize() for k in loop]
    assert [k.value for k in BLS.aggregate_priv_keys_batch(groups, secret=secret, secure_with=pk_groups)] == [k.value for k in loop]
    assert all(a is b for v, w in zip((groups, pk_groups), before) for g, h in zip(v, w) for a, b in zip(g, h))


__all__ = ["H", "HostSecureAgg", "N", "Pool", "be32", "check_hash_pks", "check_priv_keys", "check_pub_keys", "check_sigs",
           "host_digests", "host_ts", "ints32", "seeded_keys", "signature"]
