"""Shared by tests/test_sigshares_host.py and tests/test_gpu_sigshares.py: threshold sessions built from fixed seeds with
hostmath -- share keys from a small polynomial, H(m), signature shares of both forms -- with the exact per-share truth
sigma_i == c H(m), c = lambda_i sk_i (scaled) or sk_i (plain); the fixture tests/golden/sigshares.json (generated from the
reference by tests/golden/make_golden_sigshares.py) as objects; and a host-only provider whose sig_shares_check is the exact
per-share two-pair check."""
import hashlib
import random

from bls_py import hostmath as H
from bls_py import util

from lagrange_vectors import host_coeffs
from rxsecret_vectors import HostRxSecret
from subgroup_vectors import HostRLC

N = H.N
PLAYERS = 67                        # the universe: players 1 .. 67, sk_x = POLY(x)
_rng = random.Random("sigshares universe")
POLY = [_rng.randrange(1, N) for _ in range(3)]
SK = {x: sum(c * pow(x, e, N) for e, c in enumerate(POLY)) % N for x in range(1, PLAYERS + 1)}
_cache = {}


def msg_hash(tag):
    return hashlib.sha256(b"sigshares %d" % tag if isinstance(tag, int) else tag).digest()


def hm(mh):
    """H(m) as a hostmath Jacobian point"""
    key = ("H", mh)
    if key not in _cache:
        _cache[key] = H.aff_to_jac(H.F2, H.hash_to_g2_prehashed(mh, util.hash512))
    return _cache[key]


def share_bytes(c, mh):
    """(c mod n) H(m), 192 affine bytes (computed once per (c, m))"""
    key = ("S", c % N, mh)
    if key not in _cache:
        _cache[key] = H.g2_affine_bytes(H.jac_to_affine(H.F2, H.jac_mul(H.F2, hm(mh), c % N)))
    return _cache[key]


def pk_bytes(x):
    """sk_x G1, 96 affine bytes"""
    key = ("P", x)
    if key not in _cache:
        _cache[key] = H.g1_affine_bytes(H.jac_to_affine(H.F1, H.jac_mul(H.F1, H.aff_to_jac(H.F1, H.G1_GEN), SK[x])))
    return _cache[key]


def coefficient(players, j, scaled):
    """c of share j of a session: lambda_j sk_j mod n, or sk_j"""
    if not scaled:
        return SK[players[j]]
    key = ("L", tuple(players))
    if key not in _cache:
        _cache[key] = host_coeffs(list(players))[0]
    return _cache[key][j] * SK[players[j]] % N


def outside_g2(golden):
    """a point on the twist outside G2 from tests/golden/subgroup.json, 192 bytes"""
    rec = next(r for r in golden("subgroup.json")["g2"] if r["on_curve"] and not r["in_subgroup"] and any(bytes.fromhex(r["point"])))
    return bytes.fromhex(rec["point"])


def outside_g1(golden):
    rec = next(r for r in golden("subgroup.json")["g1"] if r["on_curve"] and not r["in_subgroup"] and any(bytes.fromhex(r["point"])))
    return bytes.fromhex(rec["point"])


class Session:
    """k shares of the players `players` over message hash `mh`.  bad: {position: kind}, kinds
    "wrong" (c + 1 instead of c: in G2, wrong), "other_player" (the correct share of the next player), "other_msg" (the
    player's share on another message), "infinity", "off_twist" (y.c0 + 1), or 192 bytes given outright."""

    def __init__(self, players, mh, scaled, bad=None):
        self.players, self.mh, self.scaled = list(players), mh, scaled
        k = len(self.players)
        self.good = [share_bytes(coefficient(self.players, j, scaled), mh) for j in range(k)]
        self.sigs = list(self.good)
        for j, kind in (bad or {}).items():
            self.sigs[j] = self.spoil(j, kind)
        self.keys = [pk_bytes(x) for x in self.players]

    def spoil(self, j, kind):
        c = coefficient(self.players, j, self.scaled)
        if isinstance(kind, (bytes, bytearray)):
            return bytes(kind)
        if kind == "wrong":
            return share_bytes(c + 1, self.mh)
        if kind == "other_player":
            return self.good[(j + 1) % len(self.good)]
        if kind == "other_msg":
            return share_bytes(c, msg_hash(b"another message"))
        if kind == "infinity":
            return bytes(192)
        if kind == "off_twist":
            b = bytearray(self.good[j])
            b[143] ^= 1                                   # the last byte of y.c0
            return bytes(b)
        raise ValueError(kind)

    def truth(self):
        """the exact per-share truth: sigma_i == c_i H(m)"""
        return [s == g for s, g in zip(self.sigs, self.good)]


def pack(sessions, weights=None, seed=1):
    """the arguments of sig_shares_check for sessions of one k: (sigs, keys, key_idx, x, msg_hashes, weights, k, groups) with
    the keys deduplicated into a table, and the truth as status bytes"""
    k = len(sessions[0].players)
    assert all(len(s.players) == k for s in sessions)
    table, rows = [], {}
    idx = []
    for s in sessions:
        for kb in s.keys:
            if kb not in rows:
                rows[kb] = len(table)
                table.append(kb)
            idx.append(rows[kb])
    rng = random.Random(seed)
    if weights is None:
        weights = [rng.getrandbits(64) or 1 for _ in range(k * len(sessions))]
    return dict(sigs=b"".join(b for s in sessions for b in s.sigs), keys=b"".join(table), key_idx=idx,
                x=b"".join(x.to_bytes(32, "big") for s in sessions for x in s.players),
                msg_hashes=b"".join(s.mh for s in sessions), weights=list(weights), k=k, groups=len(sessions))


def truth_bytes(sessions):
    return bytes(int(t) for s in sessions for t in s.truth())


# ---- the fixture as objects -----------------------------------------------------------------------------------------------
def fixture_objects(fx):
    """(share public keys as PublicKey objects, player p at index p - 1; per message a dict with hash, signers, unit / plain
    Signature objects and the combined serialisation)"""
    from bls_py.keys import PublicKey
    from bls_py.signature import Signature
    pks = [PublicKey.from_bytes(bytes.fromhex(h)) for h in fx["share_pks_ser"]]
    msgs = []
    for m in fx["messages"]:
        msgs.append({"hash": bytes.fromhex(m["msg_hash"]), "signers": list(m["signers"]),
                     "unit": [Signature.from_bytes(bytes.fromhex(h)) for h in m["unit_sigs"]],
                     "plain": [Signature.from_bytes(bytes.fromhex(h)) for h in m["plain_sigs"]], "combined": m["combined"]})
    return pks, msgs


def fixture_truth(fx, m, sigs, players, scaled):
    """sigma_i == c_i H(m) for Signature objects against the fixture's secret shares"""
    mh = bytes.fromhex(fx["messages"][m]["msg_hash"])
    sk = [int(s, 16) for s in fx["shares"]]
    lam = host_coeffs(list(players))[0] if scaled else [1] * len(players)
    return [H.g2_affine_bytes(sg.value.to_affine()._aff()) == share_bytes(l * sk[p - 1] % N, mh)
            for sg, p, l in zip(sigs, players, lam)]


# ---- the host provider ------------------------------------------------------------------------------------------------------
class HostSigShares(HostRLC, HostRxSecret):
    """sig_shares_check of bls_py.backend.HipProvider on the host by the device's contract -- the exact per-share two-pair
    check, no randomisation: the weights are ignored -- on the CPU oracle's pairings and sums (HostRLC); the Lagrange,
    share-check and combine operations from the other host providers."""
    LAGRANGE_MAX_K = 1024

    def __init__(self, oracle):
        HostRLC.__init__(self, oracle)
        self.inner = None

    def sig_shares_check(self, sigs, keys, key_idx, x, msg_hashes, weights, k, groups=1, scaled=True):
        from bls_py.threshold import Threshold
        from subgroup_vectors import g1_status, g2_status
        self.calls.append(("sig_shares_check", k, groups, scaled))
        n = k * groups
        assert len(sigs) == 192 * n and len(key_idx) == n and len(msg_hashes) == 32 * groups and len(weights) in (n, 8 * n)
        assert all(0 <= i < len(keys) // 96 for i in key_idx) and (not scaled or len(x) == 32 * n)
        key_st = [g1_status(H.g1_from_abi(keys[96 * i:96 * (i + 1)])) for i in range(len(keys) // 96)]
        status, sess, items, where = bytearray(n), bytearray(groups), [], []
        for g in range(groups):
            lam, ok = [1] * k, 1
            if scaled:
                lam, ok = host_coeffs([int.from_bytes(x[32 * (g * k + j):32 * (g * k + j + 1)], "big") for j in range(k)])
            sess[g] = ok
            for j in range(k):
                i = g * k + j
                sb = sigs[192 * i:192 * (i + 1)]
                if not ok or not any(sb) or g2_status(H.g2_from_abi(sb)) != 1:
                    status[i] = 0
                elif key_st[key_idx[i]] != 1:
                    status[i] = 2
                else:
                    items.append((sb, keys[96 * key_idx[i]:96 * (key_idx[i] + 1)], lam[j], msg_hashes[32 * g:32 * (g + 1)]))
                    where.append(i)
        for i, okay in zip(where, Threshold._sig_shares_exact(self, items)):
            status[i] = 1 if okay else 0
        return bytes(status), bytes(sess), (0, len(items))
