"""Shared by tests/test_hd_host.py and tests/test_gpu_hd_keys.py: the HD key vectors of tests/golden/hd.json (generated
from the reference by tests/golden/make_golden_hd.py) checked through whatever provider bls_py.backend holds, and a
host-only provider of the two HD operations (hostmath + util.hmac256) for the CPU tests."""
import hashlib

from bls_py import hostmath as H
from bls_py.util import hmac256


def xprv_index(k):
    return k // 2 + (2**31 if k & 1 else 0)


class HostHD:
    """g1_mul_gen / hd_children of bls_py.backend.HipProvider on the host: the reference's formulas, no GPU."""

    def __init__(self, inner=None):
        self.inner = inner
        self.calls = []

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def g1_mul_gen(self, scalars, add=None, n_add=0):
        self.calls.append(("g1_mul_gen", len(scalars) // 32))
        aff, ser = [], []
        for i in range(len(scalars) // 32):
            s = int.from_bytes(scalars[32 * i:32 * (i + 1)], "big") % H.N
            P = H.jac_mul(H.F1, H.aff_to_jac(H.F1, H.G1_GEN), s)
            if n_add:
                j = i if n_add > 1 else 0
                P = H.jac_add(H.F1, P, H.aff_to_jac(H.F1, H.g1_from_abi(add[96 * j:96 * (j + 1)])))
            A = H.jac_to_affine(H.F1, P)
            aff.append(H.g1_affine_bytes(A))
            ser.append(H.g1_compress(A))
        return b"".join(aff), b"".join(ser)

    def hd_children(self, chain_code, parent_pk_aff, parent_sk, indices):
        self.calls.append(("hd_children", len(indices)))
        pk_ser = H.g1_compress(H.g1_from_abi(parent_pk_aff))
        chains, scal = [], []
        for i in indices:
            if parent_sk is None and i >= 2**31:
                raise ValueError("hardened index in public mode")
            msg = (parent_sk if parent_sk is not None and i >= 2**31 else pk_ser) + i.to_bytes(4, "big")
            il, ir = hmac256(msg + b"\x00", chain_code), hmac256(msg + b"\x01", chain_code)
            chains.append(ir)
            if parent_sk is None:
                scal.append(il)
            else:
                scal.append(((int.from_bytes(il, "big") + int.from_bytes(parent_sk, "big")) % H.N).to_bytes(32, "big"))
        sb = b"".join(scal)
        aff, ser = self.g1_mul_gen(sb, parent_pk_aff if parent_sk is None else None, 1 if parent_sk is None else 0)
        return b"".join(chains), (sb if parent_sk is not None else None), aff, ser


def check_seed_record(rec):
    """one seed of hd.json: the root keys, its children at the fixture's indices (batched and one by one), the
    two-level chains"""
    from bls_py.keys import ExtendedPrivateKey, ExtendedPublicKey
    esk = ExtendedPrivateKey.from_seed(bytes.fromhex(rec["seed"]))
    epk = esk.get_extended_public_key()
    assert esk.serialize().hex() == rec["esk"]
    assert epk.serialize().hex() == rec["epk"]
    assert esk.get_public_key().get_fingerprint() == rec["fingerprint"]
    assert esk.chain_code.hex() == rec["chain_code"]
    assert ExtendedPublicKey.from_bytes(bytes.fromhex(rec["epk"])) == epk
    kids = rec["children"]
    batch = esk.private_child_batch([c["i"] for c in kids])
    pubs = [c for c in kids if c["pub"] is not None]
    pbatch = epk.public_child_batch([c["i"] for c in pubs])
    for c, b in zip(kids, batch):
        assert b.serialize().hex() == c["esk"], c["i"]
        assert b.get_extended_public_key().serialize().hex() == c["epk"], c["i"]
        assert b.get_public_key().get_fingerprint() == c["fingerprint"]
        assert b.child_number == c["i"] and b.depth == 1
    assert [p.serialize().hex() for p in pbatch] == [c["pub"] for c in pubs]
    assert [e.serialize().hex() for e in esk.public_child_batch([c["i"] for c in kids])] == [c["epk"] for c in kids]
    # one by one: the same objects
    for c in kids[:3] + kids[-2:]:
        assert esk.private_child(c["i"]).serialize().hex() == c["esk"]
        assert esk.public_child(c["i"]).serialize().hex() == c["epk"]
        if c["pub"] is not None:
            assert epk.public_child(c["i"]).serialize().hex() == c["pub"]
    for ch in rec["chains"]:
        k = esk
        for i in ch["path"]:
            k = k.private_child(i)
        assert k.serialize().hex() == ch["esk"], ch["path"]
        assert k.get_extended_public_key().serialize().hex() == ch["epk"], ch["path"]
        if ch["pub"] is not None:
            p = epk
            for i in ch["path"]:
                p = p.public_child(i)
            assert p.serialize().hex() == ch["pub"]
            assert p == k.get_extended_public_key()


def check_xpub_range(rec, full=True):
    from bls_py.keys import ExtendedPublicKey
    xpub = ExtendedPublicKey.from_bytes(bytes.fromhex(rec["xpub"]))
    if full:
        kids = [k.serialize() for k in xpub.public_child_batch(range(rec["count"]))]
        assert hashlib.sha256(b"".join(kids)).hexdigest() == rec["sha256"]
        for i, h in rec["every64"].items():
            assert kids[int(i)].hex() == h
    else:
        idx = sorted(int(i) for i in rec["every64"])[:4]
        assert [k.serialize().hex() for k in xpub.public_child_batch(idx)] == [rec["every64"][str(i)] for i in idx]


def check_xprv_range(rec, full=True):
    from bls_py.keys import ExtendedPrivateKey
    xprv = ExtendedPrivateKey.from_seed(bytes.fromhex(rec["seed"]))
    ks = list(range(rec["count"])) if full else sorted(int(k) for k in rec["every32"])[:4]
    kids = [k.serialize() for k in xprv.private_child_batch([xprv_index(k) for k in ks])]
    if full:
        assert hashlib.sha256(b"".join(kids)).hexdigest() == rec["sha256"]
        for k, h in rec["every32"].items():
            assert kids[int(k)].hex() == h
    else:
        assert [k.hex() for k in kids] == [rec["every32"][str(k)] for k in ks]
