#!/usr/bin/env python3
"""Generate tests/golden/sigshares.json -- a 3-of-5 Joint-Feldman key and its signature shares of both forms -- by IMPORTING
the reference.

Runs only in the build container (needs the reference tree, read-only).  Nothing of the reference is copied: this script
patches the reference's keys.RNG with a seeded random.Random, calls PrivateKey.new_threshold (keys.py:95-117) once per
dealer, BLS.aggregate_priv_keys / aggregate_pub_keys without secure aggregation (bls.py:203-249) for the shares and the
master key, PrivateKey.sign_threshold (keys.py:134-143), PrivateKey.sign (keys.py:123-126), BLS.aggregate_sigs_simple (the sum of
the unit signatures) and Threshold.aggregate_unit_sigs (threshold.py:127-136), and records what they return.  Under a minute.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_sigshares.py

Contents (everything hex):
  T, N, seed     the sharing: 3-of-5, and the seed of the patched RNG
  commitments    per dealer its T commitments, 96-byte affine G1
  shares         the five secret shares (player p at index p - 1), 32 bytes
  share_pks      their public keys, 96-byte affine G1, and share_pks_ser, the 48-byte serialisations
  master_pk      the master public key, serialised (48 bytes)
  messages       two records: msg, msg_hash (sha256, what hash_to_point_Fq2 hashes), signers (the signer set of the unit
                 signatures), unit_sigs (sign_threshold of every signer, in the signers' order) and plain_sigs (sign of all
                 five players) as 96-byte serialisations, and combined: the master signature, which the sum of the unit signatures,
                 aggregate_unit_sigs of the first three plain shares and the master secret's own sign all return
"""
import hashlib
import json
import logging
import os
import random
import sys

logging.disable(logging.CRITICAL)
sys.dont_write_bytecode = True
REF = os.environ.get("BLS_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from bls_py import keys  # noqa: E402
from bls_py.bls import BLS  # noqa: E402
from bls_py.keys import PrivateKey  # noqa: E402
from bls_py.threshold import Threshold  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sigshares.json")
T, N, SEED = 3, 5, "sigshares 3-of-5"
MESSAGES = [(b"sigshares fixture message one", [4, 1, 5]), (b"sigshares fixture message two", [2, 3, 1])]


def g1_hex(J):
    A = J.to_affine()
    return (int(A.x).to_bytes(48, "big") + int(A.y).to_bytes(48, "big")).hex()


def main():
    keys.RNG = random.Random(SEED)
    dealt = [PrivateKey.new_threshold(T, N) for _ in range(N)]
    master_sk = BLS.aggregate_priv_keys([d[0] for d in dealt], None, False)
    master_pk = BLS.aggregate_pub_keys([d[0].get_public_key() for d in dealt], False)
    assert master_sk.get_public_key().serialize() == master_pk.serialize()
    for p in range(1, N + 1):
        for d in dealt:
            assert Threshold.verify_secret_fragment(T, d[2][p - 1], p, d[1])
    shares = [BLS.aggregate_priv_keys([PrivateKey(d[2][p - 1]) for d in dealt], None, False) for p in range(1, N + 1)]
    share_pks = [s.get_public_key() for s in shares]
    messages = []
    for msg, signers in MESSAGES:
        unit = [shares[p - 1].sign_threshold(msg, p, signers) for p in signers]
        plain = [s.sign(msg) for s in shares]
        combined = BLS.aggregate_sigs_simple(unit)
        master = master_sk.sign(msg)
        assert combined.serialize() == master.serialize()
        assert Threshold.aggregate_unit_sigs(plain[:T], list(range(1, T + 1)), T).serialize() == master.serialize()
        messages.append({"msg": msg.hex(), "msg_hash": hashlib.sha256(msg).hexdigest(), "signers": signers,
                         "unit_sigs": [u.serialize().hex() for u in unit], "plain_sigs": [s.serialize().hex() for s in plain],
                         "combined": master.serialize().hex()})
    doc = {"T": T, "N": N, "seed": SEED,
           "commitments": [[g1_hex(c.to_jacobian() if hasattr(c, "to_jacobian") else c) for c in d[1]] for d in dealt],
           "shares": ["%064x" % int(s.value) for s in shares],
           "share_pks": [g1_hex(pk.value) for pk in share_pks], "share_pks_ser": [pk.serialize().hex() for pk in share_pks],
           "master_pk": master_pk.serialize().hex(), "messages": messages}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
