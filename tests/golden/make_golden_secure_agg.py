#!/usr/bin/env python3
"""Generate tests/golden/secure_agg.json -- hash_pks exponents and the three secure aggregations -- by IMPORTING the
reference.

Runs only in the build container (needs the reference tree, read-only).  Nothing of the reference is copied: this script
calls util.hash_pks (util.py:36-50), BLS.aggregate_pub_keys / aggregate_priv_keys with secure=True (bls.py:203-249),
BLS.aggregate_sigs_secure (bls.py:28-56) and PrivateKey.sign on seeded keys and records what they return.  A few seconds.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_secure_agg.py

Contents:
  pool       65 seeded private keys (hex) and the 48-byte serialisations of their public keys;
  hash_pks   for k in 1..9, 64, 65: the pool indices of a shuffled group of k keys and hash_pks(k + 3, keys) -- the
             exponents for num_outputs 1 and k are its first 1 and k entries (asserted here against the reference);
  pub_keys   aggregate_pub_keys(keys, secure=True) for groups of 1, 2, 3, 5 and 9 keys given UNSORTED: the serialised result;
  sigs       aggregate_sigs_secure(sigs, keys, message_hashes) for groups of 1, 2, 3 and 5 signers over one message, over
             distinct messages and over a mixture: pool indices, messages, the signatures as 192-byte affine hex and the
             serialised result.  As it stands the reference's function cannot run on its own types: bls.py:49 reads `.ec` of
             a PublicKey, which has none, and bls.py:54 multiplies a Signature by an integer, which it does not define
             (BLS.aggregate_sigs, bls.py:141, writes signature.value * t).  The objects handed to this one call carry
             exactly those two things -- an `ec` attribute and a __mul__ that is value * t -- so that the reference's own
             lines decide the order of the signatures and of the exponents;
  priv_keys  aggregate_priv_keys(sks, pks, secure=True) for groups whose public_keys argument is deliberately NOT sorted
             (pks[i] is the key of sks[i], shuffled) and one group whose public keys are not the private keys' own: the
             reference sorts the (public, private) pairs and hashes the public keys as given (bls.py:239-241).
"""
import json
import logging
import os
import random
import sys

logging.disable(logging.CRITICAL)
sys.dont_write_bytecode = True
REF = os.environ.get("BLS_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from bls_py.bls import BLS  # noqa: E402
from bls_py.ec import default_ec  # noqa: E402
from bls_py.keys import PrivateKey  # noqa: E402
from bls_py.signature import Signature  # noqa: E402
from bls_py.util import hash256, hash_pks  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "secure_agg.json")
N_ORDER = default_ec.n
KS = list(range(1, 10)) + [64, 65]


class _MulSignature(Signature):
    """a reference Signature that bls.py:54 can multiply (see the module docstring)"""

    def __mul__(self, t):
        return self.value * t


def aff_hex(J):
    A = J.to_affine()
    if A.infinity:
        return bytes(192).hex()
    return b"".join(int(c).to_bytes(48, "big") for c in (A.x[0], A.x[1], A.y[0], A.y[1])).hex()


def main():
    rng = random.Random("secure-agg")
    sks = [PrivateKey(rng.randrange(1, N_ORDER)) for _ in range(65)]
    pks = [sk.get_public_key() for sk in sks]
    pool = {"sks": ["%064x" % sk.value for sk in sks], "pks": [pk.serialize().hex() for pk in pks]}

    hp = []
    for k in KS:
        idx = rng.sample(range(65), k)
        keys = [pks[i] for i in idx]
        ts = hash_pks(k + 3, keys)
        assert hash_pks(1, keys) == ts[:1] and hash_pks(k, keys) == ts[:k] and all(0 <= t < N_ORDER for t in ts)
        hp.append({"k": k, "keys": idx, "num_outputs": [1, k, k + 3], "ts": ["%064x" % t for t in ts]})

    pub = []
    for k in (1, 2, 3, 5, 9):
        idx = rng.sample(range(65), k)
        agg = BLS.aggregate_pub_keys([pks[i] for i in idx], True)          # (sorts its own list)
        pub.append({"keys": idx, "aggregate": agg.serialize().hex()})

    sg = []
    for k, kind in ((1, "one"), (2, "one"), (3, "distinct"), (5, "mixed"), (5, "one")):
        idx = rng.sample(range(65), k)
        if kind == "one":
            msgs = [b"secure agg fixture"] * k
        elif kind == "distinct":
            msgs = [b"message %d" % j for j in range(k)]
        else:
            msgs = [b"message %d" % (j % 2) for j in range(k)]
        sigs = [sks[i].sign(m) for i, m in zip(idx, msgs)]
        keys = [pks[i] for i in idx]
        for pk in keys:
            pk.ec = default_ec
        for sig in sigs:
            sig.__class__ = _MulSignature
        agg = BLS.aggregate_sigs_secure(sigs, keys, [hash256(m) for m in msgs])
        sg.append({"keys": idx, "kind": kind, "msgs": [m.hex() for m in msgs], "sigs": [aff_hex(s.value) for s in sigs],
                   "aggregate": agg.serialize().hex()})

    pv = []
    for k in (1, 2, 3, 5, 9):
        while True:
            idx = rng.sample(range(65), k)
            ser = [pool["pks"][i] for i in idx]
            if k < 3 or (ser != sorted(ser) and ser != sorted(ser, reverse=True)):
                break
        agg = BLS.aggregate_priv_keys([sks[i] for i in idx], [pks[i] for i in idx], True)
        pv.append({"sks": idx, "pks": idx, "aggregate": "%064x" % agg.value})
    idx, other = rng.sample(range(65), 4), rng.sample(range(65), 4)
    agg = BLS.aggregate_priv_keys([sks[i] for i in idx], [pks[i] for i in other], True)
    pv.append({"sks": idx, "pks": other, "aggregate": "%064x" % agg.value})

    with open(OUT, "w") as f:
        json.dump({"pool": pool, "hash_pks": hp, "pub_keys": pub, "sigs": sg, "priv_keys": pv}, f, indent=0)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
