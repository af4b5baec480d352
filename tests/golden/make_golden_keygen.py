#!/usr/bin/env python3
"""Generate tests/golden/keygen.json -- public keys of fixed and seeded private keys -- by IMPORTING the reference.

Runs only in the build container (needs the reference tree, read-only).  Nothing of the reference is copied: this script
calls PrivateKey.get_public_key (keys.py:104-105) and PublicKey.serialize on the keys below and records what they return.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_keygen.py

Contents:
  cases   40 records {sk, aff, ser}: the private key (64 hex digits), the 96 affine bytes x || y of its public key and the
          48 bytes of PublicKey.serialize().  Records 0 .. 9 use sk = 1, 2, 7, 8, 9, 15, 16, 17, 2^255 mod n and n - 1 (the
          digit boundaries of a signed 4-bit recoding); the rest are seeded keys in [1, n).
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

from bls_py.ec import default_ec  # noqa: E402
from bls_py.keys import PrivateKey  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "keygen.json")
N_ORDER = default_ec.n


def record(sk):
    pk = PrivateKey(sk).get_public_key()
    A = pk.value.to_affine()
    assert not A.infinity
    aff = int(A.x).to_bytes(48, "big") + int(A.y).to_bytes(48, "big")
    return {"sk": "%064x" % sk, "aff": aff.hex(), "ser": pk.serialize().hex()}


def main():
    rng = random.Random(21)
    sks = [1, 2, 7, 8, 9, 15, 16, 17, (1 << 255) % N_ORDER, N_ORDER - 1]
    while len(sks) < 40:
        sks.append(rng.randrange(1, N_ORDER))
    cases = [record(sk) for sk in sks]
    with open(OUT, "w") as f:
        json.dump({"cases": cases}, f, indent=0)
    print("wrote", OUT, os.path.getsize(OUT), "bytes", len(cases), "cases")


if __name__ == "__main__":
    main()
