#!/usr/bin/env python3
"""Generate tests/golden/sign.json -- signatures of seeded (private key, message) pairs -- by IMPORTING the reference.

Runs only in the build container (needs the reference tree, read-only).  Nothing of the reference is copied: this script
calls PrivateKey.sign_prehashed (keys.py:128-132) and Signature.serialize on seeded inputs and records what they return.
About a minute (the reference signs in pure Python).

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_sign.py

Contents:
  cases   32 records {sk, msg, hash, sig, aff}: the private key (64 hex digits), the message and its hash256, the 96 bytes
          of sign_prehashed(hash).serialize() and the 192 affine bytes x.c0 x.c1 y.c0 y.c1 of the signature point.
          Records 0 .. 2 use sk = 1, 2, n - 1; records 3 .. 7 are five seeded keys on ONE message (the same-message group,
          listed in `same_message`); the rest are seeded keys below n on seeded messages of 0 .. 70 bytes.
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
from bls_py.util import hash256  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sign.json")
N_ORDER = default_ec.n


def record(sk, msg):
    h = hash256(msg)
    sig = PrivateKey(sk).sign_prehashed(h)
    A = sig.value.to_affine()
    assert not A.infinity
    aff = b"".join(int(c).to_bytes(48, "big") for c in (A.x[0], A.x[1], A.y[0], A.y[1]))
    return {"sk": "%064x" % sk, "msg": msg.hex(), "hash": h.hex(), "sig": sig.serialize().hex(), "aff": aff.hex()}


def main():
    rng = random.Random(20)
    cases = [record(sk, b"sign fixture, small and large keys") for sk in (1, 2, N_ORDER - 1)]
    same = list(range(len(cases), len(cases) + 5))
    cases += [record(rng.randrange(1, N_ORDER), b"sign fixture, one message for five keys") for _ in same]
    while len(cases) < 32:
        msg = bytes(rng.randrange(256) for _ in range(rng.randrange(71)))
        cases.append(record(rng.randrange(1, N_ORDER), msg))
    with open(OUT, "w") as f:
        json.dump({"cases": cases, "same_message": same}, f, indent=0)
    print("wrote", OUT, os.path.getsize(OUT), "bytes", len(cases), "cases")


if __name__ == "__main__":
    main()
