#!/usr/bin/env python3
"""Generate tests/golden/seeds.json -- keys from seeds -- by IMPORTING the reference.

Runs only in the build container (needs the reference tree, read-only).  Nothing of the reference is copied: this script
calls PrivateKey.from_seed (keys.py:89-92), ExtendedPrivateKey.from_seed (keys.py:180-189), get_public_key and
private_child (keys.py:191-215) on seeded seeds and records what they return.  A few seconds.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_seeds.py

Contents:
  lengths   the seed lengths: every padding boundary of the HMAC's inner hash for a message of L and of L + 1 bytes (a
            block holds 55 message bytes beside the padding, 64 without), the empty seed and the device's limit of 1024;
  seeds     four seeds per length from a fixed random.Random, then -- only if a class below were missing -- more seeds of 32
            bytes: per seed its bytes, and for `plain` (PrivateKey.from_seed) and `hd` (ExtendedPrivateKey.from_seed) the
            private key, the public key serialised and affine, for hd the chain code, and `cls`: the class of the raw digest
            i_left the key was reduced from -- 0: below n, 1: in [n, 2n), 2: 2n and above (util.hmac256 of the reference,
            asserted here to reduce to the recorded key).  n = 0.453 * 2^256, so class 2 is about 9 % of digests: each mode
            is asserted to hold all three;
  paths     for the four seeds of 32 and of 64 bytes: the serialised leaf of private_child folded over PATH from the master.
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
from bls_py.keys import ExtendedPrivateKey, PrivateKey  # noqa: E402
from bls_py.util import hmac256  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "seeds.json")
N_ORDER = default_ec.n
LENGTHS = [0, 1, 31, 32, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 128, 1023, 1024]
PATH = [2**31 + 44, 0, 5]
PATH_LENGTHS = (32, 64)


def key_record(sk, i_left):
    pk = sk.get_public_key()
    A = pk.value.to_affine()
    assert not A.infinity
    raw = int.from_bytes(i_left, "big")
    assert raw % N_ORDER == sk.value
    return {"sk": "%064x" % sk.value, "ser": pk.serialize().hex(),
            "aff": (int(A.x).to_bytes(48, "big") + int(A.y).to_bytes(48, "big")).hex(), "cls": raw // N_ORDER}


def seed_record(seed):
    plain = key_record(PrivateKey.from_seed(seed), hmac256(seed, b"BLS private key seed"))
    esk = ExtendedPrivateKey.from_seed(seed)
    assert (esk.version, esk.depth, esk.parent_fingerprint, esk.child_number) == (1, 0, 0, 0)
    hd = key_record(esk.private_key, hmac256(seed + bytes([0]), b"BLS HD seed"))
    hd["chain"] = esk.chain_code.hex()
    return {"seed": seed.hex(), "plain": plain, "hd": hd}


def classes(recs, mode):
    return {r[mode]["cls"] for r in recs}


def main():
    rng = random.Random("seeds")
    recs = [seed_record(bytes(rng.randrange(256) for _ in range(L))) for L in LENGTHS for _ in range(4)]
    while classes(recs, "plain") != {0, 1, 2} or classes(recs, "hd") != {0, 1, 2}:
        recs.append(seed_record(bytes(rng.randrange(256) for _ in range(32))))
    for mode in ("plain", "hd"):
        assert classes(recs, mode) == {0, 1, 2}, mode

    paths = []
    for r in recs[:4 * len(LENGTHS)]:
        seed = bytes.fromhex(r["seed"])
        if len(seed) in PATH_LENGTHS:
            leaf = ExtendedPrivateKey.from_seed(seed)
            for i in PATH:
                leaf = leaf.private_child(i)
            paths.append({"seed": r["seed"], "leaf": leaf.serialize().hex(), "leaf_pk": leaf.get_public_key().serialize().hex()})
    assert len(paths) == 4 * len(PATH_LENGTHS)

    with open(OUT, "w") as f:
        json.dump({"lengths": LENGTHS, "path": PATH, "seeds": recs, "paths": paths}, f, indent=0)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(recs), "seeds")


if __name__ == "__main__":
    main()
