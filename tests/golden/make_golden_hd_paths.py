#!/usr/bin/env python3
"""Generate tests/golden/hd_paths.json -- HD derivation PATHS -- by IMPORTING the reference.

Runs only in the build container (needs the reference tree, read-only).  Nothing of the reference is copied: this
script folds ExtendedPrivateKey.private_child / ExtendedPublicKey.public_child (keys.py:191-215 / 276-296 of the
reference) over deterministic paths and records digests and samples of the serialisations they produce.  About 4500
steps at ~4 ms each: roughly 20 s.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_hd_paths.py
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

from bls_py.keys import ExtendedPrivateKey  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hd_paths.json")
SEEDS = [hashlib.sha256(b"blsgpu hd paths seed 0").digest(), hashlib.sha256(b"blsgpu hd paths seed 1").digest()[:19]]
PATHS = 256
MAX_DEPTH = 6
GRID = 32
H = 2**31


def private_paths(rnd):
    """PATHS paths of depth 1 .. MAX_DEPTH: an all-hardened and an all-non-hardened one at each depth, the rest mixed"""
    paths = []
    for d in range(1, MAX_DEPTH + 1):
        paths.append([H + rnd.randrange(H) for _ in range(d)])
        paths.append([rnd.randrange(H) for _ in range(d)])
    edge = [0, 1, H - 1, H, H + 1, 2**32 - 1]
    while len(paths) < PATHS:
        d = 1 + len(paths) % MAX_DEPTH
        paths.append([rnd.choice(edge) if rnd.random() < 0.2 else rnd.randrange(2**32) for _ in range(d)])
    rnd.shuffle(paths)
    return paths


def public_paths(rnd):
    edge = [0, 1, H - 1]
    return [[rnd.choice(edge) if rnd.random() < 0.2 else rnd.randrange(H) for _ in range(1 + k % MAX_DEPTH)] for k in range(PATHS)]


def fold(key, path, step):
    for i in path:
        key = getattr(key, step)(i)
    return key


def digest(sers, every=16):
    return {"count": len(sers), "sha256": hashlib.sha256(b"".join(sers)).hexdigest(),
            "every16": {str(k): sers[k].hex() for k in range(0, len(sers), every)}}


def main():
    rnd = random.Random(20240601)
    private = []
    for seed in SEEDS:
        esk = ExtendedPrivateKey.from_seed(seed)
        paths = private_paths(rnd)
        leaves = [fold(esk, p, "private_child") for p in paths]
        private.append({"seed": seed.hex(), "paths": paths, "esk": digest([k.serialize() for k in leaves]),
                        "epk": digest([k.get_extended_public_key().serialize() for k in leaves])})

    xpub = ExtendedPrivateKey.from_seed(SEEDS[0]).private_child(H + 9).get_extended_public_key()
    paths = public_paths(rnd)
    public = {"xpub": xpub.serialize().hex(), "paths": paths,
              "epk": digest([fold(xpub, p, "public_child").serialize() for p in paths])}

    root = ExtendedPrivateKey.from_seed(SEEDS[1]).private_child(H + 3).private_child(7).get_extended_public_key()
    accounts = [root.public_child(a) for a in range(GRID)]
    grid = {"xpub": root.serialize().hex(), "accounts": GRID, "addresses": GRID,
            "parents": digest([a.serialize() for a in accounts]),
            "epk": digest([a.public_child(i).serialize() for a in accounts for i in range(GRID)])}

    with open(OUT, "w") as f:
        json.dump({"private": private, "public": public, "grid": grid}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
