#!/usr/bin/env python3
"""Generate tests/golden/hd.json -- HD key vectors -- by IMPORTING the reference.

Runs only in the build container (needs the reference tree, read-only).  Nothing of the reference is copied: this
script calls ExtendedPrivateKey / ExtendedPublicKey (keys.py:167-316 of the reference) on deterministic seeds and
records the serialisations they produce.  About 3000 children at ~4 ms each: roughly 15 s.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_hd.py
"""
import hashlib
import json
import logging
import os
import sys

logging.disable(logging.CRITICAL)
sys.dont_write_bytecode = True
REF = os.environ.get("BLS_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from bls_py.keys import ExtendedPrivateKey, ExtendedPublicKey  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hd.json")
INDICES = [0, 1, 77, 2**31 - 1, 2**31, 2**31 + 77, 2**32 - 1]
CHAINS = [[0, 5], [3, 17], [2**31 + 1, 7], [7, 2**31 + 2], [2**31 - 1, 2**32 - 1]]
SEEDS = [
    bytes([1, 50, 6, 244, 24, 199, 1, 25]),                                         # tests.py:202
    bytes([1, 50, 6, 244, 24, 199, 1, 25, 52, 88, 192, 19, 18, 12, 89, 6, 220, 18, 102, 58, 209,
           82, 12, 62, 89, 110, 182, 9, 44, 20, 254, 22]),                          # tests.py:293
    b"",
    hashlib.sha256(b"blsgpu hd seed 0").digest(),
    hashlib.sha256(b"blsgpu hd seed 1").digest()[:17],
]
XPUB_COUNT = 2048
XPRV_COUNT = 512


def xprv_index(k):
    """hardened and non-hardened indices interleaved"""
    return k // 2 + (2**31 if k & 1 else 0)


def main():
    seeds = []
    for seed in SEEDS:
        esk = ExtendedPrivateKey.from_seed(seed)
        epk = esk.get_extended_public_key()
        rec = {"seed": seed.hex(), "esk": esk.serialize().hex(), "epk": epk.serialize().hex(),
               "fingerprint": esk.get_public_key().get_fingerprint(), "chain_code": esk.chain_code.hex(), "children": [], "chains": []}
        for i in INDICES:
            c = esk.private_child(i)
            rec["children"].append({"i": i, "esk": c.serialize().hex(), "epk": c.get_extended_public_key().serialize().hex(),
                                    "fingerprint": c.get_public_key().get_fingerprint(),
                                    "pub": epk.public_child(i).serialize().hex() if i < 2**31 else None})
        for path in CHAINS:
            c, p = esk, epk if all(i < 2**31 for i in path) else None
            for i in path:
                c = c.private_child(i)
                p = p.public_child(i) if p is not None else None
            rec["chains"].append({"path": path, "esk": c.serialize().hex(), "epk": c.get_extended_public_key().serialize().hex(),
                                  "pub": p.serialize().hex() if p is not None else None})
        seeds.append(rec)

    xpub = ExtendedPrivateKey.from_seed(SEEDS[3]).private_child(2**31 + 44).get_extended_public_key()
    kids = [xpub.public_child(i).serialize() for i in range(XPUB_COUNT)]
    xpub_rec = {"xpub": xpub.serialize().hex(), "count": XPUB_COUNT, "sha256": hashlib.sha256(b"".join(kids)).hexdigest(),
                "every64": {str(i): kids[i].hex() for i in range(0, XPUB_COUNT, 64)}}

    xprv = ExtendedPrivateKey.from_seed(SEEDS[1])
    kids = [xprv.private_child(xprv_index(k)).serialize() for k in range(XPRV_COUNT)]
    xprv_rec = {"seed": SEEDS[1].hex(), "count": XPRV_COUNT, "indices": "k // 2 + 2^31 (k odd)",
                "sha256": hashlib.sha256(b"".join(kids)).hexdigest(), "every32": {str(k): kids[k].hex() for k in range(0, XPRV_COUNT, 32)}}

    with open(OUT, "w") as f:
        json.dump({"seeds": seeds, "xpub_range": xpub_rec, "xprv_range": xprv_rec}, f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
