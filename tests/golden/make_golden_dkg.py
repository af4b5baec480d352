#!/usr/bin/env python3
"""Generate tests/golden/dkg.json -- Joint-Feldman dealing and share-check vectors -- by IMPORTING the reference.

Runs only in the build container (needs the reference tree, read-only).  Nothing of the reference is copied: this
script patches the reference's keys.RNG with a seeded random.Random, calls PrivateKey.new_threshold (keys.py:95-117) and
Threshold.verify_secret_fragment (threshold.py:104-125), and records what they return.  A few seconds.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_dkg.py

Contents:
  dealings  for each (T, N): the seed, then N dealers in turn (N new_threshold calls on one seeded RNG): coefficients,
            commitments (96-byte affine, x || y big-endian), fragments P(1..N), and verify[j] for player j + 1;
  checks    single verify_secret_fragment calls (T, commitments, fragment, player -> expect): tampered fragments,
            players and commitments, players n, n + 1, -1 and 2^255 - 1, and a polynomial with a commitment outside the
            order-n subgroup (C_2 = 11 G1 + (0, 2), the second point of order 3) where x^k and x^k mod n differ.
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

from bls_py import keys  # noqa: E402
from bls_py.ec import AffinePoint, default_ec, generator_Fq  # noqa: E402
from bls_py.fields import Fq  # noqa: E402
from bls_py.keys import PrivateKey  # noqa: E402
from bls_py.threshold import Threshold  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dkg.json")
N_ORDER = default_ec.n
Q = default_ec.q
SHAPES = [(1, 1), (2, 3), (3, 5), (5, 7)]


class Recorder:
    """keys.RNG stand-in: a seeded random.Random whose randint draws are kept (the coefficients new_threshold makes)"""

    def __init__(self, seed):
        self.rng, self.drawn = random.Random(seed), []

    def randint(self, a, b):
        v = self.rng.randint(a, b)
        self.drawn.append(v)
        return v


def aff_hex(p):
    if p.infinity:
        return bytes(96).hex()
    return (p.x.Z.to_bytes(48, "big") + p.y.Z.to_bytes(48, "big")).hex()


def infinity():
    return AffinePoint(Fq(Q, 0), Fq(Q, 0), True, default_ec)


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % N_ORDER
    return acc


def check(out, what, T, C, frag, player):
    out.append({"what": what, "T": T, "commitments": [aff_hex(p) for p in C], "fragment": "%064x" % int(frag),
                "player": player, "expect": bool(Threshold.verify_secret_fragment(T, frag, player, C))})


def main():
    dealings, checks = [], []
    for T, N in SHAPES:
        seed = 1000 * T + N
        rec = Recorder(seed)
        keys.RNG = rec
        dealers = []
        for d in range(N):
            before = len(rec.drawn)
            sk, C, frags = PrivateKey.new_threshold(T, N)
            coeffs = rec.drawn[before:]
            assert sk.value == coeffs[0] and len(coeffs) == T
            dealers.append({"coefficients": ["%064x" % c for c in coeffs], "commitments": [aff_hex(p) for p in C],
                            "fragments": ["%064x" % int(f) for f in frags],
                            "verify": [bool(Threshold.verify_secret_fragment(T, frags[j], j + 1, C)) for j in range(N)],
                            "_C": C, "_f": frags, "_c": coeffs})
        dealings.append({"T": T, "N": N, "seed": seed, "dealers": dealers})
        if T < 3:
            continue
        for d, dl in enumerate(dealers[:2]):
            C, frags, coeffs = dl["_C"], dl["_f"], dl["_c"]
            other = dealers[(d + 1) % N]["_C"]
            check(checks, "fragment + 1", T, C, frags[1] + 1, 2)
            check(checks, "wrong player", T, C, frags[1], 3)
            check(checks, "another dealer's commitments", T, other, frags[1], 2)
            for k in (0, 1, T - 1):
                neg = list(C)
                neg[k] = C[k].negate()
                check(checks, "C_%d negated" % k, T, neg, frags[2], 3)
                inf = list(C)
                inf[k] = infinity()
                check(checks, "C_%d infinity" % k, T, inf, frags[2], 3)
            for p in (N_ORDER, N_ORDER + 1, -1, 2**255 - 1):
                f = horner(coeffs, p)
                check(checks, "player %d" % p, T, C, Fq(N_ORDER, f), p)
                check(checks, "player %d, fragment + 1" % p, T, C, Fq(N_ORDER, f + 1), p)
    # C_2 outside the order-n subgroup: 11 G1 + (0, 2) (order 3 n); an honest fragment of c0 + c1 x + 11 x^2
    g1 = generator_Fq()
    rng = random.Random(3)
    c0, c1 = rng.randint(1, N_ORDER - 1), rng.randint(1, N_ORDER - 1)
    C = [g1 * c0, g1 * c1, g1 * 11 + AffinePoint(Fq(Q, 0), Fq(Q, 2), False, default_ec)]
    for x in (3, 3 << 199, 3 << 200, 4):
        check(checks, "order-3 C_2, player %d" % x, 3, C, Fq(N_ORDER, horner([c0, c1, 11], x)), x)
    for dl in dealings:
        for d in dl["dealers"]:
            for k in ("_C", "_f", "_c"):
                del d[k]
    with open(OUT, "w") as f:
        json.dump({"dealings": dealings, "checks": checks}, f, indent=1)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
