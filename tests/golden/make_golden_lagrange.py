#!/usr/bin/env python3
"""Generate tests/golden/lagrange.json -- Lagrange coefficients, interpolations and threshold combines -- by IMPORTING the
reference.

Runs only in the build container (needs the reference tree, read-only).  Nothing of the reference is copied: this script
calls Threshold.lagrange_coeffs_at_zero / interpolate_at_zero / aggregate_unit_sigs (threshold.py:56-101, 127-136) and
PrivateKey.sign (keys.py:123-126) on seeded inputs and records what they return.  A few seconds.

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_lagrange.py

Contents:
  groups    seeded groups of players X with the reference's coefficients and interpolate_at_zero(X, Y) for the values
            Y = [random.Random(y_seed).randrange(n) for _ in X] (kept as their seed: the file stays small), for
            k in {1, 2, 3, 5, 63, 64, 65, 67, 128, 200} and players that are small (a shuffled subset of 1..100, or of
            1..k+33 where k > 100), up to 2^32 - 1, near 2^200, and n - 1, n - 2 among others (a few kinds per k: the file
            stays near 100 KB);
  combine   a seeded 3-of-5 sharing: the secret polynomial, the five shares, the message, and for all ten 3-subsets the
            players, their unit signatures (share_i * H(m), 192-byte affine) and the serialised aggregate_unit_sigs;
  asserts   groups on which lagrange_coeffs_at_zero asserts (a duplicate, a zero, x = n) with what the reference did.
"""
import itertools
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
from bls_py.fields import Fq  # noqa: E402
from bls_py.keys import PrivateKey  # noqa: E402
from bls_py.threshold import Threshold  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lagrange.json")
N_ORDER = default_ec.n
KS = [1, 2, 3, 5, 63, 64, 65, 67, 128, 200]
# kinds per k (the long groups are the expensive lines of the file)
KINDS = {1: "small u32 2^200 top", 2: "small u32 2^200 top", 3: "small u32 2^200 top", 5: "small u32 2^200 top mixed",
         63: "small", 64: "u32", 65: "2^200", 67: "small u32 top mixed", 128: "small", 200: "small 2^200"}


def players(kind, k, rng):
    if kind == "small":
        return rng.sample(range(1, max(100, k + 33) + 1), k)
    if kind == "u32":
        X = set()
        while len(X) < k - 1:
            X.add(rng.randrange(1, 2**32))
        return rng.sample(sorted(X | {2**32 - 1}), k)
    if kind == "2^200":
        return rng.sample([2**200 + d for d in range(-k, k + 1)], k)
    if kind == "top":                                   # n - 1, n - 2 and their neighbours
        return rng.sample([N_ORDER - 1 - d for d in range(k)], k)
    X = [N_ORDER - 1, N_ORDER - 2, 1, 2**32 - 1, 2**200][:k]
    seen = set(X)
    while len(X) < k:
        x = rng.randrange(1, N_ORDER)
        if x not in seen:
            seen.add(x)
            X.append(x)
    rng.shuffle(X)
    return X


def aff_hex(J):
    A = J.to_affine()
    if A.infinity:
        return bytes(192).hex()
    return b"".join(int(c).to_bytes(48, "big") for c in (A.x[0], A.x[1], A.y[0], A.y[1])).hex()


def main():
    groups = []
    for k in KS:
        for kind in KINDS[k].split():
            rng = random.Random("%s-%d" % (kind, k))
            X = players(kind, k, rng)
            assert len(X) == k
            y_seed = "Y-%s-%d" % (kind, k)
            yr = random.Random(y_seed)
            Y = [yr.randrange(N_ORDER) for _ in range(k)]
            L = Threshold.lagrange_coeffs_at_zero(X)
            v = Threshold.interpolate_at_zero(X, [Fq(N_ORDER, y) for y in Y])
            groups.append({"k": k, "kind": kind, "X": ["%x" % x for x in X], "y_seed": y_seed, "y0": "%064x" % Y[0],
                           "coeffs": ["%064x" % int(l) for l in L], "interpolate": "%064x" % int(v)})
    # a 3-of-5 sharing: shares P(1..5), unit signatures share_i * H(m), every 3-subset combined
    rng = random.Random(35)
    poly = [rng.randrange(1, N_ORDER) for _ in range(3)]
    shares = [sum(c * pow(x, e, N_ORDER) for e, c in enumerate(poly)) % N_ORDER for x in range(1, 6)]
    msg = b"lagrange fixture 3-of-5"
    unit = [PrivateKey(s).sign(msg) for s in shares]
    master = PrivateKey(poly[0]).sign(msg)
    subsets = []
    for sub in itertools.combinations(range(1, 6), 3):
        order = list(sub)
        rng.shuffle(order)
        agg = Threshold.aggregate_unit_sigs([unit[p - 1] for p in order], order, 3)
        assert agg.serialize() == master.serialize()
        subsets.append({"players": order, "aggregate": agg.serialize().hex()})
    combine = {"poly": ["%064x" % c for c in poly], "shares": ["%064x" % s for s in shares], "msg": msg.hex(),
               "unit_sigs": [aff_hex(u.value) for u in unit], "unit_sigs_ser": [u.serialize().hex() for u in unit],
               "master": master.serialize().hex(), "subsets": subsets}
    asserts = []
    for what, X in (("duplicate", [3, 7, 3]), ("zero", [0, 4, 9]), ("x = n", [1, N_ORDER, 2]), ("x = n + 1", [1, N_ORDER + 1, 2]),
                    ("duplicate of n - 1", [N_ORDER - 1, 5, N_ORDER - 1]), ("zero alone", [0])):
        try:
            Threshold.lagrange_coeffs_at_zero(X)
            raised = False
        except AssertionError:
            raised = True
        asserts.append({"what": what, "X": ["%x" % x for x in X], "raises": raised})
    assert all(a["raises"] for a in asserts)
    with open(OUT, "w") as f:
        json.dump({"groups": groups, "combine": combine, "asserts": asserts}, f, indent=0)
    print("wrote", OUT, os.path.getsize(OUT), "bytes", len(groups), "groups")


if __name__ == "__main__":
    main()
