#!/usr/bin/env python3
"""Generate tests/golden/hash_to_g1.json -- hash-to-G1 vectors -- by IMPORTING the reference.

Runs only in the build container (needs the reference tree, read-only).  Nothing of the reference is copied: this script
calls the reference's sw_encode, hash_to_point_prehashed_Fq, point addition and multiplication and records what they
return.  About half a minute (the reference's curve arithmetic is pure Python).

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_h2g1.py

Field elements are 48 bytes big-endian, points affine x || y (96 bytes, all zero = infinity), "ser" the 48 bytes of
AffinePoint.serialize() (48 zero bytes for infinity).  Three sections:
  sw_encode  {"t", "point", "inf", "index"}: the reference's sw_encode(t); index = which of x1, x2, x3 it took (ec.py:500),
             None where it takes none (t = 0: infinity; t^2 = -5: the generator)
  map        {"kind", "t0", "t1", "point", "ser", "inf"}: h (sw_encode(t0) + sw_encode(t1)), the reference's
             hash_to_point_prehashed_Fq from its two field elements on.  Where one encoding is infinity the sum is the other
             one: the reference's own `+` cannot add its infinity (a JacobianPoint) to an AffinePoint.
  hash       {"msg_hash", "point", "ser"}: hash_to_point_prehashed_Fq(msg_hash) of 32-byte hashes; the first is hash256(b"")
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

from bls_py.ec import AffinePoint, default_ec, generator_Fq, hash_to_point_prehashed_Fq, sw_encode, y_for_x  # noqa: E402
from bls_py.fields import Fq  # noqa: E402
from bls_py.util import hash256  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "hash_to_g1.json")
ec = default_ec
Q = ec.q
INF = AffinePoint(Fq.zero(Q), Fq.zero(Q), True, ec)


def fe(v):
    return (int(v) % Q).to_bytes(48, "big").hex()


def enc(P):
    return "00" * 96 if P.infinity else fe(P.x.Z) + fe(P.y.Z)


def ser(P):
    return "00" * 48 if P.infinity else P.serialize().hex()


def encode(t):
    """the reference's sw_encode(t) as an AffinePoint (its infinity is a JacobianPoint)"""
    P = sw_encode(Fq(Q, t), ec, Fq)
    return INF if P.infinity else P


def index_taken(t, P):
    """which candidate of ec.py:477-503 the point's x is; None for the cases before them"""
    t = Fq(Q, t)
    if t == 0 or t * t + ec.b + 1 == 0:
        return None
    w = ~(t * t + ec.b + 1) * ec.sqrt_n3 * t
    x1 = -w * t + ec.sqrt_n3m1o2
    xs = [x1, Fq(Q, -1) - x1, ~(w * w) + 1]

    def valid(x):
        try:
            y_for_x(x, ec, Fq)
            return 1
        except Exception:
            return -1
    idx = ((valid(xs[0]) - 1) * valid(xs[1])) % 3
    assert xs[idx] == P.x
    return idx


def mapped(t0, t1):
    A, B = encode(t0), encode(t1)
    S = B if A.infinity else (A if B.infinity else A + B)
    return INF if S.infinity else S * ec.h


def main():
    rng = random.Random(20261020)
    r5 = Fq(Q, -5).modsqrt().Z
    assert r5 * r5 % Q == Q - 5                              # -5 is a square mod q: w = 0 is reachable
    roots = [r5, Q - r5]
    edge_t = [0, 1, 2, Q - 1, Q - 2] + roots
    sw, taken = [], [0, 0, 0]

    def add_sw(t):
        P = encode(t)
        idx = index_taken(t, P)
        if idx is not None:
            taken[idx] += 1
        sw.append({"t": fe(t), "point": enc(P), "inf": bool(P.infinity), "index": idx})
    for t in edge_t:
        add_sw(t)
    n_random = 0
    while n_random < 20 or min(taken) < 3:
        add_sw(rng.randrange(1, Q))
        n_random += 1
    assert min(taken) >= 3, taken
    g = generator_Fq(ec)
    assert sw[5]["point"] in (enc(g), enc(g.negate())) and sw[6]["point"] in (enc(g), enc(g.negate())) and sw[5]["point"] != sw[6]["point"]

    maps = []

    def add_map(kind, t0, t1):
        P = mapped(t0, t1)
        maps.append({"kind": kind, "t0": fe(t0), "t1": fe(t1), "point": enc(P), "ser": ser(P), "inf": bool(P.infinity)})
    for _ in range(32):
        add_map("random", rng.randrange(Q), rng.randrange(Q))
    sw_t = [int(r["t"], 16) for r in sw]
    for t in sw_t:
        add_map("t_zero", t, 0)
    t = rng.randrange(1, Q)
    add_map("zero_t", 0, t)
    add_map("zero_zero", 0, 0)
    add_map("opposite", t, Q - t)
    add_map("equal", t, t)
    add_map("root_t", r5, t)
    add_map("root_opposite", r5, Q - r5)
    assert [m["inf"] for m in maps if m["kind"] in ("zero_zero", "opposite", "root_opposite")] == [True] * 3

    hashes = []
    for k in range(70):
        h = hash256(b"") if k == 0 else bytes(rng.randrange(256) for _ in range(32))
        P = hash_to_point_prehashed_Fq(h, ec)
        hashes.append({"msg_hash": h.hex(), "point": enc(P), "ser": ser(P)})
    with open(os.path.join(HERE, "hash_to_curve.json")) as f:
        assert json.load(f)["hash_to_g1_empty"]["point"] == hashes[0]["point"]

    with open(OUT, "w") as f:
        json.dump({"sw_encode": sw, "map": maps, "hash": hashes}, f, indent=1)
    print("wrote", OUT, len(sw), len(maps), len(hashes), "indices taken", taken)


if __name__ == "__main__":
    main()
