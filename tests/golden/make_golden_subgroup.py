#!/usr/bin/env python3
"""Generate tests/golden/subgroup.json -- order-n subgroup membership vectors for G1 and G2 -- by IMPORTING the reference.

Runs only in the build container (needs the reference tree, read-only).  Nothing of the reference is copied: this script
builds points with the reference's own curve code (generator multiples, y_for_x on seeded random x without clearing the
cofactor, their pure-torsion parts [n] P, sums P + T) and records, for each, the reference's verdict (P * n).infinity and
whether the point is on the curve.  About a minute (the reference's field arithmetic is pure Python).

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_subgroup.py

Points are affine, big-endian: G1 x || y (96 bytes), G2 x.c0 x.c1 y.c0 y.c1 (192 bytes), all zero = infinity.  Each
record: {"kind", "point", "on_curve", "in_subgroup"}.
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

from bls_py.ec import (AffinePoint, default_ec, default_ec_twist, generator_Fq, generator_Fq2,  # noqa: E402
                       y_for_x)
from bls_py.fields import Fq, Fq2  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "subgroup.json")
Q, N = default_ec.q, default_ec.n


def enc(P):
    if P.infinity:
        return "00" * (96 if P.FE is Fq else 192)
    if P.FE is Fq:
        cs = [P.x.Z, P.y.Z]
    else:
        cs = [P.x[0].Z, P.x[1].Z, P.y[0].Z, P.y[1].Z]
    return "".join((int(c) % Q).to_bytes(48, "big").hex() for c in cs)


def rec(kind, P):
    """the record of P, or None where the reference's multiplication raises: its Jacobian addition of a point to
    itself calls the doubling with one argument too many (fields_t.py:781), which [n] P of a point of small order reaches"""
    try:
        inside = bool((P * N).infinity)
    except TypeError:
        return None
    return {"kind": kind, "point": enc(P), "on_curve": bool(P.infinity or P.is_on_curve()), "in_subgroup": inside}


def random_point(rng, ec, FE):
    """y_for_x of a random x, no cofactor clearing"""
    while True:
        x = Fq(Q, rng.randrange(Q)) if FE is Fq else Fq2(Q, rng.randrange(Q), rng.randrange(Q))
        try:
            y = y_for_x(x, ec, FE)[rng.randrange(2)]
        except ValueError:
            continue
        return AffinePoint(x, y, False, ec)


def group(rng, gen, ec, FE, extra):
    out = [rec("generator", gen)]
    sub = [gen * rng.randrange(1, N) for _ in range(4)]
    out += [rec("subgroup", P) for P in sub]
    anyp = [random_point(rng, ec, FE) for _ in range(6)]
    out += [rec("random", P) for P in anyp]
    tors = [P * N for P in anyp[:4]]                                       # (no doubling inside an addition here)
    out += [rec("torsion", T) for T in tors]
    out += [rec("mixed", sub[j] + tors[j]) for j in range(4)]
    out += [rec("negated", P.negate()) for P in (sub[0], anyp[0])]
    out.append(rec("infinity", AffinePoint(FE.zero(Q), FE.zero(Q), True, ec)))
    out += extra
    # off the curve: a subgroup point with y + 1, a random point with x + 1
    for P in (sub[1], anyp[1]):
        one = FE.one(Q)
        out.append(rec("off_curve", AffinePoint(P.x, P.y + one, False, ec)))
        out.append(rec("off_curve", AffinePoint(P.x + one, P.y, False, ec)))
    return out


def main():
    rng = random.Random(20261016)
    two = Fq(Q, 2)
    g1_extra = [rec("order3", AffinePoint(Fq(Q, 0), two, False, default_ec)),       # (0, +-2): order 3 (b = 4)
                rec("order3", AffinePoint(Fq(Q, 0), -two, False, default_ec))]
    g1 = group(rng, generator_Fq(default_ec), default_ec, Fq, g1_extra)
    g2 = group(rng, generator_Fq2(default_ec_twist), default_ec_twist, Fq2, [])
    with open(OUT, "w") as f:
        json.dump({"g1": [r for r in g1 if r], "g2": [r for r in g2 if r]}, f, indent=1)
    print("wrote", OUT, sum(1 for r in g1 if r), sum(1 for r in g2 if r))


if __name__ == "__main__":
    main()
