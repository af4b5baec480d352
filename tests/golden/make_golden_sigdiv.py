#!/usr/bin/env python3
"""Generate tests/golden/sigdiv.json -- Signature.divide_by on nested and securely merged aggregates -- by IMPORTING the
reference.

Runs only in the build container (needs the reference tree, read-only).  Nothing of the reference is copied: this script
calls PrivateKey.sign, BLS.aggregate_sigs, Signature.divide_by (signature.py:44-103) and BLS.verify on the keys and
messages of the reference's own test (tests.py:150-198) and records what they return.  About a minute (the pairings).

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_golden_sigdiv.py

Contents: a list of cases {name, dividend, divisors, result | error, verify}.  A signature is {sig: the 96 serialised bytes,
tree: [[message hash, 48-byte public key, exponent] ...]} in hex, in the order of the info's sorted lists; `result` is the
quotient in the same form, `error` the text of the exception divide_by raised instead, `verify` what BLS.verify says of the
quotient (null where the quotient has an empty tree).
  nested_three_leaves    sig_final / [sig2, sig5, sig6] of tests.py:174 (sig5's quotient is a hash_pks exponent);
  empty_divisor_list     that quotient / [];
  not_a_subset           that quotient / [sig6]: the error of tests.py:180;
  nested_one_leaf        sig_final / [sig1] (tests.py:184);
  not_unique             sig_final / [sig_L]: the error of tests.py:186;
  by_aggregate           sig_final2 / [sig_R2] (tests.py:196);
  secure_one_leaf        sig_R = aggregate(sig3, sig4, sig5), merged securely on the shared message, / [sig3]: quotient != 1;
  secure_two_leaves      sig_R / [sig3, sig5]: two quotients that differ;
  all_parts              sig_L / [sig1, sig2]: the quotient is infinity with an empty tree.
"""
import json
import logging
import os
import sys

logging.disable(logging.CRITICAL)
sys.dont_write_bytecode = True
REF = os.environ.get("BLS_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from bls_py.bls import BLS  # noqa: E402
from bls_py.keys import PrivateKey  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sigdiv.json")


def record(sig):
    info = sig.aggregation_info
    return {"sig": sig.serialize().hex(),
            "tree": [[mh.hex(), pk.serialize().hex(), "%064x" % int(info.tree[(mh, pk)])]
                     for mh, pk in zip(info.message_hashes, info.public_keys)]}


def case(name, dividend, divisors):
    c = {"name": name, "dividend": record(dividend), "divisors": [record(d) for d in divisors]}
    try:
        q = dividend.divide_by(divisors)
    except Exception as e:
        c["error"] = str(e)
        return c, None
    c["result"] = record(q)
    c["verify"] = bool(BLS.verify(q)) if q.aggregation_info.tree else None
    return c, q


def main():
    m1, m2, m3, m4 = bytes([1, 2, 3, 40]), bytes([5, 6, 70, 201]), bytes([9, 10, 11, 12, 13]), bytes([15, 63, 244, 92, 0, 1])
    sk1 = PrivateKey.from_seed(bytes([1, 2, 3, 4, 5]))
    sk2 = PrivateKey.from_seed(bytes([1, 2, 3, 4, 5, 6]))
    sig1, sig2, sig3, sig4, sig5, sig6 = sk1.sign(m1), sk2.sign(m2), sk2.sign(m1), sk1.sign(m3), sk1.sign(m1), sk1.sign(m4)
    sig_L = BLS.aggregate_sigs([sig1, sig2])
    sig_R = BLS.aggregate_sigs([sig3, sig4, sig5])
    sig_final = BLS.aggregate_sigs([sig_L, sig_R, sig6])
    sig_R2 = BLS.aggregate_sigs([sk2.sign(m3), sk2.sign(m4)])
    sig_final2 = BLS.aggregate_sigs([sig_final, sig_R2])

    cases = []
    c, quotient = case("nested_three_leaves", sig_final, [sig2, sig5, sig6])
    assert quotient.serialize().hex().startswith("8ebc8a73a2291e68") and c["verify"]          # tests.py:177
    cases.append(c)
    for name, dividend, divisors in (("empty_divisor_list", quotient, []), ("not_a_subset", quotient, [sig6]),
                                     ("nested_one_leaf", sig_final, [sig1]), ("not_unique", sig_final, [sig_L]),
                                     ("by_aggregate", sig_final2, [sig_R2]), ("secure_one_leaf", sig_R, [sig3]),
                                     ("secure_two_leaves", sig_R, [sig3, sig5]), ("all_parts", sig_L, [sig1, sig2])):
        cases.append(case(name, dividend, divisors)[0])
    by = {c["name"]: c for c in cases}
    assert by["not_a_subset"]["error"] == "Signature is not a subset" and "not unique" in by["not_unique"]["error"]
    assert by["by_aggregate"]["result"]["sig"].startswith("06af6930bd06838f")                 # tests.py:198
    assert by["all_parts"]["result"]["tree"] == []
    with open(OUT, "w") as f:
        json.dump(cases, f, indent=0)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
