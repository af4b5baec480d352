"""The integer model of the scalar-independent G2 multiplication (vmgen/g2smul_model.py, the specification of
csrc/blsgpu_g2smul.hip): the signed recoding, the value of the window schedule against the host's double-and-add, and
the uniformity of its trace -- the same operations on the same table entries for every scalar."""
import json
import os
import random

import pytest

from bls_py import hostmath as H
from bls_py.util import hash256, hash512
from vmgen import g2smul_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = H.N


def scalars():
    rng = random.Random(0x62736d)
    fixed = [0, 1, 7, 8, 9, 15, 16, N - 1, N, N + 1, 1 << 255, (1 << 256) - 1,
             int("88" * 32, 16), int("77" * 32, 16), int("f0" * 32, 16)]
    return fixed + [rng.randrange(1 << 256) for _ in range(200)]


SCALARS = scalars()


def twist_point_outside_subgroup():
    with open(os.path.join(GOLDEN, "subgroup.json")) as f:
        rec = next(r for r in json.load(f)["g2"] if r["on_curve"] and not r["in_subgroup"] and any(bytes.fromhex(r["point"])))
    return H.g2_from_abi(bytes.fromhex(rec["point"]))


@pytest.fixture(scope="module")
def runs():
    """{point name: [(value, trace) per scalar]}: the hashed point with a table per scalar, the twist point outside the
    subgroup with one shared table, infinity both ways (its arithmetic is free)"""
    hashed = H.hash_to_g2_prehashed(hash256(b"g2smul model"), hash512)
    twist = twist_point_outside_subgroup()
    assert H.on_curve(H.F2, twist) and H.jac_mul(H.F2, H.aff_to_jac(H.F2, twist), N) is not None
    shared, _ = M.build_table(twist)
    shared_inf, _ = M.build_table(None)
    return {"points": {"hashed": hashed, "twist": twist, "infinity": None},
            "hashed": [M.smul(hashed, s) for s in SCALARS],
            "twist": [M.smul(twist, s, table=shared) for s in SCALARS],
            "infinity": [M.smul(None, s) for s in SCALARS],
            "infinity_shared": [M.smul(None, s, table=shared_inf) for s in SCALARS]}


def test_recoding():
    assert M.BIAS == int("8" * 65, 16) and len(SCALARS) == 215
    for s in SCALARS:
        d = M.recode(s)
        assert len(d) == M.WINDOWS == 65
        assert all(-8 <= x < 8 for x in d)
        assert sum(x << (4 * w) for w, x in enumerate(d)) == s
    with pytest.raises(ValueError):
        M.recode(1 << 256)
    with pytest.raises(ValueError):
        M.recode(-1)


@pytest.mark.parametrize("name", ["hashed", "twist", "infinity"])
def test_model_value(runs, name):
    P = runs["points"][name]
    J = H.aff_to_jac(H.F2, P)
    for s, (got, _) in zip(SCALARS, runs[name]):
        assert got == H.jac_to_affine(H.F2, H.jac_mul(H.F2, J, s)), hex(s)
    if name == "infinity":
        assert all(got is None for got, _ in runs["infinity_shared"])


def test_no_reduction_mod_n(runs):
    """the twist point has an order that does not divide n: n P is a point, and (n + 1) P is not P"""
    by_scalar = dict(zip(SCALARS, (v for v, _ in runs["twist"])))
    assert by_scalar[N] is not None and by_scalar[N + 1] != runs["points"]["twist"]
    hashed = dict(zip(SCALARS, (v for v, _ in runs["hashed"])))
    assert hashed[N] is None and hashed[N + 1] == runs["points"]["hashed"] and hashed[0] is None


def test_trace_is_the_same_for_every_scalar(runs):
    own = [t for _, t in runs["hashed"]] + [t for _, t in runs["infinity"]]
    shared = [t for _, t in runs["twist"]] + [t for _, t in runs["infinity_shared"]]
    assert all(t == own[0] for t in own)
    assert all(t == shared[0] for t in shared)
    # a table per scalar: the table steps, then the shared schedule
    head = own[0][:len(own[0]) - len(shared[0])]
    assert own[0][len(head):] == shared[0]
    assert head == [("load", (), 0)] + [("table_add", (e - 1, 0), e) for e in range(1, 8)]
    # 65 windows of four doublings, a read of all eight entries and one addition
    window = [("dbl", (), None)] * 4 + [("select", tuple(range(8)), None), ("add", (), None)]
    assert shared[0] == window * 65
    assert sum(op == "dbl" for op, _, _ in own[0]) == 260 and sum(op == "add" for op, _, _ in own[0]) == 65
