"""The integer model of the scalar-independent fixed-base G1 multiplication (vmgen/g1fixs_model.py, the specification of
csrc/blsgpu_g1fix.hip k_fix_table_t<4> / k_fix_mul_secret): its table, the value of the window schedule against the
host's double-and-add and the reference's public keys (tests/golden/keygen.json), and the uniformity of its trace -- the
same operations on the same table entries for every scalar."""
import json
import os
import random

import pytest

from bls_py import hostmath as H
from vmgen import g1fixs_model as M
from vmgen import g2smul_model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = H.N


def scalars():
    """the scalar list of tests/test_g2smul_model.py"""
    rng = random.Random(0x62736d)
    fixed = [0, 1, 7, 8, 9, 15, 16, N - 1, N, N + 1, 1 << 255, (1 << 256) - 1,
             int("88" * 32, 16), int("77" * 32, 16), int("f0" * 32, 16)]
    return fixed + [rng.randrange(1 << 256) for _ in range(200)]


SCALARS = scalars()
G = H.aff_to_jac(H.F1, H.G1_GEN)


@pytest.fixture(scope="module")
def table():
    return M.build_table()


@pytest.fixture(scope="module")
def runs(table):
    return [M.mul_gen(s, table) for s in SCALARS]


def test_table(table):
    assert M.recode is g2smul_model.recode
    assert len(table) == M.WINDOWS == 65 and all(len(row) == M.TABLE == 8 for row in table)
    assert M.TABLE_BYTES == 58240
    for w in (0, 1, 31, 64):
        for e in (0, 3, 7):
            assert H.jac_to_affine(H.F1, table[w][e]) == H.jac_to_affine(H.F1, H.jac_mul(H.F1, G, ((e + 1) << (4 * w)) % N))
    # no entry is infinity: every one can be an affine addend
    assert all(H.jac_to_affine(H.F1, P) is not None for row in table for P in row)


def test_model_value(runs):
    assert len(SCALARS) == 215
    for s, (got, _) in zip(SCALARS, runs):
        assert got == H.jac_to_affine(H.F1, H.jac_mul(H.F1, G, s)), hex(s)
    by_scalar = dict(zip(SCALARS, (v for v, _ in runs)))
    assert by_scalar[0] is None and by_scalar[N] is None and by_scalar[N + 1] == H.G1_GEN and by_scalar[1] == H.G1_GEN


def test_trace_is_the_same_for_every_scalar(runs):
    traces = [t for _, t in runs]
    assert all(t == traces[0] for t in traces)
    want = []
    for w in range(65):
        want += [("select", tuple((w, e) for e in range(8))), ("madd", ()), ("keep", ())]
    assert traces[0] == want
    assert sum(op == "madd" for op, _ in traces[0]) == 65 and not any(op == "dbl" for op, _ in traces[0])


def test_reference_public_keys(table):
    with open(os.path.join(GOLDEN, "keygen.json")) as f:
        recs = json.load(f)["cases"]
    assert len(recs) == 40
    sks = [int(r["sk"], 16) for r in recs]
    assert {1, 2, 8, 9, 16, N - 1} <= set(sks) and all(0 < s < N for s in sks)
    for r, s in zip(recs, sks):
        A, _ = M.mul_gen(s, table)
        assert H.g1_affine_bytes(A).hex() == r["aff"], r["sk"]
        assert H.g1_compress(A).hex() == r["ser"], r["sk"]
