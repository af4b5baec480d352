"""k_ml_lines2 (one pair per lane pair) at call sizes that leave the last wavefront partly filled: its spare lanes repeat
the last pair, so a record written past pair n - 1 would land on line L + 1 of pair 0.  Forced onto lane pairs for every
size (BLSGPU_LS_WIDE_MAX=0, BLSGPU_LS_QUAD_MAX=0, set_ls_threshold(1, 1)) and compared with the CPU oracle.  Needs an
MI355X."""
import pytest

from conftest import engine_with_env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pairs_engine():
    e = engine_with_env({"BLSGPU_LS_WIDE_MAX": "0", "BLSGPU_LS_QUAD_MAX": "0"})
    e.set_ls_threshold(1, 1)
    return e


def mixed(seeded_pairs, n):
    """n pairs from the 1025 seeded points: pair i = (P[i mod 1025], Q[(i + i // 1025) mod 1025]), so no two calls'
    neighbouring records repeat"""
    g1, g2 = seeded_pairs
    a = b"".join(g1[96 * (i % 1025):96 * (i % 1025 + 1)] for i in range(n))
    b = b"".join(g2[192 * ((i + i // 1025) % 1025):192 * ((i + i // 1025) % 1025 + 1)] for i in range(n))
    return a, b


@pytest.mark.parametrize("n", [33, 63, 2305, 20481])
def test_partial_last_wavefront(pairs_engine, seeded_pairs, oracle, n):
    a, b = mixed(seeded_pairs, n)
    assert pairs_engine.pairing_multi(a, b, n) == oracle.pairing_multi(a, b, n, threads=8)


def test_degenerate_pair_in_last_wavefront(pairs_engine, seeded_pairs, golden, oracle):
    """a reference-generated degenerate case appended after 33 ordinary pairs: its pairs sit in the second, partly
    filled wavefront, are flagged there and rewritten by k_ml_lines_exact"""
    for name in ("ord13_in_team", ):
        v = golden("pairing_degenerate.json")["cases"][name]
        k = len(v["g1"])
        a, b = mixed(seeded_pairs, 33)
        a += b"".join(bytes.fromhex(x) for x in v["g1"])
        b += b"".join(bytes.fromhex(x) for x in v["g2"])
        inf = bytes(66) + bytes(int(f) for pr in v["inf"] for f in pr)
        n = 33 + k
        assert pairs_engine.pairing_multi(a, b, n, inf) == oracle.pairing_multi(a, b, n, threads=8, inf=inf), name


def test_batch_ending_mid_wavefront(pairs_engine, seeded_pairs, oracle):
    """3 groups of 35 pairs: 105 pairs, 210 lanes -- the last wavefront holds 18 of them"""
    gsz, groups = 35, 3
    a, b = mixed(seeded_pairs, gsz * groups)
    out = pairs_engine.pairing_multi_batch(a, b, gsz, groups)
    for g in range(groups):
        want = oracle.pairing_multi(a[96 * gsz * g:96 * gsz * (g + 1)], b[192 * gsz * g:192 * gsz * (g + 1)], gsz, threads=8)
        assert out[576 * g:576 * (g + 1)] == want, g
