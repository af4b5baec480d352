"""k_ml_lines2 (one pair per lane PAIR, csrc/blsgpu_ml.hip namespace sp) at the smallest counts at which its lane-pair
helpers can go wrong, with the line-stream path forced for every size (blsgpu_ctx_set_ls_threshold) and the sixteen-lane
and lane-quad chains switched off, against the golden vectors and the CPU oracle -- never against the engine itself.
A wavefront holds 32 pairs, so the counts are 1, 2, 31, 32, 33 and 65: one pair, one lane quad, one short of a wavefront,
a full one, one pair into the second and into the third.  The same batches with k_ml_lines4 forced (the QUAD = true
instantiation shares every helper) must give the same bytes.  Bit-exact (576-byte canonical Fq12 serialisations).
Needs an MI355X."""
import pytest

from conftest import cat, engine_with_env

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 31, 32, 33, 65]
# (pairs per group, groups): the groups of one call are of one size, so unequal sizes are unequal calls; the totals are
# 33, 32, 33, 62, 66 and 65 pairs -- either side of one and two wavefronts, with group boundaries at even and odd pair indices
GROUPED = [(1, 33), (2, 16), (3, 11), (31, 2), (33, 2), (13, 5)]
FORMS = {"lines2": {"BLSGPU_LS_WIDE_MAX": "0", "BLSGPU_LS_QUAD_MAX": "0"}, "lines4": {"BLSGPU_LS_WIDE_MAX": "0"}}


@pytest.fixture(scope="module")
def chains():
    """one engine per chain kernel, every multi-pairing on the line-stream kernels, no group 'small'"""
    es = {}
    for name, env in FORMS.items():
        es[name] = engine_with_env(env)
        es[name].set_ls_threshold(1, 1)
    return es


@pytest.fixture(scope="module")
def expected(golden, seeded_pairs, oracle):
    """the value of the first n seeded pairs, computed once: the reference's vector where there is one, else the oracle"""
    g1, g2 = seeded_pairs
    seeded = golden("pairing.json")["seeded"]
    cache = {}

    def want(lo, n):
        if (lo, n) not in cache:
            if lo == 0 and str(n) in seeded and isinstance(seeded[str(n)], dict):
                cache[(lo, n)] = bytes.fromhex(seeded[str(n)]["out"])
            else:
                cache[(lo, n)] = oracle.pairing_multi(g1[96 * lo:96 * (lo + n)], g2[192 * lo:192 * (lo + n)], n, threads=8)
        return cache[(lo, n)]
    return want


@pytest.mark.parametrize("n", COUNTS)
def test_one_group(chains, seeded_pairs, expected, n):
    g1, g2 = seeded_pairs
    want = expected(0, n)
    for name, e in chains.items():
        assert e.pairing_multi(g1[:96 * n], g2[:192 * n], n) == want, name


@pytest.mark.parametrize("n", [8, 65])
def test_golden_vectors_byte_for_byte(chains, seeded_pairs, golden, n):
    g1, g2 = seeded_pairs
    v = golden("pairing.json")["seeded"][str(n)]
    for name, e in chains.items():
        assert e.pairing_multi(g1[:96 * n], g2[:192 * n], n).hex() == v["out"], name


@pytest.mark.parametrize("gsz,groups", GROUPED)
def test_groups(chains, seeded_pairs, expected, gsz, groups):
    g1, g2 = seeded_pairs
    m = gsz * groups
    want = b"".join(expected(gsz * g, gsz) for g in range(groups))
    for name, e in chains.items():
        assert e.pairing_multi_batch(g1[:96 * m], g2[:192 * m], gsz, groups) == want, name


@pytest.mark.parametrize("at", [16, 17, 32])
def test_degenerate_pair_at_even_and_odd_index(chains, seeded_pairs, golden, oracle, at):
    """a Q of order 13 (the chain ends with Z = 0: flagged behind the tangent steps, listed, its records rewritten by
    k_ml_lines_exact) at an even and an odd pair index of the first wavefront and alone in the second, in a 33-pair batch"""
    g1, g2 = seeded_pairs
    c = golden("pairing_degenerate.json")["cases"]["ord13"]
    a = g1[:96 * at] + cat(c["g1"]) + g1[96 * at:96 * 32]
    b = g2[:192 * at] + cat(c["g2"]) + g2[192 * at:192 * 32]
    assert len(a) == 96 * 33
    want = oracle.pairing_multi(a, b, 33, threads=8)
    for name, e in chains.items():
        assert e.pairing_multi(a, b, 33) == want, name


def test_flagged_pair_at_even_and_odd_index(chains, seeded_pairs, golden, oracle):
    """the caller's flag on a valid Q (q_flagged in front of the chain) at pair 7 and at pair 8 of a 33-pair batch"""
    g1, g2 = seeded_pairs
    for at in (7, 8):
        inf = bytes(2 * at) + bytes([0, 1]) + bytes(2 * (32 - at))
        want = oracle.pairing_multi(g1[:96 * 33], g2[:192 * 33], 33, threads=8, inf=inf)
        for name, e in chains.items():
            assert e.pairing_multi(g1[:96 * 33], g2[:192 * 33], 33, inf) == want, (name, at)
