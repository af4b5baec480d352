"""blsgpu_g?_msm_ranges across its slice boundaries: engines created under BLSGPU_TEST_SLICE_CAP cut the chunks into launches
and the partials' prefix records into slices.  The launch slice is the cap rounded up to a wavefront of units, so in G1 caps 1,
3 and 64 all give launches of 64 chunks (in G2: 32, 32 and 64) and cap 128 gives 128 in both; the range-sum passes over the
partials see the cap itself (1, 3, 64, 128 records a slice).  The skewed mix -- one range of 512 points, 64 chunks, ending
exactly on the 64-chunk edge, then 8 ranges of one --, ranges whose chunks straddle the edges at 32, 64 and 128 chunks, and a
mix of more than 128 chunks in which no edge coincides with a range's end; the bytes must be those of the uncapped engine."""
import hashlib
import random

import pytest

from bls_py import _native_msmr as R
from bls_py import hostmath as H
from conftest import engine_with_env

pytestmark = pytest.mark.gpu

N = H.N
MSG = hashlib.sha256(b"msm ranges slices").digest()
NPTS = 560


@pytest.fixture(scope="module")
def capped():
    made = {}

    def get(cap):
        if cap not in made:
            made[cap] = engine_with_env({"BLSGPU_TEST_SLICE_CAP": str(cap)})
        return made[cap]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def worlds(engine):
    out = {}
    for deg in (1, 2):
        rng = random.Random("msm ranges slices %d" % deg)
        t = [rng.randrange(1, N) for _ in range(NPTS)]
        s = [rng.randrange(1 << 256) for _ in range(NPTS)]
        t[300], s[300] = N - t[299], s[299]                  # a cancelling couple inside the long range ([299, 301) is one chunk)
        # [310, 319): chunk 0 is 310 .. 317, chunk 1 is point 318 alone -- two finite partials that cancel across a chunk boundary
        t[318] = (-sum(a * b for a, b in zip(s[310:318], t[310:318]))) * pow(s[318], -1, N) % N
        buf = engine.g1_mul_gen(t, aff=True, ser=False)[0] if deg == 1 else engine.sign(t, MSG, aff=True, ser=False)[0]
        bad = bytearray(buf)
        bad[96 * deg * 530 + 96 * deg - 1] ^= 1              # point 530 off the curve in the second input
        out[deg] = (s, buf, bytes(bad))
    return out


def mixes():
    skew = [(0, 512)] + [(512 + i, 513 + i) for i in range(8)]
    # ranges whose chunks straddle the boundaries at 32 and 64 chunks: 30 single chunks, then ranges of 3 and 5 chunks, then more
    straddle = [(i, i + 1) for i in range(30)] + [(100, 124), (200, 237), (0, 0), (3, 20), (3, 20), (40, 300), (520, 560), (299, 301), (310, 319)]
    # more than 128 chunks, no range ending on a multiple of 64: 29 + 3 + 33 (chunk 64 inside it) + 65 (chunk 128 inside it) + ...
    long = [(i, i + 1) for i in range(29)] + [(100, 124), (40, 300), (0, 515), (310, 319), (530, 531), (7, 77)]
    return {"skew": skew, "straddle": straddle, "both": skew + straddle, "long": long}


@pytest.mark.parametrize("deg", [1, 2])
@pytest.mark.parametrize("cap", [1, 3, 64, 128])
def test_capped_engines_give_the_bytes_of_the_uncapped_one(engine, capped, worlds, deg, cap):
    s, buf, bad = worlds[deg]
    fn = R.g1_msm_ranges if deg == 1 else R.g2_msm_ranges
    for name, ranges in mixes().items():
        want = fn(engine, buf, s, ranges)
        assert fn(capped(cap), buf, s, ranges) == want, name
        if name != "skew":
            j = ranges.index((310, 319))
            assert want[1][j] == 1 and want[0][96 * deg * j:96 * deg * (j + 1)] == bytes(96 * deg)
        if name in ("straddle", "both"):
            assert want[1][ranges.index((299, 301))] == 1
    # a point off the curve in a late slice flags the ranges that hold it, and only them
    ranges = mixes()["both"]
    want = fn(engine, bad, s, ranges)
    assert [f == 2 for f in want[1]] == [b <= 530 < e for b, e in ranges] and any(f == 2 for f in want[1])
    assert fn(capped(cap), bad, s, ranges) == want
