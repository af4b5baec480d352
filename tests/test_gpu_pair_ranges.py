"""The ragged multi-pairing on the device: blsgpu_pairing_multi_ranges and its _dev form (csrc/blsgpu_mlr.hip, schedule in
csrc/pairing_ranges_plan.h) through bls_py._native_pairranges, and BLS.verify_batch(ragged=True) on the HIP provider.
Expected values are oracle.pairing_multi per range (the CPU restatement pinned to the reference fixtures) and the
reference-generated fixtures themselves (pairing.json, pairing_degenerate.json) -- never the new call; byte equality with
blsgpu_pairing_multi_batch is asserted beside that.  C = 16 is the default chunk, FAN = 8 the fold's fan."""
import pytest

from conftest import cat, engine_with_env

pytestmark = pytest.mark.gpu

C, FAN = 16, 8


@pytest.fixture(scope="module")
def R():
    from bls_py import _native_pairranges
    return _native_pairranges


@pytest.fixture(scope="module")
def expect(oracle, seeded_pairs):
    """oracle.pairing_multi of every range of a pair list, each distinct run of the seeded pairs computed once"""
    seen = {}

    def run(ranges, g1=None, g2=None, inf=None):
        out = b""
        for b, e in ranges:
            key = (b, e) if g1 is None else None
            if key in seen:
                out += seen[key]
                continue
            a1, a2 = (seeded_pairs[0], seeded_pairs[1]) if g1 is None else (g1, g2)
            v = oracle.pairing_multi(a1[96 * b:96 * e], a2[192 * b:192 * e], e - b, threads=8, inf=None if inf is None else inf[2 * b:2 * e])
            if key is not None:
                seen[key] = v
            out += v
        return out
    return run


def seeded(seeded_pairs, n):
    return seeded_pairs[0][:96 * n], seeded_pairs[1][:192 * n]


def side_by_side(lens):
    ranges, at = [], 0
    for v in lens:
        ranges.append((at, at + v))
        at += v
    return at, ranges


@pytest.fixture(scope="module")
def ONE(oracle):
    """Fq12 one, as the reference serialises it: also the oracle's product of no pairs"""
    from bls_py.ec import default_ec
    from bls_py.fields import Fq12
    one = Fq12.one(default_ec.q).serialize()
    assert oracle.pairing_multi(b"", b"", 0) == one
    return one


def test_lengths(engine, R, seeded_pairs, expect, ONE):
    """0, 1, 2, C-1, C, C+1, 2C+1 pairs in one call, an empty range first, in the middle and last"""
    n, ranges = side_by_side([0, 1, 2, C - 1, C, 0, C + 1, 2 * C + 1, 0])
    g1, g2 = seeded(seeded_pairs, n)
    got = R.pairing_multi_ranges(engine, g1, g2, ranges)
    assert got == expect(ranges)
    assert [got[576 * j:576 * (j + 1)] == ONE for j in range(len(ranges))] == [True, False, False, False, False, True, False, False, True]


@pytest.mark.parametrize("k", [9, 10, 11, 19, 20, 21])
def test_chunk_counts_around_a_wavefront_of_ten_teams(engine, R, seeded_pairs, expect, k):
    g1, g2 = seeded(seeded_pairs, k)
    ranges = [(i, i + 1) for i in range(k)]
    assert R.pairing_multi_ranges(engine, g1, g2, ranges) == expect(ranges)


def test_one_long_chunk_beside_nine_of_one_pair(engine, R, seeded_pairs, expect):
    """the divergent trip count: the second wavefront's teams run 16, 1, 1, .. pairs -- every position of the long one"""
    for at in (0, 4, 9):
        lens = [1] * 10 + [1] * at + [C] + [1] * (9 - at)
        n, ranges = side_by_side(lens)
        g1, g2 = seeded(seeded_pairs, n)
        assert R.pairing_multi_ranges(engine, g1, g2, ranges) == expect(ranges), at
    # ... and an empty chunk, a long one and a short one in a last wavefront of three teams
    n, ranges = side_by_side([2] * 10 + [0, C, 3])
    g1, g2 = seeded(seeded_pairs, n)
    assert R.pairing_multi_ranges(engine, g1, g2, ranges) == expect(ranges)


@pytest.fixture(scope="module")
def chunk2():
    e = engine_with_env({"BLSGPU_PAIR_RANGES_CHUNK": "2"})
    yield e
    e.close()


def test_fold(chunk2, R, seeded_pairs, expect):
    """chunks of 2: ranges of FAN, FAN + 1 and FAN^2 + 1 chunks (16, 17 and 129 pairs; the last one a pair short of a chunk, and
    FAN^2 chunks beside them) fold in one, two and three levels"""
    ranges = [(0, 2 * FAN), (0, 2 * FAN + 1), (1, 2 * FAN * FAN + 1), (0, 2 * FAN * FAN + 1), (5, 6), (3, 3)]
    g1, g2 = seeded(seeded_pairs, 2 * FAN * FAN + 2)
    assert R.pairing_multi_ranges(chunk2, g1, g2, ranges) == expect(ranges)


def test_overlapping_and_repeated_ranges_and_the_fixture_of_65_pairs(engine, R, golden, seeded_pairs, expect):
    ranges = [(0, 65), (10, 30), (0, 65), (64, 100), (10, 30), (99, 100), (100, 100), (30, 99)]
    g1, g2 = seeded(seeded_pairs, 100)
    got = R.pairing_multi_ranges(engine, g1, g2, ranges)
    assert got == expect(ranges)
    assert got[:576].hex() == golden("pairing.json")["seeded"]["65"]["out"]
    assert got[:576] == got[2 * 576:3 * 576] and got[576:2 * 576] == got[4 * 576:5 * 576]


def test_degenerate_pairs_inside_ranges(engine, R, golden, seeded_pairs, expect):
    """every case of pairing_degenerate.json (k pairs) alone -- the fixture's bytes --, then followed by ordinary pairs in ranges
    of 3 and of C + 1 pairs, against the oracle with the flags"""
    cases = golden("pairing_degenerate.json")["cases"]
    g1 = g2 = inf = b""
    ranges, alone = [], []
    for i, (name, v) in enumerate(sorted(cases.items())):
        k, at = len(v["g1"]), len(g1) // 96
        fill = C + 1 - k
        g1 += cat(v["g1"]) + seeded_pairs[0][96 * 20 * i:96 * (20 * i + fill)]
        g2 += cat(v["g2"]) + seeded_pairs[1][192 * 20 * i:192 * (20 * i + fill)]
        inf += bytes(int(f) for pq in v["inf"] for f in pq) + bytes(2 * fill)
        alone.append((len(ranges), name))
        ranges += [(at, at + k), (at, at + max(k, 3)), (at, at + C + 1), (at + k - 1, at + k)]
    got = R.pairing_multi_ranges(engine, g1, g2, ranges, inf=inf)
    want = expect(ranges, g1, g2, inf)
    for j, name in alone:
        assert got[576 * j:576 * (j + 1)].hex() == cases[name]["out"], name
    assert got == want


@pytest.mark.parametrize("gsz", [2, 5])
def test_equal_lengths_give_the_bytes_of_the_batch_call(engine, R, seeded_pairs, expect, gsz):
    groups = 23
    g1, g2 = seeded(seeded_pairs, gsz * groups)
    ranges = [(gsz * g, gsz * (g + 1)) for g in range(groups)]
    got = R.pairing_multi_ranges(engine, g1, g2, ranges)
    assert got == expect(ranges)
    assert got == engine.pairing_multi_batch(g1, g2, gsz, groups)


def test_slices(R, seeded_pairs, expect):
    """slices of 24 pairs: [20, 30) spans two of them, [0, 60) three, the boundary at 24 falls inside the chunk-sized run
    [16, 32) of [0, 60), an empty range sits on a boundary; results go through the final stage 24 at a time (30 ranges)"""
    e = engine_with_env({"BLSGPU_TEST_SLICE_CAP": "24"})
    try:
        ranges = [(20, 30), (0, 60), (23, 25), (24, 24), (47, 49), (60, 60)] + [(2 * i, 2 * i + 3) for i in range(24)]
        g1, g2 = seeded(seeded_pairs, 60)
        assert R.pairing_multi_ranges(e, g1, g2, ranges) == expect(ranges)
    finally:
        e.close()


def test_refusals_leave_out_untouched(engine, R, seeded_pairs):
    import ctypes
    from bls_py._native import BlsGpuError
    g1, g2 = seeded(seeded_pairs, 4)

    def call(a1, a2, n, ranges, m, out, tab=None):
        tab = tab if tab is not None else (R.range_table(engine, ranges)[0] if ranges is not None else None)
        return engine.lib.blsgpu_pairing_multi_ranges(engine.h, a1, a2, None, n, tab, m, out)

    out = ctypes.create_string_buffer(b"\xa5" * (2 * 576), 2 * 576)
    EINVAL = -22
    assert call(g1, g2, 4, [(0, 2), (3, 2)], 2, out) == EINVAL                # begin > end
    assert call(g1, g2, 4, [(0, 2), (3, 5)], 2, out) == EINVAL                # end > n
    assert call(None, g2, 4, [(0, 2)], 1, out) == EINVAL and call(g1, None, 4, [(0, 2)], 1, out) == EINVAL
    assert call(g1, g2, 4, None, 1, out) == EINVAL and call(g1, g2, 4, [(0, 2)], 1, None) == EINVAL
    assert call(g1, g2, 0x3FFFFFF1, [(0, 2)], 1, out) == EINVAL               # too many pairs (nothing is read)
    assert engine.lib.blsgpu_pairing_multi_ranges(None, g1, g2, None, 4, R.range_table(engine, [(0, 2)])[0], 1, out) == EINVAL
    assert out.raw == b"\xa5" * (2 * 576)
    with pytest.raises(BlsGpuError):
        R.pairing_multi_ranges(engine, g1, g2, [(0, 5)])
    # 2^31 chunks: 2048 times the range [0, 2^20) in chunks of one pair -- refused by the host plan before any buffer is touched
    e = engine_with_env({"BLSGPU_PAIR_RANGES_CHUNK": "1"})
    try:
        tab = R.range_table(e, [(0, 1 << 20)] * 2048)[0]
        assert e.lib.blsgpu_pairing_multi_ranges(e.h, g1, g2, None, 1 << 20, tab, 2048, out) == EINVAL
        assert b"2^31" in e.lib.blsgpu_last_error()
    finally:
        e.close()
    assert out.raw == b"\xa5" * (2 * 576)


def test_no_ranges_and_no_pairs(engine, R, ONE):
    assert R.pairing_multi_ranges(engine, b"", b"", []) == b""
    assert engine.lib.blsgpu_pairing_multi_ranges(engine.h, None, None, None, 0, None, 0, None) == 0
    assert R.pairing_multi_ranges(engine, b"", b"", [(0, 0), (0, 0), (0, 0)]) == ONE * 3


def test_dev_form_on_a_stream_with_the_workspace_accounted(R, seeded_pairs, expect):
    import torch
    from bls_py import _native
    e = _native.Engine(0)
    try:
        n, ranges = side_by_side([3, 0, C + 5, 1, 40])
        ranges.append((2, 30))
        g1, g2 = seeded(seeded_pairs, n)
        dev = torch.device("cuda:0")
        d1 = torch.frombuffer(bytearray(g1), dtype=torch.uint8).to(dev)
        d2 = torch.frombuffer(bytearray(g2), dtype=torch.uint8).to(dev)
        dout = torch.zeros(576 * len(ranges), dtype=torch.uint8, device=dev)
        before = e.workspace_bytes()
        st = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            R.pairing_multi_ranges_dev(e, d1.data_ptr(), d2.data_ptr(), n, ranges, dout.data_ptr(), stream=st.cuda_stream)
            R.pairing_multi_ranges_dev(e, d1.data_ptr(), d2.data_ptr(), n, ranges[::-1], dout.data_ptr(), stream=st.cuda_stream)
            R.pairing_multi_ranges_dev(e, d1.data_ptr(), d2.data_ptr(), n, ranges, dout.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        assert bytes(dout.cpu().numpy().tobytes()) == expect(ranges)
        after = e.workspace_bytes()
        # the line records of the n pairs, and at least the partials (a slot per range and per chunk of the folded ones) and
        # the tables in the total
        assert after["lines"] - before["lines"] >= n * 68 * 84 * 4 or before["lines"] >= n * 68 * 84 * 4
        grown = sum(after[k] - before[k] for k in after if k != "total")
        assert after["total"] - before["total"] >= grown + (len(ranges) + 2 + 3 + 2) * 576     # chunks of 16: 21, 40 and 28 pairs fold
    finally:
        e.close()


def test_verify_batch_ragged_on_the_hip_provider():
    """the batch of test_gpu_verify_ragged.py::test_the_batch_verifications_agree -- aggregates of 7 pairs each, one key or one
    exponent changed in two of them -- through ONE ranges call"""
    from bls_py import backend
    from bls_py.bls import BLS
    import test_gpu_verify_ragged as V
    backend.use(None)
    try:
        good, bad_exp, bad_key = _world(V)
        _, second = V.aggregate(b"second")
        batch = [good, bad_exp, second, bad_key, good]
        assert backend.extension("pairing_multi_ranges") is not None
        assert BLS.verify_batch(batch, ragged=True) == [True, False, True, False, True]
        assert BLS.verify_batch(batch) == [True, False, True, False, True]
    finally:
        backend.use(None)


def _world(V):
    """test_gpu_verify_ragged.world's aggregates (the fixture's body, for a caller that is not a test of that module)"""
    from bls_py.bls12381 import n as ORDER
    sks, good = V.aggregate(b"ragged")
    tree = dict(good.aggregation_info.tree)
    by_msg = {}
    for mh, pk in tree:
        by_msg.setdefault(mh, []).append(pk)
    shared = next(mh for mh, v in by_msg.items() if len(v) == 9)
    victim = sorted(pk for mh, pk in tree if mh == shared)[4]
    bad_exp = dict(tree)
    bad_exp[(shared, victim)] = (tree[(shared, victim)] + 1) % ORDER
    bad_key = dict(tree)
    del bad_key[(shared, victim)]
    other = next(pk for mh, pk in tree if mh != shared)
    bad_key[(shared, other)] = tree[(shared, victim)]
    return good, V.with_tree(good, bad_exp), V.with_tree(good, bad_key)
