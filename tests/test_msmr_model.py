"""The integer model of the ragged multi-scalar sums (vmgen/msmr_model.py, the specification of csrc/blsgpu_msmr.hip and of
msm_ranges_dev) against sums by the chord-and-tangent rule on integers: the chunk table at the lengths where it changes shape,
a chunk's window recurrence at the scalars where a digit or a reduction could go wrong, the cases an incomplete formula fails,
a point off the curve; and the boundary of the four new calls -- header, prototype table, extension lookup."""
import ctypes

import pytest

from test_abi_and_host import header_declarations
from test_pscan_model import G1, G2, INF, aff_add, aff_mul, aff_neg
from vmgen import msmr_model as M
from vmgen import pscan_model as P

NEW_SYMBOLS = ("blsgpu_g1_msm_ranges", "blsgpu_g2_msm_ranges", "blsgpu_g1_msm_ranges_dev", "blsgpu_g2_msm_ranges_dev")
N = P.R
GEN = {P.FQ: G1, P.FQ2: G2}
SPECIAL = [0, 1, N - 1, N, 1 << 255, (1 << 256) - 1]


def naive(F, pts, scalars):
    """sum s_i P_i by double-and-add and the textbook addition; a point off the curve adds nothing"""
    acc = INF[F]
    for p, s in zip(pts, scalars):
        if P.kind_of(F, p) == 1:
            acc = aff_add(F, acc, aff_mul(F, p, s))
    return acc


def test_chunk_table_at_the_lengths_where_it_changes_shape():
    lengths = [0, 1, 7, 8, 9, 16, 17]
    ranges, lo = [], 0
    for L in lengths:
        ranges.append((lo, lo + L))
        lo += L
    n = lo
    ranges += [(3, 20), (3, 20), (0, n), (n, n), (5, 5), (10, 11)]           # overlapping, repeated, whole, empty
    counts = M.chunk_counts(ranges, n)
    assert counts[:7] == [0, 1, 1, 1, 2, 2, 3] and counts[7:] == [3, 3, -(-n // 8), 0, 0, 1]
    first, table = M.chunk_table(ranges, n)
    assert first == M.exclusive_scan(counts) and first[0] == 0 and len(first) == len(ranges) + 1 and first[-1] == len(table)
    for j, (b, e) in enumerate(ranges):
        mine = table[first[j]:first[j + 1]]
        assert all(1 <= c <= M.CHUNK for _, c in mine)
        assert all(c == M.CHUNK for _, c in mine[:-1])                       # only a range's last chunk is short
        covered = [i for p, c in mine for i in range(p, p + c)]
        assert covered == list(range(b, e)), (j, b, e)
    assert M.chunk_table([], 5) == ([0], []) and M.chunk_table([(0, 0)], 0) == ([0, 0], [])
    for bad in ([(3, 2)], [(0, n + 1)], [(0, 1), (n + 1, n + 1)]):
        with pytest.raises(ValueError):
            M.chunk_table(bad, n)
    with pytest.raises(ValueError):                                          # 2^31 chunks: sixteen ranges of 2^27 chunks each
        M.chunk_counts([(0, 1 << 30)] * 16, 1 << 30)
    assert sum(M.chunk_counts([(0, 1 << 30)] * 15, 1 << 30)) == 15 << 27


def test_digits_are_the_nibbles_of_the_big_endian_words():
    for s in SPECIAL + [0x0123456789abcdef << 64 | 0xfedcba9876543210]:
        d = M.digits(s)
        assert len(d) == 64 and all(0 <= x < 16 for x in d) and sum(x << (4 * w) for w, x in enumerate(d)) == s
    with pytest.raises(ValueError):
        M.digits(1 << 256)


@pytest.mark.parametrize("F", [P.FQ, P.FQ2], ids=["g1", "g2"])
def test_chunk_recurrence_equals_the_sum_at_the_special_scalars(F):
    g = GEN[F]
    pts = [aff_mul(F, g, k) for k in (1, 2, 3, 5, 7, 11)]
    acc, bad, ops = M.chunk_sum(F, pts, SPECIAL)
    assert bad == 0 and P.affine(F, acc) == naive(F, pts, SPECIAL)
    assert ops == {"dbl": 252, "add": 64 * 6, "table_add": 14 * 6}
    # N P = infinity for a point of the subgroup: the scalar is not reduced, the sum is what it is
    for s in SPECIAL:
        acc, _, ops = M.chunk_sum(F, [g], [s])
        assert P.affine(F, acc) == aff_mul(F, g, s % N) and ops == {"dbl": 252, "add": 64, "table_add": 14}
    # a full chunk of eight and every digit value
    pts8 = [aff_mul(F, g, k) for k in range(2, 10)]
    sc8 = [0x0123456789abcdef * (k + 1) + (k << 200) for k in range(8)]
    acc, bad, _ = M.chunk_sum(F, pts8, sc8)
    assert bad == 0 and P.affine(F, acc) == naive(F, pts8, sc8)
    with pytest.raises(ValueError):
        M.chunk_sum(F, pts8 + [g], sc8 + [1])
    with pytest.raises(ValueError):
        M.chunk_sum(F, [], [])


@pytest.mark.parametrize("F", [P.FQ, P.FQ2], ids=["g1", "g2"])
def test_the_cases_an_incomplete_formula_fails(F):
    g = GEN[F]
    p, q = aff_mul(F, g, 5), aff_mul(F, g, 9)
    s = 0xdeadbeef << 100 | 12345
    # P and -P under one scalar in one chunk: infinity, with other terms or alone
    acc, _, _ = M.chunk_sum(F, [p, aff_neg(F, p)], [s, s])
    assert P.affine(F, acc) == INF[F]
    acc, _, _ = M.chunk_sum(F, [p, q, aff_neg(F, p)], [s, 3, s])
    assert P.affine(F, acc) == aff_mul(F, q, 3)
    # one point twice in a chunk: the window's second addition meets acc = T[d] -- a doubling inside an addition
    acc, _, _ = M.chunk_sum(F, [p, p], [7, 7])
    assert P.affine(F, acc) == aff_mul(F, p, 14)
    acc, _, _ = M.chunk_sum(F, [p, p, q], [s, s, 1])
    assert P.affine(F, acc) == naive(F, [p, p, q], [s, s, 1])
    # (0, 0) inputs and zero scalars
    acc, bad, _ = M.chunk_sum(F, [INF[F], p, INF[F]], [5, 0, 0])
    assert bad == 0 and P.affine(F, acc) == INF[F]
    # through the per-range combination.  Chunks are cut from a range's own begin, so [7, 9) is ONE chunk ...
    pts = [q] * 7 + [p, aff_neg(F, p)] + [q] * 3
    sc = [1] * 7 + [s, s] + [2] * 3
    got = M.msm_ranges(F, pts, sc, [(7, 9), (0, 12), (0, 0), (8, 9)])
    assert got[0] == (1, INF[F]) and got[2] == (1, INF[F])
    assert got[1] == (0, naive(F, pts, sc)) and got[3] == (0, aff_mul(F, aff_neg(F, p), s))
    # ... and ACROSS a chunk boundary: in [0, 10) chunk 0 is points 0 .. 7 and ends with P, chunk 1 is points 8 .. 9 and
    # begins with -P, every other scalar zero -- two finite partials s P and -s P, flag 1 from the range difference
    sc = [0] * 7 + [s, s] + [0] * 3
    first, table = M.chunk_table([(0, 10)], len(pts))
    assert table == [(0, 8), (8, 2)]
    halves = [P.affine(F, M.chunk_sum(F, pts[a:a + c], sc[a:a + c])[0]) for a, c in table]
    assert halves[0] == aff_mul(F, p, s) and halves[1] == aff_neg(F, halves[0]) and halves[0] != INF[F]
    got = M.msm_ranges(F, pts, sc, [(0, 10), (0, 8), (8, 10), (0, 12)])
    assert got == [(1, INF[F]), (0, halves[0]), (0, halves[1]), (1, INF[F])]
    # the general form: nine points under different scalars, the ninth the negative of the first eight's sum
    eight = [aff_mul(F, g, k) for k in range(2, 10)]
    sc8 = [0x1234567 * (k + 1) + (k << 140) for k in range(8)]
    total = naive(F, eight, sc8)
    assert total != INF[F]
    got = M.msm_ranges(F, eight + [aff_neg(F, total)], sc8 + [1], [(0, 9), (0, 8), (1, 9)])
    assert got[0] == (1, INF[F]) and got[1] == (0, total) and got[2][0] == 0


def test_ranges_of_every_shape_against_the_naive_sums():
    F = P.FQ
    n = 40
    pts = [aff_mul(F, G1, 3 * k + 1) for k in range(n)]
    pts[4] = INF[F]
    sc = [(k * 0x9e3779b97f4a7c15 + (k << 130)) % (1 << 256) for k in range(n)]
    sc[6], sc[20], sc[21] = 0, N, (1 << 256) - 1
    ranges = [(0, 0), (0, 1), (0, 7), (0, 8), (0, 9), (8, 24), (3, 20), (3, 20), (0, n), (n, n), (39, 40), (23, 40)]
    got = M.msm_ranges(F, pts, sc, ranges)
    for (b, e), (flag, pt) in zip(ranges, got):
        want = naive(F, pts[b:e], sc[b:e])
        assert pt == want and flag == (1 if want == INF[F] else 0), (b, e)


@pytest.mark.parametrize("F", [P.FQ, P.FQ2], ids=["g1", "g2"])
def test_a_point_off_the_curve_flags_exactly_the_ranges_that_hold_it(F):
    g = GEN[F]
    n = 20
    pts = [aff_mul(F, g, k + 1) for k in range(n)]
    x, y = pts[9]
    pts[9] = (x, F.add(y, F.one))
    assert P.kind_of(F, pts[9]) == 2
    acc, bad, _ = M.chunk_sum(F, pts[8:12], [1, 2, 3, 4])
    assert bad == 1 and P.affine(F, acc) == naive(F, pts[8:12], [1, 2, 3, 4])
    sc = [k + 2 for k in range(n)]
    ranges = [(0, n), (0, 9), (9, 10), (10, n), (8, 12), (0, 10), (9, 9), (10, 10), (16, 20)]
    got = M.msm_ranges(F, pts, sc, ranges)
    for (b, e), (flag, pt) in zip(ranges, got):
        if b <= 9 < e:
            assert (flag, pt) == (2, INF[F])
        else:
            want = naive(F, pts[b:e], sc[b:e])
            assert (flag, pt) == (1 if want == INF[F] else 0, want), (b, e)


def test_header_and_prototype_table_cover_the_new_calls():
    from bls_py import _native

    def kind(t):
        return "pointer" if t in (ctypes.c_void_p, ctypes.c_char_p) else {ctypes.c_size_t: "size_t", ctypes.c_int: "int"}[t]

    declared = header_declarations()
    for name in NEW_SYMBOLS:
        assert declared[name][0] == "int"
        assert name in _native.PROTOTYPES and name in _native.SYMBOLS, name
        assert [kind(t) for t in _native.PROTOTYPES[name]] == declared[name][1], name
    sums = ["pointer", "pointer", "pointer", "size_t", "pointer", "size_t", "pointer", "pointer"]
    assert declared["blsgpu_g1_msm_ranges"][1] == declared["blsgpu_g2_msm_ranges"][1] == sums
    assert declared["blsgpu_g1_msm_ranges_dev"][1] == declared["blsgpu_g2_msm_ranges_dev"][1] == sums + ["pointer"]


def test_extension_lookup():
    from bls_py import _native, _native_msmr, backend
    assert set(backend.EXTENSIONS) == {"keys_from_seeds"}
    assert backend.MSM_RANGE_EXTENSIONS == {"g1_msm_ranges": "_native_msmr", "g2_msm_ranges": "_native_msmr"}
    for method in ("g1_msm_ranges", "g2_msm_ranges"):
        assert callable(getattr(_native_msmr, method)) and callable(getattr(_native_msmr, method + "_dev"))
        assert not hasattr(_native.Engine, method) and not hasattr(backend.HipProvider, method) and method not in backend.PROVIDER_METHODS
    p = backend.HipProvider.__new__(backend.HipProvider)
    p._eng = object()
    old = backend._provider
    try:
        backend.use(p)
        fn = backend.extension("g1_msm_ranges")
        assert fn.func is _native_msmr.g1_msm_ranges and fn.args == (p._eng,)
        assert backend.extension("g2_msm_ranges").func is _native_msmr.g2_msm_ranges
        backend.use(object())                                              # a bare stand-in
        assert backend.extension("g1_msm_ranges") is None and backend.extension("g2_msm_ranges") is None
    finally:
        backend.use(old)
