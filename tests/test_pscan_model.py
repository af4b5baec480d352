"""The integer model of the point prefix sums and range sums (vmgen/pscan_model.py, the specification of csrc/blsgpu_pscan.hip)
against sums by the chord-and-tangent rule on integers, at the sizes where a pass changes shape and at the inputs where an
incomplete formula would fail; and the boundary of the six new calls -- header, prototype table, extension lookup."""
import ctypes
import random

import pytest

from test_abi_and_host import header_declarations
from vmgen import pscan_model as M

NEW_SYMBOLS = ("blsgpu_g1_range_sums", "blsgpu_g2_range_sums", "blsgpu_g1_range_sums_dev", "blsgpu_g2_range_sums_dev",
               "blsgpu_verify_find_folded", "blsgpu_verify_find_folded_dev")
G1 = (0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
      0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1)
G2 = ((0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
       0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e),
      (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
       0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be))
INF = {M.FQ: (0, 0), M.FQ2: ((0, 0), (0, 0))}


def aff_add(F, p, q):
    """the textbook rule on affine points, every case spelled out; (0, 0) is infinity"""
    if p == INF[F]:
        return q
    if q == INF[F]:
        return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if F.add(y1, y2) == F.zero:
            return INF[F]
        lam = F.mul(F.mul(F.add(F.add(x1, x1), x1), x1), F.inv(F.add(y1, y1)))
    else:
        lam = F.mul(F.sub(y2, y1), F.inv(F.sub(x2, x1)))
    x3 = F.sub(F.sub(F.mul(lam, lam), x1), x2)
    return (x3, F.sub(F.mul(lam, F.sub(x1, x3)), y1))


def aff_neg(F, p):
    return (p[0], F.sub(F.zero, p[1]))


def aff_mul(F, p, k):
    r = INF[F]
    while k:
        if k & 1:
            r = aff_add(F, r, p)
        p = aff_add(F, p, p)
        k >>= 1
    return r


def multiples(F, g, count, seed):
    """count points k g for small random k, by additions of a short table"""
    rng = random.Random(seed)
    table = [INF[F]]
    for _ in range(40):
        table.append(aff_add(F, table[-1], g))
    return [table[rng.randrange(1, 41)] for _ in range(count)]


def check(F, pts, ranges, chunk=M.CHUNK, mid=M.MID_THREADS):
    S, cnt = M.scan(F, pts, chunk, mid)
    assert len(S) == len(cnt) == len(pts) + 1
    naive, bad = [INF[F]], [0]
    for p in pts:
        k = M.kind_of(F, p)
        naive.append(aff_add(F, naive[-1], p) if k == 1 else naive[-1])
        bad.append(bad[-1] + (k == 2))
    assert [M.affine(F, s) for s in S] == naive and cnt == bad
    for b, e in ranges:
        want = INF[F]
        for p in pts[b:e]:
            if M.kind_of(F, p) == 1:
                want = aff_add(F, want, p)
        flag, got = M.range_sum(F, S, cnt, b, e)
        if bad[e] != bad[b]:
            assert (flag, got) == (2, INF[F])
        else:
            assert got == want and flag == (1 if want == INF[F] else 0), (b, e)
    return S, cnt


def test_group_orders_are_odd():
    assert M.ORDER_G1 % 2 == 1 and M.ORDER_G2 % 2 == 1
    assert M.H1 == 0x396c8c005555e1568c00aaab0000aaab
    assert aff_mul(M.FQ, G1, M.R) == INF[M.FQ] and aff_mul(M.FQ2, G2, M.R) == INF[M.FQ2]
    assert M.on_curve(M.FQ, *G1) and M.on_curve(M.FQ2, *G2)


@pytest.mark.parametrize("n", [0, 1, 2, 15, 16, 17, 31, 32, 33])
def test_scan_around_the_chunk_boundaries(n):
    pts = multiples(M.FQ, G1, n, n)
    ranges = [(0, 0), (0, n), (n, n)] + [(b, e) for b in range(0, n + 1, 5) for e in range(b, n + 1, 7)] + [(0, e) for e in range(0, n + 1, 16)]
    check(M.FQ, pts, ranges)


@pytest.mark.parametrize("n", [15, 16, 17, 31, 33, 63, 64, 65, 70])
def test_scan_around_the_workgroup_boundaries_of_a_small_shape(n):
    """chunk 4 and 4 middle lanes: 16 points are one lane each of the middle, 17 give a lane two totals, 65 give five"""
    pts = multiples(M.FQ, G1, n, 100 + n)
    check(M.FQ, pts, [(0, n), (3, n - 2), (n // 2, n // 2 + 1)] + [(b, min(b + 4, n)) for b in range(0, n, 4)], chunk=4, mid=4)


@pytest.mark.parametrize("n", [2047, 2048, 2049, 2064, 2065])
def test_scan_around_the_workgroup_boundary_of_the_device_shape(n):
    """128 middle lanes of 16 points: 2048 points are one total a lane, 2049 make some lanes take two"""
    pts = multiples(M.FQ, G1, n, 7)
    check(M.FQ, pts, [(0, n), (2040, n), (1, 2047), (min(2048, n), n), (16 * 127, min(16 * 128, n))])


def test_g2_scan():
    pts = multiples(M.FQ2, G2, 37, 3)
    pts[5] = INF[M.FQ2]
    pts[8] = pts[7]
    pts[20] = aff_neg(M.FQ2, pts[19])
    check(M.FQ2, pts, [(0, 37), (5, 6), (7, 9), (19, 21), (16, 32), (0, 0)])
    check(M.FQ2, pts, [(0, 37), (19, 21)], chunk=4, mid=4)


def test_the_cases_an_incomplete_formula_fails():
    F = M.FQ
    p, q, r = aff_mul(F, G1, 5), aff_mul(F, G1, 11), aff_mul(F, G1, 3)
    # inputs at infinity, first and last and a whole chunk of them
    pts = [INF[F]] + [p, q] + [INF[F]] * 18 + [r, INF[F]]
    check(F, pts, [(0, len(pts)), (0, 1), (3, 21), (2, 22), (len(pts) - 1, len(pts))])
    # adjacent equal points (the mixed addition meets P + P when the prefix equals the point) and P then -P
    pts = [p, p, p, p, q, aff_neg(F, q), r, aff_neg(F, r), aff_neg(F, p)]
    check(F, pts, [(0, 2), (0, 4), (1, 3), (4, 6), (4, 8), (5, 7), (0, 9), (3, 9)])
    # a range summing to infinity whose two prefixes are FINITE AND EQUAL: S[b] - S[a] is P + (-P)
    pts = [p, q, aff_neg(F, q), r]
    S, cnt = check(F, pts, [(1, 3)])
    assert M.affine(F, S[1]) == M.affine(F, S[3]) == p and M.range_sum(F, S, cnt, 1, 3) == (1, INF[F])
    # a range whose prefixes are NEGATIVES of one another: S[b] - S[a] is P + P
    pts = [p, aff_neg(F, p), aff_neg(F, p), q]
    S, cnt = check(F, pts, [(1, 3), (0, 3)])
    assert M.affine(F, S[3]) == aff_neg(F, M.affine(F, S[1]))
    assert M.range_sum(F, S, cnt, 1, 3) == (0, aff_mul(F, aff_neg(F, p), 2))
    # both prefixes at infinity, and the doubling inside the middle scan (equal chunk totals)
    pts = [p, aff_neg(F, p)] * 3
    check(F, pts, [(0, 2), (2, 4), (0, 6), (2, 6)], chunk=2, mid=2)
    pts = [p, q] * 8
    check(F, pts, [(0, 16), (2, 6)], chunk=2, mid=4)


def test_a_point_off_the_curve_is_counted_and_adds_nothing():
    F = M.FQ
    pts = multiples(F, G1, 40, 9)
    pts[17] = (pts[17][0], (pts[17][1] + 1) % M.Q)
    assert M.kind_of(F, pts[17]) == 2
    S, cnt = check(F, pts, [(0, 40), (0, 17), (17, 18), (18, 40), (16, 33), (0, 18)])
    assert cnt[17] == 0 and cnt[18] == cnt[40] == 1
    with pytest.raises(ValueError):
        M.range_sum(F, S, cnt, 3, 2)
    with pytest.raises(ValueError):
        M.range_sum(F, S, cnt, 0, 41)


@pytest.mark.parametrize("slice_len", [1, 5, 16, 17, 32, 40])
def test_chained_slices_carry_on(slice_len):
    """more points than a slice of records holds: the carry into the next slice's middle scan, the begin kept from its slice"""
    F = M.FQ
    n = 70
    pts = multiples(F, G1, n, 11)
    pts[20] = INF[F]
    pts[31] = aff_neg(F, pts[30])
    pts[33] = (pts[33][0], (pts[33][1] + 1) % M.Q)                         # off the curve: the count is carried too
    S, cnt = M.scan(F, pts, 4, 4)
    slices = M.scan_slices(F, pts, slice_len, 4, 4)
    assert len(slices) == -(-n // slice_len) and slices[0][0] == 0 and slices[-1][1] == n
    for lo, hi, Ss, cs in slices:
        assert len(Ss) == hi - lo + 1
        assert [M.affine(F, x) for x in Ss] == [M.affine(F, x) for x in S[lo:hi + 1]] and cs == cnt[lo:hi + 1]
    edges = sorted({0, 1, n - 1, n, 30, 32, 33, 34} | {j for lo, hi, _, _ in slices for j in (lo, hi)})
    for b in edges:
        for e in edges:
            if b <= e:
                assert M.range_sum_slices(F, slices, b, e) == M.range_sum(F, S, cnt, b, e), (b, e)
    one = M.scan_slices(F, pts, 200, 4, 4)
    assert len(one) == 1 and M.range_sum_slices(F, one, 3, n) == M.range_sum(F, S, cnt, 3, n)


def test_header_and_prototype_table_cover_the_new_calls():
    from bls_py import _native

    def kind(t):
        return "pointer" if t in (ctypes.c_void_p, ctypes.c_char_p) else {ctypes.c_size_t: "size_t", ctypes.c_int: "int"}[t]

    declared = header_declarations()
    for name in NEW_SYMBOLS:
        assert declared[name][0] == "int"
        assert name in _native.PROTOTYPES and name in _native.SYMBOLS, name
        assert [kind(t) for t in _native.PROTOTYPES[name]] == declared[name][1], name
    sums = ["pointer", "pointer", "size_t", "pointer", "size_t", "pointer", "pointer"]
    assert declared["blsgpu_g1_range_sums"][1] == declared["blsgpu_g2_range_sums"][1] == sums
    assert declared["blsgpu_g1_range_sums_dev"][1] == declared["blsgpu_g2_range_sums_dev"][1] == sums + ["pointer"]
    assert declared["blsgpu_verify_find_folded"][1] == declared["blsgpu_verify_find"][1]
    assert declared["blsgpu_verify_find_folded_dev"][1] == declared["blsgpu_verify_find_dev"][1]


def test_extension_lookup():
    from bls_py import _native, _native_ranges, backend
    assert set(backend.EXTENSIONS) == {"keys_from_seeds"}
    for method in ("g1_range_sums", "g2_range_sums", "verify_find_folded"):
        assert callable(getattr(_native_ranges, method)) and callable(getattr(_native_ranges, method + "_dev"))
        assert not hasattr(_native.Engine, method) and not hasattr(backend.HipProvider, method) and method not in backend.PROVIDER_METHODS
    p = backend.HipProvider.__new__(backend.HipProvider)
    p._eng = object()
    old = backend._provider
    try:
        backend.use(p)
        fn = backend.extension("verify_find_folded")
        assert fn.func is _native_ranges.verify_find_folded and fn.args == (p._eng,)
        assert backend.extension("g1_range_sums").func is _native_ranges.g1_range_sums
        backend.use(object())                                              # a stand-in without the call
        assert backend.extension("verify_find_folded") is None
    finally:
        backend.use(old)
