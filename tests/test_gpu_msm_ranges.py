"""blsgpu_g1_msm_ranges / blsgpu_g2_msm_ranges on the device.  The points are t_i G1 (g1_mul_gen) and t_i H(m) (blsgpu_sign with
one message), so the expected sum of a range is the SINGLE multiplication by sum s_i t_i mod N from the same calls, compared
byte for byte: no curve arithmetic on the host.  Point counts around a chunk (8 points) and a wavefront of units (64 lanes in
G1, 32 lane pairs in G2); ranges of every length where the chunk table changes shape, empty, whole, overlapping and repeated;
the special scalars; sums at infinity inside a chunk and across a chunk boundary (chunks are cut from a range's own begin: the
ranges [22, 31) and [41, 51) are two chunks whose finite partials cancel), equal neighbours, (0,0) inputs, a point off
the curve; the bytes of the uniform group sums and of the oracle; -EINVAL; the _dev form; workspace."""
import ctypes
import hashlib
import random
import struct

import pytest

from bls_py import _native_msmr as R
from bls_py import hostmath as H

pytestmark = pytest.mark.gpu

N = H.N
TOP = 603
SIZES = [1, 7, 8, 9, 63, 64, 65, 520]
SPECIAL = [0, 1, N - 1, N, 1 << 255, (1 << 256) - 1]
MSG = hashlib.sha256(b"msm ranges").digest()


class Group:
    def __init__(self, engine, deg):
        self.deg, self.size, self.engine = deg, 96 * deg, engine
        self.sums = R.g1_msm_ranges if deg == 1 else R.g2_msm_ranges
        self.sums_dev = R.g1_msm_ranges_dev if deg == 1 else R.g2_msm_ranges_dev
        self.name = "blsgpu_g%d_msm_ranges" % deg

    def mul(self, scalars):
        """t G for every scalar ((0,0) for 0), one call"""
        e = self.engine
        out = e.g1_mul_gen(scalars, aff=True, ser=False)[0] if self.deg == 1 else e.sign(scalars, MSG, aff=True, ser=False)[0]
        return [out[self.size * i:self.size * (i + 1)] for i in range(len(scalars))]

    def msm(self, pts, scalars, k, groups):
        return (self.engine.g1_msm if self.deg == 1 else self.engine.g2_msm)(pts, scalars, k, groups)


@pytest.fixture(scope="module")
def worlds(engine):
    """per group: TOP discrete logarithms t with the special neighbours planted, their points, and TOP scalars s"""
    out = {}
    for deg in (1, 2):
        rng = random.Random("msm ranges %d" % deg)
        t = [rng.randrange(1, N) for _ in range(TOP)]
        s = [rng.randrange(1 << 256) for _ in range(TOP)]
        for i, v in enumerate(SPECIAL):                      # the special scalars: 16 .. 21, in two chunks of any range from 0
            s[16 + i] = v
        t[3], s[3] = N - t[2], s[2]                          # P, -P under one scalar inside one chunk: [2, 4) is infinity
        t[8], s[8] = N - t[7], s[7]                          # ... and again: [7, 9) is ONE chunk, chunks being cut from a range's begin
        t[13], s[13] = t[12], s[12]                          # equal neighbours under one scalar: a doubling inside an addition
        t[5] = 0                                             # an input at infinity
        t[40] = (-sum(a * b for a, b in zip(s[33:40], t[33:40]))) * pow(s[40], -1, N) % N   # [33, 41) sums to infinity: one chunk of 8
        # ACROSS a chunk boundary.  [22, 31): chunk 0 is 22 .. 29, chunk 1 is point 30 alone, two finite partials that cancel
        t[30] = (-sum(a * b for a, b in zip(s[22:30], t[22:30]))) * pow(s[30], -1, N) % N
        assert sum(a * b for a, b in zip(s[22:30], t[22:30])) % N != 0 and s[30] * t[30] % N != 0
        # ... and P, -P under one scalar either side of the boundary.  [41, 51): chunk 0 is 41 .. 48 and ends with P, chunk 1 is
        # 49 .. 50 and begins with -P; every other scalar of the range is zero
        t[49], s[49] = N - t[48], s[48]
        for i in (41, 42, 43, 44, 45, 46, 47, 50):
            s[i] = 0
        assert s[48] * t[48] % N != 0
        g = Group(engine, deg)
        pts = g.mul(t)
        assert pts[5] == bytes(g.size) and pts[12] == pts[13]
        out[deg] = (g, t, s, pts)
    return out


def ranges_for(n):
    rng = random.Random(n)
    r = [(0, 0), (n, n), (0, n), (0, 1), (n - 1, n), (0, n), (n // 2, n // 2)]
    r += [(min(2, n), min(4, n)), (min(7, n), min(9, n)), (min(12, n), min(14, n)), (min(5, n), min(6, n)), (min(33, n), min(41, n))]
    r += [(min(22, n), min(31, n)), (min(41, n), min(51, n)), (min(22, n), min(30, n)), (min(48, n), min(50, n))]
    r += [(0, min(L, n)) for L in (7, 8, 9, 16, 17)] + [(min(3, n), min(3 + L, n)) for L in (1, 7, 8, 9, 16, 17)]
    r += [(min(16, n), min(22, n)), (min(14, n), min(24, n))]                                 # the special scalars
    r += [tuple(sorted((rng.randrange(n + 1), rng.randrange(n + 1)))) for _ in range(12)]
    return r


def expect(g, t, s, ranges):
    """(bytes, flags) from ONE multiplication per range by sum s_i t_i mod N"""
    want = g.mul([sum(a * b for a, b in zip(s[b_:e_], t[b_:e_])) % N for b_, e_ in ranges])
    return b"".join(want), bytes(1 if not any(w) else 0 for w in want)


@pytest.mark.parametrize("deg", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_ranges(engine, worlds, deg, n):
    g, t, s, pts = worlds[deg]
    ranges = ranges_for(n)
    out, flag = g.sums(engine, b"".join(pts[:n]), s[:n], ranges)
    want, wflag = expect(g, t[:n], s[:n], ranges)
    assert flag == wflag
    assert out == want
    if n >= 41:
        for r in ((2, 4), (7, 9), (33, 41), (5, 6), (0, 0)):
            assert flag[ranges.index(r)] == 1, r
    if n >= 51:
        # two chunks whose finite partials cancel: flag 1 and (0,0); the first chunk of [22, 31) alone is finite
        for r in ((22, 31), (41, 51), (48, 50)):
            j = ranges.index(r)
            assert flag[j] == 1 and out[g.size * j:g.size * (j + 1)] == bytes(g.size), r
        assert flag[ranges.index((22, 30))] == 0


@pytest.mark.parametrize("deg", [1, 2])
@pytest.mark.parametrize("singles", [23, 31, 32, 33, 55, 56, 57, 58])
def test_chunk_counts_around_a_wavefront_of_units(engine, worlds, deg, singles):
    """the skewed mix: one range of 64 points (8 chunks) and `singles` ranges of one point -- 31 .. 66 chunks, across 32 units (a
    wavefront of G2 pairs), 64 and 65 (of G1 lanes) --, the singles overlapping the long range and repeating"""
    g, t, s, pts = worlds[deg]
    n = 100
    ranges = [(0, 64)] + [(i % 90 + 5, i % 90 + 6) for i in range(singles)] + [(0, 0)]
    out, flag = g.sums(engine, b"".join(pts[:n]), s[:n], ranges)
    assert (out, flag) == expect(g, t[:n], s[:n], ranges)


@pytest.mark.parametrize("deg", [1, 2])
def test_the_skewed_mix(engine, worlds, deg):
    g, t, s, pts = worlds[deg]
    n = 520
    ranges = [(0, 512)] + [(512 + i, 513 + i) for i in range(8)]
    out, flag = g.sums(engine, b"".join(pts[:n]), s[:n], ranges)
    assert (out, flag) == expect(g, t[:n], s[:n], ranges)
    # scalars as bytes give the same
    assert g.sums(engine, b"".join(pts[:n]), b"".join(v.to_bytes(32, "big") for v in s[:n]), ranges) == (out, flag)


@pytest.mark.parametrize("deg", [1, 2])
def test_special_scalars_one_by_one(engine, worlds, deg):
    g, t, s, pts = worlds[deg]
    sc = SPECIAL * 3
    n = len(sc)
    ranges = [(i, i + 1) for i in range(n)] + [(0, 6), (0, n), (5, 13)]
    out, flag = g.sums(engine, b"".join(pts[40:40 + n]), sc, ranges)
    assert (out, flag) == expect(g, t[40:40 + n], sc, ranges)
    assert flag[0] == flag[3] == 1 and flag[1] == 0                          # 0 P and N P are infinity, 1 P is P
    assert out[g.size:2 * g.size] == pts[41]


@pytest.mark.parametrize("deg", [1, 2])
def test_off_curve_point_and_infinity_inputs(engine, worlds, deg):
    g, t, s, pts = worlds[deg]
    n = 70
    pts, t, s = list(pts[:n]), list(t[:n]), list(s[:n])
    bad = bytearray(pts[37])
    bad[-1] ^= 1                                             # y + 1 or y - 1: off the curve, not (0,0)
    pts[37] = bytes(bad)
    for i in (0, 15, 16, 31, 32, 69):                        # (0,0) inputs, first, last and at chunk boundaries
        pts[i], t[i] = bytes(g.size), 0
    for i in (44, 45):                                       # zero scalars
        s[i] = 0
    ranges = [(0, n), (0, 37), (37, 38), (38, n), (30, 50), (36, 38), (0, 38), (16, 33), (0, 1), (69, 70), (31, 33), (37, 37), (38, 38),
              (44, 46), (32, 40), (40, 48)]
    out, flag = g.sums(engine, b"".join(pts), s, ranges)
    t[37] = 0
    want, wflag = expect(g, t, s, ranges)
    holds = [b <= 37 < e for b, e in ranges]
    assert flag == bytes(2 if h else f for h, f in zip(holds, wflag))
    assert flag[ranges.index((44, 46))] == 1 and flag[ranges.index((0, 1))] == 1
    for j, h in enumerate(holds):
        assert out[g.size * j:g.size * (j + 1)] == (bytes(g.size) if h else want[g.size * j:g.size * (j + 1)])


@pytest.mark.parametrize("deg", [1, 2])
def test_equal_length_ranges_give_the_group_sums_bytes(engine, worlds, deg):
    g, t, s, pts = worlds[deg]
    for k, groups in ((1, 20), (3, 9), (8, 5), (9, 4), (67, 9)):
        buf = b"".join(pts[:k * groups])
        out, flag = g.sums(engine, buf, s[:k * groups], [(j * k, (j + 1) * k) for j in range(groups)])
        wout, winf = g.msm(buf, s[:k * groups], k, groups)
        assert out == wout and [f == 1 for f in flag] == list(winf), k


@pytest.mark.parametrize("deg", [1, 2])
def test_forty_points_against_the_oracle(engine, oracle, worlds, deg):
    g, t, s, pts = worlds[deg]
    buf = b"".join(pts[:40])
    out, flag = g.sums(engine, buf, s[:40], [(0, 40), (0, 17), (17, 40)])
    ofn = oracle.g1_msm if deg == 1 else oracle.g2_msm
    for j, (b, e) in enumerate(((0, 40), (0, 17), (17, 40))):
        wout, winf = ofn(buf[g.size * b:g.size * e], s[b:e], e - b)
        assert out[g.size * j:g.size * (j + 1)] == wout and (flag[j] == 1) == bool(winf)


@pytest.mark.parametrize("deg", [1, 2])
def test_einval_leaves_the_outputs_untouched(engine, worlds, deg):
    g, t, s, pts = worlds[deg]
    n, lib, h = 10, engine.lib, engine.h
    buf, sc = b"".join(pts[:n]), b"".join(v.to_bytes(32, "big") for v in s[:n])
    fn = getattr(lib, g.name)
    out, flag = ctypes.create_string_buffer(b"\xee" * (2 * g.size), 2 * g.size), ctypes.create_string_buffer(b"\xee" * 2, 2)
    arr = lambda *v: (ctypes.c_uint32 * len(v))(*v)
    for rg in (arr(0, 3, 5, 4), arr(0, 3, 2, 11), arr(11, 11, 0, 1)):
        assert fn(h, buf, sc, n, rg, 2, out, flag) == -22 and lib.blsgpu_last_error()
        assert out.raw == b"\xee" * (2 * g.size) and flag.raw == b"\xee" * 2
    ok = arr(0, 3, 2, 10)
    for args in ((None, sc, n, ok, 2, out, flag), (buf, None, n, ok, 2, out, flag), (buf, sc, n, None, 2, out, flag),
                 (buf, sc, n, ok, 2, None, flag), (buf, sc, n, ok, 2, out, None)):
        assert fn(h, *args) == -22
    assert out.raw == b"\xee" * (2 * g.size) and flag.raw == b"\xee" * 2
    assert fn(h, buf, sc, n, ok, 0, out, flag) == 0 and out.raw == b"\xee" * (2 * g.size)
    # no points at all: every range is empty and gives infinity
    assert fn(h, None, None, 0, arr(0, 0, 0, 0), 2, out, flag) == 0
    assert out.raw == bytes(2 * g.size) and flag.raw == b"\x01\x01"
    assert fn(h, buf, sc, n, ok, 2, out, flag) == 0
    assert (out.raw, flag.raw) == g.sums(engine, buf, s[:n], [(0, 3), (2, 10)]) == expect(g, t[:n], s[:n], [(0, 3), (2, 10)])


@pytest.mark.parametrize("deg", [1, 2])
def test_dev_form_and_workspace(engine, worlds, deg):
    import torch
    from bls_py import _native
    g, t, s, pts = worlds[deg]
    n = 300
    ranges = ranges_for(n)
    m = len(ranges)
    buf, sc = b"".join(pts[:n]), b"".join(v.to_bytes(32, "big") for v in s[:n])
    host = g.sums(engine, buf, sc, ranges)
    # a context of its own: tables, partials and prefix records count in the total (net of the host form's staging), once
    fresh = _native.Engine(0)
    try:
        before = fresh.workspace_bytes()
        assert g.sums(fresh, buf, sc, ranges) == host
        first = fresh.workspace_bytes()
        grown = (first["total"] - before["total"]) - (first["staging"] - before["staging"])
        chunks = sum(-(-(e - b) // 8) for b, e in ranges)
        assert grown >= min(chunks, 2048 * 64 // deg) * 8 * 16 * 168 * deg
        assert g.sums(fresh, buf, sc, ranges) == host and fresh.workspace_bytes() == first
    finally:
        fresh.close()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d_p, d_s, d_r = up(buf), up(sc), up(struct.pack("<%dI" % (2 * m), *[v for r in ranges for v in r]))
    d_o = torch.full((m * g.size,), 0xAA, dtype=torch.uint8, device=dev)
    d_f = torch.full((m,), 0xAA, dtype=torch.uint8, device=dev)
    g.sums_dev(engine, d_p.data_ptr(), d_s.data_ptr(), n, d_r.data_ptr(), m, d_o.data_ptr(), d_f.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert (bytes(d_o.cpu().numpy()), bytes(d_f.cpu().numpy())) == host
    # the _dev form checks the ranges on the device, before anything is written
    for bad in ((5, 4), (0, n + 1)):
        d_o.fill_(0xAA)
        d_f.fill_(0xAA)
        d_b = up(struct.pack("<%dI" % (2 * m), *[v for r in ranges[:-1] + [bad] for v in r]))
        with pytest.raises(_native.BlsGpuError, match="-22"):
            g.sums_dev(engine, d_p.data_ptr(), d_s.data_ptr(), n, d_b.data_ptr(), m, d_o.data_ptr(), d_f.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert bytes(d_o.cpu().numpy()) == b"\xaa" * (m * g.size) and bytes(d_f.cpu().numpy()) == b"\xaa" * m
