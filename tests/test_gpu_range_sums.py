"""blsgpu_g1_range_sums / blsgpu_g2_range_sums on the device.  The points are s_i G1 (g1_mul_gen) and s_i H(m) (blsgpu_sign with
one message), so the expected sum of a range is the SINGLE multiplication by sum s_i mod n from the same calls, compared byte
for byte: no curve arithmetic on the host.  Sizes around a chunk (16 points) and around one middle workgroup's worth of chunks
(128 x 16 = 2048 points); empty, single, whole, overlapping and repeated ranges and one ending at every chunk boundary; sums at
infinity, equal neighbours, (0,0) inputs, a point off the curve; the plain group sums' bytes; -EINVAL; the _dev form; workspace."""
import ctypes
import hashlib
import random
import struct

import pytest

from bls_py import _native_ranges as R
from bls_py import hostmath as H

pytestmark = pytest.mark.gpu

N = H.N
TOP = 2065
CHUNK, MID = 16, 128
SIZES = [1, 2, 15, 16, 17, 63, 64, 65, CHUNK * MID - 1, CHUNK * MID, CHUNK * MID + 1, TOP]
MSG = hashlib.sha256(b"range sums").digest()


class Group:
    def __init__(self, engine, deg):
        self.deg, self.size, self.engine = deg, 96 * deg, engine
        self.sums = R.g1_range_sums if deg == 1 else R.g2_range_sums
        self.sums_dev = R.g1_range_sums_dev if deg == 1 else R.g2_range_sums_dev
        self.name = "blsgpu_g%d_range_sums" % deg

    def mul(self, scalars):
        """s G for every scalar ((0,0) for 0), one call"""
        e = self.engine
        out = e.g1_mul_gen(scalars, aff=True, ser=False)[0] if self.deg == 1 else e.sign(scalars, MSG, aff=True, ser=False)[0]
        return [out[self.size * i:self.size * (i + 1)] for i in range(len(scalars))]

    def msm(self, pts, k, groups):
        return (self.engine.g1_msm if self.deg == 1 else self.engine.g2_msm)(pts, None, k, groups)


@pytest.fixture(scope="module")
def worlds(engine):
    """per group: TOP scalars with the special neighbours planted, their points, and the inputs' bytes"""
    out = {}
    for deg in (1, 2):
        rng = random.Random("range sums %d" % deg)
        s = [rng.randrange(1, N) for _ in range(TOP)]
        s[5] = N - s[4]                                      # P then -P: the range [4, 6) sums to infinity
        s[9] = s[8]                                          # equal neighbours
        s[11] = 0                                            # an input at infinity
        s[40] = (-sum(s[33:40])) % N                         # [33, 41) sums to infinity across a chunk boundary
        g = Group(engine, deg)
        pts = g.mul(s)
        assert pts[11] == bytes(g.size) and pts[8] == pts[9]
        out[deg] = (g, s, pts)
    return out


def ranges_for(n):
    rng = random.Random(n)
    r = [(0, 0), (n, n), (0, n), (0, 1), (n - 1, n), (0, n), (n // 2, n // 2)]
    r += [(min(4, n), min(6, n)), (min(8, n), min(10, n)), (min(11, n), min(12, n)), (min(33, n), min(41, n)), (min(3, n), min(12, n))]
    r += [(0, e) for e in range(0, n + 1, CHUNK)] + [(max(0, e - 3), e) for e in range(CHUNK, n + 1, CHUNK)]
    r += [tuple(sorted((rng.randrange(n + 1), rng.randrange(n + 1)))) for _ in range(24)]
    return r


def expect(g, s, ranges):
    """(bytes, flags) from ONE multiplication per range by the sum of its scalars"""
    want = g.mul([sum(s[b:e]) % N for b, e in ranges])
    return b"".join(want), bytes(1 if not any(w) else 0 for w in want)


@pytest.mark.parametrize("deg", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_ranges(engine, worlds, deg, n):
    g, s, pts = worlds[deg]
    ranges = ranges_for(n)
    out, flag = g.sums(engine, b"".join(pts[:n]), ranges)
    want, wflag = expect(g, s[:n], ranges)
    assert flag == wflag
    assert out == want
    if n >= 41:
        assert flag[ranges.index((4, 6))] == 1 and flag[ranges.index((33, 41))] == 1 and flag[0] == 1


@pytest.mark.parametrize("deg", [1, 2])
def test_off_curve_point_and_infinity_inputs(engine, worlds, deg):
    g, s, pts = worlds[deg]
    n = 70
    pts, s = list(pts[:n]), list(s[:n])
    bad = bytearray(pts[37])
    bad[-1] ^= 1                                             # y + 1 or y - 1: off the curve, not (0,0)
    pts[37] = bytes(bad)
    for i in (0, 16, 31, 32, 69):                            # (0,0) inputs, first, last and at chunk boundaries
        pts[i], s[i] = bytes(g.size), 0
    ranges = [(0, n), (0, 37), (37, 38), (38, n), (30, 50), (36, 38), (0, 38), (16, 33), (0, 1), (69, 70), (31, 33), (37, 37), (38, 38)]
    out, flag = g.sums(engine, b"".join(pts), ranges)
    s[37] = 0
    want, wflag = expect(g, s, ranges)
    holds = [b <= 37 < e for b, e in ranges]
    assert flag == bytes(2 if h else f for h, f in zip(holds, wflag))
    for j, h in enumerate(holds):
        assert out[g.size * j:g.size * (j + 1)] == (bytes(g.size) if h else want[g.size * j:g.size * (j + 1)])


@pytest.mark.parametrize("deg", [1, 2])
def test_equal_length_ranges_give_the_group_sums_bytes(engine, worlds, deg):
    g, s, pts = worlds[deg]
    for k, groups in ((1, 20), (7, 9), (16, 4), (33, 3)):
        buf = b"".join(pts[:k * groups])
        out, flag = g.sums(engine, buf, [(j * k, (j + 1) * k) for j in range(groups)])
        wout, winf = g.msm(buf, k, groups)
        assert out == wout and [f == 1 for f in flag] == list(winf)


@pytest.mark.parametrize("deg", [1, 2])
def test_einval_leaves_the_outputs_untouched(engine, worlds, deg):
    g, s, pts = worlds[deg]
    n, lib, h = 10, engine.lib, engine.h
    buf = b"".join(pts[:n])
    fn = getattr(lib, g.name)
    out, flag = ctypes.create_string_buffer(b"\xee" * (2 * g.size), 2 * g.size), ctypes.create_string_buffer(b"\xee" * 2, 2)
    arr = lambda *v: (ctypes.c_uint32 * len(v))(*v)
    for rg in (arr(0, 3, 5, 4), arr(0, 3, 2, 11), arr(11, 11, 0, 1)):
        assert fn(h, buf, n, rg, 2, out, flag) == -22 and lib.blsgpu_last_error()
        assert out.raw == b"\xee" * (2 * g.size) and flag.raw == b"\xee" * 2
    ok = arr(0, 3, 2, 10)
    for args in ((None, n, ok, 2, out, flag), (buf, n, None, 2, out, flag), (buf, n, ok, 2, None, flag), (buf, n, ok, 2, out, None)):
        assert fn(h, *args) == -22
    assert out.raw == b"\xee" * (2 * g.size) and flag.raw == b"\xee" * 2
    assert fn(h, buf, n, ok, 0, out, flag) == 0 and out.raw == b"\xee" * (2 * g.size)
    # no points at all: every range is empty and gives infinity
    assert fn(h, None, 0, arr(0, 0, 0, 0), 2, out, flag) == 0
    assert out.raw == bytes(2 * g.size) and flag.raw == b"\x01\x01"
    assert fn(h, buf, n, ok, 2, out, flag) == 0
    assert (out.raw, flag.raw) == g.sums(engine, buf, [(0, 3), (2, 10)]) == expect(g, s[:n], [(0, 3), (2, 10)])


@pytest.mark.parametrize("deg", [1, 2])
def test_dev_form_and_workspace(engine, worlds, deg):
    import torch
    from bls_py import _native
    g, s, pts = worlds[deg]
    n = 300
    ranges = ranges_for(n)
    m = len(ranges)
    buf = b"".join(pts[:n])
    host = g.sums(engine, buf, ranges)
    # a context of its own: the prefix records count in the total (net of the staging of the host-buffer form), once
    fresh = _native.Engine(0)
    try:
        before = fresh.workspace_bytes()
        assert g.sums(fresh, buf, ranges) == host
        first = fresh.workspace_bytes()
        grown = (first["total"] - before["total"]) - (first["staging"] - before["staging"])
        assert grown >= (n + 1) * 168 * deg
        assert g.sums(fresh, buf, ranges) == host and fresh.workspace_bytes() == first
    finally:
        fresh.close()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d_p, d_r = up(buf), up(struct.pack("<%dI" % (2 * m), *[v for r in ranges for v in r]))
    d_o = torch.full((m * g.size,), 0xAA, dtype=torch.uint8, device=dev)
    d_f = torch.full((m,), 0xAA, dtype=torch.uint8, device=dev)
    g.sums_dev(engine, d_p.data_ptr(), n, d_r.data_ptr(), m, d_o.data_ptr(), d_f.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert (bytes(d_o.cpu().numpy()), bytes(d_f.cpu().numpy())) == host
    # the _dev form scans the ranges on the device
    for bad in ((5, 4), (0, n + 1)):
        d_o.fill_(0xAA)
        d_f.fill_(0xAA)
        d_b = up(struct.pack("<%dI" % (2 * m), *[v for r in ranges[:-1] + [bad] for v in r]))
        with pytest.raises(_native.BlsGpuError, match="-22"):
            g.sums_dev(engine, d_p.data_ptr(), n, d_b.data_ptr(), m, d_o.data_ptr(), d_f.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert bytes(d_o.cpu().numpy()) == b"\xaa" * (m * g.size) and bytes(d_f.cpu().numpy()) == b"\xaa" * m
