"""blsgpu_g1_mul_short / blsgpu_g2_mul_short on the device: the bytes of blsgpu_g1_msm / blsgpu_g2_msm(k = 1, groups = n) on
the weights zero-extended to 32 bytes -- at the wavefront and lane-pair tails, with edge weights, infinity and the generator
among random subgroup points --, a handful of entries against the CPU oracle's scalar multiplication as well, out_inf against
the bytes, n == 0 and NULL buffers, and the _dev forms."""
import ctypes
import random

import pytest

from bls_py import _native_find as F
from bls_py import hostmath as H

pytestmark = pytest.mark.gpu

EDGE = [0, 1, 15, 16, 1 << 63, (1 << 64) - 1, 0x00000000ffffffff, 0xffff0000ffff0f0f, 0xfffffffffffffff0, 0x1234567800000000]
SIZES = {1: [1, 63, 64, 65, 129], 2: [1, 31, 32, 33, 65]}
PSZ = {1: 96, 2: 192}
NMAX = 129


@pytest.fixture(scope="module")
def pool(engine):
    """per group NMAX points (random subgroup points with (0,0) and the generator among them), NMAX weights (the edge weights
    mixed with random ones) and the reference bytes of the msm call on the zero-extended weights, computed once"""
    rng = random.Random(0x6d756c73)
    g1 = engine.g1_mul_gen([rng.randrange(1, H.N) for _ in range(NMAX)], aff=True, ser=False)[0]
    g2 = engine.hash_to_g2(b"".join(rng.getrandbits(256).to_bytes(32, "big") for _ in range(NMAX)))
    out = {}
    for deg, pts, gen in ((1, g1, H.g1_affine_bytes(H.G1_GEN)), (2, g2, H.g2_affine_bytes(H.G2_GEN))):
        sz = PSZ[deg]
        p = [pts[sz * i:sz * (i + 1)] for i in range(NMAX)]
        p[0] = gen                                        # n = 1 multiplies the generator
        for i in (3, 30, 62, 64, 128):
            p[i] = bytes(sz)
        p[31], p[63] = gen, gen
        w = [rng.getrandbits(64) for _ in range(NMAX)]
        for j, e in enumerate(EDGE):
            w[(2 * j + 1) % NMAX] = e                     # 1, 3 (an infinity point), 5, ...
        w[0], w[64], w[128] = (1 << 64) - 1, 5, 1 << 63
        w[32], w[33] = 0, 16
        msm = engine.g1_msm if deg == 1 else engine.g2_msm
        ref, ref_inf = msm(b"".join(p), w, 1, NMAX)
        out[deg] = (p, w, ref, ref_inf)
    return out


def mul_short(engine, deg, pts, w):
    return (F.g1_mul_short if deg == 1 else F.g2_mul_short)(engine, pts, w)


@pytest.mark.parametrize("deg,n", [(d, n) for d in (1, 2) for n in SIZES[d]])
def test_bytes_of_the_msm_call(engine, pool, deg, n):
    p, w, ref, ref_inf = pool[deg]
    sz = PSZ[deg]
    # the first n and the last n of the pool: every size meets infinity points, the generator and edge weights
    for lo in (0, NMAX - n):
        got, inf = mul_short(engine, deg, b"".join(p[lo:lo + n]), w[lo:lo + n])
        assert got == ref[sz * lo:sz * (lo + n)]
        assert inf == ref_inf[lo:lo + n]
        assert inf == [not any(got[sz * i:sz * (i + 1)]) for i in range(n)]
        for i in range(n):
            if w[lo + i] == 0 or not any(p[lo + i]):
                assert inf[i]


def test_against_the_oracle(engine, pool, oracle):
    for deg in (1, 2):
        p, w, ref, _ = pool[deg]
        sz = PSZ[deg]
        mul = oracle.g1_msm if deg == 1 else oracle.g2_msm
        for i in (0, 1, 5, 31, 32, 64, 127, 128):
            want, want_inf = mul(p[i], [w[i]], 1)
            got, inf = mul_short(engine, deg, p[i], [w[i]])
            assert got == ref[sz * i:sz * (i + 1)] and inf == [want_inf], (deg, i)
            assert got == (bytes(sz) if want_inf else want), (deg, i)
    # and hostmath: 2^63 times the generator of G1
    got, _ = F.g1_mul_short(engine, H.g1_affine_bytes(H.G1_GEN), [1 << 63])
    assert got == H.g1_affine_bytes(H.jac_to_affine(H.F1, H.jac_mul(H.F1, H.aff_to_jac(H.F1, H.G1_GEN), 1 << 63)))


def test_empty_and_null(engine, pool):
    lib, h = engine.lib, engine.h
    for deg, name in ((1, "blsgpu_g1_mul_short"), (2, "blsgpu_g2_mul_short")):
        p, w, ref, _ = pool[deg]
        sz = PSZ[deg]
        fn = getattr(lib, name)
        pts, wb = b"".join(p[:3]), b"".join(x.to_bytes(8, "big") for x in w[:3])
        out = ctypes.create_string_buffer(b"\xee" * (3 * sz), 3 * sz)
        inf = ctypes.create_string_buffer(b"\xee" * 3, 3)
        assert fn(h, pts, wb, 0, out, inf) == 0 and out.raw == b"\xee" * (3 * sz) and inf.raw == b"\xee" * 3
        assert fn(h, None, None, 0, None, None) == 0
        for args in ((None, wb, 3, out, inf), (pts, None, 3, out, inf), (pts, wb, 3, None, inf)):
            assert fn(h, *args) == -22
            assert out.raw == b"\xee" * (3 * sz) and inf.raw == b"\xee" * 3
        assert fn(h, pts, wb, 3, out, None) == 0 and out.raw == ref[:3 * sz]      # out_inf may be NULL
        assert fn(None, pts, wb, 3, out, inf) == -22


@pytest.mark.parametrize("deg", [1, 2])
def test_dev_forms(engine, pool, deg):
    import torch
    p, w, ref, ref_inf = pool[deg]
    sz = PSZ[deg]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    dev_fn = F.g1_mul_short_dev if deg == 1 else F.g2_mul_short_dev
    fn = lambda *a: dev_fn(engine, *a)
    for n in (SIZES[deg][-2], SIZES[deg][-1]):
        d_p = torch.frombuffer(bytearray(b"".join(p[:n])), dtype=torch.uint8).to(dev)
        d_w = torch.frombuffer(bytearray(b"".join(x.to_bytes(8, "big") for x in w[:n])), dtype=torch.uint8).to(dev)
        d_out = torch.full((n * sz,), 0xAA, dtype=torch.uint8, device=dev)
        d_inf = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
        fn(d_p.data_ptr(), d_w.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert bytes(d_out.cpu().numpy()) == ref[:n * sz]
        assert [b != 0 for b in bytes(d_inf.cpu().numpy())] == ref_inf[:n]
        d_out.fill_(0xAA)
        fn(d_p.data_ptr(), d_w.data_ptr(), n, d_out.data_ptr(), None, stream.cuda_stream)
        stream.synchronize()
        assert bytes(d_out.cpu().numpy()) == ref[:n * sz]
    fn(None, None, 0, None, None, stream.cuda_stream)                              # n == 0: nothing to do
    with pytest.raises(Exception, match="-22"):
        fn(None, d_w.data_ptr(), 3, d_out.data_ptr(), None, stream.cuda_stream)
