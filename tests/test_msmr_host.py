"""The g1_msm_ranges extension without a GPU: a recording host provider (tests/subgroup_vectors.HostRLC) that offers it, its ragged
sums computed on Python integers (bls_py.hostmath), against the padded group sums; that bls.py -- which is NOT routed through
the extension, the ragged call having measured slower than the per-length-class calls -- takes exactly the calls it took; and
the argument validation of bls_py._native_msmr."""
import random

import pytest

from subgroup_vectors import HostRLC, N, secret_keys


def host_msm_ranges(pts, scalars, ranges):
    """(affine bytes, flag bytes) of sum scalars[i] pts[i] over every range, by double-and-add on integers"""
    from bls_py import hostmath as H
    if isinstance(scalars, (bytes, bytearray)):
        scalars = [int.from_bytes(scalars[32 * i:32 * (i + 1)], "big") for i in range(len(scalars) // 32)]
    assert len(pts) == 96 * len(scalars)
    out, flag = b"", []
    for b, e in ranges:
        acc = None
        for i in range(b, e):
            A = H.g1_from_abi(pts[96 * i:96 * (i + 1)])
            if A is not None:
                acc = H.jac_add(H.F1, acc, H.jac_mul(H.F1, H.aff_to_jac(H.F1, A), int(scalars[i])))
        A = None if acc is None else H.jac_to_affine(H.F1, acc)
        out += bytes(96) if A is None else H.g1_affine_bytes(A)
        flag.append(1 if A is None else 0)
    return out, bytes(flag)


class WithExtension(HostRLC):
    """a stand-in that offers the extension as a stand-in does: an attribute of that name"""

    def g1_msm_ranges(self, pts, scalars, ranges):
        self.calls.append(("g1_msm_ranges", len(pts) // 96, list(ranges)))
        return host_msm_ranges(pts, scalars, ranges)


@pytest.fixture
def use(oracle):
    from bls_py import backend
    old = backend._provider

    def install(cls):
        p = cls(oracle)
        backend.use(p)
        return p
    yield install
    backend.use(old)


@pytest.fixture(scope="module")
def world(oracle):
    """a ragged aggregate (one message with 4 signers, three with 1: secure-aggregation exponents in the tree), a forged
    copy of it, and a uniform aggregate (two messages of 2 signers)"""
    from bls_py import backend
    from bls_py.bls import BLS
    old = backend._provider
    backend.use(HostRLC(oracle))
    try:
        sks = secret_keys(b"ragged", 7)
        ragged = BLS.aggregate_sigs([sk.sign(b"shared") for sk in sks[:4]] + [sk.sign(b"own%d" % i) for i, sk in enumerate(sks[4:])])
        sigs = [sk.sign(b"shared") for sk in sks[:4]] + [sk.sign(b"own%d" % i) for i, sk in enumerate(sks[4:])]
        sigs[1] = sks[1].sign(b"other")
        forged = BLS.aggregate_sigs_simple(sigs)
        forged.set_aggregation_info(ragged.aggregation_info)
        uniform = BLS.aggregate_sigs([sks[0].sign(b"u0"), sks[1].sign(b"u0"), sks[2].sign(b"u1"), sks[3].sign(b"u1")])
        return ragged, forged, uniform
    finally:
        backend.use(old)


def sums(p):
    return [c[:3] for c in p.calls if c[0] in ("g1_msm_ranges", "g1_msm")]


def test_the_extension_is_found_and_gives_the_padded_sums(use, world):
    """the per-message key sums of a ragged aggregate through the extension -- the groups concatenated, one range each -- are
    the sums the padded g1_msm call gives"""
    from bls_py import backend, hostmath as H
    ragged = world[0]
    info = ragged.aggregation_info
    by_message = {}
    for mh, pk in zip(info.message_hashes, info.public_keys):
        by_message.setdefault(mh, []).append(pk)
    assert sorted(len(v) for v in by_message.values()) == [1, 1, 1, 4]
    p = use(WithExtension)
    fn = backend.extension("g1_msm_ranges")
    assert fn is not None and backend.extension("g2_msm_ranges") is None
    pts, sc, ranges, pad_p, pad_s = b"", [], [], b"", []
    for mh, keys in by_message.items():
        kb = [H.g1_affine_bytes(pk.value.to_affine()._aff()) for pk in keys]
        e = [int(info.tree[(mh, pk)]) for pk in keys]
        ranges.append((len(sc), len(sc) + len(keys)))
        pts, sc = pts + b"".join(kb), sc + e
        pad_p, pad_s = pad_p + b"".join(kb) + bytes(96) * (4 - len(keys)), pad_s + e + [0] * (4 - len(keys))
    out, flag = fn(pts, sc, ranges)
    wout, winf = p.g1_msm(pad_p, pad_s, 4, 4)
    assert out == wout and [f == 1 for f in flag] == [bool(i) for i in winf]
    assert fn(pts, b"".join(v.to_bytes(32, "big") for v in sc), ranges) == (out, flag)
    use(HostRLC)
    assert backend.extension("g1_msm_ranges") is None


def test_bls_takes_exactly_the_calls_it_took(use, world):
    """the ragged call measured slower than the per-length-class calls on the skewed shape (profiles/msm_ranges_probe.txt), so
    bls.py is not routed through it: with the extension present BLS.verify, verify_batch, verify_batch_randomized and
    _g1_group_sums make the calls, and give the answers, of a provider without it"""
    from bls_py.bls import BLS, _g1_group_sums
    ragged, forged, uniform = world
    batch = [ragged, forged, uniform]
    seen = []
    for cls in (HostRLC, WithExtension):
        p = use(cls)
        got = [BLS.verify(s) for s in batch], BLS.verify_batch(batch), BLS.verify_batch_randomized(batch, rng=random.Random(3))
        assert got == ([True, False, True],) * 3
        seen.append(sums(p))
    assert seen[0] == seen[1] and ("g1_msm", 4, 4) in seen[0] and all(c[0] == "g1_msm" for c in seen[1])
    p = use(WithExtension)
    from bls_py import hostmath as H
    pts = [H.g1_affine_bytes(H.jac_to_affine(H.F1, H.jac_mul(H.F1, H.aff_to_jac(H.F1, H.G1_GEN), k + 2))) for k in range(6)]
    groups = [[(pts[0], 5), (pts[1], 7)], [(pts[2], 1), (pts[3], 2), (pts[4], N - 1)], [(pts[5], 0)]]
    res = _g1_group_sums(p, groups)
    assert sorted(sums(p)) == [("g1_msm", 1, 1), ("g1_msm", 2, 1), ("g1_msm", 4, 1)]
    out, flag = p.g1_msm_ranges(b"".join(b for g in groups for b, _ in g), [s for g in groups for _, s in g], [(0, 2), (2, 5), (5, 6)])
    assert [r[0] for r in res] == [out[96 * j:96 * (j + 1)] for j in range(3)] and [bool(r[1]) for r in res] == [f == 1 for f in flag]


class FakeEngine:
    """_native.Engine's marshalling helpers over a device call that must not happen"""

    def __init__(self):
        from bls_py import _native
        self._scalars, self._indices = _native.Engine._scalars, _native.Engine._indices
        self.calls = []

    def _call_out(self, name, *args, out, tail=()):
        self.calls.append((name, args[2], args[4], out))
        return [bytes(size) for size in out]

    def _call(self, name, *args):
        self.calls.append((name,) + args)


def test_argument_validation_raises_before_any_device_call():
    from bls_py import _native_msmr as R
    eng = FakeEngine()
    for fn, psz in ((R.g1_msm_ranges, 96), (R.g2_msm_ranges, 192)):
        pts = bytes(psz * 3)
        with pytest.raises(ValueError):
            fn(eng, pts[:-1], [1, 2, 3], [(0, 3)])                           # not whole points
        with pytest.raises(ValueError):
            fn(eng, pts, [1, 2], [(0, 3)])                                   # a scalar per point
        with pytest.raises(ValueError):
            fn(eng, pts, bytes(95), [(0, 3)])
        with pytest.raises(ValueError):
            fn(eng, pts, [1, 2, 1 << 256], [(0, 3)])                         # scalars are 256-bit
        with pytest.raises(ValueError):
            fn(eng, pts, [1, 2, -1], [(0, 3)])
        with pytest.raises(ValueError):
            fn(eng, pts, [1, 2, 3], [(0, 3), (1,)])                          # a range is a pair
        with pytest.raises(OverflowError):
            fn(eng, pts, [1, 2, 3], [(0, 1 << 32)])                          # 32-bit indices
        assert eng.calls == []
        out, flag = fn(eng, pts, [1, 2, (1 << 256) - 1], [(0, 3), (1, 1)])
        assert len(out) == 2 * psz and len(flag) == 2
        out, flag = fn(eng, pts, bytes(96), [])
        assert (out, flag) == (b"", b"")
        assert [c[1:3] for c in eng.calls] == [(3, 2), (3, 0)]
        eng.calls.clear()
    R.g1_msm_ranges_dev(eng, 1, 2, 3, 4, 5, 6, 7)
    R.g2_msm_ranges_dev(eng, 1, 2, 3, 4, 5, 6, 7, stream=9)
    assert eng.calls == [("blsgpu_g1_msm_ranges_dev", 1, 2, 3, 4, 5, 6, 7, 0), ("blsgpu_g2_msm_ranges_dev", 1, 2, 3, 4, 5, 6, 7, 9)]
