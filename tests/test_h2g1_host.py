"""Hash to G1 without a GPU: the host arithmetic against tests/golden/hash_to_g1.json (written from the reference by
tests/golden/make_golden_h2g1.py), the batch forms ec.hash_to_points_prehashed_Fq / hash_to_points_Fq over a stand-in provider
built on that host arithmetic, and the four entry points in the header, the prototype table and the built library."""
import os

import pytest

from bls_py import bls12381 as C
from bls_py import backend, ec
from bls_py import hostmath as H
from bls_py.util import hash256, hash512
from conftest import ROOT, load_golden

Q = C.q
ENTRY_POINTS = ("blsgpu_map_to_g1", "blsgpu_map_to_g1_dev", "blsgpu_hash_to_g1", "blsgpu_hash_to_g1_dev")


@pytest.fixture(scope="module")
def fx():
    return load_golden("hash_to_g1.json")


def num(h):
    return int(h, 16)


def candidates(t):
    """x1, x2, x3 of ec.py:475-485"""
    w = H.fq_inv((t * t + 5) % Q) * C.sqrt_n3 * t % Q
    x1 = (-w * t + C.sqrt_n3m1o2) % Q
    return [x1, (-1 - x1) % Q, (H.fq_inv(w * w % Q) + 1) % Q]


def test_fixture_shape(fx):
    """what the generator promises: the edge t first, every candidate index taken three times, 70 hashes, the first the
    vector hash_to_curve.json has carried since round 1"""
    sw = fx["sw_encode"]
    r5 = [num(r["t"]) for r in sw[5:7]]
    assert [num(r["t"]) for r in sw[:5]] == [0, 1, 2, Q - 1, Q - 2]
    assert all(r * r % Q == Q - 5 for r in r5) and r5[0] == Q - r5[1]
    for idx in (0, 1, 2):
        assert sum(1 for r in sw if r["index"] == idx) >= 3
    assert [r["index"] is None for r in sw] == [True, False, False, False, False, True, True] + [False] * (len(sw) - 7)
    assert len(fx["hash"]) == 70 and len(fx["map"]) >= 32 + len(sw) + 6
    assert fx["hash"][0]["msg_hash"] == hash256(b"").hex()
    assert fx["hash"][0]["point"] == load_golden("hash_to_curve.json")["hash_to_g1_empty"]["point"]
    kinds = {m["kind"] for m in fx["map"]}
    assert kinds == {"random", "t_zero", "zero_t", "zero_zero", "opposite", "equal", "root_t", "root_opposite"}
    assert all(m["inf"] == (m["point"] == "00" * 96) for m in fx["map"])


def test_sw_encode_every_record(fx):
    for r in fx["sw_encode"]:
        t = num(r["t"])
        A = H.sw_encode(H.F1, t)
        assert H.g1_affine_bytes(A).hex() == r["point"] and (A is None) == r["inf"], r["t"]
        if r["index"] is None:
            assert t == 0 or (t * t + 5) % Q == 0
        else:
            assert candidates(t)[r["index"]] == A[0], r["t"]


def host_map(t0, t1):
    P = H.jac_add(H.F1, H.aff_to_jac(H.F1, H.sw_encode(H.F1, t0)), H.aff_to_jac(H.F1, H.sw_encode(H.F1, t1)))
    return H.jac_to_affine(H.F1, H.jac_mul(H.F1, P, C.h))


def test_map_every_record(fx):
    for m in fx["map"]:
        A = host_map(num(m["t0"]), num(m["t1"]))
        assert H.g1_affine_bytes(A).hex() == m["point"] and H.g1_compress(A).hex() == m["ser"] and (A is None) == m["inf"], m["kind"]


def test_hash_every_record(fx):
    for r in fx["hash"]:
        h = bytes.fromhex(r["msg_hash"])
        A = H.hash_to_g1_prehashed(h, hash512)
        assert H.g1_affine_bytes(A).hex() == r["point"] and H.g1_compress(A).hex() == r["ser"]
        t = H.g1_hash_field_elements(h, hash512)
        assert host_map(int.from_bytes(t[:48], "big"), int.from_bytes(t[48:], "big")) == A


class StandIn:
    """hash_to_g1 / map_to_g1 with the results of bls_py._native_h2g1, on hostmath; records which was called with what"""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _out(points, aff, ser):
        return (b"".join(H.g1_affine_bytes(A) for A in points) if aff else None,
                b"".join(H.g1_compress(A) for A in points) if ser else None, [A is None for A in points])

    def hash_to_g1(self, msg_hashes, aff=True, ser=False):
        self.calls.append(("hash_to_g1", len(msg_hashes) // 32))
        assert len(msg_hashes) % 32 == 0
        return self._out([H.hash_to_g1_prehashed(msg_hashes[i:i + 32], hash512) for i in range(0, len(msg_hashes), 32)], aff, ser)

    def map_to_g1(self, t, aff=True, ser=False):
        self.calls.append(("map_to_g1", len(t) // 96))
        assert len(t) % 96 == 0
        return self._out([host_map(int.from_bytes(t[i:i + 48], "big"), int.from_bytes(t[i + 48:i + 96], "big"))
                          for i in range(0, len(t), 96)], aff, ser)


class InfinityStandIn(StandIn):
    """a provider that reports infinity for every message: what the batch form makes of the flag"""

    def hash_to_g1(self, msg_hashes, aff=True, ser=False):
        n = len(msg_hashes) // 32
        return bytes(96 * n), None, [True] * n


class Bare:
    """a provider without the extension"""


@pytest.fixture
def provider():
    old = backend._provider

    def install(p):
        backend.use(p)
        return p
    yield install
    backend.use(old)


def same_points(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert type(g) is type(w) is ec.AffinePoint and g == w and g.infinity == w.infinity and g.ec is w.ec


def test_batch_forms_equal_the_loop_and_route_by_length(fx, provider):
    p = provider(StandIn())
    hashes = [bytes.fromhex(r["msg_hash"]) for r in fx["hash"][:4]]
    same_points(ec.hash_to_points_prehashed_Fq(hashes), [ec.hash_to_point_prehashed_Fq(h) for h in hashes])
    assert p.calls == [("hash_to_g1", 4)]
    for got, r in zip(ec.hash_to_points_prehashed_Fq(hashes), fx["hash"]):
        assert H.g1_affine_bytes(got._aff()).hex() == r["point"] and got.serialize().hex() == r["ser"]
    # one message of another length sends the whole call to map_to_g1 with the host's field elements; str is utf-8
    p.calls.clear()
    mixed = [hashes[0], b"", "abc", b"x" * 33]
    same_points(ec.hash_to_points_prehashed_Fq(mixed), [ec.hash_to_point_prehashed_Fq(m) for m in mixed])
    assert p.calls == [("map_to_g1", 4)]
    p.calls.clear()
    msgs = [b"", b"one", b"two" * 40]
    same_points(ec.hash_to_points_Fq(msgs), [ec.hash_to_point_Fq(m) for m in msgs])
    assert p.calls == [("hash_to_g1", 3)]                    # hash256 gives 32 bytes
    p.calls.clear()
    assert ec.hash_to_points_prehashed_Fq([]) == [] and ec.hash_to_points_Fq([]) == [] and p.calls == []


def test_infinity_is_the_single_calls_object(provider):
    provider(InfinityStandIn())
    got = ec.hash_to_points_prehashed_Fq([bytes(32)])[0]
    want = ec.AffinePoint._from(H.F1, None, ec.default_ec)   # what hash_to_point_prehashed_Fq makes of an infinite sum
    assert type(got) is ec.AffinePoint and got.infinity and got == want and got.serialize() == want.serialize() == bytes(48)


def test_fallback_without_the_extension(fx, provider):
    provider(Bare())
    assert backend.extension("hash_to_g1") is None and backend.extension("map_to_g1") is None
    hashes = [bytes.fromhex(r["msg_hash"]) for r in fx["hash"][:2]]
    same_points(ec.hash_to_points_prehashed_Fq(hashes + [b"short"]), [ec.hash_to_point_prehashed_Fq(m) for m in hashes + [b"short"]])
    same_points(ec.hash_to_points_Fq([b"m"]), [ec.hash_to_point_Fq(b"m")])
    assert H.g1_affine_bytes(ec.hash_to_points_prehashed_Fq(hashes)[1]._aff()).hex() == fx["hash"][1]["point"]


def test_extension_table_and_binding():
    from bls_py import _native, _native_h2g1
    assert backend.H2G1_EXTENSIONS == {"map_to_g1": "_native_h2g1", "hash_to_g1": "_native_h2g1"}
    for name in backend.H2G1_EXTENSIONS:
        assert callable(getattr(_native_h2g1, name)) and callable(getattr(_native_h2g1, name + "_dev"))
        assert not hasattr(_native.Engine, name) and name not in backend.PROVIDER_METHODS
    p = backend.HipProvider.__new__(backend.HipProvider)     # (no engine is created)
    p._eng = object()
    old = backend._provider
    backend.use(p)
    try:
        fn = backend.extension("hash_to_g1")
        assert fn.func is _native_h2g1.hash_to_g1 and fn.args == (p._eng,)
        assert backend.extension("map_to_g1").func is _native_h2g1.map_to_g1
    finally:
        backend.use(old)


def test_marshalling_over_a_stub_engine():
    """what _native_h2g1 hands to the library: NULL for the output that is not asked for, lengths checked first"""
    from bls_py import _native_h2g1

    class Eng:
        def __init__(self):
            self.calls = []

        def _call_out(self, name, *args, out):
            self.calls.append((name, args, out))
            return [None if s is None else bytes(s) for s in out]

        _flags = staticmethod(lambda b: [c != 0 for c in b])
    e = Eng()
    assert _native_h2g1.hash_to_g1(e, bytes(64)) == (bytes(192), None, [False, False])
    assert _native_h2g1.map_to_g1(e, bytes(96), aff=False, ser=True) == (None, bytes(48), [False])
    assert e.calls == [("blsgpu_hash_to_g1", (bytes(64), 2), [192, None, 2]), ("blsgpu_map_to_g1", (bytes(96), 1), [None, 48, 1])]
    with pytest.raises(ValueError):
        _native_h2g1.hash_to_g1(e, bytes(33))
    with pytest.raises(ValueError):
        _native_h2g1.map_to_g1(e, bytes(95))
    with pytest.raises(ValueError):
        _native_h2g1.map_to_g1(e, bytes(96), aff=False, ser=False)


def test_header_prototypes_and_library():
    import ctypes

    from bls_py import _native
    from test_abi_and_host import header_declarations
    declared = header_declarations()
    host = ["pointer", "pointer", "size_t", "pointer", "pointer", "pointer"]
    for name in ENTRY_POINTS:
        assert tuple(declared[name]) == ("int", host + (["pointer"] if name.endswith("_dev") else [])), name
        assert name in _native.PROTOTYPES and name in _native.SYMBOLS
    lib = ctypes.CDLL(os.path.join(ROOT, "python-bls_amd", "csrc", "libblsgpu.so"))
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None
