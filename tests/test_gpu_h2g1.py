"""Hash to G1 on the device (blsgpu_map_to_g1 / blsgpu_hash_to_g1 and their _dev forms, csrc/blsgpu_h2g1.hip) against
tests/golden/hash_to_g1.json, the reference's own values (tests/golden/make_golden_h2g1.py): byte equality of the affine
points, the compressed points and the infinity flags.  Every record of the fixture is used: the `map` section whole and
its edge records one by one (it holds (t, 0) for every t of the `sw_encode` section -- the only way an encoding shows
through the ABI), the `hash` section at sizes around a wavefront and cycled across a block boundary."""
import ctypes

import pytest

from bls_py import _native, _native_h2g1, backend, ec
from bls_py import bls12381 as C
from bls_py import hostmath as H
from bls_py.util import hash512
from conftest import cat, engine_with_env, load_golden

pytestmark = pytest.mark.gpu
Q = C.q
BLOCK = 256                         # k_h2g1's workgroup


@pytest.fixture(scope="module")
def fx():
    return load_golden("hash_to_g1.json")


def want(records):
    return cat(r["point"] for r in records), cat(r["ser"] for r in records)


def t_bytes(records):
    return cat(r["t0"] + r["t1"] for r in records)


def fe(v):
    return int(v).to_bytes(48, "big")


def test_map_section_in_one_call(engine, fx):
    recs = fx["map"]
    aff, ser, inf = _native_h2g1.map_to_g1(engine, t_bytes(recs), aff=True, ser=True)
    assert (aff, ser) == want(recs) and inf == [r["inf"] for r in recs]
    # (t, 0) is h sw_encode(t): every record of the sw_encode section is among them
    zero = {r["t0"] for r in recs if r["kind"] == "t_zero"}
    assert {r["t"] for r in fx["sw_encode"]} == zero


def test_map_edge_records_one_at_a_time(engine, fx):
    edge = [r for r in fx["map"] if r["kind"] != "random"]
    assert len(edge) == len(fx["sw_encode"]) + 6
    for r in edge:
        aff, ser, inf = _native_h2g1.map_to_g1(engine, t_bytes([r]), aff=True, ser=True)
        assert (aff, ser) == want([r]) and inf == [r["inf"]], r["kind"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 70])
def test_hash_section(engine, fx, n):
    recs = fx["hash"][:n]
    aff, ser, inf = _native_h2g1.hash_to_g1(engine, cat(r["msg_hash"] for r in recs), aff=True, ser=True)
    assert (aff, ser) == want(recs) and inf == [False] * n


def test_hash_across_a_block_boundary(engine, fx):
    n = 4 * BLOCK + 1
    recs = [fx["hash"][i % 70] for i in range(n)]
    aff, ser, inf = _native_h2g1.hash_to_g1(engine, cat(r["msg_hash"] for r in recs), aff=True, ser=True)
    assert (aff, ser) == want(recs) and not any(inf)


def test_hash_equals_map_of_the_host_field_elements(engine, fx):
    hashes = [bytes.fromhex(r["msg_hash"]) for r in fx["hash"]]
    t = b"".join(H.g1_hash_field_elements(h, hash512) for h in hashes)
    assert _native_h2g1.map_to_g1(engine, t, aff=True, ser=True) == _native_h2g1.hash_to_g1(engine, b"".join(hashes), aff=True, ser=True)


def test_field_elements_are_taken_mod_q(engine, fx):
    other = int(fx["map"][0]["t1"], 16)
    top = (1 << 384) - 1
    pairs = [(Q, 0), (Q + 1, 1), (top, top % Q)]
    big = b"".join(fe(a) + fe(other) + fe(other) + fe(a) + fe(a) + fe(a) for a, _ in pairs)
    red = b"".join(fe(b) + fe(other) + fe(other) + fe(b) + fe(b) + fe(b) for _, b in pairs)
    got = _native_h2g1.map_to_g1(engine, big, aff=True, ser=True)
    assert got == _native_h2g1.map_to_g1(engine, red, aff=True, ser=True)
    # ... and those are the host's values: (q, other) is (0, other), (q, q) is (0, 0) = infinity
    from test_h2g1_host import host_map
    pts = [host_map(int.from_bytes(red[i:i + 48], "big"), int.from_bytes(red[i + 48:i + 96], "big")) for i in range(0, len(red), 96)]
    assert got == (b"".join(H.g1_affine_bytes(A) for A in pts), b"".join(H.g1_compress(A) for A in pts), [A is None for A in pts])
    assert got[2][2] and not got[2][0]


def test_outputs_and_arguments(engine, fx):
    recs = fx["map"][30:40]                                 # random pairs and edge records
    t, n = t_bytes(recs), 10
    aff, ser = want(recs)
    assert _native_h2g1.map_to_g1(engine, t, aff=True, ser=False)[:2] == (aff, None)
    assert _native_h2g1.map_to_g1(engine, t, aff=False, ser=True)[:2] == (None, ser)
    lib, h = engine.lib, engine.h
    for name, data in (("blsgpu_map_to_g1", t), ("blsgpu_hash_to_g1", cat(r["msg_hash"] for r in fx["hash"][:n]))):
        fn = getattr(lib, name)
        exp = (aff, ser) if name == "blsgpu_map_to_g1" else want(fx["hash"][:n])
        a, s, f = (ctypes.create_string_buffer(b"\xaa" * k, k) for k in (96 * n, 48 * n, n))
        assert fn(h, data, n, a, s, None) == 0 and (a.raw, s.raw) == exp                    # out_inf = NULL
        # both outputs NULL, or a NULL input: -EINVAL and nothing written
        a, s, f = (ctypes.create_string_buffer(b"\xaa" * k, k) for k in (96 * n, 48 * n, n))
        assert fn(h, data, n, None, None, f) == -22 and f.raw == b"\xaa" * n
        assert fn(h, None, n, a, s, f) == -22 and (a.raw, s.raw, f.raw) == (b"\xaa" * 96 * n, b"\xaa" * 48 * n, b"\xaa" * n)
        # n = 0 writes nothing
        assert fn(h, data, 0, a, s, f) == 0 and fn(h, None, 0, a, s, f) == 0
        assert (a.raw, s.raw, f.raw) == (b"\xaa" * 96 * n, b"\xaa" * 48 * n, b"\xaa" * n)
    assert _native_h2g1.hash_to_g1(engine, b"") == (b"", None, [])


def dev_call(eng, fn, data, n, stream, aff=True, ser=True, inf=True):
    import torch
    dev = torch.device("cuda", 0)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    outs = [torch.full((k * n,), 0xAA, dtype=torch.uint8, device=dev) if on else None for k, on in ((96, aff), (48, ser), (1, inf))]
    torch.cuda.synchronize(dev)                             # the uploads ran on the default stream
    fn(eng, d_in.data_ptr(), n, *[None if o is None else o.data_ptr() for o in outs], stream.cuda_stream)
    stream.synchronize()
    return tuple(None if o is None else bytes(o.cpu().numpy()) for o in outs)


def test_dev_forms_on_a_stream(engine, fx):
    import torch
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    assert stream.cuda_stream != 0
    recs = fx["map"]
    aff, ser = want(recs)
    inf = bytes(r["inf"] for r in recs)
    assert dev_call(engine, _native_h2g1.map_to_g1_dev, t_bytes(recs), len(recs), stream) == (aff, ser, inf)
    assert dev_call(engine, _native_h2g1.map_to_g1_dev, t_bytes(recs), len(recs), stream, ser=False, inf=False) == (aff, None, None)
    hs = fx["hash"]
    assert dev_call(engine, _native_h2g1.hash_to_g1_dev, cat(r["msg_hash"] for r in hs), 70, stream) == want(hs) + (bytes(70),)
    assert dev_call(engine, _native_h2g1.hash_to_g1_dev, cat(r["msg_hash"] for r in hs), 70, stream, aff=False) == (None, want(hs)[1], bytes(70))
    with pytest.raises(_native.BlsGpuError, match="-22"):
        dev_call(engine, _native_h2g1.hash_to_g1_dev, cat(r["msg_hash"] for r in hs), 70, stream, aff=False, ser=False)


def test_across_slices(engine, fx):
    """a context whose slices hold 7 items: 70 hashes are ten slices, the map section nine full ones and a short one"""
    eng = engine_with_env({"BLSGPU_TEST_SLICE_CAP": "7"})
    try:
        import torch
        hashes = cat(r["msg_hash"] for r in fx["hash"])
        single = _native_h2g1.hash_to_g1(engine, hashes, aff=True, ser=True)
        assert single[:2] == want(fx["hash"])
        assert _native_h2g1.hash_to_g1(eng, hashes, aff=True, ser=True) == single
        assert _native_h2g1.hash_to_g1(eng, hashes, aff=False, ser=True) == (None,) + single[1:]
        recs = fx["map"]
        assert len(recs) % 7
        got = _native_h2g1.map_to_g1(eng, t_bytes(recs), aff=True, ser=True)
        assert got[:2] == want(recs) and got[2] == [r["inf"] for r in recs]
        stream = torch.cuda.Stream(torch.device("cuda", 0))
        assert dev_call(eng, _native_h2g1.hash_to_g1_dev, hashes, 70, stream) == want(fx["hash"]) + (bytes(70),)
        assert dev_call(eng, _native_h2g1.map_to_g1_dev, t_bytes(recs), len(recs), stream) == want(recs) + (bytes(r["inf"] for r in recs),)
    finally:
        eng.close()


def test_outputs_are_in_the_subgroup(engine, fx):
    aff, _, inf = _native_h2g1.map_to_g1(engine, t_bytes(fx["map"]))
    aff2, _, _ = _native_h2g1.hash_to_g1(engine, cat(r["msg_hash"] for r in fx["hash"]))
    finite = b"".join(aff[96 * i:96 * (i + 1)] for i in range(len(inf)) if not inf[i]) + aff2
    assert len(finite) // 96 > 120 and engine.g1_subgroup(finite) == b"\x01" * (len(finite) // 96)


def test_python_batch_forms_under_the_hip_provider(engine, fx):
    p = backend.HipProvider.__new__(backend.HipProvider)
    p._eng = engine
    old = backend._provider
    backend.use(p)
    try:
        hashes = [bytes.fromhex(r["msg_hash"]) for r in fx["hash"]]
        pts = ec.hash_to_points_prehashed_Fq(hashes)
        assert [H.g1_affine_bytes(P._aff()).hex() for P in pts] == [r["point"] for r in fx["hash"]]
        assert [P.serialize().hex() for P in pts] == [r["ser"] for r in fx["hash"]]
        assert pts[:3] == [ec.hash_to_point_prehashed_Fq(h) for h in hashes[:3]]
        msgs = [b"", b"abc", "text", b"y" * 100]
        assert ec.hash_to_points_prehashed_Fq(msgs) == [ec.hash_to_point_prehashed_Fq(m) for m in msgs]      # map_to_g1
        assert ec.hash_to_points_Fq(msgs[:2]) == [ec.hash_to_point_Fq(m) for m in msgs[:2]]
        assert ec.hash_to_points_Fq([b""])[0] == pts[0]
    finally:
        backend.use(old)
