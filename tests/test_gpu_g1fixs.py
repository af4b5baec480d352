"""Fixed-base G1 multiplication for secret keys on the GPU: blsgpu_g1_mul_gen_secret / blsgpu_hd_paths_secret
(csrc/blsgpu_g1fix.hip k_fix_mul_secret, one scalar per lane on a schedule that does not depend on the scalar) against the
digit-indexed path of the same engine (blsgpu_g1_mul_gen, blsgpu_hd_paths in private mode), against the reference's public
keys (tests/golden/keygen.json) and HD vectors (hd_paths.json, hd.json), and through the secret=True keyword of bls_py.keys.

k_fix_mul_secret runs 256 lanes per workgroup, 64 per wavefront: the sizes sit on those boundaries +-1."""
import ctypes
import hashlib
import json
import os
import random

import pytest

from bls_py import hostmath as H
from hd_paths_vectors import check_digest
from hd_vectors import xprv_index

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = H.N
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 513]
NMAX = max(SIZES)
H31 = 2**31
WIDTHS = (32, 32, 96, 48, 4)            # chain code, key, affine, serialised, parent fingerprint
G1_AFF = H.g1_affine_bytes(H.G1_GEN)


def scalars():
    """the scalar list of tests/test_g2smul_model.py"""
    rng = random.Random(0x62736d)
    fixed = [0, 1, 7, 8, 9, 15, 16, N - 1, N, N + 1, 1 << 255, (1 << 256) - 1,
             int("88" * 32, 16), int("77" * 32, 16), int("f0" * 32, 16)]
    return fixed + [rng.randrange(1 << 256) for _ in range(200)]


@pytest.fixture
def hip_backend(engine):
    from bls_py import backend
    old = backend._provider
    backend.use(backend.HipProvider())
    yield
    backend.use(old)


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "keygen.json")) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def cases(engine):
    """NMAX scalars -- scalar i is the same whatever the size of the call -- and the digit-indexed path's bytes for them,
    computed once.  The head pins 0 and n (infinity) and n + 1 (G1 itself); then the scalar list is spread over the lanes
    with a stride coprime to 64."""
    S = scalars()
    head = [0, N, N + 1, 1, (1 << 256) - 1, 8, N - 1]
    body = [S[(i * 7) % len(S)] for i in range(NMAX - len(head))]
    sc = b"".join(s.to_bytes(32, "big") for s in head + body)
    aff, ser = engine.g1_mul_gen(sc)
    return {"scalars": sc, "aff": aff, "ser": ser}


def test_the_head_is_pinned(cases):
    aff, ser = cases["aff"], cases["ser"]
    for i in (0, 1):                                                        # 0 and n: infinity
        assert aff[96 * i:96 * (i + 1)] == bytes(96) and ser[48 * i:48 * (i + 1)] == bytes(48)
    for i in (2, 3):                                                        # n + 1 and 1: G1 itself
        assert aff[96 * i:96 * (i + 1)] == G1_AFF and ser[48 * i:48 * (i + 1)] == H.g1_compress(H.G1_GEN)


@pytest.mark.parametrize("n", SIZES)
def test_against_the_table_path(engine, cases, n):
    sc = cases["scalars"][:32 * n]
    aff, ser = engine.g1_mul_gen_secret(sc)
    assert aff == cases["aff"][:96 * n]
    assert ser == cases["ser"][:48 * n]
    # each output alone
    assert engine.g1_mul_gen_secret(sc, ser=False) == (aff, None)
    assert engine.g1_mul_gen_secret(sc, aff=False) == (None, ser)


def test_against_the_fixture(engine, fixture):
    aff, ser = engine.g1_mul_gen_secret(b"".join(bytes.fromhex(r["sk"]) for r in fixture))
    assert aff.hex() == "".join(r["aff"] for r in fixture)
    assert ser.hex() == "".join(r["ser"] for r in fixture)
    assert engine.g1_mul_gen_secret([int(r["sk"], 16) for r in fixture[:3]])[1].hex() == "".join(r["ser"] for r in fixture[:3])


def test_dev_form_on_a_stream(engine, cases):
    import torch
    dev = torch.device("cuda", 0)
    n = 257
    d_sc = torch.frombuffer(bytearray(cases["scalars"][:32 * n]), dtype=torch.uint8).to(dev)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        d_aff = torch.full((96 * (n + 1),), 0xAA, dtype=torch.uint8, device=dev)
        d_ser = torch.full((48 * (n + 1),), 0xAA, dtype=torch.uint8, device=dev)
        d_ser1 = torch.full((48 * n,), 0xAA, dtype=torch.uint8, device=dev)
        engine.g1_mul_gen_secret_dev(d_sc.data_ptr(), n, d_aff.data_ptr(), d_ser.data_ptr(), stream.cuda_stream)
        engine.g1_mul_gen_secret_dev(d_sc.data_ptr(), n, None, d_ser1.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    # the spare lanes of the last workgroup store nothing: the record behind the last one is untouched
    assert bytes(d_aff.cpu().numpy()) == cases["aff"][:96 * n] + b"\xaa" * 96
    assert bytes(d_ser.cpu().numpy()) == cases["ser"][:48 * n] + b"\xaa" * 48
    assert bytes(d_ser1.cpu().numpy()) == cases["ser"][:48 * n]


def _aff(pk):
    return H.g1_affine_bytes(H.jac_to_affine(H.F1, pk.value._jac()))


def _record(k):
    return k.chain_code + _aff(k.private_key.get_public_key()) + k.private_key.serialize()


@pytest.fixture(scope="module")
def parents(engine):
    from bls_py import backend
    from bls_py.keys import ExtendedPrivateKey
    old = backend._provider
    backend.use(backend.HipProvider())
    try:
        esk = ExtendedPrivateKey.from_seed(b"gpu secret paths")
        keys = [esk] + esk.private_child_batch([H31 + 1, 5, H31 + 9])
        return b"".join(_record(k) for k in keys)
    finally:
        backend.use(old)


@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("depth", [1, 4])
def test_paths_against_the_private_mode(engine, parents, n, depth):
    rnd = random.Random(100 * n + depth)
    edge = [0, 1, H31 - 1, H31, H31 + 1, 2**32 - 1]
    paths = [[rnd.choice(edge) if rnd.random() < 0.3 else rnd.randrange(2**32) for _ in range(depth)] for _ in range(n)]
    assert n == 1 or (any(i >> 31 for p in paths for i in p) and any(not i >> 31 for p in paths for i in p))
    parent_of = [rnd.randrange(4) for _ in range(n)]
    for pof, recs in ((parent_of, parents), (None, parents[160:320])):
        want = engine.hd_paths(recs, True, pof, paths)
        got = engine.hd_paths_secret(recs, pof, paths)
        assert len(got) == 5 and all(len(g) == w * n for g, w in zip(got, WIDTHS))
        assert got == want
    full =engine.hd_paths(parents, True, parent_of, paths)
    assert engine.hd_paths_secret(parents, parent_of, paths, ser=False, fp=False) == (full[0], full[1], full[2], None, None)
    assert engine.hd_paths_secret(parents, parent_of, paths, aff=False) == (full[0], full[1], None, full[3], full[4])


def test_paths_dev_form_on_a_stream(engine, parents):
    import torch
    dev = torch.device("cuda", 0)
    rnd = random.Random(7)
    n, depth = 65, 3
    paths = [[rnd.randrange(2**32) for _ in range(depth)] for _ in range(n)]
    parent_of = [rnd.randrange(4) for _ in range(n)]
    d_par = torch.tensor(list(parents), dtype=torch.uint8, device=dev)
    d_of = torch.tensor(parent_of, dtype=torch.int64, device=dev).to(torch.int32)
    d_idx = torch.tensor([i for p in paths for i in p], dtype=torch.int64, device=dev).to(torch.int32)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        outs = [torch.full((w * n,), 0xAA, dtype=torch.uint8, device=dev) for w in WIDTHS]
        engine.hd_paths_secret_dev(d_par.data_ptr(), 4, d_of.data_ptr(), d_idx.data_ptr(), depth, n, *[o.data_ptr() for o in outs],
                                   stream.cuda_stream)
    stream.synchronize()
    assert tuple(bytes(o.cpu().numpy()) for o in outs) == engine.hd_paths(parents, True, parent_of, paths)


def test_reference_hd_vectors(golden, hip_backend):
    from bls_py.keys import ExtendedPrivateKey
    for rec in golden("hd_paths.json")["private"]:
        esk = ExtendedPrivateKey.from_seed(bytes.fromhex(rec["seed"]))
        leaves = esk.private_path_batch(rec["paths"], secret=True)
        check_digest([k.serialize() for k in leaves], rec["esk"])
        check_digest([k.get_extended_public_key().serialize() for k in leaves], rec["epk"])
    rec = golden("hd.json")["xprv_range"]
    xprv = ExtendedPrivateKey.from_seed(bytes.fromhex(rec["seed"]))
    assert rec["count"] == 512
    kids = [k.serialize() for k in xprv.private_child_batch([xprv_index(k) for k in range(rec["count"])], secret=True)]
    assert hashlib.sha256(b"".join(kids)).hexdigest() == rec["sha256"]
    for k, h in rec["every32"].items():
        assert kids[int(k)].hex() == h


def _same_extended(a, b):
    assert a.serialize() == b.serialize() and a == b
    assert a.get_extended_public_key().serialize() == b.get_extended_public_key().serialize()
    assert a.get_public_key() == b.get_public_key() and a.get_public_key().serialize() == b.get_public_key().serialize()
    assert (a.depth, a.child_number, a.parent_fingerprint) == (b.depth, b.child_number, b.parent_fingerprint)


def test_python_secret_keyword(engine, hip_backend):
    from bls_py.bls import BLS
    from bls_py.keys import ExtendedPrivateKey, PrivateKey
    rng = random.Random(41)
    sks = [PrivateKey(v) for v in (1, 2, N - 1)] + [PrivateKey(rng.randrange(1, N)) for _ in range(37)]
    pks = PrivateKey.get_public_key_batch(sks)
    got = PrivateKey.get_public_key_batch(sks, secret=True)
    assert got == pks and [p.serialize() for p in got] == [p.serialize() for p in pks]
    assert got == [sk.get_public_key() for sk in sks]
    assert PrivateKey.get_public_key_batch([], secret=True) == []
    msgs = [b"secret keygen %d" % i for i in range(len(sks))]
    ref = PrivateKey.sign_batch_uniform(sks, msgs)
    uni = PrivateKey.sign_batch_uniform(sks, msgs, secret=True)
    assert len(uni) == len(ref)
    for a, b in zip(uni, ref):
        assert a == b and a.serialize() == b.serialize()
        ia, ib = a.get_aggregation_info(), b.get_aggregation_info()
        assert ia.tree == ib.tree and ia.message_hashes == ib.message_hashes and ia.public_keys == ib.public_keys
    assert BLS.verify(uni[0])
    assert BLS.verify(BLS.aggregate_sigs(uni[:3]))
    assert PrivateKey.sign_batch_uniform([], [], secret=True) == []
    # HD: children, paths of mixed length (an empty one included), paths of several parents
    esk = ExtendedPrivateKey.from_seed(b"secret keyword")
    idx = [5, H31 + 3, 0, 5, 2**32 - 1, H31 - 1]
    for a, b in zip(esk.private_child_batch(idx, secret=True), esk.private_child_batch(idx)):
        _same_extended(a, b)
    assert esk.private_child_batch([], secret=True) == []
    paths = [[1], [H31 + 2, 7, H31], [], [3, 4], [2**32 - 1] * 5]
    for a, b in zip(esk.private_path_batch(paths, secret=True), esk.private_path_batch(paths)):
        _same_extended(a, b)
    # (fresh parents: their own public keys are not cached, so the secret form computes them on its path as well)
    fresh = [ExtendedPrivateKey.from_seed(b"secret parent %d" % i) for i in range(3)]
    fresh2 = [ExtendedPrivateKey.from_seed(b"secret parent %d" % i) for i in range(3)]
    pof, pp = [2, 0, 1, 2, 0], [[9], [H31, 1], [4, 4, 4], [0], [H31 + 1]]
    for a, b in zip(ExtendedPrivateKey.private_paths_from(fresh, pof, pp, secret=True), ExtendedPrivateKey.private_paths_from(fresh2, pof, pp)):
        _same_extended(a, b)
    with pytest.raises(OverflowError):
        esk.private_child_batch([2**32], secret=True)
    deep = ExtendedPrivateKey(1, 255, 0, 0, esk.chain_code, esk.private_key)
    with pytest.raises(Exception, match="Cannot go further than 255 levels"):
        deep.private_child_batch([0], secret=True)


def test_argument_errors_leave_the_outputs_untouched(engine, cases, parents):
    L = engine.lib
    sc = cases["scalars"][:32 * 5]
    aff, ser = (ctypes.create_string_buffer(b"\xAA" * m, m) for m in (96 * 5, 48 * 5))
    assert L.blsgpu_g1_mul_gen_secret(engine.h, None, 5, aff, ser) == -22
    assert L.blsgpu_g1_mul_gen_secret(engine.h, sc, 5, None, None) == -22
    assert L.blsgpu_g1_mul_gen_secret(None, sc, 5, aff, ser) == -22
    assert L.blsgpu_g1_mul_gen_secret_dev(engine.h, None, 5, None, None, None) == -22
    assert aff.raw == b"\xAA" * (96 * 5) and ser.raw == b"\xAA" * (48 * 5)
    idx = (ctypes.c_uint32 * 10)(*range(10))
    bad_of = (ctypes.c_uint32 * 5)(0, 1, 4, 0, 0)
    outs = [ctypes.create_string_buffer(b"\xAA" * (w * 5), w * 5) for w in WIDTHS]
    o = [ctypes.cast(b, ctypes.c_void_p) for b in outs]
    P = L.blsgpu_hd_paths_secret
    assert P(engine.h, parents, 4, None, idx, 0, 5, *o) == -22                       # depth 0
    assert P(engine.h, parents, 4, None, idx, 256, 5, *o) == -22                     # depth > 255
    assert P(engine.h, parents, 0, None, idx, 2, 5, *o) == -22                       # no parents
    assert P(engine.h, None, 4, None, idx, 2, 5, *o) == -22
    assert P(engine.h, parents, 4, None, None, 2, 5, *o) == -22
    assert P(engine.h, parents, 4, None, idx, 2, 5, None, o[1], o[2], o[3], o[4]) == -22
    assert P(engine.h, parents, 4, None, idx, 2, 5, o[0], None, o[2], o[3], o[4]) == -22    # private derivation needs out_sk
    assert P(engine.h, parents, 4, None, idx, 2, 5, o[0], o[1], None, None, o[4]) == -22
    assert P(engine.h, parents, 4, bad_of, idx, 2, 5, *o) == -22                     # parent index out of range
    assert L.blsgpu_hd_paths_secret_dev(engine.h, None, 4, None, None, 2, 5, None, None, None, None, None, None) == -22
    assert L.blsgpu_hd_paths_secret_dev(engine.h, None, 4, None, None, 0, 5, None, None, None, None, None, None) == -22
    assert all(b.raw == b"\xAA" * len(b.raw) for b in outs)


def test_empty_calls(engine):
    L = engine.lib
    buf = ctypes.create_string_buffer(b"\xAA" * 8, 8)
    assert L.blsgpu_g1_mul_gen_secret(engine.h, None, 0, buf, buf) == 0
    assert L.blsgpu_g1_mul_gen_secret(engine.h, None, 0, None, None) == 0
    assert L.blsgpu_g1_mul_gen_secret_dev(engine.h, None, 0, None, None, None) == 0
    assert L.blsgpu_hd_paths_secret(engine.h, None, 0, None, None, 1, 0, buf, buf, buf, buf, buf) == 0
    assert L.blsgpu_hd_paths_secret_dev(engine.h, None, 0, None, None, 1, 0, None, None, None, None, None, None) == 0
    assert buf.raw == b"\xAA" * 8
    assert engine.g1_mul_gen_secret(b"") == (b"", b"")


def test_workspace_counts_the_table_once():
    """a fresh context: the total grows by the signed-window table (58 240 bytes) on first use and not again"""
    from bls_py import _native
    e = _native.Engine(0)
    try:
        sc = (5).to_bytes(32, "big")
        e.g1_mul_gen(sc)                                     # staging and the 8-bit table are there before the first secret call
        before = e.workspace_bytes()
        e.g1_mul_gen_secret(sc)
        first = e.workspace_bytes()
        e.g1_mul_gen_secret(sc)
        again = e.workspace_bytes()
        assert first["total"] - before["total"] == 65 * 8 * 112 == 58240
        assert again == first
        assert {k: v for k, v in first.items() if k != "total"} == {k: v for k, v in before.items() if k != "total"}
    finally:
        e.close()
