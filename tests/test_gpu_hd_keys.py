"""HD keys and the fixed-base G1 kernel on the GPU (csrc/blsgpu_g1fix.hip): every record of tests/golden/hd.json (generated
from the reference) through the real engine, blsgpu_g1_mul_gen against the CPU oracle and hostmath, blsgpu_hd_children at
65 536 children, and the refusal of hardened indices in public mode."""
import ctypes
import random

import pytest

from hd_vectors import HostHD, check_seed_record, check_xprv_range, check_xpub_range

pytestmark = pytest.mark.gpu

N = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


@pytest.fixture
def hip_backend(engine):
    from bls_py import backend
    old = backend._provider
    backend.use(backend.HipProvider())
    yield
    backend.use(old)


def _gen_bytes():
    from bls_py import hostmath as H
    return H.g1_affine_bytes(H.G1_GEN)


def _want(oracle, s, add=None):
    """(affine, serialised) of s G1 (+ add) by the oracle's double-and-add and hostmath's addition / compression"""
    from bls_py import hostmath as H
    aff, inf = oracle.g1_msm(_gen_bytes(), [s], 1)
    A = None if inf else H.g1_from_abi(aff)
    if add is not None:
        A = H.jac_to_affine(H.F1, H.jac_add(H.F1, H.aff_to_jac(H.F1, A), H.aff_to_jac(H.F1, H.g1_from_abi(add))))
    return H.g1_affine_bytes(A), H.g1_compress(A)


def _check(engine, oracle, scalars, positions=None, add=None, n_add=0):
    aff, ser = engine.g1_mul_gen(scalars, add, n_add)
    n = len(scalars)
    assert len(aff) == 96 * n and len(ser) == 48 * n
    for i in (range(n) if positions is None else positions):
        a = None if n_add == 0 else add[96 * (i if n_add > 1 else 0):][:96]
        wa, ws = _want(oracle, scalars[i], a)
        assert aff[96 * i:96 * (i + 1)] == wa, (i, scalars[i])
        assert ser[48 * i:48 * (i + 1)] == ws, (i, scalars[i])
    return aff, ser


def test_hd_fixture_through_the_engine(golden, hip_backend):
    hd = golden("hd.json")
    for rec in hd["seeds"]:
        check_seed_record(rec)
    check_xpub_range(hd["xpub_range"], full=True)
    check_xprv_range(hd["xprv_range"], full=True)


def test_g1_mul_gen_corner_scalars(engine, oracle):
    sc = [0, 1, 2, N - 1, N, N + 1, 2 * N, 2 * N + 5, 2**255, 2**256 - 1]
    aff, ser = _check(engine, oracle, sc)
    assert aff[:96] == bytes(96) and ser[:48] == bytes(48)          # 0 G1 = infinity
    assert aff[96 * 4:96 * 5] == bytes(96) and ser[48 * 4:48 * 5] == bytes(48)   # n G1 = infinity
    assert aff[96:192] == _gen_bytes()
    # affine-only / serialised-only outputs
    from bls_py import _native
    a2, s2 = engine.g1_mul_gen(sc, ser=False)
    assert a2 == aff and s2 is None
    a3, s3 = engine.g1_mul_gen(sc, aff=False)
    assert s3 == ser and a3 is None
    with pytest.raises(ValueError):
        engine.g1_mul_gen(sc, aff=False, ser=False)
    assert _native.load_library().blsgpu_g1_mul_gen(engine.h, b"", 0, None, 0, None, None) == 0


def test_g1_mul_gen_every_table_entry(engine, oracle):
    # d 2^(8w) for every window w and digit d: each scalar is exactly one table entry
    sc = [d << (8 * w) for w in range(32) for d in range(1, 256)]
    aff, ser = engine.g1_mul_gen(sc)
    from bls_py import hostmath as H
    for i, s in enumerate(sc):
        a, inf = oracle.g1_msm(_gen_bytes(), [s], 1)
        assert not inf and aff[96 * i:96 * (i + 1)] == a, (i, s)
        assert ser[48 * i:48 * (i + 1)] == H.g1_compress(H.g1_from_abi(a)), (i, s)


def test_g1_mul_gen_added_points(engine, oracle):
    from bls_py import hostmath as H
    rnd = random.Random(5)
    s = rnd.randrange(N)
    sG = H.g1_affine_bytes(H.jac_to_affine(H.F1, H.jac_mul(H.F1, H.aff_to_jac(H.F1, H.G1_GEN), s)))
    negsG = H.g1_affine_bytes(H.jac_to_affine(H.F1, H.jac_neg(H.F1, H.aff_to_jac(H.F1, H.g1_from_abi(sG)))))
    # infinity added, the doubling case, P + (-P)
    _check(engine, oracle, [s, s + N], add=bytes(96), n_add=1)
    _check(engine, oracle, [s, s + N], add=sG, n_add=1)
    aff, ser = engine.g1_mul_gen([s, s + N, s], negsG, 1)
    assert aff == bytes(96 * 3) and ser == bytes(48 * 3)
    # one point per scalar, 0 G1 + A = A
    sc = [rnd.randrange(2**256) for _ in range(70)] + [0]
    pts = [sG, negsG, bytes(96)] + [_want(oracle, rnd.randrange(N))[0] for _ in range(68)]
    _check(engine, oracle, sc, add=b"".join(pts), n_add=len(sc))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 65539])
def test_g1_mul_gen_batch_sizes(engine, oracle, n):
    from bls_py import hostmath as H
    rnd = random.Random(n)
    sc = [rnd.randrange(2**256) for _ in range(n)]
    pos = sorted(set([0, n - 1] + [rnd.randrange(n) for _ in range(min(n, 96))]))
    aff, ser = _check(engine, oracle, sc, positions=pos)
    # every position: the serialised form is the compression of the affine one, and the point is on the curve
    for i in range(0, n, max(1, n // 2048)):
        A = H.g1_from_abi(aff[96 * i:96 * (i + 1)])
        assert H.on_curve(H.F1, A) and ser[48 * i:48 * (i + 1)] == H.g1_compress(A)


def test_hd_children_65536(engine):
    from bls_py import hostmath as H
    from bls_py.keys import ExtendedPrivateKey
    rnd = random.Random(9)
    esk = ExtendedPrivateKey.from_seed(b"wide")
    pk = esk.private_key.get_public_key()
    pk_aff = H.g1_affine_bytes(H.jac_to_affine(H.F1, pk.value._jac()))
    idx = [rnd.randrange(2**32) for _ in range(65536)]
    chain, sks, aff, ser = engine.hd_children(esk.chain_code, pk_aff, esk.private_key.serialize(), idx)
    host = HostHD()
    pos = sorted(rnd.sample(range(65536), 256))
    hc, hsk, haff, hser = host.hd_children(esk.chain_code, pk_aff, esk.private_key.serialize(), [idx[p] for p in pos])
    for j, p in enumerate(pos):
        assert chain[32 * p:32 * (p + 1)] == hc[32 * j:32 * (j + 1)]
        assert sks[32 * p:32 * (p + 1)] == hsk[32 * j:32 * (j + 1)]
        assert aff[96 * p:96 * (p + 1)] == haff[96 * j:96 * (j + 1)]
        assert ser[48 * p:48 * (p + 1)] == hser[48 * j:48 * (j + 1)]
    # public derivation of the non-hardened indices gives the same chain codes and keys
    soft = [p for p in range(65536) if idx[p] < 2**31]
    pc, psk, paff, pser = engine.hd_children(esk.chain_code, pk_aff, None, [idx[p] for p in soft])
    assert psk is None
    for j, p in enumerate(soft):
        assert pc[32 * j:32 * (j + 1)] == chain[32 * p:32 * (p + 1)]
        assert paff[96 * j:96 * (j + 1)] == aff[96 * p:96 * (p + 1)]
        assert pser[48 * j:48 * (j + 1)] == ser[48 * p:48 * (p + 1)]


def test_hd_children_refuses_hardened_in_public_mode(engine):
    from bls_py import _native
    from bls_py import hostmath as H
    L = _native.load_library()
    n = 100
    idx = (ctypes.c_uint32 * n)(*([1] * 99 + [2**31]))
    bufs = [ctypes.create_string_buffer(b"\xaa" * (w * n), w * n) for w in (32, 32, 96, 48)]
    rc = L.blsgpu_hd_children(engine.h, b"\x01" * 32, H.g1_affine_bytes(H.G1_GEN), None, idx, n, *bufs)
    assert rc == -22
    assert "hardened" in L.blsgpu_last_error().decode()
    assert all(b.raw == b"\xaa" * len(b.raw) for b in bufs)        # nothing written
    with pytest.raises(_native.BlsGpuError):
        engine.hd_children(b"\x01" * 32, H.g1_affine_bytes(H.G1_GEN), None, [0, 2**31 + 1])


def test_dev_forms_and_workspace(oracle):
    import torch
    from bls_py import _native
    from bls_py import hostmath as H
    e = _native.Engine(0)
    try:
        before = e.workspace_bytes()["total"]
        rnd = random.Random(3)
        sc = [rnd.randrange(2**256) for _ in range(1000)]
        aff, ser = e.g1_mul_gen(sc)
        assert e.workspace_bytes()["total"] >= before + 32 * 255 * 112      # the table counts in the total
        e.trim()                                                           # ... and survives a trim
        dev = torch.device("cuda", 0)
        d_sc = torch.tensor(list(b"".join(s.to_bytes(32, "big") for s in sc)), dtype=torch.uint8, device=dev)
        d_aff = torch.zeros(96 * 1000, dtype=torch.uint8, device=dev)
        d_ser = torch.zeros(48 * 1000, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev)
        e.g1_mul_gen_dev(d_sc.data_ptr(), 1000, d_aff.data_ptr(), d_ser.data_ptr(), st.cuda_stream)
        st.synchronize()
        assert bytes(d_aff.cpu().numpy()) == aff and bytes(d_ser.cpu().numpy()) == ser
        # hd_children_dev, public mode, against the host-buffer form; then a hardened index: -EINVAL, nothing written
        chain_code = bytes(range(32))
        pk_aff = aff[:96]
        idx = [rnd.randrange(2**31) for _ in range(3000)]
        want = e.hd_children(chain_code, pk_aff, None, idx)
        d_idx = torch.tensor(idx, dtype=torch.int64, device=dev).to(torch.int32)
        outs = [torch.full((w * 3000,), 0xAA, dtype=torch.uint8, device=dev) for w in (32, 96, 48)]
        e.hd_children_dev(chain_code, pk_aff, None, d_idx.data_ptr(), 3000, outs[0].data_ptr(), None, outs[1].data_ptr(),
                          outs[2].data_ptr(), st.cuda_stream)
        st.synchronize()
        assert [bytes(o.cpu().numpy()) for o in outs] == [want[0], want[2], want[3]]
        for o in outs:
            o.fill_(0xAA)
        d_idx[1234] = -5                                                   # 2^32 - 5 as uint32
        with pytest.raises(_native.BlsGpuError):
            e.hd_children_dev(chain_code, pk_aff, None, d_idx.data_ptr(), 3000, outs[0].data_ptr(), None, outs[1].data_ptr(),
                              outs[2].data_ptr(), st.cuda_stream)
        st.synchronize()
        assert all(bool((o == 0xAA).all()) for o in outs)
        assert H.on_curve(H.F1, H.g1_from_abi(want[2][:96]))
    finally:
        e.close()
