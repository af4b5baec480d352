"""Device signing: blsgpu_g2_mul_secret / blsgpu_sign (csrc/blsgpu_g2smul.hip k_g2_smul, one scalar per lane pair on a
schedule that does not depend on the scalar) against the reference's signatures (tests/golden/sign.json), against the G2
multi-scalar sum of the same engine, and through PrivateKey's batch methods.

k_g2_smul runs 128 lane pairs per 256-thread workgroup (32 per wavefront): the sizes sit on those boundaries +-1."""
import ctypes
import json
import os
import random

import pytest

from bls_py import hostmath as H
from bls_py.ec import JacobianPoint, default_ec_twist
from bls_py.signature import Signature
from bls_py.util import hash256

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = H.N
SIZES = [1, 2, 31, 32, 33, 127, 128, 129, 257]
NMAX = max(SIZES)


def scalars():
    """the scalar list of tests/test_g2smul_model.py"""
    rng = random.Random(0x62736d)
    fixed = [0, 1, 7, 8, 9, 15, 16, N - 1, N, N + 1, 1 << 255, (1 << 256) - 1,
             int("88" * 32, 16), int("77" * 32, 16), int("f0" * 32, 16)]
    return fixed + [rng.randrange(1 << 256) for _ in range(200)]


def mirror_ser(aff):
    """Signature.from_g2(point).serialize() of the host mirror for 192 affine bytes ((0, 0): infinity)"""
    J = JacobianPoint._from(H.F2, H.aff_to_jac(H.F2, H.g2_from_abi(aff)), default_ec_twist)
    return Signature.from_g2(J).serialize()


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "sign.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cases(engine):
    """NMAX (point, scalar) pairs -- case i is the same whatever the size of the call -- and the engine's own G2 sums
    (groups of one point) for them, computed once.  Points: four hashed points, (0, 0) and a twist point outside the
    subgroup; the first cases pin the results at infinity (s = 0 and s = n on a subgroup point), infinity as input, and
    n / n + 1 on the twist point (no reduction mod n); then the scalar list is spread over the lanes."""
    with open(os.path.join(GOLDEN, "subgroup.json")) as f:
        twist = next(bytes.fromhex(r["point"]) for r in json.load(f)["g2"]
                     if r["on_curve"] and not r["in_subgroup"] and any(bytes.fromhex(r["point"])))
    hm = engine.hash_to_g2(b"".join(hash256(b"sign test point %d" % i) for i in range(4)))
    hashed = [hm[192 * i:192 * (i + 1)] for i in range(4)]
    kinds = hashed + [bytes(192), twist]
    S = scalars()
    head = [(hashed[0], 0), (hashed[0], N), (bytes(192), 5), (twist, N), (twist, N + 1), (hashed[1], (1 << 256) - 1),
            (twist, 0), (bytes(192), 0)]
    body = [(kinds[(i * 5 + i // 6) % 6], S[(i * 7) % len(S)]) for i in range(NMAX - len(head))]
    pairs = head + body
    pts = b"".join(p for p, _ in pairs)
    sc = b"".join(s.to_bytes(32, "big") for _, s in pairs)
    want, want_inf = engine.g2_msm(pts, sc, 1, NMAX)
    assert want_inf[:3] == [True, True, True] and want_inf[3:6] == [False, False, False] and want_inf[6:8] == [True, True]
    assert want[192 * 4:192 * 5] != twist                    # (n + 1) P != P outside the subgroup
    return {"pts": pts, "scalars": sc, "aff": want, "inf": want_inf, "ser": b"".join(mirror_ser(want[192 * i:192 * (i + 1)]) for i in range(NMAX)),
            "twist": twist, "hashed": hashed}


@pytest.mark.parametrize("n", SIZES)
def test_primitive_against_the_group_sums(engine, cases, n):
    aff, ser, inf = engine.g2_mul_secret(cases["pts"][:192 * n], cases["scalars"][:32 * n])
    assert inf == cases["inf"][:n]
    assert aff == cases["aff"][:192 * n]
    assert ser == cases["ser"][:96 * n]
    # each output alone
    aff2, none, _ = engine.g2_mul_secret(cases["pts"][:192 * n], cases["scalars"][:32 * n], ser=False)
    none2, ser2, _ = engine.g2_mul_secret(cases["pts"][:192 * n], cases["scalars"][:32 * n], aff=False)
    assert none is None and none2 is None and aff2 == aff and ser2 == ser


def test_infinity_serialisation_is_pinned(cases):
    for i in (0, 1, 2, 6, 7):
        assert cases["inf"][i] and cases["aff"][192 * i:192 * (i + 1)] == bytes(192) and cases["ser"][96 * i:96 * (i + 1)] == bytes(96)


def test_primitive_against_the_fixture(engine, fixture):
    recs = fixture["cases"]
    pts = engine.hash_to_g2(b"".join(bytes.fromhex(r["hash"]) for r in recs))
    aff, ser, inf = engine.g2_mul_secret(pts, b"".join(bytes.fromhex(r["sk"]) for r in recs))
    assert not any(inf)
    assert aff.hex() == "".join(r["aff"] for r in recs)
    assert ser.hex() == "".join(r["sig"] for r in recs)


@pytest.mark.parametrize("n", [1, 33, 129])
def test_shared_point(engine, cases, n):
    sc = cases["scalars"][:32 * n]
    for P in (cases["hashed"][2], cases["twist"], bytes(192)):
        one = engine.g2_mul_secret(P, sc)
        assert one == engine.g2_mul_secret(P * n, sc)
        want, want_inf = engine.g2_msm(P * n, sc, 1, n)
        assert one[0] == want and one[2] == want_inf


def test_sign_against_the_fixture(engine, fixture):
    recs = fixture["cases"]
    sks = b"".join(bytes.fromhex(r["sk"]) for r in recs)
    aff, ser = engine.sign(sks, b"".join(bytes.fromhex(r["hash"]) for r in recs))
    assert aff.hex() == "".join(r["aff"] for r in recs)
    assert ser.hex() == "".join(r["sig"] for r in recs)
    same = [recs[i] for i in fixture["same_message"]]
    assert len(same) == 5 and len({r["hash"] for r in same}) == 1
    aff, ser = engine.sign(b"".join(bytes.fromhex(r["sk"]) for r in same), bytes.fromhex(same[0]["hash"]))
    assert aff.hex() == "".join(r["aff"] for r in same)
    assert ser.hex() == "".join(r["sig"] for r in same)
    # one key, one message is both forms at once
    aff, ser = engine.sign(bytes.fromhex(recs[0]["sk"]), bytes.fromhex(recs[0]["hash"]))
    assert aff.hex() == recs[0]["aff"] and ser.hex() == recs[0]["sig"]


def test_dev_forms_on_a_stream(engine, cases, fixture):
    import torch
    dev = torch.device("cuda", 0)

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    n = 129
    recs = fixture["cases"]
    d_pts, d_sc = up(cases["pts"][:192 * n]), up(cases["scalars"][:32 * n])
    d_one = up(cases["hashed"][3])
    d_sks, d_h = up(b"".join(bytes.fromhex(r["sk"]) for r in recs)), up(b"".join(bytes.fromhex(r["hash"]) for r in recs))
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        d_aff = torch.full((192 * n,), 0xAA, dtype=torch.uint8, device=dev)
        d_ser = torch.full((96 * n,), 0xAA, dtype=torch.uint8, device=dev)
        d_inf = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
        d_ser1 = torch.full((96 * n,), 0xAA, dtype=torch.uint8, device=dev)
        d_saff = torch.full((192 * len(recs),), 0xAA, dtype=torch.uint8, device=dev)
        d_sser = torch.full((96 * len(recs),), 0xAA, dtype=torch.uint8, device=dev)
        d_sser1 = torch.full((96 * 5,), 0xAA, dtype=torch.uint8, device=dev)
        engine.g2_mul_secret_dev(d_pts.data_ptr(), n, d_sc.data_ptr(), n, d_aff.data_ptr(), d_ser.data_ptr(), d_inf.data_ptr(), stream.cuda_stream)
        engine.g2_mul_secret_dev(d_one.data_ptr(), 1, d_sc.data_ptr(), n, None, d_ser1.data_ptr(), None, stream.cuda_stream)
        engine.sign_dev(d_sks.data_ptr(), d_h.data_ptr(), len(recs), len(recs), d_saff.data_ptr(), d_sser.data_ptr(), stream.cuda_stream)
        lo = fixture["same_message"][0]
        engine.sign_dev(d_sks[32 * lo:].data_ptr(), d_h[32 * lo:].data_ptr(), 1, 5, None, d_sser1.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    aff, ser, inf = engine.g2_mul_secret(cases["pts"][:192 * n], cases["scalars"][:32 * n])
    assert bytes(d_aff.cpu().numpy()) == aff and bytes(d_ser.cpu().numpy()) == ser
    assert [bool(b) for b in d_inf.cpu().numpy()] == inf
    assert bytes(d_ser1.cpu().numpy()) == engine.g2_mul_secret(cases["hashed"][3], cases["scalars"][:32 * n])[1]
    assert bytes(d_saff.cpu().numpy()).hex() == "".join(r["aff"] for r in recs)
    assert bytes(d_sser.cpu().numpy()).hex() == "".join(r["sig"] for r in recs)
    assert bytes(d_sser1.cpu().numpy()).hex() == "".join(recs[i]["sig"] for i in fixture["same_message"])


def test_python_batches_and_verification(engine):
    from bls_py.bls import BLS
    from bls_py.keys import PrivateKey
    rng = random.Random(40)
    sks = [PrivateKey(rng.randrange(1, N)) for _ in range(40)]
    msgs = [b"uniform signing %d" % i for i in range(40)]
    ref = PrivateKey.sign_batch(sks, msgs)
    assert PrivateKey.sign_serialized_batch(sks, msgs) == [s.serialize() for s in ref]
    assert PrivateKey.sign_prehashed_serialized_batch(sks, [hash256(m) for m in msgs]) == [s.serialize() for s in ref]
    # one message for every key
    one = PrivateKey.sign_serialized_batch(sks[:7], msgs[0])
    assert one == [s.serialize() for s in PrivateKey.sign_batch(sks[:7], [msgs[0]] * 7)]
    assert PrivateKey.sign_prehashed_serialized_batch(sks[:7], hash256(msgs[0])) == one
    assert all(type(b) is bytes and len(b) == 96 for b in one)
    uni = PrivateKey.sign_batch_uniform(sks, msgs)
    assert len(uni) == 40
    for a, b in zip(uni, ref):
        assert a == b and a.serialize() == b.serialize()
        ia, ib = a.get_aggregation_info(), b.get_aggregation_info()
        assert ia.tree == ib.tree and ia.message_hashes == ib.message_hashes and ia.public_keys == ib.public_keys
    assert BLS.verify(uni[0])
    assert BLS.verify(BLS.aggregate_sigs(uni[:3]))
    assert PrivateKey.sign_serialized_batch([], []) == [] and PrivateKey.sign_batch_uniform([], []) == []
    with pytest.raises(ValueError):
        PrivateKey.sign_serialized_batch(sks[:3], msgs[:2])


def test_argument_errors_leave_the_outputs_untouched(engine, cases):
    L = engine.lib
    pts, sc = cases["pts"][:192 * 5], cases["scalars"][:32 * 5]
    aff, ser, inf = (ctypes.create_string_buffer(b"\xAA" * m, m) for m in (192 * 5, 96 * 5, 5))
    assert L.blsgpu_g2_mul_secret(engine.h, pts, 2, sc, 5, aff, ser, inf) == -22
    assert L.blsgpu_g2_mul_secret(engine.h, pts, 5, sc, 5, None, None, inf) == -22
    assert L.blsgpu_g2_mul_secret(engine.h, pts, 1, sc, 5, None, None, inf) == -22
    assert L.blsgpu_sign(engine.h, sc, sc, 2, 5, aff, ser) == -22
    assert L.blsgpu_sign(engine.h, sc, sc, 5, 5, None, None) == -22
    assert L.blsgpu_g2_mul_secret_dev(engine.h, None, 2, None, 5, None, None, None, None) == -22
    assert L.blsgpu_sign_dev(engine.h, None, None, 2, 5, None, None, None) == -22
    assert aff.raw == b"\xAA" * (192 * 5) and ser.raw == b"\xAA" * (96 * 5) and inf.raw == b"\xAA" * 5


def test_empty_call(engine):
    L = engine.lib
    aff = ctypes.create_string_buffer(b"\xAA" * 8, 8)
    assert L.blsgpu_g2_mul_secret(engine.h, None, 0, None, 0, aff, aff, aff) == 0
    assert L.blsgpu_g2_mul_secret(engine.h, None, 1, None, 0, None, None, None) == 0
    assert L.blsgpu_sign(engine.h, None, None, 0, 0, aff, aff) == 0
    assert L.blsgpu_g2_mul_secret_dev(engine.h, None, 0, None, 0, None, None, None, None) == 0
    assert L.blsgpu_sign_dev(engine.h, None, None, 1, 0, None, None, None) == 0
    assert aff.raw == b"\xAA" * 8
    assert engine.g2_mul_secret(b"", b"") == (b"", b"", []) and engine.sign(b"", b"") == (b"", b"")
