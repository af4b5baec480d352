"""Signing without a GPU: the reference's vectors (tests/golden/sign.json) against the host mirror's decompression, and
the routing of PrivateKey's serialised batch methods under a host provider of `sign` (hostmath's hash to G2 and
double-and-add in place of blsgpu_sign)."""
import json
import os

import pytest

from bls_py import backend
from bls_py import hostmath as H
from bls_py.keys import PrivateKey
from bls_py.signature import Signature
from bls_py.util import hash256, hash512

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "sign.json")) as f:
        return json.load(f)


def test_fixture_shape(fixture):
    recs = fixture["cases"]
    assert 30 <= len(recs) <= 40
    assert [int(r["sk"], 16) for r in recs[:3]] == [1, 2, H.N - 1]
    same = fixture["same_message"]
    assert len(same) == 5 and len({recs[i]["hash"] for i in same}) == 1 and len({recs[i]["sk"] for i in same}) == 5
    for r in recs:
        assert hash256(bytes.fromhex(r["msg"])).hex() == r["hash"]
        assert len(r["sig"]) == 192 and len(r["aff"]) == 384 and 0 < int(r["sk"], 16) < H.N


def test_serialised_signatures_decompress_to_the_affine_bytes(fixture):
    for r in fixture["cases"]:
        sig = Signature.from_bytes(bytes.fromhex(r["sig"]))
        A = H.jac_to_affine(H.F2, sig.value._jac())
        assert H.g2_affine_bytes(A).hex() == r["aff"]
        assert H.on_curve(H.F2, A)
        assert sig.serialize().hex() == r["sig"]


class HostSign:
    """provider with `sign` alone: sk_i H(h_i) on the host"""

    def __init__(self):
        self.calls = []

    def sign(self, sks, msg_hashes, aff=True, ser=True):
        n, n_msg = len(sks) // 32, len(msg_hashes) // 32
        self.calls.append((n, n_msg, aff, ser))
        assert n_msg in (1, n)
        pts = [H.hash_to_g2_prehashed(msg_hashes[32 * i:32 * (i + 1)], hash512) for i in range(n_msg)]
        out = [H.jac_to_affine(H.F2, H.jac_mul(H.F2, H.aff_to_jac(H.F2, pts[i if n_msg > 1 else 0]),
                                               int.from_bytes(sks[32 * i:32 * (i + 1)], "big"))) for i in range(n)]
        return (b"".join(H.g2_affine_bytes(A) for A in out) if aff else None,
                b"".join(H.g2_compress(A) for A in out) if ser else None)


@pytest.fixture()
def host_sign():
    old = backend._provider
    prov = HostSign()
    backend.use(prov)
    yield prov
    backend.use(old)


def test_serialised_batches_route_to_sign(fixture, host_sign):
    recs = fixture["cases"]
    pick = [recs[i] for i in (0, 2, 9)]
    sks = [PrivateKey(int(r["sk"], 16)) for r in pick]
    got = PrivateKey.sign_prehashed_serialized_batch(sks, [bytes.fromhex(r["hash"]) for r in pick])
    assert [g.hex() for g in got] == [r["sig"] for r in pick]
    assert PrivateKey.sign_serialized_batch(sks, [bytes.fromhex(r["msg"]) for r in pick]) == got
    assert host_sign.calls == [(3, 3, False, True)] * 2
    same = [recs[i] for i in fixture["same_message"][:2]]
    sks = [PrivateKey(int(r["sk"], 16)) for r in same]
    got = PrivateKey.sign_serialized_batch(sks, bytes.fromhex(same[0]["msg"]))
    assert [g.hex() for g in got] == [r["sig"] for r in same]
    assert host_sign.calls[-1] == (2, 1, False, True)
    assert all(type(g) is bytes and len(g) == 96 for g in got)
    assert PrivateKey.sign_serialized_batch([], []) == [] and PrivateKey.sign_prehashed_serialized_batch([], b"\x00" * 32) == []
    with pytest.raises(ValueError):
        PrivateKey.sign_prehashed_serialized_batch(sks, [bytes(32)])
    with pytest.raises(ValueError):
        PrivateKey.sign_prehashed_serialized_batch(sks, bytes(31))
    with pytest.raises(ValueError):
        PrivateKey.sign_prehashed_serialized_batch(sks, [bytes(32), bytes(33)])
