"""Subgroup membership and randomized batch verification without a GPU: the endomorphism tests of csrc/blsgpu_subgroup.hip
restated on the host against the reference's own [n] P verdicts (tests/golden/subgroup.json), PublicKey / Signature
.in_subgroup_batch, and BLS.verify_batch_randomized against BLS.verify_batch through a host provider of the device operations
(tests/subgroup_vectors.HostRLC)."""
import random

import pytest

from subgroup_vectors import HostRLC, N, aggregates, expected_status, g1_status, g2_status, secret_keys


@pytest.fixture(scope="module")
def sub(golden):
    return golden("subgroup.json")


@pytest.fixture
def host(oracle):
    from bls_py import backend
    old = backend._provider
    p = HostRLC(oracle)
    backend.use(p)
    yield p
    backend.use(old)


def _one():
    from bls_py.ec import default_ec
    from bls_py.fields import Fq12
    return Fq12.one(default_ec.q).serialize()


def _pk(A):
    from bls_py import hostmath as H
    from bls_py.ec import JacobianPoint, default_ec
    from bls_py.keys import PublicKey
    return PublicKey(JacobianPoint._from(H.F1, H.aff_to_jac(H.F1, A), default_ec))


def _g2(A):
    from bls_py import hostmath as H
    from bls_py.ec import JacobianPoint, default_ec_twist
    return JacobianPoint._from(H.F2, H.aff_to_jac(H.F2, A), default_ec_twist)


def test_fixture_covers_every_kind(sub):
    for g in ("g1", "g2"):
        kinds = {r["kind"] for r in sub[g]}
        assert {"generator", "subgroup", "random", "torsion", "mixed", "infinity", "off_curve"} <= kinds
        assert {expected_status(r) for r in sub[g]} == {0, 1, 2}


def test_endomorphism_tests_match_n_times_p(sub):
    """phi(P) == -[u^2] P with the pinned beta, psi(Q) == [u] Q with the cofactor clearing's psi: the same verdict as
    the reference's (P * n).infinity on every on-curve fixture point, and as [n] P == O on the host"""
    from bls_py import hostmath as H
    for g, F, dec, status in (("g1", H.F1, H.g1_from_abi, g1_status), ("g2", H.F2, H.g2_from_abi, g2_status)):
        for r in sub[g]:
            A = dec(bytes.fromhex(r["point"]))
            assert status(A) == expected_status(r), (g, r["kind"])
            if r["on_curve"]:
                assert (H.jac_mul(F, H.aff_to_jac(F, A), N) is None) == r["in_subgroup"], (g, r["kind"])


def test_the_other_cube_root_fails():
    """beta is a sign convention: the other cube root of unity rejects G1 itself"""
    from bls_py import hostmath as H
    import subgroup_vectors as V
    beta2 = V.BETA * V.BETA % H.Q
    assert beta2 != V.BETA and pow(V.BETA, 3, H.Q) == 1
    old = V.BETA
    try:
        V.BETA = beta2
        assert V.g1_status(H.G1_GEN) == 2
    finally:
        V.BETA = old
    assert V.g1_status(H.G1_GEN) == 1


def test_in_subgroup_batch_is_exact(sub, host):
    from bls_py import hostmath as H
    from bls_py.keys import PublicKey
    from bls_py.signature import Signature
    keys = [_pk(H.g1_from_abi(bytes.fromhex(r["point"]))) for r in sub["g1"]]
    assert PublicKey.in_subgroup_batch(keys) == [r["in_subgroup"] for r in sub["g1"]]
    sigs = [Signature(_g2(H.g2_from_abi(bytes.fromhex(r["point"])))) for r in sub["g2"]]
    assert Signature.in_subgroup_batch(sigs) == [r["in_subgroup"] for r in sub["g2"]]
    assert host.names() == ["g1_subgroup", "g2_subgroup"]
    assert PublicKey.in_subgroup_batch([]) == [] and Signature.in_subgroup_batch([]) == []


def _check(batch, host, seed=1):
    from bls_py.bls import BLS
    want = BLS.verify_batch(batch)
    host.calls.clear()
    host.products.clear()
    got = BLS.verify_batch_randomized(batch, rng=random.Random(seed))
    assert got == want
    return got


def test_valid_batches_need_one_pairing(host):
    batch = aggregates(3, 4)
    from bls_py.keys import PrivateKey
    batch += PrivateKey.sign_batch(secret_keys(b"single", 3), [b"s0", b"s1", b"s2"])
    assert _check(batch, host) == [True] * 6
    names = host.names()
    assert names.count("pairing_multi") == 1 and "pairing_multi_batch" not in names
    assert host.products == [_one()]
    # 3 x 4 + 3 distinct messages: 15 + 1 pairs
    assert ("pairing_multi", 16) in host.calls


def test_one_forgery_fails_the_combined_check(host):
    batch = aggregates(3, 4, forged_at=1)
    assert _check(batch, host) == [True, False, True]
    assert len(host.products) == 1 and host.products[0] != _one()
    assert host.names()[-1] == "pairing_multi_batch"          # all three decided by the exact path


def test_key_outside_g1_and_signature_outside_g2_take_the_exact_path(sub, host):
    from bls_py import hostmath as H
    from bls_py.aggregation_info import AggregationInfo
    from bls_py.keys import PrivateKey
    from bls_py.signature import Signature
    sks = secret_keys(b"out", 4)
    sigs = PrivateKey.sign_batch(sks, [b"m0", b"m1", b"m2", b"m3"])
    T1 = next(H.g1_from_abi(bytes.fromhex(r["point"])) for r in sub["g1"] if r["kind"] == "torsion")
    T2 = next(H.g2_from_abi(bytes.fromhex(r["point"])) for r in sub["g2"] if r["kind"] == "torsion")
    # key pk + T (outside G1), with its own aggregation info over the same message
    pk = sigs[1].aggregation_info.public_keys[0]
    bad_pk = _pk(H.jac_to_affine(H.F1, H.jac_add(H.F1, pk.value._jac(), H.aff_to_jac(H.F1, T1))))
    mh = sigs[1].aggregation_info.message_hashes[0]
    sigs[1] = Signature(sigs[1].value, AggregationInfo.from_msg_hash(bad_pk, mh))
    # signature sig + T2 (outside G2)
    v = sigs[2].value
    sigs[2] = Signature(_g2(H.jac_to_affine(H.F2, H.jac_add(H.F2, v._jac(), H.aff_to_jac(H.F2, T2)))), sigs[2].aggregation_info)
    got = _check(sigs, host)
    # (e(T, H(m)) = 1 for a torsion part T of order prime to n: the key pk + T still verifies; the signature does not)
    assert got == [True, True, False, True]
    # two eligible signatures got weights: the G2 sum has two terms
    assert [c[1] for c in host.calls if c[0] == "g2_msm"] == [2]


def test_infinity_signature_and_missing_tree_entry(host):
    from bls_py import hostmath as H
    from bls_py.aggregation_info import AggregationInfo
    from bls_py.keys import PrivateKey
    from bls_py.signature import Signature
    from bls_py.ec import JacobianPoint, default_ec_twist
    sks = secret_keys(b"inf", 3)
    sigs = PrivateKey.sign_batch(sks, [b"a", b"b", b"c"])
    sigs[0] = Signature(JacobianPoint._from(H.F2, None, default_ec_twist), sigs[0].aggregation_info)
    info = sigs[2].aggregation_info
    broken = Signature(sigs[2].value, AggregationInfo({}, info.message_hashes, info.public_keys))
    got = _check(sigs + [broken], host)
    assert got == [False, True, True, False]
    assert [c[1] for c in host.calls if c[0] == "g2_msm"] == [2]


def test_key_sum_at_infinity(host):
    """pk and -pk with equal exponents over one message: P_im = O, which the reference's Miller loop does not treat as
    infinity -- that signature is decided by the exact path"""
    from bls_py import hostmath as H
    from bls_py.aggregation_info import AggregationInfo
    from bls_py.keys import PrivateKey
    from bls_py.signature import Signature
    from bls_py.util import hash256
    sks = secret_keys(b"neg", 2)
    sigs = PrivateKey.sign_batch(sks, [b"x", b"y"])
    pk = sigs[0].aggregation_info.public_keys[0]
    neg = _pk(H.jac_to_affine(H.F1, H.jac_neg(H.F1, pk.value._jac())))
    mh = hash256(b"x")
    odd = Signature(sigs[0].value, AggregationInfo._from_tree({(mh, pk): 1, (mh, neg): 1}))
    got = _check([odd] + sigs, host)
    assert got[1:] == [True, True]
    assert [c[1] for c in host.calls if c[0] == "g2_msm"] == [2]


def test_shared_messages(host):
    """committee shape: many signatures over few messages -> messages + 1 pairs"""
    from bls_py.keys import PrivateKey
    sks = secret_keys(b"committee", 9)
    sigs = PrivateKey.sign_batch(sks, [b"block %d" % (i % 3) for i in range(9)])
    assert _check(sigs, host) == [True] * 9
    assert ("pairing_multi", 4) in host.calls
    sigs[4] = sks[4].sign(b"block 0")                            # a valid signature over another message ...
    sigs[4].set_aggregation_info(sigs[5].aggregation_info)       # ... claimed for block 2
    assert _check(sigs, host) == [True] * 4 + [False] + [True] * 4


def test_empty_list(host):
    from bls_py.bls import BLS
    assert BLS.verify_batch_randomized([]) == []
    assert host.calls == []


def test_weights_drawn_in_list_order(host):
    """one getrandbits(64) per eligible signature, in the list's order, none for the others; the G2 sum takes them as drawn"""
    from bls_py.bls import BLS
    from bls_py import hostmath as H
    from bls_py.ec import JacobianPoint, default_ec_twist
    from bls_py.keys import PrivateKey
    from bls_py.signature import Signature

    class Rec(random.Random):
        def __init__(self, seed):
            super().__init__(seed)
            self.drawn = []

        def getrandbits(self, k):
            v = super().getrandbits(k)
            self.drawn.append((k, v))
            return v

    sigs = PrivateKey.sign_batch(secret_keys(b"w", 4), [b"w0", b"w1", b"w2", b"w3"])
    sigs.insert(2, Signature(JacobianPoint._from(H.F2, None, default_ec_twist), sigs[0].aggregation_info))
    rng = Rec(7)
    assert BLS.verify_batch_randomized(sigs, rng=rng) == BLS.verify_batch(sigs)
    ref = random.Random(7)
    want = [ref.getrandbits(64) for _ in range(4)]
    assert rng.drawn == [(64, v) for v in want] and all(want)
    assert [c[3] for c in host.calls if c[0] == "g2_msm" and c[2] == 1 and c[1] == 4] == [want]
    # the same seed gives the same calls
    calls = list(host.calls)
    host.calls.clear()
    BLS.verify_batch_randomized(sigs, rng=Rec(7))
    assert [c for c in host.calls if c[0] == "g2_msm"] == [c for c in calls if c[0] == "g2_msm" and c[1] == 4]
