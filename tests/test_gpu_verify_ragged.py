"""Aggregates whose messages have UNEQUAL numbers of signers on the device -- one message with 9 signers (two chunks of the
ragged kernel) and five messages with one, the secure-aggregation exponents in the tree.
Only test_the_ragged_call_gives_the_key_sums_verify_uses runs new code: the per-message key sums from ONE call of the
g1_msm_ranges extension are the points bls.py's padded sums give, and they verify the aggregate in the pipeline.
test_verify and test_the_batch_verifications_agree run bls.py as it was -- it is deliberately NOT routed through the extension
(profiles/msm_ranges_probe.txt) -- and pass without the new calls: they hold the ragged shape's answers (True, False after one
changed exponent or key, the three verifications agreeing) for whoever routes it later."""
import random

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def hip_provider():
    from bls_py import backend
    backend.use(None)          # default HIP provider
    yield
    backend.use(None)


def aggregate(tag):
    from bls_py.bls import BLS
    from bls_py.keys import PrivateKey
    sks = [PrivateKey.from_seed(b"%s-%d" % (tag, i)) for i in range(14)]
    msgs = [b"%s shared" % tag] * 9 + [b"%s own %d" % (tag, i) for i in range(5)]
    return sks, BLS.aggregate_sigs(PrivateKey.sign_batch(sks, msgs))


def with_tree(sig, tree):
    from bls_py.aggregation_info import AggregationInfo
    from bls_py.signature import Signature
    out = Signature.from_g2(sig.value)
    out.set_aggregation_info(AggregationInfo._from_tree(tree))
    return out


@pytest.fixture(scope="module")
def world():
    from bls_py.bls12381 import n as ORDER
    sks, good = aggregate(b"ragged")
    tree = dict(good.aggregation_info.tree)
    by_msg = {}
    for mh, pk in tree:
        by_msg.setdefault(mh, []).append(pk)
    assert sorted(len(v) for v in by_msg.values()) == [1, 1, 1, 1, 1, 9]
    shared = next(mh for mh, v in by_msg.items() if len(v) == 9)
    assert any(e != 1 for (mh, _), e in tree.items() if mh == shared)        # secure aggregation: hash_pks exponents
    victim = sorted(pk for mh, pk in tree if mh == shared)[4]
    bad_exp = dict(tree)
    bad_exp[(shared, victim)] = (tree[(shared, victim)] + 1) % ORDER
    bad_key = dict(tree)
    del bad_key[(shared, victim)]
    other = next(pk for mh, pk in tree if mh != shared)
    bad_key[(shared, other)] = tree[(shared, victim)]
    return good, with_tree(good, bad_exp), with_tree(good, bad_key)


def key_groups(sig):
    info = sig.aggregation_info
    by_message = {}
    for mh, pk in zip(info.message_hashes, info.public_keys):
        by_message.setdefault(mh, []).append(pk)
    return [[pk.value for pk in keys] for keys in by_message.values()], [[info.tree[(mh, pk)] for pk in keys] for mh, keys in by_message.items()]


def test_verify(world):
    from bls_py.bls import BLS
    good, bad_exp, bad_key = world
    assert BLS.verify(good) is True
    assert BLS.verify(bad_exp) is False
    assert BLS.verify(bad_key) is False


def test_the_ragged_call_gives_the_key_sums_verify_uses(world):
    """the per-message key sums of the aggregate -- groups of 9, 1, 1, 1, 1, 1 keys under their exponents -- from ONE call of the
    g1_msm_ranges extension are the points bls.py's padded sums give, and they verify the aggregate in the pipeline"""
    from bls_py import backend, hostmath as H
    from bls_py.bls import BLS, _g1_sums
    from bls_py.ec import default_ec
    from bls_py.fields import Fq12
    good = world[0]
    kg, eg = key_groups(good)
    fn = backend.extension("g1_msm_ranges")
    assert fn is not None
    pts = b"".join(H.g1_affine_bytes(p.to_affine()._aff()) for g in kg for p in g)
    ranges, lo = [], 0
    for g in kg:
        ranges.append((lo, lo + len(g)))
        lo += len(g)
    out, flag = fn(pts, [int(x) for e in eg for x in e], ranges)
    want = b"".join(H.g1_affine_bytes(p.to_affine()._aff()) for p in _g1_sums(kg, eg))
    assert out == want and flag == bytes(6)
    BLS.verify(good)                                         # (fills BLS._NEG_G1)
    info = good.aggregation_info
    hashes = b"".join(dict.fromkeys(info.message_hashes))
    sig = H.g2_affine_bytes(good.value.to_affine()._aff())
    assert backend.get().verify_pipeline(BLS._NEG_G1, sig, hashes, 6, keys_affine=out) == Fq12.one(default_ec.q).serialize()


def test_the_batch_verifications_agree(world):
    from bls_py.bls import BLS
    good, bad_exp, bad_key = world
    _, second = aggregate(b"second")
    batch = [good, bad_exp, second, bad_key, good]
    want = [True, False, True, False, True]
    assert [BLS.verify(s) for s in batch] == want
    assert BLS.verify_batch(batch) == want
    assert BLS.verify_batch_randomized(batch, rng=random.Random(11)) == want
    assert BLS.verify_batch_randomized([good, second], rng=random.Random(12)) == [True, True]
