"""Signature-share verification through the host provider (no GPU): Threshold.verify_sig_shares_batch, share_public_keys and
recover_batch against the reference's 3-of-5 fixture (tests/golden/sigshares.json) and the exact truth of
tests/sigshares_vectors.py."""
import random

import pytest

from sigshares_vectors import HostSigShares, Session, fixture_objects, fixture_truth, msg_hash, pack, truth_bytes


@pytest.fixture(scope="module")
def fx(golden):
    return golden("sigshares.json")


@pytest.fixture
def host(oracle):
    from bls_py import backend
    old = backend._provider
    p = HostSigShares(oracle)
    backend.use(p)
    yield p
    backend.use(old)


def test_fixture_shares_verify_scaled_and_plain(fx, host):
    from bls_py.threshold import Threshold
    pks, msgs = fixture_objects(fx)
    sig_groups = [m["unit"] for m in msgs]
    players = [m["signers"] for m in msgs]
    keys = [[pks[p - 1] for p in m["signers"]] for m in msgs]
    hashes = [m["hash"] for m in msgs]
    got = Threshold.verify_sig_shares_batch(sig_groups, players, keys, hashes, scaled=True, rng=random.Random(1))
    assert got == [[True] * 3, [True] * 3]
    assert got == [fixture_truth(fx, i, s, p, True) for i, (s, p) in enumerate(zip(sig_groups, players))]
    all5 = [1, 2, 3, 4, 5]
    got = Threshold.verify_sig_shares_batch([m["plain"] for m in msgs], [all5, all5], [pks, pks], hashes, scaled=False,
                                            rng=random.Random(2))
    assert got == [[True] * 5, [True] * 5]
    assert ("sig_shares_check", 3, 2, True) in host.calls and ("sig_shares_check", 5, 2, False) in host.calls


def test_swapped_share_and_share_of_the_other_message(fx, host):
    from bls_py.threshold import Threshold
    pks, msgs = fixture_objects(fx)
    all5 = [1, 2, 3, 4, 5]
    # plain: players 2 and 4 swapped in message 0; player 3's share of message 1 in message 0's session
    swapped = list(msgs[0]["plain"])
    swapped[1], swapped[3] = swapped[3], swapped[1]
    crossed = list(msgs[0]["plain"])
    crossed[2] = msgs[1]["plain"][2]
    got = Threshold.verify_sig_shares_batch([swapped, crossed], [all5, all5], [pks, pks], [msgs[0]["hash"]] * 2, scaled=False,
                                            rng=random.Random(3))
    assert got == [[True, False, True, False, True], [True, True, False, True, True]]
    assert got == [fixture_truth(fx, 0, swapped, all5, False), fixture_truth(fx, 0, crossed, all5, False)]
    # scaled: the first two unit signatures swapped between their players
    unit, signers = list(msgs[0]["unit"]), msgs[0]["signers"]
    unit[0], unit[1] = unit[1], unit[0]
    keys = [pks[p - 1] for p in signers]
    got = Threshold.verify_sig_shares_batch([unit], [signers], [keys], [msgs[0]["hash"]], scaled=True, rng=random.Random(4))
    assert got == [[False, False, True]] == [fixture_truth(fx, 0, unit, signers, True)]
    # a unit signature of message 1 (other signer set, other message) in message 0's session
    unit = list(msgs[0]["unit"])
    unit[2] = msgs[1]["unit"][2]
    got = Threshold.verify_sig_shares_batch([unit], [signers], [keys], [msgs[0]["hash"]], scaled=True, rng=random.Random(5))
    assert got == [[True, True, False]]


def test_without_the_entry_the_exact_pairings_decide(fx, oracle):
    from bls_py import backend
    from bls_py.threshold import Threshold
    from subgroup_vectors import HostRLC
    pks, msgs = fixture_objects(fx)
    old = backend._provider
    p = HostRLC(oracle)
    backend.use(p)
    try:
        crossed = list(msgs[0]["plain"])
        crossed[4] = msgs[1]["plain"][4]
        got = Threshold.verify_sig_shares_batch([crossed], [[1, 2, 3, 4, 5]], [pks], [msgs[0]["hash"]], scaled=False)
    finally:
        backend.use(old)
    assert got == [[True, True, True, True, False]]
    assert ("pairing_multi_batch", 2, 5) in p.calls


def test_share_public_keys_equal_sk_g1(fx, host):
    from bls_py.threshold import Threshold
    from dkg_vectors import point
    commitments = [[point(h) for h in dealer] for dealer in fx["commitments"]]
    got = Threshold.share_public_keys(commitments, [1, 2, 3, 4, 5])
    assert [pk.serialize().hex() for pk in got] == fx["share_pks_ser"]
    from bls_py import hostmath as H
    assert [H.g1_affine_bytes(pk.value.to_affine()._aff()).hex() for pk in got] == fx["share_pks"]
    assert ("g1_msm", 5, 3) in host.calls and ("g1_poly_check", 1, 5) in host.calls


def test_recover_batch_skips_the_bad_share_and_gives_up_below_t(fx, host):
    from bls_py.threshold import Threshold
    pks, msgs = fixture_objects(fx)
    all5 = [1, 2, 3, 4, 5]
    one_bad = list(msgs[0]["plain"])
    one_bad[1] = msgs[1]["plain"][1]
    three_bad = list(msgs[1]["plain"])
    for j in (0, 2, 3):
        three_bad[j] = msgs[0]["plain"][j]
    out = Threshold.recover_batch([one_bad, three_bad], [all5, all5], [pks, pks], [msgs[0]["hash"], msgs[1]["hash"]], fx["T"],
                                  rng=random.Random(6))
    assert out[0][1] == [True, False, True, True, True] and out[1][1] == [False, True, False, False, True]
    assert out[0][0].serialize().hex() == msgs[0]["combined"]
    assert out[1][0] is None


def test_repeated_player_raises_the_reference_assertion(fx, host):
    from bls_py.threshold import Threshold
    pks, msgs = fixture_objects(fx)
    with pytest.raises(AssertionError):
        Threshold.verify_sig_shares_batch([msgs[0]["unit"]], [[4, 1, 4]], [[pks[3], pks[0], pks[3]]], [msgs[0]["hash"]], scaled=True)
    with pytest.raises(AssertionError):
        Threshold.lagrange_coeffs_at_zero([4, 1, 4])


def test_host_provider_meets_the_truth_on_seeded_sessions(host):
    """the vectors module against itself: the exact provider on seeded sessions of both forms with every kind of bad share"""
    sessions = [Session([3, 1, 7], msg_hash(1), True, {1: "wrong"}), Session([2, 5, 6], msg_hash(2), True, {0: "other_player", 2: "infinity"}),
                Session([9, 4, 8], msg_hash(1), True, {2: "other_msg", 0: "off_twist"})]
    a = pack(sessions)
    status, sess, _ = host.sig_shares_check(a["sigs"], a["keys"], a["key_idx"], a["x"], a["msg_hashes"], a["weights"], 3, 3, True)
    assert status == truth_bytes(sessions) and sess == b"\x01\x01\x01"
    plain = [Session([3, 1, 7], msg_hash(3), False, {2: "wrong"})]
    a = pack(plain)
    status, sess, _ = host.sig_shares_check(a["sigs"], a["keys"], a["key_idx"], None, a["msg_hashes"], a["weights"], 3, 1, False)
    assert status == truth_bytes(plain) == b"\x01\x01\x00"
