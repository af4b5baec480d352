"""blsgpu_sig_shares_check on the device against the exact truth of tests/sigshares_vectors.py (sigma_i == c H(m) by
hostmath): status and session_status of the host-buffer and _dev forms, the Python layer, the infinity rule, the -EINVAL
cases, and the work bound of the bisection read from `stats`."""
import ctypes
import random
import struct

import pytest

import bisect_model
from bls_py import hostmath as H

from sigshares_vectors import (N, SK, Session, fixture_objects, fixture_truth, msg_hash, outside_g1, outside_g2, pack, pk_bytes,
                               share_bytes, truth_bytes)

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 5, 8, 67]
GROUPS = [1, 3, 65]


def patterns(k):
    """bad-share patterns: none; the first, middle and last share; two in the same half; two in different halves; all"""
    K = 1
    while K < k:
        K *= 2
    raw = [(), (0,), (k // 2,), (k - 1,), (0, min(1, k - 1)) if K >= 4 else (0,), (0, k - 1), tuple(range(k))]
    out = []
    for p in raw:
        p = tuple(sorted(set(p)))
        if p not in out:
            out.append(p)
    return out


def check(engine, sessions, scaled, seed=1, weights=None):
    a = pack(sessions, weights=weights, seed=seed)
    status, sess, stats = engine.sig_shares_check(a["sigs"], a["keys"], a["key_idx"], a["x"] if scaled else None, a["msg_hashes"],
                                                  a["weights"], a["k"], a["groups"], scaled)
    return status, sess, stats


@pytest.mark.parametrize("k", KS)
def test_sizes_and_bad_share_patterns(engine, k):
    players = list(range(1, k + 1))
    pats = patterns(k)
    for scaled in (True, False):
        mh = msg_hash(1)
        for groups in GROUPS:
            if groups == 1:
                runs = [[Session(players, mh, scaled, {j: "wrong" for j in p})] for p in pats]
            else:
                runs = [[Session(players, mh, scaled, {j: "wrong" for j in pats[g % len(pats)]}) for g in range(groups)]]
            for sessions in runs:
                status, sess, stats = check(engine, sessions, scaled, seed=k * 100 + groups)
                print("k", k, "groups", groups, "scaled", scaled, "stats", stats)
                assert status == truth_bytes(sessions)
                assert sess == b"\x01" * groups
                bad = [[j for j, ok in enumerate(truth_bytes([s])) if not ok] for s in sessions]
                assert stats == bisect_model.shares(k, bad)["stats"]
                if not any(0 in truth_bytes([s]) for s in sessions):
                    assert stats == (1, groups)


def test_mixed_scenarios_and_undecided_key(engine, golden):
    players = [2, 9, 4, 7, 11]
    mh, mh2 = msg_hash(2), msg_hash(3)
    kinds = [{}, {1: "wrong"}, {0: "other_player"}, {4: "other_msg"}, {2: outside_g2(golden)}, {3: "off_twist"}, {1: "infinity"},
             {0: "wrong", 2: "infinity", 4: "other_msg"}]
    for scaled in (True, False):
        sessions = [Session(players, mh if i % 2 else mh2, scaled, bad) for i, bad in enumerate(kinds)]
        status, sess, _ = check(engine, sessions, scaled, seed=7)
        assert status == truth_bytes(sessions) and sess == b"\x01" * len(kinds)
    # a key outside G1: status 2 for its shares that are themselves in G2; 0 for a share that is bad whatever the key
    sessions = [Session(players, mh, False), Session(players, mh, False, {3: "infinity"}), Session(players, mh, False, {1: "wrong"})]
    bad_key = outside_g1(golden)
    sessions[0].keys[2] = bad_key
    sessions[1].keys[3] = bad_key
    status, sess, _ = check(engine, sessions, False, seed=8)
    expect = bytearray(truth_bytes(sessions))
    expect[2] = 2
    assert status == bytes(expect) and sess == b"\x01\x01\x01"


def test_python_layer_decides_an_undecided_key_exactly(engine, golden, oracle):
    from bls_py import backend
    from bls_py.ec import JacobianPoint
    from bls_py.keys import PublicKey
    from bls_py.signature import Signature
    from bls_py.threshold import Threshold
    from subgroup_vectors import HostRLC
    players = [2, 9, 4]
    s = Session(players, msg_hash(2), False, {0: "wrong"})
    sigs = [Signature.from_g2(JacobianPoint._from(H.F2, H.aff_to_jac(H.F2, H.g2_from_abi(b)))) for b in s.sigs]
    keys = [PublicKey(JacobianPoint._from(H.F1, H.aff_to_jac(H.F1, H.g1_from_abi(b)))) for b in s.keys]
    keys[1] = PublicKey(JacobianPoint._from(H.F1, H.aff_to_jac(H.F1, H.g1_from_abi(outside_g1(golden)))))
    got = Threshold.verify_sig_shares_batch([sigs], [players], [keys], [s.mh], scaled=False, rng=random.Random(9))
    exact = Threshold._sig_shares_exact(HostRLC(oracle), [(s.sigs[1], outside_g1(golden), 1, s.mh)])
    assert got == [[False, exact[0], True]]
    assert type(backend.get()).__name__ == "HipProvider"


def test_python_layer_on_the_fixture(engine, golden):
    from bls_py.threshold import Threshold
    fx = golden("sigshares.json")
    pks, msgs = fixture_objects(fx)
    all5 = [1, 2, 3, 4, 5]
    crossed = list(msgs[0]["plain"])
    crossed[1] = msgs[1]["plain"][1]
    out = Threshold.recover_batch([crossed, msgs[1]["plain"]], [all5, all5], [pks, pks], [msgs[0]["hash"], msgs[1]["hash"]], fx["T"],
                                  rng=random.Random(10))
    assert out[0][1] == fixture_truth(fx, 0, crossed, all5, False) == [True, False, True, True, True]
    assert out[1][1] == [True] * 5
    assert [o[0].serialize().hex() for o in out] == [m["combined"] for m in msgs]
    unit = list(msgs[0]["unit"])
    unit[0], unit[1] = unit[1], unit[0]
    signers = msgs[0]["signers"]
    got = Threshold.verify_sig_shares_batch([unit, msgs[1]["unit"]], [signers, msgs[1]["signers"]],
                                            [[pks[p - 1] for p in signers], [pks[p - 1] for p in msgs[1]["signers"]]],
                                            [msgs[0]["hash"], msgs[1]["hash"]], scaled=True, rng=random.Random(11))
    assert got == [[False, False, True], [True, True, True]]
    from dkg_vectors import point
    got = Threshold.share_public_keys([[point(h) for h in dealer] for dealer in fx["commitments"]], all5)
    assert [pk.serialize().hex() for pk in got] == fx["share_pks_ser"]


def test_refused_player_sets_give_session_status_zero(engine):
    players = [3, 5, 8]
    mh = msg_hash(4)
    sessions = [Session(players, mh, True), Session(players, mh, True), Session(players, mh, True, {2: "wrong"}), Session(players, mh, True)]
    a = pack(sessions, seed=12)
    x = bytearray(a["x"])
    x[32 * 3:32 * 4] = (8).to_bytes(32, "big")               # session 1: players 8, 5, 8
    x[32 * 9:32 * 10] = bytes(32)                            # session 3: players 0, 5, 8
    status, sess, _ = engine.sig_shares_check(a["sigs"], a["keys"], a["key_idx"], bytes(x), a["msg_hashes"], a["weights"], 3, 4, True)
    assert sess == b"\x01\x00\x01\x00"
    assert status == b"\x01\x01\x01" + b"\x00\x00\x00" + b"\x01\x01\x00" + b"\x00\x00\x00"


def _raw(engine, a, scaled=1, **over):
    """blsgpu_sig_shares_check called directly; -> (rc, status, session status), the outputs pre-filled with 0xEE"""
    n = a["k"] * a["groups"]
    v = dict(sigs=a["sigs"], keys=a["keys"], n_keys=len(a["keys"]) // 96, key_idx=(ctypes.c_uint32 * n)(*a["key_idx"]), x=a["x"],
             msg_hashes=a["msg_hashes"], weights=b"".join(w.to_bytes(8, "big") for w in a["weights"]), k=a["k"], groups=a["groups"])
    v.update(over)
    st = ctypes.create_string_buffer(b"\xee" * n, n)
    ss = ctypes.create_string_buffer(b"\xee" * a["groups"], a["groups"])
    rc = engine.lib.blsgpu_sig_shares_check(engine.h, v["sigs"], v["keys"], v["n_keys"], v["key_idx"], v["x"], v["msg_hashes"], v["weights"],
                                            scaled, v["k"], v["groups"], st if over.get("status", 1) else None, ss, None)
    return rc, st.raw, ss.raw


def test_einval_before_anything_is_written_and_zero_weights(engine):
    players = [3, 5, 8]
    sessions = [Session(players, msg_hash(4), True, {1: "wrong"}), Session(players, msg_hash(4), True)]
    a = pack(sessions, seed=13)
    untouched = (b"\xee" * 6, b"\xee" * 2)
    bad_idx = (ctypes.c_uint32 * 6)(*([0, 1, 2, 0, 1, 3]))
    for over in (dict(k=0), dict(k=1025), dict(n_keys=0), dict(key_idx=bad_idx), dict(sigs=None), dict(keys=None), dict(key_idx=None),
                 dict(x=None), dict(msg_hashes=None), dict(weights=None), dict(status=0)):
        rc, st, ss = _raw(engine, a, **over)
        assert rc == -22 and (st, ss) == untouched, over
        assert engine.lib.blsgpu_last_error()
    rc, st, ss = _raw(engine, a, groups=0)
    assert rc == 0 and (st, ss) == untouched
    # x is ignored when not scaled; a unit signature is a valid plain share exactly where lambda_j = 1 (player 8 of 3, 5, 8)
    plain = Session(players, msg_hash(4), False)
    rc, st, ss = _raw(engine, a, scaled=0, x=None)
    assert rc == 0 and ss == b"\x01\x01" and st == bytes(int(b == g) for s in sessions for b, g in zip(s.sigs, plain.good))
    assert st == b"\x00\x00\x01\x00\x00\x01"
    rc, st, ss = _raw(engine, a)
    assert rc == 0 and st == truth_bytes(sessions) and ss == b"\x01\x01"
    # a zero weight is taken as 1: the bad share is still found, the good ones still pass
    status, sess, _ = check(engine, sessions, True, weights=[0] * 6)
    assert status == truth_bytes(sessions) == b"\x01\x00\x01\x01\x01\x01" and sess == b"\x01\x01"


def test_infinity_rule(engine):
    """plain, k = 2: keys PK and -PK, shares sigma and -sigma, weights (5, 5): both node sums are at infinity and both
    shares valid; with a wrong second share S != O and P = O, and exactly that share is invalid"""
    mh = msg_hash(5)
    sk = SK[1]
    P = H.g1_from_abi(pk_bytes(1))
    keys = pk_bytes(1) + H.g1_affine_bytes((P[0], -P[1] % H.Q))
    good = share_bytes(sk, mh) + share_bytes(N - sk, mh)
    status, sess, stats = engine.sig_shares_check(good, keys, [0, 1], None, mh, [5, 5], 2, 1, False)
    assert (status, sess, stats) == (b"\x01\x01", b"\x01", (1, 1))
    wrong = share_bytes(sk, mh) + share_bytes(sk + 5, mh)
    status, sess, stats = engine.sig_shares_check(wrong, keys, [0, 1], None, mh, [5, 5], 2, 1, False)
    assert (status, sess, stats) == (b"\x01\x00", b"\x01", (2, 3))


def test_host_and_dev_forms_agree(engine):
    import torch
    from bls_py import _native
    players = list(range(1, 6))
    pats = patterns(5)
    sessions = [Session(players, msg_hash(1), True, {j: "wrong" for j in pats[g % len(pats)]}) for g in range(9)]
    a = pack(sessions, seed=14)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d = {name: up(a[name]) for name in ("sigs", "keys", "x", "msg_hashes")}
    d_idx = up(struct.pack("<45I", *a["key_idx"]))
    d_w = up(b"".join(w.to_bytes(8, "big") for w in a["weights"]))
    for scaled in (True, False):
        d_st = torch.full((45,), 0xAA, dtype=torch.uint8, device=dev)
        d_ss = torch.full((9,), 0xAA, dtype=torch.uint8, device=dev)
        stats = engine.sig_shares_check_dev(d["sigs"].data_ptr(), d["keys"].data_ptr(), len(a["keys"]) // 96, d_idx.data_ptr(),
                                            d["x"].data_ptr() if scaled else None, d["msg_hashes"].data_ptr(), d_w.data_ptr(), scaled, 5, 9,
                                            d_st.data_ptr(), d_ss.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        host = engine.sig_shares_check(a["sigs"], a["keys"], a["key_idx"], a["x"] if scaled else None, a["msg_hashes"], a["weights"], 5, 9,
                                       scaled)
        assert (bytes(d_st.cpu().numpy()), bytes(d_ss.cpu().numpy()), stats) == host
        if scaled:
            assert host[0] == truth_bytes(sessions)
    # the _dev form scans the indices on the device
    d_bad = up(struct.pack("<45I", *(a["key_idx"][:44] + [len(a["keys"]) // 96])))
    d_st = torch.full((45,), 0xAA, dtype=torch.uint8, device=dev)
    d_ss = torch.full((9,), 0xAA, dtype=torch.uint8, device=dev)
    with pytest.raises(_native.BlsGpuError, match="-22"):
        engine.sig_shares_check_dev(d["sigs"].data_ptr(), d["keys"].data_ptr(), len(a["keys"]) // 96, d_bad.data_ptr(), d["x"].data_ptr(),
                                    d["msg_hashes"].data_ptr(), d_w.data_ptr(), True, 5, 9, d_st.data_ptr(), d_ss.data_ptr(),
                                    stream.cuda_stream)
    stream.synchronize()
    assert bytes(d_st.cpu().numpy()) == b"\xaa" * 45 and bytes(d_ss.cpu().numpy()) == b"\xaa" * 9


def test_work_bound_of_the_bisection(engine):
    """A condition derived from the tree, not a measurement: with k = 64 and one bad share per session a failing node is
    halved and both halves are tested, so node tests <= groups (1 + 2 log2 64) = 13 per session in <= 7 rounds -- the
    fallback is bisection, not the per-share loop (64 per session); with no bad share exactly one test per session, one
    round."""
    players = list(range(1, 65))
    mh = msg_hash(1)
    groups = 5
    sessions = [Session(players, mh, False, {(11 * g + 3) % 64: "wrong"}) for g in range(groups)]
    status, sess, (rounds, tests) = check(engine, sessions, False, seed=15)
    assert status == truth_bytes(sessions) and status.count(0) == groups
    print("one bad share per session: rounds", rounds, "node tests", tests)
    assert tests <= groups * (1 + 2 * 6) and rounds <= 7
    assert (rounds, tests) == bisect_model.shares(64, [[(11 * g + 3) % 64] for g in range(groups)])["stats"]
    clean = [Session(players, mh, False) for _ in range(groups)]
    status, sess, (rounds, tests) = check(engine, clean, False, seed=16)
    assert status == b"\x01" * (64 * groups) and (rounds, tests) == (1, groups)
