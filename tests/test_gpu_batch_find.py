"""blsgpu_verify_find on the device.  The signatures are the library's own (blsgpu_sign), the expected statuses are known by
construction and cross-checked against BLS.verify_batch (exact): sizes and forgery positions around the short node, the three
forgery kinds, the work bound read from `stats`, ineligible items among valid ones, shared and permuted tables, the infinity
rule, zero weights, the _dev form and BLS.verify_batch_find on a mixed list."""
import ctypes
import hashlib
import random
import struct

import pytest

import bisect_model
from bls_py import _native_find as F
from bls_py import hostmath as H

pytestmark = pytest.mark.gpu

N = H.N
PLAYERS = 101
SIZES = [1, 2, 3, 5, 64, 65, 100]
KINDS = ("wrong_key", "wrong_msg", "swapped")


def mh(i):
    return hashlib.sha256(b"batch find %d" % i).digest()


@pytest.fixture(scope="module")
def world(engine):
    """PLAYERS keys and messages; per item i the valid signature and the three forgeries: signed by the next key, the
    signature on the next message, and the (valid) signature of the next item"""
    rng = random.Random("batch find world")
    sks = [rng.randrange(1, N) for _ in range(PLAYERS)]
    nxt = sks[1:] + sks[:1]
    hashes = [mh(i) for i in range(PLAYERS)]
    pks = engine.g1_mul_gen(sks, aff=True, ser=False)[0]
    cut = lambda b, sz: [b[sz * i:sz * (i + 1)] for i in range(PLAYERS)]
    good = cut(engine.sign(sks, b"".join(hashes), aff=True, ser=False)[0], 192)
    return {"sks": sks, "keys": cut(pks, 96), "hashes": hashes, "good": good,
            "wrong_key": cut(engine.sign(nxt, b"".join(hashes), aff=True, ser=False)[0], 192),
            "wrong_msg": cut(engine.sign(sks, b"".join(hashes[1:] + hashes[:1]), aff=True, ser=False)[0], 192),
            "swapped": good[1:] + good[:1]}


def items_of(world, n, forged=None):
    """n items (sig, key, hash) with the positions of `forged` ({position: kind}) spoiled, and the expected status bytes"""
    forged = forged or {}
    items = [(world[forged.get(i, "good")][i], world["keys"][i], world["hashes"][i]) for i in range(n)]
    return items, bytes(0 if i in forged else 1 for i in range(n))


def pack(items):
    keys, msgs = {}, {}
    key_idx = [keys.setdefault(k, len(keys)) for _, k, _ in items]
    msg_idx = [msgs.setdefault(m, len(msgs)) for _, _, m in items]
    return b"".join(s for s, _, _ in items), b"".join(keys), key_idx, b"".join(msgs), msg_idx


def run(engine, items, weights=None, seed=1):
    rng = random.Random(seed)
    if weights is None:
        weights = [rng.getrandbits(64) or 1 for _ in items]
    return F.verify_find(engine, *pack(items), weights)


def lg(n):
    return (n - 1).bit_length()


def objects(items):
    """the items as Signature objects with their AggregationInfo"""
    from bls_py.aggregation_info import AggregationInfo
    from bls_py.ec import JacobianPoint, default_ec, default_ec_twist
    from bls_py.keys import PublicKey
    from bls_py.signature import Signature
    out = []
    for s, k, m in items:
        pk = PublicKey.from_g1(JacobianPoint._from(H.F1, H.aff_to_jac(H.F1, H.g1_from_abi(k)), default_ec))
        sig = JacobianPoint._from(H.F2, H.aff_to_jac(H.F2, H.g2_from_abi(s)) if any(s) else None, default_ec_twist)
        out.append(Signature.from_g2(sig, AggregationInfo.from_msg_hash(pk, m)))
    return out


def positions(n):
    """forgery patterns: none; first; last; middle; both sides of the boundary the short node begins at; all three kinds"""
    half = 1 << (lg(n) - 1) if n > 1 else 0              # K / 2: the root's second half (the short node when n < K) begins here
    raw = [(), (0,), (n - 1,), (n // 2,), (half - 1, half), (0, n // 2, n - 1)]
    out = []
    for p in raw:
        p = tuple(sorted({i for i in p if 0 <= i < n}))
        if p not in out:
            out.append(p)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_forgery_positions(engine, world, n):
    from bls_py.bls import BLS
    for c, pos in enumerate(positions(n)):
        forged = {i: KINDS[(c + j) % 3] for j, i in enumerate(pos)}
        items, want = items_of(world, n, forged)
        status, stats = run(engine, items, seed=100 * n + c)
        print("n", n, "forged", forged, "stats", stats)
        assert status == want
        assert stats == bisect_model.plain(n, sorted(forged))["stats"]
        if not forged:
            assert stats[:2] == (1, 1) and stats[2] == n + 1
        elif len(forged) == 1:
            assert stats[1] <= 1 + 2 * lg(n) and stats[0] <= lg(n) + 1
        if n == 5 and len(forged) == 3:
            assert BLS.verify_batch(objects(items)) == [s == 1 for s in want]


def test_work_bound_of_the_bisection(engine, world):
    """derived from the tree, not measured: a failing node is halved and both halves are tested, so ONE forgery costs at most
    1 + 2 ceil(log2 n) node tests; with every item forged every node of the tree is tested once"""
    from bls_py.bls import BLS
    for n, at in ((64, 37), (100, 81)):
        items, want = items_of(world, n, {at: "wrong_msg"})
        status, (rounds, tests, pairs) = run(engine, items, seed=n)
        print("n", n, "one forgery: rounds", rounds, "node tests", tests, "pairs", pairs)
        assert status == want and status.count(0) == 1
        assert (rounds, tests, pairs) == bisect_model.plain(n, [at])["stats"]
        assert tests <= 1 + 2 * lg(n) and rounds <= lg(n) + 1
        assert tests <= (13 if n == 64 else 15)
        if n == 100:
            assert BLS.verify_batch(objects(items)) == [s == 1 for s in want]
    items, want = items_of(world, 8, {i: KINDS[i % 3] for i in range(8)})
    status, (rounds, tests, pairs) = run(engine, items, seed=8)
    assert status == want == bytes(8) and tests <= 2 * 8 - 1 and rounds == 4
    assert (rounds, tests, pairs) == bisect_model.plain(8, range(8))["stats"]


def test_ineligible_items_among_valid_ones(engine, world, golden):
    sub = golden("subgroup.json")
    pick = lambda g, **kw: next(bytes.fromhex(r["point"]) for r in sub[g]
                                if all(r[k] == v for k, v in kw.items()) and any(bytes.fromhex(r["point"])))
    sig_off, sig_out = pick("g2", on_curve=False), pick("g2", on_curve=True, in_subgroup=False)
    key_off, key_out = pick("g1", on_curve=False), pick("g1", on_curve=True, in_subgroup=False)
    items, _ = items_of(world, 16)
    spoil = {1: (sig_off, None, 0), 3: (sig_out, None, 0), 4: (bytes(192), None, 0), 6: (None, key_off, 2), 8: (None, key_out, 2),
             9: (None, bytes(96), 2), 11: (sig_out, key_out, 0), 12: (bytes(192), bytes(96), 0), 14: (world["wrong_key"][14], None, 0),
             15: (world["swapped"][15], key_out, 2)}
    want = bytearray(b"\x01" * 16)
    for i, (s, k, st) in spoil.items():
        items[i] = (s if s is not None else items[i][0], k if k is not None else items[i][1], items[i][2])
        want[i] = st
    status, stats = run(engine, items, seed=3)
    assert status == bytes(want)
    # nothing eligible at all: no round is run
    status, stats = run(engine, [items[1], items[6], items[12]], seed=4)
    assert status == b"\x00\x02\x00" and stats == (0, 0, 0)


def test_shared_tables_permutations_and_einval(engine, world):
    # many items on one message (n_msgs = 1): every key signs hash 0; one forgery among them
    n = 9
    one = engine.sign(world["sks"][:n], world["hashes"][0], aff=True, ser=False)[0]
    items = [(one[192 * i:192 * (i + 1)], world["keys"][i], world["hashes"][0]) for i in range(n)]
    items[4] = (items[5][0], items[4][1], items[4][2])
    sigs, keys, key_idx, msgs, msg_idx = pack(items)
    assert len(msgs) == 32 and len(keys) == 96 * n
    status, _ = F.verify_find(engine, sigs, keys, key_idx, msgs, msg_idx, [7] * n)
    assert status == b"\x01\x01\x01\x01\x00\x01\x01\x01\x01"
    # many items share one key: key 0 signs nine messages
    many = engine.sign([world["sks"][0]] * n, b"".join(world["hashes"][:n]), aff=True, ser=False)[0]
    items = [(many[192 * i:192 * (i + 1)], world["keys"][0], world["hashes"][i]) for i in range(n)]
    items[8] = (items[0][0], items[8][1], items[8][2])
    sigs, keys, key_idx, msgs, msg_idx = pack(items)
    assert len(keys) == 96 and len(msgs) == 32 * n
    status, _ = F.verify_find(engine, sigs, keys, key_idx, msgs, msg_idx, list(range(1, n + 1)))
    assert status == b"\x01" * 8 + b"\x00"
    # permuted tables: the tables reversed and padded with an entry nobody names
    items, want = items_of(world, 7, {2: "wrong_key"})
    sigs, keys, key_idx, msgs, msg_idx = pack(items)
    rk = world["keys"][50] + b"".join(reversed([keys[96 * i:96 * (i + 1)] for i in range(7)]))
    rm = b"".join(reversed([msgs[32 * i:32 * (i + 1)] for i in range(7)])) + world["hashes"][50]
    status, _ = F.verify_find(engine, sigs, rk, [7 - i for i in key_idx], rm, [6 - i for i in msg_idx], [3, 1, 4, 1, 5, 9, 2])
    assert status == want
    # -EINVAL before anything is written
    lib, h = engine.lib, engine.h
    wb = b"".join(w.to_bytes(8, "big") for w in range(1, 8))
    ki, mi = (ctypes.c_uint32 * 7)(*key_idx), (ctypes.c_uint32 * 7)(*msg_idx)
    bad_k, bad_m = (ctypes.c_uint32 * 7)(*(key_idx[:6] + [7])), (ctypes.c_uint32 * 7)(*([7] + msg_idx[1:]))
    st = ctypes.create_string_buffer(b"\xee" * 7, 7)
    base = dict(sigs=sigs, keys=keys, n_keys=7, ki=ki, msgs=msgs, n_msgs=7, mi=mi, wb=wb, n=7, st=st)
    call = lambda v: lib.blsgpu_verify_find(h, v["sigs"], v["keys"], v["n_keys"], v["ki"], v["msgs"], v["n_msgs"], v["mi"], v["wb"], v["n"],
                                            v["st"], None)
    for over in (dict(ki=bad_k), dict(mi=bad_m), dict(n_keys=0), dict(n_msgs=0), dict(n_keys=6), dict(sigs=None), dict(keys=None),
                 dict(ki=None), dict(msgs=None), dict(mi=None), dict(wb=None), dict(st=None)):
        assert call(dict(base, **over)) == -22, over
        assert st.raw == b"\xee" * 7 and lib.blsgpu_last_error()
    assert call(dict(base, n=0)) == 0 and st.raw == b"\xee" * 7
    assert call(base) == 0 and st.raw == want


def test_infinity_rule_and_zero_weights(engine, world):
    sk, h0, h1 = world["sks"][0], world["hashes"][0], world["hashes"][1]
    pk, npk = world["keys"][0], engine.g1_mul_gen([N - sk], aff=True, ser=False)[0]
    pair = engine.sign([sk, N - sk], h0, aff=True, ser=False)[0]
    sig, nsig = pair[:192], pair[192:]
    assert H.g1_from_abi(npk)[1] == -H.g1_from_abi(pk)[1] % H.Q
    # case 1: (PK, h, sigma), (-PK, h, -sigma) with equal weights: S = O at the root, both valid, one node test
    status, stats = F.verify_find(engine, sig + nsig, pk + npk, [0, 1], h0, [0, 0], [5, 5])
    assert (status, stats) == (b"\x01\x01", (1, 1, 3))
    # case 2: the second item on another message: the root fails with S = O, the leaves give 1 and 0
    status, stats = F.verify_find(engine, sig + nsig, pk + npk, [0, 1], h0 + h1, [0, 1], [5, 5])
    assert (status, stats) == (b"\x01\x00", (2, 3, 7))
    # an all-zero weight behaves as 1: with weights (0, 1) the sum is at infinity again, and forgeries are still found
    status, stats = F.verify_find(engine, sig + nsig, pk + npk, [0, 1], h0, [0, 0], [0, 1])
    assert (status, stats) == (b"\x01\x01", (1, 1, 3))
    items, want = items_of(world, 6, {1: "wrong_key", 4: "swapped"})
    status, _ = run(engine, items, weights=[0] * 6)
    assert status == want


def test_host_and_dev_forms_agree(engine, world):
    import torch
    from bls_py import _native
    items, want = items_of(world, 37, {0: "wrong_key", 20: "wrong_msg", 36: "swapped"})
    sigs, keys, key_idx, msgs, msg_idx = pack(items)
    weights = [random.Random(5).getrandbits(64) or 1 for _ in items]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d_s, d_k, d_m = up(sigs), up(keys), up(msgs)
    d_ki, d_mi = up(struct.pack("<37I", *key_idx)), up(struct.pack("<37I", *msg_idx))
    d_w = up(b"".join(w.to_bytes(8, "big") for w in weights))
    d_st = torch.full((37,), 0xAA, dtype=torch.uint8, device=dev)
    stats = F.verify_find_dev(engine, d_s.data_ptr(), d_k.data_ptr(), 37, d_ki.data_ptr(), d_m.data_ptr(), 37, d_mi.data_ptr(), d_w.data_ptr(),
                                   37, d_st.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    host = F.verify_find(engine, sigs, keys, key_idx, msgs, msg_idx, weights)
    assert (bytes(d_st.cpu().numpy()), stats) == host and host[0] == want
    # the _dev form scans the indices on the device
    for bad_ki, bad_mi in ((key_idx[:36] + [37], msg_idx), (key_idx, [99] + msg_idx[1:])):
        d_st.fill_(0xAA)
        d_bk, d_bm = up(struct.pack("<37I", *bad_ki)), up(struct.pack("<37I", *bad_mi))
        with pytest.raises(_native.BlsGpuError, match="-22"):
            F.verify_find_dev(engine, d_s.data_ptr(), d_k.data_ptr(), 37, d_bk.data_ptr(), d_m.data_ptr(), 37, d_bm.data_ptr(), d_w.data_ptr(),
                                   37, d_st.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert bytes(d_st.cpu().numpy()) == b"\xaa" * 37


class Recorder:
    """the installed provider with verify_find's arguments recorded; without=True: a provider that lacks the call"""

    def __init__(self, inner, without=False):
        self._inner, self.calls = inner, []
        if not without:
            self.verify_find = self._verify_find

    def _verify_find(self, sigs, keys, key_idx, msg_hashes, msg_idx, weights):
        self.calls.append((len(sigs) // 192, len(keys) // 96, len(msg_hashes) // 32, list(weights)))
        return F.verify_find(self._inner._eng, sigs, keys, key_idx, msg_hashes, msg_idx, weights)

    def __getattr__(self, name):
        if name == "verify_find":
            raise AttributeError(name)
        return getattr(self._inner, name)


def test_verify_batch_find_on_a_mixed_list(engine, world):
    from bls_py import backend
    from bls_py.aggregation_info import AggregationInfo
    from bls_py.bls import BLS
    from bls_py.ec import JacobianPoint
    from bls_py.signature import Signature
    singles = objects(items_of(world, 12, {2: "wrong_key", 7: "swapped"})[0])
    multi = BLS.aggregate_sigs(objects(items_of(world, 15)[0][12:15]))                        # three messages
    multi_bad = BLS.aggregate_sigs(objects(items_of(world, 18, {16: "wrong_msg"})[0][15:18]))
    # secure aggregates on one message: two keys with hash_pks exponents -> the key-sum path
    one = engine.sign(world["sks"][20:24], world["hashes"][20], aff=True, ser=False)[0]
    same = objects([(one[192 * i:192 * (i + 1)], world["keys"][20 + i], world["hashes"][20]) for i in range(4)])
    secure = BLS.aggregate_sigs(same[:2])
    secure_bad = BLS.aggregate_sigs([same[2], objects([(world["good"][23], world["keys"][23], world["hashes"][20])])[0]])
    assert len(set(secure.aggregation_info.message_hashes)) == 1 and len(secure.aggregation_info.tree) == 2
    broken = objects(items_of(world, 31)[0][30:31])[0]
    info = broken.aggregation_info
    broken.set_aggregation_info(AggregationInfo({}, info.message_hashes, info.public_keys))   # the tree lacks its key
    infinity = Signature.from_g2(JacobianPoint._from(H.F2, None), objects(items_of(world, 33)[0][32:33])[0].aggregation_info)
    sigs = singles[:6] + [multi, secure, broken] + singles[6:] + [multi_bad, secure_bad, infinity]
    want = BLS.verify_batch(sigs)
    assert want == [True, True, False, True, True, True, True, True, False, True, False, True, True, True, True, False, False, False]
    old = backend.get()
    assert type(old).__name__ == "HipProvider"
    try:
        rec = Recorder(old)
        backend.use(rec)
        assert BLS.verify_batch_find(sigs, rng=random.Random(21)) == want
        # twelve singles and two key sums went to the device, in list order, with the seeded weights in that order
        r = random.Random(21)
        assert rec.calls == [(14, 14, 13, [r.getrandbits(64) for _ in range(14)])]
        assert BLS.verify_batch_find(sigs, rng=random.Random(21)) == want and rec.calls[1] == rec.calls[0]
        lacking = Recorder(old, without=True)
        backend.use(lacking)
        assert backend.extension("verify_find") is None
        assert BLS.verify_batch_find(sigs, rng=random.Random(22)) == want and lacking.calls == []
    finally:
        backend.use(old)
    assert BLS.verify_batch_find(sigs) == want
    assert BLS.verify_batch_find([]) == []
