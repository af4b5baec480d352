"""blsgpu_verify_find_folded on the device: n items over m messages, sorted by message.  The signatures are the library's own
(blsgpu_sign), the expected statuses are known by construction and equal blsgpu_verify_find's on the same inputs and weights:
forgeries of the three kinds at none, first, last and middle positions, at both sides of a run boundary and of the short
node's boundary; the pair counts read from `stats`; sums at infinity inside a node; ineligible items inside runs; zero
weights; the precondition; the _dev form; BLS.verify_batch_find(fold=True)."""
import ctypes
import random
import struct

import pytest

import bisect_model
from bls_py import _native_find as F
from bls_py import _native_ranges as R
from bls_py import hostmath as H
from test_gpu_batch_find import KINDS, PLAYERS, lg, mh, objects

pytestmark = pytest.mark.gpu

N = H.N
SIZES = [1, 2, 3, 5, 64, 65, 100]


@pytest.fixture(scope="module")
def keys(engine):
    rng = random.Random("folded world")
    sks = [rng.randrange(1, N) for _ in range(PLAYERS)]
    pks = engine.g1_mul_gen(sks, aff=True, ser=False)[0]
    return sks, [pks[96 * i:96 * (i + 1)] for i in range(PLAYERS)]


def build(engine, keys, n, m):
    """n items over m messages in runs of (nearly) equal length: per item the valid signature and the three forgeries -- signed
    by the next key, the signature on another message, the (valid) signature of the next item"""
    sks, pks = keys
    msg = [i * m // n for i in range(n)]
    cut = lambda b: [b[192 * i:192 * (i + 1)] for i in range(n)]
    sign = lambda ks, ms: cut(engine.sign(ks, b"".join(mh(j) for j in ms), aff=True, ser=False)[0])
    good = sign(sks[:n], msg)
    return {"n": n, "msg": msg, "keys": pks[:n], "good": good, "wrong_key": sign(sks[1:n + 1], msg),
            "wrong_msg": sign(sks[:n], [j + 1 for j in msg]), "swapped": good[1:] + good[:1]}


def pack(w, forged=None):
    forged = forged or {}
    n = w["n"]
    sigs = b"".join(w[forged.get(i, "good")][i] for i in range(n))
    hashes = b"".join(mh(j) for j in range(max(w["msg"]) + 1))
    return (sigs, b"".join(w["keys"]), list(range(n)), hashes, w["msg"]), bytes(0 if i in forged else 1 for i in range(n))


def positions(n, msg):
    half = 1 << (lg(n) - 1) if n > 1 else 0              # the root's second half (the short node when n < K) begins here
    edge = next((i for i in range(1, n) if msg[i] != msg[i - 1]), 0)         # the first run boundary
    raw = [(), (0,), (n - 1,), (n // 2,), (edge - 1,), (edge,), (half - 1,), (half,), (edge - 1, edge), (0, n // 2, n - 1)]
    out = []
    for p in raw:
        p = tuple(sorted({i for i in p if 0 <= i < n}))
        if p not in out:
            out.append(p)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sizes_messages_and_forgery_positions(engine, keys, n):
    for m in sorted({1, min(2, n), min(3, n), n}):
        w = build(engine, keys, n, m)
        for c, pos in enumerate(positions(n, w["msg"])):
            forged = {i: KINDS[(c + j) % 3] for j, i in enumerate(pos)}
            forged = {i: ("wrong_msg" if k == "swapped" and n == 1 else k) for i, k in forged.items()}
            args, want = pack(w, forged)
            weights = [random.Random(1000 * n + 10 * m + c).getrandbits(64) or 1 for _ in range(n)]
            status, stats = R.verify_find_folded(engine, *args, weights)
            plain, pstats = F.verify_find(engine, *args, weights)
            print("n", n, "m", m, "forged", forged, "stats", stats, "verify_find", pstats)
            assert status == want == plain
            assert stats == bisect_model.folded(w["msg"], sorted(forged))["stats"]
            assert pstats == bisect_model.plain(n, sorted(forged))["stats"]
            if not forged:
                assert stats == (1, 1, m + 1)
            elif len(forged) == 1:
                assert stats[0] <= lg(n) + 1 and stats[1] <= 1 + 2 * lg(n) and stats[2] <= stats[1] * (m + 1)
                if n == 64 and m == 2:
                    assert stats[2] < pstats[2]


def test_sums_at_infinity_inside_a_node(engine, keys):
    sks, pks = keys
    sk, h0, h1 = sks[0], mh(0), mh(1)
    pk, npk = pks[0], engine.g1_mul_gen([N - sk], aff=True, ser=False)[0]
    pair = engine.sign([sk, N - sk], h0, aff=True, ser=False)[0]
    sig, nsig = pair[:192], pair[192:]
    # keys P and -P on one message with equal weights: B_r and S are both at infinity in the root; both items are valid
    status, stats = R.verify_find_folded(engine, sig + nsig, pk + npk, [0, 1], h0, [0, 0], [5, 5])
    assert (status, stats) == (b"\x01\x01", (1, 1, 2))
    # one of the two forged (the signature on another message): only B_r is at infinity, the root fails, the leaves decide
    other = engine.sign([N - sk], h1, aff=True, ser=False)[0]
    status, stats = R.verify_find_folded(engine, sig + other, pk + npk, [0, 1], h0, [0, 0], [5, 5])
    assert (status, stats) == (b"\x01\x00", (2, 3, 6))
    status, stats = R.verify_find_folded(engine, other + nsig, pk + npk, [0, 1], h0, [0, 0], [5, 5])
    assert (status, stats) == (b"\x00\x01", (2, 3, 6))
    # S at infinity with two messages: the root has three pairs and fails, as in blsgpu_verify_find
    status, stats = R.verify_find_folded(engine, sig + nsig, pk + npk, [0, 1], h0 + h1, [0, 1], [5, 5])
    assert (status, stats) == (b"\x01\x00", (2, 3, 7))
    # a zero weight is taken as 1
    status, stats = R.verify_find_folded(engine, sig + nsig, pk + npk, [0, 1], h0, [0, 0], [0, 1])
    assert (status, stats) == (b"\x01\x01", (1, 1, 2))


def test_ineligible_items_inside_runs_and_zero_weights(engine, keys, golden):
    sub = golden("subgroup.json")
    pick = lambda g, **kw: next(bytes.fromhex(r["point"]) for r in sub[g]
                                if all(r[k] == v for k, v in kw.items()) and any(bytes.fromhex(r["point"])))
    sig_off, sig_out = pick("g2", on_curve=False), pick("g2", on_curve=True, in_subgroup=False)
    key_off, key_out = pick("g1", on_curve=False), pick("g1", on_curve=True, in_subgroup=False)
    w = build(engine, keys, 20, 5)                                           # runs of four items
    (sigs, pks, key_idx, hashes, msg_idx), _ = pack(w, {13: "wrong_key"})
    sig = [sigs[192 * i:192 * (i + 1)] for i in range(20)]
    key = [pks[96 * i:96 * (i + 1)] for i in range(20)]
    want = bytearray(b"\x01" * 20)
    want[13] = 0
    spoil = {0: (sig_off, None, 0), 2: (None, key_out, 2), 3: (bytes(192), None, 0), 7: (None, bytes(96), 2),
             8: (sig_out, None, 0), 9: (None, key_off, 2), 10: (sig_out, key_out, 0), 11: (bytes(192), bytes(96), 0),   # the whole run 8 .. 11
             16: (None, key_out, 2)}
    for i, (s, k, st) in spoil.items():
        sig[i], key[i], want[i] = s if s is not None else sig[i], k if k is not None else key[i], st
    args = (b"".join(sig), b"".join(key), key_idx, hashes, msg_idx)
    for weights in ([random.Random(9).getrandbits(64) for _ in range(20)], [0] * 20):
        status, stats = R.verify_find_folded(engine, *args, weights)
        assert status == bytes(want) == F.verify_find(engine, *args, weights)[0]
    # nothing eligible at all: no round is run
    status, stats = R.verify_find_folded(engine, sig[0] + sig[3] + sig[8], key[0] + key[3] + key[8], [0, 1, 2], hashes, [0, 0, 2], [1, 2, 3])
    assert status == b"\x00\x00\x00" and stats == (0, 0, 0)


def test_precondition_and_dev_form(engine, keys):
    import torch
    from bls_py import _native
    n = 37
    w = build(engine, keys, n, 4)
    (sigs, pks, key_idx, hashes, msg_idx), want = pack(w, {0: "wrong_key", 20: "wrong_msg", 36: "swapped"})
    weights = [random.Random(5).getrandbits(64) or 1 for _ in range(n)]
    host = R.verify_find_folded(engine, sigs, pks, key_idx, hashes, msg_idx, weights)
    assert host[0] == want
    # a decreasing msg_idx: -EINVAL, the status buffer untouched
    lib, h = engine.lib, engine.h
    down = msg_idx[:20] + [msg_idx[20] - 1] + msg_idx[21:]
    st = ctypes.create_string_buffer(b"\xee" * n, n)
    wb = b"".join(x.to_bytes(8, "big") for x in weights)
    arr = lambda v: (ctypes.c_uint32 * len(v))(*v)
    assert lib.blsgpu_verify_find_folded(h, sigs, pks, n, arr(key_idx), hashes, 4, arr(down), wb, n, st, None) == -22
    assert st.raw == b"\xee" * n and b"decrease" in lib.blsgpu_last_error()
    assert lib.blsgpu_verify_find_folded(h, sigs, pks, n, arr(key_idx), hashes, 4, arr(msg_idx), wb, n, st, None) == 0 and st.raw == want
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d_s, d_k, d_m, d_w = up(sigs), up(pks), up(hashes), up(wb)
    d_ki, d_mi = up(struct.pack("<%dI" % n, *key_idx)), up(struct.pack("<%dI" % n, *msg_idx))
    d_st = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
    call = lambda ki, mi: R.verify_find_folded_dev(engine, d_s.data_ptr(), d_k.data_ptr(), n, ki.data_ptr(), d_m.data_ptr(), 4, mi.data_ptr(),
                                                   d_w.data_ptr(), n, d_st.data_ptr(), stream.cuda_stream)
    stats = call(d_ki, d_mi)
    stream.synchronize()
    assert (bytes(d_st.cpu().numpy()), stats) == host
    for bad_ki, bad_mi in ((key_idx[:36] + [37], msg_idx), (key_idx, msg_idx[:36] + [4]), (key_idx, down)):
        d_st.fill_(0xAA)
        with pytest.raises(_native.BlsGpuError, match="-22"):
            call(up(struct.pack("<%dI" % n, *bad_ki)), up(struct.pack("<%dI" % n, *bad_mi)))
        stream.synchronize()
        assert bytes(d_st.cpu().numpy()) == b"\xaa" * n


def test_verify_batch_find_fold(engine, keys):
    """an unsorted mixed list: fold=True equals fold=False and BLS.verify_batch"""
    from bls_py import backend
    from bls_py.bls import BLS
    w = build(engine, keys, 12, 3)
    (sigs, pks, _, _, msg_idx), want = pack(w, {1: "wrong_key", 6: "wrong_msg", 11: "swapped"})
    items = [(sigs[192 * i:192 * (i + 1)], pks[96 * i:96 * (i + 1)], mh(msg_idx[i])) for i in range(12)]
    order = list(range(12))
    random.Random(3).shuffle(order)
    objs = objects([items[i] for i in order])
    expect = [want[i] == 1 for i in order]
    assert backend.extension("verify_find_folded") is not None
    folded = BLS.verify_batch_find(objs, rng=random.Random(1), fold=True)
    plain = BLS.verify_batch_find(objs, rng=random.Random(1))
    assert folded == plain == expect == BLS.verify_batch(objs)
