"""Batched threshold recovery on the GPU (csrc/blsgpu_lagrange.hip): every group of tests/golden/lagrange.json (generated
from the reference) through the real engine in the host and _dev forms, the 3-of-5 combines against the reference's
bytes, status-0 groups inside good batches, the -EINVAL refusals, batch sizes around the wavefront and workgroup
boundaries against the host mirror, k = 667, and 10 000 different 67-subsets of a 67-of-100 sharing combined to the one
signature of tests/golden/threshold.json."""
import ctypes
import random

import pytest

from lagrange_vectors import (N, be32, by_k, check_batches, group_coeffs, group_players, group_values, host_coeffs, ints32,
                              unit_signatures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lag(golden):
    return golden("lagrange.json")


@pytest.fixture
def hip_backend(engine):
    from bls_py import backend
    old = backend._provider
    backend.use(backend.HipProvider())
    yield
    backend.use(old)


def _tb(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(torch.device("cuda", 0))


def _bytes(t):
    return bytes(t.cpu().numpy())


def test_fixture_groups_host_and_dev_forms(engine, lag):
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for k, gs in by_k(lag["groups"]).items():
        m = len(gs)
        x = be32([v for g in gs for v in group_players(g)])
        y = be32([v for g in gs for v in group_values(g)])
        want = be32([c for g in gs for c in group_coeffs(g)])
        want_dot = be32([int(g["interpolate"], 16) for g in gs])
        co, st = engine.lagrange_at_zero(x, k, m)
        assert st == b"\x01" * m and co == want, k
        out, st = engine.fr_interpolate_at_zero(x, y, k, m)
        assert st == b"\x01" * m and out == want_dot, k
        d_x, d_y = _tb(x), _tb(y)
        d_co = torch.full((32 * k * m,), 0xAA, dtype=torch.uint8, device=dev)
        d_st = torch.full((m,), 0xAA, dtype=torch.uint8, device=dev)
        d_out = torch.full((32 * m,), 0xAA, dtype=torch.uint8, device=dev)
        d_st2 = torch.full((m,), 0xAA, dtype=torch.uint8, device=dev)
        engine.lagrange_at_zero_dev(d_x.data_ptr(), k, m, d_co.data_ptr(), d_st.data_ptr(), stream.cuda_stream)
        engine.fr_interpolate_at_zero_dev(d_x.data_ptr(), d_y.data_ptr(), k, m, d_out.data_ptr(), d_st2.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert _bytes(d_co) == want and _bytes(d_st) == b"\x01" * m, k
        assert _bytes(d_out) == want_dot and _bytes(d_st2) == b"\x01" * m, k
    # y values of any size below 2^256 are reduced on the device
    g = by_k(lag["groups"])[5][0]
    X, Y, L = group_players(g), group_values(g), group_coeffs(g)
    big = [y + N if y + N < 2**256 else y for y in Y]
    out, _ = engine.fr_interpolate_at_zero(X, big, 5, 1)
    assert int.from_bytes(out, "big") == sum(l * y for l, y in zip(L, Y)) % N


def test_three_of_five_combines_against_the_reference(engine, lag, hip_backend):
    import torch
    cb = lag["combine"]
    subs = cb["subsets"]
    unit = [bytes.fromhex(h) for h in cb["unit_sigs"]]
    from bls_py import hostmath as H
    want = b"".join(H.g2_affine_bytes(H.g2_decompress(bytes.fromhex(s["aggregate"]))) for s in subs)
    sigs = b"".join(unit[p - 1] for s in subs for p in s["players"])
    x = be32([p for s in subs for p in s["players"]])
    out, inf, st = engine.threshold_combine(sigs, x, 3, 10)
    assert out == want and not any(inf) and st == b"\x01" * 10
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    d_sigs, d_x = _tb(sigs), _tb(x)
    d_out = torch.full((192 * 10,), 0xAA, dtype=torch.uint8, device=dev)
    d_inf = torch.full((10,), 0xAA, dtype=torch.uint8, device=dev)
    d_st = torch.full((10,), 0xAA, dtype=torch.uint8, device=dev)
    engine.threshold_combine_dev(d_sigs.data_ptr(), d_x.data_ptr(), 3, 10, d_out.data_ptr(), d_inf.data_ptr(), d_st.data_ptr(),
                                 stream.cuda_stream)
    stream.synchronize()
    assert _bytes(d_out) == want and _bytes(d_inf) == bytes(10) and _bytes(d_st) == b"\x01" * 10
    assert engine.workspace_bytes()["total"] >= 10 * 3 * 32                   # the coefficients count in the total
    # the Python batch methods over the whole fixture, on the real engine
    check_batches(lag)
    check_batches(lag, shuffle_seed=9)


def test_status_zero_groups_inside_a_batch(engine, lag):
    rnd = random.Random(41)
    k, m = 5, 200
    Xs = [rnd.sample(range(1, 1000), k) for _ in range(m)]
    bad = {3: "dup", 64: "zero", 65: "n", 130: "n+1", 199: "dup-last", 100: "2^256-1"}
    Xs[3][4] = Xs[3][0]
    Xs[64][2] = 0
    Xs[65][0] = N
    Xs[130][4] = N + 1
    Xs[199][3] = Xs[199][4]
    Xs[100][1] = 2**256 - 1
    x = be32([v for X in Xs for v in X])
    co, st = engine.lagrange_at_zero(x, k, m)
    assert [g for g in range(m) if st[g] != 1] == sorted(bad)
    assert all(b in (0, 1) for b in st)
    for g in range(m):
        got = ints32(co[32 * k * g:32 * k * (g + 1)])
        assert got == ([0] * k if g in bad else host_coeffs(Xs[g])[0]), g
    ys = [rnd.randrange(N) for _ in range(k * m)]
    out, st2 = engine.fr_interpolate_at_zero(x, ys, k, m)
    assert st2 == st
    assert all(int.from_bytes(out[32 * g:32 * (g + 1)], "big") == 0 for g in bad)
    # combine: a flagged group is the all-zero point with out_inf = 1
    cb = lag["combine"]
    unit = [bytes.fromhex(h) for h in cb["unit_sigs"]]
    players = [[1, 2, 3], [2, 2, 5], [4, 5, 1], [0, 1, 2], [3, 4, 5]]
    sigs = b"".join(unit[max(p, 1) - 1] for P in players for p in P)
    out, inf, st = engine.threshold_combine(sigs, be32([p for P in players for p in P]), 3, 5)
    assert st == bytes([1, 0, 1, 0, 1]) and inf == [False, True, False, True, False]
    from bls_py import hostmath as H
    master = H.g2_affine_bytes(H.g2_decompress(bytes.fromhex(cb["master"])))
    assert [out[192 * g:192 * (g + 1)] for g in range(5)] == [master, bytes(192), master, bytes(192), master]


def test_einval_refusals_and_empty_batches(engine):
    from bls_py import _native
    L = _native.load_library()
    kmax = _native.LAGRANGE_MAX_K
    x = be32(range(1, 9))
    fill = b"\xaa" * 256
    for k, groups, xin in ((0, 4, x), (kmax + 1, 1, x), (2, 4, None)):
        co, st = ctypes.create_string_buffer(fill, 256), ctypes.create_string_buffer(fill, 256)
        assert L.blsgpu_lagrange_at_zero(engine.h, xin, k, groups, co, st) == -22, (k, groups)
        assert L.blsgpu_fr_interpolate_at_zero(engine.h, xin, x, k, groups, co, st) == -22
        assert L.blsgpu_threshold_combine(engine.h, bytes(192 * 8), xin, k, groups, co, None, st) == -22
        assert L.blsgpu_lagrange_at_zero_dev(engine.h, None, k, groups, None, None, None) == -22
        assert L.blsgpu_fr_interpolate_at_zero_dev(engine.h, None, None, k, groups, None, None, None) == -22
        assert L.blsgpu_threshold_combine_dev(engine.h, None, None, k, groups, None, None, None, None) == -22
        assert co.raw == fill and st.raw == fill                               # nothing written
    co, st = ctypes.create_string_buffer(fill, 256), ctypes.create_string_buffer(fill, 256)
    assert L.blsgpu_lagrange_at_zero(engine.h, x, 2, 4, None, st) == -22
    assert L.blsgpu_lagrange_at_zero(engine.h, x, 2, 4, co, None) == -22
    assert L.blsgpu_fr_interpolate_at_zero(engine.h, x, None, 2, 4, co, st) == -22
    assert L.blsgpu_threshold_combine(engine.h, None, x, 2, 4, co, None, st) == -22
    assert L.blsgpu_lagrange_at_zero(None, x, 2, 4, co, st) == -22
    # groups == 0 writes nothing and returns 0
    assert L.blsgpu_lagrange_at_zero(engine.h, None, 2, 0, co, st) == 0
    assert L.blsgpu_fr_interpolate_at_zero(engine.h, None, None, 2, 0, co, st) == 0
    assert L.blsgpu_threshold_combine(engine.h, None, None, 2, 0, co, None, st) == 0
    assert L.blsgpu_lagrange_at_zero_dev(engine.h, None, 2, 0, None, None, None) == 0
    assert co.raw == fill and st.raw == fill
    assert engine.lagrange_at_zero(b"", 3, 0) == (b"", b"")
    with pytest.raises(_native.BlsGpuError):
        engine.lagrange_at_zero(be32(range(1, kmax + 2)), kmax + 1, 1)
    with pytest.raises(ValueError):
        engine.lagrange_at_zero(x, 3, 2)


def _mirror(X):
    from bls_py.threshold import Threshold
    return [int(l) for l in Threshold.lagrange_coeffs_at_zero(X)]


def test_batch_sizes_around_wavefront_and_workgroup_boundaries(engine):
    """seeded random 67-subsets of 1..100 against the host mirror (pinned to the reference by test_scheme_host.py)"""
    rnd = random.Random(42)
    k = 67
    for m in (1, 63, 64, 65, 1000):
        Xs = [rnd.sample(range(1, 101), k) for _ in range(m)]
        co, st = engine.lagrange_at_zero(be32([v for X in Xs for v in X]), k, m)
        assert st == b"\x01" * m, m
        check = range(m) if m <= 65 else sorted(set([0, 1, 2, 3, 998, 999] + rnd.sample(range(m), 40)))
        for g in check:
            assert ints32(co[32 * k * g:32 * k * (g + 1)]) == _mirror(Xs[g]), (m, g)
        # every group of the batch, cheaply: sum_j L_j = 1 and sum_j L_j x_j = 0 (a polynomial of degree < k)
        for g in range(m):
            L = ints32(co[32 * k * g:32 * k * (g + 1)])
            assert sum(L) % N == 1 and sum(l * x for l, x in zip(L, Xs[g])) % N == 0, (m, g)
    # groups of every length around the 256-lane workgroup and the 64-lane wavefront
    for k in (4, 16, 85, 86, 127, 129, 255, 256, 257, 320, 321, 1023, 1024):
        m = 3
        Xs = [rnd.sample(range(1, 3000), k) for _ in range(m)]
        co, st = engine.lagrange_at_zero(be32([v for X in Xs for v in X]), k, m)
        assert st == b"\x01" * m, k
        for g in range(m):
            L = ints32(co[32 * k * g:32 * k * (g + 1)])
            assert sum(L) % N == 1 and all(sum(l * pow(x, e, N) for l, x in zip(L, Xs[g])) % N == 0 for e in (1, 2, k - 1)), (k, g)
        if k <= 129:
            assert ints32(co[:32 * k]) == _mirror(Xs[0]), k


def test_one_batch_of_k_667(engine):
    rnd = random.Random(43)
    k, m = 667, 5
    Xs = [rnd.sample(range(1, 1001), k) for _ in range(m)]
    Xs[3][500] = Xs[3][2]                                                     # one flagged group among them
    co, st = engine.lagrange_at_zero(be32([v for X in Xs for v in X]), k, m)
    assert st == bytes([1, 1, 1, 0, 1])
    assert ints32(co[:32 * k]) == _mirror(Xs[0])
    assert ints32(co[32 * k * 4:]) == host_coeffs(Xs[4])[0]
    assert co[32 * k * 3:32 * k * 4] == bytes(32 * k)
    ys = [rnd.randrange(N) for _ in range(k * m)]
    out, _ = engine.fr_interpolate_at_zero(be32([v for X in Xs for v in X]), ys, k, m)
    L1 = ints32(co[32 * k:64 * k])
    assert int.from_bytes(out[32:64], "big") == sum(l * y for l, y in zip(L1, ys[k:2 * k])) % N


def test_10000_different_subsets_recover_the_one_signature(engine, golden):
    """10 000 groups, each a different seeded 67-subset of players 1..100 of threshold.json's 67-of-100 sharing: any 67
    shares recover the fixture's combined signature.  The 100 unit signatures P(x) H(m) are built once on the device from
    the fixture's polynomial; every group is decided on the device (status sum 10 000)."""
    from bls_py import hostmath as H, util
    th = golden("threshold.json")["67_of_100"]
    groups, k = 10000, 67
    poly = [int(c, 16) for c in th["poly"]]
    assert len(poly) == 67 and th["N"] == 100

    def share(x):
        acc = 0
        for c in reversed(poly):
            acc = (acc * x + c) % N
        return acc
    shares = [share(x) for x in range(1, 101)]
    assert [shares[p - 1] for p in th["players"]] == [int(s, 16) for s in th["shares"]]      # the fixture's own 67 players
    hm = engine.hash_to_g2(util.hash256(bytes.fromhex(th["msg"])))
    unit, inf = engine.g2_msm(hm * 100, shares, 1, 100)
    assert not any(inf)
    unit = [unit[192 * i:192 * (i + 1)] for i in range(100)]
    assert [unit[p - 1] for p in th["players"]] == [bytes.fromhex(h) for h in th["unit_sigs_affine"]]
    rnd = random.Random(10000)
    subsets, seen = [], set()
    while len(subsets) < groups:
        S = rnd.sample(range(1, 101), k)
        if frozenset(S) not in seen:
            seen.add(frozenset(S))
            subsets.append(S)
    swapped = 4321                                                            # one group holds another player's share
    sigs = bytearray(b"".join(unit[p - 1] for S in subsets for p in S))
    other = next(p for p in range(1, 101) if p not in subsets[swapped])
    sigs[192 * (k * swapped + 5):192 * (k * swapped + 6)] = unit[other - 1]
    x = be32([p for S in subsets for p in S])
    out, inf, st = engine.threshold_combine(bytes(sigs), x, k, groups)
    assert sum(st) == groups and set(st) == {1}                               # all decided on the device
    assert not any(inf)
    gold = bytes.fromhex(th["combined_affine"])
    differ = [g for g in range(groups) if out[192 * g:192 * (g + 1)] != gold]
    assert differ == [swapped]
    # and the coefficients of a few of those groups against the host mirror
    co, st = engine.lagrange_at_zero(x, k, groups)
    assert sum(st) == groups
    for g in (0, swapped, groups - 1):
        assert ints32(co[32 * k * g:32 * k * (g + 1)]) == _mirror(subsets[g])
    assert H.g2_compress(H.g2_from_abi(gold)).hex() == th["combined"]


def test_sign_threshold_batch_on_the_engine(engine, golden, lag, hip_backend):
    from bls_py import hostmath as H
    from bls_py.keys import PrivateKey
    th = golden("threshold.json")["67_of_100"]
    poly = [int(c, 16) for c in th["poly"]]
    msg = bytes.fromhex(th["msg"])

    def share(x):
        acc = 0
        for c in reversed(poly):
            acc = (acc * x + c) % N
        return acc
    rnd = random.Random(44)
    gold = H.g2_from_abi(bytes.fromhex(th["combined_affine"]))
    for _ in range(3):
        players = rnd.sample(range(1, 101), 67)
        out = PrivateKey.sign_threshold_batch([PrivateKey(share(p)) for p in players], msg, players)
        pts = b"".join(H.g2_affine_bytes(s.value.to_affine()._aff()) for s in out)
        total, inf = engine.g2_msm(pts, None, 67, 1)
        assert not inf[0] and H.g2_from_abi(total) == gold
    cb = lag["combine"]
    shares = [int(s, 16) for s in cb["shares"]]
    m35 = bytes.fromhex(cb["msg"])
    for sub in cb["subsets"][:4]:
        players = sub["players"]
        sks = [PrivateKey(shares[p - 1]) for p in players]
        out = PrivateKey.sign_threshold_batch(sks, m35, players)
        for sk, p, sig in zip(sks, players, out):
            assert sig == sk.sign_threshold(m35, p, players)
