"""Joint-Feldman dealing and share checks without a GPU: PrivateKey.new_threshold and Threshold.verify_secret_fragment
against vectors generated from the reference (tests/golden/dkg.json), and the batch forms new_threshold_batch /
verify_secret_fragment_batch -- their assertions, deduplication and routing -- through a host provider of the device
operations (tests/dkg_vectors.HostDKG)."""
import random

import pytest

from dkg_vectors import HostDKG, check_batch, check_records, dealing_records, point

N = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


@pytest.fixture(scope="module")
def dkg(golden):
    return golden("dkg.json")


@pytest.fixture
def host_dkg():
    from bls_py import backend
    old = backend._provider
    p = HostDKG(old)
    backend.use(p)
    yield p
    backend.use(old)


@pytest.fixture
def seeded_rng():
    from bls_py import keys
    old = keys.RNG

    def seed(s):
        keys.RNG = random.Random(s)
    yield seed
    keys.RNG = old


def _aff_hex(p):
    from bls_py import hostmath as H
    return H.g1_affine_bytes(p._aff()).hex()


def test_fixture_new_threshold(dkg, seeded_rng):
    from bls_py.keys import PrivateKey
    from bls_py.threshold import Threshold
    assert [(d["T"], d["N"]) for d in dkg["dealings"]] == [(1, 1), (2, 3), (3, 5), (5, 7)]
    for dl in dkg["dealings"]:
        T, N_ = dl["T"], dl["N"]
        seeded_rng(dl["seed"])
        for d in dl["dealers"]:
            sk, C, frags = PrivateKey.new_threshold(T, N_)
            assert sk.value == int(d["coefficients"][0], 16)
            assert [_aff_hex(c) for c in C] == d["commitments"]
            assert ["%064x" % int(f) for f in frags] == d["fragments"]
            assert [Threshold.verify_secret_fragment(T, f, j + 1, C) for j, f in enumerate(frags)] == d["verify"]


def test_fixture_single_checks(dkg):
    from bls_py.threshold import Threshold
    recs = check_records(dkg)
    assert len(recs) >= 60 and {r[4] for r in recs} == {True, False}
    for T, s, p, C, want in recs:
        assert Threshold.verify_secret_fragment(T, s, p, C) == want, (T, p)


def test_new_threshold_batch_equals_loop(seeded_rng, host_dkg):
    from bls_py.keys import PrivateKey
    for T, N_, count in ((1, 1, 1), (3, 5, 4), (4, 9, 3)):
        seeded_rng(77 + T)
        loop = [PrivateKey.new_threshold(T, N_) for _ in range(count)]
        seeded_rng(77 + T)
        host_dkg.calls.clear()
        batch = PrivateKey.new_threshold_batch(T, N_, count)
        assert host_dkg.calls == [("g1_mul_gen", count * T)]            # one device call for every commitment
        assert len(batch) == count
        for (sk, C, f), (sk2, C2, f2) in zip(loop, batch):
            assert sk.value == sk2.value
            assert C == C2 and f == f2
            assert all(type(a) is type(b) for a, b in zip(C + f, C2 + f2))
    with pytest.raises(AssertionError):
        PrivateKey.new_threshold_batch(3, 2, 1)
    assert PrivateKey.new_threshold_batch(2, 2, 0) == []


def test_fixture_through_the_batch(dkg, host_dkg):
    check_batch(dealing_records(dkg) + check_records(dkg), shuffle_seed=1)


def test_batch_assertions_before_device_work(dkg, host_dkg):
    from bls_py.fields import Fq
    from bls_py.threshold import Threshold
    d = dkg["dealings"][2]["dealers"][0]
    C = [point(h) for h in d["commitments"]]
    s = Fq(N, int(d["fragments"][0], 16))
    for args in ((3, [s, s], [1, 2], [C, C[:2]]),           # a commitment list of the wrong length
                 (3, [s, Fq(N, 0)], [1, 2], [C, C]),       # a zero fragment
                 (3, [s, s], [1, 0], [C, C]),              # player 0
                 (4, [s], [1], [C])):
        host_dkg.calls.clear()
        with pytest.raises(AssertionError):
            Threshold.verify_secret_fragment_batch(*args)
        assert host_dkg.calls == []
    with pytest.raises(ValueError):
        Threshold.verify_secret_fragment_batch(3, [s, s], [1], [C, C])
    assert Threshold.verify_secret_fragment_batch(3, [], [], []) == []


def test_batch_deduplicates_commitment_lists(dkg, host_dkg):
    from bls_py.fields import Fq
    from bls_py.threshold import Threshold
    dl = dkg["dealings"][3]
    dealers = dl["dealers"][:3]
    lists = [[point(h) for h in d["commitments"]] for d in dealers]
    copies = [[point(h) for h in d["commitments"]] for d in dealers]       # equal content, other objects
    frs, pls, cms, want = [], [], [], []
    for k in range(3):
        for j in range(dl["N"]):
            for src in (lists, copies):
                frs.append(Fq(N, int(dealers[k]["fragments"][j], 16)))
                pls.append(j + 1)
                cms.append(src[k])
                want.append(True)
    frs[5] = frs[5] + 1
    want[5] = False
    host_dkg.calls.clear()
    assert Threshold.verify_secret_fragment_batch(dl["T"], frs, pls, cms) == want
    assert host_dkg.calls == [("g1_poly_check", 3, len(frs))]


def test_batch_routing(dkg, host_dkg):
    from bls_py.ec import AffinePoint
    from bls_py.fields import Fq
    from bls_py.threshold import Threshold
    from bls_py import hostmath as H
    d = dkg["dealings"][2]["dealers"][1]
    C = [point(h) for h in d["commitments"]]
    f = [Fq(N, int(h, 16)) for h in d["fragments"]]
    jac = [c.to_jacobian() for c in C]                              # not AffinePoints: the host loop
    off = list(C)
    off[1] = AffinePoint(Fq(H.Q, 1), Fq(H.Q, 1), False)            # off the curve: the host loop
    cases = [
        (f[0], 1, C), (int(f[1]), 2, C),                            # device: Fq mod n, int in [1, n)
        (f[2], 3, jac), (f[3], 4, off),
        (int(f[0]) + N, 1, C),                                      # an int >= n: the host loop
        (Fq(H.Q, int(f[0])), 1, C),                                 # an Fq mod q: the host loop
        (f[0], True, C),                                            # a player that is not an int: the host loop
        (f[4], 5 - N, C), (f[4], 5 + 3 * N, C),                     # ints, any value: the device, x = player mod n
    ]
    want = [Threshold.verify_secret_fragment(3, s, p, CC) for s, p, CC in cases]
    assert want[:2] == [True, True] and want[-2:] == [True, True]
    host_dkg.calls.clear()
    got = Threshold.verify_secret_fragment_batch(3, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    assert got == want
    assert host_dkg.calls == [("g1_poly_check", 1, 4)]
    # a commitment outside the order-n subgroup: status 2, decided by one grouped multi-scalar sum
    order3 = [r for c, r in zip(dkg["checks"], check_records(dkg)) if c["what"].startswith("order-3")]
    assert [r[4] for r in order3] == [True, True, False, False]
    host_dkg.calls.clear()
    recs = order3 + [(3, f[0], 1, C, True), (3, f[0] + 1, 1, C, False)]
    got = Threshold.verify_secret_fragment_batch(3, [r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs])
    assert got == [r[4] for r in recs]
    assert [c[0] for c in host_dkg.calls] == ["g1_poly_check", "g1_msm", "g1_mul_gen"]
    assert host_dkg.calls[1] == ("g1_msm", 3, 4)


def test_host_provider_contract():
    """the test tree's provider gives status 2 exactly where plain Horner and the reference differ"""
    from bls_py import hostmath as H
    g = H.aff_to_jac(H.F1, H.G1_GEN)
    p3 = H.jac_to_affine(H.F1, H.jac_add(H.F1, H.jac_mul(H.F1, g, 11), H.aff_to_jac(H.F1, (0, 2))))
    C = [H.G1_GEN, H.jac_to_affine(H.F1, H.jac_mul(H.F1, g, 5)), p3]
    commit = b"".join(H.g1_affine_bytes(c) for c in C) + b"".join(H.g1_affine_bytes(c) for c in C[:2] + [None])
    x = b"".join(v.to_bytes(32, "big") for v in (3 << 200, 4, 3 << 200))
    s = b"".join((v % N).to_bytes(32, "big") for v in (1 + 5 * (3 << 200) + 11 * (3 << 200) ** 2, 1, 1 + 5 * (3 << 200)))
    st, aff = HostDKG().g1_poly_check(commit, 2, 3, [0, 0, 1], x, s, aff=True)
    assert st == bytes([2, 2, 1])
    assert H.g1_from_abi(aff[192:]) == H.jac_to_affine(H.F1, H.jac_mul(H.F1, g, (1 + 5 * (3 << 200)) % H.N))
