"""Secure aggregation on the GPU: blsgpu_hash_pks (k_hash_pks_digest, k_hash_pks_exp, csrc/blsgpu_hashpks.hip) against hashlib
and Python integers with the digests computed on the device and handed in; blsgpu_aggregate_pub_keys_secure,
blsgpu_aggregate_sigs_secure and blsgpu_aggregate_priv_keys_secure against their existing compositions byte for byte -- host
hash_pks, then blsgpu_g1_msm / blsgpu_g2_msm / Python integers; the _dev forms on a stream with guard records; and the
four Python entry points over tests/golden/secure_agg.json with HipProvider.

k_hash_pks_digest runs one group per lane in workgroups of 64 and its padding has one case per k mod 4: the group counts sit
either side of a wavefront and of several workgroups, the key counts cover every k mod 4 with and without whole quads before
the tail.  k_hash_pks_exp runs one exponent per lane in workgroups of 256: m = 257 with 257 groups is 258 workgroups, the last
one with a single live lane."""
import ctypes

import pytest

from secure_agg_vectors import (H, N, Pool, be32, check_hash_pks, check_priv_keys, check_pub_keys, check_sigs, host_digests,
                                host_ts, ints32, seeded_keys)

pytestmark = pytest.mark.gpu

EINVAL = -22
KS = [1, 2, 3, 4, 5, 8, 9, 65]


@pytest.fixture
def hip_backend(engine):
    from bls_py import backend
    old = backend._provider
    backend.use(backend.HipProvider())
    yield
    backend.use(old)


# ---- the exponents ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 63, 64, 65, 257])
def test_hash_pks_against_hashlib(engine, groups):
    for k in KS:
        ser = seeded_keys(1000 * groups + k, k * groups)
        dg = host_digests(ser, k, groups)
        for m in sorted({1, k, k + 3, 257}):
            want = be32(host_ts(ser, k, m, groups, dg))
            assert engine.hash_pks(ser, k, m, groups, pk_hash=False, want_pk_hash=True) == (want, dg), (k, m, "device digests")
            assert engine.hash_pks(ser, k, m, groups, pk_hash=dg, want_pk_hash=True) == (want, dg), (k, m, "digests handed in")
            assert engine.hash_pks(ser, k, m, groups) == want, (k, m, "the 64-group rule")
    assert all(t < N for t in ints32(want))


def test_supplied_digests_are_used_as_they_are(engine):
    """with pk_hash_in the keys are not read: other digests give other exponents, and pks_ser may be NULL"""
    k, groups, m = 5, 3, 4
    dg = bytes(range(96))
    out = ctypes.create_string_buffer(32 * m * groups)
    assert engine.lib.blsgpu_hash_pks(engine.h, None, k, groups, dg, m, out, None) == 0
    assert out.raw == be32(host_ts(None, k, m, groups, dg))


# ---- the three sums against their compositions -----------------------------------------------------------------------------
def _points(engine, seed, count):
    """`count` seeded G1 points: (affine bytes, serialised bytes)"""
    import random
    rnd = random.Random(seed)
    return engine.g1_mul_gen([rnd.randrange(1, N) for _ in range(count)])


@pytest.mark.parametrize("groups", [1, 65])
@pytest.mark.parametrize("k", [1, 4, 5, 65])
def test_pub_key_sums_equal_hash_pks_then_g1_msm(engine, groups, k):
    aff, ser = _points(engine, 31 * k + groups, k * groups)
    # the last group is k points at infinity (serialised as PublicKey.serialize() writes infinity): its sum is infinity
    aff = aff[:96 * k * (groups - 1)] + bytes(96 * k)
    ser = ser[:48 * k * (groups - 1)] + (b"\xc0" + bytes(47)) * k
    want = engine.g1_msm(aff, host_ts(ser, k, k, groups), k, groups)
    assert want[1][-1] and want[0][-96:] == bytes(96) and (groups == 1 or not any(want[1][:-1]))
    assert engine.aggregate_pub_keys_secure(aff, ser, k, groups, pk_hash=False) == want
    assert engine.aggregate_pub_keys_secure(aff, ser, k, groups, pk_hash=host_digests(ser, k, groups)) == want
    assert engine.aggregate_pub_keys_secure(aff, ser, k, groups) == want
    if groups == 1 and k > 1:                                         # and a single group that is not infinity
        aff, ser = _points(engine, 77 + k, k)
        want = engine.g1_msm(aff, host_ts(ser, k, k, 1), k, 1)
        assert not want[1][0] and engine.aggregate_pub_keys_secure(aff, ser, k, 1, pk_hash=False) == want


@pytest.mark.parametrize("groups", [1, 65])
@pytest.mark.parametrize("k", [1, 4, 5, 65])
def test_signature_sums_equal_hash_pks_then_g2_msm(engine, groups, k):
    import random
    rnd = random.Random(17 * k + groups)
    g2 = H.g2_affine_bytes(H.G2_GEN)
    sigs, _, _ = engine.g2_mul_secret(g2, [rnd.randrange(1, N) for _ in range(k * groups)], ser=False)
    if groups > 1:
        sigs = sigs[:192 * k * (groups - 1)] + bytes(192 * k)         # a group of infinities
    for k_pks in (k, k + 2):                                          # the exponents may be hashed over another number of keys
        ser = seeded_keys(5 * k + k_pks, k_pks * groups)
        want = engine.g2_msm(sigs, host_ts(ser, k_pks, k, groups), k, groups)
        assert want[1][-1] == (groups > 1)
        assert engine.aggregate_sigs_secure(sigs, k, ser, k_pks, groups, pk_hash=False) == want
        assert engine.aggregate_sigs_secure(sigs, k, ser, k_pks, groups) == want
    if groups == 1:
        want = engine.g2_msm(bytes(192 * k), host_ts(ser, k + 2, k, 1), k, 1)
        assert want[1] == [True] and engine.aggregate_sigs_secure(bytes(192 * k), k, ser, k + 2, 1, pk_hash=False) == want


def _priv_case(engine, seed, k, groups):
    import random
    rnd = random.Random(seed)
    sks = [rnd.choice((rnd.randrange(N), rnd.randrange(2**256), 2**256 - 1, 0)) for _ in range(k * groups)]
    ser = seeded_keys(seed + 1, k * groups)
    ts = host_ts(ser, k, k, groups)
    want = be32([sum(t * s for t, s in zip(ts[g * k:(g + 1) * k], sks[g * k:(g + 1) * k])) % N for g in range(groups)])
    return sks, ser, want, engine.g1_mul_gen(want)


@pytest.mark.parametrize("groups", [1, 65])
@pytest.mark.parametrize("k", [1, 4, 5, 65])
def test_private_key_sums_equal_python_integers(engine, groups, k):
    sks, ser, want, (want_aff, want_ser) = _priv_case(engine, 900 + 7 * k + groups, k, groups)
    assert engine.aggregate_priv_keys_secure(sks, ser, k, groups, pk_hash=False) == (want, None, None)
    assert engine.aggregate_priv_keys_secure(be32(sks), ser, k, groups, pk=True) == (want, want_aff, want_ser)
    assert engine.aggregate_priv_keys_secure(sks, ser, k, groups, aff=True, pk_hash=host_digests(ser, k, groups)) == (want, want_aff, None)
    assert engine.aggregate_priv_keys_secure(sks, ser, k, groups, ser=True, pk_hash=False) == (want, None, want_ser)


def test_private_key_sum_at_the_k_limit(engine):
    from bls_py import _native
    k = _native.LAGRANGE_MAX_K
    sks, ser, want, (want_aff, want_ser) = _priv_case(engine, 1024, k, 2)
    assert engine.aggregate_priv_keys_secure(sks, ser, k, 2, pk=True, pk_hash=False) == (want, want_aff, want_ser)
    assert engine.aggregate_priv_keys_secure(sks, ser, k, 2, pk=True) == (want, want_aff, want_ser)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(engine):
    from bls_py import _native
    L = engine.lib
    k, groups = 3, 4
    aff, ser = _points(engine, 5, k * groups)
    sks = be32(range(1, k * groups + 1))
    sigs = bytes(192 * k * groups)
    outs = [ctypes.create_string_buffer(b"\xaa" * n, n) for n in (32 * k * groups, 32 * groups, 192 * groups, groups, 96 * groups, 48 * groups)]
    ts, dg, pt, inf, pka, pks = [ctypes.cast(b, ctypes.c_void_p) for b in outs]
    HP, PUB, SIG, PRIV = L.blsgpu_hash_pks, L.blsgpu_aggregate_pub_keys_secure, L.blsgpu_aggregate_sigs_secure, L.blsgpu_aggregate_priv_keys_secure
    assert HP(engine.h, ser, 0, groups, None, k, ts, dg) == EINVAL                       # k == 0
    assert HP(engine.h, ser, k, groups, None, 0, ts, dg) == EINVAL                       # m == 0
    assert HP(engine.h, ser, 0, 0, None, k, ts, dg) == EINVAL                            # (checked before the empty call)
    assert HP(engine.h, None, k, groups, None, k, ts, dg) == EINVAL                      # neither keys nor digests
    assert HP(engine.h, ser, k, groups, None, k, None, dg) == EINVAL
    assert HP(None, ser, k, groups, None, k, ts, dg) == EINVAL
    assert PUB(engine.h, aff, ser, None, 0, groups, pt, inf) == EINVAL
    assert PUB(engine.h, None, ser, None, k, groups, pt, inf) == EINVAL
    assert SIG(engine.h, sigs, 0, ser, k, None, groups, pt, inf) == EINVAL               # no exponents asked for
    assert SIG(engine.h, sigs, k, ser, 0, None, groups, pt, inf) == EINVAL               # no keys to hash
    assert PRIV(engine.h, sks, ser, None, 0, groups, dg, pka, pks) == EINVAL
    assert PRIV(engine.h, sks, ser, None, _native.LAGRANGE_MAX_K + 1, groups, dg, pka, pks) == EINVAL
    assert b"BLSGPU_LAGRANGE_MAX_K" in L.blsgpu_last_error()
    assert PRIV(engine.h, sks, ser, None, k, groups, None, pka, pks) == EINVAL           # out is required
    for D in (L.blsgpu_hash_pks_dev, ):
        assert D(engine.h, None, 0, groups, None, k, None, None, None) == EINVAL
        assert D(engine.h, None, k, groups, None, k, None, None, None) == EINVAL
        assert D(engine.h, None, k, 0, None, k, None, None, None) == 0
    assert L.blsgpu_aggregate_priv_keys_secure_dev(engine.h, None, None, None, _native.LAGRANGE_MAX_K + 1, 0, None, None, None, None) == EINVAL
    assert L.blsgpu_aggregate_pub_keys_secure_dev(engine.h, None, None, None, k, 0, None, None, None) == 0
    assert L.blsgpu_aggregate_sigs_secure_dev(engine.h, None, k, None, k, None, 0, None, None, None) == 0
    assert HP(engine.h, None, k, 0, None, k, None, None) == 0                            # groups == 0: nothing written
    assert PUB(engine.h, None, None, None, k, 0, None, None) == 0
    assert SIG(engine.h, None, k, None, k, None, 0, None, None) == 0
    assert PRIV(engine.h, None, None, None, k, 0, None, None, None) == 0
    assert all(b.raw == b"\xaa" * len(b.raw) for b in outs)
    assert HP(engine.h, ser, k, groups, None, k, ts, None) == 0                          # the digests are optional
    assert outs[0].raw == be32(host_ts(ser, k, k, groups)) and outs[1].raw == b"\xaa" * (32 * groups)
    with pytest.raises(_native.BlsGpuError):
        engine.aggregate_priv_keys_secure([1] * 1025, bytes(48 * 1025), 1025, 1)
    with pytest.raises(ValueError):
        engine.hash_pks(ser[:-1], k, 2, groups)


# ---- device forms ----------------------------------------------------------------------------------------------------------
def test_dev_forms_on_a_stream(engine):
    import torch
    dev = torch.device("cuda", 0)

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def guarded(nbytes, guard):
        """a record of 0xAA either side of the output"""
        return torch.full((guard + nbytes + guard,), 0xAA, dtype=torch.uint8, device=dev)

    def check(tn, want, guard):
        b = bytes(tn.cpu().numpy())
        assert b[:guard] == b"\xaa" * guard and b[len(b) - guard:] == b"\xaa" * guard, "a store outside the output"
        assert b[guard:len(b) - guard] == want

    groups, k, m = 67, 5, 9                                           # 67 lanes of the digest kernel: 61 spare ones
    aff, ser = _points(engine, 41, k * groups)
    sks, _, want_sum, want_pk = _priv_case(engine, 42, k, groups)
    ser_priv = seeded_keys(43, k * groups)
    g2 = H.g2_affine_bytes(H.G2_GEN)
    sigs, _, _ = engine.g2_mul_secret(g2, list(range(2, 2 + k * groups)), ser=False)
    dg = host_digests(ser, k, groups)
    want_ts = be32(host_ts(ser, k, m, groups, dg))
    want_pub = engine.g1_msm(aff, host_ts(ser, k, k, groups), k, groups)
    want_sig = engine.g2_msm(sigs, host_ts(ser, k, k, groups), k, groups)
    d_aff, d_ser, d_sks, d_sigs, d_dg, d_ser_priv = up(aff), up(ser), up(be32(sks)), up(sigs), up(dg), up(ser_priv)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        d_ts, d_ts1, d_odg = guarded(32 * m * groups, 32), guarded(32 * m * groups, 32), guarded(32 * groups, 32)
        d_pub, d_pinf = guarded(96 * groups, 96), guarded(groups, 1)
        d_sig, d_sinf = guarded(192 * groups, 192), guarded(groups, 1)
        d_out, d_pka, d_pks, d_out1 = guarded(32 * groups, 32), guarded(96 * groups, 96), guarded(48 * groups, 48), guarded(32 * groups, 32)
        q = stream.cuda_stream
        engine.hash_pks_dev(d_ser.data_ptr(), k, groups, None, m, d_ts.data_ptr() + 32, d_odg.data_ptr() + 32, q)
        engine.hash_pks_dev(None, k, groups, d_dg.data_ptr(), m, d_ts1.data_ptr() + 32, None, q)
        engine.aggregate_pub_keys_secure_dev(d_aff.data_ptr(), d_ser.data_ptr(), None, k, groups, d_pub.data_ptr() + 96, d_pinf.data_ptr() + 1, q)
        engine.aggregate_sigs_secure_dev(d_sigs.data_ptr(), k, d_ser.data_ptr(), k, None, groups, d_sig.data_ptr() + 192, d_sinf.data_ptr() + 1, q)
        engine.aggregate_priv_keys_secure_dev(d_sks.data_ptr(), d_ser_priv.data_ptr(), None, k, groups, d_out.data_ptr() + 32,
                                              d_pka.data_ptr() + 96, d_pks.data_ptr() + 48, q)
        engine.aggregate_priv_keys_secure_dev(d_sks.data_ptr(), d_ser_priv.data_ptr(), None, k, groups, d_out1.data_ptr() + 32, None, None, q)
    stream.synchronize()
    check(d_ts, want_ts, 32)
    check(d_ts1, want_ts, 32)
    check(d_odg, dg, 32)
    check(d_pub, want_pub[0], 96)
    check(d_pinf, bytes(want_pub[1]), 1)
    check(d_sig, want_sig[0], 192)
    check(d_sinf, bytes(want_sig[1]), 1)
    # (_priv_case hashed seeded_keys(43): ser_priv)
    check(d_out, want_sum, 32)
    check(d_out1, want_sum, 32)
    check(d_pka, want_pk[0], 96)
    check(d_pks, want_pk[1], 48)


def test_timing_kinds():
    """a fresh context: k_hash_pks_digest is timing kind 11 -- absent when the digests are handed in -- k_hash_pks_exp kind 12"""
    from bls_py import _native
    e = _native.Engine(0)
    try:
        ser = seeded_keys(3, 6)
        e.timing_enable(True)
        e.hash_pks(ser, 3, 2, 2, pk_hash=False)
        assert [k for k, _ in e.timing_read()] == [11, 12]
        e.hash_pks(ser, 3, 2, 2)
        assert [k for k, _ in e.timing_read()] == [12]
        e.aggregate_priv_keys_secure([1] * 6, ser, 3, 2, pk=True, pk_hash=False)
        assert [k for k, _ in e.timing_read()] == [11, 12, 10, 9]
        e.timing_enable(False)
    finally:
        e.close()


# ---- Python end to end -----------------------------------------------------------------------------------------------------
def test_python_end_to_end_on_the_fixture(engine, hip_backend, golden):
    fx = golden("secure_agg.json")
    pool = Pool(fx)
    check_hash_pks(fx, pool)
    check_pub_keys(fx, pool)
    check_sigs(fx, pool)
    check_priv_keys(fx, pool, secret=True)
    check_priv_keys(fx, pool, secret=False)
    # 70 groups in one call: past the 64-group rule, the device hashes the keys itself
    from bls_py.bls import BLS
    from bls_py.util import hash_pks, hash_pks_batch
    groups = [[pool.pks[(3 * g + j) % 65] for j in range(4)] for g in range(70)]
    assert hash_pks_batch(5, groups) == [hash_pks(5, g) for g in groups]
    got = BLS.aggregate_pub_keys_batch(groups, True)
    assert got[:3] == [BLS.aggregate_pub_keys(list(g), True) for g in groups[:3]] and got[69] == BLS.aggregate_pub_keys(list(groups[69]), True)
