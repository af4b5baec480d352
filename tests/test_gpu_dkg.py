"""Feldman share checks on the GPU (csrc/blsgpu_g1poly.hip): every record of tests/golden/dkg.json (generated from the
reference) through the real engine, the Horner values against hostmath, batch sizes around the wavefront, a full
100-dealer x 100-player T = 67 matrix, polynomials outside G1, the _dev form, the -EINVAL refusals, and the commitments
of PrivateKey.new_threshold_batch."""
import ctypes
import random

import pytest

from dkg_vectors import check_batch, check_records, dealing_records, horner_aff

pytestmark = pytest.mark.gpu

N = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


@pytest.fixture
def hip_backend(engine):
    from bls_py import backend
    old = backend._provider
    backend.use(backend.HipProvider())
    yield
    backend.use(old)


def _commitments(engine, scalars):
    """affine tuples (None for infinity) of c G1 from the fixed-base path"""
    from bls_py import hostmath as H
    aff, _ = engine.g1_mul_gen(scalars, ser=False)
    return [H.g1_from_abi(aff[96 * i:96 * (i + 1)]) for i in range(len(scalars))]


def _commit_bytes(polys):
    from bls_py import hostmath as H
    return b"".join(H.g1_affine_bytes(c) for P in polys for c in P)


def _order3():
    """11 G1 + (0, 2): on the curve, order 3 n"""
    from bls_py import hostmath as H
    g = H.aff_to_jac(H.F1, H.G1_GEN)
    return H.jac_to_affine(H.F1, H.jac_add(H.F1, H.jac_mul(H.F1, g, 11), H.aff_to_jac(H.F1, (0, 2))))


def test_dkg_fixture_through_the_engine(golden, hip_backend):
    dkg = golden("dkg.json")
    check_batch(dealing_records(dkg) + check_records(dkg))
    check_batch(dealing_records(dkg) + check_records(dkg), shuffle_seed=2)


def test_horner_values_against_hostmath(engine):
    from bls_py import hostmath as H
    rnd = random.Random(21)
    players = [1, 2, 3, 7, 100, 2**32 - 1, 2**200, 0, N, 2 * N, N + 5]
    for T in (1, 2, 3, 67, 200):
        polys = [_commitments(engine, [rnd.randrange(1, N) for _ in range(T)]) for _ in range(2)]
        polys[1][T // 2] = None                                     # an infinity commitment
        if T >= 3:
            polys[1][1] = _order3()                                 # outside G1: the Horner value is still exact
        heavy = T == 200
        xs = players if not heavy else [1, 3, 2**32 - 1, 2**200, N]
        poly = [j for j in range(2) for _ in xs]
        x = [v for _ in range(2) for v in xs]
        st, aff = engine.g1_poly_check(_commit_bytes(polys), 2, T, poly, x, None, aff=True)
        assert st is None
        for i, (p, v) in enumerate(zip(poly, x)):
            if heavy and v == 2**200 and p == 1:
                continue                                            # (the slowest host value: one of each kind is enough)
            assert H.g1_from_abi(aff[96 * i:96 * (i + 1)]) == horner_aff(polys[p], v), (T, p, v)


def _ragged_case(engine, n, T, n_polys, rnd):
    """n fragments over n_polys polynomials in a shuffled order (wavefronts mix polynomials); every 7th tampered"""
    coeffs = [[rnd.randrange(1, N) for _ in range(T)] for _ in range(n_polys)]
    polys = _commitments(engine, [c for cs in coeffs for c in cs])
    polys = [polys[j * T:(j + 1) * T] for j in range(n_polys)]
    poly = [rnd.randrange(n_polys) for _ in range(n)]
    x = [rnd.choice((rnd.randrange(1, 200), rnd.randrange(1, N))) for _ in range(n)]
    s, want = [], []
    for i in range(n):
        v = 0
        for c in reversed(coeffs[poly[i]]):
            v = (v * x[i] + c) % N
        bad = i % 7 == 3
        s.append((v + 1) % N if bad else v + (N if i % 5 == 0 else 0))    # s + n: reduced on the device
        want.append(0 if bad else 1)
    return polys, poly, x, s, want


def test_batch_sizes_and_ragged_wavefronts(engine):
    rnd = random.Random(22)
    for n in (1, 63, 64, 65, 4097):
        polys, poly, x, s, want = _ragged_case(engine, n, 3, 5, rnd)
        st, aff = engine.g1_poly_check(_commit_bytes(polys), 5, 3, poly, x, s, aff=True)
        assert list(st) == want, n
        # the Horner values of the same call, sampled
        for i in sorted(rnd.sample(range(n), min(n, 8))):
            from bls_py import hostmath as H
            assert H.g1_from_abi(aff[96 * i:96 * (i + 1)]) == horner_aff(polys[poly[i]], x[i]), (n, i)


def test_full_matrix_100_dealers_100_players(hip_backend):
    from bls_py import keys
    from bls_py.keys import PrivateKey
    from bls_py.threshold import Threshold
    old = keys.RNG
    keys.RNG = random.Random(67100)
    try:
        deals = PrivateKey.new_threshold_batch(67, 100, 100)
    finally:
        keys.RNG = old
    rnd = random.Random(23)
    tampered = set(rnd.sample(range(10000), 100))
    frs, pls, cms = [], [], []
    for d, (_, C, frags) in enumerate(deals):
        for j in range(100):
            k = d * 100 + j
            frs.append(frags[j] + 1 if k in tampered else frags[j])
            pls.append(j + 1)
            cms.append(C)
    got = Threshold.verify_secret_fragment_batch(67, frs, pls, cms)
    assert [k for k, ok in enumerate(got) if not ok] == sorted(tampered)
    # a few entries against the host loop
    for k in sorted(tampered)[:2] + [0, 9999]:
        assert Threshold.verify_secret_fragment(67, frs[k], pls[k], cms[k]) == got[k]


def test_non_g1_polynomials(engine, golden, hip_backend):
    from bls_py import hostmath as H
    rnd = random.Random(24)
    p3 = _order3()
    g = _commitments(engine, [rnd.randrange(1, N) for _ in range(4)])
    polys = [[g[0], g[1], p3], [p3, g[2], g[3]], [g[0], None, g[1]]]    # poly 1: a non-G1 C_0 does not matter
    x = [3, 4, 3 << 200, 5, 6]
    st, _ = engine.g1_poly_check(_commit_bytes(polys), 3, 3, [0, 0, 0, 1, 2], x, [1, 2, 3, 4, 5])
    assert list(st) == [2, 2, 2, 0, 0]
    # the reference's answers for them (status 2 decided by the grouped multi-scalar sum)
    dkg = golden("dkg.json")
    recs = [r for c, r in zip(dkg["checks"], check_records(dkg)) if c["what"].startswith("order-3")]
    assert [r[4] for r in recs] == [True, True, False, False]
    check_batch(recs)
    assert H.on_curve(H.F1, p3)


def test_dev_form_equals_host_form(engine):
    import torch
    from bls_py import _native
    rnd = random.Random(25)
    polys, poly, x, s, want = _ragged_case(engine, 3000, 4, 7, rnd)
    polys[6][2] = _order3()
    commit = _commit_bytes(polys)
    st, aff = engine.g1_poly_check(commit, 7, 4, poly, x, s, aff=True)
    assert all(b == (2 if p == 6 else w) for b, p, w in zip(st, poly, want))
    e = _native.Engine(0)
    try:
        dev = torch.device("cuda", 0)
        tb = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)     # noqa: E731
        d_commit = tb(commit)
        d_poly = torch.tensor(poly, dtype=torch.int64, device=dev).to(torch.int32)
        d_x = tb(b"".join(v.to_bytes(32, "big") for v in x))
        d_s = tb(b"".join(v.to_bytes(32, "big") for v in s))
        d_st = torch.full((3000,), 0xAA, dtype=torch.uint8, device=dev)
        d_aff = torch.full((96 * 3000,), 0xAA, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        e.g1_poly_check_dev(d_commit.data_ptr(), 7, 4, d_poly.data_ptr(), d_x.data_ptr(), d_s.data_ptr(), 3000, d_st.data_ptr(),
                            d_aff.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert bytes(d_st.cpu().numpy()) == st and bytes(d_aff.cpu().numpy()) == aff
        assert e.workspace_bytes()["total"] >= 7 * 4 * 112                 # the prepared commitments count in the total
        e.trim()
        # a bad index: -EINVAL, nothing written
        d_st.fill_(0xAA)
        d_aff.fill_(0xAA)
        d_poly[1234] = 7
        with pytest.raises(_native.BlsGpuError):
            e.g1_poly_check_dev(d_commit.data_ptr(), 7, 4, d_poly.data_ptr(), d_x.data_ptr(), d_s.data_ptr(), 3000, d_st.data_ptr(),
                                d_aff.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert bool((d_st == 0xAA).all()) and bool((d_aff == 0xAA).all())
    finally:
        e.close()


def test_einval_for_bad_indices_and_t0(engine):
    from bls_py import _native
    L = _native.load_library()
    rnd = random.Random(26)
    polys = [_commitments(engine, [rnd.randrange(1, N) for _ in range(3)]) for _ in range(2)]
    commit = _commit_bytes(polys)
    n = 100
    x = b"".join((i + 1).to_bytes(32, "big") for i in range(n))
    for idx, t in (([0] * 99 + [2], 3), ([1] * 50 + [2**32 - 1] + [0] * 49, 3), ([0] * n, 0)):
        poly = (ctypes.c_uint32 * n)(*idx)
        st = ctypes.create_string_buffer(b"\xaa" * n, n)
        oa = ctypes.create_string_buffer(b"\xaa" * (96 * n), 96 * n)
        rc = L.blsgpu_g1_poly_check(engine.h, commit, 2, t, poly, x, x, n, st, oa)
        assert rc == -22, (t, idx[-1])
        assert st.raw == b"\xaa" * n and oa.raw == b"\xaa" * (96 * n)      # nothing written
    poly = (ctypes.c_uint32 * n)(*([0] * n))
    assert L.blsgpu_g1_poly_check(engine.h, commit, 2, 3, poly, x, x, n, None, None) == -22   # no output asked for
    assert L.blsgpu_g1_poly_check(engine.h, commit, 2, 3, poly, x, None, n, ctypes.create_string_buffer(n), None) == -22
    assert L.blsgpu_g1_poly_check(engine.h, commit, 2, 3, poly, x, x, 0, None, None) == 0     # n == 0 writes nothing
    with pytest.raises(_native.BlsGpuError):
        engine.g1_poly_check(commit, 2, 3, [0, 2], x[:64], x[:64])


def test_new_threshold_batch_commitments(engine, hip_backend):
    from bls_py import keys
    from bls_py.ec import generator_Fq
    from bls_py.fields import Fq
    from bls_py.keys import PrivateKey
    old = keys.RNG
    try:
        keys.RNG = random.Random(5)
        loop = [PrivateKey.new_threshold(3, 4) for _ in range(2)]
        keys.RNG = random.Random(5)
        batch = PrivateKey.new_threshold_batch(3, 4, 2)
    finally:
        keys.RNG = old
    for (sk, C, f), (sk2, C2, f2) in zip(loop, batch):
        assert sk.value == sk2.value and C == C2 and f == f2
    keys.RNG = random.Random(6)
    try:
        big = PrivateKey.new_threshold_batch(5, 6, 20)
    finally:
        keys.RNG = old
    rng = random.Random(6)
    coeffs = [[rng.randint(1, N - 1) for _ in range(5)] for _ in range(20)]
    g1 = generator_Fq()
    for d in (0, 1, 19):
        assert big[d][1] == [g1 * Fq(N, c) for c in coeffs[d]]
        assert big[d][0].value == coeffs[d][0]
