"""The receiving side of key generation for secrets on the GPU: blsgpu_g1_poly_check_secret (k_poly_eval_secret,
csrc/blsgpu_g1poly.hip) against blsgpu_g1_poly_check byte for byte -- status and Horner values -- and against Python
integers where they decide; blsgpu_fr_sum_secret (k_fr_sum_secret, csrc/blsgpu_frsecret.hip) against Python integers and
blsgpu_g1_mul_gen; and the secret=True keyword of Threshold.verify_secret_fragment_batch and BLS.aggregate_priv_keys_batch
over every dealing of tests/golden/dkg.json.

k_poly_eval_secret runs one fragment per lane in workgroups of 256, 64 per wavefront, and the spare lanes of the last
workgroup repeat the last fragment: the fragment counts sit on those boundaries +-1.  k_fr_sum_secret packs whole groups
into a workgroup of 256 lanes up to k = 256 and strides one group over a workgroup above."""
import ctypes
import random

import pytest

from dkg_vectors import check_records, dealing_records
from frsecret_vectors import dealers
from rxsecret_vectors import (H, N, R, X_EDGE, be32, fragment_case, ints32, poly_eval, seeded_coeffs, sum_values, sums)

pytestmark = pytest.mark.gpu

COUNTS = [1, 63, 64, 65, 255, 256, 257]
EINVAL = -22


@pytest.fixture
def hip_backend(engine):
    from bls_py import backend
    old = backend._provider
    backend.use(backend.HipProvider())
    yield
    backend.use(old)


def _order3():
    """11 G1 + (0, 2): on the curve, order 3 n"""
    g = H.aff_to_jac(H.F1, H.G1_GEN)
    return H.jac_to_affine(H.F1, H.jac_add(H.F1, H.jac_mul(H.F1, g, 11), H.aff_to_jac(H.F1, (0, 2))))


def _parity(engine, commit, n_polys, t, poly, x, s, want=None):
    """both calls on one input: equal status and Horner bytes; `want`: the status Python integers give"""
    st0, aff0 = engine.g1_poly_check(commit, n_polys, t, poly, x, s, aff=True)
    st1, aff1 = engine.g1_poly_check_secret(commit, n_polys, t, poly, x, s, aff=True)
    assert st1 == st0 and aff1 == aff0
    assert engine.g1_poly_check_secret(commit, n_polys, t, poly, x, s) == (st0, None)
    if want is not None:
        assert list(st1) == want
    return st1


# ---- the share check -------------------------------------------------------------------------------------------------------
def test_every_dealing_of_the_fixture(engine, golden):
    shapes = []
    for T, n_players, ds in dealers(golden("dkg.json")):
        shapes.append((T, n_players))
        commit = bytes.fromhex("".join(c for d in ds for c in d["commitments"]))
        poly = [j for j in range(len(ds)) for _ in range(n_players)]
        x = list(range(1, n_players + 1)) * len(ds)
        s = [int(f, 16) for d in ds for f in d["fragments"]]
        _parity(engine, commit, len(ds), T, poly, x, s, [1] * len(s))
        s[-1] ^= 1
        _parity(engine, commit, len(ds), T, poly, x, s, [1] * (len(s) - 1) + [0])
    assert shapes == [(1, 1), (2, 3), (3, 5), (5, 7)]


@pytest.mark.parametrize("t", [1, 2, 5])
def test_full_width_points_and_literal_fragments(engine, t):
    """P(x), P(x) + n and P(x) + m n are one point; +-1, 0 and 2^256 - 1 are not (unless Python integers say so)"""
    rnd = random.Random(300 + t)
    coeffs = seeded_coeffs(310 + t, 3, t)
    commit, _ = engine.g1_mul_gen(coeffs)
    xs = X_EDGE + [rnd.randrange(R) for _ in range(3)]
    poly, x, s, want = fragment_case(coeffs, t, xs)
    assert len(poly) == 3 * 10 * 7 and {0, 1} == set(want)            # 210 lanes: polynomial 1 begins inside wavefront 1
    _parity(engine, commit, 3, t, poly, x, s, want)


def test_t67_players_up_to_2_16(engine):
    rnd = random.Random(67)
    coeffs = seeded_coeffs(671, 3, 67)
    commit, _ = engine.g1_mul_gen(coeffs)
    xs = [1, 2, 100, 2**16] + [rnd.randrange(1, 2**16 + 1) for _ in range(2)]
    poly, x, s, want = fragment_case(coeffs, 67, xs)
    _parity(engine, commit, 3, 67, poly, x, s, want)


@pytest.mark.parametrize("n_polys", [1, 3])
def test_fragment_counts_around_wavefront_and_workgroup(engine, n_polys):
    t = 3
    rnd = random.Random(40 + n_polys)
    coeffs = seeded_coeffs(41 + n_polys, n_polys, t)
    commit, _ = engine.g1_mul_gen(coeffs)
    polys = [coeffs[j * t:(j + 1) * t] for j in range(n_polys)]
    for n in COUNTS:
        poly = sorted(rnd.randrange(n_polys) for _ in range(n))       # sorted: the polynomial changes inside a workgroup
        x = [rnd.choice((rnd.randrange(1, 200), rnd.randrange(R))) for _ in range(n)]
        s, want = [], []
        for i in range(n):
            f = poly_eval(polys[poly[i]], x[i] % N)
            bad = i % 7 == 3 or i == n - 1 > 0                        # the last fragment -- the one spare lanes repeat -- is wrong
            s.append((f + 1) % N if bad else f + (N if i % 5 == 0 else 0))
            want.append(0 if bad else 1)
        _parity(engine, commit, n_polys, t, poly, x, s, want)


def test_infinity_commitments(engine):
    """(0, 0) at the top, in the middle and at C_0, and a polynomial of nothing else"""
    t = 5
    coeffs = seeded_coeffs(55, 5, t, zero_at=(4, 2, 0, None))
    coeffs[4 * t:5 * t] = [0] * t
    commit, _ = engine.g1_mul_gen(coeffs)
    for j, k in enumerate((4, 2, 0)):
        assert commit[96 * (j * t + k):96 * (j * t + k + 1)] == bytes(96)
    assert commit[96 * 4 * t:] == bytes(96 * t)
    poly, x, s, want = fragment_case(coeffs, t, [0, 1, 3, N, N + 2, 2**200])
    st = _parity(engine, commit, 5, t, poly, x, s, want)
    # the all-infinity polynomial: the fragments 0, n and m n are right, and so is the edge value 0
    last = [b for b, p in zip(st, poly) if p == 4]
    assert last[:7] == [1, 1, 1, 0, 0, 1, 0]


def test_a_commitment_outside_the_subgroup_is_status_2(engine):
    rnd = random.Random(24)
    p3 = _order3()
    aff, _ = engine.g1_mul_gen([rnd.randrange(1, N) for _ in range(4)])
    g = [H.g1_from_abi(aff[96 * i:96 * (i + 1)]) for i in range(4)]
    polys = [[g[0], g[1], p3], [p3, g[2], g[3]], [g[0], None, g[1]]]    # poly 1: a non-G1 C_0 does not matter
    commit = b"".join(H.g1_affine_bytes(c) for P in polys for c in P)
    x = [3, 4, 3 << 200, 5, 6]
    st = _parity(engine, commit, 3, 3, [0, 0, 0, 1, 2], x, [1, 2, R - 1, 4, 5])
    assert list(st) == [2, 2, 2, 0, 0]


def test_refusals_leave_the_outputs_untouched(engine):
    L = engine.lib
    C = L.blsgpu_g1_poly_check_secret
    D = L.blsgpu_g1_poly_check_secret_dev
    n = 100
    commit, _ = engine.g1_mul_gen(seeded_coeffs(26, 2, 3))
    x = be32(range(1, n + 1))
    ok = (ctypes.c_uint32 * n)(*([0] * 50 + [1] * 50))
    st = ctypes.create_string_buffer(b"\xaa" * n, n)
    oa = ctypes.create_string_buffer(b"\xaa" * (96 * n), 96 * n)
    assert C(engine.h, commit, 2, 3, ok, x, None, n, st, oa) == EINVAL                 # s NULL: no evaluation-only mode
    assert C(engine.h, commit, 2, 3, ok, x, x, n, None, oa) == EINVAL                  # status NULL
    assert C(engine.h, commit, 2, 0, ok, x, x, n, st, oa) == EINVAL                    # t == 0
    assert C(engine.h, commit, 2, 0, ok, x, x, 0, st, oa) == EINVAL                    # (t is checked before the empty call)
    for idx in ([0] * 99 + [2], [1] * 50 + [2**32 - 1] + [0] * 49):                    # a polynomial index >= n_polys
        assert C(engine.h, commit, 2, 3, (ctypes.c_uint32 * n)(*idx), x, x, n, st, oa) == EINVAL
    assert C(engine.h, commit, 0, 3, ok, x, x, n, st, oa) == EINVAL
    assert C(engine.h, None, 2, 3, ok, x, x, n, st, oa) == EINVAL
    assert C(None, commit, 2, 3, ok, x, x, n, st, oa) == EINVAL                        # a NULL context
    assert D(engine.h, None, 2, 3, None, None, None, n, None, None, None) == EINVAL    # the _dev form with NULL buffers
    assert D(None, None, 2, 3, None, None, None, n, None, None, None) == EINVAL
    assert C(engine.h, commit, 2, 3, ok, x, x, 0, st, oa) == 0                         # n == 0 writes nothing
    assert C(engine.h, None, 2, 3, None, None, None, 0, None, None) == 0
    assert D(engine.h, None, 2, 3, None, None, None, 0, None, None, None) == 0
    assert st.raw == b"\xaa" * n and oa.raw == b"\xaa" * (96 * n)
    assert C(engine.h, commit, 2, 3, ok, x, x, n, st, None) == 0                       # out_aff is optional
    assert st.raw == engine.g1_poly_check(commit, 2, 3, list(ok), x, x)[0] and oa.raw == b"\xaa" * (96 * n)
    from bls_py import _native
    with pytest.raises(_native.BlsGpuError):
        engine.g1_poly_check_secret(commit, 2, 3, [0, 2], x[:64], x[:64])


# ---- the sums --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_sums_against_python_integers(engine, k):
    for groups in ((1, 3, 257) if k <= 65 else (1, 3)):
        ys = sum_values(9 * k + groups, k, groups)
        want = sums(ys, k)
        want_aff, want_ser = engine.g1_mul_gen(want)
        yb = be32(ys)
        assert engine.fr_sum_secret(yb, k, groups) == (want, None, None), (k, groups)
        assert engine.fr_sum_secret(yb, k, groups, pk=True) == (want, want_aff, want_ser), (k, groups)
        # each key output alone
        assert engine.fr_sum_secret(yb, k, groups, aff=True) == (want, want_aff, None)
        assert engine.fr_sum_secret(yb, k, groups, ser=True) == (want, None, want_ser)
    assert engine.fr_sum_secret(ys, k, groups) == (want, None, None)                    # ints


def test_sum_refusals_leave_the_outputs_untouched(engine):
    L = engine.lib
    S = L.blsgpu_fr_sum_secret
    D = L.blsgpu_fr_sum_secret_dev
    y = be32(range(1, 13))
    outs = [ctypes.create_string_buffer(b"\xaa" * m, m) for m in (32 * 4, 96 * 4, 48 * 4)]
    o = [ctypes.cast(b, ctypes.c_void_p) for b in outs]
    assert S(engine.h, y, 0, 4, *o) == EINVAL                                          # k == 0
    assert S(engine.h, y, 0, 0, *o) == EINVAL                                          # (k is checked before the empty call)
    assert S(engine.h, None, 3, 4, *o) == EINVAL
    assert S(engine.h, y, 3, 4, None, o[1], o[2]) == EINVAL                            # out is required
    assert S(None, y, 3, 4, *o) == EINVAL
    assert D(engine.h, None, 3, 4, None, None, None, None) == EINVAL
    assert D(engine.h, None, 0, 4, None, None, None, None) == EINVAL
    assert S(engine.h, None, 3, 0, *o) == 0                                            # groups == 0: nothing written
    assert D(engine.h, None, 3, 0, None, None, None, None) == 0
    assert all(b.raw == b"\xaa" * len(b.raw) for b in outs)
    assert S(engine.h, y, 3, 4, o[0], None, None) == 0                                 # the keys are optional
    assert ints32(outs[0].raw) == [6, 15, 24, 33] and outs[1].raw == b"\xaa" * (96 * 4) and outs[2].raw == b"\xaa" * (48 * 4)


# ---- device forms ----------------------------------------------------------------------------------------------------------
def test_dev_forms_on_a_stream(engine):
    import torch
    dev = torch.device("cuda", 0)

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def guarded(nbytes, guard):
        return torch.full((nbytes + guard,), 0xAA, dtype=torch.uint8, device=dev)

    def down(tn):
        return bytes(tn.cpu().numpy())
    t, n_polys = 4, 3
    coeffs = seeded_coeffs(77, n_polys, t)
    commit, _ = engine.g1_mul_gen(coeffs)
    poly, x, s, want = fragment_case(coeffs, t, [1, 2, 3, N + 4, R - 1])                # 105 lanes: 151 spare ones
    n = len(poly)
    want_st, want_aff = engine.g1_poly_check(commit, n_polys, t, poly, x, s, aff=True)
    assert list(want_st) == want
    groups, k = 5, 67
    ys = sum_values(78, k, groups)
    want_sum = sums(ys, k)
    want_pk = engine.g1_mul_gen(want_sum)
    d_commit, d_x, d_s, d_y = up(commit), up(be32(x)), up(be32(s)), up(be32(ys))
    d_poly = torch.tensor(poly, dtype=torch.int64, device=dev).to(torch.int32)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        d_st, d_aff, d_st1 = guarded(n, 1), guarded(96 * n, 96), guarded(n, 1)
        d_out, d_pka, d_pks, d_out1 = guarded(32 * groups, 32), guarded(96 * groups, 96), guarded(48 * groups, 48), guarded(32 * groups, 32)
        q = stream.cuda_stream
        engine.g1_poly_check_secret_dev(d_commit.data_ptr(), n_polys, t, d_poly.data_ptr(), d_x.data_ptr(), d_s.data_ptr(), n,
                                        d_st.data_ptr(), d_aff.data_ptr(), q)
        engine.g1_poly_check_secret_dev(d_commit.data_ptr(), n_polys, t, d_poly.data_ptr(), d_x.data_ptr(), d_s.data_ptr(), n,
                                        d_st1.data_ptr(), None, q)
        engine.fr_sum_secret_dev(d_y.data_ptr(), k, groups, d_out.data_ptr(), d_pka.data_ptr(), d_pks.data_ptr(), q)
        engine.fr_sum_secret_dev(d_y.data_ptr(), k, groups, d_out1.data_ptr(), None, None, q)
    stream.synchronize()
    # the spare lanes store nothing: the record behind the last one is untouched
    assert down(d_st) == want_st + b"\xaa" and down(d_aff) == want_aff + b"\xaa" * 96 and down(d_st1) == down(d_st)
    assert down(d_out) == want_sum + b"\xaa" * 32 and down(d_out1) == down(d_out)
    assert down(d_pka) == want_pk[0] + b"\xaa" * 96 and down(d_pks) == want_pk[1] + b"\xaa" * 48
    # a bad index: -EINVAL after the scan, nothing written
    from bls_py import _native
    d_st.fill_(0xAA)
    d_aff.fill_(0xAA)
    d_poly[n // 2] = n_polys
    with torch.cuda.stream(stream):
        with pytest.raises(_native.BlsGpuError):
            engine.g1_poly_check_secret_dev(d_commit.data_ptr(), n_polys, t, d_poly.data_ptr(), d_x.data_ptr(), d_s.data_ptr(), n,
                                            d_st.data_ptr(), d_aff.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert bool((d_st == 0xAA).all()) and bool((d_aff == 0xAA).all())


def test_timing_kinds():
    """a fresh context: k_poly_eval_secret is timing kind 9 (beside k_fix_mul_secret), k_fr_sum_secret kind 10"""
    from bls_py import _native
    e = _native.Engine(0)
    try:
        commit, _ = e.g1_mul_gen([5, 6])
        e.timing_enable(True)
        e.g1_poly_check_secret(commit, 1, 2, [0], [3], [23])
        assert [k for k, _ in e.timing_read()] == [9]
        assert e.fr_sum_secret([1, 2, 3, 4], 2, 2)[0] == be32([3, 7])
        assert [k for k, _ in e.timing_read()] == [10]
        e.fr_sum_secret([1, 2, 3, 4], 2, 2, pk=True)
        assert [k for k, _ in e.timing_read()] == [10, 9]
        e.timing_enable(False)
    finally:
        e.close()


# ---- Python end to end -----------------------------------------------------------------------------------------------------
def test_python_end_to_end_on_every_dealing(engine, hip_backend, golden):
    from bls_py.bls import BLS
    from bls_py.keys import PrivateKey, _pk_affine
    from bls_py.threshold import Threshold
    dkg = golden("dkg.json")
    records = dealing_records(dkg)
    for T, n_players, ds in dealers(dkg):
        rs = [r for r in records if r[0] == T]
        assert len(rs) == len(ds) * n_players
        # step 2: every player checks every fragment it was dealt
        got = Threshold.verify_secret_fragment_batch(T, [r[1] for r in rs], [r[2] for r in rs], [r[3] for r in rs], secret=True)
        assert got == [True] * len(rs)
        # step 3: every player's share and its public key
        columns = [[PrivateKey(int(d["fragments"][j], 16)) for d in ds] for j in range(n_players)]
        shares, pks = BLS.aggregate_priv_keys_batch(columns, secret=True, public_keys=True)
        loop = [BLS.aggregate_priv_keys(c, None, False) for c in columns]
        assert [s.value for s in shares] == [s.value for s in loop]
        assert pks == [s.get_public_key() for s in loop]
        assert [p.serialize() for p in pks] == [s.get_public_key().serialize() for s in loop]
        # the joint polynomial -- the coefficient-wise sum of the dealers' commitments -- evaluated at the player in the exponent
        by_coeff = b"".join(bytes.fromhex(d["commitments"][k]) for k in range(T) for d in ds)
        joint, inf = engine.g1_msm(by_coeff, None, len(ds), T)
        assert not any(inf)
        _, horner = engine.g1_poly_check(joint, 1, T, [0] * n_players, list(range(1, n_players + 1)), None, aff=True)
        assert horner == b"".join(_pk_affine(p) for p in pks)
    # the fixture's single checks as well: the false records and the undecided ones
    checks = check_records(dkg)
    for T in sorted({r[0] for r in checks}):
        rs = [r for r in checks if r[0] == T]
        assert Threshold.verify_secret_fragment_batch(T, [r[1] for r in rs], [r[2] for r in rs], [r[3] for r in rs], secret=True) == [r[4] for r in rs]
