"""Threshold dealing, recovery and share signing for secrets on the GPU (csrc/blsgpu_frsecret.hip on the masked forms of
csrc/fr_scalar.h): blsgpu_threshold_deal_secret against the reference's dealings (tests/golden/dkg.json), Python integers and
the digit-indexed blsgpu_g1_mul_gen; blsgpu_fr_interpolate_at_zero_secret against blsgpu_fr_interpolate_at_zero and the
reference's vectors (lagrange.json); blsgpu_sign_threshold against the default PrivateKey.sign_threshold_batch and the
reference's combined signatures (threshold.json); and the secret=True keyword of the three Python calls.

k_fr_poly_eval_secret serves a polynomial with workgroups of 256 points, 64 per wavefront: the point counts sit on those
boundaries +-1.  k_fr_dot_secret has k_lagrange's shapes: whole groups per 256-thread workgroup up to k = 256, one group per
workgroup above."""
import ctypes
import random

import pytest

from bls_py import hostmath as H
from frsecret_vectors import N, be32, dealers, fragments, ints32, values
from lagrange_vectors import by_k, group_players, group_values

pytestmark = pytest.mark.gpu

NX = [1, 63, 64, 65, 255, 256, 257]
EINVAL = -22


@pytest.fixture
def hip_backend(engine):
    from bls_py import backend
    old = backend._provider
    backend.use(backend.HipProvider())
    yield
    backend.use(old)


# ---- dealing ---------------------------------------------------------------------------------------------------------------
def test_dealing_against_the_reference_dealings(engine, golden):
    shapes = []
    for T, n_players, ds in dealers(golden("dkg.json")):
        shapes.append((T, n_players))
        coeffs = bytes.fromhex("".join(c for d in ds for c in d["coefficients"]))
        commit, frag = engine.threshold_deal_secret(coeffs, T, be32(range(1, n_players + 1)))
        assert commit.hex() == "".join(c for d in ds for c in d["commitments"])
        assert frag.hex() == "".join(f for d in ds for f in d["fragments"])
    assert shapes == [(1, 1), (2, 3), (3, 5), (5, 7)]


@pytest.mark.parametrize("t", [1, 2, 67, 1024])
def test_dealing_against_python_integers(engine, t):
    for n_polys in (1, 3):
        coeffs = values(1000 * t + n_polys, n_polys * t)
        cb = be32(coeffs)
        want_commit, _ = engine.g1_mul_gen(cb)
        for n_x in ([65, 257] if t == 1024 else NX):
            xs = values(7 * n_x + t, n_x)
            want_frag = fragments(coeffs, t, xs)
            commit, frag = engine.threshold_deal_secret(cb, t, be32(xs))
            assert frag == want_frag, (n_polys, t, n_x)
            assert commit == want_commit, (n_polys, t, n_x)
            # each output alone
            assert engine.threshold_deal_secret(cb, t, be32(xs), commit=False) == (None, want_frag)
            assert engine.threshold_deal_secret(cb, t, None, frag=False) == (want_commit, None)
    assert engine.threshold_deal_secret(coeffs, t, xs) == (commit, frag)             # ints


def test_dealing_refusals_leave_the_outputs_untouched(engine):
    L = engine.lib
    D = L.blsgpu_threshold_deal_secret
    co, x = be32(values(3, 1025 * 2)), be32([1, 2, 3])
    commit = ctypes.create_string_buffer(b"\xAA" * (96 * 2050), 96 * 2050)
    frag = ctypes.create_string_buffer(b"\xAA" * (32 * 6), 32 * 6)
    assert D(engine.h, co, 2, 1025, x, 3, commit, frag) == EINVAL                    # t above BLSGPU_LAGRANGE_MAX_K
    assert D(engine.h, co, 2, 0, x, 3, commit, frag) == EINVAL
    assert D(engine.h, co, 0, 0, x, 3, commit, frag) == EINVAL                       # (t is checked before the empty call)
    assert D(engine.h, None, 2, 4, x, 3, commit, frag) == EINVAL
    assert D(engine.h, co, 2, 4, x, 3, None, None) == EINVAL
    assert D(engine.h, co, 2, 4, x, 0, commit, frag) == EINVAL                       # fragments at no point
    assert D(engine.h, co, 2, 4, None, 3, commit, frag) == EINVAL
    assert D(None, co, 2, 4, x, 3, commit, frag) == EINVAL
    assert L.blsgpu_threshold_deal_secret_dev(engine.h, None, 2, 4, None, 3, None, None, None) == EINVAL
    assert L.blsgpu_threshold_deal_secret_dev(engine.h, None, 2, 1025, None, 3, None, None, None) == EINVAL
    assert D(engine.h, None, 0, 4, None, 0, commit, frag) == 0                       # n_polys == 0: nothing written
    assert L.blsgpu_threshold_deal_secret_dev(engine.h, None, 0, 4, None, 0, None, None, None) == 0
    assert commit.raw == b"\xAA" * len(commit.raw) and frag.raw == b"\xAA" * len(frag.raw)
    assert D(engine.h, co, 2, 4, None, 0, commit, None) == 0                         # without fragments x is not looked at
    assert commit.raw[:96 * 8] == engine.g1_mul_gen(co[:32 * 8])[0] and commit.raw[96 * 8:] == b"\xAA" * (96 * 2042)


# ---- recovery --------------------------------------------------------------------------------------------------------------
def _players(rnd, k):
    edge = [1, 2, N - 1, N - 2, 2**200, 2**32 - 1, 2**32]
    X = set(edge[:k])
    while len(X) < k:
        X.add(rnd.randrange(1, N))
    X = list(X)
    rnd.shuffle(X)
    return X


@pytest.mark.parametrize("groups,k", [(1, 1), (3, 67), (5, 256), (2, 257), (1, 1024)])
def test_interpolation_equals_the_default_call(engine, groups, k):
    rnd = random.Random(31 * groups + k)
    Xs = [_players(rnd, k) for _ in range(groups)]
    if groups >= 3:
        Xs[1][k // 2] = Xs[1][0]                                                 # a repeated point: status 0, output 0
        Xs[2][k - 1] = 0                                                         # x = 0 likewise
    x = be32([v for X in Xs for v in X])
    y = be32(values(k + groups, k * groups))
    want = engine.fr_interpolate_at_zero(x, y, k, groups)
    got = engine.fr_interpolate_at_zero_secret(x, y, k, groups)
    assert got == want
    res, status = got
    assert status == (b"\x01\x00\x00" + b"\x01" * (groups - 3) if groups >= 3 else b"\x01" * groups)
    if groups >= 3:
        assert res[32:96] == bytes(64)
    # and Python integers for the first group
    co, _ = engine.lagrange_at_zero(x[:32 * k], k, 1)
    assert ints32(res[:32]) == [sum(l * (v % N) for l, v in zip(ints32(co), ints32(y[:32 * k]))) % N]


def test_interpolation_recovers_the_fixture_secrets(engine, golden):
    for k, gs in by_k(golden("lagrange.json")["groups"]).items():
        x = be32([v for g in gs for v in group_players(g)])
        y = be32([v for g in gs for v in group_values(g)])
        res, status = engine.fr_interpolate_at_zero_secret(x, y, k, len(gs))
        assert status == b"\x01" * len(gs)
        assert res.hex() == "".join(g["interpolate"] for g in gs), k


# ---- threshold signing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3_of_5", "67_of_100"])
def test_sign_threshold_batch_against_the_reference_sessions(engine, golden, hip_backend, name):
    """The fixture's unit_sigs are plain PrivateKey.sign outputs, not sign_threshold outputs: a unit signature of the secret
    form is lambda_i times one of them (checked on the host for the small session), and their plain sum is `combined`."""
    from bls_py.bls import BLS
    from bls_py.keys import PrivateKey
    from bls_py.signature import Signature
    th = golden("threshold.json")[name]
    players = th["players"]
    sks = [PrivateKey(int(s, 16)) for s in th["shares"]]
    msg = bytes.fromhex(th["msg"])
    want = PrivateKey.sign_threshold_batch(sks, msg, players)
    got = PrivateKey.sign_threshold_batch(sks, msg, players, secret=True)
    assert got == want and [s.serialize() for s in got] == [s.serialize() for s in want]
    assert BLS.aggregate_sigs_simple(got).serialize().hex() == th["combined"]
    if len(players) <= 3:
        for sig, unit, lam in zip(got, th["unit_sigs"], th["lambdas"]):
            assert sig.value == Signature.from_bytes(bytes.fromhex(unit)).value * int(lam, 16)


def test_sign_threshold_sessions_and_messages(engine):
    from bls_py.util import hash256
    rnd = random.Random(0x7468)
    groups, k = 3, 67
    Xs = [rnd.sample(range(1, 101), k) for _ in range(groups)]
    sks = [[rnd.randrange(2**256) for _ in range(k)] for _ in range(groups)]
    sks[1][5] = 0                                                                    # a key 0: infinity
    sks[2][0] = N                                                                    # and n, which is 0 mod n
    hashes = [hash256(b"session %d" % g) for g in range(groups)]
    x, sk = be32([v for X in Xs for v in X]), be32([v for S in sks for v in S])
    aff, ser, inf, status = engine.sign_threshold(sk, x, k, b"".join(hashes), groups)
    assert status == b"\x01\x01\x01"
    assert [i for i, f in enumerate(inf) if f] == [k + 5, 2 * k]
    assert aff[192 * (k + 5):192 * (k + 6)] == bytes(192) and ser[96 * 2 * k:96 * (2 * k + 1)] == bytes(96)
    # a message per session equals three one-session calls
    for g in range(groups):
        one = engine.sign_threshold(be32(sks[g]), be32(Xs[g]), k, hashes[g], 1)
        assert one == (aff[192 * k * g:192 * k * (g + 1)], ser[96 * k * g:96 * k * (g + 1)], inf[k * g:k * (g + 1)], b"\x01")
    # and they are (lambda sk mod n) H(m): the G2 sum path on the same scalars
    co, _ = engine.lagrange_at_zero(be32(Xs[0]), k, 1)
    scal = [l * (s % N) % N for l, s in zip(ints32(co), sks[0])]
    want, _ = engine.g2_msm(engine.hash_to_g2(hashes[0]) * k, scal, 1, k)
    assert aff[:192 * k] == want
    # one message for every session (the shared table) equals the per-session form on the repeated message
    shared = engine.sign_threshold(sk, x, k, hashes[1], groups)
    assert shared == engine.sign_threshold(sk, x, k, hashes[1] * groups, groups)
    assert shared[0][192 * k:192 * 2 * k] == aff[192 * k:192 * 2 * k]
    # each output alone
    assert engine.sign_threshold(sk, x, k, hashes[1], groups, ser=False) == (shared[0], None, shared[2], shared[3])
    assert engine.sign_threshold(sk, x, k, b"".join(hashes), groups, aff=False) == (None, ser, inf, status)
    # a session where the reference asserts: status 0, every signer's point at infinity
    Xs[1][3] = Xs[1][4]
    bad = engine.sign_threshold(sk, be32([v for X in Xs for v in X]), k, b"".join(hashes), groups)
    assert bad[3] == b"\x01\x00\x01" and all(bad[2][k:2 * k]) and bad[0][192 * k:192 * 2 * k] == bytes(192 * k)
    assert bad[0][:192 * k] == aff[:192 * k] and bad[0][192 * 2 * k:] == aff[192 * 2 * k:]


def test_sign_threshold_refusals_leave_the_outputs_untouched(engine):
    L = engine.lib
    S = L.blsgpu_sign_threshold
    n = 9
    sk, x, h = be32(range(5, 5 + n)), be32(range(1, 1 + n)), bytes(96)
    outs = [ctypes.create_string_buffer(b"\xAA" * m, m) for m in (192 * n, 96 * n, n, 3)]
    o = [ctypes.cast(b, ctypes.c_void_p) for b in outs]
    assert S(engine.h, sk, x, 3, 3, h, 2, *o) == EINVAL                              # n_msg neither 1 nor groups
    assert S(engine.h, sk, x, 0, 3, h, 1, *o) == EINVAL
    assert S(engine.h, sk, x, 1025, 3, h, 1, *o) == EINVAL
    assert S(engine.h, None, x, 3, 3, h, 1, *o) == EINVAL
    assert S(engine.h, sk, None, 3, 3, h, 1, *o) == EINVAL
    assert S(engine.h, sk, x, 3, 3, None, 1, *o) == EINVAL
    assert S(engine.h, sk, x, 3, 3, h, 1, None, None, o[2], o[3]) == EINVAL
    assert S(engine.h, sk, x, 3, 3, h, 1, o[0], o[1], o[2], None) == EINVAL
    assert S(None, sk, x, 3, 3, h, 1, *o) == EINVAL
    assert L.blsgpu_sign_threshold_dev(engine.h, None, None, 3, 3, None, 2, None, None, None, None, None) == EINVAL
    assert L.blsgpu_fr_interpolate_at_zero_secret(engine.h, x, sk, 1025, 1, o[0], o[3]) == EINVAL
    assert L.blsgpu_fr_interpolate_at_zero_secret(engine.h, x, None, 3, 3, o[0], o[3]) == EINVAL
    assert S(engine.h, None, None, 3, 0, None, 1, *o) == 0                           # groups == 0: nothing written
    assert L.blsgpu_fr_interpolate_at_zero_secret(engine.h, None, None, 3, 0, o[0], o[3]) == 0
    assert all(b.raw == b"\xAA" * len(b.raw) for b in outs)
    assert S(engine.h, sk, x, 3, 3, h, 1, o[0], None, None, o[3]) == 0               # out_inf is optional
    assert outs[3].raw == b"\x01\x01\x01" and outs[1].raw == b"\xAA" * (96 * n)


# ---- device forms ----------------------------------------------------------------------------------------------------------
def test_dev_forms_on_a_stream(engine):
    import torch
    from bls_py.util import hash256
    dev = torch.device("cuda", 0)

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def guarded(nbytes, guard):
        return torch.full((nbytes + guard,), 0xAA, dtype=torch.uint8, device=dev)

    def down(tn):
        return bytes(tn.cpu().numpy())
    n_polys, t, n_x = 3, 5, 65                                               # 191 spare lanes per polynomial
    coeffs, xs = values(11, n_polys * t), values(12, n_x)
    groups, k = 3, 67
    rnd = random.Random(5)
    X = be32([v for _ in range(groups) for v in rnd.sample(range(1, 1000), k)])
    Y = be32(values(13, groups * k))
    hashes = b"".join(hash256(b"dev %d" % g) for g in range(groups))
    want_deal = engine.threshold_deal_secret(coeffs, t, xs)
    want_dot = engine.fr_interpolate_at_zero_secret(X, Y, k, groups)
    want_sig = engine.sign_threshold(Y, X, k, hashes, groups)
    d_co, d_xs, d_X, d_Y, d_h = up(be32(coeffs)), up(be32(xs)), up(X), up(Y), up(hashes)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        d_commit, d_frag = guarded(96 * n_polys * t, 96), guarded(32 * n_polys * n_x, 32)
        d_frag1 = guarded(32 * n_polys * n_x, 32)
        d_out, d_st = guarded(32 * groups, 32), guarded(groups, 1)
        d_aff, d_ser, d_inf, d_st2 = guarded(192 * groups * k, 192), guarded(96 * groups * k, 96), guarded(groups * k, 1), guarded(groups, 1)
        s = stream.cuda_stream
        engine.threshold_deal_secret_dev(d_co.data_ptr(), n_polys, t, d_xs.data_ptr(), n_x, d_commit.data_ptr(), d_frag.data_ptr(), s)
        engine.threshold_deal_secret_dev(d_co.data_ptr(), n_polys, t, d_xs.data_ptr(), n_x, None, d_frag1.data_ptr(), s)
        engine.fr_interpolate_at_zero_secret_dev(d_X.data_ptr(), d_Y.data_ptr(), k, groups, d_out.data_ptr(), d_st.data_ptr(), s)
        engine.sign_threshold_dev(d_Y.data_ptr(), d_X.data_ptr(), k, groups, d_h.data_ptr(), groups, d_aff.data_ptr(), d_ser.data_ptr(),
                                  d_inf.data_ptr(), d_st2.data_ptr(), s)
    stream.synchronize()
    # the spare lanes store nothing: the record behind the last one is untouched
    assert down(d_commit) == want_deal[0] + b"\xaa" * 96
    assert down(d_frag) == want_deal[1] + b"\xaa" * 32 and down(d_frag1) == down(d_frag)
    assert down(d_out) == want_dot[0] + b"\xaa" * 32 and down(d_st) == want_dot[1] + b"\xaa"
    assert down(d_aff) == want_sig[0] + b"\xaa" * 192 and down(d_ser) == want_sig[1] + b"\xaa" * 96
    assert down(d_inf) == bytes(want_sig[2]) + b"\xaa" and down(d_st2) == want_sig[3] + b"\xaa"


def test_python_secret_keyword(engine, hip_backend, golden):
    from bls_py.fields import Fq
    from bls_py.keys import PrivateKey
    from bls_py.threshold import Threshold
    out = PrivateKey.new_threshold_batch(3, 5, 4, secret=True)
    assert len(out) == 4
    for sk, commitments, frags in out:
        assert len(commitments) == 3 and len(frags) == 5 and all(type(f) is Fq and f.Q == N for f in frags)
        assert commitments[0] == sk.get_public_key().value.to_affine()
        assert all(Threshold.verify_secret_fragment_batch(3, frags, range(1, 6), [commitments] * 5))
        assert int(Threshold.interpolate_at_zero_batch([[2, 4, 5]], [[frags[1], frags[3], frags[4]]], secret=True)[0]) == sk.value
    with pytest.raises(ValueError):
        Threshold.interpolate_at_zero_batch([list(range(1, 1026))], [list(range(1, 1026))], secret=True)


def test_timing_kind_and_workspace():
    """a fresh context: the scalar kernels are timing kind 10 beside the G1 (9) and G2 (8) halves, and the workspace of
    blsgpu_sign_threshold is counted in the total once"""
    from bls_py import _native
    e = _native.Engine(0)
    try:
        e.timing_enable(True)
        e.threshold_deal_secret([1, 2, 3, 4], 2, [1, 2, 3])
        assert sorted(k for k, _ in e.timing_read()) == [9, 10]
        e.fr_interpolate_at_zero_secret([1, 2, 3], [4, 5, 6], 3)
        assert [k for k, _ in e.timing_read()] == [10]
        before = e.workspace_bytes()
        sk, x, h = be32(range(5, 11)), be32([1, 2, 3, 1, 2, 4]), bytes(64)
        e.sign_threshold(sk, x, 3, h, 2)
        kinds = [k for k, _ in e.timing_read()]                          # (the hash to G2 between them records kinds of its own)
        assert kinds.count(10) == 1 and kinds.count(8) == 1 and kinds.index(10) < kinds.index(8)
        first = e.workspace_bytes()
        e.sign_threshold(sk, x, 3, h, 2)
        assert e.workspace_bytes() == first
        assert first["total"] - before["total"] >= 6 * 32 + 6 * 192
        e.timing_enable(False)
    finally:
        e.close()
