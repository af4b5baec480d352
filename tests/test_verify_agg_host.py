"""The verify_aggregates extension without a GPU: a recording host provider (tests/subgroup_vectors.HostRLC) that offers it, the
call computed on Python integers (bls_py.hostmath) and by the CPU oracle -- host_verify_aggregates below, which the GPU test
uses as well --; BLS.verify_batch(fused=True) against BLS.verify one by one on a mixed batch, with exactly one extension call,
every shared message once in its table and the exponents handed over only where one differs from 1; status 2 decided by
BLS.verify; the default paths' calls unchanged; a provider without the extension raises; and the argument validation of
bls_py._native_veragg."""
import pytest

from subgroup_vectors import HostRLC, N, aggregates, secret_keys
from test_msmr_host import world                                             # noqa: F401  (the ragged, forged and uniform aggregates)


def neg_g1_bytes():
    from bls_py import hostmath as H
    return H.g1_affine_bytes(H.jac_to_affine(H.F1, H.jac_mul(H.F1, H.aff_to_jac(H.F1, H.G1_GEN), N - 1)))


def host_pairs(sigs, msg_hashes, keys, exps, grp_off, grp_msg, agg_off):
    """per aggregate (g1 bytes, g2 bytes, pairs, undecided) as include/blsgpu.h states the call: (-G1, sig_j), then
    (sum e_i pk_i, H(hash)) per group; a sum at infinity is (0,0); a key off the curve or a (0,0) signature leaves it undecided"""
    from bls_py import hostmath as H, util
    if isinstance(exps, (bytes, bytearray)):
        exps = [int.from_bytes(exps[32 * i:32 * (i + 1)], "big") for i in range(len(exps) // 32)]
    hm = [H.g2_affine_bytes(H.hash_to_g2_prehashed(msg_hashes[32 * i:32 * (i + 1)], util.hash512)) for i in range(len(msg_hashes) // 32)]
    neg, out = neg_g1_bytes(), []
    for j in range(len(agg_off) - 1):
        sig = sigs[192 * j:192 * (j + 1)]
        g1, g2, undecided = neg, sig, not any(sig)
        for g in range(agg_off[j], agg_off[j + 1]):
            acc, off = None, False
            for i in range(grp_off[g], grp_off[g + 1]):
                A = H.g1_from_abi(keys[96 * i:96 * (i + 1)])
                if A is not None and not H.on_curve(H.F1, A):
                    off = True
                elif A is not None:
                    acc = H.jac_add(H.F1, acc, H.jac_mul(H.F1, H.aff_to_jac(H.F1, A), 1 if exps is None else int(exps[i])))
            A = None if acc is None or off else H.jac_to_affine(H.F1, acc)
            g1, g2, undecided = g1 + H.g1_affine_bytes(A), g2 + hm[grp_msg[g]], undecided or off
        out.append((g1, g2, len(g1) // 96, undecided))
    return out


def host_verify_aggregates(O, sigs, msg_hashes, keys, exps, grp_off, grp_msg, agg_off):
    """(status bytes, m x 576 bytes) of the call by hostmath and the oracle's multi-pairing"""
    from bls_py.ec import default_ec
    from bls_py.fields import Fq12
    one = Fq12.one(default_ec.q).serialize()
    status, gt = [], b""
    for g1, g2, n, undecided in host_pairs(sigs, msg_hashes, keys, exps, grp_off, grp_msg, agg_off):
        v = O.pairing_multi(g1, g2, n, threads=8)
        status.append(2 if undecided else 1 if v == one else 0)
        gt += v
    return bytes(status), gt


class WithExtension(HostRLC):
    """a stand-in that offers the extension as a stand-in does: an attribute of that name"""

    def verify_aggregates(self, sigs, msg_hashes, keys, exps, grp_off, grp_msg, agg_off, gt=False):
        self.calls.append(("verify_aggregates", len(sigs) // 192, msg_hashes, exps, list(grp_off), list(grp_msg), list(agg_off)))
        status, out = host_verify_aggregates(self.O, sigs, msg_hashes, keys, exps, grp_off, grp_msg, agg_off)
        return status, out if gt else None


@pytest.fixture
def use(oracle):
    from bls_py import backend
    old = backend._provider

    def install(cls):
        p = cls(oracle)
        backend.use(p)
        return p
    yield install
    backend.use(old)


@pytest.fixture(scope="module")
def plain(oracle):
    """three plain aggregates of three signatures over distinct messages (exponent 1 throughout), the second forged"""
    from bls_py import backend
    old = backend._provider
    backend.use(HostRLC(oracle))
    try:
        return aggregates(3, 3, forged_at=1)
    finally:
        backend.use(old)


@pytest.fixture(scope="module")
def sharing(oracle):
    """two aggregates by different signers over the SAME two messages, and a single signature over one of them"""
    from bls_py import backend
    from bls_py.bls import BLS
    old = backend._provider
    backend.use(HostRLC(oracle))
    try:
        a, b = secret_keys(b"share-a", 2), secret_keys(b"share-b", 2)
        msgs = [b"common 0", b"common 1"]
        return [BLS.aggregate_sigs([sk.sign(m) for sk, m in zip(a, msgs)]), BLS.aggregate_sigs([sk.sign(m) for sk, m in zip(b, msgs)]),
                a[1].sign(msgs[0])]
    finally:
        backend.use(old)


def missing_key(sig):
    from bls_py.aggregation_info import AggregationInfo
    from bls_py.signature import Signature
    info = sig.aggregation_info
    tree = dict(info.tree)
    del tree[sorted(tree)[0]]
    out = Signature.from_g2(sig.value)
    out.set_aggregation_info(AggregationInfo(tree, info.message_hashes, info.public_keys))
    return out


def fused_calls(p):
    return [c for c in p.calls if c[0] == "verify_aggregates"]


def test_fused_equals_verify_one_by_one_with_one_extension_call(use, world, plain, sharing):      # noqa: F811
    from bls_py import backend
    from bls_py.bls import BLS
    ragged, forged, uniform = world                           # secure aggregates: hash_pks exponents in their trees
    batch = plain + [ragged, missing_key(uniform), forged, uniform] + sharing
    p = use(WithExtension)
    assert backend.extension("verify_aggregates") is not None
    want = [BLS.verify(s) for s in batch]
    assert want == [True, False, True, True, False, False, True, True, True, True]
    p.calls.clear()
    assert BLS.verify_batch(batch, fused=True) == want
    (call,) = fused_calls(p)
    assert [c[0] for c in p.calls] == ["verify_aggregates"]                   # nothing else: no hash, sum or pairing call
    _, m, msg_hashes, exps, grp_off, grp_msg, agg_off = call
    assert m == 9 and len(agg_off) == 10                                      # the one with the missing tree key is not sent
    hashes = [msg_hashes[32 * i:32 * (i + 1)] for i in range(len(msg_hashes) // 32)]
    assert len(set(hashes)) == len(hashes)                                    # every message hash once
    # the last three share two messages: four groups and one more over two table entries
    assert len(set(grp_msg[-5:])) == 2 and grp_msg[-5:-3] == grp_msg[-3:-1] and grp_msg[-1] in grp_msg[-5:-3]
    assert exps is not None and len(exps) == grp_off[-1] and any(int(e) != 1 for e in exps)
    assert grp_off == sorted(grp_off) and agg_off == sorted(agg_off) and agg_off[-1] == len(grp_msg)


def test_exponents_are_handed_over_only_where_one_differs_from_one(use, world, plain, sharing):   # noqa: F811
    from bls_py.bls import BLS
    p = use(WithExtension)
    assert BLS.verify_batch(plain + sharing, fused=True) == [True, False, True, True, True, True]
    (call,) = fused_calls(p)
    assert call[3] is None
    p.calls.clear()
    assert BLS.verify_batch(plain + [world[0]], fused=True) == [True, False, True, True]
    (call,) = fused_calls(p)
    assert call[3] is not None and [int(e) for e in call[3][:9]] == [1] * 9


def test_status_two_reaches_verify(use, plain):
    """an infinity signature comes back undecided (its (0,0) bytes) and is decided by BLS.verify, as is a status 2 the provider
    gives for a reason of its own"""
    from bls_py.bls import BLS
    from bls_py.ec import JacobianPoint
    from bls_py import hostmath as H
    from bls_py.signature import Signature
    inf = Signature.from_g2(JacobianPoint._from(H.F2, None))
    inf.set_aggregation_info(plain[0].aggregation_info)
    batch = [plain[0], inf, plain[1]]
    p = use(WithExtension)
    want = [BLS.verify(s) for s in batch]
    p.calls.clear()
    assert BLS.verify_batch(batch, fused=True) == want == [True, False, False]
    assert len(fused_calls(p)) == 1 and len(p.calls) > 1                      # BLS.verify's own calls follow for the undecided one

    class AllUndecided(WithExtension):
        def verify_aggregates(self, *a, **k):
            status, out = super().verify_aggregates(*a, **k)
            return bytes([2] * len(status)), out
    p = use(AllUndecided)
    assert BLS.verify_batch(batch, fused=True) == want
    assert BLS.verify_batch([], fused=True) == []


def test_the_default_paths_take_exactly_the_calls_they_took(use, world, plain):              # noqa: F811
    from bls_py.bls import BLS
    batch = list(world) + plain
    seen = []
    for cls in (HostRLC, WithExtension):
        p = use(cls)
        got = BLS.verify_batch(batch), BLS.verify_batch(batch, ragged=False, fused=False)
        assert got == ([True, False, True, True, False, True],) * 2
        seen.append([c[:3] for c in p.calls])
    assert seen[0] == seen[1] and all(c[0] != "verify_aggregates" for c in seen[1])


def test_a_provider_without_the_extension_raises(use, world):                                # noqa: F811
    from bls_py import backend
    from bls_py.bls import BLS
    p = use(HostRLC)
    assert backend.extension("verify_aggregates") is None
    with pytest.raises(NotImplementedError):
        BLS.verify_batch(list(world), fused=True)
    assert p.calls == []                                                     # raised before any work
    assert backend.VERIFY_AGG_EXTENSIONS == {"verify_aggregates": "_native_veragg"}


class FakeEngine:
    """_native.Engine's marshalling helpers over a device call that must not happen"""

    def __init__(self):
        from bls_py import _native
        self._scalars, self._indices = _native.Engine._scalars, _native.Engine._indices
        self.calls = []

    def _call_out(self, name, *args, out, tail=()):
        self.calls.append((name, args[2], args[4], args[5], list(args[6]), list(args[7]), args[8], list(args[9]), args[10], out))
        return [None if size is None else bytes(size) for size in out]

    def _call(self, name, *args):
        self.calls.append((name,) + args[:6] + (list(args[6]), list(args[7]), args[8], list(args[9])) + args[10:])


def test_tables_and_argument_validation():
    from bls_py import _native, _native_veragg as V
    assert V.tables([[(0, 1), (1, 2)], [], [(1, 9)]]) == ([0, 1, 3, 12], [0, 1, 1], [0, 2, 2, 3])
    assert V.tables([]) == ([0], [], [0])
    with pytest.raises(ValueError):
        V.tables([[(0, -1)]])
    eng = FakeEngine()
    sigs, hashes, keys = bytes(192 * 2), bytes(32 * 2), bytes(96 * 3)
    t = V.tables([[(0, 1)], [(1, 2)]])
    for bad in ((sigs[:-1], hashes, keys), (sigs, hashes[:-1], keys), (sigs, hashes, keys[:-1]), (sigs[:192], hashes, keys)):
        with pytest.raises(ValueError):
            V.verify_aggregates(eng, *bad, None, *t)
    with pytest.raises(ValueError):
        V.verify_aggregates(eng, sigs, hashes, keys, [1, 2], *t)                  # an exponent per key
    with pytest.raises(ValueError):
        V.verify_aggregates(eng, sigs, hashes, keys, [1, 2, 1 << 256], *t)        # exponents are 256-bit
    with pytest.raises(ValueError):
        V.verify_aggregates(eng, sigs, hashes, keys, None, [0, 1], [0, 1], [0, 1, 2])    # grp_off holds n_grp + 1 offsets
    with pytest.raises(OverflowError):
        V.verify_aggregates(eng, sigs, hashes, keys, None, [0, 1, 1 << 32], [0, 1], [0, 1, 2])
    assert eng.calls == []
    status, out = V.verify_aggregates(eng, sigs, hashes, keys, None, *t)
    assert (len(status), out) == (2, None)
    status, out = V.verify_aggregates(eng, sigs, hashes, keys, [1, 2, 3], *t, gt=True)
    assert len(out) == 2 * 576
    assert eng.calls == [("blsgpu_verify_aggregates", 2, None, 3, [0, 1, 3], [0, 1], 2, [0, 1, 2], 2, [2, None]),
                         ("blsgpu_verify_aggregates", 2, b"".join(v.to_bytes(32, "big") for v in (1, 2, 3)), 3, [0, 1, 3], [0, 1], 2, [0, 1, 2], 2,
                          [2, 1152])]
    eng.calls.clear()
    V.verify_aggregates_dev(eng, 1, 2, 2, 3, None, 3, *t, 7)
    V.verify_aggregates_dev(eng, 1, 2, 2, 3, 4, 3, *t, 7, d_out_gt=8, stream=9)
    assert eng.calls == [("blsgpu_verify_aggregates_dev", 1, 2, 2, 3, None, 3, [0, 1, 3], [0, 1], 2, [0, 1, 2], 2, 7, None, 0),
                         ("blsgpu_verify_aggregates_dev", 1, 2, 2, 3, 4, 3, [0, 1, 3], [0, 1], 2, [0, 1, 2], 2, 7, 8, 9)]
    assert {"blsgpu_verify_aggregates", "blsgpu_verify_aggregates_dev"} <= set(_native.PROTOTYPES)
