"""blsgpu_verify_aggregates and its _dev form on the device (csrc/blsgpu_veragg.hip, schedule in csrc/verify_agg_plan.h) through
bls_py._native_veragg, and BLS.verify_batch(fused=True) on the HIP provider.  The aggregates are signed with the host mirror;
the expected products are oracle.pairing_multi on pair lists assembled with hostmath (test_verify_agg_host.host_pairs), the
expected status bytes BLS.verify under the host provider -- never the new call.

(The aggregate of NO messages is the one-pair product e(-G1, sig): not one for any signature but infinity, so BLS.verify says
False for it and its status is 0 beside the forged aggregate's.)"""
import ctypes

import pytest

from conftest import engine_with_env
from subgroup_vectors import HostRLC, N, secret_keys
from test_verify_agg_host import host_pairs, host_verify_aggregates

pytestmark = pytest.mark.gpu

EINVAL = -22


@pytest.fixture(scope="module")
def V():
    from bls_py import _native_veragg
    return _native_veragg


@pytest.fixture(scope="module")
def host(oracle):
    """run(fn): fn() under the host provider"""
    from bls_py import backend

    def run(fn):
        old = backend._provider
        backend.use(HostRLC(oracle))
        try:
            return fn()
        finally:
            backend.use(old)
    return run


def with_info(value, tree):
    from bls_py.aggregation_info import AggregationInfo
    from bls_py.signature import Signature
    out = Signature.from_g2(value)
    out.set_aggregation_info(AggregationInfo._from_tree(tree))
    return out


@pytest.fixture(scope="module")
def world(host):
    """17 signers over 17 messages; the aggregates of the first 0, 1, 2, 15, 16 and 17 of them (exponent 1 throughout), the one
    of 16 forged; a secure aggregate with messages of 1, 2, 8 and 9 signers (hash_pks exponents in its tree) and a forged copy"""
    from bls_py.bls import BLS

    def make():
        sks = secret_keys(b"veragg", 20)
        sigs = [sk.sign(b"message %d" % i) for i, sk in enumerate(sks[:17])]
        lens = {}
        for k in (1, 2, 15, 16, 17):
            lens[k] = BLS.aggregate_sigs(sigs[:k])
        lens[0] = with_info(sigs[0].value, {})
        lens[16] = with_info(lens[15].value, lens[16].aggregation_info.tree)       # the signature of 15 under the info of 16
        msgs = [b"one"] + [b"two"] * 2 + [b"eight"] * 8 + [b"nine"] * 9
        secure = BLS.aggregate_sigs([sk.sign(m) for sk, m in zip(sks, msgs)])
        forged = with_info(lens[17].value, secure.aggregation_info.tree)
        return dict(sks=sks, sigs=sigs, lens=lens, secure=secure, forged=forged)
    return host(make)


def inputs(batch, extra_first=None):
    """the call's arguments for a list of signatures, as BLS.verify_batch(fused=True) assembles them; extra_first: a message
    hash no group names, put first in the table"""
    from bls_py import hostmath as H
    from bls_py.bls import _jac_g1_bytes
    msgs = {} if extra_first is None else {extra_first: 0}
    sigs, keys, exps, shapes = b"", b"", [], []
    for s in batch:
        info = s.aggregation_info
        by_message = {}
        for mh, pk in zip(info.message_hashes, info.public_keys):
            by_message.setdefault(mh, []).append(pk)
        groups = []
        for mh, pks in by_message.items():
            uniq = sorted(set(pks))
            groups.append((msgs.setdefault(mh, len(msgs)), len(uniq)))
            keys += b"".join(_jac_g1_bytes(pk.value) for pk in uniq)
            exps += [int(info.tree[(mh, pk)]) % N for pk in uniq]
        shapes.append(groups)
        sigs += H.g2_affine_bytes(s.value.to_affine()._aff())
    return sigs, b"".join(msgs), keys, exps, shapes


def check(engine, V, oracle, host, batch, args, exps, want_status=None):
    """one call with out_gt, against the oracle's products and BLS.verify's answers; -> (status, gt)"""
    from bls_py.bls import BLS
    sigs, hashes, keys, _, shapes = args
    t = V.tables(shapes)
    status, gt = V.verify_aggregates(engine, sigs, hashes, keys, exps, *t, gt=True)
    if want_status is None:
        want_status = bytes(1 if v else 0 for v in host(lambda: [BLS.verify(s) for s in batch]))
    want_gt = b"".join(oracle.pairing_multi(g1, g2, n, threads=8) for g1, g2, n, _ in host_pairs(sigs, hashes, keys, exps, *t))
    assert status == want_status
    for j, st in enumerate(status):
        if st != 2:
            assert gt[576 * j:576 * (j + 1)] == want_gt[576 * j:576 * (j + 1)], j
    assert V.verify_aggregates(engine, sigs, hashes, keys, exps, *t) == (status, None)       # out_gt NULL
    return status, gt


def test_aggregates_of_0_1_2_15_16_17_messages(engine, V, oracle, host, world):
    """with the signature's pair 1, 2, 3, 16, 17 and 18 pairs: either side of the multi-pairing's chunk of 16"""
    batch = [world["lens"][k] for k in (0, 1, 2, 15, 16, 17)]
    args = inputs(batch)
    assert all(e == 1 for e in args[3]) and [len(g) for g in args[4]] == [0, 1, 2, 15, 16, 17]
    status, _ = check(engine, V, oracle, host, batch, args, None)
    assert status == bytes([0, 1, 1, 1, 0, 1])


def test_groups_of_1_2_8_9_keys_with_256_bit_exponents(engine, V, oracle, host, world):
    """either side of the sums' chunk of 8 points.  The secure aggregate's own exponents (below n), then the same keys with
    exponents raised by n and 2n, up to 2^256 - 1: the same points, so the same products"""
    batch = [world["secure"], world["forged"]]
    args = inputs(batch)
    assert sorted(k for _, k in args[4][0]) == [1, 2, 8, 9] and any(e != 1 for e in args[3])
    status, gt = check(engine, V, oracle, host, batch, args, args[3])
    assert status == bytes([1, 0])
    big = [e + min(i % 3, ((1 << 256) - 1 - e) // N) * N for i, e in enumerate(args[3])]
    big[0] = (1 << 256) - 1 - ((1 << 256) - 1 - args[3][0]) % N
    assert max(big) >= 1 << 255 and all(b % N == e for b, e in zip(big, args[3]))
    t = V.tables(args[4])
    assert V.verify_aggregates(engine, args[0], args[1], args[2], big, *t, gt=True) == (status, gt)


def test_unit_exponents_given_and_null_agree(engine, V, oracle, host, world):
    """the secure aggregate's keys with every exponent 1: through the ragged multi-scalar sums (exps given) and through the
    range sums (exps NULL) the same bytes, both the oracle's"""
    sigs, hashes, keys, exps, shapes = inputs([world["secure"], world["lens"][2]])
    t = V.tables(shapes)
    ones = [1] * len(exps)
    want = host_verify_aggregates(oracle, sigs, hashes, keys, None, *t)
    assert want[0] == bytes([0, 1])
    assert V.verify_aggregates(engine, sigs, hashes, keys, ones, *t, gt=True) == want
    assert V.verify_aggregates(engine, sigs, hashes, keys, None, *t, gt=True) == want


def test_a_message_shared_by_three_aggregates_and_an_unused_entry(engine, V, oracle, host, world):
    from bls_py.bls import BLS
    from bls_py.util import hash256
    sks = world["sks"]

    def make():
        return [BLS.aggregate_sigs([sks[0].sign(b"common"), sks[1].sign(b"a")]), sks[2].sign(b"common"),
                BLS.aggregate_sigs([sks[3].sign(b"b"), sks[4].sign(b"common")])]
    batch = host(make)
    args = inputs(batch, extra_first=hash256(b"nobody signs this"))
    used = [msg for groups in args[4] for msg, _ in groups]
    assert len(args[1]) == 32 * 4 and 0 not in used and sum(used.count(v) == 3 for v in set(used)) == 1
    status, _ = check(engine, V, oracle, host, batch, args, None)
    assert status == bytes([1, 1, 1])


def test_a_key_sum_at_infinity(engine, V, oracle, host, world):
    """pk and -pk under one message: the sum's (0,0) goes into the pair list with no flag; what BLS.verify gives under the host
    provider is what the status says"""
    from bls_py.keys import PublicKey
    from bls_py.util import hash256
    sk = world["sks"][5]
    pk = sk.get_public_key()
    neg = PublicKey.from_g1(pk.value * (N - 1))
    mh = hash256(b"cancel")
    batch = [with_info(world["sigs"][5].value, {(mh, pk): 1, (mh, neg): 1}), world["lens"][2]]
    args = inputs(batch)
    assert args[4][0] == [(0, 2)]
    sums = [g1[96:192] for g1, _, _, _ in host_pairs(args[0], args[1], args[2], None, *V.tables(args[4]))]
    assert sums[0] == bytes(96)
    check(engine, V, oracle, host, batch, args, None)


def test_a_key_off_the_curve_and_an_infinity_signature_are_undecided(engine, V, oracle, host, world):
    batch = [world["lens"][2], world["secure"], world["lens"][1], world["lens"][15]]
    sigs, hashes, keys, exps, shapes = inputs(batch)
    t = V.tables(shapes)
    at = 2 + 12                                                              # a key of the secure aggregate: the first aggregate has two
    bad = bytearray(keys)
    bad[96 * at + 95] ^= 1                                                   # y + 1: off the curve
    sigs = sigs[:192 * 2] + bytes(192) + sigs[192 * 3:]                      # the third signature (0,0)
    want = host_verify_aggregates(oracle, sigs, hashes, bytes(bad), exps, *t)
    assert want[0] == bytes([1, 2, 2, 1])
    for e in (exps, None):
        status, gt = V.verify_aggregates(engine, sigs, hashes, bytes(bad), e, *t, gt=True)
        assert status == bytes([1, 2, 2, 1])
        assert gt[:576] == want[1][:576] and gt[3 * 576:] == want[1][3 * 576:]


def test_slices_of_five_pairs(V, oracle, host, world, engine):
    """aggregates of 3, 3 and 7 pairs under BLSGPU_TEST_SLICE_CAP=5: three slices, the last one an aggregate longer than the cap
    (its pair list cut again by the multi-pairing) -- the unsliced bytes"""
    from bls_py.bls import BLS
    sigs17 = world["sigs"]
    batch = host(lambda: [BLS.aggregate_sigs(sigs17[0:2]), BLS.aggregate_sigs(sigs17[2:4]), BLS.aggregate_sigs(sigs17[4:10])])
    args = inputs(batch)
    assert [len(g) + 1 for g in args[4]] == [3, 3, 7]
    status, gt = check(engine, V, oracle, host, batch, args, None)
    assert status == bytes([1, 1, 1])
    e = engine_with_env({"BLSGPU_TEST_SLICE_CAP": "5"})
    try:
        t = V.tables(args[4])
        assert V.verify_aggregates(e, args[0], args[1], args[2], None, *t, gt=True) == (status, gt)
        assert V.verify_aggregates(e, args[0], args[1], args[2], args[3], *t, gt=True) == (status, gt)
    finally:
        e.close()


def test_refusals_leave_status_and_out_gt_untouched(engine, V, world):
    sigs, hashes, keys, exps, shapes = inputs([world["lens"][2], world["lens"][1]])
    go, gm, ao = V.tables(shapes)
    assert (go, gm, ao) == ([0, 1, 2, 3], [0, 1, 0], [0, 2, 3])
    status = ctypes.create_string_buffer(b"\xa5" * 2, 2)
    gt = ctypes.create_string_buffer(b"\xa5" * 1152, 1152)
    U = lambda v: None if v is None else engine._indices(v, "t")

    def call(sigs=sigs, hashes=hashes, n_msgs=2, keys=keys, n_keys=3, go=go, gm=gm, n_grp=3, ao=ao, m=2, status=status, h=engine.h):
        return engine.lib.blsgpu_verify_aggregates(h, sigs, hashes, n_msgs, keys, None, n_keys, U(go), U(gm), n_grp, U(ao), m, status, gt)

    for null in ("sigs", "hashes", "keys", "go", "gm", "ao", "status", "h"):
        assert call(**{null: None}) == EINVAL, null
    for text, kw in ((b"grp_off steps down (entry 1)", dict(go=[0, 2, 1, 3])), (b"grp_off does not end at n_keys (entry 3)", dict(n_keys=4)),
                     (b"agg_off steps down (entry 0)", dict(ao=[2, 1, 3])), (b"agg_off does not end at n_grp (entry 2)", dict(ao=[0, 2, 2])),
                     (b"grp_msg out of range (entry 1)", dict(gm=[0, 2, 0])), (b"grp_msg out of range (entry 0)", dict(n_msgs=0, hashes=None)),
                     (b"batch too large", dict(m=0x3FFFFFF1)), (b"batch too large", dict(n_msgs=0x03FFFFF1)),
                     (b"batch too large", dict(n_keys=0xFFFFFFF1))):
        assert call(**kw) == EINVAL and engine.lib.blsgpu_last_error().startswith(text), text
    assert status.raw == b"\xa5" * 2 and gt.raw == b"\xa5" * 1152
    assert call() == 0 and status.raw == bytes([1, 1])


def test_no_aggregates(engine, V):
    assert V.verify_aggregates(engine, b"", b"", b"", None, [0], [], [0], gt=True) == (b"", b"")
    assert engine.lib.blsgpu_verify_aggregates(engine.h, None, None, 0, None, None, 0, None, None, 0, None, 0, None, None) == 0


def test_dev_form_three_times_on_a_stream_with_the_workspace_accounted(V, oracle, world):
    import torch
    from bls_py import _native
    e = _native.Engine(0)
    try:
        sigs, hashes, keys, exps, shapes = inputs([world["secure"], world["lens"][16], world["lens"][2]])
        t = V.tables(shapes)
        want = host_verify_aggregates(oracle, sigs, hashes, keys, exps, *t)
        assert want[0] == bytes([1, 0, 1])
        dev = torch.device("cuda:0")
        up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
        ds, dh, dk, de = up(sigs), up(hashes), up(keys), up(b"".join(x.to_bytes(32, "big") for x in exps))
        dst = [torch.full((3,), 0xA5, dtype=torch.uint8, device=dev) for _ in range(3)]
        dgt = torch.zeros(3 * 576, dtype=torch.uint8, device=dev)
        before = e.workspace_bytes()
        st = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        n_msgs, n_keys = len(hashes) // 32, len(keys) // 96
        with torch.cuda.stream(st):
            V.verify_aggregates_dev(e, ds.data_ptr(), dh.data_ptr(), n_msgs, dk.data_ptr(), de.data_ptr(), n_keys, *t, dst[0].data_ptr(),
                                    d_out_gt=dgt.data_ptr(), stream=st.cuda_stream)
            V.verify_aggregates_dev(e, ds.data_ptr(), dh.data_ptr(), n_msgs, dk.data_ptr(), None, n_keys, *t, dst[1].data_ptr(), stream=st.cuda_stream)
            V.verify_aggregates_dev(e, ds.data_ptr(), dh.data_ptr(), n_msgs, dk.data_ptr(), de.data_ptr(), n_keys, *t, dst[2].data_ptr(),
                                    stream=st.cuda_stream)
        st.synchronize()
        assert bytes(dst[0].cpu().numpy().tobytes()) == bytes(dst[2].cpu().numpy().tobytes()) == want[0]
        assert bytes(dgt.cpu().numpy().tobytes()) == want[1]
        unit = host_verify_aggregates(oracle, sigs, hashes, keys, None, *t)
        assert bytes(dst[1].cpu().numpy().tobytes()) == unit[0] == bytes([0, 0, 1])
        after = e.workspace_bytes()
        # the sums, flags, hashed points, pair list and results of the call, and its tables, in the total beside what the
        # stages' own fields grew by
        pairs, n_grp = sum(len(g) + 1 for g in shapes), sum(len(g) for g in shapes)
        grown = sum(after[k] - before[k] for k in after if k != "total")
        assert after["total"] - before["total"] >= grown + 96 * n_grp + 192 * n_msgs + 288 * pairs + 576 * 3 + 12 * pairs
        assert after["lines"] - before["lines"] >= pairs * 68 * 84 * 4
    finally:
        e.close()


def test_verify_batch_fused_on_the_hip_provider(world):
    from bls_py import backend
    from bls_py.bls import BLS
    backend.use(None)
    try:
        batch = [world["lens"][2], world["secure"], world["lens"][16], world["forged"], world["lens"][17], world["lens"][1]]
        assert backend.extension("verify_aggregates") is not None
        want = BLS.verify_batch(batch)
        assert want == [True, True, False, False, True, True]
        assert BLS.verify_batch(batch, fused=True) == want
    finally:
        backend.use(None)
