"""Ragged secure aggregation on the GPU: blsgpu_hash_pks_ranges, blsgpu_aggregate_pub_keys_secure_ranges and
blsgpu_aggregate_sigs_secure_ranges (k_secr_check, k_hash_pks_digest_ranges, k_hash_pks_exp_ranges of csrc/blsgpu_hashpks.hip in
front of the ragged sums) through ctypes: the exponents against hashlib and Python integers, the sums against the uniform calls
group length by group length, the refusals with their outputs untouched, the host-buffer forms against the _dev forms and
across their slice boundaries, and the ragged=True forms of the Python entry points against their defaults.

The shape: 70 groups -- a second wavefront of the digest kernel with 58 spare lanes -- whose lengths cycle through 0, 1, 2, 3,
4, 5, 7, 8, 9, 67: every residue of len mod 4, with and without whole quads before the tail, and empty groups."""
import ctypes
import functools
import random

import pytest

import secure_ranges_model as M
from bls_py import _native_secranges as S
from bls_py import hostmath as H
from conftest import engine_with_env
from secure_agg_vectors import Pool, seeded_keys

pytestmark = pytest.mark.gpu

EINVAL = -22
N = H.N
GROUPS = 70
KEY_LENS = (M.LENGTHS * 7)[:GROUPS]
# the exponents (signatures) of group g: another cycle of the same lengths, so groups have more and fewer exponents than keys,
# no exponents with keys and exponents with no keys
EXP_LENS = [M.LENGTHS[(3 * g + 4) % 10] for g in range(GROUPS)]


def u32(v):
    return (ctypes.c_uint32 * len(v))(*v)


@pytest.fixture(scope="module")
def world(engine):
    """the 70-group shape: G1 keys (affine, serialised) counted by KEY_LENS, G2 points counted by EXP_LENS, with a (0,0) point
    planted in a long group of each"""
    rnd = random.Random("secure ranges")
    pk_off, sig_off = M.offsets(KEY_LENS), M.offsets(EXP_LENS)
    aff, ser = engine.g1_mul_gen([rnd.randrange(1, N) for _ in range(pk_off[-1])])
    sigs, _, _ = engine.g2_mul_secret(H.g2_affine_bytes(H.G2_GEN), [rnd.randrange(1, N) for _ in range(sig_off[-1])], ser=False)
    g1_long, g2_long = KEY_LENS.index(67), EXP_LENS.index(67)
    z1, z2 = pk_off[g1_long] + 11, sig_off[g2_long] + 13
    aff = aff[:96 * z1] + bytes(96) + aff[96 * (z1 + 1):]
    sigs = sigs[:192 * z2] + bytes(192) + sigs[192 * (z2 + 1):]
    return {"pk_off": pk_off, "sig_off": sig_off, "aff": aff, "ser": ser, "sigs": sigs, "g1_long": g1_long, "g2_long": g2_long}


@pytest.fixture(scope="module")
def capped():
    made = {}

    def get(cap):
        if cap not in made:
            made[cap] = engine_with_env({"BLSGPU_TEST_SLICE_CAP": str(cap)})
        return made[cap]
    yield get
    for e in made.values():
        e.close()


# ---- the exponents against hashlib ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 64, 65, 70])
def test_hash_lengths_against_hashlib(engine, groups):
    for key_lens in ([[0], [5], [67]] if groups == 1 else [KEY_LENS[:groups]]):
        pk_off = M.offsets(key_lens)
        ser = seeded_keys(100 * groups + key_lens[0], pk_off[-1])
        for exp_lens in (key_lens, EXP_LENS[:groups], [0] * groups):
            exp_off = M.offsets(exp_lens)
            dg, ts = M.hash_pks_ranges(ser, pk_off, exp_off)
            assert len(ts) == 32 * exp_off[-1]
            assert S.hash_pks_ranges(engine, ser, pk_off, exp_off, pk_hash=False, want_pk_hash=True) == (ts, dg), "device digests"
            assert S.hash_pks_ranges(engine, ser, pk_off, exp_off, pk_hash=dg, want_pk_hash=True) == (ts, dg), "digests handed in"
            assert S.hash_pks_ranges(engine, ser, pk_off, exp_off) == ts, "the 64-group rule"
            # with the digests the keys and their table are not read: both may be NULL
            out = ctypes.create_string_buffer(max(1, len(ts)))
            assert engine.lib.blsgpu_hash_pks_ranges(engine.h, None, 0, None, u32(exp_off), groups, dg, out, None) == 0
            assert out.raw[:len(ts)] == ts
            assert all(int.from_bytes(ts[i:i + 32], "big") < N for i in range(0, len(ts), 32))


# ---- equal-length groups give the uniform calls' bytes ------------------------------------------------------------------------
def test_equal_length_groups_give_the_uniform_bytes(engine, world):
    groups, k, k_pks = 65, 5, 7
    aff, ser = world["aff"][:96 * k * groups], world["ser"][:48 * k * groups]
    aff = aff[:96 * k * 64] + bytes(96 * k)                                # the last group sums infinities
    off = [k * g for g in range(groups + 1)]
    assert S.hash_pks_ranges(engine, ser, off, off, pk_hash=False) == engine.hash_pks(ser, k, k, groups, pk_hash=False)
    assert S.hash_pks_ranges(engine, ser, off, [9 * g for g in range(groups + 1)], pk_hash=False) == engine.hash_pks(ser, k, 9, groups, pk_hash=False)
    want, inf = engine.aggregate_pub_keys_secure(aff, ser, k, groups, pk_hash=False)
    got, flag = S.aggregate_pub_keys_secure_ranges(engine, aff, ser, off, pk_hash=False)
    assert got == want and [f == 1 for f in flag] == inf and set(flag) == {0, 1} and inf[-1]
    sigs = world["sigs"][:192 * k * 64] + bytes(192 * k)
    keys = seeded_keys(9, k_pks * groups)
    want, inf = engine.aggregate_sigs_secure(sigs, k, keys, k_pks, groups, pk_hash=False)
    got, flag = S.aggregate_sigs_secure_ranges(engine, sigs, off, keys, [k_pks * g for g in range(groups + 1)], pk_hash=False)
    assert got == want and [f == 1 for f in flag] == inf and set(flag) == {0, 1} and inf[-1]


# ---- the mixed shape, group length by group length against the uniform calls --------------------------------------------------
def gather(buf, item, off, gs):
    return b"".join(buf[item * off[g]:item * off[g + 1]] for g in gs)


def check_against_uniform(engine, deg, pts, pt_off, ser, pk_off, got, flag):
    """every group's output and flag against the uniform call over the groups of its (points, keys) lengths"""
    psz = 96 * deg
    classes = {}
    for g in range(len(pt_off) - 1):
        classes.setdefault((pt_off[g + 1] - pt_off[g], pk_off[g + 1] - pk_off[g]), []).append(g)
    for (k, k_pks), gs in classes.items():
        if k == 0:                                                           # an empty sum: infinity
            assert all(got[psz * g:psz * (g + 1)] == bytes(psz) and flag[g] == 1 for g in gs)
            continue
        # (the uniform call refuses k_pks == 0: its digests are those of nothing, handed in)
        dg = M.hash_pks_ranges(b"", [0] * (len(gs) + 1), [0] * (len(gs) + 1))[0] if k_pks == 0 else None
        p, s = gather(pts, psz, pt_off, gs), gather(ser, 48, pk_off, gs)
        if deg == 1:
            want, inf = engine.aggregate_pub_keys_secure(p, s, k, len(gs), pk_hash=False)
        else:
            want, inf = engine.aggregate_sigs_secure(p, k, s if k_pks else bytes(48 * len(gs)), max(1, k_pks), len(gs), pk_hash=dg if k_pks == 0 else False)
        for q, g in enumerate(gs):
            assert got[psz * g:psz * (g + 1)] == want[psz * q:psz * (q + 1)] and (flag[g] == 1) == inf[q] and flag[g] < 2, (k, k_pks, g)


@pytest.mark.parametrize("deg", [1, 2])
def test_mixed_aggregates(engine, world, deg):
    psz = 96 * deg
    pk_off, ser = world["pk_off"], world["ser"]
    pts, pt_off, long = (world["aff"], pk_off, world["g1_long"]) if deg == 1 else (world["sigs"], world["sig_off"], world["g2_long"])

    def run(p, **kw):
        if deg == 1:
            return S.aggregate_pub_keys_secure_ranges(engine, p, ser, pk_off, **kw)
        return S.aggregate_sigs_secure_ranges(engine, p, pt_off, ser, pk_off, **kw)
    got, flag = run(pts, pk_hash=False)
    assert set(flag) == {0, 1} and [f == 1 for f in flag] == [a == b for a, b in zip(pt_off, pt_off[1:])]     # infinity: the empty groups alone
    check_against_uniform(engine, deg, pts, pt_off, ser, pk_off, got, flag)
    assert run(pts, pk_hash=M.hash_pks_ranges(ser, pk_off, pk_off)[0]) == (got, flag)
    # the planted (0,0) entered as infinity: the long group's sum is that of its other 66 points
    z = pt_off[long] + (11 if deg == 1 else 13)
    ts = M.hash_pks_ranges(ser, pk_off, pt_off)[1]
    idx = [i for i in range(pt_off[long], pt_off[long + 1]) if i != z]
    sc = [int.from_bytes(ts[32 * i:32 * (i + 1)], "big") for i in idx]
    msm = engine.g1_msm if deg == 1 else engine.g2_msm
    want, inf = msm(b"".join(pts[psz * i:psz * (i + 1)] for i in idx), sc, 66, 1)
    assert not inf[0] and got[psz * long:psz * (long + 1)] == want
    # a point off the curve: flag 2 and (0,0) on its group, the other groups undisturbed
    bad_at = pt_off[long] + 40
    bad = bytearray(pts)
    bad[psz * bad_at + psz - 1] ^= 1
    got2, flag2 = run(bytes(bad), pk_hash=False)
    assert list(flag2) == [2 if g == long else f for g, f in enumerate(flag)]
    assert got2 == got[:psz * long] + bytes(psz) + got[psz * (long + 1):]


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def damaged(off, count):
    """(name, table, count): a decreasing offset, a first offset that is not 0, a last offset past the buffer"""
    down, first, past = list(off), list(off), list(off)
    down[31], down[32] = down[32], down[31]                                  # group 31 is not empty in either table: a step down at 31
    assert down[31] > down[32]
    first[0] = 1
    return [("down", down, count), ("first", first, count), ("past", past, count - 1)]


def test_refusals_leave_the_outputs_untouched(engine, world):
    L = engine.lib
    pk_off, sig_off, aff, ser, sigs = (world[k] for k in ("pk_off", "sig_off", "aff", "ser", "sigs"))
    n_keys, n_sigs = pk_off[-1], sig_off[-1]
    outs = [ctypes.create_string_buffer(b"\xaa" * n, n) for n in (32 * n_sigs, 32 * GROUPS, 192 * GROUPS, GROUPS)]
    ts, dg, pt, fl = [ctypes.cast(b, ctypes.c_void_p) for b in outs]
    HP, PUB, SIG = L.blsgpu_hash_pks_ranges, L.blsgpu_aggregate_pub_keys_secure_ranges, L.blsgpu_aggregate_sigs_secure_ranges
    po, so = u32(pk_off), u32(sig_off)

    def refused(rc):
        assert rc == EINVAL and L.blsgpu_last_error() != b""
        assert all(b.raw == b"\xaa" * len(b.raw) for b in outs)
    for name, t, count in damaged(pk_off, n_keys):                          # the key table
        refused(HP(engine.h, ser, count, u32(t), so, GROUPS, None, ts, dg))
        refused(PUB(engine.h, aff, ser, count, u32(t), GROUPS, None, pt, fl))
        refused(SIG(engine.h, sigs, n_sigs, so, ser, count, u32(t), GROUPS, None, pt, fl))
    for name, t, count in damaged(sig_off, n_sigs):                         # the exponent table
        if name != "past":                                                   # (the host form of the hash call counts its exponents by the table itself)
            refused(HP(engine.h, ser, n_keys, po, u32(t), GROUPS, None, ts, dg))
        refused(SIG(engine.h, sigs, count, u32(t), ser, n_keys, po, GROUPS, None, pt, fl))
    for rc in (HP(engine.h, None, n_keys, po, so, GROUPS, None, ts, dg), HP(engine.h, ser, n_keys, None, so, GROUPS, None, ts, dg),
               HP(engine.h, ser, n_keys, po, None, GROUPS, None, ts, dg), HP(engine.h, ser, n_keys, po, so, GROUPS, None, None, dg),
               HP(None, ser, n_keys, po, so, GROUPS, None, ts, dg),
               PUB(engine.h, None, ser, n_keys, po, GROUPS, None, pt, fl), PUB(engine.h, aff, None, n_keys, po, GROUPS, None, pt, fl),
               PUB(engine.h, aff, ser, n_keys, None, GROUPS, None, pt, fl), PUB(engine.h, aff, ser, n_keys, po, GROUPS, None, None, fl),
               PUB(engine.h, aff, ser, n_keys, po, GROUPS, None, pt, None),
               SIG(engine.h, None, n_sigs, so, ser, n_keys, po, GROUPS, None, pt, fl), SIG(engine.h, sigs, n_sigs, None, ser, n_keys, po, GROUPS, None, pt, fl),
               SIG(engine.h, sigs, n_sigs, so, None, n_keys, po, GROUPS, None, pt, fl), SIG(engine.h, sigs, n_sigs, so, ser, n_keys, None, GROUPS, None, pt, fl),
               SIG(engine.h, sigs, n_sigs, so, ser, n_keys, po, GROUPS, None, None, fl),
               HP(engine.h, ser, 1 << 31, po, so, GROUPS, None, ts, dg), PUB(engine.h, aff, ser, 1 << 31, po, GROUPS, None, pt, fl),
               SIG(engine.h, sigs, 1 << 31, so, ser, n_keys, po, GROUPS, None, pt, fl)):
        refused(rc)
    # groups == 0 writes nothing and returns 0
    assert HP(engine.h, None, 0, None, None, 0, None, None, None) == 0 and PUB(engine.h, None, None, 0, None, 0, None, None, None) == 0
    assert SIG(engine.h, None, 0, None, None, 0, None, 0, None, None, None) == 0
    assert HP(engine.h, ser, n_keys, po, so, 0, None, ts, dg) == 0 and PUB(engine.h, aff, ser, n_keys, po, 0, None, pt, fl) == 0
    assert all(b.raw == b"\xaa" * len(b.raw) for b in outs)
    assert HP(engine.h, ser, n_keys, po, so, GROUPS, None, ts, None) == 0  # the digests are optional
    assert outs[0].raw == M.hash_pks_ranges(ser, pk_off, sig_off)[1] and outs[1].raw == b"\xaa" * (32 * GROUPS)
    with pytest.raises(ValueError):
        S.hash_pks_ranges(engine, ser, damaged(pk_off, n_keys)[0][1], sig_off)


# ---- the _dev forms: the host forms' bytes, guard records, refusals on the device -----------------------------------------------
def test_dev_forms_on_a_stream(engine, world):
    import torch
    dev = torch.device("cuda", 0)
    pk_off, sig_off, aff, ser, sigs = (world[k] for k in ("pk_off", "sig_off", "aff", "ser", "sigs"))
    n_keys, n_sigs = pk_off[-1], sig_off[-1]

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def table(off):
        return torch.tensor(off, dtype=torch.int64).to(torch.int32).to(dev)     # (offsets below 2^31)

    def guarded(nbytes, guard):
        return torch.full((guard + nbytes + guard,), 0xAA, dtype=torch.uint8, device=dev)

    def check(tn, want, guard):
        b = bytes(tn.cpu().numpy())
        assert b[:guard] == b"\xaa" * guard and b[len(b) - guard:] == b"\xaa" * guard, "a store outside the output"
        assert b[guard:len(b) - guard] == want

    dg, want_ts = M.hash_pks_ranges(ser, pk_off, sig_off)
    want_pub = S.aggregate_pub_keys_secure_ranges(engine, aff, ser, pk_off, pk_hash=False)
    want_sig = S.aggregate_sigs_secure_ranges(engine, sigs, sig_off, ser, pk_off, pk_hash=False)
    d_aff, d_ser, d_sigs, d_dg, d_po, d_so = up(aff), up(ser), up(sigs), up(dg), table(pk_off), table(sig_off)
    bad = {name: (table(t), count) for name, t, count in damaged(pk_off, n_keys)}
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        q = stream.cuda_stream
        # room for 5 exponents more than the table counts: they stay as they were
        d_ts, d_ts1, d_odg = guarded(32 * (n_sigs + 5), 32), guarded(32 * n_sigs, 32), guarded(32 * GROUPS, 32)
        d_pub, d_pfl, d_sig, d_sfl = guarded(96 * GROUPS, 96), guarded(GROUPS, 1), guarded(192 * GROUPS, 192), guarded(GROUPS, 1)
        S.hash_pks_ranges_dev(engine, d_ser.data_ptr(), n_keys, d_po.data_ptr(), d_so.data_ptr(), n_sigs + 5, GROUPS, None, d_ts.data_ptr() + 32,
                              d_odg.data_ptr() + 32, q)
        S.hash_pks_ranges_dev(engine, None, 0, None, d_so.data_ptr(), n_sigs, GROUPS, d_dg.data_ptr(), d_ts1.data_ptr() + 32, None, q)
        S.aggregate_pub_keys_secure_ranges_dev(engine, d_aff.data_ptr(), d_ser.data_ptr(), n_keys, d_po.data_ptr(), GROUPS, None,
                                               d_pub.data_ptr() + 96, d_pfl.data_ptr() + 1, q)
        S.aggregate_sigs_secure_ranges_dev(engine, d_sigs.data_ptr(), n_sigs, d_so.data_ptr(), d_ser.data_ptr(), n_keys, d_po.data_ptr(), GROUPS, None,
                                           d_sig.data_ptr() + 192, d_sfl.data_ptr() + 1, q)
        stream.synchronize()
        check(d_ts, want_ts + b"\xaa" * 160, 32)
        check(d_ts1, want_ts, 32)
        check(d_odg, dg, 32)
        check(d_pub, want_pub[0], 96)
        check(d_pfl, want_pub[1], 1)
        check(d_sig, want_sig[0], 192)
        check(d_sfl, want_sig[1], 1)
        # a bad table on the device: -EINVAL with a text, nothing written
        r_ts, r_dg, r_pt, r_fl = guarded(32 * n_sigs, 0), guarded(32 * GROUPS, 0), guarded(192 * GROUPS, 0), guarded(GROUPS, 0)
        L = engine.lib
        for name, (d_bad, count) in bad.items():
            rcs = [L.blsgpu_hash_pks_ranges_dev(engine.h, d_ser.data_ptr(), count, d_bad.data_ptr(), d_so.data_ptr(), n_sigs, GROUPS, None,
                                                r_ts.data_ptr(), r_dg.data_ptr(), q),
                   L.blsgpu_aggregate_pub_keys_secure_ranges_dev(engine.h, d_aff.data_ptr(), d_ser.data_ptr(), count, d_bad.data_ptr(), GROUPS, None,
                                                                 r_pt.data_ptr(), r_fl.data_ptr(), q),
                   L.blsgpu_aggregate_sigs_secure_ranges_dev(engine.h, d_sigs.data_ptr(), n_sigs, d_so.data_ptr(), d_ser.data_ptr(), count,
                                                             d_bad.data_ptr(), GROUPS, None, r_pt.data_ptr(), r_fl.data_ptr(), q)]
            assert rcs == [EINVAL] * 3 and b"offsets" in L.blsgpu_last_error(), name
        # ... the exponent table too: the last offset past the room of the output
        assert L.blsgpu_hash_pks_ranges_dev(engine.h, d_ser.data_ptr(), n_keys, d_po.data_ptr(), d_so.data_ptr(), n_sigs - 1, GROUPS, None,
                                            r_ts.data_ptr(), r_dg.data_ptr(), q) == EINVAL
        assert L.blsgpu_aggregate_sigs_secure_ranges_dev(engine.h, d_sigs.data_ptr(), n_sigs - 1, d_so.data_ptr(), d_ser.data_ptr(), n_keys,
                                                         d_po.data_ptr(), GROUPS, None, r_pt.data_ptr(), r_fl.data_ptr(), q) == EINVAL
        stream.synchronize()
        for t in (r_ts, r_dg, r_pt, r_fl):
            assert bool((t == 0xAA).all())
        assert L.blsgpu_hash_pks_ranges_dev(engine.h, None, 0, None, None, 0, 0, None, None, None, q) == 0


# ---- the host-buffer forms across their slice boundaries ----------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 3, 64])
def test_host_forms_across_slices(engine, capped, world, cap):
    """a fresh context per setting (the knob is read when a context is created): slices of at most `cap` groups, keys and
    exponents -- cap 1 a slice per group, cap 3 the short groups in twos and threes, cap 64 the 67-key groups alone -- give
    the bytes of the unsliced call"""
    pk_off, sig_off, aff, ser, sigs = (world[k] for k in ("pk_off", "sig_off", "aff", "ser", "sigs"))
    assert len(M.cut(pk_off, sig_off, cap)) > 1
    e = capped(cap)
    dg = M.hash_pks_ranges(ser, pk_off, pk_off)[0]
    for kw in ({"pk_hash": False}, {"pk_hash": dg}):
        assert S.hash_pks_ranges(e, ser, pk_off, sig_off, want_pk_hash=True, **kw) == (M.hash_pks_ranges(ser, pk_off, sig_off)[1], dg)
        assert S.aggregate_pub_keys_secure_ranges(e, aff, ser, pk_off, **kw) == S.aggregate_pub_keys_secure_ranges(engine, aff, ser, pk_off, **kw)
        assert (S.aggregate_sigs_secure_ranges(e, sigs, sig_off, ser, pk_off, **kw)
                == S.aggregate_sigs_secure_ranges(engine, sigs, sig_off, ser, pk_off, **kw))


# ---- Python ---------------------------------------------------------------------------------------------------------------------
class Counting:
    """a provider that hands every call on to a HipProvider and records its name; with_ext: it offers the three *_ranges
    extensions (bound to the engine), as a stand-in does, and counts them too"""
    EXT = ("hash_pks_ranges", "aggregate_pub_keys_secure_ranges", "aggregate_sigs_secure_ranges")

    def __init__(self, inner, eng, with_ext):
        self._inner, self._eng, self._with_ext, self.calls = inner, eng, with_ext, []

    def __getattr__(self, name):
        if name in self.EXT:
            if not self._with_ext:
                raise AttributeError(name)
            fn = functools.partial(getattr(S, name), self._eng)
        else:
            fn = getattr(self._inner, name)
        if not callable(fn):
            return fn

        def counted(*a, **kw):
            self.calls.append(name)
            return fn(*a, **kw)
        return counted


def test_python_ragged_equals_the_default(engine, golden):
    from bls_py import backend
    from bls_py.bls import BLS
    from bls_py.keys import PrivateKey
    from bls_py.util import hash256, hash_pks, hash_pks_batch
    pool = Pool(golden("secure_agg.json"))
    rnd = random.Random("ragged python")
    extra = [PrivateKey(rnd.randrange(1, N)) for _ in range(15)]            # 67 keys do not fit the fixture's 65
    sks = pool.sks + extra
    pks = pool.pks + PrivateKey.get_public_key_batch(extra)
    lens = [v for v in M.LENGTHS if v] * 8
    lens = lens[:GROUPS]
    idx = [[(3 * g + j) % 80 for j in range(v)] for g, v in enumerate(lens)]
    groups = [[pks[i] for i in ix] for ix in idx]
    msgs = [hash256(b"m%d" % (i % 7)) for i in range(80)]
    sig_all = PrivateKey.sign_batch(sks, [b"m%d" % (i % 7) for i in range(80)])
    sig_groups, mh_groups = [[sig_all[i] for i in ix] for ix in idx], [[msgs[i] for i in ix] for ix in idx]
    old = backend._provider
    prov = Counting(backend.HipProvider(), engine, True)
    backend.use(prov)
    try:
        before = [list(g) for g in groups]
        hash_groups = groups + [[]]                                          # hash_pks of no keys is legal
        want = hash_pks_batch(5, hash_groups)
        assert prov.calls.count("hash_pks") == len(set(lens)) and "hash_pks_ranges" not in prov.calls
        del prov.calls[:]
        assert hash_pks_batch(5, hash_groups, ragged=True) == want and prov.calls == ["hash_pks_ranges"]
        del prov.calls[:]
        want = BLS.aggregate_pub_keys_batch(groups, True)
        assert prov.calls.count("aggregate_pub_keys_secure") == len(set(lens))
        del prov.calls[:]
        got = BLS.aggregate_pub_keys_batch(groups, True, ragged=True)
        assert got == want and [p.serialize() for p in got] == [p.serialize() for p in want]
        assert prov.calls == ["aggregate_pub_keys_secure_ranges"]
        assert all(a is b for g, h in zip(groups, before) for a, b in zip(g, h)), "the caller's lists were reordered"
        assert BLS.aggregate_pub_keys_batch(groups[:3], False, ragged=True) == BLS.aggregate_pub_keys_batch(groups[:3], False)
        del prov.calls[:]
        want = BLS.aggregate_sigs_secure_batch(sig_groups + [[]], groups + [[]], mh_groups + [[]])
        assert prov.calls.count("aggregate_sigs_secure") == len(set(lens))
        del prov.calls[:]
        got = BLS.aggregate_sigs_secure_batch(sig_groups + [[]], groups + [[]], mh_groups + [[]], ragged=True)
        assert got == want and [s.serialize() for s in got] == [s.serialize() for s in want]
        assert prov.calls == ["aggregate_sigs_secure_ranges"]
        # an empty group raises as the default does
        for ragged in (False, True):
            with pytest.raises(Exception, match="Invalid number of keys"):
                BLS.aggregate_pub_keys_batch(groups[:2] + [[]], True, ragged=ragged)
            with pytest.raises(Exception, match="Invalid number of keys"):
                BLS.aggregate_sigs_secure_batch(sig_groups[:2], [groups[0], groups[1][:-1]], mh_groups[:2], ragged=ragged)
        # a provider without the extension
        backend.use(Counting(backend.HipProvider(), engine, False))
        with pytest.raises(NotImplementedError):
            hash_pks_batch(5, groups[:2], ragged=True)
        with pytest.raises(NotImplementedError):
            BLS.aggregate_pub_keys_batch(groups[:2], True, ragged=True)
        with pytest.raises(NotImplementedError):
            BLS.aggregate_sigs_secure_batch(sig_groups[:2], groups[:2], mh_groups[:2], ragged=True)
        assert hash_pks_batch(5, groups[:2]) == [hash_pks(5, g) for g in groups[:2]]     # ... and the default goes on without it
    finally:
        backend.use(old)
