"""blsgpu_sig_divide on the device.  The expected scalars are Python integers, (-a_0 * pow(b_0, -1, n)) % n, and the
expected sums are blsgpu_g2_msm_ranges on those scalars: an independent route through existing code.  The points are t_i H(m)
from blsgpu_sign.  Shapes: no dividend, no divisor, one entry, nine divisors (past the 8-point chunk of the ragged sums),
divisors of 1, 63, 64, 65 and 257 entries in one call (wavefront and workgroup edges of the per-entry lanes and of their
binary search), a mismatch in the last entry, zero exponents, (0,0) inputs, a point off the twist, 1000 seeded dividends; the
plain path against the scalar path; the _dev form; every -EINVAL; Signature.divide_by_batch on the fixture."""
import ctypes
import hashlib
import random
import struct

import pytest

from bls_py import _native_msmr as R
from bls_py import _native_sigdiv as S
from bls_py import hostmath as H
from conftest import engine_with_env
from sigdiv_vectors import case_objects, expected_of, expected_scalars, outcome

pytestmark = pytest.mark.gpu

N = H.N
MSG = hashlib.sha256(b"sig divide").digest()
POOL = 67


@pytest.fixture(scope="module")
def pool(engine):
    rng = random.Random("sigdiv pool")
    out = engine.sign([rng.randrange(1, N) for _ in range(POOL)], MSG, aff=True, ser=False)[0]
    return [out[192 * i:192 * (i + 1)] for i in range(POOL)]


@pytest.fixture(scope="module")
def forced(engine):
    """an engine whose every call takes the scalar path"""
    e = engine_with_env({"BLSGPU_SIGDIV_PLAIN": "0"})
    yield e
    e.close()


def divisor(rng, k, q=None):
    """k entries (a, b) with one quotient q (seeded when None)"""
    q = rng.randrange(2, N) if q is None else q
    b = [rng.randrange(1, N) for _ in range(k)]
    return [(q * y % N, y) for y in b]


def layout(pool, dividends, start=0):
    """dividends: per dividend a list of divisors, a divisor a list of entries (a, b) -> (pts, pt_off, ent_off, ea, eb)"""
    pts, pt_off, ent_off, ea, eb = [], [0], [0], [], []
    for divs in dividends:
        for row in [[]] + list(divs):
            pts.append(pool[(start + len(pts)) % POOL])
            ea += [a for a, _ in row]
            eb += [b for _, b in row]
            ent_off.append(len(ea))
        pt_off.append(len(pts))
    return pts, pt_off, ent_off, ea, eb


def expect(engine, pts, pt_off, ent_off, ea, eb):
    """(out, flag, status, scalar bytes, non-unit count): the sums by blsgpu_g2_msm_ranges on the Python scalars, a dividend with
    a refused divisor at flag 3 and (0,0)"""
    status, scalars, nonunit = expected_scalars(pt_off, ent_off, ea, eb)
    m = len(pt_off) - 1
    out, flag = R.g2_msm_ranges(engine, b"".join(pts), scalars, [(pt_off[j], pt_off[j + 1]) for j in range(m)])
    out, flag = bytearray(out), bytearray(flag)
    for j in range(m):
        if any(status[pt_off[j]:pt_off[j + 1]]):
            out[192 * j:192 * (j + 1)] = bytes(192)
            flag[j] = 3
    return bytes(out), bytes(flag), status, b"".join(s.to_bytes(32, "big") for s in scalars), nonunit


def check(engine, pts, pt_off, ent_off, ea, eb, path=None):
    got = S.sig_divide(engine, b"".join(pts), pt_off, ent_off, ea, eb)
    wout, wflag, wstatus, wsc, nonunit = expect(engine, pts, pt_off, ent_off, ea, eb)
    assert got[2] == wstatus
    assert got[3] == wsc
    assert got[1] == wflag
    assert got[0] == wout
    assert got[4] == ((1 if nonunit else 0) if path is None else path, nonunit)
    return got


def test_no_dividend_no_divisor_one_entry(engine, pool):
    assert S.sig_divide(engine, b"", [0], [0], [], []) == (b"", b"", b"", b"", (0, 0))
    out = check(engine, *layout(pool, [[]]))
    assert out[0] == pool[0] and out[1] == b"\0" and out[4] == (0, 0)                    # the dividend itself, on the plain path
    rng = random.Random(1)
    check(engine, *layout(pool, [[divisor(rng, 1)]]))
    check(engine, *layout(pool, [[divisor(rng, 1, 1)]]))
    check(engine, *layout(pool, [[divisor(rng, 1, N - 1)], [], [divisor(rng, 2, 1)]]))


def test_nine_divisors_under_one_dividend(engine, forced, pool):
    rng = random.Random(9)
    for q in (None, 1):
        lay = layout(pool, [[divisor(rng, 1 + i % 3, q) for i in range(9)], [divisor(rng, 2, q)]])
        got = check(engine, *lay)
        assert check(forced, *lay, path=1)[:4] == got[:4]
        assert got[4][0] == (0 if q == 1 else 1)


def test_entry_counts_around_wavefronts_and_a_mismatch_in_the_last_entry(engine, forced, pool):
    rng = random.Random(257)
    dividends = [[divisor(rng, k)] for k in (1, 63, 64, 65, 257)] + [[divisor(rng, 65, 1), divisor(rng, 63)]]
    lay = layout(pool, dividends)
    good = check(engine, *lay)
    assert good[4] == (1, 6) and set(good[2]) == {0}
    # the last entry of the 257-entry divisor (dividend 4, point 9) no longer fits its first
    pts, pt_off, ent_off, ea, eb = lay
    last = ent_off[10] - 1
    assert ent_off[10] - ent_off[9] == 257
    bad_a = list(ea)
    bad_a[last] = (bad_a[last] + 1) % N
    for e in (engine, forced):
        got = check(e, pts, pt_off, ent_off, bad_a, eb, path=1 if e is forced else None)
        assert got[2] == bytes(1 if p == 9 else 0 for p in range(len(pts)))
        assert got[1] == bytes(3 if j == 4 else good[1][j] for j in range(6))
        for j in range(6):
            assert got[0][192 * j:192 * (j + 1)] == (bytes(192) if j == 4 else good[0][192 * j:192 * (j + 1)])
        assert got[4] == (1, 5)
    # ... and the first entry after the first: entry 1
    bad_b = list(eb)
    bad_b[ent_off[9] + 1] = (bad_b[ent_off[9] + 1] + 1) % N or 1
    assert check(engine, pts, pt_off, ent_off, ea, bad_b)[2][9] == 1


def test_zero_exponents_are_status_two(engine, forced, pool):
    rng = random.Random(2)
    for z in (0, N):
        for at in (0, 4):
            d = divisor(rng, 5, 1)
            d[at] = (d[at][0], z)
            lay = layout(pool, [[divisor(rng, 2, 1)], [divisor(rng, 3, 1), d], [divisor(rng, 1, 1)]])
            for e in (engine, forced):
                got = check(e, *lay, path=1 if e is forced else None)
                assert got[2] == bytes([0, 0, 0, 0, 2, 0, 0]) and got[1] == bytes([0, 3, 0])
    # a zero dividend exponent is an ordinary quotient 0: the divisor enters with scalar 0
    lay = layout(pool, [[[(0, 5), (N, 7)]]])
    got = check(engine, *lay)
    assert got[2] == b"\0\0" and got[3][32:] == bytes(32) and got[0] == pool[0] and got[4] == (1, 1)


def test_points_at_infinity_and_a_point_off_the_twist(engine, forced, pool):
    rng = random.Random(3)
    for q in (1, None):
        dividends = [[divisor(rng, 2, q)], [divisor(rng, 1, q), divisor(rng, 1, q)], [divisor(rng, 3, q)], [divisor(rng, 1, q)]]
        pts, pt_off, ent_off, ea, eb = layout(pool, dividends)
        pts[0] = bytes(192)                                  # a dividend at (0,0)
        pts[3] = bytes(192)                                  # a divisor at (0,0)
        pts[8] = pts[7]                                      # dividend 3 divided by itself
        off = bytearray(pts[6])
        off[-1] ^= 1                                         # y + 1 or y - 1: off the twist, not (0,0)
        pts[6] = bytes(off)
        for e in (engine, forced):
            got = check(e, pts, pt_off, ent_off, ea, eb, path=1 if e is forced else None)
            assert got[1][2] == 2 and got[0][384:576] == bytes(192)
            assert got[1][3] == (1 if q == 1 else 0) and got[1][0] == 0 and set(got[2]) == {0}
    # a refused divisor outranks the point off the twist
    ea[ent_off[6]] = (ea[ent_off[6]] + 1) % N
    got = check(engine, pts, pt_off, ent_off, ea, eb)
    assert got[1][2] == 3 and got[2][6] == 1


def test_a_thousand_seeded_dividends(engine, forced, pool):
    rng = random.Random(1000)
    for q in (1, None):
        lay = layout(pool, [[divisor(rng, 4, q) for _ in range(3)] for _ in range(1000)], start=5)
        got = check(engine, *lay)
        assert got[4] == ((0, 0) if q == 1 else (1, 3000))
        if q == 1:
            assert check(forced, *lay, path=1)[:4] == got[:4]


def test_plain_and_scalar_paths_give_the_same_bytes(engine, forced, pool):
    rng = random.Random(4)
    dividends = [[divisor(rng, 1 + (i + j) % 5, 1) for i in range(j % 4)] for j in range(40)]
    lay = layout(pool, dividends)
    a, b = check(engine, *lay), check(forced, *lay, path=1)
    assert a[:4] == b[:4] and a[4] == (0, 0) and b[4] == (1, 0)
    # one quotient other than 1 sends the whole call down the scalar path
    dividends[18][1] = divisor(rng, 3, 2)
    assert check(engine, *layout(pool, dividends))[4] == (1, 1)


def test_dev_form_equals_the_host_form(engine, pool):
    import torch
    rng = random.Random(5)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    up = lambda b: torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).to(dev)
    words = lambda v: struct.pack("<%dI" % len(v), *v)
    for q in (1, None):
        pts, pt_off, ent_off, ea, eb = layout(pool, [[divisor(rng, 1 + i, q) for i in range(j)] for j in range(12)])
        host = S.sig_divide(engine, b"".join(pts), pt_off, ent_off, ea, eb)
        n_pts, m, n_ent = len(pts), len(pt_off) - 1, len(ea)
        d_p, d_po, d_eo = up(b"".join(pts)), up(words(pt_off)), up(words(ent_off))
        d_a, d_b = up(b"".join(v.to_bytes(32, "big") for v in ea)), up(b"".join(v.to_bytes(32, "big") for v in eb))
        outs = [torch.full((size,), 0xAA, dtype=torch.uint8, device=dev) for size in (192 * m, m, n_pts, 32 * n_pts)]
        call = lambda po, eo, sc: S.sig_divide_dev(engine, d_p.data_ptr(), n_pts, po.data_ptr(), m, eo.data_ptr(), d_a.data_ptr(), d_b.data_ptr(),
                                                   n_ent, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), sc, stream.cuda_stream)
        stats = call(d_po, d_eo, outs[3].data_ptr())
        stream.synchronize()
        assert tuple(bytes(o.cpu().numpy()) for o in outs) + (stats,) == host
        # without the scalars
        outs[3].fill_(0xAA)
        assert call(d_po, d_eo, None) == stats
        stream.synchronize()
        assert bytes(outs[3].cpu().numpy()) == b"\xaa" * (32 * n_pts) and bytes(outs[0].cpu().numpy()) == host[0]
        # the _dev form checks the offsets on the device, before anything is written
        from bls_py import _native
        bad_po, bad_eo = list(pt_off), list(ent_off)
        bad_po[5], bad_po[6] = bad_po[6], bad_po[5]
        bad_eo[7] = bad_eo[8]                                # a divisor without entries
        for po, eo in ((bad_po, ent_off), (pt_off, bad_eo)):
            for o in outs:
                o.fill_(0xAA)
            with pytest.raises(_native.BlsGpuError, match="-22"):
                call(up(words(po)), up(words(eo)), outs[3].data_ptr())
            stream.synchronize()
            assert all(bytes(o.cpu().numpy()) == b"\xaa" * o.numel() for o in outs)


def test_einval_leaves_the_outputs_untouched(engine, pool):
    rng = random.Random(6)
    pts, pt_off, ent_off, ea, eb = layout(pool, [[divisor(rng, 2, 1)], [divisor(rng, 1), divisor(rng, 3)], []])
    assert (pt_off, ent_off) == ([0, 2, 5, 6], [0, 0, 2, 2, 3, 6, 6])
    lib, h, n_pts, m, n_ent = engine.lib, engine.h, 6, 3, 6
    buf = b"".join(pts)
    a, b = b"".join(v.to_bytes(32, "big") for v in ea), b"".join(v.to_bytes(32, "big") for v in eb)
    arr = lambda v: (ctypes.c_uint32 * len(v))(*v)
    sizes = (192 * m, m, n_pts, 32 * n_pts)
    outs = [ctypes.create_string_buffer(b"\xee" * s, s) for s in sizes]
    stats = (ctypes.c_uint32 * 2)(7, 7)
    clean = lambda: all(o.raw == b"\xee" * s for o, s in zip(outs, sizes)) and list(stats) == [7, 7]
    fn = lib.blsgpu_sig_divide
    bad_offsets = [
        ([0, 5, 2, 6], ent_off, n_ent),                      # point offsets that decrease
        ([1, 2, 5, 6], ent_off, n_ent),                      # pt_off[0] != 0
        ([0, 2, 5, 5], ent_off, n_ent),                      # pt_off[m] != n_pts
        ([0, 2, 5, 7], ent_off, n_ent),
        ([0, 2, 2, 6], ent_off, n_ent),                      # an empty dividend range
        (pt_off, [0, 0, 2, 2, 6, 3, 6], n_ent),              # entry offsets that decrease
        (pt_off, [0, 0, 2, 2, 3, 6, 5], n_ent),              # ent_off[n_pts] != n_ent
        (pt_off, ent_off, n_ent - 1),
        (pt_off, [0, 1, 2, 2, 3, 6, 6], n_ent),              # a dividend's own row with entries
        (pt_off, [0, 0, 2, 2, 2, 6, 6], n_ent),              # a divisor's row with none
        (pt_off, [0, 0, 2, 3, 3, 6, 6], n_ent),              # both at once: dividend 1's own row, and its first divisor's
        (pt_off, [1, 1, 2, 2, 3, 6, 6], n_ent),              # ent_off[0] != 0
    ]
    for po, eo, ne in bad_offsets:
        assert fn(h, buf, n_pts, arr(po), m, arr(eo), a, b, ne, *outs, stats) == -22 and lib.blsgpu_last_error(), (po, eo, ne)
        assert clean(), (po, eo, ne)
    po, eo = arr(pt_off), arr(ent_off)
    for args in ((None, n_pts, po, m, eo, a, b, n_ent, *outs), (buf, n_pts, None, m, eo, a, b, n_ent, *outs),
                 (buf, n_pts, po, m, None, a, b, n_ent, *outs), (buf, n_pts, po, m, eo, None, b, n_ent, *outs),
                 (buf, n_pts, po, m, eo, a, None, n_ent, *outs), (buf, n_pts, po, m, eo, a, b, n_ent, None, outs[1], outs[2], outs[3]),
                 (buf, n_pts, po, m, eo, a, b, n_ent, outs[0], None, outs[2], outs[3]),
                 (buf, n_pts, po, m, eo, a, b, n_ent, outs[0], outs[1], None, outs[3])):
        assert fn(h, *args, stats) == -22
        assert clean()
    assert fn(h, buf, n_pts, po, 0, eo, a, b, n_ent, *outs, stats) == 0 and clean()          # m == 0 writes nothing
    # the same arguments in order: out_scalars and stats may be NULL
    assert fn(h, buf, n_pts, po, m, eo, a, b, n_ent, outs[0], outs[1], outs[2], None, None) == 0
    assert outs[3].raw == b"\xee" * sizes[3] and list(stats) == [7, 7]
    assert fn(h, buf, n_pts, po, m, eo, a, b, n_ent, *outs, stats) == 0
    want = expect(engine, pts, pt_off, ent_off, ea, eb)
    assert tuple(o.raw for o in outs) == want[:4] and list(stats) == [1, want[4]]


def test_workspace_counts_in_the_total(pool):
    from bls_py import _native
    rng = random.Random(7)
    lay = layout(pool, [[divisor(rng, 2, 1)] for _ in range(300)])
    fresh = _native.Engine(0)
    try:
        before = fresh.workspace_bytes()
        first = S.sig_divide(fresh, b"".join(lay[0]), *lay[1:])
        after = fresh.workspace_bytes()
        grown = (after["total"] - before["total"]) - (after["staging"] - before["staging"])
        assert grown >= 600 * (192 + 32 + 4)                 # the working copy, the scalars and the bytes per point, at least
        assert S.sig_divide(fresh, b"".join(lay[0]), *lay[1:]) == first and fresh.workspace_bytes() == after
    finally:
        fresh.close()


@pytest.fixture()
def hip_provider():
    from bls_py import backend
    old = backend._provider
    backend.use(backend.HipProvider())
    yield backend
    backend.use(old)


def test_divide_by_batch_on_the_device_equals_the_loop(golden, hip_provider):
    from bls_py.bls import BLS
    from bls_py.signature import Signature
    from sigdiv_vectors import record_of
    assert hip_provider.extension("sig_divide").func is S.sig_divide
    cases = [(c, case_objects(c)) for c in golden("sigdiv.json")]
    for c, (dividend, divisors) in cases:
        got = outcome(lambda: Signature.divide_by_batch([dividend], [divisors]))
        assert got == outcome(lambda: [dividend.divide_by(divisors)]) == expected_of(c), c["name"]
    good = [(c, o) for c, o in cases if "error" not in c]
    quotients = Signature.divide_by_batch([d for _, (d, _) in good], [ds for _, (_, ds) in good])
    assert [record_of(s) for s in quotients] == [c["result"] for c, _ in good]
    checked = [(c, s) for (c, _), s in zip(good, quotients) if c["verify"] is not None]
    assert BLS.verify_batch([s for _, s in checked]) == [c["verify"] for c, _ in checked] and len(checked) >= 6
    # the first failing dividend in input order, behind dividends the device accepts
    by = {c["name"]: o for c, o in cases}
    for order in (["nested_one_leaf", "not_unique", "not_a_subset"], ["secure_one_leaf", "not_a_subset", "not_unique"]):
        ds = [by[name] for name in order]
        assert (outcome(lambda: Signature.divide_by_batch([d for d, _ in ds], [v for _, v in ds]))
                == outcome(lambda: [d.divide_by(v) for d, v in ds]))
