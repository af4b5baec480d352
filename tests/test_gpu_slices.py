"""Every sliced call of the C ABI across its slice boundaries on the device.  BLSGPU_TEST_SLICE_CAP (csrc/blsgpu_ctx.h:
slice_len) caps the slice lengths of the host loops, so 23 items run through four full slices and a short one.  Expected values
never come from the capped engine: they are the vectors, fixtures, host arithmetic and the statuses by construction that the
existing test of each call uses (imported from it), and byte equality with the default engine is asserted on top of that."""
import random
import struct

import pytest

import test_gpu_hd_keys as THD
import test_gpu_hd_paths as TPATH
import test_gpu_msm_ranges as TMR
import test_gpu_mul_short as TSHORT
import test_gpu_seeds as TSEED
import test_gpu_sigdiv as TDIV
import test_gpu_sign as TSIGN
import test_gpu_subgroup as TSUB
from bls_py import _native_find as F
from bls_py import _native_ranges as R
from bls_py import _native_sigdiv as S
from bls_py import hostmath as H
from conftest import engine_with_env
from sigshares_vectors import Session, msg_hash, truth_bytes
from sigshares_vectors import pack as pack_sessions
from test_gpu_batch_find import KINDS, objects
from test_gpu_hd_paths import fx as paths_fx  # noqa: F401  (fixtures of the tests called below, under names of their own)
from test_gpu_msm_ranges import worlds as msmr_worlds  # noqa: F401
from test_gpu_mul_short import pool as short_pool  # noqa: F401
from test_gpu_range_sums import expect, ranges_for, worlds  # noqa: F401
from test_gpu_seeds import drawn as seeds_drawn  # noqa: F401
from test_gpu_seeds import fx as seeds_fx  # noqa: F401
from test_gpu_sigdiv import pool as sigdiv_pool  # noqa: F401
from test_gpu_sign import cases as sign_cases  # noqa: F401
from test_gpu_sign import fixture as sign_fixture  # noqa: F401
from test_gpu_subgroup import sub as subgroup_sub  # noqa: F401
from test_gpu_verify_find_folded import build, mh
from test_gpu_verify_find_folded import keys as fold_keys  # noqa: F401
from test_gpu_verify_find_folded import pack as pack_items

pytestmark = pytest.mark.gpu

N = H.N
CAP = 5
SIZES = [23, 20, 6, 5]              # four full slices and a short one; the last slice exactly full; two; one (cap == n)
PSCAN_CAPS = [1, 5, 16, 17, 40]     # the slice lengths of tests/test_pscan_model.py; 16 and 17 straddle CHUNK


@pytest.fixture(scope="module")
def capped():
    """capped(cap, **knobs): the engine whose slices hold at most `cap` items, created once per module"""
    made = {}

    def get(cap, **knobs):
        key = (cap,) + tuple(sorted(knobs.items()))
        if key not in made:
            made[key] = engine_with_env(dict({"BLSGPU_TEST_SLICE_CAP": str(cap)}, **{k: str(v) for k, v in knobs.items()}))
        return made[key]
    yield get
    for e in made.values():
        e.close()


def up(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(torch.device("cuda", 0))


def blank(n):
    import torch
    return torch.full((n,), 0xAA, dtype=torch.uint8, device=torch.device("cuda", 0))


def down(t):
    return bytes(t.cpu().numpy())                            # (the copy waits for the null stream's work)


def words(v):
    return up(struct.pack("<%dI" % len(v), *v))


class provider:
    """the installed provider on another engine"""

    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        from bls_py import backend
        self.old = backend._provider
        p = backend.HipProvider()
        p._eng = self.eng
        backend.use(p)

    def __exit__(self, *a):
        from bls_py import backend
        backend.use(self.old)


# ------------------------------------------------------------------------------------------------ range sums --
def edge_ranges(n, cap):
    """every (b, e), b <= e, over {slice edges, edges +- 1, 0, n}; with many slices the edges of the first three, a middle one
    and the last three"""
    edges = list(range(0, n + 1, cap))
    if len(edges) > 8:
        edges = edges[:4] + [edges[len(edges) // 2]] + edges[-3:]
    at = sorted({0, n} | {e + d for e in edges for d in (-1, 0, 1) if 0 <= e + d <= n})
    return [(b, e) for b in at for e in at if b <= e]


def planted(g, s, n, cap):
    """the first n scalars with, where the slices allow it: equal neighbours on both sides of the first edge, a pair P, -P across
    the second edge, (0,0) inputs at the first and last place of a slice -- and the points, from the DEFAULT engine"""
    s = list(s[:n])
    if n > cap:
        s[cap] = s[cap - 1]
    if n > 2 * cap:
        s[2 * cap] = N - s[2 * cap - 1]
    if n > 4 * cap:
        s[3 * cap], s[4 * cap - 1] = 0, 0
        s[n - 1] = 0
    return s, g.mul(s)


def sums_dev(g, eng, buf, n, ranges):
    m = len(ranges)
    d_p, d_r, d_o, d_f = up(buf) if n else None, words([v for r in ranges for v in r]), blank(m * g.size), blank(m)
    g.sums_dev(eng, d_p.data_ptr() if n else None, n, d_r.data_ptr(), m, d_o.data_ptr(), d_f.data_ptr(), 0)
    return down(d_o), down(d_f)


@pytest.mark.parametrize("deg", [1, 2])
@pytest.mark.parametrize("cap", PSCAN_CAPS)
def test_range_sums_across_slices(engine, capped, worlds, deg, cap):
    g, s0, _ = worlds[deg]
    eng = capped(cap)
    for n in (100, cap, cap + 1):
        s, pts = planted(g, s0, n, cap)
        ranges = edge_ranges(n, cap) + ranges_for(n)
        if n > 2 * cap:
            ranges += [(2 * cap - 1, 2 * cap + 1), (cap - 1, cap + 1)]
        want, wflag = expect(g, s, ranges)
        if n > 2 * cap:
            assert wflag[-2] == 1 and wflag[-1] == 0         # P, -P across an edge: infinity; P, P across an edge: 2 P
        buf = b"".join(pts)
        host = g.sums(eng, buf, ranges)
        assert host[1] == wflag, (n, cap)
        assert host[0] == want, (n, cap)
        assert sums_dev(g, eng, buf, n, ranges) == (want, wflag), (n, cap)
        assert g.sums(engine, buf, ranges) == host


@pytest.mark.parametrize("deg", [1, 2])
@pytest.mark.parametrize("cap", [5, 16])
def test_range_sums_off_curve_point_in_an_earlier_slice(engine, capped, worlds, deg, cap):
    g, s0, pts0 = worlds[deg]
    eng = capped(cap)
    n, at = 100, cap + 2                                     # the bad point lies in the second slice
    s, pts = list(s0[:n]), list(pts0[:n])
    bad = bytearray(pts[at])
    bad[-1] ^= 1                                             # y + 1 or y - 1: off the curve, not (0,0)
    pts[at] = bytes(bad)
    ranges = edge_ranges(n, cap) + [(0, n), (at, at + 1), (at + 1, n), (at, at), (at + 1, at + 1), (at - 1, 3 * cap + 1), (3 * cap, 5 * cap)]
    s[at] = 0
    want, wflag = expect(g, s, ranges)
    holds = [b <= at < e for b, e in ranges]
    assert any(h and e > 2 * cap for h, (b, e) in zip(holds, ranges)) and any(not h and b > at for h, (b, e) in zip(holds, ranges))
    wflag = bytes(2 if h else f for h, f in zip(holds, wflag))
    want = b"".join(bytes(g.size) if h else want[g.size * j:g.size * (j + 1)] for j, h in enumerate(holds))
    buf = b"".join(pts)
    assert g.sums(eng, buf, ranges) == (want, wflag)
    assert sums_dev(g, eng, buf, n, ranges) == (want, wflag)
    assert g.sums(engine, buf, ranges) == (want, wflag)


@pytest.mark.parametrize("deg", [1, 2])
def test_range_sums_workspace_holds_one_slice_of_records(worlds, deg):
    g, s, pts = worlds[deg]
    n, ranges = 100, [(0, 100), (3, 61), (50, 50)]
    fresh = engine_with_env({"BLSGPU_TEST_SLICE_CAP": str(CAP)})
    try:
        before = fresh.workspace_bytes()
        assert g.sums(fresh, b"".join(pts[:n]), ranges) == expect(g, s[:n], ranges)
        after = fresh.workspace_bytes()
        grown = (after["total"] - before["total"]) - (after["staging"] - before["staging"])
        # a record is 168 bytes per degree: a slice's worth of them (and the rest of the scan's workspace), not n + 1
        assert (CAP + 1) * 168 * deg <= grown < (n + 1) * 168 * deg
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ ragged multi-scalar sums --
# BLSGPU_TEST_SLICE_CAP rounds a chunk slice up to a wavefront of units (64 chunks in G1, 32 in G2: csrc/ragged_plan.h) and cuts
# the range sums over the chunk partials into slices of `cap` partials.  Expected values: the single multiplications of
# test_gpu_msm_ranges.py on the default engine.
@pytest.mark.parametrize("deg", [1, 2])
@pytest.mark.parametrize("cap", [5, 16])
@pytest.mark.parametrize("n", [65, 520])
def test_msm_ranges_across_slices(engine, capped, msmr_worlds, deg, cap, n):
    g, t, s, pts = msmr_worlds[deg]
    eng, ranges = capped(cap), TMR.ranges_for(n)
    chunks = sum(-(-(e - b) // 8) for b, e in ranges)
    assert chunks > (2 if n == 520 else 1) * 64 // deg and chunks > 2 * cap         # several chunk slices, many slices of partials
    TMR.test_sizes_and_ranges(eng, msmr_worlds, deg, n)                             # the expectation and the planted cases
    buf, sc = b"".join(pts[:n]), b"".join(v.to_bytes(32, "big") for v in s[:n])
    want = TMR.expect(g, t[:n], s[:n], ranges)
    host = g.sums(eng, buf, sc, ranges)
    assert host == want
    assert g.sums(engine, buf, sc, ranges) == host
    m = len(ranges)
    d_p, d_s, d_r, d_o, d_f = up(buf), up(sc), words([v for r in ranges for v in r]), blank(m * g.size), blank(m)
    g.sums_dev(eng, d_p.data_ptr(), d_s.data_ptr(), n, d_r.data_ptr(), m, d_o.data_ptr(), d_f.data_ptr(), 0)
    assert (down(d_o), down(d_f)) == host


@pytest.mark.parametrize("deg", [1, 2])
def test_msm_ranges_off_curve_point_across_slices(capped, msmr_worlds, deg):
    """flag 2 from a chunk of an earlier slice of partials (and, in G2, of an earlier chunk slice)"""
    TMR.test_off_curve_point_and_infinity_inputs(capped(CAP), msmr_worlds, deg)
    TMR.test_chunk_counts_around_a_wavefront_of_units(capped(CAP), msmr_worlds, deg, 57)


@pytest.mark.parametrize("deg", [1, 2])
def test_msm_ranges_workspace_holds_one_chunk_slice_of_tables(msmr_worlds, deg):
    import ragged_plan_model as RM
    g, t, s, pts = msmr_worlds[deg]
    n, ranges = 520, TMR.ranges_for(520)
    m, chunks = len(ranges), sum(-(-(e - b) // 8) for b, e in ranges)
    fresh = engine_with_env({"BLSGPU_TEST_SLICE_CAP": str(CAP)})
    try:
        before = fresh.workspace_bytes()["group_sums"]
        assert g.sums(fresh, b"".join(pts[:n]), s[:n], ranges) == TMR.expect(g, t[:n], s[:n], ranges)
        grown = fresh.workspace_bytes()["group_sums"] - before
    finally:
        fresh.close()
    one, every = (RM.msmr_body(RM.knobs(test_slice_cap=cap), deg, n, m, chunks) for cap in (CAP, 0))
    assert one["units0"] == 64 // deg < chunks <= every["units0"]
    # B_MSM_PART holds the head words and B_BUCKETS one chunk slice's tables, each through the headroom rule (bytes + bytes / 4)
    assert before == 0 and grown == RM.grown_bytes(RM.msmr_heads(m)["words"]) + RM.grown_bytes(one["words"])
    assert grown < RM.grown_bytes(every["words"])


# ------------------------------------------------------------------------------------------------ signature division --
@pytest.mark.parametrize("plain", [1, 0])
def test_sig_divide_across_slices(engine, capped, sigdiv_pool, plain):
    """forty dividends over 100 points in slices of five: the plain path's range sums over the working copy, the scalar path's
    chunk slices and range sums over the partials; unit and seeded quotients, a refused divisor, a point off the twist and a
    (0,0) divisor.  Expected: the Python scalars and blsgpu_g2_msm_ranges on the DEFAULT engine (test_gpu_sigdiv.expect)"""
    eng = capped(CAP, BLSGPU_SIGDIV_PLAIN=plain)
    rng = random.Random("slices sigdiv")
    for q in (1, None):
        dividends = [[TDIV.divisor(rng, 1 + (i + j) % 5, q) for i in range(j % 4)] for j in range(40)]
        pts, pt_off, ent_off, ea, eb = TDIV.layout(sigdiv_pool, dividends)
        assert len(pts) == 100 and len(dividends) > 2 * CAP
        for spoil in (False, True):
            if spoil:
                ea = list(ea)
                ea[ent_off[7]] = (ea[ent_off[7]] + 1) % N                        # point 7, a divisor of dividend 3: refused
                off = bytearray(pts[26])
                off[-1] ^= 1                                                     # off the twist
                pts[26], pts[51] = bytes(off), bytes(192)
            wout, wflag, wstatus, wsc, nonunit = TDIV.expect(engine, pts, pt_off, ent_off, ea, eb)
            got = S.sig_divide(eng, b"".join(pts), pt_off, ent_off, ea, eb)
            assert got[:4] == (wout, wflag, wstatus, wsc)
            assert got[4] == (0 if plain and not nonunit else 1, nonunit)
            assert S.sig_divide(engine, b"".join(pts), pt_off, ent_off, ea, eb)[:4] == got[:4]
            if spoil:
                assert 3 in wflag and 2 in wflag and wstatus[7] == 1


@pytest.mark.parametrize("plain", [1, 0])
def test_divide_by_batch_through_the_capped_engine(capped, golden, plain):
    """the cases of tests/golden/sigdiv.json, as test_gpu_sigdiv.py runs them"""
    from bls_py import backend
    with provider(capped(CAP, BLSGPU_SIGDIV_PLAIN=plain)):
        TDIV.test_divide_by_batch_on_the_device_equals_the_loop(golden, backend)


# ------------------------------------------------------------------------------------------------ verify_find --
FIND_N, FIND_M = 23, 3


@pytest.fixture(scope="module")
def find_world(engine, fold_keys):
    """23 items over 3 messages sorted by message (runs cross the slice edges), the key table shuffled"""
    w = build(engine, fold_keys, FIND_N, FIND_M)
    perm = list(range(FIND_N))
    random.Random("slices").shuffle(perm)
    assert perm != sorted(perm)
    table = [None] * FIND_N
    for i, p in enumerate(perm):
        table[p] = w["keys"][i]
    return w, perm, table


def find_args(find_world, forged=None, spoil=None):
    """(sigs, keys, key_idx, hashes, msg_idx), expected status; spoil: {item: (sig or None, key or None, status)}"""
    w, perm, table = find_world
    (sigs, _, _, hashes, msg_idx), want = pack_items(w, forged)
    sig, table, want = [sigs[192 * i:192 * (i + 1)] for i in range(FIND_N)], list(table), bytearray(want)
    for i, (s, k, st) in (spoil or {}).items():
        if s is not None:
            sig[i] = s
        if k is not None:
            table[perm[i]] = k
        want[i] = st
    return (b"".join(sig), b"".join(table), perm, hashes, msg_idx), bytes(want)


def find_calls(eng, args, weights):
    """the four forms -> [(status, stats)]: plain host, plain _dev, folded host, folded _dev"""
    sigs, keys, key_idx, hashes, msg_idx = args
    n = len(key_idx)
    d = [up(sigs), up(keys), words(key_idx), up(hashes), words(msg_idx), up(b"".join(x.to_bytes(8, "big") for x in weights))]
    out = [F.verify_find(eng, *args, weights)]
    for fn in (F.verify_find_dev, R.verify_find_folded_dev):
        d_st = blank(n)
        stats = fn(eng, d[0].data_ptr(), d[1].data_ptr(), len(keys) // 96, d[2].data_ptr(), d[3].data_ptr(), len(hashes) // 32,
                   d[4].data_ptr(), d[5].data_ptr(), n, d_st.data_ptr(), 0)
        out.append((down(d_st), stats))
    out.insert(2, R.verify_find_folded(eng, *args, weights))
    return out


def slices_of(n, cap=CAP):
    return [range(lo, min(lo + cap, n)) for lo in range(0, n, cap)]


FORGERIES = [(), (0,), (4, 5), (19, 20), (22,), (5, 6, 7, 8, 9)]


@pytest.mark.parametrize("pos", FORGERIES, ids=lambda p: "forged_" + "_".join(map(str, p)))
def test_verify_find_forgeries_across_slices(engine, capped, find_world, pos):
    eng = capped(CAP)
    forged = {i: KINDS[(len(pos) + j) % 3] for j, i in enumerate(pos)}
    args, want = find_args(find_world, forged)
    weights = [random.Random(7 + len(pos)).getrandbits(64) or 1 for _ in range(FIND_N)]
    got = find_calls(eng, args, weights)
    print("forged", forged, "stats", [g[1] for g in got])
    assert [g[0] for g in got] == [want] * 4
    assert got[0][1] == got[1][1] and got[2][1] == got[3][1]
    assert F.verify_find(engine, *args, weights)[0] == want == R.verify_find_folded(engine, *args, weights)[0]
    if not pos:
        # one round and one node test per slice; pairs: items + 1 per slice (plain), runs in the slice + 1 (folded)
        msg_idx, sl = args[4], slices_of(FIND_N)
        assert got[0][1] == (len(sl), len(sl), sum(len(r) + 1 for r in sl)) == (5, 5, 28)
        assert got[2][1] == (len(sl), len(sl), sum(len({msg_idx[i] for i in r}) + 1 for r in sl)) == (5, 5, 12)


@pytest.mark.parametrize("m", [2, 7])
def test_folded_run_table_below_and_above_a_slice(engine, capped, fold_keys, m):
    """the folded form's run table has min(slice, n_msgs) + 1 entries, of which a slice of k items reads min(k, n_msgs) + 1
    (find::plan_find, csrc/find_plan.h): 12 items in slices of five over 2 messages (fewer than a slice) and over 7 (more), one
    forgery in the last slice of two items"""
    w = build(engine, fold_keys, 12, m)
    assert len(set(w["msg"])) == m and (m < CAP) == (m == 2)
    args, want = pack_items(w, {10: "wrong_key"})
    weights = [random.Random(13 + m).getrandbits(64) or 1 for _ in range(12)]
    got = find_calls(capped(CAP), args, weights)
    assert [g[0] for g in got] == [want] * 4 and want[10] == 0
    assert got[0][1] == got[1][1] and got[2][1] == got[3][1]
    assert F.verify_find(engine, *args, weights)[0] == want == R.verify_find_folded(engine, *args, weights)[0]


def test_verify_find_ineligible_slices(engine, capped, find_world, golden):
    eng = capped(CAP)
    sub = golden("subgroup.json")
    pick = lambda g, **kw: next(bytes.fromhex(r["point"]) for r in sub[g]
                                if all(r[k] == v for k, v in kw.items()) and any(bytes.fromhex(r["point"])))
    sig_off, sig_out = pick("g2", on_curve=False), pick("g2", on_curve=True, in_subgroup=False)
    key_off, key_out = pick("g1", on_curve=False), pick("g1", on_curve=True, in_subgroup=False)
    weights = [random.Random(11).getrandbits(64) or 1 for _ in range(FIND_N)]
    # the whole second slice ineligible, the slices after it fine: n_e == 0, then the next slice
    whole = {5: (sig_off, None, 0), 6: (None, key_out, 2), 7: (bytes(192), None, 0), 8: (sig_out, None, 0), 9: (None, key_off, 2)}
    # ineligible items at the first and the last place of a slice, a forgery between them
    ends = {10: (sig_out, None, 0), 14: (None, key_out, 2), 15: (None, bytes(96), 2), 19: (bytes(192), None, 0)}
    for spoil, forged, rounds in ((whole, None, 4), (ends, {12: "wrong_key"}, None)):
        args, want = find_args(find_world, forged, spoil)
        got = find_calls(eng, args, weights)
        assert [g[0] for g in got] == [want] * 4
        assert got[0][1] == got[1][1] and got[2][1] == got[3][1]
        assert F.verify_find(engine, *args, weights)[0] == want == R.verify_find_folded(engine, *args, weights)[0]
        if rounds:
            assert got[0][1] == (4, 4, 18 + 4) and got[2][1][:2] == (4, 4)


@pytest.mark.parametrize("at", [5, 10])
def test_folded_dev_refuses_a_decrease_at_a_slice_edge(capped, find_world, at):
    """msg_idx decreases exactly at `at`, item 0 of a later launch of the scan: k_fold_mono reads the item before it"""
    from bls_py import _native
    eng = capped(CAP)
    (sigs, keys, key_idx, hashes, msg_idx), _ = find_args(find_world)
    bad = [2] * at + [1] * (FIND_N - at)
    assert [i for i in range(1, FIND_N) if bad[i] < bad[i - 1]] == [at]
    d = [up(sigs), up(keys), words(key_idx), up(hashes), up(bytes(8 * FIND_N))]
    d_st = blank(FIND_N)
    call = lambda mi: R.verify_find_folded_dev(eng, d[0].data_ptr(), d[1].data_ptr(), FIND_N, d[2].data_ptr(), d[3].data_ptr(), FIND_M,
                                               mi.data_ptr(), d[4].data_ptr(), FIND_N, d_st.data_ptr(), 0)
    d_bad, d_ok = words(bad), words(msg_idx)
    with pytest.raises(_native.BlsGpuError, match="-22"):
        call(d_bad)
    assert down(d_st) == b"\xaa" * FIND_N
    call(d_ok)
    assert down(d_st) == b"\x01" * FIND_N


def test_verify_batch_find_through_the_capped_engine(capped, find_world):
    from bls_py.bls import BLS
    w, _, _ = find_world
    (sigs, pks, _, _, msg_idx), want = pack_items(w, {4: "wrong_key", 5: "wrong_msg", 22: "swapped"})
    objs = objects([(sigs[192 * i:192 * (i + 1)], pks[96 * i:96 * (i + 1)], mh(msg_idx[i])) for i in range(FIND_N)])
    with provider(capped(CAP)):
        for fold in (True, False):
            assert BLS.verify_batch_find(objs, rng=random.Random(1), fold=fold) == [s == 1 for s in want]


# ------------------------------------------------------------------------------------------------ signature shares --
@pytest.mark.parametrize("scaled", [True, False])
def test_sig_shares_across_slices(engine, capped, scaled):
    """five sessions of three shares in slices of two: bad shares in the second and in the last slice, and (scaled) a repeated
    player in a session of the second slice, whose session status lagrange_launch writes at d_sess + lo"""
    eng = capped(2)
    players, k, groups = [3, 5, 8], 3, 5
    bad = {2: {1: "wrong"}, 4: {2: "wrong"}}
    sessions = [Session(players, msg_hash(10 + g), scaled, bad.get(g, {})) for g in range(groups)]
    a = pack_sessions(sessions, seed=21)
    want, wsess = bytearray(truth_bytes(sessions)), bytearray(b"\x01" * groups)
    x = bytearray(a["x"])
    if scaled:
        x[32 * 9:32 * 10] = (8).to_bytes(32, "big")          # session 3: players 8, 5, 8
        want[9:12], wsess[3] = bytes(3), 0
    x = bytes(x)
    host = eng.sig_shares_check(a["sigs"], a["keys"], a["key_idx"], x if scaled else None, a["msg_hashes"], a["weights"], k, groups, scaled)
    assert host[:2] == (bytes(want), bytes(wsess))
    d_st, d_ss = blank(k * groups), blank(groups)
    d = [up(a["sigs"]), up(a["keys"]), words(a["key_idx"]), up(x), up(a["msg_hashes"]), up(b"".join(w.to_bytes(8, "big") for w in a["weights"]))]
    stats = eng.sig_shares_check_dev(d[0].data_ptr(), d[1].data_ptr(), len(a["keys"]) // 96, d[2].data_ptr(), d[3].data_ptr() if scaled else None,
                                     d[4].data_ptr(), d[5].data_ptr(), scaled, k, groups, d_st.data_ptr(), d_ss.data_ptr(), 0)
    assert (down(d_st), down(d_ss), stats) == host
    assert engine.sig_shares_check(a["sigs"], a["keys"], a["key_idx"], x if scaled else None, a["msg_hashes"], a["weights"], k, groups,
                                   scaled)[:2] == host[:2]


# ------------------------------------------------------------------------------------------------ fixed-base G1, HD --
@pytest.fixture(scope="module")
def gen_world(oracle):
    """23 scalars, 23 addends and the oracle's s G1 (+ A) for n_add = 0, 1 and n"""
    rnd = random.Random("slices g1")
    sc = [rnd.randrange(2**256) for _ in range(23)]
    sc[4], sc[5] = 0, N
    add = [THD._want(oracle, rnd.randrange(1, N))[0] for _ in range(23)]
    add[10] = bytes(96)
    want = {0: [THD._want(oracle, s) for s in sc], 1: [THD._want(oracle, s, add[7]) for s in sc],
            23: [THD._want(oracle, s, a) for s, a in zip(sc, add)]}
    return sc, add, {k: (b"".join(a for a, _ in v), b"".join(s for _, s in v)) for k, v in want.items()}


@pytest.mark.parametrize("n", SIZES)
def test_g1_mul_gen_across_slices(engine, capped, gen_world, n):
    eng = capped(CAP)
    sc, add, want = gen_world
    d_sc = up(b"".join(s.to_bytes(32, "big") for s in sc[:n]))
    for n_add, a in ((0, None), (1, add[7]), (n, b"".join(add[:n]))):
        waff, wser = want[23 if n_add > 1 else n_add]
        waff, wser = waff[:96 * n], wser[:48 * n]
        assert eng.g1_mul_gen(sc[:n], a, n_add) == (waff, wser), n_add
        d_aff, d_ser, d_add = blank(96 * n), blank(48 * n), up(a) if a else None
        eng.g1_mul_gen_dev(d_sc.data_ptr(), n, d_aff.data_ptr(), d_ser.data_ptr(), 0, d_add.data_ptr() if a else None, n_add)
        assert (down(d_aff), down(d_ser)) == (waff, wser), n_add
        assert engine.g1_mul_gen(sc[:n], a, n_add) == (waff, wser)
    waff, wser = want[0][0][:96 * n], want[0][1][:48 * n]
    assert eng.g1_mul_gen_secret(sc[:n]) == (waff, wser)
    d_aff, d_ser = blank(96 * n), blank(48 * n)
    eng.g1_mul_gen_secret_dev(d_sc.data_ptr(), n, d_aff.data_ptr(), d_ser.data_ptr(), 0)
    assert (down(d_aff), down(d_ser)) == (waff, wser)


def test_hd_children_across_slices(engine, capped):
    from bls_py import _native
    from bls_py.keys import ExtendedPrivateKey
    from hd_vectors import HostHD
    eng = capped(CAP)
    n = 23
    rnd = random.Random("slices hd")
    esk = ExtendedPrivateKey.from_seed(b"slices")
    pk_aff, sk = TPATH._aff(esk.private_key.get_public_key()), esk.private_key.serialize()
    for priv in (True, False):
        idx = [rnd.randrange(2**32 if priv else 2**31) for _ in range(n)]
        want = HostHD().hd_children(esk.chain_code, pk_aff, sk if priv else None, idx)
        want = tuple(bytes(w) if w is not None else None for w in want)
        assert eng.hd_children(esk.chain_code, pk_aff, sk if priv else None, idx) == want
        assert engine.hd_children(esk.chain_code, pk_aff, sk if priv else None, idx) == want
        outs = [blank(w * n) for w in (32, 32, 96, 48)]
        d_idx = words(idx)
        eng.hd_children_dev(esk.chain_code, pk_aff, sk if priv else None, d_idx.data_ptr(), n, outs[0].data_ptr(),
                            outs[1].data_ptr() if priv else None, outs[2].data_ptr(), outs[3].data_ptr(), 0)
        got = [down(o) for o in outs]
        assert (got[0], got[1] if priv else None, got[2], got[3]) == want
    # a hardened index in a later slice, public mode: -EINVAL before anything is written, both forms
    idx[CAP] |= 2**31
    with pytest.raises(_native.BlsGpuError):
        eng.hd_children(esk.chain_code, pk_aff, None, idx)
    outs, d_idx = [blank(w * n) for w in (32, 96, 48)], words(idx)
    with pytest.raises(_native.BlsGpuError):
        eng.hd_children_dev(esk.chain_code, pk_aff, None, d_idx.data_ptr(), n, outs[0].data_ptr(), None, outs[1].data_ptr(),
                            outs[2].data_ptr(), 0)
    assert all(down(o) == b"\xaa" * len(down(o)) for o in outs)


def test_hd_paths_across_slices(capped, paths_fx):
    """the private and public records of tests/golden/hd_paths.json (host and _dev forms, fingerprints, every depth) and its
    grid (a parent per path) against the digests of hd_paths_vectors.py"""
    from hd_paths_vectors import check_grid_record
    eng = capped(CAP)
    TPATH.test_fixture_through_the_dev_form(paths_fx, eng)
    with provider(eng):
        check_grid_record(paths_fx["grid"], full=True)


def test_hd_paths_public_private_and_secret_across_slices(engine, capped, paths_fx):
    """23 paths of depth 3 from four parents through a shuffled parent_of, fingerprints asked for, in slices of five: the three
    modes, host and _dev forms, against HostHDPaths (hd_children chained on the host; the indices are not hardened, so the
    public derivation gives the private one's chain codes, keys and fingerprints), and the secret form on the private record of
    tests/golden/hd_paths.json against its digests"""
    from bls_py.keys import ExtendedPrivateKey
    from hd_paths_vectors import HostHDPaths, check_digest
    eng = capped(CAP)
    n, depth = 23, 3
    rnd = random.Random("slices paths")
    parents = b"".join(TPATH._record(ExtendedPrivateKey.from_seed(b"slices parent %d" % j)) for j in range(4))
    parent_of = [rnd.randrange(4) for _ in range(n)]
    assert len(set(parent_of[:CAP])) > 1 and parent_of != [0] * n
    paths = [[rnd.randrange(2**31) for _ in range(depth)] for _ in range(n)]
    want = tuple(bytes(w) for w in HostHDPaths().hd_paths(parents, True, parent_of, paths))
    public = (want[0], None, want[2], want[3], want[4])
    for e in (eng, engine):
        assert e.hd_paths(parents, True, parent_of, paths) == want
        assert e.hd_paths_secret(parents, parent_of, paths) == want
        assert e.hd_paths(parents, False, parent_of, paths) == public
    assert TPATH._dev_call(eng, parents, True, parent_of, paths) == want
    assert TPATH._dev_call(eng, parents, False, parent_of, paths) == public
    d_par, d_of, d_idx = up(parents), words(parent_of), words([i for q in paths for i in q])
    outs = [blank(w * n) for w in TPATH.WIDTHS]
    eng.hd_paths_secret_dev(d_par.data_ptr(), 4, d_of.data_ptr(), d_idx.data_ptr(), depth, n, *[o.data_ptr() for o in outs], 0)
    assert tuple(down(o) for o in outs) == want
    # the fixture's private record, every depth, on the secret form
    rec = paths_fx["private"][0]
    esk = ExtendedPrivateKey.from_seed(bytes.fromhex(rec["seed"]))
    sers = [None] * len(rec["paths"])
    for d in range(1, 7):
        pos = [j for j, q in enumerate(rec["paths"]) if len(q) == d]
        sub = [rec["paths"][j] for j in pos]
        got = eng.hd_paths_secret(TPATH._record(esk), None, sub)
        for t, j in enumerate(pos):
            sers[j] = (bytes([0, 0, 0, 1, d]) + got[4][4 * t:4 * t + 4] + sub[t][-1].to_bytes(4, "big") + got[0][32 * t:32 * t + 32] +
                       got[1][32 * t:32 * t + 32])
    check_digest(sers, rec["esk"])


def grown_by(fresh, call):
    """what `call` adds to the workspace of `fresh` beside the staging of the host-buffer form"""
    before = fresh.workspace_bytes()
    got = call()
    after = fresh.workspace_bytes()
    return got, (after["total"] - before["total"]) - (after["staging"] - before["staging"])


def test_hd_paths_workspace_holds_one_slice_of_path_state(engine):
    """23 public paths of depth 3 in slices of five: B_HDP_WS holds the state of one slice (256 bytes a path), not of the call.
    The fixed-base table counts in the total and is allocated apart: one multiplication warms the engine first.  The outputs: the
    default engine's, which test_hd_paths_public_private_and_secret_across_slices holds against the host's on these inputs."""
    import keys_plan_model as KP
    from bls_py.keys import ExtendedPrivateKey
    n, depth = 23, 3
    rnd = random.Random("slices paths")
    parents = b"".join(TPATH._record(ExtendedPrivateKey.from_seed(b"slices parent %d" % j)) for j in range(4))
    parent_of = [rnd.randrange(4) for _ in range(n)]
    paths = [[rnd.randrange(2**31) for _ in range(depth)] for _ in range(n)]
    one, whole = KP.plan_paths(CAP, n, depth, False), KP.plan_paths(0, n, depth, False)
    assert one["S"] == CAP and whole["S"] == n
    fresh = engine_with_env({"BLSGPU_TEST_SLICE_CAP": str(CAP)})
    try:
        fresh.g1_mul_gen([1])
        got, grown = grown_by(fresh, lambda: fresh.hd_paths(parents, False, parent_of, paths))
        assert got == engine.hd_paths(parents, False, parent_of, paths)
        assert CAP * 256 == one["bytes"] - one["o_chain"] <= grown < whole["bytes"] - whole["o_chain"] == n * 256
    finally:
        fresh.close()


@pytest.mark.parametrize("mode", ["plain", "hd"])
def test_keys_from_seeds_across_slices(capped, seeds_fx, seeds_drawn, mode):
    eng = capped(CAP)
    TSEED.test_every_fixture_length(eng, seeds_fx, mode)
    for n in SIZES:
        TSEED.test_counts_against_the_host(eng, seeds_drawn, 56, mode == "hd", n)
    if mode == "hd":
        TSEED.test_dev_form_every_output_on_a_stream(eng, seeds_drawn)


# ------------------------------------------------------------------------------------------------ subgroup checks --
@pytest.mark.parametrize("g,psz", TSUB.GROUPS)
def test_subgroup_checks_across_slices(engine, capped, subgroup_sub, g, psz):
    from subgroup_vectors import expected_status
    eng = capped(CAP)
    recs = subgroup_sub[g]
    good = [r for r in recs if expected_status(r) == 1]
    bad = [r for r in recs if expected_status(r) != 1]
    assert good and {expected_status(r) for r in bad} == {0, 2}
    pick = [good[i % len(good)] for i in range(23)]
    pick[4], pick[5], pick[19], pick[20], pick[22] = bad[0], bad[-1], bad[1 % len(bad)], bad[-2 % len(bad)], bad[0]   # both sides of two edges, the last item
    pts, want = b"".join(bytes.fromhex(r["point"]) for r in pick), bytes(expected_status(r) for r in pick)
    host = (eng.g1_subgroup if g == "g1" else eng.g2_subgroup)(pts)
    assert host == want == (engine.g1_subgroup if g == "g1" else engine.g2_subgroup)(pts)
    d_st, d_pts = blank(23), up(pts)
    (eng.g1_subgroup_dev if g == "g1" else eng.g2_subgroup_dev)(d_pts.data_ptr(), 23, d_st.data_ptr(), 0)
    assert down(d_st) == want
    TSUB.test_shuffled_repeats(eng, subgroup_sub, g, psz, 100)


# ------------------------------------------------------------------------------------------------ short and secret scalars, signing --
@pytest.mark.parametrize("deg", [1, 2])
def test_mul_short_across_slices(capped, short_pool, deg):
    """the pool of test_gpu_mul_short.py (reference: the default engine's msm bytes) with a (0,0) point and a zero weight at
    slice edges: items 30 and 64 are (0,0), weight 32 is zero -- at cap 5 item 30 opens a slice and 64 closes one"""
    eng = capped(CAP)
    p, w, _, _ = short_pool[deg]
    assert not any(p[30]) and not any(p[64]) and w[32] == 0
    TSHORT.test_bytes_of_the_msm_call(eng, short_pool, deg, 65)
    TSHORT.test_bytes_of_the_msm_call(eng, short_pool, deg, 23)
    TSHORT.test_dev_forms(eng, short_pool, deg)
    # items 2 .. 34 of the pool: the zero weight (item 32) opens the slice [30, 35) of the call
    p, w, ref, ref_inf = short_pool[deg]
    lo, n, sz = 2, 33, TSHORT.PSZ[deg]
    assert (32 - lo) % CAP == 0
    pts, want = b"".join(p[lo:lo + n]), (ref[sz * lo:sz * (lo + n)], ref_inf[lo:lo + n])
    assert want[1][32 - lo] and TSHORT.mul_short(eng, deg, pts, w[lo:lo + n]) == want
    d_p, d_w, d_out, d_inf = up(pts), up(b"".join(x.to_bytes(8, "big") for x in w[lo:lo + n])), blank(n * sz), blank(n)
    (F.g1_mul_short_dev if deg == 1 else F.g2_mul_short_dev)(eng, d_p.data_ptr(), d_w.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr(), 0)
    assert (down(d_out), [b != 0 for b in down(d_inf)]) == want


def test_g2_mul_secret_and_sign_across_slices(engine, capped, sign_cases, sign_fixture):
    eng = capped(CAP)
    # 23 scalars, a point each and one shared point, host and _dev forms: the default engine's group sums (sign_cases, g2_msm)
    n = 23
    pts, sc = sign_cases["pts"][:192 * n], sign_cases["scalars"][:32 * n]
    d_pts, d_sc = up(pts), up(sc)
    shared = sign_cases["hashed"][2]
    s_aff, s_inf = engine.g2_msm(shared * n, sc, 1, n)
    s_ser = b"".join(TSIGN.mirror_ser(s_aff[192 * i:192 * (i + 1)]) for i in range(n))
    for P, d_P, n_pts, want in ((pts, d_pts, n, (sign_cases["aff"][:192 * n], sign_cases["ser"][:96 * n], sign_cases["inf"][:n])),
                                (shared, up(shared), 1, (s_aff, s_ser, s_inf))):
        assert eng.g2_mul_secret(P, sc) == want
        d_aff, d_ser, d_inf = blank(192 * n), blank(96 * n), blank(n)
        eng.g2_mul_secret_dev(d_P.data_ptr(), n_pts, d_sc.data_ptr(), n, d_aff.data_ptr(), d_ser.data_ptr(), d_inf.data_ptr(), 0)
        assert (down(d_aff), down(d_ser), [b != 0 for b in down(d_inf)]) == want
    for n in (33, 23, 20, 6, 5):
        TSIGN.test_primitive_against_the_group_sums(eng, sign_cases, n)
    TSIGN.test_shared_point(eng, sign_cases, 33)
    TSIGN.test_sign_against_the_fixture(eng, sign_fixture)
    TSIGN.test_dev_forms_on_a_stream(eng, sign_cases, sign_fixture)
    # 23 keys on 23 messages and on one message: the records of tests/golden/sign.json, repeated
    recs = sign_fixture["cases"]
    rep = [recs[i % len(recs)] for i in range(23)]
    cat = lambda rs, k: b"".join(bytes.fromhex(r[k]) for r in rs)
    assert eng.sign(cat(rep, "sk"), cat(rep, "hash")) == (cat(rep, "aff"), cat(rep, "sig"))
    same = [recs[sign_fixture["same_message"][i % 5]] for i in range(23)]
    assert eng.sign(cat(same, "sk"), bytes.fromhex(same[0]["hash"])) == (cat(same, "aff"), cat(same, "sig"))
    d_aff, d_ser = blank(192 * 23), blank(96 * 23)
    d_sk, d_h = up(cat(rep, "sk")), up(cat(rep, "hash"))
    eng.sign_dev(d_sk.data_ptr(), d_h.data_ptr(), 23, 23, d_aff.data_ptr(), d_ser.data_ptr(), 0)
    assert (down(d_aff), down(d_ser)) == (cat(rep, "aff"), cat(rep, "sig"))
    d_sk, d_h = up(cat(same, "sk")), up(bytes.fromhex(same[0]["hash"]))
    eng.sign_dev(d_sk.data_ptr(), d_h.data_ptr(), 1, 23, d_aff.data_ptr(), d_ser.data_ptr(), 0)
    assert (down(d_aff), down(d_ser)) == (cat(same, "aff"), cat(same, "sig"))


def test_sign_workspace_holds_one_slice_of_tables(sign_fixture):
    """23 keys on 23 messages in slices of five: B_SMUL_WS holds the H(m) points and the tables of one slice -- at least five
    tables, less than 23 slices' worth.  The hash to G2 has workspaces of its own: hashing one slice of messages warms the engine
    first."""
    import keys_plan_model as KP
    recs = sign_fixture["cases"]
    rep = [recs[i % len(recs)] for i in range(23)]
    cat = lambda rs, k: b"".join(bytes.fromhex(r[k]) for r in rs)
    one = KP.plan_sign(CAP, CAP, CAP)                                       # what a staged slice asks of blsgpu_sign_dev
    assert one["held"] == CAP and KP.staged_slice(CAP, 23, KP.SMUL_SLICE) == CAP
    fresh = engine_with_env({"BLSGPU_TEST_SLICE_CAP": str(CAP)})
    try:
        fresh.hash_to_g2(cat(rep[:CAP], "hash"))
        got, grown = grown_by(fresh, lambda: fresh.sign(cat(rep, "sk"), cat(rep, "hash")))
        assert got == (cat(rep, "aff"), cat(rep, "sig"))
        assert CAP * KP.TABLE_DW * 4 == KP.smul_table_bytes(one["held"]) <= grown < 23 * KP.smul_table_bytes(one["held"])
    finally:
        fresh.close()


@pytest.mark.parametrize("deg", [1, 2])
@pytest.mark.parametrize("k,groups", [(1, 70), (3, 150)])
def test_small_sums_with_scalars_across_slices(engine, capped, oracle, seeded_pairs, deg, k, groups):
    """cap 5 is no multiple of the unit (64 groups in G1, 32 in G2): the slices hold one unit's groups"""
    from test_gpu_msm import test_batches_of_small_sums_with_scalars as check
    eng = capped(CAP, BLSGPU_SMUL_MIN_GROUPS=1)
    fixed = engine_with_env({"BLSGPU_MSM_SORT_THRESHOLD": str(1 << 40), "BLSGPU_MSM_SORT2_THRESHOLD": str(1 << 40),
                             "BLSGPU_MSM_PLAIN_THRESHOLD": str(1 << 40), "BLSGPU_SMUL_MIN_GROUPS": str(1 << 40)})
    try:
        check(eng, engine, fixed, oracle, seeded_pairs, k, groups, deg)
    finally:
        fixed.close()


# ------------------------------------------------------------------------------------------------ polynomials, dealing, sums of secrets --
def test_share_checks_dealing_and_sums_across_slices(capped, golden):
    """slices of two polynomials / groups (host forms) and of two fragments (_dev forms): the dealings of tests/golden/dkg.json
    by dkg_vectors.py and rxsecret_vectors.py, the Horner values against hostmath, sums against Python integers"""
    import test_gpu_dkg as TDKG
    import test_gpu_frsecret as TFR
    import test_gpu_rxsecret as TRX
    eng = capped(2)
    TDKG.test_horner_values_against_hostmath(eng)
    TFR.test_dealing_against_the_reference_dealings(eng, golden)
    TFR.test_dealing_against_python_integers(eng, 2)
    TRX.test_every_dealing_of_the_fixture(eng, golden)
    TRX.test_full_width_points_and_literal_fragments(eng, 2)
    TRX.test_sums_against_python_integers(eng, 2)
    TRX.test_dev_forms_on_a_stream(eng)


def test_sign_threshold_with_a_message_per_session_across_slices(engine, capped):
    """five sessions of three signers, a message each, in slices of two scalars: k_g2_spread and k_g2_smul at lo > 0.  Expected:
    (lambda_j sk_j mod n) H(h_g) from the default engine's blsgpu_sign on coefficients computed with Python integers"""
    from bls_py.util import hash256
    eng = capped(2)
    groups, k = 5, 3
    rnd = random.Random("slices threshold")
    Xs = [rnd.sample(range(1, 50), k) for _ in range(groups)]
    sks = [[rnd.randrange(1, N) for _ in range(k)] for _ in range(groups)]
    hashes = [hash256(b"slices session %d" % g) for g in range(groups)]
    scal = []
    for X, S in zip(Xs, sks):
        for j in range(k):
            lam = 1
            for m in range(k):
                if m != j:
                    lam = lam * X[m] * pow(X[m] - X[j], -1, N) % N
            scal.append(lam * S[j] % N)
    waff, wser = engine.sign(scal, b"".join(h for h in hashes for _ in range(k)))
    be = lambda v: b"".join(x.to_bytes(32, "big") for x in v)
    x, sk, hb = be([v for X in Xs for v in X]), be([v for S in sks for v in S]), b"".join(hashes)
    want = (waff, wser, [False] * (k * groups), b"\x01" * groups)
    assert eng.sign_threshold(sk, x, k, hb, groups) == want == engine.sign_threshold(sk, x, k, hb, groups)
    d_sk, d_x, d_h = up(sk), up(x), up(hb)
    d_aff, d_ser, d_inf, d_st = blank(192 * k * groups), blank(96 * k * groups), blank(k * groups), blank(groups)
    eng.sign_threshold_dev(d_sk.data_ptr(), d_x.data_ptr(), k, groups, d_h.data_ptr(), groups, d_aff.data_ptr(), d_ser.data_ptr(),
                           d_inf.data_ptr(), d_st.data_ptr(), 0)
    assert (down(d_aff), down(d_ser), [b != 0 for b in down(d_inf)], down(d_st)) == want


def test_share_check_dev_and_sums_of_secrets_across_slices(engine, capped):
    """the _dev share checks (the index scan and k_poly_eval in slices of two fragments) and blsgpu_fr_sum_secret (slices of two
    groups): statuses by construction (rxsecret_vectors.fragment_case), sums by Python integers, the Horner values and the public
    keys of the sums from the DEFAULT engine"""
    from rxsecret_vectors import R as RX, be32, fragment_case, seeded_coeffs, sum_values, sums
    eng = capped(2)
    t, n_polys = 4, 3
    coeffs = seeded_coeffs(177, n_polys, t)
    commit, _ = engine.g1_mul_gen(coeffs)
    poly, x, s, want = fragment_case(coeffs, t, [1, 2, 3, N + 4, RX - 1])
    poly, x, s, want = poly[:23], x[:23], s[:23], want[:23]
    n = len(poly)
    assert n == 23 and 0 in want and 1 in want
    ref = engine.g1_poly_check(commit, n_polys, t, poly, x, s, aff=True)
    assert list(ref[0]) == want
    d_commit, d_poly, d_x, d_s = up(commit), words(poly), up(be32(x)), up(be32(s))
    for secret in (False, True):
        assert eng.g1_poly_check(commit, n_polys, t, poly, x, s, aff=True, secret=secret) == ref
        d_st, d_aff = blank(n), blank(96 * n)
        (eng.g1_poly_check_secret_dev if secret else eng.g1_poly_check_dev)(d_commit.data_ptr(), n_polys, t, d_poly.data_ptr(), d_x.data_ptr(),
                                                                            d_s.data_ptr(), n, d_st.data_ptr(), d_aff.data_ptr(), 0)
        assert (down(d_st), down(d_aff)) == ref
    groups, k = 5, 3
    ys = sum_values(178, k, groups)
    wsum = sums(ys, k)
    wpk = engine.g1_mul_gen(wsum)
    assert eng.fr_sum_secret(be32(ys), k, groups, pk=True) == (wsum,) + tuple(wpk)
    d_y, d_out, d_pka, d_pks = up(be32(ys)), blank(32 * groups), blank(96 * groups), blank(48 * groups)
    eng.fr_sum_secret_dev(d_y.data_ptr(), k, groups, d_out.data_ptr(), d_pka.data_ptr(), d_pks.data_ptr(), 0)
    assert (down(d_out), down(d_pka), down(d_pks)) == (wsum,) + tuple(wpk)


# ------------------------------------------------------------------------------------------------ pairings --
# The pairing path's slices (csrc/pairing_plan.h Limits: groups per call of the grouped kernels, pairs per line-stream launch
# sequence, pairs per slice of blsgpu_miller_loop_batch) all hold CAP items here.  Expected values are the CPU oracle's and the
# reference's own Miller values of tests/golden/pairing.json.
LS_RUNS = {"BLSGPU_LS_THRESHOLD": 1, "BLSGPU_LS_MIN_GROUP": 2}      # every call asks for the line-stream kernels, chunked from two pairs on
LS_SMALL = {"BLSGPU_LS_THRESHOLD": 1}                               # ... one accumulator per group below 64 pairs


def slice_edges(n, cap=CAP):
    """the pairs that get a degenerate: the last of the first slice, the first of the second, the last of the second, the last"""
    return sorted({p for p in (cap - 1, cap, 2 * cap - 1, n - 1) if 0 <= p < n})


@pytest.fixture(scope="module")
def pair_world(golden, seeded_pairs):
    """world(n, at, py_zero) -> g1, g2, inf, miller: the first n seeded pairs with the reference's infinity vectors (flag on P, on
    Q, on both) and, if asked for, a pair with py = 0 planted at the places `at`, in turn; miller[i] is the reference's Miller value of pair i where a
    vector gives it, else None"""
    g1, g2 = seeded_pairs
    edge = golden("pairing.json")["edge"]
    flagged = [edge[k] for k in ("p_inf", "q_inf", "both_inf")]

    def world(n, at, py_zero=False):
        kinds = [None] * py_zero + flagged                   # (py = 0 only where the call is blsgpu_miller_loop_batch)
        a, b, inf, miller = bytearray(g1[:96 * n]), bytearray(g2[:192 * n]), bytearray(2 * n), [None] * n
        for j, i in enumerate(at):
            v = kinds[j % len(kinds)]
            if v is None:
                a[96 * i + 48:96 * (i + 1)] = bytes(48)      # py = 0: not a point of G1, but the loops are total functions
            else:
                a[96 * i:96 * (i + 1)], b[192 * i:192 * (i + 1)] = bytes.fromhex(v["g1"][0]), bytes.fromhex(v["g2"][0])
                inf[2 * i:2 * i + 2] = bytes(int(x) for x in v["inf"][0])
                miller[i] = bytes.fromhex(v["miller"][0])
        return bytes(a), bytes(b), bytes(inf), miller
    return world


def want_groups(oracle, a, b, inf, gsz, groups):
    return b"".join(oracle.pairing_multi(a[96 * gsz * g:96 * gsz * (g + 1)], b[192 * gsz * g:192 * gsz * (g + 1)], gsz, threads=8,
                                         inf=inf[2 * gsz * g:2 * gsz * (g + 1)]) for g in range(groups))


@pytest.mark.parametrize("n", SIZES)
def test_one_long_group_in_runs(engine, capped, pair_world, oracle, n):
    """blsgpu_pairing_multi_dev: runs of one long group, each leaves a partial for the reduce chain (five, four, two, one)"""
    a, b, inf, _ = pair_world(n, slice_edges(n))
    want = oracle.pairing_multi(a, b, n, threads=8, inf=inf)
    got = []
    for eng in (capped(CAP, **LS_RUNS), engine):
        d_a, d_b, d_i, d_o = up(a), up(b), up(inf), blank(576)
        eng.pairing_multi_dev(d_a.data_ptr(), d_b.data_ptr(), n, d_o.data_ptr(), 0, d_i.data_ptr())
        got.append(down(d_o))
    assert got[0] == want
    assert got[1] == want


def product_then_final(eng, a, b, inf, gsz, groups):
    d_a, d_b, d_i, d_p, d_o = up(a), up(b), up(inf), blank(576 * groups), blank(576 * groups)
    eng.miller_product_batch_dev(d_a.data_ptr(), d_b.data_ptr(), gsz, groups, d_p.data_ptr(), 0, d_i.data_ptr())
    eng.final_exp_product_batch_dev(d_p.data_ptr(), 1, groups, d_o.data_ptr(), 0)
    return down(d_o)


@pytest.mark.parametrize("gsz,groups,knobs", [(2, 7, LS_RUNS), (1, 23, LS_SMALL), (7, 3, LS_RUNS)])
def test_groups_in_slices(engine, capped, pair_world, oracle, gsz, groups, knobs):
    """blsgpu_miller_product_batch_dev, then blsgpu_final_exp_product_batch_dev: 7 groups of 2 pairs are two slices of at most
    five groups, the first of them three line-stream slices of whole groups; 23 groups of one pair five slices of groups; of 3
    groups of 7 pairs every one is longer than a slice, so the VM kernels take them"""
    n = gsz * groups
    at = sorted(set(slice_edges(n) + slice_edges(n, CAP * gsz) + slice_edges(n, CAP // gsz * gsz or gsz)))
    a, b, inf, _ = pair_world(n, at)
    want = want_groups(oracle, a, b, inf, gsz, groups)
    assert product_then_final(capped(CAP, **knobs), a, b, inf, gsz, groups) == want
    assert product_then_final(engine, a, b, inf, gsz, groups) == want


def test_batch_tree_under_the_cap(engine, capped, pair_world, oracle):
    """blsgpu_pairing_multi_batch_dev with groups of 24 pairs: the per-group product tree"""
    gsz, groups = 24, 2
    n = gsz * groups
    a, b, inf, _ = pair_world(n, sorted(set(slice_edges(n) + [gsz - 1, gsz, n - 1])))
    want = want_groups(oracle, a, b, inf, gsz, groups)
    for eng in (capped(CAP, **LS_RUNS), engine):
        d_a, d_b, d_i, d_o = up(a), up(b), up(inf), blank(576 * groups)
        eng.pairing_multi_batch_dev(d_a.data_ptr(), d_b.data_ptr(), gsz, groups, d_o.data_ptr(), 0, d_i.data_ptr())
        assert down(d_o) == want


@pytest.mark.parametrize("fast", [1, 0])
@pytest.mark.parametrize("n", SIZES)
def test_miller_loop_batch_in_slices(engine, capped, pair_world, oracle, n, fast):
    """blsgpu_miller_loop_batch_dev on the fast form and on the reference's lines for every pair"""
    a, b, inf, miller = pair_world(n, slice_edges(n), py_zero=True)
    want = b"".join(miller[i] or oracle.miller_loop(a[96 * i:96 * (i + 1)], b[192 * i:192 * (i + 1)]) for i in range(n))
    for eng in (capped(CAP, BLSGPU_MILLER_EXACT_FAST=fast), engine):
        d_a, d_b, d_i, d_o = up(a), up(b), up(inf), blank(576 * n)
        eng.miller_loop_batch_dev(d_a.data_ptr(), d_b.data_ptr(), n, d_o.data_ptr(), 0, d_i.data_ptr())
        assert down(d_o) == want
