"""The plans of tests/msm_plan_model.py against the device: one smallest call per kernel family of the G1 / G2 sums, each on a fresh
context.  The result equals the oracle's bytes, and the two buffers the sums share grew by exactly what the model's totals give
through the buffers' headroom rule (bytes + bytes / 4), as blsgpu_ctx_workspace_bytes reports them under "group_sums".  Only the
public binding and the model are used, so the same file holds the library of before csrc/msm_plan.h to the model."""
import random

import pytest

import msm_plan_model as M
from conftest import engine_with_env

pytestmark = pytest.mark.gpu
N = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
BIG = 1 << 40
UNSORTED = dict(msm_sort_threshold=BIG, msm_sort2_threshold=BIG)
LANE = dict(pip_group_threshold=2, msm_lane_threshold=1)

# (what, route, degree, k, groups, scalars, knobs, what the plan must say)
CASES = [("plain", "PLAIN", deg, k, 1, 0, {}, dict(U=M.cdiv(k, 4))) for deg in (1, 2) for k in (2, 9)]
CASES += [
    ("7-bit windows", "SORTED", 1, 1, 1, 1, {}, dict(cb=7, wide=1)),
    ("13-bit windows", "SORTED", 1, 512, 1, 1, {}, dict(cb=13)),
    ("9-bit windows", "SORTED", 2, 1, 1, 1, {}, dict(cb=9)),
    ("11-bit windows", "SORTED", 2, 512, 1, 1, {}, dict(cb=11)),
    ("5-bit windows, no fold", "SORTED", 2, 2, 1, 1, dict(sort2_bits=5), dict(cb=5, nch=1, folds=[], pass5=0)),
]
for deg in (1, 2):
    CASES += [
        ("one slice", "SMALL_GROUPS", deg, 2, 3, 1, dict(smul_min_groups=2), dict(slice=3)),
        ("capped slices", "SMALL_GROUPS", deg, 2, 3, 1, dict(smul_min_groups=2, test_slice_cap=1), dict(slice=3, units0=64 // deg)),
        ("buckets in LDS", "BUCKET_VM", deg, 3, 2, 1, dict(pip_group_threshold=2), dict(chunks=1, tail=M.T_PIP)),
        ("a lane per window", "BUCKET_LANE", deg, 3, 2, 1, LANE, dict(pairs=deg - 1, fold_n=0, tail=M.T_QUADS if deg == 2 else M.T_PIP)),
        ("lane fold", "BUCKET_LANE", deg, 97, 1, 1, dict(UNSORTED, pip_threshold=1, msm_lane_threshold=1, pip_chunks=97),
         dict(chunks=97, fold_n=2, lane_last=0, tail=M.T_PIP)),
        ("wavefront VM", "VM", deg, 1, 2, 1, {}, dict(blocks=2)),
    ]
CASES.append(("single lanes", "BUCKET_LANE", 2, 3, 2, 1, dict(LANE, msm_lane_pairs=0), dict(pairs=0, lane_last=1, tail=M.T_PIP)))


@pytest.mark.parametrize("what,route,deg,k,groups,scalars,over,says", CASES,
                         ids=["G%d %s, %s, k=%d" % (c[2], c[1].lower(), c[0], c[3]) for c in CASES])
def test_one_call_per_route(oracle, seeded_pairs, what, route, deg, k, groups, scalars, over, says):
    c = M.knobs(**over)
    routes = M.msm_dev(c, deg, k, groups, scalars)
    assert routes[0][0] == route and all(routes[0][1][x] == v for x, v in says.items()), routes[0]
    ran = routes[:1]                                           # (on the device the first route asked has room and serves the call)
    assert len(routes) == 1 or route == "SMALL_GROUPS"
    sz, n = 96 * deg, k * groups
    pts = seeded_pairs[deg - 1][sz * 7:sz * (7 + n)]
    rnd = random.Random(1000 * k + 10 * groups + deg)
    sc = [rnd.randrange(N) for _ in range(n)] if scalars else None
    fresh = engine_with_env({M.ENV[x]: str(v) for x, v in over.items()})
    try:
        before = fresh.workspace_bytes()["group_sums"]
        got, inf = (fresh.g1_msm if deg == 1 else fresh.g2_msm)(pts, sc, k, groups)
        grown = fresh.workspace_bytes()["group_sums"] - before
    finally:
        fresh.close()
    om = oracle.g1_msm if deg == 1 else oracle.g2_msm
    for g in range(groups):
        want, _ = om(pts[sz * k * g:sz * k * (g + 1)], sc[k * g:k * (g + 1)] if scalars else None, k)
        assert got[sz * g:sz * (g + 1)] == want and inf[g] == (want == bytes(sz)), g
    print("group_sums grew by", grown, "bytes; the model:", M.group_sums_bytes(ran))
    assert before == 0 and grown == M.group_sums_bytes(ran)
