"""CPU: the limb model of tests/ml_vectors.py (the lane-pair, lane-quad and team routines of csrc/blsgpu_ml.hip) against plain
integers mod q -- vmgen/linestream_model.py's tangent, chord, Fq2 and sparse / dense Fq12 products --, the contracts of every
operand, and the proof that the extreme sets reach the column bounds the routines are argued from.
tests/test_gpu_ml_steps.py runs the same sets on the compiled routines."""
import pytest

import ml_vectors as V
from vmgen import linestream_model as LM

Q = V.Q


@pytest.fixture(scope="module")
def ops():
    return V.ops()


def _out_pairs(want, n):
    return [(want[k * V.V2:k * V.V2 + V.L], want[k * V.V2 + V.L:(k + 1) * V.V2]) for k in range(n)]


def _digits(x):
    return all(0 <= d <= V.MASK for d in x[:13])


def test_every_operand_satisfies_its_contract(ops):
    for op in ops.values():
        assert op.sets, op.name
        assert len({tag for tag, _, _, _ in op.sets}) == len(op.sets), op.name
        for tag, words, want, parts in op.sets:
            assert len(parts) == len(op.kinds)
            for kind, x in zip(op.kinds, parts):
                assert V.admissible(kind, x), (op.name, tag, kind)
        for n in op.counts:
            assert len(V.call_sets(op, n)) == n
    assert not V.admissible("hn", V.to_limbs(-Q)) and not V.admissible("hn", [-1] + [0] * 13) and not V.admissible(1, [1 << 28] + [0] * 13)
    assert V.admissible("l0", [-V.MASK] * 13 + [0]) and not V.admissible("hn", [V.MASK] * 13 + [V.HN_TOP_MAX + 1])


def test_lane_pair_ops_agree_with_plain_integers(ops):
    mul2, add2, sub2, scl2 = LM.mul2, LM.add2, LM.sub2, LM.scl2
    plain = {
        # products divide by R once: limbs of x R, y R -> x y R
        "mul": lambda r, k: mul2(r[0], r[1]), "dot2": lambda r, k: add2(mul2(r[0], r[1]), mul2(r[2], r[3])), "sqr": lambda r, k: mul2(r[0], r[0]),
        "sqrsum": lambda r, k: mul2(add2(r[0], r[1]), add2(r[0], r[1])), "m12": lambda r, k: sub2(mul2(r[0], r[0]), scl2(mul2(r[1], r[1]), 12)),
        "mulf": lambda r, k: scl2(r[0], k),
    }
    n = 0
    for op in ops.values():
        if op.value is None:
            continue
        fn = plain[op.value] if isinstance(op.value, str) else op.value
        for tag, words, want, parts in op.sets:
            nv = len(parts) // 2
            r = [V.res2(p) for p in V.pairs_of(parts[:2 * nv])]
            k = V.res(parts[2 * nv]) if len(parts) > 2 * nv else None
            got = _out_pairs(want, 1)[0]
            expect = fn(r, k)
            assert V.res2(got) == (expect[0] % Q, expect[1] % Q), (op.name, tag)
            if op.name != "MUL_XI":                     # everything else returns an hn: digits
                assert _digits(got[0]) and _digits(got[1]), (op.name, tag)
            if op.name.startswith("NORM") or op.name.startswith("MULC_NORM"):   # a carry pass keeps the VALUE, not only the residue
                c = {"NORM_2": 1, "NORM_4": 1, "MULC_NORM_4_S3": 4, "MULC_NORM_3_S2": 3, "MULC_NORM_12_S2": 12, "MULC_NORM_N12_S2": -12}[op.name]
                assert [V.from_limbs(x) for x in got] == [c * V.from_limbs(x) for x in parts[:2]], (op.name, tag)
            n += 1
    assert n > 500


def test_zero_test_and_loads(ops):
    ones = 0
    for tag, words, want, parts in ops["IS_ZERO2"].sets:
        z = 1 if V.from_limbs(parts[0]) % Q == 0 and V.from_limbs(parts[1]) % Q == 0 else 0
        assert want == [z, z], tag
        ones += z
    assert ones == 4                                   # (0, 0), (0, q), (q, 0), (q, q)
    for tag, words, want, parts in ops["LOAD_STORE"].sets:
        for c in range(6):
            v = int.from_bytes(b"".join((w & 0xFFFFFFFF).to_bytes(4, "little") for w in words[12 * c:12 * c + 12]), "big")
            x = want[c * V.L:(c + 1) * V.L]
            assert V.res(x) == v % Q and _digits(x), (tag, c)


def _step_values(parts):
    X, Y, Z, xq, yq = (V.res2(p) for p in V.pairs_of(parts[:6]) + V.pairs_of(parts[8:12]))
    return (X, Y, Z), V.res(parts[6]), V.res(parts[7]), (xq, yq)


def _check_step(want, T3, line, name, tag):
    got = _out_pairs(want, 6)
    for g, w in zip(got[:3], T3):
        assert V.res2(g) == w and _digits(g[0]) and _digits(g[1]), (name, tag)
    for g, w in zip(got[3:], line):
        assert V.res2(g) == w, (name, tag)
    # the record as the team kernels read it: coefficient 0 signed limbs below 2^28, the rest digits
    assert all(V.admissible("l0", x) for x in got[3]) and all(_digits(x) for c in got[4:] for x in c), (name, tag)


def test_steps_agree_with_the_line_stream_model(ops):
    for name in ("SP_TANGENT", "SQ_TANGENT"):
        for tag, words, want, parts in ops[name].sets:
            T, px3n, py, _ = _step_values(parts)
            T3, line = LM.tangent(T, px3n, py)
            _check_step(want, T3, line, name, tag)
            if name == "SQ_TANGENT":                   # both pairs of the quad end with the same X, Y, Z
                assert want[:3 * V.V2] == want[3 * V.V2 + V.REC:], tag
    for tag, words, want, parts in ops["SP_CHORD"].sets:
        T, px3n, py, Qa = _step_values(parts)
        T3, line = LM.chord(T, Qa, px3n, py)
        _check_step(want, T3, line, "SP_CHORD", tag)


def test_pair_and_quad_tangent_agree_mod_q(ops):
    """the same sets through both forms: equal residues (the two forms reduce differently, so the limbs need not be equal)"""
    sp, sq = ops["SP_TANGENT"], ops["SQ_TANGENT"]
    assert [t for t, _, _, _ in sp.sets] == [t for t, _, _, _ in sq.sets]
    differ = 0
    for (tag, _, a, pa), (_, _, b, pb) in zip(sp.sets, sq.sets):
        ra, rb = [V.res2(x) for x in _out_pairs(a, 6)], [V.res2(x) for x in _out_pairs(b, 6)]
        assert ra == rb, tag
        differ += a[:3 * V.V2] != b[:3 * V.V2]
    assert differ > 0


def _team_res(words, n=6):
    return [V.res2(x) for x in _out_pairs(words, n)]


def test_team_ops_agree_with_plain_integers(ops):
    for tag, words, want, parts in ops["SET_ONE"].sets:
        assert _team_res(want) == LM.one6(), tag
    for name in ("PUBLISH_RAW", "PUBLISH_NORM"):
        for tag, words, want, parts in ops[name].sets:
            f = [V.val2(x) for x in V.team_of(parts)]
            for c in range(6):
                re, im, nim, xre, xim, nxim = (V.from_limbs(want[(6 * c + k) * V.L:(6 * c + k + 1) * V.L]) % Q for k in range(6))
                assert (re, im) == f[c] and (nim + im) % Q == 0 and (xre, xim) == LM.xi2(f[c]) and (nxim + xim) % Q == 0, (name, tag, c)
    for J in range(6):
        for tag, words, want, parts in ops["FETCH_%d" % J].sets:
            f = [V.val2(x) for x in V.team_of(parts)]
            for c in range(6):
                re, im, nim = (V.from_limbs(want[(3 * c + k) * V.L:(3 * c + k + 1) * V.L]) % Q for k in range(3))
                src = f[(c - J) % 6]
                assert (re, im) == (LM.xi2(src) if J > c else src) and (nim + im) % Q == 0, (J, tag, c)
    for tag, words, want, parts in ops["FETCH2_RT"].sets:
        f, J = [V.val2(x) for x in V.team_of(parts)], words[-1]
        got = [V.val2(x) for x in _out_pairs(want, 6)]
        assert got == [LM.xi2(f[(c - J) % 6]) if J > c else f[(c - J) % 6] for c in range(6)], tag
    assert {w[-1] for _, w, _, _ in ops["FETCH2_RT"].sets} == {2, 3, 4, 5}
    for name in ("MUL3_012", "MUL3_345", "MUL3_012_RAW"):
        for tag, words, want, parts in ops[name].sets:
            f, ys = [V.res2(x) for x in V.team_of(parts)], [V.res2(y) for y in V.pairs_of(parts[12:18])]
            assert _team_res(want) == LM.mul_terms(f, list(zip(ops[name].Js, ys))), (name, tag)
    for tag, words, want, parts in ops["TEAM_LINE"].sets:
        f, ys = [V.res2(x) for x in V.team_of(parts)], [V.res2(y) for y in V.pairs_of(parts[12:18])]
        jA, jB = words[-2:]
        assert _team_res(want) == LM.mul_terms(f, [(0, ys[0]), (jA, ys[1]), (jB, ys[2])]), tag
        assert all(V.admissible("f", x) for x in (want[k * V.L:(k + 1) * V.L] for k in range(12))), tag       # the result is an operand again
    assert {tuple(w[-2:]) for _, w, _, _ in ops["TEAM_LINE"].sets} == set(V.POSITIONS)
    for name in ("TEAM_DENSE", "TEAM_TEAMREC"):
        for tag, words, want, parts in ops[name].sets:
            f, g = [V.res2(x) for x in V.team_of(parts)], [V.res2(y) for y in V.pairs_of(parts[12:24])]
            assert _team_res(want) == LM.mul_dense(f, g), (name, tag)
    for tag, words, want, parts in ops["TEAM_SQUARE"].sets:
        f = [V.res2(x) for x in V.team_of(parts)]
        assert _team_res(want) == LM.mul_dense(f, f), tag


def test_team_sets_tell_lanes_and_forms_apart(ops):
    """operands that differ per lane: in a random set no two lanes hold the same value and no value equals its xi form, so a
    wrong source lane or a wrong form changes the expected words"""
    for name in ("FETCH_1", "FETCH2_RT", "TEAM_LINE", "MUL3_345", "TEAM_DENSE"):
        rnd = [p for t, _, _, p in ops[name].sets if t.startswith("random")]
        assert len(rnd) >= V.NR
        for parts in rnd:
            f = [V.val2(x) for x in V.team_of(parts)]
            assert len(set(f) | {LM.xi2(x) for x in f}) == 12


def test_extreme_sets_reach_the_column_bounds(ops, capsys):
    """every product op: the largest column of limb products the model met is inside 64 bits, and an extreme set -- not a random
    one -- comes within a factor of two of the bound the routine's comment claims (13 digit limbs x units x 2^56)"""
    lines = []
    for name, units in V.BOUND.items():
        peaks = V.PEAK[name]
        tag, pk = max(peaks.items(), key=lambda kv: kv[1])
        bound = 13 * units << 56
        lines.append("%-14s %d units claimed: %.3f reached (%.4f x 2^63) on %s" % (name, units, pk * units / float(bound), pk / float(1 << 63), tag))
        assert pk < 1 << 63, name
        assert 2 * pk >= bound, (name, tag, pk / float(bound))
        assert pk <= 14 * units << 56, (name, tag)      # and never past what the comment admits
        assert max(v for t, v in peaks.items() if t.startswith("extreme")) == pk, (name, tag)
        rnd = max(v for t, v in peaks.items() if t.startswith("random"))
        assert rnd < pk, name
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    for g, (n, s, p) in V.summary().items():
        assert n and s and p < 1.0, g
    # the sites the comments call the whole column: more than 7 of the 8 units
    for name in ("SQR_HN2", "SP_TANGENT", "TEAM_LINE"):
        assert max(V.PEAK[name].values()) > 13 * 7 << 56, name
