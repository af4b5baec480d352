"""CPU: the limb model of tests/curve_vectors.py (sp2, sp4, SrtG<1> / SrtG<2> and the digit routines of csrc/blsgpu_msm.hip) against
bls_py.hostmath on every set, the sp2 and sp4 forms against each other, the contract of every operand, the column sums the extreme
sets reach, what the limbs of the Jacobian infinity (1 : 1 : 0) do over 60 doublings, and the mutants of the model the sets must
tell from it.  tests/test_gpu_curve.py runs the same sets on the compiled routines."""
import os
import shutil
import subprocess

import pytest

import curve_vectors as V
import ml_vectors as MV

Q = V.Q
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-bls_amd", "csrc")


@pytest.fixture(scope="module")
def ops():
    return V.ops()


def test_op_table(ops):
    assert len(ops) == 38 and {g: len(V.group(g)) for g in V.GROUPS} == {"pair": 14, "quad": 5, "lane": 2, "chain": 14, "digit": 3}
    for op in ops.values():
        assert op.sets and len({s[0] for s in op.sets}) == len(op.sets), op.name
        for n in op.counts:
            assert len(V.call_sets(op, n)) == n
    classes = {"sub", "off", "gold", "dbl", "inv", "inf", "lam", "coord", "extreme"}
    for name in ("PADD", "SRTG2_ADD", "SP4_PADD"):
        assert {s[0].split("/")[0] for s in ops[name].sets} == classes, name
    assert {s[0].split("/")[0] for s in ops["PMADD_NEG"].sets} == classes
    tags = {s[0] for s in ops["PADD"].sets}
    for inf in ("pt_inf", "scaled", "cancelled", "z-limbs-of-q", "x-z-limbs-of-q"):
        assert {"inf/%s/%s" % (inf, side) for side in ("first", "second", "both")} <= tags
    assert {"inf/one-one-zero", "inf/z-limbs-of-q", "coord/x-zero", "coord/y-real"} <= {s[0] for s in ops["PDBLJ"].sets}
    assert {"coord/z-real/store1", "coord/z-imag/store1", "coord/z-zero/store1", "coord/z-norm-one/store1"} <= {s[0] for s in ops["SRTG2_AFFINE_OUT"].sets}
    assert len(V.base_points()["gold"]) >= 4            # the fixtures have small-order and torsion points of the twist


def test_every_operand_lies_in_the_contract(ops):
    n = 0
    for op in ops.values():
        for tag, words, want, coords, chk in op.sets:
            for x in coords:
                assert V.in_contract(x), (op.name, tag)
                n += 1
    assert n > 10000
    lo, hi = V.CONTRACT
    assert not V.in_contract(V.to_limbs(hi)) and not V.in_contract(V.to_limbs(lo)) and not V.in_contract([-1] + [0] * 13)
    assert V.in_contract([V.MASK] * 13 + [V.TOP_HI]) and V.in_contract([0] * 13 + [V.TOP_LO + 1]) and not V.in_contract([V.MASK] * 13 + [V.TOP_HI + 1])
    # the affine operands of the mixed additions are from_raw's: (-q, 2q)
    for name, at in (("PMADD_NEG", V.PT), ("SRTG2_MADD", V.PT)):
        for tag, words, want, coords, chk in ops[name].sets:
            for k in range(4):
                assert -Q < V.from_limbs(words[at + k * V.L:at + (k + 1) * V.L]) < 2 * Q, (name, tag)


def test_model_agrees_with_hostmath_on_every_set(ops):
    """the expected words, read as points (or bytes), are the host's; sets that are no curve point have a check only where the
    routine is a polynomial map hostmath has too (pdblj) or writes canonical values (affine_out, st_vm)"""
    ran = 0
    for op in ops.values():
        for tag, words, want, coords, chk in op.sets:
            if chk is not None:
                try:
                    chk(want)
                except AssertionError as e:
                    raise AssertionError("%s %s: %s" % (op.name, tag, e))
                ran += 1
    assert ran > 900
    for name in ("PADD", "PDBL", "PDBLJ", "TO_JACOBIAN", "TO_HOMOGENEOUS", "SP4_PADD", "SP4_PDBL", "SP4_PDBLJ", "PMADD_NEG", "SRTG2_MADD", "SRTG1_MADD"):
        assert sum(1 for s in ops[name].sets if s[4] is not None) >= 30, name
    for name in [n for n in ops if n.startswith("CHAIN")]:
        assert all(s[4] is not None for s in ops[name].sets), name


def test_affine_and_vm_words_are_the_hosts(ops):
    for tag, words, want, coords, chk in ops["SRTG2_AFFINE_OUT"].sets:
        P = V.pt_of(words[:V.PT])
        if not words[V.PT]:
            assert want == [V.FILL] * 49, tag
            continue
        X, Y, Z = V.vals(P)
        b = b"".join((w & 0xFFFFFFFF).to_bytes(4, "little") for w in want[:48])
        x, y = ((int.from_bytes(b[96 * k:96 * k + 48], "big"), int.from_bytes(b[96 * k + 48:96 * k + 96], "big")) for k in range(2))
        assert max(x + y) < Q, tag
        if V.F2.is_zero(Z):
            assert (x, y) == ((0, 0), (0, 0)) and want[48] & 0xFF == 1, tag
        else:
            assert V.F2.mul(x, Z) == X and V.F2.mul(y, Z) == Y and want[48] & 0xFF == (0 if b.strip(b"\0") else 1), tag
    for tag, words, want, coords, chk in ops["ST_VM"].sets:
        for k, part in enumerate(coords):
            v = sum((w & 0xFFFFFFFF) << (32 * i) for i, w in enumerate(want[12 * k:12 * k + 12]))
            assert v < Q and v == MV.res(part) * (1 << 384) % Q, (tag, k)
    for tag, words, want, coords, chk in ops["PT_LD_ST"].sets:
        assert want == words, tag


def _pairs_of_quad(want, npts):
    pw = npts * V.PT
    return want[:pw], want[pw:2 * pw]


def test_pair_and_quad_forms_agree(ops):
    """the same sets through sp2 and sp4: both pairs of the quad end with the same words, every coordinate is the same residue as
    sp2's (the formulas are the same polynomials, on the curve or not), and the words differ where sp4 reduces differently"""
    for a, b, npts in (("PADD", "SP4_PADD", 1), ("PDBL", "SP4_PDBL", 1), ("PDBLJ", "SP4_PDBLJ", 1), ("TO_JACOBIAN", "SP4_TO_JACOBIAN", 1),
                       ("TO_HOMOGENEOUS", "SP4_TO_HOMOGENEOUS", 1), ("CHAIN_ADD8_2", "CHAIN_ADD8_4", 8), ("CHAIN_JAC_16_2", "CHAIN_JAC_16_4", 18),
                       ("CHAIN_JAC_60_2", "CHAIN_JAC_60_4", 62), ("CHAIN_CANCEL_2", "CHAIN_CANCEL_4", 5), ("CHAIN_RUNNING_2", "CHAIN_RUNNING_4", 8)):
        sa, sb = ops[a].sets, ops[b].sets
        assert [s[0] for s in sa] == [s[0] for s in sb] and [s[1] for s in sa] == [s[1] for s in sb], (a, b)
        differ = 0
        for (tag, _, wa, _, _), (_, _, wb, _, _) in zip(sa, sb):
            p0, p1 = _pairs_of_quad(wb, npts)
            assert p0 == p1, (b, tag)
            for k in range(npts):
                ra, rb = V.vals(V.pt_of(wa[k * V.PT:(k + 1) * V.PT])), V.vals(V.pt_of(p0[k * V.PT:(k + 1) * V.PT]))
                if a.startswith("CHAIN") and k > 0:     # later steps start from different words of the same point: equal as points
                    continue
                assert ra == rb, (a, tag, k)
            differ += wa[:npts * V.PT] != p0
            assert wa[npts * V.PT:] == wb[2 * npts * V.PT:], (a, tag)          # affine_out's bytes
        if a in ("PADD", "PDBL", "CHAIN_ADD8_2"):
            assert differ > 0, a


def test_outputs_stay_in_the_contract(ops):
    """what a routine stores is an operand again: every coordinate of every expected point of the on-curve sets and of every chain"""
    for op in ops.values():
        if op.group not in ("pair", "quad", "chain") or op.name in ("ST_VM", "SRTG2_AFFINE_OUT"):
            continue
        npts = (op.wout - (49 if op.name.startswith("CHAIN_CANCEL") else 0)) // V.PT
        for tag, words, want, coords, chk in op.sets:
            if tag.startswith(("coord", "extreme")):
                continue
            for P in V.pts_of(want, npts):
                for c in P:
                    assert V.in_contract(c[0]) and V.in_contract(c[1]), (op.name, tag)


def test_extreme_sets_reach_the_largest_columns(ops, capsys):
    """the largest column sum of limb products of every formula is met on an extreme set, not a random one, and fits 64 bits"""
    lines = []
    for name in ("PNEG", "PDBL", "PADD", "PMADD_NEG", "TO_JACOBIAN", "PDBLJ", "TO_HOMOGENEOUS", "SP4_PDBLJ", "SP4_PDBL", "SP4_PADD",
                 "SP4_TO_JACOBIAN", "SP4_TO_HOMOGENEOUS"):
        peaks = V.PEAK[name]
        tag, pk = max(peaks.items(), key=lambda kv: kv[1])
        lines.append("%-18s %.4f x 2^63 (%.2f units of 13 x 2^56) on %s" % (name, pk / float(1 << 63), pk / (13.0 * (1 << 56)), tag))
        if name == "PNEG":
            assert pk == 0
            continue
        assert pk < 1 << 63, name
        assert tag.startswith("extreme"), (name, tag)
        assert max(v for t, v in peaks.items() if not t.startswith(("extreme", "coord"))) < pk, name
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    for g, (n, s, p) in V.summary().items():
        assert n and s and p < 1.0, g


def test_jacobian_infinity_is_a_fixed_point_for_60_steps(ops, capsys):
    """pdblj "fixes (1 : 1 : 0)": in VALUE it does, for 60 steps, on pairs and on quads; the LIMBS are recorded here"""
    lines = []
    for name in ("CHAIN_JAC_60_2", "CHAIN_JAC_60_4"):
        for tag, words, want, coords, chk in ops[name].sets:
            if not tag.startswith("inf/"):
                continue
            steps = V.pts_of(want, 62)
            assert steps[0][0] == V.ONE2 and steps[0][1] == V.ONE2, (name, tag)     # to_jacobian recognised the zero
            seen = []
            for k, P in enumerate(steps[:61]):
                X, Y, Z = V.vals(P)
                assert X == (1, 0) and Y == (1, 0) and Z == (0, 0), (name, tag, k)
                assert all(V.in_contract(part) for c in P for part in c), (name, tag, k)
                seen.append(tuple(V.from_limbs(part) for c in P[:2] for part in c))
            X, Y, Z = V.vals(steps[61])
            assert X == (0, 0) and Y == (1, 0) and Z == (0, 0), (name, tag)
            period = next((k for k in range(1, 60) if seen[60] == seen[60 - k]), None)
            first = next(k for k in range(61) if seen[k:] == seen[k:k + 1] * (61 - k)) if period == 1 else None
            top = max(abs(P[i][j][13]) for P in steps for i in range(3) for j in range(2))
            lines.append("%s %-22s X, Y of (1 : 1 : 0) over 60 pdblj: %d different limb forms, %s; largest |top digit| %d (q's: %d)"
                         % (name, tag, len(set(seen)), "stationary from step %d" % first if period == 1 else "period %s" % period, top, V.QT))
    assert len(lines) >= 6
    with capsys.disabled():
        print("\n" + "\n".join(lines))


POINT_MUTANTS = {
    "pick_swapped": ("SP4_PADD", "CHAIN_ADD8_4", "CHAIN_RUNNING_4"),
    "pair1_no_oth": ("SP4_PADD", "CHAIN_ADD8_4"),
    "t1m_z3": ("PADD", "SRTG2_ADD", "SP4_PADD", "CHAIN_ADD8_2", "CHAIN_RUNNING_2"),
    "b3_no_3": ("PADD", "PDBL", "SRTG2_DBL", "SP4_PADD", "SP4_PDBL", "CHAIN_ADD8_2"),
    "pmadd_z2_zero": ("PMADD_NEG", "SRTG2_MADD"),
    "toj_no_select": ("TO_JACOBIAN", "SP4_TO_JACOBIAN", "CHAIN_JAC_1_2", "CHAIN_JAC_16_4", "CHAIN_CANCEL_2", "CHAIN_CANCEL_4"),
    "toh_leaves_z": ("TO_HOMOGENEOUS", "SP4_TO_HOMOGENEOUS", "CHAIN_JAC_2_2", "CHAIN_JAC_2_4"),
    "dblj_4c": ("PDBLJ", "SP4_PDBLJ", "CHAIN_JAC_1_2", "CHAIN_JAC_1_4"),
}
DIGIT_MUTANTS = {"no_carry": "LANE_DIGIT", "big_ge": "LANE_DIGIT", "no_second_word": "SRT_DIGIT_KEY", "sign_at_half": "SRT_DIGIT_KEY"}


@pytest.mark.parametrize("mutant", sorted(POINT_MUTANTS) + sorted(DIGIT_MUTANTS) + ["affine_no_conjugate"])
def test_mutants_of_the_model_are_caught(ops, mutant):
    """a subtly wrong routine: its words differ from the expected ones on some set of every op it belongs to, and where the op has
    an independent check, that check refuses the mutant's words on some set"""
    if mutant == "affine_no_conjugate":                 # 1 / Z taken as Z / N(Z): wrong unless Z is real
        op = ops["SRTG2_AFFINE_OUT"]
        caught = 0
        for tag, words, want, coords, chk in op.sets:
            X, Y, Z = V.vals(V.pt_of(words[:V.PT]))
            if not words[V.PT] or V.F2.is_zero(Z):
                continue
            zi = V.F2.mul(Z, (pow(Z[0] * Z[0] + Z[1] * Z[1], -1, Q), 0))
            wrong = V.affine_words(2, (V.F2.mul(X, zi), V.F2.mul(Y, zi)))
            caught += wrong != want
            if "z-real" in tag:
                assert wrong == want
        assert caught >= 10
        return
    names = POINT_MUTANTS.get(mutant) or (DIGIT_MUTANTS[mutant],)
    V.MUT.add(mutant)
    try:
        for name in names:
            op = ops[name]
            differ = refused = 0
            for tag, words, want, coords, chk in op.sets:
                got = [int(w) for w in op.model(words)]
                if got == want:
                    continue
                differ += 1
                if chk is not None:
                    try:
                        chk(got)
                    except AssertionError:
                        refused += 1
            assert differ > 0, (mutant, name)
            if any(s[4] is not None for s in op.sets):
                assert refused > 0, (mutant, name)
    finally:
        V.MUT.discard(mutant)
    assert not V.MUT


def test_digit_models_put_the_scalar_together_again(ops):
    for tag, s in V.digit_scalars():
        w = V.scalar_words(s)
        d = [V.lane_digit(w, win) for win in range(64)]
        assert sum(x << (4 * i) for i, (x, _) in enumerate(d)) == s, tag
        assert {b for _, b in d} == {int((s >> 224) > 0x77777776)}, tag
        for cb in range(5, V.SRT_MAXBITS + 1):
            half, rec = 1 << (cb - 1), V.srt_record(s, cb)
            rows = [V.srt_digit_key(rec, i, cb) for i in range(V.srt_windows(cb))]
            assert sum((v - half) << (cb * i) for i, (v, k, sg, nz) in enumerate(rows)) == s, (tag, cb)
            assert all(nz == int(v != half) and sg == int(v < half) and (not nz or k == abs(v - half) - 1) for v, k, sg, nz in rows), (tag, cb)
    assert sum(V.lane_digit_null(win) << (4 * win) for win in range(64)) == 1
    # the classes of the issue are there: both sides of the `big` switch, the ripples, every nibble at every window, every cb and
    # window, the ninth word, the biased digits at their ends
    tags = {s[0] for s in ops["LANE_DIGIT"].sets}
    assert {"top/77777776/ones/w63", "top/77777777/zeros/w0", "ripple/1/w1", "ripple/8/w63", "nibbles-8/w5", "nibble/15/w63", "nibble/0/w0"} <= tags
    srt = ops["SRT_DIGIT_KEY"].sets
    assert {(s[1][10], s[1][9]) for s in srt} == {(cb, w) for cb in range(5, 15) for w in range(V.srt_windows(cb))}
    ninth = [s for s in srt if s[1][10] in (13, 14) and s[1][9] == V.srt_windows(s[1][10]) - 1]
    assert ninth and all((s[1][9] * s[1][10] & 31) + s[1][10] > 32 and (s[1][9] * s[1][10] >> 5) == 7 for s in ninth)
    for cb in range(5, 15):
        half = 1 << (cb - 1)
        assert {0, half - 1, half, half + 1, (1 << cb) - 1} <= {s[2][0] for s in srt if s[1][10] == cb}, cb


needs_hipcc = pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="no hipcc")


@needs_hipcc
def test_check_file_compiles():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", CSRC, os.path.join(CSRC, "blsgpu_curve_check.hip")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
