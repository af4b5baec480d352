"""CPU: the limb model of tests/fx_vectors.py (reduce_small, cyc_sqr, frob, tinv, fq_inverse of csrc/blsgpu_fexp.hip and k_fexp_team's
inline CONJ and slot traffic) against vmgen/fexp_model.py mod q on every set, the contract of every operand and of every result, the two
range claims at reduce_small, the column sums the extreme sets reach, what the limbs of the constant 1 do under repeated squaring, the
whole script on limbs with every column asserted, and the mutants of the model the sets must tell from it.  tests/test_gpu_fx.py runs the
same sets on the compiled routines."""
import os
import shutil
import subprocess

import pytest

import fx_vectors as V
from vmgen import fexp_model as F

Q = V.Q
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-bls_amd", "csrc")
UNIT = 13.0 * (1 << 56)                                # a full column of products of digits: 13 of them (the top limbs are small)


@pytest.fixture(scope="module")
def ops():
    return V.ops()


def test_op_table(ops):
    assert {n: op.code for n, op in ops.items()} == {"REDUCE_SMALL": 0, "FQ_INVERSE": 1, "CYC_SQR": 10, "CYC_SQR_CHAIN": 11, "FROB": 12, "TINV": 13,
                                                    "CONJ": 14, "SLOT_ROUNDTRIP": 15}
    for op in ops.values():
        assert op.sets and len({s[0] for s in op.sets}) == len(op.sets), op.name
        for n in op.counts:
            assert len(V.call_sets(op, n)) == n
    for name in ("CYC_SQR", "CONJ", "TINV"):
        assert {"random", "special", "subfield", "extreme"} <= {s[0].split("/")[0] for s in ops[name].sets}, name
        tags = {s[0] for s in ops[name].sets}
        assert {"subfield/fq2", "subfield/fq6", "subfield/cyc/golden0", "subfield/cyc/model0", "subfield/one/form0", "special/zero-team"} <= tags
        assert {"subfield/w%d" % k for k in range(6)} <= tags and len([t for t in tags if t.startswith("extreme/")]) == 16
    assert {"t/real", "t/imag", "t/norm1", "t/norm-1", "t/zero-q-limbs"} <= {s[0] for s in ops["TINV"].sets}
    rs = {s[0].split("/")[0] for s in ops["REDUCE_SMALL"].sets}
    assert rs == {"random", "special", "multiple", "switch", "float"}
    # the chain lengths are read from the script
    run = max(a for op, a in F.script() if op == F.CSQ)
    assert sorted(ops["CYC_SQR_CHAIN"].by_n) == [1, 2, run, run + 1] and run + 1 <= V.MAX_CHAIN
    # a uniform run-time word per call, and every set reached
    for name in ("CYC_SQR_CHAIN", "FROB"):
        op, seen, base = ops[name], set(), 0
        while len(seen) < len(op.sets):
            sets = V.call_sets(op, 41, base)
            assert len({op.sets[k][1][V.TV] for k in sets}) == 1, name
            seen |= set(sets)
            base += 41
            assert base < 64 * 41


def test_every_operand_lies_in_the_contract_it_claims(ops):
    n = 0
    for op in ops.values():
        for s in op.sets:
            kind = "rsclaim" if op.name == "REDUCE_SMALL" and s[0].endswith("/claim") else V.CONTRACT[op.name][0]
            for x in s[3]:
                assert V.in_kind(kind, x), (op.name, s[0])
                n += 1
    assert n > 5000
    # the contract has edges
    t_lo, t_hi = V.top_ends("dense")
    assert V.in_kind("dense", [V.MASK] * 13 + [t_hi]) and not V.in_kind("dense", [V.MASK] * 13 + [t_hi + 1])
    assert V.in_kind("dense", [0] * 13 + [t_lo]) and not V.in_kind("dense", [0] * 13 + [t_lo - 1]) and not V.in_kind("dense", [-1] + [0] * 13)
    assert not V.in_kind("rs", [V.RS_HI] + [0] * 13) and not V.in_kind("rs", [V.RS_LO] + [0] * 13) and V.in_kind("rs", [V.RS_HI - 1] * 13 + [0])
    # the call-site sets of reduce_small are many, and some operand goes below the -10 q of the old comment
    rs = [s for s in ops["REDUCE_SMALL"].sets if not s[0].endswith("/claim")]
    assert len(rs) > 150 and min(V.from_limbs(s[1]) for s in rs) < -10 * Q and max(V.from_limbs(s[1]) for s in rs) > 13 * Q


def test_model_agrees_with_the_independent_reference_on_every_set(ops):
    """the expected words, read as residues, are vmgen/fexp_model's (or satisfy the defining identity), and lie in the result's contract"""
    ran = 0
    for op in ops.values():
        for s in op.sets:
            try:
                s[4](s[2])
            except AssertionError as e:
                raise AssertionError("%s %s: %s" % (op.name, s[0], e))
            ran += 1
    assert ran == sum(len(op.sets) for op in ops.values()) > 1000


def test_results_stay_in_the_contract_of_the_next_step(ops):
    for name in ("CYC_SQR", "FROB", "TINV", "CONJ", "SLOT_ROUNDTRIP"):
        kind = V.CONTRACT[name][1]
        for s in ops[name].sets:
            assert all(V.in_kind(kind, p) for p in V.parts_of(V.team_of(s[2]))), (name, s[0])
    for s in ops["CYC_SQR_CHAIN"].sets:                # what a chain step returns is an operand of cyc_sqr, CONJ, MUL and ST again
        n = s[1][V.TV]
        for i in range(3 if n >= 2 else 2):
            for p in V.parts_of(V.team_of(s[2][i * V.TV:(i + 1) * V.TV])):
                assert V.in_kind("small", p) and V.in_kind("dense", p) and V.in_kind("acc", p), s[0]
    for s in ops["REDUCE_SMALL"].sets + ops["FQ_INVERSE"].sets:
        assert V.in_kind("small", s[2]), s[0]


def test_the_two_range_claims_at_reduce_small(ops, capsys):
    """(-11q, 14q), not (-10q, 14q), is what 3 t -+ 2 f can be; and "(-2q, 2q) for any |x| < 2^12 q" holds with room: the result is within
    q / 2 + q / 512 of zero on every set, the multiples of q up to 4095 q and both sides of every switch of the estimate included"""
    fe, dense = V.KINDS["fe"], V.KINDS["dense"]
    lo = min(3 * fe[0] - 2 * dense[1], 3 * fe[0] + 2 * dense[0])
    hi = max(3 * fe[1] - 2 * dense[0], 3 * fe[1] + 2 * dense[1])
    assert (lo, hi) == V.KINDS["rs"] == (-11 * Q, 14 * Q)
    t, f = V.to_limbs(-Q + 1), V.to_limbs(4 * Q - 1)   # admissible, and below the old comment's -10 q
    x = [3 * a - 2 * b for a, b in zip(t, f)]
    assert V.in_kind("fe", t) and V.in_kind("dense", f) and V.in_kind("rs", x) and V.from_limbs(x) < -10 * Q
    V.chk_reduce(x)(V.reduce_small(x))
    worst, worst_tag, ks = 0, None, set()
    for s in ops["REDUCE_SMALL"].sets:
        v, k = V.from_limbs(s[2]), (V.from_limbs(s[1]) - V.from_limbs(s[2])) // Q
        assert (V.from_limbs(s[1]) - v) % Q == 0 and -2 * Q < v < 2 * Q and V.nearest_ok(v), s[0]
        ks.add(k)
        if abs(v) > worst:
            worst, worst_tag = abs(v), s[0]
    assert {0, 1, -1, 10, -10, 14, -14, 4095, -4095, 2048, -2048} <= ks
    # the switches were found: either side of each, the estimate differs by one, and the top limbs past 2^24 are there
    pts = V.rs_switch_points()
    assert len(pts) == 32 and all(V.rs_estimate(t) == k and V.rs_estimate(t + 1) == k + 1 for k, t in pts)
    assert any(abs(s[1][13]) > 1 << 24 for s in ops["REDUCE_SMALL"].sets)
    with capsys.disabled():
        print("\nreduce_small: largest |result| %.6f q on %s (claimed: < 2 q; nearest multiple: <= %.6f q)" % (worst / Q, worst_tag, V.NEAREST / Q))


def test_extreme_sets_reach_the_largest_columns(ops, capsys):
    """cyc_sqr's comment counts 8 units for the imaginary part of an even lane; digits in [0, 2^28) reach 4.000 (fx_vectors' docstring):
    met on extreme (and all-ones special) sets, never on a random one"""
    lines = []
    for name in ("CYC_SQR", "CYC_SQR_CHAIN", "FROB", "TINV"):
        peaks = V.PEAK[name]
        tag, pk = max(peaks.items(), key=lambda kv: kv[1])
        lines.append("%-14s %.4f x 2^63 (%.3f units of 13 x 2^56, bound %d) on %s" % (name, pk / float(1 << 63), pk / UNIT, V.BOUND.get(name, 4), tag))
        assert pk < 1 << 63 and pk / UNIT <= V.BOUND.get(name, 4), name
        rnd = max(v for t, v in peaks.items() if "random" in t)
        assert rnd < pk, name
    ext = max(v for t, v in V.PEAK["CYC_SQR"].items() if t.startswith("extreme"))
    assert ext == max(V.PEAK["CYC_SQR"].values()) and 3.999 < ext / UNIT <= 4.0 < V.CLAIMED["CYC_SQR"]
    # the attainable figure by enumeration: over all 16 patterns of (xr, xi, yr, yi) in {0, 1} the columns of every lane role
    best = 0
    for p in range(16):
        xr, xi, yr, yi = (p & 1, p >> 1 & 1, p >> 2 & 1, p >> 3 & 1)
        cols = [xr * xr - xi * xi + (yr - yi) ** 2 - 2 * yi * yi, 2 * xr * xi + (yr + yi) ** 2 - 2 * yi * yi,        # even lanes
                2 * xr * (yr - yi) - 2 * xi * (yr + yi), 2 * xr * (yr + yi) + 2 * xi * (yr - yi),                    # lane 1
                2 * xr * yr - 2 * xi * yi, 2 * xr * yi + 2 * xi * yr]                                                # lanes 3, 5
        best = max(best, max(abs(c) for c in cols))
    assert best == 4
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_the_constant_one_is_stationary_under_squaring(ops, capsys):
    """the script squares 315 times; a team in a subfield squares the constant 1 (or 0) on some lanes every time.  From R + rep q on
    lane 0 the limbs reach R itself after one squaring and stay there"""
    forms, info = V.one_chain()
    assert sorted(info) == [-1, 0, 1, 2, 3] and len(forms) == 5
    one = V.flat_team(V.team_mont([(1, 0)] + [(0, 0)] * 5))
    for rep, (nforms, start, period) in info.items():
        assert period == 1 and start <= 1 and nforms <= 2, rep
    assert V.flat_team(V.cyc_sqr(V.team_of(one))) == one
    for w in forms:
        assert V.res6(V.team_of(w)) == [(1, 0)] + [(0, 0)] * 5 and V.flat_team(V.cyc_sqr(V.team_of(w))) == one
    run = V.longest_run()
    for s in ops["CYC_SQR_CHAIN"].sets:
        if "subfield/one" in s[0]:
            assert s[2][:V.TV] == one and s[2][V.TV:2 * V.TV] == one, s[0]
        if "zero-team" in s[0]:
            assert s[2][:V.TV] == [0] * V.TV, s[0]
    with capsys.disabled():
        print("\nthe constant 1 over %d squarings: %d limb forms (R + rep q, rep = 0, 1, -1, 2, 3), stationary at R from step 1 on" % (run + 1, len(forms)))


def test_script_sites_are_what_the_check_file_lists():
    sites = V.script_sites()
    assert sites["CSQ"] == {"dense", "small"} and sites["TINV"] == {"dense"}
    assert sites["FROB0"] == sites["FROB1"] == sites["FROB2"] == {"dense"}
    assert sites["CONJ"] == {"dense", "fe", "small"}
    hull = {"dense", "fe", "small", "conj(dense)", "conj(fe)", "conj(small)"}
    assert sites["MUL"] <= hull and sites["MUL/slot"] <= hull and sites["ST"] <= hull
    lo, hi = V.KINDS["acc"]
    for k in ("dense", "fe", "small"):                 # conj(k) is norm(-x) on odd lanes, x on even ones: inside acc
        assert lo <= -V.KINDS[k][1] and V.KINDS[k][1] <= hi and lo <= V.KINDS[k][0]


def test_script_audit(capsys):
    """the limb model through the WHOLE script, the 64-bit column asserted in every dot, the residues compared with vmgen/fexp_model
    after every entry, every operand inside the contract of the op it enters: the reference's vectors and a team of every subfield class"""
    import random
    rnd = random.Random("fx:audit")
    z = (0, 0)
    inputs = [("golden%d" % i, v) for i, v in enumerate(V.golden_inputs())]
    inputs += [("one", [(1, 0)] + [z] * 5), ("fq2", [(rnd.randrange(Q), rnd.randrange(Q))] + [z] * 5),
               ("fq6", [(rnd.randrange(Q), rnd.randrange(Q)) if k % 2 == 0 else z for k in range(6)]),
               ("w1", [z, (1, 0)] + [z] * 4), ("cyclotomic", V.cyclotomic_of(V.rnd_val(rnd)))]
    S = F.script()
    assert len(S) == 122 and sum(a for op, a in S if op == F.CSQ) == 315
    audit = {}
    for name, vals in inputs:
        got = V.run_script_limbs(vals, audit)
        assert got == F.run_script(vals), name
        if name.startswith("golden"):
            assert got == V.golden_cyclotomic()[int(name[6:])], name
    lines = ["op kind   largest column (units of 13 x 2^56 / bound)   widest operand (|value| / q, contract)"]
    for kind, width in (("MUL", 4), ("CSQ", 4), ("FROB", 4), ("TINV", 4), ("CONJ", 4)):
        pk, wide = audit[kind]
        assert wide < width, kind
        if kind in V.AUDIT_BOUND:
            assert pk / UNIT <= V.AUDIT_BOUND[kind] and pk < 1 << 63, kind
        lines.append("%-8s  %.3f / %s   %.3f / %d" % (kind, pk / UNIT, V.AUDIT_BOUND.get(kind, "-"), wide, width))
    with capsys.disabled():
        print("\n" + "\n".join(lines))


MUTANTS = {
    "rs_floor": ("REDUCE_SMALL", "CYC_SQR", "CYC_SQR_CHAIN"),
    "rs_k_plus_1": ("REDUCE_SMALL", "CYC_SQR", "CYC_SQR_CHAIN"),
    "no_3x": ("CYC_SQR", "CYC_SQR_CHAIN"),
    "parity": ("CYC_SQR", "CYC_SQR_CHAIN"),
    "pair_swapped": ("CYC_SQR", "CYC_SQR_CHAIN"),
    "lane1_no_xi": ("CYC_SQR", "CYC_SQR_CHAIN"),
    "a3_odd": ("CYC_SQR", "CYC_SQR_CHAIN"),
    "frob_conj_q2": ("FROB",),
    "frob_gamma_rev": ("FROB",),
    "tinv_leaves_lanes": ("TINV",),
    "conj_even": ("CONJ",),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutants_of_the_model_are_caught(ops, mutant):
    """a subtly wrong routine: on some set of every op it belongs to its words differ from the expected ones AND the op's independent
    check refuses them.  (The issue's "pair table with lanes 1 and 4 exchanged" is the identity -- both lanes square pair 2 --, so
    pair_swapped exchanges the entries of lanes 1, 4 with those of lanes 2, 5.)"""
    V.MUT.add(mutant)
    try:
        for name in MUTANTS[mutant]:
            op = ops[name]
            differ = refused = 0
            for k, s in enumerate(op.sets):
                got = [int(w) for w in V.model_of(op, k)(s[1])]
                if got == s[2]:
                    continue
                differ += 1
                try:
                    s[4](got)
                except AssertionError:
                    refused += 1
            assert differ > 0 and refused > 0, (mutant, name, differ, refused)
    finally:
        V.MUT.discard(mutant)
    assert not V.MUT


def test_an_inversion_without_zero_to_zero(ops):
    """0 -> 0 is the inversion's own property: fq_inverse's check refuses a routine that lacks it.  tinv cannot show the lack in VALUE
    -- conj(t) times anything is 0 when t is, and tr^2 + ti^2 = 0 only then (q = 3 mod 4) --, but its WORDS differ where t is zero in
    the limbs of q"""
    V.MUT.add("tinv_no_zero")
    try:
        op = ops["TINV"]
        differ = [s[0] for s in op.sets if [int(w) for w in op.model(s[1])] != s[2]]
        assert "t/zero-q-limbs" in differ
        for s in op.sets:
            s[4]([int(w) for w in op.model(s[1])])
    finally:
        V.MUT.discard("tinv_no_zero")
    inv = ops["FQ_INVERSE"]
    zeros = [s for s in inv.sets if V.from_limbs(s[1]) % Q == 0]
    assert len(zeros) >= 2 and all(V.from_limbs(s[2]) % Q == 0 for s in zeros)
    for s in zeros:
        with pytest.raises(AssertionError):
            s[4](V.to_limbs(V.ONE))


needs_hipcc = pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="no hipcc")


def _hipcc(args):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", CSRC] + args,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


@needs_hipcc
def test_check_file_compiles():
    r = _hipcc([os.path.join(CSRC, "blsgpu_fx_check.hip")])
    assert r.returncode == 0, r.stdout[-4000:]


@needs_hipcc
def test_fermat_branch_compiles():
    """tinv's BLSGPU_FEXP_FERMAT branch, which no library builds: the check file is a translation unit that includes blsgpu_fexp.hip"""
    r = _hipcc(["-DBLSGPU_FEXP_FERMAT", os.path.join(CSRC, "blsgpu_fx_check.hip")])
    assert r.returncode == 0, r.stdout[-4000:]
