"""CPU: the limb model of tests/h2c_vectors.py (swl::jacobi, chi, sgn, red, inv, scale, ldv / stv / st_zero, the two power loops, pow_e,
field_element<0 / 1>, sel, sha256_block) against the independent integer reference on every set, the range every operand claims, the
schedule and slot numbers against csrc/vm_tables.h, the largest iteration the binary symbol routine works in, and the mutants of the
model the sets must tell from it.  tests/test_gpu_h2c_check.py runs the same sets on the compiled routines.  None of the routines has a
host build (fp28.h is device code), so the check file is compiled for the device with -fsyntax-only here and the model stands alone."""
import os
import re
import shutil
import subprocess

import pytest

import h2c_vectors as V
import test_jacobi_model as J

Q = V.Q


@pytest.fixture(scope="module")
def ops():
    return V.ops()


def test_op_table(ops):
    assert {n: op.code for n, op in ops.items()} == {
        "JACOBI_BIN": 0, "CHI": 1, "SGN": 2, "RED_02": 3, "RED_11": 4, "INV": 5, "INV_WAVE": 5, "SCALE": 6, "LDV_STV": 7, "POW_E": 10,
        "POW_LOOP_WIN": 11, "POW_LOOP_B4": 12, "FIELD_ELEMENT_0": 20, "FIELD_ELEMENT_1": 21, "FE1_REDUCE": 22, "SEL": 23, "SHA256_BLOCK": 24}
    with open(os.path.join(V.CSRC, "blsgpu_h2c_check.hip")) as f:
        listed = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"X\((\w+), (\d+)\)", f.read()))
    assert listed == {n: op.code for n, op in ops.items() if n != "INV_WAVE"}
    for op in ops.values():
        assert op.sets and all(len(V.call_sets(op, n)) == n for n in op.counts), op.name
    assert ops["POW_LOOP_WIN"].counts == ops["POW_LOOP_B4"].counts == (1, 63, 64, 65, 127, 128, 129, 257)
    assert all(n % 128 for n in ops["POW_LOOP_B4"].counts if n != 128)       # k_pow2's clamp repeats the last value


def test_classes_are_present(ops):
    tags = lambda name: {s[0] for s in ops[name].sets}
    jb = {s[0]: V.from_words(s[1]) for s in ops["JACOBI_BIN"].sets}
    vals = set(V.from_words(s[1]) for s in ops["JACOBI_BIN"].sets)
    assert {0, 1, 2, 3, Q - 1, Q - 2, (Q - 1) // 2, (Q + 1) // 2} <= vals
    assert all({(1 << k) - 1, 1 << k, (1 << k) + 1} <= vals for k in range(2, 381))
    assert {"mod8/%d/%d" % (r, c) for r in range(8) for c in (1, -1)} <= set(jb) and all(jb["mod8/%d/1" % r] % 8 == r for r in range(8))
    assert {"longest", "random"} <= set(jb)
    chi = tags("CHI")
    assert {"corner/+0", "corner/+1", "corner/-1", "corner/zero-q-limbs", "longest/+0", "random/+0", "random/+1", "random/-1"} <= chi
    assert sum(1 for s in ops["CHI"].sets if s[0].startswith("pow2/")) >= 1100
    sg = tags("SGN")
    for v in ("half", "half+1", "zero", "q-1"):
        assert {"%s/%+d" % (v, k) for k in (-2, -1, 0, 1, 2, 3)} <= sg | {"zero/-2"}, v      # (0 - 2q is the open end of the range)
    assert {"zero/+0", "zero/+1", "one/+0", "q-1/+0", "random/+0"} <= tags("INV") and len(ops["INV_WAVE"].sets) >= 5
    zeros = [i for i, s in enumerate(ops["INV"].sets[:64]) if V.res(s[1]) == 0]
    assert len(zeros) >= 4 and len(zeros) < 16         # zero beside non-zero values inside the first wavefront
    for name in ("POW_E", "POW_LOOP_WIN", "POW_LOOP_B4"):
        assert {"zero", "one", "q-1", "R", "R2", "square", "non-square", "random"} <= {t.split("/")[0] for t in tags(name)}, name
    assert any(V.from_words(s[1]) >= Q for s in ops["POW_LOOP_WIN"].sets)     # a base in (q, 2q)
    pe = [(s[0].split("/")[0], V.from_limbs(s[1])) for s in ops["POW_E"].sets]
    for tag in ("zero", "one", "q-1", "random"):       # pow_e's operand is red's output, (-q, 2q): every third of it
        assert any(t == tag and Q <= v < 2 * Q for t, v in pe) and any(t == tag and 0 <= v < Q for t, v in pe), tag
    assert all(any(t == tag and -Q < v < 0 for t, v in pe) for tag in ("one", "q-1", "random"))
    assert all(any(t == tag and 0 <= v < Q for t, v in pe) for tag in ("R", "R2", "square", "non-square", "half"))
    assert sum(1 for _, v in pe if Q < v < 2 * Q) >= 6 and sum(1 for _, v in pe if v < 0) >= 6
    ts = set()
    for s in ops["FIELD_ELEMENT_0"].sets:
        b = V.struct.pack("<24I", *[w & V.M32 for w in s[1]])
        ts |= {int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big")}
    assert {0, 1, Q - 1, Q, Q + 1, 2 * Q, V.R384 - 1} <= ts
    fr = {(V.from_words(s[1][3::-1]), V.from_words(s[1][:3:-1])) for s in ops["FE1_REDUCE"].sets}
    assert {(h, l) for h in (0, (1 << 128) - 1) for l in (0, Q - 1, Q, V.R384 - 1)} <= fr
    conds = [s[1][0] != 0 for s in ops["SEL"].sets]
    assert any(a != b for a, b in zip(conds, conds[1:])) and True in conds and False in conds
    slots = {w for s in ops["LDV_STV"].sets for w in s[1][:3]}
    assert {V.STATE0, V.STATE1 - 1} <= slots and all(V.STATE0 <= w < V.STATE1 for w in slots)


def test_every_operand_lies_in_the_range_it_claims(ops):
    ranges = {"CHI": (0, 1, -1, 2), "SGN": (0, 1, -2, 4), "RED_02": (0, 2, -2, 4), "RED_11": (1, 1, -3, 3), "INV": (0, 1, -1, 2), "INV_WAVE": (0, 1, -1, 2),
              "POW_E": (0, 1, -1, 2)}
    n = 0
    for name, r in ranges.items():
        for s in ops[name].sets:
            assert V.in_range(s[1], *r), (name, s[0])
            n += 1
    for s in ops["SCALE"].sets:
        assert all(V.in_range(s[1][V.L * k:V.L * (k + 1)], 0, 1, -1, 2) for k in range(3)), s[0]
    for s in ops["SEL"].sets:
        assert all(0 <= d <= V.MASK for k in range(2) for d in s[1][1 + V.L * k:V.L * (k + 1)]), s[0]      # (a select: any digits)
    for s in ops["LDV_STV"].sets:
        assert V.in_range(s[1][3:], 0, 2, -2, 4), s[0]
    for s in ops["JACOBI_BIN"].sets:
        assert 0 <= V.from_words(s[1]) < Q, s[0]
    for name in ("POW_LOOP_WIN", "POW_LOOP_B4"):
        assert all(0 <= V.from_words(s[1]) < 1 << 384 for s in ops[name].sets)
    assert n > 2000
    # the ranges have ends: both are met, and what lies outside is refused
    vals = lambda name: [V.from_limbs(s[1]) for s in ops[name].sets]
    assert min(vals("SGN")) < -Q and max(vals("SGN")) > 3 * Q and min(vals("RED_11")) < -2 * Q and max(vals("RED_02")) > 3 * Q
    assert not V.in_range(V.to_limbs(2 * Q), 0, 1, -1, 2) and not V.in_range([-1] + [0] * 13, 0, 1, -1, 2) and not V.in_range([1 << 28] + [0] * 13, 0, 1, -1, 2)


def test_model_agrees_with_the_independent_reference_on_every_set(ops):
    ran = 0
    for op in ops.values():
        for s in op.sets:
            try:
                s[3](s[2])
            except AssertionError as e:
                raise AssertionError("%s %s: %s" % (op.name, s[0], e))
            ran += 1
    assert ran == sum(len(op.sets) for op in ops.values()) > 3500


def test_schedule_and_slots_are_the_tables(ops):
    """the window schedule and the exponent the model runs are what csrc/vm_tables.h holds"""
    with open(os.path.join(V.CSRC, "vm_tables.h")) as f:
        text = f.read()
    win = re.search(r"BLSVM_POW_WIN\[(\d+)\]\[2\] = \{(.*?)\};", text)
    pairs = [tuple(int(x) for x in p.split(",")) for p in re.findall(r"\{(\d+, \d+)\}", win.group(2))]
    assert pairs == V.POW_WIN and int(win.group(1)) == len(V.POW_WIN)
    e = re.search(r"BLSVM_POW_E\[12\] = \{(.*?)\}", text).group(1)
    assert sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(e.split(","))) == V.EXP_E == (Q - 3) // 4
    assert int(re.search(r"#define BLSVM_POW_WINDOW (\d+)", text).group(1)) == V.E.POW_WINDOW
    assert V.IMG_DW == (V.STATE1 - V.STATE0) * 12 and V.STATE0 == V.H1["H1_T"]
    c2 = re.search(r"#define BLS28_WIDE_C2 \{(.*?)\}", open(os.path.join(V.CSRC, "fp28_mul_gfx950.h")).read()).group(1)
    assert [int(x, 16) for x in c2.split(",")] == V.L_C2


def test_binary_jacobi_iterations(ops, capsys):
    """the routine's budget is 768 iterations, counted from 0; at most bits(a) + bits(q) = 762 of them do work, so the latest working one
    is number 761 at the most: the latest over every set against that"""
    worst, at = 0, None
    for s in ops["JACOBI_BIN"].sets:
        a = V.from_words(s[1])
        j, last = J.jacobi_fixed(a)
        assert [j] == s[2] == [V.m_jacobi(a)], s[0]
        if last > worst:
            worst, at = last, s[0]
    assert worst == V.WORST_ITERATION[0] and 750 <= worst <= 761, worst
    assert all(J.jacobi_fixed(V.from_words(s[1]), worst + 1)[0] == s[2][0] for s in ops["JACOBI_BIN"].sets)
    with capsys.disabled():
        print("\nswl::jacobi: the latest working iteration is number %d (class %s); none works after 761, the budget ends at 767" % (worst, at))


MUTANTS = {
    "recip_or": ("JACOBI_BIN",),
    "halve_37": ("JACOBI_BIN",),
    "sgn_ge": ("SGN",),
    "red_skipped": ("RED_02", "RED_11", "FE1_REDUCE"),
    "inv_zero_one": ("INV", "INV_WAVE"),
    "win_pick_off": ("POW_E", "POW_LOOP_WIN"),
    "b4_digit_bit": ("POW_LOOP_B4",),
    "b4_b2_b3": ("POW_LOOP_B4",),
    "no_hi_c2": ("FIELD_ELEMENT_1", "FE1_REDUCE"),
    "selector_swapped": ("FIELD_ELEMENT_1",),
    "sha_no_final_add": ("SHA256_BLOCK", "FIELD_ELEMENT_1"),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutants_of_the_model_are_caught(ops, mutant):
    """a subtly wrong routine: on some set of every op it belongs to its words differ from the expected ones AND the op's independent
    check refuses them"""
    V.MUT.add(mutant)
    try:
        for name in MUTANTS[mutant]:
            op = ops[name]
            differ = refused = 0
            for s in op.sets:
                got = [int(w) for w in op.model(s[1])]
                if got == s[2]:
                    continue
                differ += 1
                try:
                    s[3](got)
                except AssertionError:
                    refused += 1
                if refused and name.startswith("POW"):
                    break                              # (a power costs ~0.1 s in the model)
            assert differ > 0 and refused > 0, (mutant, name, differ, refused)
    finally:
        V.MUT.discard(mutant)
    assert not V.MUT


needs_hipcc = pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="no hipcc")


@needs_hipcc
def test_check_file_compiles():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", V.CSRC, os.path.join(V.CSRC, "blsgpu_h2c_check.hip")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
