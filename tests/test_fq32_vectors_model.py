"""CPU: the operand sets of tests/fq32_vectors.py (a) through the HOST build of csrc/fq32.h (g++, as
tests/test_abi_and_host.py compiles it; the op bodies are csrc/blsgpu_fq32_check.hip's own, included by the driver)
against the same Python-integer references the GPU test uses -- the first direct test of fat_flip / fat_mac_plain / fat_reduce, fq_sgn, fq_mul_relaxed, fq_canon and fq_sub_mod, and the proof of the
references before a GPU sees them; (b) inside the preconditions each set claims; (c) a range audit of every LIN round
that vmgen packs into vm_tables.h, against the bounds fat_flip and fat_reduce state (no other test asserts them:
vmgen/tablesim.py checks 0 <= V < 2^396 on residues below q only).  Needs no GPU."""
import os
import subprocess

import pytest

import fq32_vectors as V
from vmgen import emit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")
Q, M32 = V.Q, V.M32

# the op bodies of csrc/blsgpu_fq32_check.hip themselves, compiled for the host on fq32.h's host code
HOST_DRIVER = r'''
#include "blsgpu_fq32_check.hip"
#include <stdio.h>
#include <vector>
int main() {
    int op, win, wout, n;
    while (scanf("%d %d %d %d", &op, &win, &wout, &n) == 4) {
        std::vector<uint32_t> in(win), out(wout);
        for (int i = 0; i < n; i++) {
            for (int j = 0; j < win; j++) if (scanf("%x", &in[j]) != 1) return 1;
            for (int j = 0; j < wout; j++) out[j] = 0xAAAAAAAAu;
            if (!fq32check_host(op, in.data(), out.data())) return 2;
            for (int j = 0; j < wout; j++) printf("%08x ", out[j]);
            printf("\n");
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def host_outputs(tmp_path_factory):
    """every set of every host-compilable op through the host build, one process: {op name: [output words per set]}"""
    d = tmp_path_factory.mktemp("fq32host")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(HOST_DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", str(exe), str(src)])
    ops = [op for op in V.OPS.values() if op.host]
    lines = []
    for op in ops:
        lines.append("%d %d %d %d" % (op.code, op.win, op.wout, len(op.sets)))
        lines += [" ".join("%x" % w for w in ws) for _, ws in op.sets]
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    res, at = {}, 0
    for op in ops:
        res[op.name] = [[int(x, 16) for x in out[at + i].split()] for i in range(len(op.sets))]
        at += len(op.sets)
        assert all(len(r) == op.wout for r in res[op.name]), op.name
    return res


@pytest.mark.parametrize("group", V.GROUPS)
def test_host_build_matches_the_references(host_outputs, group):
    """(a) word for word, and the independent integer check on the expected words"""
    n = 0
    for op in V.OPS.values():
        if op.group != group or not op.host:
            continue
        want = V.expected(op.name)
        for k, ((cls, w), e, g) in enumerate(zip(op.sets, want, host_outputs[op.name])):
            if op.check is not None:
                op.check(w, e)
            assert g == e, "%s, set %d of class %s: host build and reference differ\n got  %s\n want %s" % (op.name, k, cls, g, e)
            n += 1
    assert n


def test_layout():
    """item i is the same set whatever n is; 257 items meet every set; the wave-layout ops give a wavefront one set"""
    for name, op in V.OPS.items():
        w257, i257, _, _ = V.call(name, 257)
        assert set(i257) == set(range(len(op.sets))), name
        for n in V.N_ITEMS[:-1]:
            w, idx, want, chk = V.call(name, n)
            assert idx == i257[:n] and w == w257[:len(w)] and len(w) == n * op.win and len(want) == len(chk) == n
        if op.wave:
            assert all(len(set(i257[64 * k:64 * k + 64])) == 1 for k in range(5))
    # zero next to non-zero values in the mixed inversions: lanes of one wavefront end at different batches
    _, idx, _, _ = V.call("fq_inv_var", 257)
    zero = [V.OPS["fq_inv_var"].sets[k][0] == "zero" for k in idx]
    assert any(zero[i] != zero[i + 1] for i in range(63)) and any(zero[i] != zero[i + 1] for i in range(64, 255))
    for name in ("fq_inv_uni", "fq_inv_var_uni"):
        assert any(V.from_words(w[12 * t:12 * t + 12]) % Q == 0 for _, w in V.OPS[name].sets for t in range(V.UNI))


def test_operand_classes_are_present():
    ops = V.OPS
    prod = lambda name: [V.two(w) for _, w in ops[name].sets]
    assert all(a < Q and b < Q for a, b in prod("fq_mul"))
    rel = prod("fq_mul_relaxed")
    for v in (0, 1, Q - 1, Q, Q + 1, 2 * Q - 1, 2 * Q, 3 * Q - 1, V.ONE, V.R * V.R % Q, V.ALL1, V.ALT_ODD, V.ALT_EVEN):
        assert any(a == v for a, _ in rel), hex(v)
    sq = [V.from_words(w) for _, w in ops["fq_sqr_relaxed"].sets]
    for v in (0, 1, Q - 1, Q, Q + 1, 2 * Q - 1, 2 * Q, 3 * Q - 1, V.ALT_EVEN):
        assert v in sq
    for k in range(12):
        assert any(a == 1 << (32 * k) for a, _ in rel) and any(a == 1 << (32 * k) for a, _ in prod("fq_mul"))
    sg = [V.from_words(w) for _, w in ops["fq_sgn"].sets]
    for c in (0, 1, (Q - 1) // 2, (Q + 1) // 2, Q - 1):
        assert c * V.R % Q in sg and c * V.R % Q + Q in sg
    gt = [V.from_words(w) for _, w in ops["gt_half_q_mask"].sets]
    for v in (Q // 2 - 1, Q // 2, Q // 2 + 1, 0, Q - 1):
        assert v in gt
    for k in range(12):                                   # differs from q // 2 in word k and in no other
        assert any(v != V.HALF and (v ^ V.HALF) >> (32 * k) << (32 * k) == v ^ V.HALF and (v ^ V.HALF) >> (32 * k + 32) == 0 for v in gt), k
    inv = [V.from_words(w) for _, w in ops["fq_inv"].sets]
    assert set(V.INV_CORNERS + V.INV_PATTERNS) <= set(inv)
    jac = [V.from_words(w) for _, w in ops["fq_jacobi_var"].sets]
    assert set(V.JACOBI_CORNERS) <= set(jac) and all(a < Q for a in jac)
    # fat_reduce: k q + d and k q - 1 for k over 0, 1, 2, powers of two and the largest below 2^396, three forms each
    red = {}
    for cls, w in ops["fat_reduce"].sets:
        red.setdefault(V.fat_value(V.fat_limbs(w)), set()).add(cls)
    kmax = (V.V_LIMIT - 1) // Q
    for k in [0, 1, 2, kmax] + [1 << i for i in range(2, 16)]:
        for v in (k * Q, k * Q + 1, k * Q + Q - 1, k * Q - 1):
            if 0 <= v < V.V_LIMIT:
                assert red[v] == {"tight", "ceil", "spread"}, (k, v - k * Q)
    # lin: 1 .. 30 micro-ops, coefficients 1 and 31, the three operands, MN = 0 / K / between, a negative sum of 255
    lin = [V.lin_unwords(w) for _, w in ops["lin"].sets]
    assert {k for _, k, _, _, _, _ in lin} == set(range(1, 31))
    assert any(mn == 0 for mn, *_ in lin) and any(mn == k for mn, k, *_ in lin) and any(0 < mn < k for mn, k, *_ in lin)
    assert any(set(c[:k]) == {1} for _, k, _, _, c, _ in lin) and any(set(c[:k]) == {31} for _, k, _, _, c, _ in lin)
    for v in (0, 2 * Q - 1, V.ALL1):
        assert any(v in o[:k] for _, k, _, _, _, o in lin)
    assert any(sum(c[:mn]) == 255 and set(o[:mn]) == {V.ALL1} for mn, _, _, _, c, o in lin)
    ab = [r for _, r in ops["lin_absorb"].sets]
    assert {r["levels"] for r in ab} == {0, 1, 2} and any(r["mn"] == 0 for r in ab) and any(r["mn"] == r["k"] for r in ab)


def test_operand_sets_lie_inside_their_preconditions():
    """(b)"""
    ops = V.OPS
    for _, w in ops["fq_mul_relaxed"].sets:
        a, b = V.two(w)
        assert a * b < 9 * Q * Q
    assert any(a * b >= 9 * Q * Q - a for a, b in (V.two(w) for _, w in ops["fq_mul_relaxed"].sets) if a)     # and reach the bound
    assert all(V.from_words(w) < 3 * Q for _, w in ops["fq_sqr_relaxed"].sets)
    for _, w in ops["fq_add_mod"].sets:
        a, s = V.two(w)
        assert a < Q and s <= Q
    assert all(V.from_words(w) <= Q for _, w in ops["fq_neg_raw"].sets)
    assert all(x < Q and y < Q for x, y in (V.two(w) for _, w in ops["fq_sub_mod"].sets))
    assert all(V.from_words(w) < 2 * Q for _, w in ops["fq_canon"].sets + ops["fq_sgn"].sets + ops["fq_inv"].sets)
    assert all(a < 1 << 40 for _, w in ops["fat_flip"].sets for a in V.fat_limbs(w))
    for _, w in ops["fat_mac_plain"].sets:
        assert all(a + w[36] * s < 1 << 64 for a, s in zip(V.fat_limbs(w[:24]), w[24:36]))
    for _, w in ops["fat_reduce"].sets:
        limbs = V.fat_limbs(w)
        assert all(a < V.FAT_LIMIT for a in limbs) and V.fat_value(limbs) < V.V_LIMIT
        _, e = V.estimate_k(limbs[11])
        assert abs(e - round(e)) > 1e-6           # a fused multiply-subtract on the device rounds to the same quotient
    assert any(max(V.fat_limbs(w)[:11]) >= V.FAT_LIMIT - (1 << 32) for c, w in ops["fat_reduce"].sets if c == "ceil")
    for _, w in ops["lin"].sets:
        mn, k, _, _, cfs, opr = V.lin_unwords(w)
        assert 1 <= k <= 30 and sum(cfs[:mn]) <= V.NEG_CF_MAX and all(0 <= c < 32 for c in cfs)
        acc = V.m_lin_share(mn, k, cfs, opr)                 # (asserts every limb below 2^40 at the flip)
        assert all(0 <= a < V.FAT_LIMIT for a in acc) and V.fat_value(acc) == V.lin_value(mn, k, cfs, opr) < V.V_LIMIT
        _, e = V.estimate_k(acc[11])
        assert abs(e - round(e)) > 1e-6
    top = 0
    for k, (_, r) in enumerate(ops["lin_absorb"].sets):
        assert len(r["lanes"]) == 64 and 1 <= r["k"] <= 30
        for f, cfs, opr in r["lanes"]:
            assert sum(cfs[:r["mn"]]) <= V.NEG_CF_MAX and len(cfs) == r["k"] and all(0 <= c < 32 for c in cfs)
        for nlive in (1, 63, 64):
            V.absorb_expected(k, nlive)                      # (asserts limbs below 2^44 and V below 2^396 in every lane)
        top = max(top, sum(sum(cfs[r["mn"]:]) for f, cfs, opr in r["lanes"][:4]))
    assert top == V.POS_GROUP_MAX                            # one group of four sits on the 2^44 bound


def test_constants_of_the_header():
    """the constants the references rebuild are the header's"""
    with open(os.path.join(CSRC, "fq32.h")) as f:
        hdr = f.read()
    for name, limbs, fmt in (("BLS_BIAS1_FAT", [b + 1 for b in V.BIAS_LIMBS], "0x%016xull"), ("BLS_QC_LIMBS", V.words12(V.QC), "0x%08xu"),
                             ("BLS_HALF_LIMBS", V.words12(V.HALF), "0x%08xu"), ("BLS_ONE_MONT_LIMBS", V.words12(V.ONE), "0x%08xu")):
        at = hdr.index("#define " + name)
        body = hdr[at:hdr.index("}", at)].replace("\\\n", " ")
        assert body.split("{")[1].replace(" ", "") == ",".join(fmt % x for x in limbs), name
    assert "HALF_Q_WORDS[12] = {" + ", ".join("0x%08xu" % x for x in V.words12(Q // 2)) in " ".join(hdr.split()).replace("{ ", "{")
    assert V.BIAS % Q == 0 and V.fat_value(V.BIAS_LIMBS) == V.BIAS and Q >> 352 == 436277738


# ---- (c) the emitted programs ------------------------------------------------------------------------------------------
def lin_groups(plan):
    """the lane shares of a plan, group by group (plan_lin_round lays out groups of four, then pairs, then single lanes,
    each aligned; bit 15 opens a group of four, bit 14 outside one a pair)"""
    groups, at = [], 0
    while at < len(plan):
        f = plan[at][1]
        g = 4 if f >> 15 & 1 else 2 if f >> 14 & 1 else 1
        assert at % g == 0 and at + g <= len(plan)
        groups.append(plan[at:at + g])
        at += g
    return groups


@pytest.fixture(scope="module")
def tables():
    return emit.build_tables()


def test_range_audit_of_the_emitted_lin_rounds(tables):
    """every LIN round of every packed segment: negative coefficients of a lane share sum to at most 255 (every limb
    below 2^40 at the flip for operand limbs up to 2^32 - 1); per group sum cf (2^32 - 1) + 4 (largest BIAS limb) < 2^44
    at the reduce; and V < 2^396 for operands below 2q"""
    rounds = worst_neg = worst_limb = worst_v = 0
    for name in tables["order"]:
        for rnd in tables["segs"][name].rounds:
            if rnd["kind"] != "lin":
                continue
            plan, mn, mp, lv = emit.plan_lin_round(rnd["lanes"])
            assert mn + mp <= V.LIN_MAXK
            rounds += 1
            for grp in lin_groups(plan):
                assert len(grp) <= 1 << lv
                tot = 0
                for d, flags, negs, poss in grp:
                    assert all(0 < cf < 32 for _, cf, _ in negs + poss)
                    nsum = sum(cf for _, cf, _ in negs)
                    assert nsum <= V.NEG_CF_MAX, (name, nsum)
                    worst_neg = max(worst_neg, nsum)
                    tot += nsum + sum(cf for _, cf, _ in poss)
                limb = tot * M32 + 4 * max(V.BIAS_LIMBS)
                assert limb < V.FAT_LIMIT, (name, tot)
                v = len(grp) * V.BIAS + sum(cf for d, f, n, p in grp for _, cf, _ in p) * (2 * Q - 1)
                assert v < V.V_LIMIT, (name, v.bit_length())
                worst_limb, worst_v = max(worst_limb, limb), max(worst_v, v)
    assert rounds > 100
    print("LIN rounds %d: largest negative sum %d, largest limb 2^%.2f, largest V 2^%.2f" % (
        rounds, worst_neg, __import__("math").log2(worst_limb), __import__("math").log2(worst_v)))


def test_emit_refuses_a_share_outside_the_bounds():
    """the same bounds are asserted where the tables are packed: a record of 30 micro-ops of coefficient 31 is refused"""
    ok = [(0, 0, [(1, 31, 5)] * 8 + [(1, 7, 5)], [(0, 31, 6)] * 21)]
    emit.check_lin_bounds(ok, 9)
    with pytest.raises(AssertionError):
        emit.check_lin_bounds([(0, 0, [(1, 31, 5)] * 8 + [(1, 8, 5)], [])], 9)                      # 256 at the flip
    with pytest.raises(AssertionError):
        emit.check_lin_bounds([(0, 3 << 14, [], [(0, 31, 6)] * 30)] + [(None, 0, [], [(0, 31, 6)] * 30)] * 3, 0)   # 2^44 at the reduce


# ---- the wait states of lin_absorb's DPP reads in the built check library --------------------------------------------------
SCAN_FIXTURE = """
0000000000001000 <k>:
	v_mov_b32_e32 v17, v21                                     // 000000001000: 7E220315
	v_and_b32_dpp v18, v20, v16 quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf bound_ctrl:1 // 000000001004: 00
	v_and_b32_dpp v19, v17, v16 quad_perm:[1,1,3,3] row_mask:0xf bank_mask:0xf bound_ctrl:1 // 00000000100C: 00
	v_mov_b32_e32 v22, v21                                     // 000000001014: 7E220315
	s_nop 1                                                    // 000000001018: BF800001
	v_and_b32_dpp v19, v22, v16 quad_perm:[2,2,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1 // 00000000101C: 00
"""


def test_dpp_reads_of_the_check_library_keep_their_wait_states():
    """The first device run of lin_absorb was wrong in a few words: the compiler had left register copies between the
    helper's asm blocks, one instruction ahead of a DPP read of the copied register, where the hazard recogniser does
    not look.  The check kernel now settles its accumulators ahead of the helper's s_nop 4; this reads the built code
    object and asserts that no DPP read follows a write of its source by fewer than two wait states.  (The same scan of
    libblsgpu.so -- tools/dpp_hazard_scan.py, about a minute -- found none in 21 470 DPP instructions.)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("dpp_hazard_scan", os.path.join(ROOT, "tools", "dpp_hazard_scan.py"))
    scan = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(scan)
    n, bad = scan.scan(SCAN_FIXTURE)
    assert n == 3 and [(b[1], b[2]) for b in bad] == [("v17", 1)]        # the scan sees what it is meant to see
    lib = os.path.join(CSRC, "libblsgpu_fq32check.so")
    assert os.path.exists(lib), "libblsgpu_fq32check.so is not built: run __graft_entry__.build()"
    n, bad = scan.scan_file(lib)
    assert n == 48 and not bad, bad
