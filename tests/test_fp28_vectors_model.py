"""CPU: the operand classes of tests/fp28_vectors.py against the integer model (vmgen.gen_fp28.model_dot, whose 64-bit
accumulator assertions every set has to pass), against plain Python integers and, for Fq2 and the curve, against
bls_py.hostmath; the column-sum bookkeeping; and the compile-time side of the safety argument: hipcc refuses a product
one unit past the column bound and accepts the widest forms the vectors use.  Needs no GPU; the compile-time tests are
skipped where hipcc is absent."""
import os
import shutil
import subprocess

import pytest

import fp28_vectors as V
from vmgen import gen_fp28 as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")


def _check_group(group):
    n = 0
    for op in V.OPS.values():
        if op.group != group:
            continue
        exp = V.expected(op.name)
        for (cls, w), e in zip(op.sets, exp):
            assert len(e) == op.wout and V.fits32(e), (op.name, cls)
            if op.check is not None:
                try:
                    op.check(w, e)
                except AssertionError as err:
                    raise AssertionError("%s, class %s: %s" % (op.name, cls, err))
            n += 1
    assert n


def test_counts():
    """the counts the module's docstring states are the ones it computes; every op has every class that applies"""
    assert V.counts_table() in V.__doc__, "\n" + V.counts_table()
    for name, c in V.COUNTS_PER_OP.items():
        op = V.OPS[name]
        assert sum(c.values()) == len(op.sets) <= V.MAX_SETS
        if op.group in ("raw", "typed"):
            assert c["random"] and c["edge"] and c["reduce"] and c["range"], name
        elif op.group == "curve":
            assert c["curve"], name
            # the non-canonical coordinate forms: the limbs of q, -q + 1 and 2q - 1 for 0, 1 and q - 1
            for v in (V.Q, -V.Q + 1, 2 * V.Q - 1):
                assert V.has_limbs(op, v), (name, v)
        else:
            assert c["random"] and c["edge"], name
            if name in ("f2_mul", "f2_mul_w", "f2_sqr", "f2_sqr_w", "f2_dot2", "f2_dot2_w"):
                assert c["reduce"] and c["range"], name
            if op.group == "linear" and name not in ("lin_canon", "lin_is_zero"):      # these two take fe values only
                assert c["range"], name


def test_item_layout():
    """item i is the same set whatever n is, every set is met within 257 items, and on lanes that vary"""
    for nsets in (1, 2, 29, 64, 72, 257):
        idx = [V.item_set(i, nsets) for i in range(257)]
        assert set(idx) == set(range(nsets))
        if 1 < nsets <= 64:
            for s in range(nsets):
                assert len({i % 64 for i, k in enumerate(idx) if k == s}) > 1
    w65, i65 = V.call_words("raw_dot1", 65)
    w257, i257 = V.call_words("raw_dot1", 257)
    assert i257[:65] == i65 and w257[:len(w65)] == w65


def test_raw_products_model_and_integers():
    _check_group("raw")


def test_typed_products_model_and_integers():
    _check_group("typed")


def test_linear_and_carry_ops_are_exact():
    _check_group("linear")
    # the promised digit form, spelled out once: norm keeps the value and leaves digits 0..12 in [0, 2^28)
    x = [V.digit(7, j % 2 == 0) for j in range(13)] + [-V.TOP]
    r = V.l_norm(x)
    assert G.from_limbs(r) == G.from_limbs(x) and all(0 <= d <= V.MASK for d in r[:13])
    assert V.l_is_zero(G.to_limbs(0)) == 1 and V.l_is_zero(G.to_limbs(V.Q)) == 1
    assert all(V.l_is_zero(G.to_limbs(v)) == 0 for v in (1, -1, V.Q - 1, V.Q + 1, 2 * V.Q - 1, -V.Q + 1))


def test_boundaries():
    _check_group("boundary")
    # round trips: pack32(unpack32(x)) = x, to_raw(from_raw(c)) = c mod q, to_vm(from_vm(x)) = x mod q
    for (_, w), e in zip(V.OPS["b_unpack32"].sets, V.expected("b_unpack32")):
        assert V.OPS["b_pack32"].ref(e) == w
    for frm, to in (("b_from_raw", "b_to_raw"), ("b_from_vm", "b_to_vm")):
        for (_, w), e in zip(V.OPS[frm].sets, V.expected(frm)):
            assert V.from_words(V.OPS[to].ref(e)) == V.from_words(w) % V.Q


def test_fq2_against_hostmath():
    _check_group("fq2")


def test_curve_model_against_hostmath():
    """the limb model of padd / pmadd / pdbl / pneg (every product through model_dot, so no column of any of them leaves
    64 bits on these inputs) gives hostmath's point: doubling inside an addition, P + (-P), infinity, small order"""
    _check_group("curve")
    for g in ("g1", "g2"):
        M = V.M1 if g == "g1" else V.M2
        PW = 3 * M.DW
        for (_, w) in V.OPS[g + "_padd"].sets:           # P + P through padd and pmadd is pdbl's point
            P, Qp = V.pt_unflat(M, w[:PW]), V.pt_unflat(M, w[PW:])
            if V.affine_of(M, P) == V.affine_of(M, Qp):
                assert V.affine_of(M, V.m_padd(M, P, Qp)) == V.affine_of(M, V.m_pdbl(M, P))


def test_reduction_extremes():
    """(q, 1): every quotient digit is 0xFFFFFFF and the result is the digits of q; (R mod q, x) gives x; (0, x) gives 0"""
    q, one = G.to_limbs(V.Q), G.to_limbs(1)
    assert G.model_dot([(q, one)]) == q
    x = 0x1234567 * V.Q // 0x2000001
    assert G.from_limbs(G.model_dot([(G.to_limbs(V.ONE), G.to_limbs(x))])) % V.Q == x
    assert G.model_dot([(G.to_limbs(0), G.to_limbs(x))]) == [0] * 14
    for name in ("raw_dot1", "raw_dot4", "raw_dot6", "t_dot2", "f2_mul"):
        assert any(cls == "reduce" and G.to_limbs(V.Q) == e[:14] for (cls, _), e in zip(V.OPS[name].sets, V.expected(name))), name


def test_column_units_bookkeeping():
    """column_units is fp28.h's Term arithmetic; the range sets reach 8 units (9 on the negative side) and no more"""
    top = V.MASK
    assert V.column_units([([top] * 13 + [0], [top] * 13 + [0])]) == (1, 0)
    assert V.column_units([([-(8 << 28)] * 13 + [0], [top] * 13 + [0])]) == (0, 8)
    assert V.column_units([([V.digit(2, True)] * 13 + [0], [V.digit(2, False)] * 13 + [0])] * 2) == (0, 8)
    assert V.column_units([([V.SQRT8] * 13 + [0],) * 2]) == (8, 0) and (V.SQRT8 + 1) ** 2 > 8 << 56
    full = {"raw_dot1": 9, "raw_dot2": 8, "raw_dot3": 8, "raw_dot4": 8, "raw_dot6": 8, "raw_sqr1": 8, "raw_sqr2": 8,
            "t_mul_8x1": 8, "t_mul_4x2": 8, "t_mul_2x4": 8, "t_mul_neg9": 9, "t_sqr_2": 4, "t_dot2_2222": 8, "t_dot2_4122": 8, "t_dot4_21": 8}
    for name, want in full.items():
        op = V.OPS[name]
        nops = op.win // 14
        tt = V.sqr_terms if nops % 2 else V.dot_terms
        units = [V.column_units(tt(V.split(w, nops))) for cls, w in op.sets if cls == "range"]
        assert max(max(u) for u in units) == want and all(u[0] <= 8 and u[1] <= 9 for u in units), (name, units)
    # one unit more trips the model's own assertion: the bound is tight, not merely sufficient
    over = [V.digit(8, False)] * 14
    with pytest.raises(AssertionError):
        G.model_dot([(over, over)] * 2)


SNIPPET = """#include <hip/hip_runtime.h>
#include "fp28.h"
using namespace blsgpu::r28;
template <int A, int B> __device__ F<A, B> ld(const int32_t* p) { F<A, B> r; for (int j = 0; j < NL; j++) r.v[j] = p[j]; return r; }
template <int A, int B> __device__ F2<A, B> ld2(const int32_t* p) { return {ld<A, B>(p), ld<A, B>(p + NL)}; }
__global__ void k(const int32_t* in, int32_t* out) {
%s}
"""
BLOCK = "    { const fe r = %s; for (int j = 0; j < NL; j++) out[%d + j] = r.v[j]; }\n"
FITS = {
    "mul_8x1": "mul(ld<8, 8>(in), ld<1, 1>(in + 14))",
    "mul_4x2": "mul(ld<4, 4>(in), ld<2, 2>(in + 14))",
    "mul_neg9": "mul(ld<3, 0>(in), ld<0, 3>(in + 14))",
    "sqr_2": "sqr(ld<2, 2>(in))",
    "dot2_2222": "dot2(ld<2, 2>(in), ld<2, 2>(in + 14), ld<2, 2>(in + 28), ld<2, 2>(in + 42))",
    "dot4_21": "dot4(ld<2, 2>(in), ld<1, 1>(in + 14), ld<2, 2>(in + 28), ld<1, 1>(in + 42), ld<2, 2>(in + 56), ld<1, 1>(in + 70), ld<2, 2>(in + 84), ld<1, 1>(in + 98))",
    "f2_mul_22": "mul(ld2<2, 2>(in), ld2<2, 2>(in + 28)).a",
    "f2_sqr_02": "sqr(ld2<0, 2>(in)).a",
    "f2_dot2_padd": "dot2(ld2<2, 1>(in), ld2<1, 1>(in + 28), ld2<1, 2>(in + 56), ld2<0, 1>(in + 84)).b",
    "norm_7": "norm(ld<7, 7>(in))",
    "neg_7": "norm(neg(ld<7, 7>(in)))",
}
COLUMN = "a column of this sum of products may overflow 64 bits"
REFUSED = {
    "mul_8x2": ("mul(ld<8, 8>(in), ld<2, 2>(in + 14))", COLUMN),
    "mul_3x3": ("mul(ld<3, 3>(in), ld<3, 3>(in + 14))", COLUMN),
    "mul_neg10": ("mul(ld<5, 0>(in), ld<0, 2>(in + 14))", COLUMN),
    "sqr_3": ("sqr(ld<3, 3>(in))", COLUMN),
    "dot4_sum9": ("dot4(ld<2, 2>(in), ld<1, 1>(in + 14), ld<2, 2>(in + 28), ld<1, 1>(in + 42), ld<2, 2>(in + 56), ld<1, 1>(in + 70), ld<3, 3>(in + 84), ld<1, 1>(in + 98))", COLUMN),
    "f2_mul_32": ("mul(ld2<3, 3>(in), ld2<2, 2>(in + 28)).a", COLUMN),
    "f2_sqr_12": ("sqr(ld2<1, 2>(in)).a", COLUMN),
    "f2_dot2_padd_wider": ("dot2(ld2<2, 1>(in), ld2<1, 2>(in + 28), ld2<1, 2>(in + 56), ld2<0, 1>(in + 84)).b", COLUMN),
    "norm_8": ("norm(ld<8, 8>(in))", "plus the carry leaves int32"),
    "neg_8": ("mulc_norm<3>(neg(ld<8, 1>(in)))", "the negative of -2^31 leaves int32"),
}


def _syntax_only(tmp_path, name, exprs):
    src = os.path.join(tmp_path, name + ".hip")
    with open(src, "w") as f:
        f.write(SNIPPET % "".join(BLOCK % (e, 14 * n) for n, e in enumerate(exprs)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", CSRC, src],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


needs_hipcc = pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="no hipcc")


@needs_hipcc
def test_widest_admitted_forms_compile(tmp_path):
    r = _syntax_only(tmp_path, "fits", list(FITS.values()))
    assert r.returncode == 0, r.stdout[-3000:]


@needs_hipcc
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_one_unit_past_the_bound_is_refused(tmp_path, name):
    expr, message = REFUSED[name]
    r = _syntax_only(tmp_path, name, [expr])
    assert r.returncode != 0, "compiled: " + expr
    assert "static assertion failed" in r.stdout and message in r.stdout, r.stdout[-3000:]
