"""Operand sets and CPU references for the 28-bit-limb field layer (csrc/fp28.h, csrc/fp28_mul_gfx950.h), one list per
op of the test-only device library csrc/blsgpu_fp28_check.hip.  Pure Python: tests/test_fp28_vectors_model.py checks the
references against each other on the CPU, tests/test_gpu_fp28.py compares the compiled kernels with them limb for limb.

References, none shared with the device code:
  * products: vmgen.gen_fp28.model_dot (the column arithmetic with the 64-bit accumulator range asserted) gives the
    expected limbs; check_product() checks a result in plain Python integers, independently of the model:
    value = sum a_t b_t / R (mod q), digits 0..12 in [0, 2^28), and -q < value < 2q where the operands are `fe` values;
  * linear and carry ops: the exact integer value, and the one digit form the header promises;
  * Fq2 and the curve: a limb model that transcribes fp28.h's formulas over model_dot gives the expected limbs, and
    bls_py.hostmath (Jacobian, plain residues) the value: points are compared after both sides are made affine.

Operand classes (CLASSES), as the issue names them:
  1 random   seeded random values in (-q, 2q), digits as to_limbs writes them
  2 edge     0, +-1, q - 1, q, q + 1, 2q - 1, -q + 1, R mod q, R^2 mod q; digits 0..12 all 2^28 - 1; one nonzero digit
             at each of the 14 positions; alternating 0 / 2^28 - 1
  3 reduce   (q, 1): every m_k = 0xFFFFFFF and the result is the digits of q; (0, x); (R mod q, x) -> x;
             (q - 1, q - 1); (2q - 1, 2q - 1); (-q + 1, 2q - 1) -- alone (other terms zero) and in every term
  4 range    digits 0..12 at HI 2^28 - 1 or -LO 2^28 so that the column sum S is the largest ColumnsFit admits (8 units
             of 2^56; 9 on the negative side), in three sign patterns (products positive / negative / alternating by
             limb) times three top digits (0, +-(2^23 - 1)); S is asserted for every set (column_units)
  5 curve    random P + Q, P + P, P + (-P), infinity on either side and both, points off the r-torsion subgroup and of
             small order (tests/golden/subgroup.json, pairing_degenerate.json), non-canonical coordinates (q, -q + 1,
             2q - 1 for 0, 1, q - 1), and a chain of eight additions with nothing canonical in between

Two places where the sets differ from the issue's table, both forced by the arithmetic:
  * a lone square of magnitude 2 x 2 has S = 4, not 8, and 3 x 3 = 9 does not compile: sqr1 gets the 2 x 2 sets (the
    widest typed square) AND raw sets at limb magnitude floor(sqrt(8) 2^28), S = 8;
  * norm, neg and conj run at F<7, 7>: at F<8, 8> the carry added to a limb at 2^31 - 1 (norm) and the negative of
    -2^31 (neg, conj) leave int32.  No kernel instantiates them there; fp28.h now refuses to compile it.

Vectors per class and op (COUNTS, computed at import and asserted in tests/test_fp28_vectors_model.py::test_counts):
  group    ops  random  edge  reduce  range  curve
  raw        7     112   196      84    102      0
  linear    10     160   326       0     72      0
  typed     12     192   336     144     78      0
  boundary   7      84   117       0      0      0
  fq2       12     144   337      48    120      0
  curve     14       0     0       0      0   1134
"""
import json
import os
import random
from math import isqrt

from vmgen import gen_fp28 as G
from bls_py import hostmath as H

Q, R, L, W, MASK = G.Q, G.R, G.L, G.W, G.MASK
RINV = pow(R, -1, Q)
ONE = R % Q                                            # the Montgomery form of 1
TOP = (1 << 23) - 1                                    # the header's limit on a signed top digit
N_ITEMS = (1, 63, 64, 65, 257)                         # items per call: one lane, either side of a wavefront, two workgroups
MAX_SETS = 257
STRIDE = 37                                            # coprime to 64 and to 257
CLASSES = ("random", "edge", "reduce", "range", "curve")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

to_limbs, from_limbs = G.to_limbs, G.from_limbs


def s32(w):
    """a 32-bit word as the signed integer that travels"""
    w &= 0xFFFFFFFF
    return w - (1 << 32) if w >> 31 else w


def words12(x):
    assert 0 <= x < 1 << 384
    return [s32(x >> (32 * i)) for i in range(12)]


def from_words(ws):
    return sum((w & 0xFFFFFFFF) << (32 * i) for i, w in enumerate(ws))


def item_set(i, nsets):
    """the operand set of item i, whatever the number of items: 37 i mod 257 walks all of 0..256, so every set of an
    op (at most 257) is met within 257 items, each on lanes that differ from call to call"""
    return ((i * STRIDE) % MAX_SETS) % nsets


# ---- values -----------------------------------------------------------------------------------------------------
def edge_values():
    vals = [0, 1, -1, Q - 1, Q, Q + 1, 2 * Q - 1, -Q + 1, R % Q, R * R % Q]
    out = [to_limbs(v) for v in vals]
    out.append([MASK] * 13 + [0])
    for j in range(L):
        out.append([(MASK if i == j else 0) for i in range(L)] if j < 13 else [0] * 13 + [1 << 16])
    out.append([(MASK if i % 2 else 0) for i in range(13)] + [0])
    out.append([(0 if i % 2 else MASK) for i in range(13)] + [0])
    return out


EDGE = edge_values()
NE = len(EDGE)                                         # 27
NR = 16                                                # random sets per op
REDUCE = [(Q, 1), (0, None), (R % Q, None), (Q - 1, Q - 1), (2 * Q - 1, 2 * Q - 1), (-Q + 1, 2 * Q - 1)]


def rnd_fe(rnd):
    return to_limbs(rnd.randrange(-Q + 1, 2 * Q))


def column_units(terms):
    """(pos, neg): the most a column of sum_t a_t b_t can hold on either side, in units of 2^56, from digits 0..12 --
    what fp28.h's Term / ColumnsFit compute from the types"""
    pos = neg = 0
    for a, b in terms:
        ah, al, bh, bl = max(max(a[:13]), 0), max(-min(a[:13]), 0), max(max(b[:13]), 0), max(-min(b[:13]), 0)
        pos += max(ah * bh, al * bl)
        neg += max(ah * bl, al * bh)
    u = 1 << 56
    return (-(-pos // u), -(-neg // u))


dot = G.model_dot


def check_product(terms, r, bounded):
    """a product's result in Python integers, independently of model_dot"""
    want = sum(from_limbs(a) * from_limbs(b) for a, b in terms)
    v = from_limbs(r)
    assert (v - want * RINV) % Q == 0, "not the Montgomery sum of products"
    assert all(0 <= d <= MASK for d in r[:13]), "digits 0..12 leave [0, 2^28)"
    assert -(1 << 31) <= r[13] < (1 << 31)
    if bounded:
        assert -Q < v < 2 * Q, "value leaves (-q, 2q)"


def digit(m, positive):
    """the end of a limb range of magnitude m units of 2^28"""
    return (m << W) - 1 if positive else -(m << W)


SQRT8 = isqrt(8 << 56)                                 # limb magnitude whose square is 8 units of 2^56


def range_sets(mags, patterns=("pos", "neg", "alt"), tops=(0, TOP, -TOP), raw_mag=None):
    """mags: per term (ma, mb) in units of 2^28.  pos: even terms (+, +), odd terms (-, -); neg: (+, -) and (-, +);
    alt: a alternates by limb, b positive"""
    out = []
    for pat in patterns:
        for top in tops:
            terms = []
            for t, (ma, mb) in enumerate(mags):
                def dg(m, p):
                    return (raw_mag if p else -raw_mag) if raw_mag else digit(m, p)
                if pat == "pos":
                    sa = sb = (t % 2 == 0)
                    a, b = [dg(ma, sa)] * 13, [dg(mb, sb)] * 13
                elif pat == "neg":
                    sa = (t % 2 == 0)
                    a, b = [dg(ma, sa)] * 13, [dg(mb, not sa)] * 13
                else:
                    a, b = [dg(ma, j % 2 == 0) for j in range(13)], [dg(mb, True)] * 13
                terms.append((a + [top], b + [top]))
            out.append(terms)
    return out


# ---- the limb model of fp28.h's Fq2 and curve formulas ------------------------------------------------------------------
def l_add(x, y): return [a + b for a, b in zip(x, y)]
def l_sub(x, y): return [a - b for a, b in zip(x, y)]
def l_neg(x): return [-a for a in x]
def l_mulc(c, x): return [c * a for a in x]
def l_norm(x): return to_limbs(from_limbs(x))
def l_mulc_norm(c, x): return to_limbs(c * from_limbs(x))


def l_canon(x):
    v = from_limbs(x)
    assert -Q < v < 2 * Q
    return to_limbs(v % Q)


def l_is_zero(x):
    return 1 if from_limbs(x) in (0, Q) and all(0 <= d <= MASK for d in x[:13]) else 0


def fits32(x):
    return all(-(1 << 31) <= d < (1 << 31) for d in x)


class M1:
    """F<LO, HI> on limb lists"""
    zero, one, DW = [0] * L, to_limbs(ONE), L
    add, sub, neg = staticmethod(l_add), staticmethod(l_sub), staticmethod(l_neg)
    mulc, norm, mulc_norm = staticmethod(l_mulc), staticmethod(l_norm), staticmethod(l_mulc_norm)
    mul = staticmethod(lambda x, y: dot([(x, y)]))
    sqr = staticmethod(lambda x: dot([(x, x)]))
    dot2 = staticmethod(lambda a, b, c, d: dot([(a, b), (c, d)]))
    b3 = staticmethod(lambda x: l_mulc_norm(12, x))
    tight = staticmethod(lambda x: x)
    flat = staticmethod(lambda x: list(x))
    unflat = staticmethod(lambda w: list(w))


class M2:
    """F2<LO, HI> as pairs of limb lists: f2_mul_call, f2_sqr_call, f2_dot2_call of fp28.h"""
    zero, one, DW = ([0] * L, [0] * L), (to_limbs(ONE), [0] * L), 2 * L
    add = staticmethod(lambda x, y: (l_add(x[0], y[0]), l_add(x[1], y[1])))
    sub = staticmethod(lambda x, y: (l_sub(x[0], y[0]), l_sub(x[1], y[1])))
    neg = staticmethod(lambda x: (l_neg(x[0]), l_neg(x[1])))
    mulc = staticmethod(lambda c, x: (l_mulc(c, x[0]), l_mulc(c, x[1])))
    norm = staticmethod(lambda x: (l_norm(x[0]), l_norm(x[1])))
    mulc_norm = staticmethod(lambda c, x: (l_mulc_norm(c, x[0]), l_mulc_norm(c, x[1])))
    conj = staticmethod(lambda x: (list(x[0]), l_neg(x[1])))
    mul_xi = staticmethod(lambda x: (l_sub(x[0], x[1]), l_add(x[0], x[1])))
    # the sums of products behind the real and the imaginary part (what column_units is asked about)
    mul_terms = staticmethod(lambda x, y: ([(x[0], y[0]), (l_neg(x[1]), y[1])], [(x[0], y[1]), (x[1], y[0])]))
    sqr_terms = staticmethod(lambda x: ([(l_add(x[0], x[1]), l_sub(x[0], x[1]))], [(l_mulc(2, x[0]), x[1])]))
    dot2_terms = staticmethod(lambda x, y, z, w: ([(x[0], y[0]), (l_neg(x[1]), y[1]), (z[0], w[0]), (l_neg(z[1]), w[1])],
                                                  [(x[0], y[1]), (x[1], y[0]), (z[0], w[1]), (z[1], w[0])]))
    mul = staticmethod(lambda x, y: tuple(dot(t) for t in M2.mul_terms(x, y)))
    sqr = staticmethod(lambda x: tuple(dot(t) for t in M2.sqr_terms(x)))
    dot2 = staticmethod(lambda x, y, z, w: tuple(dot(t) for t in M2.dot2_terms(x, y, z, w)))
    b3 = staticmethod(lambda x: M2.mulc_norm(12, M2.mul_xi(x)))
    tight = staticmethod(lambda x: M2.norm(x))
    flat = staticmethod(lambda x: list(x[0]) + list(x[1]))
    unflat = staticmethod(lambda w: (list(w[:L]), list(w[L:2 * L])))


def m_padd(M, P, Qp):
    (X1, Y1, Z1), (X2, Y2, Z2) = P, Qp
    t0, t1, t2 = M.mul(X1, X2), M.mul(Y1, Y2), M.mul(Z1, Z2)
    t3 = M.sub(M.sub(M.mul(M.add(X1, Y1), M.add(X2, Y2)), t0), t1)
    t4 = M.sub(M.sub(M.mul(M.add(Y1, Z1), M.add(Y2, Z2)), t1), t2)
    t5 = M.sub(M.sub(M.mul(M.add(X1, Z1), M.add(X2, Z2)), t0), t2)
    x3, bz = M.mulc_norm(3, t0), M.b3(t2)
    z3, t1m, y3 = M.tight(M.add(t1, bz)), M.sub(t1, bz), M.b3(t5)
    return (M.dot2(t3, t1m, M.neg(t4), y3), M.dot2(t1m, z3, y3, x3), M.dot2(z3, M.tight(t4), x3, M.tight(t3)))


def m_pmadd(M, P, x2, y2):
    X, Y, Z = P
    t0, t1 = M.mul(X, x2), M.mul(Y, y2)
    t3 = M.sub(M.sub(M.mul(M.add(x2, y2), M.add(X, Y)), t0), t1)
    t4 = M.add(M.mul(y2, Z), Y)
    y3 = M.b3(M.add(M.mul(x2, Z), X))
    x3, bz = M.mulc_norm(3, t0), M.b3(Z)
    z3, t1m = M.tight(M.add(t1, bz)), M.sub(t1, bz)
    return (M.dot2(t3, t1m, M.neg(t4), y3), M.dot2(y3, x3, t1m, z3), M.dot2(z3, t4, x3, t3))


def m_pdbl(M, P):
    X, Y, Z = P
    t0, t1, t2, txy = M.sqr(Y), M.mul(Y, Z), M.b3(M.sqr(Z)), M.mul(X, Y)
    z8 = M.mulc_norm(8, t0)
    d = M.tight(M.sub(t0, M.mulc(3, t2)))
    return (M.mul(d, M.add(txy, txy)), M.dot2(t2, z8, d, M.add(t0, t2)), M.mul(t1, z8))


def m_pneg(M, P):
    return (P[0], M.norm(M.neg(P[1])), P[2])


def pt_flat(M, P):
    return M.flat(P[0]) + M.flat(P[1]) + M.flat(P[2])


def pt_unflat(M, w):
    return tuple(M.unflat(w[k * M.DW:(k + 1) * M.DW]) for k in range(3))


# ---- values behind the limbs: residues, points as hostmath sees them ---------------------------------------------------
def res(x):
    """limbs of x R -> x mod q"""
    return from_limbs(x) * RINV % Q


def el_res(M, e):
    return res(e) if M is M1 else (res(e[0]), res(e[1]))


def mont(M, v, rep=0):
    """a residue (or pair) -> Montgomery limbs; rep picks the representative: 0 canonical, 1 the other one in (-q, 2q)"""
    def one(x):
        m = x * R % Q
        if rep:
            m = m + Q if rep == 1 else (m - Q if m else Q)
        return to_limbs(m)
    return one(v) if M is M1 else (one(v[0]), one(v[1]))


def HF(M):
    return H.F1 if M is M1 else H.F2


def affine_of(M, P):
    """a device point (X : Y : Z), x = X / Z, as hostmath's affine pair, None at infinity (Z = 0 mod q)"""
    F = HF(M)
    X, Y, Z = (el_res(M, c) for c in P)
    if F.is_zero(Z):
        return None
    zi = F.inv(Z)
    return (F.mul(X, zi), F.mul(Y, zi))


def proj(M, A, lam=None, rep=0):
    """hostmath affine pair (None: infinity) -> device limbs (x lam : y lam : lam)"""
    F = HF(M)
    lam = F.one if lam is None else lam
    if A is None:
        return (mont(M, F.zero, rep), mont(M, lam, rep), mont(M, F.zero, rep))
    return (mont(M, F.mul(A[0], lam), rep), mont(M, F.mul(A[1], lam), rep), mont(M, lam, rep))


NONCANON = {0: Q, 1: -Q + 1, Q - 1: 2 * Q - 1}             # a residue -> the value whose limbs stand for it in the curve sets


def M1_nc(v):
    return to_limbs(NONCANON.get(v * R % Q, v * R % Q))


def has_limbs(op, value):
    """does some curve set of the op hold a coordinate (or Fq2 part) with exactly the limbs of value"""
    want = to_limbs(value)
    return any(w[k:k + L] == want for _, w in op.sets for k in range(0, len(w), L))


def host_add(M, A, B):
    F = HF(M)
    return H.jac_to_affine(F, H.jac_add(F, H.aff_to_jac(F, A), H.aff_to_jac(F, B)))


def host_neg(M, A):
    return None if A is None else (A[0], HF(M).neg(A[1]))


# ---- the op table -----------------------------------------------------------------------------------------------------
class Op:
    def __init__(self, name, code, group, win, wout, ref, check=None):
        self.name, self.code, self.group, self.win, self.wout, self.ref, self.check = name, code, group, win, wout, ref, check
        self.sets = []                                 # (class, input words)

    def add(self, cls, words):
        words = [int(w) for w in words]
        assert len(words) == self.win and fits32(words), (self.name, cls, len(words))
        self.sets.append((cls, words))


OPS = {}


def defop(*a, **k):
    op = Op(*a, **k)
    OPS[op.name] = op
    return op


def split(words, n):
    return [list(words[k * L:(k + 1) * L]) for k in range(n)]


def flat(lists):
    return [d for x in lists for d in x]


def terms_of(ops):
    return [(ops[2 * t], ops[2 * t + 1]) for t in range(len(ops) // 2)]


def _seed(name):
    return random.Random("fp28:" + name)


# raw and typed products: (name, code, terms builder, K operands, range configs)
def product_op(name, code, group, nops, to_terms):
    def ref(w):
        return dot(to_terms(split(w, nops)))

    def check(w, out):
        terms = to_terms(split(w, nops))
        bounded = all(abs(d) <= MASK for x in split(w, nops) for d in x[:13]) and all(-(1 << 17) <= x[13] < (1 << 18) for x in split(w, nops)) \
            and len(terms) <= 8 and all(-Q < from_limbs(x) < 2 * Q for x in split(w, nops))
        check_product(terms, out, bounded)
    return defop(name, code, group, nops * L, L, ref, check)


def reduce_sets(nops, rnd):
    """class 3 operand lists: each pair of REDUCE alone (every other term is (0, x)) and in every term; an op that
    squares its first operand (an odd number of operands) takes the pair's first value there"""
    square, nterms, out = nops % 2, (nops + 1) // 2, []
    for a, b in REDUCE:
        for every in (False, True):
            ops = []
            for t in range(nterms):
                if t == 0 or every:
                    pair = [rnd_fe(rnd) if v is None else to_limbs(v) for v in (a, b)]
                else:
                    pair = [[0] * L, rnd_fe(rnd)]
                ops += pair[:1] if square and t == 0 else pair
            out.append(ops)
    return out


def fill_product(op, nops, to_terms, ranges, want_units, classes=("random", "edge", "reduce")):
    rnd = _seed(op.name)
    if "random" in classes:
        for _ in range(NR):
            op.add("random", flat(rnd_fe(rnd) for _ in range(nops)))
    if "edge" in classes:
        for j in range(NE + 1):
            op.add("edge", flat(EDGE[(j + 5 * m) % NE] if j < NE else EDGE[(7 * m) % NE] for m in range(nops)))
    if "reduce" in classes:
        for ops in reduce_sets(nops, rnd):
            op.add("reduce", flat(ops))
    for terms in ranges:
        ops = []
        for a, b in terms:
            ops += [a, b]
        if nops % 2:                                    # square: the first term is (a, a)
            ops = [terms[0][0]] + ops[2:]
        got = column_units(to_terms(ops))
        # (a square cannot be negative: with its partner term negative the units split between the two sides)
        assert max(got) == want_units or (nops % 2 and sum(got) == want_units), (op.name, got, want_units)
        assert max(got) <= 9 and got[0] <= 8
        op.add("range", flat(ops))


def dot_terms(ops):
    return terms_of(ops)


def sqr_terms(ops):
    return [(ops[0], ops[0])] + terms_of(ops[1:])


RAW_MAGS = {
    "raw_dot1": [[(8, 1)], [(4, 2)], [(2, 4)]],
    "raw_dot2": [[(2, 2), (2, 2)], [(4, 1), (2, 2)]],
    "raw_dot3": [[(2, 2), (2, 1), (2, 1)]],
    "raw_dot4": [[(2, 1)] * 4],
    "raw_dot6": [[(1, 1), (1, 1), (1, 1), (2, 1), (1, 1), (2, 1)]],
    "raw_sqr2": [[(2, 2), (2, 2)]],
}


def build_products():
    for k, (name, code) in enumerate((("raw_dot1", 0), ("raw_dot2", 1), ("raw_dot3", 2), ("raw_dot4", 3), ("raw_dot6", 4))):
        K = (1, 2, 3, 4, 6)[k]
        op = product_op(name, code, "raw", 2 * K, dot_terms)
        fill_product(op, 2 * K, dot_terms, [s for mags in RAW_MAGS[name] for s in range_sets(mags)], 8)
    op = product_op("raw_sqr1", 5, "raw", 1, sqr_terms)
    fill_product(op, 1, sqr_terms, range_sets([(2, 2)]), 4)                            # the widest typed square
    fill_product(op, 1, sqr_terms, range_sets([(0, 0)], raw_mag=SQRT8), 8, classes=())   # and the full column, raw
    op = product_op("raw_sqr2", 6, "raw", 3, sqr_terms)
    fill_product(op, 3, sqr_terms, [s for mags in RAW_MAGS["raw_sqr2"] for s in range_sets(mags)], 8)
    # neg 9: the negative side admits one more unit (no m q part on that side): 3 x 3, all products negative
    neg9 = [[([digit(3, False)] * 13 + [top], [digit(3, True)] * 13 + [top])] for top in (0, TOP, -TOP)]
    fill_product(OPS["raw_dot1"], 2, dot_terms, neg9, 9, classes=())

    typed = (("t_mul", 20, 2, dot_terms, None), ("t_mul_8x1", 21, 2, dot_terms, [(8, 1)]), ("t_mul_4x2", 22, 2, dot_terms, [(4, 2)]),
             ("t_mul_2x4", 23, 2, dot_terms, [(2, 4)]), ("t_mul_neg9", 24, 2, dot_terms, "neg9"), ("t_sqr", 25, 1, sqr_terms, None),
             ("t_sqr_2", 26, 1, sqr_terms, [(2, 2)]), ("t_dot2", 27, 4, dot_terms, None), ("t_dot2_2222", 28, 4, dot_terms, [(2, 2), (2, 2)]),
             ("t_dot2_4122", 29, 4, dot_terms, [(4, 1), (2, 2)]), ("t_dot4", 30, 8, dot_terms, None), ("t_dot4_21", 31, 8, dot_terms, [(2, 1)] * 4))
    for name, code, nops, tt, mags in typed:
        op = product_op(name, code, "typed", nops, tt)
        if mags == "neg9":
            fill_product(op, nops, tt, neg9, 9)
        elif mags is None:
            # F<0, 1> operands: digits in [0, 2^28), so the only end is 2^28 - 1; top digits as everywhere
            fe_ends = [[([MASK] * 13 + [top], [MASK] * 13 + [top])] * (max(nops, 2) // 2) for top in (0, TOP, -TOP)]
            fill_product(op, nops, tt, fe_ends, max(nops, 2) // 2)
        else:
            fill_product(op, nops, tt, range_sets(mags), 4 if name == "t_sqr_2" else 8)


# ---- linear / carry -----------------------------------------------------------------------------------------------------
def lin_values(op, nops, mag, rnd, with_range=True):
    """class 1 / 2 / 4 sets for a linear op whose operands are F<mag, mag>"""
    for _ in range(NR):
        op.add("random", flat([rnd.randrange(-(mag << W), mag << W) for _ in range(13)] + [rnd.randrange(-TOP, TOP + 1)] if mag > 1 else rnd_fe(rnd)
                              for _ in range(nops)))
    for j in range(NE):
        op.add("edge", flat(EDGE[(j + 5 * m) % NE] for m in range(nops)))
    if with_range:
        for pat in ("pos", "neg", "alt"):
            for top in (0, TOP, -TOP):
                ops = []
                for m in range(nops):
                    if pat == "pos":
                        x = [digit(mag, True)] * 13
                    elif pat == "neg":
                        x = [digit(mag, m % 2 == 1)] * 13 if nops > 1 else [digit(mag, False)] * 13
                    else:
                        x = [digit(mag, (j + m) % 2 == 0) for j in range(13)]
                    ops.append(x + [top])
                op.add("range", flat(ops))


def build_linear():
    two = lambda f: (lambda w: f(*split(w, 2)))
    one = lambda f: (lambda w: f(w))

    def exact(valfn, nops, digits_normal):
        """the result's value is exact (not only mod q); digits_normal: digits 0..12 in [0, 2^28)"""
        def check(w, out):
            assert from_limbs(out) == valfn(*[from_limbs(x) for x in split(w, nops)]), "value is not exact"
            if digits_normal:
                assert all(0 <= d <= MASK for d in out[:13]), "digits 0..12 leave [0, 2^28)"
        return check
    specs = (("lin_add", 10, 2, 4, two(l_add), exact(lambda a, b: a + b, 2, False)),
             ("lin_sub", 11, 2, 4, two(l_sub), exact(lambda a, b: a - b, 2, False)),
             ("lin_neg", 12, 1, 7, one(l_neg), exact(lambda a: -a, 1, False)),
             ("lin_mulc3", 13, 1, 2, one(lambda x: l_mulc(3, x)), exact(lambda a: 3 * a, 1, False)),
             ("lin_norm", 14, 1, 7, one(l_norm), exact(lambda a: a, 1, True)),
             ("lin_mulc_norm3", 15, 1, 8, one(lambda x: l_mulc_norm(3, x)), exact(lambda a: 3 * a, 1, True)),
             ("lin_mulc_norm8", 16, 1, 8, one(lambda x: l_mulc_norm(8, x)), exact(lambda a: 8 * a, 1, True)),
             ("lin_mulc_norm12", 17, 1, 8, one(lambda x: l_mulc_norm(12, x)), exact(lambda a: 12 * a, 1, True)))
    for name, code, nops, mag, ref, check in specs:
        op = defop(name, code, "linear", nops * L, L, ref, check)
        lin_values(op, nops, mag, _seed(name))

    def canon_check(w, out):
        v = from_limbs(w)
        assert from_limbs(out) == v % Q and all(0 <= d <= MASK for d in out[:13]) and out[13] >= 0
    op = defop("lin_canon", 18, "linear", L, L, l_canon, canon_check)
    lin_values(op, 1, 1, _seed("lin_canon"), with_range=False)

    def zero_check(w, out):
        assert out[0] == (1 if from_limbs(w) % Q == 0 else 0)       # the sets are all in (-q, 2q), digits normal: 0 and q only
    op = defop("lin_is_zero", 19, "linear", L, 1, lambda w: [l_is_zero(w)], zero_check)
    lin_values(op, 1, 1, _seed("lin_is_zero"), with_range=False)
    for name in ("lin_canon", "lin_is_zero"):                          # one bit away from 0 and from q, at every digit position
        for base in (0, Q):
            d = to_limbs(base)
            for j in range(L):
                e = list(d)
                e[j] ^= 1
                if -Q < from_limbs(e) < 2 * Q:
                    OPS[name].add("edge", e)


# ---- boundaries -------------------------------------------------------------------------------------------------------
C_FROM_VM, C_TO_VM, C_R2 = (1 << 400) % Q, (1 << 384) % Q, R * R % Q


def vm_mul28(A, B):
    """the word model of fp28.h vm_mul28 (the MUL round of the wavefront VM): two integers below 2^384 standing for 12 words each
    -> the integer of the 12 result words, through the column arithmetic of model_dot on A shifted left by 8 bits"""
    assert 0 <= A < 1 << 384 and 0 <= B < 1 << 384 and A * B < 9 * Q * Q
    D = from_limbs(dot([(to_limbs(A << 8), to_limbs(B))]))
    assert 0 <= D < 2 * Q and (D - A * B * pow(1 << 384, -1, Q)) % Q == 0
    return D


QNEG_R = (-pow(Q, -1, R)) % R


def vm_mul28_closed(A, B):
    """the same words without the columns: with non-negative digits model_dot's m is the one m < 2^392 that makes
    (A 2^8 B + m q) divisible by 2^392 (tests/test_vm_vectors_model.py holds the two against each other)"""
    t = (A << 8) * B
    return (t + ((t * QNEG_R) % R) * Q) >> (W * L)


def build_boundaries():
    rnd = _seed("boundaries")
    top384 = (1 << 384) - 1
    ints = [0, 1, top384, Q, Q - 1, Q + 1, 2 * Q - 1, C_TO_VM, 1 << 383, (1 << 384) - (1 << 32), int("5" * 96, 16), int("a" * 96, 16)]
    canon_ints = [0, 1, Q - 1, Q - 2, C_TO_VM, ONE, int("5" * 95, 16) % Q]
    fe_edge = [e for e in EDGE if -Q < from_limbs(e) < 2 * Q]

    op = defop("b_unpack32", 40, "boundary", 12, L, lambda w: to_limbs(from_words(w)))
    for _ in range(NR - 4):
        op.add("random", words12(rnd.randrange(1 << 384)))
    for v in ints:
        op.add("edge", words12(v))

    def pack_ref(w):
        v = from_limbs(w)
        assert 0 <= v < 1 << 384 and all(0 <= d <= MASK for d in w)
        return words12(v)
    op = defop("b_pack32", 41, "boundary", L, 12, pack_ref)
    for _ in range(NR - 4):
        op.add("random", to_limbs(rnd.randrange(1 << 384)))
    for v in ints:
        op.add("edge", to_limbs(v))

    def mk_from(name, code, const, factor):
        def ref(w):
            return dot([(to_limbs(from_words(w)), to_limbs(const))])

        def check(w, out):
            x = from_words(w)
            check_product([(to_limbs(x), to_limbs(const))], out, x < 9 * Q)
            assert (from_limbs(out) - x * factor) % Q == 0
        op = defop(name, code, "boundary", 12, L, ref, check)
        for _ in range(NR - 4):
            op.add("random", words12(rnd.randrange(1 << 384)))
        for v in ints:
            op.add("edge", words12(v))
    mk_from("b_from_vm", 42, C_FROM_VM, 1 << 8)        # x = v 2^384 -> v R = x 2^8
    mk_from("b_from_raw", 44, C_R2, R)                 # content c -> c R

    def mk_to(name, code, factor):
        def ref(w):
            return words12(from_limbs(w) * factor % Q)
        op = defop(name, code, "boundary", L, 12, ref)
        for _ in range(NR - 4):
            op.add("random", rnd_fe(rnd))
        for e in fe_edge:
            op.add("edge", e)
    mk_to("b_to_vm", 43, C_TO_VM * RINV % Q)           # x R -> x 2^384, canonical
    mk_to("b_to_raw", 45, RINV)                        # x R -> x, canonical

    def vm_ref(w):
        return words12(vm_mul28(from_words(w[:12]), from_words(w[12:])))

    def vm_check(w, out):
        A, B, D = from_words(w[:12]), from_words(w[12:]), from_words(out)
        assert D < 2 * Q and (D * (1 << 384) - A * B) % Q == 0
    op = defop("b_vm_mul28", 46, "boundary", 24, 12, vm_ref, vm_check)
    for _ in range(NR - 4):
        op.add("random", words12(rnd.randrange(3 * Q)) + words12(rnd.randrange(3 * Q)))
    x = rnd.randrange(Q)
    for A, B in ((0, x), (x, 0), (1, 1), (3 * Q - 1, 3 * Q - 1), (Q, Q), (C_TO_VM, x), (Q, C_TO_VM), (2 * Q - 1, 2 * Q - 1), (Q - 1, Q - 1),
                 (Q, 1), (1, Q), ((1 << 383) - 1, 1 << 380), (int("5" * 95, 16), 3), (3 * Q - 1, 0), (0, 0)):
        op.add("edge", words12(A) + words12(B))


# ---- Fq2 --------------------------------------------------------------------------------------------------------------
def unflat2(w, n):
    return [M2.unflat(w[k * 2 * L:(k + 1) * 2 * L]) for k in range(n)]


def build_fq2():
    def host_check(hostfn, nops):
        def check(w, out):
            xs = [el_res(M2, x) for x in unflat2(w, nops)]
            got = M2.unflat(out)
            want = hostfn(*xs)
            # products divide by R once more: x R y R / R = x y R; the linear ones keep the form
            assert el_res(M2, got) == (want[0] % Q, want[1] % Q), "differs from hostmath"
        return check
    XI = (1, 1)
    f2_dot2 = lambda a, b, c, d: H.f2_add(H.f2_mul(a, b), H.f2_mul(c, d))
    prod_terms = {"f2_mul": M2.mul_terms, "f2_mul_w": M2.mul_terms, "f2_sqr": M2.sqr_terms, "f2_sqr_w": M2.sqr_terms,
                  "f2_dot2": M2.dot2_terms, "f2_dot2_w": M2.dot2_terms}
    specs = (("f2_mul", 50, 2, lambda w: M2.mul(*unflat2(w, 2)), H.f2_mul, [(0, 1)] * 2),
             ("f2_mul_w", 51, 2, lambda w: M2.mul(*unflat2(w, 2)), H.f2_mul, [(2, 2)] * 2),
             ("f2_sqr", 52, 1, lambda w: M2.sqr(*unflat2(w, 1)), H.f2_sqr, [(0, 1)]),
             ("f2_sqr_w", 53, 1, lambda w: M2.sqr(*unflat2(w, 1)), H.f2_sqr, [(0, 2)]),
             ("f2_dot2", 54, 4, lambda w: M2.dot2(*unflat2(w, 4)), f2_dot2, [(0, 1)] * 4),
             ("f2_dot2_w", 55, 4, lambda w: M2.dot2(*unflat2(w, 4)), f2_dot2, [(2, 1), (1, 1), (1, 2), (0, 1)]),
             ("f2_mul_xi", 56, 1, lambda w: M2.mul_xi(*unflat2(w, 1)), lambda a: H.f2_mul(a, XI), [(4, 4)]),
             ("f2_conj", 57, 1, lambda w: M2.conj(*unflat2(w, 1)), H.f2_conj, [(7, 7)]),
             ("f2_b3", 58, 1, lambda w: M2.b3(*unflat2(w, 1)), lambda a: H.f2_muli(H.f2_mul(a, XI), 12), [(4, 4)]),
             ("f2_norm", 59, 1, lambda w: M2.norm(*unflat2(w, 1)), lambda a: a, [(7, 7)]),
             ("f2_canon", 60, 1, lambda w: (l_canon(w[:L]), l_canon(w[L:])), lambda a: a, [(0, 1)]))
    # (a square of F2<A, B> has (a + b)(a - b) at 2 max(A, B) (A + B) units: F2<0, 2> is the full column)
    want_units = {"f2_mul": 2, "f2_mul_w": 8, "f2_sqr": 2, "f2_sqr_w": 8, "f2_dot2": 4, "f2_dot2_w": 8}
    for name, code, nops, ref, hostfn, ranges in specs:
        op = defop(name, code, "fq2", nops * 2 * L, 2 * L, (lambda r: (lambda w: M2.flat(r(w))))(ref), host_check(hostfn, nops))
        rnd = _seed(name)
        is_prod = name in want_units
        for _ in range(NR - 4):
            if is_prod or name == "f2_canon":
                op.add("random", flat(rnd_fe(rnd) for _ in range(2 * nops)))
            else:
                lo, hi = ranges[0]
                op.add("random", flat([rnd.randrange(-(lo << W), hi << W) for _ in range(13)] + [rnd.randrange(-TOP, TOP + 1)] for _ in range(2)))
        fe_edge = [e for e in EDGE if -Q < from_limbs(e) < 2 * Q] if name == "f2_canon" else EDGE
        for j in range(len(fe_edge)):
            op.add("edge", flat(fe_edge[(j + 5 * m) % len(fe_edge)] for m in range(2 * nops)))
        if is_prod:
            for a, b in REDUCE:                          # x = a + 0 u, y = b + 0 u: the real part is the lone product (a, b);
                ops = []                                 # a square takes a + 0 u, then 0 + a u: (a + b)(a - b) = -a^2, sign included
                for m in range(nops):
                    src = b if m % 2 else a
                    re = rnd_fe(rnd) if src is None else to_limbs(src)
                    ops += [re if m < 2 else [0] * L, [0] * L]
                op.add("reduce", flat(ops))
                if nops == 1:
                    op.add("reduce", flat([ops[1], ops[0]]))
        if name == "f2_canon":
            continue
        # range ends: every part of operand m at its HI end or its -LO end, by pattern, times the three top digits
        pats = {"hi": lambda m, part, j: True, "lo": lambda m, part, j: False, "swap": lambda m, part, j: (m + part) % 2 == 0,
                "alt": lambda m, part, j: (j + part) % 2 == 0}
        if name == "f2_dot2_w":                          # the imaginary part's full column: x0 = -2, y0 = -1, x1 = +2, y1 = +1
            pats = {"imag8": lambda m, part, j: m >= 2, "hi": pats["hi"], "lo": pats["lo"], "alt": pats["alt"]}
        best = (0, 0)
        for pname, pat in pats.items():
            for top in (0, TOP, -TOP):
                ops = []
                for m in range(nops):
                    lo, hi = ranges[m]
                    for part in range(2):
                        ops.append([(digit(hi, True) if pat(m, part, j) else digit(lo, False)) for j in range(13)] + [top])
                if is_prod:
                    got = [column_units(t) for t in prod_terms[name](*unflat2(flat(ops), nops))]
                    best = (max(best[0], max(g[0] for g in got)), max(best[1], max(g[1] for g in got)))
                    assert all(g[0] <= 8 and g[1] <= 9 for g in got), (name, pname, got)
                    if pname == "imag8" or (name == "f2_mul_w" and pname in ("hi", "lo")) or (name in ("f2_sqr", "f2_sqr_w") and pname == "hi"):
                        assert max(max(g) for g in got) == want_units[name], (name, pname, got)
                op.add("range", flat(ops))
        if is_prod:
            assert max(best) == want_units[name], (name, best)

    def zero_check(w, out):
        a, b = unflat2(w, 1)[0]
        assert out[0] == (1 if from_limbs(a) % Q == 0 and from_limbs(b) % Q == 0 else 0)
    op = defop("f2_is_zero", 61, "fq2", 2 * L, 1, lambda w: [l_is_zero(w[:L]) & l_is_zero(w[L:])], zero_check)
    rnd = _seed("f2_is_zero")
    for _ in range(NR - 4):
        op.add("random", rnd_fe(rnd) + rnd_fe(rnd))
    zs = [to_limbs(0), to_limbs(Q)]
    near = [to_limbs(1), to_limbs(Q - 1), to_limbs(Q + 1), to_limbs(-1), [0] * 13 + [1], to_limbs(Q)[:13] + [to_limbs(Q)[13] - 1]]
    for a in zs + near:
        for b in zs + near[:3]:
            op.add("edge", a + b)


# ---- curve ------------------------------------------------------------------------------------------------------------
def golden_points():
    """affine points of the reference's fixtures: off the subgroup, small order, in the subgroup"""
    with open(os.path.join(GOLDEN, "subgroup.json")) as f:
        sg = json.load(f)
    with open(os.path.join(GOLDEN, "pairing_degenerate.json")) as f:
        dg = json.load(f)["cases"]
    out = {}
    for g, M, dec in (("g1", M1, H.g1_from_abi), ("g2", M2, H.g2_from_abi)):
        pts = []
        for kind in ("random", "torsion", "mixed", "subgroup"):
            pts += [dec(bytes.fromhex(r["point"])) for r in sg[g] if r["kind"] == kind and r["on_curve"]][:3]
        for case in ("ord13", "ord11_embedded"):
            pts.append(dec(bytes.fromhex(dg[case][g][0])))
        pts = [p for p in pts if p is not None and H.on_curve(HF(M), p)]
        out[g] = pts
    return out


def build_curve():
    gp = golden_points()
    for g, M, base in (("g1", M1, 70), ("g2", M2, 80)):
        build_curve_group(g, M, base, gp)


def build_curve_group(g, M, base, gp):
    F, rnd = HF(M), _seed("curve" + g)
    PW = 3 * M.DW

    def rnd_el():
        return rnd.randrange(1, Q) if M is M1 else (rnd.randrange(1, Q), rnd.randrange(Q))

    def rnd_point():
        """on the curve, as a rule off the r-torsion subgroup (the cofactor is large)"""
        while True:
            x = rnd_el()
            try:
                return (x, H.y_for_x(F, x)[rnd.randrange(2)])
            except Exception:
                continue
    gen = H.G1_GEN if M is M1 else H.G2_GEN
    sub = [H.jac_to_affine(F, H.jac_mul(F, H.aff_to_jac(F, gen), k)) for k in (1, 2, 0x1234567)]
    pts = [rnd_point() for _ in range(6)] + sub + gp[g]
    # (P, Q, lam_P, lam_Q, rep): the addition cases
    pairs = []
    for i in range(len(pts)):
        pairs.append(("sum", pts[i], pts[(i + 1) % len(pts)]))
    for p in pts[:6] + gp[g][:4]:
        pairs += [("dbl", p, p), ("inv", p, host_neg(M, p)), ("pinf", p, None), ("infq", None, p)]
    pairs.append(("infinf", None, None))

    def pt_check_fn(hostfn, parse, lo=-Q):
        def check(w, out):
            want = hostfn(*parse(w))
            got = pt_unflat(M, out)
            for c in got:
                for x in (c,) if M is M1 else c:
                    assert all(0 <= d <= MASK for d in x[:13]) and lo < from_limbs(x) < 2 * Q, "coordinate leaves the fe form"
            assert affine_of(M, got) == want, "differs from hostmath"
        return check

    def two_pts(w):
        return affine_of(M, pt_unflat(M, w[:PW])), affine_of(M, pt_unflat(M, w[PW:2 * PW]))

    def one_pt(w):
        return (affine_of(M, pt_unflat(M, w[:PW])),)

    def pm_parse(w):
        x2, y2 = M.unflat(w[PW:PW + M.DW]), M.unflat(w[PW + M.DW:PW + 2 * M.DW])
        return affine_of(M, pt_unflat(M, w[:PW])), (el_res(M, x2), el_res(M, y2))

    def chain_parse(w):
        return tuple(affine_of(M, pt_unflat(M, w[k * PW:(k + 1) * PW])) for k in range(9))

    def host_chain(*ps):
        acc = ps[0]
        for p in ps[1:]:
            acc = host_add(M, acc, p)
        return acc

    def m_chain(w):
        acc = pt_unflat(M, w[:PW])
        for k in range(1, 9):
            acc = m_padd(M, acc, pt_unflat(M, w[k * PW:(k + 1) * PW]))
        return pt_flat(M, acc)
    add_ref = lambda w: pt_flat(M, m_padd(M, pt_unflat(M, w[:PW]), pt_unflat(M, w[PW:])))
    dbl_ref = lambda w: pt_flat(M, m_pdbl(M, pt_unflat(M, w)))
    pm_ref = lambda w: pt_flat(M, m_pmadd(M, pt_unflat(M, w[:PW]), M.unflat(w[PW:PW + M.DW]), M.unflat(w[PW + M.DW:])))
    hadd = lambda a, b: host_add(M, a, b)
    hdbl = lambda a: host_add(M, a, a)
    o_padd = defop(g + "_padd", base + 0, "curve", 2 * PW, PW, add_ref, pt_check_fn(hadd, two_pts))
    o_pmadd = defop(g + "_pmadd", base + 1, "curve", PW + 2 * M.DW, PW, pm_ref, pt_check_fn(hadd, pm_parse))
    o_pdbl = defop(g + "_pdbl", base + 2, "curve", PW, PW, dbl_ref, pt_check_fn(hdbl, one_pt))
    o_pneg = defop(g + "_pneg", base + 3, "curve", PW, PW, lambda w: pt_flat(M, m_pneg(M, pt_unflat(M, w))),
                   pt_check_fn(lambda a: host_neg(M, a), one_pt, lo=-2 * Q))   # -Y of a Y in (-q, 2q): normal digits, value in (-2q, q)
    o_padd_fn = defop(g + "_padd_fn", base + 4, "curve", 2 * PW, PW, add_ref, pt_check_fn(hadd, two_pts))
    o_pdbl_fn = defop(g + "_pdbl_fn", base + 5, "curve", PW, PW, dbl_ref, pt_check_fn(hdbl, one_pt))
    o_chain = defop(g + "_chain8", base + 6, "curve", 9 * PW, PW, m_chain, pt_check_fn(host_chain, chain_parse))

    for n, (kind, P, Qp) in enumerate(pairs):
        rep = n % 3                                 # non-canonical coordinates: q for 0, m + q, m - q
        lp, lq = (rnd_el(), rnd_el()) if n % 2 else (F.one, rnd_el())
        dP, dQ = proj(M, P, lp, rep), proj(M, Qp, lq, (rep + 1) % 3)
        for op in (o_padd, o_padd_fn):
            op.add("curve", pt_flat(M, dP) + pt_flat(M, dQ))
        if Qp is not None:                          # the mixed addition takes an affine second point
            o_pmadd.add("curve", pt_flat(M, dP) + M.flat(mont(M, Qp[0], (rep + 1) % 3)) + M.flat(mont(M, Qp[1], (rep + 2) % 3)))
    for n, P in enumerate(pts + [None]):
        for rep in range(3):
            d = proj(M, P, rnd_el() if (n + rep) % 2 else F.one, rep)
            for op in (o_pdbl, o_pdbl_fn, o_pneg):
                op.add("curve", pt_flat(M, d))
    # non-canonical forms as coordinates: the limbs of q, -q + 1 and 2q - 1 where 0, 1 and q - 1 would stand (NONCANON).
    # Z = -q + 1 / 2q - 1 is the point scaled by lam = +-1/R (X is one of them too when x = +-1 is on the curve), X or Y
    # is one under lam = 1/(R x), -1/(R y); the
    # affine x2 of pmadd when x = +-1/R is; infinity as (q : y : q) and (0 : y : q) with y in both forms
    def nc_el(v):
        return M1_nc(v) if M is M1 else (M1_nc(v[0]), M1_nc(v[1]))

    def nc_proj(A, lam):
        return (nc_el(F.mul(A[0], lam)), nc_el(F.mul(A[1], lam)), nc_el(lam))

    def on_curve_with_x(cands):
        for x in cands:
            try:
                return (x, H.y_for_x(F, x)[0])
            except Exception:
                continue
        return None
    unit = [1, Q - 1] if M is M1 else [(1, 0), (Q - 1, 0), (0, 1), (0, Q - 1), (1, 1), (Q - 1, 1), (1, Q - 1), (Q - 1, Q - 1)]
    scaled = [F.muli(u, RINV) for u in unit] if M is M2 else [u * RINV % Q for u in unit]
    lams = [F.muli(F.one, RINV), F.muli(F.one, Q - RINV)] if M is M2 else [RINV, Q - RINV]
    A1, A2 = on_curve_with_x(unit), on_curve_with_x(scaled)
    nc_pts = [nc_proj(A, lam) for A in [a for a in (A1,) if a] + pts[:2] for lam in lams]
    for A in pts[:2]:                                        # and scaled so that X is the form of 1, Y the form of q - 1
        nc_pts += [nc_proj(A, F.mul(lams[0], F.inv(A[0]))), nc_proj(A, F.mul(lams[1], F.inv(A[1])))]
    y_forms = [nc_el(lams[0]), nc_el(lams[1])]               # Y of infinity: the limbs of -q + 1 and of 2q - 1
    nc_inf = [(nc_el(F.zero), y_forms[0], nc_el(F.zero)), (M.zero, y_forms[1], nc_el(F.zero))]
    other = proj(M, pts[3], rnd_el(), 0)
    nc_pairs = []
    for d in nc_pts:
        A = affine_of(M, d)
        nc_pairs += [(d, other), (other, d), (d, d), (d, nc_proj(host_neg(M, A), lams[1])), (d, nc_inf[0]), (nc_inf[1], d)]
    nc_pairs += [(nc_inf[0], nc_inf[1]), (nc_inf[1], nc_inf[0]), (nc_inf[0], other)]
    for dP, dQ in nc_pairs:
        for op in (o_padd, o_padd_fn):
            op.add("curve", pt_flat(M, dP) + pt_flat(M, dQ))
    for d in nc_pts + nc_inf:
        for op in (o_pdbl, o_pdbl_fn, o_pneg):
            op.add("curve", pt_flat(M, d))
        for A in [a for a in (A2,) if a] + [pts[4]]:
            o_pmadd.add("curve", pt_flat(M, d) + M.flat(nc_el(A[0])) + M.flat(nc_el(A[1])))
    chain = [nc_inf[0]] + (nc_pts + nc_inf + nc_pts)[:8]
    o_chain.add("curve", flat(pt_flat(M, d) for d in chain))
    # chains: eight additions on product-form accumulators, with a doubling, an inverse and infinity on the way
    for n in range(6):
        ps = [pts[(n + 3 * k) % len(pts)] for k in range(9)]
        if n == 1:
            ps[3] = host_chain(*ps[:3])             # the running sum meets itself: P + P inside the chain
        if n == 2:
            ps[4] = host_neg(M, host_chain(*ps[:4]))   # ... and its negative: the sum passes through infinity
            ps[5] = None
        if n == 3:
            ps[0] = None
        w = []
        for k, p in enumerate(ps):
            w += pt_flat(M, proj(M, p, rnd_el() if k % 2 else F.one, (n + k) % 3))
        o_chain.add("curve", w)


def build_all():
    build_products()
    build_linear()
    build_boundaries()
    build_fq2()
    build_curve()
    for op in OPS.values():
        assert 0 < len(op.sets) <= MAX_SETS, (op.name, len(op.sets))
    assert len({op.code for op in OPS.values()}) == len(OPS)


build_all()
GROUPS = ("raw", "linear", "typed", "boundary", "fq2", "curve")


def counts():
    """{group: {"ops": n, class: vectors}} and {op: {class: vectors}}"""
    by_group = {g: dict({"ops": 0}, **{c: 0 for c in CLASSES}) for g in GROUPS}
    by_op = {}
    for op in OPS.values():
        by_group[op.group]["ops"] += 1
        by_op[op.name] = {c: 0 for c in CLASSES}
        for cls, _ in op.sets:
            by_group[op.group][cls] += 1
            by_op[op.name][cls] += 1
    return by_group, by_op


COUNTS, COUNTS_PER_OP = counts()


def counts_table():
    lines = ["  group    ops  random  edge  reduce  range  curve"]
    for g in GROUPS:
        c = COUNTS[g]
        lines.append("  %-8s %3d  %6d %5d  %6d %6d %6d" % (g, c["ops"], c["random"], c["edge"], c["reduce"], c["range"], c["curve"]))
    return "\n".join(lines)


_EXPECTED = {}


def expected(name):
    """the expected output words of every set of an op (computed once)"""
    if name not in _EXPECTED:
        op = OPS[name]
        _EXPECTED[name] = [[int(v) for v in op.ref(w)] for _, w in op.sets]
    return _EXPECTED[name]


def call_words(name, n):
    """input words of a call with n items, and the set index of each item"""
    op = OPS[name]
    idx = [item_set(i, len(op.sets)) for i in range(n)]
    w = []
    for k in idx:
        w += op.sets[k][1]
    return w, idx


if __name__ == "__main__":
    print(counts_table())
    for name, c in COUNTS_PER_OP.items():
        print("  %-16s %s" % (name, " ".join("%s=%d" % kv for kv in c.items() if kv[1])))
