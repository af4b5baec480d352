"""Operand sets, a limb-exact model and independent references for the G2 curve layer on lane pairs (sp2) and lane quads (sp4), the
group traits SrtG<1> / SrtG<2> and the digit routines of csrc/blsgpu_msm.hip, one list per op of the test-only device library
csrc/blsgpu_curve_check.hip.  Pure Python: tests/test_curve_vectors_model.py checks the model on the CPU, tests/test_gpu_curve.py
compares the compiled routines with it word for word and checks the device's own words with the independent reference.

Limb model: the formulas of sp2 and sp4 line by line over ml_vectors' p_mul, p_dot2, p_sqr, p_b3, p_norm, p_mulc_norm, p_add, p_sub,
p_neg, p_mulf, p_is_zero2 (whose products are vmgen.gen_fp28.model_dot with the 64-bit accumulator asserted).  A pair value is
(re, im), two lists of 14 limbs; a quad value is [pair 0's, pair 1's] and sp4's model follows sp4's own dataflow (pick / oth per
level, two reduced products added, then norm), so its words differ from sp2's.  SrtG<1> is fp28_vectors' one-lane m_pmadd.

Independent reference: bls_py.hostmath on Python integers.  The output words, read as a homogeneous (x = X / Z) or Jacobian
(x = X / Z^2, y = Y / Z^3) point, must be the host's point (cross-multiplied mod q); infinity is Z = 0 with (0 : Y : 0), Y != 0,
resp. (X : Y : 0), X^3 = Y^2 != 0.  pdblj is a polynomial map, so it is compared coordinate by coordinate with hostmath.jac_double on
ANY operand, on the curve or not.  affine_out and st_vm write canonical words: the host's bytes.  Digits: sum d_w 16^w = s,
sum (v_w - 2^(cb-1)) 2^(cb w) = s with the record s + C built here, key = |d| - 1 and the sign.

CONTRACT of an h coordinate (the header of the check file derives it): limbs 0 .. 12 digits in [0, 2^28), value in (-17q, 22q).

Set classes (the tag's prefix): sub (random points of the twist's subgroup), off (points of the twist outside it), gold (the
fixtures' small-order and torsion points), dbl (P, P), inv (P, -P), inf (infinity first, second, both; as pt_inf's (0 : R : 0), the
Jacobian (1 : 1 : 0), the Z left by a cancellation in the model, Z with the limbs of q), lam (one point scaled by 1, -1, 2, R, random,
real and purely imaginary factors), coord (coordinates 0, 1, q - 1, u-only: not on the curve, compared word for word and, for pdblj
and the affine conversions, by value), extreme (digits all 0 / all 2^28 - 1 in sign patterns with the top digit at both ends of the
contract: word for word, and sp2 against sp4 coordinate by coordinate mod q)."""
import random

import fp28_vectors as FV
import ml_vectors as MV
from bls_py import hostmath as H
from ml_vectors import (p_add, p_sub, p_neg, p_mulc, p_norm, p_mulc_norm, p_b3, p_mul, p_dot2, p_sqr, p_mulf, p_is_zero2, s32, to_limbs,
                        from_limbs, res2, Q, R, L, MASK, ONE, QT)

F2 = H.F2
M1, M2 = FV.M1, FV.M2
V2, PT, P1 = 2 * L, 6 * L, 3 * L
N_PAIR_ITEMS = (1, 31, 32, 33, 129)
N_QUAD_ITEMS = (1, 15, 16, 17, 65)
N_LANE_ITEMS = (1, 63, 64, 65, 257)
CONTRACT = (-17 * Q, 22 * Q)
FILL = s32(0xAAAAAAAA)                                 # what check_runner.h fills the output with: a word nothing stored to
N_GROUP = H.N
SRT_SCW, SRT_MAXBITS = 9, 14
PEAK = {}                                              # op -> {set tag: largest |column sum| of its products}
MUT = set()                                            # the mutants of the model that are switched on (test_curve_vectors_model.py)
ONE2 = (to_limbs(ONE), [0] * L)
ZERO2 = ([0] * L, [0] * L)


def in_contract(x):
    return all(0 <= d <= MASK for d in x[:13]) and CONTRACT[0] < from_limbs(x) < CONTRACT[1]


# ---- sp2: what either lane of a pair computes ---------------------------------------------------------------------------------
def pt_inf():
    return (ZERO2, ONE2, ZERO2)


def s2_pmadd(P, x2, y2):
    X, Y, Z = P
    t0, t1 = p_mul(x2, X), p_mul(y2, Y)
    t3 = p_norm(p_sub(p_sub(p_mul(p_add(x2, y2), p_add(X, Y)), t0), t1))
    t4 = p_norm(p_add(p_mul(y2, Z), Y))
    y3 = p_b3(p_add(p_mul(x2, Z), X))
    x3 = p_mulc_norm(3, t0)
    bz = p_b3(ZERO2 if "pmadd_z2_zero" in MUT else Z)
    z3, t1m = p_norm(p_add(t1, bz)), p_norm(p_sub(t1, bz))
    return (p_dot2(t3, t1m, p_neg(t4), y3), p_dot2(y3, x3, t1m, z3), p_dot2(z3, t4, x3, t3))


def _b3(x):
    return p_mulc_norm(4, MV.p_mul_xi(x)) if "b3_no_3" in MUT else p_b3(x)


def s2_padd(P, Qp):
    (X1, Y1, Z1), (X2, Y2, Z2) = P, Qp
    t0, t1, t2 = p_mul(X1, X2), p_mul(Y1, Y2), p_mul(Z1, Z2)
    t3 = p_norm(p_sub(p_sub(p_mul(p_add(X1, Y1), p_add(X2, Y2)), t0), t1))
    t4 = p_norm(p_sub(p_sub(p_mul(p_add(Y1, Z1), p_add(Y2, Z2)), t1), t2))
    t5 = p_sub(p_sub(p_mul(p_add(X1, Z1), p_add(X2, Z2)), t0), t2)
    x3, bz = p_mulc_norm(3, t0), _b3(t2)
    z3, t1m = p_norm(p_add(t1, bz)), p_norm(p_sub(t1, bz))
    if "t1m_z3" in MUT:
        z3, t1m = t1m, z3
    y3 = _b3(t5)
    return (p_dot2(t3, t1m, p_neg(t4), y3), p_dot2(t1m, z3, y3, x3), p_dot2(z3, t4, x3, t3))


def s2_pdbl(P):
    X, Y, Z = P
    t0, t1, t2, txy = p_sqr(Y), p_mul(Y, Z), _b3(p_sqr(Z)), p_mul(X, Y)
    z8 = p_mulc_norm(8, t0)
    d = p_norm(p_sub(t0, p_mulc(3, t2)))
    return (p_mul(d, p_add(txy, txy)), p_dot2(t2, z8, d, p_add(t0, t2)), p_mul(t1, z8))


def s2_pneg(P):
    return (P[0], p_norm(p_neg(P[1])), P[2])


def s2_pdblj(P):
    X, Y, Z = P
    A, B = p_sqr(X), p_sqr(Y)
    C = p_sqr(B)
    D = p_mulc_norm(2, p_sub(p_sub(p_sqr(p_norm(p_add(X, B))), A), C))
    E = p_mulc_norm(3, A)
    X3 = p_norm(p_sub(p_sqr(E), p_mulc(2, D)))
    Z3 = p_mul(p_add(Y, Y), Z)
    Y3 = p_norm(p_sub(p_mul(E, p_norm(p_sub(D, X3))), p_mulc_norm(4 if "dblj_4c" in MUT else 8, C)))
    return (X3, Y3, Z3)


def zero2(x):
    return p_is_zero2(p_mulf(x, to_limbs(ONE)))


def s2_to_jacobian(P):
    X, Y, Z = P
    inf = zero2(Z) and "toj_no_select" not in MUT
    zz = p_sqr(Z)
    x, y = p_mul(X, Z), p_mul(Y, zz)
    return (ONE2 if inf else x, ONE2 if inf else y, Z)


def s2_to_homogeneous(P):
    X, Y, Z = P
    zz = p_sqr(Z)
    return (p_mul(X, Z), Y, Z if "toh_leaves_z" in MUT else p_mul(zz, Z))


# ---- sp4: a value per pair of the quad ---------------------------------------------------------------------------------------------
def lift(f):
    return lambda *a: [f(*(x[k] for x in a)) for k in range(2)]


def liftc(f):
    return lambda c, x: [f(c, x[k]) for k in range(2)]


q_add, q_sub, q_neg, q_norm, q_mul, q_sqr, q_b3 = (lift(f) for f in (p_add, p_sub, p_neg, p_norm, p_mul, p_sqr, p_b3))
q_mulc, q_mulc_norm = liftc(p_mulc), liftc(p_mulc_norm)


def pick(a, b): return [a[0], b[1]]
def oth(x): return [x[1], x[0]]
def both(P): return tuple([c, c] for c in P)


def s4_pdblj(P):
    X, Y, Z = P
    r1 = q_sqr(pick(X, Y)); o1 = oth(r1)
    A, B = pick(r1, o1), pick(o1, r1)
    r2 = q_sqr(pick(B, q_norm(q_add(X, B)))); o2 = oth(r2)
    C, T = pick(r2, o2), pick(o2, r2)
    D = q_mulc_norm(2, q_sub(q_sub(T, A), C))
    E = q_mulc_norm(3, A)
    X3 = q_norm(q_sub(q_sqr(E), q_mulc(2, D)))
    r4 = q_mul(pick(E, q_add(Y, Y)), pick(q_norm(q_sub(D, X3)), Z)); o4 = oth(r4)
    return (X3, q_norm(q_sub(pick(r4, o4), q_mulc_norm(4 if "dblj_4c" in MUT else 8, C))), pick(o4, r4))


def s4_pdbl(P):
    X, Y, Z = P
    s1, m1 = q_sqr(pick(Y, Z)), q_mul(pick(Y, X), pick(Z, Y))
    os_, om = oth(s1), oth(m1)
    t0, t1, t2, txy = pick(s1, os_), pick(m1, om), lift(_b3)(pick(os_, s1)), pick(om, m1)
    z8 = q_mulc_norm(8, t0)
    d = q_norm(q_sub(t0, q_mulc(3, t2)))
    ma = q_mul(pick(d, t2), pick(q_norm(q_add(txy, txy)), z8))
    mb = q_mul(pick(t1, d), pick(z8, q_norm(q_add(t0, t2))))
    oa, ob = oth(ma), oth(mb)
    return (pick(ma, oa), q_norm(q_add(pick(oa, ma), pick(ob, mb))), pick(mb, ob))


def s4_padd(P, Qp):
    (X1, Y1, Z1), (X2, Y2, Z2) = P, Qp
    l0, l1, l2 = pick(X1, q_add(X1, Y1)), pick(Y1, q_add(Y1, Z1)), pick(Z1, q_add(X1, Z1))
    q0, q1, q2 = pick(X2, q_add(X2, Y2)), pick(Y2, q_add(Y2, Z2)), pick(Z2, q_add(X2, Z2))
    a0, a1, a2 = q_mul(l0, q0), q_mul(l1, q1), q_mul(l2, q2)
    if "pair1_no_oth" in MUT:
        b0, b1, b2 = [a0[1], a0[1]], [a1[1], a1[1]], [a2[1], a2[1]]      # pair 1 keeps its own products
    else:
        b0, b1, b2 = oth(a0), oth(a1), oth(a2)
    t0, t1, t2 = pick(a0, b0), pick(a1, b1), pick(a2, b2)
    u3, u4, u5 = pick(b0, a0), pick(b1, a1), pick(b2, a2)
    t3 = q_norm(q_sub(q_sub(u3, t0), t1))
    t4 = q_norm(q_sub(q_sub(u4, t1), t2))
    t5 = q_sub(q_sub(u5, t0), t2)
    x3, bz = q_mulc_norm(3, t0), lift(_b3)(t2)
    z3, t1m = q_norm(q_add(t1, bz)), q_norm(q_sub(t1, bz))
    if "t1m_z3" in MUT:
        z3, t1m = t1m, z3
    y3 = lift(_b3)(t5)
    nt4 = q_norm(q_neg(t4))
    c0 = q_mul(pick(t3, nt4), pick(t1m, y3))
    c1 = q_mul(pick(y3, t1m), pick(z3, x3)) if "pick_swapped" in MUT else q_mul(pick(t1m, y3), pick(z3, x3))
    c2 = q_mul(pick(z3, x3), pick(t4, t3))
    return tuple(q_norm(q_add(c, oth(c))) for c in (c0, c1, c2))


def s4_to_jacobian(P):
    X, Y, Z = P
    inf = [zero2(Z[k]) and "toj_no_select" not in MUT for k in range(2)]
    zz = q_sqr(Z)
    m = q_mul(pick(X, Y), pick(Z, zz)); o = oth(m)
    x, y = pick(m, o), pick(o, m)
    return ([ONE2 if inf[k] else x[k] for k in range(2)], [ONE2 if inf[k] else y[k] for k in range(2)], Z)


def s4_to_homogeneous(P):
    X, Y, Z = P
    zz = q_sqr(Z)
    m = q_mul(pick(X, zz), [Z[0], Z[1]]); o = oth(m)
    return (pick(m, o), Y, Z if "toh_leaves_z" in MUT else pick(o, m))


class A2:
    add, dblj, toj, toh, neg, lanes = staticmethod(s2_padd), staticmethod(s2_pdblj), staticmethod(s2_to_jacobian), staticmethod(s2_to_homogeneous), staticmethod(s2_pneg), 2
    enter = staticmethod(lambda P: P)
    words = staticmethod(lambda pts: [d for P in pts for c in P for part in c for d in part])
    first = staticmethod(lambda P: P)


class A4:
    add, dblj, toj, toh, lanes = staticmethod(s4_padd), staticmethod(s4_pdblj), staticmethod(s4_to_jacobian), staticmethod(s4_to_homogeneous), 4
    neg = staticmethod(lambda P: (P[0], q_norm(q_neg(P[1])), P[2]))
    enter = staticmethod(both)
    words = staticmethod(lambda pts: [d for k in range(2) for P in pts for c in P for part in c[k] for d in part])
    first = staticmethod(lambda P: tuple(c[0] for c in P))


def chain_add8(A, P):
    acc, out = A.enter(pt_inf()), []
    for _ in range(8):
        acc = A.add(acc, A.enter(P))
        out.append(acc)
    return out


def chain_jac(A, P, k):
    P = A.toj(A.enter(P))
    out = [P]
    for _ in range(k):
        P = A.dblj(P)
        out.append(P)
    return out + [A.toh(P)]


def chain_cancel(A, P):
    P = A.enter(P)
    out = [A.add(P, A.neg(P))]
    out.append(A.toj(out[-1]))
    out.append(A.dblj(out[-1]))
    out.append(A.dblj(out[-1]))
    out.append(A.toh(out[-1]))
    return out


def chain_running(A, Bs):
    acc = tot = A.enter(pt_inf())
    out = []
    for it in range(8):
        if it % 2 == 0:
            acc = A.add(acc, A.enter(Bs[3 - it // 2]))
            out.append(acc)
        else:
            tot = A.add(tot, acc)
            out.append(tot)
    return out


# ---- words and values ------------------------------------------------------------------------------------------------------------
def pt_words(P):
    return [d for c in P for part in c for d in part]


def pt_of(w):
    return tuple((list(w[k * V2:k * V2 + L]), list(w[k * V2 + L:(k + 1) * V2])) for k in range(3))


def pts_of(w, n):
    return [pt_of(w[k * PT:(k + 1) * PT]) for k in range(n)]


def pt1_of(w):
    return tuple(list(w[k * L:(k + 1) * L]) for k in range(3))


def vals(P):
    return tuple(res2(c) for c in P)


def hom_affine(P):
    """the words of a homogeneous point -> hostmath's affine pair, None at infinity (which must be (0 : Y : 0), Y != 0)"""
    X, Y, Z = vals(P)
    if F2.is_zero(Z):
        assert F2.is_zero(X) and not F2.is_zero(Y), "Z = 0 but not (0 : Y : 0)"
        return None
    zi = F2.inv(Z)
    return (F2.mul(X, zi), F2.mul(Y, zi))


def jac_affine(P):
    X, Y, Z = vals(P)
    if F2.is_zero(Z):
        assert not F2.is_zero(X) and F2.mul(F2.sqr(X), X) == F2.sqr(Y), "Z = 0 but not (l^2 : l^3 : 0)"
        return None
    return H.jac_to_affine(F2, (X, Y, Z))


def host_add(A, B):
    return H.jac_to_affine(F2, H.jac_add(F2, H.aff_to_jac(F2, A), H.aff_to_jac(F2, B)))


def host_neg(A):
    return None if A is None else (A[0], F2.neg(A[1]))


def host_mul(A, k):
    return None if A is None else H.jac_to_affine(F2, H.jac_mul(F2, H.aff_to_jac(F2, A), k))


def le_words(b):
    return [s32(int.from_bytes(b[4 * i:4 * i + 4], "little")) for i in range(len(b) // 4)]


def affine_words(DEG, A, store=1):
    """affine_out's output: the canonical bytes, then the flag byte in a word of its own"""
    n = 24 * DEG
    if not store:
        return [FILL] * (n + 1)
    b = (H.g1_affine_bytes if DEG == 1 else H.g2_affine_bytes)(A)
    return le_words(b) + [s32(0xAAAAAA00 | (1 if A is None else 0))]


def affine2_value(P):
    """(X, Y) / Z by value for ANY words ((0, 0) for Z = 0) -- what SrtG<2>::affine_out computes"""
    X, Y, Z = vals(P)
    if F2.is_zero(Z):
        return None
    zi = F2.inv(Z)
    A = (F2.mul(X, zi), F2.mul(Y, zi))
    return None if A == ((0, 0), (0, 0)) else A


def vm_words(P):
    """sp2::st_vm: every part x R as the canonical x 2^384, twelve words, least significant first"""
    return [w for c in P for part in c for w in FV.words12(MV.res(part) * (1 << 384) % Q)]


# ---- operands --------------------------------------------------------------------------------------------------------------------
def _rnd(tag):
    return random.Random("curve:" + tag)


def mont2(v, rep=0):
    return FV.mont(M2, v, rep)


def hproj(A, lam=None, rep=0):
    return FV.proj(M2, A, lam, rep)


def jproj(A, lam=None, rep=0):
    lam = F2.one if lam is None else lam
    l2 = F2.sqr(lam)
    if A is None:
        return (mont2(l2, rep), mont2(F2.mul(l2, lam), rep), mont2(F2.zero, rep))
    return (mont2(F2.mul(A[0], l2), rep), mont2(F2.mul(A[1], F2.mul(l2, lam)), rep), mont2(lam, rep))


_BASE = None


def base_points():
    """{class: affine points of the twist}"""
    global _BASE
    if _BASE is None:
        rnd = _rnd("points")
        G = H.G2_GEN
        sub = [host_mul(G, k) for k in (1, 2, 0x1234567, rnd.randrange(1, N_GROUP))]
        off = []
        while len(off) < 4:
            x = (rnd.randrange(Q), rnd.randrange(Q))
            try:
                off.append((x, H.y_for_x(F2, x)[rnd.randrange(2)]))
            except Exception:
                continue
        assert all(host_mul(p, N_GROUP) is not None for p in off)
        gold = FV.golden_points()["g2"]
        _BASE = {"sub": sub, "off": off, "gold": gold}
    return _BASE


def lambdas(rnd):
    return [("1", F2.one), ("-1", (Q - 1, 0)), ("2", (2, 0)), ("R", (R % Q, 0)), ("rnd", (rnd.randrange(1, Q), rnd.randrange(1, Q))),
            ("real", (rnd.randrange(2, Q), 0)), ("imag", (0, rnd.randrange(1, Q)))]


TOP_HI, TOP_LO = (CONTRACT[1] >> (28 * 13)) - 1, -((-CONTRACT[0]) >> (28 * 13))


def extreme_parts():
    """digit patterns at both ends of the contract: all 0 / all 2^28 - 1, the top digit 0 and at its extremes"""
    out = [[MASK] * 13 + [0], [0] * 13 + [0], [MASK] * 13 + [TOP_HI], [0] * 13 + [TOP_LO + 1], [MASK] * 13 + [TOP_LO], [0] * 13 + [TOP_HI]]
    assert all(in_contract(x) for x in out)
    return out


def coord_values():
    return [(0, 0), (1, 0), (Q - 1, 0), (0, 1), (0, Q - 1), (1, 1)]


def cancelled(P):
    """the Z (and X, Y) an actual cancellation leaves: padd(P, -P) in the model"""
    return s2_padd(P, s2_pneg(P))


def point_sets(jac=False):
    """[(tag, point limbs, host affine point or "free" for words that are no curve point)]"""
    B, rnd = base_points(), _rnd("point_sets/%d" % jac)
    pr = jproj if jac else hproj
    out = []
    for cls in ("sub", "off", "gold"):
        for i, A in enumerate(B[cls]):
            lam = (rnd.randrange(1, Q), rnd.randrange(Q)) if i % 2 else None
            out.append(("%s/%d" % (cls, i), pr(A, lam, i % 3), A))
    for name, lam in lambdas(rnd):
        out.append(("lam/" + name, pr(B["sub"][3], lam), B["sub"][3]))
    qq = (to_limbs(Q), to_limbs(Q))
    if jac:
        out += [("inf/one-one-zero", (ONE2, ONE2, ZERO2), None), ("inf/scaled", jproj(None, (5, 7)), None), ("inf/z-limbs-of-q", (ONE2, ONE2, qq), None)]
    else:
        c = cancelled(hproj(B["sub"][0], (3, 4)))
        out += [("inf/pt_inf", pt_inf(), None), ("inf/scaled", hproj(None, (5, 7), 1), None), ("inf/cancelled", c, None),
                ("inf/z-limbs-of-q", (ZERO2, ONE2, qq), None), ("inf/x-z-limbs-of-q", (qq, mont2((9, 9)), (to_limbs(Q), [0] * L)), None)]
    cv = coord_values()
    for i in range(len(cv)):
        out.append(("coord/%d" % i, tuple(mont2(cv[(i + k) % len(cv)], (i + k) % 3) for k in range(3)), "free"))
    ex = extreme_parts()
    for i in range(len(ex)):
        out.append(("extreme/%d" % i, tuple((ex[(i + 2 * k) % len(ex)], ex[(i + 2 * k + 1) % len(ex)]) for k in range(3)), "free"))
    out.append(("extreme/ones", tuple((ex[0], ex[0]) for _ in range(3)), "free"))
    out.append(("extreme/re-only", tuple((ex[0], ex[1]) for _ in range(3)), "free"))
    out.append(("extreme/im-only", tuple((ex[1], ex[0]) for _ in range(3)), "free"))
    if jac:
        out.append(("coord/x-zero", (mont2((0, 0), 2), mont2((3, 5)), mont2((7, 2))), "free"))
        out.append(("coord/y-real", (mont2((11, 13)), mont2((rnd.randrange(1, Q), 0)), mont2((7, 2))), "free"))
    return out


def pair_sets():
    """[(tag, P limbs, Q limbs, host P, host Q)]: the operands of an addition"""
    B, rnd = base_points(), _rnd("pair_sets")
    pts = B["sub"] + B["off"] + B["gold"]
    rl = lambda: (rnd.randrange(1, Q), rnd.randrange(Q))
    out = []
    for i, A in enumerate(pts):
        Bq = pts[(i + 1) % len(pts)]
        cls = "sub" if i < 4 else "off" if i < 8 else "gold"
        out.append(("%s/sum/%d" % (cls, i), hproj(A, rl() if i % 2 else None, i % 3), hproj(Bq, rl(), (i + 1) % 3), A, Bq))
    for i, A in enumerate(pts[:2] + pts[4:6] + B["gold"][:2]):
        out.append(("dbl/%d" % i, hproj(A, rl(), i % 3), hproj(A, rl(), (i + 1) % 3), A, A))
        out.append(("dbl/same-words/%d" % i, hproj(A), hproj(A), A, A))
        out.append(("inv/%d" % i, hproj(A, rl(), i % 3), hproj(host_neg(A), rl(), (i + 2) % 3), A, host_neg(A)))
        out.append(("inv/pneg/%d" % i, hproj(A, (2, 1)), s2_pneg(hproj(A, (2, 1))), A, host_neg(A)))
    A = pts[3]
    infs = [t for t in point_sets() if t[0].startswith("inf/")]
    for tag, Pi, _ in infs:
        out.append((tag + "/first", Pi, hproj(A, rl()), None, A))
        out.append((tag + "/second", hproj(A, rl()), Pi, A, None))
        out.append((tag + "/both", Pi, infs[0][1], None, None))
    for name, lam in lambdas(rnd):
        out.append(("lam/" + name, hproj(A, lam), hproj(pts[5], lam), A, pts[5]))
    free = [t for t in point_sets() if t[2] == "free"]
    for i, (tag, Pf, _) in enumerate(free):
        out.append((tag, Pf, free[(i + 1) % len(free)][1], "free", "free"))
    return out


# ---- the ops of the device library -----------------------------------------------------------------------------------------------
class Op:
    def __init__(self, name, code, win, wout, lanes, group, model):
        self.name, self.code, self.win, self.wout, self.lanes, self.group, self.model = name, code, win, wout, lanes, group, model
        self.sets = []                                 # (tag, words in, expected words out, operand coordinates, check or None)

    def add(self, tag, words, coords=(), check=None):
        words = [int(w) for w in words]
        MV._peak[0] = 0
        want = [int(w) for w in self.model(words)]
        PEAK.setdefault(self.name, {})[tag] = MV._peak[0]
        assert len(words) == self.win and len(want) == self.wout, (self.name, tag, len(words), len(want))
        assert all(-(1 << 31) <= w < (1 << 31) for w in words + want), (self.name, tag)
        self.sets.append((tag, words, want, list(coords), check))

    @property
    def counts(self):
        return {1: N_LANE_ITEMS, 2: N_PAIR_ITEMS, 4: N_QUAD_ITEMS}[self.lanes]


def coords_of(*pts):
    return [part for P in pts for c in P for part in c]


def expect_hom(want_aff):
    def check(got):
        assert hom_affine(pt_of(got)) == want_aff, "differs from hostmath"
    return check


def expect_jac(want_aff):
    def check(got):
        assert jac_affine(pt_of(got)) == want_aff, "differs from hostmath"
    return check


def expect_jac_double(P):
    """pdblj against hostmath.jac_double on the residues, coordinate by coordinate (any operand with Y != 0)"""
    want = H.jac_double(F2, vals(P))

    def check(got):
        if want is not None:
            assert vals(pt_of(got)) == want, "differs from hostmath.jac_double"
    return check


def both_pairs(check, pw):
    """a quad op's output: pair 1's words equal pair 0's, which the check reads"""
    def chk(got):
        assert got[:pw] == got[pw:2 * pw], "the two pairs of the quad differ"
        check(got[:pw])
    return chk


def _point_ops(o):
    PS, JS, PAIRS = point_sets(), point_sets(True), pair_sets()
    B = base_points()

    def unary(name, code, lanes, group, fn, sets, check_of):
        A = A4 if lanes == 4 else A2
        op = o[name] = Op(name, code, PT, PT * (lanes // 2), lanes, group, lambda w: A.words([fn(A.enter(pt_of(w)))]))
        for tag, P, host in sets:
            chk = check_of(P, host)
            op.add(tag, pt_words(P), coords_of(P), both_pairs(chk, PT) if (lanes == 4 and chk) else chk)

    hom1 = lambda f: (lambda P, host: None if host == "free" else expect_hom(f(host)))
    dbl = lambda A: host_add(A, A)
    jac_of_hom = lambda P, host: None if host == "free" else expect_jac(host)
    hom_of_jac = lambda P, host: None if host == "free" else expect_hom(host)
    jdbl = lambda P, host: expect_jac_double(P) if host == "free" else (lambda c1, c2: (lambda g: (c1(g), c2(g))))(expect_jac(dbl(host)), expect_jac_double(P))
    op = o["PT_INF"] = Op("PT_INF", 0, 1, PT, 2, "pair", lambda w: pt_words(pt_inf()))
    op.add("inf/pt_inf", [0], (), expect_hom(None))
    op = o["PT_LD_ST"] = Op("PT_LD_ST", 1, PT, PT, 2, "pair", lambda w: list(w))
    for tag, P, host in PS:
        op.add(tag, pt_words(P), coords_of(P))
    op.add("extreme/negative-top", pt_words(tuple(([5] * 13 + [TOP_LO], [MASK] * 13 + [-1]) for _ in range(3))), ())
    unary("PNEG", 2, 2, "pair", s2_pneg, PS, hom1(host_neg))
    unary("PDBL", 3, 2, "pair", s2_pdbl, PS, hom1(dbl))
    unary("SRTG2_DBL", 7, 2, "pair", s2_pdbl, PS, hom1(dbl))
    unary("TO_JACOBIAN", 10, 2, "pair", s2_to_jacobian, PS, jac_of_hom)
    unary("PDBLJ", 11, 2, "pair", s2_pdblj, JS, jdbl)
    unary("TO_HOMOGENEOUS", 12, 2, "pair", s2_to_homogeneous, JS, hom_of_jac)
    unary("SP4_PDBLJ", 20, 4, "quad", s4_pdblj, JS, jdbl)
    unary("SP4_PDBL", 21, 4, "quad", s4_pdbl, PS, hom1(dbl))
    unary("SP4_TO_JACOBIAN", 23, 4, "quad", s4_to_jacobian, PS, jac_of_hom)
    unary("SP4_TO_HOMOGENEOUS", 24, 4, "quad", s4_to_homogeneous, JS, hom_of_jac)
    for name, code, lanes, group, A in (("PADD", 4, 2, "pair", A2), ("SRTG2_ADD", 8, 2, "pair", A2), ("SP4_PADD", 22, 4, "quad", A4)):
        op = o[name] = Op(name, code, 2 * PT, PT * (lanes // 2), lanes, group,
                          lambda w, A=A: A.words([A.add(A.enter(pt_of(w[:PT])), A.enter(pt_of(w[PT:])))]))
        for tag, P, Qp, hp, hq in PAIRS:
            chk = None if hp == "free" else expect_hom(host_add(hp, hq))
            op.add(tag, pt_words(P) + pt_words(Qp), coords_of(P, Qp), both_pairs(chk, PT) if (lanes == 4 and chk) else chk)
    # the mixed additions: an accumulator and an affine point (x, y) resp. the prepared record (x, y, -y)
    rnd = _rnd("madd")
    pts = B["sub"] + B["off"] + B["gold"]
    madd = []                                          # (tag, accumulator limbs, host accumulator, affine point)
    for i, A in enumerate(pts):
        madd.append(("%s/%d" % ("sub" if i < 4 else "off" if i < 8 else "gold", i), hproj(pts[(i + 3) % len(pts)], (rnd.randrange(1, Q), rnd.randrange(Q)), i % 3), pts[(i + 3) % len(pts)], A))
    for i, A in enumerate(pts[:2] + pts[4:6]):
        madd += [("dbl/%d" % i, hproj(A, (rnd.randrange(1, Q), 3), i % 3), A, A), ("dbl/z-one/%d" % i, hproj(A), A, A),
                 ("inv/%d" % i, hproj(host_neg(A), (7, rnd.randrange(Q)), i % 3), host_neg(A), A)]
    for tag, Pi, host in PS:
        if tag.startswith("inf/"):
            madd.append((tag, Pi, None, pts[1]))
    for name, lam in lambdas(rnd):
        madd.append(("lam/" + name, hproj(pts[2], lam), pts[2], pts[6]))
    free = [t for t in PS if t[2] == "free"]

    def pm_model(w):
        P, x2, y2 = pt_of(w[:PT]), (w[PT:PT + L], w[PT + L:PT + V2]), (w[PT + V2:PT + V2 + L], w[PT + V2 + L:PT + 2 * V2])
        return pt_words(s2_pmadd(P, x2, p_norm(p_neg(y2))))
    op = o["PMADD_NEG"] = Op("PMADD_NEG", 5, PT + 2 * V2, PT, 2, "pair", pm_model)
    for i, (tag, P, hp, A) in enumerate(madd):
        x2, y2 = mont2(A[0], i % 3), mont2(A[1], (i + 1) % 3)
        op.add(tag, pt_words(P) + x2[0] + x2[1] + y2[0] + y2[1], coords_of(P) + [x2[0], x2[1], y2[0], y2[1]], expect_hom(host_add(hp, host_neg(A))))
    for i, (tag, P, _) in enumerate(free):
        x2, y2 = free[(i + 1) % len(free)][1][0], free[(i + 2) % len(free)][1][1]
        y2 = tuple(x if from_limbs(x) < 2 * Q and from_limbs(x) > -Q else to_limbs(from_limbs(x) % Q) for x in y2)   # an affine y is from_raw's
        x2 = tuple(x if from_limbs(x) < 2 * Q and from_limbs(x) > -Q else to_limbs(from_limbs(x) % Q) for x in x2)
        op.add(tag, pt_words(P) + x2[0] + x2[1] + y2[0] + y2[1], coords_of(P) + [x2[0], x2[1], y2[0], y2[1]])

    def srt2_model(w):
        P, neg = pt_of(w[:PT]), w[PT + 3 * V2]
        x2 = (w[PT:PT + L], w[PT + L:PT + V2])
        y2 = (w[PT + (1 + neg) * V2:PT + (1 + neg) * V2 + L], w[PT + (1 + neg) * V2 + L:PT + (2 + neg) * V2])
        return pt_words(s2_pmadd(P, x2, y2))
    op = o["SRTG2_MADD"] = Op("SRTG2_MADD", 6, PT + 3 * V2 + 1, PT, 2, "pair", srt2_model)
    for i, (tag, P, hp, A) in enumerate(madd):
        for neg in (0, 1):
            x2, y2 = mont2(A[0]), mont2(A[1])          # k_srt_prep: from_raw's digits, -y = norm(neg(y))
            ny = p_norm(p_neg(y2))
            rec = x2[0] + x2[1] + y2[0] + y2[1] + ny[0] + ny[1]
            op.add("%s/neg%d" % (tag, neg), pt_words(P) + rec + [neg], coords_of(P) + [x2[0], x2[1], y2[0], y2[1]],
                   expect_hom(host_add(hp, host_neg(A) if neg else A)))
    # the conversions out
    op = o["ST_VM"] = Op("ST_VM", 13, PT, 72, 2, "pair", lambda w: vm_words(pt_of(w)))
    for tag, P, host in PS:
        op.add(tag, pt_words(P), coords_of(P))
    aff = [(tag, P) for tag, P, host in PS]
    z_forms = [("z-real", mont2((rnd.randrange(1, Q), 0))), ("z-imag", mont2((0, rnd.randrange(1, Q)))), ("z-zero", mont2((0, 0), 2)),
               ("z-norm-one", mont2(F2.mul((3, 4), F2.inv((3, Q - 4)))))]
    assert F2.mul(res2(z_forms[3][1]), H.f2_conj(res2(z_forms[3][1]))) == (1, 0)
    for name, z in z_forms:
        aff.append(("coord/" + name, (mont2((rnd.randrange(Q), rnd.randrange(Q))), mont2((rnd.randrange(Q), rnd.randrange(Q)), 1), z)))
    op = o["SRTG2_AFFINE_OUT"] = Op("SRTG2_AFFINE_OUT", 14, PT + 1, 49, 2, "pair", lambda w: affine_words(2, affine2_value(pt_of(w[:PT])), w[PT]))
    for i, (tag, P) in enumerate(aff):
        for store in ((1, 0) if i % 4 == 0 else (1,)):
            op.add("%s/store%d" % (tag, store), pt_words(P) + [store], coords_of(P))


def _lane_ops(o):
    B1 = FV.golden_points()["g1"]
    F1, rnd = H.F1, _rnd("g1")
    mul1 = lambda A, k: H.jac_to_affine(F1, H.jac_mul(F1, H.aff_to_jac(F1, A), k))
    pts = [mul1(H.G1_GEN, k) for k in (1, 2, 0xABCDEF, rnd.randrange(1, N_GROUP))] + B1[:6]
    hadd = lambda a, b: FV.host_add(M1, a, b)
    hneg = lambda a: FV.host_neg(M1, a)

    def chk(want):
        def check(got):
            assert FV.affine_of(M1, pt1_of(got)) == want, "differs from hostmath"
        return check

    def model(w):
        P, neg = pt1_of(w[:P1]), w[P1 + 3 * L]
        return FV.pt_flat(M1, FV.m_pmadd(M1, P, w[P1:P1 + L], w[P1 + (1 + neg) * L:P1 + (2 + neg) * L]))
    op = o["SRTG1_MADD"] = Op("SRTG1_MADD", 30, P1 + 3 * L + 1, P1, 1, "lane", model)
    cases = [("sum/%d" % i, FV.proj(M1, pts[(i + 3) % len(pts)], rnd.randrange(1, Q), i % 3), pts[(i + 3) % len(pts)], A) for i, A in enumerate(pts)]
    for i, A in enumerate(pts[:3] + pts[4:6]):
        cases += [("dbl/%d" % i, FV.proj(M1, A, rnd.randrange(1, Q), i % 3), A, A), ("inv/%d" % i, FV.proj(M1, hneg(A), rnd.randrange(1, Q)), hneg(A), A)]
    cases += [("inf/pt_inf", FV.proj(M1, None), None, pts[0]), ("inf/scaled", FV.proj(M1, None, 77, 1), None, pts[1]),
              ("inf/z-limbs-of-q", (to_limbs(Q), to_limbs(ONE), to_limbs(Q)), None, pts[2])]
    for tag, P, hp, A in cases:
        x, y = FV.mont(M1, A[0]), FV.mont(M1, A[1])
        ny = FV.l_norm(FV.l_neg(y))
        for neg in (0, 1):
            op.add("%s/neg%d" % (tag, neg), FV.pt_flat(M1, P) + x + y + ny + [neg], list(P) + [x, y], chk(hadd(hp, hneg(A) if neg else A)))

    def aff1(w):
        X, Y, Z = (MV.res(c) for c in pt1_of(w[:P1]))
        A = None if Z == 0 else (X * pow(Z, -1, Q) % Q, Y * pow(Z, -1, Q) % Q)
        return affine_words(1, None if A == (0, 0) else A, w[P1])
    op = o["SRTG1_AFFINE_OUT"] = Op("SRTG1_AFFINE_OUT", 32, P1 + 1, 25, 1, "lane", aff1)
    for i, (tag, P, hp, A) in enumerate(cases):
        for store in ((1, 0) if i % 4 == 0 else (1,)):
            op.add("%s/store%d" % (tag, store), FV.pt_flat(M1, P) + [store], list(P))


def _chain_ops(o):
    B, rnd = base_points(), _rnd("chains")
    rl = lambda: (rnd.randrange(1, Q), rnd.randrange(Q))
    pts = [("sub/0", B["sub"][0]), ("sub/3", B["sub"][3]), ("off/0", B["off"][0]), ("off/1", B["off"][1])] + [("gold/%d" % i, A) for i, A in enumerate(B["gold"])]
    starts = [(tag, hproj(A, rl() if i % 2 else None, i % 3), A) for i, (tag, A) in enumerate(pts)]
    infs = [(t, P, None) for t, P, h in point_sets() if t.startswith("inf/")]

    def per_step(A, checks):
        """every step's point against the host's (both pairs of a quad the same words)"""
        n = len(checks)

        def check(got):
            pw = n * PT
            if A.lanes == 4:
                assert got[:pw] == got[pw:2 * pw], "the two pairs of the quad differ"
            for k, c in enumerate(checks):
                c(got[k * PT:(k + 1) * PT])
        return check
    for A, sfx, c0 in ((A2, "_2", 40), (A4, "_4", 41)):
        op = o["CHAIN_ADD8" + sfx] = Op("CHAIN_ADD8" + sfx, c0, PT, 8 * PT * (A.lanes // 2), A.lanes, "chain", lambda w, A=A: A.words(chain_add8(A, pt_of(w))))
        for tag, P, host in starts + infs:
            op.add(tag, pt_words(P), coords_of(P), per_step(A, [expect_hom(host_mul(host, k)) for k in range(1, 9)]))
    for A, sfx, c0 in ((A2, "_2", 42), (A4, "_4", 46)):
        for j, k in enumerate((1, 2, 16, 60)):
            name = "CHAIN_JAC_%d%s" % (k, sfx)
            op = o[name] = Op(name, c0 + j, PT, (k + 2) * PT * (A.lanes // 2), A.lanes, "chain", lambda w, A=A, k=k: A.words(chain_jac(A, pt_of(w), k)))
            for tag, P, host in ((infs + starts[:1]) if k == 60 else (starts + infs)):
                checks = [expect_jac(host_mul(host, 1 << i)) for i in range(k + 1)] + [expect_hom(host_mul(host, 1 << k))]
                op.add(tag, pt_words(P), coords_of(P), per_step(A, checks))
    for A, sfx, code in ((A2, "_2", 50), (A4, "_4", 51)):
        def model(w, A=A):
            steps = chain_cancel(A, pt_of(w))
            return A.words(steps) + affine_words(2, affine2_value(A.first(steps[-1])))
        name = "CHAIN_CANCEL" + sfx
        op = o[name] = Op(name, code, PT, 5 * PT * (A.lanes // 2) + 49, A.lanes, "chain", model)
        for tag, P, host in starts + infs:
            def check(got, A=A):
                pw = 5 * PT
                per_step(A, [expect_hom(None), expect_jac(None), expect_jac(None), expect_jac(None), expect_hom(None)])(got[:pw * (A.lanes // 2)])
                assert got[-49:] == affine_words(2, None), "not (0, 0) and flag 1"
            op.add(tag, pt_words(P), coords_of(P), check)
    hp = [A_ for _, A_ in pts]
    layouts = [[hp[0], None, hp[1], None], [None, None, hp[2], hp[3]], [hp[1], hp[1], None, None], [None, hp[0], None, host_neg(hp[0])],
               [hp[4 % len(hp)], None, None, hp[5 % len(hp)]], [None, hp[2], hp[2], None]]
    buckets = [[pt_inf() if (h is None and (i + j) % 2) else hproj(h, rl() if h is not None else (3, 1), (i + j) % 3) for j, h in enumerate(hb)]
               for i, hb in enumerate(layouts)]
    for A, sfx, code in ((A2, "_2", 52), (A4, "_4", 53)):
        name = "CHAIN_RUNNING" + sfx
        op = o[name] = Op(name, code, 4 * PT, 8 * PT * (A.lanes // 2), A.lanes, "chain", lambda w, A=A: A.words(chain_running(A, pts_of(w, 4))))
        for i, (hb, Bs) in enumerate(zip(layouts, buckets)):
            acc = tot = None
            checks = []
            for it in range(8):
                if it % 2 == 0:
                    acc = host_add(acc, hb[3 - it // 2])
                    checks.append(expect_hom(acc))
                else:
                    tot = host_add(tot, acc)
                    checks.append(expect_hom(tot))
            op.add("running/%d" % i, [d for P in Bs for d in pt_words(P)], coords_of(*Bs), per_step(A, checks))


# ---- digits ----------------------------------------------------------------------------------------------------------------------
def scalar_words(s):
    """32 big-endian bytes as the words that lie in memory"""
    return le_words(s.to_bytes(32, "big"))


def _sc_word(w, j):
    """bswap32(sc[7 - j]): word j of the scalar, least significant first"""
    return int.from_bytes((w[7 - j] & 0xFFFFFFFF).to_bytes(4, "little"), "big")


def lane_digit(w, win):
    """lane_digit word for word: (digit, big)"""
    top = _sc_word(w, 7)
    big = top >= 0x77777776 if "big_ge" in MUT else top > 0x77777776
    if not big:
        c = word = 0
        for j in range(win // 8 + 1):
            t = _sc_word(w, j) + 0x88888888 + c
            word, c = t & 0xFFFFFFFF, 0 if "no_carry" in MUT else t >> 32
    else:
        word = _sc_word(w, win // 8)
    nib = (word >> (4 * (win % 8))) & 15
    return (nib if big else nib - 8), int(big)


def lane_digit_null(win):
    word = 0x88888889 if win < 8 else 0x88888888
    return ((word >> (4 * (win % 8))) & 15) - 8


def srt_windows(cb):
    return (258 + cb - 1) // cb


def srt_record(s, cb):
    """s + C, C = sum_w 2^(cb - 1) 2^(cb w) over the windows (blsgpu_api.hip sets bit cb w + cb - 1 of the bias for every window)"""
    C = sum(1 << (cb * w + cb - 1) for w in range(srt_windows(cb)))
    t = s + C
    assert t < 1 << (32 * SRT_SCW)
    return [s32(t >> (32 * j)) for j in range(SRT_SCW)]


def srt_digit_key(rec, w, cb):
    rec = [x & 0xFFFFFFFF for x in rec]
    o = w * cb
    j, sft = o >> 5, o & 31
    v = rec[j] >> sft
    if sft + cb > 32 and j + 1 < SRT_SCW and "no_second_word" not in MUT:
        v |= (rec[j + 1] << (32 - sft)) & 0xFFFFFFFF
    v &= (1 << cb) - 1
    half = 1 << (cb - 1)
    sign = 1 if v < half else 0
    if "sign_at_half" in MUT and v == half - 1:
        sign = 0
    k = ((half - v) if sign else (v - half)) - 1
    return [v, s32(k), sign, int(v != half)]


def digit_scalars():
    rnd = _rnd("scalars")
    n = N_GROUP
    out = [("s/0", 0), ("s/1", 1), ("s/n-1", n - 1), ("s/n", n), ("s/2^255", 1 << 255), ("s/2^256-1", (1 << 256) - 1)]
    for top in (0x77777776, 0x77777777):
        out += [("top/%x/ones" % top, (top << 224) | ((1 << 224) - 1)), ("top/%x/zeros" % top, top << 224)]
    for k in range(1, 9):                              # 0x7777..78 in the k low words: the carry ripples through k words
        out.append(("ripple/%d" % k, int("7" * (8 * k - 1) + "8", 16)))
    out.append(("nibbles-8", int("8" * 56, 16)))
    out.append(("nibbles-8/below-big", int("77777776" + "8" * 56, 16)))
    out += [("random/%d" % i, rnd.randrange(n)) for i in range(4)] + [("random/big/%d" % i, rnd.randrange(1 << 255, 1 << 256)) for i in range(2)]
    return out


def _digit_ops(o):
    def check_digits(s, big):
        def note(w, d):
            check_digits.acc[(s, big)] = check_digits.acc.get((s, big), 0) + d * 16 ** w
        return note
    op = o["LANE_DIGIT"] = Op("LANE_DIGIT", 60, 9, 2, 1, "digit", lambda w: [s32(x) for x in lane_digit(w[:8], w[8])])
    for tag, s in digit_scalars():
        for win in range(64):
            op.add("%s/w%d" % (tag, win), scalar_words(s) + [win])
    for win in range(64):                              # every nibble value at every window
        for nib in range(16):
            s = (nib << (4 * win)) | (0x3 << 252 if win < 63 else 0)
            if win == 63 and nib > 7:
                s = nib << 252
            op.add("nibble/%d/w%d" % (nib, win), scalar_words(s) + [win])
    op = o["LANE_DIGIT_NULL"] = Op("LANE_DIGIT_NULL", 61, 2, 1, 1, "digit", lambda w: [lane_digit_null(w[0])])
    for win in range(64):
        op.add("w%d" % win, [win, 0])
    op = o["SRT_DIGIT_KEY"] = Op("SRT_DIGIT_KEY", 62, SRT_SCW + 2, 4, 1, "digit", lambda w: srt_digit_key(w[:9], w[9], w[10]))
    scal = [t for t in digit_scalars() if not t[0].startswith("ripple") or t[0] in ("ripple/1", "ripple/8")]
    for cb in range(5, SRT_MAXBITS + 1):
        half, nw = 1 << (cb - 1), srt_windows(cb)
        for tag, s in scal:
            rec = srt_record(s, cb)
            for w in range(nw):
                op.add("cb%d/%s/w%d" % (cb, tag, w), rec + [w, cb])
        for v in (0, half - 1, half, half + 1, (1 << cb) - 1):          # a chosen biased digit in every window (the others half: digit 0)
            for w in range(nw):
                t = sum((v if x == w else half) << (cb * x) for x in range(nw))
                if t < 1 << (32 * SRT_SCW):
                    op.add("cb%d/v%d/w%d" % (cb, v, w), [s32(t >> (32 * j)) for j in range(SRT_SCW)] + [w, cb])


_OPS = None


def ops():
    """name -> Op, built once (the expected words are the limb model's)"""
    global _OPS
    if _OPS is None:
        assert not MUT
        o = {}
        _point_ops(o)
        _lane_ops(o)
        _chain_ops(o)
        _digit_ops(o)
        assert len({op.code for op in o.values()}) == len(o)
        _OPS = o
    return _OPS


GROUPS = ("pair", "quad", "lane", "chain", "digit")


def group(name):
    return [op for op in ops().values() if op.group == name]


def call_sets(op, n, base=0):
    """the set of every item of a call of n items: item i is the same set in every call (base: where a further call goes on)"""
    return [(base + i) % len(op.sets) for i in range(n)]


def xor_call(DEG, n, off):
    """xor_lanes on whole wavefronts: (words in, expected words): every unit another point, the result the unit `off` away's"""
    rnd = _rnd("xor/%d/%d/%d" % (DEG, n, off))
    pw = PT if DEG == 2 else P1
    items = [[s32(rnd.randrange(1 << 32)) for _ in range(pw)] for _ in range(n)]
    return [w for it in items for w in it + [off]], [items[i ^ off] for i in range(n)]


def summary():
    out = {}
    for g in GROUPS:
        sel = group(g)
        peak = max((max(PEAK[op.name].values()) for op in sel), default=0)
        out[g] = (len(sel), sum(len(op.sets) for op in sel), peak / float(1 << 63))
    return out


if __name__ == "__main__":
    for g, (n, s, p) in summary().items():
        print("%-6s %2d ops %5d sets  largest column %.4f x 2^63" % (g, n, s, p))
