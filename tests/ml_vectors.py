"""Operand sets and a limb-exact integer model of the lane-pair (ml::sp), lane-quad (ml::sq) and six-lane-team routines of
csrc/blsgpu_ml.hip, one list per op of the test-only device library csrc/blsgpu_ml_check.hip.  Pure Python:
tests/test_ml_vectors_model.py checks the model against plain integers mod q (vmgen/linestream_model.py) on the CPU,
tests/test_gpu_ml_steps.py compares the compiled routines with it word for word.

The reduction of fp28_dot1/2/3/4/6 is tests/fp28_vectors.dot (vmgen.gen_fp28.model_dot, the 64-bit accumulator asserted);
this file only says which limbs every lane hands to it.  A pair value is (re, im), two lists of 14 limbs: the even lane's
part and the odd lane's; a team value is six of them, lane c holding the coefficient of w^c.

Contracts (what makes an operand admissible), as blsgpu_ml.hip states them:
  S<M>   limbs 0..12 in (-M 2^28, M 2^28); limb 13 small and signed: an S<M> is a sum or difference of M values of (-q, 2q),
         so |limb 13| <= M (q >> 364) here (the products of limb 13 sit inside the two units of slack of a column, fp28.h)
  hn     limbs 0..12 DIGITS in [0, 2^28), value in (-q, 2q): what a product, a carry pass or a load returns
  fe     the same (both lanes of a pair hold it); the slab's -3 px is r28::mulc_norm<3>(neg(px)): digits, value in (-6q, 3q)
  team f "normalised digits (value in (-2q, 3q))" for mul_line_k3, (-2q, 4q) after mul_dense: limbs 0..12 in [0, 2^28)
  line record, as the chain kernels and k_ml_lines_exact store it:
         coefficient 0   tangent_step / sq::tangent_step store sub(B, E), a difference of two hn: limbs 0..12 in (-2^28, 2^28);
                         B is a square, value in (-q, 2q), E = b3(C) = 12 (1 + u) C a carry pass, value in (-36q, 48q): the
                         difference lies in (-49q, 38q), |limb 13| <= 49 (q >> 364) < 2^23; chord_step stores a dot2 result
                         (hn); k_ml_lines_exact py or px (hn) and zeros
         coefficients 1, 2   always the result of a product (mulf, or 0): hn
         so: parts 0, 1 have limbs in (-2^28, 2^28), parts 2..5 digits in [0, 2^28) -- the ranges the column bounds of
         mul_line_k3 are argued from (P3: (2 x 2) + (2 x 1) + (2 x 1) = 8)
  dense record (mul_dense's g): a team value as stored: digits.

Set classes per op (the tag's prefix): random; special (0, 1 R, q - 1, q, and -q as the negated limbs of q where the type is
signed; all digits 0 and all digits 2^28 - 1 with the top digit at both ends); extreme (limbs 0..12 at +-(bound - 1), or at
0 / 2^28 - 1 for digits, in every sign pattern of the operand parts -- among them the aligned and the anti-aligned one of either
lane's formula).  BOUND gives, per product op, the column bound in units of 2^56 per limb product that the comment at the
routine claims; PEAK (filled while the expected words are computed) the largest |column sum of limb products| the model met.
Two claims are not attainable, because u and w of a lane's square are not independent, and are replaced by the derived ones,
written down here.  sqr(h) says 4 units (|u|, |w| < 2^29), but u w is (a + b)(a - b) = a^2 - b^2 on the even lane and 2 b a on
the odd one, so |u w| < 2^57: 2 units.  sqr_m12sqr says 4 + 2; the even lane has |a^2 - b^2| < 2^56 for g and a digit of
-12 u_e times |a - b| < 2^29 for e (1 + 2), the odd lane 2 b a for g and a digit times |a| < 2^28 for e (2 + 1): 3 units.
"""
import random

from vmgen import gen_fp28 as G
from vmgen import linestream_model as LM
from fp28_vectors import dot as _dot, l_add, l_sub, l_neg, l_mulc, l_norm, l_mulc_norm, l_is_zero, s32

Q, R, L, W, MASK = G.Q, G.R, G.L, G.W, G.MASK
to_limbs, from_limbs = G.to_limbs, G.from_limbs
RINV = pow(R, -1, Q)
ONE = R % Q
QT = Q >> (W * (L - 1))                                # limb 13 of q
L0_TOP = 49 * QT                                       # |limb 13| of a line record's coefficient 0 (module docstring)
V2, REC, TV = 2 * L, 6 * L, 12 * L
N_PAIR_ITEMS = (1, 31, 32, 33, 129)                    # a wavefront holds 32 pairs, a workgroup 128
N_QUAD_ITEMS = (1, 15, 16, 17, 65)
N_TEAM_ITEMS = (1, 9, 10, 11, 41)                      # ten teams per wavefront, forty per workgroup
POSITIONS = ((2, 3), (3, 5), (4, 5))                   # line_positions(): scaled lines, the reference's lines, its vertical chords

# per product op: the claimed column bound in units of 2^56 (see the module docstring for SQR_H and SQR_M12SQR)
BOUND = {"MUL_31": 6, "MUL_11": 2, "DOT2_1111": 4, "SQR_H": 2, "SQR_HN2": 8, "SQR_M12SQR": 3, "MULF_1": 1, "MULF_3": 3,
         "SP_TANGENT": 8, "MUL3_012": 6, "MUL3_345": 6, "MUL3_012_RAW": 8, "TEAM_LINE": 8, "TEAM_DENSE": 6, "TEAM_SQUARE": 6,
         "TEAM_TEAMREC": 6}
PEAK = {}                                              # op -> {set tag: largest |column sum| of its products}
_peak = [0]


def dot(terms):
    """fp28_vectors.dot, noting the largest column of sum_t a_t b_t on the way (the m q part and the carry are the model's)"""
    for k in range(2 * L - 1):
        lo, hi = max(0, k - L + 1), min(k, L - 1)
        c = abs(sum(a[i] * b[k - i] for a, b in terms for i in range(lo, hi + 1)))
        if c > _peak[0]:
            _peak[0] = c
    return _dot(terms)


def top32(x):
    assert -(1 << 31) <= x[L - 1] < (1 << 31), "limb 13 leaves int32"
    return x


# ---- lane pairs: what either lane computes (sp::) --------------------------------------------------------------------------
def p_add(x, y): return (l_add(x[0], y[0]), l_add(x[1], y[1]))
def p_sub(x, y): return (l_sub(x[0], y[0]), l_sub(x[1], y[1]))
def p_neg(x): return (l_neg(x[0]), l_neg(x[1]))
def p_mulc(c, x): return (l_mulc(c, x[0]), l_mulc(c, x[1]))
def p_norm(x): return (top32(l_norm(x[0])), top32(l_norm(x[1])))
def p_mulc_norm(c, x): return (top32(l_mulc_norm(c, x[0])), top32(l_mulc_norm(c, x[1])))
def p_mul_xi(x): return (l_sub(x[0], x[1]), l_add(x[0], x[1]))         # even lane re - im, odd lane re + im
def p_b3(x): return p_mulc_norm(12, p_mul_xi(x))


def p_mul(x, y):
    """left(x): a = re on both lanes, b = -im on the even lane, im on the odd one; right(y): own part, partner's part"""
    return (dot([(x[0], y[0]), (l_neg(x[1]), y[1])]), dot([(x[0], y[1]), (x[1], y[0])]))


def p_dot2(x0, y0, x1, y1):
    return (dot([(x0[0], y0[0]), (l_neg(x0[1]), y0[1]), (x1[0], y1[0]), (l_neg(x1[1]), y1[1])]),
            dot([(x0[0], y0[1]), (x0[1], y0[0]), (x1[0], y1[1]), (x1[1], y1[0])]))


def _uw(x):
    """sqr_parts: u = im + own part, w = re - (im on the even lane, 0 on the odd one)"""
    return (l_add(x[1], x[0]), l_sub(x[0], x[1])), (l_add(x[1], x[1]), list(x[0]))


def p_sqr(x):
    (ue, we), (uo, wo) = _uw(x)
    return (dot([(ue, we)]), dot([(uo, wo)]))


def p_sqr_m12sqr(g, e):
    out = []
    for lane in range(2):
        ug, wg = _uw(g)[lane]
        ue, we = _uw(e)[lane]
        out.append(dot([(ug, wg), (top32(l_mulc_norm(-12, ue)), we)]))
    return tuple(out)


def p_mulf(x, k): return (dot([(x[0], k)]), dot([(x[1], k)]))
def p_is_zero2(x): return l_is_zero(x[0]) & l_is_zero(x[1])


def be_words(v):
    """a coordinate as load_coord reads it: 48 big-endian bytes seen as 12 little-endian words"""
    b = v.to_bytes(48, "big")
    return [s32(int.from_bytes(b[4 * i:4 * i + 4], "little")) for i in range(12)]


def load_part(words):
    v = int.from_bytes(b"".join((w & 0xFFFFFFFF).to_bytes(4, "little") for w in words), "big")
    return dot([(to_limbs(v), to_limbs(R * R % Q))])   # r28::from_raw


def rec_of(l0, l1, l2):
    return list(l0[0]) + list(l0[1]) + list(l1[0]) + list(l1[1]) + list(l2[0]) + list(l2[1])


def sp_tangent(X, Y, Z, px3n, py):
    XX = p_sqr(X)
    l1 = p_mulf(XX, px3n)
    C, B = p_sqr(Z), p_sqr(Y)
    H = p_sub(p_sub(p_sqr(p_add(Y, Z)), B), C)
    l2 = p_mulf(H, py)
    z8, E = p_mulc_norm(4, H), p_b3(C)
    A2 = p_sub(p_sub(p_sqr(p_add(X, Y)), XX), B)
    l0 = p_sub(B, E)
    F3 = p_mulc(3, E)
    BmF, Gg = p_norm(p_sub(B, F3)), p_norm(p_add(B, F3))
    return p_mul(A2, BmF), p_sqr_m12sqr(Gg, E), p_mul(B, z8), rec_of(l0, l1, l2)


def sq_tangent(X, Y, Z, px3n, py):
    """sq::tangent_step: every value ends up the same on both pairs of the quad"""
    XX, C, B = p_sqr(X), p_sqr(Z), p_sqr(Y)
    T1, T2 = p_sqr(p_norm(p_add(Y, Z))), p_sqr(p_norm(p_add(X, Y)))
    H = p_sub(p_sub(T1, B), C)
    z8, E = p_mulc_norm(4, H), p_b3(C)
    A2 = p_sub(p_sub(T2, XX), B)
    l0 = p_sub(B, E)
    F3 = p_mulc(3, E)
    BmF, Gg = p_norm(p_sub(B, F3)), p_norm(p_add(B, F3))
    l1, l2 = p_mulf(XX, px3n), p_mulf(H, py)
    X3, Z3 = p_mul(A2, BmF), p_mul(B, z8)
    Y3 = p_norm(p_sub(p_sqr(Gg), p_mulc_norm(12, p_sqr(E))))
    return X3, Y3, Z3, rec_of(l0, l1, l2)


def sp_chord(X, Y, Z, px3n, py, xq, yq):
    th, la = p_norm(p_sub(Y, p_mul(yq, Z))), p_norm(p_sub(X, p_mul(xq, Z)))
    xq3, nyq3 = p_mulc_norm(3, xq), p_mulc_norm(3, p_neg(yq))
    l0 = p_dot2(th, xq3, la, nyq3)
    l1, l2 = p_mulf(th, px3n), p_mulf(la, top32(l_mulc_norm(3, py)))
    C, D = p_sqr(th), p_sqr(la)
    E, Fz, Gg = p_mul(la, D), p_mul(Z, C), p_mul(X, D)
    H = p_norm(p_sub(p_add(E, Fz), p_add(Gg, Gg)))
    GH, nE = p_norm(p_sub(Gg, H)), p_norm(p_neg(E))
    return p_mul(la, H), p_dot2(th, GH, nE, Y), p_mul(Z, E), rec_of(l0, l1, l2)


# ---- teams of six lanes --------------------------------------------------------------------------------------------------
def publish(f, norm):
    out = []
    for re, im in f:
        xre, xim = l_sub(re, im), l_add(re, im)
        if norm:
            xre, xim = top32(l_norm(xre)), top32(l_norm(xim))
        out.append({"re": list(re), "im": list(im), "nim": l_neg(im), "xre": xre, "xim": xim, "nxim": l_neg(xim)})
    return out


def fetch(P, c, J):
    """lane c's operand F_{c - J}: from lane (c - J) mod 6, the xi form iff the source wraps (src + J >= 6)"""
    src = (c - J) % 6
    xi = J > 0 and src + J >= 6
    p = P[src]
    return {"re": p["xre"] if xi else p["re"], "im": p["xim"] if xi else p["im"], "nim": p["nxim"] if xi else p["nim"]}


def mul3(P, Js, ys):
    """ys: three (re, im); per lane (re, im) = sum_J F_{c - J} y_J"""
    out = []
    for c in range(6):
        X = [fetch(P, c, J) for J in Js]
        re = dot([t for x, y in zip(X, ys) for t in ((x["re"], y[0]), (x["nim"], y[1]))])
        im = dot([t for x, y in zip(X, ys) for t in ((x["re"], y[1]), (x["im"], y[0]))])
        out.append((re, im))
    return out


def mul_dense(f, g):
    P = publish(f, True)
    a, b = mul3(P, (0, 1, 2), g[:3]), mul3(P, (3, 4, 5), g[3:])
    return [(top32(l_norm(l_add(a[c][0], b[c][0]))), top32(l_norm(l_add(a[c][1], b[c][1])))) for c in range(6)]


def mul_line_k3(f, jA, jB, y):
    """y: the record's six parts"""
    P = publish(f, False)
    ys0, ys1, ys2 = l_add(y[0], y[1]), top32(l_norm(l_add(y[2], y[3]))), top32(l_norm(l_add(y[4], y[5])))
    out = []
    for c in range(6):
        X1, X2 = fetch(P, c, jA), fetch(P, c, jB)
        re, im = f[c]
        p1 = dot([(re, y[0]), (X1["re"], y[2]), (X2["re"], y[4])])
        p2 = dot([(im, y[1]), (X1["im"], y[3]), (X2["im"], y[5])])
        p3 = dot([(l_add(re, im), ys0), (l_add(X1["re"], X1["im"]), ys1), (l_add(X2["re"], X2["im"]), ys2)])
        out.append((top32(l_norm(l_sub(p1, p2))), top32(l_norm(l_sub(l_sub(p3, p1), p2)))))
    return out


# ---- values behind the limbs ---------------------------------------------------------------------------------------------
def res(x): return from_limbs(x) * RINV % Q
def res2(x): return (res(x[0]), res(x[1]))
def val2(x): return (from_limbs(x[0]) % Q, from_limbs(x[1]) % Q)


# ---- operands --------------------------------------------------------------------------------------------------------------
def _rnd(tag):
    return random.Random("ml:" + tag)


HN_TOP_MAX, HN_TOP_MIN = ((2 * Q) >> (W * (L - 1))) - 1, -QT


def admissible(kind, x):
    """kind: 'hn' / 'fe' (digits, value in (-q, 2q)), 'px3n' (digits, (-6q, 3q)), 'f' (digits, (-2q, 3q)), an int M for S<M>,
    'l0' a part of a record's coefficient 0"""
    if kind in ("hn", "fe", "px3n", "f"):
        lo, hi = {"hn": (-Q, 2 * Q), "fe": (-Q, 2 * Q), "px3n": (-6 * Q, 3 * Q), "f": (-2 * Q, 3 * Q)}[kind]
        return all(0 <= d <= MASK for d in x[:13]) and lo < from_limbs(x) < hi
    if kind == "l0":
        return all(abs(d) < 1 << W for d in x[:13]) and abs(x[13]) <= L0_TOP
    return all(abs(d) < kind << W for d in x[:13]) and abs(x[13]) <= kind * QT


def rnd_part(kind, rnd):
    if kind in ("hn", "fe"):
        return to_limbs(rnd.randrange(-Q + 1, 2 * Q))
    if kind == "px3n":
        return to_limbs(rnd.randrange(-6 * Q + 1, 3 * Q))
    if kind == "f":
        return to_limbs(rnd.randrange(-2 * Q + 1, 3 * Q))
    if kind == "l0":
        return [rnd.randrange(-MASK, MASK + 1) for _ in range(13)] + [rnd.randrange(-L0_TOP, L0_TOP + 1)]
    return [rnd.randrange(-(kind << W) + 1, kind << W) for _ in range(13)] + [rnd.randrange(-kind * QT, kind * QT + 1)]


def specials(kind):
    """(name, limbs)"""
    out = [("0", to_limbs(0)), ("1R", to_limbs(ONE)), ("q-1", to_limbs(Q - 1)), ("q", to_limbs(Q)), ("ones", [MASK] * 13 + [0])]
    if kind in ("hn", "fe", "px3n", "f"):
        lo = {"hn": HN_TOP_MIN, "fe": HN_TOP_MIN, "px3n": -6 * QT, "f": -2 * QT}[kind]
        hi = {"hn": HN_TOP_MAX, "fe": HN_TOP_MAX, "px3n": 3 * QT - 1, "f": 3 * QT - 1}[kind]
        out += [("ones/top+", [MASK] * 13 + [hi]), ("ones/top-", [MASK] * 13 + [lo]), ("zeros/top+", [0] * 13 + [hi]),
                ("zeros/top-", [0] * 13 + [lo + 1])]
    else:
        m = 1 if kind == "l0" else kind
        t = L0_TOP if kind == "l0" else kind * QT
        e = (m << W) - 1
        out += [("-q", l_neg(to_limbs(Q))), ("-ones", [-MASK] * 13 + [0]), ("hi/top+", [e] * 13 + [t]), ("lo/top-", [-e] * 13 + [-t]),
                ("hi/top-", [e] * 13 + [-t]), ("zeros/top+", [0] * 13 + [t]), ("alt", [e if j % 2 else -e for j in range(13)] + [0])]
    assert all(admissible(kind, x) for _, x in out), kind
    return out


def ext_part(kind, sign):
    if kind in ("hn", "fe", "px3n", "f"):
        return [MASK if sign > 0 else 0] * 13 + [0]
    m = 1 if kind == "l0" else kind
    return [sign * ((m << W) - 1)] * 13 + [0]


def sign_patterns(n, limit=64):
    """all 2^n patterns of +-1, or (n large) `limit` of them: all plus, all minus, and those whose halves repeat or oppose"""
    if (1 << n) <= limit:
        return [[1 if (p >> i) & 1 == 0 else -1 for i in range(n)] for p in range(1 << n)]
    h = n // 2
    out = []
    for p in range(1 << h):
        first = [1 if (p >> i) & 1 == 0 else -1 for i in range(h)]
        out += [first + first, first + [-s for s in first]]
    return out[:limit]


NR = 12


def part_sets(kinds, tag):
    """kinds: the kind of every 14-limb part of an item, in order -> [(set tag, [parts])]"""
    rnd = _rnd(tag)
    out = [("random/%d" % i, [rnd_part(k, rnd) for k in kinds]) for i in range(NR)]
    sp = [specials(k) for k in kinds]
    for j in range(max(len(s) for s in sp)):
        picks = [s[(j + 3 * m) % len(s)] for m, s in enumerate(sp)]
        out.append(("special/%d/%s" % (j, picks[0][0]), [x for _, x in picks]))
    for pat in sign_patterns(len(kinds)):
        out.append(("extreme/" + "".join("+" if s > 0 else "-" for s in pat), [ext_part(k, s) for k, s in zip(kinds, pat)]))
    return out


# ---- the ops of the device library -------------------------------------------------------------------------------------------
class Op:
    def __init__(self, name, code, win, wout, lanes, kinds, model, value=None):
        self.name, self.code, self.win, self.wout, self.lanes = name, code, win, wout, lanes
        self.kinds, self.model, self.value = kinds, model, value
        self.sets = []                                 # (tag, words in, expected words out, parts)

    def add(self, tag, parts, extra=()):
        words = [d for x in parts for d in x] + list(extra)
        _peak[0] = 0
        want = [int(w) for w in self.model(parts, list(extra))]
        PEAK.setdefault(self.name, {})[tag] = _peak[0]
        assert len(words) == self.win and len(want) == self.wout, (self.name, tag, len(words), len(want))
        assert all(-(1 << 31) <= w < (1 << 31) for w in words + want), (self.name, tag)
        self.sets.append((tag, words, want, parts))

    @property
    def counts(self):
        return {2: N_PAIR_ITEMS, 4: N_QUAD_ITEMS, 6: N_TEAM_ITEMS}[self.lanes]


def pairs_of(parts):
    return [(parts[2 * i], parts[2 * i + 1]) for i in range(len(parts) // 2)]


def flat2(*vals):
    return [d for v in vals for part in v for d in part]


def _pair_ops(o):
    S = lambda m, n=1: [m] * (2 * n)
    specs = (
        ("MUL_XI", 0, S(1), lambda v, k: p_mul_xi(v[0]), lambda r, k: LM.xi2(r[0])),
        ("B3", 1, S(1), lambda v, k: p_b3(v[0]), lambda r, k: LM.scl2(LM.xi2(r[0]), 12)),
        ("MUL_31", 2, S(3) + S(1), lambda v, k: p_mul(v[0], v[1]), "mul"),
        ("MUL_11", 3, S(1, 2), lambda v, k: p_mul(v[0], v[1]), "mul"),
        ("DOT2_1111", 4, S(1, 4), lambda v, k: p_dot2(*v), "dot2"),
        ("SQR_H", 5, S(1), lambda v, k: p_sqr(v[0]), "sqr"),
        ("SQR_HN2", 6, ["hn"] * 4, lambda v, k: p_sqr(p_add(v[0], v[1])), "sqrsum"),
        ("SQR_M12SQR", 7, S(1, 2), lambda v, k: p_sqr_m12sqr(v[0], v[1]), "m12"),
        ("MULF_1", 8, S(1) + ["fe"], lambda v, k: p_mulf(v[0], k), "mulf"),
        ("MULF_3", 9, S(3) + ["fe"], lambda v, k: p_mulf(v[0], k), "mulf"),
        ("NORM_2", 10, S(2), lambda v, k: p_norm(v[0]), lambda r, k: r[0]),
        ("NORM_4", 11, S(4), lambda v, k: p_norm(v[0]), lambda r, k: r[0]),
        ("MULC_NORM_4_S3", 12, S(3), lambda v, k: p_mulc_norm(4, v[0]), lambda r, k: LM.scl2(r[0], 4)),
        ("MULC_NORM_3_S2", 13, S(2), lambda v, k: p_mulc_norm(3, v[0]), lambda r, k: LM.scl2(r[0], 3)),
        ("MULC_NORM_12_S2", 14, S(2), lambda v, k: p_mulc_norm(12, v[0]), lambda r, k: LM.scl2(r[0], 12)),
        ("MULC_NORM_N12_S2", 15, S(2), lambda v, k: p_mulc_norm(-12, v[0]), lambda r, k: LM.scl2(r[0], -12)),
    )
    for name, code, kinds, fn, value in specs:
        nv = len(kinds) // 2

        def model(parts, extra, fn=fn, nv=nv):
            return flat2(fn(pairs_of(parts[:2 * nv]), parts[2 * nv] if len(parts) > 2 * nv else None))
        op = o[name] = Op(name, code, len(kinds) * L, V2, 2, kinds, model, value)
        for tag, parts in part_sets(kinds, name):
            op.add(tag, parts)
    # is_zero2: the flag of either lane
    op = o["IS_ZERO2"] = Op("IS_ZERO2", 16, V2, 2, 2, ["hn"] * 2, lambda parts, extra: [p_is_zero2(parts)] * 2)
    zs, near = [to_limbs(0), to_limbs(Q)], [to_limbs(1), to_limbs(Q - 1), to_limbs(Q + 1), to_limbs(-1), [0] * 13 + [1],
                                            to_limbs(Q)[:13] + [QT - 1], to_limbs(2 * Q - 1), [MASK] * 13 + [0]]
    for i, a in enumerate(zs + near):
        for j, b in enumerate(zs + near[:4]):
            op.add("special/%d/%d" % (i, j), [a, b])
    rnd = _rnd("IS_ZERO2")
    for i in range(NR):
        op.add("random/%d" % i, [rnd_part("hn", rnd), rnd_part("hn", rnd)])
    # load_part x 3, store_part for the coefficients 0, 1, 2
    def ls_model(parts, extra):
        return [d for c in range(6) for d in load_part(extra[12 * c:12 * c + 12])]
    op = o["LOAD_STORE"] = Op("LOAD_STORE", 17, 72, REC, 2, [], ls_model)
    rnd = _rnd("LOAD_STORE")
    coords = [0, 1, Q - 1, Q, Q + 1, 2 * Q - 1, (1 << 384) - 1, 1 << 383, int("5" * 96, 16), int("a" * 96, 16), R % Q, (1 << 384) - (1 << 32)]
    for i in range(NR):
        op.add("random/%d" % i, [], [w for _ in range(6) for w in be_words(rnd.randrange(Q))])
    for j in range(len(coords)):
        op.add("special/%d" % j, [], [w for c in range(6) for w in be_words(coords[(j + 5 * c) % len(coords)])])


STEP_KINDS = ["hn"] * 6 + ["px3n", "fe"] + ["hn"] * 4      # X, Y, Z, -3 px, py, xq, yq


def step_parts(tag):
    """the sets of a step: random points' worth of values, the special values, and digits all 0 / all 2^28 - 1 in every pattern
    of the six parts of X, Y, Z (the slab at 2^28 - 1, then at 0)"""
    rnd = _rnd(tag)
    out = [("random/%d" % i, [rnd_part(k, rnd) for k in STEP_KINDS]) for i in range(NR)]
    sp = [specials(k) for k in STEP_KINDS]
    for j in range(9):
        picks = [s[(j + 3 * m) % len(s)] for m, s in enumerate(sp)]
        out.append(("special/%d/%s" % (j, picks[0][0]), [x for _, x in picks]))
    for pat in sign_patterns(6):
        slab = 1 if pat[0] > 0 or pat[3] > 0 else -1
        out.append(("extreme/" + "".join("+" if s > 0 else "-" for s in pat) + ("/slab+" if slab > 0 else "/slab-"),
                    [ext_part("hn", s) for s in pat] + [ext_part(k, slab) for k in STEP_KINDS[6:]]))
    return out


def _step_ops(o):
    def tangent_model(fn, both):
        def model(parts, extra):
            X, Y, Z = pairs_of(parts[:6])
            X3, Y3, Z3, rec = fn(X, Y, Z, parts[6], parts[7])
            return flat2(X3, Y3, Z3) + rec + (flat2(X3, Y3, Z3) if both else [])
        return model

    def chord_model(parts, extra):
        X, Y, Z = pairs_of(parts[:6])
        xq, yq = pairs_of(parts[8:12])
        X3, Y3, Z3, rec = sp_chord(X, Y, Z, parts[6], parts[7], xq, yq)
        return flat2(X3, Y3, Z3) + rec
    for name, code, lanes, wout, model in (("SP_TANGENT", 18, 2, 3 * V2 + REC, tangent_model(sp_tangent, False)),
                                           ("SP_CHORD", 19, 2, 3 * V2 + REC, chord_model),
                                           ("SQ_TANGENT", 32, 4, 6 * V2 + REC, tangent_model(sq_tangent, True))):
        op = o[name] = Op(name, code, 12 * L, wout, lanes, STEP_KINDS, model)
        for tag, parts in step_parts("SP_CHORD" if name == "SP_CHORD" else "TANGENT"):     # (both tangent forms run the same sets)
            op.add(tag, parts)


def _quad_ops(o):
    op = o["OTH"] = Op("OTH", 30, 2 * V2, 2 * V2, 4, [1] * 4, lambda parts, extra: [d for x in parts[2:4] + parts[0:2] for d in x])
    for tag, parts in part_sets([1] * 4, "OTH")[:NR + 8]:
        op.add(tag, parts)
    # (a, b) of pair 0, (a, b) of pair 1 -> pair 0's a, pair 1's b
    op = o["PICK"] = Op("PICK", 31, 4 * V2, 2 * V2, 4, [1] * 8, lambda parts, extra: [d for x in parts[0:2] + parts[6:8] for d in x])
    for tag, parts in part_sets([1] * 8, "PICK")[:NR + 8]:
        op.add(tag, parts)


def team_of(parts):
    return pairs_of(parts[:12])


def team_sets(tag, extra_kinds=()):
    """f (six lanes, all different in the random and special sets) and further parts"""
    kinds = ["f"] * 12 + list(extra_kinds)
    rnd = _rnd(tag)
    out = [("random/%d" % i, [rnd_part(k, rnd) for k in kinds]) for i in range(NR)]
    sp = [specials(k) for k in kinds]
    for j in range(9):
        picks = [s[(j + 2 * m) % len(s)] for m, s in enumerate(sp)]
        out.append(("special/%d/%s" % (j, picks[0][0]), [x for _, x in picks]))
    return kinds, out


def team_extremes(extra_kinds, extra_patterns):
    """f: every lane's (re, im) at (2^28 - 1 or 0) in the patterns ++, +-, -+ and alternating by lane; the further parts by pattern"""
    out = []
    fpats = {"f++": lambda c: (1, 1), "f+-": lambda c: (1, -1), "f-+": lambda c: (-1, 1), "falt": lambda c: (1, -1) if c % 2 else (-1, 1)}
    for fname, fp in fpats.items():
        f = [ext_part("f", s) for c in range(6) for s in fp(c)]
        for pname, pat in extra_patterns:
            out.append(("extreme/%s/%s" % (fname, pname), f + [ext_part(k, s) for k, s in zip(extra_kinds, pat)]))
    return out


def _team_ops(o):
    flat_team = lambda t: [d for re, im in t for d in re + im]
    kinds, base = team_sets("TEAM")
    ones = [("extreme/ones", [ext_part("f", 1)] * 12), ("extreme/zeros", [ext_part("f", -1)] * 12)]

    def simple(name, code, wout, fn):
        op = o[name] = Op(name, code, TV, wout, 6, kinds, lambda parts, extra: fn(team_of(parts)))
        for tag, parts in base + ones:
            op.add(tag, parts)
    one = [(to_limbs(ONE), [0] * L)] + [([0] * L, [0] * L)] * 5
    simple("SET_ONE", 40, TV, lambda f: flat_team(one))
    pub_words = lambda P: [d for p in P for k in ("re", "im", "nim", "xre", "xim", "nxim") for d in p[k]]
    simple("PUBLISH_RAW", 41, 3 * TV, lambda f: pub_words(publish(f, False)))
    simple("PUBLISH_NORM", 42, 3 * TV, lambda f: pub_words(publish(f, True)))
    for J in range(6):
        def fetched(f, J=J):
            P = publish(f, True)
            return [d for c in range(6) for k in ("re", "im", "nim") for d in fetch(P, c, J)[k]]
        simple("FETCH_%d" % J, 43 + J, 18 * L, fetched)

    def f2rt(parts, extra):
        P = publish(team_of(parts), False)
        return [d for c in range(6) for k in ("re", "im") for d in fetch(P, c, extra[0])[k]]
    op = o["FETCH2_RT"] = Op("FETCH2_RT", 49, TV + 1, TV, 6, kinds, f2rt)
    for i, (tag, parts) in enumerate(base + ones):
        for J in ((2, 3, 4, 5) if i < 4 or tag.startswith("extreme") else (2 + i % 4,)):
            op.add("%s/J%d" % (tag, J), parts, [J])
    # mul3: y0, y1, y2 of a dense record (digits)
    ykinds = ["f"] * 6
    k3, base3 = team_sets("MUL3", ykinds)
    ypats = [("y+", [1] * 6), ("yre", [1, -1] * 3), ("yim", [-1, 1] * 3), ("y0", [1, 1, -1, -1, -1, -1]), ("y12", [-1, -1, 1, 1, 1, 1])]
    for name, code, Js, norm in (("MUL3_012", 50, (0, 1, 2), True), ("MUL3_345", 51, (3, 4, 5), True), ("MUL3_012_RAW", 52, (0, 1, 2), False)):
        def m3(parts, extra, Js=Js, norm=norm):
            return flat_team(mul3(publish(team_of(parts), norm), Js, pairs_of(parts[12:18])))
        op = o[name] = Op(name, code, TV + 3 * V2, TV, 6, k3, m3)
        op.Js = Js
        for tag, parts in base3 + team_extremes(ykinds, ypats):
            op.add(tag, parts)
    # mul_line_k3: the record's six parts, then jA, jB
    lkinds = ["l0", "l0", "hn", "hn", "hn", "hn"]
    kl, basel = team_sets("TEAM_LINE", lkinds)
    lpats = [("l+", [1] * 6), ("l-", [-1, -1, 1, 1, 1, 1]), ("l-re", [-1, 1, 1, -1, 1, -1]), ("l0only", [1, 1, -1, -1, -1, -1]),
             ("p3", [1, 1, 1, -1, 1, -1]), ("p3n", [-1, -1, 1, -1, 1, -1]), ("p2", [-1, 1, -1, 1, -1, 1])]

    def line_model(parts, extra):
        return flat_team(mul_line_k3(team_of(parts), extra[0], extra[1], parts[12:18]))
    op = o["TEAM_LINE"] = Op("TEAM_LINE", 53, TV + REC + 2, TV, 6, kl, line_model)
    for i, (tag, parts) in enumerate(basel + team_extremes(lkinds, lpats)):
        for pos in (POSITIONS if i < 4 or tag.startswith("extreme") else (POSITIONS[i % 3],)):
            op.add("%s/pos%d%d" % (tag, pos[0], pos[1]), parts, list(pos))
    # the exact kernel's records: coefficient 0 in Fq (imaginary part zeros), and the line "1" of a team past its last pair
    rnd = _rnd("TEAM_LINE/exact")
    for pos in POSITIONS:
        f = [rnd_part("f", rnd) for _ in range(12)]
        op.add("special/exact-record/pos%d%d" % pos, f + [rnd_part("hn", rnd), [0] * L] + [rnd_part("hn", rnd) for _ in range(4)], list(pos))
        op.add("special/line-one/pos%d%d" % pos, f + [to_limbs(ONE)] + [[0] * L] * 5, list(pos))
    # mul_dense
    gk = ["f"] * 12
    kd, based = team_sets("TEAM_DENSE", gk)
    gpats = [("g+", [1] * 12), ("gre", [1, -1] * 6), ("gim", [-1, 1] * 6), ("galt", [1, 1, -1, -1] * 3)]

    def dense_model(parts, extra):
        return flat_team(mul_dense(team_of(parts), pairs_of(parts[12:24])))
    for name, code in (("TEAM_DENSE", 54), ("TEAM_TEAMREC", 56)):
        op = o[name] = Op(name, code, 2 * TV, TV, 6, kd, dense_model)
        for tag, parts in based + team_extremes(gk, gpats):
            op.add(tag, parts)
    op = o["TEAM_SQUARE"] = Op("TEAM_SQUARE", 55, TV, TV, 6, kinds, lambda parts, extra: flat_team(mul_dense(team_of(parts), team_of(parts))))
    for tag, parts in base + team_extremes([], [("sq", [])]):
        op.add(tag, parts)


_OPS = None


def ops():
    """name -> Op, built once (the expected words are the limb model's)"""
    global _OPS
    if _OPS is None:
        o = {}
        _pair_ops(o)
        _step_ops(o)
        _quad_ops(o)
        _team_ops(o)
        assert len({op.code for op in o.values()}) == len(o)
        _OPS = o
    return _OPS


GROUPS = {"pair": lambda op: op.lanes == 2 and op.code < 18, "steps": lambda op: op.code in (18, 19, 32),
          "quad": lambda op: op.code in (30, 31), "team": lambda op: op.lanes == 6}


def call_sets(op, n, base=0):
    """the set of every item of a call of n items: item i is the same set in every call (base: where a further call goes on)"""
    return [(base + i) % len(op.sets) for i in range(n)]


def summary():
    """per group: ops, sets, the largest column reached as a fraction of 2^63"""
    out = {}
    for g, sel in GROUPS.items():
        sel_ops = [op for op in ops().values() if sel(op)]
        peak = max((max(PEAK[op.name].values()) for op in sel_ops), default=0)
        out[g] = (len(sel_ops), sum(len(op.sets) for op in sel_ops), peak / float(1 << 63))
    return out


if __name__ == "__main__":
    for g, (n, s, p) in summary().items():
        print("%-6s %2d ops %4d sets  largest column %.4f x 2^63" % (g, n, s, p))
    for name in BOUND:
        tag, pk = max(PEAK[name].items(), key=lambda kv: kv[1])
        print("  %-14s claimed %d units: peak %.3f units of 13 x 2^56 (%.4f x 2^63) on %s" % (name, BOUND[name], pk / (13.0 * (1 << 56)), pk / float(1 << 63), tag))
