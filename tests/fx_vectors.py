"""Operand sets and a limb-exact integer model of the routines of csrc/blsgpu_fexp.hip, namespace fx -- the steps of k_fexp_team, the
six-lanes-per-result final exponentiation --, one list per op of the test-only device library csrc/blsgpu_fx_check.hip.  Pure Python:
tests/test_fx_vectors_model.py checks the model against plain integers mod q (vmgen/fexp_model.py) on the CPU, tests/test_gpu_fx.py
compares the compiled routines with it word for word.

The model adds no reduction of its own: fp28_dot2 / fp28_dot3 are ml_vectors.dot (fp28_vectors.dot with the 64-bit accumulator asserted,
noting the largest column), the carry passes fp28_vectors' l_norm etc., the dense product ml_vectors.mul_dense.  cyc_sqr, frob, tinv,
fq_inverse and the kernel's inline CONJ are transcribed line by line; reduce_small's estimate is repeated in IEEE single precision
with numpy.float32 (the reciprocal formed in single precision, one rounded multiply, rint to even).

The INDEPENDENT reference of every set (its fifth entry) never uses that estimate, the C oracle or the code under test: plain Python
integers on the words it is handed -- the device's own in tests/test_gpu_fx.py.

CONTRACT (per op: what its call sites in k_fexp_team deliver, script_sites() derives which from vmgen/fexp_model.script(); what it returns):
  kind    limbs 0 .. 12          value
  fe      digits [0, 2^28)       (-q, 2q)     a product's output: from_vm, frob, tinv, fq_inverse
  small   digits                 (-2q, 2q)    reduce_small's output as the comment at it claims (the sets reach |v| < 0.51 q, SMALL_SEEN)
  dense   digits                 (-2q, 4q)    mul_dense's output
  acc     digits                 (-4q, 4q)    CONJ of a dense value: norm(-x) lies in (-4q, 2q); the hull of what MUL / ST meet
  rs      (-2^29, 5 x 2^28)      (-11q, 14q)  3 t -+ 2 f, t fe, f dense: 3 (-q, 2q) - 2 (-2q, 4q) = (-11q, 10q), + gives (-7q, 14q)
  rsclaim (-2^29, 5 x 2^28)      |x| < 2^12 q the range reduce_small's comment claims for itself
  REDUCE_SMALL rs -> small | CYC_SQR dense -> small | FROB dense -> fe | TINV dense -> fe (lanes 1 .. 5 zero) | FQ_INVERSE fe -> fe |
  CONJ dense -> acc | SLOT_ROUNDTRIP acc, acc -> dense
Every operand of every set is asserted to lie in the contract it claims when it is added (Op.add), every result of every chain step in
the operand contract of the next step (chain_steps).

Set classes (the tag's prefix): random; special (0, R, -1, q - 1, q, all digits 0 / 2^28 - 1 with the top digit at both ends of the
contract; the negated limbs of q where limbs are signed: REDUCE_SMALL); subfield (Fq2, Fq6, w^k, the cyclotomic subgroup, the limb forms
of 1); extreme (digits 0 / 2^28 - 1 in all 16 patterns of (xr, xi, yr, yi), every pattern on every pair and so on every lane role).
Lanes of a wavefront differ because item i of a call is set i: a zero team stands beside non-zero ones.

Columns (units of 2^56 per limb product, 13 products to a full column): the comment in cyc_sqr counts |a||b| per term, "real 2 + 1 + 2,
imaginary 2 + 4 + 2 = 8 on even lanes; 2 + 4 on lane 1".  With digits in [0, 2^28) the terms are NOT independent: on an even lane the
imaginary column is 2 xr xi + (yr + yi)^2 - 2 yi^2 = 2 xr xi + yr^2 + 2 yr yi - yi^2 <= 2 + 1 + 2 - 1 = 4 units (all four parts at
2^28 - 1), the real one xr^2 - xi^2 + (yr - yi)^2 - 2 yi^2 lies in [-3, 2]; lane 1 has 2 xr (yr - yi) - 2 xi (yr + yi) in [-4, 2] and
2 xr (yr + yi) + 2 xi (yr - yi) <= 4; lanes 3, 5 reach 2 and 4.  So 4.000 of the 8 a column holds is the attainable figure
(BOUND), met by extreme sets only.
"""
import json
import os
import random

import numpy as np

from vmgen import fexp_model as F
from vmgen import gen_fp28 as G
from vmgen import linestream_model as LM
from vmgen.gen_fexp import pow_windows
from fp28_vectors import l_add, l_sub, l_neg, l_norm, C_FROM_VM, C_TO_VM
import ml_vectors as MV

Q, R, L, W, MASK = G.Q, G.R, G.L, G.W, G.MASK
to_limbs, from_limbs = G.to_limbs, G.from_limbs
RINV = pow(R, -1, Q)
ONE = R % Q
V2, TV = 2 * L, 12 * L
SH = W * (L - 1)                                       # the top limb's weight: 2^364
FILL = -1431655766                                     # a word no lane stored: 0xAAAAAAAA
N_TEAM_ITEMS = (1, 9, 10, 11, 41)                      # ten teams per wavefront, forty per workgroup
N_LANE_ITEMS = (1, 63, 64, 65, 257)
MAX_CHAIN = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MUT = set()                                            # mutants of the model that are switched on (tests/test_fx_vectors_model.py)
dot = MV.dot

KINDS = {"fe": (-Q, 2 * Q), "small": (-2 * Q, 2 * Q), "dense": (-2 * Q, 4 * Q), "acc": (-4 * Q, 4 * Q),
         "rs": (-11 * Q, 14 * Q), "rsclaim": (-(Q << 12), Q << 12)}
RS_LO, RS_HI = -(1 << 29), 5 << 28                     # limbs 0 .. 12 of 3 t -+ 2 f, exclusive
CONTRACT = {"REDUCE_SMALL": ("rs", "small"), "CYC_SQR": ("dense", "small"), "CYC_SQR_CHAIN": ("dense", "small"), "FROB": ("dense", "fe"),
            "TINV": ("dense", "fe"), "FQ_INVERSE": ("fe", "fe"), "CONJ": ("dense", "acc"), "SLOT_ROUNDTRIP": ("acc", "dense")}
BOUND = {"CYC_SQR": 4, "FROB": 2, "TINV": 2, "SLOT_ROUNDTRIP": 6}     # units of 2^56 (module docstring; FROB, TINV: a dot2 of digits)
CLAIMED = {"CYC_SQR": 8}                               # the comment's count of |a||b|
PEAK = {}                                              # op -> {set tag: largest |column sum| of its products}
SMALL_SEEN = [0]                                       # the largest |value| reduce_small's model returned, over everything built


def in_kind(kind, x):
    lo, hi = KINDS[kind]
    if kind in ("rs", "rsclaim"):
        return all(RS_LO < d < RS_HI for d in x[:13]) and lo < from_limbs(x) < hi and -(1 << 31) <= x[13] < (1 << 31)
    return all(0 <= d <= MASK for d in x[:13]) and lo < from_limbs(x) < hi


# ---- the limb model --------------------------------------------------------------------------------------------------------
RECIP = np.float32(1.0) / np.float32(106513.12)        # 1.0f / 106513.12f, folded in single precision


def rs_estimate(top):
    """(int32_t)rintf((float)top * (1.0f / 106513.12f)): the int -> float conversion rounds to nearest even, one rounded product"""
    p = np.float32(top) * RECIP
    assert p.dtype == np.float32
    if "rs_floor" in MUT:
        return int(np.floor(p))
    return int(np.rint(p)) + (1 if "rs_k_plus_1" in MUT else 0)


def reduce_small(x):
    k = rs_estimate(x[L - 1])
    r = to_limbs(from_limbs(x) - k * Q)                # the 64-bit carry chain of x_j - k n_j: exact
    MV.top32(r)
    SMALL_SEEN[0] = max(SMALL_SEEN[0], abs(from_limbs(r)))
    return r


def cyc_sqr(f):
    """f: six (re, im) of 14 limbs -> the same after fx::cyc_sqr, lane by lane"""
    out = []
    for c in range(6):
        pair = 0 if c in (0, 3) else (1 if c in (2, 5) else 2)
        if "pair_swapped" in MUT:                          # the entries of lanes 1, 4 and of lanes 2, 5 exchanged
            pair = (0, 1, 2, 0, 1, 2)[c]
        (xr, xi), (yr, yi) = f[pair], f[pair + 3]
        ev, l1 = c % 2 == 0, c == 1
        if "lane1_no_xi" in MUT:
            l1 = False
        xs, xd, ys, yd = l_add(xr, xi), l_sub(xr, xi), l_add(yr, yi), l_sub(yr, yi)
        x2i, x2r = l_add(xi, xi), l_add(xr, xr)
        a1r = xs if ev else x2r
        b1r = xd if ev else (yd if l1 else yr)
        a2r = yd if ev else l_neg(x2i)
        b2r = yd if ev else (ys if l1 else yi)
        a3on = (not ev) if "a3_odd" in MUT else ev
        a3 = l_neg(l_add(yi, yi)) if a3on else [0] * L
        b1i = xi if ev else (ys if l1 else yi)
        a2i = ys if ev else x2i
        b2i = ys if ev else (yd if l1 else yr)
        tr = dot([(a1r, b1r), (a2r, b2r), (a3, yi)])
        ti = dot([(x2r, b1i), (a2i, b2i), (a3, yi)])
        m = 1 if "no_3x" in MUT else 3
        minus = (not ev) if "parity" in MUT else ev
        fre, fim = f[c]
        sr = [m * t + (-2 * d if minus else 2 * d) for t, d in zip(tr, fre)]
        si = [m * t + (-2 * d if minus else 2 * d) for t, d in zip(ti, fim)]
        out.append((reduce_small(sr), reduce_small(si)))
    return out


GAMMA_LIMBS = {j3: [(to_limbs(g[0] * R % Q), to_limbs(g[1] * R % Q)) for g in F.GAMMA[i]] for j3, i in enumerate(F.FROB_POW)}


def frob(f, j3):
    cj = j3 == 0
    if "frob_conj_q2" in MUT:
        cj = j3 in (0, 1)
    out = []
    for c in range(6):
        gr, gi = GAMMA_LIMBS[j3][5 - c if "frob_gamma_rev" in MUT else c]
        fre, fim = f[c]
        xim, nxim = (l_neg(fim), list(fim)) if cj else (list(fim), l_neg(fim))
        out.append((dot([(fre, gr), (nxim, gi)]), dot([(fre, gi), (xim, gr)])))
    return out


INV_WIN = pow_windows(Q - 2)                           # the schedule of fexp_tables_gfx950.h


def fq_inverse(b):
    """a^(q-2) on limbs (r28::sqr and r28::mul are fp28 products of one term)"""
    b2 = dot([(b, b)])
    tbl = [list(b)]
    for i in range(1, 4):
        tbl.append(dot([(tbl[i - 1], b2)]))
    a = tbl[INV_WIN[0][1]]
    for nsq, k in INV_WIN[1:]:
        for _ in range(nsq):
            a = dot([(a, a)])
        if k != 255:
            a = dot([(a, tbl[k])])
    return a


def vm_inverse(n):
    """to_vm, the VM's fq_inv (0 -> 0, the result canonical), from_vm: 1/n in the limb form, up to the factor 2^8 of the forms"""
    w = from_limbs(n) * C_TO_VM * RINV % Q
    v = pow(w, -1, Q) * (1 << 768) % Q if w else 0
    if "tinv_no_zero" in MUT and not w:
        v = 1
    return dot([(to_limbs(v), to_limbs(C_FROM_VM))])


def tinv(f):
    """every lane runs it on its own words; lane 0's survives"""
    re, im = f[0]
    n = dot([(re, re), (im, im)])
    ni = vm_inverse(n)
    a, b = dot([(re, ni)]), dot([(l_neg(im), ni)])
    if "tinv_leaves_lanes" in MUT:
        return [(a, b)] + [(list(x), list(y)) for x, y in f[1:]]
    return [(a, b)] + [([0] * L, [0] * L)] * 5


def conj(f):
    """the kernel's inline op 5: odd coefficients negated, then the carry pass on every lane"""
    odd = 0 if "conj_even" in MUT else 1
    return [(MV.top32(l_norm(l_neg(re) if c % 2 == odd else re)), MV.top32(l_norm(l_neg(im) if c % 2 == odd else im))) for c, (re, im) in enumerate(f)]


mul_dense = MV.mul_dense


# ---- values behind the limbs -------------------------------------------------------------------------------------------------
def res(x): return from_limbs(x) * RINV % Q
def res6(f): return [(res(re), res(im)) for re, im in f]
def team_of(words): return [(list(words[c * V2:c * V2 + L]), list(words[c * V2 + L:c * V2 + V2])) for c in range(6)]
def flat_team(f): return [d for re, im in f for d in list(re) + list(im)]
def is_zero_team(words): return all(w == 0 for w in words)


def mont(v, rep=0):
    """residue -> limbs of v R + rep q"""
    return to_limbs(v * R % Q + rep * Q)


def team_mont(vals, reps=None):
    return [(mont(a, (reps or [0] * 12)[2 * c]), mont(b, (reps or [0] * 12)[2 * c + 1])) for c, (a, b) in enumerate(vals)]


def digits_ok(f, kind):
    assert all(in_kind(kind, part) for v in f for part in v), "a result leaves the %s contract" % kind


# ---- the independent checks: plain integers on the words handed in ------------------------------------------------------------
NEAREST = Q // 2 + Q // 512


def nearest_ok(v):
    """reduce_small subtracts "the multiple of q nearest to x": |result| <= q / 2 plus what the estimate may be off by -- the lower
    limbs (< 1e-4, the comment at the routine) and three single-precision roundings of a quotient below 2^12 (3 x 2^-24 x 2^12 < 2^-10):
    less than q / 512 together.  Derived from the routine's own statement, not from its output; far inside the claimed (-2q, 2q)"""
    return abs(v) < NEAREST


def chk_reduce(x):
    def chk(out):
        v = from_limbs(out)
        assert (v - from_limbs(x)) % Q == 0, "not the operand mod q"
        assert all(0 <= d <= MASK for d in out[:13]), "limbs 0..12 leave [0, 2^28)"
        assert -2 * Q < v < 2 * Q, "value leaves (-2q, 2q)"
        assert nearest_ok(v), "not the nearest multiple of q"
    return chk


def _steps_check(f0, steps, n_done):
    """steps: [(team words, number of squarings)]"""
    want, k = res6(f0), 0
    for words, n in sorted(steps, key=lambda s: s[1]):
        while k < n:
            want, k = F.cyc_sqr_lane_forms(want), k + 1
        g = team_of(words)
        assert res6(g) == want, "not the lane forms of vmgen/fexp_model after %d squarings" % n
        if n:
            digits_ok(g, "small")
            assert all(nearest_ok(from_limbs(p)) for p in parts_of(g)), "a part is not reduced by the nearest multiple of q"


def chk_cyc(f, cyclotomic):
    def chk(out):
        _steps_check(f, [(out, 1)], 1)
        if cyclotomic:
            assert res6(team_of(out)) == LM.mul_dense(res6(f), res6(f)), "not f^2 in the cyclotomic subgroup"
    return chk


def chk_chain(f, n):
    def chk(out):
        steps = [(out[:TV], n)]
        for i in (1, 2):
            if n >= i:
                steps.append((out[i * TV:(i + 1) * TV], i))
            else:
                assert out[i * TV:(i + 1) * TV] == [FILL] * TV, "step %d stored although n = %d" % (i, n)
        _steps_check(f, steps, n)
    return chk


def chk_frob(f, j3):
    def chk(out):
        g = team_of(out)
        assert res6(g) == F.frob(res6(f), F.FROB_POW[j3]), "not f^(q^%d)" % F.FROB_POW[j3]
        digits_ok(g, "fe")
    return chk


def chk_tinv(f):
    def chk(out):
        tr, ti = res6(f)[0]
        n = (tr * tr + ti * ti) % Q
        ni = pow(n, -1, Q) if n else 0
        g = team_of(out)
        assert res6(g)[0] == (tr * ni % Q, -ti * ni % Q), "not conj(t) / (tr^2 + ti^2)"
        assert out[V2:] == [0] * (TV - V2), "lanes 1..5 are not zero words"
        digits_ok(g[:1], "fe")
    return chk


def chk_fq_inverse(a):
    def chk(out):
        va, vo = from_limbs(a) % Q, from_limbs(out) % Q
        assert (va * vo - R * R) % Q == 0 if va else vo == 0, "a out != R^2 (mod q)"
        assert in_kind("fe", out), "leaves the fe contract"
    return chk


def chk_conj(f):
    def chk(out):
        g = team_of(out)
        assert res6(g) == F.conj6(res6(f)), "not conj(f)"
        digits_ok(g, "acc")
        for c in range(6):                                   # the carry pass keeps the VALUE, not only the residue
            for p in range(2):
                assert from_limbs(g[c][p]) == (-1 if c % 2 else 1) * from_limbs(f[c][p]), "value changed"
    return chk


def chk_slot(f, g):
    def chk(out):
        h = team_of(out)
        assert res6(h) == LM.mul_dense(res6(f), res6(g)), "not f g"
        digits_ok(h, "dense")
    return chk


# ---- operands ------------------------------------------------------------------------------------------------------------------
def _rnd(tag):
    return random.Random("fx:" + tag)


def top_ends(kind):
    """(lowest top digit with digits all 0, highest top digit with digits all 2^28 - 1) inside the contract"""
    lo, hi = KINDS[kind]
    t_lo = -((-lo) >> SH)
    while not in_kind(kind, [0] * 13 + [t_lo]):
        t_lo += 1
    t_hi = hi >> SH
    while not in_kind(kind, [MASK] * 13 + [t_hi]):
        t_hi -= 1
    return t_lo, t_hi


def specials(kind):
    t_lo, t_hi = top_ends(kind)
    out = [("0", to_limbs(0)), ("R", to_limbs(ONE)), ("-1", to_limbs(-1)), ("q-1", to_limbs(Q - 1)), ("q", to_limbs(Q)),
           ("zeros/top-", [0] * 13 + [t_lo]), ("zeros/top+", [0] * 13 + [t_hi]), ("ones/top-", [MASK] * 13 + [t_lo]),
           ("ones/top+", [MASK] * 13 + [t_hi]), ("ones", [MASK] * 13 + [0])]
    assert all(in_kind(kind, x) for _, x in out), kind
    return out


def rnd_part(kind, rnd):
    lo, hi = KINDS[kind]
    return to_limbs(rnd.randrange(lo + 1, hi))


def rnd_val(rnd):
    return [(rnd.randrange(Q), rnd.randrange(Q)) for _ in range(6)]


def cyclotomic_of(f):
    """f^((q^6 - 1)(q^2 + 1)): the model's own t"""
    t = F.mul_dense(F.conj6(f), F.inverse(f))
    return F.mul_dense(F.frob(t, 2), t)


def golden_cyclotomic():
    with open(os.path.join(GOLDEN, "pairing.json")) as fh:
        g = json.load(fh)
    outs = [g["gen"]["final_exp"]] + [r["out"] for r in g["final_exp"]]
    ints = lambda b: [int.from_bytes(b[48 * i:48 * (i + 1)], "big") for i in range(12)]
    return [F.from_flat12(ints(bytes.fromhex(h))) for h in outs]


def golden_inputs():
    with open(os.path.join(GOLDEN, "pairing.json")) as fh:
        g = json.load(fh)
    ins = [g["gen"]["miller"]] + [r["in"] for r in g["final_exp"]]
    ints = lambda b: [int.from_bytes(b[48 * i:48 * (i + 1)], "big") for i in range(12)]
    return [F.from_flat12(ints(bytes.fromhex(h))) for h in ins]


def subfield_values(rnd):
    """(name, plain values, cyclotomic?)"""
    z = (0, 0)
    out = [("fq2", [(rnd.randrange(Q), rnd.randrange(Q))] + [z] * 5, False),
           ("fq6", [(rnd.randrange(Q), rnd.randrange(Q)) if k % 2 == 0 else z for k in range(6)], False)]
    for k in range(6):
        out.append(("w%d" % k, [(1, 0) if c == k else z for c in range(6)], k == 0))
    for i, v in enumerate(golden_cyclotomic()):
        out.append(("cyc/golden%d" % i, v, True))
    for i in range(2):
        out.append(("cyc/model%d" % i, cyclotomic_of(rnd_val(rnd)), True))
    return out


def extreme_teams():
    """all 16 patterns of (xr, xi, yr, yi) at 2^28 - 1 / 0; set p puts pattern (p + 5 j) mod 16 on pair j, so every pair (every lane
    role: pairs 0, 1 serve an even lane and lane 3 / 5, pair 2 serves lane 4 and lane 1) meets every pattern"""
    part = lambda on: [MASK if on else 0] * 13 + [0]
    out = []
    for p in range(16):
        f = [None] * 6
        name = []
        for j in range(3):
            pat = (p + 5 * j) % 16
            f[j] = (part(pat & 1), part(pat & 2))
            f[j + 3] = (part(pat & 4), part(pat & 8))
            name.append("%x" % pat)
        out.append(("extreme/" + "".join(name), f))
    return out


_ONE_FORMS = []


def one_chain():
    """the constant 1 (R on lane 0) under repeated cyc_sqr: the limb forms it passes through, in order, until one repeats"""
    if not _ONE_FORMS:
        forms, info = [], {}
        for rep in (0, 1, -1, 2, 3):                       # R + rep q on lane 0: every form of 1 the dense contract admits
            f = team_mont(LM.one6(), [rep] + [0] * 11)
            seen = []
            while flat_team(f) not in seen:
                seen.append(flat_team(f))
                f = cyc_sqr(f)
            back = seen.index(flat_team(f))
            info[rep] = (len(seen), back, len(seen) - back)   # forms met, the step the cycle starts at, the cycle's length
            forms += [w for w in seen if w not in forms]
        _ONE_FORMS.extend([forms, info])
    return _ONE_FORMS


def team_sets(tag, kind="dense", nr=8):
    """[(set tag, team, cyclotomic?)]"""
    rnd = _rnd(tag)
    out = [("random/%d" % i, [(rnd_part(kind, rnd), rnd_part(kind, rnd)) for _ in range(6)], False) for i in range(nr)]
    sp = specials(kind)
    for j in range(len(sp)):
        picks = [sp[(j + 3 * m) % len(sp)] for m in range(12)]
        out.append(("special/%d/%s" % (j, picks[0][0]), [(picks[2 * c][1], picks[2 * c + 1][1]) for c in range(6)], False))
    out.append(("special/zero-team", [([0] * L, [0] * L)] * 6, False))
    for name, vals, cyc in subfield_values(rnd):
        reps = [rnd.choice((0, 0, 1, -1)) for _ in range(12)]
        out.append(("subfield/" + name, team_mont(vals, reps), cyc))
    forms, _ = one_chain()
    for i, w in enumerate(forms):
        out.append(("subfield/one/form%d" % i, team_of(w), True))
    out += [(t, f, False) for t, f in extreme_teams()]
    return out


# ---- the ops of the device library -----------------------------------------------------------------------------------------------
class Op:
    def __init__(self, name, code, win, wout, lanes, model):
        self.name, self.code, self.win, self.wout, self.lanes, self.model = name, code, win, wout, lanes, model
        self.sets = []                                 # (tag, words in, expected words out, operand parts, independent check)

    def add(self, tag, words, parts, chk, kind=None):
        kind = kind or CONTRACT[self.name][0]
        assert all(in_kind(kind, x) for x in parts), (self.name, tag, "an operand leaves the %s contract" % kind)
        MV._peak[0] = 0
        want = [int(w) for w in self.model(words)]
        PEAK.setdefault(self.name, {})[tag] = MV._peak[0]
        assert len(words) == self.win and len(want) == self.wout, (self.name, tag, len(words), len(want))
        assert all(-(1 << 31) <= w < (1 << 31) for w in list(words) + want), (self.name, tag)
        self.sets.append((tag, [int(w) for w in words], want, parts, chk))

    @property
    def counts(self):
        return N_TEAM_ITEMS if self.lanes == 6 else N_LANE_ITEMS


def parts_of(f):
    return [p for v in f for p in v]


def rs_loose(x, m):
    """the same value with limbs 0 .. 12 moved by m 2^28 (m = 4: towards 5 x 2^28, m = -2: towards -2^29)"""
    d = to_limbs(x)
    ms = [m + 1 if m < 0 else m] + [m] * 12            # (limb 0 has no borrow to give back: one step less on the negative side)
    out = [d[0] + (ms[0] << W)] + [d[j] + (ms[j] << W) - ms[j - 1] for j in range(1, 13)] + [d[13] - ms[12]]
    assert from_limbs(out) == x
    return out


def rs_switch_points(kmax=16):
    """for every k in -kmax .. kmax - 1 the top limb t with estimate(t) = k and estimate(t + 1) = k + 1, found with the float32
    emulation by bisection (the estimate is monotone in t)"""
    out = []
    for k in range(-kmax, kmax):
        lo, hi = int((k + 0.25) * 106513.12), int((k + 0.75) * 106513.12) + 1
        if k < 0:
            lo, hi = int((k + 0.25) * 106513.12) - 1, int((k + 0.75) * 106513.12)
        assert rs_estimate(lo) == k and rs_estimate(hi) == k + 1, k
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if rs_estimate(mid) == k:
                lo = mid
            else:
                hi = mid
        out.append((k, lo))
    return out


def reduce_small_sets():
    """(tag, limbs, kind)"""
    out = []
    rnd = _rnd("REDUCE_SMALL")
    for i in range(16):
        t = rnd_part("fe", rnd)
        f = rnd_part("dense", rnd)
        sg = -2 if i % 2 else 2
        out.append(("random/%d" % i, [3 * a + sg * b for a, b in zip(t, f)], "rs"))
    for name, x in specials("small") + [("-q", l_neg(to_limbs(Q))), ("q-limbs-x3", [3 * d for d in to_limbs(Q)])]:
        out.append(("special/" + name, x, "rs"))
    ks = [0, 1, -1, 10, -10, 14, -14, 4095, -4095] + [s * (1 << e) for e in range(1, 12) for s in (1, -1)]
    deltas = [("0", 0), ("+1", 1), ("-1", -1), ("+h", (Q - 1) // 2), ("-h", -(Q - 1) // 2), ("h-", (Q - 1) // 2), ("h+", (Q + 1) // 2)]
    for k in ks:
        for dn, dv in deltas:
            x = k * Q + dv
            kind = "rs" if KINDS["rs"][0] < x < KINDS["rs"][1] else "rsclaim"
            if abs(x) >= Q << 12:
                continue
            out.append(("multiple/k%d%s/tight" % (k, dn), to_limbs(x), kind))
            if dn in ("0", "+h", "-h", "h+"):
                out.append(("multiple/k%d%s/hi" % (k, dn), rs_loose(x, 4), kind))
                out.append(("multiple/k%d%s/lo" % (k, dn), rs_loose(x, -2), kind))
    for k, t in rs_switch_points():
        for dt in (0, 1):
            for ln, lower in (("zeros", [0] * 13), ("ones", [MASK] * 13), ("hi", [RS_HI - 1] * 13), ("lo", [RS_LO + 1] * 13)):
                x = lower + [t + dt]
                kind = "rs" if in_kind("rs", x) else "rsclaim"
                out.append(("switch/k%d/%s/%s" % (k, "above" if dt else "below", ln), x, kind))
    for t in ((1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6, -(1 << 24) - 1, -(1 << 24) - 3, 3 * (1 << 24) + 1, (1 << 28) + 8, (1 << 28) + 24):
        for ln, lower in (("zeros", [0] * 13), ("ones", [MASK] * 13)):
            out.append(("float/top%d/%s" % (t, ln), lower + [t], "rsclaim"))
    return out


_CHAINS = {}


def chain_steps(tag, f, n):
    """the teams after 0 .. n squarings of f (computed once per start, the longest first); every step's result is asserted to be an
    operand of the next"""
    key = tag
    if key not in _CHAINS or len(_CHAINS[key]) <= n:
        steps = [f]
        for _ in range(n):
            steps.append(cyc_sqr(steps[-1]))
            assert all(in_kind("small", p) and in_kind("dense", p) for p in parts_of(steps[-1])), (tag, "a chain step leaves the contract")
        _CHAINS[key] = steps
    return _CHAINS[key]


def longest_run():
    return max(a for op, a in F.script() if op == F.CSQ)


def script_sites():
    """what precedes every CSQ, FROB, CONJ and TINV of the script: the kind of the accumulator there.  MUL leaves dense, CSQ small,
    FROB and TINV fe, CONJ of kind k `conj(k)`; ST / LD move kinds through the slots; the input is from_vm's (fe)"""
    names = {F.CSQ: "CSQ", F.FROB: "FROB", F.CONJ: "CONJ", F.TINV: "TINV", F.MUL: "MUL", F.ST: "ST"}
    acc, M, sites = "fe", [None] * F.NSLOTS, {}
    for op, a in F.script():
        if op in names:
            sites.setdefault(names[op] + (str(a) if op == F.FROB else ""), set()).add(acc)
        if op == F.MUL:
            sites.setdefault("MUL/slot", set()).add(M[a])
            acc = "dense"
        elif op == F.CSQ:
            acc = "small"
        elif op == F.ST:
            M[a] = acc
        elif op == F.LD:
            acc = M[a]
        elif op == F.CONJ:
            acc = "conj(%s)" % acc
        elif op in (F.FROB, F.TINV):
            acc = "fe"
        elif op == F.END:
            break
    return sites


def _build(o):
    # REDUCE_SMALL
    op = o["REDUCE_SMALL"] = Op("REDUCE_SMALL", 0, L, L, 1, lambda w: reduce_small(list(w)))
    for tag, x, kind in reduce_small_sets():
        op.add(tag + ("" if kind == "rs" else "/claim"), x, [x], chk_reduce(x), kind)
    # FQ_INVERSE: the norm of tinv, a dot2 output; zero in both its limb forms beside non-zero values
    op = o["FQ_INVERSE"] = Op("FQ_INVERSE", 1, L, L, 1, lambda w: fq_inverse(list(w)))
    rnd = _rnd("FQ_INVERSE")
    vals = [("random/%d" % i, rnd_part("fe", rnd)) for i in range(6)] + [("special/" + n, x) for n, x in specials("fe")]
    vals += [("special/2q-1", to_limbs(2 * Q - 1)), ("special/R2", to_limbs(R * R % Q)), ("special/2", mont(2)), ("special/-1R", mont(Q - 1, -1))]
    for tag, x in vals:
        op.add(tag, x, [x], chk_fq_inverse(x))
    # team ops
    base = team_sets("TEAM")
    op = o["CYC_SQR"] = Op("CYC_SQR", 10, TV, TV, 6, lambda w: flat_team(cyc_sqr(team_of(w))))
    for tag, f, cyc in base:
        op.add(tag, flat_team(f), parts_of(f), chk_cyc(f, cyc))
    # chains: n = 1, 2, the script's longest run and that plus one
    run = longest_run()
    assert run + 1 <= MAX_CHAIN
    op = o["CYC_SQR_CHAIN"] = Op("CYC_SQR_CHAIN", 11, TV + 1, 3 * TV, 6, None)
    by_tag = {t: f for t, f, _ in base}
    forms, _ = one_chain()
    starts = [("subfield/cyc/model0", by_tag["subfield/cyc/model0"]), ("subfield/cyc/golden0", by_tag["subfield/cyc/golden0"]),
              ("extreme/f49", by_tag["extreme/f49"]), ("extreme/5af", by_tag["extreme/5af"]), ("random/0", by_tag["random/0"]),
              ("special/zero-team", by_tag["special/zero-team"])]
    starts += [("subfield/one/form%d" % i, team_of(w)) for i, w in enumerate(forms)]
    op.by_n = {}
    for n in (1, 2, run, run + 1):
        for tag, f in starts:
            def model(words, tag=tag, f=f, n=n):
                if MUT:                                    # a mutant is not cached
                    g, st = team_of(words), []
                    for _ in range(n):
                        g = cyc_sqr(g)
                        st.append(g)
                else:
                    st = chain_steps(tag, f, max(n, run + 1))[1:n + 1]
                return flat_team(st[n - 1]) + flat_team(st[0]) + (flat_team(st[1]) if n >= 2 else [FILL] * TV)
            op.model = model
            op.add("n%d/%s" % (n, tag), flat_team(f) + [n], parts_of(f), chk_chain(f, n))
            op.sets[-1] = op.sets[-1] + (model,)
            op.by_n.setdefault(n, []).append(len(op.sets) - 1)
    op.model = None
    # FROB: every set with every j3
    op = o["FROB"] = Op("FROB", 12, TV + 1, TV, 6, lambda w: flat_team(frob(team_of(w), w[TV])))
    op.by_n = {}
    for j3 in range(3):
        for tag, f, cyc in base:
            op.add("j%d/%s" % (j3, tag), flat_team(f) + [j3], parts_of(f), chk_frob(f, j3))
            op.by_n.setdefault(j3, []).append(len(op.sets) - 1)
    # TINV: the team sets, and t real, purely imaginary, of norm 1 and of norm q - 1 on lane 0 (the other lanes random: not read)
    op = o["TINV"] = Op("TINV", 13, TV, TV, 6, lambda w: flat_team(tinv(team_of(w))))
    rnd = _rnd("TINV")
    tsets = [(t, f) for t, f, _ in base]
    z = (rnd.randrange(1, Q), rnd.randrange(1, Q))
    zi = LM.inv2(z)
    n1 = LM.mul2(z, (zi[0], (-zi[1]) % Q))                # z / conj(z): norm 1
    a = next(a for a in range(2, 1000) if pow((-1 - a * a) % Q, (Q - 1) // 2, Q) == 1)
    nm1 = (a, pow((-1 - a * a) % Q, (Q + 1) // 4, Q))     # a^2 + b^2 = -1
    assert (n1[0] ** 2 + n1[1] ** 2) % Q == 1 and (nm1[0] ** 2 + nm1[1] ** 2) % Q == Q - 1
    for name, t0 in (("real", (rnd.randrange(1, Q), 0)), ("imag", (0, rnd.randrange(1, Q))), ("norm1", n1), ("norm-1", nm1), ("one", (1, 0)),
                     ("u", (0, 1)), ("zero-q-limbs", None)):
        rest = [(rnd_part("dense", rnd), rnd_part("dense", rnd)) for _ in range(5)]
        first = (to_limbs(Q), to_limbs(0)) if t0 is None else (mont(t0[0], 1), mont(t0[1], -1 if t0[1] else 0))
        tsets.append(("t/" + name, [first] + rest))
    for tag, f in tsets:
        op.add(tag, flat_team(f), parts_of(f), chk_tinv(f))
    # CONJ
    op = o["CONJ"] = Op("CONJ", 14, TV, TV, 6, lambda w: flat_team(conj(team_of(w))))
    for tag, f, cyc in base:
        op.add(tag, flat_team(f), parts_of(f), chk_conj(f))
    # SLOT_ROUNDTRIP: f, g of the hull of what MUL and ST meet (acc); g = the next set's team, conjugated on every other set
    op = o["SLOT_ROUNDTRIP"] = Op("SLOT_ROUNDTRIP", 15, 2 * TV, TV, 6, lambda w: flat_team(mul_dense(team_of(w[:TV]), team_of(w[TV:]))))
    accs = team_sets("SLOT", "acc", nr=6)
    pool = [f for _, f, _ in base]
    for i, (tag, f, cyc) in enumerate(accs):
        g = pool[(7 * i + 3) % len(pool)]
        if i % 2:
            g = conj(g)
        op.add(tag, flat_team(f) + flat_team(g), parts_of(f) + parts_of(g), chk_slot(f, g))


_OPS = None


def ops():
    """name -> Op, built once (the expected words are the limb model's)"""
    global _OPS
    if _OPS is None:
        o = {}
        _build(o)
        assert len({op.code for op in o.values()}) == len(o)
        _OPS = o
    return _OPS


def model_of(op, k):
    """the model of set k of an op (a chain set has its own: it knows its start)"""
    s = op.sets[k]
    return s[5] if len(s) > 5 else op.model


def call_sets(op, n, base=0):
    """the set of every item of a call of n items: item i is the same set in every call (base: where a further call goes on).  The ops
    with a uniform run-time word (CYC_SQR_CHAIN's n, FROB's j3) walk the sets of ONE value of it per call, the values taking turns"""
    by = getattr(op, "by_n", None)
    if not by:
        return [(base + i) % len(op.sets) for i in range(n)]
    keys = sorted(by)
    turn = base // max(N_TEAM_ITEMS)
    ks = by[keys[turn % len(keys)]]
    start = (turn // len(keys)) * n
    return [ks[(start + i) % len(ks)] for i in range(n)]


# ---- the whole script on limbs ------------------------------------------------------------------------------------------------------
AUDIT_BOUND = {"MUL": 6, "CSQ": 4, "FROB": 2, "TINV": 2}    # units of 2^56 x 13 products a column may hold by the routine's own count


def from_vm_team(vals):
    """what k_fexp_team loads: the VM's words x 2^384 mod q through r28::from_vm"""
    c = to_limbs(C_FROM_VM)
    return [(dot([(to_limbs(a * (1 << 384) % Q), c)]), dot([(to_limbs(b * (1 << 384) % Q), c)])) for a, b in vals]


def run_script_limbs(vals, audit):
    """the script on limbs (every dot with the 64-bit column asserted), beside fexp_model's interpreter on plain integers: the residues
    are compared after EVERY entry.  audit: op kind -> [largest column sum, widest |value| / q that entered it]"""
    acc, M = from_vm_team(vals), [None] * F.NSLOTS
    ref, RM = [(a % Q, b % Q) for a, b in vals], [None] * F.NSLOTS
    names = {F.MUL: "MUL", F.CSQ: "CSQ", F.FROB: "FROB", F.TINV: "TINV", F.CONJ: "CONJ"}

    def note(kind, operands):
        a = audit.setdefault(kind, [0, 0.0])
        a[0] = max(a[0], MV._peak[0])
        a[1] = max(a[1], max(abs(from_limbs(p)) for f in operands for p in parts_of(f)) / Q)
    for pc, (op, a) in enumerate(F.script()):
        MV._peak[0] = 0
        if op == F.MUL:
            assert all(in_kind("acc", p) for p in parts_of(acc) + parts_of(M[a])), pc
            ins = [acc, M[a]]
            acc, ref = mul_dense(acc, M[a]), F.mul_dense(ref, RM[a])
            assert all(in_kind("dense", p) for p in parts_of(acc)), pc
        elif op == F.CSQ:
            ins = [acc]
            for _ in range(a):
                assert all(in_kind("dense", p) for p in parts_of(acc)), pc
                acc, ref = cyc_sqr(acc), F.cyc_sqr_lane_forms(ref)
        elif op == F.ST:
            M[a], RM[a] = acc, ref
        elif op == F.LD:
            acc, ref = M[a], RM[a]
        elif op == F.CONJ:
            ins = [acc]
            assert all(in_kind("dense", p) for p in parts_of(acc)), pc
            acc, ref = conj(acc), F.conj6(ref)
        elif op == F.FROB:
            ins = [acc]
            assert all(in_kind("dense", p) for p in parts_of(acc)), pc
            acc, ref = frob(acc, a), F.frob(ref, F.FROB_POW[a])
        elif op == F.TINV:
            ins = [acc]
            assert all(in_kind("dense", p) for p in parts_of(acc)), pc
            acc = tinv(acc)
            t = ref[0]
            ni = F.fq_inv((t[0] * t[0] + t[1] * t[1]) % Q)
            ref = [(t[0] * ni % Q, (-t[1]) * ni % Q)] + [(0, 0)] * 5
        else:
            break
        if op in names:
            note(names[op], ins)
        assert res6(acc) == ref, "entry %d (%s %d): the limb model leaves vmgen/fexp_model" % (pc, names.get(op, "ST/LD"), a)
    return res6(acc)


def summary():
    out = {}
    for name, op in ops().items():
        pk = max(PEAK[name].values())
        out[name] = (len(op.sets), pk / (13.0 * (1 << 56)))
    return out


if __name__ == "__main__":
    import time
    t0 = time.time()
    for name, (n, pk) in summary().items():
        tag = max(PEAK[name].items(), key=lambda kv: kv[1])[0]
        print("%-15s %4d sets  peak %.3f units of 13 x 2^56 on %s" % (name, n, pk, tag))
    forms, info = one_chain()
    print("the constant 1: %d limb forms; from R + rep q: (forms, cycle start, cycle length) %s" % (len(forms), info))
    print("largest |reduce_small result| / q: %.6f" % (SMALL_SEEN[0] / Q))
    print("script sites:", {k: sorted(map(str, v)) for k, v in script_sites().items()})
    print("vectors built in %.1f s" % (time.time() - t0))
