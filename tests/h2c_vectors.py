"""Operand sets, the limb model and the independent checks for the register layer behind hash to G2, hash to G1 and decompression
(csrc/blsgpu_h2c.hip namespace swl and the power loops of k_pow / k_pow2, csrc/blsgpu_h2g1.hip's helpers, sha256_block), one list per op
of the test-only device library csrc/blsgpu_h2c_check.hip.  Pure Python: tests/test_h2c_vectors_model.py checks the model against the
independent reference and against its mutants on the CPU, tests/test_gpu_h2c_check.py compares the compiled routines with it word
for word.

The LIMB MODEL is built over tests/fp28_vectors.py -- `dot` (vmgen.gen_fp28.model_dot, the column arithmetic), the carry pass, from_raw /
to_raw / from_vm / to_vm as that file has them -- and over the window schedule vmgen.emit.pow_windows produces (BLSVM_POW_WIN) and the
bits of (q - 3) / 4 (BLSVM_POW_E).  It gives exact words for every op.  The INDEPENDENT REFERENCE works on the device's own words in
Python integers: pow(a, (q - 1) // 2, q) for the symbols, pow(b, (q - 3) // 4, q) for the powers, a out = 1, int.from_bytes(...) % q,
canonical > (q - 1) // 2, hashlib.sha256 on a block that is a whole padded one-block message.  Neither the C oracle nor the code under
test is a reference.

An `fe` result travels as FE = 26 words: the 14 limbs as they are, then the 12 words of to_vm.

Value ranges.  Every operand of chi, sgn, inv, pow_e and sel is an fe: digits 0 .. 12 in [0, 2^28).  The call sites differ in the value:
(-q, 2q) from a product, (-2q, 4q) for sgn in the wide stage 0 (norm of a sum of two products).  red takes F<0, 2> (a sum: limbs below
2^29, value in (-2q, 4q)) and F<1, 1> (a difference: limbs in (-2^28, 2^28), value in (-3q, 3q)).  Every set asserts its range (in_range).

FIELD_ELEMENT_1 takes message hashes, so its 512-bit values are what SHA-256 gives: no digest with hi = 0, hi = 2^128 - 1, lo = q or any
other chosen value can be found by search (each asks for 128 or more fixed bits).  Those classes run through FE1_REDUCE instead, a
marked copy of field_element<1>'s last statement that takes the two digests as operands; the sha256_block calls are covered by
SHA256_BLOCK and by FIELD_ELEMENT_1's random messages.

Two mutants the issue lists are the identity inside the contract and are left out: `sgn without norm` (sgn's operand is an fe: the
carry pass changes nothing) and `767 iterations` (at most bits(a) + bits(q) = 762 iterations do work, so none
works after iteration 761, counted from 0; WORST_ITERATION is the latest found)."""
import hashlib
import json
import os
import random
import re
import struct

import fp28_vectors as P
import test_jacobi_model as J
from fp28_vectors import Q, R, L, MASK, RINV, ONE, TOP, C_FROM_VM, C_TO_VM, C_R2, dot, to_limbs, from_limbs, words12, from_words, s32, l_norm, l_canon, l_add, l_sub
from vmgen import emit as E

HALF = (Q - 1) // 2
EXP_E = (Q - 3) // 4
EXP_BITS = EXP_E.bit_length()
POW_WIN = E.pow_windows(EXP_E)
NT = 1 << (E.POW_WINDOW - 1)
R384 = 1 << 384
C2 = R384 * R * R % Q                                  # BLS28_WIDE_C2
L_ONE, L_RAW1, L_TO_VM, L_FROM_VM, L_R2, L_C2 = to_limbs(ONE), [1] + [0] * (L - 1), to_limbs(C_TO_VM), to_limbs(C_FROM_VM), to_limbs(C_R2), to_limbs(C2)
FE = L + 12
N_ITEMS = (1, 63, 64, 65, 257)
POW_TOTALS = (1, 63, 64, 65, 127, 128, 129, 257)
FILL = s32(0xAAAAAAAA)                                 # what the runner fills the output with
MUT = set()                                            # the mutants of the model that are switched on (tests/test_h2c_vectors_model.py)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-bls_amd", "csrc")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def table_defines():
    """the BLSVM_H1_* slot numbers of csrc/vm_tables.h"""
    with open(os.path.join(CSRC, "vm_tables.h")) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define BLSVM_(H1_\w+) (\d+)$", f.read(), re.M)}


H1 = table_defines()
STATE0, STATE1 = H1["H1_STATE0"], H1["H1_STATE1"]
IMG_DW = (STATE1 - STATE0) * 12


def euler(a):
    return {0: 0, 1: 1, Q - 1: -1}[pow(a % Q, (Q - 1) // 2, Q)]


def in_range(x, lo, hi, vlo, vhi):
    """limbs 0 .. 12 in [-lo 2^28, hi 2^28), the top digit small, the value in (vlo q, vhi q)"""
    return all(-(lo << 28) <= d < (hi << 28) for d in x[:13]) and abs(x[13]) <= TOP and vlo * Q < from_limbs(x) < vhi * Q


def forms(m, vlo, vhi):
    """the limbs of every m + k q inside (vlo q, vhi q): the forms a residue takes"""
    m %= Q
    return [to_limbs(m + k * Q) for k in range(vlo - 1, vhi + 1) if vlo * Q < m + k * Q < vhi * Q]


def mont(v):
    return v * R % Q


def res(x):
    """the residue a limb list stands for"""
    return from_limbs(x) * RINV % Q


# ---- the limb model ------------------------------------------------------------------------------------------------------------
def m_to_raw(x): return from_limbs(l_canon(dot([(x, L_RAW1)])))
def m_to_vm(x): return from_limbs(l_canon(dot([(x, L_TO_VM)])))
def m_from_vm(v): return dot([(to_limbs(v), L_FROM_VM)])
def m_from_raw(v): return dot([(to_limbs(v), L_R2)])
def m_mul(x, y): return dot([(x, y)])
def m_fe(x): return [int(d) for d in x] + words12(m_to_vm(x))


def m_jacobi(a):
    """swl::jacobi on the integer of the 12 words"""
    n, s = Q, 0
    for _ in range(768):
        odd = a & 1
        if odd and a < n:
            both = (a | n) if "recip_or" in MUT else (a & n)
            s ^= (both >> 1) & 1
            a, n = n - a, a
        elif odd:
            a -= n
        if a:
            s ^= ((n >> 1) & 1) if "halve_37" in MUT else (((n >> 1) ^ (n >> 2)) & 1)
        a >>= 1
    return 0 if n != 1 else (-1 if s else 1)


def m_chi(x):
    a = m_to_raw(l_norm(x))
    r = J.jacobi_divsteps(a)[0]
    return m_jacobi(a) if r == 2 else r


def m_sgn(x):
    a = m_to_raw(l_norm(x))
    return 1 if (a >= HALF if "sgn_ge" in MUT else a > HALF) else 0


def m_red(x):
    return list(x) if "red_skipped" in MUT else m_mul(x, L_ONE)


def m_inv(x):
    w = m_to_vm(x)                                     # x 2^384, canonical
    v = pow(w, -1, Q) * R384 * R384 % Q if w else (R384 % Q if "inv_zero_one" in MUT else 0)
    return m_from_vm(v)


def m_pow_win(b):
    """h2g1::pow_e and k_pow's loop: the sliding-window schedule, odd powers in a table"""
    tbl, t = [b], m_mul(b, b)
    for i in range(1, NT):
        tbl.append(m_mul(tbl[i - 1], t))
    off = 1 if "win_pick_off" in MUT else 0
    pick = lambda k: tbl[k + off] if 0 < k + off < NT else tbl[0]      # (the kernel's select: an index the table lacks gives entry 0)
    a = pick(POW_WIN[0][1])
    for nsq, k in POW_WIN[1:]:
        for _ in range(nsq):
            a = m_mul(a, a)
        if k != 255:
            a = m_mul(a, pick(k))
    return a


def m_pow_b4(b):
    """k_pow2's loop: right to left in base 4, three buckets, b^e = B1 B2^2 B3^3 in four products"""
    digits = (EXP_BITS + 1) // 2
    sh = 1 if "b4_digit_bit" in MUT else 0
    p, B = b, [None, L_ONE, L_ONE, L_ONE]
    for j in range(digits):
        d = (EXP_E >> (2 * j + sh)) & 3
        if d:
            B[d] = m_mul(B[d], p)
        if j + 1 < digits:
            p = m_mul(p, p)
            p = m_mul(p, p)
    B1, B2, B3 = (B[1], B[3], B[2]) if "b4_b2_b3" in MUT else (B[1], B[2], B[3])
    run = m_mul(B3, B2)
    acc = m_mul(B3, run)
    run = m_mul(run, B1)
    return m_mul(acc, run)


K256 = [int(x, 16) for x in """428a2f98 71374491 b5c0fbcf e9b5dba5 3956c25b 59f111f1 923f82a4 ab1c5ed5 d807aa98 12835b01 243185be 550c7dc3
72be5d74 80deb1fe 9bdc06a7 c19bf174 e49b69c1 efbe4786 0fc19dc6 240ca1cc 2de92c6f 4a7484aa 5cb0a9dc 76f988da 983e5152 a831c66d b00327c8
bf597fc7 c6e00bf3 d5a79147 06ca6351 14292967 27b70a85 2e1b2138 4d2c6dfc 53380d13 650a7354 766a0abb 81c2c92e 92722c85 a2bfe8a1 a81a664b
c24b8b70 c76c51a3 d192e819 d6990624 f40e3585 106aa070 19a4c116 1e376c08 2748774c 34b0bcb5 391c0cb3 4ed8aa4a 5b9cca4f 682e6ff3 748f82ee
78a5636f 84c87814 8cc70208 90befffa a4506ceb bef9a3f7 c67178f2""".split()]
H256 = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]
M32 = 0xFFFFFFFF


def m_sha_block(w16):
    """sha256_block: one compression from the initial state, on 16 words"""
    rotr = lambda x, n: ((x >> n) | (x << (32 - n))) & M32
    w = [x & M32 for x in w16]
    for i in range(16, 64):
        s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)
        s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10)
        w.append((w[i - 16] + s0 + w[i - 7] + s1) & M32)
    a, b, c, d, e, f, g, h = H256
    for i in range(64):
        t1 = (h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g & M32)) + K256[i] + w[i]) & M32
        t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & M32
        h, g, f, e, d, c, b, a = g, f, e, (d + t1) & M32, c, b, a, (t1 + t2) & M32
    out = [a, b, c, d, e, f, g, h]
    return out if "sha_no_final_add" in MUT else [(x + y) & M32 for x, y in zip(out, H256)]


def m_fe1_reduce(be):
    """field_element<1> after its two hashes: be = the 16 digest words, word 0 most significant"""
    lo = sum((be[15 - k] & M32) << (32 * k) for k in range(12))
    hi = sum((be[3 - k] & M32) << (32 * k) for k in range(4))
    s = m_from_raw(lo) if "no_hi_c2" in MUT else l_add(m_from_raw(lo), m_mul(to_limbs(hi), L_C2))
    return m_red(s)


def bswap(w):
    return struct.unpack("<I", struct.pack(">I", w & M32))[0]


def m_field_element_1(words8, j):
    w = [bswap(x) for x in words8] + [0x47315F00 | (0x30 + j), 0, 0, 0, 0, 0, 0, 296]
    sel = (0x01800000, 0x00800000) if "selector_swapped" in MUT else (0x00800000, 0x01800000)
    be = []
    for s in sel:
        w[9] = s
        be += m_sha_block(w)
    return m_fe1_reduce(be)


def mem_words(b):
    """bytes as the 32-bit words a little-endian machine reads from them"""
    return [s32(x) for x in struct.unpack("<%dI" % (len(b) // 4), b)]


# ---- independent checks on output words -----------------------------------------------------------------------------------------
def chk_fe(got, want_res):
    """an FE record: digits, the range of a product, the residue, and to_vm's words = residue 2^384 canonical"""
    x = got[:L]
    assert in_range(x, 0, 1, -1, 2), "limbs or value leave the form of a product"
    assert res(x) == want_res % Q, "wrong residue"
    assert from_words(got[L:FE]) == res(x) * R384 % Q, "to_vm's words are not the residue times 2^384, canonical"


def eq(want):
    def chk(got):
        assert list(got) == list(want), "got %s, the reference says %s" % (got, want)
    return chk


# ---- ops -----------------------------------------------------------------------------------------------------------------------
class Op:
    def __init__(self, name, code, win, wout, model, counts=N_ITEMS, wave=False):
        self.name, self.code, self.win, self.wout, self.model, self.counts, self.wave = name, code, win, wout, model, counts, wave
        self.sets = []                                 # (tag, input words, expected words, independent check of output words)

    def add(self, tag, words, check):
        words = [int(w) for w in words]
        assert len(words) == self.win and P.fits32(words), (self.name, tag)
        want = [int(w) for w in self.model(words)]
        assert len(want) == self.wout, (self.name, tag)
        self.sets.append((tag, words, want, check))


def call_sets(op, n, base=0):
    """the set of every item of a call: item i holds set base + i (a wave op: base + i // 64), modulo the number of sets"""
    return [(base + (i // 64 if op.wave else i)) % len(op.sets) for i in range(n)]


WORST_ITERATION = [0, None]                            # the last iteration of swl::jacobi that did work, and on which value


def symbol_values(rnd, nrandom):
    vals = [("corner", v) for v in (0, 1, 2, 3, Q - 1, Q - 2, HALF, HALF + 1)]
    for k in range(381):
        vals += [("pow2", v) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 3 < v < Q]
    with open(os.path.join(GOLDEN, "h2c_corners.json")) as f:
        for c in json.load(f)["cases"]:
            vals += [("golden-norm", int(c[k], 16)) for k in ("norm_x1", "norm_x2") if k in c]
    for r8 in range(8):                                # a square and a non-square of every residue mod 8
        for want in (1, -1):
            while True:
                v = rnd.randrange(Q) & ~7 | r8
                if v < Q and euler(v) == want:
                    break
            vals.append(("mod8/%d/%d" % (r8, want), v))
    # the longest runs: among q - 2^k, 2^k and seeded values, the ones whose last working iteration is latest
    cand = [Q - (1 << k) for k in range(1, 381)] + [(1 << 380) + rnd.randrange(1 << 300) for _ in range(40)] + [v for _, v in vals]
    ranked = sorted(((J.jacobi_fixed(v)[1], v) for v in cand), reverse=True)
    WORST_ITERATION[:] = ranked[0]
    vals += [("longest", v) for _, v in ranked[:8]]
    vals += [("random", rnd.randrange(Q)) for _ in range(nrandom)]
    seen, out = set(), []
    for tag, v in vals:
        if (tag == "random" or tag.startswith("mod8") or v not in seen) and 0 <= v < Q:
            seen.add(v)
            out.append((tag, v))
    return out


def sha_blocks(rnd):
    """16 words each: a whole padded message of one block, so that hashlib is the reference"""
    out = []
    for n, fill in ((0, None), (1, 0), (1, 0xFF), (3, None), (37, None), (40, None), (55, None), (55, 0xFF), (55, 0), (32, None), (4, 0x80)):
        for _ in range(2 if fill is None else 1):
            msg = bytes(rnd.randrange(256) if fill is None else fill for _ in range(n))
            blk = msg + b"\x80" + bytes(55 - n) + (8 * n).to_bytes(8, "big")
            out.append(("len%d" % n, msg, [s32(x) for x in struct.unpack(">16I", blk)]))
    return out


_OPS = {}


def ops():
    if _OPS:
        return _OPS
    rnd = random.Random("h2c:vectors")

    def op(*a, **k):
        o = Op(*a, **k)
        _OPS[o.name] = o
        return o

    # ---- symbols
    sym = symbol_values(rnd, 24)
    jb = op("JACOBI_BIN", 0, 12, 1, lambda w: [m_jacobi(from_words(w))])
    for tag, v in sym:
        jb.add(tag, words12(v), eq([euler(v)]))
    chi = op("CHI", 1, L, 1, lambda w: [m_chi(w)])
    for i, (tag, v) in enumerate(sym):
        fs = forms(mont(v), -1, 2)
        if tag == "pow2" and i % 8:                   # the many powers of two in one form each, everything else in every form
            fs = fs[i % len(fs):][:1]
        for x in fs:
            assert in_range(x, 0, 1, -1, 2)
            chi.add("%s/%+d" % (tag, from_limbs(x) // Q), x, eq([euler(v)]))
    chi.add("corner/zero-q-limbs", to_limbs(Q), eq([0]))

    # ---- sign: both sides of (q - 1) / 2, 0, q - 1, each in every form of (-2q, 4q)
    sg = op("SGN", 2, L, 1, lambda w: [m_sgn(w)])
    for tag, v in [("half", HALF), ("half+1", HALF + 1), ("half-1", HALF - 1), ("half+2", HALF + 2), ("zero", 0), ("one", 1), ("q-1", Q - 1), ("q-2", Q - 2)] + \
            [("random", rnd.randrange(Q)) for _ in range(24)]:
        for x in forms(mont(v), -2, 4):
            assert in_range(x, 0, 1, -2, 4)
            sg.add("%s/%+d" % (tag, from_limbs(x) // Q), x, eq([1 if v > HALF else 0]))

    # ---- red at both instantiations, inv, scale
    fes = [("zero", 0), ("zero+q", Q), ("one", ONE), ("q-1", Q - 1), ("2q-1", 2 * Q - 1), ("-q+1", -Q + 1), ("R2", R * R % Q), ("digits", (1 << 364) - 1)] + \
        [("random", rnd.randrange(-Q + 1, 2 * Q)) for _ in range(12)]
    for name, code, comb, lo, hi, vlo, vhi in (("RED_02", 3, l_add, 0, 2, -2, 4), ("RED_11", 4, l_sub, 1, 1, -3, 3)):
        o = op(name, code, L, FE, lambda w: m_fe(m_red(w)))
        for ta, a in fes:
            for tb, b in fes[:8] + fes[-2:]:
                x = comb(to_limbs(a), to_limbs(b))
                assert in_range(x, lo, hi, vlo, vhi)
                o.add("%s,%s" % (ta, tb), x, lambda g, v=from_limbs(x): chk_fe(g, v * RINV))
    inv_vals = [("zero", 0), ("one", 1), ("q-1", Q - 1), ("two", 2), ("half", HALF), ("R", R % Q), ("R2", R * R % Q), ("2^380", (1 << 380) % Q)] + \
        [("random", rnd.randrange(1, Q)) for _ in range(20)]

    def chk_inv(v):
        def chk(g):
            chk_fe(g, res(g[:L]))
            assert (res(g[:L]) * v - 1) % Q == 0 if v % Q else res(g[:L]) == 0, "a out != 1 (0 -> 0)"
        return chk
    inv = op("INV", 5, L, FE, lambda w: m_fe(m_inv(w)))
    invw = op("INV_WAVE", 5, L, FE, lambda w: m_fe(m_inv(w)), wave=True)      # one value per wavefront
    for i, (tag, v) in enumerate(inv_vals):
        for x in forms(mont(v), -1, 2):
            inv.add("%s/%+d" % (tag, from_limbs(x) // Q), x, chk_inv(v))
        if i % 3 == 0:
            invw.add(tag, to_limbs(mont(v)), chk_inv(v))
    for at in (5, 17, 40):                             # zero beside non-zero values, in its other form as well
        inv.sets.insert(at, inv.sets[0 if at != 17 else 1])
    sc = op("SCALE", 6, 3 * L, 2 * FE, lambda w: m_fe(m_mul(w[:L], w[2 * L:])) + m_fe(m_mul(w[L:2 * L], w[2 * L:])))
    for ta, a in fes[:8] + fes[-4:]:
        for tk, k in fes[2:7] + fes[-2:]:
            b = fes[(len(sc.sets) * 5 + 3) % len(fes)][1]
            w = to_limbs(a) + to_limbs(b) + to_limbs(k)
            sc.add("%s,%s" % (ta, tk), w, lambda g, a=a, b=b, k=k: (chk_fe(g[:FE], a * k * RINV * RINV), chk_fe(g[FE:], b * k * RINV * RINV)))

    # ---- the image: stv<0, 2> at a, ldv from a, stv at b, st_zero at z
    def m_img(w):
        a, b, z = w[0] - STATE0, w[1] - STATE0, w[2] - STATE0
        img = [FILL] * IMG_DW
        y = m_to_vm(l_norm(w[3:]))
        img[12 * a:12 * a + 12] = words12(y)
        img[12 * b:12 * b + 12] = words12(m_to_vm(l_norm(m_from_vm(y))))
        img[12 * z:12 * z + 12] = [0] * 12
        return img

    def chk_img(w):
        def chk(g):
            a, b, z = w[0] - STATE0, w[1] - STATE0, w[2] - STATE0
            y = words12(from_limbs(w[3:]) * RINV % Q * R384 % Q)
            for s in range(STATE1 - STATE0):
                want = y if s in (a, b) else ([0] * 12 if s == z else [FILL] * 12)
                assert g[12 * s:12 * s + 12] == want, "slot %d of the image" % (STATE0 + s)
        return chk
    ls = op("LDV_STV", 7, 3 + L, IMG_DW, m_img)
    lowest, highest = H1["H1_T"], H1["H1_S"] + 5 * H1["H1_NE"] - 1
    assert (lowest, highest) == (STATE0, STATE1 - 1)
    slots = [(lowest, highest, H1["H1_ACC"]), (highest, lowest, H1["H1_BASE"]), (H1["H1_N"], lowest + 1, highest), (H1["H1_U"], highest - 1, lowest)]
    for i, (ta, a) in enumerate(fes):
        x = l_add(to_limbs(a), to_limbs(fes[(3 * i + 1) % 8][1]))
        assert in_range(x, 0, 2, -2, 4)
        w = list(slots[i % 4]) + x
        ls.add("%s/slots%d" % (ta, i % 4), w, chk_img(w))

    # ---- powers
    nsq = next(v for v in range(2, 99) if euler(v) == -1)
    pw_vals = [("zero", 0), ("one", 1), ("q-1", Q - 1), ("R", R % Q), ("R2", R * R % Q), ("square", 4), ("non-square", nsq), ("half", HALF)] + \
        [("random", rnd.randrange(Q)) for _ in range(4)]

    def chk_pow(b):
        def chk(g):
            chk_fe(g, pow(b, EXP_E, Q))
            root = res(g[:L]) * b % Q                  # b^((q + 1) / 4): a root of b or of -b
            assert root * root % Q in (b % Q, -b % Q)
        return chk
    pe = op("POW_E", 10, L, FE, lambda w: m_fe(m_pow_win(w)))
    nrandom = 0
    for i, (tag, v) in enumerate(pw_vals):
        # red's whole range (-q, 2q): 0, 1, q - 1 and two random values in every form (v - q, v, v + q; for 0 the limbs of 0 and of q),
        # the others canonical and, in turn, above q or below 0
        fs = forms(mont(v), -1, 2)
        nrandom += tag == "random"
        if tag == "random" and nrandom > 2:
            fs = [f for f in fs if 0 <= from_limbs(f) < Q]
        elif tag not in ("zero", "one", "q-1", "random"):
            fs = [f for f in fs if 0 <= from_limbs(f) < Q] + [fs[-1] if i % 2 else fs[0]]
        for x in fs:
            assert in_range(x, 0, 1, -1, 2)
            pe.add("%s/%+d" % (tag, from_limbs(x) // Q), x, chk_pow(v))
    pw = op("POW_LOOP_WIN", 11, 12, FE, lambda w: m_fe(m_pow_win(m_from_vm(from_words(w)))), counts=POW_TOTALS)
    pb = op("POW_LOOP_B4", 12, 12, FE, lambda w: m_fe(m_pow_b4(m_from_vm(from_words(w)))), counts=POW_TOTALS)
    for tag, v in pw_vals:                             # the VM's form: v 2^384, canonical (stv) or plus q (a base in (q, 2q))
        for y in [v * R384 % Q] + ([v * R384 % Q + Q] if tag in ("zero", "one", "random", "q-1") else []):
            assert y < 2 * Q
            for o in (pw, pb):
                o.add("%s/%s" % (tag, "q+" if y >= Q else "canon"), words12(y), chk_pow(v))
    pw.add("top/2^384-1", words12(R384 - 1), chk_pow((R384 - 1) * pow(R384, -1, Q)))
    pb.add("top/2^384-1", words12(R384 - 1), chk_pow((R384 - 1) * pow(R384, -1, Q)))

    # ---- field elements
    ts = [0, 1, Q - 1, Q, Q + 1, 2 * Q, R384 - 1] + [rnd.randrange(R384) for _ in range(6)]
    f0 = op("FIELD_ELEMENT_0", 20, 24, 2 * FE, lambda w: sum((m_fe(m_from_raw(int.from_bytes(struct.pack("<12I", *[x & M32 for x in w[12 * j:12 * j + 12]]), "big")))
                                                             for j in range(2)), []))
    for i, t0 in enumerate(ts):
        t1 = ts[(3 * i + 2) % len(ts)]
        f0.add("t%d" % i, mem_words(t0.to_bytes(48, "big") + t1.to_bytes(48, "big")), lambda g, t0=t0, t1=t1: (chk_fe(g[:FE], t0), chk_fe(g[FE:], t1)))
    f1 = op("FIELD_ELEMENT_1", 21, 8, 2 * FE, lambda w: m_fe(m_field_element_1(w, 0)) + m_fe(m_field_element_1(w, 1)))
    for i in range(12):
        m = bytes(32) if i == 0 else (b"\xff" * 32 if i == 1 else bytes(rnd.randrange(256) for _ in range(32)))
        want = [int.from_bytes(hashlib.sha256(m + b"G1_%d" % j + b"\x00").digest() + hashlib.sha256(m + b"G1_%d" % j + b"\x01").digest(), "big") for j in range(2)]
        f1.add("msg%d" % i, mem_words(m), lambda g, want=want: (chk_fe(g[:FE], want[0]), chk_fe(g[FE:], want[1])))
    fr = op("FE1_REDUCE", 22, 16, FE, lambda w: m_fe(m_fe1_reduce(w)))
    for hi in (0, (1 << 128) - 1, 1, 1 << 127, rnd.randrange(1 << 128)):
        for lo in (0, Q - 1, Q, R384 - 1, 2 * Q, rnd.randrange(R384)):
            v = (hi << 384) | lo
            x = l_add(m_from_raw(lo), m_mul(to_limbs(hi), L_C2))
            assert in_range(x, 0, 2, -2, 4)
            fr.add("hi%x/lo%x" % (hi >> 96, lo >> 352), [s32(v >> (32 * (15 - k))) for k in range(16)], lambda g, v=v: chk_fe(g, v))

    # ---- sel, sha
    se = op("SEL", 23, 1 + 2 * L, L, lambda w: w[1:1 + L] if w[0] else w[1 + L:])
    for i in range(16):
        a, b = to_limbs(rnd.randrange(-Q + 1, 2 * Q)), to_limbs(rnd.randrange(-Q + 1, 2 * Q))
        if i == 0:
            a, b = [MASK] * 13 + [TOP], [0] * 13 + [-TOP]
        c = (1, 0, 1, 1, 0, 0, 1, 0, s32(0x80000000), 0, 2, 0, 0, 1, 0, 1)[i]     # neighbouring lanes differ
        se.add("c%d" % i, [c] + a + b, eq(a if c else b))
    sh = op("SHA256_BLOCK", 24, 16, 8, lambda w: [s32(x) for x in m_sha_block(w)])
    for tag, msg, w in sha_blocks(rnd):
        sh.add(tag, w, eq([s32(x) for x in struct.unpack(">8I", hashlib.sha256(msg).digest())]))
    return _OPS
