"""Operand sets and CPU references for the 32-bit-limb field layer (csrc/fq32.h, csrc/fq_mul_gfx950.h) and the LIN-round
helpers of run_rounds, one list per op of the test-only device library csrc/blsgpu_fq32_check.hip.  Pure Python:
tests/test_fq32_vectors_model.py runs the host build of fq32.h on the same sets against the same references and checks
the preconditions every set claims; tests/test_gpu_fq32.py compares the compiled kernels with them word for word.

References are Python integers, none shared with the device code:
  * products: r = (a b + m q) / 2^384 with m = -a b q^-1 mod 2^384 (unique), one conditional subtraction for fq_mul;
    the independent check is r R = a b (mod q) and r < q (fq_mul) or r < 2q (relaxed, square);
  * linear ops, decisions, inversions: the integer identity of the op; Euler's criterion for fq_jacobi_var;
  * fat_reduce, lin, lin_absorb: a limb model that repeats the quotient estimate in Python floats (IEEE double, as on the
    device) gives the expected words; the independent check is out = V (mod q) and 0 <= out < 2q with V taken from the
    integers (for lin / lin_absorb from the coefficients and operands, not from the limbs).  The device may contract the
    estimate's multiply and subtract into one fused operation; that rounds differently only when the estimate lies
    within an ulp of an integer, and the model test asserts that no set comes closer than 1e-6.

Layout: item i of a call holds set (37 i mod 257) mod nsets, whatever the number of items (N_ITEMS), so 257 items meet
every set.  Three ops are laid out by WAVEFRONT instead (Op.wave): item i holds set (37 (i // 64) mod 257) mod nsets --
fq_inv_uni / fq_inv_var_uni (eight values per item, every lane of the wavefront the same item) and lin_absorb, whose set
is a whole round: MN, K and levels shared by 64 lane records, lane i % 64 taking its own record.  Lanes past the last
item of a lin_absorb call run a share of zero coefficients (absorb_expected's `nlive`).

fat_reduce decompositions: `tight` (32-bit digits, the rest in acc[11] -- which is also "everything possible pushed into
acc[11]": the limbs are non-negative, so no other form has a larger top limb), `ceil` (every lower limb within 2^32 of
its 2^44 - 1 ceiling as far as V allows, the top limb adjusted) and `spread` (every lower limb carries a 12-bit excess
taken from the limb above).
"""
import random

Q = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
R = 1 << 384
RINV = pow(R, -1, Q)
QNEGINV = (-pow(Q, -1, R)) % R
ONE = R % Q                                            # the Montgomery form of 1
HALF = (Q - 1) // 2                                    # = q // 2
M32 = 0xFFFFFFFF
ALL1 = R - 1
N_ITEMS = (1, 63, 64, 65, 257)                         # items per call: one lane, either side of a wavefront, two workgroups
MAX_SETS = 257
STRIDE = 37                                            # coprime to 64 and to 257
LIN_MAXK = 30                                          # micro-ops of a LIN record (csrc/blsgpu_kernels.hip LIN_CHUNKS)
LIN_WIN = 4 + LIN_MAXK + 12 * LIN_MAXK
UNI = 8                                                # values per item of the wave-uniform inversions
QC = R - Q
T0 = sum((1 << 40) << (32 * j) for j in range(12))
BIAS = T0 + (-T0) % Q                                  # fq32.h BLS_BIAS1_FAT minus one per limb (vmgen/tablesim.py)
BIAS_LIMBS = [(1 << 40) + ((((-T0) % Q) >> (32 * j)) & M32) for j in range(12)]
NEG_CF_MAX = 255                                       # sum of a share's negative coefficients: 255 (2^32 - 1) < 2^40
FAT_LIMIT = 1 << 44                                    # per limb at the reduce
V_LIMIT = 1 << 396


def words12(x):
    assert 0 <= x < R, x
    return [(x >> (32 * i)) & M32 for i in range(12)]


def from_words(ws):
    return sum((w & M32) << (32 * i) for i, w in enumerate(ws))


def fat_words(limbs):
    out = []
    for a in limbs:
        assert 0 <= a < 1 << 64
        out += [a & M32, a >> 32]
    return out


def fat_limbs(ws):
    return [ws[2 * j] | (ws[2 * j + 1] << 32) for j in range(12)]


def fat_value(limbs):
    return sum(a << (32 * j) for j, a in enumerate(limbs))


def item_set(i, nsets):
    return ((i * STRIDE) % MAX_SETS) % nsets


# ---- the value lists shared with tests/test_abi_and_host.py::test_fq32_host_build_matches_python_ints ----------------
INV_CORNERS = [0, 1, 2, Q - 1, Q - 2, R % Q]
INV_PATTERNS = [(1 << k) % Q for k in range(0, 384, 7)] + [(Q - (1 << k)) % Q for k in range(0, 380, 11)] + [Q, Q + 1, 2 * Q - 1]
JACOBI_CORNERS = [0, 1, 2, 3, 4, Q - 1, Q - 2, (Q - 1) // 2, (Q + 1) // 2, 1 << 380]

ALT_ODD = sum(M32 << (32 * j) for j in range(1, 12, 2))     # limbs 1, 3, .. 11 all ones
ALT_EVEN = sum(M32 << (32 * j) for j in range(0, 12, 2))    # limbs 0, 2, .. 10 all ones (top limb 0: below q)
POW32 = [1 << (32 * k) for k in range(12)]
POW32M1 = [(1 << (32 * k)) - 1 for k in range(1, 13)]       # the last one is ALL1


# operand pairs found by a seeded search with an emulation of fq_mul_gfx950.h's columns: each makes a multiply-accumulate carry
# into the third accumulator word at a position that no pair above reaches ("The 32-bit field layer on its own")
CARRY_PAIRS = {
    "fq_mul": [
        (0x879b86a7c55dde1d5d1cbd047e5eb8dab163406b4581e37ffffffff5d09dd294e424b92c277af3208c9196da9fd1ce9,
         0x1002dc29d111eb3749f088d476832b6246103a2babf0ca69ffffffff402d5ebbc61251908c07985b796bfa0002f6f33d),
        (0x10f4acb4bb34e7074bfc89839d1305f5560c117eb54146ec889351cd4847ec0e4cfa01162043a7e2c2a97ce2ffffffff,
         0x813d94bffffffff095367c221ea2f04973efa14d0090a86beb9722bae87eb6f5c6d13a1598a2ea576dec5ce06d04b90),
        (0x7d8f4645882b1beff2c1501e33768aae32190be203a4766f180a0644a20061221330ce02e48357ffe01a209da734629,
         0x180b5a93d23737519c2c8736ffffffffc59e161cb9c85448ffffffff2440f8bcc8317e67cfb8e19796d1cc3df4596410),
        (0x13f696c6cba40efea4f63f05d62d69b64fe3a67814c01f4c5047ac0cd640c73d0000f9a90ed8f43d6f07155d3bc58d3c,
         0xfcdca28d8962d8da286df691c6e05788567f88c15437a93475ce7bcffffffffedb442ed1cc3bcec08f45e66fc9d0d9c),
    ],
    "fq_mul_relaxed": [
        (0xfcf5e26e1917c8db237afb98874f661047e555e645cc8f51d8430f4c20833652d83d3fb9ffffffff5f46d2023187a1f9,
         0x3de061affffffff0a4cdb9ae8e1983322358d0d7c142a40a3509647f29b43b352c15775014f0d7c5008a30aa0567ac8),
        (0x97439ccffffffffd2f08a2eed3a9917ec81b827178ac654f50dfe137555e0fb654c8eac37729bed40cbb75521a12265,
         0xffffffff3cb09d4e4578d70b08a7e7016618541affffffffb40532ec3088356f5228f3bad39d6ce4f57ee98f419ba2c4),
        (0x159bd6fad3b82419ba556fd4b8cec85461d6b5147860e31d5af5010ff1a7839d7dd36638d6199c14c453286b5f6e3f99,
         0xf9bcce715ad96f583106359effffffffc6f5c64af0505e2c69a1775cbd8b87f9133d0909234684b54d87177ff1dbb9fc),
        (0x84a0a6c11e902740b1c483821e312406ec0a53ca2ec75e1e8f23b67ffffffff278da6cde9e6191288ddfedaa7cd8248,
         0xe96c01da5a9fb22975440ef6ffffffffffffffffae7850efc8880a74970ce6826d11339ec2a5432799f9cae9180f59d3),
        (0x1437aed3eb581b17e78ffe2ea1829b7258a91436a5bb6ab3a291682d0c8119e42d966be5cfc313326bd2f8f1fe9171cc,
         0xf8e45abb55bf688facbba4a89d541fef98f3318beff11fc0effaf8dd49cd64f2f5d7c0a06da07709459b2f08e5ded46b),
        (0x9c59178ffffffff9b8cdd35a45e32334e38e24ffc5200f3cef98fe6ae7a475c70a1c121a8ba391a8602388f91ea7884,
         0xffffffffffffffff9b0f9f42f692e5d4b0c796644c90dc87edcd04c799d43473193ad2dfdd69751c243ccf89c0da793a),
        (0xff3f7b3917d7f4e260a7c2aae9eb412bb1661f1aa8975ad407970fa2052031f3f853a36fa85cbea592b86136cb1538c,
         0xffffffff4507d7caca9c44e3ffffffffc7b9205a41866e1069034bf88f414aff42b32173490b53a6d50f93471e4f5910),
        (0x69f0d699baf73657170da68fad94b4b0ebd8652547cbd7661597af1f0686db7c12949fda54f869ec1e1a020fafe991c,
         0xffffffff91f125d4841bc5f3f5ec3f631709c9bdc4255c6aea58397891ddd5c0c603e6ca80a63e5c9bda436f79d24bc9),
        (0x15a0ffdabcc3b24cffffffff4c2aa7d0a029bd52785f802069caac859b02392aa0ef2218025a82670031330d36951944,
         0xf3e610709fa54fc5967ec3af00f0ee477ebaed172050dcb81f7a1c86978257f6285cbcc056de84682e8884b8159c9aef),
    ],
}


def _rnd(name):
    return random.Random("fq32:" + name)


# ---- references --------------------------------------------------------------------------------------------------------
def mont(a, b):
    """(a b + m q) / 2^384, m = -a b q^-1 mod 2^384: the one value every Montgomery reduction of a b gives"""
    t = a * b
    m = (t * QNEGINV) % R
    r, rem = divmod(t + m * Q, R)
    assert rem == 0
    return r


def estimate_k(acc11):
    """fat_reduce's quotient estimate, the same IEEE double operations"""
    hf = float(acc11 >> 32) * 4294967296.0 + float(acc11 & M32)
    e = hf * (1.0 / 436277738.0) - 0.001
    return (int(e) if e > 0.0 else 0), e


def m_fat_reduce(limbs):
    k, _ = estimate_k(limbs[11])
    return (fat_value(limbs) + k * QC) % R


def m_lin_share(mn, k, cfs, ops):
    """one lane's accumulators as run_rounds leaves them; the bounds the code states are asserted on the way"""
    acc = [0] * 12
    assert 1 <= k <= LIN_MAXK and 0 <= mn <= k
    for p in range(k):
        if p > 0 and p == mn:
            acc = m_fat_flip(acc)
        w = words12(ops[p])
        acc = [a + cfs[p] * x for a, x in zip(acc, w)]
    if mn == k:
        acc = m_fat_flip(acc)
    return acc


def m_fat_flip(acc):
    assert all(0 <= a < 1 << 40 for a in acc), "fat_flip: a limb is not below 2^40"
    return [b - a for b, a in zip(BIAS_LIMBS, acc)]


def lin_value(mn, k, cfs, ops):
    """the integer a share stands for, from coefficients and operands alone"""
    v = sum(cfs[p] * ops[p] for p in range(mn, k)) - sum(cfs[p] * ops[p] for p in range(mn))
    return v + (BIAS if mn > 0 else 0)


def lin_words(mn, k, flags, levels, cfs, ops):
    cfs = list(cfs) + [0] * (LIN_MAXK - len(cfs))
    ops = list(ops) + [0] * (LIN_MAXK - len(ops))
    w = [mn, k, flags, levels] + cfs
    for x in ops:
        w += words12(x)
    assert len(w) == LIN_WIN
    return w


def lin_unwords(w):
    mn, k, flags, levels = w[:4]
    cfs = w[4:4 + LIN_MAXK]
    ops = [from_words(w[4 + LIN_MAXK + 12 * p: 4 + LIN_MAXK + 12 * (p + 1)]) for p in range(LIN_MAXK)]
    return mn, k, flags, levels, cfs, ops


def check_reduced(out_words, value):
    got = from_words(out_words)
    assert 0 <= got < 2 * Q, "not below 2q"
    assert (got - value) % Q == 0, "not congruent to V mod q"


def euler(a):
    return {0: 0, 1: 1, Q - 1: -1}[pow(a, (Q - 1) // 2, Q)]


# ---- the op table ------------------------------------------------------------------------------------------------------
class Op:
    def __init__(self, name, code, group, win, wout, ref, check=None, host=True, wave=False):
        self.name, self.code, self.group, self.win, self.wout = name, code, group, win, wout
        self.ref, self.check, self.host, self.wave = ref, check, host, wave
        self.sets = []                                 # (class, input words); lin_absorb: (class, round)

    def add(self, cls, words):
        words = [int(w) for w in words]
        assert len(words) == self.win and all(0 <= w <= M32 for w in words), (self.name, cls, len(words))
        self.sets.append((cls, words))


OPS = {}
GROUPS = ("products", "linear", "fat", "decisions", "inversions")


def defop(*a, **k):
    op = Op(*a, **k)
    OPS[op.name] = op
    return op


def two(w):
    return from_words(w[:12]), from_words(w[12:24])


# ---- products ----------------------------------------------------------------------------------------------------------
def _chk_prod(bound):
    def chk(w, out):
        a, b = two(w) if len(w) == 24 else (from_words(w), from_words(w))
        r = from_words(out)
        assert r < bound, "result not below the bound"
        assert (r * R - a * b) % Q == 0, "r R != a b (mod q)"
    return chk


def ref_mul(w):
    a, b = two(w)
    r = mont(a, b)
    return words12(r - Q if r >= Q else r)


def ref_mul_relaxed(w):
    a, b = two(w)
    r = mont(a, b)
    assert r < 2 * Q
    return words12(r)


def ref_sqr_relaxed(w):
    a = from_words(w)
    r = mont(a, a)
    assert r < 2 * Q
    return words12(r)


def build_products():
    rnd = _rnd("products")
    canon = defop("fq_mul", 0, "products", 24, 12, ref_mul, _chk_prod(Q))
    ce = [0, 1, Q - 1, Q - 2, ONE, R * R % Q, ALT_EVEN, ALT_ODD & ((1 << 352) - 1), (1 << 380) - 1] + POW32 + POW32M1[:11]
    assert all(v < Q for v in ce)
    seen = set()

    def addp(op, cls, a, b):
        if (a, b) not in seen:
            seen.add((a, b))
            op.add(cls, words12(a) + words12(b))
    for a in ce:
        for b in (a, Q - 1, ALT_EVEN):
            addp(canon, "edge", a, b)
        addp(canon, "edge", Q - 1, a)
        addp(canon, "edge", a, rnd.randrange(Q))
    for _ in range(40):
        addp(canon, "random", rnd.randrange(Q), rnd.randrange(Q))
    for a, b in CARRY_PAIRS["fq_mul"]:
        assert a < Q and b < Q
        addp(canon, "carry", a, b)

    relaxed = defop("fq_mul_relaxed", 1, "products", 24, 12, ref_mul_relaxed, _chk_prod(2 * Q))
    seen = set()
    lim = 9 * Q * Q
    re_ = [0, 1, Q - 1, Q, Q + 1, 2 * Q - 1, 2 * Q, 3 * Q - 1, ONE, R * R % Q, ALL1, ALT_ODD, ALT_EVEN] + POW32 + POW32M1[:11]
    for a in re_:
        partners = [a, 3 * Q - 1, 2 * Q - 1, 1]
        if a:
            partners.append(min((lim - 1) // a, ALL1))      # the largest partner the bound admits
        for b in partners:
            if a * b < lim:
                addp(relaxed, "edge", a, b)
                if b in (3 * Q - 1,) or a == ALL1:
                    addp(relaxed, "edge", b, a)
    for _ in range(32):
        addp(relaxed, "random", rnd.randrange(3 * Q), rnd.randrange(3 * Q))
    for a, b in CARRY_PAIRS["fq_mul_relaxed"]:
        assert a * b < lim
        addp(relaxed, "carry", a, b)

    sqr = defop("fq_sqr_relaxed", 2, "products", 12, 12, ref_sqr_relaxed, _chk_prod(2 * Q))
    top3 = (3 * Q) >> 352                                     # 0x4e0335be
    se = [0, 1, Q - 1, Q, Q + 1, 2 * Q - 1, 2 * Q, 3 * Q - 1, ONE, R * R % Q, ALT_EVEN,
          (ALT_ODD & ((1 << 352) - 1)) | ((top3 - 1) << 352),            # alternating limbs, the top one just below 3q's
          ((1 << 352) - 1) | ((top3 - 1) << 352),                        # every lower limb all ones
          sum(0x80000000 << (32 * j) for j in range(11)),                # every doubling carries into the next limb
          sum(0x7FFFFFFF << (32 * j) for j in range(11))] + POW32 + POW32M1[:11]
    se += [(1 << (32 * k + 31)) for k in range(11)]
    for a in se:
        assert a < 3 * Q
        sqr.add("edge", words12(a))
    for _ in range(40):
        sqr.add("random", words12(rnd.randrange(3 * Q)))


# ---- linear ------------------------------------------------------------------------------------------------------------
def build_linear():
    rnd = _rnd("linear")
    edge = [0, 1, 2, Q - 1, Q - 2, ONE, ALT_EVEN, HALF, HALF + 1] + POW32 + POW32M1[:11]

    def chk_add(w, out):
        a, s = two(w)
        assert from_words(out) == (a + s) % Q
    add = defop("fq_add_mod", 10, "linear", 24, 12, lambda w: words12(sum(two(w)) % Q), chk_add)
    for a in edge:
        for s in (0, 1, Q, Q - 1, Q - a, (Q - a - 1) % Q, rnd.randrange(Q + 1)):
            add.add("edge", words12(a) + words12(s))
    for _ in range(24):
        add.add("random", words12(rnd.randrange(Q)) + words12(rnd.randrange(Q + 1)))
    del add.sets[MAX_SETS:]

    def chk_neg(w, out):
        assert from_words(out) + from_words(w) == Q
    neg = defop("fq_neg_raw", 11, "linear", 12, 12, lambda w: words12(Q - from_words(w)), chk_neg)
    for s in edge + [Q] + [Q - v for v in POW32]:
        neg.add("edge", words12(s))
    for _ in range(24):
        neg.add("random", words12(rnd.randrange(Q + 1)))

    def chk_sub(w, out):
        x, y = two(w)
        assert from_words(out) == (x - y) % Q
    sub = defop("fq_sub_mod", 12, "linear", 24, 12, lambda w: words12((two(w)[0] - two(w)[1]) % Q), chk_sub)
    for x in edge:
        for y in (x, 0, 1, Q - 1, (x + 1) % Q, rnd.randrange(Q)):
            sub.add("edge", words12(x) + words12(y))
    for v in POW32:
        sub.add("edge", words12(0) + words12(v))
    for _ in range(24):
        sub.add("random", words12(rnd.randrange(Q)) + words12(rnd.randrange(Q)))
    del sub.sets[MAX_SETS:]

    def chk_canon(w, out):
        x = from_words(w)
        assert from_words(out) == x % Q
    can = defop("fq_canon", 13, "linear", 12, 12, lambda w: words12(from_words(w) % Q), chk_canon)
    vals = [0, 1, Q - 1, Q, Q + 1, 2 * Q - 1, 2 * Q - 2, HALF, ONE, ONE + Q]
    for k in range(12):                                       # q with one word one up / one down
        vals += [Q + (1 << (32 * k)), Q - (1 << (32 * k))]
    vals += POW32 + POW32M1[:11] + [v + Q for v in POW32]
    for v in vals:
        assert 0 <= v < 2 * Q
        can.add("edge", words12(v))
    for _ in range(32):
        can.add("random", words12(rnd.randrange(2 * Q)))

    isz = defop("fq_is_zero", 14, "linear", 12, 1, lambda w: [int(from_words(w) == 0)], lambda w, out: None)
    for v in [0, 1, Q, ALL1] + POW32 + [1 << (32 * k + 31) for k in range(12)]:
        isz.add("edge", words12(v))
    for _ in range(8):
        isz.add("random", words12(rnd.randrange(R)))


# ---- fat accumulators and LIN shares -----------------------------------------------------------------------------------
def decompositions(v):
    """v < 2^396 as twelve fat limbs below 2^44, three ways (the module docstring)"""
    tight = [(v >> (32 * j)) & M32 for j in range(11)] + [v >> 352]
    ceil = list(tight)
    for _ in range(3):
        for j in range(10, -1, -1):
            t = min(ceil[j + 1], (FAT_LIMIT - 1 - ceil[j]) >> 32)
            ceil[j + 1] -= t
            ceil[j] += t << 32
    rnd = random.Random(v)
    spread = list(tight)
    for j in range(10, -1, -1):
        t = min(spread[j + 1], rnd.randrange(1 << 12))
        spread[j + 1] -= t
        spread[j] += t << 32
    return (("tight", tight), ("ceil", ceil), ("spread", spread))


def reduce_values():
    kmax = (V_LIMIT - 1) // Q
    ks = [0, 1, 2] + [1 << i for i in range(2, 16)] + [kmax]
    vals = []
    for k in ks:
        for v in [k * Q + d for d in (0, 1, Q - 1)] + ([k * Q - 1] if k >= 1 else []):
            if v < V_LIMIT and v not in vals:
                vals.append(v)
    vals.append(V_LIMIT - 1)
    return vals


def build_fat():
    rnd = _rnd("fat")

    def ref_mac(w):
        acc, s, cf = fat_limbs(w[:24]), w[24:36], w[36]
        return fat_words([a + cf * x for a, x in zip(acc, s)])
    mac = defop("fat_mac_plain", 20, "fat", 37, 24, ref_mac, lambda w, out: None)
    ones = [M32] * 12
    for cf in (0, 1, 31):
        for acc in ([0] * 12, [(1 << 40) - 1] * 12, BIAS_LIMBS, [FAT_LIMIT - 1 - 31 * M32] * 12, [(1 << 64) - 1 - 31 * M32] * 12):
            for s in (ones, [0] * 12, words12(2 * Q - 1), words12(ALT_ODD)):
                mac.add("edge", fat_words(acc) + s + [cf])
    for _ in range(24):
        mac.add("random", fat_words([rnd.randrange(1 << 43) for _ in range(12)]) + words12(rnd.randrange(R)) + [rnd.randrange(32)])

    flip = defop("fat_flip", 21, "fat", 24, 24, lambda w: fat_words(m_fat_flip(fat_limbs(w))),
                 lambda w, out: check_flip(w, out))
    for acc in ([0] * 12, [(1 << 40) - 1] * 12, [1 << 39] * 12, [NEG_CF_MAX * M32] * 12, [1] * 12, [M32] * 12, [1 << 32] * 12,
                [(1 << 40) - 1 if j % 2 else 0 for j in range(12)], [0 if j % 2 else (1 << 40) - 1 for j in range(12)]):
        flip.add("edge", fat_words(acc))
    for _ in range(24):
        flip.add("random", fat_words([rnd.randrange(1 << 40) for _ in range(12)]))

    red = defop("fat_reduce", 22, "fat", 24, 12, lambda w: words12(m_fat_reduce(fat_limbs(w))),
                lambda w, out: check_reduced(out, fat_value(fat_limbs(w))))
    for v in reduce_values():
        for cls, limbs in decompositions(v):
            red.add(cls, fat_words(limbs))
    for _ in range(6):
        for cls, limbs in decompositions(rnd.randrange(V_LIMIT)):
            red.add("random", fat_words(limbs))
    assert len(red.sets) <= MAX_SETS, len(red.sets)

    def ref_lin(w):
        mn, k, _, _, cfs, ops = lin_unwords(w)
        acc = m_lin_share(mn, k, cfs, ops)
        assert all(0 <= a < FAT_LIMIT for a in acc)
        return words12(m_fat_reduce(acc))

    def chk_lin(w, out):
        mn, k, _, _, cfs, ops = lin_unwords(w)
        check_reduced(out, lin_value(mn, k, cfs, ops))
    lin = defop("lin", 23, "fat", LIN_WIN, 12, ref_lin, chk_lin)
    OPERANDS = (0, 2 * Q - 1, ALL1)

    def operand(kind, p):
        if kind < 3:
            return OPERANDS[kind]
        if kind == 3:
            return rnd.randrange(2 * Q)
        return OPERANDS[p % 3]                                # mixed

    def neg_cfs(n, mode):
        """n negative coefficients with sum <= 255: mode 1 all ones, 31 as many 31s as the budget allows, 0 random"""
        if mode == 1:
            return [1] * n
        out, left = [], NEG_CF_MAX
        for p in range(n):
            room = left - (n - p - 1)                         # the rest need at least 1 each
            c = min(31, room) if mode == 31 else rnd.randrange(1, min(31, room) + 1)
            out.append(c)
            left -= c
        return out
    kind = 0
    for k in range(1, LIN_MAXK + 1):
        for mn_mode, cf_modes in (("none", (1, 31)), ("all", (1, 31)), ("mixed", (1, 31, 0))):
            if mn_mode == "mixed" and k < 2:
                continue
            mn = {"none": 0, "all": k, "mixed": (k + 1) // 2}[mn_mode]
            for cm in cf_modes:
                cfs = neg_cfs(mn, cm) + [(1 if cm == 1 else 31 if cm == 31 else rnd.randrange(1, 32)) for _ in range(k - mn)]
                ops = [operand(kind % 5, p) for p in range(k)]
                kind += 1
                lin.add("mn_" + mn_mode, lin_words(mn, k, 0, 0, cfs, ops))
    # the negative sum exactly 255, on operands of all-ones limbs: every accumulator limb 255 (2^32 - 1) at the flip
    for cfs, npos in (([31] * 8 + [7], 0), ([31] * 8 + [7], 21), ([9] * 15 + [8] * 15, 0), ([31] * 8 + [7], 1)):
        mn = len(cfs)
        lin.add("neg255", lin_words(mn, mn + npos, 0, 0, cfs + [31] * npos, [ALL1] * (mn + npos)))
    assert len(lin.sets) <= MAX_SETS, len(lin.sets)

    ab = defop("lin_absorb", 24, "fat", LIN_WIN, 12, None, None, host=False, wave=True)
    for r in absorb_rounds(rnd):
        ab.sets.append(("round", r))


def check_flip(w, out):
    acc, got = fat_limbs(w), fat_limbs(out)
    assert fat_value(got) + fat_value(acc) == BIAS and all(0 <= g < 1 << 64 for g in got)


# a lin_absorb round: dict(mn, k, levels, lanes = 64 x (flags, cfs, ops)); groups are aligned, 4 / 2 / 1 lanes wide
POS_GROUP_MAX = (FAT_LIMIT - 1 - 4 * max(BIAS_LIMBS)) // M32      # positive coefficients of a group of four: 3067


def absorb_rounds(rnd):
    def lanes_of(mn, k, groups, cf_of, op_of):
        lanes = []
        for gi, g in enumerate(groups):
            for part in range(g):
                flags = (1 << 14 if g >= 2 and part % 2 == 0 else 0) | (1 << 15 if g == 4 and part == 0 else 0)
                cfs = [cf_of(gi, part, p) for p in range(k)]
                # a shorter share is padded with zero micro-ops; the negative sum of a lane stays within 255
                while sum(cfs[:mn]) > NEG_CF_MAX:
                    cfs[max(range(mn), key=lambda p: cfs[p])] -= 1
                lanes.append((flags, cfs, [op_of(gi, part, p) for p in range(k)]))
        assert len(lanes) == 64
        return lanes
    vals = (ALL1, 2 * Q - 1, 0)
    rounds = []
    # 0: four-lane groups, pairs and single lanes in one round of two levels, 30 micro-ops, negatives and positives;
    #    group 0 carries the largest positive sum the 2^44 bound admits on all-ones operands, group 1 negatives of 255 per lane
    groups = [4] * 10 + [2] * 8 + [1] * 8

    def cf0(gi, part, p):
        if gi == 0:
            left = POS_GROUP_MAX - 31 * 26 * part
            return 31 if p < 4 else max(0, min(31, left - 31 * (p - 4)))
        if gi == 1:
            return 31 if p < 4 or p % 3 else 0
        return rnd.randrange(32) if (gi + p) % 4 else 0
    low1 = ((1 << 352) - 1) | (((2 * Q - 1) >> 352) << 352)   # lower limbs all ones under the top limb of 2q - 1: V stays below 2^396

    def op0(gi, part, p):
        if gi == 0:
            return 0 if p < 4 else low1
        return ALL1 if gi == 1 else (vals[(gi + p) % 3] if gi % 2 else rnd.randrange(2 * Q))
    rounds.append(dict(mn=4, k=30, levels=2, lanes=lanes_of(4, 30, groups, cf0, op0)))
    # 1: pairs and single lanes, one level, negatives (eight per lane, 255 in the pairs) and positives
    groups = [2] * 24 + [1] * 16
    rounds.append(dict(mn=9, k=14, levels=1, lanes=lanes_of(9, 14, groups,
                       lambda gi, part, p: ([31] * 8 + [7] + [31] * 5)[p] if gi < 12 else rnd.randrange(29),
                       lambda gi, part, p: ALL1 if gi % 2 == 0 else rnd.randrange(2 * Q))))
    # 2: two levels, every micro-op negative (the flip comes last)
    groups = [4] * 12 + [2] * 6 + [1] * 4
    rounds.append(dict(mn=10, k=10, levels=2, lanes=lanes_of(10, 10, groups,
                       lambda gi, part, p: 31 if gi == 0 else rnd.randrange(26),
                       lambda gi, part, p: vals[(gi + part) % 3] if gi < 6 else rnd.randrange(2 * Q))))
    # 3: no level: the merge flags of a lane are ignored
    lanes = lanes_of(2, 5, [4] * 8 + [2] * 16, lambda gi, part, p: rnd.randrange(1, 32), lambda gi, part, p: rnd.randrange(2 * Q))
    rounds.append(dict(mn=2, k=5, levels=0, lanes=lanes))
    # 4: one level, no negative term (no flip anywhere in the round)
    groups = [2] * 32
    rounds.append(dict(mn=0, k=7, levels=1, lanes=lanes_of(0, 7, groups,
                       lambda gi, part, p: 31 if gi < 4 else rnd.randrange(32),
                       lambda gi, part, p: ALL1 if gi < 4 else rnd.randrange(2 * Q))))
    return rounds


PERM_L1, PERM_L2 = (1, 1, 3, 3), (2, 2, 2, 2)                # the quad_perm of the two DPP steps


def _absorb(vals, flags, levels, add):
    for lv, perm, bit in ((1, PERM_L1, 14), (2, PERM_L2, 15)):
        if levels >= lv:
            vals = [add(vals[l], vals[(l & ~3) + perm[l & 3]]) if (flags[l] >> bit) & 1 else vals[l] for l in range(64)]
    return vals


_ABSORB = {}


def absorb_expected(k, nlive):
    """(expected words, integer value) of every lane of round k when lanes nlive .. 63 run zero shares"""
    if (k, nlive) not in _ABSORB:
        r = OPS["lin_absorb"].sets[k][1]
        mn, kk = r["mn"], r["k"]
        accs, ints, flags = [], [], []
        for l in range(64):
            f, cfs, ops = r["lanes"][l] if l < nlive else (0, [0] * kk, [0] * kk)
            accs.append(m_lin_share(mn, kk, cfs, ops))
            ints.append(lin_value(mn, kk, cfs, ops))
            flags.append(f)
        accs = _absorb(accs, flags, r["levels"], lambda a, b: [x + y for x, y in zip(a, b)])
        ints = _absorb(ints, flags, r["levels"], lambda a, b: a + b)
        for a in accs:
            assert all(0 <= x < FAT_LIMIT for x in a) and fat_value(a) < V_LIMIT
        _ABSORB[(k, nlive)] = ([words12(m_fat_reduce(a)) for a in accs], ints)
    return _ABSORB[(k, nlive)]


def absorb_lane_words(k, lane):
    r = OPS["lin_absorb"].sets[k][1]
    f, cfs, ops = r["lanes"][lane]
    return lin_words(r["mn"], r["k"], f, r["levels"], cfs, ops)


# ---- decisions ---------------------------------------------------------------------------------------------------------
def build_decisions():
    rnd = _rnd("decisions")

    def ref_sgn(w):
        c = from_words(w) * RINV % Q
        return words12(ONE if c > HALF else 0)
    sgn = defop("fq_sgn", 30, "decisions", 12, 12, ref_sgn, None)
    for c in [0, 1, 2, HALF - 1, HALF, HALF + 1, HALF + 2, Q - 2, Q - 1] + [rnd.randrange(Q) for _ in range(24)]:
        a = c * R % Q
        sgn.add("edge" if c < 3 or c > Q - 3 or abs(c - HALF) < 3 else "random", words12(a))
        sgn.add("relaxed", words12(a + Q))

    gt = defop("gt_half_q_mask", 31, "decisions", 12, 1, lambda w: [M32 if from_words(w) > HALF else 0], None)
    vals = [HALF - 1, HALF, HALF + 1, 0, Q - 1]
    for k in range(12):                                       # q // 2 with exactly one word changed, either way
        hw = (HALF >> (32 * k)) & M32
        vals += [HALF + (1 << (32 * k)) if hw < M32 else HALF - (1 << (32 * k)), HALF - (1 << (32 * k)) if hw > 0 else HALF + (1 << (32 * k))]
        vals += [HALF - (hw << (32 * k)), HALF + ((M32 - hw) << (32 * k))]            # that word 0 and all ones
    for v in vals:
        gt.add("edge", words12(v))
    for _ in range(16):
        gt.add("random", words12(rnd.randrange(Q)))

    def chk_jac(w, out):
        assert out[0] != 2, "fq_jacobi_var did not converge"
    jac = defop("fq_jacobi_var", 32, "decisions", 12, 1, lambda w: [euler(from_words(w)) & M32], chk_jac)
    for a in JACOBI_CORNERS:
        jac.add("edge", words12(a))
    for a in [rnd.randrange(Q) for _ in range(120)] + [rnd.randrange(1 << k) for k in (8, 64, 200, 380) for _ in range(12)]:
        jac.add("random", words12(a))


# ---- inversions --------------------------------------------------------------------------------------------------------
def inv_ref(a):
    c = a % Q
    return pow(c, -1, Q) * R * R % Q if c else 0


def chk_inv1(a, r):
    assert r < Q, "not canonical"
    assert (r * a - R * R) % Q == 0 if a % Q else r == 0, "r a != R^2 (mod q)"


def inversion_values():
    rnd = _rnd("inversions")
    vals = []
    for v in INV_CORNERS + INV_PATTERNS:
        if v not in vals:
            vals.append(v)
    vals += [rnd.randrange(Q) for _ in range(48)] + [Q + rnd.randrange(Q) for _ in range(16)]
    # zero (and its relaxed form q) between non-zero values, so that lanes of one wavefront end at different batches
    for at in (40, 80, 120):
        vals.insert(at, 0 if at != 80 else Q)
    assert len(vals) <= MAX_SETS and all(0 <= v < 2 * Q for v in vals)
    return vals


def build_inversions():
    vals = inversion_values()
    for name, code in (("fq_inv", 40), ("fq_inv_var", 41)):
        op = defop(name, code, "inversions", 12, 12, lambda w: words12(inv_ref(from_words(w))),
                   lambda w, out: chk_inv1(from_words(w), from_words(out)))
        for v in vals:
            op.add("zero" if v % Q == 0 else "value", words12(v))

    def ref_uni(w):
        return [x for t in range(UNI) for x in words12(inv_ref(from_words(w[12 * t:12 * t + 12])))]

    def chk_uni(w, out):
        for t in range(UNI):
            chk_inv1(from_words(w[12 * t:12 * t + 12]), from_words(out[12 * t:12 * t + 12]))
    first = [0, 1, ONE, Q - 1, Q, (1 << 380) % Q, 2 * Q - 1, Q + 1]
    for name, code in (("fq_inv_uni", 42), ("fq_inv_var_uni", 43)):
        op = defop(name, code, "inversions", 12 * UNI, 12 * UNI, ref_uni, chk_uni, wave=True)
        op.add("uniform", [x for v in first for x in words12(v)])
        for s in range(1, 5):
            pick = vals[s::5][:UNI]
            op.add("uniform", [x for v in pick for x in words12(v)])


def build_all():
    build_products()
    build_linear()
    build_fat()
    build_decisions()
    build_inversions()
    for op in OPS.values():
        assert 0 < len(op.sets) <= MAX_SETS, (op.name, len(op.sets))


build_all()

_EXPECTED = {}


def expected(name):
    """the expected output words of every set of a lane-layout op (computed once)"""
    if name not in _EXPECTED:
        op = OPS[name]
        assert op.ref is not None
        _EXPECTED[name] = [[int(v) & M32 for v in op.ref(w)] for _, w in op.sets]
    return _EXPECTED[name]


def call(name, n):
    """a call with n items: (input words, set index of each item, expected words of each item,
    independent check of each item: a function of the item's output words, or None)"""
    op = OPS[name]
    ns = len(op.sets)
    words, idx, want, chk = [], [], [], []
    if name == "lin_absorb":
        for i in range(n):
            w, lane = i // 64, i % 64
            k = item_set(w, ns)
            nlive = min(64, n - 64 * w)
            exp, ints = absorb_expected(k, nlive)
            words += absorb_lane_words(k, lane)
            idx.append(k)
            want.append(exp[lane])
            chk.append(lambda out, v=ints[lane]: check_reduced(out, v))
        return words, idx, want, chk
    exp = expected(name)
    for i in range(n):
        k = item_set(i // 64 if op.wave else i, ns)
        w = op.sets[k][1]
        words += w
        idx.append(k)
        want.append(exp[k])
        chk.append((lambda out, w=w: op.check(w, out)) if op.check is not None else None)
    return words, idx, want, chk


if __name__ == "__main__":
    for g in GROUPS:
        for op in OPS.values():
            if op.group == g:
                cls = {}
                for c, _ in op.sets:
                    cls[c] = cls.get(c, 0) + 1
                print("%-10s %-16s %3d  %s" % (g, op.name, len(op.sets), " ".join("%s=%d" % kv for kv in cls.items())))
