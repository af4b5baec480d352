"""Operand sets and CPU references for the scalar-field and byte-hashing layer (csrc/fr_scalar.h, hd_derive.h, hash_pks.h,
sigdiv.h, secret_window.h), one list per op of the test-only device library csrc/blsgpu_fr_check.hip.  Pure Python:
tests/test_fr_vectors_model.py runs the host build of the same op bodies on the same sets against the same references,
checks the preconditions every set claims and that a list of mutated references is caught; tests/test_gpu_fr.py compares
the compiled kernels with them word for word.

References, none shared with the device code and none from the C oracle:
  * scalars: Python integers -- a b R^-1 mod n, pow(a, -1, n) with 0 -> 0, the barycentric weights, Horner;
  * hashing: hashlib.sha256 and hmac; a plain FIPS 180-4 compression in Python (sha_compress) where a chaining state is an
    operand (the midstates of a key), itself held against hashlib by the model test;
  * windows: vmgen.g2smul_model.recode (vmgen.g1fixs_model uses the same function) and the identity sum_w d_w 16^w = s.
cios() is a word-level emulation of frs::mul's loop that reports what happened on the way (the quotient words m, word 8 of
every outer step, whether the last subtraction fired); the product sets that claim such a property were found with it and
the model test asserts that they have it.  Which sets reach which property of a Montgomery product:
  * the last subtraction fires / does not fire: the classes `fires` (results 1 and 2) and `stays` (results 1, 2, n - 1 and
    n - 2; a sum that fires is below n (n + R) / R < 1.46 n, so n - 1 cannot come out of a subtraction), and the random pairs
    either way.  A running sum EQUAL to n before the subtraction -- the only input on which `>` and `>=`
    differ -- is unreachable for a, b < n (a b + m n = n R needs n | a b); the class `wide_b` reaches it with b = n;
  * word 8 non-zero after the multiply pass of step i, for each of the eight steps: every random pair;
    word 8 zero at every step: (1, 1), (0, x);
  * m = 0: a = 0 (every step); m = 0xFFFFFFFF: (1, 1), step 0;
  * result 0: a or b = 0 (the only way: n is prime); result n - 1: (n - 1, R mod n) and the `stays` / `fires` pairs;
  * `t[8] + (uint32_t)c` carrying out of 32 bits is unreachable inside the contract (a < n keeps the sum below 2n < 2^256,
    see the header of csrc/blsgpu_fr_check.hip) and is not searched for.
The top digit (w = 64) of a recoding is 0 or +1, never negative: s + C < 2 * 16^64, so its nibble is 8 or 9.

Layout: item i of a call holds set (37 i mod 257) mod nsets, whatever the number of items (N_ITEMS), so 257 items meet
every set.  inv_uni is laid out by WAVEFRONT (Op.wave): every lane of wavefront w holds set (37 w mod 257) mod nsets.
select_g2 is lane-strided (Op.strided): ad, keep0 of every item, then dword d of item i's table at word 2 n + d n + i.
BYTES travel as they lie in memory, four to a little-endian word.
"""
import hashlib
import hmac
import random
import struct

from frsecret_vectors import EDGE as Y_EDGE
from fq32_vectors import Q
from vmgen import g1fixs_model, g2smul_model

N = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
R = 1 << 256
RINV = pow(R, -1, N)
NNEGINV = (-pow(N, -1, R)) % R
R1 = R % N
R2 = R * R % N
M32 = 0xFFFFFFFF
ALL1 = R - 1
N_ITEMS = (1, 63, 64, 65, 257)                         # items per call: one lane, either side of a wavefront, two workgroups
MAX_SETS = 257
STRIDE = 37                                            # coprime to 64 and to 257
MAXK, MAXT, MSGW, MAXKEYS, DIGITS = 67, 16, 52, 9, 65  # csrc/blsgpu_fr_check.hip
G1_DW, G2_DW = 28, 42                                  # g1fix::ENTRY_DW, g2smul::PT_DW
IV = (0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19)
ALT = sum(M32 << (32 * j) for j in range(1, 8, 2))    # words 1, 3, 5, 7 all ones
POW32 = [1 << (32 * k) for k in range(8)]
POW32M1 = [(1 << (32 * k)) - 1 for k in range(1, 9)]   # the last one is ALL1
LONG_LENS = (0, 1, 54, 55, 56, 63, 64, 65, 118, 119, 120, 127, 128, 200)
# the 256-bit edge values; BELOW_N is the part an op with the `below n` contract takes
WIDE = [0, 1, 2, N - 1, N, N + 1, 2 * N - 1, 2 * N, 2 * N + 1, 1 << 255, ALL1, R1, R2, ALT, ALL1 ^ ALT] + POW32 + POW32M1
BELOW_N = [v for v in dict.fromkeys(WIDE) if v < N]


def words8(x):
    assert 0 <= x < R, x
    return [(x >> (32 * i)) & M32 for i in range(8)]


def from_words(ws):
    return sum((w & M32) << (32 * i) for i, w in enumerate(ws))


def bytes_words(b):
    b = bytes(b) + b"\0" * (-len(b) % 4)
    return list(struct.unpack("<%dI" % (len(b) // 4), b))


def words_bytes(ws):
    return struct.pack("<%dI" % len(ws), *ws)


def be_words(x):
    """x as 32 bytes big-endian, as words in memory"""
    return bytes_words(x.to_bytes(32, "big"))


def from_be_words(ws):
    return int.from_bytes(words_bytes(ws), "big")


def be_state(ws):
    """big-endian words (a SHA-256 state) -> bytes"""
    return struct.pack(">%dI" % len(ws), *ws)


def state_words(b):
    return list(struct.unpack(">%dI" % (len(b) // 4), b))


def item_set(i, nsets):
    return ((i * STRIDE) % MAX_SETS) % nsets


def _rnd(name):
    return random.Random("fr:" + name)


# ---- references --------------------------------------------------------------------------------------------------------
def mont(a, b):
    """a b R^-1 mod n"""
    return a * b * RINV % N


def pre_sub(a, b):
    """frs::mul's running sum before the last subtraction: (a b + m n) / R, m = -a b n^-1 mod R (unique)"""
    t = a * b
    v, rem = divmod(t + (t * NNEGINV % R) * N, R)
    assert rem == 0
    return v


def cios(a, b, ge=True, drop_t8=False, m_from=0):
    """frs::mul word for word -> (result, quotient words m, word 8 after each multiply pass, the last subtraction fired).
    ge / drop_t8 / m_from are the mutations of the model test."""
    aw, bw, nw = words8(a), words8(b), words8(N)
    t, ms, t8s = [0] * 9, [], []
    for i in range(8):
        c = 0
        for j in range(8):
            c += aw[j] * bw[i] + t[j]
            t[j] = c & M32
            c >>= 32
        t[8] = c & M32
        t8s.append(t[8])
        m = (-t[m_from]) & M32
        ms.append(m)
        c = (m * nw[0] + t[0]) >> 32
        for j in range(1, 8):
            c += m * nw[j] + t[j]
            t[j - 1] = c & M32
            c >>= 32
        t[7] = ((0 if drop_t8 else t[8]) + c) & M32
    v = from_words(t[:8])
    fired = v >= N if ge else v > N
    return ((v - N) % R if fired else v), ms, t8s, fired


_K = None


def sha_compress(state, block):
    """FIPS 180-4 6.2.2 on 8 state words and 16 big-endian message words"""
    global _K
    if _K is None:
        primes = [p for p in range(2, 312) if all(p % d for d in range(2, int(p ** 0.5) + 1))][:64]

        def frac_cbrt(p):                                  # floor(2^32 frac(p^(1/3))) by integer search
            lo, hi = 0, 1 << 36
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (mid, hi) if mid ** 3 <= p << 96 else (lo, mid)
            return lo & M32
        _K = [frac_cbrt(p) for p in primes]
        assert _K[0] == 0x428a2f98 and _K[63] == 0xc67178f2
    rotr = lambda x, n: ((x >> n) | (x << (32 - n))) & M32
    w = list(block)
    for i in range(16, 64):
        s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)
        s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10)
        w.append((w[i - 16] + s0 + w[i - 7] + s1) & M32)
    a, b, c, d, e, f, g, h = state
    for i in range(64):
        t1 = (h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g & M32)) + _K[i] + w[i]) & M32
        t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & M32
        h, g, f, e, d, c, b, a = g, f, e, (d + t1) & M32, c, b, a, (t1 + t2) & M32
    return [(x + y) & M32 for x, y in zip(state, (a, b, c, d, e, f, g, h))]


def sha_blocks(state, data):
    assert len(data) % 64 == 0
    for o in range(0, len(data), 64):
        state = sha_compress(state, state_words(data[o:o + 64]))
    return list(state)


def key_states(key):
    """the midstates of util.hmac256's key blocks: ipad, opad (16 words)"""
    assert len(key) <= 64
    k = bytes(key) + b"\0" * (64 - len(key))
    return sha_blocks(IV, bytes(x ^ 0x36 for x in k)) + sha_blocks(IV, bytes(x ^ 0x5c for x in k))


def hmac_words(key, msg):
    return state_words(hmac.new(bytes(key), bytes(msg), hashlib.sha256).digest())


def padded(msg, total_before=64, extra_blocks=0):
    """msg with SHA-256 padding for a message that follows total_before hashed bytes"""
    p = bytes(msg) + b"\x80"
    p += b"\0" * ((-len(p) - 8) % 64 + 64 * extra_blocks)
    return p + struct.pack(">Q", 8 * (total_before + len(msg)))


def hdk_blocks(n, suffix=False):
    """hdk::long_blocks' formula, held against the padding itself by the model test"""
    return (n + (1 if suffix else 0) + 8) // 64 + 1


def hmac_from_states(states, msg, extra_blocks=0):
    """HMAC from the key's midstates, on sha_compress alone (the second reference of the long form; the mutants)"""
    inner = sha_blocks(states[:8], padded(msg, 64, extra_blocks))
    return sha_blocks(states[8:], padded(be_state(inner), 64))


def digits_of(s):
    d = g2smul_model.recode(s)
    assert d == g1fixs_model.recode(s)
    return d


def digit_words(ds):
    out = []
    for d in ds:
        out += [M32 if d < 0 else 0, abs(d), M32 if d == 0 else 0]
    return out


# ---- the op table ------------------------------------------------------------------------------------------------------
class Op:
    def __init__(self, name, code, group, win, wout, ref, check=None, host=True, wave=False, strided=False):
        self.name, self.code, self.group, self.win, self.wout = name, code, group, win, wout
        self.ref, self.check, self.host, self.wave, self.strided = ref, check, host, wave, strided
        self.sets = []                                 # (class, input words)

    def add(self, cls, words):
        words = [int(w) for w in words]
        assert len(words) <= self.win and all(0 <= w <= M32 for w in words), (self.name, cls, len(words))
        self.sets.append((cls, words + [0] * (self.win - len(words))))


OPS = {}
GROUPS = ("reduce", "products", "inversions", "lagrange", "sigdiv", "sha", "window")


def defop(*a, **k):
    op = Op(*a, **k)
    OPS[op.name] = op
    return op


def two(w):
    return from_words(w[:8]), from_words(w[8:16])


# ---- reduce ------------------------------------------------------------------------------------------------------------
def build_reduce():
    rnd = _rnd("reduce")

    def chk_mod(bound):
        def chk(w, out):
            r, x = from_words(out), from_words(w)
            assert r < bound and (r - x) % N == 0 and x - r in (0, N, 2 * N)
        return chk
    one_sub = lambda w: words8(from_words(w) - N if from_words(w) >= N else from_words(w))
    full = lambda w: words8(from_words(w) % N)
    near = [N + (1 << (32 * k)) for k in range(8)] + [N - (1 << (32 * k)) for k in range(8)]
    for code, name, ref in ((0, "sub_n_if_ge", one_sub), (3, "sub_n_if_ge_masked", one_sub), (1, "reduce_n", full), (4, "reduce_n_masked", full)):
        op = defop(name, code, "reduce", 8, 8, ref, chk_mod(N if "reduce" in name else R))
        for v in WIDE + [2 * N - (1 << 32), 2 * N + (1 << 224)] + near + [2 * N - 1 - v for v in POW32]:
            op.add("edge", words8(v % R))
        for _ in range(32):
            op.add("random", words8(rnd.randrange(R)))

    def chk_add(w, out):
        a, b = two(w)
        assert from_words(out) == (a + b) % N
    add_ref = lambda w: words8(sum(two(w)) % N)
    for code, name in ((2, "add_mod_n"), (5, "add_mod_n_masked"), (10, "add"), (11, "add_masked")):
        op = defop(name, code, "reduce", 16, 8, add_ref, chk_add)
        for a in BELOW_N:
            for b in dict.fromkeys((0, 1, N - 1, N - a if a else 0, (N - a - 1) % N, (N - a + 1) % N, rnd.randrange(N))):
                op.add("edge", words8(a) + words8(b))
        for _ in range(24):
            op.add("random", words8(rnd.randrange(N)) + words8(rnd.randrange(N)))
        del op.sets[MAX_SETS:]

    below = defop("below_n", 6, "reduce", 8, 1, lambda w: [int(from_words(w) < N)])
    for v in WIDE + near + [rnd.randrange(R) for _ in range(16)]:
        below.add("edge", words8(v))
    for k in range(8):                                        # n with word k all ones / zero: the borrow chain at every word
        nk = (N >> (32 * k)) & M32
        below.add("edge", words8(N + ((M32 - nk) << (32 * k))))
        below.add("edge", words8(N - (nk << (32 * k))))
    isz = defop("is_zero", 7, "reduce", 8, 1, lambda w: [int(from_words(w) == 0)])
    for v in [0, 1, N, ALL1] + POW32 + [1 << (32 * k + 31) for k in range(8)] + [rnd.randrange(R) for _ in range(8)]:
        isz.add("edge", words8(v))

    def chk_sub(w, out):
        a, b = two(w)
        assert from_words(out) == (a - b) % N
    sub = defop("sub", 8, "reduce", 16, 8, lambda w: words8((two(w)[0] - two(w)[1]) % N), chk_sub)
    for a in BELOW_N:
        for b in dict.fromkeys((a, 0, 1, N - 1, (a + 1) % N, (a - 1) % N, rnd.randrange(N))):
            sub.add("edge", words8(a) + words8(b))
    for v in POW32:
        sub.add("edge", words8(0) + words8(v))
    for _ in range(24):
        sub.add("random", words8(rnd.randrange(N)) + words8(rnd.randrange(N)))
    del sub.sets[MAX_SETS:]

    def chk_neg(w, out):
        assert from_words(out) == (-from_words(w)) % N
    neg = defop("neg", 9, "reduce", 8, 8, lambda w: words8((-from_words(w)) % N), chk_neg)
    for v in BELOW_N + [N - v for v in POW32] + [rnd.randrange(N) for _ in range(24)]:
        neg.add("edge", words8(v))


# ---- products ----------------------------------------------------------------------------------------------------------
def find_pair(rnd, result, fires):
    """a seeded search with the emulation: a pair below n with the given result whose last subtraction fires / does not"""
    for i in range(256):
        # (a small result that stays needs a b = result R exactly, m = 0: powers of two do it; a random a never will)
        a = 1 << 128 if i == 0 and result < 1 << 120 else rnd.randrange(1, N)
        b = result * R % N * pow(a, -1, N) % N
        if (pre_sub(a, b) >= N) == fires:
            assert cios(a, b)[0] == result and cios(a, b)[3] == fires
            return a, b
    raise AssertionError("no pair found")


def build_products():
    rnd = _rnd("products")

    def chk_prod(w, out):
        a, b = two(w) if len(w) == 16 else (from_words(w), from_words(w))
        r = from_words(out)
        assert r < N, "result not below n"
        assert (r * R - a * b) % N == 0, "r R != a b (mod n)"
    for code, name in ((20, "mul"), (21, "mul_masked")):
        op = defop(name, code, "products", 16, 8, lambda w: words8(mont(*two(w))), chk_prod)
        seen = set()

        def addp(cls, a, b, op=op, seen=seen):
            if (a, b) not in seen:
                seen.add((a, b))
                op.add(cls, words8(a) + words8(b))
        for a in BELOW_N:
            for b in (a, N - 1, R1, 1):
                addp("edge", a, b)
            addp("edge", N - 1, a)
            addp("edge", a, rnd.randrange(N))
        for _ in range(32):
            addp("random", rnd.randrange(N), rnd.randrange(N))
        for result in (1, 2, N - 1, N - 2):
            if result < N // 4:                               # (a sum that fires is below n (n + R) / R < 1.46 n: its result below 0.46 n)
                addp("fires", *find_pair(rnd, result, True))
            addp("stays", *find_pair(rnd, result, False))
        # b in [n, 2^256) with a below n: inside what the loop can take (the header of csrc/blsgpu_fr_check.hip); no call
        # site does this, the class states what comes out if one ever does
        for b in (N, N + 1, 2 * N - 1, 2 * N, 2 * N + 1, 1 << 255, ALL1, ALT, R - N):
            for a in (1, N - 1, R1, rnd.randrange(N), rnd.randrange(N)):
                addp("wide_b", a, b)
        assert len(op.sets) <= MAX_SETS, len(op.sets)

    sq = defop("sqr", 22, "products", 8, 8, lambda w: words8(mont(from_words(w), from_words(w))), chk_prod)
    for a in BELOW_N + [(N - 1) // 2, (N + 1) // 2] + [rnd.randrange(N) for _ in range(32)]:
        sq.add("edge", words8(a))

    def chk_to(w, out):
        assert from_words(out) == from_words(w) * R % N

    def chk_from(w, out):
        assert from_words(out) * R % N == from_words(w) and from_words(out) < N
    for code, name, ref, chk in ((23, "to_mont", lambda w: words8(from_words(w) * R % N), chk_to),
                                 (25, "to_mont_masked", lambda w: words8(from_words(w) * R % N), chk_to),
                                 (24, "from_mont", lambda w: words8(from_words(w) * RINV % N), chk_from),
                                 (26, "from_mont_masked", lambda w: words8(from_words(w) * RINV % N), chk_from)):
        op = defop(name, code, "products", 8, 8, ref, chk)
        for a in BELOW_N + [RINV, N - RINV] + [rnd.randrange(N) for _ in range(32)]:
            op.add("edge", words8(a))


# ---- inversions --------------------------------------------------------------------------------------------------------
def inv_ref(x):
    """Montgomery form in and out: (a R)^-1 R^2 = a^-1 R; 0 -> 0"""
    return pow(x, -1, N) * R2 % N if x else 0


def inversion_values():
    rnd = _rnd("inversions")
    vals = []
    for c in [0, 1, N - 1, 2, (N + 1) // 2, R1, R2, N - 2, 3] + [(1 << k) % N for k in range(5, 256, 23)]:
        for v in (c, c * R % N):                              # the value itself and its Montgomery form
            if v not in vals:
                vals.append(v)
    vals += [rnd.randrange(N) for _ in range(40)]
    for at in (7, 20, 33, 46, 59):                            # zero next to non-zero values
        vals.insert(at, 0)
    return vals


def build_inversions():
    rnd = _rnd("quotient")

    def chk_inv(w, out):
        x, r = from_words(w), from_words(out)
        assert r < N, "not canonical"
        assert mont(x, r) == (R1 if x else 0) and (x or r == 0), "x x^-1 != 1"
    vals = inversion_values()
    inv = defop("inv", 30, "inversions", 8, 8, lambda w: words8(inv_ref(from_words(w))), chk_inv)
    for v in vals:
        inv.add("zero" if v == 0 else "value", words8(v))
    uni = defop("inv_uni", 31, "inversions", 8, 8, lambda w: words8(inv_ref(from_words(w))), chk_inv, wave=True)
    for v in (R1, 0, N - 1, vals[-1], 2 * R % N):
        uni.add("uniform", words8(v))

    def ref_quot(w):
        a0, b0 = from_be_words(w[:8]) % N, from_be_words(w[8:]) % N
        q = a0 * pow(b0, -1, N) % N if b0 else 0
        return be_words((N - q) % N) + [int(q == 1)]

    def chk_quot(w, out):
        a0, b0 = from_be_words(w[:8]) % N, from_be_words(w[8:]) % N
        s = from_be_words(out[:8])
        assert s < N and ((N - s) * b0 - a0) % N == 0 if b0 else s == 0
        assert out[8] == int(b0 != 0 and a0 == b0)
    quot = defop("quotient_scalar", 32, "inversions", 16, 9, ref_quot, chk_quot)
    for a0, b0 in [(1, 1), (5, 5), (N + 5, 5), (2 * N + 5, N + 5), (0, 1), (1, 0), (0, 0), (N, 3), (3, N), (3, 2 * N), (1, N - 1), (N - 1, 1),
                   (ALL1, ALL1), (ALL1, 1), (1, ALL1), (2, 1), (1, 2), (1 << 255, 3)]:
        quot.add("edge", be_words(a0) + be_words(b0))
    for _ in range(24):
        b0 = rnd.randrange(R)
        quot.add("random", be_words(rnd.randrange(R)) + be_words(b0))
        quot.add("unit", be_words((b0 % N) + (N if b0 % N + N < R and rnd.random() < .5 else 0)) + be_words(b0))


# ---- lagrange ----------------------------------------------------------------------------------------------------------
def point_sets(rnd):
    """(class, k, j, canonical points with 0 for a refused one) for lagrange_weight"""
    out = []
    for k in (1, 2, 3, 67):
        js = sorted({0, k // 2, k - 1})
        base = list(range(1, k + 1))
        high = [N - 1 - i for i in range(k)]
        mixed = [rnd.randrange(1, N) for _ in range(k)]
        for j in js:
            out.append(("one_to_k", k, j, base))
            out.append(("top", k, j, high))
            out.append(("random", k, j, mixed))
            if k > 1:
                rep = list(mixed)
                rep[(j + 1) % k] = rep[j]                      # another point equals x_j: weight 0
                out.append(("repeated", k, j, rep))
                far = list(mixed)
                far[(j + 1) % k] = far[(j + 2) % k] if k > 2 else far[(j + 1) % k]   # a repeat elsewhere (k > 2): weight j stays non-zero
                out.append(("repeated_elsewhere", k, j, far))
                z = list(base)
                z[(j + 1) % k] = 0                             # a refused point (0, or >= n: lagrange_point stores 0) beside x_j
                out.append(("zero_other", k, j, z))
            z = list(base)
            z[j] = 0                                           # x_j itself refused: weight 0
            out.append(("zero_self", k, j, z))
    return out


def weight_value(xs, j):
    v = (-xs[j]) % N
    for i, x in enumerate(xs):
        if i != j:
            v = v * (xs[j] - x) % N
    return v


def build_lagrange():
    rnd = _rnd("lagrange")

    def ref_point(w):
        x = from_be_words(w)
        return (words8(x * R % N) + [1]) if 0 < x < N else [0] * 9
    lp = defop("lagrange_point", 40, "lagrange", 8, 9, ref_point)
    for x in WIDE + [rnd.randrange(N) for _ in range(16)] + [rnd.randrange(N, R) for _ in range(8)]:
        lp.add("refused" if x == 0 or x >= N else "point", be_words(x))

    def unpack_w(w):
        k, j = w[0], w[1]
        return k, j, [from_words(w[2 + 8 * i:10 + 8 * i]) * RINV % N for i in range(k)]
    lw = defop("lagrange_weight", 41, "lagrange", 2 + 8 * MAXK, 8, lambda w: words8(weight_value(unpack_w(w)[2], unpack_w(w)[1]) * R % N))
    for cls, k, j, xs in point_sets(rnd):
        assert 1 <= k <= MAXK and j < k and all(0 <= x < N for x in xs)
        lw.add(cls, [k, j] + [x for v in xs for x in words8(v * R % N)])

    def ref_den(w):
        s = sum(from_words(w[1 + 8 * i:9 + 8 * i]) for i in range(w[0])) % N
        return words8(inv_ref(s))
    ld = defop("lagrange_den", 42, "lagrange", 1 + 8 * MAXK, 8, ref_den)
    for k in (1, 2, 3, 67):
        for fill in ("random", "top", "cancel"):
            ss = [rnd.randrange(N) if fill == "random" else N - 1 for _ in range(k)]
            if fill == "cancel" and k > 1:
                ss = [rnd.randrange(N) for _ in range(k - 1)]
                ss.append((-sum(ss)) % N)                      # the shifts add up to 0: den = inv(0) = 0
            ld.add(fill, [k] + [x for v in ss for x in words8(v)])

    def chk_dot(w, out):
        assert from_words(out) == from_be_words(w[:8]) * (from_be_words(w[8:]) % N) % N
    ls = [0, 1, 2, N - 1, N - 2, R1, R2, (N + 1) // 2, rnd.randrange(N), rnd.randrange(N)]
    for code, name in ((43, "dot_term"), (44, "dot_term_masked")):
        op = defop(name, code, "lagrange", 16, 8, lambda w: words8(from_be_words(w[:8]) * (from_be_words(w[8:]) % N) % N), chk_dot)
        for l in ls:
            for y in Y_EDGE + [2 * N - 1, 2 * N, 2 * N + 1, rnd.randrange(R)]:
                op.add("edge", be_words(l) + be_words(y))
        for _ in range(24):
            op.add("random", be_words(rnd.randrange(N)) + be_words(rnd.randrange(R)))

    st = defop("sum_term_masked", 45, "lagrange", 16, 8, lambda w: words8((from_be_words(w[:8]) + from_words(w[8:])) % N))
    for acc in (0, 1, N - 1, (N - 1) // 2, rnd.randrange(N)):
        for y in WIDE[:11] + [N - acc, 2 * N - acc, (N - acc - 1) % R, rnd.randrange(R)]:
            st.add("edge", be_words(y % R) + words8(acc))

    for code, name in ((46, "poly_coeff_masked"), (47, "poly_point")):
        op = defop(name, code, "lagrange", 8, 8, lambda w: words8(from_be_words(w) % N * R % N))
        for v in WIDE + [rnd.randrange(R) for _ in range(24)]:
            op.add("edge", be_words(v))

    def ref_horner(w):
        t, x = w[0], from_words(w[1:9]) * RINV % N
        cs = [from_words(w[9 + 8 * k:17 + 8 * k]) * RINV % N for k in range(t)]
        return words8(sum(c * pow(x, k, N) for k, c in enumerate(cs)) % N)
    ph = defop("poly_horner_masked", 48, "lagrange", 9 + 8 * MAXT, 8, ref_horner)
    for t in (1, 2, 3, 16):
        for x in (0, 1, 2, N - 1, rnd.randrange(N), rnd.randrange(N)):
            for fill in ("random", "top", "zero_top"):
                cs = [rnd.randrange(N) if fill != "top" else N - 1 for _ in range(t)]
                if fill == "zero_top":
                    cs[-1] = 0
                ph.add(fill, [t] + words8(x * R % N) + [v for c in cs for v in words8(c * R % N)])


# ---- sigdiv ------------------------------------------------------------------------------------------------------------
def build_sigdiv():
    rnd = _rnd("sigdiv")
    ex = defop("sd_exponent", 50, "sigdiv", 8, 8, lambda w: words8(from_be_words(w) % N * R % N))
    for v in WIDE + [rnd.randrange(R) for _ in range(24)]:
        ex.add("edge", be_words(v))

    def quads(wide):
        lim = R if wide else N
        out = []
        for a0, b0, q in [(3, 1, 5), (1, 1, 1), (N - 1, N - 1, N - 1), (rnd.randrange(1, N), rnd.randrange(1, N), rnd.randrange(1, N)), (7, 11, 13),
                          (rnd.randrange(1, N), rnd.randrange(1, N), rnd.randrange(1, N))]:
            ae, be = a0 * q % N, b0 * q % N                    # a_e / b_e == a_0 / b_0
            out += [("equal", a0, b0, ae, be), ("entry0", a0, b0, a0, b0), ("differs", a0, b0, (ae + 1) % N, be), ("differs", a0, b0, ae, (be + 1) % N or 1),
                    ("zero_be", a0, b0, ae, 0), ("zero_b0", a0, 0, ae, be), ("zeros", 0, 0, 0, 0), ("zero_a", 0, b0, 0, be)]
            if wide:
                out += [("equal_wide", a0 + N, b0, ae, be + N), ("zero_be_wide", a0, b0, ae, N), ("zero_be_wide", a0, b0, ae, 2 * N)]
        out += [("random", *[rnd.randrange(lim) for _ in range(4)]) for _ in range(16)]
        return out
    ce = defop("sd_cross_equal", 51, "sigdiv", 32, 1, lambda w: [int((from_words(w[16:24]) * from_words(w[8:16]) - from_words(w[:8]) * from_words(w[24:])) % N == 0)])
    for cls, *v in quads(False):
        ce.add(cls, [x for t in v for x in words8(t * R % N)])

    def ref_bits(w):
        a0, b0, ae, be = (from_be_words(w[8 * i:8 * i + 8]) % N for i in range(4))
        return [int((ae * b0 - a0 * be) % N != 0) | (2 if be == 0 else 0)]
    eb = defop("sd_entry_bits", 52, "sigdiv", 32, 1, ref_bits)
    for cls, *v in quads(True):
        eb.add(cls, [x for t in v for x in be_words(t)])
    so = defop("sd_status_of", 53, "sigdiv", 2, 1, lambda w: [2 if w[1] else (1 if w[0] else 0)])
    for m in (0, 1):
        for z in (0, 1):
            so.add("all", [m, z])

    def coord(ws):
        return int.from_bytes(words_bytes(ws), "big")

    def neg_words(ws):
        y = coord(ws)
        return bytes_words(((Q - y) if y else 0).to_bytes(48, "big"))
    cvals = [0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, (Q + 1) // 2] + [1 << (32 * k) for k in range(12)] + [(1 << (32 * k)) - 1 for k in range(1, 12)]
    cvals += [Q - (1 << (32 * k)) for k in range(12)] + [rnd.randrange(Q) for _ in range(16)]
    nc = defop("sd_neg_coord", 54, "sigdiv", 12, 12, neg_words)
    for v in cvals:
        assert v < Q
        nc.add("zero" if v == 0 else "value", bytes_words(v.to_bytes(48, "big")))
    npt = defop("sd_neg_point", 55, "sigdiv", 48, 48, lambda w: w[:24] + neg_words(w[24:36]) + neg_words(w[36:48]))
    npt.add("infinity", [0] * 48)
    for i in range(24):
        cs = [rnd.randrange(Q), rnd.randrange(Q), cvals[i % len(cvals)], cvals[(3 * i + 1) % len(cvals)]]
        npt.add("point", [x for c in cs for x in bytes_words(c.to_bytes(48, "big"))])


# ---- sha ---------------------------------------------------------------------------------------------------------------
# i with SHA256(be32(i) || EXP_DIGEST) in [0, n), [n, 2n) and [2n, 2^256): found by a search on the CPU (the model test asserts them)
EXP_DIGEST = hashlib.sha256(b"fr_vectors: hpk::exponent").digest()
EXP_INDEX = {"below_n": (1, 2, 4, 0xFFFFFFFF), "n_to_2n": (0, 3, 6, 198), "above_2n": (9, 17, 23, 199)}


def exp_value(dg, i):
    return int.from_bytes(hashlib.sha256(struct.pack(">I", i) + bytes(dg)).digest(), "big")


def fills(rnd, n):
    return (("zeros", b"\0" * n), ("ones", b"\xff" * n), ("random", bytes(rnd.randrange(256) for _ in range(n))))


def long_message(w, hdr, length, shift):
    return words_bytes(w[hdr:])[shift:shift + length]


def place(msg, shift):
    """the message `shift` bytes into its words; the bytes around it are 0xA5 (nothing may read them)"""
    b = b"\xa5" * shift + bytes(msg)
    b += b"\xa5" * (4 * MSGW - len(b))
    return bytes_words(b)


def build_sha():
    rnd = _rnd("sha")
    rw = lambda n: [rnd.randrange(1 << 32) for _ in range(n)]
    sc = defop("sha_compress", 60, "sha", 24, 8, lambda w: sha_compress(w[:8], w[8:]))
    for blk in ([0] * 16, [M32] * 16, state_words(padded(b"abc", 0)), state_words(padded(b"", 0)), rw(16), rw(16)):
        sc.add("from_iv", list(IV) + blk)
        for st in ([0] * 8, [M32] * 8, rw(8)):
            sc.add("from_state", st + blk)

    hk = defop("hmac_key", 61, "sha", 17, 16, lambda w: key_states(words_bytes(w[1:])[:w[0]]))
    for klen in (0, 1, 31, 32, 33, 64, 20, 11):
        for cls, key in fills(rnd, klen):
            hk.add(cls, [klen] + bytes_words(key + b"\xa5" * (64 - klen)))   # bytes past klen are not the key's
    hkw = defop("hmac_key_words", 62, "sha", 8, 16, lambda w: key_states(be_state(w)))
    for ch in ([0] * 8, [M32] * 8, [0x36363636] * 8, [0x5c5c5c5c] * 8, rw(8), rw(8), rw(8)):
        hkw.add("chain", ch)

    def ref_pad(w):
        n, msg = w[0], words_bytes(w[17:])[:w[0]]
        blk = state_words(padded(msg, 64))
        assert len(blk) == 16
        return blk + hmac_from_states(w[1:17], msg)
    pb = defop("pad_hmac_block", 63, "sha", 31, 24, ref_pad)
    for n in (0, 1, 3, 4, 37, 53, 55, 2, 54):
        for cls, msg in fills(rnd, n):
            key = bytes(rnd.randrange(256) for _ in range(32))
            pb.add(cls, [n] + key_states(key) + bytes_words(msg + b"\xa5" * (56 - n)))

    def child_msgs(w, ser_at):
        sw, index = w[0], w[1]
        ser = be_state(w[ser_at:ser_at + sw])
        return [ser + struct.pack(">I", index) + bytes([b]) for b in (0, 1)]

    def ref_child(w):
        m0, m1 = child_msgs(w, 18)
        return hmac_from_states(w[2:18], m0) + hmac_from_states(w[2:18], m1)

    def ref_path(w):
        key = be_state(w[2:10])
        m0, m1 = child_msgs(w, 10)
        return hmac_words(key, m0) + hmac_words(key, m1)
    ch = defop("child_hmacs", 64, "sha", 30, 16, ref_child)
    ps = defop("path_step", 65, "sha", 22, 16, ref_path)
    for sw in (8, 12):
        for index in (0, 1, 0x7FFFFFFF, 0x80000000, M32, rnd.randrange(1 << 32)):
            for ser in ([0] * 12, [M32] * 12, rw(12)):
                key = bytes(rnd.randrange(256) for _ in range(32))
                ch.add("sw%d" % sw, [sw, index] + key_states(key) + ser)    # (sw = 8 leaves ser[8 .. 12) unread)
                ps.add("sw%d" % sw, [sw, index] + state_words(key) + ser)
    fp = defop("fingerprint", 66, "sha", 12, 1, lambda w: state_words(hashlib.sha256(be_state(w)).digest())[:1])
    for ser in ([0] * 12, [M32] * 12, rw(12), rw(12), rw(12)):
        fp.add("ser", ser)

    def ref_blocks(w):
        m = w[0] + (0 if w[1] == M32 else 1)
        return [len(padded(b"\0" * m, 64)) // 64]
    lb = defop("long_blocks", 67, "sha", 2, 1, ref_blocks)
    for n in sorted(set(LONG_LENS) | set(range(52, 60)) | set(range(116, 124)) | {183, 184, 1023, 1024}):
        for suffix in (M32, 0, 1):
            lb.add("len", [n, suffix])

    def ref_word(w):
        n, has, suffix, off, shift = w[:5]
        stream = long_message(w, 5, n, shift) + (bytes([suffix]) if has else b"") + b"\x80"
        return state_words((stream + b"\0" * (off + 4))[off:off + 4])
    lw = defop("long_word", 68, "sha", 5 + MSGW, 1, ref_word)
    for n in (0, 1, 2, 3, 4, 5, 7, 55, 64, 200):
        msg = bytes(rnd.randrange(1, 256) for _ in range(n))
        for has, suffix in ((0, 0), (1, 0), (1, 1), (1, 0xEE)):
            for off in sorted({0, max(0, (n & ~3) - 4), n & ~3, (n & ~3) + 4, (n & ~3) + 8}):
                lw.add("word", [n, has, suffix, off, (n + off // 4) % 4] + place(msg, (n + off // 4) % 4))
    del lw.sets[MAX_SETS:]

    def ref_long(w):
        n, suffix, shift = w[:3]
        msg = long_message(w, 19, n, shift) + (b"" if suffix == M32 else bytes([suffix]))
        return hmac_from_states(w[3:19], msg)
    hl = defop("hmac_long", 69, "sha", 19 + MSGW, 8, ref_long)
    key = b"BLS private key seed"
    i = 0
    for n in LONG_LENS:
        for suffix in (M32, 0, 1):
            for cls, msg in fills(rnd, n):
                hl.add(cls, [n, suffix, i % 4] + key_states(key) + place(msg, i % 4))
                i += 1

    def ref_pair(w):
        n, shift = w[:2]
        msg = long_message(w, 18, n, shift)
        return hmac_from_states(w[2:18], msg + b"\0") + hmac_from_states(w[2:18], msg + b"\1")
    hp = defop("hmac_long_pair", 70, "sha", 18 + MSGW, 16, ref_pair)
    key = b"BLS HD seed"
    for n in LONG_LENS:
        for shift in range(4):
            for cls, msg in fills(rnd, n):
                hp.add(cls, [n, shift] + key_states(key) + place(msg, shift))

    dg = defop("hpk_digest", 71, "sha", 4 + 12 * MAXKEYS, 8, lambda w: state_words(hashlib.sha256(words_bytes(w[4:4 + 12 * w[0]])).digest()))
    for k in (1, 2, 3, 4, 5, 8, 9, 6, 7):
        for cls, keys in fills(rnd, 48 * k):
            dg.add("k%d_%s" % (k, cls), [k, 0, 0, 0] + bytes_words(keys + b"\xa5" * (48 * (MAXKEYS - k))))

    he = defop("hpk_exponent", 72, "sha", 9, 8, lambda w: words8(exp_value(be_state(w[1:]), w[0]) % N))
    for cls, idx in EXP_INDEX.items():
        for i in idx:
            he.add(cls, [i] + state_words(EXP_DIGEST))
    for dgst in ([0] * 8, [M32] * 8, rw(8), rw(8)):
        for i in (0, 1, M32, rnd.randrange(1 << 32)):
            he.add("other", [i] + dgst)


# ---- window ------------------------------------------------------------------------------------------------------------
def g2smul_scalars():
    """the scalar list of tests/test_g2smul_model.py (the model test holds the two equal)"""
    rng = random.Random(0x62736d)
    fixed = [0, 1, 7, 8, 9, 15, 16, N - 1, N, N + 1, 1 << 255, (1 << 256) - 1, int("88" * 32, 16), int("77" * 32, 16), int("f0" * 32, 16)]
    return fixed + [rng.randrange(1 << 256) for _ in range(200)]


def build_window():
    rnd = _rnd("window")
    edge = [0, 1, ALL1, N, N - 1] + [int(c * 64, 16) for c in "078f"] + [int("87" * 32, 16), int("78" * 32, 16), int("f7" * 32, 16)]
    nib8 = [8 << (4 * p) for p in range(64)]
    listed = g2smul_scalars()

    def ref_rec(w):
        return digit_words(digits_of(from_be_words(w)))

    def chk_rec(w, out):
        ds = []
        for i in range(DIGITS):
            sgn, ad, mz = out[3 * i:3 * i + 3]
            assert sgn in (0, M32) and mz == (M32 if ad == 0 else 0) and ad <= 8 and not (sgn and ad == 0)
            ds.append(-ad if sgn else ad)
        assert sum(d << (4 * i) for i, d in enumerate(ds)) == from_be_words(w), "sum d_w 16^w != s"
    # the two ops share the edge values; the single nibbles 8 and the listed scalars are split so that each stays within 257 sets
    g1 = defop("recode_g1", 80, "window", 8, 3 * DIGITS, ref_rec, chk_rec, host=False)
    g2 = defop("recode_g2", 81, "window", 8, 3 * DIGITS, ref_rec, chk_rec, host=False)
    for s in edge:
        g1.add("edge", be_words(s))
        g2.add("edge", be_words(s))
    for s in nib8:
        g1.add("nibble8", be_words(s))
    for s in nib8[::9] + nib8[-1:]:
        g2.add("nibble8", be_words(s))
    for s in listed[:115]:
        g1.add("listed", be_words(s))
    for s in listed:
        g2.add("listed", be_words(s))
    for _ in range(24):
        g1.add("random", be_words(rnd.randrange(R)))
    for _ in range(12):
        g2.add("random", be_words(rnd.randrange(R)))

    sl = defop("sel", 82, "window", 3, 2, lambda w: [(w[0] & w[2]) | (w[1] & ~w[2] & M32)] * 2, host=False)
    for a, b in ((0, M32), (M32, 0), (0x12345678, 0x9abcdef0), (0x80000000, 0x7FFFFFFF), (rnd.randrange(1 << 32), rnd.randrange(1 << 32))):
        for m in (0, M32):
            sl.add("mask", [a, b, m])

    def ref_select(dw):
        def ref(w):
            ad, keep0, T = w[0], w[1], w[2:]
            q = T[(ad - 1) * dw:ad * dw] if ad else [0] * dw
            return [x | (t & keep0) for x, t in zip(q, T[:dw])]
        return ref
    for code, name, dw, strided in ((83, "select_g1", G1_DW, False), (84, "select_g2", G2_DW, True)):
        op = defop(name, code, "window", 2 + 8 * dw, dw, ref_select(dw), host=False, strided=strided)
        for rep in range(3):
            for ad in range(9):
                for keep0 in (0, M32):
                    T = rnd.sample(range(1, 1 << 32), 8 * dw)  # every word distinct, none zero
                    if rep == 2:                               # entries that differ in one bit of one word only
                        T = T[:dw] * 8
                        for e in range(8):
                            T[e * dw + (e * 5) % dw] ^= 1 << (e + 3)
                    op.add("ad%d_keep%d" % (ad, keep0 & 1), [ad, keep0] + T)


def build_all():
    build_reduce()
    build_products()
    build_inversions()
    build_lagrange()
    build_sigdiv()
    build_sha()
    build_window()
    for op in OPS.values():
        assert 0 < len(op.sets) <= MAX_SETS, (op.name, len(op.sets))


build_all()

_EXPECTED = {}


def expected(name):
    """the expected output words of every set of an op (computed once)"""
    if name not in _EXPECTED:
        op = OPS[name]
        _EXPECTED[name] = [[int(v) & M32 for v in op.ref(w)] for _, w in op.sets]
        assert all(len(e) == op.wout for e in _EXPECTED[name]), name
    return _EXPECTED[name]


def call(name, n):
    """a call with n items: (input words, set index of each item, expected words of each item,
    independent check of each item: a function of the item's output words, or None)"""
    op = OPS[name]
    ns = len(op.sets)
    exp = expected(name)
    idx = [item_set(i // 64 if op.wave else i, ns) for i in range(n)]
    if op.strided:
        words = [x for k in idx for x in op.sets[k][1][:2]]
        for d in range(op.win - 2):
            words += [op.sets[k][1][2 + d] for k in idx]
    else:
        words = [x for k in idx for x in op.sets[k][1]]
    want = [exp[k] for k in idx]
    chk = [(lambda out, w=op.sets[k][1]: op.check(w, out)) if op.check is not None else None for k in idx]
    return words, idx, want, chk


if __name__ == "__main__":
    for g in GROUPS:
        for op in OPS.values():
            if op.group == g:
                cls = {}
                for c, _ in op.sets:
                    cls[c] = cls.get(c, 0) + 1
                print("%-10s %-18s %3d  %s" % (g, op.name, len(op.sets), " ".join("%s=%d" % kv for kv in list(cls.items())[:8])))
