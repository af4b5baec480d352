"""Programs, scratchpad images and CPU references for run_rounds, the round interpreter of the wavefront VM (csrc/blsgpu_kernels.hip),
as the test-only device library csrc/blsgpu_vm_check.hip runs it.  Pure Python: tests/test_vm_vectors_model.py holds the word
machine below against vmgen/tablesim.py and runs its mutants; tests/test_gpu_vm.py compares the device with both.

Three things live here:
  * Program: a builder that packs rounds the way vmgen.emit.pack does (emit.kpad, emit.INACTIVE, the merge flags of plan_lin_round),
    from explicit lane plans instead of a scheduler, so that a test can ask for record shapes no production table has.  Every LIN
    round goes through emit.check_lin_bounds before it is packed: the vectors stay inside the contract csrc/fq32.h states.
  * WordMachine: executes packed rounds on slots of 12 words (held as integers below 2^384) out of the word models that exist:
    fp28_vectors.vm_mul28 for a MUL lane, fq32_vectors.m_lin_share / m_fat_flip / _absorb / m_fat_reduce for a LIN round,
    fq32_vectors.inv_ref and the sign reference for INV / SGN.  All of them fix the words, so the comparison with the device is word
    for word everywhere.  `exact` runs the limb models themselves (with the bounds they assert); the default is the same arithmetic
    on packed integers -- twelve 64-bit accumulators side by side in one integer, vm_mul28 in closed form -- which the model test
    holds against `exact` on every synthetic program.  MUTANTS names the deliberate defects the model test must tell from tablesim.
  * the independent reference: vmgen.tablesim.TableMachine on residues mod q (tablesim_run), once per program and image.

Values come from fq32_vectors' classes (CLASS_VALUES): 0, 1, q - 1, R, values in [q, 2q), the lower eleven limbs all 2^32 - 1, and
seeded random values below 2q.
"""
import random

import fp28_vectors as F28
import fq32_vectors as F32
from vmgen import emit, tablesim
from vmgen.emit import INACTIVE, kpad

Q, R, ONE, M32 = F32.Q, F32.R, F32.ONE, F32.M32
LANES = 64
OPS = {"RUN_FULL": 0, "RUN_LIGHT": 1, "RUN_LIGHT_STASH": 2, "RUN_FULL_CHK": 3, "RUN_LIGHT_CHK": 4}      # csrc/blsgpu_vm_check.hip
LIGHT_OPS = ("RUN_LIGHT", "RUN_LIGHT_STASH", "RUN_LIGHT_CHK")
GEOMETRIES = (1, 4, 8)                                  # teams per workgroup: 64, 256, 512 threads
HDR, TRAILER, MAX_ROUNDS, LDS_MAX = 8, 2 + 3 * 64, 1 << 16, 65536                                       # csrc/vm_check_plan.h
LOW1 = ((((2 * Q - 1) >> 352) - 1) << 352) | ((1 << 352) - 1)      # lower limbs all ones, below 2q (and above q)
CLASS_VALUES = [0, 1, Q - 1, ONE, Q, Q + 1, 2 * Q - 1, ONE + Q, LOW1, F32.ALT_EVEN]
assert all(0 <= v < 2 * Q for v in CLASS_VALUES) and Q < LOW1
MUTANTS = {                                             # name -> the program classes it belongs to
    "uop_shift": ("lin_shape", "transitions"),          # micro-op p read at position p + 1
    "flip_late": ("lin_shape",),                        # the flip one micro-op late
    "no_flip_all_negative": ("lin_shape",),             # no flip when MN = K
    "cut4": ("lin_shape", "transitions"),               # records cut at four chunks
    "level2_wrong_lane": ("groups",),                   # level-2 merge from lane 3 of the quad
    "write_first": ("read_before_write",),              # writes applied before the round's reads
    "inactive_mul_stores": ("groups",),                 # an inactive MUL lane that stores (to its first operand's slot)
    "light_drops_odd_last": ("lengths",),               # LIGHT dropping the last round of an odd length
    "window11": ("stash",),                             # a window of 11 slots
    "check_after": ("check_at",),                       # the check evaluated after round check_at instead of before it
    "base_ignored": ("teams",),                         # base16 ignored on stores: every team stores into team 0's area
}


def slot_words(v):
    return F32.words12(v)


# ---- the builder ---------------------------------------------------------------------------------------------------------------
class Program:
    """rounds packed as emit.pack packs them.  nslots: slots of a team; cls: the program class; name: for messages"""

    def __init__(self, name, cls, nslots, ops=("RUN_FULL", "RUN_LIGHT"), nimg=2, check=None, note=""):
        self.name, self.cls, self.nslots, self.ops, self.nimg, self.note = name, cls, nslots, tuple(ops), nimg, note
        self.check = check                              # (check_at, chk_slot) for the _CHK ops
        self.rounds, self.data, self.plans = [], [], []

    def _lanes(self, lanes):
        if isinstance(lanes, dict):
            return [lanes.get(l) for l in range(LANES)]
        return list(lanes) + [None] * (LANES - len(lanes))

    def mul(self, lanes):
        """lanes: {lane: (a, b, d)} in slots; d None: an inactive lane that still names operands"""
        off = len(self.data)
        for e in self._lanes(lanes):
            a, b, d = e if e is not None else (0, 0, None)
            self.data += [emit.sref(a), emit.sref(b), emit.sref(d) if d is not None else INACTIVE, 0]
        self.rounds.append((off, 0))
        return self

    def unary(self, kind, lanes):
        """kind 'inv' / 'sgn'; lanes: {lane: (a, d)}"""
        off = len(self.data)
        for e in self._lanes(lanes):
            a, d = e if e is not None else (0, None)
            self.data += [emit.sref(a), 0, emit.sref(d) if d is not None else INACTIVE, 0]
        self.rounds.append((off, emit.KIND[kind]))
        return self

    def window(self, kind, K):
        """'save' / 'restore' of the 12-slot window at slot K (light programs): no lane records, data_off 0 as emit.pack writes it"""
        assert 0 <= K < 256
        self.rounds.append((0, (2 if kind == "save" else 3) | (K << 8)))
        return self

    def lin(self, lanes, levels=None, pad_k=0):
        """lanes: {lane: (d | None, flags, negatives, positives)}, terms (coefficient, slot); groups are the caller's: the first lane
        of a group of 4 carries flags 3 << 14 and its third lane 1 << 14, the first lane of a pair 1 << 14 (emit.plan_lin_round).
        pad_k: at least that many micro-ops (shorter shares are padded with zero micro-ops, as emit.pack pads them)"""
        plan = []
        for e in self._lanes(lanes):
            d, flags, negs, poss = e if e is not None else (None, 0, [], [])
            plan.append((d, flags, [(1, cf, s) for cf, s in negs], [(0, cf, s) for cf, s in poss]))
        mn = max(len(x[2]) for x in plan)
        mp = max(max(len(x[3]) for x in plan), pad_k - mn)
        if mn + mp == 0:
            mp = 1
        K = mn + mp
        emit.check_lin_bounds(plan, mn)                  # the contract of csrc/fq32.h: every synthetic round is inside it
        self.plans.append((plan, mn))
        if levels is None:
            levels = 2 if any(x[1] >> 15 & 1 for x in plan) else 1 if any(x[1] >> 14 & 1 for x in plan) else 0
        off, kp = len(self.data), kpad(K)
        assert len(self.data) % 4 == 0 and 1 <= K <= 30
        for d, flags, negs, poss in plan:
            rec = [0] * kp
            rec[0] = emit.sref(d) if d is not None else INACTIVE
            rec[1] = flags
            for base, lst in ((2, negs), (2 + mn, poss)):
                for k, (neg, cf, s) in enumerate(lst):
                    assert 0 < cf < 32 and 0 <= s < 1024
                    rec[base + k] = (cf << 10) | s
            self.data += rec
        self.rounds.append((off, emit.KIND["lin"] | (K << 8) | (levels << 16) | (mn << 18)))
        return self

    def table(self):
        """the u16 table (at least one SAVE / RESTORE look-ahead fetch long)"""
        return self.data + [0] * max(0, 256 - len(self.data))


def images(nslots, nimg, seed):
    """nimg scratchpad images (integers below 2q per slot): the class values at seeded places among seeded random values"""
    out = []
    for t in range(nimg):
        rnd = random.Random("vm:image:%s:%d" % (seed, t))
        img = [rnd.randrange(2 * Q) for _ in range(nslots)]
        for v in CLASS_VALUES:
            img[rnd.randrange(nslots)] = v
        out.append(img)
    return out


def call_words(rounds, table, nslots, imgs, tpw, check_at=0, chk_slot=0):
    """the input words of one call of blsgpu_vm_check (csrc/vm_check_plan.h)"""
    w = [len(rounds), nslots, len(table), check_at, chk_slot, tpw, 0, 0]
    for off, meta in rounds:
        w += [off, meta]
    t = list(table) + [0] * (len(table) & 1)
    w += [t[i] | (t[i + 1] << 16) for i in range(0, len(t), 2)]
    for img in imgs:
        for v in img:
            w += slot_words(v)
    return w


# ---- the word machine ------------------------------------------------------------------------------------------------------------
def _spread(v):
    """12 words -> twelve 64-bit fields of one integer"""
    return sum(((v >> (32 * j)) & M32) << (64 * j) for j in range(12))


BIAS_SPREAD = sum(b << (64 * j) for j, b in enumerate(F32.BIAS_LIMBS))
M64 = (1 << 64) - 1


def _unspread(a):
    return [(a >> (64 * j)) & M64 for j in range(12)]


def sgn_ref(a):
    return ONE if (a * F32.RINV) % Q > F32.HALF else 0


class WordMachine:
    """one workgroup: a list of team images (integers standing for 12 words per slot)"""

    def __init__(self, data, imgs, exact=False, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.data, self.teams, self.exact, self.mutant = data, [list(i) for i in imgs], exact, mutant
        self.mul = F28.vm_mul28 if exact else F28.vm_mul28_closed

    # -- one LIN round on one team: {slot: value}
    def _lin(self, team, off, meta):
        K, levels, mn = (meta >> 8) & 0xFF, (meta >> 16) & 3, (meta >> 18) & 0xFF
        rl, d16, mut = kpad(K), self.data, self.mutant
        recs = [d16[off + rl * l: off + rl * (l + 1)] for l in range(LANES)]
        if mut == "cut4":
            recs = [r[:16] + [0] * (len(r) - 16) for r in recs]
        # the lanes whose accumulators are looked at: the live ones and those a looked-at lane absorbs
        perm2 = (3, 3, 3, 3) if mut == "level2_wrong_lane" else F32.PERM_L2
        need = set(l for l in range(LANES) if recs[l][0] != INACTIVE)
        if levels >= 2:
            need |= set((l & ~3) + perm2[l & 3] for l in list(need) if recs[l][1] >> 15 & 1)
        if levels >= 1:
            need |= set((l & ~3) + F32.PERM_L1[l & 3] for l in list(need) if recs[l][1] >> 14 & 1)
        flip_at = mn + 1 if mut == "flip_late" else mn
        accs = [0] * LANES
        for l in need:
            rec, acc = recs[l], 0
            uops = [rec[2 + p + (1 if mut == "uop_shift" else 0)] if 2 + p + (1 if mut == "uop_shift" else 0) < rl else 0 for p in range(K)]
            for p in range(K):
                if mn > 0 and p == flip_at:
                    acc = BIAS_SPREAD - acc
                acc += ((uops[p] >> 10) & 31) * _spread(team[uops[p] & 1023])
            if flip_at >= K and mn > 0 and not (mut == "no_flip_all_negative" and mn == K):
                acc = BIAS_SPREAD - acc
            assert acc >= 0 or mut is not None
            acc &= (1 << 768) - 1                         # (a mutant's borrow: sixty-four-bit registers wrap)
            if self.exact and mut is None:
                want = F32.m_lin_share(mn, K, [(u >> 10) & 31 for u in uops], [team[u & 1023] for u in uops])
                assert _unspread(acc) == want and all(a < F32.FAT_LIMIT for a in want)
            accs[l] = acc
        flags = [r[1] for r in recs]
        for lv, perm, bit in ((1, F32.PERM_L1, 14), (2, perm2, 15)):
            if levels >= lv:
                accs = [accs[l] + accs[(l & ~3) + perm[l & 3]] if (flags[l] >> bit) & 1 else accs[l] for l in range(LANES)]
        out = {}
        for l in range(LANES):
            if recs[l][0] != INACTIVE:
                limbs = _unspread(accs[l] & ((1 << 768) - 1))
                if mut is None:
                    assert accs[l] >> 768 == 0 and all(a < F32.FAT_LIMIT for a in limbs) and F32.fat_value(limbs) < F32.V_LIMIT
                out[recs[l][0] // 3] = F32.m_fat_reduce(limbs)
        return out

    def _round(self, t, off, meta, light, stash):
        """one round of team t; returns nothing, stores applied after the reads"""
        team, d16, mut = self.teams[t], self.data, self.mutant
        dest = self.teams[0] if mut == "base_ignored" else team
        kind, K = meta & 3, (meta >> 8) & 0xFF
        if light and kind >= 2:
            if stash is not None:
                n = 11 if mut == "window11" else 12
                if kind == 2:
                    stash[:n] = team[K:K + n]
                else:
                    dest[K:K + n] = stash[:n]
            return
        writes = {}
        if kind == 1:
            if mut == "write_first":                     # lane by lane, each store seen by the lanes after it
                return self._write_first_lin(t, off, meta)
            writes = self._lin(team, off, meta)
        else:
            for l in range(LANES):
                a, b, d, _ = d16[off + 4 * l: off + 4 * l + 4]
                if d == INACTIVE:
                    if kind == 0 and mut == "inactive_mul_stores":
                        writes[a // 3] = self.mul(team[a // 3], team[b // 3])
                    continue
                x = team[a // 3]
                val = self.mul(x, team[b // 3]) if kind == 0 else F32.inv_ref(x) if kind == 2 else sgn_ref(x)
                if mut == "write_first":
                    dest[d // 3] = val
                else:
                    writes[d // 3] = val
        for s, v in writes.items():
            dest[s] = v

    def _write_first_lin(self, t, off, meta):
        team, rl = self.teams[t], kpad((meta >> 8) & 0xFF)
        for l in range(LANES):
            d = self.data[off + rl * l]
            if d != INACTIVE:
                team[d // 3] = self._lin(team, off, meta)[d // 3]

    def run(self, rounds, op, check_at=0, chk_slot=0):
        """every team of the workgroup through the rounds: [(return value, functor calls, stash words)], images in self.teams"""
        light, res = op in LIGHT_OPS, []
        if not hasattr(self, "stash"):
            self.stash = [[0] * 12 for _ in self.teams]  # (kept between calls: a program run in pieces)
        for t in range(len(self.teams)):
            stash = self.stash[t] if op == "RUN_LIGHT_STASH" else None
            n, ret, calls = len(rounds), 1, 0
            if light and self.mutant == "light_drops_odd_last" and n % 2 == 1:
                n -= 1
            for i in range(n):
                at = check_at + 1 if self.mutant == "check_after" else check_at
                if op.endswith("_CHK") and i == at:
                    calls += 1
                    if self.teams[t][chk_slot] % Q == 0:
                        ret = 0
                        break
                self._round(t, rounds[i][0], rounds[i][1], light, stash)
            sw = [0] * 192
            if stash is not None:
                sw[:144] = [w for v in stash for w in slot_words(v)]
            res.append((ret, calls, sw))
        return res


def expected_words(imgs, results):
    """the output words of a call: the images, then the trailers"""
    w = [x for img in imgs for v in img for x in slot_words(v)]
    for ret, calls, sw in results:
        w += [ret, calls] + sw
    return w


def tablesim_run(data, img, rounds, light):
    """the independent reference: residues mod q of every slot after the rounds (and the residues of the stash window)"""
    m = tablesim.TableMachine([], len(img), data)
    m.team = [v % Q for v in img]
    m.stash = [0] * 12
    m.run(rounds, light=light)
    return m.team, m.stash


def strip_windows(rounds):
    return [r for r in rounds if r[1] & 3 < 2]


# ---- synthetic programs ----------------------------------------------------------------------------------------------------------
def _rnd(name):
    return random.Random("vm:" + name)


def _terms(rnd, n, lo, hi, cfs=None):
    return [(cfs[k % len(cfs)] if cfs else rnd.randrange(1, 32), rnd.randrange(lo, hi)) for k in range(n)]


def _neg_terms(rnd, n, lo, hi, total=None):
    """n negative terms whose coefficients sum to at most NEG_CF_MAX (exactly `total` if given)"""
    if n == 0:
        return []
    total = total if total is not None else min(emit.NEG_CF_MAX, 31 * n)
    assert n <= total <= 31 * n
    cfs = [total // n + (1 if k < total % n else 0) for k in range(n)]
    return [(cf, rnd.randrange(lo, hi)) for cf in cfs]


def _free_dst(rnd, used, lo, hi):
    while True:
        d = rnd.randrange(lo, hi)
        if d not in used:
            used.add(d)
            return d


def _rand_round(p, rnd, kind, hi, live=8):
    """one round of a kind on a few seeded lanes; slots below hi"""
    used = set()
    lanes = sorted(rnd.sample(range(LANES), live))
    if kind == "mul":
        p.mul({l: (rnd.randrange(hi), rnd.randrange(hi), _free_dst(rnd, used, 0, hi)) for l in lanes})
    elif kind == "lin":
        K = rnd.randrange(1, 12)
        mn = rnd.randrange(0, K + 1)
        p.lin({l: (_free_dst(rnd, used, 0, hi), 0, _neg_terms(rnd, mn, 0, hi, min(255, 7 * mn)), _terms(rnd, K - mn, 0, hi)) for l in lanes})
    elif kind in ("inv", "sgn"):
        p.unary(kind, {l: (rnd.randrange(hi), _free_dst(rnd, used, 0, hi)) for l in lanes})
    else:
        raise ValueError(kind)


def build_lengths():
    """nr = 1 .. 5, 9 and 12; each kind first and last; LIGHT leaves its two-copy loop from either copy"""
    out = []
    for nr in (1, 2, 3, 4, 5, 9, 12):
        for first, last, ops in (("mul", "lin", ("RUN_FULL", "RUN_LIGHT")), ("lin", "mul", ("RUN_FULL", "RUN_LIGHT")),
                                 ("inv", "sgn", ("RUN_FULL",)), ("sgn", "inv", ("RUN_FULL",))):
            rnd = _rnd("lengths:%d:%s" % (nr, first))
            p = Program("len%d_%s_first" % (nr, first), "lengths", 36, ops)
            kinds = [first] + [rnd.choice(("mul", "lin")) for _ in range(nr - 2)] + ([last] if nr > 1 else [])
            for k in kinds:
                _rand_round(p, rnd, k, 24)
            out.append(p)
    return out


def build_lin_shape():
    out = []
    # every K from 1 to 30 with MN from {0, 1, K - 1, K}; coefficients 1 and 31; one program per MN choice
    for tag in ("mn0", "mn1", "mnK-1", "mnK"):
        rnd = _rnd("linshape:" + tag)
        p = Program("lin_K1to30_" + tag, "lin_shape", 40)
        for K in range(1, 31):
            mn = {"mn0": 0, "mn1": min(1, K), "mnK-1": K - 1, "mnK": K}[tag]
            used, lanes = set(), {}
            for l in (0, 5, 31, 32, 63):
                negs = _neg_terms(rnd, mn, 0, 28, max(mn, min(255, mn * (31 if l == 5 else 3))))
                poss = _terms(rnd, K - mn, 0, 28, cfs=(1, 31) if l != 31 else None)
                lanes[l] = (_free_dst(rnd, used, 0, 28), 0, negs, poss)
            p.lin(lanes)
        out.append(p)
    # slot indices 0 and nslots - 1 with nslots = 1023 (one-team geometry): both bit fields of a micro-op all ones
    rnd = _rnd("linshape:fields")
    p = Program("lin_fields_all_ones", "lin_shape", 1023, note="one team only: 1023 slots")
    p.lin({0: (1022, 0, [(31, 1022), (1, 0)], [(31, 1022), (31, 0)]), 63: (0, 0, [], [(31, 1022), (1, 1022)])})
    p.lin({7: (1021, 0, [(31, 1022)] * 8, [(31, 1022)] * 22)})
    p.mul({63: (1022, 0, 1020), 0: (1021, 1022, 1019)})
    out.append(p)
    # a negative share whose coefficients sum to exactly NEG_CF_MAX; a group at the largest total check_lin_bounds admits
    rnd = _rnd("linshape:bounds")
    p = Program("lin_bounds", "lin_shape", 40)
    neg255 = [(31, rnd.randrange(28)) for _ in range(8)] + [(7, rnd.randrange(28))]
    assert sum(c for c, s in neg255) == emit.NEG_CF_MAX
    p.lin({2: (30, 0, neg255, _terms(rnd, 5, 0, 28)), 40: (31, 0, list(neg255), [])})
    # the 2^44 limb bound: tot 0xFFFFFFFF + 4 BIAS_LIMB_MAX < 2^44 -> tot <= 3067 over a group of four, 30 micro-ops a lane
    tot = (((1 << 44) - 1 - 4 * emit.BIAS_LIMB_MAX) // 0xFFFFFFFF)
    cfs = [tot // 120 + (1 if k < tot % 120 else 0) for k in range(120)]
    assert sum(cfs) == tot and max(cfs) <= 31
    shares = [[(cf, rnd.randrange(28)) for cf in cfs[part::4]] for part in range(4)]

    def quad(sh):
        return {8: (32, 3 << 14, [], sh[0]), 9: (None, 0, [], sh[1]), 10: (None, 1 << 14, [], sh[2]), 11: (None, 0, [], sh[3])}
    p.lin(quad(shares))
    over = [list(sh) for sh in shares]                    # one more unit is refused: the group above is the largest admitted
    over[3][-1] = (over[3][-1][0] + 1, over[3][-1][1])
    try:
        Program("over", "lin_shape", 40).lin(quad(over))
    except AssertionError:
        pass
    else:
        raise RuntimeError("check_lin_bounds admits more than its own bound")
    out.append(p)
    return out


def _euler_pairs(n):
    """a closed walk over 1 .. n that takes every ordered pair (a, b), a = b included, exactly once (n^2 steps)"""
    nxt = {a: list(range(n, 0, -1)) for a in range(1, n + 1)}
    stack, walk = [1], []
    while stack:
        a = stack[-1]
        if nxt[a]:
            stack.append(nxt[a].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == n * n + 1 and set(zip(walk, walk[1:])) == set((a, b) for a in range(1, n + 1) for b in range(1, n + 1))
    return walk


def build_transitions():
    """every ordered pair of chunk counts (1 .. 8, 1 .. 8) as consecutive rounds, MUL rounds as the one-chunk case"""
    rnd = _rnd("transitions")
    p = Program("chunk_transitions", "transitions", 40)
    for c in _euler_pairs(8):
        lanes = sorted(rnd.sample(range(LANES), 6))
        used = set()
        if c == 1:
            p.mul({l: (rnd.randrange(28), rnd.randrange(28), _free_dst(rnd, used, 0, 28)) for l in lanes})
        else:
            K = 4 * c - 2
            mn = rnd.randrange(0, 6)
            p.lin({l: (_free_dst(rnd, used, 0, 28), 0, _neg_terms(rnd, mn, 0, 28, min(255, 9 * mn)), _terms(rnd, K - mn, 1, 28)) for l in lanes})
    assert [kpad((m >> 8) & 255) // 4 if m & 3 else 1 for o, m in p.rounds] == _euler_pairs(8)
    return [p]


def build_groups():
    out = []
    rnd = _rnd("groups")
    p = Program("groups_mixed", "groups", 40)
    # groups of 4, 2 and 1 mixed in one round at every aligned position of the wavefront, inactive lanes between live ones
    for shift in range(4):
        lanes, used = {}, set()
        for quad in range(16):
            base, g = 4 * quad, (4, 2, 1, 0)[(quad + shift) % 4]
            if g == 4:
                lanes[base] = (_free_dst(rnd, used, 0, 28), 3 << 14, _neg_terms(rnd, 2, 0, 28, 40), _terms(rnd, 5, 0, 28))
                lanes[base + 1] = (None, 0, _neg_terms(rnd, 2, 0, 28, 33), _terms(rnd, 4, 0, 28))
                lanes[base + 2] = (None, 1 << 14, _neg_terms(rnd, 1, 0, 28, 31), _terms(rnd, 5, 0, 28))
                lanes[base + 3] = (None, 0, [], _terms(rnd, 3, 0, 28))
            elif g == 2:
                for h in (0, 2):                          # both aligned pairs of the quad
                    lanes[base + h] = (_free_dst(rnd, used, 0, 28), 1 << 14, _neg_terms(rnd, 2, 0, 28, 20), _terms(rnd, 4, 0, 28))
                    lanes[base + h + 1] = (None, 0, _neg_terms(rnd, 1, 0, 28, 9), _terms(rnd, 5, 0, 28))
            elif g == 1:
                for h in (1, 3):                          # single lanes with inactive lanes between them
                    lanes[base + h] = (_free_dst(rnd, used, 0, 28), 0, _neg_terms(rnd, 1, 0, 28, 5), _terms(rnd, 3, 0, 28))
        p.lin(lanes)
    # levels 1 and 0: pairs only; merge flags set with level 0 are ignored
    for levels in (1, 0):
        used = set()
        p.lin({l: ((_free_dst(rnd, used, 0, 40) if l % 2 == 0 or levels == 0 else None), (1 << 14) if l % 2 == 0 else 0,
                   _neg_terms(rnd, 1, 0, 28, 6), _terms(rnd, 3, 0, 28)) for l in range(0, 64) if l % 8 < 4}, levels=levels)
    # a round with all 64 lanes inactive, of either kind; a MUL with rd = INACTIVE on lanes that name real operands
    p.lin({}, pad_k=3)
    p.mul({})
    used = set()
    p.mul({l: (rnd.randrange(1, 28), rnd.randrange(1, 28), None if l % 3 == 0 else _free_dst(rnd, used, 0, 28)) for l in range(0, 64, 2)})
    _rand_round(p, rnd, "lin", 28, live=20)
    out.append(p)
    return out


def build_read_before_write():
    rnd = _rnd("rbw")
    p = Program("read_before_write", "read_before_write", 40)
    # a lane whose destination is one of its own sources; a destination that is another lane's source in the same round (a ring)
    p.mul({0: (3, 4, 3), 1: (5, 6, 6), 7: (8, 9, 10), 9: (10, 8, 9), 40: (9, 10, 8)})
    p.mul({l: (11 + (l + 1) % 16, 11 + (l + 5) % 16, 11 + l) for l in range(16)})
    # LIN: the destination is read at the LAST micro-op of the lane itself and of another lane
    for K in (1, 2, 6, 7, 29, 30):
        mn = min(K - 1, 3)
        lanes = {}
        for l, (d, other) in {2: (20, 21), 33: (21, 22), 63: (22, 20)}.items():
            negs = _neg_terms(rnd, mn, 0, 28, 5 * mn)
            poss = _terms(rnd, K - mn - 1, 0, 28, cfs=(3, 1)) + [(2, d if l != 33 else other)]
            lanes[l] = (d, 0, negs, poss)
        lanes[5] = (23, 1 << 14, [], [(1, 23), (1, 24)])         # a pair whose second lane reads the first lane's destination
        lanes[6] = (None, 0, [], [(7, 23)])
        p.lin(lanes, pad_k=K)
    # all-negative shares whose last negative micro-op is the destination
    p.lin({0: (25, 0, [(4, 26), (9, 25)], []), 1: (26, 0, [(1, 25), (30, 26)], [])})
    return [p]


def build_inv_sgn():
    """full interpreter only: INV and SGN on 0, 1, q - 1, their forms v + q; zero beside non-zero in one round; (q -+ 1) / 2 for SGN"""
    half = F32.HALF
    inv_vals = [0, 1, Q - 1, Q, Q + 1, 2 * Q - 1, ONE, ONE + Q]
    sgn_c = [0, 1, Q - 1, half, half + 1, half - 1, 2]
    sgn_vals = [c * R % Q for c in sgn_c] + [c * R % Q + Q for c in sgn_c]
    assert all(v < 2 * Q for v in sgn_vals)
    vals = inv_vals + sgn_vals
    p = Program("inv_sgn_values", "inv_sgn", 64, ops=("RUN_FULL",))
    p.fixed = dict(enumerate(vals))                       # slot -> value in every image
    n = len(vals)
    p.unary("inv", {2 * k: (k, n + k) for k in range(len(inv_vals))})
    p.unary("sgn", {63 - 3 * k: (len(inv_vals) + k, n + len(inv_vals) + k) for k in range(len(sgn_vals))})
    p.unary("inv", {5: (n, n)})                           # in place, on a zero the round before wrote (0 -> 0)
    p.unary("sgn", {l: (l % n, 2 * n + l % 8) for l in range(8)})
    p.unary("inv", {})
    p.unary("sgn", {})
    assert 2 * n + 8 <= 64 - 12
    return [p]


def build_stash():
    """LIGHT with kinds 2 / 3: SAVE, clobber the window, RESTORE; RESTORE twice; SAVE twice; windows at slot 0, at nslots - 12 and at
    243 -- the window's start is the header's 8-bit K field, and 243 is the largest start whose twelve slots 243 .. 254 all have
    numbers that field can hold (K + 12 <= 255), which is as far as emit.pack's `K < 256` can place a window and name its slots"""
    out = []
    for nslots, wins in ((40, (0, 28, 7)), (255, (243, 0)), (300, (243,))):
        rnd = _rnd("stash:%d" % nslots)
        p = Program("stash_%d" % nslots, "stash", nslots, ops=("RUN_LIGHT_STASH", "RUN_LIGHT"),
                    note="" if 8 * nslots * 48 <= LDS_MAX else "geometries that fit")
        hi = nslots
        for K in wins:
            p.window("save", K)
            used = set()
            p.mul({l: (rnd.randrange(hi), rnd.randrange(hi), K + l) for l in range(12)})           # clobber the whole window
            p.lin({l: (K + 11 - l, 0, [(3, rnd.randrange(hi))], _terms(rnd, 4, 0, hi)) for l in range(0, 12, 2)})
            p.window("restore", K)
            p.mul({3: (K, K + 11, K + 5)})
            p.window("restore", K)                                                                  # RESTORE twice
            p.window("save", K)
            p.mul({0: (K + 1, K + 2, K + 1)})
            p.window("save", K)                                                                     # SAVE twice: the second one holds
            p.mul({l: (rnd.randrange(hi), rnd.randrange(hi), K + l) for l in range(12)})
            p.window("restore", K)
        out.append(p)
    return out


def build_check_at():
    """check_at = 0, 1, 2, nr - 1, nr and nr + 1; a functor slot that is zero, and one that is non-zero at that round only because
    the round just before wrote it (the same slot is zero again one round later)"""
    out = []
    nr = 6
    for check_at in (0, 1, 2, nr - 1, nr, nr + 1):
        for answer in ("zero", "fresh"):
            rnd = _rnd("check:%d:%s" % (check_at, answer))
            p = Program("check_at%d_%s" % (check_at, answer), "check_at", 40, ops=("RUN_FULL_CHK", "RUN_LIGHT_CHK"), check=(check_at, 20))
            p.fixed = {20: Q if answer == "zero" else 0, 21: 0, 22: ONE}
            if answer == "fresh" and check_at == 0:
                p.fixed[20] = LOW1
            for i in range(nr):
                lanes = {l: (rnd.randrange(19), rnd.randrange(19), d) for l, d in zip(rnd.sample(range(LANES), 5), rnd.sample(range(19), 5))}
                if answer == "fresh":
                    # slot 20 becomes non-zero in round check_at - 1 and zero (in the limbs of q or of 0) in every other round
                    lanes[9] = (22, 22, 20) if i == check_at - 1 else (21, 22, 20)
                else:
                    lanes[9] = (21, 22, 20)
                if i % 2:
                    p.lin({l: (d, 0, [], [(1, a), (2, b)]) if l != 9 else (d, 0, [(1, 21)], [(1, a)]) for l, (a, b, d) in lanes.items()})
                else:
                    p.mul(lanes)
            out.append(p)
    return out


def build_teams():
    """eight different images per program: every team of a 4- or 8-team workgroup equals its own one-team run; the last twelve slots
    of every team's area are referenced by no round and come back as loaded"""
    rnd = _rnd("teams")
    p = Program("teams", "teams", 36, nimg=8)
    for i in range(10):
        _rand_round(p, rnd, ("mul", "lin")[i % 2], 24, live=16)
    return [p]


CLASSES = ("lengths", "lin_shape", "transitions", "groups", "read_before_write", "inv_sgn", "stash", "check_at", "teams")
_BUILDERS = (build_lengths, build_lin_shape, build_transitions, build_groups, build_read_before_write, build_inv_sgn, build_stash,
             build_check_at, build_teams)
_PROGRAMS = None


def programs():
    global _PROGRAMS
    if _PROGRAMS is None:
        _PROGRAMS = [p for b in _BUILDERS for p in b()]
        assert set(p.cls for p in _PROGRAMS) == set(CLASSES)
        for p in _PROGRAMS:
            p.images = images(p.nslots, p.nimg, p.name)
            for img in p.images:
                for s, v in getattr(p, "fixed", {}).items():
                    img[s] = v
            if p.cls == "teams":
                assert max(referenced_slots(p.rounds, p.table(), False)) < p.nslots - 12
    return _PROGRAMS


def referenced_slots(rounds, data, light):
    """every slot a round names (operands, destinations, windows)"""
    s = set()
    for off, meta in rounds:
        kind, K = meta & 3, (meta >> 8) & 0xFF
        if kind == 1:
            rl = kpad(K)
            for l in range(LANES):
                rec = data[off + rl * l: off + rl * (l + 1)]
                if rec[0] != INACTIVE:
                    s.add(rec[0] // 3)
                s.update(u & 1023 for u in rec[2:2 + K])
        elif kind >= 2 and light:                         # a window header
            s.update(range(K, K + 12))
        else:
            for l in range(LANES):
                a, b, d, _ = data[off + 4 * l: off + 4 * l + 4]
                s.update((a // 3, b // 3))
                if d != INACTIVE:
                    s.add(d // 3)
    return s


def geometries(p):
    return [g for g in GEOMETRIES if g * p.nslots * 48 <= LDS_MAX]


def reference(p, op, img):
    """(residues of every slot, stash residues or None) from tablesim for one image of a program under an op"""
    light = op in LIGHT_OPS
    rounds = p.rounds
    if op == "RUN_LIGHT":
        rounds = strip_windows(rounds)                    # stash = nullptr: as a program without those rounds
    if op.endswith("_CHK"):
        check_at, slot = p.check
        if check_at < len(rounds):
            before, _ = tablesim_run(p.table(), img, rounds[:check_at], light)
            if before[slot] == 0:
                return before, None, 0, 1
            after, _ = tablesim_run(p.table(), img, rounds, light)
            return after, None, 1, 1
        after, _ = tablesim_run(p.table(), img, rounds, light)
        return after, None, 1, 0                         # check_at >= nr: the functor is never called (read from the loop)
    team, stash = tablesim_run(p.table(), img, rounds, light)
    return team, (stash if op == "RUN_LIGHT_STASH" else None), 1, 0


# ---- production programs -----------------------------------------------------------------------------------------------------------
_PRODUCTION = None


def production():
    """[(name, op, rounds, cuts)] over the tables of emit.build_tables(), and (data, consts): every flat program under the mode its
    kernels use with a cut at every segment boundary of its script, the stage segments and the directly called segments whole"""
    global _PRODUCTION
    if _PRODUCTION is not None:
        return _PRODUCTION
    from vmgen import h2c_programs as HP
    tb = emit.build_tables()
    sr, data = tb["seg_rounds"], tb["data"]
    out = []

    def flat(name, script, op):
        rounds, cuts = [], []
        for seg in script:
            rounds += sr[seg]
            cuts.append(len(rounds))
        out.append((name, op, rounds, sorted(set(c for c in cuts if c))))
    flat("mscript", tb["mscript"], "RUN_LIGHT")
    flat("mpscript", tb["mpscript"], "RUN_LIGHT_STASH")
    flat("mp2", tb["mp2"][1], "RUN_LIGHT_STASH")
    flat("fscript", tb["fscript"], "RUN_FULL")
    flat("slow", tb["slow"][1], "RUN_FULL")
    flat("h2", tb["h2"][2], "RUN_FULL")
    direct = list(emit.DIRECT_SEGS) + sorted(n for n in tb["segs"] if n.startswith(("g1_", "g2_", "g1h_", "g2h_")))
    for n in direct:
        rounds = sr[n]
        op = "RUN_FULL" if any(m & 3 >= 2 for o, m in rounds) else "RUN_LIGHT"
        out.append((n, op, list(rounds), [len(rounds)]))
    _PRODUCTION = (out, data, HP.h2c_scratch_consts())
    return _PRODUCTION


def production_image(name, op, rounds, data, consts):
    """the constants, then seeded residues below q; as many slots as the rounds name"""
    nslots = max(max(referenced_slots(rounds, data, op in LIGHT_OPS)) + 1, len(consts) + 1)
    rnd = random.Random("vm:production:" + name)
    return list(consts) + [rnd.randrange(Q) for _ in range(nslots - len(consts))]


def production_snapshots(op, rounds, cuts, data, img):
    """one pass of the word machine and one of tablesim over the rounds: {cut: (image as the word machine has it, the stash words,
    tablesim's residues)}"""
    light = op in LIGHT_OPS
    wm = WordMachine(data, [img])
    ts = tablesim.TableMachine([], len(img), data)
    ts.team, ts.stash = [v % Q for v in img], [0] * 12
    snaps, at = {}, 0
    for c in cuts:
        (ret, calls, sw), = wm.run(rounds[at:c], op)
        ts.run(rounds[at:c], light=light)
        snaps[c] = (list(wm.teams[0]), sw, list(ts.team))
        at = c
    return snaps
