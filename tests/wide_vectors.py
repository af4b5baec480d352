"""Operand sets and CPU references for the step routines of the wide machine (csrc/blsgpu_mlw.hip mlw::, csrc/blsgpu_lsw.hip
lsw::, csrc/blsgpu_fexpw.hip fxw::), one list per op of the test-only device library csrc/blsgpu_wide_check.hip.  Pure Python:
tests/test_wide_vectors_model.py checks the references against each other, audits every record of every table for its worst
case and shows that the sets tell wrong arithmetic from right; tests/test_gpu_wide.py compares the compiled steps with the
expected words, word for word.

References:
  * digit level: an executor of ARBITRARY packed records (exec_wstep / exec_lstep / exec_fxw / exec_tinv below: the words the
    device reads, decoded the way the device decodes them) over vmgen.gen_fp28.model_dot, vmgen.mlw_model.scale_reduce_norm and
    vmgen.fexpw_model.norm -- the arithmetic is the models', only the record decoding is here;
  * plain Python integers, independently of the digits' route: an output is = s sum A B / R (mod q), its digits 0 .. 12 lie in
    [0, 2^28) and, for the value-file steps, the value lies in (-q/64, q + q/64) (check_* below); tinv is conj(t) / (tr^2 + ti^2)
    with 0 -> 0.

A value file image is a list of dwords; slot address a (dwords) holds digit j at a + 64 j.  Slots that MORE than one lane of a
step stores to (the write sink TRASH) hold whichever lane the hardware served last: they are left out of the comparison
(written_mask), every other dword is compared -- the stored results and the unchanged rest.
"""
import random

from vmgen import gen_fp28 as G
from vmgen import mlw_model as MW
from vmgen import lsw_model as LW
from vmgen import fexpw_model as FW
from vmgen import h2cw_model as HW
from vmgen import g1w_model as GW
from vmgen import gen_mlw, gen_lsw, gen_fexpw

Q, R, L, W, MASK = G.Q, G.R, G.L, G.W, G.MASK
RINV = pow(R, -1, Q)
to_limbs, from_limbs, model_dot = G.to_limbs, G.from_limbs, G.model_dot
srn_model, norm_model = MW.scale_reduce_norm, FW.norm
QD = to_limbs(Q)
LANES = 64
N_LANE_ITEMS = (1, 63, 64, 65, 257)                    # per lane ops: one lane, either side of a wavefront, two workgroups
N_WAVE_ITEMS = (1, 3, 4, 5, 65)                        # per wavefront ops: either side of the four-wavefront workgroup, many workgroups
STRIDE, MAX_SETS = 37, 257
# the stored range of the value files: the integers inside (-q/64, q + q/64)
LO, HI = -(Q // 64), Q + Q // 64
MVF = MW.PAGES * MW.PAGE                               # dwords of blsgpu_mlw.hip's value file (mlw::VF_DW)
LVF = LW.ROWS * LW.ROW                                 # dwords of a wavefront's four pairs (lsw::VF_DW)
LINE_DW = 6 * L
FX_MAX = 16 * Q                                        # |value| the fxw steps are run with (tests/test_fexpw_model.py: max_abs < 16)


def s32(w):
    w &= 0xFFFFFFFF
    return w - (1 << 32) if w >> 31 else w


def _rnd(tag):
    return random.Random("wide-vectors/" + tag)


def in_range(v):
    return LO <= v <= HI


def item_set(i, nsets):
    return ((i * STRIDE) % MAX_SETS) % nsets


# ---- stored values ------------------------------------------------------------------------------------------------------------
def stored_values():
    """(name, integer) of the classes the issue lists, every one inside the stored range"""
    vals = [("lo", LO), ("hi", HI), ("zero", 0), ("q", Q), ("q-1", Q - 1), ("one", 1), ("minus-one", -1), ("R", R % Q), ("R2", R * R % Q)]
    tmin, tmax = to_limbs(LO)[L - 1], to_limbs(HI)[L - 1]
    low_all = (1 << (W * (L - 1))) - 1
    for name, top, low in (("ones/tmin", tmin, low_all), ("zeros/tmin+1", tmin + 1, 0), ("ones/tmax-1", tmax - 1, low_all),
                           ("zeros/tmax", tmax, 0), ("ones/0", 0, low_all), ("zeros/-1", -1, 0)):
        v = (top << (W * (L - 1))) + low
        if in_range(v):
            vals.append((name, v))
    return vals


STORED = stored_values()
STORED_INTS = [v for _, v in STORED]


def rnd_stored(rnd):
    return rnd.randrange(LO, HI + 1)


def neg_digits(d):
    """what lsw::st14n stores: the negative limb by limb, no carry pass"""
    return [-x for x in d]


def all_scales():
    """every scale of every table of the wide machine, by table family"""
    out = {}
    for fam, kinds in (("mlw", MW.KINDS), ("h2cw", HW.KINDS), ("g1w", GW.KINDS)):
        out[fam] = sorted({rec[9] for s in kinds for rec in s.rec})
    ls = {r.scale for recs in LW.RECS for r in recs}
    ls |= {2 * r.scale for recs, h in zip(LW.RECS, LW.HAS2) if h for r in recs}
    for _, outs in LW.input_records():
        for _, sc in outs:
            ls |= {sc, 2 * sc}
    out["lsw"] = sorted(ls)
    out["inputs"] = sorted({c * s for c in MW.VARIANT for s in (1, 3, -3)})          # k_miller_wide's input quads
    out["fexpw"] = sorted({sc * c for _, _, _, sc in FW.KINDS.values() for c in FW.VARIANT} | {0})
    return out


SCALES = all_scales()
SRN_SCALES = sorted(set().union(*(SCALES[f] for f in ("mlw", "h2cw", "g1w", "lsw", "inputs"))) | {0})


# ---- mutants of the executor: names -> what is done wrong ---------------------------------------------------------------------
MUTANTS = ("m47+1", "m47-1", "quot_unscaled", "quad_miss_lane", "oct_miss_quad", "addr_swap", "bs_adds_second", "scale_zext",
           "st14n_carry", "has2_reuse", "fxw_lane_index", "tinv_no_zero")


def _srn(t, s, mut=None):
    if mut == "m47+1":
        return srn_model(t, s, m47=MW.M47 + 1)
    if mut == "m47-1":
        return srn_model(t, s, m47=MW.M47 - 1)
    if mut == "quot_unscaled":
        return srn_model(t, s, quotient_top=t[L - 1])
    return srn_model(t, s)


# ---- the value-file step of blsgpu_mlw.hip --------------------------------------------------------------------------------------
def vf_rd(vf, byte_addr):
    a = byte_addr >> 2
    return [vf[a + 64 * j] for j in range(L)]


def vf_wr(vf, byte_addr, d):
    a = byte_addr >> 2
    for j in range(L):
        vf[a + 64 * j] = d[j]


def _rd2(vf, w):
    lo, hi = w & 0xFFFF, w >> 16
    return [x + y for x, y in zip(vf_rd(vf, lo), vf_rd(vf, hi))]


SHAPES = {"WSTEP_2": (2, False, False), "WSTEP_2BS": (2, True, False), "WSTEP_1": (1, False, False), "WSTEP_1OCT": (1, False, True)}


def exec_wstep(vf, rec, shape, mut=None):
    """mlw::wstep<K, BS, OCT> on an image: rec[lane] = five packed words.  Returns (new image, stores [(byte address, digits)])"""
    K, BS, OCT = SHAPES[shape]
    P = []
    for lane in range(LANES):
        w = rec[lane]
        terms = []
        for k in range(K):
            A = _rd2(vf, w[2 * k])
            if BS and mut != "bs_adds_second":
                B = vf_rd(vf, (w[2 * k + 1] >> 16) if mut == "addr_swap" else (w[2 * k + 1] & 0xFFFF))
            else:
                B = _rd2(vf, w[2 * k + 1])
            terms.append((A, B))
        P.append(model_dot(terms))
    grp = 8 if OCT else 4
    stores = []
    for lane in range(LANES):
        g0 = lane & ~(grp - 1)
        lanes = list(range(g0, g0 + grp))
        if mut == "quad_miss_lane":
            lanes.remove(g0 + ((lane + 1) & 3) + (lane & 4 if OCT else 0))
        if mut == "oct_miss_quad" and OCT:
            lanes = [x for x in lanes if (x & 4) == (lane & 4)]
        t = [sum(P[x][j] for x in lanes) for j in range(L)]
        sw = rec[lane][4]
        scale = (sw >> 16) if mut == "scale_zext" else s32(sw) >> 16
        stores.append((sw & 0xFFFF, _srn(t, scale, mut)))
    out = list(vf)
    for a, v in stores:                            # every lane reads before any lane writes
        vf_wr(out, a, v)
    return out, stores


def written_mask(stores, size):
    """dwords stored to by more than one lane: whichever lane came last holds them -- not compared"""
    seen, multi = {}, set()
    for i, st in enumerate(stores):                # (address, digits) of lane i, or (address, digits, lane): a lane's own stores are in order
        seen.setdefault(st[0], set()).add(st[2] if len(st) > 2 else i)
    for a, c in seen.items():
        if len(c) > 1:
            multi |= {(a >> 2) + 64 * j for j in range(L)}
    assert all(x < size for x in multi)
    return multi


def check_wstep(vf, rec, shape, out):
    """plain integers: every singly stored slot = scale x (sum over the lane group of sum_k A B) / R (mod q), digits normalised,
    inside the stored range"""
    K, BS, OCT = SHAPES[shape]
    val = lambda a: from_limbs(vf_rd(vf, a))
    T = []
    for lane in range(LANES):
        w, s = rec[lane], 0
        for k in range(K):
            A = val(w[2 * k] & 0xFFFF) + val(w[2 * k] >> 16)
            B = val(w[2 * k + 1] & 0xFFFF) + (0 if BS else val(w[2 * k + 1] >> 16))
            s += A * B
        T.append(s)
    grp = 8 if OCT else 4
    count = {}
    for lane in range(LANES):
        count[rec[lane][4] & 0xFFFF] = count.get(rec[lane][4] & 0xFFFF, 0) + 1
    for lane in range(LANES):
        a, scale = rec[lane][4] & 0xFFFF, s32(rec[lane][4]) >> 16
        if count[a] > 1:
            continue
        g0 = lane & ~(grp - 1)
        d = vf_rd(out, a)
        v = from_limbs(d)
        assert all(0 <= x <= MASK for x in d[:L - 1]), "digits not normalised"
        assert (v * R - scale * sum(T[g0:g0 + grp])) % Q == 0, "lane %d: wrong residue" % lane
        assert LO <= v <= HI, "lane %d: %.4f q outside the stored range" % (lane, v / Q)


# ---- images -----------------------------------------------------------------------------------------------------------------
FILLS = ("lo", "hi", "alt", "ones", "random")


def _fill_value(fill, i, rnd):
    if fill == "lo":
        return LO
    if fill == "hi":
        return HI
    if fill == "alt":
        return HI if i & 1 else LO
    if fill == "alt2":
        return LO if i & 1 else HI
    if fill == "ones":
        return dict(STORED)["ones/tmax-1"] if i % 3 else dict(STORED)["ones/tmin"]
    return rnd_stored(rnd)


def mlw_image(fill, tag, zero_slots=()):
    """an image of blsgpu_mlw.hip's value file with every slot of every page filled; zero_slots (dword addresses) hold zero"""
    rnd = _rnd("image/%s/%s" % (fill, tag))
    vf = [0] * MVF
    for page in range(MW.PAGES):
        for s in range(64):
            a = page * MW.PAGE + s
            d = to_limbs(_fill_value(fill, s + page, rnd))
            for j in range(L):
                vf[a + 64 * j] = d[j]
    for a in zero_slots:
        for j in range(L):
            vf[a + 64 * j] = 0
    return vf


def _zero_quad(names):
    return [names.slot("ZERO", c) for c in MW.VARIANT]


def step_shape(step):
    return ("WSTEP_2", "WSTEP_2BS", "WSTEP_1", "WSTEP_1OCT")[MW.variant_of(step)]


TABLES = (("mlw", MW.KINDS, MW.N), ("h2cw", HW.KINDS, HW.N), ("g1w", GW.KINDS, GW.N))


def real_wstep_items():
    """every kind of every table of the machine as ONE step from images filled per class: [(family, kind index, shape, tag, image, rec)]"""
    out = []
    for fam, kinds, names in TABLES:
        for index, step in enumerate(kinds):
            rec = gen_mlw.record_words(step)
            for fill in FILLS:
                tag = "%s/%s/%s" % (fam, step.name, fill)
                out.append((fam, index, step_shape(step), tag, mlw_image(fill, tag, _zero_quad(names)), rec))
    return out


def real_wstep_sets():
    """the same by shape: {shape: [(tag, image, rec)]}"""
    out = {s: [] for s in SHAPES}
    for fam, index, shape, tag, image, rec in real_wstep_items():
        out[shape].append((tag, image, rec))
    return out


# the table-driven ops of the device library: (family, shape) -> op name and code
TREC = {("mlw", "WSTEP_2"): ("TREC_MLW_2", 40), ("mlw", "WSTEP_2BS"): ("TREC_MLW_2BS", 41), ("mlw", "WSTEP_1"): ("TREC_MLW_1", 42),
        ("mlw", "WSTEP_1OCT"): ("TREC_MLW_1OCT", 43), ("h2cw", "WSTEP_2"): ("TREC_H2CW_2", 44), ("h2cw", "WSTEP_2BS"): ("TREC_H2CW_2BS", 45),
        ("h2cw", "WSTEP_1"): ("TREC_H2CW_1", 46), ("g1w", "WSTEP_1"): ("TREC_G1W_1", 47)}


def _pk(a, b):
    return (4 * a) | ((4 * b) << 16)


def synthetic_wstep_sets():
    """records no table has: {shape: [(tag, image, rec)]}"""
    out = {s: [] for s in SHAPES}
    Z = MW.ZERO
    TR = MW.TRASH
    top = MVF - 64 * (L - 1) - 1                   # the largest slot address of the value file
    real_top = max(max(r[:9]) for s in MW.KINDS for r in s.rec)
    for shape, (K, BS, OCT) in SHAPES.items():
        def rec_of(f):
            rows = []
            for lane in range(LANES):
                a, b, a2, b2, dst, scale = f(lane)
                rows.append((_pk(*a), _pk(*b), _pk(*a2) if K == 2 else 0, _pk(*b2) if K == 2 else 0, (4 * dst) | ((scale & 0xFFFF) << 16)))
            return rows
        dst_of = lambda lane: 5 * MW.PAGE + lane   # page 5: one slot per lane
        img = lambda fill, tag, zero=(): mlw_image(fill, "syn/%s/%s" % (shape, tag), zero)
        # all 64 lanes read the same slot
        out[shape].append(("same-slot", img("random", "same"), rec_of(lambda l: ((7, 7), (7, 7), (7, 7), (7, 7), dst_of(l), MW.VARIANT[l & 3]))))
        # 64 lanes read 64 different slots (and both halves of an address word equal)
        out[shape].append(("own-slots", img("random", "own"),
                           rec_of(lambda l: ((l, l), (MW.PAGE + l, MW.PAGE + l), (2 * MW.PAGE + l, 2 * MW.PAGE + l), (3 * MW.PAGE + l, 3 * MW.PAGE + l), dst_of(l), 1))))
        # halves differ: a swap of the halves must show (first operand of a one-slot form: its second half is another slot)
        out[shape].append(("halves", img("random", "halves", [Z]),
                           rec_of(lambda l: ((l, Z), (MW.PAGE + l, 2 * MW.PAGE + (l ^ 1)), (Z, 3 * MW.PAGE + l), (MW.PAGE + (l ^ 5), Z), dst_of(l), -MW.VARIANT[l & 3]))))
        # a lane reads the slot another lane of the same step writes: every lane reads before any lane writes
        out[shape].append(("read-written", img("random", "rw"),
                           rec_of(lambda l: (((l + 1) & 63, (l + 9) & 63), ((l + 2) & 63, l), ((l + 63) & 63, (l + 5) & 63), ((l + 17) & 63, (l + 33) & 63), l, MW.VARIANT[l & 3]))))
        # many lanes store to TRASH, the largest slot addresses (of the file, and of the tables' own use), extreme scales
        out[shape].append(("trash-top", img("hi", "top"),
                           rec_of(lambda l: ((top, real_top), (top - l, real_top), (top, top), (real_top, top - 1), TR if l & 7 else dst_of(l), (72, -72, 36, -36)[(l >> 3) & 3]))))
        out[shape].append(("scale-zero", img("alt", "zero"), rec_of(lambda l: ((l, MW.PAGE + l), (l, 1), (2, l), (l, 3), dst_of(l), 0))))
        out[shape].append(("scales", img("alt2", "scales"),
                           rec_of(lambda l: ((l, MW.PAGE + l), (2 * MW.PAGE + l, 3 * MW.PAGE + l), (4 * MW.PAGE + l, l), (MW.PAGE + l, l), dst_of(l), SCALES["mlw"][l % len(SCALES["mlw"])]))))
        if BS:
            # the second address of a one-slot operand is garbage: ignored
            rnd = _rnd("garbage")
            garbage = lambda: rnd.randrange(MVF - 64 * (L - 1))     # (some other slot, wherever: never read)
            out[shape].append(("bs-garbage", img("random", "garbage"),
                               rec_of(lambda l: ((l, 3 * MW.PAGE + l), (MW.PAGE + l, garbage()), (4 * MW.PAGE + l, 2 * MW.PAGE + l), (l, garbage()), dst_of(l), MW.VARIANT[l & 3]))))
    return out


def wload_sets():
    """(tag, image, 64 digit vectors, 64 byte destinations, 64 factors): residues in Montgomery digits, quad i to value i's four slots, times
    the factor k_miller_wide gives that quad (-3 for quad 0, 3 for quad 2: the scales +-3, +-6 with the multiples)"""
    rnd = _rnd("wload")
    sets = []
    for tag, vals in (("edges", [0, 1, Q - 1, R % Q, R * R % Q, (Q - 1) // 2, (Q + 1) // 2] + [rnd.randrange(Q) for _ in range(9)]),
                      ("random", [rnd.randrange(Q) for _ in range(16)])):
        digs, dst = [], []
        sc = [-3 if lane >> 2 == 0 else (3 if lane >> 2 == 2 else 1) for lane in range(LANES)]
        for lane in range(LANES):
            qd = lane >> 2
            digs.append(to_limbs(vals[qd]))
            dst.append(4 * (MW.PAGE + 4 * qd + (lane & 3)) if qd < 14 else 4 * MW.TRASH)
        sets.append((tag, mlw_image("random", "wload/" + tag), digs, dst, sc))
    return sets


def exec_wload(vf, digs, dst, sc):
    out, stores = list(vf), []
    for lane in range(LANES):
        stores.append((dst[lane], srn_model(digs[lane], sc[lane] * MW.VARIANT[lane & 3])))
    for a, v in stores:
        vf_wr(out, a, v)
    return out, stores


# ---- line-stream steps ------------------------------------------------------------------------------------------------------------
LSHAPES = {"LSTEP_2": (2, False), "LSTEP_3": (3, False), "LSTEP_4": (4, False), "LSTEP_4_HAS2": (4, True), "LSTEP_2_HAS2": (2, True),
           "LSTEP_3_HAS2": (3, True)}
LSLOT_KIND = {s: v for (n, v), s in LW.SLOT.items()}   # slot -> the multiple it holds (+-1, +-2); ZERO and TRASH: 1


def lsw_rec_words(rec, K):
    w = gen_lsw._words(rec, K)
    return tuple(w[:2 * K] + w[8:11])


def lsw_image(fills, tag):
    """four pairs, pair i filled by class fills[i]; negated slots hold limb-negated digits, ZERO zero"""
    vf = [0] * LVF
    for i in range(4):
        rnd = _rnd("limage/%s/%s/%d" % (fills[i], tag, i))
        for slot in range(LW.NSLOTS):
            v = _fill_value(fills[i], slot, rnd)
            d = to_limbs(v)
            if LSLOT_KIND[slot] < 0:
                d = neg_digits(d)
            if slot == LW.SLOT[("ZERO", 1)]:
                d = [0] * L
            a = LW.rel_addr(slot) + i
            for j in range(L):
                vf[a + 64 * j] = d[j]
    return vf


# the instantiation k_ml_lines_wide runs every kind with (blsgpu_lsw.hip: a kind of fewer products is padded with ZERO x ZERO)
KERNEL_LSTEP = {"CK1": "LSTEP_2", "CK2": "LSTEP_4", "L1": "LSTEP_2_HAS2", "L2": "LSTEP_3_HAS2", "C1": "LSTEP_3", "C2": "LSTEP_4", "C3": "LSTEP_4",
                "C4": "LSTEP_4_HAS2"}


def lstep_shape(kind):
    shape = KERNEL_LSTEP[LW.KINDS[kind].name]
    assert LSHAPES[shape][0] >= LW.KINDS[kind].K and LSHAPES[shape][1] == LW.HAS2[kind]
    return shape


def lstep_sets():
    """{shape: [(tag, image, rec (64 lanes), has_line)]}: every kind of lsw_model.RECS, pairs at different classes"""
    out = {s: [] for s in LSHAPES}
    for kind, recs in enumerate(LW.RECS):
        K = LSHAPES[lstep_shape(kind)][0]
        rec = [lsw_rec_words(recs[lane & 15], K) for lane in range(LANES)]
        for n, fills in enumerate((("lo", "hi", "alt", "random"), ("ones", "alt2", "random", "hi"), ("random", "random", "lo", "alt"))):
            tag = "%s/%d" % (LW.KINDS[kind].name, n)
            out[lstep_shape(kind)].append((tag, lsw_image(fills, tag), rec, n != 2))
    real_count = {shape: len(v) for shape, v in out.items()}
    # no table has a negative scale (the sign-extended field of the record): the first kind of every shape with the scales -1, 2, -3, 1
    for shape, sets in out.items():
        tag, image, rec, _ = sets[0]
        K = LSHAPES[shape][0]
        neg = [w[:2 * K + 2] + ((w[2 * K + 2] & 0xFFFF0000) | ((-1, 2, -3, 1)[lane & 3] & 0xFFFF),) for lane, w in enumerate(rec)]
        sets.append((tag + "/signed-scales", image, neg, True))
    for shape, sets in synthetic_lstep_sets().items():
        out[shape] += sets
    lstep_sets.real_count = real_count             # the first real_count[shape] sets of a shape are the tables' own kinds, three per kind
    return out


def synthetic_lstep_sets():
    """records no table has, per shape: {shape: [(tag, image, rec, has_line)]}.  Column sums stay within 8 / 9 units (gen_lsw asserts it
    while packing): with K products the second operand is one slot where two would not fit"""
    Z, TR = LW.SLOT[("ZERO", 1)], LW.SLOT[("TRASH", 1)]
    P = [s for s in range(LW.NSLOTS) if s not in (Z, TR) and LSLOT_KIND[s] > 0]
    M = [s for s in range(LW.NSLOTS) if LSLOT_KIND[s] < 0]
    assert len(P) >= 32 and len(M) >= 4
    top = 16 * LW.ROWS - 1                         # the largest slot address of a pair's file (past the named slots: reads zero)
    out = {}
    for shape, (K, HAS2) in LSHAPES.items():
        second = (lambda s: (s, s)) if K == 2 else (lambda s: (s, Z))

        def build(f):
            rows = []
            for lane in range(LANES):
                prods, dsts, scale, lineout = f(lane & 15, lane >> 4)
                prods = (prods * K)[:K]
                rows.append(lsw_rec_words(LW.Rec([(a[0], a[1], b[0], b[1]) for a, b in prods], dsts, scale, lineout), K))
            return rows
        sets = []
        img = lambda tag: lsw_image(("random", "hi", "lo", "alt"), "syn/%s/%s" % (shape, tag))
        own = lambda r: (P[r], M[r % len(M)] if r < len(M) else TR, P[16 + r], TR)
        # all lanes read the same slot, both halves of an address word equal
        sets.append(("same-slot", img("same"), build(lambda r, p: ([((P[3], P[3]), second(P[3]))], own(r), 1, None)), False))
        # a lane reads the slots the other lanes of its pair write (value, negative and double): every lane reads before any lane writes
        sets.append(("read-written", img("rw"),
                     build(lambda r, p: ([((P[(r + 1) & 15], M[(r + 1) % len(M)]), second(P[16 + ((r + 5) & 15)])), ((P[(r + 7) & 15], Z), second(P[(r + 2) & 15]))],
                                         own(r), (1, -1, 2, -3)[r & 3], r % 6 if r < 6 else None)), True))
        # a lane's own stores land on one slot: st14, then st14n, then the two of a second reduction -- the last one stays
        sets.append(("store-order", img("order"), build(lambda r, p: ([((P[r], P[16 + r]), second(P[(r + 3) & 15]))], (P[r], P[r], P[r], P[16 + r]), 1, None)), False))
        # many lanes on TRASH, the largest slot address
        sets.append(("trash-top", img("top"),
                     build(lambda r, p: ([((top, P[r]), second(top - 1))], (top, TR, TR, TR) if r == 0 else ((TR, TR, TR, TR) if r & 3 else own(r)), 3, None)), False))
        # an operand made only of limb-negated slots, alone and beside a normal one
        sets.append(("negated-operands", img("neg"),
                     build(lambda r, p: ([((M[r % len(M)], M[(r + 1) % len(M)]), second(P[r])), ((M[(r + 2) % len(M)], P[16 + r]), (M[(r + 3) % len(M)], Z))],
                                         own(r), -1 if r & 1 else 1, None)), False))
        out[shape] = sets
    return out


def exec_lstep(vf, rec, shape, has_line, mut=None):
    """lsw::lstep<K, HAS2> for the four pairs of a wavefront: (new image, stores, line words 4 x 84 with None where nothing is written)"""
    K, HAS2 = LSHAPES[shape]
    stores, lines = [], [None] * (4 * LINE_DW)
    for lane in range(LANES):
        base = 4 * (lane >> 4)
        w = rec[lane]
        terms = []
        for k in range(K):
            A = [x + y for x, y in zip(vf_rd(vf, base + (w[2 * k] & 0xFFFF)), vf_rd(vf, base + (w[2 * k] >> 16)))]
            B = [x + y for x, y in zip(vf_rd(vf, base + (w[2 * k + 1] & 0xFFFF)), vf_rd(vf, base + (w[2 * k + 1] >> 16)))]
            terms.append((A, B))
        p = model_dot(terms)
        d1, d2, sl = w[2 * K], w[2 * K + 1], w[2 * K + 2]
        if mut == "addr_swap":
            d1, d2 = (d1 >> 16) | ((d1 & 0xFFFF) << 16), (d2 >> 16) | ((d2 & 0xFFFF) << 16)
        scale = (sl & 0xFFFF) if mut == "scale_zext" else s32(sl << 16) >> 16
        V = _srn(p, scale, mut)

        def negated(v):
            if mut == "st14n_carry":
                return norm_model(neg_digits(v))
            return neg_digits(v)
        mine = [(base + (d1 & 0xFFFF), V), (base + (d1 >> 16), negated(V))]
        lo = (sl >> 16) & 0xFF
        if has_line and lo != 0xFF:
            for j in range(L):
                lines[(lane >> 4) * LINE_DW + lo * L + j] = V[j]
        if HAS2:
            V2 = [2 * x for x in V] if mut == "has2_reuse" else _srn(p, 2 * scale, mut)
            mine += [(base + (d2 & 0xFFFF), V2), (base + (d2 >> 16), negated(V2))]
        stores.append(mine)
    out = list(vf)
    flat = []
    for i in range(4):                             # the lanes run in step: store i of every lane before store i + 1 of any
        for lane, mine in enumerate(stores):
            if i < len(mine):
                vf_wr(out, mine[i][0], mine[i][1])
                flat.append((mine[i][0], mine[i][1], lane))
    return out, flat, lines


def check_lstep(vf, rec, shape, out):
    """plain integers: singly stored slots hold +-(1 or 2) scale sum_k A B / R (mod q); the value and its double in the stored range"""
    K, HAS2 = LSHAPES[shape]
    val = lambda a: from_limbs(vf_rd(vf, a))
    count = {}
    plan = []
    for lane in range(LANES):
        base = 4 * (lane >> 4)
        w = rec[lane]
        T = sum((val(base + (w[2 * k] & 0xFFFF)) + val(base + (w[2 * k] >> 16))) * (val(base + (w[2 * k + 1] & 0xFFFF)) + val(base + (w[2 * k + 1] >> 16)))
                for k in range(K))
        scale = s32(w[2 * K + 2] << 16) >> 16
        d1, d2 = w[2 * K], w[2 * K + 1]
        mine = [(base + (d1 & 0xFFFF), scale, 1), (base + (d1 >> 16), scale, -1)]
        if HAS2:
            mine += [(base + (d2 & 0xFFFF), 2 * scale, 1), (base + (d2 >> 16), 2 * scale, -1)]
        for a, _, _ in mine:
            count[a] = count.get(a, 0) + 1
        plan.append((T, mine))
    for T, mine in plan:
        for a, sc, sign in mine:
            if count[a] > 1:
                continue
            d = vf_rd(out, a)
            v = sign * from_limbs(d)
            assert all(0 <= sign * x <= MASK for x in d[:L - 1]), "digits not normalised"
            assert (v * R - sc * T) % Q == 0, "wrong residue"
            assert LO <= v <= HI, "%.4f q outside the stored range" % (v / Q)


# ---- per lane ops -------------------------------------------------------------------------------------------------------------
def srn_sets():
    """(tag, t, s, ranged): t the sum of a lane group's product results, s a scale of the tables.  ranged: the result must lie in the
    stored range (the sets made the way a step makes them: at most four -- eight for |s| <= 2 -- results of products, each in
    (-q/256, q + q/256))"""
    rnd = _rnd("srn")
    sets = []
    plo, phi = -(Q // 256), Q + Q // 256
    for s in SRN_SCALES:
        for n, v in ((4, plo), (4, phi), (1, 0), (1, Q), (2, Q - 1), (3, 1)):
            t = [n * x for x in to_limbs(v)]
            sets.append(("edge/%d/%d" % (s, n), t, s, True))
        if abs(s) <= 2:
            sets.append(("oct/%d" % s, [8 * x for x in to_limbs(phi)], s, True))
            sets.append(("oct-lo/%d" % s, [8 * x for x in to_limbs(plo)], s, True))
        for _ in range(2):
            t = [sum(c) for c in zip(*[to_limbs(rnd.randrange(plo, phi + 1)) for _ in range(4)])]
            sets.append(("random/%d" % s, t, s, True))
    # inputs: a residue's digits times the multiples the kernels store
    for s in SCALES["inputs"] + SCALES["lsw"]:
        for v in (0, 1, Q - 1, R % Q, rnd.randrange(Q)):
            sets.append(("input/%d" % s, to_limbs(v), s, True))
    # digit patterns of the sum itself: every limb 0 .. 12 at the most four stored limbs give, negative limbs (sums with st14n's slots)
    for s in (1, -2, 72, -72):
        sets.append(("limbs-max/%d" % s, [4 * MASK] * (L - 1) + [4 * to_limbs(HI)[L - 1] - 4], s, False))
        sets.append(("limbs-neg/%d" % s, [-MASK] * (L - 1) + [to_limbs(HI)[L - 1]], s, False))
    # top limbs at which the quotient estimate turns on the last bit of M47: top = m QTOP (top M47 mod 2^47 just below 2^47), and
    # the tops with top M47 mod 2^47 < top
    for m in (1, 2, 3, 4, 8):
        for s in (1, -1):
            sets.append(("m47-edge/%d" % (s * m), [0] * (L - 1) + [m * MW.QTOP], s, False))
    found = 0
    for j in range(1, 20000):
        top = -(-(j << 47) // MW.M47)
        if found < 4 and top < (1 << 31) and top * MW.M47 - (j << 47) < top:
            sets.append(("m47-low/%d" % j, [MASK] * (L - 1) + [top], 1, False))
            found += 1
    assert found >= 2
    return sets


def check_srn(t, s, out, ranged):
    v = from_limbs(out)
    assert all(0 <= x <= MASK for x in out[:L - 1]) and -(1 << 31) <= out[L - 1] < (1 << 31)
    assert (v - s * from_limbs(t)) % Q == 0
    if ranged:
        assert LO <= v <= HI, "%.4f q" % (v / Q)


def scale_norm_sets():
    rnd = _rnd("scale_norm")
    sets = []
    for s in SCALES["fexpw"]:
        for v in (FX_MAX - 1, -FX_MAX + 1, 0, 1, -1, Q, rnd.randrange(-FX_MAX, FX_MAX)):
            sets.append(("fx/%d" % s, [4 * x for x in norm_model([c for c in to_limbs(v)])], s))
        sets.append(("neg-limbs/%d" % s, [-MASK] * (L - 1) + [3], s))
        sets.append(("max-limbs/%d" % s, [4 * MASK] * (L - 1) + [-5], s))
    return sets


def exec_scale_norm(t, s):
    return norm_model([s * x for x in t])


def stored_zero_sets():
    """(tag, digits, is zero mod q): both digit forms of zero, the neighbours, the limb-negated q, the range's ends"""
    sets = [("zero", [0] * L, True), ("q", list(QD), True)]
    for name, v in STORED:
        if v not in (0, Q):
            sets.append((name, to_limbs(v), False))
    for j in range(L):
        d = list(QD)
        d[j] ^= 1
        sets.append(("q^bit/%d" % j, d, False))
        z = [0] * L
        z[j] = 1
        sets.append(("0^bit/%d" % j, z, False))
    sets.append(("neg-q", neg_digits(QD), False))      # = -q: zero mod q, but no stored value has these digits (st14n's slots are never tested)
    return sets


# ---- final-exponentiation steps ---------------------------------------------------------------------------------------------
def fx_bank(fill, tag):
    """64 x 14 digits: lane r of a quad holds VARIANT[r] x the quad's value, |value| < 16 q; quads 12 .. 15 as the kernel holds them"""
    rnd = _rnd("fx/%s/%s" % (fill, tag))
    bank = []
    for quad in range(16):
        if fill == "max":
            v = FX_MAX - 1 - quad
        elif fill == "min":
            v = -FX_MAX + 1 + quad
        elif fill == "alt":
            v = (FX_MAX - 1) if quad & 1 else (-FX_MAX + 1)
        else:
            v = rnd.randrange(-FX_MAX + 1, FX_MAX)
        if quad == FW.THIRD_QUAD:
            v = FW.THIRD
        if quad > FW.THIRD_QUAD:
            v = 0
        bank += [norm_model([c * d for d in to_limbs(v)]) for c in FW.VARIANT]
    return bank


def fx_tables():
    """the real tables as the header holds them: name -> rows of 64 byte addresses (vv: 4 rows; vg: 9 rows, product-major)"""
    t = {n: gen_fexpw._kind_vv(FW.KINDS[n][0]) for n in ("CSQ", "CONJ")}
    for n in ("MUL", "FROBC", "FROB"):
        t[n] = [row for prod in gen_fexpw._kind_vg(FW.KINDS[n][0]) for row in prod]
    return t


FX_TABLES = fx_tables()


def exec_fxw(V, G, rows, vg, mut=None):
    """fxw::step_vv (rows s1 .. s4, scale 3) / step_vg (rows s1 s2 s3 per product, scale 1): the new V"""
    at = lambda row, lane: lane if mut == "fxw_lane_index" else (rows[row][lane] >> 2) & 63
    P = []
    for lane in range(LANES):
        add = lambda x, y: [a + b for a, b in zip(x, y)]
        if vg:
            terms = [(add(V[at(3 * i, lane)], V[at(3 * i + 1, lane)]), G[at(3 * i + 2, lane)]) for i in range(3)]
        else:
            terms = [(add(V[at(0, lane)], V[at(1, lane)]), add(V[at(2, lane)], V[at(3, lane)]))]
        P.append(model_dot(terms))
    out = [list(v) for v in V]
    for lane in range(4 * FW.HOME_QUADS):
        q0 = lane & ~3
        lanes = [q0, q0 + 1, q0 + 2, q0 + 3]
        if mut == "quad_miss_lane":
            lanes.remove(q0 + ((lane + 1) & 3))
        sc = (1 if vg else 3) * FW.VARIANT[lane & 3]
        out[lane] = norm_model([sc * sum(P[x][j] for x in lanes) for j in range(L)])
    return out


def check_fxw(V, G, rows, vg, out):
    val = lambda bank, row, lane: from_limbs(bank[(rows[row][lane] >> 2) & 63])
    T = []
    for lane in range(LANES):
        if vg:
            T.append(sum((val(V, 3 * i, lane) + val(V, 3 * i + 1, lane)) * val(G, 3 * i + 2, lane) for i in range(3)))
        else:
            T.append((val(V, 0, lane) + val(V, 1, lane)) * (val(V, 2, lane) + val(V, 3, lane)))
    for lane in range(LANES):
        if lane >= 4 * FW.HOME_QUADS:
            assert out[lane] == V[lane], "a lane outside the home quads changed"
            continue
        q0 = lane & ~3
        sc = (1 if vg else 3) * FW.VARIANT[lane & 3]
        assert all(0 <= x <= MASK for x in out[lane][:L - 1])
        assert (from_limbs(out[lane]) * R - sc * sum(T[q0:q0 + 4])) % Q == 0, "lane %d" % lane


def fxw_sets():
    """{op: [(tag, V, G or None, rows or None)]}; rows None: the op reads the real table itself"""
    out = {}
    for name in ("CSQ", "CONJ"):
        out["FXW_VV_" + name] = [("%s/%s" % (name, f), fx_bank(f, name), None, None) for f in ("max", "min", "alt", "random")]
    for name in ("MUL", "FROB", "FROBC"):
        sets = [("%s/%s" % (name, f), fx_bank(f, name + "V"), fx_bank(g, name + "G"), None) for f, g in (("max", "max"), ("min", "max"), ("alt", "random"), ("random", "random"))]
        if name != "MUL":
            sets.append((name + "/gamma", fx_bank("random", name + "gV"), [list(x) for x in FW.frob_constants(1 if name == "FROB" else 0)], None))
        out["FXW_VG_" + name] = sets
    rnd = _rnd("fx-tables")
    syn_vv, syn_vg = [], []
    patterns = {
        "same-lane": lambda l, i: 4 * 5,
        "cross-quads": lambda l, i: 4 * ((l + 4 * (i + 1)) & 63),
        "cross-halves": lambda l, i: 4 * ((l + 32 + i) & 63),
        "reverse": lambda l, i: 4 * (63 - l),
        "random": lambda l, i: 4 * rnd.randrange(64),
        "own-lane": lambda l, i: 4 * ((l + (i & 1)) & 63),
    }
    for tag, f in patterns.items():
        syn_vv.append((tag, fx_bank("random" if tag != "reverse" else "alt", "vv" + tag), None, [[f(l, i) for l in range(LANES)] for i in range(4)]))
        syn_vg.append((tag, fx_bank("random", "vgV" + tag), fx_bank("random" if tag != "reverse" else "max", "vgG" + tag),
                       [[f(l, i) for l in range(LANES)] for i in range(9)]))
    # the real tables through the table-driven op as well: the same words must come out of both routes
    for name in ("CSQ", "CONJ"):
        syn_vv.append(("table/" + name, fx_bank("random", "t" + name), None, FX_TABLES[name]))
    for name in ("MUL", "FROB", "FROBC"):
        syn_vg.append(("table/" + name, fx_bank("random", "tV" + name), fx_bank("random", "tG" + name), FX_TABLES[name]))
    out["FXW_STEP_VV"], out["FXW_STEP_VG"] = syn_vv, syn_vg
    return out


FX_TABLE_OF = {"FXW_VV_CSQ": "CSQ", "FXW_VV_CONJ": "CONJ", "FXW_VG_MUL": "MUL", "FXW_VG_FROB": "FROB", "FXW_VG_FROBC": "FROBC"}
TO_VM_D, FROM_VM_D = to_limbs((1 << 384) % Q), to_limbs((1 << 400) % Q)


def tinv_sets():
    rnd = _rnd("tinv")
    sets = []
    for tag, (tr, ti) in (("zero", (0, 0)), ("zero-as-q", (Q, Q)), ("zero-mixed", (Q, 0)), ("one", (R % Q, 0)), ("i", (0, R % Q)), ("re-only", (rnd.randrange(Q), 0)),
                          ("im-only", (Q, rnd.randrange(Q))), ("max", (FX_MAX - 1, -FX_MAX + 1)), ("random", (rnd.randrange(Q), rnd.randrange(Q))),
                          ("random-wide", (rnd.randrange(-FX_MAX, FX_MAX), rnd.randrange(-FX_MAX, FX_MAX)))):
        V = fx_bank("random", "tinv" + tag)
        for part, v in enumerate((tr, ti)):
            for r, c in enumerate(FW.VARIANT):
                V[4 * part + r] = norm_model([c * d for d in to_limbs(v)])
        sets.append((tag, V, (tr, ti)))
    return sets


def exec_tinv(V, mut=None):
    """fxw::tinv digit by digit: norm = re^2 + im^2 (fp28_dot2), through the 32-bit-limb inversion (to_vm: canonical x 2^384;
    fq_inv_var: canonical, 0 -> 0; from_vm), conj(t) x 1 / norm, every lane its multiple"""
    re, im = V[0], V[4]
    n = model_dot([(re, re), (im, im)])
    w = from_limbs(model_dot([(n, TO_VM_D)])) % Q
    if w == 0:
        v = 1 if mut == "tinv_no_zero" else 0
    else:
        v = pow(w, -1, Q) * (1 << 768) % Q
    ni = model_dot([(to_limbs(v), FROM_VM_D)])
    a, b = model_dot([(re, ni)]), model_dot([(neg_digits(im), ni)])
    out = [list(x) for x in V]
    for lane in range(4 * FW.HOME_QUADS):
        src = a if lane >> 2 == 0 else (b if lane >> 2 == 1 else [0] * L)
        out[lane] = norm_model([FW.VARIANT[lane & 3] * d for d in src])
    return out


def check_tinv(V, out):
    tr, ti = from_limbs(V[0]) * RINV % Q, from_limbs(V[4]) * RINV % Q
    nrm = (tr * tr + ti * ti) % Q
    inv = pow(nrm, -1, Q) if nrm else 0
    want = (tr * inv % Q, -ti * inv % Q)
    for lane in range(LANES):
        if lane >= 4 * FW.HOME_QUADS:
            assert out[lane] == V[lane]
            continue
        w = want[lane >> 2] if lane >> 2 < 2 else 0
        assert (from_limbs(out[lane]) * RINV - FW.VARIANT[lane & 3] * w) % Q == 0, "lane %d" % lane


# ---- the ops of the device library: code, words in / out per item, the sets as words, the expected words ---------------------------
class Op:
    def __init__(self, name, code, win, wout, wave):
        self.name, self.code, self.win, self.wout, self.wave = name, code, win, wout, wave
        self.sets = []                             # (tag, words in, expected words out with None where not compared)

    def add(self, tag, words, expected):
        assert len(words) == self.win and len(expected) == self.wout, (self.name, tag, len(words), len(expected))
        self.sets.append((tag, [s32(w) for w in words], expected))


def _rows64(rec, nw):
    return [rec[lane][i] for i in range(nw) for lane in range(LANES)]


def _masked(image, stores):
    m = written_mask(stores, len(image))
    return [None if i in m else x for i, x in enumerate(image)]


def _flat(bank):
    return [x for lane in bank for x in lane]


_OPS = None


def ops():
    """name -> Op, built once (the expected words are the digit-level reference's)"""
    global _OPS
    if _OPS is not None:
        return _OPS
    o = {}
    op = o["SRN"] = Op("SRN", 0, L + 1, L, False)
    for tag, t, s, _ in srn_sets():
        op.add(tag, t + [s], srn_model(t, s))
    op = o["FXW_SCALE_NORM"] = Op("FXW_SCALE_NORM", 1, L + 1, L, False)
    for tag, t, s in scale_norm_sets():
        op.add(tag, t + [s], exec_scale_norm(t, s))
    op = o["STORED_ZERO"] = Op("STORED_ZERO", 2, L, L + 1, False)
    for tag, d, z in stored_zero_sets():
        assert MW.is_zero_stored(d) == z
        op.add(tag, d, list(d) + [1 if z else 0])
    real, syn = real_wstep_sets(), synthetic_wstep_sets()
    for code, (name, shape) in enumerate((("WSTEP_2", "WSTEP_2"), ("WSTEP_2BS", "WSTEP_2BS"), ("WSTEP_1", "WSTEP_1"), ("WSTEP_1OCT", "WSTEP_1OCT"),
                                          ("WSTEP_2_X4", "WSTEP_2"), ("WSTEP_1_X4", "WSTEP_1")), 10):
        op = o[name] = Op(name, code, MVF + 320, MVF, True)
        op.shape = shape
        sets = syn[shape] + real[shape]
        if name.endswith("_X4"):                   # the four-wavefront form: the synthetic records and a table kind of each family
            sets = syn[shape] + real[shape][::7]
        for tag, image, rec in sets:
            new, stores = exec_wstep(image, rec, shape)
            op.add(tag, image + _rows64(rec, 5), _masked(new, stores))
    op = o["WLOAD"] = Op("WLOAD", 16, MVF + 64 * L + 128, MVF, True)
    for tag, image, digs, dst, sc in wload_sets():
        new, stores = exec_wload(image, digs, dst, sc)
        op.add(tag, image + _flat(digs) + dst + sc, _masked(new, stores))
    for (fam, shape), (name, code) in TREC.items():
        o[name] = Op(name, code, MVF + 1, MVF, True)
    first = {}
    for fam, index, shape, tag, image, rec in real_wstep_items():
        new, stores = exec_wstep(image, rec, shape)
        o[TREC[(fam, shape)][0]].add(tag, image + [index], _masked(new, stores))
        if index == 0 and fam not in first:        # a kind past the table reads kind 0
            first[fam] = True
            nk = len(dict((f, k) for f, k, _ in TABLES)[fam])
            o[TREC[(fam, shape)][0]].add(tag + "/clamped", image + [nk + 3], _masked(new, stores))
    for name in [n for n, op in o.items() if op.code >= 40 and not op.sets]:
        del o[name]                                # (h2cw has one-product kinds only)
    ls = lstep_sets()
    for code, name in enumerate(("LREC_2", "LREC_3", "LREC_4", "LREC_4_HAS2", "LREC_2_HAS2", "LREC_3_HAS2"), 50):
        shape = name.replace("LREC", "LSTEP")
        op = o[name] = Op(name, code, LVF + 2, LVF + 4 * LINE_DW, True)
        kinds = [k for k in range(len(LW.RECS)) if lstep_shape(k) == shape]
        for n, (tag, image, rec, has_line) in enumerate(ls[shape][:lstep_sets.real_count[shape]]):
            new, stores, lines = exec_lstep(image, rec, shape, has_line)
            op.add(tag, image + [kinds[n // 3], 1 if has_line else 0],
                   _masked(new, stores) + [s32(0xAAAAAAAA) if x is None else x for x in lines])
    for code, name in enumerate(("LSTEP_2", "LSTEP_3", "LSTEP_4", "LSTEP_4_HAS2", "LSTEP_2_HAS2", "LSTEP_3_HAS2"), 20):
        K = LSHAPES[name][0]
        op = o[name] = Op(name, code, LVF + (2 * K + 3) * 64 + 1, LVF + 4 * LINE_DW, True)
        op.shape = name
        for tag, image, rec, has_line in ls[name]:
            new, stores, lines = exec_lstep(image, rec, name, has_line)
            op.add(tag, image + _rows64(rec, 2 * K + 3) + [1 if has_line else 0],
                   _masked(new, stores) + [s32(0xAAAAAAAA) if x is None else x for x in lines])
    fx = fxw_sets()
    for code, name in enumerate(("FXW_STEP_VV", "FXW_STEP_VG", "FXW_VV_CSQ", "FXW_VV_CONJ", "FXW_VG_MUL", "FXW_VG_FROB", "FXW_VG_FROBC"), 30):
        vg = "_VG" in name
        table = name in ("FXW_STEP_VV", "FXW_STEP_VG")
        regs = 64 * L
        op = o[name] = Op(name, code, (2 if vg else 1) * regs + ((9 if vg else 4) * 64 if table else 0), (2 if vg else 1) * regs, True)
        for tag, V, Gb, rows in fx[name]:
            use = rows if table else FX_TABLES[FX_TABLE_OF[name]]
            new = exec_fxw(V, Gb, use, vg)
            words = _flat(V) + (_flat(Gb) if vg else []) + ([x for row in rows for x in row] if table else [])
            op.add(tag, words, _flat(new) + (_flat(Gb) if vg else []))
    op = o["FXW_TINV"] = Op("FXW_TINV", 37, 64 * L, 64 * L, True)
    for tag, V, _ in tinv_sets():
        op.add(tag, _flat(V), _flat(exec_tinv(V)))
    _OPS = o
    return o


def call_sets(op, n, base=0):
    """the set of every item of a call of n items (base: where a further call of the largest count goes on)"""
    if op.wave:
        return [(base + i) % len(op.sets) for i in range(n)]
    return [(item_set(i, MAX_SETS) + base) % len(op.sets) for i in range(n)]


# ---- the static audit: every record of every table, worst case instead of as seen ------------------------------------------------
def _bounds(kind):
    """(limb lo, limb hi, value lo, value hi) of a slot: 'n' normal, 'm' limb-negated (st14n), 'z' the ZERO slot"""
    if kind == "z":
        return (0, 0, 0, 0)
    if kind == "m":
        return (-MASK, 0, -HI, -LO)
    return (0, MASK, LO, HI)


def _operand(kinds):
    b = [_bounds(k) for k in kinds]
    return tuple(sum(x[i] for x in b) for i in range(4))


def _prod_iv(a, b):
    c = [a[2] * b[2], a[2] * b[3], a[3] * b[2], a[3] * b[3]]
    return min(c), max(c)


def _audit_output(prod_groups, scales, group):
    """prod_groups: per lane of the group, a list of products (operand A, operand B), operands as _operand tuples; scales: the scales
    the group's sum is stored with.  Returns the worst column units (pos, neg), |top x scale|, |carry|, and the stored interval / q"""
    from fractions import Fraction
    res = {"pos": 0, "neg": 0, "top": 0, "carry": 0, "lo": Fraction(0), "hi": Fraction(1)}
    plo = phi = 0                                  # the sum of the group's top limbs
    u = 1 << 56
    for prods in prod_groups:
        pos = neg = tlo = thi = 0
        for a, b in prods:
            ah, al, bh, bl = max(a[1], 0), max(-a[0], 0), max(b[1], 0), max(-b[0], 0)
            pos += max(ah * bh, al * bl)
            neg += max(ah * bl, al * bh)
            lo, hi = _prod_iv(a, b)
            tlo, thi = tlo + lo, thi + hi
        res["pos"], res["neg"] = max(res["pos"], Fraction(pos, u)), max(res["neg"], Fraction(neg, u))
        # the product's result lies in (T / R, T / R + q), its digits normalised: top limb = floor(result / 2^364)
        plo += (tlo // R) >> (W * (L - 1))
        phi += ((-(-thi // R)) + Q) >> (W * (L - 1))
    delta = Fraction(1 << (W * (L - 1))) - Fraction(MW.M47 * Q, 1 << 47)
    low = group << (W * (L - 1))                   # the digits 0 .. 12 of the sum: [0, group x 2^364)
    for s in scales:
        tops = (s * plo, s * phi)
        res["top"] = max(res["top"], abs(tops[0]), abs(tops[1]))
        k = max(abs(t) * MW.M47 >> 47 for t in tops) + 1
        res["carry"] = max(res["carry"], 2 * (abs(s) * group * (MASK + 1) + k * (MASK + 1)))
        for t in tops:
            res["lo"] = min(res["lo"], (t * delta + min(0, s * low)) / Q)
            res["hi"] = max(res["hi"], (t * delta + Q + max(0, s * low)) / Q)
    return res


def _merge(a, b):
    if a is None:
        return b
    return {k: (min if k == "lo" else max)(a[k], b[k]) for k in a}


def audit():
    """{table: worst case over its records}: column units fed to fp28_dotK (8 admitted, 9 on the negative side), |top limb x scale|
    (against 2^31), |carry| (against 2^63), the interval of the stored result in units of q (against (-1/64, 1 + 1/64))"""
    out = {}
    for fam, kinds, names in TABLES:
        zero = {4 * a for a in _zero_quad(names)}
        worst = None
        for step in kinds:
            K, BS, OCT = SHAPES[step_shape(step)]
            grp = 8 if OCT else 4
            rec = gen_mlw.record_words(step)
            cls = lambda a: "z" if a in zero else "n"
            lanes = []
            for w in rec:
                prods = []
                for k in range(K):
                    A = _operand([cls(w[2 * k] & 0xFFFF), cls(w[2 * k] >> 16)])
                    B = _operand([cls(w[2 * k + 1] & 0xFFFF)] + ([] if BS else [cls(w[2 * k + 1] >> 16)]))
                    prods.append((A, B))
                lanes.append(prods)
            for g0 in range(0, LANES, grp):
                scales = {s32(rec[l][4]) >> 16 for l in range(g0, g0 + grp)}
                worst = _merge(worst, _audit_output(lanes[g0:g0 + grp], scales, grp))
        out[fam] = worst
    worst = None
    zslot = LW.SLOT[("ZERO", 1)]
    cls = lambda s: "z" if s == zslot else ("m" if LSLOT_KIND[s] < 0 else "n")
    for kind, recs in enumerate(LW.RECS):
        for r in recs:
            prods = [(_operand([cls(a1), cls(a2)]), _operand([cls(b1), cls(b2)])) for a1, a2, b1, b2 in r.prods]
            worst = _merge(worst, _audit_output([prods], {r.scale} | ({2 * r.scale} if LW.HAS2[kind] else set()), 1))
    out["lsw"] = worst
    return out
