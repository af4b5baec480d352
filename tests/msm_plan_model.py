"""The host side of a G1 / G2 sum (msm_dev) stated on its own: which kernel family serves a call of `groups` sums of `k` points,
and every number its launches and its two workspace buffers take.  Written from msm_dev as it stood BEFORE csrc/msm_plan.h
existed -- one function body that chose, sized, laid out and launched -- so that the header is held against what the library
did, not against itself (tests/test_msm_plan_host.py; tests/test_gpu_msm_plan.py holds the totals against the device).

msm_dev(knobs, deg, k, groups, scalars) -> "too_large" or a list of (route, plan): the routes in the order they are asked, up to
the first that cannot answer "not me".  A plan is a dict; `words` are the u32 words of B_BUCKETS, `part_words` of B_MSM_PART."""

# the kernel files' constants (blsgpu_msm.hip, vm_tables.h, fp28.h)
NL = 14                                   # 28-bit limbs of an Fq value
L28_AFF, L28_PJ = 2 * NL, 3 * NL
SRT_LANES, SRT_SCW, SRT_BITADDS, SRT_MAXBITS, SRT_SLICE = 2048 * 64, 9, 8, 14, 65536
SMUL_T, PIP_C, PIP_W, PIP_NB = 16, 4, 64, 16
MSM_WAVES, HMSM2_NP = 4, 5
NP = {1: 6, 2: 2}                         # MsmCfg<DEG>::NP
LP = {1: 1, 2: 2}                         # SrtG<DEG>: lanes per unit, words of its affine (x, y, live) and projective point
AFF = {1: 3 * NL, 2: 6 * NL}
PJ = {1: L28_PJ, 2: 2 * L28_PJ}
CONSTS = [SRT_LANES, SRT_SCW, SRT_BITADDS, SRT_MAXBITS, SRT_SLICE, SMUL_T, PIP_W, PIP_NB, L28_AFF, L28_PJ, MSM_WAVES, HMSM2_NP,
          NP[1], NP[2], LP[1], LP[2], AFF[1], AFF[2], PJ[1], PJ[2]]

ROUTES = ("EMPTY", "PLAIN", "SMALL_GROUPS", "SORTED", "BUCKET_VM", "BUCKET_LANE", "VM")
HORNER_WIDE, SRT_FOLD, LANE_FOLD = range(3)                  # the kernel of a fold level
T_QUADS, T_NP, T_PIP = range(3)                              # the tail of a bucket sum

# the knobs, in the order the host test passes them, with the defaults of blsgpu_ctx
KNOBS = dict(pip_threshold=4096, pip_group_threshold=48, pip_chunks=0, msm_sort_threshold=1, msm_sort2_threshold=1, sort_bits=0,
             sort2_bits=0, msm_plain_threshold=2, smul_min_groups=4096, smul_max_k=8, msm_wide_tail=1, msm_lane_threshold=65536,
             msm_lane_pairs=1, horner_np_threshold=1024, horner_quads_threshold=2, test_slice_cap=0)
# the environment variable of each (blsgpu_ctx.h KNOBS)
ENV = dict(pip_threshold="BLSGPU_PIP_THRESHOLD", pip_group_threshold="BLSGPU_PIP_GROUP_THRESHOLD", pip_chunks="BLSGPU_PIP_CHUNKS",
           msm_sort_threshold="BLSGPU_MSM_SORT_THRESHOLD", msm_sort2_threshold="BLSGPU_MSM_SORT2_THRESHOLD", sort_bits="BLSGPU_MSM_SORT_BITS",
           sort2_bits="BLSGPU_MSM_SORT2_BITS", msm_plain_threshold="BLSGPU_MSM_PLAIN_THRESHOLD", smul_min_groups="BLSGPU_SMUL_MIN_GROUPS",
           smul_max_k="BLSGPU_SMUL_MAX_K", msm_wide_tail="BLSGPU_MSM_WIDE_TAIL", msm_lane_threshold="BLSGPU_MSM_LANE_THRESHOLD",
           msm_lane_pairs="BLSGPU_MSM_LANE_PAIRS", horner_np_threshold="BLSGPU_HORNER_NP_THRESHOLD",
           horner_quads_threshold="BLSGPU_HORNER_QUADS_THRESHOLD", test_slice_cap="BLSGPU_TEST_SLICE_CAP")


def knobs(**over):
    assert set(over) <= set(KNOBS)
    return dict(KNOBS, **over)


def cdiv(a, b):
    return -(-a // b)


class Take:
    """consecutive arrays, each rounded up to `unit`"""

    def __init__(self, unit):
        self.unit, self.off = unit, 0

    def __call__(self, count):
        o = self.off
        self.off += cdiv(count, self.unit) * self.unit
        return o


def slice_len(c, natural, unit=1):
    if not c["test_slice_cap"]:
        return natural
    cap = cdiv(c["test_slice_cap"], unit) * unit
    return max(min(natural, cap), unit)


def sort2_bits(n):
    return 13 if n >= 16384 else 11 if n >= 512 else 9


def blocks(nunits, deg):
    return cdiv(nunits * LP[deg], 64)


def fold(kernel, cur, nfold, ftotal, npts, last, grid, src, dst):
    return dict(kernel=kernel, cur=cur, nfold=nfold, ftotal=ftotal, npts=npts, last=last, grid=grid, src=src, dst=dst)


def sorted_plan(c, deg, n):
    pinned = c["sort_bits"] if deg == 1 else c["sort2_bits"]
    if pinned and (pinned < 5 or pinned > SRT_MAXBITS):
        return dict(bad_bits=1)
    cb = pinned if pinned else ((7 if n < 512 else 13) if deg == 1 else sort2_bits(n))
    kb, nwin = cb - 1, (258 + cb - 1) // cb
    nkeys = nwin << kb
    p = dict(bad_bits=0, not_me=0, cb=cb, kb=kb, nwin=nwin, nkeys=nkeys)
    if nwin * n > 0xFFFFFFF0 or n >= 0x80000000:
        return dict(p, not_me=1)
    nch, nsum = (1 << (cb - 2)) // SRT_BITADDS, nwin * cb
    units = SRT_LANES // LP[deg]
    wide = deg == 2 or bool(c["msm_wide_tail"])
    take, pj = Take(4), PJ[deg]
    names = ("o_prep", "o_rec", "o_cnt", "o_start", "o_cur", "o_max", "o_idx", "o_bsum", "o_hp", "o_hk", "o_b0", "o_b1", "o_win", "o_live",
             "o_wtot", "o_long")
    sizes = (n * AFF[deg], n * SRT_SCW, nkeys, nkeys + 1, nkeys, 4, nwin * n, nkeys * pj, units * pj, units, nsum * nch * pj,
             nsum * cdiv(nch, 8) * pj + pj, nwin * pj, cdiv(n, 4), 2 * nwin, nkeys + 4)
    p.update({name: take(size) for name, size in zip(names, sizes)})
    p["sizes"] = dict(zip(names, sizes))
    bias = 0
    for w in range(nwin):
        bias |= 1 << (cb * w + cb - 1)
    p.update(nch=nch, nsum=nsum, units=units, wide=int(wide), words=take.off, btotal=nsum * nch,
             bias=[(bias >> (32 * j)) & 0xFFFFFFFF for j in range(SRT_SCW)], bias_rest=bias >> (32 * SRT_SCW),
             g_prep=cdiv(n, 256), g_slices=cdiv(n, SRT_SLICE), g_accum=blocks(units, deg), g_fix=blocks(nkeys, deg),
             g_bits=blocks(nsum * nch, deg), pass5=0, g_pass5=0, folds=[])
    src, dst = p["o_b0"], p["o_b1"]
    if nch == 1 and not wide:
        p.update(pass5=1, g_pass5=cdiv(nsum, 64))
        src = dst
    cur = nch
    while cur > 1:
        nfold = cdiv(cur, 8)
        ftotal = nsum * nfold
        if wide and ftotal <= 4096 and (cur <= 8 or cur % 8 == 0):
            f = fold(HORNER_WIDE, cur, nfold, ftotal, min(cur, 8), int(nfold == 1), ftotal, src, dst)
        elif wide:
            f = fold(SRT_FOLD, cur, nfold, ftotal, min(cur, 8), int(nfold == 1), blocks(ftotal, deg), src, dst)
        else:
            f = fold(LANE_FOLD, cur, nfold, ftotal, min(cur, 8), int(nfold == 1), cdiv(ftotal, 64), src, dst)
        p["folds"].append(f)
        src, dst = dst, src
        cur = nfold
    p["src"] = src
    return p


def plain_plan(deg, n):
    units_max = SRT_LANES // LP[deg]
    U = min(cdiv(n, 4), units_max)
    chunk = cdiv(n, U)
    U = cdiv(n, chunk)
    take, pj = Take(4), PJ[deg]
    names = ("o_prep", "o_live", "o_b0", "o_b1")
    sizes = (n * L28_AFF * deg, cdiv(n, 4), U * pj, cdiv(U, 8) * pj + pj)
    p = dict(U=U, chunk=chunk)
    p.update({name: take(size) for name, size in zip(names, sizes)})
    p.update(sizes=dict(zip(names, sizes)), words=take.off, g_prep=cdiv(n, 256), g_chunks=blocks(U, deg), folds=[])
    src, dst, cur = p["o_b0"], p["o_b1"], U
    while cur > 8:
        nfold = cdiv(cur, 8)
        if nfold <= 4096 and cur % 8 == 0:
            p["folds"].append(fold(HORNER_WIDE, cur, nfold, nfold, 8, 0, nfold, src, dst))
        else:
            p["folds"].append(fold(SRT_FOLD, cur, nfold, nfold, 8, 0, blocks(nfold, deg), src, dst))
        src, dst = dst, src
        cur = nfold
    p.update(src=src, last_n=cur)
    return p


def small_plan(c, deg, k, groups):
    upw, per_group = 64 // LP[deg], k * SMUL_T * PJ[deg] * 4
    slice_ = (2 << 30) // per_group // upw * upw
    slice_ = max(slice_, upw)
    slice_ = slice_len(c, slice_, upw)
    slice_ = min(slice_, groups)
    units0, n0 = cdiv(slice_, upw) * upw, k * slice_
    take = Take(4)
    names = ("o_prep", "o_live", "o_tab")
    sizes = (n0 * L28_AFF * deg, cdiv(n0, 4), units0 * k * SMUL_T * PJ[deg])
    p = dict(upw=upw, slice=slice_, units0=units0)
    p.update({name: take(size) for name, size in zip(names, sizes)})
    p.update(sizes=dict(zip(names, sizes)), words=take.off, slices=[])
    for lo in range(0, groups, slice_):
        m = min(groups - lo, slice_)
        n, units = k * m, cdiv(m, upw) * upw
        p["slices"].append(dict(lo=lo, m=m, n=n, units=units, pts=lo * k * 24 * deg, scalars=lo * k * 8, out=lo * 24 * deg,
                                g_prep=cdiv(n, 256), g_smul=units * LP[deg] // 64))
    return p


def bucket_plan(c, deg, k, groups):
    n = k * groups
    lane_path = n >= c["msm_lane_threshold"]
    want = c["pip_chunks"] if c["pip_chunks"] else (3072 if lane_path else 256)
    chunk = k if groups > 1 else cdiv(k, want)
    if not lane_path and chunk < 64 * NP[deg] and groups == 1:
        chunk = 64 * NP[deg]
    if not lane_path:
        chunk = cdiv(chunk, NP[deg]) * NP[deg]
    if chunk == 0:
        chunk = 1
    chunks = cdiv(k, chunk)
    fold_n = cdiv(chunks, 64) if (lane_path and chunks > 96) else 0
    pj28 = L28_PJ * deg
    need = (chunks + 1) * groups * PIP_W * pj28 + n * 36 * deg + cdiv(n, 4) + 4
    o_win = chunks * groups * PIP_W * pj28
    o_prep = o_win + groups * PIP_W * pj28
    p = dict(lane_path=int(lane_path), n=n, chunk=chunk, chunks=chunks, fold_n=fold_n, part_words=need, o_win=o_win, o_prep=o_prep,
             o_live=o_prep + n * L28_AFF * deg, words=0, o_fold=0, lanes=0, ftotal=0, wchunks=chunks, pairs=0, lane_last=0, g_lane=0, g_fold=0,
             quad_waves=0)
    quads = False
    if lane_path:
        lanes = groups * chunks * PIP_W
        p["words"] = lanes * (PIP_NB - 1) * pj28 + fold_n * groups * PIP_W * 36 * deg
        quads = deg == 2 and bool(c["msm_lane_pairs"]) and chunks == 1 and groups >= c["horner_quads_threshold"]
        if deg == 2 and c["msm_lane_pairs"]:
            p.update(pairs=1, g_lane=cdiv(2 * lanes, 64), lane_last=0 if (fold_n or quads) else 1)
        else:
            p.update(pairs=0, g_lane=cdiv(lanes, 64), lane_last=0 if fold_n else 1)
        p.update(lanes=lanes, g_prep=cdiv(n, 256), o_fold=lanes * (PIP_NB - 1) * pj28, quad_waves=cdiv(4 * groups, 64))
        if fold_n:
            ftotal = groups * PIP_W * fold_n
            p.update(ftotal=ftotal, g_fold=cdiv(ftotal, 64), wchunks=fold_n)
    else:
        p["g_prep"] = cdiv(n, MSM_WAVES * NP[deg])
    p["tail"] = T_QUADS if quads else T_NP if (deg == 2 and groups >= c["horner_np_threshold"]) else T_PIP
    p["g_np"] = cdiv(groups, HMSM2_NP)
    return p


def vm_plan(deg, k, groups):
    per_pass = MSM_WAVES * NP[deg]
    chunk = k
    if groups < 1024 and k > 4 * per_pass:
        want_blocks = 2048 // groups + 1
        chunk = cdiv(k, want_blocks)
        chunk = cdiv(chunk, per_pass) * per_pass
        chunk = min(chunk, k)
    bpg = cdiv(k, chunk)
    return dict(chunk=chunk, bpg=bpg, blocks=bpg * groups, part_words=bpg * groups * 36 * deg, fblocks=cdiv(groups, MSM_WAVES))


def msm_dev(c, deg, k, groups, scalars):
    """groups >= 1.  The if-chain of msm_dev; a route that can still answer "not me" is followed by the next one."""
    if k == 0:
        return [("EMPTY", {})]
    if k > 0x7FFFFFFF or groups > 0x7FFFFFFF or k * groups > 0xFFFFFFF0:
        return "too_large"
    out = []
    if groups == 1 and not scalars and k >= c["msm_plain_threshold"]:
        return [("PLAIN", plain_plan(deg, k))]
    if scalars and groups >= c["smul_min_groups"] and k <= c["smul_max_k"]:
        out.append(("SMALL_GROUPS", small_plan(c, deg, k, groups)))          # (no room for its tables: the next route)
    if groups == 1 and scalars and k >= (c["msm_sort_threshold"] if deg == 1 else c["msm_sort2_threshold"]):
        p = sorted_plan(c, deg, k)
        out.append(("SORTED", p))
        if p["bad_bits"] or not p["not_me"]:
            return out
    if (groups == 1 and k >= c["pip_threshold"]) or (1 < groups <= 65535 and k >= c["pip_group_threshold"]):
        p = bucket_plan(c, deg, k, groups)
        return out + [("BUCKET_LANE" if p["lane_path"] else "BUCKET_VM", p)]
    return out + [("VM", vm_plan(deg, k, groups))]


def buffer_words(route, p):
    """(words of B_MSM_PART, words of B_BUCKETS) the route asks for"""
    return p.get("part_words", 0), p.get("words", 0)


def grown_bytes(words, held=0):
    """Buf::grow: a buffer that must hold more than it does is replaced by one of bytes + bytes / 4"""
    need = 4 * words
    return held if need <= held else need + need // 4


def group_sums_bytes(routes):
    """what BLSGPU_WS_GROUP_SUMS reports after the routes of one call on a fresh context (both buffers count in whole words)"""
    part = buckets = 0
    for route, p in routes:
        pw, bw = buffer_words(route, p)
        part, buckets = grown_bytes(pw, part), grown_bytes(bw, buckets)
    return part // 4 * 4 + buckets // 4 * 4


# ---- the lines the host program prints (tests/test_msm_plan_host.py)
def fold_words(f):
    return [f[x] for x in ("kernel", "cur", "nfold", "ftotal", "npts", "last", "grid", "src", "dst")]


SORTED_OFFSETS = ("o_prep", "o_rec", "o_cnt", "o_start", "o_cur", "o_max", "o_idx", "o_bsum", "o_hp", "o_hk", "o_b0", "o_b1", "o_win", "o_live",
                  "o_wtot", "o_long", "words")
BUCKET_FIELDS = ("lane_path", "n", "chunk", "chunks", "fold_n", "part_words", "o_win", "o_prep", "o_live", "words", "o_fold", "lanes", "ftotal",
                 "wchunks", "pairs", "lane_last", "tail", "g_prep", "g_lane", "g_fold", "g_np", "quad_waves")


def plan_words(route, p):
    """the numbers of a plan in the order the host program prints them"""
    if route == "EMPTY":
        return []
    if route == "SORTED":
        if p["bad_bits"]:
            return [1]
        head = [0, p["not_me"], p["cb"], p["kb"], p["nwin"], p["nkeys"]]
        if p["not_me"]:
            return head
        w = head + [p[x] for x in ("nch", "nsum", "units", "btotal", "wide", "pass5")] + p["bias"] + [p[x] for x in SORTED_OFFSETS]
        w += [p[x] for x in ("src", "g_prep", "g_slices", "g_accum", "g_fix", "g_bits", "g_pass5")] + [len(p["folds"])]
        return w + [x for f in p["folds"] for x in fold_words(f)]
    if route == "PLAIN":
        w = [p[x] for x in ("U", "chunk", "o_prep", "o_live", "o_b0", "o_b1", "words", "src", "last_n", "g_prep", "g_chunks")] + [len(p["folds"])]
        return w + [x for f in p["folds"] for x in fold_words(f)]
    if route == "SMALL_GROUPS":
        w = [p[x] for x in ("upw", "slice", "units0", "o_prep", "o_live", "o_tab", "words")] + [len(p["slices"])]
        return w + [s[x] for s in p["slices"] for x in ("lo", "m", "n", "units", "pts", "scalars", "out", "g_prep", "g_smul")]
    if route in ("BUCKET_VM", "BUCKET_LANE"):
        return [p[x] for x in BUCKET_FIELDS]
    return [p[x] for x in ("chunk", "bpg", "blocks", "part_words", "fblocks")]


def lines(c, deg, k, groups, scalars):
    r = msm_dev(c, deg, k, groups, scalars)
    if r == "too_large":
        return ["too_large"]
    return [" ".join(map(str, [route] + plan_words(route, p))) for route, p in r] + ["end"]
