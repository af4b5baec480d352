"""The host side of the point range sums (range_sums_run), the ragged multi-scalar sums (msm_ranges_dev), the short-scalar
multiplications (smul64_launch) and the batched signature division (sig_divide_dev) stated on its own: every slice, grid and
workspace offset of a call.  Written from those functions as they stood BEFORE csrc/ragged_plan.h existed -- each laid out its
buffers inline, two of them with a rounding lambda of their own -- so that the header is held against what the library did, not
against itself (tests/test_ragged_plan_host.py; tests/test_gpu_slices.py holds one total against the device).

A plan is a dict; `sizes` names what each region of a layout must hold, in the layout's own unit (bytes or u32 words)."""
from msm_plan_model import L28_AFF, L28_PJ, LP, PJ, SMUL_T, SRT_LANES, cdiv, grown_bytes, knobs, slice_len  # noqa: F401

PSCAN_CHUNK, PSCAN_MID_THREADS = 16, 128                     # blsgpu_pscan.hip
MSMR_CHUNK, MSMR_SCAN_THREADS = 8, 1024                      # blsgpu_msmr.hip
CONSTS = [PSCAN_CHUNK, PSCAN_MID_THREADS, MSMR_CHUNK, MSMR_SCAN_THREADS]
PSCAN_RECORD_BYTES = (2 << 30) - (1 << 20)
NONE = (1 << 64) - 1


def al(b, unit=256):
    return (b + unit - 1) & ~(unit - 1)


# ---- the refusals
def too_large(n, m, n_ent=0):
    """range_sums_args / msm_ranges_args (n_ent = 0) and sig_divide_args"""
    return n > 0xFFFFFFF0 or n_ent > 0xFFFFFFF0 or m > 0x7FFFFFF0 // LP[2]


def first_bad_range(ranges, n):
    """the loop of range_sums_host / msm_ranges_host"""
    for i, (b, e) in enumerate(ranges):
        if b > e or e > n:
            return i
    return NONE


# ---- range sums
def scan_grids(m):
    """pscan_launch over m points"""
    chunks = cdiv(m, PSCAN_CHUNK) if m else 1
    return dict(chunks=chunks, g_prep=cdiv(m, 256), g_chunks=cdiv(chunks, 64))


SCAN_WS = ("o_prep", "o_live", "o_kind", "o_ct", "o_cb", "o_s", "o_cnt", "o_carry", "o_cc")


def scan_ws(deg, pts):
    """pscan_ws"""
    pj = L28_PJ * deg
    chunks = cdiv(pts, PSCAN_CHUNK) if pts else 1
    sizes = (pts * L28_AFF * deg * 4, pts, pts, chunks * pj * 4, chunks * 4, (pts + 1) * pj * 4, (pts + 1) * 4, pj * 4, 4)
    w, off = {}, 0
    for name, size in zip(SCAN_WS, sizes):
        w[name] = off
        off += al(size)
    w.update(bytes=off, sizes=dict(zip(SCAN_WS, sizes)))
    return w


def scan_plan(c, deg, n, m):
    """range_sums_run"""
    pj = L28_PJ * deg
    SL = slice_len(c, PSCAN_RECORD_BYTES // (pj * 4) - 1)
    S = min(n, SL)
    single = n <= SL
    o_base = 256
    o_basec = o_base + ((0 if single else m * pj * 4 + 255) & ~255)
    p = dict(SL=SL, S=S, single=int(single), ws=scan_ws(deg, S), o_base=o_base, o_basec=o_basec, range_bytes=o_basec + (0 if single else m * 4),
             begin_total=m * pj, g_check=cdiv(m, 256), g_begin=cdiv(m * pj, 256), g_range=cdiv(m * LP[deg], 64))

    def at(lo):                                              # the body of the do-while loop
        ln = min(n - lo, SL)
        hi = lo + ln
        last = hi == n
        return dict(lo=lo, len=ln, hi=hi, first=int(lo == 0), more=int(not last), last=int(last), **scan_grids(ln))
    return dict(p, at=at, step=SL, items=n, nslices=max(cdiv(n, SL), 1))


# ---- ragged multi-scalar sums
def words64(w):
    return (w + 63) & ~63


def msmr_heads(m):
    h_cnt = 64
    h_first = h_cnt + words64(m)
    h_cr = h_first + words64(m + 1)
    return dict(h_cnt=h_cnt, h_first=h_first, h_cr=h_cr, words=h_cr + words64(2 * m), g_count=cdiv(m, 256),
                sizes=dict(h_cnt=m, h_first=m + 1, h_cr=2 * m))


MSMR_BODY = ("o_prep", "o_live", "o_tab", "o_part", "o_bad", "o_bpre", "o_table")


def msmr_body(c, deg, n, m, total):
    if total >= 1 << 31:
        return dict(too_many=1)
    upw, per_unit = 64 // LP[deg], MSMR_CHUNK * SMUL_T * PJ[deg] * 4
    slice_ = (2 << 30) // per_unit // upw * upw
    slice_ = min(slice_, SRT_LANES // LP[deg])
    slice_ = slice_len(c, slice_, upw)
    units0 = cdiv(min(total, slice_), upw) * upw
    sizes = (n * L28_AFF * deg, cdiv(n, 4), 2 * total, total * 24 * deg, total, total + 1, units0 * MSMR_CHUNK * SMUL_T * PJ[deg])
    p, off = dict(too_many=0, total=total, slice=slice_, units0=units0), 0
    for name, size in zip(MSMR_BODY, sizes):
        p[name] = off
        off += words64(size) if name != "o_table" else size
    p.update(words=off, sizes=dict(zip(MSMR_BODY, sizes)), g_fill=cdiv(max(total, m), 256), g_prep=cdiv(n, 256), g_offcurve=cdiv(m, 256))

    def at(lo):                                              # the body of for_slices(total, slice, ...)
        k = min(total - lo, slice_)
        units = cdiv(k, upw) * upw
        return dict(lo=lo, k=k, units=units, tab=p["o_tab"] + 2 * lo, part=p["o_part"] + lo * 24 * deg, bad=p["o_bad"] + lo, g_smul=units * LP[deg] // 64)
    return dict(p, at=at, step=slice_, items=total, nslices=cdiv(total, slice_))


# ---- short public scalars
def smul64(c, deg, n_pts, n, indexed):
    upw = 64 // LP[deg]
    S = slice_len(c, SRT_LANES // LP[deg])
    m0 = min(n, S)
    units0 = cdiv(m0, upw) * upw
    np0 = n_pts if indexed else m0
    sizes = (np0 * L28_AFF * deg, cdiv(np0, 4), units0 * SMUL_T * PJ[deg])
    p, off = dict(S=S, units0=units0, np0=np0), 0
    for name, size in zip(("o_prep", "o_live", "o_tab"), sizes):
        p[name] = off
        off += al(size, 4)
    p.update(words=off, sizes=dict(zip(("o_prep", "o_live", "o_tab"), sizes)), g_prep_all=cdiv(n_pts, 256))

    def at(lo):                                              # the body of for_slices(n, S, ...)
        m = min(n - lo, S)
        units = cdiv(m, upw) * upw
        return dict(lo=lo, m=m, units=units, pts=lo * 24 * deg, w=lo * 8, out=lo * 24 * deg, g_prep=cdiv(m, 256), g_smul=units * LP[deg] // 64)
    return dict(p, at=at, step=S, items=n, nslices=cdiv(n, S))


# ---- signature division
SIGDIV = ("o_mism", "o_zero", "o_nonunit", "o_status", "o_refused", "o_ranges", "o_scalars", "o_work")


def sigdiv(n_pts, m, n_ent):
    sizes = (n_pts, n_pts, n_pts, n_pts, m, 8 * m, 32 * n_pts, 192 * n_pts)
    p, off = {}, 256
    for name, size in zip(SIGDIV, sizes):
        p[name] = off
        off += al(size)
    p.update(bytes=off, memset_bytes=p["o_nonunit"], sizes=dict(zip(SIGDIV, sizes)), g_check=cdiv(max(m, n_pts) + 1, 256), g_cross=cdiv(n_ent, 256),
             g_quot=cdiv(n_pts, 256), g_fold=cdiv(m, 256), g_refuse=cdiv(m, 256))
    return p


# ---- the lines the host program prints (tests/test_ragged_plan_host.py)
def join(name, values):
    return " ".join([name] + [str(int(v)) for v in values])


def shown(p):
    """the slices a line shows: all of up to six, else the first three and the last two"""
    k = p["nslices"]
    return [p["at"](i * p["step"]) for i in (range(k) if k <= 6 else (0, 1, 2, k - 2, k - 1))]


def scan_line(c, deg, n, m):
    p = scan_plan(c, deg, n, m)
    w = [p[x] for x in ("SL", "S", "single")] + [p["ws"][x] for x in SCAN_WS + ("bytes",)]
    w += [p[x] for x in ("o_base", "o_basec", "range_bytes", "begin_total", "g_check", "g_begin", "g_range")]
    w += [p["nslices"]] + [s[x] for s in shown(p) for x in ("lo", "len", "hi", "first", "more", "last", "chunks", "g_prep", "g_chunks")]
    return join("scan", w)


def msmr_lines(c, deg, n, m, total):
    h, p = msmr_heads(m), msmr_body(c, deg, n, m, total)
    heads = join("heads", [h[x] for x in ("h_cnt", "h_first", "h_cr", "words", "g_count")])
    if p["too_many"]:
        return [heads, "body 1"]
    w = [0] + [p[x] for x in ("total", "slice", "units0") + MSMR_BODY + ("words", "g_fill", "g_prep", "g_offcurve")]
    w += [p["nslices"]] + [s[x] for s in shown(p) for x in ("lo", "k", "units", "tab", "part", "bad", "g_smul")]
    return [heads, join("body", w)]


def smul64_line(c, deg, n_pts, n, indexed):
    p = smul64(c, deg, n_pts, n, indexed)
    w = [p[x] for x in ("S", "units0", "np0", "o_prep", "o_live", "o_tab", "words", "g_prep_all")]
    w += [p["nslices"]] + [s[x] for s in shown(p) for x in ("lo", "m", "units", "pts", "w", "out", "g_prep", "g_smul")]
    return join("smul64", w)


def sigdiv_line(n_pts, m, n_ent):
    p = sigdiv(n_pts, m, n_ent)
    return join("sigdiv", [p[x] for x in SIGDIV + ("bytes", "memset_bytes", "g_check", "g_cross", "g_quot", "g_fold", "g_refuse")])
