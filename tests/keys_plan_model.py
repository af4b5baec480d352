"""Python model of csrc/keys_plan.h: the refusals, slice lengths, grids and workspaces of the calls that handle key material, stated
the way blsgpu_api.hip computed them before the header existed (sums written out, not a layout helper).
tests/test_keys_plan_host.py holds the header, compiled for the host, against it; tests/test_gpu_slices.py takes the bounds of
its two workspace tests from here."""

FIX_SLICE, FIX_HOST_SLICE, SEED_SLICE, STAGE_TARGET = 1 << 22, 1 << 18, 1 << 20, 1 << 26
SMUL_SLICE, SMUL_PAIRS, TABLE_DW = 65536, 128, 672
SUM_THREADS, EVAL_THREADS, ENTRY_DW, PARENT_DW, MAX_K, PARENT_BYTES = 256, 256, 28, 40, 1024, 160
SEED_MAX_BYTES = 1024
G1, G2, FR = 96, 192, 32
SIZE_MAX = (1 << 64) - 1


def up(v, unit=256):
    return (v + unit - 1) // unit * unit


def blocks(items, threads=256):
    return -(-items // threads)


def slice_len(cap, natural):
    """msm::slice_len with unit 1: the natural length unless the test hook caps it, then never less than one"""
    return natural if not cap else max(1, min(natural, cap))


def run_len(n, step, lo):
    return min(n - lo, step)


def runs(n, step):
    """[(lo, m)] of for_slices(n, step)"""
    return [(lo, run_len(n, step, lo)) for lo in range(0, n, step)] if n else []


# ---- grids
def eval_bpp(n_x):
    return blocks(n_x, EVAL_THREADS)


def lagrange_shape(k):
    """-> (threads, groups per workgroup, LDS bytes)"""
    threads = 256 if k <= 256 else up(k, 64)
    gpb = 256 // k if k <= 256 else 1
    return threads, gpb, (gpb * k + gpb) * 32 + gpb * 4


def sum_shape(k):
    per = min(k, SUM_THREADS)
    return per, SUM_THREADS // per


# ---- refusals
def bad_k(k):
    return k == 0 or k > MAX_K


def too_many_lanes(n):
    return n > 0xFFFFFFFF


def hd_paths_too_large(n, n_parents):
    return n > 0xFFFFFFFF or n_parents > 0xFFFFFFFF


def poly_too_many(n_polys, t):
    return n_polys > 0x7FFFFFFF // t


def lagrange_too_large(k, groups):
    return groups > 0x7FFFFFFF or k * groups > 0xFFFFFFF0


def fr_sum_too_large(k, groups):
    return groups > 0x7FFFFFFF or k > (SIZE_MAX >> 6) // groups


def deal_too_large(n_polys, t, n_x, frag):
    return n_polys > 0x7FFFFFFF or n_x > 0xFFFFFF00 or bool(frag and n_polys * eval_bpp(n_x) > 0x7FFFFFFF) or n_polys * t > 0xFFFFFFF0


def g2_smul_too_large(n):
    return n > 0xFFFFFFF0


# ---- slices
def staged_slice(cap, n, natural):
    return min(n, slice_len(cap, natural))


def staged_fit(cap, n, item_bytes):
    fit = slice_len(cap, STAGE_TARGET // item_bytes)
    return n if n < fit else max(fit, 1)


def deal_item_bytes(t, n_x, frag):
    return t * (32 + 96) + (n_x * 32 if frag else 0)


def fr_sum_item_bytes(k):
    return k * 32 + 176


def seeds_item_bytes(seed_len):
    return seed_len + 368


def fix_at(n, step, lo):
    m = run_len(n, step, lo)
    return dict(m=m, scalars=lo * 8, add=lo * 24, aff=lo * 24, ser=lo * 12, grid=blocks(m))


# ---- the plans: dicts of the header's fields; "regions": (name, bytes) in the order of the layout
def plan_children(cap, n, pub):
    slice_ = staged_slice(cap, n, FIX_HOST_SLICE) if pub else 0
    step = slice_ if pub else slice_len(cap, FIX_SLICE)

    def at(lo):
        m = run_len(n, step, lo)
        return dict(m=m, idx=lo, chain=lo * 8, sk=lo * 8, aff=lo * 96, ser=lo * 48, grid=blocks(m))
    return dict(n=n, step=step, o_parent=0, o_flag=128, o_ileft=256, bytes=256 + slice_ * 32, at=at,
                regions=[("o_parent", 96), ("o_flag", 4), ("o_ileft", slice_ * 32)])


def plan_paths(cap, n, depth, priv):
    S = staged_slice(cap, n, FIX_HOST_SLICE)
    chain = 256
    scal = chain + S * 32
    aff0 = scal + S * 32
    aff1 = aff0 + S * 96
    total = 256 + S * (160 if priv else 256)

    def at(lo):
        m = run_len(n, S, lo)
        return dict(m=m, parent_of=lo, idx=lo * depth, chain=lo * 8, sk=lo * 8, aff=lo * 96, ser=lo * 48, fp=lo, grid=blocks(m))
    return dict(n=n, depth=depth, S=S, o_flag=0, o_chain=chain, o_scal=scal, o_aff0=aff0, o_aff1=aff1, bytes=total, at=at,
                regions=[("o_flag", 4), ("o_chain", S * 32), ("o_scal", S * 32), ("o_aff0", S * 96), ("o_aff1", 0 if priv else S * 96)])


def plan_seeds(cap, seed_len, n, out_sk, out_aff, out_parents):
    S = staged_slice(cap, n, SEED_SLICE)
    ws_sk = 0 if out_sk else S * 32
    ws_aff = S * 96 if out_parents and not out_aff else 0

    def at(lo):
        m = run_len(n, S, lo)
        return dict(m=m, seeds=lo * seed_len, sk=lo * 8, chain=lo * 8, par=lo * PARENT_DW, aff=lo * 24, ser=lo * 48, grid=blocks(m),
                    g_pack=blocks(m * 24))
    return dict(n=n, S=S, o_sk=0, o_aff=ws_sk, bytes=ws_sk + ws_aff, at=at, regions=[("o_sk", ws_sk), ("o_aff", ws_aff)])


def plan_poly(n_polys, t):
    m, mk = n_polys * t, n_polys * (t - 1)
    l28 = 256 + up(n_polys * 4)
    return dict(m=m, mk=mk, o_flag=0, o_sub=256, o_l28=l28, bytes=l28 + m * ENTRY_DW * 4, sub_bytes=n_polys * 4, g_prep=blocks(m), g_sub=blocks(mk),
                regions=[("o_flag", 4), ("o_sub", n_polys * 4), ("o_l28", m * ENTRY_DW * 4)])


def coeff_bytes(k, groups):
    return groups * k * 32


def smul_at(n, step, lo):
    m = run_len(n, step, lo)
    return dict(m=m, pts=lo * 48, scalars=lo * 8, aff=lo * 48, ser=lo * 24, inf=lo, grid=blocks(m, SMUL_PAIRS))


def smul_held(cap, shared, n):
    return 1 if shared else staged_slice(cap, n, SMUL_SLICE)


def smul_table_bytes(held):
    return held * TABLE_DW * 4


def plan_sign(cap, n_msg, n):
    shared = n_msg == 1
    held = smul_held(cap, shared, n)
    step = n if shared else held
    pts_bytes = up(held * 192)

    def at(lo):
        m = run_len(n, step, lo)
        return dict(m=m, msgs=1 if shared else m, hashes=0 if shared else lo * 32, sks=lo * 32, aff=lo * 192, ser=lo * 96)
    return dict(n=n, held=held, step=step, shared=shared, o_pts=0, o_table=pts_bytes, bytes=pts_bytes + held * TABLE_DW * 4, at=at,
                regions=[("o_pts", held * 192), ("o_table", held * TABLE_DW * 4)])


def plan_threshold(cap, k, groups, n_msg):
    n, shared = k * groups, n_msg == 1
    held = smul_held(cap, shared, n)
    sc_bytes, hm_bytes = up(n * 32), up(n_msg * 192)
    rep = 0 if shared else held * 192

    def at(lo):
        m = run_len(n, held, lo)
        return dict(m=m, sc=lo * 32, aff=lo * 192, ser=lo * 96, inf=lo, g_spread=blocks(m * 48))
    return dict(n=n, held=held, shared=shared, lagr_bytes=n * 32, o_sc=0, o_rep=sc_bytes, frs_bytes=sc_bytes + rep, o_hm=0, o_table=hm_bytes,
                smul_bytes=hm_bytes + held * TABLE_DW * 4, g_scale=blocks(n), at=at,
                frs_regions=[("o_sc", n * 32), ("o_rep", rep)], smul_regions=[("o_hm", n_msg * 192), ("o_table", held * TABLE_DW * 4)])


# ---- what the program of tests/test_keys_plan_host.py prints for a case: the kind, then the numbers
def join(kind, values):
    return kind + "".join(" %d" % int(v) for v in values)


def _ats(at, n, step, names):
    """a sliced plan prints its first and its last slice"""
    out = []
    for lo in ((0, (n - 1) // step * step) if n and step else ()):
        a = at(lo)
        out += [a[x] for x in names]
    return out


def line(case):
    kind, a = case[0], case[1:]
    if kind == "large":
        f = {"k": bad_k, "lanes": too_many_lanes, "paths": hd_paths_too_large, "poly": poly_too_many, "lagrange": lagrange_too_large, "frsum": fr_sum_too_large,
             "deal": deal_too_large, "smul": g2_smul_too_large}[a[0]]
        return join("large", [f(*a[1:])])
    if kind == "staged":
        return join(kind, [staged_slice(*a)])
    if kind == "fit":
        cap, n, which = a[:3]
        item = {"deal": deal_item_bytes, "frsum": fr_sum_item_bytes, "seeds": seeds_item_bytes}[which](*a[3:])
        return join(kind, [item, staged_fit(cap, n, item)])
    if kind == "lagr":
        k, groups = a
        threads, gpb, lds = lagrange_shape(k)
        return join(kind, [threads, gpb, lds, blocks(groups, gpb), coeff_bytes(k, groups)])
    if kind == "sum":
        k, groups = a
        per, gpb = sum_shape(k)
        return join(kind, [per, gpb, blocks(groups, gpb)])
    if kind == "eval":
        n_polys, n_x = a
        return join(kind, [eval_bpp(n_x), n_polys * eval_bpp(n_x)])
    if kind == "fix":
        cap, n = a
        step = slice_len(cap, FIX_SLICE)
        at = lambda lo: fix_at(n, step, lo)
        return join(kind, [step] + _ats(at, n, step, ("m", "scalars", "add", "aff", "ser", "grid")))
    if kind == "children":
        p = plan_children(*a)
        return join(kind, [p[x] for x in ("step", "o_parent", "o_flag", "o_ileft", "bytes")] +
                    _ats(p["at"], p["n"], p["step"], ("m", "idx", "chain", "sk", "aff", "ser", "grid")))
    if kind == "paths":
        p = plan_paths(*a)
        return join(kind, [p[x] for x in ("S", "o_flag", "o_chain", "o_scal", "o_aff0", "o_aff1", "bytes")] +
                    _ats(p["at"], p["n"], p["S"], ("m", "parent_of", "idx", "chain", "sk", "aff", "ser", "fp", "grid")))
    if kind == "seeds":
        p = plan_seeds(*a)
        return join(kind, [p[x] for x in ("S", "o_sk", "o_aff", "bytes")] +
                    _ats(p["at"], p["n"], p["S"], ("m", "seeds", "sk", "chain", "par", "aff", "ser", "grid", "g_pack")))
    if kind == "poly":
        p = plan_poly(*a)
        return join(kind, [p[x] for x in ("m", "mk", "o_flag", "o_sub", "o_l28", "bytes", "sub_bytes", "g_prep", "g_sub")])
    if kind == "smul":
        cap, shared, n = a
        step = slice_len(cap, SMUL_SLICE)
        held = smul_held(cap, shared, n)
        at = lambda lo: smul_at(n, step, lo)
        return join(kind, [step, held, smul_table_bytes(held)] + _ats(at, n, step, ("m", "pts", "scalars", "aff", "ser", "inf", "grid")))
    if kind == "sign":
        p = plan_sign(*a)
        return join(kind, [p[x] for x in ("held", "step", "shared", "o_pts", "o_table", "bytes")] +
                    _ats(p["at"], p["n"], p["step"], ("m", "msgs", "hashes", "sks", "aff", "ser")))
    if kind == "threshold":
        p = plan_threshold(*a)
        return join(kind, [p[x] for x in ("n", "held", "shared", "lagr_bytes", "o_sc", "o_rep", "frs_bytes", "o_hm", "o_table", "smul_bytes", "g_scale")] +
                    _ats(p["at"], p["n"], p["held"], ("m", "sc", "aff", "ser", "inf", "g_spread")))
    raise ValueError(kind)
