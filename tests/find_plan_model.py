"""The host side of the three forgery finders -- blsgpu_sig_shares_check (sig_shares_dev), blsgpu_verify_find (verify_find_dev) and
blsgpu_verify_find_folded (verify_find_folded_dev) -- stated on its own: the refusals, every slice, workspace offset, round layout
and grid of a call.  Written from those functions as they stood BEFORE csrc/find_plan.h existed -- each added up its bytes per
item by hand beside the layout it had to repeat, and the finders and the share check had a slice rule each -- so that the header,
which derives the sums from its region lists, is held against what the library did, not against itself
(tests/test_find_plan_host.py).

A plan is a dict; `sizes` names what each region of a layout must hold, in bytes."""
from bisect_model import ceil_pow2, layout, pair_ranges
from msm_plan_model import cdiv, knobs, slice_len  # noqa: F401

G1, G2, FQ12, NODE = 96, 192, 576, 8                         # include/blsgpu.h; sizeof(sigsh::Node)
THREADS, G1_Q, G2_Q = 256, 6, 12                             # blsgpu_sigshares.hip, blsgpu_batchfind.hip, blsgpu_pscan.hip


def laid(names, sizes, start):
    offs, end = layout(256, start, sizes)
    return dict(zip(names, offs), bytes=end, sizes=dict(zip(names, sizes)))


# ---- the refusals
def find_too_large(n, n_keys, n_msgs):
    """verify_find_args"""
    return n > 0x7FFFFFF0 or n_keys > 0x7FFFFFFF or n_msgs > (2 << 30) // G2


def shares_too_large(k, groups, n_keys):
    """sig_shares_args"""
    return groups > 0x7FFFFFFF or n_keys > 0x7FFFFFFF or k * groups > 0xFFFFFFF0


# ---- the share check
SHR_WS = ("keyst", "sigst", "h", "hinf", "lam", "r", "w", "pk", "elig", "a", "b")
SHR_ROUND = ("nodes", "ga", "gb", "s", "p", "sinf", "pinf", "g1", "g2", "e", "v")


def plan_shares(c, k, groups, n_keys, scaled):
    """the head of sig_shares_dev"""
    K = ceil_pow2(k)
    keep_per = k * (2 + 3 * 32 + 2 * G1 + G2) + G2 + 1
    round_per = K * (NODE + 3 * G1 + 4 * G2 + FQ12 + 3)
    slice_ = (2 << 30) // max(keep_per, round_per)
    slice_ = max(slice_, 1)
    slice_ = slice_len(c, slice_)
    slice_ = min(slice_, groups)
    n0 = slice_ * k
    sizes = (n_keys, n0, slice_ * G2, slice_, n0 * 32 if scaled else 0, n0 * 32, n0 * 32, n0 * G1, n0, n0 * G2, n0 * G1)
    p = dict(k=k, K=K, keep_per=keep_per, round_per=round_per, slice=slice_, n0=n0, groups=groups, w=laid(SHR_WS, sizes, 256))
    p["at"] = lambda m: dict(n=m * k, g_weights=cdiv(m * k, THREADS))
    return p


def shares_round(nn, ln, k):
    """the head of a round of sig_shares_dev"""
    slots = nn * ln
    sizes = (nn * NODE, slots * G2, slots * G1, nn * G2, nn * G1, nn, nn, nn * 2 * G1, nn * 2 * G2, nn * FQ12, nn)
    gtotal, ptotal = slots * (G1_Q + G2_Q), nn * (2 * G1_Q + 2 * G2_Q)
    return dict(nn=nn, slots=slots, gtotal=gtotal, ptotal=ptotal, lg=ln.bit_length() - 1, g_gather=cdiv(gtotal, THREADS),
                g_pairs=cdiv(ptotal, THREADS), g_verdict=cdiv(nn, THREADS), w=laid(SHR_ROUND, sizes, 0))


# ---- the two finders
FIND_WS = ("keyst", "h", "sigst", "r", "elig", "dense", "a", "b")
FOLD_WS = FIND_WS + ("ad", "bd", "rb", "rmsg")
PLAIN_PART = ("ga", "s", "sinf", "g1", "g2", "e")
FOLD_ROUND = ("tab", "code", "bflag", "b", "sflag", "odd", "v", "s", "g1", "g2", "e")


def find_slice(c, n, keep_per, round_per):
    slice_ = slice_len(c, ((2 << 30) - (1 << 20)) // max(keep_per, round_per))
    return min(slice_, n)


def plan_find(c, n, n_keys, n_msgs, folded):
    """the heads of verify_find_dev and verify_find_folded_dev, find_ws, and what a slice of m items computes"""
    if folded:
        keep_per = 1 + 8 + 1 + 4 + 2 * (G2 + G1) + 8
        slot_per = 8 + 4 + 4 + 1 + 1 + 2 * G1 + G2
        round_per = 3 * slot_per + 4 + 8 + 4 + G2 + 3 + FQ12
    else:
        keep_per = 1 + 8 + 1 + 4 + G2 + G1
        round_per = 4 + 2 * G2 + 1 + 2 * G1 + 2 * G2 + FQ12 + 1
    slice_ = find_slice(c, n, keep_per, round_per)
    rcap = min(slice_, n_msgs) + 1 if folded else 0
    sizes = (n_keys, n_msgs * G2, slice_, slice_ * 8, slice_, slice_ * 4, slice_ * G2, slice_ * G1)
    if folded:
        sizes += (slice_ * G2, slice_ * G1, rcap * 4, rcap * 4)
    p = dict(n=n, keep_per=keep_per, round_per=round_per, slice=slice_, rcap=rcap, w=laid(FOLD_WS if folded else FIND_WS, sizes, 256))
    p["at"] = lambda m: dict(m=m, rn=min(m, n_msgs) + 1 if folded else 0, ltotal=m * 18, g_settle=cdiv(m, THREADS), g_leaves=cdiv(m * 18, THREADS))
    return p


def plain_parts(nodes, L, n_e):
    """bisect::plain_round: -> the nodes in the round's order, [(nodes, len)] * 2"""
    full, short = [o for o in nodes if o + L <= n_e], [o for o in nodes if o + L > n_e]
    assert len(short) <= 1
    return full + short, [(len(full), L), (len(short), n_e - short[0] if short else 0)]


def plain_round(parts):
    """the head of a round of verify_find_dev"""
    nn = parts[0][0] + parts[1][0]
    sizes, out, first = [nn * 4, nn], [], 0
    for nodes, ln in parts:
        sizes += [nodes * ln * G2, nodes * G2, nodes, nodes * (ln + 1) * G1, nodes * (ln + 1) * G2, nodes * FQ12]
        gtotal, ptotal = nodes * ln * G2_Q, nodes * (ln + 1) * (G1_Q + G2_Q)
        out.append(dict(nodes=nodes, len=ln, first=first, gsz=ln + 1, pairs=nodes * (ln + 1), gtotal=gtotal, ptotal=ptotal,
                        g_gather=cdiv(gtotal, THREADS), g_pairs=cdiv(ptotal, THREADS), g_verdict=cdiv(nodes, THREADS)))
        first += nodes
    names = ("off", "v") + tuple("%s%d" % (x, i) for i in (0, 1) for x in PLAIN_PART)
    w = laid(names, sizes, 0)
    for i, p in enumerate(out):
        p["w"] = {x: w["%s%d" % (x, i)] for x in PLAIN_PART}
    return dict(nn=nn, bytes=w["bytes"], w=w, names=names, part=out)


def fold_shape(msgs, nodes, L):
    """bisect::fold_round on the leaves' messages: -> nn, slots, nb, the words of the table"""
    n_e = len(msgs)
    cnts = [1 + len(pair_ranges(msgs, o, min(o + L, n_e))) for o in nodes]
    nn, slots = len(nodes), sum(cnts)
    nb = slots - nn
    return nn, slots, nb, layout(64, 0, [nn + 1, nn, 2 * nn, slots, slots, 2 * nb])[1]


def folded_round(nn, slots, nb, tab_words):
    """the head of a round of verify_find_folded_dev"""
    sizes = (tab_words * 4, slots, nb, nb * G1, nn, nn, nn, nn * G2, slots * G1, slots * G2, nn * FQ12)
    ftotal = slots * 18
    return dict(nn=nn, slots=slots, nb=nb, ftotal=ftotal, g_codes=cdiv(nn, THREADS), g_fill=cdiv(ftotal, THREADS), g_verdict=cdiv(nn, THREADS),
                w=laid(FOLD_ROUND, sizes, 0))


# ---- the lines the host program prints (tests/test_find_plan_host.py)
def join(name, values):
    return " ".join([name] + [str(int(v)) for v in values])


def last_len(items, step):
    """the length of the last slice of for_slices(items, step, ...); 0 when there is none"""
    return items - (cdiv(items, step) - 1) * step if items and step else 0


def shares_line(c, k, groups, n_keys, scaled):
    p = plan_shares(c, k, groups, n_keys, scaled)
    v = [p[x] for x in ("K", "keep_per", "round_per", "slice", "n0")] + [p["w"][x] for x in SHR_WS + ("bytes",)]
    for m in (p["slice"], last_len(groups, p["slice"])):
        v += [p["at"](m)[x] for x in ("n", "g_weights")]
    return join("shares", v)


def find_line(c, n, n_keys, n_msgs, folded):
    p = plan_find(c, n, n_keys, n_msgs, folded)
    v = [p[x] for x in ("keep_per", "round_per", "slice", "rcap")] + [p["w"][x] for x in (FOLD_WS if folded else FIND_WS) + ("bytes",)]
    for m in (p["slice"], last_len(n, p["slice"])):
        v += [p["at"](m)[x] for x in ("m", "rn", "ltotal", "g_settle", "g_leaves")]
    return join("find", v)


def shround_line(nn, ln, k):
    r = shares_round(nn, ln, k)
    return join("shround", [r[x] for x in ("nn", "slots", "gtotal", "ptotal", "lg", "g_gather", "g_pairs", "g_verdict")] +
                [r["w"][x] for x in SHR_ROUND + ("bytes",)])


def plainr_line(n_e, L, nodes):
    order, parts = plain_parts(nodes, L, n_e)
    r = plain_round(parts)
    v = list(order) + [r["nn"], r["bytes"], r["w"]["off"], r["w"]["v"]]
    for p in r["part"]:
        v += [p[x] for x in ("nodes", "len", "first", "gsz", "pairs", "gtotal", "ptotal", "g_gather", "g_pairs", "g_verdict")] + [p["w"][x] for x in PLAIN_PART]
    return join("plainr", v)


def foldr_line(msgs, L, nodes):
    r = folded_round(*fold_shape(msgs, nodes, L))
    return join("foldr", [r[x] for x in ("nn", "slots", "nb", "ftotal", "g_codes", "g_fill", "g_verdict")] + [r["w"][x] for x in FOLD_ROUND + ("bytes",)])
