"""The schedule of blsgpu_verify_aggregates* stated on its own, as the specification that csrc/verify_agg_plan.h is held against
(tests/test_verify_agg_plan_host.py): the validation of the three tables, the key ranges of the sums, the pair slots, the cut
into slices, each slice's range table and source table, the workspace and the grids.

The rules, in the order plan() applies them:
  * sizes first (nothing of a table is read): m or n_grp > 0x3FFFFFF0, m + n_grp > 0x3FFFFFF0, n_msgs > 0x03FFFFF0,
    n_keys > 0xFFFFFFF0 or n_grp > 0x7FFFFFF0 / 2 are "batch too large".
  * then the first g with grp_off[g] > grp_off[g + 1]; grp_off[n_grp] != n_keys; the first j with agg_off[j] > agg_off[j + 1];
    agg_off[m] != n_grp; the first g with grp_msg[g] >= n_msgs.  Each names its entry.
  * group g's key range is (grp_off[g], grp_off[g + 1]).
  * slot(j) = agg_off[j] - agg_off[0] + j; aggregate j's slots are [slot(j), slot(j + 1)): the signature's, then its groups'.
  * a slot's source is (SIG, j, j) or (g, grp_msg[g], j).
  * a slice takes aggregates while its pairs stay within the cap; the first aggregate of a slice is always taken.
  * a slice's range table is (slot(j) - slot0, slot(j + 1) - slot0) per aggregate, and its multi-pairing is
    pairing_ranges_model's plan of those ranges with the same cap.
  * the workspace, every array on a 256-byte boundary: sums (96 n_grp), flags (n_grp), hashed points (192 n_msgs), undecided
    bytes (m), g1 / g2 of the longest slice, results of the slice with most aggregates (576 each); then the tables: -G1 (96), the
    key ranges (8 n_grp), and per slice its sources (12 per slot) and the image of its multi-pairing's tables.

plan() returns the list of numbers the host test's program prints for the same plan."""
import errno

import pairing_ranges_model as R

SIG = 0xFFFFFFFF
MAX_MSGS = 0x03FFFFF0
MAX_AGGS = 0x3FFFFFF0
OK, TOO_LARGE, GRP_OFF_DOWN, GRP_OFF_END, AGG_OFF_DOWN, AGG_OFF_END, BAD_MSG = range(7)
TEXTS = ["", "batch too large", "grp_off steps down", "grp_off does not end at n_keys", "agg_off steps down",
         "agg_off does not end at n_grp", "grp_msg out of range"]
REFUSALS = {r: (0 if r == OK else -errno.EINVAL, TEXTS[r]) for r in range(7)}
PIECES, THREADS = 18, 256
NEG_G1 = list(range(1, 25))                                   # the 24 words the host program hands to fill_tables


def up256(v):
    return (v + 255) // 256 * 256


def validate(grp_off, grp_msg, agg_off, m, n_grp, n_keys, n_msgs):
    """(refusal, first offending entry)"""
    if (m > MAX_AGGS or n_grp > MAX_AGGS or m + n_grp > R.MAX_PAIRS or n_msgs > MAX_MSGS or n_keys > 0xFFFFFFF0
            or n_grp > 0x7FFFFFF0 // 2):
        return TOO_LARGE, 0
    for g in range(n_grp):
        if grp_off[g] > grp_off[g + 1]:
            return GRP_OFF_DOWN, g
    if grp_off[n_grp] != n_keys:
        return GRP_OFF_END, n_grp
    for j in range(m):
        if agg_off[j] > agg_off[j + 1]:
            return AGG_OFF_DOWN, j
    if agg_off[m] != n_grp:
        return AGG_OFF_END, m
    for g in range(n_grp):
        if grp_msg[g] >= n_msgs:
            return BAD_MSG, g
    return OK, 0


def slots(agg_off):
    return [a - agg_off[0] + j for j, a in enumerate(agg_off)]


def sources(grp_msg, agg_off):
    out = []
    for j in range(len(agg_off) - 1):
        out.append((SIG, j, j))
        out += [(g, grp_msg[g], j) for g in range(agg_off[j], agg_off[j + 1])]
    return out


def slices(agg_off, cap):
    """[(agg0, aggs, slot0, pairs)]"""
    sl, m, out, j = slots(agg_off), len(agg_off) - 1, [], 0
    while j < m:
        a0 = j
        j += 1
        while j < m and sl[j + 1] - sl[a0] <= cap:
            j += 1
        out.append((a0, j - a0, sl[a0], sl[j] - sl[a0]))
    return out


def plan(grp_off, grp_msg, agg_off, n_keys, n_msgs, cap=1 << 20, max_groups=32768, m=None, n_grp=None):
    """the numbers the host program prints"""
    m = len(agg_off) - 1 if m is None else m
    n_grp = len(grp_msg) if n_grp is None else n_grp
    refusal, bad = validate(grp_off, grp_msg, agg_off, m, n_grp, n_keys, n_msgs)
    if refusal:
        return [refusal, bad]
    cap = cap or 1
    sl, src = slots(agg_off), sources(grp_msg, agg_off)
    rows, lines, badb, degen, pairr, max_pairs, max_aggs = [], 0, 0, 0, 0, 0, 0
    for a0, aggs, s0, pairs in slices(agg_off, cap):
        ranges = [(sl[j] - s0, sl[j + 1] - s0) for j in range(a0, a0 + aggs)]
        pr = R.plan(pairs, ranges, R.DEFAULT_CHUNK, cap, max_groups)
        assert pr[0] == R.OK
        lines, badb, degen, pairr = max(lines, pr[8]), max(badb, pr[9]), max(degen, pr[10]), max(pairr, pr[13])
        max_pairs, max_aggs = max(max_pairs, pairs), max(max_aggs, aggs)
        rows.append([a0, aggs, s0, pairs, ranges, pr])
    off = 0
    offs = []
    for size in (96 * n_grp, n_grp, 192 * n_msgs, m, 96 * max_pairs, 192 * max_pairs, 576 * max_aggs):
        offs.append(off)
        off += up256(size)
    o_tables = off
    o_neg, off = off, off + up256(96)
    o_kr, off = off, off + up256(8 * n_grp)
    words = {}                                                # word index within the image -> value, the multi-pairings' left zero
    for i, w in enumerate(NEG_G1):
        words[(o_neg - o_tables) // 4 + i] = w
    for g in range(n_grp):
        words[(o_kr - o_tables) // 4 + 2 * g], words[(o_kr - o_tables) // 4 + 2 * g + 1] = grp_off[g], grp_off[g + 1]
    out_rows = []
    for a0, aggs, s0, pairs, ranges, pr in rows:
        src_off, off = off, off + up256(12 * pairs)
        prtab_off, off = off, off + up256(pr[13] - pr[12])
        for i, e in enumerate(src[s0:s0 + pairs]):
            for k in range(3):
                words[(src_off - o_tables) // 4 + 3 * i + k] = e[k]
        out_rows.append([a0, aggs, s0, pairs, src_off, prtab_off, -(-pairs * PIECES // THREADS), -(-aggs // THREADS), pr[12], pr[13], pr[6],
                         pr[7], pr[-1]] + [v for r in ranges for v in r])
    image_sum = sum((i + 1) * w for i, w in words.items()) % (1 << 64)
    out = [OK, 0, m, n_grp, n_keys, n_msgs, sl[m], cap, max_pairs, max_aggs, lines, badb, degen, pairr] + offs + [o_tables, o_neg, o_kr, off,
                                                                                                                len(out_rows)]
    out += [v for g in range(n_grp) for v in (grp_off[g], grp_off[g + 1])]
    out += [v for e in src for v in e]
    for row in out_rows:
        out += row
    return out + [image_sum]


def check_invariants(nums, grp_msg, agg_off):
    """what every plan must satisfy, whatever produced it: every aggregate in exactly one slice, its slots consecutive, the
    first the signature's and the others its groups' in order; no slice past the cap unless it is one aggregate; the arrays of
    the workspace apart"""
    it = iter(nums)
    take = lambda k: [next(it) for _ in range(k)]
    refusal, _ = take(2)
    assert refusal == OK
    m, n_grp, n_keys, n_msgs, pairs, cap, max_pairs, max_aggs = take(8)
    take(4)
    offs = take(11)
    ws_bytes, nslices = offs[-1], next(it)
    take(2 * n_grp)
    src = [tuple(take(3)) for _ in range(pairs)]
    assert pairs == m + agg_off[m] - agg_off[0]
    at_agg, at_slot, ends = 0, 0, []
    for _ in range(nslices):
        a0, aggs, s0, sp, src_off, prtab_off, g_pairs, g_status, pr_ot, pr_ws = take(10)
        take(3)
        ranges = [tuple(take(2)) for _ in range(aggs)]
        assert (a0, s0) == (at_agg, at_slot) and aggs >= 1 and (sp <= cap or aggs == 1) and sp <= max_pairs and aggs <= max_aggs
        assert g_pairs * THREADS >= sp * PIECES > (g_pairs - 1) * THREADS and g_status * THREADS >= aggs
        at = 0
        for i, (b, e) in enumerate(ranges):
            j = a0 + i
            assert b == at and e - b == 1 + agg_off[j + 1] - agg_off[j]
            assert src[s0 + b] == (SIG, j, j)
            assert src[s0 + b + 1:s0 + e] == [(g, grp_msg[g], j) for g in range(agg_off[j], agg_off[j + 1])]
            at = e
        assert at == sp
        at_agg, at_slot = a0 + aggs, s0 + sp
        ends += [(src_off, src_off + 12 * sp), (prtab_off, prtab_off + pr_ws - pr_ot)]
    assert (at_agg, at_slot) == (m, pairs)
    sizes = [96 * n_grp, n_grp, 192 * n_msgs, m, 96 * max_pairs, 192 * max_pairs, 576 * max_aggs, 0, 96, 8 * n_grp]
    spans = [(o, o + s) for o, s in zip(offs[:7] + offs[7:10], sizes) if s] + ends
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0 and b0 % 256 == 0
    assert spans[-1][1] <= ws_bytes
    assert next(it) is not None and next(it, None) is None
