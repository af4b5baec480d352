"""Integer model of the ragged multi-scalar sums (csrc/blsgpu_msmr.hip and blsgpu_api.hip msm_ranges_dev): the SPECIFICATION of
the chunk table, of a chunk's digits and window recurrence, of the count of points off the curve and of the per-range
combination.  out_j = sum_{i in [begin_j, end_j)} s_i P_i for ranges of any lengths; points, scalars and ranges are PUBLIC data.

  chunk_counts(ranges, n)   ceil(len / CHUNK) per range after the check begin <= end <= n (k_msmr_count; ValueError where the
                            device returns -EINVAL, also for 2^31 chunks or more in all).
  exclusive_scan(v)         len(v) + 1 prefix sums, the last one the total (k_msmr_scan).
  chunk_table(ranges, n)    -> (first_chunk, table): table[c] = (first point, count), 1 <= count <= CHUNK, the chunks of range j
                            being exactly first_chunk[j] .. first_chunk[j + 1] (k_msmr_fill; an empty range owns none).
  digits(s)                 the 64 plain nibbles of a 256-bit scalar, least significant first, read as the device reads them
                            from the eight big-endian words; the scalar is NOT reduced.
  chunk_sum(F, pts, scalars)   k_smul_seg on one chunk: per point the on-curve test (a point off the curve is counted and
                            enters as infinity) and the table 0 .. 15 P by mixed additions; then from the top window down four
                            doublings (not before the top window) and one complete addition of the digit-selected entry per
                            point.  -> (projective sum, count of points off the curve, operation counts).
  msm_ranges(F, pts, scalars, ranges)   the whole call: chunk table, every chunk's affine partial and count, the prefix sums of
                            both (pscan_model.scan over the partials, exclusive_scan over the counts) and per range ONE
                            difference (pscan_model.range_sum), flag 2 and (0, 0) where the range's chunks counted a point off
                            the curve.  -> [(flag, affine point)].

The curve arithmetic is pscan_model's (complete formulas; both curves have odd order, so P + (-P), P + P and infinity need no
branch); the doubling is the complete addition of a point to itself, which is what a doubling formula computes.
tests/test_msmr_model.py holds all of this against sums by the chord-and-tangent rule on integers."""
from . import pscan_model as P
from . import smul64_model as S64

CHUNK = 8
WINDOWS = 64
TABLE = S64.TABLE


def chunk_counts(ranges, n):
    out = []
    for b, e in ranges:
        if not 0 <= b <= e <= n:
            raise ValueError("begin <= end <= n")
        out.append(-(-(e - b) // CHUNK))
    if sum(out) >= 1 << 31:
        raise ValueError("too many chunks")
    return out


def exclusive_scan(v):
    out = [0]
    for x in v:
        out.append(out[-1] + x)
    return out


def chunk_table(ranges, n):
    first = exclusive_scan(chunk_counts(ranges, n))
    table = []
    for c in range(first[-1]):
        j = max(j for j in range(len(ranges)) if first[j] <= c)          # the LAST range that begins at or before chunk c
        p = ranges[j][0] + (c - first[j]) * CHUNK
        table.append((p, min(CHUNK, ranges[j][1] - p)))
    return first, table


def digits(s):
    """digits d_w in [0, 16), least significant first: window w is nibble w % 8 of big-endian word 7 - w // 8"""
    if not 0 <= s < 1 << 256:
        raise ValueError("scalars are 256-bit")
    words = [int.from_bytes(s.to_bytes(32, "big")[4 * k:4 * k + 4], "big") for k in range(8)]
    return [(words[7 - (w >> 3)] >> (4 * (w & 7))) & 15 for w in range(WINDOWS)]


def chunk_sum(F, pts, scalars):
    if not 1 <= len(pts) <= CHUNK or len(pts) != len(scalars):
        raise ValueError("a chunk holds 1 .. %d points and a scalar each" % CHUNK)
    ops = {"dbl": 0, "add": 0, "table_add": 0}
    tables, bad = [], 0
    for pt in pts:
        kind = P.kind_of(F, pt)
        bad += kind == 2
        m, T = P.inf(F), [P.inf(F)]
        for _ in range(1, TABLE):
            if kind == 1:
                m = P.pmadd(F, m, *pt)
            T.append(m)
        ops["table_add"] += TABLE - 2                        # (T[1] = infinity + P costs nothing)
        tables.append(T)
    d = [digits(s) for s in scalars]
    acc = P.inf(F)
    for w in range(WINDOWS - 1, -1, -1):
        if w != WINDOWS - 1:
            for _ in range(4):
                acc = P.padd(F, acc, acc)
                ops["dbl"] += 1
        for T, dg in zip(tables, d):
            acc = P.padd(F, acc, T[dg[w]])
            ops["add"] += 1
    return acc, bad, ops


def msm_ranges(F, pts, scalars, ranges):
    if len(pts) != len(scalars):
        raise ValueError("a scalar per point")
    first, table = chunk_table(ranges, len(pts))
    partial, bad = [], []
    for p, count in table:
        acc, nb, _ = chunk_sum(F, pts[p:p + count], scalars[p:p + count])
        partial.append(P.affine(F, acc))
        bad.append(nb)
    S, cnt = P.scan(F, partial)
    assert cnt[-1] == 0, "a partial sum is a point of the curve"
    badpre = exclusive_scan(bad)
    out = []
    for j in range(len(ranges)):
        if badpre[first[j + 1]] != badpre[first[j]]:
            out.append((2, (F.zero, F.zero)))
        else:
            out.append(P.range_sum(F, S, cnt, first[j], first[j + 1]))
    return out
