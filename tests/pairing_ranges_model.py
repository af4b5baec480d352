"""The schedule of the ragged multi-pairing (blsgpu_pairing_multi_ranges*) stated on its own, as the specification that
csrc/pairing_ranges_plan.h is held against (tests/test_pairing_ranges_plan_host.py): the validation of the ranges, the slices of
the pair list, the chunks of every range, each slice's chunk table, the fold levels, the buffer sizes and the grids.

The rules, in the order plan() applies them:
  * n > 0x3FFFFFF0 is refused; then the first range with begin > end or end > n; then 2^31 chunks or more.
  * slice s holds the pairs [s S, min(n, (s + 1) S)); a call of no pairs has one slice of none.
  * the pairs of a range that lie in one slice are cut into runs of C from the first of them on; an empty range is one chunk of
    length 0 in the slice of its begin (the last slice when begin == n is a multiple of S).
  * a slice's table lists its chunks range after range, a range's chunks in the order of its pairs.
  * slot j < m is range j's.  A range of one chunk sends it to slot j.  A range of k > 1 chunks takes the next k slots behind
    everything handed out so far (ranges in order), and at every fold level cdiv(k, FAN) more -- or slot j when that is 1.
  * level l lists, range after range, the entries (first source, count <= FAN, destination) of the ranges still folding.
  * the workspace: the partials, then every non-empty slice's table, then every level's, each on a 256-byte boundary.

plan() returns the list of numbers the host test's program prints for the same plan."""
import errno

import pairing_plan_model as P

MAX_PAIRS = 0x3FFFFFF0
MAX_CHUNKS = 1 << 31
OK, TOO_MANY_PAIRS, BAD_RANGE, TOO_MANY_CHUNKS = range(4)
REFUSALS = {OK: (0, ""), TOO_MANY_PAIRS: (-errno.EINVAL, "batch too large"),
            BAD_RANGE: (-errno.EINVAL, "a range with begin > end or end > n"), TOO_MANY_CHUNKS: (-errno.EINVAL, "2^31 chunks or more")}
FAN, TEAMS = P.FAN, P.TEAMS
DEFAULT_CHUNK = 16


def up256(v):
    return (v + 255) // 256 * 256


def pieces(b, e, C, S):
    """the chunks (slice, first pair within it, length) of the range [b, e)"""
    if b == e:
        return None
    out = []
    for s in range(b // S, (e - 1) // S + 1):
        lo, hi = max(b, s * S), min(e, (s + 1) * S)
        out += [(s, q - s * S, min(C, hi - q)) for q in range(lo, hi, C)]
    return out


def count_chunks(b, e, C, S):
    """... their number, without listing them (ranges of 2^20 pairs a thousand times over)"""
    if b == e:
        return 1
    return sum(P.cdiv(min(e, (s + 1) * S) - max(b, s * S), C) for s in range(b // S, (e - 1) // S + 1))


def schedule(n, ranges, C, S, c=None):
    """(refusal, bad range) or the plan as a dict: slices [(lo, pairs, chunks [(first, len, dest)])], levels [[(src, count,
    dest)]], slots"""
    C, S = C or 1, S or 1
    if n > MAX_PAIRS:
        return TOO_MANY_PAIRS, 0
    total = 0
    for j, (b, e) in enumerate(ranges):
        if b > e or e > n:
            return BAD_RANGE, j
        total += count_chunks(b, e, C, S)
        if total >= MAX_CHUNKS:
            return TOO_MANY_CHUNKS, 0
    m = len(ranges)
    ns = P.cdiv(n, S) if n else 1
    slices = [[s * S, min(S, n - s * S), []] for s in range(ns)]
    slots, runs = m, []
    for j, (b, e) in enumerate(ranges):
        ps = pieces(b, e, C, S)
        if ps is None:
            slices[min(b // S, ns - 1)][2].append((0, 0, j))
        elif len(ps) == 1:
            slices[ps[0][0]][2].append((ps[0][1], ps[0][2], j))
        else:
            for i, (s, first, ln) in enumerate(ps):
                slices[s][2].append((first, ln, slots + i))
            runs.append((j, slots, len(ps)))
            slots += len(ps)
    levels = []
    while runs:
        level, nxt = [], []
        for j, base, k in runs:
            ko = P.cdiv(k, FAN)
            if ko == 1:
                level.append((base, k, j))
            else:
                level += [(base + i * FAN, min(FAN, k - i * FAN), slots + i) for i in range(ko)]
                nxt.append((j, slots, ko))
                slots += ko
        levels.append(level)
        runs = nxt
    return dict(n=n, m=m, C=C, S=S, slices=slices, levels=levels, slots=slots, nchunks=total)


def image_sum(tables, o_tables, ws_bytes):
    """sum of (index + 1) * word over the 32-bit words of the table image [o_tables, ws_bytes), mod 2^64"""
    words = [0] * ((ws_bytes - o_tables) // 4)
    for off, rows in tables:
        at = (off - o_tables) // 4
        for r in rows:
            words[at:at + 3] = r
            at += 3
    return sum((i + 1) * w for i, w in enumerate(words)) % (1 << 64)


def plan(n, ranges, C=DEFAULT_CHUNK, S=P.LITERALS[1], max_groups=P.LITERALS[0], c=None):
    """the numbers the host program prints"""
    c = c or P.knobs()
    s = schedule(n, ranges, C, S)
    if isinstance(s, tuple):
        return [s[0], s[1]]
    out = [OK, 0, n, s["m"], s["C"], s["S"], s["nchunks"], s["slots"]]
    off = up256(s["slots"] * 576)
    o_tables = off
    lines = bad = degen = 0
    rows, tables, at = [], [], 0
    for lo, pairs, chunks in s["slices"]:
        chains = int(any(ln for _, ln, _ in chunks))
        tab_off = 0
        if chunks:
            tab_off, off = off, off + up256(12 * len(chunks))
            tables.append((tab_off, chunks))
        row = [lo, pairs, at, len(chunks), chains, P.cdiv(len(chunks), TEAMS), tab_off]
        if chains:
            ls = P.ls(c, 1, pairs, 1, 0)
            row += [ls[9], ls[10], ls[11], ls[4], ls[7], ls[8]]
            lines, bad, degen = max(lines, ls[4]), max(bad, ls[7]), max(degen, ls[8])
        else:
            row += [0] * 6
        rows.append(row)
        at += len(chunks)
    lrows, at = [], 0
    for level in s["levels"]:
        lrows.append([at, len(level), P.cdiv(len(level), TEAMS), off])
        tables.append((off, level))
        off += up256(12 * len(level))
        at += len(level)
    out += [lines, bad, degen, 0, o_tables, off, max_groups or 1, len(rows), len(lrows)]
    for row in rows:
        out += row
    for _, _, chunks in s["slices"]:
        for ch in chunks:
            out += ch
    for row in lrows:
        out += row
    for level in s["levels"]:
        for f in level:
            out += f
    return out + [image_sum(tables, o_tables, off)]


def parse(nums):
    """the printed numbers back into (head dict, slices [(row, chunks)], levels [(row, folds)])"""
    it = iter(nums)
    take = lambda k: [next(it) for _ in range(k)]
    refusal, bad_range = take(2)
    if refusal:
        return dict(refusal=refusal, bad_range=bad_range), [], []
    keys = ["n", "m", "C", "S", "nchunks", "slots", "lines_bytes", "bad_bytes", "degen_bytes", "o_partials", "o_tables", "ws_bytes",
            "final_step", "nslices", "nlevels"]
    head = dict(zip(keys, take(len(keys))), refusal=0)
    srows = [take(13) for _ in range(head["nslices"])]
    slices = [(r, [tuple(take(3)) for _ in range(r[3])]) for r in srows]
    lrows = [take(4) for _ in range(head["nlevels"])]
    levels = [(r, [tuple(take(3)) for _ in range(r[1])]) for r in lrows]
    head["image_sum"] = next(it)
    assert next(it, None) is None
    return head, slices, levels


def check_invariants(nums, ranges):
    """what every plan must satisfy, whatever produced it: every pair of every range in exactly one chunk of that range, no
    chunk across a slice, every range ending in its own slot j alone, every fold entry with 1 <= count <= FAN and reading slots
    that were written before and by nothing else"""
    head, slices, levels = parse(nums)
    assert head["refusal"] == OK
    m, S, C = head["m"], head["S"], head["C"]
    owner = {}                                                # slot -> pairs (absolute) its product covers, as a sorted list
    written = set()
    for row, chunks in slices:
        lo, pairs = row[0], row[1]
        assert row[4] == int(any(ln for _, ln, _ in chunks)) and row[5] == P.cdiv(len(chunks), TEAMS)
        for first, ln, dest in chunks:
            assert ln <= C and first + ln <= pairs and (ln == 0 or first < pairs), "a chunk leaves its slice"
            assert dest not in written and dest < head["slots"]
            written.add(dest)
            owner[dest] = list(range(lo + first, lo + first + ln))
    assert sum(len(ch) for _, ch in slices) == head["nchunks"]
    for row, folds in levels:
        assert row[2] == P.cdiv(len(folds), TEAMS) and folds
        new = {}
        for src, count, dest in folds:
            assert 1 <= count <= FAN
            assert dest not in written and dest not in new and dest < head["slots"]
            got = []
            for q in range(src, src + count):
                assert q >= m and q in owner, "a fold reads a slot nothing wrote (or a result slot)"
                got += owner.pop(q)
            new[dest] = got
        written |= set(new)
        owner.update(new)
    assert sorted(owner) == list(range(m)), "every range ends in its own slot, and nothing else is left over"
    for j, (b, e) in enumerate(ranges):
        assert owner[j] == list(range(b, e)), "range %d" % j
    # the tables do not overlap each other or the partials
    spans = [(0, head["slots"] * 576)] + [(r[6], r[6] + 12 * r[3]) for r, _ in slices if r[3]] + [(r[3], r[3] + 12 * r[1]) for r, _ in levels]
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0 and b0 % 256 == 0
    assert spans[-1][1] <= head["ws_bytes"] and head["o_tables"] == up256(head["slots"] * 576)
