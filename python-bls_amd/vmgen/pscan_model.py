"""Integer model of the point prefix sums and range sums (csrc/blsgpu_pscan.hip): the SPECIFICATION of its three passes and of
the range difference, on Python integers with the complete formulas of Renes-Costello-Batina for a = 0 (algorithms 7 and 8,
the ones fp28.h's padd and pmadd compute).

  FQ, FQ2        the two coordinate fields (an element of Fq2 is a pair (a, b) = a + b u, u^2 = -1) with the curve's 3 b:
                 12 on G1, 12 (1 + u) on the twist.
  padd, pmadd    complete addition of two projective points, complete mixed addition of an affine point; INF = (0 : 1 : 0).
  scan           the three passes over n affine points ((0, 0) = infinity): chunk totals and counts of points off the curve
                 (k_pscan_totals), their exclusive scan by MID_THREADS lanes -- lane sums, Kogge-Stone over the lanes, replay
                 (k_pscan_mid) --, and the replay of every chunk from its carry-in (k_pscan_replay).  -> (S, cnt): n + 1
                 projective prefixes S[j] = sum_{i<j} P_i and n + 1 counts.  A point off the curve is counted and adds nothing.
  scan_slices,   the same for more points than one slice of records holds: every slice's middle scan starts from the last
  range_sum_slices   record of the slice before, the record at a range's begin is kept from its slice and the range is finished
                 in the slice that holds its end (k_pscan_begin, and k_pscan_range with base / basec).
  range_sum      S[end] + (-S[begin]) by ONE complete addition -> (flag, affine point): flag 0 finite, 1 infinity, 2 when the
                 counts differ (the output is (0, 0)), as k_pscan_range.

Why no case analysis: the formulas are complete on a curve without a point of order two, and both E(Fq) and E'(Fq2) have ODD
order -- #E = H1 R and #E' = H2 R, the cofactors odd because the curve parameter Z is even.  ORDER_G1 and ORDER_G2 are computed
from Z below and asserted odd (and the trace relation that ties H1 R to q is asserted too).  So P + (-P), P + P and infinity
on either side need no branch, for every point of either curve and not only for the subgroups.
tests/test_pscan_model.py holds scan and range_sum against sums by the chord-and-tangent rule."""
Q = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
Z = -0xd201000000010000
R = Z ** 4 - Z ** 2 + 1
H1 = (Z - 1) ** 2 // 3
H2 = (Z ** 8 - 4 * Z ** 7 + 5 * Z ** 6 - 4 * Z ** 4 + 6 * Z ** 3 - 4 * Z ** 2 - 4 * Z + 13) // 9
ORDER_G1 = H1 * R
ORDER_G2 = H2 * R
assert Z % 2 == 0 and (Z - 1) ** 2 % 3 == 0 and Q == (Z - 1) ** 2 * R // 3 + Z
assert ORDER_G1 == Q + 1 - (Z + 1), "the trace of Frobenius is z + 1"
assert R % 2 == 1 and H1 % 2 == 1 and H2 % 2 == 1 and ORDER_G1 % 2 == 1 and ORDER_G2 % 2 == 1, "no point of order two on either curve"

CHUNK = 16
MID_THREADS = 128


class FQ:
    zero, one = 0, 1
    add = staticmethod(lambda a, b: (a + b) % Q)
    sub = staticmethod(lambda a, b: (a - b) % Q)
    mul = staticmethod(lambda a, b: a * b % Q)
    b3 = staticmethod(lambda a: 12 * a % Q)
    b = 4
    inv = staticmethod(lambda a: pow(a, -1, Q))


class FQ2:
    zero, one = (0, 0), (1, 0)
    add = staticmethod(lambda a, b: ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q))
    sub = staticmethod(lambda a, b: ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q))
    mul = staticmethod(lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q))
    b3 = staticmethod(lambda a: (12 * (a[0] - a[1]) % Q, 12 * (a[0] + a[1]) % Q))
    b = (4, 4)

    @staticmethod
    def inv(a):
        n = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
        return (a[0] * n % Q, -a[1] * n % Q)


def inf(F):
    return (F.zero, F.one, F.zero)


def padd(F, P, T):
    """RCB algorithm 7 (a = 0): complete addition"""
    X1, Y1, Z1 = P
    X2, Y2, Z2 = T
    t0, t1, t2 = F.mul(X1, X2), F.mul(Y1, Y2), F.mul(Z1, Z2)
    t3 = F.sub(F.sub(F.mul(F.add(X1, Y1), F.add(X2, Y2)), t0), t1)
    t4 = F.sub(F.sub(F.mul(F.add(Y1, Z1), F.add(Y2, Z2)), t1), t2)
    t5 = F.sub(F.sub(F.mul(F.add(X1, Z1), F.add(X2, Z2)), t0), t2)
    x3 = F.add(F.add(t0, t0), t0)
    bz = F.b3(t2)
    z3, t1m, y3 = F.add(t1, bz), F.sub(t1, bz), F.b3(t5)
    return (F.sub(F.mul(t3, t1m), F.mul(t4, y3)), F.add(F.mul(t1m, z3), F.mul(y3, x3)), F.add(F.mul(z3, t4), F.mul(x3, t3)))


def pmadd(F, P, x2, y2):
    """RCB algorithm 8 (a = 0): complete mixed addition of the affine point (x2, y2)"""
    X1, Y1, Z1 = P
    t0, t1 = F.mul(X1, x2), F.mul(Y1, y2)
    t3 = F.sub(F.sub(F.mul(F.add(x2, y2), F.add(X1, Y1)), t0), t1)
    t4 = F.add(F.mul(y2, Z1), Y1)
    y3 = F.b3(F.add(F.mul(x2, Z1), X1))
    x3 = F.add(F.add(t0, t0), t0)
    bz = F.b3(Z1)
    z3, t1m = F.add(t1, bz), F.sub(t1, bz)
    return (F.sub(F.mul(t3, t1m), F.mul(t4, y3)), F.add(F.mul(y3, x3), F.mul(t1m, z3)), F.add(F.mul(z3, t4), F.mul(x3, t3)))


def pneg(F, P):
    return (P[0], F.sub(F.zero, P[1]), P[2])


def on_curve(F, x, y):
    return F.sub(F.mul(y, y), F.add(F.mul(F.mul(x, x), x), F.b)) == F.zero


def kind_of(F, pt):
    """0 infinity ((0, 0)), 1 a point of the curve, 2 neither"""
    x, y = pt
    if x == F.zero and y == F.zero:
        return 0
    return 1 if on_curve(F, x, y) else 2


def scan(F, pts, chunk=CHUNK, mid=MID_THREADS, carry=None):
    """-> (S, cnt) by the three passes.  carry: None, or (point, count) -- the last record and count of the SLICE before, which
    the middle scan adds to every lane's carry-in (k_pscan_mid's carry_pt / carry_cnt); S and cnt then continue that slice's."""
    n = len(pts)
    chunks = (n + chunk - 1) // chunk if n else 1
    kind = [kind_of(F, p) for p in pts]
    # pass 1: chunk totals and counts
    ct, cb = [], []
    for t in range(chunks):
        acc, bad = inf(F), 0
        for i in range(t * chunk, min((t + 1) * chunk, n)):
            if kind[i] == 1:
                acc = pmadd(F, acc, *pts[i])
            bad += kind[i] == 2
        ct.append(acc)
        cb.append(bad)
    # pass 2: exclusive scan of the totals by `mid` lanes
    per = (chunks + mid - 1) // mid
    span = [(min(t * per, chunks), min(t * per + per, chunks)) for t in range(mid)]
    v, c = [], []
    for lo, hi in span:
        acc, cnt = inf(F), 0
        for j in range(lo, hi):
            acc = padd(F, acc, ct[j])
            cnt += cb[j]
        v.append(acc)
        c.append(cnt)
    d = 1
    while d < mid:                                       # Kogge-Stone: every lane reads the step's values before any is replaced
        v = [padd(F, v[t - d], v[t]) if t >= d else v[t] for t in range(mid)]
        c = [c[t - d] + c[t] if t >= d else c[t] for t in range(mid)]
        d <<= 1
    for t, (lo, hi) in enumerate(span):
        run, cnt = (v[t - 1], c[t - 1]) if t else (inf(F), 0)
        if carry is not None:
            run, cnt = padd(F, carry[0], run), cnt + carry[1]
        for j in range(lo, hi):
            own, oc = ct[j], cb[j]
            ct[j], cb[j] = run, cnt
            run, cnt = padd(F, run, own), cnt + oc
    # pass 3: every chunk again from its carry-in
    S, counts = [None] * (n + 1), [0] * (n + 1)
    for t in range(chunks):
        run, cnt = ct[t], cb[t]
        hi = min((t + 1) * chunk, n)
        for i in range(t * chunk, hi):
            S[i], counts[i] = run, cnt
            if kind[i] == 1:
                run = pmadd(F, run, *pts[i])
            cnt += kind[i] == 2
        if hi == n:
            S[n], counts[n] = run, cnt
    return S, counts


def scan_slices(F, pts, slice_len, chunk=CHUNK, mid=MID_THREADS):
    """the records of n points taken in slices of slice_len as blsgpu_api.hip's range_sums_dev does: per slice (lo, hi, S, cnt)
    with S[j - lo] the prefix of the WHOLE input at j for lo <= j <= hi; record hi of a slice is the carry of the next"""
    out, carry, lo = [], None, 0
    while True:
        hi = min(lo + slice_len, len(pts))
        S, cnt = scan(F, pts[lo:hi], chunk, mid, carry)
        out.append((lo, hi, S, cnt))
        carry, lo = (S[hi - lo], cnt[hi - lo]), hi
        if lo >= len(pts):
            return out


def in_slice(j, lo, hi, last):
    """record j is taken from the slice [lo, hi]: lo <= j < hi, or j = hi in the last slice (k_pscan_begin, k_pscan_range)"""
    return lo <= j and (j < hi or (last and j == hi))


def range_sum_slices(F, slices, begin, end):
    """range_sum over scan_slices' records: the record at `begin` is kept from its slice (k_pscan_begin), the range is finished
    in the slice that holds `end` (k_pscan_range with base / basec)"""
    base = fin = None
    for k, (lo, hi, S, cnt) in enumerate(slices):
        last = k == len(slices) - 1
        if in_slice(begin, lo, hi, last):
            assert base is None
            base = (S[begin - lo], cnt[begin - lo])
        if in_slice(end, lo, hi, last):
            assert fin is None and base is not None, "the begin is copied before the end's slice is finished"
            fin = (S[end - lo], cnt[end - lo])
    if fin[1] != base[1]:
        return 2, (F.zero, F.zero)
    a = affine(F, padd(F, fin[0], pneg(F, base[0])))
    return (1 if a == (F.zero, F.zero) else 0), a


def affine(F, P):
    """(X, Y) / Z, (0, 0) for Z = 0"""
    if P[2] == F.zero:
        return (F.zero, F.zero)
    zi = F.inv(P[2])
    return (F.mul(P[0], zi), F.mul(P[1], zi))


def range_sum(F, S, cnt, begin, end):
    """-> (flag, affine point)"""
    if not 0 <= begin <= end < len(S):
        raise ValueError("begin <= end <= n")
    if cnt[end] != cnt[begin]:
        return 2, (F.zero, F.zero)
    a = affine(F, padd(F, S[end], pneg(F, S[begin])))
    return (1 if a == (F.zero, F.zero) else 0), a
