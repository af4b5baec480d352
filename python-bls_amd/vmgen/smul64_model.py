"""Integer model of the multiplication by a short PUBLIC scalar (csrc/blsgpu_smul64.hip k_smul64): the SPECIFICATION of its
digits and of its window recurrence.  out = w P for a 64-bit weight w.  The weights are public data, so -- unlike
g2smul_model.py -- nothing here is uniform across scalars: the table entry a window adds is chosen by its digit.

  digits(w)      the sixteen plain nibbles of w, least significant first: d_j in [0, 16), sum_j d_j 16^j = w.  The device
                 reads them from the two 32-bit halves of the big-endian weight (digit j from the high half when j >= 8).
  smul(x, w)     the recurrence on INTEGERS, where a point is the integer x, an addition is + and a doubling is 2 *: a table
                 T[e] = e x for e < 16 -- T[0] = 0 is infinity, T[e] = T[e - 1] + x by fourteen real additions (T[1] = 0 + x
                 costs nothing: the first mixed addition meets infinity) --; then from the top window down four doublings
                 (not before the top window) and ONE addition of T[d_j].  60 doublings and 16 additions for every weight,
                 against 252 and 64 of k_smul (blsgpu_msm.hip) on the same weight zero-extended to 256 bits.

ops(w) counts what a run does; tests/test_smul64_model.py holds digits and recurrence against w x.
"""
WINDOWS = 16
TABLE = 16


def digits(w):
    """digits d_j in [0, 16), least significant first"""
    if not 0 <= w < 1 << 64:
        raise ValueError("weights are 64-bit")
    hi, lo = w >> 32, w & 0xFFFFFFFF                     # the device's two words
    return [((hi if j >= 8 else lo) >> (4 * (j & 7))) & 15 for j in range(WINDOWS)]


def build_table(x):
    """T[e] = e x by repeated addition of x; k_smul64's first loop"""
    T = [0]
    for _ in range(1, TABLE):
        T.append(T[-1] + x)
    return T


def smul(x, w):
    """(w x by the window recurrence, {"dbl": doublings, "add": window additions, "table_add": table additions})"""
    T = build_table(x)
    ops = {"dbl": 0, "add": 0, "table_add": TABLE - 2}
    acc = 0
    d = digits(w)
    for j in range(WINDOWS - 1, -1, -1):
        if j != WINDOWS - 1:
            for _ in range(4):
                acc = 2 * acc
                ops["dbl"] += 1
        acc = acc + T[d[j]]
        ops["add"] += 1
    return acc, ops
