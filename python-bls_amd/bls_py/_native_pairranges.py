"""Marshalling of blsgpu_pairing_multi_ranges and its _dev form (include/blsgpu.h): multi-pairings over ranges of ANY lengths of
one list of pairs, out_j = fq_ate_pairing_multi of the pairs [begin_j, end_j), in one device call with nothing padded.

The two prototypes are rows of _native.PROTOTYPES like every other; the functions here take a _native.Engine and go through its
shared call helpers.  pairing_multi_ranges is reached through backend.extension("pairing_multi_ranges"), not as a method of the
engine or of the provider, whose method sets are fixed lists."""

__all__ = ["pairing_multi_ranges", "pairing_multi_ranges_dev", "range_table"]


def range_table(eng, ranges):
    """(the c_uint32 array begin_0, end_0, begin_1, .. of `ranges`, m): host memory in both forms of the call"""
    flat = [v for r in ranges for v in r]
    if len(flat) % 2:
        raise ValueError("a range is (begin, end)")
    if any(int(v) < 0 for v in flat):
        raise ValueError("range bounds are non-negative")
    return eng._indices(flat, "range"), len(flat) // 2


def pairing_multi_ranges(eng, g1, g2, ranges, inf=None):
    """fq_ate_pairing_multi of the pairs [begin, end) for m ranges (begin, end), begin <= end <= n, over n pairs (g1: n x 96
    bytes, g2: n x 192 bytes affine, inf: None or 2 flag bytes per pair, as pairing_multi_batch takes them) by
    blsgpu_pairing_multi_ranges.  Ranges may overlap, repeat or be empty (Fq12 one).  -> m x 576 bytes"""
    if len(g1) % 96 or len(g2) != 2 * len(g1):
        raise ValueError("need n x 96 bytes of g1 and n x 192 bytes of g2")
    n = len(g1) // 96
    if inf is not None:
        inf = bytes(inf)
        if len(inf) != 2 * n:
            raise ValueError("inf must hold 2 flags per pair")
    tab, m = range_table(eng, ranges)
    return eng._call_out("blsgpu_pairing_multi_ranges", bytes(g1), bytes(g2), inf, n, tab, m, out=[576 * m])[0]


def pairing_multi_ranges_dev(eng, d_g1, d_g2, n, ranges, d_out, stream=0, d_inf=None):
    """the device form: the pairs, the flags and the m x 576 result bytes in device memory; `ranges` is the HOST table as above
    (the library plans the whole call from it before it returns, nothing is read back)"""
    tab, m = range_table(eng, ranges)
    eng._call("blsgpu_pairing_multi_ranges_dev", d_g1, d_g2, d_inf, n, tab, m, d_out, stream)
