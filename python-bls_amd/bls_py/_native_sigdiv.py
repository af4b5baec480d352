"""Marshalling of blsgpu_sig_divide and its _dev form (include/blsgpu.h): the device work of a batch of Signature.divide_by
calls -- the quotient scalar of every divisor from its aggregation-tree exponents, checked for uniqueness, and the G2 sums
out_j = S_j + sum_d (n - q_d) D_d -- in one call.

The two prototypes are rows of _native.PROTOTYPES like every other; the functions here take a _native.Engine and go through
its shared call helpers.  They are reached through backend.extension("sig_divide"), not as methods of the engine or of the
provider, whose method sets are fixed lists."""
import ctypes

__all__ = ["sig_divide", "sig_divide_dev"]


def _exponents(eng, v, n, what):
    if not isinstance(v, (bytes, bytearray)):
        v = list(v)
        if any(not 0 <= int(e) < 1 << 256 for e in v):
            raise ValueError("%s are integers in [0, 2^256)" % what)
    return eng._scalars(v, n, what)


def sig_divide(eng, pts, pt_off, ent_off, ent_dividend, ent_divisor):
    """m dividends over n_pts affine G2 points (n_pts x 192 bytes, (0,0) = infinity) by blsgpu_sig_divide.  pt_off: m + 1
    offsets, dividend j owns the points [pt_off[j], pt_off[j + 1]) -- its own signature, then its divisors.  ent_off: n_pts + 1
    offsets, point p owns the entries [ent_off[p], ent_off[p + 1]) -- none for a dividend's own point.  ent_dividend /
    ent_divisor: per entry the dividend's and the divisor's exponent, ints in [0, 2^256) or 32 bytes big-endian each.  PUBLIC data.
    -> (m x 192 affine bytes, m flag bytes: 0 finite, 1 infinity, 2 a point off the twist, 3 a refused divisor;
        n_pts status bytes: 0 fine, 1 pairs not unique, 2 a divisor exponent that is 0 mod n;
        n_pts x 32 scalar bytes; (0 the plain path ran | 1 the scalar path, divisors with a quotient other than 1))"""
    if len(pts) % 192:
        raise ValueError("need n x 192 bytes")
    n_pts = len(pts) // 192
    pt_off, ent_off = list(pt_off), list(ent_off)
    if not pt_off or len(ent_off) != n_pts + 1:
        raise ValueError("pt_off holds m + 1 offsets, ent_off n_pts + 1")
    m = len(pt_off) - 1
    n_ent = len(ent_dividend) // 32 if isinstance(ent_dividend, (bytes, bytearray)) else len(ent_dividend)
    ea = _exponents(eng, ent_dividend, n_ent, "ent_dividend")
    eb = _exponents(eng, ent_divisor, n_ent, "ent_divisor")
    stats = (ctypes.c_uint32 * 2)()
    out, flag, status, scalars = eng._call_out("blsgpu_sig_divide", bytes(pts), n_pts, eng._indices(pt_off, "point"), m,
                                               eng._indices(ent_off, "entry"), ea, eb, n_ent, out=[192 * m, m, n_pts, 32 * n_pts],
                                               tail=(stats,))
    return out, flag, status, scalars, (int(stats[0]), int(stats[1]))


def sig_divide_dev(eng, d_pts, n_pts, d_pt_off, m, d_ent_off, d_ent_dividend, d_ent_divisor, n_ent, d_out_aff, d_out_flag, d_out_status,
                   d_out_scalars=None, stream=0):
    """blsgpu_sig_divide_dev on device pointers; -> (path, divisors with a quotient other than 1), which the call reads in its
    one synchronisation"""
    stats = (ctypes.c_uint32 * 2)()
    eng._call("blsgpu_sig_divide_dev", d_pts, n_pts, d_pt_off, m, d_ent_off, d_ent_dividend, d_ent_divisor, n_ent, d_out_aff, d_out_flag,
              d_out_status, d_out_scalars, stats, stream)
    return int(stats[0]), int(stats[1])
