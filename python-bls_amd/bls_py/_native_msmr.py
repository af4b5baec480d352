"""Marshalling of blsgpu_g1_msm_ranges / blsgpu_g2_msm_ranges and their _dev forms (include/blsgpu.h): multi-scalar sums over
ranges of ANY lengths of a list of points, out_j = sum_{i in [begin_j, end_j)} s_i P_i, in one device call with nothing padded.

The four prototypes are rows of _native.PROTOTYPES like every other; the functions here take a _native.Engine and go through
its shared call helpers.  They are reached through backend.extension("g1_msm_ranges") and ("g2_msm_ranges"), not as methods of
the engine or of the provider, whose method sets are fixed lists."""

__all__ = ["g1_msm_ranges", "g2_msm_ranges", "g1_msm_ranges_dev", "g2_msm_ranges_dev"]


def _msm_ranges(eng, name, psz, pts, scalars, ranges):
    if len(pts) % psz:
        raise ValueError("need n x %d bytes" % psz)
    n = len(pts) // psz
    if not isinstance(scalars, (bytes, bytearray)):
        scalars = list(scalars)
        if any(not 0 <= int(s) < 1 << 256 for s in scalars):
            raise ValueError("scalars are integers in [0, 2^256)")
    sb = eng._scalars(scalars, n, "scalars")
    flat = [v for r in ranges for v in r]
    if len(flat) % 2:
        raise ValueError("a range is (begin, end)")
    m = len(flat) // 2
    out, flag = eng._call_out(name, bytes(pts), sb, n, eng._indices(flat, "range"), m, out=[psz * m, m])
    return out, flag


def g1_msm_ranges(eng, pts, scalars, ranges):
    """sum_{i in [begin, end)} scalars[i] * pts[i] for m ranges (begin, end), begin <= end <= n, over n affine G1 points (n x 96
    bytes, (0,0) = infinity) by blsgpu_g1_msm_ranges.  scalars: n ints in [0, 2^256) or 32 n bytes big-endian, PUBLIC data.
    -> (m x 96 affine bytes, m flag bytes: 0 finite, 1 infinity, 2 the range holds a point off the curve and its output is
    (0,0))"""
    return _msm_ranges(eng, "blsgpu_g1_msm_ranges", 96, pts, scalars, ranges)


def g2_msm_ranges(eng, pts, scalars, ranges):
    """the same in G2 (blsgpu_g2_msm_ranges): points of 192 bytes"""
    return _msm_ranges(eng, "blsgpu_g2_msm_ranges", 192, pts, scalars, ranges)


def g1_msm_ranges_dev(eng, d_pts, d_scalars, n, d_ranges, m, d_out_aff, d_out_flag, stream=0):
    eng._call("blsgpu_g1_msm_ranges_dev", d_pts, d_scalars, n, d_ranges, m, d_out_aff, d_out_flag, stream)


def g2_msm_ranges_dev(eng, d_pts, d_scalars, n, d_ranges, m, d_out_aff, d_out_flag, stream=0):
    eng._call("blsgpu_g2_msm_ranges_dev", d_pts, d_scalars, n, d_ranges, m, d_out_aff, d_out_flag, stream)
