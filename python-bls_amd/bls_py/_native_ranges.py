"""Marshalling of blsgpu_g1_range_sums / blsgpu_g2_range_sums / blsgpu_verify_find_folded and their _dev forms
(include/blsgpu.h): sums over ranges of a list of points from prefix sums on the device, and the batch verification that names
the forgeries with the items of one message folded inside every node.

The six prototypes are rows of _native.PROTOTYPES like every other; the functions here take a _native.Engine and go through
its shared call helpers.  They are reached through backend.extension("g1_range_sums"), ("g2_range_sums") and
("verify_find_folded"), not as methods of the engine or of the provider, whose method sets are fixed lists."""
import ctypes

__all__ = ["g1_range_sums", "g2_range_sums", "g1_range_sums_dev", "g2_range_sums_dev", "verify_find_folded", "verify_find_folded_dev"]


def _range_sums(eng, name, psz, pts, ranges):
    if len(pts) % psz:
        raise ValueError("need n x %d bytes" % psz)
    flat = [v for r in ranges for v in r]
    if len(flat) % 2:
        raise ValueError("a range is (begin, end)")
    m = len(flat) // 2
    out, flag = eng._call_out(name, bytes(pts), len(pts) // psz, eng._indices(flat, "range"), m, out=[psz * m, m])
    return out, flag


def g1_range_sums(eng, pts, ranges):
    """the sums of pts[begin:end] for m ranges (begin, end), begin <= end <= n, over n affine G1 points (n x 96 bytes, (0,0) =
    infinity) by blsgpu_g1_range_sums.  -> (m x 96 affine bytes, m flag bytes: 0 finite, 1 infinity, 2 the range holds a
    point off the curve and its output is (0,0))"""
    return _range_sums(eng, "blsgpu_g1_range_sums", 96, pts, ranges)


def g2_range_sums(eng, pts, ranges):
    """the same in G2 (blsgpu_g2_range_sums): points of 192 bytes"""
    return _range_sums(eng, "blsgpu_g2_range_sums", 192, pts, ranges)


def g1_range_sums_dev(eng, d_pts, n, d_ranges, m, d_out_aff, d_out_flag, stream=0):
    eng._call("blsgpu_g1_range_sums_dev", d_pts, n, d_ranges, m, d_out_aff, d_out_flag, stream)


def g2_range_sums_dev(eng, d_pts, n, d_ranges, m, d_out_aff, d_out_flag, stream=0):
    eng._call("blsgpu_g2_range_sums_dev", d_pts, n, d_ranges, m, d_out_aff, d_out_flag, stream)


def verify_find_folded(eng, sigs, keys, key_idx, msg_hashes, msg_idx, weights):
    """_native_find.verify_find's arguments and results through blsgpu_verify_find_folded: msg_idx must be non-decreasing, and
    a node test takes one pair per distinct message in the node plus one.
    -> (n status bytes: 1 valid, 0 invalid, 2 not decided; (rounds, node tests, pairs fed to the pairing))"""
    if len(sigs) % 192 or len(keys) % 96 or len(msg_hashes) % 32:
        raise ValueError("signatures are 192, keys 96, message hashes 32 bytes")
    n = len(sigs) // 192
    wb = eng._scalars(weights, n, "weights", width=8)
    if len(key_idx) != n or len(msg_idx) != n:
        raise ValueError("one key index and one message index per signature")
    stats = (ctypes.c_uint64 * 3)()
    st = eng._call_out("blsgpu_verify_find_folded", bytes(sigs), bytes(keys), len(keys) // 96, eng._indices(key_idx, "key"),
                       bytes(msg_hashes), len(msg_hashes) // 32, eng._indices(msg_idx, "message"), wb, n, out=[n], tail=(stats,))[0]
    return st, tuple(int(v) for v in stats)


def verify_find_folded_dev(eng, d_sigs, d_keys, n_keys, d_key_idx, d_msg_hashes, n_msgs, d_msg_idx, d_weights, n, d_status, stream=0):
    """-> (rounds, node tests, pairs); the status bytes are in d_status when the call returns"""
    stats = (ctypes.c_uint64 * 3)()
    eng._call("blsgpu_verify_find_folded_dev", d_sigs, d_keys, n_keys, d_key_idx, d_msg_hashes, n_msgs, d_msg_idx, d_weights, n,
              d_status, stats, stream)
    return tuple(int(v) for v in stats)
