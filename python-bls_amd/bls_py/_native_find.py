"""Marshalling of blsgpu_g1_mul_short / blsgpu_g2_mul_short / blsgpu_verify_find and their _dev forms (include/blsgpu.h):
points by short public scalars, and batch verification that names the forgeries.

The six prototypes are rows of _native.PROTOTYPES like every other; the functions here take a _native.Engine and go through
its shared call helpers.  They are reached through backend.extension("verify_find") (and "g1_mul_short", "g2_mul_short"), not
as methods of the engine or of the provider, whose method sets are fixed lists."""
import ctypes

__all__ = ["g1_mul_short", "g2_mul_short", "g1_mul_short_dev", "g2_mul_short_dev", "verify_find", "verify_find_dev"]


def _mul_short(eng, name, psz, pts, weights):
    if len(pts) % psz:
        raise ValueError("need n x %d bytes" % psz)
    n = len(pts) // psz
    out, inf = eng._call_out(name, bytes(pts), eng._scalars(weights, n, "weights", width=8), n, out=[psz * n, n])
    return out, eng._flags(inf)


def g1_mul_short(eng, pts, weights):
    """w_i P_i for n PUBLIC 64-bit weights (n x 8 bytes big-endian, or ints below 2^64) on the 16-window schedule of
    blsgpu_g1_mul_short; the bytes of g1_msm(k=1) on the zero-extended weights.  -> (n x 96 affine bytes, [is_infinity])"""
    return _mul_short(eng, "blsgpu_g1_mul_short", 96, pts, weights)


def g2_mul_short(eng, pts, weights):
    """the same in G2 (blsgpu_g2_mul_short).  -> (n x 192 affine bytes, [is_infinity])"""
    return _mul_short(eng, "blsgpu_g2_mul_short", 192, pts, weights)


def g1_mul_short_dev(eng, d_pts, d_w, n, d_out_aff, d_out_inf=None, stream=0):
    eng._call("blsgpu_g1_mul_short_dev", d_pts, d_w, n, d_out_aff, d_out_inf, stream)


def g2_mul_short_dev(eng, d_pts, d_w, n, d_out_aff, d_out_inf=None, stream=0):
    eng._call("blsgpu_g2_mul_short_dev", d_pts, d_w, n, d_out_aff, d_out_inf, stream)


def verify_find(eng, sigs, keys, key_idx, msg_hashes, msg_idx, weights):
    """n signatures with their own keys and messages checked on the device by one random linear combination, and what
    fails bisected down to the forgeries (blsgpu_verify_find): sigs n x 192 affine bytes, keys n_keys x 96 affine bytes,
    key_idx n indices into them, msg_hashes n_msgs x 32 bytes, msg_idx n indices into them, weights n x 8 bytes big-endian
    (or ints below 2^64; a zero weight is taken as 1).
    -> (n status bytes: 1 valid, 0 invalid, 2 not decided (the key is off the curve, outside G1 or at infinity, or H(h) is
    at infinity); (rounds, node tests, pairs fed to the pairing))"""
    if len(sigs) % 192 or len(keys) % 96 or len(msg_hashes) % 32:
        raise ValueError("signatures are 192, keys 96, message hashes 32 bytes")
    n = len(sigs) // 192
    wb = eng._scalars(weights, n, "weights", width=8)
    if len(key_idx) != n or len(msg_idx) != n:
        raise ValueError("one key index and one message index per signature")
    stats = (ctypes.c_uint64 * 3)()
    st = eng._call_out("blsgpu_verify_find", bytes(sigs), bytes(keys), len(keys) // 96, eng._indices(key_idx, "key"),
                       bytes(msg_hashes), len(msg_hashes) // 32, eng._indices(msg_idx, "message"), wb, n, out=[n], tail=(stats,))[0]
    return st, tuple(int(v) for v in stats)


def verify_find_dev(eng, d_sigs, d_keys, n_keys, d_key_idx, d_msg_hashes, n_msgs, d_msg_idx, d_weights, n, d_status, stream=0):
    """-> (rounds, node tests, pairs); the status bytes are in d_status when the call returns"""
    stats = (ctypes.c_uint64 * 3)()
    eng._call("blsgpu_verify_find_dev", d_sigs, d_keys, n_keys, d_key_idx, d_msg_hashes, n_msgs, d_msg_idx, d_weights, n, d_status,
              stats, stream)
    return tuple(int(v) for v in stats)
