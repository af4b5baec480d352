"""Marshalling of blsgpu_map_to_g1 / blsgpu_hash_to_g1 and their _dev forms (include/blsgpu.h): hash to G1 on the device, one
message per lane -- the batch form of ec.hash_to_point_prehashed_Fq.

The four prototypes are rows of _native.PROTOTYPES like every other; the functions here take a _native.Engine and go through
its shared call helpers.  They are reached through backend.extension("map_to_g1") and ("hash_to_g1"), not as methods of the
engine or of the provider, whose method sets are fixed lists."""

__all__ = ["map_to_g1", "hash_to_g1", "map_to_g1_dev", "hash_to_g1_dev"]


def _h2g1(eng, name, item, data, aff, ser):
    data = bytes(data)
    if len(data) % item:
        raise ValueError("need n x %d bytes" % item)
    if not (aff or ser):
        raise ValueError("ask for at least one output")
    n = len(data) // item
    out_aff, out_ser, inf = eng._call_out(name, data if n else None, n, out=[96 * n if aff else None, 48 * n if ser else None, n])
    return out_aff, out_ser, eng._flags(inf)


def map_to_g1(eng, t, aff=True, ser=False):
    """h (sw_encode(t0) + sw_encode(t1)) for n pairs of field elements (blsgpu_map_to_g1).  t: n x 96 bytes, t0 || t1 as
    48-byte big-endian integers, any value below 2^384 taken mod q.
    -> (n x 96 affine bytes, (0, 0) for infinity | None, n x 48 serialised bytes | None, [is_inf])"""
    return _h2g1(eng, "blsgpu_map_to_g1", 96, t, aff, ser)


def hash_to_g1(eng, msg_hashes, aff=True, ser=False):
    """hash_to_point_prehashed_Fq of n 32-byte message hashes, the SHA-256 chain on the device too (blsgpu_hash_to_g1).
    -> as map_to_g1"""
    return _h2g1(eng, "blsgpu_hash_to_g1", 32, msg_hashes, aff, ser)


def map_to_g1_dev(eng, d_t, n, d_out_aff, d_out_ser, d_out_inf, stream=0):
    eng._call("blsgpu_map_to_g1_dev", d_t, n, d_out_aff, d_out_ser, d_out_inf, stream)


def hash_to_g1_dev(eng, d_msg_hashes, n, d_out_aff, d_out_ser, d_out_inf, stream=0):
    eng._call("blsgpu_hash_to_g1_dev", d_msg_hashes, n, d_out_aff, d_out_ser, d_out_inf, stream)
