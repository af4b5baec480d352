"""Marshalling of blsgpu_hash_pks_ranges, blsgpu_aggregate_pub_keys_secure_ranges, blsgpu_aggregate_sigs_secure_ranges and their
_dev forms (include/blsgpu.h): secure aggregation for groups of ANY sizes in one device call -- group g hashes the keys
[pk_off[g], pk_off[g + 1]) of one list of serialised keys and owns the exponents [exp_off[g], exp_off[g + 1]).

The six prototypes are rows of _native.PROTOTYPES like every other; the functions here take a _native.Engine and go through
its shared call helpers.  They are reached through backend.extension("hash_pks_ranges"), ("aggregate_pub_keys_secure_ranges")
and ("aggregate_sigs_secure_ranges"), not as methods of the engine or of the provider, whose method sets are fixed lists."""
import hashlib

from . import _native

__all__ = ["hash_pks_ranges", "aggregate_pub_keys_secure_ranges", "aggregate_sigs_secure_ranges", "hash_pks_ranges_dev",
           "aggregate_pub_keys_secure_ranges_dev", "aggregate_sigs_secure_ranges_dev"]


def _offsets(off, count, what):
    off = [int(v) for v in off]
    if not off or off[0] != 0 or any(a > b for a, b in zip(off, off[1:])) or off[-1] > count:
        raise ValueError("%s: groups + 1 offsets from 0, never stepping down, ending within the %d items" % (what, count))
    return off


def _pk_hashes(pks_ser, pk_off, pk_hash):
    """the pk_hash_in of a call: the caller's digests, the host's for fewer than HASH_PKS_DEVICE_GROUPS groups (one group per
    lane cannot fill a wavefront; hashlib runs at memory speed), or None: the device hashes the keys.
    pk_hash: bytes, None (that rule) or False (the device, whatever the count)"""
    groups = len(pk_off) - 1
    if pk_hash is False or (pk_hash is None and groups >= _native.HASH_PKS_DEVICE_GROUPS):
        return None
    if pk_hash is None:
        mv = memoryview(pks_ser)
        return b"".join(hashlib.sha256(mv[48 * pk_off[g]:48 * pk_off[g + 1]]).digest() for g in range(groups))
    if len(pk_hash) != 32 * groups:
        raise ValueError("need one digest of 32 bytes per group")
    return bytes(pk_hash)


def _keys(pks_ser, pk_off):
    pks_ser = bytes(pks_ser)
    if len(pks_ser) % 48:
        raise ValueError("need n_keys serialised keys of 48 bytes")
    return pks_ser, _offsets(pk_off, len(pks_ser) // 48, "pk_off")


def hash_pks_ranges(eng, pks_ser, pk_off, exp_off, pk_hash=None, want_pk_hash=False):
    """util.hash_pks(exp_off[g + 1] - exp_off[g], the keys [pk_off[g], pk_off[g + 1])) for every group g of one list of
    serialised keys (n_keys x 48 bytes) by blsgpu_hash_pks_ranges; pk_hash: see _pk_hashes.
    -> exp_off[-1] x 32 exponent bytes big-endian, below n (, groups x 32 digest bytes)"""
    pks_ser, pk_off = _keys(pks_ser, pk_off)
    exp_off = _offsets(exp_off, 1 << 32, "exp_off")
    if len(exp_off) != len(pk_off):
        raise ValueError("pk_off and exp_off hold groups + 1 offsets each")
    groups = len(pk_off) - 1
    ph = _pk_hashes(pks_ser, pk_off, pk_hash)
    out, dg = eng._call_out("blsgpu_hash_pks_ranges", None if ph else pks_ser, len(pks_ser) // 48, None if ph else eng._indices(pk_off, "offset"),
                            eng._indices(exp_off, "offset"), groups, ph, out=[32 * exp_off[-1], 32 * groups if want_pk_hash else None])
    return (out, dg) if want_pk_hash else out


def aggregate_pub_keys_secure_ranges(eng, pts_aff, pks_ser, pk_off, pk_hash=None):
    """sum_i t_i P_i per group (blsgpu_aggregate_pub_keys_secure_ranges): pts_aff n_keys x 96 affine bytes, pks_ser the same
    keys serialised, both in the order to be hashed; group g is the keys [pk_off[g], pk_off[g + 1]).
    -> (groups x 96 affine bytes, groups flag bytes: 0 finite, 1 infinity, 2 a point off the curve in the group)"""
    pks_ser, pk_off = _keys(pks_ser, pk_off)
    n = len(pks_ser) // 48
    if len(pts_aff) != 96 * n:
        raise ValueError("point buffer length does not match the keys")
    groups = len(pk_off) - 1
    ph = _pk_hashes(pks_ser, pk_off, pk_hash)
    out, flag = eng._call_out("blsgpu_aggregate_pub_keys_secure_ranges", bytes(pts_aff), None if ph else pks_ser, n, eng._indices(pk_off, "offset"),
                              groups, ph, out=[96 * groups, groups])
    return out, flag


def aggregate_sigs_secure_ranges(eng, sigs_aff, sig_off, pks_ser, pk_off, pk_hash=None):
    """sum_i t_i S_i per group (blsgpu_aggregate_sigs_secure_ranges): sigs_aff n_sigs x 192 affine bytes in the order the
    exponents multiply them, group g owning the signatures [sig_off[g], sig_off[g + 1]) and hashing the keys
    [pk_off[g], pk_off[g + 1]).  -> (groups x 192 affine bytes, groups flag bytes)"""
    pks_ser, pk_off = _keys(pks_ser, pk_off)
    if len(sigs_aff) % 192:
        raise ValueError("need n_sigs affine signatures of 192 bytes")
    n_sigs = len(sigs_aff) // 192
    sig_off = _offsets(sig_off, n_sigs, "sig_off")
    if len(sig_off) != len(pk_off):
        raise ValueError("pk_off and sig_off hold groups + 1 offsets each")
    groups = len(pk_off) - 1
    ph = _pk_hashes(pks_ser, pk_off, pk_hash)
    out, flag = eng._call_out("blsgpu_aggregate_sigs_secure_ranges", bytes(sigs_aff), n_sigs, eng._indices(sig_off, "offset"),
                              None if ph else pks_ser, len(pks_ser) // 48, None if ph else eng._indices(pk_off, "offset"), groups, ph,
                              out=[192 * groups, groups])
    return out, flag


def hash_pks_ranges_dev(eng, d_pks_ser, n_keys, d_pk_off, d_exp_off, n_exp, groups, d_pk_hash_in, d_out_ts, d_out_pk_hash=None, stream=0):
    eng._call("blsgpu_hash_pks_ranges_dev", d_pks_ser, n_keys, d_pk_off, d_exp_off, n_exp, groups, d_pk_hash_in, d_out_ts, d_out_pk_hash, stream)


def aggregate_pub_keys_secure_ranges_dev(eng, d_pts_aff, d_pks_ser, n_keys, d_pk_off, groups, d_pk_hash_in, d_out_aff, d_out_flag, stream=0):
    eng._call("blsgpu_aggregate_pub_keys_secure_ranges_dev", d_pts_aff, d_pks_ser, n_keys, d_pk_off, groups, d_pk_hash_in, d_out_aff, d_out_flag,
              stream)


def aggregate_sigs_secure_ranges_dev(eng, d_sigs_aff, n_sigs, d_sig_off, d_pks_ser, n_keys, d_pk_off, groups, d_pk_hash_in, d_out_aff, d_out_flag,
                                     stream=0):
    eng._call("blsgpu_aggregate_sigs_secure_ranges_dev", d_sigs_aff, n_sigs, d_sig_off, d_pks_ser, n_keys, d_pk_off, groups, d_pk_hash_in,
              d_out_aff, d_out_flag, stream)
