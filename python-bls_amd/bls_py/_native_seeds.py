"""Marshalling of blsgpu_keys_from_seeds / blsgpu_keys_from_seeds_dev (include/blsgpu.h): keys from seeds on the device.

The two prototypes are rows of _native.PROTOTYPES like every other; the functions here take a _native.Engine and go through
its shared call helpers.  They are reached through backend.extension("keys_from_seeds"), not as methods of the engine or of
the provider, whose method sets are fixed lists."""
from ._native import HD_PARENT_BYTES, SEED_MAX_BYTES

__all__ = ["SEED_MAX_BYTES", "keys_from_seeds", "keys_from_seeds_dev"]


def keys_from_seeds(eng, seeds, seed_len, n, hd=False, sk=True, chain=None, aff=True, ser=True, parents=False):
    """PrivateKey.from_seed (hd false) or ExtendedPrivateKey.from_seed (hd true) of n seeds of seed_len bytes each, seeds
    their concatenation (blsgpu_keys_from_seeds); chain: None = with hd.  parents: the n records of HD_PARENT_BYTES that
    hd_paths_secret takes (hd only).
    -> (n x 32 key bytes, n x 32 chain codes, n x 96 affine public keys, n x 48 serialised public keys, n x 160 parent
    records), None for what is not asked for"""
    seeds = bytes(seeds)
    if seed_len > SEED_MAX_BYTES:
        raise ValueError("seeds are at most %d bytes" % SEED_MAX_BYTES)
    if len(seeds) != seed_len * n:
        raise ValueError("need n x seed_len bytes of seeds")
    chain = bool(hd) if chain is None else chain
    if not hd and (chain or parents):
        raise ValueError("chain codes and parent records belong to hd")
    if not (sk or chain or aff or ser or parents):
        raise ValueError("ask for at least one output")
    return tuple(eng._call_out("blsgpu_keys_from_seeds", seeds if seed_len else None, seed_len, n, 1 if hd else 0,
                               out=[32 * n if sk else None, 32 * n if chain else None, 96 * n if aff else None,
                                    48 * n if ser else None, HD_PARENT_BYTES * n if parents else None]))


def keys_from_seeds_dev(eng, d_seeds, seed_len, n, hd, d_out_sk, d_out_chain, d_out_pk_aff, d_out_pk_ser, d_out_parents, stream=0):
    eng._call("blsgpu_keys_from_seeds_dev", d_seeds, seed_len, n, 1 if hd else 0, d_out_sk, d_out_chain, d_out_pk_aff, d_out_pk_ser,
              d_out_parents, stream)
