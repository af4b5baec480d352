"""Marshalling of blsgpu_verify_aggregates and its _dev form (include/blsgpu.h): BLS.verify of m aggregates of any shapes in one
device call -- hash to G2, the ragged key sums, the ragged multi-pairing and the comparison with one, with nothing returning to
the host in between.

The two prototypes are rows of _native.PROTOTYPES like every other; the functions here take a _native.Engine and go through its
shared call helpers.  verify_aggregates is reached through backend.extension("verify_aggregates"), not as a method of the engine
or of the provider, whose method sets are fixed lists."""

__all__ = ["verify_aggregates", "verify_aggregates_dev", "tables"]


def tables(aggregates):
    """The three tables of the call from Python lists.  aggregates: per aggregate a list of groups, a group being (message
    index, number of keys); the keys of the call lie group after group, aggregate after aggregate.
    -> (grp_off: n_grp + 1 offsets into the keys, grp_msg: n_grp message indices, agg_off: m + 1 offsets into the groups)"""
    grp_off, grp_msg, agg_off = [0], [], [0]
    for groups in aggregates:
        for msg, nkeys in groups:
            if int(nkeys) < 0 or int(msg) < 0:
                raise ValueError("a group is (message index, number of keys), both non-negative")
            grp_msg.append(int(msg))
            grp_off.append(grp_off[-1] + int(nkeys))
        agg_off.append(len(grp_msg))
    return grp_off, grp_msg, agg_off


def _tables(eng, grp_off, grp_msg, agg_off):
    if not agg_off or len(grp_off) != len(grp_msg) + 1:
        raise ValueError("grp_off holds n_grp + 1 offsets, agg_off m + 1")
    if any(int(v) < 0 for t in (grp_off, grp_msg, agg_off) for v in t):
        raise ValueError("offsets and indices are non-negative")
    return (eng._indices(grp_off, "key"), eng._indices(grp_msg, "message"), len(grp_msg), eng._indices(agg_off, "group"),
            len(agg_off) - 1)


def verify_aggregates(eng, sigs, msg_hashes, keys, exps, grp_off, grp_msg, agg_off, gt=False):
    """blsgpu_verify_aggregates.  sigs: m x 192 affine bytes; msg_hashes: n_msgs x 32 bytes, each hashed once; keys: n_keys x 96
    affine bytes; exps: None (every exponent 1), n_keys ints in [0, 2^256) or 32 n_keys bytes big-endian, PUBLIC data; the three
    tables as tables() builds them.
    -> (m status bytes: 1 the product is one, 0 it is not, 2 not decided here -- an infinity signature or a key off the
    curve --, m x 576 bytes of the products or None)"""
    if len(sigs) % 192 or len(msg_hashes) % 32 or len(keys) % 96:
        raise ValueError("need m x 192 bytes of signatures, n_msgs x 32 of hashes and n_keys x 96 of keys")
    n_keys = len(keys) // 96
    go, gm, n_grp, ao, m = _tables(eng, grp_off, grp_msg, agg_off)
    if len(sigs) != 192 * m:
        raise ValueError("one signature per aggregate")
    if exps is not None:
        if not isinstance(exps, (bytes, bytearray)):
            exps = list(exps)
            if any(not 0 <= int(e) < 1 << 256 for e in exps):
                raise ValueError("exponents are integers in [0, 2^256)")
        exps = eng._scalars(exps, n_keys, "exps")
    status, out = eng._call_out("blsgpu_verify_aggregates", bytes(sigs), bytes(msg_hashes), len(msg_hashes) // 32, bytes(keys), exps, n_keys,
                                go, gm, n_grp, ao, m, out=[m, 576 * m if gt else None])
    return status, out


def verify_aggregates_dev(eng, d_sigs, d_msg_hashes, n_msgs, d_keys, d_exps, n_keys, grp_off, grp_msg, agg_off, d_status, d_out_gt=None,
                          stream=0):
    """the device form: signatures, hashes, keys, exponents (or None), status and products (or None) in device memory; the
    three tables are HOST lists (the library plans the whole call from them before it returns)"""
    go, gm, n_grp, ao, m = _tables(eng, grp_off, grp_msg, agg_off)
    eng._call("blsgpu_verify_aggregates_dev", d_sigs, d_msg_hashes, n_msgs, d_keys, d_exps, n_keys, go, gm, n_grp, ao, m, d_status, d_out_gt,
              stream)
