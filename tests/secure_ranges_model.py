"""Python model of csrc/secure_ranges_plan.h: the refusals of the ragged secure aggregation, the validation of an offset table,
the grids, the workspace and the cut of a host-buffer call into staged slices on group boundaries.
tests/test_secure_ranges_plan_host.py holds the header, compiled for the host, against it.  hash_pks_ranges() is the oracle of the
device tests: util.hash_pks per group from hashlib and Python integers."""
import hashlib

N = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001      # the group order

CHECK_THREADS, DIGEST_THREADS, EXP_THREADS = 256, 64, 256
MAX_ITEMS = 1 << 31
MAX_GROUPS = 1 << 30
SLICE_ITEMS = 1 << 18
OK, FIRST_NOT_ZERO, DECREASING, PAST_END = 0, 1, 2, 3

# the group lengths of the device tests: every residue of len mod 4, the block-boundary and padding cases, empty groups
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 67]


def too_large(n_keys, n_exp, groups):
    return n_keys >= MAX_ITEMS or n_exp >= MAX_ITEMS or groups >= MAX_GROUPS


def validate(off, count):
    """-> (verdict, where) of one table of groups + 1 offsets over `count` items: the first offset, then group by group a step
    down, then the last offset"""
    if len(off) < 2:
        return OK, 0
    if off[0] != 0:
        return FIRST_NOT_ZERO, 0
    for g, (a, b) in enumerate(zip(off, off[1:])):
        if a > b:
            return DECREASING, g
    if off[-1] > count:
        return PAST_END, len(off) - 1
    return OK, 0


def slice_len(cap, natural):
    """msm::slice_len with unit 1: the natural length unless the test hook caps it"""
    return natural if not cap else max(1, min(natural, cap))


def grids(groups, n_exp):
    return -(-groups // CHECK_THREADS), -(-groups // DIGEST_THREADS), -(-n_exp // EXP_THREADS)


def workspace(groups, n_exp, own_digests, own_exps, pair_table):
    """-> (head, digests, exps, pairs, total), regions rounded up to 256 bytes"""
    up = lambda v: (v + 255) // 256 * 256
    head, digests = 0, 256
    exps = digests + up(32 * groups if own_digests else 0)
    pairs = exps + up(32 * n_exp if own_exps else 0)
    return head, digests, exps, pairs, pairs + up(8 * groups if pair_table else 0)


def fixed_too_large(k, m, groups):
    """the fixed-shape forms: every group hashes k keys and owns m exponents (groups >= 1)"""
    return groups > 0x7FFFFFFF or m > 0xFFFFFFFF or m * groups > 0xFFFFFFF0 or k > (((1 << 64) - 1) >> 6) // groups


def fixed_priv_too_large(k, groups):
    return k * groups > 0xFFFFFFF0


def fixed_workspace(m, groups):
    """-> (digests, exps, total): the digests rounded up to 256 bytes, then groups x m exponents"""
    dg_bytes = (groups * 32 + 255) // 256 * 256
    return 0, dg_bytes, dg_bytes + groups * m * 32


def cut(pk_off, exp_off, cap):
    """[(lo, hi)]: the rule in words -- walk the groups; a group joins the current slice when the slice's groups, keys and
    exponents all stay within the cap with it, and otherwise starts the next; a slice's first group is taken whatever its
    size.  pk_off None: the keys do not count"""
    out, lo = [], 0
    groups = len(exp_off) - 1
    for g in range(groups):
        if g == lo:
            continue
        keys = pk_off[g + 1] - pk_off[lo] if pk_off is not None else 0
        if g + 1 - lo > cap or keys > cap or exp_off[g + 1] - exp_off[lo] > cap:
            out.append((lo, g))
            lo = g
    if groups:
        out.append((lo, groups))
    return out


def extent(pk_off, exp_off, slices):
    return (max((hi - lo for lo, hi in slices), default=0),
            max((pk_off[hi] - pk_off[lo] for lo, hi in slices), default=0) if pk_off is not None else 0,
            max((exp_off[hi] - exp_off[lo] for lo, hi in slices), default=0))


def rebase(off, lo, hi):
    return [v - off[lo] for v in off[lo:hi + 1]]


def offsets(lens):
    off = [0]
    for v in lens:
        off.append(off[-1] + v)
    return off


def hash_pks_ranges(pks_ser, pk_off, exp_off):
    """-> (digest bytes, exponent bytes): per group SHA256 of its keys, then SHA256(be32(i) || digest) mod n for its exponents"""
    dg, ts = [], []
    for g in range(len(pk_off) - 1):
        d = hashlib.sha256(pks_ser[48 * pk_off[g]:48 * pk_off[g + 1]]).digest()
        dg.append(d)
        for i in range(exp_off[g + 1] - exp_off[g]):
            ts.append((int.from_bytes(hashlib.sha256(i.to_bytes(4, "big") + d).digest(), "big") % N).to_bytes(32, "big"))
    return b"".join(dg), b"".join(ts)
