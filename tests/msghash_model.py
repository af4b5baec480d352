"""Python model of csrc/msghash_plan.h: the validation of an offset table, the cut of a host-buffer call into staged slices on
message boundaries, the blocks per message, the grid and the workspace of the fused calls.  tests/test_msghash_plan_host.py holds
the header, compiled for the host, against it.  padding_list() is the message list a device test of the kernel is to hash:
every padding shape at every start residue."""
import hashlib
import random

LANES = 256
MAX_LEN = 1 << 32
OK, DECREASING, TOO_LONG, PAST_END = 0, 1, 2, 3

# every length at which the padding changes shape (55 / 56, 119 / 120, 183 / 184: one block more), the dword and block edges
# around them, and one long message
PAD_LENGTHS = [0, 1, 3, 4, 5, 31, 32, 33, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 121, 127, 128, 129, 183, 184, 1000]


def blocks(length):
    """SHA-256 compressions of a message: the padded length (0x80, zeros, 8 bytes of bit length) in 64-byte blocks"""
    return (length + 1 + 8 + 63) // 64


def grid(n):
    return -(-n // LANES)


def lengths(off):
    return [b - a for a, b in zip(off, off[1:])]


def validate(off, msgs_bytes):
    """-> (verdict, where): message by message a step down or a length of 2^32 or more, then the last offset"""
    for i, (a, b) in enumerate(zip(off, off[1:])):
        if a > b:
            return DECREASING, i
        if b - a >= MAX_LEN:
            return TOO_LONG, i
    if len(off) > 1 and off[-1] > msgs_bytes:
        return PAST_END, len(off) - 1
    return OK, 0


def cut(off, target, max_msgs):
    """[(lo, hi)]: the rule in words -- walk the messages; an empty one joins the current slice; one with bytes joins it when
    the slice holds no byte yet or stays within the target with it, and otherwise starts the next; a slice of max_msgs messages
    is full whatever comes"""
    out, cur, held = [], [], 0
    for i, length in enumerate(lengths(off)):
        fits = length == 0 or held == 0 or held + length <= target
        if cur and (len(cur) == max_msgs or not fits):
            out.append((cur[0], cur[-1] + 1))
            cur, held = [], 0
        cur.append(i)
        held += length
    if cur:
        out.append((cur[0], cur[-1] + 1))
    return out


def extent(off, slices):
    return (max((hi - lo for lo, hi in slices), default=0), max((off[hi] - off[lo] for lo, hi in slices), default=0))


def workspace(n_msg, caller_takes_digests):
    """-> (offset of the digests, total bytes), regions rounded up to 256 bytes"""
    return 0, 0 if caller_takes_digests else (32 * n_msg + 255) // 256 * 256


def message(length, tag):
    """`length` bytes that depend on (length, tag) and hold no run of equal bytes"""
    return random.Random(length * 1009 + tag).randbytes(length)


def offsets(msgs, start=0):
    off = [start]
    for m in msgs:
        off.append(off[-1] + len(m))
    return off


def padding_list():
    """Every PAD_LENGTHS length at every start residue off & 3 of the packed buffer, brought there by one-to-three-byte filler
    messages that are messages of the list themselves -> (messages, {(length, residue)} covered)"""
    msgs, covered, at = [], set(), 0
    for length in PAD_LENGTHS:
        for r in range(4):
            fill = (r - at) % 4
            if fill:
                msgs.append(message(fill, 7000 + len(msgs)))
                at += fill
            assert at % 4 == r
            msgs.append(message(length, r))
            covered.add((length, r))
            at += length
    return msgs, covered


def digests(msgs):
    return b"".join(hashlib.sha256(m).digest() for m in msgs)
