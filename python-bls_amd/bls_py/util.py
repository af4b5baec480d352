"""Hash helpers with the reference's constructions (util.py:7-50)."""
import hashlib


def _b(m):
    return m if isinstance(m, (bytes, bytearray)) else m.encode("utf-8")


def hash256(m):
    return hashlib.sha256(_b(m)).digest()


def hash256_batch(messages):
    """[hash256(m) for m in messages]; messages: bytes, bytearray, memoryview or str each.  A provider that offers a hash256
    extension (the list of bytes-like messages -> n x 32 digest bytes) gets the whole list in one call; without one -- the HIP
    provider has none yet, and the host provider of the CPU tests never will -- this is exactly that loop."""
    from . import backend
    ms = [m.encode("utf-8") if isinstance(m, str) else m for m in messages]
    fn = backend.extension("hash256") if ms else None
    if fn is None:
        return [hashlib.sha256(m).digest() for m in ms]
    out = fn(ms)
    return [out[32 * i:32 * (i + 1)] for i in range(len(ms))]


def hash512(m):
    m = bytes(_b(m))
    return hash256(m + b"\x00") + hash256(m + b"\x01")


def hmac256(m, k):
    """HMAC-SHA256 written out as the reference does (64-byte block, key hashed if longer)."""
    m, k = bytes(_b(m)), bytes(_b(k))
    if len(k) > 64:
        k = hash256(k)
    k = k.ljust(64, b"\x00")
    inner = hash256(bytes(c ^ 0x36 for c in k) + m)
    return hash256(bytes(c ^ 0x5c for c in k) + inner)


def hash_pks(num_outputs, public_keys):
    """t_i = sha256(be32(i) || sha256(ser(pk_0) || ser(pk_1) || ...)) mod n  (util.py:36-50)."""
    from .bls12381 import n
    digest = hash256(b"".join(pk.serialize() for pk in public_keys))
    return [int.from_bytes(hash256(i.to_bytes(4, "big") + digest), "big") % n for i in range(num_outputs)]


def hash_pks_batch(num_outputs, key_groups, ragged=False):
    """[hash_pks(num_outputs, g) for g in key_groups] with ONE device call per distinct group length (blsgpu_hash_pks: both
    SHA-256 steps and the reduction mod n on the GPU) when the provider has hash_pks; otherwise that loop.  Empty groups and
    num_outputs = 0 never reach the device.
    ragged=True: the same list from ONE call of the provider's hash_pks_ranges extension (blsgpu_hash_pks_ranges) whatever
    the lengths, empty groups included; NotImplementedError when the provider has none."""
    from . import backend
    key_groups = [list(g) for g in key_groups]
    if ragged:
        fn = backend.extension("hash_pks_ranges")
        if fn is None:
            raise NotImplementedError("the provider has no hash_pks_ranges extension")
        if not key_groups or num_outputs <= 0:
            return [[] for _ in key_groups]
        pk_off = [0]
        for g in key_groups:
            pk_off.append(pk_off[-1] + len(g))
        ts = fn(b"".join(pk.serialize() for g in key_groups for pk in g), pk_off, [num_outputs * j for j in range(len(key_groups) + 1)])
        return [[int.from_bytes(ts[32 * (j * num_outputs + i):32 * (j * num_outputs + i + 1)], "big") for i in range(num_outputs)]
                for j in range(len(key_groups))]
    fn = getattr(backend.get(), "hash_pks", None) if key_groups and num_outputs > 0 else None
    if fn is None:
        return [hash_pks(num_outputs, g) for g in key_groups]
    out = [None] * len(key_groups)
    buckets = {}
    for j, g in enumerate(key_groups):
        buckets.setdefault(len(g), []).append(j)
    for k, js in buckets.items():
        if k == 0:
            for j in js:
                out[j] = hash_pks(num_outputs, [])
            continue
        ts = fn(b"".join(pk.serialize() for j in js for pk in key_groups[j]), k, num_outputs, len(js))
        for q, j in enumerate(js):
            out[j] = [int.from_bytes(ts[32 * (q * num_outputs + i):32 * (q * num_outputs + i + 1)], "big") for i in range(num_outputs)]
    return out
