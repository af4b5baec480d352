"""Key types (keys.py:17-316 of the reference): PublicKey = G1 point with a
48-byte compressed form, PrivateKey = scalar mod n, and the HD keys
ExtendedPrivateKey / ExtendedPublicKey, whose children are derived on the GPU
many siblings at a time (blsgpu_hd_children) and whose descendants many whole
paths at a time, each from a parent of its own (blsgpu_hd_paths)."""
from copy import deepcopy
from random import SystemRandom

from . import hostmath as H
from .aggregation_info import AggregationInfo
from .bls12381 import n as GROUP_ORDER
from .ec import (JacobianPoint, default_ec, default_ec_twist, generator_Fq, hash_to_point_Fq2,
                 hash_to_point_prehashed_Fq2)
from .fields import Fq
from .signature import Signature
from .util import _b, hash256, hmac256

RNG = SystemRandom()


def _in_subgroup_batch(points, to_bytes, op):
    """[(P * n).infinity for P in points] (JacobianPoints; op: the provider's g1_subgroup or g2_subgroup): the device's status byte where it is 1 or 2 (on the curve,
    where [n] P is exact group arithmetic); the host's [n] P for a point off the curve and for one whose affine form is the
    all-zero encoding of infinity without being infinity"""
    from . import backend
    if not points:
        return []
    affs = [P.to_affine()._aff() for P in points]
    enc = [to_bytes(A) for A in affs]
    status = getattr(backend.get(), op)(b"".join(enc))
    zero = bytes(len(enc[0]))
    return [st == 1 if st and not (A is not None and e == zero) else (P * GROUP_ORDER).infinity
            for P, A, e, st in zip(points, affs, enc, status)]


class PublicKey:
    PUBLIC_KEY_SIZE = 48

    def __init__(self, value):
        self.value = value
        self._ser = None

    @staticmethod
    def from_bytes(buffer):
        A = H.g1_decompress(bytes(buffer))
        return PublicKey(JacobianPoint._from(H.F1, H.aff_to_jac(H.F1, A), default_ec))

    @staticmethod
    def from_bytes_batch(buffers):
        """[PublicKey.from_bytes(b) for b in buffers] with the square roots of all keys
        in one GPU call (blsgpu_g1_decompress); ValueError on the first bad encoding,
        as from_bytes raises."""
        from . import backend
        buffers = [bytes(b) for b in buffers]
        if any(len(b) != PublicKey.PUBLIC_KEY_SIZE for b in buffers):
            raise ValueError("public keys are %d bytes" % PublicKey.PUBLIC_KEY_SIZE)
        if not buffers:
            return []
        out, ok = backend.get().g1_decompress(b"".join(buffers))
        if not all(ok):
            raise ValueError("No y for point x")
        return [PublicKey(JacobianPoint._from(H.F1, H.aff_to_jac(H.F1, H.g1_from_abi(out[96 * i:96 * (i + 1)])), default_ec))
                for i in range(len(buffers))]

    @staticmethod
    def from_g1(g1_el):
        assert type(g1_el) is JacobianPoint
        return PublicKey(g1_el)

    @staticmethod
    def in_subgroup_batch(keys):
        """[(pk.value * n).infinity for pk in keys]: order-n subgroup membership of every key in one GPU call
        (blsgpu_g1_subgroup_check).  Keys off the curve (status 0) are decided by the host multiplication itself."""
        return _in_subgroup_batch([pk.value for pk in keys], H.g1_affine_bytes, "g1_subgroup")

    def serialize(self):
        if self._ser is None:
            self._ser = self.value.serialize()
        return self._ser

    def get_fingerprint(self):
        return int.from_bytes(hash256(self.serialize())[:4], "big")

    def size(self):
        return self.PUBLIC_KEY_SIZE

    def __eq__(self, other):
        return self.serialize() == other.serialize()

    def __hash__(self):
        return int.from_bytes(self.serialize(), "big")

    def __lt__(self, other):
        return self.serialize() < other.serialize()

    def __repr__(self):
        return "PublicKey(%s)" % self.serialize().hex()

    def __deepcopy__(self, memo):
        return PublicKey.from_g1(deepcopy(self.value, memo))


class PrivateKey:
    PRIVATE_KEY_SIZE = 32

    def __init__(self, value):
        self.value = int(value)

    @staticmethod
    def from_bytes(buffer):
        return PrivateKey(int.from_bytes(buffer, "big"))

    @staticmethod
    def from_seed(seed):
        return PrivateKey(int.from_bytes(hmac256(seed, b"BLS private key seed"), "big") % GROUP_ORDER)

    @staticmethod
    def from_seed_batch(seeds):
        """[PrivateKey.from_seed(s) for s in seeds] with the HMACs, the reduction mod n and the public keys on the GPU
        (blsgpu_keys_from_seeds): one call per distinct seed length, on a schedule that does not depend on the seeds, and
        every key comes back with its public key (get_public_key costs nothing).  A str seed is UTF-8 encoded as from_seed
        does.  Seeds longer than the device's limit, and every seed on a provider without the call, take from_seed."""
        seeds = [bytes(_b(s)) for s in seeds]
        out = []
        for seed, rec in zip(seeds, _keys_from_seeds(seeds, False)):
            if rec is None:
                out.append(PrivateKey.from_seed(seed))
                continue
            sk = PrivateKey.from_bytes(rec[0])
            sk.__dict__["_pk_point"] = _pk_from_device(rec[2], rec[3]).value
            out.append(sk)
        return out

    @staticmethod
    def new_threshold(T, N):
        """Joint-Feldman dealing (keys.py:92-117): a random degree T-1 polynomial,
        commitments g1*c_i and the N fragments P(1..N)."""
        assert 1 <= T <= N
        g1 = generator_Fq()
        poly = [Fq(GROUP_ORDER, RNG.randint(1, GROUP_ORDER - 1)) for _ in range(T)]
        commitments = [g1 * c for c in poly]
        fragments = [sum(c * pow(x, i, GROUP_ORDER) for i, c in enumerate(poly)) for x in range(1, N + 1)]
        return PrivateKey(poly[0]), commitments, fragments

    @staticmethod
    def new_threshold_batch(T, N, count, secret=False):
        """[PrivateKey.new_threshold(T, N) for _ in range(count)]: the coefficients drawn from RNG in the same order, the
        count x T commitments g1*c in one GPU call on the fixed-base table (blsgpu_g1_mul_gen), the fragments P(1..N)
        by Horner mod n on the host (as Fq(n, .) values).  secret=True: the same objects with commitments and fragments
        from ONE blsgpu_threshold_deal_secret call, whose sequence of instructions and addresses does not depend on the
        coefficients (a provider without it raises)."""
        from . import backend
        from .ec import AffinePoint
        assert 1 <= T <= N
        deal = _secret_call("threshold_deal_secret") if secret else None
        polys = [[RNG.randint(1, GROUP_ORDER - 1) for _ in range(T)] for _ in range(count)]
        if not polys:
            return []
        coeffs = b"".join(c.to_bytes(32, "big") for poly in polys for c in poly)
        if secret:
            aff, frag = deal(coeffs, T, b"".join(x.to_bytes(32, "big") for x in range(1, N + 1)))
        else:
            aff, _ = backend.get().g1_mul_gen(coeffs)
        out = []
        for d, poly in enumerate(polys):
            commitments = [AffinePoint._from(H.F1, H.g1_from_abi(aff[96 * (d * T + k):96 * (d * T + k + 1)]), default_ec)
                           for k in range(T)]
            fragments = []
            for x in range(1, N + 1):
                if secret:
                    acc = int.from_bytes(frag[32 * (d * N + x - 1):32 * (d * N + x)], "big")
                else:
                    acc = 0
                    for c in reversed(poly):
                        acc = (acc * x + c) % GROUP_ORDER
                fragments.append(Fq(GROUP_ORDER, acc))
            out.append((PrivateKey(poly[0]), commitments, fragments))
        return out

    def get_public_key(self):
        # sk G1 is one engine call (a scalar multiplication: ~2 ms with its round trip); the point is kept, a NEW PublicKey
        # object comes back every time as in keys.py:104-105 (callers that change `value` would lose the cache: __setattr__ below)
        pt = self.__dict__.get("_pk_point")
        if pt is None:
            pt = (self.value * generator_Fq()).to_jacobian()
            self.__dict__["_pk_point"] = pt
        return PublicKey.from_g1(pt)

    @staticmethod
    def get_public_key_batch(private_keys, secret=False):
        """[sk.get_public_key() for sk in private_keys] in one GPU call on the fixed-base table (blsgpu_g1_mul_gen);
        the keys come back with their serialisation.  secret=True: the same keys from blsgpu_g1_mul_gen_secret, whose
        sequence of instructions and addresses does not depend on the private keys (a provider without it raises)."""
        from . import backend
        sks = list(private_keys)
        if not sks:
            return []
        scalars = b"".join(sk.value.to_bytes(32, "big") for sk in sks)
        aff, ser = _secret_call("g1_mul_gen_secret")(scalars) if secret else backend.get().g1_mul_gen(scalars, None, 0)
        return [_pk_from_device(aff[96 * i:96 * (i + 1)], ser[48 * i:48 * (i + 1)]) for i in range(len(sks))]

    def __setattr__(self, name, v):
        if name == "value":
            self.__dict__.pop("_pk_point", None)
        object.__setattr__(self, name, v)

    def sign(self, m):
        # (one key, one message through the batched steps: three engine calls instead of a dozen -- 15.6 -> ~4 ms;
        # the same objects as keys.py:123-126 builds)
        return PrivateKey.sign_batch([self], [m])[0]

    @staticmethod
    def sign_batch(private_keys, messages):
        """[sk.sign(m) for sk, m in zip(private_keys, messages)] with the three heavy steps
        batched on the GPU: public keys sk*G1 (one group sum per key), H(m) (hash to G2)
        and sk*H(m) (one G2 group sum per message).  Same objects as keys.py:123-126 builds."""
        from . import backend
        from .ec import hash_to_points_prehashed_Fq2
        from .util import hash256
        sks = list(private_keys)
        hashes = [hash256(m) for m in messages]
        return PrivateKey._sign_hashes(sks, hashes)

    @staticmethod
    def _sign_hashes(sks, hashes):
        from . import backend
        from .ec import hash_to_points_prehashed_Fq2
        if len(sks) != len(hashes):
            raise ValueError("one message per key")
        if not sks:
            return []
        n = len(sks)
        prov = backend.get()
        g1 = H.g1_affine_bytes(H.G1_GEN)
        pk_bytes, pk_inf = prov.g1_msm(g1 * n, [sk.value for sk in sks], 1, n)
        Hm = hash_to_points_prehashed_Fq2(hashes)
        pts = b"".join(H.g2_affine_bytes(q._aff()) for q in Hm)
        sig_bytes, sig_inf = prov.g2_msm(pts, [sk.value for sk in sks], 1, n)
        out = []
        for i in range(n):
            pk = PublicKey.from_g1(JacobianPoint._from(
                H.F1, None if pk_inf[i] else H.aff_to_jac(H.F1, H.g1_from_abi(pk_bytes[96 * i:96 * (i + 1)])), default_ec))
            sig = JacobianPoint._from(
                H.F2, None if sig_inf[i] else H.aff_to_jac(H.F2, H.g2_from_abi(sig_bytes[192 * i:192 * (i + 1)])), default_ec_twist)
            out.append(Signature.from_g2(sig, AggregationInfo.from_msg_hash(pk, hashes[i])))
        return out

    def sign_prehashed(self, h):
        return PrivateKey._sign_hashes([self], [h])[0]

    @staticmethod
    def _sign_device(private_keys, hashes, aff, ser):
        """blsgpu_sign for the keys and their 32-byte hashes (a list with one entry per key, or ONE bytes object: every key
        signs it) -> (keys, hashes per key, affine bytes or None, serialised bytes or None)"""
        from . import backend
        sks = list(private_keys)
        if isinstance(hashes, (bytes, bytearray)):
            per_key, flat = [bytes(hashes)] * len(sks), bytes(hashes)
        else:
            per_key = [bytes(h) for h in hashes]
            if len(per_key) != len(sks):
                raise ValueError("one message per key")
            flat = b"".join(per_key)
        if any(len(h) != 32 for h in per_key) or (sks and len(flat) not in (32, 32 * len(sks))):
            raise ValueError("message hashes are 32 bytes")
        if not sks:
            return sks, per_key, b"", b""
        out_aff, out_ser = backend.get().sign(b"".join(sk.serialize() for sk in sks), flat, aff, ser)
        return sks, per_key, out_aff, out_ser

    @staticmethod
    def sign_prehashed_serialized_batch(private_keys, hashes):
        """[sk.sign_prehashed(h).serialize() for sk, h in zip(private_keys, hashes)] as 96-byte strings, in one GPU call
        (blsgpu_sign): hash to G2, the multiplication by the key on a schedule that does not depend on the key, and the
        compression all run on the device; no point object is built.  hashes: one 32-byte hash per key, or ONE bytes
        object that every key signs (a committee or threshold session: one hash, one shared table)."""
        _, _, _, ser = PrivateKey._sign_device(private_keys, hashes, False, True)
        return [ser[96 * i:96 * (i + 1)] for i in range(len(ser) // 96)]

    @staticmethod
    def sign_serialized_batch(private_keys, messages):
        """[sk.sign(m).serialize() for sk, m in zip(private_keys, messages)] as 96-byte strings (see
        sign_prehashed_serialized_batch); messages: one per key, or ONE bytes object that every key signs."""
        if isinstance(messages, (bytes, bytearray)):
            return PrivateKey.sign_prehashed_serialized_batch(private_keys, hash256(bytes(messages)))
        return PrivateKey.sign_prehashed_serialized_batch(private_keys, [hash256(m) for m in messages])

    @staticmethod
    def sign_batch_uniform(private_keys, messages, secret=False):
        """The Signature objects of sign_batch(private_keys, messages), AggregationInfo included, with the signature points
        from blsgpu_sign: the private keys meet only the scalar-independent G2 schedule there.  The public keys of the
        AggregationInfo come from get_public_key_batch: by default on the fixed-base G1 table that is indexed by the digits
        of the key -- that half is NOT scalar-independent -- and with secret=True from blsgpu_g1_mul_gen_secret, so that
        both halves run on schedules that do not depend on the keys."""
        hashes = [hash256(m) for m in messages]
        sks, hashes, aff, _ = PrivateKey._sign_device(private_keys, hashes, True, False)
        pks = PrivateKey.get_public_key_batch(sks, secret=secret)
        out = []
        for i, (pk, h) in enumerate(zip(pks, hashes)):
            sig = JacobianPoint._from(H.F2, H.aff_to_jac(H.F2, H.g2_from_abi(aff[192 * i:192 * (i + 1)])), default_ec_twist)
            out.append(Signature.from_g2(sig, AggregationInfo.from_msg_hash(pk, h)))
        return out

    def sign_threshold(self, m, player, players):
        from .threshold import Threshold
        assert player in players
        r = hash_to_point_Fq2(m).to_jacobian()
        lam = Threshold.lagrange_coeffs_at_zero(players)[players.index(player)]
        return Signature.from_g2(self.value * (r * lam))

    @staticmethod
    def sign_threshold_batch(private_keys, m, players, secret=False):
        """[sk.sign_threshold(m, p, players) for sk, p in zip(private_keys, players)]: the unit signatures of one session,
        the share of players[i] being private_keys[i].  One Lagrange evaluation for the session
        (Threshold.lagrange_coeffs_at_zero_batch: on the GPU), one hash to G2 and one grouped G2 sum of
        (lambda_i sk_i mod n) H(m) -- where every signer's own sign_threshold pays a full host Lagrange evaluation.
        secret=True: ONE blsgpu_sign_threshold call -- the coefficients, lambda_i sk_i mod n on masked arithmetic, the hash
        and the scalar-independent G2 multiplication, nothing returning to the host in between (a provider without it
        raises; so does a session of more than its LAGRANGE_MAX_K signers)."""
        from . import backend
        from .ec import hash_to_points_prehashed_Fq2
        from .threshold import Threshold
        from .util import hash256
        sks, players = list(private_keys), list(players)
        if len(sks) != len(players):
            raise ValueError("one private key per player")
        if secret:
            sign = _secret_call("sign_threshold")
            if not sks:
                return []
            assert len(set(players)) == len(players) and all(type(x) is int and 0 < x < GROUP_ORDER for x in players)
            if len(sks) > backend.get().LAGRANGE_MAX_K:
                raise ValueError("secret=True takes at most %d signers per session" % backend.get().LAGRANGE_MAX_K)
            out, _, inf, status = sign(b"".join(sk.serialize() for sk in sks), b"".join(x.to_bytes(32, "big") for x in players),
                                       len(sks), hash256(m), 1, True, False)
            assert status == b"\x01"
        else:
            if not sks:
                return []
            lam = Threshold.lagrange_coeffs_at_zero_batch([players])[0]
            r = H.g2_affine_bytes(hash_to_points_prehashed_Fq2([hash256(m)])[0]._aff())
            scalars = [int(l) * sk.value % GROUP_ORDER for l, sk in zip(lam, sks)]
            out, inf = backend.get().g2_msm(r * len(sks), scalars, 1, len(sks))
        return [Signature.from_g2(JacobianPoint._from(
            H.F2, None if inf[i] else H.aff_to_jac(H.F2, H.g2_from_abi(out[192 * i:192 * (i + 1)])), default_ec_twist))
            for i in range(len(sks))]

    def serialize(self):
        return self.value.to_bytes(self.PRIVATE_KEY_SIZE, "big")

    def size(self):
        return self.PRIVATE_KEY_SIZE

    def __lt__(self, other):
        return self.value < other.value

    def __eq__(self, other):
        return self.value == other.value

    def __hash__(self):
        return self.value

    def __repr__(self):
        return "PrivateKey(%s)" % hex(self.value)


def _pk_from_device(aff, ser):
    """PublicKey of the device's affine bytes, its 48-byte serialisation kept (no square root on the host)"""
    pk = PublicKey(JacobianPoint._from(H.F1, H.aff_to_jac(H.F1, H.g1_from_abi(aff)), default_ec))
    pk._ser = bytes(ser)
    return pk


def _keys_from_seeds(seeds, hd):
    """(key bytes, chain code|None, affine, serialised) per seed (bytes), in input order, from the provider's
    keys_from_seeds extension -- the seeds bucketed by length, one device call per distinct length; None for a seed longer
    than the device takes, and for every seed when the provider has no such extension"""
    from . import backend
    from ._native_seeds import SEED_MAX_BYTES
    out = [None] * len(seeds)
    fn = backend.extension("keys_from_seeds") if seeds else None
    if fn is None:
        return out
    buckets = {}
    for j, s in enumerate(seeds):
        if len(s) <= SEED_MAX_BYTES:
            buckets.setdefault(len(s), []).append(j)
    for length, js in buckets.items():
        sks, chain, aff, ser = fn(b"".join(seeds[j] for j in js), length, len(js), hd)[:4]
        for t, j in enumerate(js):
            out[j] = (sks[32 * t:32 * t + 32], chain[32 * t:32 * t + 32] if hd else None, aff[96 * t:96 * t + 96],
                      ser[48 * t:48 * t + 48])
    return out


def _secret_call(name):
    """the provider's scalar-independent form `name`; a provider without it raises -- secret=True never falls back to the
    digit-indexed path"""
    from . import backend
    fn = getattr(backend.get(), name, None)
    if fn is None:
        raise NotImplementedError("the provider has no %s: secret=True needs the scalar-independent device path" % name)
    return fn


def _pk_affine(pk):
    return H.g1_affine_bytes(H.jac_to_affine(H.F1, pk.value._jac()))


def _child_indices(indices):
    """the indices as ints; OverflowError outside 32 bits, as i.to_bytes(4, "big") of the reference raises"""
    out = [int(i) for i in indices]
    for i in out:
        if i < 0 or i >= 1 << 32:
            i.to_bytes(4, "big")
    return out


def _derive_paths(parents, parent_of, paths, priv, secret=False):
    """The leaves of paths[j] from parents[parent_of[j]] (extended keys; private derivation: ExtendedPrivateKeys) as
    (parent, path, chain code, key bytes|None, affine, serialised, parent fingerprint) per path, in input order; None for
    an empty path.  The reference's exceptions are raised before any device work; paths are bucketed by length, one
    blsgpu_hd_paths call per distinct length.  A provider without hd_paths gets None back: the caller chains single steps."""
    from . import backend
    parents = list(parents)
    paths = [[int(i) for i in p] for p in paths]
    flat = [i for p in paths for i in p]
    if not priv and flat and max(flat) >= 1 << 31:
        raise Exception("Cannot derive hardened children from public key")
    if flat and (min(flat) < 0 or max(flat) >= 1 << 32):
        _child_indices(flat)
    parent_of = [0] * len(paths) if parent_of is None else [int(a) for a in parent_of]
    if len(parent_of) != len(paths):
        raise ValueError("one parent index per path")
    if parent_of and (min(parent_of) < 0 or max(parent_of) >= len(parents)):
        raise IndexError("parent index out of range")
    room = [255 - k.depth for k in parents]
    if any(len(p) > room[a] for a, p in zip(parent_of, paths)):
        raise Exception("Cannot go further than 255 levels")
    prov = backend.get()
    if secret:
        derive = _secret_call("hd_paths_secret")
    elif not hasattr(prov, "hd_paths"):
        return None
    else:
        def derive(records, parent_of, paths):
            return prov.hd_paths(records, priv, parent_of, paths)
    out = [None] * len(paths)
    lengths = sorted({len(p) for p in paths} - {0})
    if not lengths:
        return out
    if priv:
        cold = [k.private_key for k in parents if k.private_key.__dict__.get("_pk_point") is None]
        for sk, pk in zip(cold, PrivateKey.get_public_key_batch(cold, secret=secret)):
            sk.__dict__["_pk_point"] = pk.value
        records = b"".join(k.chain_code + _pk_affine(k._public_key()) + k.private_key.serialize() for k in parents)
    else:
        records = b"".join(k.chain_code + _pk_affine(k.public_key) + bytes(32) for k in parents)
    for length in lengths:
        pos = range(len(paths)) if len(lengths) == 1 and all(paths) else [j for j, p in enumerate(paths) if len(p) == length]
        chain, sks, aff, ser, fps = derive(records, [parent_of[j] for j in pos], [paths[j] for j in pos])
        for t, j in enumerate(pos):
            out[j] = (parents[parent_of[j]], paths[j], chain[32 * t:32 * t + 32], sks[32 * t:32 * t + 32] if priv else None,
                      aff[96 * t:96 * t + 96], ser[48 * t:48 * t + 48], int.from_bytes(fps[4 * t:4 * t + 4], "big"))
    return out


def _fold(key, path, step):
    for i in path:
        key = getattr(key, step)(i)
    return key


class ExtendedPrivateKey:
    """HD private key (keys.py:167-255 of the reference).  private_child_batch / public_child_batch derive many
    siblings in one GPU call: both HMACs and the key multiplications of every child on the device."""
    version = 1
    EXTENDED_PRIVATE_KEY_SIZE = 77

    def __init__(self, version, depth, parent_fingerprint, child_number, chain_code, private_key):
        self.version = version
        self.depth = depth
        self.parent_fingerprint = parent_fingerprint
        self.child_number = child_number
        self.chain_code = chain_code
        self.private_key = private_key

    @staticmethod
    def from_seed(seed):
        i_left = hmac256(seed + bytes([0]), b"BLS HD seed")
        i_right = hmac256(seed + bytes([1]), b"BLS HD seed")
        sk_int = int.from_bytes(i_left, "big") % GROUP_ORDER
        sk = PrivateKey.from_bytes(sk_int.to_bytes(PrivateKey.PRIVATE_KEY_SIZE, "big"))
        return ExtendedPrivateKey(ExtendedPrivateKey.version, 0, 0, 0, i_right, sk)

    @staticmethod
    def from_seed_batch(seeds):
        """[ExtendedPrivateKey.from_seed(s) for s in seeds] with both HMACs, the reduction mod n and the public keys on the
        GPU (blsgpu_keys_from_seeds, hd form): one call per distinct seed length, on a schedule that does not depend on the
        seeds.  Every master comes back with its public key, so private_paths_from(masters, ..., secret=True) starts without
        a multiplication of its own.  A str seed raises TypeError as from_seed does (it concatenates bytes), before any
        device work.  Seeds longer than the device's limit, and every seed on a provider without the call, take from_seed."""
        seeds = [bytes(s + b"") for s in seeds]
        out = []
        for seed, rec in zip(seeds, _keys_from_seeds(seeds, True)):
            if rec is None:
                out.append(ExtendedPrivateKey.from_seed(seed))
                continue
            sk = PrivateKey.from_bytes(rec[0])
            pk = _pk_from_device(rec[2], rec[3])
            sk.__dict__["_pk_point"] = pk.value                 # the cache get_public_key fills (same point)
            master = ExtendedPrivateKey(ExtendedPrivateKey.version, 0, 0, 0, rec[1], sk)
            master.__dict__["_pk"] = pk
            out.append(master)
        return out

    def private_child(self, i):
        return self.private_child_batch([i])[0]

    def private_child_batch(self, indices, secret=False):
        """[self.private_child(i) for i in indices] in one GPU call (blsgpu_hd_children, private mode); hardened and
        non-hardened indices may be mixed.  secret=True: the same children as paths of depth 1 on blsgpu_hd_paths_secret,
        whose sequence of instructions and addresses does not depend on the keys."""
        from . import backend
        if self.depth >= 255:
            raise Exception("Cannot go further than 255 levels")
        idx = _child_indices(indices)
        if not idx:
            return []
        if secret:
            return ExtendedPrivateKey.private_paths_from([self], None, [[i] for i in idx], secret=True)
        pk = self.private_key.get_public_key()
        chain, sks, aff, ser = backend.get().hd_children(self.chain_code, _pk_affine(pk), self.private_key.serialize(), idx)
        fp = pk.get_fingerprint()
        out = []
        for j, i in enumerate(idx):
            sk = PrivateKey.from_bytes(sks[32 * j:32 * (j + 1)])
            child_pk = _pk_from_device(aff[96 * j:96 * (j + 1)], ser[48 * j:48 * (j + 1)])
            sk.__dict__["_pk_point"] = child_pk.value          # the cache get_public_key fills (same point)
            child = ExtendedPrivateKey(ExtendedPrivateKey.version, self.depth + 1, fp, i, chain[32 * j:32 * (j + 1)], sk)
            child.__dict__["_pk"] = child_pk
            out.append(child)
        return out

    def public_child(self, i):
        return self.private_child(i).get_extended_public_key()

    def public_child_batch(self, indices):
        """[self.public_child(i) for i in indices] in one GPU call"""
        return [c.get_extended_public_key() for c in self.private_child_batch(indices)]

    def private_path_batch(self, paths, secret=False):
        """[the fold of private_child over p for p in paths]: whole paths, every level on the GPU, in one call per
        distinct path length (blsgpu_hd_paths, private mode).  Hardened and non-hardened indices may be mixed; an empty
        path gives a key equal to self.  secret=True: on blsgpu_hd_paths_secret (see private_paths_from)."""
        paths = list(paths)
        return ExtendedPrivateKey.private_paths_from([self], [0] * len(paths), paths, secret=secret)

    def public_path_batch(self, paths):
        """[k.get_extended_public_key() for k in self.private_path_batch(paths)]"""
        return [c.get_extended_public_key() for c in self.private_path_batch(paths)]

    @staticmethod
    def private_paths_from(parents, parent_of, paths, secret=False):
        """[the fold of private_child over paths[j] from parents[parent_of[j]]]: the paths of many parents in one GPU call
        per distinct path length (blsgpu_hd_paths) -- the m/a/i grid is parent_of = [a ...], paths = [[i] ...].
        secret=True: every level on blsgpu_hd_paths_secret and the parents' own public keys on blsgpu_g1_mul_gen_secret --
        the sequence of instructions and addresses does not depend on the keys; a provider without them raises."""
        parents, paths = list(parents), [list(p) for p in paths]
        got = _derive_paths(parents, parent_of, paths, True, secret)
        if parent_of is None:
            parent_of = [0] * len(paths)
        if got is None:
            return [_fold(parents[a], p, "private_child") if p else ExtendedPrivateKey._copy(parents[a]) for a, p in zip(parent_of, paths)]
        out = []
        for a, rec in zip(parent_of, got):
            if rec is None:
                out.append(ExtendedPrivateKey._copy(parents[a]))
                continue
            parent, path, chain, skb, aff, ser, fp = rec
            sk = PrivateKey.from_bytes(skb)
            child_pk = _pk_from_device(aff, ser)
            sk.__dict__["_pk_point"] = child_pk.value          # the cache get_public_key fills (same point)
            child = ExtendedPrivateKey(ExtendedPrivateKey.version, parent.depth + len(path), fp, path[-1], chain, sk)
            child.__dict__["_pk"] = child_pk
            out.append(child)
        return out

    @staticmethod
    def _copy(k):
        return ExtendedPrivateKey(k.version, k.depth, k.parent_fingerprint, k.child_number, k.chain_code, k.private_key)

    def _public_key(self):
        pk = self.__dict__.get("_pk")
        if pk is None or pk.value is not self.private_key.__dict__.get("_pk_point"):
            return self.private_key.get_public_key()
        out = PublicKey(pk.value)
        out._ser = pk._ser
        return out

    def get_extended_public_key(self):
        # the reference serialises and parses back (keys.py:222-229): the same fields, without the square root of from_bytes
        return ExtendedPublicKey(int.from_bytes(self.version.to_bytes(4, "big"), "big"), self.depth, self.parent_fingerprint,
                                 self.child_number, self.chain_code, self._public_key())

    def get_private_key(self):
        return self.private_key

    def get_public_key(self):
        return self.private_key.get_public_key()

    def size(self):
        return self.EXTENDED_PRIVATE_KEY_SIZE

    def serialize(self):
        return (self.version.to_bytes(4, "big") + bytes([self.depth]) + self.parent_fingerprint.to_bytes(4, "big") +
                self.child_number.to_bytes(4, "big") + self.chain_code + self.private_key.serialize())

    def __eq__(self, other):
        return self.serialize() == other.serialize()

    def __hash__(self):
        return int.from_bytes(self.serialize(), "big")


class ExtendedPublicKey:
    """HD public key (keys.py:258-316 of the reference); public_child_batch derives many siblings in one GPU call."""
    EXTENDED_PUBLIC_KEY_SIZE = 93

    def __init__(self, version, depth, parent_fingerprint, child_number, chain_code, public_key):
        self.version = version
        self.depth = depth
        self.parent_fingerprint = parent_fingerprint
        self.child_number = child_number
        self.chain_code = chain_code
        self.public_key = public_key

    @staticmethod
    def from_bytes(serialized):
        version = int.from_bytes(serialized[:4], "big")
        depth = int.from_bytes(serialized[4:5], "big")
        parent_fingerprint = int.from_bytes(serialized[5:9], "big")
        child_number = int.from_bytes(serialized[9:13], "big")
        chain_code = serialized[13:45]
        public_key = PublicKey.from_bytes(serialized[45:])
        return ExtendedPublicKey(version, depth, parent_fingerprint, child_number, chain_code, public_key)

    def public_child(self, i):
        return self.public_child_batch([i])[0]

    def public_child_batch(self, indices):
        """[self.public_child(i) for i in indices] in one GPU call (blsgpu_hd_children, public mode)."""
        from . import backend
        if self.depth >= 255:
            raise Exception("Cannot go further than 255 levels")
        idx = [int(i) for i in indices]
        if any(i >= 1 << 31 for i in idx):
            raise Exception("Cannot derive hardened children from public key")
        idx = _child_indices(idx)
        if not idx:
            return []
        chain, _, aff, ser = backend.get().hd_children(self.chain_code, _pk_affine(self.public_key), None, idx)
        fp = self.public_key.get_fingerprint()
        return [ExtendedPublicKey(self.version, self.depth + 1, fp, i, chain[32 * j:32 * (j + 1)],
                                  _pk_from_device(aff[96 * j:96 * (j + 1)], ser[48 * j:48 * (j + 1)]))
                for j, i in enumerate(idx)]

    def public_path_batch(self, paths):
        """[the fold of public_child over p for p in paths]: whole paths, every level on the GPU, in one call per
        distinct path length (blsgpu_hd_paths, public mode); an empty path gives a key equal to self."""
        paths = list(paths)
        return ExtendedPublicKey.public_paths_from([self], [0] * len(paths), paths)

    @staticmethod
    def public_paths_from(parents, parent_of, paths):
        """[the fold of public_child over paths[j] from parents[parent_of[j]]]: the paths of many parents in one GPU call
        per distinct path length (blsgpu_hd_paths) -- the m/a/i grid is parent_of = [a ...], paths = [[i] ...]."""
        parents, paths = list(parents), [list(p) for p in paths]
        got = _derive_paths(parents, parent_of, paths, False)
        if parent_of is None:
            parent_of = [0] * len(paths)
        if got is None:
            return [_fold(parents[a], p, "public_child") if p else ExtendedPublicKey._copy(parents[a]) for a, p in zip(parent_of, paths)]
        out = []
        for a, rec in zip(parent_of, got):
            if rec is None:
                out.append(ExtendedPublicKey._copy(parents[a]))
                continue
            parent, path, chain, _, aff, ser, fp = rec
            out.append(ExtendedPublicKey(parent.version, parent.depth + len(path), fp, path[-1], chain, _pk_from_device(aff, ser)))
        return out

    @staticmethod
    def _copy(k):
        return ExtendedPublicKey(k.version, k.depth, k.parent_fingerprint, k.child_number, k.chain_code, k.public_key)

    def get_public_key(self):
        return self.public_key

    def size(self):
        return self.EXTENDED_PUBLIC_KEY_SIZE

    def serialize(self):
        return (self.version.to_bytes(4, "big") + bytes([self.depth]) + self.parent_fingerprint.to_bytes(4, "big") +
                self.child_number.to_bytes(4, "big") + self.chain_code + self.public_key.serialize())

    def __eq__(self, other):
        return self.serialize() == other.serialize()

    def __hash__(self):
        return int.from_bytes(self.serialize(), "big")
