"""Signatures: G2 points, 96-byte compressed form (signature.py:21-38, 120-121)."""
from copy import deepcopy

from . import hostmath as H
from .bls12381 import n as GROUP_ORDER
from .ec import JacobianPoint, default_ec_twist


class Signature:
    SIGNATURE_SIZE = 96

    def __init__(self, value, aggregation_info=None):
        self.value = value
        self.aggregation_info = aggregation_info

    @staticmethod
    def from_bytes(buffer, aggregation_info=None):
        A = H.g2_decompress(bytes(buffer))
        return Signature(JacobianPoint._from(H.F2, H.aff_to_jac(H.F2, A), default_ec_twist), aggregation_info)

    @staticmethod
    def from_bytes_batch(buffers, aggregation_infos=None):
        """[Signature.from_bytes(b, info) ...] with all square roots in one GPU call
        (blsgpu_g2_decompress); ValueError on the first bad encoding."""
        from . import backend
        buffers = [bytes(b) for b in buffers]
        if any(len(b) != Signature.SIGNATURE_SIZE for b in buffers):
            raise ValueError("signatures are %d bytes" % Signature.SIGNATURE_SIZE)
        if not buffers:
            return []
        infos = aggregation_infos or [None] * len(buffers)
        out, ok = backend.get().g2_decompress(b"".join(buffers))
        if not all(ok):
            raise ValueError("No y for point x")
        return [Signature(JacobianPoint._from(H.F2, H.aff_to_jac(H.F2, H.g2_from_abi(out[192 * i:192 * (i + 1)])), default_ec_twist),
                          infos[i]) for i in range(len(buffers))]

    @staticmethod
    def from_g2(g2_el, aggregation_info=None):
        return Signature(g2_el, aggregation_info)

    @staticmethod
    def in_subgroup_batch(signatures):
        """[(sig.value * n).infinity for sig in signatures]: order-n subgroup membership of every signature point in one
        GPU call (blsgpu_g2_subgroup_check); points off the twist are decided by the host multiplication itself."""
        from .keys import _in_subgroup_batch
        return _in_subgroup_batch([sig.value for sig in signatures], H.g2_affine_bytes, "g2_subgroup")

    def set_aggregation_info(self, aggregation_info):
        self.aggregation_info = aggregation_info

    def get_aggregation_info(self):
        return self.aggregation_info

    def divide_by(self, divisor_signatures):
        """Remove already-verified parts from an aggregate (signature.py:44-103):
        each divisor must be a subset with unique (message, pk) pairs and a
        consistent exponent quotient."""
        drop = []
        prod = None
        for div in divisor_signatures:
            pks, mhs = div.aggregation_info.public_keys, div.aggregation_info.message_hashes
            if len(pks) != len(mhs):
                raise Exception("Invalid aggregation info")
            quotient = None
            for mh, pk in zip(mhs, pks):
                divisor = div.aggregation_info.tree[(mh, pk)]
                try:
                    dividend = self.aggregation_info.tree[(mh, pk)]
                except KeyError:
                    raise Exception("Signature is not a subset")
                qn = dividend * pow(divisor, GROUP_ORDER - 2, GROUP_ORDER) % GROUP_ORDER
                if quotient is None:
                    quotient = qn
                elif qn != quotient:
                    raise Exception("Cannot divide by aggregate signature,msg/pk pairs are not unique")
                drop.append((mh, pk))
            term = div.value * ((-quotient) % GROUP_ORDER) if quotient is not None else None
            if term is not None:
                prod = term if prod is None else prod + term
        value = self.value if prod is None else self.value + prod
        out = Signature(deepcopy(value), deepcopy(self.aggregation_info))
        for key in drop:
            out.aggregation_info.tree.pop(key, None)
        keys = sorted(out.aggregation_info.tree)
        out.aggregation_info.message_hashes = [k[0] for k in keys]
        out.aggregation_info.public_keys = [k[1] for k in keys]
        return out

    @staticmethod
    def divide_by_batch(dividends, divisor_lists):
        """[d.divide_by(ds) for d, ds in zip(dividends, divisor_lists)] with the quotient scalars of every divisor and the G2
        sums of every dividend in one device call (blsgpu_sig_divide through backend.extension("sig_divide")); without that
        extension it is the loop.  The host keeps the dictionary work: the tree lookups that pair the dividend's exponent
        with the divisor's for every entry, and the removal and re-sort of the tree.  Raises what the loop raises for the
        first failing dividend in input order: a dividend whose lookups fail ends the batch there -- the dividends before
        it are still checked on the device, since the loop would have met their errors first -- and is then handed to
        divide_by, which raises.  A dividend with a divisor exponent that is 0 mod n, with a point off the twist or with a
        point the 192-byte form cannot carry goes through divide_by as well."""
        from . import backend
        from .aggregation_info import AggregationInfo
        dividends, divisor_lists = list(dividends), [list(ds) for ds in divisor_lists]
        if len(dividends) != len(divisor_lists):
            raise ValueError("one list of divisors per dividend")
        fn = backend.extension("sig_divide")
        if fn is None or not dividends:
            return [d.divide_by(ds) for d, ds in zip(dividends, divisor_lists)]
        # the host pass: per dividend its points (own signature first), per divisor its entries' exponents
        pts, pt_off, ent_off, ea, eb, drops, fails_at = [], [0], [0], [], [], [], None
        for j, (sig, divs) in enumerate(zip(dividends, divisor_lists)):
            mine, rows, a, b, drop = [sig.value], [0], [], [], []
            try:
                own = sig.aggregation_info.tree
                for div in divs:
                    info = div.aggregation_info
                    if len(info.public_keys) != len(info.message_hashes):
                        raise LookupError
                    for key in zip(info.message_hashes, info.public_keys):
                        b.append(info.tree[key] % GROUP_ORDER)
                        a.append(own[key] % GROUP_ORDER)
                        drop.append(key)
                    if info.public_keys:                     # a divisor with no entries has no quotient: skipped, as in the loop
                        mine.append(div.value)
                        rows.append(len(info.public_keys))
            except Exception:                                # divide_by names it, after whatever the loop meets before it
                fails_at = j
                break
            pts += mine
            for r in rows:
                ent_off.append(ent_off[-1] + r)
            pt_off.append(len(pts))
            ea += a
            eb += b
            drops.append(drop)
        m = len(drops)
        out = [None] * m
        if m:
            affs = [P.to_affine()._aff() for P in pts]
            enc = [H.g2_affine_bytes(A) for A in affs]
            odd = [A is not None and e == bytes(192) for A, e in zip(affs, enc)]
            res, flag, status, _, _ = fn(b"".join(enc), pt_off, ent_off, ea, eb)
            for j in range(m):
                sig, lo, hi = dividends[j], pt_off[j], pt_off[j + 1]
                if flag[j] == 2 or 2 in status[lo:hi] or any(odd[lo:hi]):
                    out[j] = sig.divide_by(divisor_lists[j])
                    continue
                if 1 in status[lo:hi]:
                    raise Exception("Cannot divide by aggregate signature,msg/pk pairs are not unique")
                value = JacobianPoint._from(H.F2, None if flag[j] == 1 else H.aff_to_jac(H.F2, H.g2_from_abi(res[192 * j:192 * (j + 1)])),
                                            default_ec_twist)
                tree = deepcopy(sig.aggregation_info.tree)
                for key in drops[j]:
                    tree.pop(key, None)
                out[j] = Signature(value, AggregationInfo._from_tree(tree))
        if fails_at is not None:
            dividends[fails_at].divide_by(divisor_lists[fails_at])
            raise AssertionError("divide_by accepted what the lookups refused")
        return out

    def serialize(self):
        return self.value.serialize()

    def size(self):
        return self.SIGNATURE_SIZE

    def __eq__(self, other):
        return self.serialize() == other.serialize()

    def __hash__(self):
        return int.from_bytes(self.serialize(), "big")

    def __lt__(self, other):
        return self.serialize() < other.serialize()

    def __repr__(self):
        return "Signature(%s)" % self.serialize().hex()
