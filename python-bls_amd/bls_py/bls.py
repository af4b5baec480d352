"""Scheme API (bls.py of the reference): aggregation and verification.

`verify` is the GPU hot path: it assembles Ps = [-G1] + per-message key sums and
Qs = [signature] + H(m) exactly as bls.py:153-201 does and hands them to the
multi-pairing engine.  The group sums (signature aggregation, per-message key
folding, aggregate public keys) are GPU multi-scalar sums as well."""
import secrets

from . import hostmath as H
from .aggregation_info import AggregationInfo
from .bls12381 import n as GROUP_ORDER
from .ec import (AffinePoint, JacobianPoint, default_ec, generator_Fq,
                 hash_to_points_prehashed_Fq2)
from .fields import Fq12
from .keys import PrivateKey, PublicKey
from .pairing import ate_pairing_multi
from .signature import Signature
from .util import hash_pks


from . import backend


def _g2_sum(points, scalars=None):
    """sum_i scalars[i] * points[i] (JacobianPoint over Fq2) on the GPU."""
    if not points:
        return JacobianPoint._from(H.F2, None)
    pts = b"".join(H.g2_affine_bytes(p.to_affine()._aff()) for p in points)
    out, inf = backend.get().g2_msm(pts, scalars, len(points), 1)
    return JacobianPoint._from(H.F2, None if inf[0] else H.aff_to_jac(H.F2, H.g2_from_abi(out)))


def _g1_sums(groups_of_points, groups_of_scalars):
    """One G1 multi-scalar sum per group (ragged groups are padded with infinity)."""
    if not groups_of_points:
        return []
    k = max(len(g) for g in groups_of_points)
    pts, sc = bytearray(), []
    for g, s in zip(groups_of_points, groups_of_scalars):
        for p in g:
            pts += H.g1_affine_bytes(p.to_affine()._aff())
        pts += bytes(96) * (k - len(g))
        sc += [int(x) for x in s] + [0] * (k - len(g))
    out, inf = backend.get().g1_msm(bytes(pts), sc, k, len(groups_of_points))
    return [JacobianPoint._from(H.F1, None if inf[i] else H.aff_to_jac(H.F1, H.g1_from_abi(out[96 * i:96 * (i + 1)])))
            for i in range(len(groups_of_points))]


def _jac_g1_bytes(J):
    """affine bytes (x || y, (0,0) for infinity) of a G1 JacobianPoint; no inversion when z = 1"""
    if J.infinity:
        return bytes(96)
    if J.z.Z == 1:
        return int(J.x.Z).to_bytes(48, "big") + int(J.y.Z).to_bytes(48, "big")
    return H.g1_affine_bytes(J.to_affine()._aff())


def _g1_group_sums(prov, groups):
    """[(affine bytes, is_infinity) of sum_j s_j P_j] for groups of (P bytes, scalar) pairs: one g1_msm per power-of-two
    group length (padded with infinity), so that one long group does not pad every other to its length"""
    out = [None] * len(groups)
    by_len = {}
    for j, g in enumerate(groups):
        by_len.setdefault(1 << (len(g) - 1).bit_length(), []).append(j)
    for k, js in by_len.items():
        pts, sc = bytearray(), []
        for j in js:
            for b, s in groups[j]:
                pts += b
                sc.append(s)
            pts += bytes(96) * (k - len(groups[j]))
            sc += [0] * (k - len(groups[j]))
        res, inf = prov.g1_msm(bytes(pts), sc, k, len(js))
        for q, j in enumerate(js):
            out[j] = (res[96 * q:96 * (q + 1)], inf[q])
    return out


class BLS:
    @staticmethod
    def aggregate_sigs_simple(signatures):
        """Plain sum; NOT safe for signatures over one message (rogue keys)."""
        return Signature.from_g2(_g2_sum([sig.value for sig in signatures]))

    @staticmethod
    def aggregate_sigs_secure(signatures, public_keys, message_hashes):
        if not (len(signatures) == len(public_keys) == len(message_hashes)):
            raise Exception("Invalid number of keys")
        ordered = sorted(zip(message_hashes, public_keys, signatures))
        ts = hash_pks(len(public_keys), public_keys)
        return Signature.from_g2(_g2_sum([sig.value for _, _, sig in ordered], ts))

    @staticmethod
    def aggregate_sigs(signatures):
        infos = []
        for sig in signatures:
            if sig.aggregation_info is None or sig.aggregation_info.empty():
                raise Exception("Each signature must have a valid aggregation info")
            infos.append(sig.aggregation_info)
        colliding = AggregationInfo._colliding_messages(infos)
        if not colliding:
            out = BLS.aggregate_sigs_simple(signatures)
            out.set_aggregation_info(AggregationInfo.merge_infos(infos))
            return out
        hit = [s for s in signatures if any(m in colliding for m in s.aggregation_info.message_hashes)]
        rest = [s for s in signatures if not any(m in colliding for m in s.aggregation_info.message_hashes)]
        hit.sort(key=lambda s: s.aggregation_info)
        keys = sorted((mh, pk) for s in hit
                      for mh, pk in zip(s.aggregation_info.message_hashes, s.aggregation_info.public_keys))
        ts = hash_pks(len(hit), [pk for _, pk in keys])
        out = Signature.from_g2(_g2_sum([s.value for s in hit] + [s.value for s in rest], ts + [1] * len(rest)))
        out.set_aggregation_info(AggregationInfo.merge_infos(infos))
        return out

    @staticmethod
    def verify(signature):
        info = signature.aggregation_info
        by_message = {}
        for mh, pk in zip(info.message_hashes, info.public_keys):
            by_message.setdefault(mh, []).append(pk)
        key_groups, exp_groups = [], []
        for mh, keys in by_message.items():
            uniq = list(set(keys))
            try:
                exp_groups.append([info.tree[(mh, pk)] for pk in uniq])
            except KeyError:
                return False
            key_groups.append([pk.value for pk in uniq])
        prov = backend.get()
        # (an infinity SIGNATURE keeps the tuple path: its flag is the one flag the reference's Miller loop reads)
        if hasattr(prov, "verify_pipeline") and not signature.value.infinity and all(len(m) == 32 for m in by_message):
            return BLS._verify_on_device(prov, signature, list(by_message), key_groups, exp_groups)
        Qs = hash_to_points_prehashed_Fq2(list(by_message))
        Ps = [t.to_affine() for t in _g1_sums(key_groups, exp_groups)]
        neg_g1 = generator_Fq() * (GROUP_ORDER - 1)
        res = ate_pairing_multi([neg_g1] + Ps, [signature.value.to_affine()] + Qs, default_ec)
        return res == Fq12.one(default_ec.q)

    _NEG_G1 = None

    @staticmethod
    def _verify_on_device(prov, signature, hashes, key_groups, exp_groups):
        """The same Ps / Qs as above (bls.py:177-199), assembled as bytes and left on the GPU between hash-to-G2, the
        per-message key sums and the multi-pairing (HipProvider.verify_pipeline): no Python point objects per pair."""
        if BLS._NEG_G1 is None:
            BLS._NEG_G1 = H.g1_affine_bytes((generator_Fq() * (GROUP_ORDER - 1))._aff())
        n = len(hashes)
        sig = H.g2_affine_bytes(signature.value.to_affine()._aff())
        if all(len(g) == 1 and e[0] % GROUP_ORDER == 1 for g, e in zip(key_groups, exp_groups)):
            # one key with exponent 1 per message (a plain aggregate): the key itself is the pairing's P
            keys = b"".join(_jac_g1_bytes(g[0]) for g in key_groups)
            out = prov.verify_pipeline(BLS._NEG_G1, sig, b"".join(hashes), n, keys_affine=keys)
        else:
            k = max(len(g) for g in key_groups)
            pts, sc = bytearray(), bytearray()
            for g, e in zip(key_groups, exp_groups):
                for p, x in zip(g, e):
                    pts += _jac_g1_bytes(p)
                    sc += (int(x) % GROUP_ORDER).to_bytes(32, "big")
                pts += bytes(96) * (k - len(g))
                sc += bytes(32) * (k - len(g))
            out = prov.verify_pipeline(BLS._NEG_G1, sig, b"".join(hashes), n, key_pts=bytes(pts), key_scalars=bytes(sc), k=k)
        return out == Fq12.one(default_ec.q).serialize()

    @staticmethod
    def verify_batch(signatures, ragged=False, fused=False):
        """[BLS.verify(s) for s in signatures] with every GPU step batched across the
        signatures: one hash-to-G2 call for all distinct (signature, message) pairs, one call
        for all per-message key sums, and blsgpu_pairing_multi_batch per distinct pair count
        (independent multi-pairings side by side).  Same results as verify, one by one.
        ragged=True: ONE pair list with one range per aggregate and one call of the pairing_multi_ranges
        extension (blsgpu_pairing_multi_ranges) in place of the call per distinct pair count; a provider
        without the extension raises.  Not the default: which is faster is measured by
        tools/pair_ranges_probe.py, and routing is a later decision.
        fused=True: after the dictionary work per signature, ONE call of the verify_aggregates extension
        (blsgpu_verify_aggregates) for all signatures whose tree holds their keys: the distinct message hashes
        of the whole batch, every key as affine bytes, the exponents (None when every one is 1 mod n) and the
        three tables go up once; hash to G2, the key sums, the multi-pairings and the comparison with one stay
        on the device.  A signature that comes back undecided (status 2: an infinity signature, a key off the
        curve) and one with a message hash that is not 32 bytes are decided by BLS.verify.  A provider without
        the extension raises.  Not the default either: tools/verify_aggregates_probe.py measures it."""
        from . import backend
        prov = backend.get()
        fused_fn = None
        if fused:
            fused_fn = backend.extension("verify_aggregates")
            if fused_fn is None:
                raise NotImplementedError("verify_batch(fused=True) needs a provider with the verify_aggregates extension")
        ranges_fn = None
        if ragged:
            ranges_fn = backend.extension("pairing_multi_ranges")
            if ranges_fn is None:
                raise NotImplementedError("verify_batch(ragged=True) needs a provider with the pairing_multi_ranges extension")
        ONE = Fq12.one(default_ec.q).serialize()
        results = [None] * len(signatures)
        plans = []                                        # (index, message hashes, key groups, exponent groups)
        for i, sig in enumerate(signatures):
            info = sig.aggregation_info
            by_message = {}
            for mh, pk in zip(info.message_hashes, info.public_keys):
                by_message.setdefault(mh, []).append(pk)
            kg, eg = [], []
            try:
                for mh, keys in by_message.items():
                    uniq = list(set(keys))
                    eg.append([info.tree[(mh, pk)] for pk in uniq])
                    kg.append([pk.value for pk in uniq])
            except KeyError:
                results[i] = False                        # bls.py:189-190
                continue
            plans.append((i, list(by_message), kg, eg))
        if not plans:
            return results
        if fused:
            return BLS._verify_batch_fused(fused_fn, signatures, plans, results)
        all_hashes = [mh for _, mhs, _, _ in plans for mh in mhs]
        Qs = hash_to_points_prehashed_Fq2(all_hashes)
        Ps = _g1_sums([g for _, _, kg, _ in plans for g in kg], [e for _, _, _, eg in plans for e in eg])
        neg_g1 = H.g1_affine_bytes((generator_Fq() * (GROUP_ORDER - 1))._aff())
        if ragged:
            # -G1 / sig first, then the per-message keys and hashes, aggregate after aggregate: one range each
            g1s, g2s, ranges, pos = [], [], [], 0
            for i, mhs, _, _ in plans:
                k = len(mhs)
                g1s.append(neg_g1 + b"".join(H.g1_affine_bytes(p.to_affine()._aff()) for p in Ps[pos:pos + k]))
                g2s.append(H.g2_affine_bytes(signatures[i].value.to_affine()._aff()) +
                           b"".join(H.g2_affine_bytes(q._aff()) for q in Qs[pos:pos + k]))
                lo = ranges[-1][1] if ranges else 0
                ranges.append((lo, lo + k + 1))
                pos += k
            out = ranges_fn(b"".join(g1s), b"".join(g2s), ranges)
            for j, (i, _, _, _) in enumerate(plans):
                results[i] = out[576 * j:576 * (j + 1)] == ONE
            return results
        by_size, pos = {}, 0
        for i, mhs, _, _ in plans:
            k = len(mhs)
            g1 = neg_g1 + b"".join(H.g1_affine_bytes(p.to_affine()._aff()) for p in Ps[pos:pos + k])
            g2 = H.g2_affine_bytes(signatures[i].value.to_affine()._aff()) + \
                b"".join(H.g2_affine_bytes(q._aff()) for q in Qs[pos:pos + k])
            pos += k
            by_size.setdefault(k + 1, []).append((i, g1, g2))
        for size, items in by_size.items():
            out = prov.pairing_multi_batch(b"".join(x[1] for x in items), b"".join(x[2] for x in items), size, len(items))
            for j, (i, _, _) in enumerate(items):
                results[i] = out[576 * j:576 * (j + 1)] == ONE
        return results

    @staticmethod
    def _verify_batch_fused(fused_fn, signatures, plans, results):
        """verify_batch(fused=True) behind the dictionary work: the tables of ONE verify_aggregates call, its status bytes"""
        from ._native_veragg import tables
        msgs, keys, exps, shapes, sigs, sent = {}, [], [], [], [], []
        for i, mhs, kg, eg in plans:
            if not all(len(mh) == 32 for mh in mhs):
                continue
            shapes.append([(msgs.setdefault(mh, len(msgs)), len(g)) for mh, g in zip(mhs, kg)])
            for g, e in zip(kg, eg):
                keys += [_jac_g1_bytes(p) for p in g]
                exps += [int(x) % GROUP_ORDER for x in e]
            sigs.append(H.g2_affine_bytes(signatures[i].value.to_affine()._aff()))
            sent.append(i)
        if sent:
            status, _ = fused_fn(b"".join(sigs), b"".join(msgs), b"".join(keys), None if all(x == 1 for x in exps) else exps,
                                 *tables(shapes))
            for i, st in zip(sent, status):
                if st != 2:
                    results[i] = st == 1
        for i, _, _, _ in plans:
            if results[i] is None:
                results[i] = BLS.verify(signatures[i])
        return results

    @staticmethod
    def verify_batch_randomized(signatures, rng=None):
        """verify_batch(signatures) by a random linear combination: ONE multi-pairing of (distinct messages + 1) pairs
        decides every eligible signature, e(-G1, sum r_i sig_i) * prod_m e(sum_i r_i P_im, H(m)) == 1, with r_i drawn
        uniformly from [1, 2^64) (rng.getrandbits(64), in the order of the list; default secrets.SystemRandom()).
        Eligible: a signature point in G2 and not infinity, every key in G1, 32-byte message hashes, every per-message
        key sum P_im and every H(m) not infinity.  The others, and all eligible ones if the product
        is not 1, are decided by verify_batch in the same call.  The answers equal verify_batch's except that an invalid
        eligible signature is reported True with probability at most 1 / (2^64 - 1)."""
        prov = backend.get()
        rng = rng or secrets.SystemRandom()
        results = [None] * len(signatures)
        plans = []                                        # (index, message hashes, key groups (PublicKey), exponent groups)
        for i, sig in enumerate(signatures):
            info = sig.aggregation_info
            by_message = {}
            for mh, pk in zip(info.message_hashes, info.public_keys):
                by_message.setdefault(mh, []).append(pk)
            kg, eg = [], []
            try:
                for mh, keys in by_message.items():
                    uniq = list(set(keys))
                    eg.append([info.tree[(mh, pk)] for pk in uniq])
                    kg.append(uniq)
            except KeyError:
                results[i] = False                        # bls.py:189-190
                continue
            plans.append((i, list(by_message), kg, eg))
        elig = [p for p in plans if not signatures[p[0]].value.infinity and all(len(mh) == 32 for mh in p[1])]

        # subgroup membership: the distinct keys, the signature points (one device call each)
        sig_bytes = [H.g2_affine_bytes(signatures[p[0]].value.to_affine()._aff()) for p in elig]
        if elig:
            st = prov.g2_subgroup(b"".join(sig_bytes))
            keep = [st[j] == 1 and any(sig_bytes[j]) for j in range(len(elig))]
            elig, sig_bytes = [p for p, k in zip(elig, keep) if k], [b for b, k in zip(sig_bytes, keep) if k]
        key_bytes = {}
        for p in elig:
            for g in p[2]:
                for pk in g:
                    if pk not in key_bytes:
                        key_bytes[pk] = _jac_g1_bytes(pk.value)
        if key_bytes:
            st = prov.g1_subgroup(b"".join(key_bytes.values()))
            key_ok = {pk: st[j] == 1 and (pk.value.infinity or any(b)) for j, (pk, b) in enumerate(key_bytes.items())}
            keep = [all(key_ok[pk] for g in p[2] for pk in g) for p in elig]
            elig, sig_bytes = [p for p, k in zip(elig, keep) if k], [b for b, k in zip(sig_bytes, keep) if k]

        # P_im: one key -> e pk, infinity iff e = 0 mod n or pk = O (pk in G1); several -> one grouped G1 sum
        multi = [[(key_bytes[pk], int(e) % GROUP_ORDER) for pk, e in zip(g, eg)]
                 for p in elig for g, eg in zip(p[2], p[3]) if len(g) > 1]
        sums = iter(_g1_group_sums(prov, multi))
        terms, keep = [], []                              # per signature: [(message hash, P bytes, scalar factor)]
        for p in elig:
            t, ok = [], True
            for mh, g, eg in zip(p[1], p[2], p[3]):
                if len(g) > 1:
                    b, inf = next(sums)
                    t.append((mh, b, 1))
                else:
                    e = int(eg[0]) % GROUP_ORDER
                    inf = e == 0 or g[0].value.infinity
                    t.append((mh, key_bytes[g[0]], e))
                ok = ok and not inf
            terms.append(t)
            keep.append(ok)
        elig, sig_bytes, terms = ([x for x, k in zip(v, keep) if k] for v in (elig, sig_bytes, terms))

        # H(m) of every distinct message (one call); a message that hashes to infinity leaves the combined check
        msgs = list(dict.fromkeys(mh for p in elig for mh in p[1]))
        if msgs:
            hm = prov.hash_to_g2(b"".join(msgs))
            hm = {mh: hm[192 * j:192 * (j + 1)] for j, mh in enumerate(msgs)}
            keep = [all(any(hm[mh]) for mh in p[1]) for p in elig]
            elig, sig_bytes, terms = ([x for x, k in zip(v, keep) if k] for v in (elig, sig_bytes, terms))

        ok = True
        if elig:
            r = []
            for _ in elig:
                x = 0
                while x == 0:
                    x = rng.getrandbits(64)
                r.append(x)
            S, s_inf = prov.g2_msm(b"".join(sig_bytes), r, len(elig), 1)
            by_msg = {}
            for ri, t in zip(r, terms):
                for mh, b, e in t:
                    by_msg.setdefault(mh, []).append((b, ri * e % GROUP_ORDER))
            order = list(by_msg)
            Pm = _g1_group_sums(prov, [by_msg[mh] for mh in order])
            if BLS._NEG_G1 is None:
                BLS._NEG_G1 = H.g1_affine_bytes((generator_Fq() * (GROUP_ORDER - 1))._aff())
            g1, g2 = ([], []) if s_inf[0] else ([BLS._NEG_G1], [S])
            for mh, (b, inf) in zip(order, Pm):
                if not inf:                               # a combined sum at infinity pairs to 1: left out, not fed as (0, 0)
                    g1.append(b)
                    g2.append(hm[mh])
            if g1:
                ok = prov.pairing_multi(b"".join(g1), b"".join(g2), len(g1)) == Fq12.one(default_ec.q).serialize()
        done = {p[0] for p in elig} if ok else set()
        for i in done:
            results[i] = True
        rest = [p[0] for p in plans if p[0] not in done]
        if rest:
            for i, v in zip(rest, BLS.verify_batch([signatures[i] for i in rest])):
                results[i] = v
        return results

    @staticmethod
    def verify_batch_find(signatures, rng=None, fold=False):
        """verify_batch(signatures) with the forgeries NAMED on the device (blsgpu_verify_find): every signature over exactly
        one 32-byte message hash is an item (signature, key, message) of one call that checks all items by a random linear
        combination and bisects only what fails -- one forgery among n costs about 2 log2 n node tests, not n pairings.  The
        item's key is the signature's one key when its exponent is 1, otherwise the per-message key sum sum_j e_j pk_j (one
        grouped G1 sum, every contributing key checked for G1 membership first); keys and message hashes are deduplicated
        into the call's two tables.  The weights are rng.getrandbits(64), redrawn while zero, in the order of the list
        (default secrets.SystemRandom()).  Status 1 is True and 0 False; every other signature -- several messages, status 2
        (a key or key sum outside G1 or at infinity, H(m) at infinity), a tree without one of its keys, an infinity signature,
        a provider without the verify_find extension -- is decided by verify_batch in the same call.  The answers equal verify_batch's
        except that an invalid item is reported True with probability at most 2^-64 per node that holds it (DESIGN.md
        section 2u).
        fold=True (many signers over few messages): the items, their weights drawn as above, are stably sorted by message hash
        and go to the verify_find_folded extension (blsgpu_verify_find_folded), whose node tests take one
        pair per distinct message instead of one per item; the verdicts come back in the order of the list.  A provider without
        that extension takes the path of fold=False."""
        prov = backend.get()
        rng = rng or secrets.SystemRandom()
        results = [None] * len(signatures)
        plans = []                                        # (index, message hashes, key groups (PublicKey), exponent groups)
        for i, sig in enumerate(signatures):
            info = sig.aggregation_info
            by_message = {}
            for mh, pk in zip(info.message_hashes, info.public_keys):
                by_message.setdefault(mh, []).append(pk)
            kg, eg = [], []
            try:
                for mh, keys in by_message.items():
                    uniq = list(set(keys))
                    eg.append([info.tree[(mh, pk)] for pk in uniq])
                    kg.append(uniq)
            except KeyError:
                results[i] = False                        # bls.py:189-190
                continue
            plans.append((i, list(by_message), kg, eg))
        items = []
        find = backend.extension("verify_find")
        if find is not None:
            items = [p for p in plans if not signatures[p[0]].value.infinity and len(p[1]) == 1 and len(p[1][0]) == 32]

        # the item's key: the one key itself, or the key sum of keys that are all in G1
        def single(p):
            return len(p[2][0]) == 1 and int(p[3][0][0]) % GROUP_ORDER == 1
        key_bytes = {}
        for p in items:
            for pk in p[2][0]:
                if pk not in key_bytes:
                    key_bytes[pk] = _jac_g1_bytes(pk.value)
        summed = [p for p in items if not single(p)]
        if summed:
            contributing = list(dict.fromkeys(pk for p in summed for pk in p[2][0]))
            st = prov.g1_subgroup(b"".join(key_bytes[pk] for pk in contributing))
            in_g1 = {pk: st[j] == 1 for j, pk in enumerate(contributing)}
            bad = {p[0] for p in summed if not all(in_g1[pk] for pk in p[2][0])}
            items = [p for p in items if p[0] not in bad]
            summed = [p for p in summed if p[0] not in bad]
        sums = iter(_g1_group_sums(prov, [[(key_bytes[pk], int(e) % GROUP_ORDER) for pk, e in zip(p[2][0], p[3][0])] for p in summed]))

        if items:
            keys, msgs, key_idx, msg_idx, sigs, weights = {}, {}, [], [], [], []
            for p in items:
                kb = key_bytes[p[2][0][0]] if single(p) else next(sums)[0]
                key_idx.append(keys.setdefault(kb, len(keys)))
                msg_idx.append(msgs.setdefault(p[1][0], len(msgs)))
                sigs.append(H.g2_affine_bytes(signatures[p[0]].value.to_affine()._aff()))
                x = 0
                while x == 0:
                    x = rng.getrandbits(64)
                weights.append(x)
            folded = backend.extension("verify_find_folded") if fold else None
            if folded is not None:
                table = sorted(msgs)
                order = sorted(range(len(items)), key=lambda j: items[j][1][0])          # stable: input order within a message
                place = {mh: j for j, mh in enumerate(table)}
                status, _ = folded(b"".join(sigs[j] for j in order), b"".join(keys), [key_idx[j] for j in order], b"".join(table),
                                   [place[items[j][1][0]] for j in order], [weights[j] for j in order])
                items = [items[j] for j in order]
            else:
                status, _ = find(b"".join(sigs), b"".join(keys), key_idx, b"".join(msgs), msg_idx, weights)
            for p, s in zip(items, status):
                if s != 2:
                    results[p[0]] = s == 1
        rest = [p[0] for p in plans if results[p[0]] is None]
        if rest:
            for i, v in zip(rest, BLS.verify_batch([signatures[i] for i in rest])):
                results[i] = v
        return results

    @staticmethod
    def aggregate_pub_keys(public_keys, secure):
        if len(public_keys) < 1:
            raise Exception("Invalid number of keys")
        public_keys.sort()                 # in place, like the reference (bls.py:210)
        ts = hash_pks(len(public_keys), public_keys)
        return PublicKey.from_g1(_g1_sums([[pk.value for pk in public_keys]], [ts if secure else [1] * len(public_keys)])[0])

    @staticmethod
    def aggregate_priv_keys(private_keys, public_keys, secure):
        if not secure:
            total = sum(sk.value for sk in private_keys) % GROUP_ORDER
        else:
            if not public_keys:
                raise Exception("Must include public keys in secure aggregation")
            if len(private_keys) != len(public_keys):
                raise Exception("Invalid number of keys")
            pairs = sorted(zip(public_keys, private_keys))
            ts = hash_pks(len(private_keys), public_keys)
            total = sum(sk.value * t for t, (_, sk) in zip(ts, pairs)) % GROUP_ORDER
        return PrivateKey.from_bytes(total.to_bytes(32, "big"))

    @staticmethod
    def aggregate_pub_keys_batch(groups, secure, ragged=False):
        """[BLS.aggregate_pub_keys(list(g), secure) for g in groups] without sorting the caller's lists: one device call per
        distinct group length.  secure=True: blsgpu_aggregate_pub_keys_secure -- the hash_pks exponents of every group
        (both SHA-256 steps and the reduction mod n) and the G1 sums behind them in one call, the exponents never on the
        host; a provider without the entry runs the loop above.  secure=False: one grouped plain sum (g1_msm).
        ragged=True (with secure=True; without it the keyword changes nothing): ALL groups in ONE call of the provider's
        aggregate_pub_keys_secure_ranges extension (blsgpu_aggregate_pub_keys_secure_ranges) whatever their lengths;
        NotImplementedError when the provider has none."""
        groups = [sorted(g) for g in groups]                 # copies: the reference sorts in place (bls.py:210)
        if any(not g for g in groups):
            raise Exception("Invalid number of keys")
        if ragged and secure:
            fn = backend.extension("aggregate_pub_keys_secure_ranges")
            if fn is None:
                raise NotImplementedError("the provider has no aggregate_pub_keys_secure_ranges extension")
            if not groups:
                return []
            pk_off = [0]
            for g in groups:
                pk_off.append(pk_off[-1] + len(g))
            res, flag = fn(b"".join(_jac_g1_bytes(pk.value) for g in groups for pk in g), b"".join(pk.serialize() for g in groups for pk in g),
                           pk_off)
            if 2 in bytes(flag):
                raise ValueError("a public key that is not on the curve")
            return [PublicKey.from_g1(JacobianPoint._from(H.F1, None if flag[q] else H.aff_to_jac(H.F1, H.g1_from_abi(res[96 * q:96 * (q + 1)]))))
                    for q in range(len(groups))]
        prov = backend.get()
        fn = getattr(prov, "aggregate_pub_keys_secure", None) if secure else prov.g1_msm
        if fn is None:
            return [BLS.aggregate_pub_keys(g, secure) for g in groups]
        buckets = {}
        for j, g in enumerate(groups):
            buckets.setdefault(len(g), []).append(j)
        out = [None] * len(groups)
        for k, js in buckets.items():
            pts = b"".join(_jac_g1_bytes(pk.value) for j in js for pk in groups[j])
            if secure:
                res, inf = fn(pts, b"".join(pk.serialize() for j in js for pk in groups[j]), k, len(js))
            else:
                res, inf = fn(pts, None, k, len(js))
            for q, j in enumerate(js):
                out[j] = PublicKey.from_g1(JacobianPoint._from(H.F1, None if inf[q] else H.aff_to_jac(H.F1, H.g1_from_abi(res[96 * q:96 * (q + 1)]))))
        return out

    @staticmethod
    def aggregate_sigs_secure_batch(sig_groups, pk_groups, mh_groups, ragged=False):
        """[BLS.aggregate_sigs_secure(s, p, m) for s, p, m in zip(sig_groups, pk_groups, mh_groups)]: one
        blsgpu_aggregate_sigs_secure call per distinct group length.  As in bls.py:39-45 the signatures are ordered by
        (message hash, public key, signature) and the exponents hashed over the public keys in the CALLER's order.  A
        provider without the entry runs that loop.
        ragged=True: ALL groups, empty ones included, in ONE call of the provider's aggregate_sigs_secure_ranges extension
        (blsgpu_aggregate_sigs_secure_ranges) whatever their lengths; NotImplementedError when the provider has none."""
        trip = [(list(s), list(p), list(m)) for s, p, m in zip(sig_groups, pk_groups, mh_groups)]
        for s, p, m in trip:
            if not (len(s) == len(p) == len(m)):
                raise Exception("Invalid number of keys")
        if ragged:
            fn = backend.extension("aggregate_sigs_secure_ranges")
            if fn is None:
                raise NotImplementedError("the provider has no aggregate_sigs_secure_ranges extension")
            if not trip:
                return []
            sigs, sers, off = bytearray(), bytearray(), [0]
            for s, p, m in trip:
                for _, _, sig in sorted(zip(m, p, s)):
                    sigs += H.g2_affine_bytes(sig.value.to_affine()._aff())
                for pk in p:
                    sers += pk.serialize()
                off.append(off[-1] + len(s))
            res, flag = fn(bytes(sigs), off, bytes(sers), off)
            if 2 in bytes(flag):
                raise ValueError("a signature that is not on the curve")
            return [Signature.from_g2(JacobianPoint._from(H.F2, None if flag[q] else H.aff_to_jac(H.F2, H.g2_from_abi(res[192 * q:192 * (q + 1)]))))
                    for q in range(len(trip))]
        fn = getattr(backend.get(), "aggregate_sigs_secure", None)
        if fn is None:
            return [BLS.aggregate_sigs_secure(s, p, m) for s, p, m in trip]
        buckets = {}
        for j, (s, _, _) in enumerate(trip):
            buckets.setdefault(len(s), []).append(j)
        out = [None] * len(trip)
        for k, js in buckets.items():
            if k == 0:                                       # an empty sum: infinity, no exponents
                for j in js:
                    out[j] = Signature.from_g2(JacobianPoint._from(H.F2, None))
                continue
            sigs, sers = bytearray(), bytearray()
            for j in js:
                s, p, m = trip[j]
                for _, _, sig in sorted(zip(m, p, s)):
                    sigs += H.g2_affine_bytes(sig.value.to_affine()._aff())
                for pk in p:
                    sers += pk.serialize()
            res, inf = fn(bytes(sigs), k, bytes(sers), k, len(js))
            for q, j in enumerate(js):
                out[j] = Signature.from_g2(JacobianPoint._from(H.F2, None if inf[q] else H.aff_to_jac(H.F2, H.g2_from_abi(res[192 * q:192 * (q + 1)]))))
        return out

    @staticmethod
    def aggregate_priv_keys_batch(groups, secret=False, public_keys=False, secure_with=None):
        """[BLS.aggregate_priv_keys(g, None, False) for g in groups] -- step 3 of Joint-Feldman, a player's share as the sum
        of the fragments it was dealt -- and with public_keys=True (keys, [k.get_public_key() for k in keys]).  The
        default is that loop on the host.  secret=True: one blsgpu_fr_sum_secret call per distinct group length, whose
        sequence of instructions and addresses does not depend on the keys; with public_keys=True the same call
        multiplies the sums by G1 on the device (k_fix_mul_secret) before anything returns.  A provider without the
        entry raises NotImplementedError, an empty group ValueError.
        secure_with: a list of public-key lists, one per group -- secure aggregation: the result equals
        [BLS.aggregate_priv_keys(g, pks, True) for g, pks in zip(groups, secure_with)], the reference's order included
        (bls.py:239-241: the pairs sorted by public key, the exponents hashed over the public keys as given).  With
        secret=True that is one blsgpu_aggregate_priv_keys_secure call per distinct group length (at most
        LAGRANGE_MAX_K keys per group): the hash_pks exponents on the device, the sums on k_fr_dot_secret's masked
        arithmetic, the public keys from k_fix_mul_secret; a provider without the entry raises NotImplementedError."""
        groups = [list(g) for g in groups]
        if secure_with is not None:
            return BLS._aggregate_priv_keys_secure_batch(groups, [list(p) for p in secure_with], secret, public_keys)
        if not secret:
            keys = [BLS.aggregate_priv_keys(g, None, False) for g in groups]
            return (keys, [k.get_public_key() for k in keys]) if public_keys else keys
        from .keys import _pk_from_device, _secret_call
        fr_sum = _secret_call("fr_sum_secret")
        if any(not g for g in groups):
            raise ValueError("secret=True: an empty group has no device form")
        buckets = {}
        for i, g in enumerate(groups):
            buckets.setdefault(len(g), []).append(i)
        keys, pks = [None] * len(groups), [None] * len(groups)
        for k, idx in buckets.items():
            yb = b"".join(sk.value.to_bytes(32, "big") for i in idx for sk in groups[i])
            out, aff, ser = fr_sum(yb, k, len(idx), public_keys)
            for q, i in enumerate(idx):
                keys[i] = PrivateKey.from_bytes(out[32 * q:32 * (q + 1)])
                if public_keys:
                    pks[i] = _pk_from_device(aff[96 * q:96 * (q + 1)], ser[48 * q:48 * (q + 1)])
                    keys[i].__dict__["_pk_point"] = pks[i].value          # the cache get_public_key fills (same point)
        return (keys, pks) if public_keys else keys

    @staticmethod
    def _aggregate_priv_keys_secure_batch(groups, pk_groups, secret, public_keys):
        if len(groups) != len(pk_groups):
            raise ValueError("secure_with holds one list of public keys per group")
        if not secret:
            keys = [BLS.aggregate_priv_keys(g, p, True) for g, p in zip(groups, pk_groups)]
            return (keys, [k.get_public_key() for k in keys]) if public_keys else keys
        from .keys import _pk_from_device, _secret_call
        agg = _secret_call("aggregate_priv_keys_secure")
        for g, p in zip(groups, pk_groups):
            if not p:
                raise Exception("Must include public keys in secure aggregation")
            if len(g) != len(p):
                raise Exception("Invalid number of keys")
        buckets = {}
        for i, g in enumerate(groups):
            buckets.setdefault(len(g), []).append(i)
        keys, pks = [None] * len(groups), [None] * len(groups)
        for k, idx in buckets.items():
            # bls.py:239-241: key i of the SORTED pairs meets exponent i, hashed over the public keys in the caller's order
            yb = b"".join(sk.value.to_bytes(32, "big") for i in idx for _, sk in sorted(zip(pk_groups[i], groups[i])))
            sers = b"".join(pk.serialize() for i in idx for pk in pk_groups[i])
            out, aff, ser = agg(yb, sers, k, len(idx), public_keys)
            for q, i in enumerate(idx):
                keys[i] = PrivateKey.from_bytes(out[32 * q:32 * (q + 1)])
                if public_keys:
                    pks[i] = _pk_from_device(aff[96 * q:96 * (q + 1)], ser[48 * q:48 * (q + 1)])
                    keys[i].__dict__["_pk_point"] = pks[i].value          # the cache get_public_key fills (same point)
        return (keys, pks) if public_keys else keys
