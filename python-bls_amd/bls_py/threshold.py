"""k-of-n threshold helpers (threshold.py:56-136 of the reference)."""
from .bls12381 import n as GROUP_ORDER, q as FIELD_Q
from .ec import AffinePoint, JacobianPoint, default_ec, generator_Fq
from .fields import Fq
from . import hostmath as H
from .signature import Signature


class Threshold:
    @staticmethod
    def lagrange_coeffs_at_zero(X, ec=default_ec):
        """L_j with P(0) = sum_j L_j P(X[j]) (second barycentric form), as Fq(n, .)."""
        n = ec.n
        k = len(X)
        assert len(set(X)) == k and all(0 != x < n for x in X)
        shifts = []
        for j in range(k):
            w = 1
            for i in range(k):
                if i != j:
                    w = w * (X[j] - X[i]) % n
            shifts.append(pow(w, n - 2, n) * pow(-X[j] % n, n - 2, n) % n)
        den = pow(sum(shifts) % n, n - 2, n)
        return [Fq(n, s * den) for s in shifts]

    @staticmethod
    def interpolate_at_zero(X, Y, ec=default_ec):
        acc = Fq(ec.n, 0)
        for lam, y in zip(Threshold.lagrange_coeffs_at_zero(X, ec), Y):
            acc += lam * y
        return acc

    @staticmethod
    def verify_secret_fragment(T, secret_fragment, player, commitment, ec=default_ec):
        assert len(commitment) == T and secret_fragment != 0 and player != 0
        lhs = generator_Fq(ec) * secret_fragment
        rhs = commitment[0]
        for k in range(1, T):
            rhs = rhs + commitment[k] * pow(player, k, ec.n)
        return lhs == rhs

    @staticmethod
    def verify_secret_fragment_batch(T, secret_fragments, players, commitments, ec=default_ec, secret=False):
        """[verify_secret_fragment(T, s, p, C) for s, p, C in zip(secret_fragments, players, commitments)] with the
        checks of on-curve G1 commitments on the GPU (blsgpu_g1_poly_check): the commitment lists are deduplicated into
        polynomials, every fragment is one lane of a Horner evaluation in the exponent.  The assertions of the single
        call run for every element first.  Lists holding anything but on-curve G1 AffinePoints, fragments that are
        neither an Fq mod n nor an int in [1, n) and players that are not ints take the host loop; a polynomial with a
        commitment C_k (k >= 1) outside the order-n subgroup (where Horner's x^k and the reference's x^k mod n differ)
        is decided exactly by one grouped multi-scalar sum with the scalars x^k mod n.
        secret=True (a player checking what it was dealt): every record on blsgpu_g1_poly_check_secret, whose sequence of
        instructions and addresses does not depend on the fragments -- the left-hand sides of the undecided records come
        from blsgpu_g1_mul_gen_secret likewise.  Nothing takes the host loop then: a provider without the entries raises
        NotImplementedError, a record the device cannot take -- a commitment list that is not all on-curve G1
        AffinePoints, a player that is not an int, a fragment that is neither an Fq mod n nor an int in [1, n), another
        curve, T < 1 -- ValueError.  The results themselves are public: a player publishes them as complaints."""
        secret_fragments, players, commitments = list(secret_fragments), list(players), list(commitments)
        if not (len(secret_fragments) == len(players) == len(commitments)):
            raise ValueError("need one player and one commitment list per fragment")
        for s, p, C in zip(secret_fragments, players, commitments):
            assert len(C) == T
            assert s != 0
            assert p != 0
        n = ec.n
        check = mul_gen = None
        if secret:
            from .keys import _secret_call
            check, mul_gen = _secret_call("g1_poly_check_secret"), _secret_call("g1_mul_gen_secret")
        host_only = T < 1 or ec is not default_ec          # (the device knows the one curve, and t >= 1)
        results = [None] * len(players)
        polys, by_id, by_content = [], {}, {}      # device polynomials: commitment lists deduplicated
        dev = []                                   # (fragment, polynomial)
        for i, (s, p, C) in enumerate(zip(secret_fragments, players, commitments)):
            j = by_id.get(id(C))
            if j is None:
                key = _g1_content(C)
                j = -1 if key is None else by_content.get(key)
                if j is None:
                    j = by_content[key] = len(polys)
                    polys.append(C)
                by_id[id(C)] = j
            if (j < 0 or host_only or type(p) is not int
                    or not ((type(s) is Fq and s.Q == n) or (type(s) is int and 0 < s < n))):
                if secret:
                    raise ValueError("secret=True: a record that the device cannot take (see verify_secret_fragment_batch)")
                results[i] = Threshold.verify_secret_fragment(T, s, p, C, ec)
            else:
                dev.append((i, j))
        if not dev:
            return results
        from . import backend
        dev.sort(key=lambda e: e[1])               # a wavefront reads one polynomial
        commit = b"".join(H.g1_affine_bytes(pt._aff()) for C in polys for pt in C)
        xb = b"".join((players[i] % n).to_bytes(32, "big") for i, _ in dev)
        sb = b"".join(int(secret_fragments[i]).to_bytes(32, "big") for i, _ in dev)
        if secret:
            status, _ = check(commit, len(polys), T, [j for _, j in dev], xb, sb)
        else:
            status, _ = backend.get().g1_poly_check(commit, len(polys), T, [j for _, j in dev], xb, sb)
        undecided = []
        for (i, j), st in zip(dev, status):
            if st == 2:
                undecided.append((i, j))
            else:
                results[i] = st == 1
        if undecided:
            # sum_k (x^k mod n) C_k exactly as the reference forms it (C_0 with 1), against (s mod n) G1
            from .bls import _g1_sums
            sums = _g1_sums([[pt.to_jacobian() for pt in polys[j]] for _, j in undecided],
                            [[pow(players[i], k, n) for k in range(T)] for i, _ in undecided])
            ub = b"".join(int(secret_fragments[i]).to_bytes(32, "big") for i, _ in undecided)
            lhs, _ = mul_gen(ub) if secret else backend.get().g1_mul_gen(ub)
            for e, ((i, _), J) in enumerate(zip(undecided, sums)):
                rhs = bytes(96) if J.infinity else H.g1_affine_bytes(J.to_affine()._aff())
                results[i] = lhs[96 * e:96 * (e + 1)] == rhs
        return results

    @staticmethod
    def aggregate_unit_sigs(signatures, players, T, ec=default_ec):
        """sum_i lambda_i * sig_i  (a |players|-point G2 multi-scalar multiplication)."""
        from .bls import _g2_sum
        lam = Threshold.lagrange_coeffs_at_zero(players, ec)
        return Signature.from_g2(_g2_sum([sig.value for sig in signatures], [int(l) for l in lam]))

    # ---- many signer sets at once: the coefficients on the GPU (blsgpu_lagrange_at_zero and its two consumers) ----
    @staticmethod
    def _device_buckets(Xs, ec, entry, also=None):
        """The routing the three *_batch methods share.  The assertion of lagrange_coeffs_at_zero runs for every group
        first, as a loop of single calls would raise it.  -> (provider, {k: [group indices]}): the groups the device takes,
        one call per distinct k.  Every other group -- a player that is not an int or is negative (the assertion lets
        negatives through), k = 0, k above the device limit, another curve, a provider without `entry`, or `also(i)`
        false -- is left to the caller's host loop."""
        n = ec.n
        for X in Xs:
            assert len(set(X)) == len(X) and all(0 != x < n for x in X)
        if ec is not default_ec:
            return None, {}
        fit = [i for i, X in enumerate(Xs) if X and all(type(x) is int and x > 0 for x in X) and (also is None or also(i))]
        if not fit:
            return None, {}
        from . import backend
        prov = backend.get()
        if not hasattr(prov, entry):
            return None, {}
        kmax = prov.LAGRANGE_MAX_K
        buckets = {}
        for i in fit:
            if len(Xs[i]) <= kmax:
                buckets.setdefault(len(Xs[i]), []).append(i)
        return prov, buckets

    @staticmethod
    def lagrange_coeffs_at_zero_batch(Xs, ec=default_ec):
        """[lagrange_coeffs_at_zero(X, ec) for X in Xs] with the coefficients of every group of positive int players
        computed on the GPU, one call per distinct group length (routing: _device_buckets)."""
        Xs = [list(X) for X in Xs]
        prov, buckets = Threshold._device_buckets(Xs, ec, "lagrange_at_zero")
        out = [None] * len(Xs)
        for k, idx in buckets.items():
            xb = b"".join(x.to_bytes(32, "big") for i in idx for x in Xs[i])
            co, status = prov.lagrange_at_zero(xb, k, len(idx))
            for q, i in enumerate(idx):
                if status[q] == 1:
                    out[i] = [Fq(ec.n, int.from_bytes(co[32 * (q * k + j):32 * (q * k + j + 1)], "big")) for j in range(k)]
        return [Threshold.lagrange_coeffs_at_zero(X, ec) if r is None else r for X, r in zip(Xs, out)]

    @staticmethod
    def interpolate_at_zero_batch(Xs, Ys, ec=default_ec, secret=False):
        """[interpolate_at_zero(X, Y, ec) for X, Y in zip(Xs, Ys)]: coefficients and the sums sum_j L_j y_j on the GPU
        (blsgpu_fr_interpolate_at_zero) for groups whose Y holds one Fq mod n or int per player.
        secret=True (the Y are shares of a private key): every group on blsgpu_fr_interpolate_at_zero_secret, whose
        sequence of instructions and addresses does not depend on the Y.  Nothing takes the host loop then: a provider
        without the entry raises NotImplementedError, a group the device cannot take -- wider than its LAGRANGE_MAX_K,
        empty, players that are not positive ints, values that are not Fq mod n or int, another curve -- ValueError."""
        Xs, Ys = [list(X) for X in Xs], [list(Y) for Y in Ys]
        m = min(len(Xs), len(Ys))
        Xs, Ys = Xs[:m], Ys[:m]
        n = ec.n

        def values(i):
            return len(Ys[i]) == len(Xs[i]) and all((type(y) is Fq and y.Q == n) or type(y) is int for y in Ys[i])
        entry = "fr_interpolate_at_zero"
        if secret:
            from .keys import _secret_call
            entry = "fr_interpolate_at_zero_secret"
            _secret_call(entry)
        prov, buckets = Threshold._device_buckets(Xs, ec, entry, values)
        if secret and sum(len(idx) for idx in buckets.values()) != m:
            raise ValueError("secret=True: a group that the device cannot take (see interpolate_at_zero_batch)")
        out = [None] * m
        for k, idx in buckets.items():
            xb = b"".join(x.to_bytes(32, "big") for i in idx for x in Xs[i])
            yb = b"".join((int(y) % n).to_bytes(32, "big") for i in idx for y in Ys[i])
            res, status = getattr(prov, entry)(xb, yb, k, len(idx))
            for q, i in enumerate(idx):
                if status[q] == 1:
                    out[i] = Fq(n, int.from_bytes(res[32 * q:32 * (q + 1)], "big"))
        assert not secret or all(r is not None for r in out)       # (the assertion of _device_buckets has passed: status 1)
        return [Threshold.interpolate_at_zero(X, Y, ec) if r is None else r for X, Y, r in zip(Xs, Ys, out)]

    @staticmethod
    def aggregate_unit_sigs_batch(signature_groups, player_groups, T, ec=default_ec):
        """[aggregate_unit_sigs(s, p, T, ec) for s, p in zip(signature_groups, player_groups)] in one device call per
        distinct group length (blsgpu_threshold_combine): the coefficients never leave the GPU.  A signature group
        whose length differs from its player group's takes the host loop, as the groups of _device_buckets do.
        T is unused, as in the reference."""
        sigs, Xs = [list(s) for s in signature_groups], [list(p) for p in player_groups]
        m = min(len(sigs), len(Xs))
        sigs, Xs = sigs[:m], Xs[:m]
        prov, buckets = Threshold._device_buckets(Xs, ec, "threshold_combine", lambda i: len(sigs[i]) == len(Xs[i]))
        out = [None] * m
        seen = {}                                   # a signature object listed in many groups is converted once

        def affine(sig):
            b = seen.get(id(sig))
            if b is None:
                b = seen[id(sig)] = H.g2_affine_bytes(sig.value.to_affine()._aff())
            return b
        for k, idx in buckets.items():
            pts = b"".join(affine(sig) for i in idx for sig in sigs[i])
            xb = b"".join(x.to_bytes(32, "big") for i in idx for x in Xs[i])
            res, inf, status = prov.threshold_combine(pts, xb, k, len(idx))
            for q, i in enumerate(idx):
                if status[q] == 1:
                    out[i] = Signature.from_g2(JacobianPoint._from(
                        H.F2, None if inf[q] else H.aff_to_jac(H.F2, H.g2_from_abi(res[192 * q:192 * (q + 1)]))))
        return [Threshold.aggregate_unit_sigs(s, X, T, ec) if r is None else r for s, X, r in zip(sigs, Xs, out)]


    # ---- signature shares: which of them are valid (blsgpu_sig_shares_check) ----
    @staticmethod
    def _sig_shares_exact(prov, items):
        """[e(G1, sig) == e(c PK, H(m))] for items (sig bytes, key bytes, c, message hash): the exact check, one two-pair
        pairing per share -- c PK by one grouped G1 sum of single points, H(m) of the distinct messages, then
        pairing_multi_batch.  A share at infinity is invalid; c PK = O or H(m) = O leaves e(G1, sig) == 1, false for
        every other share in G2 -- and the pairing decides a share outside it."""
        if not items:
            return []
        from .fields import Fq12
        ONE = Fq12.one(default_ec.q).serialize()
        neg_g1 = H.g1_affine_bytes((generator_Fq() * (GROUP_ORDER - 1))._aff())
        terms, _ = prov.g1_msm(b"".join(it[1] for it in items), [it[2] % GROUP_ORDER for it in items], 1, len(items))
        msgs = list(dict.fromkeys(it[3] for it in items))
        hm = prov.hash_to_g2(b"".join(msgs))
        hm = {mh: hm[192 * j:192 * (j + 1)] for j, mh in enumerate(msgs)}
        live = [i for i, it in enumerate(items) if any(it[0])]
        out = [False] * len(items)
        if live:
            g1 = b"".join(neg_g1 + terms[96 * i:96 * (i + 1)] for i in live)
            g2 = b"".join(items[i][0] + hm[items[i][3]] for i in live)
            res = prov.pairing_multi_batch(g1, g2, 2, len(live))
            for j, i in enumerate(live):
                out[i] = res[576 * j:576 * (j + 1)] == ONE
        return out

    @staticmethod
    def verify_sig_shares_batch(signature_groups, player_groups, public_key_groups, message_hashes, scaled=True, rng=None,
                                ec=default_ec):
        """For every session, which of its signature shares are valid: a list of lists of bool.  Session g holds the shares
        signature_groups[g] (Signature objects) of the players player_groups[g] with the share public keys
        public_key_groups[g] (PublicKey objects, PK_i = sk_i G1) over the 32-byte message hash message_hashes[g].
        scaled=True: unit signatures of PrivateKey.sign_threshold -- valid iff e(G1, sig_i) == e(lambda_i PK_i, H(m)) with
        lambda = lagrange_coeffs_at_zero(players); scaled=False: plain shares secret_share.sign(m) -- valid iff
        e(G1, sig_i) == e(PK_i, H(m)) (the players are not looked at).
        On the GPU (blsgpu_sig_shares_check, one call per distinct session length): a session is checked by ONE random
        linear combination with weights rng.getrandbits(64) drawn in list order (default secrets.SystemRandom(); a zero is
        drawn again), and only the sessions that fail are bisected down to the wrong shares.  An invalid share is reported
        valid with probability at most 2^-64 per tested node; a share reported invalid IS invalid.  A share the device does
        not decide (its key is off the curve or outside G1), a session it does not take (routing: _device_buckets) and a
        provider without the entry get the exact per-share pairings.  A player set lagrange_coeffs_at_zero asserts on
        raises the same AssertionError (scaled only)."""
        import secrets
        from . import backend
        sigs = [list(s) for s in signature_groups]
        Xs = [list(p) for p in player_groups]
        pks = [list(p) for p in public_key_groups]
        mhs = list(message_hashes)
        m = len(sigs)
        if not (len(Xs) == len(pks) == len(mhs) == m):
            raise ValueError("need one player list, one key list and one message hash per session")
        for g in range(m):
            if not (len(sigs[g]) == len(pks[g]) and (not scaled or len(Xs[g]) == len(sigs[g]))):
                raise ValueError("a session needs one key (and, scaled, one player) per share")
        rng = rng or secrets.SystemRandom()
        n = ec.n

        def fits(i):
            return len(mhs[i]) == 32
        if scaled:
            prov, buckets = Threshold._device_buckets(Xs, ec, "sig_shares_check", fits)
        else:
            prov, buckets = Threshold._device_buckets([list(range(1, len(s) + 1)) for s in sigs], ec, "sig_shares_check", fits)
        results = [None] * m
        seen_sig, key_row, key_bytes = {}, {}, []

        def sig_affine(sig):
            b = seen_sig.get(id(sig))
            if b is None:
                b = seen_sig[id(sig)] = H.g2_affine_bytes(sig.value.to_affine()._aff())
            return b

        def key_affine(pk):
            return H.g1_affine_bytes(pk.value.to_affine()._aff())
        undecided = []                                      # (session, share)
        for k, idx in buckets.items():
            for i in idx:                                   # the key table: keys deduplicated over the whole call
                for pk in pks[i]:
                    if pk not in key_row:
                        key_row[pk] = len(key_bytes)
                        key_bytes.append(key_affine(pk))
        for k, idx in buckets.items():
            weights = []
            for _ in range(k * len(idx)):
                w = 0
                while w == 0:
                    w = rng.getrandbits(64)
                weights.append(w)
            status, sess, _ = prov.sig_shares_check(
                b"".join(sig_affine(sg) for i in idx for sg in sigs[i]), b"".join(key_bytes),
                [key_row[pk] for i in idx for pk in pks[i]],
                b"".join(x.to_bytes(32, "big") for i in idx for x in Xs[i]) if scaled else None,
                b"".join(bytes(mhs[i]) for i in idx), weights, k, len(idx), scaled)
            for q, i in enumerate(idx):
                assert sess[q] == 1                         # (the assertion of _device_buckets has passed)
                results[i] = [st == 1 for st in status[q * k:(q + 1) * k]]
                undecided += [(i, j) for j in range(k) if status[q * k + j] == 2]
        for i in range(m):
            if results[i] is None:
                results[i] = [None] * len(sigs[i])
                undecided += [(i, j) for j in range(len(sigs[i]))]
        if undecided:
            if scaled:
                lam = {i: [int(l) for l in Threshold.lagrange_coeffs_at_zero(Xs[i], ec)] for i in {i for i, _ in undecided}}
            exact = Threshold._sig_shares_exact(
                prov or backend.get(),
                [(sig_affine(sigs[i][j]), key_affine(pks[i][j]), lam[i][j] if scaled else 1, bytes(mhs[i])) for i, j in undecided])
            for (i, j), ok in zip(undecided, exact):
                results[i][j] = ok
        return results

    @staticmethod
    def share_public_keys(commitments, players, ec=default_ec):
        """The share public keys PK_x = sum_d sum_j x^j C[d][j] of the players x (ints) from the dealers' commitment
        polynomials (commitments[d]: the T on-curve G1 points dealer d published, Joint-Feldman) as PublicKey objects --
        what a combiner checks signature shares against.  One plain grouped G1 sum adds the dealers' commitments per
        coefficient index, then the evaluation-only form of g1_poly_check (blsgpu_g1_poly_check with s = None) evaluates the
        summed polynomial at every player in the exponent."""
        from . import backend
        from .keys import PublicKey
        commitments, players = [list(C) for C in commitments], list(players)
        T = len(commitments[0])
        assert T >= 1 and all(len(C) == T for C in commitments)
        prov = backend.get()
        D = len(commitments)

        def aff(pt):
            return H.g1_affine_bytes((pt if type(pt) is AffinePoint else pt.to_affine())._aff())
        summed, _ = prov.g1_msm(b"".join(aff(commitments[d][j]) for j in range(T) for d in range(D)), None, D, T)
        if not players:
            return []
        _, out = prov.g1_poly_check(summed, 1, T, [0] * len(players), b"".join((x % ec.n).to_bytes(32, "big") for x in players),
                                    None, True)
        return [PublicKey.from_g1(JacobianPoint._from(H.F1, H.aff_to_jac(H.F1, H.g1_from_abi(out[96 * i:96 * (i + 1)]))))
                for i in range(len(players))]

    @staticmethod
    def recover_batch(signature_groups, player_groups, public_key_groups, message_hashes, T, rng=None, ec=default_ec):
        """Recover the signature of every session from PLAIN shares (secret_share.sign(m)) of which some may be wrong:
        verify_sig_shares_batch(..., scaled=False), then the first T valid shares of each session, in the order given,
        combined by aggregate_unit_sigs_batch.  -> [(Signature or None, flags)] per session: None when fewer than T
        shares are valid; flags are the session's list of verify_sig_shares_batch."""
        sigs = [list(s) for s in signature_groups]
        Xs = [list(p) for p in player_groups]
        flags = Threshold.verify_sig_shares_batch(sigs, Xs, public_key_groups, message_hashes, scaled=False, rng=rng, ec=ec)
        take = []
        for s, X, f in zip(sigs, Xs, flags):
            good = [j for j, ok in enumerate(f) if ok][:T]
            take.append(good if len(good) == T else None)
        live = [g for g, t in enumerate(take) if t is not None]
        combined = Threshold.aggregate_unit_sigs_batch([[sigs[g][j] for j in take[g]] for g in live],
                                                       [[Xs[g][j] for j in take[g]] for g in live], T, ec)
        out = [(None, f) for f in flags]
        for g, sig in zip(live, combined):
            out[g] = (sig, flags[g])
        return out


def _g1_content(C):
    """the content key of a commitment list whose every element is an on-curve G1 AffinePoint (the device's input), or
    None (the host loop takes it)"""
    key = []
    for pt in C:
        if type(pt) is not AffinePoint or pt.FE is not Fq or pt.x.Q != FIELD_Q or pt.y.Q != FIELD_Q:
            return None
        if pt.infinity:
            key.append(None)
        elif pt.is_on_curve():
            key.append((pt.x.Z, pt.y.Z))
        else:
            return None
    return tuple(key)
