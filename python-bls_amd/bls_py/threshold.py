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
