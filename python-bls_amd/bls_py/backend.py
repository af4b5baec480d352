"""Where the host-side scheme code gets its heavy operations from.

Default (and only shipped) provider: the HIP engine behind libblsgpu.so.
`use(provider)` exists so that CPU-only unit tests of the HOST LOGIC can plug in
a stand-in (tests/ inject the CPU oracle); the product never does that and has
no fallback -- with no GPU the default provider raises BlsGpuError.
"""
_provider = None


class HipProvider:
    def __init__(self, device=0):
        from . import _native
        self._eng = _native.engine(device)

    def pairing_multi(self, g1: bytes, g2: bytes, n: int, inf=None) -> bytes:
        return self._eng.pairing_multi(g1, g2, n, inf)

    def miller_loop_batch(self, g1: bytes, g2: bytes, n: int, inf=None) -> bytes:
        return self._eng.miller_loop_batch(g1, g2, n, inf)

    def line_eval_batch(self, r: bytes, q, p: bytes, n: int) -> bytes:
        return self._eng.line_eval_batch(r, q, p, n)

    def final_exp(self, x: bytes) -> bytes:
        return self._eng.final_exp(x)

    def pairing_multi_batch(self, g1: bytes, g2: bytes, gsz: int, groups: int, inf=None) -> bytes:
        return self._eng.pairing_multi_batch(g1, g2, gsz, groups, inf)

    def g1_msm(self, pts: bytes, scalars, k: int, groups: int = 1):
        return self._eng.g1_msm(pts, scalars, k, groups)

    def g2_msm(self, pts: bytes, scalars, k: int, groups: int = 1):
        return self._eng.g2_msm(pts, scalars, k, groups)

    def map_to_g2(self, t: bytes) -> bytes:
        return self._eng.map_to_g2(t)

    def hash_to_g2(self, msg_hashes: bytes) -> bytes:
        return self._eng.hash_to_g2(msg_hashes)

    def g1_decompress(self, data: bytes):
        return self._eng.g1_decompress(data)

    def g2_decompress(self, data: bytes):
        return self._eng.g2_decompress(data)

    def g1_mul_gen(self, scalars: bytes, add=None, n_add: int = 0):
        """(s_i mod n) G1 (+ A) -> (n x 96 affine bytes, n x 48 serialised bytes)"""
        return self._eng.g1_mul_gen(scalars, add, n_add)

    def hd_children(self, chain_code: bytes, parent_pk_aff: bytes, parent_sk, indices):
        """-> (n x 32 chain codes, n x 32 child keys or None (public), n x 96 affine keys, n x 48 serialised keys)"""
        return self._eng.hd_children(chain_code, parent_pk_aff, parent_sk, indices)

    def hd_paths(self, parents: bytes, priv: bool, parent_of, paths):
        """paths of ONE depth, path j from record parent_of[j] (None: record 0) of parents (160 bytes each: chain code,
        affine key, private key) -> (n x 32 chain codes, n x 32 keys or None (public), n x 96 affine keys, n x 48 serialised
        keys, n x 4 parent fingerprints) of the leaves"""
        return self._eng.hd_paths(parents, priv, parent_of, paths)

    def g1_mul_gen_secret(self, scalars: bytes):
        """s_i G1 on the scalar-independent schedule -> (n x 96 affine bytes, n x 48 serialised bytes)"""
        return self._eng.g1_mul_gen_secret(scalars)

    def hd_paths_secret(self, parents: bytes, parent_of, paths):
        """hd_paths in private mode on the scalar-independent schedule: the same outputs"""
        return self._eng.hd_paths_secret(parents, parent_of, paths)

    def g1_poly_check(self, commit: bytes, n_polys: int, t: int, poly, x: bytes, s=None, aff: bool = False):
        """Feldman share checks: -> (n status bytes: 1 (s_i mod n) G1 == sum_k x_i^k C[poly_i][k], 0 not, 2 poly_i has a
        C_k (k >= 1) outside the order-n subgroup; or None for s None) and the n x 96 affine Horner values (aff) or None"""
        return self._eng.g1_poly_check(commit, n_polys, t, poly, x, s, aff)

    def g1_subgroup(self, pts: bytes) -> bytes:
        """n x 96 affine bytes -> n status bytes: 1 in G1 (infinity included), 2 on the curve outside G1, 0 off the curve"""
        return self._eng.g1_subgroup(pts)

    def g2_subgroup(self, pts: bytes) -> bytes:
        """n x 192 affine bytes -> n status bytes: 1 in G2 (infinity included), 2 on the twist outside G2, 0 off the twist"""
        return self._eng.g2_subgroup(pts)

    # ---- threshold recovery for many signer sets at once (threshold.py:56-136): k <= LAGRANGE_MAX_K players per group ----
    @property
    def LAGRANGE_MAX_K(self):
        from . import _native
        return _native.LAGRANGE_MAX_K

    def lagrange_at_zero(self, x, k: int, groups: int = 1):
        """-> (groups x k x 32 coefficient bytes, groups status bytes: 1 written, 0 where the reference asserts)"""
        return self._eng.lagrange_at_zero(x, k, groups)

    def fr_interpolate_at_zero(self, x, y, k: int, groups: int = 1):
        """-> (groups x 32 bytes: sum_j L_j y_j mod n, groups status bytes)"""
        return self._eng.fr_interpolate_at_zero(x, y, k, groups)

    def threshold_combine(self, sigs: bytes, x, k: int, groups: int = 1):
        """-> (groups x 192 affine bytes: sum_j L_j sig_j, [is_infinity], groups status bytes)"""
        return self._eng.threshold_combine(sigs, x, k, groups)

    def sig_shares_check(self, sigs: bytes, keys: bytes, key_idx, x, msg_hashes: bytes, weights, k: int, groups: int = 1,
                         scaled: bool = True):
        """signature shares against their share public keys, a session by one random linear combination and the failing ones
        bisected: -> (groups x k status bytes: 1 valid, 0 invalid, 2 not decided (bad key), groups session status bytes,
        (rounds, node tests))"""
        return self._eng.sig_shares_check(sigs, keys, key_idx, x, msg_hashes, weights, k, groups, scaled)

    def g2_mul_secret(self, pts: bytes, scalars, aff: bool = True, ser: bool = True):
        """s_i P_i (one point of 192 bytes: s_i P) on the scalar-independent schedule
        -> (n x 192 affine bytes, n x 96 serialised bytes, [is_infinity])"""
        return self._eng.g2_mul_secret(pts, scalars, aff, ser)

    def sign(self, sks, msg_hashes: bytes, aff: bool = True, ser: bool = True):
        """sk_i H(h_i) (one hash of 32 bytes: sk_i H(h)): hash to G2 and the scalar-independent multiplication in one call
        -> (n x 192 affine bytes, n x 96 bytes of Signature.serialize())"""
        return self._eng.sign(sks, msg_hashes, aff, ser)

    # ---- the threshold scheme's work on secrets: schedules that do not depend on coefficients, shares or keys ----
    def threshold_deal_secret(self, coeffs, t: int, x, commit: bool = True, frag: bool = True):
        """-> (n_polys x t x 96 affine bytes c_k G1, n_polys x n_x x 32 bytes P_p(x_j) mod n)"""
        return self._eng.threshold_deal_secret(coeffs, t, x, commit, frag)

    def fr_interpolate_at_zero_secret(self, x, y, k: int, groups: int = 1):
        """fr_interpolate_at_zero on the masked sums: the same outputs"""
        return self._eng.fr_interpolate_at_zero_secret(x, y, k, groups)

    def g1_poly_check_secret(self, commit: bytes, n_polys: int, t: int, poly, x: bytes, s, aff: bool = False):
        """g1_poly_check for secret fragments (s is required), the left-hand sides on the scalar-independent schedule: the
        same outputs"""
        return self._eng.g1_poly_check_secret(commit, n_polys, t, poly, x, s, aff)

    def fr_sum_secret(self, y, k: int, groups: int = 1, pk: bool = False):
        """-> (groups x 32 bytes: sum_j y_j mod n on the masked sums, and with pk the public key of every sum, multiplied on the
        device: groups x 96 affine bytes, groups x 48 serialised bytes -- else None, None)"""
        return self._eng.fr_sum_secret(y, k, groups, pk)

    def sign_threshold(self, sks, x, k: int, msg_hashes: bytes, groups: int = 1, aff: bool = True, ser: bool = True):
        """(lambda_j sk_j mod n) H(h) per signer: -> (affine bytes, serialised bytes, [is_infinity], groups status bytes)"""
        return self._eng.sign_threshold(sks, x, k, msg_hashes, groups, aff, ser)

    # ---- secure aggregation (util.py:36-50, bls.py:28-56 and 203-249): the hash_pks exponents never visit the host ----
    def hash_pks(self, pks_ser: bytes, k: int, m: int, groups: int = 1):
        """-> groups x m x 32 bytes: t_i = sha256(be32(i) || sha256(the group's k serialised keys)) mod n"""
        return self._eng.hash_pks(pks_ser, k, m, groups)

    def aggregate_pub_keys_secure(self, pts_aff: bytes, pks_ser: bytes, k: int, groups: int = 1):
        """-> (groups x 96 affine bytes: sum_i t_i P_i, [is_infinity]); both buffers in the order to be hashed"""
        return self._eng.aggregate_pub_keys_secure(pts_aff, pks_ser, k, groups)

    def aggregate_sigs_secure(self, sigs_aff: bytes, k: int, pks_ser: bytes, k_pks: int, groups: int = 1):
        """-> (groups x 192 affine bytes: sum_i t_i S_i, [is_infinity]); k exponents hashed over k_pks keys per group"""
        return self._eng.aggregate_sigs_secure(sigs_aff, k, pks_ser, k_pks, groups)

    def aggregate_priv_keys_secure(self, sks, pks_ser: bytes, k: int, groups: int = 1, pk: bool = False):
        """-> (groups x 32 bytes: sum_i t_i sk_i mod n on the masked sums, and with pk the public key of every sum: groups x 96
        affine bytes, groups x 48 serialised bytes -- else None, None); sks in the order the exponents multiply them, pks_ser in
        the order to be hashed"""
        return self._eng.aggregate_priv_keys_secure(sks, pks_ser, k, groups, pk)

    # ---- the whole of BLS.verify's device work without a host round trip between its steps (bls.py:153-201) ----
    def verify_pipeline(self, neg_g1: bytes, sig: bytes, hashes: bytes, n: int, keys_affine=None, key_pts=None, key_scalars=None, k=0) -> bytes:
        """e(-G1, sig) * prod_i e(P_i, H(m_i)) for n message hashes (32 bytes each): blsgpu_verify_pipeline -- ONE upload,
        then on the device hash-to-G2 of the hashes, P_i = either the given affine keys (n x 96 bytes) or the per-message
        key sums (key_pts: n x k x 96 bytes, key_scalars: n x k x 32 bytes big-endian) and the (n + 1)-pair
        multi-pairing; 576 bytes come back.  Nothing but the C ABI (no torch)."""
        return self._eng.verify_pipeline(neg_g1, sig, hashes, n, keys_affine, key_pts, key_scalars, k)


def use(provider):
    """Install a provider object with pairing_multi(g1, g2, n, inf=None), final_exp(x),
    miller_loop_batch(g1, g2, n, inf=None), line_eval_batch(r, q|None, p, n),
    g1_msm / g2_msm(pts, scalars|None, k, groups) -> (bytes, [is_inf]),
    map_to_g2(t: n x 192 bytes) -> n x 192 bytes,
    g1_decompress / g2_decompress(bytes) -> (affine bytes, [accepted]),
    g1_mul_gen(scalars, add|None, n_add) -> (affine bytes, serialised bytes),
    hd_children(chain_code, parent_pk_aff, parent_sk|None, indices) -> (chain codes, child keys|None, affine, serialised),
    g1_poly_check(commit, n_polys, t, poly, x, s|None, aff) -> (status bytes|None, affine Horner values|None),
    g1_subgroup / g2_subgroup(affine bytes) -> status bytes (1 in the subgroup, 2 on the curve outside it, 0 off it).
    Optional (a provider without it sends the HD *_path_batch / *_paths_from methods to chained hd_children calls):
    hd_paths(parents, priv, parent_of|None, paths of one depth) -> (chain codes, keys|None, affine, serialised, fingerprints).
    Optional (the secret=True forms of the key methods raise without them; there is no other path for them):
    g1_mul_gen_secret(scalars) -> (affine bytes, serialised bytes), hd_paths_secret(parents, parent_of|None, paths) -> as hd_paths,
    threshold_deal_secret(coeffs, t, x) -> (commitment bytes, fragment bytes), fr_interpolate_at_zero_secret(x, y, k, groups) ->
    as fr_interpolate_at_zero, sign_threshold(sks, x, k, msg_hashes, groups) -> (affine bytes, serialised bytes, [is_inf], status bytes),
    g1_poly_check_secret(commit, n_polys, t, poly, x, s, aff) -> as g1_poly_check, fr_sum_secret(y, k, groups, pk) ->
    (32 bytes per group, affine bytes|None, serialised bytes|None), aggregate_priv_keys_secure(sks, pks_ser, k, groups, pk) ->
    likewise.
    Optional (a provider without them sends util.hash_pks_batch, BLS.aggregate_pub_keys_batch and
    BLS.aggregate_sigs_secure_batch to the per-call loop): hash_pks(pks_ser, k, m, groups) -> exponent bytes,
    aggregate_pub_keys_secure(pts_aff, pks_ser, k, groups) -> (affine bytes, [is_inf]),
    aggregate_sigs_secure(sigs_aff, k, pks_ser, k_pks, groups) -> (affine bytes, [is_inf]).
    Optional (a provider without them sends the Threshold.*_batch methods to the host loop): LAGRANGE_MAX_K,
    lagrange_at_zero(x, k, groups) -> (coefficient bytes, status bytes), fr_interpolate_at_zero(x, y, k, groups) ->
    (32 bytes per group, status bytes), threshold_combine(sigs, x, k, groups) -> (affine bytes, [is_inf], status bytes).
    Optional (a provider without it sends Threshold.verify_sig_shares_batch to the exact per-share pairings):
    sig_shares_check(sigs, keys, key_idx, x|None, msg_hashes, weights, k, groups, scaled) -> (status bytes, session status
    bytes, (rounds, node tests))."""
    global _provider
    _provider = provider


def get():
    global _provider
    if _provider is None:
        _provider = HipProvider()
    return _provider
