"""Where the host-side scheme code gets its heavy operations from.

Default (and only shipped) provider: the HIP engine behind libblsgpu.so.
`use(provider)` exists so that CPU-only unit tests of the HOST LOGIC can plug in
a stand-in (tests/ inject the CPU oracle); the product never does that and has
no fallback -- with no GPU the default provider raises BlsGpuError.
"""
_provider = None


# The engine methods a HipProvider has, and no others: the scheme code picks its path by hasattr(provider, name).
PROVIDER_METHODS = (
    "pairing_multi", "miller_loop_batch", "line_eval_batch", "final_exp", "pairing_multi_batch", "g1_msm", "g2_msm",
    "map_to_g2", "hash_to_g2", "g1_decompress", "g2_decompress", "g1_subgroup", "g2_subgroup",
    "g1_mul_gen", "hd_children", "hd_paths", "g1_mul_gen_secret", "hd_paths_secret", "g1_poly_check",
    # threshold recovery for many signer sets at once (threshold.py:56-136): k <= LAGRANGE_MAX_K players per group
    "lagrange_at_zero", "fr_interpolate_at_zero", "threshold_combine", "sig_shares_check",
    "g2_mul_secret", "sign",
    # the threshold scheme's work on secrets: schedules that do not depend on coefficients, shares or keys
    "threshold_deal_secret", "fr_interpolate_at_zero_secret", "g1_poly_check_secret", "fr_sum_secret", "sign_threshold",
    # secure aggregation (util.py:36-50, bls.py:28-56 and 203-249): the hash_pks exponents never visit the host
    "hash_pks", "aggregate_pub_keys_secure", "aggregate_sigs_secure", "aggregate_priv_keys_secure",
    # the whole of BLS.verify's device work without a host round trip between its steps (bls.py:153-201)
    "verify_pipeline",
)


def _delegate(name):
    def method(self, *args, **kwargs):
        return getattr(self._eng, name)(*args, **kwargs)
    method.__name__ = name
    method.__doc__ = "_native.Engine.%s on this provider's engine" % name
    return method


class HipProvider:
    """PROVIDER_METHODS of the process-wide engine of `device`, each with the arguments and the result of the
    _native.Engine method of its name; the contract is use()'s."""

    def __init__(self, device=0):
        from . import _native
        self._eng = _native.engine(device)

    @property
    def LAGRANGE_MAX_K(self):
        from . import _native
        return _native.LAGRANGE_MAX_K


for _name in PROVIDER_METHODS:
    setattr(HipProvider, _name, _delegate(_name))
del _name


def use(provider):
    """Install a provider object.  This is the provider contract; the buffers and results of every method are those of the
    _native.Engine method of its name, which HipProvider hands them to.  A provider has
    pairing_multi(g1, g2, n, inf=None), final_exp(x), miller_loop_batch(g1, g2, n, inf=None), line_eval_batch(r, q|None, p, n),
    pairing_multi_batch(g1, g2, gsz, groups, inf=None) -> groups x 576 bytes,
    g1_msm / g2_msm(pts, scalars|None, k, groups) -> (bytes, [is_inf]),
    map_to_g2(t: n x 192 bytes) -> n x 192 bytes,
    g1_decompress / g2_decompress(bytes) -> (affine bytes, [accepted]),
    g1_mul_gen(scalars, add|None, n_add) -> (affine bytes, serialised bytes),
    hd_children(chain_code, parent_pk_aff, parent_sk|None, indices) -> (chain codes, child keys|None, affine, serialised),
    g1_poly_check(commit, n_polys, t, poly, x, s|None, aff) -> (status bytes|None, affine Horner values|None),
    g1_subgroup / g2_subgroup(affine bytes) -> status bytes (1 in the subgroup, 2 on the curve outside it, 0 off it),
    sign(sks, msg_hashes, aff, ser) -> (affine bytes, bytes of Signature.serialize()) and g2_mul_secret(pts, scalars, aff, ser) ->
    (affine bytes, serialised bytes, [is_inf]), both on the scalar-independent schedule.
    Optional (a provider without it hashes on the host and maps with map_to_g2): hash_to_g2(n x 32-byte message hashes) ->
    n x 192 bytes.
    Optional (a provider without it sends BLS.verify to hashing, key sums and pairing_multi one after the other):
    verify_pipeline(neg_g1, sig, hashes, n, keys_affine | key_pts + key_scalars + k) -> 576 bytes.
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
    bytes, (rounds, node tests)).
    Optional extension (without it BLS.verify_batch_find sends everything to verify_batch): verify_find(sigs, keys, key_idx,
    msg_hashes, msg_idx, weights) -> (status bytes, (rounds, node tests, pairs)); with it g1_mul_short / g2_mul_short(pts,
    weights) -> (affine bytes, [is_inf]) for 64-bit public weights.  Optional extension (without it
    BLS.verify_batch_find(fold=True) takes the path of fold=False): verify_find_folded, verify_find's arguments and results
    with msg_idx non-decreasing; with it g1_range_sums / g2_range_sums(pts, ranges) -> (affine bytes, flag bytes).
    Optional extension (for callers; bls.py itself keeps its padded and per-length-class g1_msm calls, which measured faster
    on the skewed shape: DESIGN.md section 2w): g1_msm_ranges / g2_msm_ranges(pts, scalars, ranges) -> (affine bytes, flag
    bytes: 0 finite, 1 infinity, 2 a point off the curve in the range) -- sum_{i in [begin, end)} scalars[i] pts[i] for ranges
    (begin, end) of any lengths over one list of points, scalars as ints below 2^256 or 32-byte big-endian values.
    Optional extension (without it ec.hash_to_points_prehashed_Fq / hash_to_points_Fq run the per-message host calls):
    hash_to_g1(n x 32-byte message hashes, aff=True, ser=False) and map_to_g1(t: n x 96 bytes t0 || t1, aff=True, ser=False) ->
    (n x 96 affine bytes|None, n x 48 serialised bytes|None, [is_inf]).
    Optional extension (without it Signature.divide_by_batch is the loop of Signature.divide_by): sig_divide(pts, pt_off, ent_off,
    ent_dividend, ent_divisor) -> (m x 192 affine bytes, m flag bytes, n_pts status bytes, n_pts x 32 scalar bytes, (path, divisors
    with a quotient other than 1)) for m dividends whose points [pt_off[j], pt_off[j + 1]) are the dividend's own signature and
    then its divisors, and whose entries [ent_off[p], ent_off[p + 1]) carry the exponents of divisor p's tree.
    Optional extension (without it BLS.verify_batch(ragged=True) raises; the default verify_batch does not use it):
    pairing_multi_ranges(g1, g2, ranges, inf=None) -> m x 576 bytes, fq_ate_pairing_multi of the pairs [begin, end) of one
    list of pairs for m ranges (begin, end) of any lengths.
    Optional extension (without it BLS.verify_batch(fused=True) raises; the default verify_batch does not use it):
    verify_aggregates(sigs, msg_hashes, keys, exps|None, grp_off, grp_msg, agg_off, gt=False) -> (m status bytes: 1 valid, 0
    not, 2 not decided; m x 576 bytes|None) -- BLS.verify of m aggregates, group g summing the keys [grp_off[g], grp_off[g + 1])
    for message grp_msg[g], aggregate j owning the groups [agg_off[j], agg_off[j + 1]).
    Optional extensions (without them the ragged=True forms of util.hash_pks_batch, BLS.aggregate_pub_keys_batch and
    BLS.aggregate_sigs_secure_batch raise; the defaults do not use them): hash_pks_ranges(pks_ser, pk_off, exp_off) -> exponent
    bytes, aggregate_pub_keys_secure_ranges(pts_aff, pks_ser, pk_off) -> (affine bytes, flag bytes: 0 finite, 1 infinity, 2 a
    point off the curve in the group), aggregate_sigs_secure_ranges(sigs_aff, sig_off, pks_ser, pk_off) -> likewise -- group g
    hashing the keys [pk_off[g], pk_off[g + 1]) of one list and owning the exponents (signatures) [exp_off[g], exp_off[g + 1]).
    Extensions are looked up by extension(name), not by hasattr: a stand-in offers one as an attribute of that name, the
    HipProvider's come from EXTENSIONS.  Optional (without it PrivateKey.from_seed_batch and
    ExtendedPrivateKey.from_seed_batch run the per-seed host calls): keys_from_seeds(seeds, seed_len, n, hd) -> (key bytes,
    chain codes|None, affine bytes, serialised bytes, None) for n seeds of one length, at most 1024 bytes each, on the
    device's one schedule, which does not depend on the seeds."""
    global _provider
    _provider = provider


# What a HipProvider has beyond PROVIDER_METHODS: name -> the module of bls_py whose function of that name takes the
# provider's engine first.
EXTENSIONS = {"keys_from_seeds": "_native_seeds"}
# ... and the calls on short public scalars and the batch verification that names the forgeries (BLS.verify_batch_find), looked
# up by extension(name) in the same way.
FIND_EXTENSIONS = {"g1_mul_short": "_native_find", "g2_mul_short": "_native_find", "verify_find": "_native_find"}
# ... and the sums over ranges of points and the batch verification that folds shared messages (BLS.verify_batch_find(fold=True)).
RANGE_EXTENSIONS = {"g1_range_sums": "_native_ranges", "g2_range_sums": "_native_ranges", "verify_find_folded": "_native_ranges"}
# ... and the multi-scalar sums over ranges of any lengths.
MSM_RANGE_EXTENSIONS = {"g1_msm_ranges": "_native_msmr", "g2_msm_ranges": "_native_msmr"}
# ... and hash to G1 (ec.hash_to_points_prehashed_Fq / hash_to_points_Fq).
H2G1_EXTENSIONS = {"map_to_g1": "_native_h2g1", "hash_to_g1": "_native_h2g1"}
# ... and the batched Signature.divide_by (Signature.divide_by_batch).
SIGDIV_EXTENSIONS = {"sig_divide": "_native_sigdiv"}
# ... and the multi-pairings over ranges of any lengths (BLS.verify_batch(ragged=True)).
PAIR_RANGE_EXTENSIONS = {"pairing_multi_ranges": "_native_pairranges"}
# ... and the verification of many aggregates of any shapes in one device call (BLS.verify_batch(fused=True)).
VERIFY_AGG_EXTENSIONS = {"verify_aggregates": "_native_veragg"}
# ... and secure aggregation for groups of any sizes in one device call (the ragged=True forms of util.hash_pks_batch,
# BLS.aggregate_pub_keys_batch and BLS.aggregate_sigs_secure_batch).
SECURE_RANGE_EXTENSIONS = {"hash_pks_ranges": "_native_secranges", "aggregate_pub_keys_secure_ranges": "_native_secranges",
                           "aggregate_sigs_secure_ranges": "_native_secranges"}


def extension(name):
    """The installed provider's extension `name`: the provider's own attribute of that name if it has one (stand-ins), for
    a HipProvider the function of EXTENSIONS (or FIND_EXTENSIONS, RANGE_EXTENSIONS, MSM_RANGE_EXTENSIONS, H2G1_EXTENSIONS, SIGDIV_EXTENSIONS, PAIR_RANGE_EXTENSIONS, VERIFY_AGG_EXTENSIONS, SECURE_RANGE_EXTENSIONS) bound to its
    engine, otherwise None."""
    prov = get()
    fn = getattr(prov, name, None)
    if fn is not None:
        return fn
    where = (EXTENSIONS.get(name) or FIND_EXTENSIONS.get(name) or RANGE_EXTENSIONS.get(name) or MSM_RANGE_EXTENSIONS.get(name)
             or H2G1_EXTENSIONS.get(name) or SIGDIV_EXTENSIONS.get(name) or PAIR_RANGE_EXTENSIONS.get(name)
             or VERIFY_AGG_EXTENSIONS.get(name) or SECURE_RANGE_EXTENSIONS.get(name))
    if isinstance(prov, HipProvider) and where:
        import functools
        import importlib
        module = importlib.import_module("." + where, __package__)
        return functools.partial(getattr(module, name), prov._eng)
    return None


def get():
    global _provider
    if _provider is None:
        _provider = HipProvider()
    return _provider
