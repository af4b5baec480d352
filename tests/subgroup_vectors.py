"""Shared by tests/test_subgroup_host.py and tests/test_gpu_subgroup.py: the membership vectors of tests/golden/subgroup.json
(generated from the reference by tests/golden/make_golden_subgroup.py), a host restatement of the two endomorphism tests of
csrc/blsgpu_subgroup.hip, a host-only provider for the CPU tests of BLS.verify_batch_randomized, and the signature batches
both test files run."""
import hashlib

from bls_py import hostmath as H

U = 0xd201000000010000                      # |u|, u = -0xd201000000010000
# the cube root of unity that goes with phi(P) = -[u^2] P (csrc/blsgpu_subgroup.hip, BETA_WORDS)
BETA = 0x5f19672fdf76ce51ba69c6076a0f77eaddb3a93be6f89688de17d813620a00022e01fffffffefffe
N = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def expected_status(rec):
    """the kernels' status byte for a fixture record: 1 in the subgroup, 2 on the curve outside it, 0 off the curve"""
    return 0 if not rec["on_curve"] else (1 if rec["in_subgroup"] else 2)


def g1_status(A):
    """k_g1_subgroup on the host: A affine (ints) or None -> status; phi(A) == -[u^2] A with phi(x, y) = (beta x, y)"""
    if A is None:
        return 1
    if not H.on_curve(H.F1, A):
        return 0
    R = H.jac_to_affine(H.F1, H.jac_mul(H.F1, H.aff_to_jac(H.F1, A), U * U))
    return 1 if R == (BETA * A[0] % H.Q, -A[1] % H.Q) else 2


def g2_status(A):
    """k_g2_subgroup on the host: psi(A) == [u] A = -[|u|] A, psi with the cofactor clearing's constants (hostmath.psi)"""
    if A is None:
        return 1
    if not H.on_curve(H.F2, A):
        return 0
    R = H.jac_to_affine(H.F2, H.jac_neg(H.F2, H.jac_mul(H.F2, H.aff_to_jac(H.F2, A), U)))
    return 1 if R == H.psi(A) else 2


class HostRLC:
    """The device operations BLS.verify_batch_randomized and verify_batch use, on the host: the membership tests restated
    above, group sums and pairings by the CPU oracle, hash to G2 by hostmath.  Records every call."""

    def __init__(self, oracle):
        self.O = oracle
        self.calls = []
        self.products = []                       # what every pairing_multi returned

    def g1_subgroup(self, pts):
        self.calls.append(("g1_subgroup", len(pts) // 96))
        return bytes(g1_status(H.g1_from_abi(pts[96 * i:96 * (i + 1)])) for i in range(len(pts) // 96))

    def g2_subgroup(self, pts):
        self.calls.append(("g2_subgroup", len(pts) // 192))
        return bytes(g2_status(H.g2_from_abi(pts[192 * i:192 * (i + 1)])) for i in range(len(pts) // 192))

    def _msm(self, fn, psz, pts, scalars, k, groups):
        out, inf = b"", []
        for g in range(groups):
            o, i = fn(pts[psz * k * g:psz * k * (g + 1)], None if scalars is None else [int(s) for s in scalars[k * g:k * (g + 1)]], k)
            out += o
            inf.append(i)
        return out, inf

    def g1_msm(self, pts, scalars, k, groups=1):
        self.calls.append(("g1_msm", k, groups))
        return self._msm(self.O.g1_msm, 96, pts, scalars, k, groups)

    def g2_msm(self, pts, scalars, k, groups=1):
        self.calls.append(("g2_msm", k, groups, None if scalars is None else list(scalars)))
        return self._msm(self.O.g2_msm, 192, pts, scalars, k, groups)

    def hash_to_g2(self, msg_hashes):
        from bls_py import util
        self.calls.append(("hash_to_g2", len(msg_hashes) // 32))
        return b"".join(H.g2_affine_bytes(H.hash_to_g2_prehashed(msg_hashes[32 * i:32 * (i + 1)], util.hash512))
                        for i in range(len(msg_hashes) // 32))

    def pairing_multi(self, g1, g2, n, inf=None):
        self.calls.append(("pairing_multi", n))
        out = self.O.pairing_multi(g1, g2, n, threads=8, inf=inf)
        self.products.append(out)
        return out

    def pairing_multi_batch(self, g1, g2, gsz, groups, inf=None):
        self.calls.append(("pairing_multi_batch", gsz, groups))
        return b"".join(self.O.pairing_multi(g1[96 * gsz * g:96 * gsz * (g + 1)], g2[192 * gsz * g:192 * gsz * (g + 1)], gsz, threads=8,
                                             inf=None if inf is None else inf[2 * gsz * g:2 * gsz * (g + 1)])
                        for g in range(groups))

    def names(self):
        return [c[0] for c in self.calls]


def secret_keys(tag, n):
    from bls_py.keys import PrivateKey
    return [PrivateKey(int.from_bytes(hashlib.sha256(b"%s%d" % (tag, i)).digest(), "big") % (N - 1) + 1) for i in range(n)]


def aggregates(n_aggs, per_agg, forged_at=None):
    """n_aggs aggregates of per_agg signatures over distinct messages (the C2 shape of tests/test_gpu_scheme.py), the one at
    index forged_at with signature 1 replaced by one over another message under the honest aggregation info"""
    from bls_py.bls import BLS
    from bls_py.keys import PrivateKey
    sks = secret_keys(b"rlc", per_agg)
    out = []
    for a in range(n_aggs):
        msgs = [b"agg%d-%d" % (a, i) for i in range(per_agg)]
        sigs = PrivateKey.sign_batch(sks, msgs)
        agg = BLS.aggregate_sigs(sigs)
        if a == forged_at:
            sigs[1] = sks[1].sign(b"forged")
            forged = BLS.aggregate_sigs_simple(sigs)
            forged.set_aggregation_info(agg.aggregation_info)
            agg = forged
        out.append(agg)
    return out
