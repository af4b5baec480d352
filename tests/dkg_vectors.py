"""Shared by tests/test_dkg_host.py and tests/test_gpu_dkg.py: the Joint-Feldman vectors of tests/golden/dkg.json
(generated from the reference by tests/golden/make_golden_dkg.py) checked through whatever provider bls_py.backend holds,
and a host-only provider of the share-check operations (hostmath) for the CPU tests."""
import random

from bls_py import hostmath as H

from hd_vectors import HostHD


def horner_aff(C, x):
    """sum_k (x mod n)^k C_k by Horner with hostmath (C: affine tuples or None), affine or None"""
    x %= H.N
    R = None
    for c in reversed(C):
        R = H.jac_add(H.F1, H.jac_mul(H.F1, R, x) if x else None, H.aff_to_jac(H.F1, c))
    return H.jac_to_affine(H.F1, R)


class HostDKG(HostHD):
    """g1_poly_check, g1_mul_gen and g1_msm of bls_py.backend.HipProvider on the host: the device's contract (Horner with
    x mod n, status 2 for a polynomial with a C_k, k >= 1, outside the order-n subgroup), no GPU."""

    def g1_poly_check(self, commit, n_polys, t, poly, x, s=None, aff=False):
        self.calls.append(("g1_poly_check", n_polys, len(poly)))
        assert len(commit) == 96 * n_polys * t and t >= 1 and all(0 <= p < n_polys for p in poly)
        polys = [[H.g1_from_abi(commit[96 * (j * t + k):96 * (j * t + k + 1)]) for k in range(t)] for j in range(n_polys)]
        bad = [any(H.jac_mul(H.F1, H.aff_to_jac(H.F1, c), H.N) is not None for c in P[1:]) for P in polys]
        status, out = bytearray(), bytearray()
        for i, p in enumerate(poly):
            R = horner_aff(polys[p], int.from_bytes(x[32 * i:32 * (i + 1)], "big"))
            out += H.g1_affine_bytes(R)
            if s is not None:
                sv = int.from_bytes(s[32 * i:32 * (i + 1)], "big") % H.N
                L = H.jac_to_affine(H.F1, H.jac_mul(H.F1, H.aff_to_jac(H.F1, H.G1_GEN), sv))
                status.append(2 if bad[p] else int(L == R))
        return (bytes(status) if s is not None else None), (bytes(out) if aff else None)

    def g1_msm(self, pts, scalars, k, groups=1):
        self.calls.append(("g1_msm", k, groups))
        out, inf = bytearray(), []
        for g in range(groups):
            R = None
            for j in range(g * k, (g + 1) * k):
                sc = 1 if scalars is None else int(scalars[j])
                R = H.jac_add(H.F1, R, H.jac_mul(H.F1, H.aff_to_jac(H.F1, H.g1_from_abi(pts[96 * j:96 * (j + 1)])), sc))
            A = H.jac_to_affine(H.F1, R)
            out += H.g1_affine_bytes(A)
            inf.append(A is None)
        return bytes(out), inf


def point(h):
    """AffinePoint from the fixture's 96-byte hex (all zero = infinity)"""
    from bls_py.ec import AffinePoint
    return AffinePoint._from(H.F1, H.g1_from_abi(bytes.fromhex(h)))


def dealing_records(dkg):
    """(T, fragment, player, commitments, expect) for every (dealer, player) pair of every dealing"""
    from bls_py.fields import Fq
    out = []
    for dl in dkg["dealings"]:
        for d in dl["dealers"]:
            C = [point(h) for h in d["commitments"]]
            for j, (f, ok) in enumerate(zip(d["fragments"], d["verify"])):
                out.append((dl["T"], Fq(H.N, int(f, 16)), j + 1, C, ok))
    return out


def check_records(dkg):
    """(T, fragment, player, commitments, expect) of the fixture's single checks"""
    from bls_py.fields import Fq
    return [(c["T"], Fq(H.N, int(c["fragment"], 16)), c["player"], [point(h) for h in c["commitments"]], c["expect"])
            for c in dkg["checks"]]


def check_batch(records, shuffle_seed=None):
    """verify_secret_fragment_batch over records of one T at a time (optionally shuffled) against their expectations"""
    from bls_py.threshold import Threshold
    by_t = {}
    for r in records:
        by_t.setdefault(r[0], []).append(r)
    for T, rs in by_t.items():
        if shuffle_seed is not None:
            rs = list(rs)
            random.Random(shuffle_seed).shuffle(rs)
        got = Threshold.verify_secret_fragment_batch(T, [r[1] for r in rs], [r[2] for r in rs], [r[3] for r in rs])
        assert got == [r[4] for r in rs], T
