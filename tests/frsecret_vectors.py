"""Shared by tests/test_frsecret_host.py and tests/test_gpu_frsecret.py: the values the secret forms of the threshold calls
are checked with, and a host-only provider of the three device operations (Python integers + hostmath) for the CPU tests."""
import random

from bls_py import hostmath as H

from lagrange_vectors import HostLagrange, be32, host_coeffs, ints32

N = H.N
R = 2**256
EDGE = [0, 1, N - 1, N, N + 1, 2**255, 2**256 - 1]


def values(seed, count):
    """`count` 256-bit values: the edge list first (as far as it fits), then seeded random ones"""
    rnd = random.Random(seed)
    return (EDGE + [rnd.randrange(2**256) for _ in range(max(0, count - len(EDGE)))])[:count]


def poly_eval(poly, x):
    """sum_k poly[k] x^k mod n"""
    acc = 0
    for c in reversed(poly):
        acc = (acc * x + c) % N
    return acc


def fragments(coeffs, t, xs):
    """the out_frag bytes of blsgpu_threshold_deal_secret for flat coefficients (ints) and points (ints)"""
    polys = [coeffs[i:i + t] for i in range(0, len(coeffs), t)]
    return be32([poly_eval(p, x) for p in polys for x in xs])


def dealers(dkg):
    """[(T, N, [dealer records])] of tests/golden/dkg.json"""
    return [(dl["T"], dl["N"], dl["dealers"]) for dl in dkg["dealings"]]


class HostFrSecret(HostLagrange):
    """threshold_deal_secret, fr_interpolate_at_zero_secret and sign_threshold of bls_py.backend.HipProvider on the host, by
    the device's contract, with the calls recorded; the rest from HostLagrange."""

    def threshold_deal_secret(self, coeffs, t, x, commit=True, frag=True):
        cs, xs = ints32(bytes(coeffs)), ints32(bytes(x))
        self.calls.append(("threshold_deal_secret", len(cs) // t, t, len(xs)))
        assert 1 <= t <= self.LAGRANGE_MAX_K and len(cs) % t == 0 and xs
        aff = b"".join(H.g1_affine_bytes(H.jac_to_affine(H.F1, H.jac_mul(H.F1, H.aff_to_jac(H.F1, H.G1_GEN), c % N))) for c in cs)
        return (aff if commit else None), (fragments(cs, t, xs) if frag else None)

    def fr_interpolate_at_zero_secret(self, x, y, k, groups=1):
        self.calls.append(("fr_interpolate_at_zero_secret", k, groups))
        n_before = len(self.calls)
        out = self.fr_interpolate_at_zero(x, y, k, groups)
        del self.calls[n_before:]
        return out

    def sign_threshold(self, sks, x, k, msg_hashes, groups=1, aff=True, ser=True):
        self.calls.append(("sign_threshold", k, groups, len(msg_hashes) // 32))
        n_before = len(self.calls)
        n_msg = len(msg_hashes) // 32
        assert n_msg in (1, groups)
        res = [host_coeffs(X) for X in self._groups(x, k, groups)]
        lam = [l for c, _ in res for l in c]
        pts = self.hash_to_g2(msg_hashes)
        per = b"".join(pts[192 * (i // k if n_msg > 1 else 0):][:192] for i in range(k * groups))
        out, inf = self._g2_msm(per, [l * (s % N) % N for l, s in zip(lam, ints32(bytes(sks)))], 1, k * groups)
        del self.calls[n_before:]
        return out, None, inf, bytes(s for _, s in res)
