"""Shared by tests/test_rxsecret_host.py and tests/test_gpu_rxsecret.py: the receiving side of key generation for secrets --
the inputs the share check on the scalar-independent schedule (blsgpu_g1_poly_check_secret) and the masked sums of
blsgpu_fr_sum_secret are checked with, and a host-only provider of the two device operations (hostmath + Python integers) for
the CPU tests."""
import random

from bls_py import hostmath as H

from dkg_vectors import HostDKG
from frsecret_vectors import EDGE, HostFrSecret, N, be32, ints32, poly_eval, values

R = 2**256
X_EDGE = [0, 1, 2, N - 1, N, N + 1, R - 1]                  # full-width evaluation points: reduced mod n on the device


def literal_forms(v):
    """v mod n as the 256-bit integers v, v + n and v + m n for the largest m that stays below 2^256: the check takes the
    literal integer, and all three are the same point"""
    v %= N
    m = (R - 1 - v) // N
    assert m >= 1 and v + m * N < R <= v + (m + 1) * N            # (2^256 / n = 2.2: m is 1 or 2)
    return [v, v + N, v + m * N]


def fragment_case(coeffs, t, xs):
    """Every polynomial of the flat coefficient list (ints, t per polynomial) at every x, as (poly, x, s, want) sorted by
    polynomial: the right fragment in its three literal forms (want 1), the fragment +-1 (want 0) and the edge values 0 and
    2^256 - 1 (want: by Python integers)"""
    polys = [coeffs[i:i + t] for i in range(0, len(coeffs), t)]
    poly, x, s, want = [], [], [], []
    for j, P in enumerate(polys):
        for v in xs:
            f = poly_eval(P, v % N)
            for cand in literal_forms(f) + [(f + 1) % N, (f - 1) % N, 0, R - 1]:
                poly.append(j)
                x.append(v)
                s.append(cand)
                want.append(1 if cand % N == f else 0)
    return poly, x, s, want


def seeded_coeffs(seed, n_polys, t, zero_at=()):
    """n_polys x t coefficients in [1, n); polynomial j gets a zero coefficient -- an infinity commitment -- at the index
    zero_at[j], if it has one"""
    rnd = random.Random(seed)
    coeffs = [rnd.randrange(1, N) for _ in range(n_polys * t)]
    for j, k in enumerate(zero_at):
        if k is not None and j < n_polys:
            coeffs[j * t + k] = 0
    return coeffs


def sums(ys, k):
    """the `out` bytes of blsgpu_fr_sum_secret for flat values (ints) in groups of k"""
    return be32([sum(ys[i:i + k]) % N for i in range(0, len(ys), k)])


def sum_values(seed, k, groups):
    """k * groups values below 2^256: the edge list first, then seeded ones; the last group is all 2^256 - 1 (the most carries)"""
    ys = values(seed, k * groups)
    if groups > 1:
        ys[-k:] = [R - 1] * k
    return ys


class HostRxSecret(HostFrSecret, HostDKG):
    """g1_poly_check_secret, g1_mul_gen_secret and fr_sum_secret of bls_py.backend.HipProvider on the host, by the device's
    contract (the status and Horner bytes of g1_poly_check for the literal fragment; sums mod n of values below 2^256 with the
    public key of each), with the calls recorded; the rest from HostFrSecret and HostDKG."""

    def _quiet(self, fn, *args):
        n_before = len(self.calls)
        out = fn(self, *args)
        del self.calls[n_before:]
        return out

    def g1_poly_check_secret(self, commit, n_polys, t, poly, x, s, aff=False):
        self.calls.append(("g1_poly_check_secret", n_polys, len(poly)))
        assert s is not None and len(s) == 32 * len(poly)
        return self._quiet(HostDKG.g1_poly_check, commit, n_polys, t, poly, x, s, aff)

    def g1_mul_gen_secret(self, scalars):
        self.calls.append(("g1_mul_gen_secret", len(scalars) // 32))
        return self._quiet(HostDKG.g1_mul_gen, scalars)

    def fr_sum_secret(self, y, k, groups=1, pk=False):
        self.calls.append(("fr_sum_secret", k, groups, bool(pk)))
        ys = ints32(bytes(y))
        assert k >= 1 and len(ys) == k * groups
        out = sums(ys, k)
        aff, ser = self._quiet(HostDKG.g1_mul_gen, out) if pk else (None, None)
        return out, aff, ser


__all__ = ["EDGE", "H", "HostRxSecret", "N", "R", "X_EDGE", "be32", "fragment_case", "ints32", "literal_forms", "poly_eval",
           "seeded_coeffs", "sum_values", "sums", "values"]
