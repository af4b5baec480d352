"""Shared by tests/test_lagrange_host.py and tests/test_gpu_lagrange.py: the vectors of tests/golden/lagrange.json
(generated from the reference by tests/golden/make_golden_lagrange.py) in the forms the tests need, the three
Threshold.*_batch methods checked against them through whatever provider bls_py.backend holds, and a host-only provider of
the three device operations (Python integers + hostmath) for the CPU tests."""
import random

from bls_py import hostmath as H

from hd_vectors import HostHD

N = H.N


def group_players(g):
    return [int(x, 16) for x in g["X"]]


def group_values(g):
    """the Y of a fixture group (kept in the file as their seed)"""
    r = random.Random(g["y_seed"])
    Y = [r.randrange(N) for _ in g["X"]]
    assert "%064x" % Y[0] == g["y0"]
    return Y


def group_coeffs(g):
    return [int(c, 16) for c in g["coeffs"]]


def be32(values):
    return b"".join(v.to_bytes(32, "big") for v in values)


def ints32(b):
    return [int.from_bytes(b[i:i + 32], "big") for i in range(0, len(b), 32)]


def by_k(groups):
    """{k: [fixture groups]} in the file's order"""
    out = {}
    for g in groups:
        out.setdefault(g["k"], []).append(g)
    return out


def host_coeffs(X):
    """(coefficients, status) of one group by the device's contract: zeros and status 0 where the reference asserts"""
    k = len(X)
    if len(set(X)) != k or not all(0 < x < N for x in X):
        return [0] * k, 0
    sh = []
    for j in range(k):
        w = -X[j] % N
        for i in range(k):
            if i != j:
                w = w * (X[j] - X[i]) % N
        sh.append(pow(w, N - 2, N))
    den = pow(sum(sh) % N, N - 2, N)
    return [s * den % N for s in sh], 1


class HostLagrange(HostHD):
    """lagrange_at_zero, fr_interpolate_at_zero, threshold_combine and g2_msm of bls_py.backend.HipProvider on the host,
    by the device's contract, with the calls recorded; everything else from `inner`."""
    LAGRANGE_MAX_K = 1024

    def _groups(self, x, k, groups):
        xs = ints32(bytes(x)) if isinstance(x, (bytes, bytearray)) else [int(v) for v in x]
        assert 1 <= k <= self.LAGRANGE_MAX_K and len(xs) == k * groups
        return [xs[g * k:(g + 1) * k] for g in range(groups)]

    def lagrange_at_zero(self, x, k, groups=1):
        self.calls.append(("lagrange_at_zero", k, groups))
        res = [host_coeffs(X) for X in self._groups(x, k, groups)]
        return b"".join(be32(c) for c, _ in res), bytes(s for _, s in res)

    def fr_interpolate_at_zero(self, x, y, k, groups=1):
        self.calls.append(("fr_interpolate_at_zero", k, groups))
        ys = self._groups(y, k, groups)
        res = [host_coeffs(X) for X in self._groups(x, k, groups)]
        return be32([sum(l * v for l, v in zip(c, Y)) % N for (c, _), Y in zip(res, ys)]), bytes(s for _, s in res)

    def threshold_combine(self, sigs, x, k, groups=1):
        self.calls.append(("threshold_combine", k, groups))
        res = [host_coeffs(X) for X in self._groups(x, k, groups)]
        out, inf = self._g2_msm(sigs, [l for c, _ in res for l in c], k, groups)
        return out, inf, bytes(s for _, s in res)

    def g2_msm(self, pts, scalars, k, groups=1):
        self.calls.append(("g2_msm", k, groups))
        return self._g2_msm(pts, scalars, k, groups)

    @staticmethod
    def _g2_msm(pts, scalars, k, groups):
        out, inf = bytearray(), []
        for g in range(groups):
            R = None
            for j in range(g * k, (g + 1) * k):
                sc = 1 if scalars is None else int(scalars[j]) if not isinstance(scalars, (bytes, bytearray)) else ints32(scalars[32 * j:32 * j + 32])[0]
                R = H.jac_add(H.F2, R, H.jac_mul(H.F2, H.aff_to_jac(H.F2, H.g2_from_abi(pts[192 * j:192 * (j + 1)])), sc))
            A = H.jac_to_affine(H.F2, R)
            out += H.g2_affine_bytes(A)
            inf.append(A is None)
        return bytes(out), inf

    def hash_to_g2(self, msg_hashes):
        from bls_py import util
        self.calls.append(("hash_to_g2", len(msg_hashes) // 32))
        return b"".join(H.g2_affine_bytes(H.hash_to_g2_prehashed(msg_hashes[32 * i:32 * (i + 1)], util.hash512))
                        for i in range(len(msg_hashes) // 32))


def unit_signatures(combine):
    """the five unit signatures of the fixture's 3-of-5 sharing as Signature objects (player p at index p - 1)"""
    from bls_py.signature import Signature
    return [Signature.from_bytes(bytes.fromhex(h)) for h in combine["unit_sigs_ser"]]


def check_batches(lag, shuffle_seed=None):
    """the three Threshold.*_batch methods over the whole fixture in ONE call each (mixed group lengths), against the
    reference's values"""
    from bls_py.fields import Fq
    from bls_py.threshold import Threshold
    groups = list(lag["groups"])
    if shuffle_seed is not None:
        random.Random(shuffle_seed).shuffle(groups)
    Xs = [group_players(g) for g in groups]
    got = Threshold.lagrange_coeffs_at_zero_batch(Xs)
    assert [[int(l) for l in L] for L in got] == [group_coeffs(g) for g in groups]
    assert all(type(l) is Fq and l.Q == N for L in got for l in L)
    Ys = [[Fq(N, y) if i % 2 else y for i, y in enumerate(group_values(g))] for g in groups]     # Fq and int values
    vals = Threshold.interpolate_at_zero_batch(Xs, Ys)
    assert [int(v) for v in vals] == [int(g["interpolate"], 16) for g in groups]
    assert all(type(v) is Fq and v.Q == N for v in vals)
    cb = lag["combine"]
    unit = unit_signatures(cb)
    subs = cb["subsets"]
    sigs = Threshold.aggregate_unit_sigs_batch([[unit[p - 1] for p in s["players"]] for s in subs], [s["players"] for s in subs], 3)
    assert [s.serialize().hex() for s in sigs] == [s["aggregate"] for s in subs]
    assert all(s.aggregation_info is None for s in sigs)
