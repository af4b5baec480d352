"""The receiving side of key generation for secrets without a GPU: the sum step of csrc/fr_scalar.h (sum_term_masked, the
text k_fr_sum_secret runs) compiled for the host against Python integers, and the secret=True keyword of
Threshold.verify_secret_fragment_batch and BLS.aggregate_priv_keys_batch -- under a provider without the entries (they
raise) and under a host provider of them (tests/rxsecret_vectors.HostRxSecret)."""
import os
import subprocess

import pytest

from dkg_vectors import HostDKG, check_records, dealing_records, point
from frsecret_vectors import dealers, values
from rxsecret_vectors import HostRxSecret, N, be32, sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")

HOST_TEST = r'''
#include "fr_scalar.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
static char kk[16], a[70000];
int main() {
    while (scanf("%15s %69999s", kk, a) == 2) {              // k, then groups x k values (64 hex digits each) -> groups sums
        const size_t k = strtoul(kk, 0, 10), n = strlen(a) / 64;
        uint8_t* y = (uint8_t*)malloc(32 * n + 1);
        for (size_t i = 0; i < 32 * n; i++) { unsigned v; sscanf(a + 2 * i, "%2x", &v); y[i] = (uint8_t)v; }
        for (size_t g = 0; g < n / k; g++) {
            uint8_t out[32];
            frs::sum_group_masked(y + 32 * g * k, k, out);
            for (int i = 0; i < 32; i++) printf("%02x", out[i]);
        }
        printf("\n");
        free(y);
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def sum_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("rxsecret")
    src, exe = d / "t.cpp", d / "t"
    src.write_text(HOST_TEST)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC, "-o", str(exe), str(src)])
    return str(exe)


@pytest.mark.parametrize("k", [1, 2, 7])
def test_sum_step_matches_python_integers(sum_exe, k):
    ys = values(40 + k, 7 * k * 3)                       # the edge list leads: 0, 1, n - 1, n, n + 1, 2^255, 2^256 - 1
    ys += [2**256 - 1] * k + [N - 1] * k + [N] * k       # whole groups of the largest value, of n - 1 and of 0 mod n
    out = subprocess.run([sum_exe], input="%d %s\n" % (k, be32(ys).hex()), capture_output=True, text=True, check=True).stdout.split()
    assert out == [sums(ys, k).hex()]


@pytest.fixture
def host_provider():
    from bls_py import backend
    old = backend._provider
    p = HostRxSecret(None)
    backend.use(p)
    yield p
    backend.use(old)


@pytest.fixture
def without_the_entries():
    """a provider with the default paths only: secret=True has nowhere to go"""
    from bls_py import backend
    old = backend._provider
    p = HostDKG(None)
    backend.use(p)
    yield p
    backend.use(old)


@pytest.fixture
def no_host_loop(monkeypatch):
    """the single-call host loop is out of reach"""
    from bls_py.threshold import Threshold

    def refuse(*a, **kw):
        raise AssertionError("the host loop was entered")
    monkeypatch.setattr(Threshold, "verify_secret_fragment", staticmethod(refuse))


def _by_t(records):
    out = {}
    for r in records:
        out.setdefault(r[0], []).append(r)
    return out


def test_batch_parity_on_the_fixture(golden, host_provider, no_host_loop):
    from bls_py.threshold import Threshold
    dkg = golden("dkg.json")
    records = dealing_records(dkg) + check_records(dkg)
    assert {r[4] for r in records} == {True, False}
    seen = set()
    for T, rs in _by_t(records).items():
        host_provider.calls.clear()
        got = Threshold.verify_secret_fragment_batch(T, [r[1] for r in rs], [r[2] for r in rs], [r[3] for r in rs], secret=True)
        assert got == [r[4] for r in rs], T
        names = [c[0] for c in host_provider.calls]
        assert names[0] == "g1_poly_check_secret" and names.count("g1_poly_check_secret") == 1
        assert "g1_poly_check" not in names and "g1_mul_gen" not in names
        assert set(names) <= {"g1_poly_check_secret", "g1_msm", "g1_mul_gen_secret"}
        seen |= set(names)
    assert seen == {"g1_poly_check_secret", "g1_msm", "g1_mul_gen_secret"}          # the status-2 records were among them


def test_default_routing_is_unchanged(golden):
    from bls_py import backend
    from bls_py.threshold import Threshold
    dkg = golden("dkg.json")
    records = _by_t(dealing_records(dkg) + check_records(dkg))[3]
    args = (3, [r[1] for r in records], [r[2] for r in records], [r[3] for r in records])
    old = backend._provider
    try:
        calls = []
        for prov in (HostDKG(None), HostRxSecret(None)):        # with and without the new entries: the same calls
            backend.use(prov)
            assert Threshold.verify_secret_fragment_batch(*args) == [r[4] for r in records]
            assert Threshold.verify_secret_fragment_batch(*args, secret=False) == [r[4] for r in records]
            calls.append(prov.calls)
    finally:
        backend.use(old)
    assert calls[0] == calls[1]
    assert [c[0] for c in calls[0]] == ["g1_poly_check", "g1_msm", "g1_mul_gen"] * 2


def test_secret_raises_without_the_entries(golden, without_the_entries):
    from bls_py.bls import BLS
    from bls_py.keys import PrivateKey
    from bls_py.threshold import Threshold
    T, s, p, C, ok = dealing_records(golden("dkg.json"))[3]
    with pytest.raises(NotImplementedError):
        Threshold.verify_secret_fragment_batch(T, [s], [p], [C], secret=True)
    with pytest.raises(NotImplementedError):
        BLS.aggregate_priv_keys_batch([[PrivateKey(5), PrivateKey(6)]], secret=True)
    with pytest.raises(NotImplementedError):
        BLS.aggregate_priv_keys_batch([[PrivateKey(5)]], secret=True, public_keys=True)
    assert without_the_entries.calls == []
    # the defaults are still there
    assert Threshold.verify_secret_fragment_batch(T, [s], [p], [C]) == [ok]
    assert BLS.aggregate_priv_keys_batch([[PrivateKey(5), PrivateKey(6)]])[0].value == 11


def test_unfit_records_raise(golden, host_provider, no_host_loop):
    from bls_py import hostmath as H
    from bls_py.ec import AffinePoint
    from bls_py.fields import Fq
    from bls_py.threshold import Threshold
    d = golden("dkg.json")["dealings"][2]["dealers"][1]
    C = [point(h) for h in d["commitments"]]
    f = [Fq(N, int(h, 16)) for h in d["fragments"]]
    off = list(C)
    off[1] = AffinePoint(Fq(H.Q, 1), Fq(H.Q, 1), False)
    unfit = [(f[0], True, C),                                       # a player that is not an int
             (f[3], 4, off),                                        # a commitment off the curve
             (int(f[0]) + N, 1, C),                                 # a fragment >= n
             (f[2], 3, [c.to_jacobian() for c in C]),               # commitments that are not AffinePoints
             (Fq(H.Q, int(f[0])), 1, C)]                            # an Fq of another modulus
    for s, p, CC in unfit:
        host_provider.calls.clear()
        with pytest.raises(ValueError):
            Threshold.verify_secret_fragment_batch(3, [f[1], s], [2, p], [C, CC], secret=True)
        assert host_provider.calls == []
    # the reference's assertions still come first
    with pytest.raises(AssertionError):
        Threshold.verify_secret_fragment_batch(3, [f[0], Fq(N, 0)], [1, 2], [C, C], secret=True)
    with pytest.raises(AssertionError):
        Threshold.verify_secret_fragment_batch(3, [f[0]], [0], [C], secret=True)
    assert Threshold.verify_secret_fragment_batch(3, [], [], [], secret=True) == []
    assert host_provider.calls == []
    # what the device takes: Fq mod n, ints in [1, n), any int player
    assert Threshold.verify_secret_fragment_batch(3, [f[0], int(f[1]), f[4]], [1, 2, 5 + 3 * N], [C, C, C], secret=True) == [True] * 3
    assert host_provider.calls == [("g1_poly_check_secret", 1, 3)]


def test_aggregation_equals_the_loop(golden, host_provider):
    from bls_py.bls import BLS
    from bls_py.keys import PrivateKey
    groups = []
    for T, n_players, ds in dealers(golden("dkg.json")):
        groups += [[PrivateKey(int(d["fragments"][j], 16)) for d in ds] for j in range(n_players)]       # the fragment columns
    assert sorted({len(g) for g in groups}) == [1, 3, 5, 7]
    loop = [BLS.aggregate_priv_keys(g, None, False) for g in groups]
    loop_pk = [k.get_public_key() for k in loop]
    for secret in (False, True):
        host_provider.calls.clear()
        keys = BLS.aggregate_priv_keys_batch(groups, secret=secret)
        assert [type(k) for k in keys] == [PrivateKey] * len(groups) and [k.value for k in keys] == [k.value for k in loop]
        if secret:                                              # one call per distinct group length, nothing else
            assert sorted(host_provider.calls) == [("fr_sum_secret", k, k, False) for k in (1, 3, 5, 7)]
        else:
            assert host_provider.calls == []
        host_provider.calls.clear()
        keys, pks = BLS.aggregate_priv_keys_batch(groups, secret=secret, public_keys=True)
        assert [k.value for k in keys] == [k.value for k in loop]
        assert pks == loop_pk and [p.serialize() for p in pks] == [p.serialize() for p in loop_pk]
        assert [k.get_public_key() for k in keys] == loop_pk
        if secret:
            assert sorted(host_provider.calls) == [("fr_sum_secret", k, k, True) for k in (1, 3, 5, 7)]
    assert BLS.aggregate_priv_keys_batch([], secret=True) == [] and BLS.aggregate_priv_keys_batch([], secret=True, public_keys=True) == ([], [])
    host_provider.calls.clear()
    with pytest.raises(ValueError):
        BLS.aggregate_priv_keys_batch([groups[0], []], secret=True)
    assert host_provider.calls == []
    assert BLS.aggregate_priv_keys_batch([[]])[0].value == 0            # the host loop takes an empty group, as the single call does
